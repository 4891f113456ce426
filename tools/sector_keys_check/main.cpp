// sector_keys_check -- nfc_host_commands_keyed, the CPU twin of k_multi_commands with a per-sector key table (include/nfc_amd.h;
// csrc/sector_keys.h, fsm.hip.h), over the 26 frames of card 1 of tests/test_sector_keys_host.py: AUTHA 4 under K0, nested
// AUTHA 8 under K1, nested AUTHB 12 under K2, nested AUTHA 5 under K0, a READ after each.  With the right table, with a table of
// all-wrong keys in every slot, with none, and in two slices cut between every pair of frames with the state handed on.
// A stand-alone host program: the way to run the restated machine's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/sector_keys_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_commands.hip -o sector_keys_check && ./sector_keys_check
// It touches no GPU.  Exit status 0: the right table gives four AR OK, four AT OK and the four blocks as the READ answers; the wrong
// one and none give no AT OK; every two-slice run gives the whole run's records, bytes and state.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"

// the frames as the host assembly gives them (nfc_host_frames): idx, byte_off, n_bits, n_bytes, flags, type
struct Row { uint64_t idx; uint32_t byte_off, n_bits, n_bytes, flags; int32_t type; };
static const Row ROWS[26] = {
    {0, 0, 18, 2, 0x100, 0},
    {1, 0, 81, 9, 0x300, 1},
    {2, 9, 36, 4, 0x300, 1},
    {3, 2, 36, 4, 0x100, 0},
    {4, 13, 72, 8, 0x0, 1},
    {5, 6, 36, 4, 0x0, 0},
    {6, 21, 36, 4, 0x0, 1},
    {7, 10, 162, 18, 0x0, 0},
    {8, 25, 36, 4, 0x0, 1},
    {9, 28, 36, 4, 0x0, 0},
    {10, 29, 72, 8, 0x0, 1},
    {11, 32, 36, 4, 0x0, 0},
    {12, 37, 36, 4, 0x0, 1},
    {13, 36, 162, 18, 0x0, 0},
    {14, 41, 36, 4, 0x0, 1},
    {15, 54, 36, 4, 0x0, 0},
    {16, 45, 72, 8, 0x0, 1},
    {17, 58, 36, 4, 0x0, 0},
    {18, 53, 36, 4, 0x0, 1},
    {19, 62, 162, 18, 0x0, 0},
    {20, 57, 36, 4, 0x0, 1},
    {21, 80, 36, 4, 0x0, 0},
    {22, 61, 72, 8, 0x0, 1},
    {23, 84, 36, 4, 0x0, 0},
    {24, 69, 36, 4, 0x0, 1},
    {25, 88, 162, 18, 0x0, 0},
};
static const uint8_t BYTES0[106] = {
    0x04, 0x00, 0x17, 0x3A, 0x00, 0x32, 0x00, 0x66, 0xB1, 0x01, 0xB2, 0xDF, 0xD0, 0x53, 0x9D, 0x9E, 0xF6, 0x4A, 0x70, 0x88, 0x51, 0xFC, 0x32, 0x1F,
    0xF3, 0xA9, 0x90, 0xFF, 0x67, 0x01, 0x87, 0xF1, 0xA2, 0x7D, 0x4A, 0xAE, 0x19, 0x75, 0x23, 0xA1, 0xE6, 0xE3, 0x20, 0x4D, 0xF8, 0xD2, 0x4D, 0x21,
    0x46, 0xDE, 0x71, 0xF1, 0x48, 0xCB, 0xF9, 0x6F, 0xBC, 0x8C, 0xF6, 0x7E, 0x63, 0xDE, 0x3A, 0x01, 0xD9, 0x79, 0x6A, 0xD0, 0x80, 0x10, 0x03, 0x40,
    0x63, 0x5C, 0xFF, 0x78, 0x0D, 0xF0, 0xBE, 0x8A, 0x1B, 0x0F, 0xA7, 0xD5, 0xEF, 0x02, 0x16, 0xE7, 0x31, 0xD2, 0xCB, 0x26, 0xED, 0xC3, 0x7F, 0x47,
    0x4B, 0xE4, 0x2F, 0xAF, 0x18, 0xF5, 0xB7, 0x7C, 0x81, 0xD2,
};
static const uint8_t PAR0[106] = {
    0x00, 0x01, 0x01, 0x01, 0x01, 0x00, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x01, 0x01, 0x01, 0x00, 0x01, 0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x01,
    0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x01, 0x01, 0x00, 0x01, 0x01, 0x01, 0x00, 0x01, 0x01, 0x00, 0x01, 0x00, 0x00, 0x00, 0x01, 0x01, 0x00, 0x01,
    0x01, 0x01, 0x00, 0x00, 0x01, 0x01, 0x01, 0x00, 0x01, 0x01, 0x01, 0x01, 0x01, 0x00, 0x00, 0x00, 0x00, 0x01, 0x00, 0x01, 0x01, 0x01, 0x00, 0x00,
    0x01, 0x01, 0x00, 0x01, 0x00, 0x00, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x00, 0x00, 0x01,
    0x01, 0x01, 0x00, 0x00, 0x01, 0x01, 0x00, 0x01, 0x01, 0x01,
};
static const uint8_t BYTES1[73] = {
    0x93, 0x70, 0xF3, 0x86, 0xB0, 0xA2, 0x67, 0xB6, 0x3C, 0x60, 0x04, 0xD1, 0x3D, 0xC1, 0x23, 0x92, 0x43, 0x54, 0x94, 0x31, 0xAC, 0xF5, 0x09, 0x57,
    0xCE, 0xC5, 0x83, 0xFE, 0x12, 0x26, 0xAF, 0x96, 0x88, 0x9B, 0xF8, 0x8D, 0x55, 0x1C, 0x81, 0x5C, 0x5D, 0x30, 0xCB, 0xB6, 0xF8, 0xDC, 0xEA, 0x67,
    0x44, 0x2A, 0xBC, 0x7D, 0x88, 0xEA, 0x8E, 0xD1, 0xCC, 0x6F, 0xEC, 0x58, 0xA4, 0x8D, 0x20, 0x65, 0x3B, 0xEE, 0x9C, 0x7A, 0x6E, 0x5D, 0xEE, 0xAD,
    0xC4,
};
static const uint8_t PAR1[73] = {
    0x01, 0x00, 0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x01, 0x01, 0x00, 0x01, 0x00, 0x01, 0x01, 0x00, 0x01, 0x01, 0x01, 0x00, 0x00, 0x00, 0x01, 0x00,
    0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x01, 0x01, 0x01, 0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x01, 0x01, 0x00, 0x01, 0x00,
    0x01, 0x01, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x01, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00, 0x01, 0x01, 0x00, 0x01, 0x00,
    0x01,
};

static const uint8_t K0[6] = {0x2E, 0x1A, 0x2C, 0xB9, 0xB7, 0xC5}, K1[6] = {0x08, 0x67, 0xE5, 0xB4, 0xF0, 0x4C}, K2[6] = {0xE9, 0xAE, 0xEB, 0xD1, 0xF2, 0xF0}, WRONG[6] = {0x49, 0x1D, 0x3C, 0x5D, 0x2D, 0x8E};
static const uint8_t BLOCKS[4][16] = {
    {0x31, 0xEF, 0xD3, 0xCC, 0xB5, 0x47, 0x53, 0xE4, 0x58, 0x26, 0x29, 0x5E, 0x08, 0x0B, 0x54, 0x16},
    {0x30, 0xB2, 0x33, 0x6F, 0xAB, 0x2E, 0x6B, 0xA9, 0xAB, 0x15, 0xE8, 0x9A, 0xEC, 0x99, 0xEB, 0x18},
    {0x33, 0x1C, 0xFD, 0x2F, 0x6D, 0xCE, 0x07, 0x8F, 0x78, 0x6F, 0x02, 0x17, 0xB1, 0xE1, 0x25, 0x2E},
    {0xBF, 0x5B, 0xD5, 0x3E, 0x3E, 0xA5, 0x48, 0xF0, 0x29, 0xFB, 0xB4, 0x7E, 0x91, 0x7E, 0x37, 0xF6},
};
enum { READT = 22, N = 26 };

struct Run {
    nfc_fsm_state st;
    std::vector<nfc_frame> out;
    std::vector<uint8_t> data;
    std::vector<uint16_t> enc;
};

static bool run(const nfc_fsm_key_table *table, size_t cut, Run &r) {
    nfc_raw_frame fr[N];
    memset(fr, 0, sizeof fr);
    size_t cap = 0;
    for (int i = 0; i < N; i++) {
        fr[i].idx = ROWS[i].idx, fr[i].byte_off = ROWS[i].byte_off, fr[i].n_bits = ROWS[i].n_bits, fr[i].n_bytes = ROWS[i].n_bytes;
        fr[i].flags = ROWS[i].flags, fr[i].type = ROWS[i].type;
        cap += ROWS[i].n_bytes;
    }
    r.out.assign(N, nfc_frame());
    r.data.assign(cap, 0);
    r.enc.assign(cap, 0);
    if (nfc_fsm_state_init(&r.st) != NFC_OK) return false;
    size_t at = 0;
    const size_t edges[3] = {0, cut, N};
    for (int s = 0; s < 2; s++) {
        const size_t a = edges[s], b = edges[s + 1];
        size_t used = 0;
        // (exact capacity: a write past a slice's slots is a write past the vectors' end for the last slice)
        size_t room = 0;
        for (size_t i = a; i < b; i++) room += fr[i].n_bytes;
        if (nfc_host_commands_keyed(&r.st, table, fr + a, b - a, BYTES0, PAR0, BYTES1, PAR1, r.out.data() + a, r.data.data() + at, r.enc.data() + at,
                                    room, &used) != NFC_OK || used != room)
            return false;
        for (size_t i = a; i < b; i++) r.out[i].byte_off += (uint32_t)at;
        at += used;
    }
    return at == cap;
}

static int count(const Run &r, uint32_t flag) {
    int n = 0;
    for (const nfc_frame &f : r.out) n += (f.flags & flag) != 0;
    return n;
}

int main() {
    nfc_fsm_key_table right, wrong;
    if (nfc_fsm_key_table_init(&right) != NFC_OK || nfc_fsm_key_table_init(&wrong) != NFC_OK) return 1;
    memcpy(right.key[0][1], K0, 6), right.present[0][1] = 1;
    memcpy(right.key[0][2], K1, 6), right.present[0][2] = 1;
    memcpy(right.key[1][3], K2, 6), right.present[1][3] = 1;
    for (int t = 0; t < 2; t++)
        for (int s = 0; s < NFC_KEY_SECTORS; s++) memcpy(wrong.key[t][s], WRONG, 6), wrong.present[t][s] = 1;
    if (nfc_sector_of_block(4) != 1 || nfc_sector_of_block(8) != 2 || nfc_sector_of_block(12) != 3 || nfc_sector_of_block(255) != 39) {
        printf("nfc_sector_of_block: another mapping\n");
        return 1;
    }
    const nfc_fsm_key_table *tables[3] = {&right, &wrong, nullptr};
    const char *names[3] = {"the right table", "the wrong table", "no table"};
    for (int k = 0; k < 3; k++) {
        Run whole;
        if (!run(tables[k], N, whole)) {
            printf("%s: nfc_host_commands_keyed failed\n", names[k]);
            return 1;
        }
        const int ar = count(whole, NFC_FRAME_AR_OK), at = count(whole, NFC_FRAME_AT_OK);
        if (k == 0) {
            int reads = 0;
            for (const nfc_frame &f : whole.out)
                if (f.cmd == READT && f.n_crc == 2 && f.n_extra == 16) {
                    if (reads >= 4 || memcmp(whole.data.data() + f.byte_off, BLOCKS[reads], 16) != 0) {
                        printf("%s: READ answer %d is not its block\n", names[k], reads);
                        return 1;
                    }
                    reads++;
                }
            if (ar != 4 || at != 4 || reads != 4 || whole.st.cur_key != 2 + 1) {
                printf("%s: %d AR OK, %d AT OK, %d READ answers, cur_key %d\n", names[k], ar, at, reads, whole.st.cur_key);
                return 1;
            }
        } else if (at != 0) {
            printf("%s: %d AT OK\n", names[k], at);
            return 1;
        }
        for (size_t cut = 1; cut < N; cut++) {
            Run two;
            if (!run(tables[k], cut, two) || memcmp(&two.st, &whole.st, sizeof whole.st) != 0 ||
                memcmp(two.out.data(), whole.out.data(), N * sizeof(nfc_frame)) != 0 || two.data != whole.data || two.enc != whole.enc) {
                printf("%s: cut before frame %zu: another result than in one piece\n", names[k], cut);
                return 1;
            }
        }
    }
    nfc_fsm_key_table bad = right;
    bad.present[1][39] = 2;
    Run r;
    if (run(&bad, N, r)) {
        printf("a present byte of 2 was accepted\n");
        return 1;
    }
    printf("sector_keys_check: ok\n");
    return 0;
}
