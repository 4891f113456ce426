// image_check -- nfc_host_card_image, the CPU twin of k_multi_images (include/nfc_amd.h; csrc/image.hip.h), over random
// command lists: records of every command and of the three negative ones, with random flags, block numbers up to 255 and extra bytes, in
// heap blocks of exactly the size the records name.  Every list is run whole, and cut into two and into three calls at random places
// with the image handed on: the pieces must give the whole's image, tail included.  Lists whose last record reaches one byte past `data`
// must be refused with the image untouched.
// A stand-alone host program: the way to run the twin's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/image_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_image.hip usrp_nfc_amd/csrc/nfc_commands.hip -o image_check && ./image_check
// It touches no GPU.  Exit status 0: every comparison held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/nfc_amd.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct List {
    std::vector<nfc_frame> cmds;
    std::unique_ptr<uint8_t[]> data;   // exactly data_len bytes: a read past the end is the sanitizer's
    size_t data_len = 0;
};

// the commands an image reads and what surrounds them, looked up BY NAME in the library's table (READR / READT twice: they are the
// commonest in a card's reading); the three negative ones behind them
static const char *const PICK_NAMES[] = {"ATQAUL", "ATQA1K", "ATQADS", "ANTI1U", "ANTI1G", "ANTI2T", "AUTHA", "AUTHB", "RANDTA", "RANDRB", "RANDTB",
                                         "READR", "READT", "READR", "READT", "WRITE", "COMPW1", "COMPW2", "REQA", "HALT"};
static std::vector<int> PICK;
static void fill_pick() {
    for (const char *name : PICK_NAMES) {
        int found = -1;
        for (int c = 0; c < nfc_command_count(); c++) {
            nfc_command_info info;
            if (nfc_command_get(c, &info) == NFC_OK && strcmp(info.name, name) == 0) {
                found = c;
                break;
            }
        }
        if (found < 0) {
            fprintf(stderr, "image_check: the command table has no %s\n", name);
            exit(2);
        }
        PICK.push_back(found);
    }
    // (ATQA4K carries the 1K name in the table, as in the reference: it is the entry behind ATQA1K)
    PICK.push_back(PICK[1] + 1);
    for (int bad : {(int)NFC_CMD_UNKNOWN, (int)NFC_CMD_PARITY_ERROR, (int)NFC_CMD_CUT}) PICK.push_back(bad);
}

static List make(size_t n) {
    List L;
    std::vector<uint8_t> bytes;
    const int n_cmds = nfc_command_count();
    for (size_t i = 0; i < n; i++) {
        nfc_frame f;
        memset(&f, 0, sizeof f);
        int cmd = rnd() % 8 ? PICK[rnd() % PICK.size()] : (int)(rnd() % (uint32_t)n_cmds);
        f.cmd = cmd;
        f.byte_off = (uint32_t)bytes.size();
        f.flags = rnd() % 3 ? (rnd() & 0xFFu) : (NFC_FRAME_ENCRYPTED | NFC_FRAME_AR_OK | NFC_FRAME_AT_OK);
        if (cmd >= 0) {
            nfc_command_info info;
            if (nfc_command_get(cmd, &info) != NFC_OK) exit(2);
            f.type = info.type;
            f.n_header = (uint16_t)info.n_header;
            f.n_extra = (uint16_t)info.n_extra;
            f.n_crc = info.crc ? 2 : 0;
            if (rnd() % 16 == 0) f.n_extra = (uint16_t)(rnd() % 20);   // (a record the machine would not write: the twin still stays inside it)
            f.n_bytes = (uint16_t)(f.n_header + f.n_extra + f.n_crc);
            if (rnd() % 32 == 0 && f.n_bytes) f.n_bytes--;               // ... nor this one: extra bytes behind the record's end are not read
        } else if (cmd == NFC_CMD_UNKNOWN) {
            f.type = (int32_t)(rnd() & 1u);
            f.n_extra = f.n_bytes = (uint16_t)(rnd() % 24);
        }
        for (uint32_t j = 0; j < f.n_bytes; j++) bytes.push_back((uint8_t)(rnd() % 3 ? rnd() : rnd() % 70));
        L.cmds.push_back(f);
    }
    L.data_len = bytes.size();
    L.data.reset(new uint8_t[L.data_len ? L.data_len : 1]);
    if (L.data_len) memcpy(L.data.get(), bytes.data(), L.data_len);
    return L;
}

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);    \
            fails++;                                                    \
        }                                                               \
    } while (0)

int main() {
    fill_pick();
    uint8_t key_a[6] = {0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5}, key_b[6] = {0xB0, 0xB1, 0xB2, 0xB3, 0xB4, 0xB5};
    nfc_fsm_key_table table;
    nfc_fsm_key_table_init(&table);
    for (int s = 0; s < NFC_KEY_SECTORS; s += 3) {
        table.present[s & 1][s] = 1;
        for (int i = 0; i < 6; i++) table.key[s & 1][s][i] = (uint8_t)(0x10 * s + i);
    }
    size_t total = 0, known = 0, flagged = 0;
    for (int round = 0; round < 4000; round++) {
        const size_t n = rnd() % 200;
        const List L = make(n);
        const nfc_fsm_key_table *tab = round % 2 ? &table : nullptr;
        std::unique_ptr<nfc_card_image> whole(new nfc_card_image), parts(new nfc_card_image);
        nfc_card_image_init(whole.get());
        CHECK(nfc_host_card_image(whole.get(), L.cmds.data(), n, L.data.get(), L.data_len, key_a, key_b, tab) == NFC_OK);
        uint32_t cnt = 0;
        for (int i = 0; i < NFC_IMG_BYTES; i++) cnt += whole->src[i] != 0;
        CHECK(cnt == whole->info.n_known);
        total += n, known += cnt, flagged += whole->info.flags != 0;
        for (int pieces = 2; pieces <= 3; pieces++) {
            size_t c1 = n ? rnd() % (n + 1) : 0, c2 = pieces == 3 && n ? rnd() % (n + 1) : n;
            if (pieces == 2) c2 = n;
            if (c2 < c1) std::swap(c1, c2);
            nfc_card_image_init(parts.get());
            const size_t cut[4] = {0, c1, c2, n};
            for (int p = 0; p < 3; p++)
                CHECK(nfc_host_card_image(parts.get(), L.cmds.data() + cut[p], cut[p + 1] - cut[p], L.data.get(), L.data_len, key_a, key_b, tab) == NFC_OK);
            CHECK(memcmp(parts.get(), whole.get(), sizeof(nfc_card_image)) == 0);
        }
        // one byte short: refused as soon as a record that is read reaches past it, the image as it was
        if (L.data_len) {
            nfc_card_image_init(parts.get());
            nfc_card_image before = *parts;
            const int rc = nfc_host_card_image(parts.get(), L.cmds.data(), n, L.data.get(), L.data_len - 1, key_a, key_b, tab);
            CHECK(rc == NFC_OK || (rc == NFC_ERR_ARG && memcmp(parts.get(), &before, sizeof before) == 0));
        }
    }
    CHECK(total > 100000 && known > 10000 && flagged > 1000);   // (the lists do patch, and do raise flags)
    nfc_card_image bad;
    nfc_card_image_init(&bad);
    bad.src[7] = 9;
    CHECK(nfc_host_card_image(&bad, nullptr, 0, nullptr, 0, key_a, key_b, nullptr) == NFC_ERR_ARG);
    printf("image_check: %zu commands in 4000 lists, %zu known bytes, %zu flagged images: %s\n", total, known, flagged, fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
