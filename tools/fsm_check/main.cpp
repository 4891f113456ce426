// fsm_check -- the host machine (include/nfc_amd.h: nfc_fsm_*; csrc/protocol.h over csrc/fsm.hip.h) on the first 24 frames of the Classic
// trace (tests/golden/1k_with_enc.out: a first authentication, four encrypted reads, a nested authentication and one more read), by
// every route: packets (nfc_fsm_process_packets, and one by one through nfc_fsm_process with no enc buffer), frames
// (nfc_fsm_process_frames), outgoing in both roles (nfc_fsm_process_outgoing: an emulator sends the plain frames and hears the other
// side), and a state hand-over in the middle of the session.  Every buffer has exactly the capacity the header asks for, so that a write
// past a frame's room is a write past an allocation.
// A stand-alone host program: the way to run the machine's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/fsm_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_commands.hip -o fsm_check && ./fsm_check
// It touches no GPU.  Exit status 0: AR OK and AT OK twice each by the packet and by the frame route, the two routes' records, bytes
// and enc entries equal, every frame sent what the trace has on the air (the nested tag nonce excepted, which the reference's hook sends
// under the old keystream), and the machine handed over mid-session continues as the one that went on.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"

// the packets: type, bits, first byte in BITS (eight bits to a byte, the first lowest)
struct Pk { int type; uint32_t n_bits, at; };
enum { N = 24, RANDTA = 16 };
static const Pk PACKETS[N] = {
    {1, 8, 0},     {0, 18, 1},    {1, 18, 4},    {0, 45, 7},    {1, 81, 13},   {0, 27, 24},   {1, 36, 28},   {0, 36, 33},
    {1, 72, 38},   {0, 36, 47},   {1, 36, 52},   {0, 162, 57},  {1, 36, 78},   {0, 162, 83},  {1, 36, 104},  {0, 162, 109},
    {1, 36, 130},  {0, 162, 135}, {1, 36, 156},  {0, 36, 161},  {1, 72, 166},  {0, 36, 175},  {1, 36, 180},  {0, 162, 185},
};
static const uint8_t BITS[206] = {
    0x26, 0x04, 0x00, 0x02, 0x93, 0x41, 0x00, 0xCD, 0xEC, 0x48, 0xA2, 0xDB, 0x05, 0x93, 0xE1, 0x34, 0xB3, 0x23, 0x89, 0x6E, 0x97, 0x22, 0xDD, 0x01,
    0x08, 0x6C, 0x75, 0x07, 0x60, 0x79, 0x6A, 0x00, 0x04, 0x0E, 0xC2, 0x90, 0xB1, 0x06, 0x78, 0xB5, 0x06, 0x05, 0x0C, 0x85, 0xE0, 0x23, 0x11, 0xCE,
    0x95, 0x35, 0x1C, 0x04, 0x69, 0x58, 0x3D, 0x15, 0x00, 0xBC, 0x5E, 0xF4, 0x8A, 0x55, 0x97, 0x08, 0xCF, 0x6B, 0xD2, 0x51, 0xEE, 0x2C, 0x85, 0x80,
    0x00, 0x22, 0x0C, 0x89, 0x84, 0x00, 0x71, 0xEE, 0x7D, 0x8A, 0x01, 0xE2, 0x32, 0x35, 0x06, 0xF7, 0xD3, 0xD2, 0xBB, 0xE2, 0xD0, 0xA6, 0x93, 0x38,
    0x74, 0xAF, 0xA2, 0x81, 0x2A, 0xA0, 0x2E, 0x03, 0xC1, 0x87, 0x88, 0x90, 0x0C, 0xD2, 0x01, 0x74, 0x3A, 0x94, 0xAD, 0x41, 0x89, 0x39, 0x51, 0x4E,
    0x12, 0x65, 0x56, 0x95, 0x48, 0xA1, 0x4E, 0x44, 0xED, 0x03, 0x27, 0x05, 0x70, 0x0D, 0x02, 0x8B, 0xA2, 0x8D, 0x3B, 0x34, 0xA6, 0x2E, 0x51, 0x1A,
    0x3B, 0x5E, 0x9D, 0x54, 0xD0, 0x9A, 0x30, 0x87, 0x6D, 0xD8, 0x95, 0x00, 0xC6, 0xB9, 0xE9, 0x8E, 0x00, 0x70, 0x7B, 0xB7, 0x0B, 0x0C, 0xFC, 0x34,
    0x68, 0xEC, 0xD0, 0x07, 0xB2, 0x1F, 0x12, 0x87, 0x9B, 0xFE, 0x53, 0x04, 0x31, 0xAC, 0x86, 0x26, 0x0C, 0x64, 0x0A, 0x5B, 0x68, 0xF3, 0xEC, 0x1E,
    0x0F, 0x31, 0xD2, 0x69, 0xEF, 0xFC, 0x82, 0x3A, 0x6E, 0xF4, 0xB5, 0x6C, 0x84, 0x02,
};

struct Result {
    std::vector<nfc_frame> fr;
    std::vector<uint8_t> data;
    std::vector<uint16_t> enc;
    bool operator==(const Result &o) const {
        return fr.size() == o.fr.size() && memcmp(fr.data(), o.fr.data(), fr.size() * sizeof(nfc_frame)) == 0 && data == o.data && enc == o.enc;
    }
};
static int count(const Result &r, uint32_t flag) {
    int n = 0;
    for (const nfc_frame &f : r.fr) n += (f.flags & flag) != 0;
    return n;
}
static int fail(const char *what) {
    printf("fsm_check: %s\n", what);
    return 1;
}

int main() {
    // the bit arrays per type, a byte per bit, as a batch hands them over
    std::vector<uint8_t> bits[2];
    nfc_packet pk[N];
    memset(pk, 0, sizeof pk);
    size_t cap = 0;
    for (int i = 0; i < N; i++) {
        const Pk &p = PACKETS[i];
        pk[i].type = p.type, pk[i].n_bits = p.n_bits, pk[i].bit_off = (uint32_t)bits[p.type].size();
        for (uint32_t k = 0; k < p.n_bits; k++) bits[p.type].push_back((BITS[p.at + k / 8] >> (k % 8)) & 1);
        cap += p.n_bits / 9 + 1;
    }
    nfc_fsm *f = nullptr;
    if (nfc_fsm_create(&f) != NFC_OK) return fail("nfc_fsm_create");

    // 1. the packet route, in one batch
    Result packets;
    packets.fr.assign(N, nfc_frame()), packets.data.assign(cap, 0), packets.enc.assign(cap, 0);
    size_t used = 0;
    if (nfc_fsm_process_packets(f, pk, N, bits[0].data(), bits[1].data(), packets.fr.data(), packets.data.data(), cap, &used, packets.enc.data()) != NFC_OK)
        return fail("nfc_fsm_process_packets");
    packets.data.resize(used), packets.enc.resize(used);
    if (count(packets, NFC_FRAME_AR_OK) != 2 || count(packets, NFC_FRAME_AT_OK) != 2 || count(packets, NFC_FRAME_ENCRYPTED) != 16)
        return fail("the packet route: not two AR OK, two AT OK and sixteen frames inside a session");
    for (const nfc_frame &r : packets.fr)
        if (r.cmd < 0) return fail("the packet route: a frame is no command");

    // ... and one by one, every frame's room its own allocation, no enc buffer; the state in the middle of the session kept for 4.
    nfc_fsm_state mid, end;
    nfc_fsm_reset(f);
    for (int i = 0; i < N; i++) {
        const Pk &p = PACKETS[i];
        std::vector<uint8_t> room(p.n_bits / 9 + 1);
        nfc_frame r;
        if (nfc_fsm_process(f, bits[p.type].data() + pk[i].bit_off, p.n_bits, p.type, &r, room.data(), room.size(), nullptr) != NFC_OK)
            return fail("nfc_fsm_process");
        const nfc_frame &w = packets.fr[i];
        r.byte_off = w.byte_off;
        if (memcmp(&r, &w, sizeof r) != 0 || memcmp(room.data(), packets.data.data() + w.byte_off, w.n_bytes) != 0)
            return fail("one packet at a time: another record or other bytes than in the batch");
        if (i == 11 && nfc_fsm_get_state(f, &mid) != NFC_OK) return fail("nfc_fsm_get_state");
    }
    if (nfc_fsm_get_state(f, &end) != NFC_OK || mid.encrypted != 1 || mid.uid_len != 4) return fail("no session in the middle");

    // 2. the frame route: nine bits to a byte here, the verdicts as the assembly gives them
    std::vector<uint8_t> by[2], par[2];
    nfc_raw_frame raw[N];
    memset(raw, 0, sizeof raw);
    for (int i = 0; i < N; i++) {
        const Pk &p = PACKETS[i];
        const uint8_t *b = bits[p.type].data() + pk[i].bit_off;
        nfc_raw_frame &r = raw[i];
        r.idx = (uint64_t)i, r.type = p.type, r.n_bits = p.n_bits, r.byte_off = (uint32_t)by[p.type].size();
        r.n_bytes = p.n_bits % 9 == 8 ? p.n_bits / 9 + 1 : p.n_bits / 9;   // (a short frame: its eighth bit is the end bit)
        bool ok = r.n_bytes > 0;
        for (uint32_t j = 0; j < r.n_bytes; j++) {
            uint32_t v = 0;
            for (int k = 0; k < 8; k++) v |= (uint32_t)b[9 * j + k] << k;
            const uint32_t ninth = 9 * j + 8 < p.n_bits ? b[9 * j + 8] : (p.type == 0 ? 1u : 0u);
            if ((uint32_t)(__builtin_popcount(v) & 1) == ninth) ok = false;
            by[p.type].push_back((uint8_t)v), par[p.type].push_back((uint8_t)ninth);
        }
        if (ok) {
            r.flags |= NFC_RAW_PARITY_OK;
            uint8_t c[2];
            const uint8_t *d = by[p.type].data() + r.byte_off;
            if (r.n_bytes >= 2 && nfc_crc_a(d, r.n_bytes - 2, c) == NFC_OK && c[0] == d[r.n_bytes - 2] && c[1] == d[r.n_bytes - 1]) r.flags |= NFC_RAW_CRC_A_OK;
        }
    }
    Result frames;
    frames.fr.assign(N, nfc_frame()), frames.data.assign(cap, 0), frames.enc.assign(cap, 0);
    nfc_fsm_reset(f);
    if (nfc_fsm_process_frames(f, raw, N, by[0].data(), par[0].data(), by[1].data(), par[1].data(), frames.fr.data(), frames.data.data(), cap, &used,
                               frames.enc.data()) != NFC_OK)
        return fail("nfc_fsm_process_frames");
    frames.data.resize(used), frames.enc.resize(used);
    if (count(frames, NFC_FRAME_AR_OK) != 2 || count(frames, NFC_FRAME_AT_OK) != 2) return fail("the frame route: not two AR OK and two AT OK");
    if (!(frames == packets)) return fail("the packet and the frame route differ");
    nfc_fsm_state st;
    if (nfc_fsm_get_state(f, &st) != NFC_OK || memcmp(&st, &end, sizeof st) != 0) return fail("the two routes leave different states");

    // 3. outgoing, the emulator as the tag (0) and as the reader (1): it sends the plain frames -- the bytes the monitor decoded, with
    // their odd parity -- and hears the other side's frames as they were on the air
    for (int role = 0; role < 2; role++) {
        nfc_fsm_reset(f);
        bool in_session = false;
        int sent = 0, encrypted = 0;
        for (int i = 0; i < N; i++) {
            const Pk &p = PACKETS[i];
            const nfc_frame &w = packets.fr[i];
            const uint8_t *air = bits[p.type].data() + pk[i].bit_off;
            if (p.type != role) {
                std::vector<uint8_t> room(p.n_bits / 9 + 1);
                std::vector<uint16_t> enc(p.n_bits / 9 + 1);
                nfc_frame r;
                if (nfc_fsm_process(f, air, p.n_bits, p.type, &r, room.data(), room.size(), enc.data()) != NFC_OK || r.cmd != w.cmd)
                    return fail("the emulator hears another command than the monitor");
                continue;
            }
            std::vector<uint8_t> plain;
            if (p.n_bits == 8) plain.assign(air, air + 8);   // REQA: seven bits and the end bit
            else
                for (uint32_t j = 0; j < w.n_bytes; j++) {
                    const uint32_t v = packets.data[w.byte_off + j];
                    for (int k = 0; k < 8; k++) plain.push_back((v >> k) & 1);
                    plain.push_back((uint8_t)(1 - (__builtin_popcount(v) & 1)));
                }
            if (plain.size() != p.n_bits) return fail("a plain frame of another length than the one on the air");
            std::vector<uint8_t> out(plain.size());
            if (nfc_fsm_process_outgoing(f, plain.data(), plain.size(), w.cmd, out.data()) != 0) return fail("nfc_fsm_process_outgoing");
            const bool as_air = memcmp(out.data(), air, out.size()) == 0;
            if (w.cmd == RANDTA && in_session ? (as_air || out == plain) : !as_air) return fail("a frame sent is not what the trace has on the air");
            if (w.cmd == RANDTA) in_session = true;
            sent++, encrypted += out != plain;
        }
        if (sent != 12 || encrypted != 8) return fail("outgoing: not twelve frames sent, eight of them encrypted");
    }

    // 4. the hand-over in the middle of the session: another machine continues from the plain state
    nfc_fsm *g = nullptr;
    if (nfc_fsm_create(&g) != NFC_OK || nfc_fsm_set_state(g, &mid) != NFC_OK) return fail("nfc_fsm_set_state");
    if (nfc_fsm_get_state(g, &st) != NFC_OK || memcmp(&st, &mid, sizeof st) != 0) return fail("set_state / get_state: another state");
    for (int i = 12; i < N; i++) {
        const Pk &p = PACKETS[i];
        std::vector<uint8_t> room(p.n_bits / 9 + 1);
        std::vector<uint16_t> enc(p.n_bits / 9 + 1);
        nfc_frame r;
        if (nfc_fsm_process(g, bits[p.type].data() + pk[i].bit_off, p.n_bits, p.type, &r, room.data(), room.size(), enc.data()) != NFC_OK) return fail("nfc_fsm_process");
        const nfc_frame &w = packets.fr[i];
        r.byte_off = w.byte_off;
        if (memcmp(&r, &w, sizeof r) != 0 || memcmp(room.data(), packets.data.data() + w.byte_off, w.n_bytes) != 0 ||
            memcmp(enc.data(), packets.enc.data() + w.byte_off, w.n_enc * sizeof(uint16_t)) != 0)
            return fail("the machine handed over continues differently");
    }
    if (nfc_fsm_get_state(g, &st) != NFC_OK || memcmp(&st, &end, sizeof st) != 0) return fail("the machine handed over ends in another state");
    mid.uid_len = 33;
    if (nfc_fsm_set_state(g, &mid) != NFC_ERR_ARG) return fail("a UID of 33 bytes was accepted");
    nfc_fsm_destroy(g);
    nfc_fsm_destroy(f);
    printf("fsm_check: ok\n");
    return 0;
}
