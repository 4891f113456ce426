// fsm.hip.h -- THE protocol machine (fsm.py, command.py, cipher.py, lfsr.py of the reference; "next" rows f1 and f3 of SURVEY.md 8f), one
// text for host and device, without vectors and without allocation: one frame as the GPU assembled it (nfc_raw_frame, its bytes and
// ninth bits) in, one nfc_frame record, the plaintext and the `enc` entries out.  What the reference does per packet in fsm.process_bits
// (fsm.py:218-238): find the command by the protocol stage of the previous command and the leading bytes (command.py:166-199, with the
// CRC_A of utilities.py:26-46 and the BCC xor check of command.py:44-67), split it into header / extra / CRC (command.py:245-253), track
// tag type and UID (fsm.py:165-216), and decrypt the frames of a MIFARE Classic session before the parity check, nested authentications
// included (fsm.py:133-154,197-213).  Three holders instantiate it: k_multi_commands (multi_commands.hip.h) a lane per stream,
// nfc_host_commands, its twin on the CPU, and the host machine nfc_fsm (protocol.h), whose UID is unbounded.  What pins it:
// the reference's own text on malformed traffic and what the project's first, separate host machine made of the same rows
// (tests/test_fsm_fuzz.py, tests/test_fsm_parent.py).
//
// Form.  The machine lives in named scalars (Machine): the 48-bit cipher register in a uint64, ar / at and the keys as integers (byte 0
// lowest).  The UID is reached through an accessor -- uid_len(M), uid_byte(M, i), uid_clear(M), uid_append(M, B, from, n),
// overloaded on the machine's type -- as the key table is through Table (sector_keys.h).  A Machine's own,
// the kernel's and the twin's, is eight words reached through select chains -- nothing is an array with a dynamic index, so a lane
// needs no scratch -- and holds 32 bytes; the host machine derives from Machine and keeps a vector (protocol.h).
// Only a frame of at most 18 bytes can be a command (the longest total() of the table: READT / COMPW2), so the lookup sees
// the frame through five words (Bytes); the CRC_A register runs two bytes behind the byte loop as in assemble_frame (frames.hip.h).
// CRYPTO1 is bit-serial: per clock the filter reads 20 fixed register bits through truth-table words that a constexpr builds from fa /
// fb / fc as cipher.py:97-107 states them, and the feedback is the parity of popcount(st & TAPS), TAPS built from the eighteen taps.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"
#include "frames.hip.h"
#include "sector_keys.h"

namespace nfc {

// ---- ISO 14443-3 type A CRC (utilities.py:30-41): reflected 0x8408, initial 0x6363, low byte first ----
inline uint16_t crc_a(const uint8_t *data, size_t n) {
    uint32_t w = 0x6363u;
    for (size_t i = 0; i < n; i++) w = frames::crc_a_step(w, data[i]);
    return (uint16_t)w;
}

namespace fsmd {

#define NFC_HD __host__ __device__ __forceinline__

// ---- the command table (command.py:78-118, in its order: a command's number is its index; nfc_command_get names them) ----
// type: 0 tag -> reader, 1 reader -> tag (packets.py:18-20); crc: the frame ends with CRC_A; xor_check: -1 none, else the xor of the extra
// bytes, seeded with it, must be 0.  (ATQA4K carries the 1K name in the reference, command.py:84.)
enum {
    C_REQA, C_WUPA, C_ATQAUL, C_ATQA1K, C_ATQA4K, C_ATQADS, C_ANTI1R, C_ANTI1U, C_ANTI1G, C_SEL1R, C_SEL1U,
    C_SEL1K, C_ANTI2R, C_ANTI2T, C_AUTHA, C_AUTHB, C_RANDTA, C_RANDRB, C_RANDTB, C_SEL2R, C_SEL2T, C_READR,
    C_READT, C_HALT, C_WRITE, C_COMPW1, C_COMPW2, C_COUNT
};
constexpr int MAX_COMMAND_BYTES = 18;
// stage | n_header << 4 | type << 6 | crc << 7 | n_extra << 8 | has_xor << 13 | xor seed << 16 | header[0] << 24; header[1] apart
constexpr uint32_t def_word(int stage, int n_header, int h0, int type, int crc, int n_extra, int xor_check) {
    return (uint32_t)stage | (uint32_t)n_header << 4 | (uint32_t)type << 6 | (uint32_t)crc << 7 | (uint32_t)n_extra << 8 |
           (xor_check >= 0 ? 1u << 13 | (uint32_t)xor_check << 16 : 0u) | (uint32_t)h0 << 24;
}
struct Def {
    uint32_t w, h1;
    NFC_HD constexpr int stage() const { return (int)(w & 15u); }
    NFC_HD constexpr int n_header() const { return (int)((w >> 4) & 3u); }
    NFC_HD constexpr int type() const { return (int)((w >> 6) & 1u); }
    NFC_HD constexpr int crc() const { return (int)((w >> 7) & 1u); }
    NFC_HD constexpr int n_extra() const { return (int)((w >> 8) & 31u); }
    NFC_HD constexpr int xor_check() const { return (w >> 13) & 1u ? (int)((w >> 16) & 0xFFu) : -1; }
    NFC_HD constexpr uint32_t h0() const { return w >> 24; }
    NFC_HD constexpr int total() const { return n_header() + n_extra() + 2 * crc(); }
};
NFC_HD constexpr Def def_of(int cmd) {
    switch (cmd) {
    case C_REQA: return Def{def_word(0, 1, 0x26, 1, 0, 0, -1), 0};
    case C_WUPA: return Def{def_word(0, 1, 0x52, 1, 0, 0, -1), 0};
    case C_ATQAUL: return Def{def_word(0, 2, 0x44, 0, 0, 0, -1), 0x00};
    case C_ATQA1K: return Def{def_word(0, 2, 0x04, 0, 0, 0, -1), 0x00};
    case C_ATQA4K: return Def{def_word(0, 2, 0x02, 0, 0, 0, -1), 0x00};
    case C_ATQADS: return Def{def_word(0, 2, 0x03, 0, 0, 0, -1), 0x44};
    case C_ANTI1R: return Def{def_word(1, 2, 0x93, 1, 0, 0, -1), 0x20};
    case C_ANTI1U: return Def{def_word(1, 1, 0x88, 0, 0, 4, 0x88), 0};
    case C_ANTI1G: return Def{def_word(1, 0, 0, 0, 0, 5, 0), 0};
    case C_SEL1R: return Def{def_word(2, 2, 0x93, 1, 1, 5, 0), 0x70};
    case C_SEL1U: return Def{def_word(2, 1, 0x04, 0, 1, 0, -1), 0};
    case C_SEL1K: return Def{def_word(2, 1, 0x08, 0, 1, 0, -1), 0};
    case C_ANTI2R: return Def{def_word(3, 2, 0x95, 1, 0, 0, -1), 0x20};
    case C_ANTI2T: return Def{def_word(3, 0, 0, 0, 0, 5, 0), 0};
    case C_AUTHA: return Def{def_word(3, 1, 0x60, 1, 1, 1, -1), 0};
    case C_AUTHB: return Def{def_word(3, 1, 0x61, 1, 1, 1, -1), 0};
    case C_RANDTA: return Def{def_word(3, 0, 0, 0, 0, 4, -1), 0};
    case C_RANDRB: return Def{def_word(4, 0, 0, 1, 0, 8, -1), 0};
    case C_RANDTB: return Def{def_word(4, 0, 0, 0, 0, 4, -1), 0};
    case C_SEL2R: return Def{def_word(4, 2, 0x95, 1, 1, 5, 0), 0x70};
    case C_SEL2T: return Def{def_word(4, 1, 0x00, 0, 1, 0, -1), 0};
    case C_READR: return Def{def_word(5, 1, 0x30, 1, 1, 1, -1), 0};
    case C_READT: return Def{def_word(5, 0, 0, 0, 1, 16, -1), 0};
    case C_HALT: return Def{def_word(10, 2, 0x50, 1, 1, 0, -1), 0x00};
    case C_WRITE: return Def{def_word(6, 1, 0xA2, 1, 1, 5, -1), 0};
    case C_COMPW1: return Def{def_word(6, 1, 0xA0, 1, 1, 1, -1), 0};
    default: return Def{def_word(7, 0, 0, 1, 1, 16, -1), 0};   // C_COMPW2
    }
}
constexpr int longest_command() {
    int m = 0;
    for (int c = 0; c < C_COUNT; c++) m = def_of(c).total() > m ? def_of(c).total() : m;
    return m;
}
static_assert(longest_command() == MAX_COMMAND_BYTES, "the lookup inspects frames of up to MAX_COMMAND_BYTES bytes: the longest command");
// candidates per protocol stage and direction, in the reference's order (command.py:120-137), four to a word, 0xFF: none.  The reader
// table has stages 0 .. 7 and 10: the reference tests `stage < number of entries (9)` and then indexes by stage (stage 8 would raise
// KeyError there; no command has stage 7 + 1 as its successor in a trace)
constexpr uint32_t cand4(int a, int b = 0xFF, int c = 0xFF, int d = 0xFF) {
    return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16 | (uint32_t)d << 24;
}
NFC_HD uint32_t tag_stage(int v) {
    switch (v) {
    case 0: return cand4(C_ATQAUL, C_ATQA1K, C_ATQA4K, C_ATQADS);
    case 1: return cand4(C_ANTI1U, C_ANTI1G);
    case 2: return cand4(C_SEL1U, C_SEL1K);
    case 3: return cand4(C_ANTI2T, C_RANDTA);
    case 4: return cand4(C_SEL2T, C_RANDTB);
    case 5: return cand4(C_READT);
    default: return 0xFFFFFFFFu;   // (v >= 6: the reference has no entry)
    }
}
NFC_HD uint32_t reader_stage(int v) {
    switch (v) {
    case 0: return cand4(C_REQA, C_WUPA);
    case 1: return cand4(C_ANTI1R);
    case 2: return cand4(C_SEL1R);
    case 3: return cand4(C_ANTI2R, C_AUTHA, C_AUTHB);
    case 4: return cand4(C_SEL2R, C_RANDRB);
    case 5: return cand4(C_READR);
    case 6: return cand4(C_WRITE, C_COMPW1);
    case 7: return cand4(C_COMPW2);
    default: return 0xFFFFFFFFu;   // (v >= 8)
    }
}

// ---- CRYPTO1 (cipher.py) ----
// A 48-bit shift register, bit i of st the i-th oldest bit (cipher.py keeps the whole bit history and looks at its last 48); a key's bytes
// least significant bit first ARE the register (cipher.py:11-12).  One filter bit per clock; a clock shifts in L(st) ^ input.
constexpr int fa(int a, int b, int c, int d) { return ((a | b) ^ (a & d)) ^ (c & ((a ^ b) | d)); }
constexpr int fb(int a, int b, int c, int d) { return ((a & b) | c) ^ ((a ^ b) & (c | d)); }
constexpr int fc(int a, int b, int c, int d, int e) { return (a | ((b | e) & (d ^ e))) ^ ((a ^ (b & d)) & ((c ^ d) | (b & e))); }
// truth tables: bit (a | b << 1 | c << 2 | d << 3 [| e << 4]) of the word is the function's value
constexpr uint32_t table_fa() {
    uint32_t t = 0;
    for (int i = 0; i < 16; i++) t |= (uint32_t)(fa(i & 1, (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1) & 1) << i;
    return t;
}
constexpr uint32_t table_fb() {
    uint32_t t = 0;
    for (int i = 0; i < 16; i++) t |= (uint32_t)(fb(i & 1, (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1) & 1) << i;
    return t;
}
constexpr uint32_t table_fc() {
    uint32_t t = 0;
    for (int i = 0; i < 32; i++) t |= (uint32_t)(fc(i & 1, (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1, (i >> 4) & 1) & 1) << i;
    return t;
}
constexpr uint64_t taps_mask() {
    const int taps[18] = {0, 5, 9, 10, 12, 14, 15, 17, 19, 24, 25, 27, 29, 35, 39, 41, 42, 43};   // cipher.py:75-76
    uint64_t m = 0;
    for (int i = 0; i < 18; i++) m |= 1ull << taps[i];
    return m;
}
constexpr uint32_t TT_FA = table_fa(), TT_FB = table_fb(), TT_FC = table_fc();
constexpr uint64_t TAPS = taps_mask(), ST_MASK = (1ull << 48) - 1;

// register bits p, p + 2, p + 4, p + 6 as a four-bit index
NFC_HD uint32_t quad(uint64_t st, int p) {
    const uint32_t x = (uint32_t)(st >> p);
    return (x & 1u) | ((x >> 1) & 2u) | ((x >> 2) & 4u) | ((x >> 3) & 8u);
}
NFC_HD uint32_t filter(uint64_t st) {   // cipher.py:110-118
    const uint32_t a = (TT_FA >> quad(st, 9)) & 1u, b = (TT_FB >> quad(st, 17)) & 1u, c = (TT_FB >> quad(st, 25)) & 1u;
    const uint32_t d = (TT_FA >> quad(st, 33)) & 1u, e = (TT_FB >> quad(st, 41)) & 1u;
    return (TT_FC >> (a | b << 1 | c << 2 | d << 3 | e << 4)) & 1u;
}
NFC_HD uint32_t feedback(uint64_t st) { return (uint32_t)__builtin_popcountll(st & TAPS) & 1u; }
NFC_HD uint64_t shift_in(uint64_t st, uint32_t in) { return (st >> 1) | ((uint64_t)((feedback(st) ^ in) & 1u) << 47); }
// the nonce register (lfsr.py, taps 16 18 19 21) `ticks` clocks on: bit j of x is the j-th oldest of the 32 bits.  The expected reader /
// tag answers are the tag nonce after 64 and after 96 clocks (cipher.py:37-42)
NFC_HD uint32_t nonce_advance(uint32_t x, int ticks) {
    for (int t = 0; t < ticks; t++) x = (x >> 1) | ((((x >> 16) ^ (x >> 18) ^ (x >> 19) ^ (x >> 21)) & 1u) << 31);
    return x;
}

// ---- the machine in scalars ----
struct Machine {
    int32_t cur_cmd, tag_type, encrypted, cur_key;   // encrypted: 0, 1 a session, 2 a session whose ar / at nothing equals; cur_key: 0 / 1 key A / B, 2 + slot of the sector key table (sector_keys.h)
    uint64_t st, key_a, key_b;   // 48 bits each; a key's byte 0 lowest: load_key's bit order makes the key the register
    uint32_t ar, at;             // byte 0 lowest
    uint32_t uid_len, flags;
    uint32_t u0, u1, u2, u3, u4, u5, u6, u7;
};
constexpr uint32_t UID_CAP = 32;

NFC_HD uint32_t uid_byte(const Machine &M, uint32_t i) {
    const uint32_t j = i >> 2;
    const uint32_t w = j == 0 ? M.u0 : j == 1 ? M.u1 : j == 2 ? M.u2 : j == 3 ? M.u3 : j == 4 ? M.u4 : j == 5 ? M.u5 : j == 6 ? M.u6 : M.u7;
    return (w >> (8u * (i & 3u))) & 0xFFu;
}
NFC_HD void uid_put(Machine &M, uint32_t i, uint32_t b) {
    const uint32_t j = i >> 2, sh = 8u * (i & 3u), keep = ~(0xFFu << sh), v = (b & 0xFFu) << sh;
    M.u0 = j == 0 ? (M.u0 & keep) | v : M.u0;
    M.u1 = j == 1 ? (M.u1 & keep) | v : M.u1;
    M.u2 = j == 2 ? (M.u2 & keep) | v : M.u2;
    M.u3 = j == 3 ? (M.u3 & keep) | v : M.u3;
    M.u4 = j == 4 ? (M.u4 & keep) | v : M.u4;
    M.u5 = j == 5 ? (M.u5 & keep) | v : M.u5;
    M.u6 = j == 6 ? (M.u6 & keep) | v : M.u6;
    M.u7 = j == 7 ? (M.u7 & keep) | v : M.u7;
}
NFC_HD void uid_clear(Machine &M) {
    M.uid_len = 0;
    M.u0 = M.u1 = M.u2 = M.u3 = M.u4 = M.u5 = M.u6 = M.u7 = 0;
}
NFC_HD void machine_init(Machine &M) {   // nfc_fsm_reset
    M.cur_cmd = C_REQA;
    M.tag_type = -1;
    M.encrypted = 0;
    M.cur_key = 0;
    M.st = 0;
    M.key_a = M.key_b = ST_MASK;
    M.ar = M.at = 0;
    M.flags = 0;
    uid_clear(M);
}

// a frame's first 20 bytes.  On the device five words reached through select chains (no array a lane would index); on the host, where an
// index costs nothing and a select chain per byte is what a clear-text frame would spend most of its time in, twenty bytes.  Only the
// storage differs: at / put / word_at mean the same in both.
struct Bytes {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t w0, w1, w2, w3, w4;
    NFC_HD uint32_t at(uint32_t i) const {
        const uint32_t j = i >> 2;
        const uint32_t w = j == 0 ? w0 : j == 1 ? w1 : j == 2 ? w2 : j == 3 ? w3 : w4;
        return (w >> (8u * (i & 3u))) & 0xFFu;
    }
    NFC_HD void put(uint32_t i, uint32_t b) {   // (into a cleared word, i < 20)
        const uint32_t j = i >> 2, v = (b & 0xFFu) << (8u * (i & 3u));
        w0 |= j == 0 ? v : 0u;
        w1 |= j == 1 ? v : 0u;
        w2 |= j == 2 ? v : 0u;
        w3 |= j == 3 ? v : 0u;
        w4 |= j == 4 ? v : 0u;
    }
#else
    uint8_t b[20];
    uint32_t at(uint32_t i) const { return b[i < 20u ? i : 19u]; }
    void put(uint32_t i, uint32_t v) { b[i] = (uint8_t)v; }   // (i < 20)
#endif
    NFC_HD uint32_t word_at(uint32_t i) const { return at(i) | at(i + 1) << 8 | at(i + 2) << 16 | at(i + 3) << 24; }   // i + 3 < 20
};

struct Rec {
    int32_t cmd, type;
    uint32_t flags, n_bytes, n_header, n_extra, n_crc, n_enc;
};

// command.py:44-67.  crc_ok: the last two of the n bytes are the CRC_A of those before them.
NFC_HD bool compatible(const Def &c, const Bytes &B, int n, bool crc_ok) {
    if (c.total() != n) return false;
    if (c.n_header() >= 1 && c.h0() != B.at(0)) return false;
    if (c.n_header() >= 2 && c.h1 != B.at(1)) return false;
    int end = n;
    if (c.crc()) {
        end -= 2;
        if (!crc_ok) return false;
    }
    if (c.xor_check() >= 0) {
        uint32_t a = (uint32_t)c.xor_check();
#pragma unroll
        for (int i = 0; i < MAX_COMMAND_BYTES; i++)
            if (i >= c.n_header() && i < end) a ^= B.at((uint32_t)i);
        if (a != 0) return false;
    }
    return true;
}
NFC_HD int first_compatible(uint32_t cands, const Bytes &B, int n, bool crc_ok) {
    for (int k = 0; k < 4; k++) {
        const int c = (int)((cands >> (8 * k)) & 0xFFu);
        if (c == 0xFF) break;
        if (compatible(def_of(c), B, n, crc_ok)) return c;
    }
    return -1;
}
// command.py:166-199, for 1 <= n <= MAX_COMMAND_BYTES: by the stage of the previous command and the one behind it, then by leading bytes
NFC_HD int find_command(const Bytes &B, int n, int type, int prev_cmd, bool crc_ok) {
    const int ind = def_of(prev_cmd).stage();
    for (int v = ind; v <= ind + 1; v++) {
        const int c = first_compatible(type == 0 ? tag_stage(v) : reader_stage(v), B, n, crc_ok);
        if (c >= 0) return c;
    }
    // command.py:139-164: the first listed option, or the second when the second byte names it (no second byte, or one that names nothing:
    // IndexError / KeyError in the reference, caught: no command)
    int o0 = -1, o1 = -1;
    switch (B.at(0)) {
    case 0x00: o0 = C_SEL2T; break;
    case 0x02: o0 = C_ATQA4K; break;
    case 0x03: o0 = C_ATQADS; break;
    case 0x04: o0 = C_SEL1U; o1 = C_ATQA1K; break;
    case 0x08: o0 = C_SEL1K; break;
    case 0x26: o0 = C_REQA; break;
    case 0x30: o0 = C_READR; break;
    case 0x44: o0 = C_ATQAUL; break;
    case 0x50: o0 = C_HALT; break;
    case 0x52: o0 = C_WUPA; break;
    case 0x60: o0 = C_AUTHA; break;
    case 0x61: o0 = C_AUTHB; break;
    case 0x88: o0 = C_ANTI1U; break;
    case 0x93: o0 = C_ANTI1R; o1 = C_SEL1R; break;
    case 0x95: o0 = C_ANTI2R; o1 = C_SEL2R; break;
    case 0xA0: o0 = C_COMPW1; break;
    case 0xA2: o0 = C_WRITE; break;
    default: return -1;
    }
    int option = o0;
    if (o1 >= 0) {
        if (n < 2) return -1;
        bool named;
        switch (B.at(1)) {
        case 0x00: named = (o1 == C_ATQAUL || o1 == C_HALT || o1 == C_ATQA1K); break;
        case 0x20: named = (o1 == C_ANTI1R || o1 == C_ANTI2R); break;
        case 0x70: named = (o1 == C_SEL1R || o1 == C_SEL2R); break;
        default: return -1;
        }
        if (named) option = o1;
    }
    return compatible(def_of(option), B, n, crc_ok) ? option : -1;
}

// The rest of the UID accessor for the Machine's own eight words (uid_byte and uid_clear: above).
NFC_HD uint32_t uid_len(const Machine &M) { return M.uid_len; }
// the UID grows by the n bytes at B[from ..): not made when it would pass UID_CAP (the host machine's holder is unbounded)
NFC_HD void uid_append(Machine &M, const Bytes &B, uint32_t from, uint32_t n) {
    if (M.uid_len + n > UID_CAP) {
        M.flags |= NFC_FSM_UID_OVERFLOW;
        return;
    }
    for (uint32_t j = 0; j < n; j++) uid_put(M, M.uid_len + j, B.at(from + j));
    M.uid_len += n;
}

// The bytes -> command, record, tag type / UID / session state (fsm.py:165-216, 225-238).  nb plaintext bytes (0: a parity error, or
// nothing left), the first 20 of them in B.  Mach: a Machine, or one derived from it with a UID holder of its own.  tab: the stream's
// sector key table (sector_keys.h), read only where an AUTH command is recognised and where a nonce loads the register.
template <class Mach, class Table>
NFC_HD void finish(Mach &M, uint32_t nb, int type, Rec &out, const Bytes &B, bool crc_ok, const Table &tab) {
    if (nb == 0) {   // `if not bytes` (fsm.py:225)
        out.cmd = NFC_CMD_PARITY_ERROR;
        return;
    }
    out.n_bytes = nb;
    // (a frame longer than the longest command is UNKNOWN without inspection: every route of find_command ends in total() == n)
    const int cmd = nb <= (uint32_t)MAX_COMMAND_BYTES ? find_command(B, (int)nb, type, M.cur_cmd, crc_ok) : -1;
    if (cmd < 0) {
        out.cmd = NFC_CMD_UNKNOWN;
        out.n_extra = nb;
        return;
    }
    M.cur_cmd = cmd;
    out.cmd = cmd;
    const Def c = def_of(cmd);
    const uint32_t h = (uint32_t)c.n_header();
    out.n_header = h;
    out.n_crc = c.crc() ? 2u : 0u;
    out.n_extra = nb - h - out.n_crc;
    switch (cmd) {
    case C_REQA: case C_WUPA: case C_HALT:   // fsm.py:20-24
        uid_clear(M);
        M.tag_type = -1;
        M.encrypted = 0;
        break;
    case C_ATQAUL: M.tag_type = 0; break;   // command.py:70-74
    case C_ATQA1K: M.tag_type = 1; break;
    case C_ATQA4K: M.tag_type = 2; break;
    case C_ATQADS: M.tag_type = 3; break;
    case C_ANTI1U: uid_append(M, B, h, 3); break;
    case C_ANTI1G: uid_append(M, B, h, 4); break;
    case C_SEL1R: {
        const uint32_t start = M.tag_type == 0 ? 1u : 0u, n = 4u - start;
        bool same = uid_len(M) == n;
        for (uint32_t j = 0; j < n; j++) same = same && uid_byte(M, j) == B.at(h + start + j);
        if (!same) {
            out.flags |= NFC_FRAME_UID_MISMATCH;
            uid_clear(M);
            uid_append(M, B, h + start, n);
        }
        break;
    }
    case C_ANTI2T: uid_append(M, B, h, 4); break;
    case C_SEL2R: {   // (uid_byte of an index at or past the holder's end is some byte or none, never a fault: `same` is false by then)
        bool same = uid_len(M) >= 4u;
        for (uint32_t j = 0; j < 4u; j++) same = same && uid_byte(M, uid_len(M) - 4u + j) == B.at(h + j);
        if (!same) {
            out.flags |= NFC_FRAME_UID_MISMATCH;
            uid_append(M, B, h, 4);
        }
        break;
    }
    case C_AUTHA: M.cur_key = skeys::choose(tab, 0u, B.at(h)); break;
    case C_AUTHB: M.cur_key = skeys::choose(tab, 1u, B.at(h)); break;
    case C_RANDTA:
        if (!M.encrypted) {   // first authentication: the tag nonce came in the clear; uid ^ nonce goes into a fresh register
            M.st = skeys::resolve(tab, M.cur_key, M.key_a, M.key_b);
            M.ar = M.at = 0;
            const uint32_t nonce = B.word_at(h), nu = uid_len(M);
            if (nu <= 4u) {   // the UID bytes there are go in, none included (nothing at all with more UID bits than the nonce has: the reference raises)
                for (uint32_t i = 0; i < nu; i++) {
                    const uint32_t x = uid_byte(M, i) ^ ((nonce >> (8u * i)) & 0xFFu);
                    for (int k = 0; k < 8; k++) M.st = shift_in(M.st, (x >> k) & 1u);
                }
                M.ar = nonce_advance(nonce, 64);
                M.at = nonce_advance(M.ar, 32);
                M.encrypted = 1;
            }
        }
        break;
    case C_RANDRB: out.flags |= (M.encrypted == 1 && B.word_at(h + 4u) == M.ar) ? NFC_FRAME_AR_OK : NFC_FRAME_AR_ERROR; break;
    case C_RANDTB: out.flags |= (M.encrypted == 1 && B.word_at(h) == M.at) ? NFC_FRAME_AT_OK : NFC_FRAME_AT_ERROR; break;
    default: break;
    }
}

// One frame: raw_flags / n its nfc_raw_frame's flags and n_bytes (the repair's messages, the parity and CRC verdicts of assemble_frame),
// bytes / par its data bytes and ninth bits as received.  Outside a session the bytes are taken as they are; inside one every byte is
// decrypted first (fsm.py:133-154) and the parity and the CRC are those of the plaintext.  data / enc: the frame's slot, n entries each,
// ALL written: the plaintext bytes and the enc entries first, 0 behind.  An enc entry is what was on the air: the byte in the low half,
// bit 8 set when the parity bit equals the data parity (the '!' of fsm._print_enc, fsm.py:113-131).
template <class Mach, class Table>
NFC_HD Rec process_frame(Mach &M, int type, uint32_t raw_flags, uint32_t n, const uint8_t *__restrict__ bytes, const uint8_t *__restrict__ par,
                         uint8_t *__restrict__ data, uint16_t *__restrict__ enc, const Table &tab) {
    Rec out = {NFC_CMD_UNKNOWN, type, 0u, 0u, 0u, 0u, 0u, 0u};
    if (raw_flags & NFC_RAW_CUT) {   // its bits are not there: the machine is not touched, the keystream of a session is out of step from here
        out.cmd = NFC_CMD_CUT;
        M.flags |= NFC_FSM_LOST;
        return out;
    }
    out.flags = raw_flags & (uint32_t)(NFC_FRAME_EXTRA_ERROR | NFC_FRAME_MANY_MORE_ERROR);
    Bytes B = {};
    uint32_t nb;
    bool crc_ok;
    if (!M.encrypted) {
        nb = (raw_flags & NFC_RAW_PARITY_OK) ? n : 0u;
        crc_ok = (raw_flags & NFC_RAW_CRC_A_OK) != 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t b = nb ? bytes[i] : 0u;
            data[i] = (uint8_t)b;
            enc[i] = 0;
            if (i < 20u) B.put(i, b);
        }
    } else {
        out.flags |= NFC_FRAME_ENCRYPTED;
        out.n_enc = n;
        // {nr}{ar}: the reader nonce (the first half) is fed back into the register while it is decrypted
        const bool nr_ar = M.cur_cmd == C_RANDTA && n == 8u;
        // nested authentication: a fresh register keyed for the new sector swallows the encrypted tag nonce, uid ^ nonce fed in
        const bool nested = !nr_ar && (M.cur_cmd == C_AUTHA || M.cur_cmd == C_AUTHB);
        uint32_t todo = n;   // bytes that are decrypted
        if (nested) {
            M.st = skeys::resolve(tab, M.cur_key, M.key_a, M.key_b);
            M.ar = M.at = 0;
            const uint32_t nu = uid_len(M);
            todo = (nu >= 1u && nu <= n) ? nu : 0u;   // (nothing at all with no UID or a frame shorter than the UID: the reference raises)
        }
        bool bad = false;
        uint32_t crc = 0x6363u, p1 = 0, p2 = 0, nonce = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t b = bytes[i], p = par[i] & 1u;
            enc[i] = (uint16_t)(b | (((frames::popc8(b) & 1u) == p) ? 0x100u : 0u));
            uint32_t pt = 0;
            if (i < todo) {
                const uint32_t ub = nested ? uid_byte(M, i) : 0u;
                const bool feed = nested || (nr_ar && i < 4u);
                for (int k = 0; k < 8; k++) {
                    const uint32_t f = filter(M.st), ct = (b >> k) & 1u;
                    pt |= (ct ^ f) << k;
                    M.st = shift_in(M.st, feed ? (ct ^ ((ub >> k) & 1u) ^ f) : 0u);
                }
                // the ninth bit reuses the keystream bit of the next data bit: the register does not move for it
                if ((frames::popc8(pt) & 1u) == (p ^ filter(M.st))) bad = true;
                if (i < 20u) B.put(i, pt);
                if (i < 4u) nonce |= pt << (8u * i);
                if (i >= 2u) crc = frames::crc_a_step(crc, p2);
                p2 = p1;
                p1 = pt;
            }
            data[i] = (uint8_t)pt;
        }
        nb = todo;
        if (nested && todo) {
            if (todo == 4u) {   // a nonce register of 32 bits: the answers are set even when the frame then fails its parity
                M.ar = nonce_advance(nonce, 64);
                M.at = nonce_advance(M.ar, 32);
                M.encrypted = 1;
            } else {
                M.encrypted = 2;   // (as many nonce bits as UID bits: answers of another length, which nothing equals)
            }
        }
        if (bad) nb = 0;
        crc_ok = nb >= 2u && p2 == (crc & 0xFFu) && p1 == (crc >> 8);
        if (nb == 0)
            for (uint32_t i = 0; i < n; i++) data[i] = 0;
    }
    finish(M, nb, type, out, B, crc_ok, tab);
    return out;
}

// ---- what an EMULATOR is about to send: fsm.process_outgoing (fsm.py:68-112) ----
// A frame is a list of bits, its ninth bits included, reached through accessors -- in(k) the k-th bit, out(k, v) the k-th bit to put on the
// air, every k < n written once, in order -- so that one text serves the host machine's bit list (protocol.h: fsm_process_outgoing) and
// the bytes-plus-ninth-bits form of a lane's emulator (emu.hip.h: FrameIn / FrameOut).
// cipher.py:20-35 on bits [from, to) of a frame: every bit is xored with the filter output; the ninth bit of a group -- counted from `from`
// -- reuses the keystream bit of the next data bit: the register does not move for it.  feed_in: the plaintext is fed back ({nr}).
template <class In, class Out>
NFC_HD void crypt_bits(uint64_t &st, size_t from, size_t to, const In &in, Out &out, bool feed_in) {
    for (size_t k = from; k < to; k++) {
        const uint32_t b = in(k) & 1u;
        out(k, filter(st) ^ b);
        if ((k - from) % 9 != 8) st = shift_in(st, feed_in ? b : 0u);
    }
}
// cipher.py:62-72 with a plain tag nonce of n bits (bit(j): its j-th): uid ^ nonce goes into the register M.st, which holds the key -- the
// UID bits THERE ARE.  -> what `encrypted` becomes: 1 with a nonce register of 32 bits, M.ar / M.at set; 2 with another bit count -- the
// reference's answers then have that many bits, so that no {ar} / {at} ever equals them; 0 where the reference raises -- more UID bits
// than nonce bits (IndexError), a nonce of no bits (ZeroDivisionError in lfsr.py) -- with the register left at the key.
template <class Mach, class Bit>
NFC_HD int set_tag_plain(Mach &M, size_t n, Bit bit) {
    const size_t ll = 8 * (size_t)uid_len(M);
    if (n < ll || n == 0) return 0;
    for (size_t i = 0; i < ll; i++) M.st = shift_in(M.st, ((uid_byte(M, (uint32_t)(i >> 3)) >> (i & 7)) ^ bit(i)) & 1u);
    if (n != 32) return 2;
    uint32_t nonce = 0;
    for (uint32_t i = 0; i < 32; i++) nonce |= (bit(i) & 1u) << i;
    M.ar = nonce_advance(nonce, 64);
    M.at = nonce_advance(M.ar, 32);
    return 1;
}
// The machine follows the frame as if it had been heard -- tag type from an ATQA, the command in flight -- and, while a MIFARE Classic
// session is up, encrypts it.  Returns 1 when the tag is an Ultralight, nothing written: the reference then runs the frame through
// process_bits "to update state" (fsm.py:71-72) -- the caller does.
// card: what a MIFARE Classic and its reader do where the reference's hook differs (emu.hip.h: NFC_EMU_CARD) -- an outgoing AUTH sets the
// key choice even where the table has no slot (key A / key B), and a NESTED tag nonce of four bytes under a four-byte UID leaves under
// the NEW key's keystream while uid ^ nt is fed in, its ninth bits included: the frame process_frame's nested route decrypts.
template <class Mach, class Table, class In, class Out>
NFC_HD int outgoing(Mach &M, size_t n, int cmd, const In &in, Out &out, const Table &tab, bool card) {
    if (M.tag_type == 0) return 1;
    if (M.tag_type == 1) {   // CLASSIC1K (fsm.py:73-99)
        M.cur_cmd = cmd;
        if ((cmd == C_AUTHA || cmd == C_AUTHB) && n >= 17) {
            // the sector's key from the table, as a heard AUTH chooses it; with no slot present the choice stays the caller's, as ever
            uint32_t block = 0;
            for (int k = 0; k < 8; k++) block |= (uint32_t)(in((size_t)(9 + k)) & 1u) << k;
            const int c = skeys::choose(tab, cmd == C_AUTHB, block);
            if (c >= 2 || card) M.cur_key = c;
        }
        if (M.encrypted && cmd != C_RANDTA) {
            // ({nr}{ar}: the reader's own nonce, the first half, feeds the register as it is encrypted)
            const size_t ll = cmd == C_RANDRB ? n / 2 : 0;
            crypt_bits(M.st, 0, ll, in, out, true);
            crypt_bits(M.st, ll, n, in, out, false);
        } else if (cmd == C_RANDTA && card && M.encrypted && n == 36 && uid_len(M) == 4u) {
            M.st = skeys::resolve(tab, M.cur_key, M.key_a, M.key_b);
            uint32_t nonce = 0;
            for (uint32_t i = 0; i < 4u; i++) {
                const uint32_t ub = uid_byte(M, i);
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t b = in((size_t)(9u * i + k)) & 1u;
                    out((size_t)(9u * i + k), b ^ filter(M.st));
                    M.st = shift_in(M.st, b ^ ((ub >> k) & 1u));
                    nonce |= b << (8u * i + k);
                }
                out((size_t)(9u * i + 8u), (in((size_t)(9u * i + 8u)) & 1u) ^ filter(M.st));
            }
            M.ar = nonce_advance(nonce, 64);
            M.at = nonce_advance(M.ar, 32);
            M.encrypted = 1;
        } else if (cmd == C_RANDTA) {
            // the tag's nonce: a fresh register keyed for the sector takes uid ^ nonce -- the UID bits there are, the nonce bits there are
            // (fsm.py:86-97) -- and becomes the session; under a session that is already up (nested authentication) the OLD register
            // encrypts what goes on the air.  Where the reference raises it has installed nothing: the session stays as it was.
            const uint64_t st = M.st;
            const uint32_t ar = M.ar, at = M.at;
            if (M.encrypted) {
                uint64_t old = st;
                crypt_bits(old, 0, n, in, out, false);
            } else {
                for (size_t i = 0; i < n; i++) out(i, in(i) & 1u);
            }
            M.st = skeys::resolve(tab, M.cur_key, M.key_a, M.key_b);
            M.ar = M.at = 0;
            // (the nonce's j-th bit: the frame's without its ninth bits)
            const int session = set_tag_plain(M, n - n / 9, [&](size_t j) { return (uint32_t)(in(j + j / 8) & 1u); });
            if (session) M.encrypted = session;
            else M.st = st, M.ar = ar, M.at = at;
        } else {
            for (size_t i = 0; i < n; i++) out(i, in(i) & 1u);
        }
        return 0;
    }
    for (size_t i = 0; i < n; i++) out(i, in(i) & 1u);
    switch (cmd) {   // no tag type yet: an ATQA sets it (fsm.py:101-108)
    case C_ATQAUL: M.tag_type = 0; break;
    case C_ATQA1K: M.tag_type = 1; break;
    case C_ATQA4K: M.tag_type = 2; break;
    case C_ATQADS: M.tag_type = 3; break;
    default: break;
    }
    return 0;
}

// ---- Machine <-> nfc_fsm_state ----
NFC_HD uint64_t key_of(const uint8_t k[6]) {
    uint64_t v = 0;
    for (int i = 0; i < 6; i++) v |= (uint64_t)k[i] << (8 * i);
    return v;
}
NFC_HD void machine_from_state(Machine &M, const nfc_fsm_state &s) {
    M.cur_cmd = s.cur_cmd, M.tag_type = s.tag_type, M.encrypted = s.encrypted, M.cur_key = s.cur_key;
    M.st = s.cipher & ST_MASK;
    M.key_a = key_of(s.key_a), M.key_b = key_of(s.key_b);
    M.ar = (uint32_t)s.ar[0] | (uint32_t)s.ar[1] << 8 | (uint32_t)s.ar[2] << 16 | (uint32_t)s.ar[3] << 24;
    M.at = (uint32_t)s.at[0] | (uint32_t)s.at[1] << 8 | (uint32_t)s.at[2] << 16 | (uint32_t)s.at[3] << 24;
    M.flags = s.flags;
    uid_clear(M);
    M.uid_len = s.uid_len < UID_CAP ? s.uid_len : UID_CAP;
    for (uint32_t i = 0; i < M.uid_len; i++) uid_put(M, i, s.uid[i]);
}
NFC_HD void machine_to_state(const Machine &M, nfc_fsm_state &s) {
    s.cur_cmd = M.cur_cmd, s.tag_type = M.tag_type, s.encrypted = M.encrypted, s.cur_key = M.cur_key;
    s.cipher = M.st;
    for (int i = 0; i < 4; i++) s.ar[i] = (uint8_t)(M.ar >> (8 * i)), s.at[i] = (uint8_t)(M.at >> (8 * i));
    for (int i = 0; i < 6; i++) s.key_a[i] = (uint8_t)(M.key_a >> (8 * i)), s.key_b[i] = (uint8_t)(M.key_b >> (8 * i));
    s.uid_len = M.uid_len;
    for (uint32_t i = 0; i < UID_CAP; i++) s.uid[i] = i < M.uid_len ? (uint8_t)uid_byte(M, i) : (uint8_t)0;
    s.flags = M.flags;
    s.reserved = 0;
}
// what is wrong with a caller's state, or null
inline const char *state_fault(const nfc_fsm_state &s) {
    if (s.cur_cmd < 0 || s.cur_cmd >= C_COUNT) return "cur_cmd out of range";
    if (s.tag_type < -1 || s.tag_type > 3) return "tag_type out of range";
    if (s.encrypted < 0 || s.encrypted > 2) return "encrypted must be 0, 1 or 2";
    if (s.cur_key < 0 || s.cur_key > skeys::CUR_KEY_MAX) return "cur_key must be 0, 1 or 2 + a slot below 80";
    if (s.cipher >> 48) return "cipher holds more than 48 bits";
    if (s.uid_len > UID_CAP) return "uid_len exceeds 32";
    if (s.flags & ~(uint32_t)(NFC_FSM_LOST | NFC_FSM_UID_OVERFLOW)) return "unknown flags";
    if (s.reserved != 0) return "reserved must be 0";
    return nullptr;
}

// the machine as words, the layout of the device's [word][stream] arrays (multi_commands.hip.h), of one machine's blob (nfc_multi.hip:
// the same with one stream) and of nothing else
enum { W_CUR_CMD, W_TAG_TYPE, W_ENCRYPTED, W_CUR_KEY, W_ST_LO, W_ST_HI, W_AR, W_AT, W_KA_LO, W_KA_HI, W_KB_LO, W_KB_HI, W_UID_LEN, W_FLAGS,
       W_UID0, W_WORDS = W_UID0 + 8 };
// stream k of K: (words, K, k); one machine alone: (words, 1, 0)
NFC_HD void load_machine(Machine &M, const uint32_t *__restrict__ s, size_t K, size_t k) {
    M.cur_cmd = (int32_t)s[W_CUR_CMD * K + k];
    M.tag_type = (int32_t)s[W_TAG_TYPE * K + k];
    M.encrypted = (int32_t)s[W_ENCRYPTED * K + k];
    M.cur_key = (int32_t)s[W_CUR_KEY * K + k];
    M.st = (uint64_t)s[W_ST_LO * K + k] | (uint64_t)s[W_ST_HI * K + k] << 32;
    M.ar = s[W_AR * K + k];
    M.at = s[W_AT * K + k];
    M.key_a = (uint64_t)s[W_KA_LO * K + k] | (uint64_t)s[W_KA_HI * K + k] << 32;
    M.key_b = (uint64_t)s[W_KB_LO * K + k] | (uint64_t)s[W_KB_HI * K + k] << 32;
    M.uid_len = s[W_UID_LEN * K + k];
    M.flags = s[W_FLAGS * K + k];
    M.u0 = s[(W_UID0 + 0) * K + k], M.u1 = s[(W_UID0 + 1) * K + k], M.u2 = s[(W_UID0 + 2) * K + k], M.u3 = s[(W_UID0 + 3) * K + k];
    M.u4 = s[(W_UID0 + 4) * K + k], M.u5 = s[(W_UID0 + 5) * K + k], M.u6 = s[(W_UID0 + 6) * K + k], M.u7 = s[(W_UID0 + 7) * K + k];
    // (a machine is only ever written by store_machine, launch_init and a checked nfc_fsm_state; still, nothing may index by these)
    if ((uint32_t)M.cur_cmd >= (uint32_t)C_COUNT) M.cur_cmd = C_REQA;
    if ((uint32_t)M.cur_key > (uint32_t)skeys::CUR_KEY_MAX) M.cur_key = 0;
    if (M.uid_len > UID_CAP) M.uid_len = UID_CAP;
    M.st &= ST_MASK;
}
NFC_HD void store_machine(const Machine &M, uint32_t *__restrict__ s, size_t K, size_t k) {
    s[W_CUR_CMD * K + k] = (uint32_t)M.cur_cmd;
    s[W_TAG_TYPE * K + k] = (uint32_t)M.tag_type;
    s[W_ENCRYPTED * K + k] = (uint32_t)M.encrypted;
    s[W_CUR_KEY * K + k] = (uint32_t)M.cur_key;
    s[W_ST_LO * K + k] = (uint32_t)M.st;
    s[W_ST_HI * K + k] = (uint32_t)(M.st >> 32);
    s[W_AR * K + k] = M.ar;
    s[W_AT * K + k] = M.at;
    s[W_KA_LO * K + k] = (uint32_t)M.key_a;
    s[W_KA_HI * K + k] = (uint32_t)(M.key_a >> 32);
    s[W_KB_LO * K + k] = (uint32_t)M.key_b;
    s[W_KB_HI * K + k] = (uint32_t)(M.key_b >> 32);
    s[W_UID_LEN * K + k] = M.uid_len;
    s[W_FLAGS * K + k] = M.flags;
    s[(W_UID0 + 0) * K + k] = M.u0, s[(W_UID0 + 1) * K + k] = M.u1, s[(W_UID0 + 2) * K + k] = M.u2, s[(W_UID0 + 3) * K + k] = M.u3;
    s[(W_UID0 + 4) * K + k] = M.u4, s[(W_UID0 + 5) * K + k] = M.u5, s[(W_UID0 + 6) * K + k] = M.u6, s[(W_UID0 + 7) * K + k] = M.u7;
}

}  // namespace fsmd
}  // namespace nfc
