// emu.hip.h -- the two EMULATOR machines (tag.py, reader.py of the reference) and the closed loop that lets one read the other
// (usrp_nfc.py:116-136), one text for host and device, written the way fsm.hip.h is: scalar state, NFC_HD, no container a lane would
// index dynamically.  A tag answers what it hears from its memory, its nonces and its access bits (tag.py:114-175 Ultralight,
// tag.py:322-400 Classic 1K, tag.py:194-229 the access bits, tag.py:309-319 _set_at); a reader walks a card: anticollision, then an
// Ultralight's pages or every sector of a Classic from the last down, an authentication per sector (reader.py:59-149).  Both hand
// over (command, structure); what goes on the air is the business of the sender's protocol machine (fsm.hip.h: outgoing).
//
// What is emulated is a CARD: role, tag type, mode, memory, nonces, keys.  Its accessor -- mem_word(i), rand(i), n_rands -- has a host
// and a device form (HostCard: the caller's bytes; DevCard: the kernel's arrays, nfc_emu.hip says how they lie).
//
// The two MODES travel in the card.  NFC_EMU_REFERENCE is the reference with its quirks, each at its line below; NFC_EMU_CARD is what
// a MIFARE Classic does where the reference differs: the keys of the authenticated block's OWN sector, AUTHB with key B, a nested tag
// nonce under the NEW key (fsm.hip.h: outgoing), a reader that keys its machine from its table.
//
// Where the reference raises (a frame it does not know, a parity error: AttributeError on None; RANDRB before any AUTH: TypeError; more
// UID bits than nonce bits: IndexError; access bits behind the memory's end: IndexError) the machine gives no answer and sets the
// sticky NFC_EMU_RAISED.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"
#include "frames.hip.h"
#include "fsm.hip.h"
#include "sector_keys.h"

namespace nfc {
namespace emu {

using namespace fsmd;

constexpr uint32_t MAX_RANDS = 64, UL_BYTES = 64, CLASSIC_BYTES = 1024;
enum { AUTH_NONE = 0, AUTH_A = 1, AUTH_B = 2 };   // tag.py:27-30

// ---- the state, both roles in one record (nfc_emu_state) ----
struct State {
    int32_t halted, selected, auth, auth_key, auth_prosp, at_set;   // tag (auth / auth_prosp: a block, or -1 for None)
    uint32_t at, rand_idx;                                          // at: byte 0 lowest; rand_idx: both roles
    int32_t tag_type, cur_addr, auth_addr;                          // reader (tag_type: -1 for None)
    uint32_t uid_len, flags;
    uint32_t u0, u1, u2, u3, u4, u5, u6, u7;                        // reader: the UID it collected, 32 bytes
};
NFC_HD void tag_reset(State &S) {   // tag.py:177-181
    S.auth = -1;
    S.auth_key = AUTH_NONE;
    S.auth_prosp = -1;
    S.at_set = 0;
    S.at = 0;
}
NFC_HD void reader_reset_tag(State &S) {   // reader.py:32-39
    S.uid_len = 0;
    S.u0 = S.u1 = S.u2 = S.u3 = S.u4 = S.u5 = S.u6 = S.u7 = 0;
    S.tag_type = -1;
    S.cur_addr = S.auth_addr = 0;
    S.rand_idx = 0;
}
NFC_HD void state_init(State &S) {
    S.halted = S.selected = 0;
    tag_reset(S);
    reader_reset_tag(S);
    S.flags = 0;
}
NFC_HD uint32_t uid_get(const State &S, uint32_t i) {
    const uint32_t j = i >> 2;
    const uint32_t w = j == 0 ? S.u0 : j == 1 ? S.u1 : j == 2 ? S.u2 : j == 3 ? S.u3 : j == 4 ? S.u4 : j == 5 ? S.u5 : j == 6 ? S.u6 : S.u7;
    return (w >> (8u * (i & 3u))) & 0xFFu;
}
// `self._uid.extend(...)`: n bytes of B from `from`; not made past 32 bytes (NFC_EMU_UID_OVERFLOW, as NFC_FSM_UID_OVERFLOW)
NFC_HD void uid_extend(State &S, const Bytes &B, uint32_t from, uint32_t n) {
    if (S.uid_len + n > UID_CAP) {
        S.flags |= NFC_EMU_UID_OVERFLOW;
        return;
    }
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t i = S.uid_len + t, j = i >> 2, v = B.at(from + t) << (8u * (i & 3u));
        S.u0 |= j == 0 ? v : 0u, S.u1 |= j == 1 ? v : 0u, S.u2 |= j == 2 ? v : 0u, S.u3 |= j == 3 ? v : 0u;
        S.u4 |= j == 4 ? v : 0u, S.u5 |= j == 5 ? v : 0u, S.u6 |= j == 6 ? v : 0u, S.u7 |= j == 7 ? v : 0u;
    }
    S.uid_len += n;
}

NFC_HD void state_from_public(State &S, const nfc_emu_state &p) {
    S.halted = p.halted, S.selected = p.selected, S.auth = p.auth, S.auth_key = p.auth_key, S.auth_prosp = p.auth_prosp, S.at_set = p.at_set;
    S.at = (uint32_t)p.at[0] | (uint32_t)p.at[1] << 8 | (uint32_t)p.at[2] << 16 | (uint32_t)p.at[3] << 24;
    S.rand_idx = p.rand_idx;
    S.tag_type = p.tag_type, S.cur_addr = p.cur_addr, S.auth_addr = p.auth_addr;
    S.flags = p.flags;
    S.uid_len = p.uid_len < UID_CAP ? p.uid_len : UID_CAP;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < S.uid_len; i++) w[i >> 2] |= (uint32_t)p.uid[i] << (8u * (i & 3u));
    S.u0 = w[0], S.u1 = w[1], S.u2 = w[2], S.u3 = w[3], S.u4 = w[4], S.u5 = w[5], S.u6 = w[6], S.u7 = w[7];
}
NFC_HD void state_to_public(const State &S, nfc_emu_state &p) {
    p.halted = S.halted, p.selected = S.selected, p.auth = S.auth, p.auth_key = S.auth_key, p.auth_prosp = S.auth_prosp, p.at_set = S.at_set;
    for (int i = 0; i < 4; i++) p.at[i] = (uint8_t)(S.at >> (8 * i));
    p.rand_idx = S.rand_idx;
    p.tag_type = S.tag_type, p.cur_addr = S.cur_addr, p.auth_addr = S.auth_addr;
    p.uid_len = S.uid_len;
    for (uint32_t i = 0; i < UID_CAP; i++) p.uid[i] = i < S.uid_len ? (uint8_t)uid_get(S, i) : (uint8_t)0;
    p.flags = S.flags;
    p.reserved = 0;
}
inline const char *state_fault(const nfc_emu_state &s) {
    if ((uint32_t)s.halted > 1u || (uint32_t)s.selected > 1u || (uint32_t)s.at_set > 1u) return "halted, selected and at_set must be 0 or 1";
    if (s.auth < -1 || s.auth > 255 || s.auth_prosp < -1 || s.auth_prosp > 255) return "auth and auth_prosp must be -1 or a block";
    if (s.auth_key < AUTH_NONE || s.auth_key > AUTH_B) return "auth_key must be 0, 1 or 2";
    if (s.rand_idx >= MAX_RANDS) return "rand_idx exceeds 63";
    if (s.tag_type < -1 || s.tag_type > 3) return "tag_type out of range";
    if (s.cur_addr < -0x10000 || s.cur_addr > 0x10000 || s.auth_addr < -0x10000 || s.auth_addr > 0x10000) return "cur_addr or auth_addr out of range";
    if (s.uid_len > UID_CAP) return "uid_len exceeds 32";
    if (s.flags & ~(uint32_t)NFC_EMU_FLAGS_ALL) return "unknown flags";
    if (s.reserved != 0) return "reserved must be 0";
    return nullptr;
}

// ---- a card's accessors ----
struct HostCard {
    const uint8_t *mem, *rands;   // rands: four bytes each
    uint32_t n_rands;
    int32_t tag_type, mode;
    NFC_HD uint32_t mem_word(uint32_t i) const {
        const uint8_t *p = mem + 4u * i;
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    NFC_HD uint32_t rand(uint32_t i) const {
        const uint8_t *p = rands + 4u * i;
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
};
// the device's arrays: memory in units of 16 bytes, [unit][K] -- lanes of a wave that read one block, as whole-card reads in step do,
// load neighbouring 16-byte words -- and nonces as words [index][K]
struct DevCard {
    const uint32_t *mem, *rands;
    uint32_t K, k, n_rands;
    int32_t tag_type, mode;
    NFC_HD uint32_t mem_word(uint32_t i) const { return mem[((size_t)((i >> 2) & 63u) * K + k) * 4u + (i & 3u)]; }   // (64 units per card, whatever its type)
    NFC_HD uint32_t rand(uint32_t i) const { return rands[(size_t)(i & (MAX_RANDS - 1u)) * K + k]; }
};
// a reader on the device: nonces and a mode, and NO memory -- a reader step that reached for a card's memory would not compile
struct DevReader {
    const uint32_t *rands;
    uint32_t K, k, n_rands;
    int32_t mode;
    NFC_HD uint32_t rand(uint32_t i) const { return rands[(size_t)(i & (MAX_RANDS - 1u)) * K + k]; }
};
template <class Card>
NFC_HD uint32_t mem_byte(const Card &C, uint32_t i) {
    return (C.mem_word(i >> 2) >> (8u * (i & 3u))) & 0xFFu;
}
template <class Card>
NFC_HD uint32_t next_rand(State &S, const Card &C) {   // rand.py:23-27
    const uint32_t n = C.n_rands ? C.n_rands : 1u, i = S.rand_idx < n ? S.rand_idx : 0u;
    S.rand_idx = (i + 1u) % n;
    return C.n_rands ? C.rand(i) : 0u;
}
// A Classic tag's trailers as a sector key table (sector_keys.h: the accessor) -- what a tag's own protocol machine decrypts with in
// CARD mode: slot (type, sector) is key A / key B of that sector's trailer.  Empty in REFERENCE mode and for an Ultralight.
template <class Card>
struct TrailerTable {
    const Card &C;
    NFC_HD bool has(uint32_t slot) const { return C.mode == NFC_EMU_CARD && C.tag_type == 1 && slot < skeys::SLOTS && slot % skeys::SECTORS < 16u; }
    NFC_HD bool get(uint32_t slot, uint64_t &key) const {
        if (!has(slot)) return false;
        const uint32_t w = ((slot % skeys::SECTORS) * 4u + 3u) * 4u;   // the trailer's first word
        key = slot < skeys::SECTORS ? (uint64_t)C.mem_word(w) | (uint64_t)(C.mem_word(w + 1u) & 0xFFFFu) << 32
                                    : (uint64_t)(C.mem_word(w + 2u) >> 16) | (uint64_t)C.mem_word(w + 3u) << 16;
        return true;
    }
};
// tag.py:52-57: both keys from the trailer of sector 0
template <class Card>
NFC_HD void keys_from_mem(const Card &C, uint64_t &key_a, uint64_t &key_b) {
    key_a = (uint64_t)C.mem_word(12) | (uint64_t)(C.mem_word(13) & 0xFFFFu) << 32;
    key_b = (uint64_t)(C.mem_word(14) >> 16) | (uint64_t)C.mem_word(15) << 16;
}

// ---- an answer: the command and its whole frame (CommandStructure.encode_command, command.py:256-265) ----
struct Ans {
    int32_t cmd;   // -1: no answer
    uint32_t n;    // bytes of the frame: header | extra | CRC_A
    Bytes B;
};
NFC_HD Ans no_answer() {
    Ans a = {-1, 0u, {}};
    return a;
}
// header in place; the caller puts the extra bytes with add()/add_word() and ends with finish_answer()
NFC_HD Ans begin_answer(int cmd) {
    Ans a = {cmd, 0u, {}};
    const Def c = def_of(cmd);
    if (c.n_header() >= 1) a.B.put(a.n++, c.h0());
    if (c.n_header() >= 2) a.B.put(a.n++, c.h1);
    return a;
}
NFC_HD void add(Ans &a, uint32_t byte) { a.B.put(a.n++, byte & 0xFFu); }
NFC_HD void add_word(Ans &a, uint32_t w) {
    for (int i = 0; i < 4; i++) add(a, w >> (8 * i));
}
NFC_HD void finish_answer(Ans &a) {
    if (!def_of(a.cmd).crc()) return;
    uint32_t crc = 0x6363u;
    const uint32_t n = a.n;
    for (uint32_t i = 0; i < n; i++) crc = frames::crc_a_step(crc, a.B.at(i));
    add(a, crc & 0xFFu);
    add(a, crc >> 8);
}
NFC_HD Ans plain_answer(int cmd) {
    Ans a = begin_answer(cmd);
    finish_answer(a);
    return a;
}

// ---- the tag ----
// tag.py:199-222: the three access bits of data block / trailer `rem` from the four bytes at `off`
template <class Card>
NFC_HD uint32_t access_bits_at(State &S, const Card &C, uint32_t off, uint32_t rem) {
    const uint32_t b0 = mem_byte(C, off), b1 = mem_byte(C, off + 1u), b2 = mem_byte(C, off + 2u);
    const uint32_t not_ones = b0, not_twos = b0 >> 4, not_threes = b1, ones = b1 >> 4, twos = b2, threes = b2 >> 4;
    if (((ones ^ not_ones) & 0xFu) != 0xFu) S.flags |= NFC_EMU_ERR_ONES;         // tag.py:207-212, the three prints
    if (((twos ^ not_twos) & 0xFu) != 0xFu) S.flags |= NFC_EMU_ERR_TWOS;
    if (((threes ^ not_threes) & 0xFu) != 0xFu) S.flags |= NFC_EMU_ERR_THREES;
    return ((ones >> rem) & 1u) << 2 | ((twos >> rem) & 1u) << 1 | ((threes >> rem) & 1u);
}
// tag.py:224-276 for AccessType.READ, the only type ever asked for (the other branches are not restated; tag.py:277 would raise).
// -> a mask of three bits: byte groups [0, 6), [6, 10), [10, 16) that are shown (ALL 7, NONE 0, P011 3, P010 2); `raised`: the reference
// raises (the access bytes lie behind the memory's end).
template <class Card>
NFC_HD uint32_t read_access(State &S, const Card &C, uint32_t block, bool &raised) {
    raised = false;
    if (S.auth < 0) return 0u;
    const uint32_t sector = (uint32_t)S.auth;   // tag.py:225: `sector` is the AUTH's BLOCK number
    uint32_t off;
    if (C.mode == NFC_EMU_CARD) {
        if (skeys::sector_of(block) != skeys::sector_of(sector) || skeys::sector_of(sector) >= 16u) return 0u;
        off = (skeys::sector_of(sector) * 4u + 3u) * 16u + 6u;
    } else {
        if (block / 4u != sector / 4u) return 0u;   // tag.py:228: Python 2 integer division
        off = sector * 16u + 54u;                   // tag.py:194-197: the trailer's access bytes only when the AUTH named the sector's first block
        if (off + 2u >= CLASSIC_BYTES) {            // (the slice is short: IndexError)
            raised = true;
            return 0u;
        }
    }
    const uint32_t rem = block % 4u, bits = access_bits_at(S, C, off, rem);
    if (rem != 3u) {   // tag.py:233-243
        if (bits == 7u) return 0u;
        if (bits == 3u || bits == 5u) return S.auth_key == AUTH_B ? 7u : 0u;
        return 7u;
    }
    if (bits <= 2u) return S.auth_key == AUTH_A ? 3u : 0u;   // tag.py:269-276: P011, key A hidden
    return 2u;                                               // P010: the access bytes alone
}

// One heard command: cmd its index (< 0: a frame the machine does not know or a parity error), B the plain frame, h / ne its header and
// extra lengths.  tag.py:114-175 (Ultralight), tag.py:322-400 (Classic 1K).
template <class Card>
NFC_HD Ans tag_step(State &S, const Card &C, int cmd, const Bytes &B, uint32_t h, uint32_t ne) {
    if (cmd < 0 || cmd >= C_COUNT) {
        S.flags |= NFC_EMU_RAISED;
        return no_answer();
    }
    if (def_of(cmd).type() != 1) return no_answer();   // tag.py:115,323
    const bool ul = C.tag_type == 0;
    const int atqa = ul ? C_ATQAUL : C_ATQA1K;
    switch (cmd) {
    case C_WUPA:
    case C_REQA: {
        const bool answer = cmd == C_WUPA || !S.halted;
        if (!ul) {   // tag.py:337-338,343-344
            S.selected = 0;
            tag_reset(S);
        }
        return answer ? plain_answer(atqa) : no_answer();
    }
    case C_ANTI1R: {
        Ans a = begin_answer(ul ? C_ANTI1U : C_ANTI1G);   // tag.py:135 uid[0:4] behind the 0x88 header; tag.py:347 the five UID bytes
        add_word(a, C.mem_word(0));
        if (!ul) add(a, mem_byte(C, 4));
        finish_answer(a);
        return a;
    }
    case C_SEL1R: {
        bool same = ne == 5u;   // tag.py:138: [0x88] + uid[0:4]; tag.py:350: uid
        if (ul) {
            same = same && B.at(h) == 0x88u;
            for (uint32_t j = 0; j < 4u; j++) same = same && B.at(h + 1u + j) == mem_byte(C, j);
        } else {
            for (uint32_t j = 0; j < 5u; j++) same = same && B.at(h + j) == mem_byte(C, j);
        }
        if (!same) return no_answer();
        S.selected = 1;
        return plain_answer(ul ? C_SEL1U : C_SEL1K);
    }
    default: break;
    }
    if (!S.selected) return no_answer();
    if (ul) {
        switch (cmd) {
        case C_ANTI2R: {
            Ans a = begin_answer(C_ANTI2T);   // tag.py:151: uid[4:]
            for (uint32_t j = 4; j < 9u; j++) add(a, mem_byte(C, j));
            finish_answer(a);
            return a;
        }
        case C_SEL2R: {
            bool same = ne == 5u;
            for (uint32_t j = 0; j < 5u; j++) same = same && B.at(h + j) == mem_byte(C, 4u + j);
            if (same) return plain_answer(C_SEL2T);
            S.selected = 0;
            tag_reset(S);
            return no_answer();
        }
        case C_READR: {
            const uint32_t val = B.at(h);
            if (val > 0x0Fu) return no_answer();
            Ans a = begin_answer(C_READT);   // tag.py:160-168: four pages from `val`, round the end of the 64 bytes
            for (uint32_t j = 0; j < 4u; j++) add_word(a, C.mem_word((val + j) & 15u));
            finish_answer(a);
            return a;
        }
        case C_HALT:
            S.halted = 1;
            S.selected = 0;
            tag_reset(S);
            return no_answer();
        default: return no_answer();
        }
    }
    switch (cmd) {
    case C_AUTHA:
    case C_AUTHB: {   // tag.py:309-319,361-366.  REFERENCE: AUTHB is served with key A and recorded as AuthKey.A
        tag_reset(S);
        S.auth_key = (cmd == C_AUTHB && C.mode == NFC_EMU_CARD) ? AUTH_B : AUTH_A;
        S.auth_prosp = (int32_t)B.at(h);
        const uint32_t nonce = next_rand(S, C);
        S.at = nonce_advance(nonce, 96);   // cipher.py:36-41: the answer follows from the nonce alone, whichever key loads the register
        S.at_set = 1;
        Ans a = begin_answer(C_RANDTA);
        add_word(a, nonce);
        finish_answer(a);
        return a;
    }
    case C_RANDRB: {   // tag.py:367-370: the reader's answer is not checked
        S.auth = S.auth_prosp;
        if (!S.at_set) {   // (encode_command(RANDTB, None): TypeError)
            S.flags |= NFC_EMU_RAISED;
            return no_answer();
        }
        Ans a = begin_answer(C_RANDTB);
        add_word(a, S.at);
        finish_answer(a);
        return a;
    }
    case C_SEL2R:
        S.selected = 0;
        tag_reset(S);
        return no_answer();
    case C_READR: {
        const uint32_t val = B.at(h);
        if (val > 0x3Fu) return no_answer();
        bool raised;
        const uint32_t show = read_access(S, C, val, raised);
        if (raised) S.flags |= NFC_EMU_RAISED;
        if (!show) return no_answer();
        Ans a = begin_answer(C_READT);   // tag.py:379-394: the block, byte groups that may not be read as zeros
        const uint32_t w0 = C.mem_word(val * 4u), w1 = C.mem_word(val * 4u + 1u), w2 = C.mem_word(val * 4u + 2u), w3 = C.mem_word(val * 4u + 3u);
        const uint32_t m0 = (show & 4u) ? 0xFFFFFFFFu : 0u, m1 = (show & 2u) ? 0xFFFFFFFFu : 0u, m2 = (show & 1u) ? 0xFFFFFFFFu : 0u;
        add_word(a, w0 & m0);
        add_word(a, (w1 & 0xFFFFu & m0) | (w1 & 0xFFFF0000u & m1));
        add_word(a, (w2 & 0xFFFFu & m1) | (w2 & 0xFFFF0000u & m2));
        add_word(a, w3 & m2);
        finish_answer(a);
        return a;
    }
    case C_HALT:   // tag.py:395-397 (a Classic stays selected)
        S.halted = 1;
        tag_reset(S);
        return no_answer();
    default: return no_answer();
    }
}

// ---- the reader ----
// reader.py:59-149.  REFERENCE and CARD differ only in how the reader's protocol machine is keyed (outgoing): the answer {nr}{ar}
// follows from the nonces alone (cipher.py:36-41), so `keya` (reader.py:25) never shows in a plain frame.
template <class Card>
NFC_HD Ans reader_step(State &S, const Card &C, int cmd, const Bytes &B, uint32_t h, uint32_t ne) {
    (void)ne;
    if (cmd < 0 || cmd >= C_COUNT) {
        S.flags |= NFC_EMU_RAISED;
        return no_answer();
    }
    if (def_of(cmd).type() != 0) return no_answer();   // reader.py:60
    Ans a = no_answer();
    int next = C_HALT;
    switch (cmd) {
    case C_ATQAUL: S.tag_type = 0, next = C_ANTI1R; break;
    case C_ATQA1K: S.tag_type = 1, next = C_ANTI1R; break;
    case C_ATQA4K: S.tag_type = 2; break;   // reader.py:75-78: HALT
    case C_ATQADS: S.tag_type = 3; break;
    case C_ANTI1U:   // reader.py:82-86
        a = begin_answer(C_SEL1R);
        add(a, 0x88u);
        add_word(a, B.word_at(h));
        uid_extend(S, B, h, 3);
        break;
    case C_ANTI1G:   // reader.py:87-91
        a = begin_answer(C_SEL1R);
        add_word(a, B.word_at(h));
        add(a, B.at(h + 4u));
        uid_extend(S, B, h, 4);
        break;
    case C_SEL1U: next = C_ANTI2R; break;
    case C_SEL1K:   // reader.py:94-98: the last sector first
        S.auth_addr = 0x3C;
        S.cur_addr = 0x3F;
        a = begin_answer(C_AUTHA);
        add(a, (uint32_t)S.auth_addr);
        break;
    case C_ANTI2T:   // reader.py:99-103
        a = begin_answer(C_SEL2R);
        add_word(a, B.word_at(h));
        add(a, B.at(h + 4u));
        uid_extend(S, B, h, 4);
        break;
    case C_RANDTA: {   // reader.py:104-112
        const uint32_t nr = next_rand(S, C);
        if (S.uid_len > 4u) {   // (more UID bits than nonce bits: IndexError in set_tag_bits, cipher.py:67)
            S.flags |= NFC_EMU_RAISED;
            return no_answer();
        }
        a = begin_answer(C_RANDRB);
        add_word(a, nr);
        add_word(a, nonce_advance(B.word_at(h), 64));
        break;
    }
    case C_RANDTB:
        a = begin_answer(C_READR);
        add(a, (uint32_t)S.cur_addr);
        break;
    case C_SEL2T:
        S.cur_addr = 0;
        a = begin_answer(C_READR);
        add(a, 0u);
        break;
    case C_READT: {   // reader.py:120-143
        int32_t addr = S.cur_addr;
        if (S.tag_type == 0) {
            if (addr <= 0x08) {
                addr += 0x04;
                a = begin_answer(C_READR);
                add(a, (uint32_t)addr);
            }
        } else if (S.tag_type == 1) {
            if (addr % 4 == 0) {
                if (addr != 0) {   // (reader.py:132 at address 0 is a comparison, not an assignment: HALT is the default anyway)
                    addr -= 1;
                    S.auth_addr -= 0x04;
                    a = begin_answer(C_AUTHA);
                    add(a, (uint32_t)S.auth_addr);
                }
            } else {
                addr -= 1;
                a = begin_answer(C_READR);
                add(a, (uint32_t)addr);
            }
        }
        S.cur_addr = addr;
        break;
    }
    default: S.flags |= NFC_EMU_UNEXPECTED; break;   // "ERROR, Unexpected command!!" (reader.py:146): HALT
    }
    if (a.cmd < 0) a = begin_answer(next);
    finish_answer(a);
    if (a.cmd == C_HALT) reader_reset_tag(S);   // reader.py:45-46
    return a;
}

// ---- a frame on its way: plain bytes with odd parity <-> the bit list the encoders take (bit 9 i + j: bit j of byte i, j == 8 its ninth) ----
struct FrameIn {
    const Bytes &B;
    uint32_t par;   // bit i: the ninth bit of byte i
    NFC_HD uint32_t operator()(size_t k) const {
        const uint32_t i = (uint32_t)(k / 9u), j = (uint32_t)(k % 9u);
        return j == 8u ? (par >> i) & 1u : (B.at(i) >> j) & 1u;
    }
};
// written in order, every bit once: a byte is put when its eighth bit arrives
struct FrameOut {
    Bytes B;
    uint32_t par, cur;
    NFC_HD void operator()(size_t k, uint32_t v) {
        const uint32_t i = (uint32_t)(k / 9u), j = (uint32_t)(k % 9u);
        if (j == 8u) {
            par |= (v & 1u) << i;
            return;
        }
        cur |= (v & 1u) << j;
        if (j == 7u) {
            B.put(i, cur);
            cur = 0;
        }
    }
};
NFC_HD uint32_t odd_parity_of(const Bytes &B, uint32_t n) {
    uint32_t par = 0;
    for (uint32_t i = 0; i < n; i++) par |= ((frames::popc8(B.at(i)) & 1u) ^ 1u) << i;
    return par;
}
// what assemble_frame (frames.hip.h) says of n bytes and their ninth bits
NFC_HD uint32_t raw_flags_of(uint32_t n, const uint8_t *bytes, const uint8_t *par) {
    bool par_ok = n > 0;
    uint32_t crc = 0x6363u, p1 = 0, p2 = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t b = bytes[i];
        if ((frames::popc8(b) & 1u) == (par[i] & 1u)) par_ok = false;
        if (i >= 2u) crc = frames::crc_a_step(crc, p2);
        p2 = p1;
        p1 = b;
    }
    uint32_t flags = 0;
    if (par_ok) {
        flags |= NFC_RAW_PARITY_OK;
        if (n >= 2u && p2 == (crc & 0xFFu) && p1 == (crc >> 8)) flags |= NFC_RAW_CRC_A_OK;
    }
    return flags;
}

// What replay_step and run_pair ask of `scratch`: SCRATCH_BYTES of the caller's own (a lane's, a pair's), its base aligned to 2 bytes at
// least -- the enc slot at scratch + 64 holds uint16 entries; every caller here gives 16 (an alignas(16) array on the host, a 256-byte
// section in strides of 160 on the device).  [0, 20) a frame's air bytes, [20, 40) its ninth bits, [40, 60) the receiving machine's data
// slot, [64, 104) its enc slot.
constexpr uint32_t SCRATCH_BYTES = 160;
static_assert(SCRATCH_BYTES % 16 == 0 && 64 + 2 * 20 <= SCRATCH_BYTES, "a lane's scratch keeps the next lane's aligned");

// ---- the state as words: the layout of the device's [word][stream] arrays of a multi-stream context (multi_commands.hip.h) ----
enum { EW_HALTED, EW_SELECTED, EW_AUTH, EW_AUTH_KEY, EW_AUTH_PROSP, EW_AT_SET, EW_AT, EW_RAND_IDX, EW_TAG_TYPE, EW_CUR_ADDR, EW_AUTH_ADDR, EW_UID_LEN,
       EW_FLAGS, EW_UID0, EW_WORDS = EW_UID0 + 8 };
NFC_HD void load_state(State &S, const uint32_t *__restrict__ s, size_t K, size_t k) {
    S.halted = (int32_t)(s[EW_HALTED * K + k] & 1u), S.selected = (int32_t)(s[EW_SELECTED * K + k] & 1u);
    S.auth = (int32_t)s[EW_AUTH * K + k], S.auth_key = (int32_t)s[EW_AUTH_KEY * K + k], S.auth_prosp = (int32_t)s[EW_AUTH_PROSP * K + k];
    S.at_set = (int32_t)(s[EW_AT_SET * K + k] & 1u), S.at = s[EW_AT * K + k], S.rand_idx = s[EW_RAND_IDX * K + k];
    S.tag_type = (int32_t)s[EW_TAG_TYPE * K + k], S.cur_addr = (int32_t)s[EW_CUR_ADDR * K + k], S.auth_addr = (int32_t)s[EW_AUTH_ADDR * K + k];
    S.uid_len = s[EW_UID_LEN * K + k], S.flags = s[EW_FLAGS * K + k];
    S.u0 = s[(EW_UID0 + 0) * K + k], S.u1 = s[(EW_UID0 + 1) * K + k], S.u2 = s[(EW_UID0 + 2) * K + k], S.u3 = s[(EW_UID0 + 3) * K + k];
    S.u4 = s[(EW_UID0 + 4) * K + k], S.u5 = s[(EW_UID0 + 5) * K + k], S.u6 = s[(EW_UID0 + 6) * K + k], S.u7 = s[(EW_UID0 + 7) * K + k];
    if (S.uid_len > UID_CAP) S.uid_len = UID_CAP;   // (only ever written by store_state and a checked nfc_emu_state; still, nothing may index by these)
    if (S.rand_idx >= MAX_RANDS) S.rand_idx = 0;
}
NFC_HD void store_state(const State &S, uint32_t *__restrict__ s, size_t K, size_t k) {
    s[EW_HALTED * K + k] = (uint32_t)S.halted, s[EW_SELECTED * K + k] = (uint32_t)S.selected;
    s[EW_AUTH * K + k] = (uint32_t)S.auth, s[EW_AUTH_KEY * K + k] = (uint32_t)S.auth_key, s[EW_AUTH_PROSP * K + k] = (uint32_t)S.auth_prosp;
    s[EW_AT_SET * K + k] = (uint32_t)S.at_set, s[EW_AT * K + k] = S.at, s[EW_RAND_IDX * K + k] = S.rand_idx;
    s[EW_TAG_TYPE * K + k] = (uint32_t)S.tag_type, s[EW_CUR_ADDR * K + k] = (uint32_t)S.cur_addr, s[EW_AUTH_ADDR * K + k] = (uint32_t)S.auth_addr;
    s[EW_UID_LEN * K + k] = S.uid_len, s[EW_FLAGS * K + k] = S.flags;
    s[(EW_UID0 + 0) * K + k] = S.u0, s[(EW_UID0 + 1) * K + k] = S.u1, s[(EW_UID0 + 2) * K + k] = S.u2, s[(EW_UID0 + 3) * K + k] = S.u3;
    s[(EW_UID0 + 4) * K + k] = S.u4, s[(EW_UID0 + 5) * K + k] = S.u5, s[(EW_UID0 + 6) * K + k] = S.u6, s[(EW_UID0 + 7) * K + k] = S.u7;
}

// what is wrong with a card in `role`, or null (a message that continues the argument's name)
inline const char *card_fault(const nfc_emu_card &c, int role) {
    if (c.role != role) return role == NFC_EMU_TAG ? ".role must be NFC_EMU_TAG" : ".role must be NFC_EMU_READER";
    if (c.mode != NFC_EMU_REFERENCE && c.mode != NFC_EMU_CARD) return ".mode must be NFC_EMU_REFERENCE or NFC_EMU_CARD";
    if (c.reserved != 0 || c.reserved2 != 0) return ".reserved must be 0";
    if (role == NFC_EMU_TAG) {
        if (c.tag_type != 0 && c.tag_type != 1) return ".tag_type must be 0 (Ultralight) or 1 (Classic 1K)";
        if (!c.mem || c.mem_len != (c.tag_type == 0 ? UL_BYTES : CLASSIC_BYTES)) return ".mem must be exactly 64 bytes (Ultralight) or 1024 bytes (Classic 1K)";
    } else if (c.table && skeys::table_fault(*c.table)) {
        return ".table: present must be 0 or 1";
    }
    const bool needs = role == NFC_EMU_READER || c.tag_type == 1;
    if (c.n_rands > MAX_RANDS || (needs && c.n_rands == 0) || (c.n_rands && !c.rands)) return ".rands: a Classic tag and every reader need 1 .. 64 nonces";
    return nullptr;
}

// ---- replay: a machine that hears one side answers as the other (tag_emulate / reader_emulate, usrp_nfc.py:35-100) ----
// One heard command -- `r` what the stream's protocol machine M made of the frame, `data` its plain bytes -- through the emulator of
// `card`'s role, and the answer through M's own outgoing, so that M has advanced before the next heard frame is decrypted.  -> the
// answer's command or -1; its plain frame in `a`, what goes on the air in air_bytes / air_par (18 entries each, all written).
// scratch: SCRATCH_BYTES, for an Ultralight's "update state" pass.
template <class Card, class Mach, class Table>
NFC_HD int replay_step(State &S, const Card &C, int role, Mach &M, const Table &tab, const Rec &r, const uint8_t *data, Ans &a, uint8_t *air_bytes,
                       uint8_t *air_par, uint8_t *scratch) {
    for (uint32_t i = 0; i < (uint32_t)MAX_COMMAND_BYTES; i++) air_bytes[i] = 0, air_par[i] = 0;
    a = no_answer();
    if (r.cmd == NFC_CMD_CUT || r.type != (role == NFC_EMU_TAG ? 1 : 0)) return -1;   // (its own side, if the stream decodes both: not heard)
    Bytes B = {};
    for (uint32_t i = 0; i < r.n_bytes && i < 20u; i++) B.put(i, data[i]);
    a = role == NFC_EMU_TAG ? tag_step(S, C, r.cmd, B, r.n_header, r.n_extra) : reader_step(S, C, r.cmd, B, r.n_header, r.n_extra);
    if (a.cmd < 0) return -1;
    const int type = def_of(a.cmd).type();
    const uint32_t n = a.n, par = odd_parity_of(a.B, n);
    FrameOut air = {{}, 0u, 0u};
    const FrameIn in = {a.B, par};
    bool as_plain = false;
    if (outgoing(M, (size_t)9u * n, a.cmd, in, air, tab, C.mode == NFC_EMU_CARD)) {
        uint8_t *ab = scratch, *ap = scratch + 20, *d = scratch + 40;
        uint16_t *enc = (uint16_t *)(scratch + 64);
        for (uint32_t i = 0; i < n; i++) ab[i] = (uint8_t)a.B.at(i), ap[i] = (uint8_t)((par >> i) & 1u);
        (void)process_frame(M, type, raw_flags_of(n, ab, ap), n, ab, ap, d, enc, tab);
        as_plain = true;
    }
    for (uint32_t i = 0; i < n; i++) {
        air_bytes[i] = (uint8_t)(as_plain ? a.B.at(i) : air.B.at(i));
        air_par[i] = (uint8_t)(((as_plain ? par : air.par) >> i) & 1u);
    }
    return a.cmd;
}

// ---- the closed loop (usrp_nfc.py:116-136): one tag, one reader, `rounds` restarts ----
constexpr uint32_t ROUND_STEPS = 1024;   // frames of one round before the pair is stopped (a whole Classic card is 199)
struct Slab {                            // one pair's part of the outputs
    nfc_emu_frame *frames;
    uint8_t *plain, *air, *par;
    uint32_t cap_frames, cap_bytes;
};
// the reader's sector key table and the tag's trailers behind ONE accessor: the machine that is at work says which
template <class TagTab, class ReaderTab>
struct SideTable {
    const TagTab &t;
    const ReaderTab &r;
    bool tag, reader_on;   // reader_on: the reader's table counts (CARD mode)
    NFC_HD bool has(uint32_t slot) const { return tag ? t.has(slot) : (reader_on && r.has(slot)); }
    NFC_HD bool get(uint32_t slot, uint64_t &key) const { return tag ? t.get(slot, key) : (reader_on && r.get(slot, key)); }
};

template <class TagCard, class ReaderCard, class ReaderTab>
NFC_HD void run_pair(const TagCard &T, const ReaderCard &R, uint64_t reader_key_a, uint64_t reader_key_b, const ReaderTab &rtab, uint32_t link,
                     uint32_t rounds, const Slab &O, uint8_t *__restrict__ scratch, nfc_emu_pair_result &res) {
    State st, sr;
    state_init(st);
    state_init(sr);
    Machine mt, mr;
    machine_init(mt);
    machine_init(mr);
    if (T.tag_type == 1) keys_from_mem(T, mt.key_a, mt.key_b);
    mr.key_a = reader_key_a, mr.key_b = reader_key_b;
    const TrailerTable<TagCard> ttab = {T};
    uint8_t *ab = scratch, *ap = scratch + 20, *data = scratch + 40;
    uint16_t *enc = (uint16_t *)(scratch + 64);   // 40 entries to scratch + 144
    uint32_t n_frames = 0, n_bytes = 0, flags = 0, round = 0, steps = 0;
    bool to_tag = true, seed = true, open = true;   // open: the slab still takes frames (a frame that does not fit closes it for good)
    Ans cur = plain_answer(C_REQA);
    while (round < rounds) {
        const int type = def_of(cur.cmd).type();
        const uint32_t n = cur.n;
        const uint32_t plain_par = seed ? 0u : odd_parity_of(cur.B, n);   // (a short frame has no ninth bit: the repair assumes the start bit, 0)
        FrameOut air = {{}, 0u, 0u};
        bool as_plain = true;
        // the sender's machine: AIR only, and the loop's own REQA passes no machine (binary_src repeats it, usrp_nfc.py:45)
        if (link == NFC_EMU_LINK_AIR && !seed) {
            Machine M = to_tag ? mr : mt;
            const SideTable<TrailerTable<TagCard>, ReaderTab> tab = {ttab, rtab, !to_tag, R.mode == NFC_EMU_CARD};
            const bool card = (to_tag ? R.mode : T.mode) == NFC_EMU_CARD;
            const FrameIn in = {cur.B, plain_par};
            if (outgoing(M, (size_t)9u * n, cur.cmd, in, air, tab, card)) {
                // an Ultralight: the frame goes through the machine as if heard, "update state" (fsm.py:71-72)
                for (uint32_t i = 0; i < n; i++) ab[i] = (uint8_t)cur.B.at(i), ap[i] = (uint8_t)((plain_par >> i) & 1u);
                (void)process_frame(M, type, raw_flags_of(n, ab, ap), n, ab, ap, data, enc, tab);
            } else {
                as_plain = false;
            }
            if (to_tag) mr = M;
            else mt = M;
        }
        // the frame into the slab (true counts whatever fits) and into the scratch the receiving machine reads
        {
            const bool fits = open && n_frames < O.cap_frames && n_bytes + n <= O.cap_bytes;
            bool differs = false;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t pb = cur.B.at(i), b = as_plain ? pb : air.B.at(i), p = ((as_plain ? plain_par : air.par) >> i) & 1u;
                differs = differs || b != pb;
                ab[i] = (uint8_t)b, ap[i] = (uint8_t)p;
                if (fits) O.plain[n_bytes + i] = (uint8_t)pb, O.air[n_bytes + i] = (uint8_t)b, O.par[n_bytes + i] = (uint8_t)p;
            }
            if (fits) {
                nfc_emu_frame f;
                f.cmd = (int16_t)cur.cmd, f.type = (uint8_t)type;
                f.flags = (uint8_t)((seed ? NFC_EMU_FRAME_SEED : 0u) | (differs ? NFC_EMU_FRAME_ENCRYPTED : 0u));
                f.byte_off = n_bytes, f.n_bytes = (uint16_t)n, f.n_bits = (uint16_t)(seed ? 7u : 9u * n), f.round = round;
                O.frames[n_frames] = f;
            } else {
                if (open) flags |= n_frames >= O.cap_frames ? NFC_EMU_PAIR_CUT_FRAMES : NFC_EMU_PAIR_CUT_BYTES;
                open = false;
            }
            n_frames++;
            n_bytes += n;
        }
        // the receiver: its machine first (AIR), then the emulator
        int cmd = cur.cmd;
        uint32_t h = (uint32_t)def_of(cur.cmd).n_header(), ne = n - h - (def_of(cur.cmd).crc() ? 2u : 0u);
        Bytes B = cur.B;
        if (link == NFC_EMU_LINK_AIR) {
            Machine M = to_tag ? mt : mr;
            const SideTable<TrailerTable<TagCard>, ReaderTab> tab = {ttab, rtab, to_tag, R.mode == NFC_EMU_CARD};
            const Rec r = process_frame(M, type, raw_flags_of(n, ab, ap), n, ab, ap, data, enc, tab);
            if (to_tag) mt = M;
            else mr = M;
            cmd = r.cmd, h = r.n_header, ne = r.n_extra;
            Bytes D = {};
            for (uint32_t i = 0; i < r.n_bytes && i < 20u; i++) D.put(i, data[i]);
            B = D;
        }
        const Ans a = to_tag ? tag_step(st, T, cmd, B, h, ne) : reader_step(sr, R, cmd, B, h, ne);
        steps++;
        if (a.cmd < 0 || steps >= ROUND_STEPS) {   // usrp_nfc.py:125-131: REQA again, the tag woken
            if (a.cmd >= 0) flags |= NFC_EMU_PAIR_RUNAWAY;
            cur = plain_answer(C_REQA);
            seed = true;
            to_tag = true;
            st.halted = 0;
            steps = 0;
            round++;
            if (link == NFC_EMU_LINK_AIR && R.mode == NFC_EMU_CARD) {   // a reader that starts over has dropped its session (the reference's keeps it)
                uid_clear(mr);
                mr.tag_type = -1, mr.encrypted = 0, mr.cur_cmd = C_REQA;
            }
        } else {
            cur = a;
            seed = false;
            to_tag = !to_tag;
        }
    }
    res.n_frames = n_frames, res.n_bytes = n_bytes, res.flags = flags, res.rounds = round;
    res.tag_flags = st.flags, res.reader_flags = sr.flags;
    res.tag_fsm_flags = mt.flags, res.reader_fsm_flags = mr.flags;
}

}  // namespace emu
}  // namespace nfc
