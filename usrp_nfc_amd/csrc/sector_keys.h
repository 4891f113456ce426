// sector_keys.h -- the per-sector key table of the protocol machine (fsm.hip.h), stated once for its three holders: the host machine
// (protocol.h), nfc_host_commands on the CPU and k_multi_commands (multi_commands.hip.h).  DESIGN.md 8j.
//
// The rule.  A Classic card has at most 40 sectors: blocks 0 .. 127 lie four to a sector, blocks 128 .. 255 sixteen.  A table has 80
// slots, slot = (key_type & 1) * 40 + sector, each empty or six key bytes.  A machine that recognises AUTHA / AUTHB takes the block from
// the command's plaintext byte 1 and CHOOSES: the slot when the table holds it, else its own key A / key B as before.  The choice, not
// the key, is what the state carries to the nonce frame that loads the register -- cur_key: 0 / 1 the machine's key A / B, 2 + slot the
// table's slot -- so it survives a push boundary in the words the state already has.  The nonce frame RESOLVES it: the slot's key, or,
// when the slot was emptied in between (or there is no table any more), the key A / B of the slot's type.
// An empty table never chooses a slot: cur_key stays 0 / 1 and every bit is as it was without one.
//
// The table is reached through an accessor -- bool get(slot, key) -- so that one text serves the three holders:
// (has(slot): is it present, without the key.)
//   HostTable     an nfc_fsm_key_table (null: empty)
//   DeviceTable   the device's word arrays [slot][2][K], stream k (null: empty): word 0 key bits 0 .. 31, word 1 bits 32 .. 47 and
//                 PRESENT above them.  Lanes of a wave that look up one slot load neighbouring words.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"

#if defined(__HIPCC__)
#define NFC_SK_HD __host__ __device__ __forceinline__
#else
#define NFC_SK_HD inline
#endif

namespace nfc {
namespace skeys {

constexpr uint32_t SECTORS = 40, SLOTS = 2 * SECTORS, WORDS = 2 * SLOTS;   // (WORDS: one stream's words on the device)
constexpr uint32_t PRESENT = 1u << 16;                                     // in word 1, above key bits 32 .. 47
constexpr int32_t CUR_KEY_MAX = 2 + (int32_t)SLOTS - 1;                    // cur_key: 0, 1, 2 + slot

NFC_SK_HD uint32_t sector_of(uint32_t block) {
    block &= 0xFFu;
    return block < 128u ? block >> 2 : 32u + ((block - 128u) >> 4);
}
// below SLOTS by arithmetic (a byte's sector is at most 39), and clamped besides
NFC_SK_HD uint32_t slot_of(uint32_t key_type, uint32_t block) {
    const uint32_t s = (key_type & 1u) * SECTORS + sector_of(block);
    return s < SLOTS ? s : SLOTS - 1u;
}
NFC_SK_HD uint64_t key48(const uint8_t k[6]) {   // byte 0 lowest: the register load_key makes of it
    uint64_t v = 0;
    for (int i = 0; i < 6; i++) v |= (uint64_t)k[i] << (8 * i);
    return v;
}

struct HostTable {
    const nfc_fsm_key_table *t;
    NFC_SK_HD bool get(uint32_t slot, uint64_t &key) const {
        if (!t || slot >= SLOTS) return false;
        const uint32_t type = slot / SECTORS, sec = slot % SECTORS;
        if (t->present[type][sec] != 1) return false;
        key = key48(t->key[type][sec]);
        return true;
    }
    NFC_SK_HD bool has(uint32_t slot) const { return t && slot < SLOTS && t->present[slot / SECTORS][slot % SECTORS] == 1; }
};
struct DeviceTable {
    const uint32_t *w;   // [SLOTS][2][K]
    uint32_t K, k;       // k < K, the holder's promise (k_multi_commands returns before it makes one for a lane beyond K); a context holds
                         // at most 65 536 streams, so WORDS * K words are indexed in 32 bits
    NFC_SK_HD bool get(uint32_t slot, uint64_t &key) const {
        if (!w || slot >= SLOTS) return false;
        const uint32_t at = slot * 2u * K + k;
        const uint32_t hi = w[at + K];
        if (!(hi & PRESENT)) return false;
        key = (uint64_t)w[at] | (uint64_t)(hi & 0xFFFFu) << 32;
        return true;
    }
    NFC_SK_HD bool has(uint32_t slot) const { return w && slot < SLOTS && (w[slot * 2u * K + k + K] & PRESENT) != 0; }
};
// a key as the device's two words
NFC_SK_HD uint32_t word_lo(uint64_t key) { return (uint32_t)key; }
NFC_SK_HD uint32_t word_hi(uint64_t key, bool present) { return present ? ((uint32_t)(key >> 32) & 0xFFFFu) | PRESENT : 0u; }

// at an AUTHA (key_type bit 0) / AUTHB (1) on `block`: what cur_key becomes
template <class Table>
NFC_SK_HD int32_t choose(const Table &tab, uint32_t key_type, uint32_t block) {
    const uint32_t slot = slot_of(key_type, block);
    return tab.has(slot) ? (int32_t)(2u + slot) : (int32_t)(key_type & 1u);
}
// at the nonce frame: the key a cur_key stands for
template <class Table>
NFC_SK_HD uint64_t resolve(const Table &tab, int32_t cur_key, uint64_t key_a, uint64_t key_b) {
    // (cur_key 0 / 1, or the type of a slot that is no longer there)
    uint64_t key = (cur_key == 1 || cur_key >= 2 + (int32_t)SECTORS) ? key_b : key_a;
    if (cur_key >= 2) {
        const uint32_t slot = (uint32_t)cur_key - 2u;
        tab.get(slot < SLOTS ? slot : SLOTS - 1u, key);
    }
    return key;
}

// what is wrong with a caller's table, or null
inline const char *table_fault(const nfc_fsm_key_table &t) {
    for (uint32_t type = 0; type < 2; type++)
        for (uint32_t s = 0; s < SECTORS; s++)
            if (t.present[type][s] > 1) return "present must be 0 or 1";
    return nullptr;
}

}  // namespace skeys
}  // namespace nfc
