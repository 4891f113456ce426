// frames.hip.h -- closed packets -> frames: the repair of the frame end (fsm.py:49-66), nine bits to a byte with the odd-parity check
// (fsm.py:28-47) and the ISO 14443-3 CRC_A (utilities.py:30-41), per packet.  One restatement, assemble_frame, shared by the kernels
// (nfc_frames.hip) and their host twin (nfc_host_frames); and what nfc_amd.hip and nfc_multi.hip reach of nfc_frames.hip.
//
// A frame's bits come from one of three sources (the template parameter Src of assemble_frame):
//   PackedBits  32 bits to a word at an arbitrary bit offset -- what the multi-launch stages leave (decode.hip.h: k_frame_write).  A
//               nine-bit field straddles words: two words funnelled through 64 bits;
//   ByteBits    a byte per bit -- k_small_stage's batches (bits_packed == false), a multi-stream context's slab rows, the host twin.
// Neither reads a bit at or behind the packet's end: with n_bits % 9 == 8 the last field's ninth bit is NOT the array's next bit (that
// is the next packet's first) but the start bit, and the array may end with the packet.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"

namespace nfc {
namespace frames {

__host__ __device__ __forceinline__ uint32_t frame_bytes_of(uint32_t n_bits) {
    return n_bits % 9u == 8u ? (n_bits + 1u) / 9u : n_bits / 9u;
}
// one byte into the CRC_A register (fsm.hip.h: crc_a -- reflected 0x8408, the caller starts from 0x6363)
__host__ __device__ __forceinline__ uint32_t crc_a_step(uint32_t w, uint32_t byte) {
    uint32_t b = (byte ^ w) & 0xFFu;
    b ^= (b << 4) & 0xFFu;
    return ((w >> 8) ^ (b << 8) ^ (b << 3) ^ (b >> 4)) & 0xFFFFu;
}
__host__ __device__ __forceinline__ uint32_t popc8(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(b);
#else
    return (uint32_t)__builtin_popcount(b);
#endif
}

struct PackedBits {
    using Word = uint32_t;
    const uint32_t *w;
    // up to nine bits from `pos`, none at or behind `end` (pos < end)
    __host__ __device__ __forceinline__ uint32_t field(uint64_t pos, uint64_t end) const {
        const uint64_t i = pos >> 5;
        const uint32_t s = (uint32_t)pos & 31u;
        uint64_t v = w[i];
        if (s > 23u && ((i + 1) << 5) < end) v |= (uint64_t)w[i + 1] << 32;   // (the second word only where the field reaches it and the packet does)
        const uint64_t left = end - pos;
        const uint32_t m = left >= 9 ? 0x1FFu : ((1u << (uint32_t)left) - 1u);
        return (uint32_t)(v >> s) & m;
    }
};
struct ByteBits {
    using Word = uint8_t;
    const uint8_t *b;
    __host__ __device__ __forceinline__ uint32_t field(uint64_t pos, uint64_t end) const {
        const uint64_t left = end - pos;
        const uint32_t n = left >= 9 ? 9u : (uint32_t)left;
        uint32_t v = 0;
        for (uint32_t j = 0; j < n; j++) v |= (uint32_t)(b[pos + j] & 1u) << j;
        return v;
    }
};

// One frame: n_bytes = frame_bytes_of(n_bits) bytes and parity bits to bytes[0 ..) / par[0 ..); returns the record's flags.
template <class Src>
__host__ __device__ __forceinline__ uint32_t assemble_frame(const Src &S, uint64_t bit_off, uint32_t n_bits, int type, uint32_t n_bytes,
                                                            uint8_t *__restrict__ bytes, uint8_t *__restrict__ par) {
    const uint32_t rem = n_bits % 9u, start_bit = type == 0 ? 1u : 0u;   // packets.py:24-28
    const uint64_t end = bit_off + n_bits;
    uint32_t flags = 0;
    if (rem == 1u) {
        if (S.field(end - 1, end) != start_bit) flags |= NFC_FRAME_EXTRA_ERROR;
    } else if (rem >= 2u && rem <= 7u) {
        flags |= NFC_FRAME_MANY_MORE_ERROR;
    }
    bool par_ok = n_bytes > 0;
    // the CRC register runs two bytes behind: after the loop it covers bytes[0 .. n - 2) and p2, p1 are the last two (the check of a frame's CRC_A)
    uint32_t crc = 0x6363u, p1 = 0, p2 = 0;
    for (uint32_t i = 0; i < n_bytes; i++) {
        uint32_t f = S.field(bit_off + 9ull * i, end);
        if (rem == 8u && i == n_bytes - 1u) f = (f & 0xFFu) | (start_bit << 8);
        const uint32_t b = f & 0xFFu, p = f >> 8;
        bytes[i] = (uint8_t)b;
        par[i] = (uint8_t)p;
        if ((popc8(b) & 1u) == p) par_ok = false;
        if (i >= 2u) crc = crc_a_step(crc, p2);
        p2 = p1;
        p1 = b;
    }
    if (par_ok) {
        flags |= NFC_RAW_PARITY_OK;
        if (n_bytes >= 2u && p2 == (crc & 0xFFu) && p1 == (crc >> 8)) flags |= NFC_RAW_CRC_A_OK;
    }
    return flags;
}

// ---- what nfc_frames.hip offers the other translation units --------------------------------------------------------------------
// Single context.  Per type t: closes[t] cumulative bit counts at the packet closes (d_close_end) and the closing edges' stream
// indices (d_close_idx), n_close[t] of them; the type's bit array, packed or a byte per bit.  Out: records[t] (room for n_close[t]),
// bytes[t] / par[t] (room for byte_cap[t]), totals[2 * t] = frames, totals[2 * t + 1] = bytes (device memory, uint64).
struct CtxArgs {
    const uint32_t *close_end[2];
    const uint64_t *close_idx[2];
    uint32_t n_close[2];
    const void *bits[2];
    nfc_raw_frame *records[2];
    uint8_t *bytes[2], *par[2];
    uint32_t byte_cap[2];
    uint64_t *totals;
};
// enqueues the scan and the assembly on `stream` (e0 / e1: events around the two launches, or null)
void launch_ctx(const CtxArgs &A, bool packed, hipStream_t stream, hipEvent_t e0, hipEvent_t e1);

// Multi-stream context: the slabs' close rows, counts and bit rows (multi.hip.h: Out, Caps -- passed as plain pointers so that this
// header needs none of that one).  table: [4][K + 1] uint64 on the device -- frame_off[0], frame_off[1], byte_off[0], byte_off[1] --
// written by the scan; packed: the buffer the assembly fills, laid out by MultiLayout (bytes from its start); its head receives the
// four totals.  Every section is followed by guard_bytes of the guard word.
struct MultiLayout {
    uint64_t at_fr[2], at_bytes[2], at_par[2];      // section starts
    uint64_t end_fr[2], end_bytes[2], end_par[2];   // where each section's guard starts
    uint64_t total_frames[2], total_bytes[2];       // the HOST's totals: the assembly cuts every range to them
};
struct MultiArgs {
    const uint2 *close[2];
    const uint8_t *bits[2];
    const uint32_t *counts;
    uint32_t cnt_words, cnt_pk0, cnt_bits0;         // words per stream in counts; index of the type-0 packet / bit count (type 1: + 1)
    uint32_t cap_packets, cap_bits, s_packets, s_bits;
    uint32_t K;
    uint64_t *table;
    uint8_t *packed;
    uint32_t guard_word, guard_bytes;
    MultiLayout F;
};
constexpr int MULTI_HEADER_BYTES = 64;
void launch_multi(const MultiArgs &A, hipStream_t stream, hipEvent_t e0, hipEvent_t e1);

}  // namespace frames
}  // namespace nfc
