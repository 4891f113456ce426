// nfc_frames.hip -- the frame assembly kernels in a translation unit of their own (frames.hip.h says what they compute; DESIGN.md 8f
// why they have this form), and their host twin nfc_host_frames.  nfc_amd.hip (nfc_read_frames ...) and nfc_multi.hip
// (nfc_multi_fetch_frames) launch them through frames::launch_ctx / launch_multi.
//
// Two launches each.  The SCAN gives every frame its place -- the exclusive prefixes of the frame and byte counts over the packet
// closes in stream order -- in one workgroup, tile after tile, the running totals carried in registers: no look-back, no atomics, so
// the layout cannot depend on an order of arrival.  The ASSEMBLY is a lane per frame: the lane walks its frame's nine-bit fields,
// stores a byte and a parity bit per field and keeps the parity verdict and the CRC_A register in scalars of its own.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/nfc_amd.h"
#include "launch_check.h"
#include "frames.hip.h"

namespace nfc {
namespace frames {

static_assert(sizeof(nfc_raw_frame) == 32, "nfc_raw_frame is 32 bytes");

constexpr int FS_THREADS = 1024, FS_WAVES = FS_THREADS / 64, FS_ITEMS = 4, FS_TILE = FS_THREADS * FS_ITEMS;
constexpr int FA_THREADS = 256;
constexpr uint32_t FA_MAX_WG = 2048;

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) { return (uint64_t)__shfl_up((unsigned long long)v, (unsigned)d, 64); }
__device__ __forceinline__ uint64_t wave_inclusive64(uint64_t v, uint32_t lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = shfl_up64(v, d);
        if ((int)lane >= d) v += up;
    }
    return v;
}
// a frame's contribution to the scan: one frame in the high word, its bytes in the low one (both stay far below 2^32 in a batch)
__device__ __forceinline__ uint64_t amount_of(uint32_t n_bits) { return n_bits ? (1ull << 32) | frame_bytes_of(n_bits) : 0ull; }

__device__ __forceinline__ void store_record(nfc_raw_frame *r, uint64_t idx, uint32_t byte_off, uint32_t n_bits, uint32_t n_bytes, uint32_t flags,
                                             int type) {
    uint4 *q = (uint4 *)r;   // (32-byte records in a 16-byte aligned array)
    q[0] = make_uint4((uint32_t)idx, (uint32_t)(idx >> 32), byte_off, n_bits);
    q[1] = make_uint4(n_bytes, flags, (uint32_t)type, 0u);
}

// ---- single context ------------------------------------------------------------------------------------------------------------
// Workgroup t scans type t's closes.  A close with end == prev closed an empty packet: no frame (packets.py:97).  The record is written
// here but for its verdict; until the assembly replaces it, `flags` holds the frame's first bit in the type's bit array.
__global__ __launch_bounds__(FS_THREADS) void k_frames_scan(CtxArgs A) {
    __shared__ uint64_t wave_sum[FS_WAVES];
    const int t = (int)blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nc = A.n_close[t];
    const uint32_t *__restrict__ ce = A.close_end[t];
    const uint64_t *__restrict__ ci = A.close_idx[t];
    nfc_raw_frame *__restrict__ rec = A.records[t];
    uint64_t run = 0;
    for (uint32_t base = 0; base < nc; base += FS_TILE) {
        const uint32_t k0 = base + tid * FS_ITEMS;
        const uint32_t prev = (k0 > 0 && k0 <= nc) ? ce[k0 - 1] : 0u;
        const uint32_t e0 = k0 + 0 < nc ? ce[k0 + 0] : prev;
        const uint32_t e1 = k0 + 1 < nc ? ce[k0 + 1] : e0;
        const uint32_t e2 = k0 + 2 < nc ? ce[k0 + 2] : e1;
        const uint32_t e3 = k0 + 3 < nc ? ce[k0 + 3] : e2;
        const uint64_t a0 = amount_of(e0 - prev), a1 = amount_of(e1 - e0), a2 = amount_of(e2 - e1), a3 = amount_of(e3 - e2);
        const uint64_t mine = a0 + a1 + a2 + a3;
        const uint64_t inc = wave_inclusive64(mine, lane);
        if (lane == 63u) wave_sum[wave] = inc;
        __syncthreads();
        uint64_t at = run + inc - mine, tile_total = 0;
        for (uint32_t w = 0; w < FS_WAVES; w++) {
            const uint64_t s = wave_sum[w];
            if (w < wave) at += s;
            tile_total += s;
        }
#define NFC_FRAME_PUT(j, from, to, amount)                                                                                     \
    if (amount) {                                                                                                              \
        store_record(rec + (at >> 32), ci[k0 + j], (uint32_t)at, (to) - (from), (uint32_t)(amount), (from), t);               \
        at += amount;                                                                                                          \
    }
        NFC_FRAME_PUT(0, prev, e0, a0)
        NFC_FRAME_PUT(1, e0, e1, a1)
        NFC_FRAME_PUT(2, e1, e2, a2)
        NFC_FRAME_PUT(3, e2, e3, a3)
#undef NFC_FRAME_PUT
        run += tile_total;
        __syncthreads();   // (wave_sum is written again by the next tile)
    }
    if (tid == 0) {
        A.totals[2 * t] = run >> 32;
        A.totals[2 * t + 1] = run & 0xFFFFFFFFull;
    }
}

template <class Src>
__global__ __launch_bounds__(FA_THREADS) void k_frames_assemble(CtxArgs A) {
    const int t = (int)blockIdx.y;
    const uint64_t f = (uint64_t)blockIdx.x * FA_THREADS + threadIdx.x;
    if (f >= A.totals[2 * t] || f >= A.n_close[t]) return;
    nfc_raw_frame *r = A.records[t] + f;
    const uint4 q0 = ((const uint4 *)r)[0], q1 = ((const uint4 *)r)[1];
    const uint32_t byte_off = q0.z, n_bits = q0.w, n_bytes = q1.x, bit_off = q1.y;
    uint32_t flags = 0;
    if ((uint64_t)byte_off + n_bytes <= A.byte_cap[t])   // (the host sized the arrays for the most the bits can give: never false)
        flags = assemble_frame(Src{(const typename Src::Word *)A.bits[t]}, bit_off, n_bits, t, n_bytes, A.bytes[t] + byte_off, A.par[t] + byte_off);
    r->flags = flags;
}

void launch_ctx(const CtxArgs &A, bool packed, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const uint32_t most = std::max(A.n_close[0], A.n_close[1]);
    const dim3 grid((most + FA_THREADS - 1) / FA_THREADS, 2);
    auto assemble = packed ? k_frames_assemble<PackedBits> : k_frames_assemble<ByteBits>;
    if (e0) NFC_LAUNCH_EXT(k_frames_scan, dim3(2), dim3(FS_THREADS), 0, stream, e0, nullptr, 0, A);
    else NFC_LAUNCH(k_frames_scan, dim3(2), dim3(FS_THREADS), 0, stream, A);
    if (e1) NFC_LAUNCH_EXT(assemble, grid, dim3(FA_THREADS), 0, stream, nullptr, e1, 0, A);
    else NFC_LAUNCH(assemble, grid, dim3(FA_THREADS), 0, stream, A);
}

// ---- multi-stream context --------------------------------------------------------------------------------------------------------
// What stream k stores of type t: its first min(count, cap_packets) closes (non-empty packets only: multi.hip.h), over the first
// min(count, cap_bits) bits of its row.  A packet that ends behind the stored bits is CUT: a frame of no bytes.
struct StreamPart {
    uint32_t npk, stored_bits;
};
__device__ __forceinline__ StreamPart part_of(const MultiArgs &A, uint32_t k, int t) {
    const uint32_t *c = A.counts + (size_t)k * A.cnt_words;
    const uint32_t pk = c[A.cnt_pk0 + t], bits = c[A.cnt_bits0 + t];
    return StreamPart{pk < A.cap_packets ? pk : A.cap_packets, bits < A.cap_bits ? bits : A.cap_bits};
}
__device__ __forceinline__ uint64_t stream_bytes(const MultiArgs &A, uint32_t k, int t, const StreamPart &p) {
    const uint2 *cl = A.close[t] + (size_t)k * A.s_packets;
    uint64_t nb = 0;
    uint32_t prev = 0;
    for (uint32_t i = 0; i < p.npk; i++) {
        const uint32_t end = cl[i].x;
        if (end <= p.stored_bits) nb += frame_bytes_of(end - prev);
        prev = end;
    }
    return nb;
}

// table[a][0 .. K], a = frames 0, frames 1, bytes 0, bytes 1: the exclusive prefix over the streams (table[a][K]: the total), the totals
// once more at the head of the packed buffer, and the guard bytes behind the sections.  One workgroup, a thread per run of consecutive
// streams (k_multi_fetch_scan's form); a stream's amounts wait in the table's own slots between the two passes.
__global__ __launch_bounds__(FS_THREADS) void k_multi_frames_scan(MultiArgs A) {
    __shared__ uint64_t wave_sum[4][FS_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, K = A.K;
    const uint32_t per = (K + FS_THREADS - 1) / FS_THREADS;
    const uint32_t k0 = tid * per < K ? tid * per : K, k1 = k0 + per < K ? k0 + per : K;
    const size_t T = (size_t)K + 1;
    uint64_t *__restrict__ tab = A.table;
    uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (uint32_t k = k0; k < k1; k++) {
        const StreamPart p0 = part_of(A, k, 0), p1 = part_of(A, k, 1);
        const uint64_t b0 = stream_bytes(A, k, 0, p0), b1 = stream_bytes(A, k, 1, p1);
        tab[0 * T + k] = p0.npk;
        tab[1 * T + k] = p1.npk;
        tab[2 * T + k] = b0;
        tab[3 * T + k] = b1;
        m0 += p0.npk, m1 += p1.npk, m2 += b0, m3 += b1;
    }
    const uint64_t i0 = wave_inclusive64(m0, lane), i1 = wave_inclusive64(m1, lane), i2 = wave_inclusive64(m2, lane), i3 = wave_inclusive64(m3, lane);
    if (lane == 63u) wave_sum[0][wave] = i0, wave_sum[1][wave] = i1, wave_sum[2][wave] = i2, wave_sum[3][wave] = i3;
    __syncthreads();
    uint64_t r0 = i0 - m0, r1 = i1 - m1, r2 = i2 - m2, r3 = i3 - m3;
    for (uint32_t w = 0; w < wave; w++) r0 += wave_sum[0][w], r1 += wave_sum[1][w], r2 += wave_sum[2][w], r3 += wave_sum[3][w];
    for (uint32_t k = k0; k < k1; k++) {   // (the slots this thread wrote above: no other thread touches them)
        const uint64_t a0 = tab[0 * T + k], a1 = tab[1 * T + k], a2 = tab[2 * T + k], a3 = tab[3 * T + k];
        tab[0 * T + k] = r0, tab[1 * T + k] = r1, tab[2 * T + k] = r2, tab[3 * T + k] = r3;
        r0 += a0, r1 += a1, r2 += a2, r3 += a3;
    }
    if (tid == FS_THREADS - 1) {   // (its range ends at K: r0 .. r3 are the totals)
        uint64_t *head = (uint64_t *)A.packed;
        tab[0 * T + K] = head[0] = r0;
        tab[1 * T + K] = head[1] = r1;
        tab[2 * T + K] = head[2] = r2;
        tab[3 * T + K] = head[3] = r3;
        head[4] = head[5] = head[6] = head[7] = 0;
    }
    if (tid < 6u * A.guard_bytes) {
        const uint32_t s = tid / A.guard_bytes, b = tid % A.guard_bytes;
        const uint64_t at = s < 2 ? A.F.end_fr[s] : s < 4 ? A.F.end_bytes[s - 2] : A.F.end_par[s - 4];
        A.packed[at + b] = (uint8_t)(A.guard_word >> (8 * (b & 3u)));
    }
}

// A wave per stream, grid-stride over the streams; the wave's lanes take the stream's frames, 64 at a time, a frame's place among the
// stream's bytes from a scan of the byte counts across the lanes.
__global__ __launch_bounds__(FA_THREADS) void k_multi_frames_assemble(MultiArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (FA_THREADS / 64) + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * (FA_THREADS / 64);
    const size_t T = (size_t)A.K + 1;
    const uint64_t *__restrict__ tab = A.table;
    for (uint32_t k = wave; k < A.K; k += waves) {
        for (int t = 0; t < 2; t++) {
            const StreamPart p = part_of(A, k, t);
            // the stream's ranges, cut to the sections (MultiLayout): the device's counts cannot write past what the host laid out
            uint64_t fe = tab[(size_t)t * T + k + 1], fb = tab[(size_t)t * T + k];
            fe = fe < A.F.total_frames[t] ? fe : A.F.total_frames[t];
            fb = fb < fe ? fb : fe;
            const uint64_t bb = tab[(size_t)(2 + t) * T + k];
            const uint32_t nfr = (uint32_t)(fe - fb) < p.npk ? (uint32_t)(fe - fb) : p.npk;
            const uint2 *cl = A.close[t] + (size_t)k * A.s_packets;
            const ByteBits S{A.bits[t] + (size_t)k * A.s_bits};
            nfc_raw_frame *rec = (nfc_raw_frame *)(A.packed + A.F.at_fr[t]) + fb;
            uint8_t *bytes = A.packed + A.F.at_bytes[t] + bb, *par = A.packed + A.F.at_par[t] + bb;
            uint32_t run = 0;
            for (uint32_t j0 = 0; j0 < nfr; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool have = j < nfr;
                const uint2 c = have ? cl[j] : make_uint2(0u, 0u);
                const uint32_t prev = have && j ? cl[j - 1].x : 0u;
                const uint32_t n_bits = c.x - prev;
                bool cut = c.x > p.stored_bits;
                uint32_t nb = have && !cut ? frame_bytes_of(n_bits) : 0u;
                uint32_t inc = nb;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)inc, (unsigned)d, 64);
                    if ((int)lane >= d) inc += up;
                }
                const uint32_t off = run + inc - nb;
                run += (uint32_t)__shfl((int)inc, 63, 64);
                if (!have) continue;
                if (bb + off + nb > A.F.total_bytes[t]) cut = true, nb = 0;   // (never: the host's section holds the most the stored bits give)
                const uint32_t flags = cut ? (uint32_t)NFC_RAW_CUT : assemble_frame(S, prev, n_bits, t, nb, bytes + off, par + off);
                store_record(rec + j, c.y, off, n_bits, nb, flags, t);
            }
        }
    }
}

void launch_multi(const MultiArgs &A, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const uint32_t want = (A.K + FA_THREADS / 64 - 1) / (FA_THREADS / 64);
    const uint32_t blocks = std::max(1u, std::min(want, FA_MAX_WG));   // (a wave per stream, grid-stride beyond: k_multi_fetch_gather's grid)
    if (e0) NFC_LAUNCH_EXT(k_multi_frames_scan, dim3(1), dim3(FS_THREADS), 0, stream, e0, nullptr, 0, A);
    else NFC_LAUNCH(k_multi_frames_scan, dim3(1), dim3(FS_THREADS), 0, stream, A);
    if (e1) NFC_LAUNCH_EXT(k_multi_frames_assemble, dim3(blocks), dim3(FA_THREADS), 0, stream, nullptr, e1, 0, A);
    else NFC_LAUNCH(k_multi_frames_assemble, dim3(blocks), dim3(FA_THREADS), 0, stream, A);
}

}  // namespace frames
}  // namespace nfc

// ---- the host twin ------------------------------------------------------------------------------------------------------------
extern "C" int nfc_host_frames(const nfc_packet *packets, size_t n, const uint8_t *bits, int type, nfc_raw_frame *out, uint8_t *bytes,
                               uint8_t *par, size_t cap, size_t *used) {
    using namespace nfc::frames;
    if ((n && (!packets || !out)) || (type != 0 && type != 1)) return NFC_ERR_ARG;
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const nfc_packet &p = packets[i];
        if (p.type != type || p.n_bits == 0 || !bits) return NFC_ERR_ARG;
        const uint32_t nb = frame_bytes_of(p.n_bits);
        if (at + nb > cap || at + nb > 0xFFFFFFFFull || (nb && (!bytes || !par))) return NFC_ERR_ARG;
        nfc_raw_frame r;
        memset(&r, 0, sizeof r);
        r.idx = p.idx;
        r.byte_off = (uint32_t)at;
        r.n_bits = p.n_bits;
        r.n_bytes = nb;
        r.type = type;
        r.flags = assemble_frame(ByteBits{bits}, p.bit_off, p.n_bits, type, nb, bytes ? bytes + at : nullptr, par ? par + at : nullptr);
        out[i] = r;
        at += nb;
    }
    if (used) *used = at;
    return NFC_OK;
}
