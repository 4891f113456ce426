// multi_fetch.hip.h -- the fetch of a multi-stream context (nfc_multi_fetch, include/nfc_amd.h): what every stream stored in the last
// push, compacted from the per-stream slabs (multi.hip.h: Out) into ONE packed buffer that goes to the host in one copy.
//
// Two launches.  k_multi_fetch_scan turns the counts into the exclusive prefix of the stored amounts, per array: a table
// [MF_ARRAYS][K + 1] of uint64 that stays on the device (the host forms the same table from its mirror of the counts; the seven totals
// travel at the head of the packed buffer and must agree).  k_multi_fetch_gather copies every stream's stored prefix of every row to
// its place: a WAVE per stream, grid-stride over the streams, the wave looping the stream's eight rows.  The packed sections are
//     totals (MF_HEADER_BYTES) | epos | ecode | sym 0 | sym 1 | packets 0 | packets 1 | bits 0 | bits 1
// each starting on 16 bytes, tight inside (entry granularity, no padding between streams), GUARD_BYTES of the guard word behind each.
// The gather is source-centric: a stream's place is two table words, read once per row by the whole wave (no search per thread), and a
// row is one contiguous copy -- 16-byte stores to the 16-byte aligned body of the destination fed from 16-byte loads of whatever
// alignment the source then has, bytes for the head and the tail.  nfc_packet records are written from the `close` pairs; their idx is
// batch-local here and the host adds the stream's base (few packets; no upload with the fetch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "multi.hip.h"

namespace nfc {
namespace multi {

constexpr int MF_ARRAYS = 7;            // NFC_MF_*: edges, symbols 0 / 1, packets 0 / 1, bits 0 / 1 -- the order of CNT_EDGES .. CNT_BITS1
constexpr int MF_SECTIONS = 8;          // the edges are two rows: positions and codes
constexpr int MF_SCAN_THREADS = 1024;   // ONE workgroup: at most 64 consecutive streams per thread (K <= 65536)
constexpr int MF_HEADER_BYTES = 64;     // seven totals (uint64), padded to the first section's alignment
constexpr int MF_GATHER_THREADS = 256, MF_GATHER_MAX_WG = 2048;
constexpr uint32_t MF_EDGES = 1, MF_SYMBOLS = 2, MF_PACKETS = 4;   // NFC_MULTI_FETCH_*
static_assert(CNT_EDGES == 0 && CNT_SYM0 == 1 && CNT_SYM1 == 2 && CNT_PK0 == 3 && CNT_PK1 == 4 && CNT_BITS0 == 5 && CNT_BITS1 == 6,
              "the fetch's arrays are the first seven count words, in their order");

#define MF_EACH(X) X(a0) X(a1) X(a2) X(a3) X(a4) X(a5) X(a6)

// stored entries of the seven arrays, in named scalars (no indexed per-thread arrays: no scratch)
struct Amounts {
    uint64_t a0, a1, a2, a3, a4, a5, a6;
};

// what a stream stored: the count cut to the slab's capacity -- what the per-stream readers return -- and 0 for arrays not asked for
__host__ __device__ inline Amounts stored_amounts(const uint32_t *c, const Caps &C, uint32_t what) {
    Amounts r;
    const bool e = (what & MF_EDGES) != 0, s = (what & MF_SYMBOLS) != 0, p = (what & MF_PACKETS) != 0;
    r.a0 = e ? (c[CNT_EDGES] < C.edges ? c[CNT_EDGES] : C.edges) : 0u;
    r.a1 = s ? (c[CNT_SYM0] < C.symbols ? c[CNT_SYM0] : C.symbols) : 0u;
    r.a2 = s ? (c[CNT_SYM1] < C.symbols ? c[CNT_SYM1] : C.symbols) : 0u;
    r.a3 = p ? (c[CNT_PK0] < C.packets ? c[CNT_PK0] : C.packets) : 0u;
    r.a4 = p ? (c[CNT_PK1] < C.packets ? c[CNT_PK1] : C.packets) : 0u;
    r.a5 = p ? (c[CNT_BITS0] < C.bits ? c[CNT_BITS0] : C.bits) : 0u;
    r.a6 = p ? (c[CNT_BITS1] < C.bits ? c[CNT_BITS1] : C.bits) : 0u;
    return r;
}

// where the packed sections start (bytes from the buffer's start) and how many entries each array's section holds: the HOST's totals.
// The gather cuts every stream's range to them, so counts that disagree with the host's mirror cannot write past a section -- the
// host then sees the device's totals differ and refuses the fetch.
struct FetchLayout {
    uint64_t at_epos, at_ecode, at_sym0, at_sym1, at_pk0, at_pk1, at_bits0, at_bits1;
    uint64_t end_epos, end_ecode, end_sym0, end_sym1, end_pk0, end_pk1, end_bits0, end_bits1;   // where each section's guard starts
    Amounts total;
};

__device__ inline uint64_t mf_shfl_up(uint64_t v, int d) { return (uint64_t)__shfl_up((unsigned long long)v, (unsigned)d, 64); }

// The exclusive prefix of the stored amounts per array, table[a][0 .. K] (table[a][K]: the total), the totals once more at the head of
// the packed buffer, and the guard bytes behind the sections.  One workgroup; a thread sums its consecutive streams, the sums are
// scanned in the wave by __shfl_up and across the sixteen waves through LDS; no look-back, no atomics.
__global__ __launch_bounds__(MF_SCAN_THREADS) void k_multi_fetch_scan(const uint32_t *__restrict__ counts, Caps C, uint32_t K, uint32_t what,
                                                                      uint64_t *__restrict__ table, uint8_t *__restrict__ packed, FetchLayout F) {
    __shared__ uint64_t wave_sum[MF_ARRAYS][MF_SCAN_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (K + MF_SCAN_THREADS - 1) / MF_SCAN_THREADS;
    const uint32_t k0 = tid * per < K ? tid * per : K, k1 = k0 + per < K ? k0 + per : K;
    Amounts mine = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = k0; k < k1; k++) {
        const Amounts s = stored_amounts(counts + (size_t)k * CNT_WORDS, C, what);
#define X(f) mine.f += s.f;
        MF_EACH(X)
#undef X
    }
    Amounts inc = mine;   // inclusive over the wave's lanes
    for (int d = 1; d < 64; d <<= 1) {
#define X(f) { const uint64_t up = mf_shfl_up(inc.f, d); if ((int)lane >= d) inc.f += up; }
        MF_EACH(X)
#undef X
    }
    if (lane == 63u) {
        wave_sum[0][wave] = inc.a0;
        wave_sum[1][wave] = inc.a1;
        wave_sum[2][wave] = inc.a2;
        wave_sum[3][wave] = inc.a3;
        wave_sum[4][wave] = inc.a4;
        wave_sum[5][wave] = inc.a5;
        wave_sum[6][wave] = inc.a6;
    }
    __syncthreads();
    Amounts run;   // exclusive: everything before this thread's first stream
#define X(f) run.f = inc.f - mine.f;
    MF_EACH(X)
#undef X
    for (uint32_t w = 0; w < wave; w++) {
        run.a0 += wave_sum[0][w];
        run.a1 += wave_sum[1][w];
        run.a2 += wave_sum[2][w];
        run.a3 += wave_sum[3][w];
        run.a4 += wave_sum[4][w];
        run.a5 += wave_sum[5][w];
        run.a6 += wave_sum[6][w];
    }
    const size_t T = (size_t)K + 1;
    for (uint32_t k = k0; k < k1; k++) {
        const Amounts s = stored_amounts(counts + (size_t)k * CNT_WORDS, C, what);
        table[0 * T + k] = run.a0;
        table[1 * T + k] = run.a1;
        table[2 * T + k] = run.a2;
        table[3 * T + k] = run.a3;
        table[4 * T + k] = run.a4;
        table[5 * T + k] = run.a5;
        table[6 * T + k] = run.a6;
#define X(f) run.f += s.f;
        MF_EACH(X)
#undef X
    }
    if (tid == MF_SCAN_THREADS - 1) {   // (its range ends at K: `run` is the total)
        uint64_t *head = (uint64_t *)packed;
        table[0 * T + K] = head[0] = run.a0;
        table[1 * T + K] = head[1] = run.a1;
        table[2 * T + K] = head[2] = run.a2;
        table[3 * T + K] = head[3] = run.a3;
        table[4 * T + K] = head[4] = run.a4;
        table[5 * T + K] = head[5] = run.a5;
        table[6 * T + K] = head[6] = run.a6;
        head[7] = 0;
    }
    if (tid < MF_SECTIONS * GUARD_BYTES) {   // (a section's end is only as aligned as its entries: bytes)
        const uint32_t s = tid / GUARD_BYTES, b = tid % GUARD_BYTES;
        const uint64_t at = s == 0 ? F.end_epos : s == 1 ? F.end_ecode : s == 2 ? F.end_sym0 : s == 3 ? F.end_sym1 : s == 4 ? F.end_pk0
                          : s == 5 ? F.end_pk1 : s == 6 ? F.end_bits0 : F.end_bits1;
        packed[at + b] = (uint8_t)(GUARD_WORD >> (8 * (b & 3u)));
    }
}

struct Bytes16 {
    uint32_t w[4];
} __attribute__((packed, aligned(1)));   // a 16-byte load of any alignment

// n bytes from src to dst by one wave: the destination's 16-byte aligned body in 16-byte stores, head and tail in bytes
__device__ inline void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t n, uint32_t lane) {
    const uint64_t to_align = (16u - ((uintptr_t)dst & 15u)) & 15u;
    const uint32_t head = (uint32_t)(n < to_align ? n : to_align);
    if (lane < head) dst[lane] = src[lane];
    const uint64_t body = (n - head) >> 4;
    const uint8_t *s = src + head;
    uint4 *d = (uint4 *)(dst + head);
    for (uint64_t i = lane; i < body; i += 64) {
        const Bytes16 v = *(const Bytes16 *)(s + 16 * i);
        d[i] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    }
    const uint32_t tail = (uint32_t)((n - head) & 15u);
    const uint64_t done = head + 16 * body;
    if (lane < tail) dst[done + lane] = src[done + lane];
}

// nfc_packet records (idx u64 | bit_off u64 | n_bits u32 | type i32) from the (cumulative bit count, closing position) pairs: the
// bits of a packet are those since its predecessor's count; idx stays batch-local (the host adds the stream's base)
__device__ inline void wave_packets(uint64_t *__restrict__ dst, const uint2 *__restrict__ cl, uint64_t n, uint32_t type, uint32_t lane) {
    for (uint64_t i = lane; i < n; i += 64) {
        const uint2 c = cl[i];
        const uint32_t prev = i ? cl[i - 1].x : 0u;
        dst[3 * i] = c.y;
        dst[3 * i + 1] = prev;
        dst[3 * i + 2] = (uint64_t)(c.x - prev) | ((uint64_t)type << 32);
    }
}

struct GatherArgs {
    Out O;
    Caps C;
    uint32_t K;
    const uint64_t *table;
    uint8_t *packed;
    FetchLayout F;
};

__global__ __launch_bounds__(MF_GATHER_THREADS) void k_multi_fetch_gather(GatherArgs G) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (MF_GATHER_THREADS / 64) + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * (MF_GATHER_THREADS / 64);
    const size_t T = (size_t)G.K + 1;
    const uint64_t *__restrict__ tab = G.table;
    uint8_t *P = G.packed;
    for (uint32_t k = wave; k < G.K; k += waves) {
        // stream k's range of array a, cut to the section (FetchLayout): b <= e <= total
#define RANGE(a, f)                                                       \
    uint64_t e##a = tab[a * T + k + 1], b##a = tab[a * T + k];           \
    e##a = e##a < G.F.total.f ? e##a : G.F.total.f;                       \
    b##a = b##a < e##a ? b##a : e##a;
        RANGE(0, a0)
        RANGE(1, a1)
        RANGE(2, a2)
        RANGE(3, a3)
        RANGE(4, a4)
        RANGE(5, a5)
        RANGE(6, a6)
#undef RANGE
        wave_copy(P + G.F.at_epos + b0 * 4, (const uint8_t *)(G.O.epos + (size_t)k * G.C.s_epos), (e0 - b0) * 4, lane);
        wave_copy(P + G.F.at_ecode + b0 * 2, (const uint8_t *)(G.O.ecode + (size_t)k * G.C.s_ecode), (e0 - b0) * 2, lane);
        wave_copy(P + G.F.at_sym0 + b1, G.O.sym[0] + (size_t)k * G.C.s_symbols, e1 - b1, lane);
        wave_copy(P + G.F.at_sym1 + b2, G.O.sym[1] + (size_t)k * G.C.s_symbols, e2 - b2, lane);
        wave_packets((uint64_t *)(P + G.F.at_pk0) + 3 * b3, G.O.close[0] + (size_t)k * G.C.s_packets, e3 - b3, 0u, lane);
        wave_packets((uint64_t *)(P + G.F.at_pk1) + 3 * b4, G.O.close[1] + (size_t)k * G.C.s_packets, e4 - b4, 1u, lane);
        wave_copy(P + G.F.at_bits0 + b5, G.O.bits[0] + (size_t)k * G.C.s_bits, e5 - b5, lane);
        wave_copy(P + G.F.at_bits1 + b6, G.O.bits[1] + (size_t)k * G.C.s_bits, e6 - b6, lane);
    }
}

}  // namespace multi
}  // namespace nfc
