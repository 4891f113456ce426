// multi.hip.h -- K independent streams in one launch, a LANE per stream (nfc_multi, include/nfc_amd.h).
//
// The threshold recurrence (transition_sink.py:55-99) is sequential per stream, which is why the single-stream path speculates
// and certifies.  Across streams it is parallel as it stands: here every lane runs the reference's loop literally, for its own
// stream -- the fp64 window sum accumulated in the reference's order, so there is no speculation, no certification, no re-run
// and no exactness guard (nothing is reordered: the sum IS the reference's, inexact or non-finite as it may be).  When `val`
// changes or a run times out the lane builds the entry as edges.hip.h defines it (v, d, t; edge_code), appends it to the stream's
// slab, steps the routed decoder through the duration LUTs of decoder_tables.h and frames the symbols (packets.py:67-79), all in
// the same lane: entries are 6-13 % of the samples, and a second launch would read them back from memory.
//
// State: device arrays [field][stream]; the window [slot][stream], so that lanes whose streams are in step touch consecutive
// addresses.  Outputs: per-stream slabs of fixed capacity [stream][entry]; the counts are the true totals whatever was stored.
// Loads: a lane fetches MU raw samples and the MU window slots they will meet before it walks them -- MU independent loads in
// flight per round trip instead of one; the samples of a stream are consecutive, so a cache line serves the lane for 16 fc32
// samples (64 of the 2-byte kinds).  A stream's start is only sample-aligned: the loads are per sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edges.hip.h"
#include "threshold.hip.h"

namespace nfc {
namespace multi {

constexpr int MB = 64;   // one wave per workgroup: 64 streams
constexpr int MU = 8;    // samples (and window slots) fetched ahead of the walk; the window holds at least 2 MU slots for it
constexpr uint32_t GUARD_WORD = 0xA5C3F00Du;
constexpr int GUARD_BYTES = 16;   // behind every stream's row of every slab
constexpr uint32_t MAX_CAP = 1u << 26;   // the largest capacity nfc_multi_create takes: row strides (uint32) stay far from wrapping

enum : uint32_t { F_EDGES = 1, F_SYMBOLS = 2, F_PACKETS = 4, F_BITS = 8, F_PENDING = 16 };   // NFC_MULTI_*
enum : int { CNT_EDGES = 0, CNT_SYM0, CNT_SYM1, CNT_PK0, CNT_PK1, CNT_BITS0, CNT_BITS1, CNT_FLAGS, CNT_PKBITS0, CNT_PKBITS1, CNT_WORDS = 12 };

// edge word: cur_state | (last_bit + 1) << 2 | dur << 4;  dec word: miller | manchester << 4 | started[0] << 8 | started[1] << 9
__host__ __device__ inline uint32_t pack_edge(int state, int last_bit, int dur) { return (uint32_t)state | ((uint32_t)(last_bit + 1) << 2) | ((uint32_t)dur << 4); }
__host__ __device__ inline uint32_t pack_dec(int mil, int man, int s0, int s1) { return (uint32_t)mil | ((uint32_t)man << 4) | ((uint32_t)s0 << 8) | ((uint32_t)s1 << 9); }
constexpr uint32_t EDGE_INIT = 0u | (1u << 2) | (1u << 4);   // idle, last_bit 0, dur 1 (transition_sink.py:22-23,30)
constexpr uint32_t DEC_INIT = 0u | (2u << 4);                // miller.py:22,29; manchester.py:22-25: prev_set False, prev 0

struct State {
    double *ss;          // transition_sink._sum
    uint32_t *slot;      // window slot of the next sample (while the window fills: the slot the first stable sample will take)
    int32_t *filled;     // transition_sink._filled; == av_window: stable
    uint32_t *edge, *dec;
    uint32_t *npend[2];  // PacketProcessor._cur lengths
    uint32_t *flags;     // the sticky NFC_MULTI_PENDING_OVERFLOW
    float *ring;         // [slot][stream]
    uint8_t *pending[2]; // [stream][cap_pending]
};
struct Out {
    uint32_t *epos;      // [stream][stride]: batch-local sample position
    uint16_t *ecode;     // edges.hip.h: edge_code
    uint8_t *sym[2], *bits[2];
    uint2 *close[2];     // (end in the type's bit array, batch-local sample position of the closing edge), non-empty packets only
    uint32_t *counts;    // [stream][CNT_WORDS]
};
struct Caps {
    uint32_t edges, symbols, packets, bits, pending;            // entries stored per stream
    uint32_t s_epos, s_ecode, s_symbols, s_packets, s_bits, s_pending;  // row strides in entries (capacity + the guard)
};
struct Args {
    const void *in;
    const uint64_t *first;
    const uint32_t *n, *order;   // order: lane -> stream (streams of like length share a wave)
    uint32_t K;
    int32_t L, mx, nd, reader, tag, bands_ok;
    float scale;
    double lo, hi, hi_plus, lo_a, lo_b, hi_a, hi_b;
    const uint16_t *mil_step, *man_step;   // next state | out byte << 8 per (LUT row, state): decoder_tables.h
    State S;
    Out O;
    Caps C;
};

// One lane's stream while it is walked: everything in named scalars (no indexed per-thread arrays: no scratch).
struct Lane {
    uint32_t k, ne, flags;
    uint32_t nsym0, nsym1, npk0, npk1, pos0, pos1, end0, end1, st0, st1, mil, man;
};

// packets.py:67-79 for one symbol of packet type T (0 tag -> reader: start bit 1; 1 reader -> tag: start bit 0)
template <int T>
__device__ __forceinline__ void append_symbol(const Args &A, Lane &l, uint32_t sym, uint32_t m) {
    uint32_t &nsym = T ? l.nsym1 : l.nsym0, &npk = T ? l.npk1 : l.npk0, &pos = T ? l.pos1 : l.pos0, &end = T ? l.end1 : l.end0,
             &started = T ? l.st1 : l.st0;
    if (nsym < A.C.symbols) A.O.sym[T][(size_t)l.k * A.C.s_symbols + nsym] = (uint8_t)sym;
    nsym++;
    if (sym > 1u) {
        if (started) {
            if (pos > end) {   // packets.py:97 -- empty lists never reach the fsm
                if (npk < A.C.packets) A.O.close[T][(size_t)l.k * A.C.s_packets + npk] = make_uint2(pos, m);
                npk++;
                end = pos;
            }
            started = 0;
        }
    } else if (!started && sym == (T ? 0u : 1u)) {
        started = 1;
    } else {
        if (pos < A.C.bits) A.O.bits[T][(size_t)l.k * A.C.s_bits + pos] = (uint8_t)sym;
        const uint32_t open = pos - end;   // its place in the open packet, which is carried whatever the slab holds
        if (open < A.C.pending) A.S.pending[T][(size_t)l.k * A.C.s_pending + open] = (uint8_t)sym;
        else l.flags |= F_PENDING;
        pos++;
    }
}

// transition_sink.py:89-90,97 -> background.py:30-52 -> the routed decoder -> append_bit
__device__ __forceinline__ void emit(const Args &A, Lane &l, int v, int d, int t, uint32_t m) {
    const uint32_t code = edge_code(v, d, t, A.nd);
    if (l.ne < A.C.edges) {
        A.O.epos[(size_t)l.k * A.C.s_epos + l.ne] = m;
        A.O.ecode[(size_t)l.k * A.C.s_ecode + l.ne] = (uint16_t)code;
    }
    l.ne++;
    const uint32_t li = code & 0x3FFFu;
    if (t == 1 && A.reader) {
        const uint32_t e = A.mil_step[li * 16u + l.mil];
        l.mil = e & 15u;
        const uint32_t o = e >> 8, nout = o & 3u;
        if (nout >= 1u) append_symbol<1>(A, l, (o >> 2) & 7u, m);
        if (nout >= 2u) append_symbol<1>(A, l, (o >> 5) & 7u, m);
    } else if (t == 0 && A.tag) {
        const uint32_t e = A.man_step[li * 8u + l.man];
        l.man = e & 7u;
        const uint32_t o = e >> 8;
        if (o & 3u) append_symbol<0>(A, l, (o >> 2) & 7u, m);   // (the Manchester decoder gives at most one symbol per transition)
    }
}

template <int KIND>
__global__ __launch_bounds__(MB) void k_multi(Args A) {
    using Raw = typename RawOf<KIND>::T;
    const uint32_t g = blockIdx.x * MB + threadIdx.x;
    if (g >= A.K) return;
    Lane l;
    l.k = A.order[g];
    const uint32_t k = l.k, K = A.K;
    const uint32_t n = A.n[k];
    uint32_t *cnt = A.O.counts + (size_t)k * CNT_WORDS;
    l.flags = A.S.flags[k] & F_PENDING;
    if (n == 0) {   // untouched, and its outputs empty
        for (int i = 0; i < CNT_WORDS; i++) cnt[i] = i == CNT_FLAGS ? l.flags : 0u;
        return;
    }
    const size_t first = (size_t)A.first[k];
    const int L = A.L, mx = A.mx;
    const double Ld = (double)L;
    double ss = A.S.ss[k];
    uint32_t slot = A.S.slot[k];
    int filled = A.S.filled[k];
    int state, last_bit, dur;
    {
        const uint32_t e = A.S.edge[k];
        state = (int)(e & 3u);
        last_bit = (int)((e >> 2) & 3u) - 1;
        dur = (int)(e >> 4);
        const uint32_t d = A.S.dec[k];
        l.mil = d & 15u;
        l.man = (d >> 4) & 7u;
        l.st0 = (d >> 8) & 1u;
        l.st1 = (d >> 9) & 1u;
    }
    l.ne = l.nsym0 = l.nsym1 = l.npk0 = l.npk1 = l.end0 = l.end1 = 0;
    // the open packets' bits head the batch's bit arrays (what bit_off counts from)
    l.pos0 = A.S.npend[0][k];
    l.pos1 = A.S.npend[1][k];
    for (uint32_t i = 0; i < l.pos0 && i < A.C.pending && i < A.C.bits; i++)
        A.O.bits[0][(size_t)k * A.C.s_bits + i] = A.S.pending[0][(size_t)k * A.C.s_pending + i];
    for (uint32_t i = 0; i < l.pos1 && i < A.C.pending && i < A.C.bits; i++)
        A.O.bits[1][(size_t)k * A.C.s_bits + i] = A.S.pending[1][(size_t)k * A.C.s_pending + i];
    float *ring = A.S.ring + k;
    const bool ahead = L >= 2 * MU;   // (a shorter window could meet, inside one fetch, a slot the walk has just written)

    for (uint32_t m0 = 0; m0 < n; m0 += MU) {
        Raw raw[MU];
        float rp[MU];
        {
            const int rem = L - filled;   // samples the fill phase still takes
#pragma unroll
            for (int j = 0; j < MU; j++) {
                const uint32_t m = min(m0 + (uint32_t)j, n - 1u);
                raw[j] = load_raw<KIND>(A.in, first + m);
                uint32_t s = slot + (uint32_t)max(j - rem, 0);
                if (s >= (uint32_t)L) s -= (uint32_t)L;
                rp[j] = ahead ? ring[(size_t)s * K] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < MU; j++) {
            const uint32_t m = m0 + (uint32_t)j;
            if (m >= n) break;
            const float xf = env_of<KIND>(raw[j], A.scale);
            if (filled < L) {   // transition_sink.py:109-125
                ring[(size_t)filled * K] = xf;
                filled++;
                if (filled == L) {
                    double s = 0;
                    for (int i = 0; i < L; i++) s += (double)ring[(size_t)i * K];   // :122, in the reference's order
                    ss = s;
                    state = 0;
                    last_bit = 0;
                    dur = L % mx;   // :123
                }
                continue;
            }
            const double bit = (double)xf;
            const float pf = ahead ? rp[j] : ring[(size_t)slot * K];
            const double prev = (double)pf;
            // :59-77 -- the ratio against lo / hi; the division only where the products cannot decide (threshold.hip.h: classify_one)
            bool low = false, high = false, amb = true;
            const double p = bit * Ld;
            if (A.bands_ok && ss > 1e-150 && ss < 1e150) {
                amb = false;
                if (p < A.lo_a * ss) low = true;
                else if (p > A.lo_b * ss) low = false;
                else amb = true;
                if (p > A.hi_b * ss) high = true;
                else if (p < A.hi_a * ss) high = false;
                else amb = true;
            }
            if (amb) {
                double ratio;
                if (ss == 0) ratio = (bit == 0) ? 1.0 : A.hi_plus;
                else ratio = p / ss;
                low = A.lo > ratio;
                high = ratio > A.hi;
            }
            const int prev_state = state;
            int val;
            double cur = prev;
            if (low) { val = -1; state = 2; }
            else if (state != 2 && high) { val = 1; state = 1; }
            else { val = 0; cur = bit; ring[(size_t)slot * K] = xf; }
            ss += cur - prev;   // :82
            slot++;
            if (slot == (uint32_t)L) slot = 0;
            bool ev = false, timed_out = false;
            int d = mx;
            if (val == last_bit) {   // :84-85, 95-99
                dur++;
                if (dur > mx) ev = timed_out = true;
            } else {                 // :86-92
                ev = true;
                d = prev_state == 0 ? mx : dur;
            }
            if (ev) {
                emit(A, l, state == 2 ? last_bit + 1 : last_bit, d, state - 1, m);
                dur = 1;
                if (timed_out) state = 0;
                else last_bit = val;
            }
        }
    }

    A.S.ss[k] = ss;
    A.S.slot[k] = slot;
    A.S.filled[k] = filled;
    A.S.edge[k] = pack_edge(state, last_bit, dur);
    A.S.dec[k] = pack_dec((int)l.mil, (int)l.man, (int)l.st0, (int)l.st1);
    A.S.npend[0][k] = l.pos0 - l.end0;
    A.S.npend[1][k] = l.pos1 - l.end1;
    A.S.flags[k] = l.flags & F_PENDING;
    if (l.ne > A.C.edges) l.flags |= F_EDGES;
    if (l.nsym0 > A.C.symbols || l.nsym1 > A.C.symbols) l.flags |= F_SYMBOLS;
    if (l.npk0 > A.C.packets || l.npk1 > A.C.packets) l.flags |= F_PACKETS;
    if (l.pos0 > A.C.bits || l.pos1 > A.C.bits) l.flags |= F_BITS;
    cnt[CNT_EDGES] = l.ne;
    cnt[CNT_SYM0] = l.nsym0;
    cnt[CNT_SYM1] = l.nsym1;
    cnt[CNT_PK0] = l.npk0;
    cnt[CNT_PK1] = l.npk1;
    cnt[CNT_BITS0] = l.pos0;
    cnt[CNT_BITS1] = l.pos1;
    cnt[CNT_FLAGS] = l.flags;
    cnt[CNT_PKBITS0] = l.end0;
    cnt[CNT_PKBITS1] = l.end1;
    cnt[10] = cnt[11] = 0u;
}

// ---- state in and out of the [field][stream] arrays: one stream's as a contiguous block (nfc_multi_get_state / _set_state) ----
struct IoHeader {
    double ss;
    uint32_t slot;
    int32_t filled;
    uint32_t edge, dec, npend[2], flags, pad;
};
// blob: IoHeader | ring (L floats) | pending bits of type 0 (cap_pending) | of type 1
__global__ __launch_bounds__(256) void k_multi_state_io(State S, Caps C, uint32_t K, uint32_t k, int L, int set, uint8_t *blob) {
    IoHeader *h = (IoHeader *)blob;
    float *r = (float *)(blob + sizeof(IoHeader));
    uint8_t *p0 = (uint8_t *)(r + L), *p1 = p0 + C.pending;
    const int tid = threadIdx.x;
    if (set) {
        if (tid == 0) {
            S.ss[k] = h->ss;
            S.slot[k] = h->slot;
            S.filled[k] = h->filled;
            S.edge[k] = h->edge;
            S.dec[k] = h->dec;
            S.npend[0][k] = h->npend[0];
            S.npend[1][k] = h->npend[1];
            S.flags[k] = h->flags;
        }
        for (int i = tid; i < L; i += 256) S.ring[(size_t)i * K + k] = r[i];
        for (uint32_t i = tid; i < C.pending; i += 256) {
            S.pending[0][(size_t)k * C.s_pending + i] = p0[i];
            S.pending[1][(size_t)k * C.s_pending + i] = p1[i];
        }
    } else {
        if (tid == 0) {
            h->ss = S.ss[k];
            h->slot = S.slot[k];
            h->filled = S.filled[k];
            h->edge = S.edge[k];
            h->dec = S.dec[k];
            h->npend[0] = S.npend[0][k];
            h->npend[1] = S.npend[1][k];
            h->flags = S.flags[k];
            h->pad = 0;
        }
        for (int i = tid; i < L; i += 256) r[i] = S.ring[(size_t)i * K + k];
        for (uint32_t i = tid; i < C.pending; i += 256) {
            p0[i] = S.pending[0][(size_t)k * C.s_pending + i];
            p1[i] = S.pending[1][(size_t)k * C.s_pending + i];
        }
    }
}

// streams [k0, k1) back to the state of a fresh context: idle machines, an empty (zeroed) window, no open packet, no flag
__global__ __launch_bounds__(256) void k_multi_reset(State S, uint32_t K, uint32_t k0, uint32_t k1, int L, uint32_t *counts) {
    const uint32_t w = k1 - k0;
    const size_t total = (size_t)w * (size_t)L, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) S.ring[(i / w) * K + k0 + (uint32_t)(i % w)] = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < w; i += stride) {
        const uint32_t k = k0 + (uint32_t)i;
        S.ss[k] = 0.0;
        S.slot[k] = 0u;
        S.filled[k] = 0;
        S.edge[k] = EDGE_INIT;
        S.dec[k] = DEC_INIT;
        S.npend[0][k] = S.npend[1][k] = 0u;
        S.flags[k] = 0u;
        for (int j = 0; j < CNT_WORDS; j++) counts[(size_t)k * CNT_WORDS + j] = 0u;
    }
}

}  // namespace multi
}  // namespace nfc
