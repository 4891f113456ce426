// answers_tx.hip.h -- what the streams of a multi-stream context answer, as TX samples: stated ONCE for the host twin and the kernels
// (include/nfc_amd.h: nfc_answers_tx_config, nfc_host_answers_tx, nfc_multi_transmit_device).
//
// RUNS.  An answer's runs are the lists tx_encode_manchester (a tag card) / tx_encode_miller (a reader card) give for its bits, and those
// are the air interface's pieces (air.hip.h: miller_piece, manchester_piece -- every merged run belongs to the piece it starts in, a
// piece starts two runs, their durations come from a set of nine, summed in the encoder's order).  Only the COUNT of a run differs:
// here a run of d us has (uint64)(d * (samp_rate / 1e6)) samples, binary_src.work's rule as nfc_tx_sample_count states it, so the nine
// counts are computed once on the host by that expression (make_consts) and both sides index the one table through air::piece_of.
//
// SCHEDULE (schedule_stream, the one text of the twin's loop and of k_answers_tx_schedule's lanes).  Per stream: the pending entry carried
// in, then the push's answers; entry j starts at S_j = T(idx_j) + delay, is cut where the next answered command closed, and what it owns
// of the push's TX span becomes one record of the stream's compact SPAN TABLE -- 64 bytes, the answer's bits inside, so that the render
// pass reads nothing else.  The last entry stays pending when it reaches beyond the span's end.
//
// RENDER (k_answers_tx_render).  Flat tiles of 1024 samples over the packed output, 256 threads, four complex samples per thread as one
// contiguous 32-byte piece (k_tx_render's store shape, plain stores).  A workgroup finds the first stream its tile meets in a host-made
// tile table, walks the streams the tile meets, and bisects each stream's span table for the spans that meet the tile.  None: the tile
// is idle fill (and padding), nothing is staged.  Otherwise the workgroup makes the answer's run ends in LDS from its bits -- a piece
// per lane, a block scan of the pieces' sample counts -- and every thread bisects for its run.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/nfc_amd.h"
#define NFC_AIR_PIECES_ONLY
#include "air.hip.h"
#include "tx_sample.hip.h"

namespace nfc {
namespace atx {

constexpr uint32_t MAX_BITS = 162;                    // 18 bytes, the longest answer (READT)
constexpr uint32_t MAX_PIECES = MAX_BITS + 2, MAX_RUNS = 2 * MAX_PIECES;
constexpr uint32_t ANS_BYTES = 18;
constexpr uint32_t MAX_SPAN = 1u << 30;               // samples of one stream's TX span
constexpr uint32_t MAX_RATIO = 65536;
constexpr double MAX_SAMP_RATE = 1e9;                 // an answer then stays below 2^23 samples
constexpr int BLOCK = 256, PER_THREAD = 4, TILE = BLOCK * PER_THREAD;
constexpr int SCHED_BLOCK = 64;

static_assert(sizeof(nfc_answers_tx_config) == 64 && sizeof(nfc_tx_pending) == 64 && sizeof(nfc_tx_answer) == 16, "the header's structures");

struct Consts {
    air::Consts pieces;        // cnt alone is used: the nine counts by nfc_tx_sample_count's rule
    uint64_t first_index, phase_inc, delay;
    uint32_t rate_num, rate_den;
    float amp;
    int32_t carrier;
    uint32_t align;
};

// every field of the configuration; null: fine, else the message
inline const char *config_fault(const nfc_answers_tx_config *c, char *msg, size_t cap) {
    if (!c) return snprintf(msg, cap, "cfg is null"), msg;
    if (!(c->samp_rate > 0) || !(c->samp_rate <= MAX_SAMP_RATE)) return snprintf(msg, cap, "cfg.samp_rate must be above 0 and at most %g", MAX_SAMP_RATE), msg;
    if (c->rate_num < 1 || c->rate_num > MAX_RATIO) return snprintf(msg, cap, "cfg.rate_num %u is outside 1 .. %u", c->rate_num, MAX_RATIO), msg;
    if (c->rate_den < 1 || c->rate_den > MAX_RATIO) return snprintf(msg, cap, "cfg.rate_den %u is outside 1 .. %u", c->rate_den, MAX_RATIO), msg;
    if (c->align_samples == 0 || (c->align_samples & (c->align_samples - 1)) || c->align_samples > (1u << 20))
        return snprintf(msg, cap, "cfg.align_samples %u is no power of two up to 2^20", c->align_samples), msg;
    if (!isfinite(c->freq) || !isfinite(c->amp)) return snprintf(msg, cap, "cfg.freq and cfg.amp must be finite"), msg;
    if (c->delay_samples > (1ull << 40)) return snprintf(msg, cap, "cfg.delay_samples exceeds 2^40"), msg;
    for (int i = 0; i < 3; i++)
        if (c->reserved[i]) return snprintf(msg, cap, "cfg.reserved must be 0"), msg;
    return nullptr;
}

inline Consts make_consts(const nfc_answers_tx_config &c) {
    Consts C;
    memset(&C, 0, sizeof C);
    using namespace air;
    const double dur[N_COUNTS] = {T_ZERO, T_ZERO_REM, T_HALF + T_ZERO_REM, T_ONE_REM, T_HALF + T_ONE_REM, T_FULL + T_ONE_REM,
                                  T_HALF + (T_FULL + T_ONE_REM), T_HALF, T_FULL};   // (the encoder's sums, in its order: cur + back)
    const double mult = c.samp_rate / 1e6;   // binary_src.py:38
    for (int i = 0; i < N_COUNTS; i++) C.pieces.cnt[i] = (uint32_t)(uint64_t)(dur[i] * mult);   // binary_src.py:83: int(dur * mult)
    const double turns = c.freq / c.samp_rate, fr = turns - floor(turns);
    C.phase_inc = (uint64_t)(fr * 18446744073709551616.0);   // floor(frac(f / fs) * 2^64), as nfc_tx_render_device
    C.first_index = c.first_index, C.delay = c.delay_samples;
    C.rate_num = c.rate_num, C.rate_den = c.rate_den;
    C.amp = c.amp, C.carrier = c.carrier ? 1 : 0, C.align = c.align_samples;
    return C;
}

__host__ __device__ __forceinline__ bool n_bits_ok(uint32_t n) { return n >= 1 && n <= MAX_BITS && (n <= 8 || n % 9 == 0); }
// T(r) = floor(r * num / den)
__host__ __device__ __forceinline__ uint64_t tx_index(const Consts &C, uint64_t r) {
    return C.rate_num == C.rate_den ? r : r * C.rate_num / C.rate_den;
}

// one record of a stream's span table: what an answer owns of the push's TX span, relative to the span's first TX index
struct Span {
    int64_t s_rel;             // the answer's first sample (may lie before the span)
    uint32_t lo, hi;           // [lo, hi) of the span is the answer's
    uint16_t n_bits;
    uint8_t role, pad0;
    uint32_t pad1;
    uint8_t air[ANS_BYTES], par[ANS_BYTES];
    uint8_t pad2[4];
};
static_assert(sizeof(Span) == 64, "a span record is 64 bytes");

// what the host knows of a stream when it enqueues: entry K closes the layout (first_sample: the samples in all)
struct StreamIn {
    uint64_t rx_base, t0, first_sample;
    uint32_t rx_n, n_samples;
    uint32_t span_off, span_cap;
    int32_t role;              // -1: no card
    uint32_t pad;
};
static_assert(sizeof(StreamIn) == 48, "a stream record is 48 bytes");

struct Entry {
    uint64_t start;
    const uint8_t *air, *par;
    uint32_t n_bits, role;
};
__host__ __device__ inline uint32_t entry_samples(const Consts &C, const Entry &e) {
    return air::frame_samples(C.pieces, e.role, air::Bits{e.air, e.par, e.n_bits});
}

// One stream, one push.  src: idx(j) the r of answer j's command, n_bits(j) (0: an answer outside the domain, which owns nothing),
// air(j) / par(j) its bytes.  Writes at most `cap` spans, advances *pend, returns the spans written.
template <class Src>
__host__ __device__ inline uint32_t schedule_stream(const Consts &C, uint32_t role, uint64_t t0, uint32_t n, nfc_tx_pending *pend, uint32_t n_ans,
                                                    const Src &src, Span *out, uint32_t cap) {
    const uint64_t t1 = t0 + n;
    uint32_t ns = 0;
    Entry cur = {pend->start, pend->air, pend->par, pend->n_bits, pend->role};
    auto emit = [&](const Entry &e, uint64_t cut) {
        const uint64_t top = cut < t1 ? cut : t1;
        if (!e.n_bits || e.start >= top) return;
        const uint64_t end = e.start + entry_samples(C, e);
        const uint64_t a = e.start > t0 ? e.start : t0, b = end < top ? end : top;
        if (a >= b || ns >= cap) return;
        Span *s = out + ns++;
        s->s_rel = (int64_t)(e.start - t0);
        s->lo = (uint32_t)(a - t0), s->hi = (uint32_t)(b - t0);
        s->n_bits = (uint16_t)e.n_bits, s->role = (uint8_t)e.role, s->pad0 = 0, s->pad1 = 0;
        const uint32_t nb = air::frame_bytes(e.n_bits);
        for (uint32_t i = 0; i < ANS_BYTES; i++) s->air[i] = i < nb ? e.air[i] : 0, s->par[i] = i < nb ? e.par[i] : 0;
        for (int i = 0; i < 4; i++) s->pad2[i] = 0;
    };
    for (uint32_t j = 0; j < n_ans; j++) {
        const uint64_t tj = tx_index(C, src.idx(j));
        emit(cur, tj);
        cur = Entry{tj + C.delay, src.air(j), src.par(j), src.n_bits(j), role};
    }
    emit(cur, ~0ull);
    const bool keep = cur.n_bits && cur.start + entry_samples(C, cur) > t1;
    if (keep && cur.air == pend->air) return ns;   // the entry carried in is carried on
    uint8_t a[ANS_BYTES], p[ANS_BYTES];
    const uint32_t nb = keep ? air::frame_bytes(cur.n_bits) : 0u;
#pragma unroll
    for (uint32_t i = 0; i < ANS_BYTES; i++) a[i] = i < nb ? cur.air[i] : 0, p[i] = i < nb ? cur.par[i] : 0;
    pend->start = keep ? cur.start : 0ull;
    pend->n_bits = keep ? (uint16_t)cur.n_bits : 0, pend->role = keep ? (uint8_t)cur.role : 0, pend->reserved0 = 0, pend->reserved1 = 0;
#pragma unroll
    for (uint32_t i = 0; i < ANS_BYTES; i++) pend->air[i] = a[i], pend->par[i] = p[i];
#pragma unroll
    for (int i = 0; i < 12; i++) pend->reserved2[i] = 0;
    return ns;
}

// the level of position p of an answer whose run ends (end << 1 | level) are `ends`
__host__ __device__ __forceinline__ uint32_t find_run(const uint32_t *ends, uint32_t n, uint32_t p) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((ends[mid] >> 1) > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

#if defined(__HIPCC__) && defined(NFC_ANSWERS_TX_KERNELS)
// ---- the kernels -------------------------------------------------------------------------------------------------------------------
// the answers of the last tracked push, where multi_commands.hip.h's kernels left them in the tracking buffer; every range is cut to what
// the HOST laid out
struct Tracked {
    const uint8_t *buf;            // null: the push stored nothing, or ran without a card: no stream has an answer
    const uint64_t *table;         // [4][K + 1]: frame_off[0], frame_off[1], byte_off[0], byte_off[1]
    uint64_t at_fr[2], total_frames[2];
    uint64_t at_cmd_off, at_src, at_ans_n, at_ans, at_air, at_par, total_cmds;
};
struct DevSrc {
    const nfc_emu_answer *ans;
    const uint32_t *src;
    const nfc_raw_frame *rec0, *rec1;
    const uint8_t *a, *p;
    uint32_t ncmd, nfr0, nfr1;
    uint64_t rx_base;
    __device__ __forceinline__ uint64_t idx(uint32_t j) const {
        const uint32_t s = ans[j].src;
        if (s >= ncmd) return rx_base;   // (never: an answer's command is one of the stream's)
        const uint32_t w = src[s], t = w >> 31, i = w & 0x7FFFFFFFu;
        if (i >= (t ? nfr1 : nfr0)) return rx_base;   // (never)
        return rx_base + (t ? rec1 : rec0)[i].idx;   // (the records' idx is batch-local: the host adds the base when it fetches)
    }
    __device__ __forceinline__ uint32_t n_bits(uint32_t j) const {
        const uint32_t n = ans[j].n_bits;
        return n_bits_ok(n) ? n : 0u;
    }
    __device__ __forceinline__ const uint8_t *air(uint32_t j) const { return a + (size_t)j * ANS_BYTES; }
    __device__ __forceinline__ const uint8_t *par(uint32_t j) const { return p + (size_t)j * ANS_BYTES; }
};
struct ScheduleArgs {
    Consts C;
    Tracked T;
    const StreamIn *streams;       // [K + 1]
    Span *spans;
    uint32_t *n_spans;             // [K]
    nfc_tx_pending *pending;       // [K]
    uint32_t K;
    uint8_t *packed;               // the call's buffer and where its sections' guards start
    uint64_t guard_at[4];
    uint32_t guard_word, guard_bytes;
};

// A lane per stream: a stream has a few dozen answers at the most.
__global__ __launch_bounds__(SCHED_BLOCK) void k_answers_tx_schedule(ScheduleArgs A) {
    if (blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < 4u * A.guard_bytes; i += SCHED_BLOCK) {
            const uint32_t s = i / A.guard_bytes, b = i % A.guard_bytes;
            A.packed[A.guard_at[s] + b] = (uint8_t)(A.guard_word >> (8 * (b & 3u)));
        }
    const uint32_t K = A.K, k = blockIdx.x * SCHED_BLOCK + threadIdx.x;
    if (k >= K) return;
    const StreamIn S = A.streams[k];
    if (S.role < 0) {   // no card: no samples, and the pending entry is left alone
        A.n_spans[k] = 0;
        return;
    }
    DevSrc src = {};
    uint32_t na = 0;
    const Tracked &T = A.T;
    if (T.buf) {
        const size_t TK = (size_t)K + 1;
        const uint64_t *cmd_off = (const uint64_t *)(T.buf + T.at_cmd_off);
        uint64_t c1 = cmd_off[k + 1], c0 = cmd_off[k];
        c1 = c1 < T.total_cmds ? c1 : T.total_cmds;
        c0 = c0 < c1 ? c0 : c1;
        src.ncmd = (uint32_t)(c1 - c0);
        na = ((const uint32_t *)(T.buf + T.at_ans_n))[k];
        na = na < src.ncmd ? na : src.ncmd;
        src.ans = (const nfc_emu_answer *)(T.buf + T.at_ans) + c0;
        src.src = (const uint32_t *)(T.buf + T.at_src) + c0;
        src.a = T.buf + T.at_air + c0 * ANS_BYTES, src.p = T.buf + T.at_par + c0 * ANS_BYTES;
        src.rx_base = S.rx_base;
#define NFC_TX_PART(t, nfr, rec)                                                       \
    {                                                                                  \
        uint64_t fe = T.table[(size_t)t * TK + k + 1], fb = T.table[(size_t)t * TK + k]; \
        fe = fe < T.total_frames[t] ? fe : T.total_frames[t];                          \
        fb = fb < fe ? fb : fe;                                                        \
        nfr = (uint32_t)(fe - fb);                                                     \
        rec = (const nfc_raw_frame *)(T.buf + T.at_fr[t]) + fb;                        \
    }
        NFC_TX_PART(0, src.nfr0, src.rec0)
        NFC_TX_PART(1, src.nfr1, src.rec1)
#undef NFC_TX_PART
    }
    A.n_spans[k] = schedule_stream(A.C, (uint32_t)S.role, S.t0, S.n_samples, A.pending + k, na, src, A.spans + S.span_off, S.span_cap);
}

struct RenderArgs {
    Consts C;
    const StreamIn *streams;       // [K + 1]
    const uint32_t *tile_stream;   // per tile: the first stream whose part of the buffer, padding included, reaches into the tile
    const Span *spans;
    const uint32_t *n_spans;
    uint32_t K;
    uint64_t total;                // samples of the layout
    float2 *out;
};

__global__ __launch_bounds__(BLOCK) void k_answers_tx_render(RenderArgs A) {
    __shared__ uint32_t s_end[MAX_RUNS];
    __shared__ uint32_t s_scan[BLOCK / 64];
    __shared__ uint8_t s_air[ANS_BYTES + 2], s_par[ANS_BYTES + 2];
    const uint64_t tile0 = (uint64_t)blockIdx.x * TILE, tile1 = min(A.total, tile0 + (uint64_t)TILE);
    const uint64_t s0 = tile0 + (uint64_t)threadIdx.x * PER_THREAD;
    float lv[PER_THREAD];
    uint64_t t[PER_THREAD];
    uint32_t inside = 0;   // bit i: sample i lies in a stream (else it is padding, or past the layout)
#pragma unroll
    for (int i = 0; i < PER_THREAD; i++) lv[i] = 0.f, t[i] = 0;
    // (everything that steers the two loops is the same for the whole workgroup: the barriers inside are reached by all)
    for (uint32_t k = A.tile_stream[blockIdx.x]; k < A.K; k++) {
        const StreamIn S = A.streams[k];
        if (S.first_sample >= tile1) break;
        if (S.n_samples == 0) continue;
        const uint64_t f0 = S.first_sample, f1 = f0 + S.n_samples;
        if (f1 <= tile0) continue;
        const float idle = S.role == NFC_EMU_READER ? 1.f : 0.f;
#pragma unroll
        for (int i = 0; i < PER_THREAD; i++) {
            const uint64_t g = s0 + i;
            if (g >= f0 && g < f1) inside |= 1u << i, lv[i] = idle, t[i] = S.t0 + (g - f0);
        }
        const uint32_t r_lo = (uint32_t)((tile0 > f0 ? tile0 : f0) - f0), r_hi = (uint32_t)((tile1 < f1 ? tile1 : f1) - f0);
        const Span *sp = A.spans + S.span_off;
        const uint32_t ns = min(A.n_spans[k], S.span_cap);
        uint32_t lo = 0, hi = ns;   // the first span that ends behind the tile's first sample of the stream
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sp[mid].hi > r_lo) hi = mid;
            else lo = mid + 1;
        }
        for (uint32_t j = lo; j < ns && sp[j].lo < r_hi; j++) {
            const uint32_t a_lo = sp[j].lo, a_hi = sp[j].hi, n_bits = min((uint32_t)sp[j].n_bits, MAX_BITS), type = sp[j].role & 1u;
            const int64_t s_rel = sp[j].s_rel;
            if (n_bits == 0) continue;   // (never: a span has an answer)
            __syncthreads();   // (the answer before is read)
            if (threadIdx.x < ANS_BYTES) s_air[threadIdx.x] = sp[j].air[threadIdx.x], s_par[threadIdx.x] = sp[j].par[threadIdx.x];
            __syncthreads();
            const air::Bits B = {s_air, s_par, n_bits};
            const uint32_t np = air::n_pieces(type, n_bits);   // at most MAX_PIECES: one trip
            air::Piece P = {0u, 0u, 0u, 0u};
            if (threadIdx.x < np) P = air::piece_of(A.C.pieces, type, B, threadIdx.x);
            uint32_t total;
            const uint32_t at = block_exclusive<AddU32, BLOCK / 64>(P.ca + P.cb, s_scan, total);
            if (threadIdx.x < np) {
                s_end[2 * threadIdx.x] = ((at + P.ca) << 1) | P.la;
                s_end[2 * threadIdx.x + 1] = ((at + P.ca + P.cb) << 1) | P.lb;
            }
            __syncthreads();
            const uint32_t n_runs = 2 * np;
            uint32_t run = 0, end = 0, level = 0;
            bool found = false;
#pragma unroll
            for (int i = 0; i < PER_THREAD; i++) {
                const uint64_t g = s0 + i;
                if (g < f0 || g >= f1) continue;
                const uint32_t rel = (uint32_t)(g - f0);
                if (rel < a_lo || rel >= a_hi) continue;
                const uint32_t p = (uint32_t)((int64_t)rel - s_rel);
                if (!found) {
                    run = find_run(s_end, n_runs, p);
                    run = run < n_runs ? run : n_runs - 1u;
                    end = s_end[run] >> 1, level = s_end[run] & 1u;
                    found = true;
                }
                while (p >= end && run + 1u < n_runs) {   // (runs of no samples are stepped over)
                    run++;
                    end = s_end[run] >> 1, level = s_end[run] & 1u;
                }
                lv[i] = (float)level;
            }
        }
    }
    if (s0 >= tile1) return;
    float2 v[PER_THREAD];
#pragma unroll
    for (int i = 0; i < PER_THREAD; i++)
        v[i] = (inside >> i) & 1u ? tx_sample(A.C.first_index + t[i], A.C.phase_inc, A.C.amp, A.C.carrier, lv[i]) : make_float2(0.f, 0.f);
    if (s0 + PER_THREAD <= tile1) {
        float4 *o = (float4 *)(A.out + s0);   // 32-byte aligned: s0 is a multiple of PER_THREAD samples
#pragma unroll
        for (int i = 0; i < PER_THREAD / 2; i++) o[i] = make_float4(v[2 * i].x, v[2 * i].y, v[2 * i + 1].x, v[2 * i + 1].y);
    } else {
#pragma unroll
        for (int i = 0; i < PER_THREAD; i++)
            if (s0 + i < tile1) A.out[s0 + i] = v[i];
    }
}
#endif   // __HIPCC__ && NFC_ANSWERS_TX_KERNELS

}  // namespace atx
}  // namespace nfc
