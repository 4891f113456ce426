// air.hip.h -- what an eavesdropper's radio records of a transaction, stated ONCE for the host twin and the kernels (DESIGN.md 8l;
// include/nfc_amd.h: nfc_air_*).  K ragged lists of on-air frames become K IQ captures in one device buffer, in any of the four IQ
// input kinds, laid out for nfc_multi_push_device.  synth.py (modulation_profile, iq_from_profile with sigma 0, quantise_*) is the
// yardstick: with sigma 0 the bytes are its bytes.
//
// RUNS.  A reader frame is synth.miller_pulses(bits), a tag frame synth.manchester_pulses(bits): the lists tx_encode_miller /
// tx_encode_manchester give (tests/test_air_host.py asserts the equality).  Here a frame is a row of PIECES -- reader: the start of
// frame, the bits, the end zero; tag: the start bit, the bits -- and every merged run belongs to the piece it STARTS in.  Every piece
// of a reader frame ends high, so a `one` and a zero after a one always merge backwards and start nothing of their own high half;
// what a piece starts is a pause and a high run whose merged duration is decided by the next two bits, or nothing.  A tag piece starts
// its first half unless that merged backwards, and its second half, merged with the next bit's first or not.  So a piece starts two
// runs (either may have no samples), their durations come from a set of nine, and a run of d us has int(d * rate_msps) samples
// (synth.pulses_to_levels): the nine counts are computed once on the host, in double, with the merged durations added in the order
// miller_pulses adds them, and both sides index that one table (Consts::cnt).  A piece's sample count is local: the layout kernel sums
// pieces, the render kernel scans them.
//
// VALUES.  m is 1 (idle), the level (reader), fl(1 + fl(depth) * level) (tag): three values, so carrier * m has three values per
// component, and those six products are computed once on the host (make_consts) and handed to both sides.  What is left per sample
// is ONE float addition, base + noise: there is nothing a compiler could contract into an fma, on either side (and the build passes
// -ffp-contract=off).  The quantised kinds round x * full_scale (cu8: 127.5 + x * full_scale) in double with rint, one product and
// one sum, never fused for the same reason: -ffp-contract=off, on both sides.
//
// NOISE.  Counter-based, all-integer up to the last step: SplitMix64 in counter form.  A stream's key is
// mix64(mix64(seed + G) + G * (stream_seed + 1)), component c of sample i of the stream hashes to h = mix64(key + G * (2 i + c + 1))
// (G the golden-ratio increment, mix64 SplitMix64's finaliser: exactly that generator's output number 2 i + c + 1 from state `key`),
// u0 .. u3 are h's four 16-bit fields, n = fl((float)(u0 + u1 + u2 + u3 - 131070) * unit).  The integer is below 2^18, so the
// conversion is exact and the product the only rounding.  Nothing else enters: not K, not the stream's place, not the tiling.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"
#include "scan.hip.h"

namespace nfc {
namespace air {

// utilities.PulseLength, with synth.py's own expressions
constexpr double T_FULL = 9.44, T_ZERO = 3.00;
constexpr double T_HALF = T_FULL / 2, T_ZERO_REM = T_FULL - T_ZERO, T_ONE_REM = T_HALF - T_ZERO;

constexpr uint32_t MAX_BITS = 9 * 256;          // a frame of 256 bytes, the longest of ISO 14443-3
constexpr uint32_t MAX_PIECES = MAX_BITS + 2;
constexpr double MAX_RATE_MSPS = 1000.0;        // a frame then stays below 2^25 samples: run ends fit 31 bits beside their level
constexpr uint32_t MAX_STREAM_SAMPLES = 1u << 30;   // what one nfc_multi_push_device takes of a stream
constexpr int BLOCK = 256;
constexpr int START_BLOCK = 1024;

enum : int { N_PAUSE, N_ZERO_REM, N_ZERO_REM_HALF, N_ONE_REM, N_ONE_REM_HALF, N_ONE_REM_FULL, N_ONE_REM_FULL_HALF, N_HALF, N_FULL, N_COUNTS };
enum : uint32_t { M_ZERO = 0, M_ONE = 1, M_LOADED = 2 };   // the three multipliers: a pause, the carrier, a loaded half bit

struct Consts {
    double full_scale;
    uint64_t seed;
    uint32_t cnt[N_COUNTS];
    float base_i[3], base_q[3];   // fl(carrier * m) for M_ZERO, M_ONE, M_LOADED
    float unit;
    uint32_t noisy, kind, tail, align;
};

inline Consts make_consts(const nfc_air_config &c) {
    Consts C = {};
    const double dur[N_COUNTS] = {T_ZERO, T_ZERO_REM, T_HALF + T_ZERO_REM, T_ONE_REM, T_HALF + T_ONE_REM, T_FULL + T_ONE_REM,
                                  T_HALF + (T_FULL + T_ONE_REM), T_HALF, T_FULL};
    for (int i = 0; i < N_COUNTS; i++) C.cnt[i] = (uint32_t)(int64_t)(dur[i] * c.rate_msps);   // int(): towards zero
    const float m[3] = {0.f, 1.f, 1.f + c.depth * 1.f};
    for (int i = 0; i < 3; i++) C.base_i[i] = c.carrier_i * m[i], C.base_q[i] = c.carrier_q * m[i];
    C.unit = (float)((double)c.sigma / sqrt((65536.0 * 65536.0 - 1.0) / 3.0));
    C.noisy = c.sigma != 0.f;
    C.full_scale = (double)c.full_scale;
    C.seed = c.seed, C.kind = c.out_kind, C.tail = c.tail, C.align = c.align_samples;
    return C;
}

// ---- a frame's bits: bytes and ninth bits in nfc_raw_frame's form; 1 .. 8 bits: a short frame from its first byte ----
struct Bits {
    const uint8_t *air, *par;
    uint32_t n;
    __host__ __device__ __forceinline__ uint32_t at(uint32_t j) const {
        if (n <= 8) return (air[0] >> j) & 1u;
        const uint32_t b = j / 9u, k = j - 9u * b;
        return k < 8u ? (air[b] >> k) & 1u : par[b] & 1u;
    }
};
__host__ __device__ __forceinline__ uint32_t frame_bytes(uint32_t n_bits) { return n_bits == 0 ? 0u : n_bits <= 8 ? 1u : n_bits / 9u; }
__host__ __device__ __forceinline__ uint32_t n_pieces(uint32_t type, uint32_t n_bits) { return n_bits == 0 ? 0u : type ? n_bits + 2u : n_bits + 1u; }

struct Piece {
    uint32_t ca, cb;   // samples of the two runs the piece starts
    uint32_t la, lb;   // their levels
};
// reader: piece 0 the start of frame, 1 .. n the bits, n + 1 the end zero (miller_pulses: both are zeros after a zero / after the last bit)
__host__ __device__ __forceinline__ Piece miller_piece(const Consts &C, const Bits &B, uint32_t j) {
    auto bit = [&](uint32_t p) -> uint32_t { return (p >= 1 && p <= B.n) ? B.at(p - 1) : 0u; };
    const uint32_t x = bit(j), prev = j ? bit(j - 1) : 0u;
    Piece P = {0u, 0u, 0u, 1u};
    if (x) {   // HALF went to the run before; the pause, then ONE_REM and what the next pieces add to it
        P.ca = C.cnt[N_PAUSE];
        P.cb = bit(j + 1) ? C.cnt[N_ONE_REM_HALF] : bit(j + 2) ? C.cnt[N_ONE_REM_FULL_HALF] : C.cnt[N_ONE_REM_FULL];
    } else if (!prev) {   // a zero after a zero
        P.ca = C.cnt[N_PAUSE];
        P.cb = bit(j + 1) ? C.cnt[N_ZERO_REM_HALF] : C.cnt[N_ZERO_REM];
    }   // (a zero after a one is a whole bit high: it went to the run before)
    return P;
}
// tag: piece 0 the start bit (a one), 1 .. n the bits; halves x, 1 - x
__host__ __device__ __forceinline__ Piece manchester_piece(const Consts &C, const Bits &B, uint32_t j) {
    const uint32_t x = j ? B.at(j - 1) : 1u;
    const uint32_t prev = j == 0 ? x : j == 1 ? 1u : B.at(j - 2);
    const uint32_t next = j < B.n ? B.at(j) : x;
    Piece P;
    P.la = x, P.lb = 1u - x;
    P.ca = (j && prev != x) ? 0u : C.cnt[N_HALF];            // merged backwards: the run before is a whole bit long
    P.cb = (j < B.n && next != x) ? C.cnt[N_FULL] : C.cnt[N_HALF];
    return P;
}
__host__ __device__ __forceinline__ Piece piece_of(const Consts &C, uint32_t type, const Bits &B, uint32_t j) {
    return type ? miller_piece(C, B, j) : manchester_piece(C, B, j);
}
__host__ __device__ inline uint32_t frame_samples(const Consts &C, uint32_t type, const Bits &B) {
    uint32_t n = 0;
    const uint32_t np = n_pieces(type, B.n);
    for (uint32_t j = 0; j < np; j++) {
        const Piece P = piece_of(C, type, B, j);
        n += P.ca + P.cb;
    }
    return n;
}

// ---- noise ----
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {   // SplitMix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t stream_key(uint64_t seed, uint64_t stream_seed) {
    return mix64(mix64(seed + GOLDEN) + GOLDEN * (stream_seed + 1ull));
}
__host__ __device__ __forceinline__ float noise(uint64_t key, uint32_t index, uint32_t component, float unit) {
    const uint64_t h = mix64(key + GOLDEN * (2ull * index + component + 1ull));
    const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
    const int32_t s = (int32_t)((lo & 0xFFFFu) + (lo >> 16) + (hi & 0xFFFFu) + (hi >> 16)) - 131070;
    return (float)s * unit;
}

// ---- a sample ----
__host__ __device__ __forceinline__ void sample_iq(const Consts &C, uint32_t m, bool noisy, uint64_t key, uint32_t index, float &i, float &q) {
    i = m == M_ZERO ? C.base_i[0] : m == M_ONE ? C.base_i[1] : C.base_i[2];
    q = m == M_ZERO ? C.base_q[0] : m == M_ONE ? C.base_q[1] : C.base_q[2];
    if (noisy) {
        i = i + noise(key, index, 0u, C.unit);
        q = q + noise(key, index, 1u, C.unit);
    }
}
__host__ __device__ __forceinline__ int32_t quantise(uint32_t kind, float x, double full_scale) {   // synth.quantise_sc16 / _sc8 / _cu8
    double v = (double)x * full_scale;
    if (kind == NFC_IN_IQ_U8) v = 127.5 + v;
    v = rint(v);
    const double lo = kind == NFC_IN_IQ_I16 ? -32768.0 : kind == NFC_IN_IQ_I8 ? -128.0 : 0.0;
    const double hi = kind == NFC_IN_IQ_I16 ? 32767.0 : kind == NFC_IN_IQ_I8 ? 127.0 : 255.0;
    v = v < lo ? lo : v > hi ? hi : v;
    return (int32_t)v;
}
__host__ __device__ __forceinline__ uint32_t bytes_per_sample(uint32_t kind) {
    return kind == NFC_IN_IQ_F32 ? 8u : kind == NFC_IN_IQ_I16 ? 4u : 2u;
}
// a sample as it lies in memory, I first, in the low bytes_per_sample bytes
__host__ __device__ __forceinline__ uint64_t pack(uint32_t kind, float i, float q, double full_scale) {
    if (kind == NFC_IN_IQ_F32) return (uint64_t)__builtin_bit_cast(uint32_t, i) | ((uint64_t)__builtin_bit_cast(uint32_t, q) << 32);
    const uint32_t a = (uint32_t)quantise(kind, i, full_scale), b = (uint32_t)quantise(kind, q, full_scale);
    if (kind == NFC_IN_IQ_I16) return (uint64_t)((a & 0xFFFFu) | (b << 16));
    return (uint64_t)((a & 0xFFu) | ((b & 0xFFu) << 8));
}
__host__ __device__ __forceinline__ uint64_t align_up(uint64_t n, uint32_t align) { return (n + align - 1) & ~(uint64_t)(align - 1); }

#if defined(__HIPCC__) && !defined(NFC_AIR_PIECES_ONLY)   // (answers_tx.hip.h takes the pieces alone: the kernels are nfc_air.hip's)
// ---- the kernels -------------------------------------------------------------------------------------------------------------------
struct AddU64 {
    using T = uint64_t;
    static __device__ __forceinline__ T identity() { return 0ull; }
    static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};

struct Input {   // the frames as the caller gave them, and whose they are
    const nfc_air_frame *frames;
    const uint32_t *frame_off, *byte_base;   // [K + 1] each
    const uint8_t *air, *par;
    uint32_t K, F;
};
struct LayoutArgs {
    Consts C;
    Input in;
    uint32_t *rel_start;    // [F] a frame's first sample (of its idle_before) in its stream; saturates
    uint64_t *n_stream;     // [K] a stream's samples, the tail included
};
// A workgroup per stream, a lane per frame: the lane walks its frame's pieces, the workgroup scans the lengths.
__global__ __launch_bounds__(BLOCK) void k_air_layout(LayoutArgs A) {
    __shared__ uint64_t s_scan[BLOCK / 64];
    const uint32_t k = blockIdx.x;
    const uint32_t f0 = A.in.frame_off[k], f1 = A.in.frame_off[k + 1], byte0 = A.in.byte_base[k];
    uint64_t carry = 0;
    for (uint32_t base = f0; base < f1; base += BLOCK) {   // (the same trips for every lane: the scan synchronises)
        const uint32_t f = base + threadIdx.x;
        uint64_t len = 0;
        if (f < f1) {
            const nfc_air_frame fr = A.in.frames[f];
            const Bits B = {A.in.air + byte0 + fr.byte_off, A.in.par + byte0 + fr.byte_off, fr.n_bits};
            len = (uint64_t)fr.idle_before + frame_samples(A.C, fr.type, B);
        }
        uint64_t total;
        const uint64_t before = carry + block_exclusive<AddU64, BLOCK / 64>(len, s_scan, total);
        if (f < f1) A.rel_start[f] = before > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)before;
        carry += total;
    }
    if (threadIdx.x == 0) A.n_stream[k] = carry + A.C.tail;
}

// One workgroup: every stream's first sample, streams packed in stream order, each start rounded up to `align`.  All starts are
// multiples of align, so the scan is a plain sum of the rounded lengths.
__global__ __launch_bounds__(START_BLOCK) void k_air_starts(const uint64_t *n_stream, uint32_t K, uint32_t align, uint64_t *first_sample, uint32_t *n_samples) {
    __shared__ uint64_t s_scan[START_BLOCK / 64];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < K; base += START_BLOCK) {
        const uint32_t k = base + threadIdx.x;
        const uint64_t n = k < K ? n_stream[k] : 0ull;
        uint64_t total;
        const uint64_t before = carry + block_exclusive<AddU64, START_BLOCK / 64>(align_up(n, align), s_scan, total);
        if (k < K) {
            first_sample[k] = before;
            n_samples[k] = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
        }
        carry += total;
    }
}

struct RenderArgs {
    Consts C;
    Input in;
    const uint32_t *frame_stream;   // [F]
    const uint32_t *rel_start;      // [F]
    const uint64_t *first_sample;   // [K]
    const uint32_t *n_samples;      // [K]
    const uint64_t *stream_seeds;   // [K], or null: stream k's is k
    const uint32_t *empty;          // the streams without a frame
    uint8_t *out;
};

template <int KIND>
struct Group {   // what one lane writes at a time: 16-byte stores, 32 bytes of float samples as k_tx_render's lanes write
    static constexpr int BPS = KIND == NFC_IN_IQ_F32 ? 8 : KIND == NFC_IN_IQ_I16 ? 4 : 2;
    static constexpr int SAMPLES = KIND == NFC_IN_IQ_F32 ? 4 : KIND == NFC_IN_IQ_I16 ? 4 : 8;
    static constexpr int WORDS = SAMPLES * BPS / 4;
};

// first run whose end lies beyond position s; ends carry the run's level in bit 0
__device__ __forceinline__ uint32_t find_run(const uint32_t *ends, uint32_t n, uint32_t s) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((ends[mid] >> 1) > s) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// A workgroup per frame: the frame's idle_before in front of it and, behind a stream's last frame, the tail and the padding up to the next
// stream's start (idle carrier without noise); the workgroups past the frames take the streams that have no frame.  The workgroup stages
// the frame's bytes in LDS, makes the frame's run ends there from them -- a piece per lane, a block scan of the pieces' sample counts --
// and then ALL its lanes walk the whole span in groups of 16-byte-aligned samples, idle and frame alike: a long lead-in is spread over the
// lanes as the frame is.  A group that the span covers whole leaves as 16-byte stores (plain ones: tx.hip.h measured non-temporal ones
// 2.2 x slower for this pattern), a group cut by the span's end one sample at a time -- the neighbouring span's workgroup writes the rest.
// Dynamic LDS, sized by the host to the call's longest frame (render_lds_bytes): the run ends, then the frame's bytes and ninth bits.
constexpr int RENDER_BLOCK = 64;    // (measured at 1 024 whole-card reads, fc32 without noise: 0.82 ms with 64 lanes, 0.84 with 128, 0.95 with 256 -- a frame of some 1 800 samples is too little work to hide a larger workgroup's start behind: DESIGN.md 8l)
__host__ __device__ __forceinline__ uint32_t render_lds_words(uint32_t max_bits) { return 2u * (max_bits + 2u) + 2u * ((frame_bytes(max_bits) + 3u) / 4u); }

template <int KIND>
__global__ __launch_bounds__(RENDER_BLOCK) void k_air_render(RenderArgs A, uint32_t max_bits) {
    using G = Group<KIND>;
    extern __shared__ uint32_t s_dyn[];
    __shared__ uint32_t s_scan[RENDER_BLOCK / 64];
    uint32_t *s_end = s_dyn;
    uint8_t *s_air = (uint8_t *)(s_dyn + 2u * (max_bits + 2u)), *s_par = s_air + 4u * ((frame_bytes(max_bits) + 3u) / 4u);
    const uint32_t b = blockIdx.x, F = A.in.F;
    uint32_t k, rel0 = 0, idle = 0, type = 0, n_bits = 0;
    bool last = true;
    if (b < F) {
        k = A.frame_stream[b];
        const nfc_air_frame fr = A.in.frames[b];
        const uint32_t byte0 = A.in.byte_base[k] + fr.byte_off;
        rel0 = A.rel_start[b], idle = fr.idle_before, type = fr.type, n_bits = fr.n_bits;
        last = b + 1 == A.in.frame_off[k + 1];
        for (uint32_t i = threadIdx.x; i < frame_bytes(n_bits); i += RENDER_BLOCK) s_air[i] = A.in.air[byte0 + i], s_par[i] = A.in.par[byte0 + i];
    } else {
        k = A.empty[b - F];
    }
    const uint64_t first = A.first_sample[k];
    const uint32_t n_k = A.n_samples[k];
    const uint64_t key = stream_key(A.C.seed, A.stream_seeds ? A.stream_seeds[k] : (uint64_t)k);
    const bool noisy = A.C.noisy != 0;
    __syncthreads();

    const Bits B = {s_air, s_par, n_bits};
    const uint32_t np = n_pieces(type, n_bits);
    uint32_t frame_len = 0;
    for (uint32_t base = 0; base < np; base += RENDER_BLOCK) {   // (the same trips for every lane: the scan synchronises)
        const uint32_t j = base + threadIdx.x;
        Piece P = {0u, 0u, 0u, 0u};
        if (j < np) P = piece_of(A.C, type, B, j);
        uint32_t total;
        const uint32_t at = frame_len + block_exclusive<AddU32, RENDER_BLOCK / 64>(P.ca + P.cb, s_scan, total);
        if (j < np) {
            s_end[2 * j] = ((at + P.ca) << 1) | P.la;
            s_end[2 * j + 1] = ((at + P.ca + P.cb) << 1) | P.lb;
        }
        frame_len += total;
    }
    __syncthreads();
    const uint32_t n_runs = 2 * np;
    // positions in the stream; all below 2^31 (a stream and its padding: MAX_STREAM_SAMPLES + the alignment), so the walk is in int32
    const int32_t fr0 = (int32_t)(rel0 + idle), fr1 = fr0 + (int32_t)frame_len, n_stream = (int32_t)n_k;
    const int32_t lo = (int32_t)rel0, hi = !last ? fr1 : k + 1 < A.in.K ? (int32_t)(uint32_t)(A.first_sample[k + 1] - first) : n_stream;
    const uint64_t a0 = first + (uint32_t)lo, a1 = first + (uint32_t)hi;    // the span in the buffer
    const uint64_t g1 = (a1 + G::SAMPLES - 1) / G::SAMPLES;
    for (uint64_t g = a0 / G::SAMPLES + threadIdx.x; g < g1; g += RENDER_BLOCK) {
        const uint64_t s0 = g * G::SAMPLES;
        const int32_t r0 = (int32_t)(int64_t)(s0 - first);   // (below lo, even below 0, in a group the span cuts at its front)
        uint64_t v[G::SAMPLES];
        uint32_t run = 0, end = 0, level = 0;
        const bool in_frame = frame_len != 0 && r0 + G::SAMPLES > fr0 && r0 < fr1;   // (most groups of an idle stretch are not)
        if (in_frame) {
            const int32_t p0 = r0 > fr0 ? r0 - fr0 : 0;
            run = find_run(s_end, n_runs, (uint32_t)p0);
            end = s_end[run] >> 1, level = s_end[run] & 1u;
        }
#pragma unroll
        for (int i = 0; i < G::SAMPLES; i++) {
            const int32_t r = r0 + i;
            uint32_t m = M_ONE;
            if (in_frame && r >= fr0 && r < fr1) {
                const uint32_t pos = (uint32_t)(r - fr0);
                while (pos >= end) {   // (pos < frame_len, the last run's end; runs of no samples are stepped over)
                    run++;
                    end = s_end[run] >> 1, level = s_end[run] & 1u;
                }
                m = type ? level : level ? M_LOADED : M_ONE;
            }
            float si, sq;
            sample_iq(A.C, m, noisy && r < n_stream, key, (uint32_t)r, si, sq);
            v[i] = pack(KIND, si, sq, A.C.full_scale);
        }
        uint8_t *o = A.out + s0 * G::BPS;
        if (s0 >= a0 && s0 + G::SAMPLES <= a1) {
            uint32_t w[G::WORDS];
#pragma unroll
            for (int i = 0; i < G::SAMPLES; i++) {
                if constexpr (G::BPS == 8) w[2 * i] = (uint32_t)v[i], w[2 * i + 1] = (uint32_t)(v[i] >> 32);
                else if constexpr (G::BPS == 4) w[i] = (uint32_t)v[i];
                else if (i & 1) w[i / 2] |= (uint32_t)v[i] << 16;
                else w[i / 2] = (uint32_t)v[i];
            }
#pragma unroll
            for (int q = 0; q < G::WORDS / 4; q++) ((uint4 *)o)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < G::SAMPLES; i++) {
                if (s0 + i < a0 || s0 + i >= a1) continue;
                if constexpr (G::BPS == 8) ((uint2 *)o)[i] = make_uint2((uint32_t)v[i], (uint32_t)(v[i] >> 32));
                else if constexpr (G::BPS == 4) ((uint32_t *)o)[i] = (uint32_t)v[i];
                else ((uint16_t *)o)[i] = (uint16_t)v[i];
            }
        }
    }
}
#endif   // __HIPCC__

}  // namespace air
}  // namespace nfc
