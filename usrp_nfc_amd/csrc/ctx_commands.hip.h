// ctx_commands.hip.h -- commands on the GPU for ONE long stream: the protocol machine of fsm.hip.h, unchanged, a lane per TRANSACTION
// over the frames a single context assembled (frames.hip.h: CtxArgs), and a resolve step that makes the result the sequential
// machine's, bit for bit.  DESIGN.md 8o.
//
// The machine is sequential but not one chain: a plain REQA / WUPA heard outside a CRYPTO1 session leaves it in a state that does
// not depend on where it was (fsm.hip.h, finish(): the UID cleared, tag_type -1, encrypted 0, cur_cmd the command) but for cur_key,
// st, ar, at and the sticky flags, which the frame does not touch.  Such a frame is a CUT (is_cut: what the raw frame shows without
// the machine); a SEGMENT runs from a cut to the next.  Segment 0 runs from frame 0 and starts from the carried machine: exact.
// Every other segment is walked SPECULATIVELY from "the carried machine with encrypted == 0" and leaves a summary: its end machine,
// whether it wrote cur_key (an AUTHA / AUTHB recognised), whether it wrote the session words st / ar / at (a RANDTA outside a
// session: the only door into one), its flags, and whether it READ the incoming cur_key before writing it (a RANDTA by stage with
// no AUTH in the segment).  The RESOLVE walks the summaries in order: segment k stands iff the true machine entering it has
// encrypted == 0 and, where it read cur_key, the true value is the one it assumed (the carried machine's).  A segment that stands
// composes -- what it wrote replaces, what it did not write is inherited, flags are OR-ed; one that does not is walked again from
// the true machine, in place, and its summary becomes an exact one (everything written).
//
// One text for both holders: the kernels below (NFC_CTX_COMMANDS_KERNELS) and nfc_host_commands_segmented (nfc_ctx_commands.hip),
// the twin on the CPU.  They differ in the accessor that hands out frame m of the merged order (DevFrames / HostFrames) and in how
// the resolve is spread: the twin judges one summary at a time, the kernel 64 at a time by ballot, with the same predicates.
//
// Four launches behind the frames' two: k_ctx_merge (a thread per raw frame: its rank in the merged order by a binary search over
// the other type's idx, type 0 first on a tie; its slot; whether it is a cut), k_ctx_segments (one workgroup numbers the segments by
// a scan of the cut marks, tile after tile, the total carried in a register), k_ctx_walk (64 segments per workgroup, one wave, as
// k_multi_commands) and k_ctx_resolve (one wave).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"
#include "fsm.hip.h"
#include "scan.hip.h"

namespace nfc {
namespace ctxcmd {

// a reader frame that is REQA or WUPA as far as anybody can tell without the machine
NFC_HD bool is_cut(int type, uint32_t raw_flags, uint32_t n_bytes, uint32_t byte0) {
    return type == 1 && !(raw_flags & NFC_RAW_CUT) && (raw_flags & NFC_RAW_PARITY_OK) && n_bytes == 1u && (byte0 == 0x26u || byte0 == 0x52u);
}

enum { M_WROTE_KEY = 1, M_WROTE_SESS = 2, M_READ_KEY = 4, M_EXACT = 8 };   // a summary's meta word

// frame m of the merged order, as an accessor's get(m) hands it out
struct Frame {
    int type;
    uint32_t flags, n;            // the raw frame's flags; its bytes (0 with NFC_RAW_CUT)
    const uint8_t *bytes, *par;
    uint32_t slot;                // where its n entries of data / enc start
};

NFC_HD void store_rec(uint32_t *w, const fsmd::Rec &r, uint32_t slot) {   // an nfc_frame as seven words (k_multi_commands' record words)
    w[0] = (uint32_t)r.cmd;
    w[1] = (uint32_t)r.type;
    w[2] = slot;
    w[3] = r.n_bytes | r.n_header << 16;
    w[4] = r.n_extra | r.n_crc << 16;
    w[5] = r.flags;
    w[6] = r.n_enc;
}

// the speculative start of a segment that begins at a cut: any state with encrypted == 0 will do, the carried one is at hand
NFC_HD void speculative_start(fsmd::Machine &M) {
    M.encrypted = 0;
    M.flags = 0;
}

// Frames [m0, m1) through process_frame, records / data / enc written in place.  meta collects what the summary says of cur_key and
// the session words: by the command process_frame recognised and the session state it found -- finish() reads cur_key at a RANDTA
// outside a session and nowhere else before an AUTH of the same segment has written it (the nested route needs cur_cmd AUTHA / AUTHB,
// which only an AUTH behind the cut can have left).
template <class Frames, class Table>
NFC_HD void walk(fsmd::Machine &M, uint32_t &meta, const Frames &F, uint32_t m0, uint32_t m1, const Table &tab) {
    for (uint32_t m = m0; m < m1; m++) {
        const Frame f = F.get(m);
        const int32_t enc_before = M.encrypted;
        const fsmd::Rec r = fsmd::process_frame(M, f.type, f.flags, f.n, f.bytes, f.par, F.data + f.slot, F.enc + f.slot, tab);
        store_rec(F.cmd + (size_t)m * (sizeof(nfc_frame) / 4), r, f.slot);
        if (r.cmd == fsmd::C_AUTHA || r.cmd == fsmd::C_AUTHB) meta |= M_WROTE_KEY;
        else if (r.cmd == fsmd::C_RANDTA && !enc_before) meta |= (meta & M_WROTE_KEY) ? M_WROTE_SESS : (M_WROTE_SESS | M_READ_KEY);
    }
}

// does the speculative summary `meta` stand, the true machine entering its segment having these two values?
NFC_HD bool stands(uint32_t meta, int32_t true_encrypted, int32_t true_cur_key, int32_t assumed_cur_key) {
    return true_encrypted == 0 && (!(meta & M_READ_KEY) || true_cur_key == assumed_cur_key);
}
// T: the true machine entering a segment that stands; E: the segment's end machine -> the true machine behind it
NFC_HD void compose(fsmd::Machine &E, uint32_t meta, const fsmd::Machine &T) {
    if (!(meta & M_WROTE_KEY)) E.cur_key = T.cur_key;
    if (!(meta & M_WROTE_SESS)) E.st = T.st, E.ar = T.ar, E.at = T.at;
    E.flags |= T.flags;
}

// the counters beside the commands (nfc_ctx_commands)
enum { H_N_CMDS, H_N_BYTES, H_N_SEGMENTS, H_N_RERUN_SEGMENTS, H_N_RERUN_FRAMES, H_N_KEYDEP, H_FLAGS, H_WORDS = 16 };

constexpr int THREADS = 64;
constexpr int MG_THREADS = 256;
constexpr int SG_THREADS = 1024, SG_WAVES = SG_THREADS / 64, SG_ITEMS = 4, SG_TILE = SG_THREADS * SG_ITEMS;

// what the launches are given (per type named apart: no array a lane would index)
struct Args {
    const nfc_raw_frame *rec0, *rec1;     // frames::CtxArgs: records, bytes, par, the device's totals
    const uint8_t *bytes0, *bytes1, *par0, *par1;
    const uint64_t *totals;               // frames 0, bytes 0, frames 1, bytes 1
    uint32_t cap_fr0, cap_fr1, cap_by0, cap_by1;   // what the HOST laid out: the device's totals cannot reach past it
    uint32_t *state;                      // [fsmd::W_WORDS], one machine
    const uint32_t *sector_keys;          // [skeys::WORDS] as one stream's table (sector_keys.h), or null
    uint32_t *hdr;                        // [H_WORDS]
    uint32_t *cmd, *src;                  // cap_cmds records of seven words / words
    uint8_t *data;
    uint16_t *enc;                        // cap_bytes entries each
    uint32_t cap_cmds, cap_bytes, cap_seg;
    uint32_t *slot;                       // [cap_cmds]
    uint8_t *cutf;                        // [cap_cmds]
    uint32_t *seg_start;                  // [cap_seg + 1]
    uint32_t *sum, *meta;                 // [fsmd::W_WORDS][cap_seg], [cap_seg]
};
// ev: null, or three events recorded behind the segment numbering, behind the walk and behind the resolve
void launch(const Args &A, hipStream_t stream, const hipEvent_t *ev);

#ifdef NFC_CTX_COMMANDS_KERNELS
struct Totals {
    uint32_t nf0, nf1, nb0, nb1, n;
};
__device__ __forceinline__ Totals totals_of(const Args &A) {
    const uint64_t f0 = A.totals[0], b0 = A.totals[1], f1 = A.totals[2], b1 = A.totals[3];
    Totals T;
    T.nf0 = f0 < A.cap_fr0 ? (uint32_t)f0 : A.cap_fr0;
    T.nf1 = f1 < A.cap_fr1 ? (uint32_t)f1 : A.cap_fr1;
    T.nb0 = b0 < A.cap_by0 ? (uint32_t)b0 : A.cap_by0;
    T.nb1 = b1 < A.cap_by1 ? (uint32_t)b1 : A.cap_by1;
    const uint64_t n = (uint64_t)T.nf0 + T.nf1;
    T.n = n < A.cap_cmds ? (uint32_t)n : A.cap_cmds;
    return T;
}

struct DevFrames {
    const Args &A;
    Totals T;
    uint32_t *cmd;
    uint8_t *data;
    uint16_t *enc;
    __device__ __forceinline__ Frame get(uint32_t m) const {
        const uint32_t s = A.src[m], t = s >> 31;
        uint32_t i = s & 0x7FFFFFFFu;
        const uint32_t nf = t ? T.nf1 : T.nf0, nb = t ? T.nb1 : T.nb0;
        i = i < nf ? i : 0u;   // (never: k_ctx_merge wrote an index below the type's count)
        const uint4 *q = (const uint4 *)((t ? A.rec1 : A.rec0) + i);
        const uint4 q0 = q[0], q1 = q[1];
        Frame f;
        f.type = (int)t;
        f.flags = q1.y;
        f.n = q1.x;
        f.slot = A.slot[m];
        // (never: a frame's bytes lie inside its type's array, its slot inside the room the host laid out)
        if (nf == 0u || (uint64_t)q0.z + f.n > nb || (uint64_t)f.slot + f.n > A.cap_bytes) f.flags = NFC_RAW_CUT;
        if (f.flags & NFC_RAW_CUT) f.n = 0, f.slot = 0;
        const uint32_t off = f.n ? q0.z : 0u;
        f.bytes = (t ? A.bytes1 : A.bytes0) + off;
        f.par = (t ? A.par1 : A.par0) + off;
        return f;
    }
};

// ---- merged order: a thread per raw frame, blockIdx.y its type ----
__global__ __launch_bounds__(MG_THREADS) void k_ctx_merge(Args A) {
    const Totals T = totals_of(A);
    const uint32_t t = blockIdx.y, i = blockIdx.x * MG_THREADS + threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < (uint32_t)H_WORDS) A.hdr[threadIdx.x] = 0u;
    const uint32_t nf = t ? T.nf1 : T.nf0, no = t ? T.nf0 : T.nf1;
    if (i >= nf) return;
    const nfc_raw_frame *mine = (t ? A.rec1 : A.rec0) + i, *other = t ? A.rec0 : A.rec1;
    const uint4 q0 = ((const uint4 *)mine)[0], q1 = ((const uint4 *)mine)[1];
    const uint64_t idx = (uint64_t)q0.x | (uint64_t)q0.y << 32;
    // frames of the other type before this one: type 0 goes first on a tie
    uint32_t lo = 0, hi = no;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t o = other[mid].idx;
        const bool before = t ? o <= idx : o < idx;
        if (before) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t m = i + lo;
    if (m >= T.n) return;   // (never: the ranks are a permutation of [0, n))
    const uint32_t other_off = lo < no ? other[lo].byte_off : (t ? T.nb0 : T.nb1);
    const uint32_t n = q1.x, flags = q1.y, byte_off = q0.z;
    A.src[m] = t << 31 | i;
    A.slot[m] = byte_off + other_off;
    const uint32_t nb = t ? T.nb1 : T.nb0;
    const uint32_t b0 = (n >= 1u && (uint64_t)byte_off + n <= nb) ? (t ? A.bytes1 : A.bytes0)[byte_off] : 0u;
    A.cutf[m] = (m > 0u && is_cut((int)t, flags, n, b0)) ? 1 : 0;   // (a cut at frame 0 opens no segment: segment 0 starts there anyway)
}

// ---- the segments: seg_start[k] for every cut, in order ----
__global__ __launch_bounds__(SG_THREADS) void k_ctx_segments(Args A) {
    __shared__ uint32_t lds[SG_WAVES];
    const Totals T = totals_of(A);
    const uint32_t tid = threadIdx.x;
    uint32_t run = 1;   // segment 0 opens at frame 0
    for (uint32_t base = 0; base < T.n; base += SG_TILE) {
        const uint32_t m0 = base + tid * SG_ITEMS;
        uint32_t c[SG_ITEMS], mine = 0;
#pragma unroll
        for (int j = 0; j < SG_ITEMS; j++) {
            c[j] = m0 + j < T.n ? A.cutf[m0 + j] : 0u;
            mine += c[j];
        }
        uint32_t tile_total;
        uint32_t at = run + block_exclusive<AddU32, SG_WAVES>(mine, lds, tile_total);
#pragma unroll
        for (int j = 0; j < SG_ITEMS; j++)
            if (c[j]) {
                if (at < A.cap_seg) A.seg_start[at] = m0 + j;
                at++;
            }
        run += tile_total;
    }
    if (tid == 0) {
        const uint32_t S = T.n ? (run < A.cap_seg ? run : A.cap_seg) : 0u;
        A.seg_start[0] = 0;
        A.seg_start[S] = T.n;   // (S <= cap_seg: the array holds cap_seg + 1)
        A.hdr[H_N_SEGMENTS] = S;
        A.hdr[H_N_CMDS] = T.n;
        A.hdr[H_N_BYTES] = T.nb0 + T.nb1;
    }
}

// ---- the speculative walk: a lane per segment ----
__global__ __launch_bounds__(THREADS) void k_ctx_walk(Args A) {
    const Totals T = totals_of(A);
    const uint32_t S = A.hdr[H_N_SEGMENTS] < A.cap_seg ? A.hdr[H_N_SEGMENTS] : A.cap_seg;
    const uint32_t k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= S) return;
    uint32_t m0 = A.seg_start[k], m1 = A.seg_start[k + 1];
    m1 = m1 < T.n ? m1 : T.n;
    m0 = m0 < m1 ? m0 : m1;
    fsmd::Machine M;
    fsmd::load_machine(M, A.state, 1, 0);
    if (k) speculative_start(M);
    const skeys::DeviceTable keys = {A.sector_keys, 1u, 0u};
    const DevFrames F = {A, T, A.cmd, A.data, A.enc};
    uint32_t meta = 0;
    walk(M, meta, F, m0, m1, keys);
    if (k == 0) meta = M_WROTE_KEY | M_WROTE_SESS | M_EXACT;   // (its start was the carried machine itself)
    fsmd::store_machine(M, A.sum, A.cap_seg, k);
    A.meta[k] = meta;
}

// ---- the resolve: one wave, 64 summaries at a time ----
// The carry between two rounds is what validity and composition need of the true machine: encrypted and cur_key as values, the
// session words as the segment whose summary holds them, the flags.  Within a round a lane's incoming cur_key is the end cur_key of
// the nearest lane below that wrote one; the first lane that does not stand -- judged as if all below it stood, which is true of
// the FIRST -- walks its segment again from the true machine and becomes an exact summary; the round is judged again behind it.
__global__ __launch_bounds__(THREADS) void k_ctx_resolve(Args A) {
    using namespace fsmd;
    const Totals T = totals_of(A);
    const uint32_t S = A.hdr[H_N_SEGMENTS] < A.cap_seg ? A.hdr[H_N_SEGMENTS] : A.cap_seg;
    const uint32_t lane = threadIdx.x;
    const size_t C = A.cap_seg;
    Machine M0;
    load_machine(M0, A.state, 1, 0);
    if (S == 0) {
        if (lane == 0) A.hdr[H_FLAGS] = M0.flags;
        return;
    }
    const int32_t assumed = M0.cur_key;
    const skeys::DeviceTable keys = {A.sector_keys, 1u, 0u};
    const DevFrames F = {A, T, A.cmd, A.data, A.enc};
    int32_t c_enc = (int32_t)A.sum[W_ENCRYPTED * C], c_key = (int32_t)A.sum[W_CUR_KEY * C];
    uint32_t c_sess = 0, c_flags = A.sum[W_FLAGS * C];
    uint32_t n_rr = 0, n_rf = 0, n_kd = 0;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t base = 1; base < S; base += 64) {
        const uint32_t k = base + lane;
        const bool have = k < S;
        uint32_t meta = have ? A.meta[k] : 0u;
        int32_t e_enc = have ? (int32_t)A.sum[W_ENCRYPTED * C + k] : 0, e_key = have ? (int32_t)A.sum[W_CUR_KEY * C + k] : 0;
        uint32_t e_flags = have ? A.sum[W_FLAGS * C + k] : 0u;
        n_kd += (uint32_t)__builtin_popcountll(__ballot(have && (meta & M_READ_KEY)));
        uint32_t lo = 0;
        for (;;) {
            const uint64_t wk = __ballot(have && (meta & M_WROTE_KEY)), ws = __ballot(have && (meta & M_WROTE_SESS));
            const uint64_t f0 = __ballot(have && (e_flags & 1u)), f1 = __ballot(have && (e_flags & 2u));
            const uint64_t kb = wk & below, sb = ws & below;
            const int ksrc = kb ? 63 - __builtin_clzll(kb) : 0;
            const int32_t k_from = __shfl(e_key, ksrc, 64);
            const int32_t in_key = kb ? k_from : c_key;
            const int32_t up_enc = __shfl_up(e_enc, 1u, 64);
            const int32_t in_enc = lane ? up_enc : c_enc;
            const bool fails = have && lane >= lo && !stands(meta, in_enc, in_key, assumed);
            const uint64_t bad = __ballot(fails);
            if (!bad) break;
            const uint32_t f = (uint32_t)__builtin_ctzll(bad);
            if (lane == f) {
                Machine Tm;
                load_machine(Tm, A.sum, C, k - 1u);   // (k >= 1: the end machine of the segment before, exact or standing)
                const uint32_t sseg = sb ? base + (uint32_t)(63 - __builtin_clzll(sb)) : c_sess;
                Tm.cur_key = in_key;
                Tm.st = ((uint64_t)A.sum[W_ST_LO * C + sseg] | (uint64_t)A.sum[W_ST_HI * C + sseg] << 32) & ST_MASK;
                Tm.ar = A.sum[W_AR * C + sseg];
                Tm.at = A.sum[W_AT * C + sseg];
                Tm.flags = c_flags | ((f0 & below) ? 1u : 0u) | ((f1 & below) ? 2u : 0u);
                uint32_t m0 = A.seg_start[k], m1 = A.seg_start[k + 1];
                m1 = m1 < T.n ? m1 : T.n;
                m0 = m0 < m1 ? m0 : m1;
                uint32_t unused = 0;
                walk(Tm, unused, F, m0, m1, keys);
                store_machine(Tm, A.sum, C, k);
                meta = M_WROTE_KEY | M_WROTE_SESS | M_EXACT;
                A.meta[k] = meta;
                e_enc = Tm.encrypted, e_key = Tm.cur_key, e_flags = Tm.flags;
                n_rr += 1u, n_rf += m1 - m0;
            }
            lo = f + 1u;
        }
        // the carry behind this round
        const uint64_t wk = __ballot(have && (meta & M_WROTE_KEY)), ws = __ballot(have && (meta & M_WROTE_SESS));
        const uint64_t f0 = __ballot(have && (e_flags & 1u)), f1 = __ballot(have && (e_flags & 2u));
        const uint32_t last = S - base < 64u ? S - base - 1u : 63u;
        c_enc = __shfl(e_enc, (int)last, 64);
        const int32_t k_from = __shfl(e_key, wk ? 63 - __builtin_clzll(wk) : 0, 64);
        if (wk) c_key = k_from;
        if (ws) c_sess = base + (uint32_t)(63 - __builtin_clzll(ws));
        c_flags |= (f0 ? 1u : 0u) | (f1 ? 2u : 0u);
    }
    // counters: every lane's own, summed
    for (int d = 32; d >= 1; d >>= 1) {
        n_rr += (uint32_t)__shfl_down((int)n_rr, (unsigned)d, 64);
        n_rf += (uint32_t)__shfl_down((int)n_rf, (unsigned)d, 64);
    }
    if (lane == 0) {
        Machine E;
        load_machine(E, A.sum, C, S - 1u);
        E.cur_key = c_key;
        E.st = ((uint64_t)A.sum[W_ST_LO * C + c_sess] | (uint64_t)A.sum[W_ST_HI * C + c_sess] << 32) & ST_MASK;
        E.ar = A.sum[W_AR * C + c_sess];
        E.at = A.sum[W_AT * C + c_sess];
        E.flags = c_flags;
        E.key_a = M0.key_a, E.key_b = M0.key_b;
        store_machine(E, A.state, 1, 0);
        A.hdr[H_N_RERUN_SEGMENTS] = n_rr;
        A.hdr[H_N_RERUN_FRAMES] = n_rf;
        A.hdr[H_N_KEYDEP] = n_kd;
        A.hdr[H_FLAGS] = c_flags;
    }
}
#endif   // NFC_CTX_COMMANDS_KERNELS

}  // namespace ctxcmd
}  // namespace nfc
