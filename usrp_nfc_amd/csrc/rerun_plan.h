// rerun_plan.h -- what the threshold stage decides between two host turns when speculation does not certify: which failing chunks a
// round re-runs and which wait, which kernel re-runs them, when the in-place form is switched off for the rest of the batch, which
// chunks are certified again, and whether the batch's fp64 sums are provably exact (host only, no device code, no HIP include:
// host_threshold.h runs the rounds -- launches, copies, waits -- and asks here WHAT a round does; tools/rerun_plan_check drives these
// functions with a model of the device and checks their properties without a GPU, tests/test_rerun_plan_host.py runs it).
//
// An attempt: pass 0 (every chunk from a speculated state), then rounds.  A round: the pending chunks are certified against their
// predecessors' summaries (failing_of reads the verdicts), the failing ones are re-run from the exact state (plan_round says which,
// and by which kernel), and the next round certifies what was re-run and what can see it (pending_after).  Every round makes at
// least the first pending chunk final, and a chunk takes at most two rounds to become final (the workgroup kernel may give it up
// once): an attempt ends within 2 * nch + 2 rounds, the bound the host enforces.  The rules, each stated here and nowhere else:
//   1 the wait rule   a failing chunk right behind one taken in this round, that did not give up and has never been re-run, waits
//   2 lone            the failures left are few: at most lone_max, at most one chunk in lone_div
//   3 ex_off          more than a quarter of the workgroup kernel's latest re-runs gave up: no in-place form for the rest of the attempt
//   4 in place        the plan allows the in-place form, it is not switched off, and the failures fit the machine (ex_max)
//   5 assignment      per chunk: the workgroup kernel (in place or lone) until it has given the chunk up, k_threshold from then on
//   pending_after     the re-run chunks and every chunk that can see one through predecessors that left ring slots untouched
//   sums_exact        all operands multiples of 2^low, no sum reaches 2^(low + 53)
// Per-chunk flags as the kernels leave them (gflags): 1 a value the chunk cannot vouch for, 2 the chunk left ring slots untouched
// (its successor sees through it), 4 the kernel gave the chunk up, bits 4-6 why.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace nfc {

// what is fixed for an attempt
struct RerunPolicy {
    bool wg;           // pass 0 was the workgroup form (ThrForm::Workgroup): its kernels may take re-runs
    bool in_place;     // ThrPlan.in_place: k_threshold_wg<KIND, 4, true> exists for this stream
    bool rerun_lone;   // wg_rerun_lone
    size_t lone_max;   // wg_lone_max
    uint64_t lone_div; // wg_lone_div
    size_t ex_max;     // wg_ex_max: as many workgroups of the in-place form as are resident at once
    uint32_t nch;
};

// the state of an attempt's rounds.  It lives in the context, so that its vectors keep their capacity from batch to batch.
struct RerunBook {
    std::vector<uint8_t> tried_wg;    // 1: the workgroup kernel ran the chunk's latest re-run; 2: it has given up on it (or k_threshold has taken it since)
    std::vector<uint8_t> ever_rerun;  // chunks re-run at least once in this attempt
    bool ex_off = false;              // the in-place form is not used for the rest of this attempt
    std::vector<uint32_t> pending;    // the chunks the next certification is for (ascending)
    std::vector<uint8_t> ver;         // per chunk: which of its two summary buffers its latest evaluation wrote (flipped by a re-run)
    std::vector<uint32_t> failing;    // failing_of: the round's failing chunks; after plan_round: the ones the round re-runs (both ascending)
    std::vector<uint32_t> by_wg, by_general;   // plan_round: ... by kernel
    // (tried_wg / ever_rerun are sized by the first round that re-runs something: a clean batch pays for the list and the version bytes only)
    void reset(uint32_t nch) {
        tried_wg.clear();
        ever_rerun.clear();
        ex_off = false;
        pending.clear();
        for (uint32_t k = 1; k < nch; k++) pending.push_back(k);
        ver.assign(nch, 0);
    }
};

// The pending chunks whose certification failed, ascending -- and, on the first round, chunk 0 when pass 0 was by a kernel that may
// give up on a chunk (lean) and it did (cert[0] clear): re-run from the carried state.
inline const std::vector<uint32_t> &failing_of(RerunBook &b, bool first_round, bool lean, const uint8_t *cert) {
    b.failing.clear();
    if (first_round && lean && !cert[0]) b.failing.push_back(0);
    for (uint32_t k : b.pending)
        if (!cert[k]) b.failing.push_back(k);
    return b.failing;
}

struct RerunRound {
    const std::vector<uint32_t> &by_wg, &by_general;   // ascending, disjoint; together the chunks the round re-runs (RerunBook.failing)
    bool in_place;                                     // by_wg's kernel: the in-place form (else pass 0's own, mode 1)
};

// What the round re-runs of b.failing, and by which kernel.  Re-runs from the exact state: by the workgroup kernel's in-place form
// where it applies and the round's failures fit the machine (below), else by k_threshold, which decides everything in place and never
// gives up (so the rounds converge).
// (The pass-0 form of the workgroup kernel re-running whatever did not give up was measured on the stress captures in rounds 4-6 --
// the chunks behind a chunk that gave up mostly give up themselves, 6 passes / 4.7 ms against 3 / 2.1 -- and went in round 6.)
inline RerunRound plan_round(const RerunPolicy &p, RerunBook &b, const uint8_t *gflags) {
    // 1. A chunk right behind one that is re-run now and that did not give up itself is NOT re-run in this round: its own
    // evaluation may well be sound -- what failed is the comparison with a predecessor whose summary was worthless -- and
    // from the state resolved now it would only be evaluated against that worthless summary again.  It stays pending
    // (pending_after: it can see a re-run chunk) and is certified against the predecessor's new summary in the next round.
    if (b.ever_rerun.empty()) b.ever_rerun.assign(p.nch, 0);
    {
        size_t taken = 0;
        uint32_t last = 0xFFFFFFFFu;
        for (uint32_t k : b.failing) {   // (ascending)
            // (only a chunk still standing on its pass-0 evaluation: one that has been re-run already was evaluated from a
            // resolved state that has moved since -- waiting would only cost it a round, measured: 3 general passes
            // instead of 2 when every chunk fails)
            const bool gave_up = (gflags[k] & 4) != 0;
            if (!gave_up && !b.ever_rerun[k] && last != 0xFFFFFFFFu && k == last + 1) continue;
            b.failing[taken++] = k;
            last = k;
        }
        b.failing.resize(taken);
        for (uint32_t k : b.failing) b.ever_rerun[k] = 1;
    }
    const std::vector<uint32_t> &failing = b.failing;
    // 2. A LONE failure on an otherwise clean batch (round 6) -- a superstep that grew on the head-room it saw and met the next frame:
    // one chunk in a thousand -- takes the workgroup kernel too, gave up or not: from the exact state (no margin for a speculated
    // window) and with supersteps of at most two rounds it mostly gets through, and four waves walk a 98 304-sample chunk in 70 us
    // where the general kernel's one wave takes 670 (measured on configs[2] with the margin set to make a chunk give up: the step
    // 0.927 -> 0.526 ms, same call).  If it gives up again the general kernel takes it in the next round (tried_wg).
    const bool lone = p.rerun_lone && failing.size() <= p.lone_max && (uint64_t)failing.size() * p.lone_div <= (uint64_t)p.nch;
    // 3. (a stream the workgroup kernel keeps giving up on -- values out of range, a stream's first chunk: k_threshold alone for the rest of the batch)
    if (b.tried_wg.empty()) b.tried_wg.assign(p.nch, 0);
    {
        size_t ran = 0, gave = 0;
        for (uint32_t k : failing)
            if (b.tried_wg[k] == 1) ran++, gave += (gflags[k] & 4) ? 1 : 0;
        if (gave * 4 > ran) b.ex_off = true;
    }
    // 4. Up to a machine-full of failing chunks (round 6): the workgroup kernel in the form that evaluates a failed round IN PLACE
    // (k_threshold_wg<KIND, 4, true>) -- it gives up only where a round is not four whole steps or a LOW run is out of sight.
    const bool ex = p.in_place && !b.ex_off && failing.size() <= p.ex_max;
    // 5.
    b.by_wg.clear();
    b.by_general.clear();
    for (uint32_t k : failing) {
        // (a chunk the in-place form has re-run and that did NOT give up may take it again -- what failed is its incoming state;
        // one it gave up on is k_threshold's for the rest of the batch: that kernel never gives up, so the rounds converge)
        if (b.tried_wg[k] == 1 && (gflags[k] & 4)) b.tried_wg[k] = 2;
        const bool ex_again = ex && b.tried_wg[k] == 1;
        if (p.wg && (!b.tried_wg[k] || ex_again) && (ex || lone)) {
            b.by_wg.push_back(k);
            b.tried_wg[k] = 1;
        } else {
            b.by_general.push_back(k);
            if (b.tried_wg[k]) b.tried_wg[k] = 2;
        }
    }
    return RerunRound{b.by_wg, b.by_general, ex};
}

// The next round's list, from the chunks this round re-runs (b.failing after plan_round) and the flags as they were BEFORE the
// re-runs: the re-run chunks (a predecessor may have been re-run beside them) and every chunk that can see one of them through
// predecessors that left ring slots untouched.  It is made up before the re-runs have run -- a re-run chunk is taken to leave slots
// untouched (which its new summary will say): a superset of what has to be certified, and certifying a chunk nothing has changed for
// gives the verdict it had.
inline const std::vector<uint32_t> &pending_after(RerunBook &b, uint32_t nch, const uint8_t *gflags) {
    b.pending.clear();
    bool vis = false;
    size_t at = 0;   // (into the re-run chunks, ascending)
    for (uint32_t k = 0; k < nch; k++) {
        const bool ran = at < b.failing.size() && b.failing[at] == k;
        if (ran) at++;
        if (vis || ran) b.pending.push_back(k);
        const bool full = !ran && !(gflags[k] & 2);   // (a re-run chunk: not known yet -- taken as not full)
        vis = ran || (vis && !full);
    }
    return b.pending;
}

// Every fp64 sum of a batch is exact -- hence independent of the order it was added in -- when all
// operands are multiples of 2^low and no sum reaches 2^(low + 53).  Operands: ring values (24-bit mantissas)
// and the carried ss / delta (their lowest set bits); sums: the window sums (bounded by the kernel from the sums
// it tracked) and the carried ss itself.  ss_emin / ss_emax: the carried values after the batch (Carry, exponent-field scale, 255:
// zero); emin / emax / vtop: what its chunks measured.
inline bool sums_exact(int ss_emin, int ss_emax, int emin, int emax, uint32_t vtop) {
    int low = emin - 23;
    if (ss_emin != 255) low = std::min(low, ss_emin);
    float vtf;
    memcpy(&vtf, &vtop, 4);
    int high = 255 + 64;   // vtop: f32 bits of an upper bound of every window sum the batch saw
    if (std::isfinite(vtf) && vtf >= 0.f) high = vtf > 0.f ? std::ilogb((double)vtf) + 127 : 0;
    high = std::max(high, ss_emax);
    return (emax < 255) && (high - low <= 52);
}

// what the chunks of a batch measured, folded: the operands of sums_exact, and whether some chunk met a value it cannot vouch for
struct SumBounds {
    int emin = 255, emax = 0;
    bool flagged = false;
    uint32_t vtop = 0;
};
inline SumBounds fold_sum_bounds(uint32_t nch, const uint8_t *gmin, const uint8_t *gmax, const uint8_t *gflags, const uint32_t *gvtop) {
    SumBounds s;
    for (uint32_t k = 0; k < nch; k++) {
        s.emin = std::min(s.emin, (int)gmin[k]);
        s.emax = std::max(s.emax, (int)gmax[k]);
        if (gflags[k] & 1) s.flagged = true;
        s.vtop = std::max(s.vtop, gvtop[k]);
    }
    return s;
}

}  // namespace nfc
