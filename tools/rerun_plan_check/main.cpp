// rerun_plan_check -- the rounds of re-runs of the threshold stage (usrp_nfc_amd/csrc/rerun_plan.h: failing_of, plan_round, pending_after,
// sums_exact, fold_sum_bounds) driven by a small model of the device in place of the kernels, the way host_threshold.h drives them:
// reset, then per round failing_of -> plan_round -> pending_after, until nothing is pending.  After each planned round the model
// decides, from a fixed-seed generator, which re-run chunks gave up (only chunks in by_wg can), which are "full", and which pending
// chunks certify -- except that a chunk evaluated from the final state of its predecessor and not given up always certifies, as the
// kernels guarantee (k_threshold never gives up: that is why the rounds converge).  Every chunk count 1 .. 12, and every policy of
// wg x in_place x rerun_lone x ex_max {0, 2, nch} x lone_max / lone_div {4/64, 4/1, 0/1}; then hand-written cases.
// A stand-alone host program: the way to run the plan under a sanitizer.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/rerun_plan_check/main.cpp -o rerun_plan_check && ./rerun_plan_check
// It touches no GPU.  Exit status 0: in every round of every sequence
//   (a) by_wg and by_general are disjoint and ascending, their union is a subset of the failing chunks that contains the smallest, and
//       every failing chunk left out did not give up, was never re-run in the sequence and sits one above a chunk that was taken;
//   (b) a chunk plan_round has marked tried_wg 2 never appears in by_wg again, and a chunk of by_wg whose re-run gave up is in by_general
//       the next time it fails;
//   (c) by_wg is empty whenever wg is off and whenever neither in-place nor lone holds, in_place is false once ex_off has been set, and
//       ex_off is set exactly when, of this round's chunks with tried_wg 1, more than a quarter gave up;
//   (d) the pending list is ascending, contains every re-run chunk, and a chunk that was not re-run exactly when the chunk before it is
//       pending and every chunk between it and the nearest re-run chunk below it is "not full";
//   (e) the sequence ends within 2 * nch + 2 rounds, the bound the host enforces;
// and the hand-written cases hold: two waves of failures, the lone thresholds, the exactness guard at its boundaries;
//   (f) the guard's constant against fp64 itself (sum_model): operand sets that span 52 bits sum to one value in 1 000 random orders and
//       count as exact, sets that span 53 do not count as exact and a fixed-seed search finds one with two orders that differ.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <vector>

#include "../../usrp_nfc_amd/csrc/rerun_plan.h"

using namespace nfc;
typedef std::vector<uint32_t> List;

static int fail(const char *what, const char *detail = "") {
    printf("rerun_plan_check: %s%s\n", what, detail);
    return 1;
}
#define CHECK(cond, what)                          \
    do {                                           \
        if (!(cond)) return fail(what, ": " #cond); \
    } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() {   // (xorshift64*)
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    }
    bool chance(uint32_t per_256) { return (next() & 255u) < per_256; }
};

static bool ascending(const List &l) {
    for (size_t i = 1; i < l.size(); i++)
        if (l[i] <= l[i - 1]) return false;
    return true;
}
static bool has(const List &l, uint32_t k) { return std::binary_search(l.begin(), l.end(), k); }

// the device as the plan sees it, and what the checker remembers of a sequence
struct Model {
    uint32_t nch;
    std::vector<uint8_t> cert, gflags;
    std::vector<uint8_t> eval_ok;      // the chunk's latest evaluation started from the final state of its predecessor
    std::vector<uint8_t> is_final;     // certified, and so is everything before it
    std::vector<uint8_t> rerun_ever;   // the checker's own account of (a)
    std::vector<uint8_t> barred;       // tried_wg was seen at 2
    std::vector<uint8_t> wg_ever;      // the chunk has been in by_wg
    std::vector<uint8_t> owes_general; // by_wg's re-run gave up: by_general the next time it fails
};

// one round's plan against the properties (a) .. (c); `before`: the failing list as failing_of left it
static int check_round(const RerunPolicy &p, const RerunBook &b, const RerunRound &r, const List &before, const std::vector<uint8_t> &tried_before,
                       bool ex_off_before, Model &m) {
    // (a)
    CHECK(ascending(r.by_wg) && ascending(r.by_general), "(a) a list is not ascending");
    List taken;
    std::merge(r.by_wg.begin(), r.by_wg.end(), r.by_general.begin(), r.by_general.end(), std::back_inserter(taken));
    CHECK(ascending(taken), "(a) by_wg and by_general overlap");
    CHECK(taken == b.failing, "(a) the book's list is not the union");
    CHECK(!taken.empty() && taken[0] == before[0], "(a) the smallest failing chunk was not taken");
    for (uint32_t k : taken) CHECK(has(before, k), "(a) a chunk that did not fail was taken");
    for (uint32_t k : before) {
        if (has(taken, k)) continue;
        CHECK(!(m.gflags[k] & 4), "(a) a chunk that gave up was left out");
        CHECK(!m.rerun_ever[k], "(a) a chunk that had been re-run was left out");
        CHECK(k > 0 && has(taken, k - 1), "(a) a chunk was left out that is not right behind a taken one");
    }
    // (b)
    for (uint32_t k : r.by_wg) CHECK(!m.barred[k], "(b) a chunk went back to the workgroup kernel");
    for (uint32_t k : taken) {
        if (m.owes_general[k]) CHECK(has(r.by_general, k), "(b) a chunk the workgroup kernel gave up is not k_threshold's");
        m.owes_general[k] = 0;
    }
    for (uint32_t k = 0; k < m.nch; k++)
        if (b.tried_wg[k] == 2) m.barred[k] = 1;
    // (... which is what becomes of a chunk that k_threshold takes after the workgroup kernel has had it, gave up or not)
    for (uint32_t k : r.by_general) CHECK(!m.wg_ever[k] || b.tried_wg[k] == 2, "(b) a chunk k_threshold took from the workgroup kernel is not marked");
    for (uint32_t k : r.by_wg) m.wg_ever[k] = 1;
    // (c)
    size_t ran = 0, gave = 0;
    for (uint32_t k : taken)
        if (tried_before[k] == 1) ran++, gave += (m.gflags[k] & 4) ? 1 : 0;
    CHECK(b.ex_off == (ex_off_before || gave * 4 > ran), "(c) ex_off");
    if (b.ex_off) CHECK(!r.in_place, "(c) in place after ex_off");
    CHECK(r.in_place == (p.in_place && !b.ex_off && taken.size() <= p.ex_max), "(c) in_place");
    const bool lone = p.rerun_lone && taken.size() <= p.lone_max && (uint64_t)taken.size() * p.lone_div <= (uint64_t)p.nch;
    if (!p.wg || (!r.in_place && !lone)) CHECK(r.by_wg.empty(), "(c) by_wg should be empty");
    return 0;
}

// (d): `ran` the re-run chunks, gflags as before the re-runs
static int check_pending(const List &pending, const List &ran, const Model &m) {
    CHECK(ascending(pending), "(d) not ascending");
    for (uint32_t k : ran) CHECK(has(pending, k), "(d) a re-run chunk is not pending");
    for (uint32_t k = 0; k < m.nch; k++) {
        if (has(ran, k)) continue;
        bool sees = false;
        for (uint32_t j = k; j-- > 0;) {   // the nearest re-run chunk below, through chunks that left slots untouched
            if (has(ran, j)) {
                sees = true;
                break;
            }
            if (!(m.gflags[j] & 2)) break;
        }
        CHECK(has(pending, k) == sees, "(d) a chunk that was not re-run");
        if (sees) CHECK(has(pending, k - 1), "(d) pending behind a chunk that is not");
    }
    return 0;
}

static int run_sequence(const RerunPolicy &p, RerunBook &b, Rng &g, int *rounds_max) {
    const uint32_t nch = p.nch;
    Model m;
    m.nch = nch;
    m.cert.assign(nch, 1);
    m.gflags.assign(nch, 0);
    m.eval_ok.assign(nch, 0);
    m.is_final.assign(nch, 0);
    m.rerun_ever.assign(nch, 0);
    m.barred.assign(nch, 0);
    m.wg_ever.assign(nch, 0);
    m.owes_general.assign(nch, 0);
    // pass 0: by a kernel that may give up (always where it is the workgroup form; never a batch of one chunk, which is k_threshold's
    // and has no round at all)
    const bool lean = nch >= 2 && (p.wg || g.chance(128));
    static const uint32_t FAIL[3] = {24, 128, 256}, GAVE[3] = {0, 64, 200}, OPEN[3] = {32, 128, 230};   // (chances in 256, drawn per sequence)
    const uint32_t p_fail = FAIL[g.next() % 3], p_gave = GAVE[g.next() % 3], p_open = OPEN[g.next() % 3];
    for (uint32_t k = 0; k < nch; k++) {
        const bool gave = lean && g.chance(p_gave);
        m.gflags[k] = (uint8_t)((gave ? 4 | 16 : 0) | (g.chance(p_open) ? 2 : 0));
        m.cert[k] = k == 0 ? !gave : !gave && !g.chance(p_fail);
        m.eval_ok[k] = k == 0 && !gave;
    }
    b.reset(nch);
    CHECK(b.pending.size() == nch - 1 && b.ver.size() == nch && !b.ex_off, "reset");
    bool first_round = true;
    int rounds = 0;
    while (!b.pending.empty()) {
        for (uint32_t k = 0; k < nch; k++) m.is_final[k] = m.cert[k] && (k == 0 || m.is_final[k - 1]);
        const List before = failing_of(b, first_round, lean, m.cert.data());
        CHECK(ascending(before), "failing_of: not ascending");
        for (uint32_t k = 0; k < nch; k++)
            CHECK(has(before, k) == (!m.cert[k] && (has(b.pending, k) || (k == 0 && first_round && lean))), "failing_of");
        if (before.empty()) break;
        first_round = false;
        const std::vector<uint8_t> tried_before = b.tried_wg.empty() ? std::vector<uint8_t>(nch, 0) : b.tried_wg;
        const bool ex_off_before = b.ex_off;
        const RerunRound r = plan_round(p, b, m.gflags.data());
        if (check_round(p, b, r, before, tried_before, ex_off_before, m)) return 1;
        const List ran = b.failing;
        const List pending = pending_after(b, nch, m.gflags.data());
        if (check_pending(pending, ran, m)) return 1;
        CHECK(++rounds <= 2 * (int)nch + 2, "(e) the rounds did not converge");
        // the re-runs ...
        for (uint32_t k : ran) {
            const bool gave = has(r.by_wg, k) && g.chance(p_gave);
            m.gflags[k] = (uint8_t)((gave ? 4 | 16 : 0) | (g.chance(p_open) ? 2 : 0));
            m.eval_ok[k] = !gave && (k == 0 || m.is_final[k - 1]);
            m.rerun_ever[k] = 1;
            if (gave) m.owes_general[k] = 1;
        }
        // ... and their certification, ascending: what started from a final predecessor's state and was not given up is proven
        for (uint32_t k = 0; k < nch; k++) {
            const bool pred_final = k == 0 || m.is_final[k - 1];
            if (has(pending, k)) {
                if (m.gflags[k] & 4) m.cert[k] = 0;
                else if (pred_final && m.eval_ok[k]) m.cert[k] = 1;
                else m.cert[k] = !g.chance(p_fail);
            }
            m.is_final[k] = m.cert[k] && pred_final;
        }
    }
    for (uint32_t k = 0; k < nch; k++) CHECK(m.cert[k], "a sequence ended with a chunk not certified");
    *rounds_max = std::max(*rounds_max, rounds);
    return 0;
}

static int hand_written() {
    RerunBook b;
    std::vector<uint8_t> cert(8, 0), gf(8, 0);
    const RerunPolicy general{false, false, true, 4, 64, 0, 8};
    // Two waves of failures.  Every chunk fails and none gave up: round 1 takes 0, 2, 4, 6, the chunks behind them wait ...
    b.reset(8);
    failing_of(b, true, true, cert.data());
    CHECK(b.failing == (List{0, 1, 2, 3, 4, 5, 6, 7}), "two waves: round 1 failing");
    plan_round(general, b, gf.data());
    CHECK(b.failing == (List{0, 2, 4, 6}) && b.by_wg.empty() && b.by_general == b.failing, "two waves: round 1 takes every other chunk");
    CHECK(pending_after(b, 8, gf.data()) == (List{0, 1, 2, 3, 4, 5, 6, 7}), "two waves: every chunk can see a re-run one");
    // ... and when all fail again, a chunk never re-run is still deferred behind a chunk that is taken
    failing_of(b, false, true, cert.data());
    plan_round(general, b, gf.data());
    CHECK(b.failing == (List{0, 2, 4, 6}), "two waves: a chunk never re-run still waits");
    // (the case that cost a pass when waiting was applied to chunks already re-run: every chunk gave up in pass 0, so round 1 takes them
    // all; all fail again, none having given up -- all are taken again, because ever_rerun stops the waiting: 2 general passes, not 3)
    b.reset(8);
    std::vector<uint8_t> gave(8, 4);
    failing_of(b, true, true, cert.data());
    plan_round(general, b, gave.data());
    CHECK(b.failing.size() == 8, "two waves: chunks that gave up do not wait");
    pending_after(b, 8, gave.data());
    failing_of(b, false, true, cert.data());
    CHECK(b.failing.size() == 8, "two waves: round 2 failing");
    plan_round(general, b, gf.data());
    CHECK(b.failing.size() == 8 && b.by_general.size() == 8, "two waves: re-run chunks do not wait");
    // ... while a chunk never re-run among them is still deferred: chunk 3 certified in pass 0's round and fails now
    b.reset(8);
    cert[3] = 1;
    failing_of(b, true, true, cert.data());
    plan_round(general, b, gave.data());
    CHECK(b.failing == (List{0, 1, 2, 4, 5, 6, 7}), "two waves: round 1 without chunk 3");
    pending_after(b, 8, gave.data());
    cert[3] = 0;
    failing_of(b, false, true, cert.data());
    plan_round(general, b, gf.data());
    CHECK(b.failing == (List{0, 1, 2, 4, 5, 6, 7}), "two waves: the one chunk never re-run waits");

    // The lone thresholds: at most 4 failures and at most one chunk in 64
    const auto lone_count = [&](uint32_t nch, const List &failing) {
        const RerunPolicy wg{true, false, true, 4, 64, 0, nch};
        std::vector<uint8_t> f(nch, 0);
        b.reset(nch);
        b.failing = failing;
        return plan_round(wg, b, f.data()).by_wg.size();
    };
    CHECK(lone_count(256, List{10, 20, 30, 40}) == 4, "lone: four failures in 256 chunks");
    CHECK(lone_count(256, List{10, 20, 30, 40, 50}) == 0, "lone: five failures");
    CHECK(lone_count(255, List{10, 20, 30, 40}) == 0, "lone: four failures in 255 chunks");

    // sums_exact: low = min(emin - 23, ss_emin), high = max(exponent field of vtop, ss_emax); exact when high - low <= 52
    const auto bits = [](float v) {
        uint32_t u;
        memcpy(&u, &v, 4);
        return u;
    };
    CHECK(sums_exact(255, 0, 100, 120, bits(4.f)), "sums_exact: high - low == 52");     // low 77, high 129
    CHECK(!sums_exact(255, 0, 100, 120, bits(8.f)), "sums_exact: high - low == 53");    // high 130
    CHECK(!sums_exact(255, 0, 99, 120, bits(8.f)) && sums_exact(255, 0, 101, 120, bits(8.f)), "sums_exact: emin moves low");
    CHECK(!sums_exact(76, 0, 100, 120, bits(4.f)) && sums_exact(77, 0, 100, 120, bits(4.f)), "sums_exact: ss_emin moves low");
    CHECK(sums_exact(255, 129, 100, 120, bits(1.f)) && !sums_exact(255, 130, 100, 120, bits(1.f)), "sums_exact: ss_emax moves high");
    CHECK(sums_exact(255, 0, 100, 254, bits(4.f)) && !sums_exact(255, 0, 100, 255, bits(4.f)), "sums_exact: emax == 255");
    CHECK(sums_exact(255, 0, 254, 254, 0u), "sums_exact: vtop 0");
    for (uint32_t bad : {0x7FC00000u, 0x7F800000u, 0xFF800000u, bits(-1.f)})   // NaN, +-Inf, negative: the worst case, 255 + 64
        CHECK(!sums_exact(255, 0, 254, 254, bad) && !sums_exact(254, 0, 254, 254, bad), "sums_exact: a vtop that is no bound");
    // the fold: one chunk alone breaks exactness -- by its bound, by its smallest value, by a value it cannot vouch for
    const uint8_t gmin[3] = {100, 100, 100}, gmax[3] = {120, 121, 119}, gfl[3] = {0, 2, 4}, gmin_low[3] = {100, 99, 100}, gfl_flag[3] = {0, 3, 4};
    const uint32_t vt[3] = {bits(4.f), bits(2.f), bits(7.5f)}, vt_high[3] = {bits(4.f), bits(8.f), bits(1.f)};
    SumBounds s = fold_sum_bounds(3, gmin, gmax, gfl, vt);
    CHECK(s.emin == 100 && s.emax == 121 && !s.flagged && s.vtop == bits(7.5f), "fold_sum_bounds");
    CHECK(sums_exact(255, 0, s.emin, s.emax, s.vtop), "fold: exact");
    s = fold_sum_bounds(3, gmin, gmax, gfl, vt_high);
    CHECK(s.vtop == bits(8.f) && !sums_exact(255, 0, s.emin, s.emax, s.vtop), "fold: one chunk's bound breaks exactness");
    s = fold_sum_bounds(3, gmin_low, gmax, gfl, vt);
    CHECK(s.emin == 99 && !sums_exact(255, 0, s.emin, s.emax, s.vtop), "fold: one chunk's smallest value breaks exactness");
    CHECK(fold_sum_bounds(3, gmin, gmax, gfl_flag, vt).flagged, "fold: flagged");
    s = fold_sum_bounds(0, gmin, gmax, gfl, vt);
    CHECK(s.emin == 255 && s.emax == 0 && !s.flagged && s.vtop == 0, "fold: no chunk");
    return 0;
}

// The constant of sums_exact against fp64 itself.  The documented rule: every operand a multiple of 2^low, no sum of them reaching
// 2^(low + 53).  Operand sets are drawn in units of 2^low (integers held in doubles, either sign, magnitudes from one unit to the whole
// budget), their absolute values adding up to less than the budget 2^(span + 1) -- so no partial sum of any order reaches it -- and to at
// least 2^span, so that the guard's `high - low` for the set is exactly `span` (high: the exponent of the bound the kernels would report,
// here the sum of the absolute values rounded up to a float).
//   span 52: sums_exact says exact, and 1 000 random orders of summation give one value, set after set;
//   span 53: sums_exact says not exact, and the search finds a set and two orders whose sums differ -- the guard could not say more.
static double sum_in_order(const std::vector<double> &v, const std::vector<uint32_t> &order) {
    volatile double s = 0;   // (one rounding per addition, whatever the optimiser would like)
    for (uint32_t i : order) s = s + v[i];
    return s;
}
static void shuffle(std::vector<uint32_t> &o, Rng &g) {
    for (size_t i = o.size(); i > 1; i--) std::swap(o[i - 1], o[g.next() % i]);
}
static std::vector<double> draw_operands(Rng &g, int span, double *abs_sum) {
    const double budget = std::ldexp(1.0, span + 1), floor_ = std::ldexp(1.0, span);
    for (;;) {
        std::vector<double> v;
        double used = 0;
        const uint32_t n = 2 + g.next() % 63;
        for (uint32_t i = 0; i < n; i++) {
            const int mag = (int)(g.next() % (uint32_t)(span + 1));   // the operand's own exponent: anywhere in the span
            const uint64_t mant = (((uint64_t)g.next() << 32) | g.next()) >> (63 - mag);   // up to mag + 1 bits: an integer below 2^(mag + 1)
            const double x = (double)(mant | 1u);
            if (used + x >= budget) continue;
            used += x;
            v.push_back((g.next() & 1u) ? -x : x);
        }
        if (used >= floor_ && used < budget && v.size() >= 2) {
            *abs_sum = used;
            return v;
        }
    }
}
static uint32_t float_bits_at_least(double x) {   // the smallest float >= x: what an upper bound kept in a float looks like
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static int sum_model() {
    Rng g{0xD1B54A32D192ED03ull};
    const int low = 60;   // exponent-field scale of the unit (any value: the rule is about differences)
    // span 52
    int checked = 0;
    for (int set = 0; set < 40; set++) {
        double used;
        const std::vector<double> v = draw_operands(g, 52, &used);
        const uint32_t vtop = float_bits_at_least(std::ldexp(used, low - 127));
        float vt;
        memcpy(&vt, &vtop, 4);
        if (std::ilogb((double)vt) + 127 - low != 52) continue;   // (the bound rounded up into the next binade: the guard sees 53, rightly cautious)
        CHECK(sums_exact(255, 0, low + 23, low + 23 + 52, vtop), "sum model: span 52 must count as exact");
        CHECK(sums_exact(low, 0, 254, 254, vtop) && sums_exact(low, low + 52, 254, 254, 0u), "sum model: span 52 through the carried sum");
        std::vector<uint32_t> order(v.size());
        for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
        const double first = sum_in_order(v, order);
        for (int k = 0; k < 1000; k++) {
            shuffle(order, g);
            CHECK(sum_in_order(v, order) == first, "sum model: span 52, two orders of summation differ");
        }
        checked++;
    }
    CHECK(checked >= 30, "sum model: span 52, fewer than 30 of the 40 operand sets were checked");
    // span 53
    bool found = false;
    for (int set = 0; set < 4000 && !found; set++) {
        double used;
        const std::vector<double> v = draw_operands(g, 53, &used);
        const uint32_t vtop = float_bits_at_least(std::ldexp(used, low - 127));
        CHECK(!sums_exact(255, 0, low + 23, low + 23 + 52, vtop), "sum model: span 53 must not count as exact");
        std::vector<uint32_t> order(v.size());
        for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
        const double first = sum_in_order(v, order);
        for (int k = 0; k < 50 && !found; k++) {
            shuffle(order, g);
            found = sum_in_order(v, order) != first;
        }
    }
    CHECK(found, "sum model: span 53, no operand set with two orders that differ was found");
    return 0;
}

int main() {
    Rng g{0x9E3779B97F4A7C15ull};
    RerunBook b;   // (one book for every sequence, as the context keeps one for every batch)
    long sequences = 0;
    int rounds_max = 0;
    for (int wg = 0; wg < 2; wg++)
        for (int in_place = 0; in_place < 2; in_place++)
            for (int rerun_lone = 0; rerun_lone < 2; rerun_lone++)
                for (int ex = 0; ex < 3; ex++)
                    for (int lo = 0; lo < 3; lo++)
                        for (uint32_t nch = 1; nch <= 12; nch++) {
                            const size_t lone_max[3] = {4, 4, 0};
                            const uint64_t lone_div[3] = {64, 1, 1};
                            const size_t ex_max[3] = {0, 2, nch};
                            const RerunPolicy p{wg != 0, in_place != 0, rerun_lone != 0, lone_max[lo], lone_div[lo], ex_max[ex], nch};
                            for (int i = 0; i < 250; i++, sequences++)   // (3 000 per policy)
                                if (run_sequence(p, b, g, &rounds_max)) {
                                    printf("  wg %d in_place %d rerun_lone %d ex_max %zu lone %zu/%llu nch %u, sequence %d\n", wg, in_place, rerun_lone,
                                           ex_max[ex], lone_max[lo], (unsigned long long)lone_div[lo], nch, i);
                                    return 1;
                                }
                        }
    if (hand_written()) return 1;
    if (sum_model()) return 1;
    printf("rerun_plan_check: %ld sequences (%d rounds at most), the hand-written cases and the exactness guard: every property held\n", sequences, rounds_max);
    return 0;
}
