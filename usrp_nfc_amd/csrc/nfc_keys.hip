// nfc_keys.hip -- the host side of the key recovery (keys.hip.h states the method and holds the kernels, DESIGN.md 8h the layout):
// nfc_find_auths picks the first authentications out of a stream's frames, nfc_host_recover_keys is the CPU twin (sort and search for the
// join), nfc_recover_keys_device batches the traces, reads the exact counts, places every trace's table in the scratch and launches.
// The capacity rules live in ONE place (plan_batch) that both use, so their statuses and statistics agree by construction.
// Both searches are stated once over a list of RECORDS (keys::Prepared): host_search and device_search.  A first authentication is one
// record; a nested one is up to 64, one per candidate nonce -- virtual traces -- which k_nested_candidates writes on the
// device and nested_records lists on the host, and reduce_nested folds a nested trace's verdicts into its one result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/nfc_amd.h"
#include "launch_check.h"
#include "dev_buf.h"
#include "keys.hip.h"

static_assert(sizeof(nfc_auth_trace) == 40 && sizeof(nfc_key_result) == 24 && sizeof(nfc_key_config) == 32 && sizeof(nfc_key_stats) == 56,
              "the key recovery's public structures");
static_assert(sizeof(nfc_nested_trace) == 40 && sizeof(nfc_nested_result) == 48 && sizeof(nfc_nested_config) == 48,
              "the nested key recovery's public structures");
static_assert(sizeof(nfc_reader_pair) == 80 && sizeof(nfc_reader_key_result) == 32 && sizeof(nfc_reader_key_config) == 48,
              "the reader-pair key recovery's public structures");
static_assert(sizeof(nfc::keys::Prepared) == 48, "a record is twelve words");
static_assert(sizeof(nfc::keys::PairRecord) == 72, "a pair record is eighteen words");

namespace {
using namespace nfc;
using namespace nfc::keys;

constexpr uint64_t DEFAULT_INITIAL = 1ull << 26, DEFAULT_MAX = 1ull << 28, LIMIT_MAX = 1ull << 32;
constexpr uint32_t DEFAULT_BATCH = 16, LIMIT_BATCH = 4096;
constexpr uint32_t DEFAULT_STAGE = 1u << 18, LIMIT_STAGE = 1u << 24;   // joined candidates per pair (reader pairs: DESIGN.md 8n)

struct Limits {
    uint64_t initial, max;
    uint32_t max_batch;
    bool timing;
    uint32_t stage = DEFAULT_STAGE;   // reader pairs only: 0 verifies in the walking lane
};
bool limits_of(const nfc_key_config *c, Limits &L) {
    L = Limits{DEFAULT_INITIAL, DEFAULT_MAX, DEFAULT_BATCH, false, DEFAULT_STAGE};
    if (!c) return true;
    if (c->reserved[0] || c->reserved[1] || (c->flags & ~(uint32_t)NFC_KEY_TIMING)) return false;
    if (c->max_capacity) L.max = c->max_capacity;
    if (c->initial_capacity) L.initial = c->initial_capacity;
    else L.initial = std::min(L.initial, L.max);
    if (c->max_batch) L.max_batch = c->max_batch;
    L.timing = (c->flags & NFC_KEY_TIMING) != 0;
    return L.max <= LIMIT_MAX && L.initial <= L.max && L.max_batch <= LIMIT_BATCH;
}

// One batch: every trace's table from its exact odd count; a trace whose table alone passes `max` overflows; the others go, in order,
// into groups whose tables together fit `max`.
struct Group {
    uint32_t t0, t1;   // traces [t0, t1) of the batch (overflowed ones among them take no part)
    uint64_t slots;
};
struct Plan {
    std::vector<uint32_t> log2;   // 0: overflow
    std::vector<uint64_t> off;    // within its group
    std::vector<Group> groups;
};
Plan plan_batch(const uint32_t *n_odd, uint32_t nb, uint64_t max) {
    Plan p;
    p.log2.assign(nb, 0);
    p.off.assign(nb, 0);
    Group g{0, 0, 0};
    for (uint32_t i = 0; i < nb; i++) {
        const uint32_t l = table_log2(n_odd[i]);
        const uint64_t size = 1ull << l;
        if (size > max) {
            g.t1 = i + 1;
            continue;
        }
        if (g.slots + size > max) {
            g.t1 = i;
            p.groups.push_back(g);
            g = Group{i, i, 0};
        }
        p.log2[i] = l;
        p.off[i] = g.slots;
        g.slots += size;
        g.t1 = i + 1;
    }
    if (g.slots) p.groups.push_back(g);
    return p;
}
// the scratch follows the groups: it grows to fit one that needs more
void account(const Plan &p, uint64_t &capacity, nfc_key_stats &S) {
    for (const Group &g : p.groups)
        if (g.slots > capacity) capacity = g.slots, S.n_grown++;
}

// what the search says of one record
struct Verdict {
    bool overflow;
    uint32_t n_found, n_odd, n_even;
    uint64_t min_key;
    uint32_t n_joined;   // equal signatures.  Only the PAIR kind reports it: the twin counts it for both kinds (it costs nothing there),
                         // the kernels only where Kind::PAIR, and result_of, the full search's, never reads it
};

void result_of(nfc_key_result &r, const Verdict &v, const Prepared &P) {
    memset(&r, 0, sizeof r);
    r.n_odd = v.n_odd, r.n_even = v.n_even;
    if (v.overflow) {
        r.status = NFC_KEY_OVERFLOW;
        return;
    }
    r.n_candidates = v.n_found;
    r.status = v.n_found == 0 ? NFC_KEY_NONE : v.n_found == 1 ? NFC_KEY_OK : NFC_KEY_AMBIGUOUS;
    if (v.n_found) {
        for (int i = 0; i < 6; i++) r.key[i] = (uint8_t)(v.min_key >> (8 * i));
        (void)verify(v.min_key, P, &r.nr);
    }
}

// ---- the CPU twin over records of a kind: record_of(v) -> Kind::Record, sink(v, verdict, record) ----
template <class Kind, class RecordOf, class Sink>
void host_search(const Limits &L, nfc_key_stats &S, size_t nv, RecordOf &&record_of, Sink &&sink) {
    uint64_t capacity = L.initial;
    std::vector<std::pair<uint64_t, uint64_t>> odd;   // (signature, sequence)
    std::vector<uint32_t> n_odd;
    for (size_t b0 = 0; b0 < nv; b0 += L.max_batch) {
        const uint32_t nb = (uint32_t)std::min<size_t>(L.max_batch, nv - b0);
        n_odd.assign(nb, 0);
        for (uint32_t i = 0; i < nb; i++) {
            const typename Kind::Record R = record_of(b0 + i);
            const Prepared &P = Kind::base(R);
            odd.clear();
            for (uint32_t w = 0; w < WINDOWS; w++)
                walk<Kind::DEPTH>(w, P.ks_odd, [&](uint64_t seq) { odd.emplace_back(signature<0, Kind::NREL>(seq), seq); });
            n_odd[i] = (uint32_t)odd.size();
            Verdict V{(1ull << table_log2(odd.size())) > L.max, 0u, n_odd[i], 0u, ~0ull, 0u};
            if (!V.overflow) std::sort(odd.begin(), odd.end());
            for (uint32_t w = 0; w < WINDOWS; w++)
                V.n_even += walk<Kind::DEPTH>(w, P.ks_even, [&](uint64_t seq) {
                    if (V.overflow) return;
                    const uint64_t sig = signature<1, Kind::NREL>(seq);
                    for (auto it = std::lower_bound(odd.begin(), odd.end(), std::make_pair(sig, (uint64_t)0)); it != odd.end() && it->first == sig; ++it) {
                        V.n_joined++;
                        const uint64_t key = rollback(join_state(it->second, seq), P);
                        if (Kind::check(key, R)) {
                            if (V.n_found != 0xFFFFFFFFu) V.n_found++;
                            V.min_key = std::min(V.min_key, key);
                        }
                    }
                });
            sink(b0 + i, V, R);
        }
        account(plan_batch(n_odd.data(), nb, L.max), capacity, S);
        S.n_batches++;
    }
    S.scratch_bytes = nv ? capacity * 16 : 0;
}

// ---- the device search over records ----
// prelude(D) runs once the device is set and the events exist: it may allocate and launch (D.timed), and leaves D.nv, the number of
// records, and -- where they already lie on the device -- D.d_records with D.map, the place of record v in it.  Without d_records the
// batch's records, record_of(v), are uploaded.  sink(v, verdict, record) sees every record in order.
struct DeviceSearch {
    const Limits &L;
    nfc_key_stats &S;
    int rc = NFC_OK;
    Event e0, e1;
    size_t nv = 0;
    const Prepared *d_records = nullptr;
    const uint32_t *map = nullptr;   // [nv], the host's
    double ms_prelude = 0;
    std::vector<DevBuf> owned;   // device memory of the prelude's, released with the search

    bool bad(hipError_t e, int status = NFC_ERR_DEVICE) {
        if (e == hipSuccess) return false;
        rc = (e == hipErrorOutOfMemory) ? NFC_ERR_NOMEM : status;
        return true;
    }
    template <class T>
    bool alloc(T *&p, size_t bytes) {
        DevBuf b;
        if (bad(b.ensure(bytes ? bytes : 1))) return false;
        p = b.as<T>();
        owned.push_back(std::move(b));
        return true;
    }
    // one launch, timed by HIP events when asked
    template <class Launch>
    bool timed(double &ms, Launch &&launch) {
        if (L.timing && bad(hipEventRecord(e0, 0))) return false;
        launch_error() = LaunchError{};
        launch();
        S.n_launches++;
        if (bad(launch_error().err)) return false;
        if (L.timing) {
            float t = 0.f;
            if (bad(hipEventRecord(e1, 0)) || bad(hipEventSynchronize(e1)) || bad(hipEventElapsedTime(&t, e0, e1))) return false;
            ms += t;
        }
        return true;
    }
};

// A kind whose probe STAGES (reader pairs with L.stage > 0) has besides a section of L.stage words per trace of the batch, and a verify
// launch after every probe launch; both count in ms_probe.
template <class Kind, class Prelude, class RecordOf, class Sink>
int device_search(int device, const Limits &L, nfc_key_stats &S, Prelude &&prelude, RecordOf &&record_of, Sink &&sink) {
    using Record = typename Kind::Record;
    if (hipSetDevice(device) != hipSuccess) return NFC_ERR_DEVICE;
    DeviceSearch D{L, S};
    DevBuf small_buf, scratch, stage_buf;
    const bool staged = Kind::PAIR && L.stage > 0;
    uint64_t capacity = L.initial;
    auto bad = [&](hipError_t e) { return D.bad(e); };
    const bool searched = [&] {   // (false: it ended before there was anything to search; D.rc holds the status)
        if (L.timing && (bad(D.e0.create()) || bad(D.e1.create()))) return false;
        if (!prelude(D) || D.nv == 0) return false;
        const size_t nv = D.nv;
        const uint32_t mb = (uint32_t)std::min<size_t>(L.max_batch, nv);
        // the small per-batch arrays in one allocation:
        // prep | place | counts [2 mb] | n_found [mb] | n_joined [mb] | err [1] (padded) | min_key [mb] | map [mb]
        const size_t o_place = sizeof(Record) * mb, o_counts = o_place + sizeof(Place) * mb, o_found = o_counts + 8 * (size_t)mb,
                     o_joined = o_found + 4 * (size_t)mb, o_err = o_joined + 4 * (size_t)mb, o_min = (o_err + 4 + 7) & ~(size_t)7,
                     o_map = o_min + 8 * (size_t)mb, small_bytes = o_map + 4 * (size_t)mb;
        static_assert(sizeof(Record) % 8 == 0, "place, an array of 64-bit words, follows the records");
        if (bad(small_buf.ensure(small_bytes)) || bad(scratch.ensure(capacity * 16))) return true;
        if (staged && bad(stage_buf.ensure(8 * (size_t)L.stage * mb))) return true;
        uint8_t *const small = small_buf.as<uint8_t>();
        Record *d_prep = (Record *)small;
        Place *d_place = (Place *)(small + o_place);
        uint32_t *d_counts = (uint32_t *)(small + o_counts), *d_found = (uint32_t *)(small + o_found), *d_err = (uint32_t *)(small + o_err);
        uint32_t *d_joined = (uint32_t *)(small + o_joined);
        unsigned long long *d_min = (unsigned long long *)(small + o_min);
        uint32_t *d_map_buf = (uint32_t *)(small + o_map);
        uint64_t *d_stage = staged ? stage_buf.as<uint64_t>() : nullptr;
        const Record *k_prep = D.d_records ? reinterpret_cast<const Record *>(D.d_records) : d_prep;   // (only the full kind's prelude leaves records)
        const uint32_t *k_map = D.d_records ? d_map_buf : nullptr;
        const dim3 block(KEYS_BLOCK);
        std::vector<Record> prep(mb);
        std::vector<Place> place(mb);
        std::vector<uint32_t> counts(2 * (size_t)mb), n_odd(mb), found(mb), joined(mb);
        std::vector<uint64_t> min_key(mb);
        for (size_t b0 = 0; b0 < nv && D.rc == NFC_OK; b0 += mb) {
            const uint32_t nb = (uint32_t)std::min<size_t>(mb, nv - b0);
            for (uint32_t i = 0; i < nb; i++) prep[i] = record_of(b0 + i);
            // the batch's records, or where they lie; counts, found and err to 0, min_key to all ones
            if (D.d_records ? bad(hipMemcpy(d_map_buf, D.map + b0, 4 * (size_t)nb, hipMemcpyHostToDevice))
                            : bad(hipMemcpy(d_prep, prep.data(), sizeof(Record) * nb, hipMemcpyHostToDevice)))
                return true;
            if (bad(hipMemsetAsync(d_counts, 0, o_min - o_counts, 0)) || bad(hipMemsetAsync(d_min, 0xFF, 8 * (size_t)mb, 0))) return true;
            if (!D.timed(S.ms_count, [&] { NFC_LAUNCH(k_keys_count<Kind>, dim3(WINDOWS / KEYS_BLOCK, 2, nb), block, 0, 0, k_prep, k_map, d_counts); })) return true;
            if (bad(hipMemcpy(counts.data(), d_counts, 8 * (size_t)nb, hipMemcpyDeviceToHost))) return true;   // (waits for the launch)
            for (uint32_t i = 0; i < nb; i++) n_odd[i] = counts[2 * i];
            const Plan plan = plan_batch(n_odd.data(), nb, L.max);
            for (const Group &g : plan.groups) {
                if (g.slots > capacity) {   // grow to fit: the old tables are not needed
                    scratch.release();
                    capacity = g.slots;
                    S.n_grown++;
                    if (bad(scratch.ensure(capacity * 16))) return true;
                }
                for (uint32_t i = 0; i < nb; i++) {
                    const bool in = i >= g.t0 && i < g.t1 && plan.log2[i];
                    place[i] = Place{in ? plan.off[i] : 0, in ? plan.log2[i] : 0u, 0u};
                }
                uint64_t *sig_tab = scratch.as<uint64_t>(), *seq_tab = sig_tab + capacity;
                if (bad(hipMemcpy(d_place, place.data(), sizeof(Place) * nb, hipMemcpyHostToDevice)) ||
                    bad(hipMemsetAsync(sig_tab, 0xFF, g.slots * 8, 0)))
                    return true;
                const dim3 grid(WINDOWS / KEYS_BLOCK, 1, g.t1 - g.t0);
                if (!D.timed(S.ms_fill, [&] { NFC_LAUNCH(k_keys_fill_odd<Kind>, grid, block, 0, 0, k_prep, k_map, d_place, g.t0, sig_tab, seq_tab, d_err); }))
                    return true;
                bool probed = false;
                if constexpr (Kind::PAIR) if (staged) {
                    probed = true;
                    // the verify grid: a lane per place of the stage, at most VERIFY_BLOCKS workgroups per trace (they stride)
                    constexpr uint32_t VERIFY_BLOCKS = 1024;
                    const dim3 vgrid(std::min<uint32_t>((L.stage + KEYS_BLOCK - 1) / KEYS_BLOCK, VERIFY_BLOCKS), 1, g.t1 - g.t0);
                    if (!D.timed(S.ms_probe, [&] {
                            NFC_LAUNCH((k_keys_probe_even<Kind, true>), grid, block, 0, 0, k_prep, k_map, d_place, g.t0, sig_tab, seq_tab, d_found, d_min,
                                       d_joined, d_stage, L.stage);
                        }) ||
                        !D.timed(S.ms_probe, [&] {
                            NFC_LAUNCH(k_keys_verify_stage<Kind>, vgrid, block, 0, 0, k_prep, k_map, d_place, g.t0, d_joined, d_stage, L.stage, d_found, d_min);
                        }))
                        return true;
                }
                if (!probed && !D.timed(S.ms_probe, [&] {
                        NFC_LAUNCH((k_keys_probe_even<Kind, false>), grid, block, 0, 0, k_prep, k_map, d_place, g.t0, sig_tab, seq_tab, d_found, d_min,
                                   d_joined, d_stage, 0u);
                    }))
                    return true;
                if (bad(hipStreamSynchronize(0))) return true;   // (the next group rewrites d_place and the tables)
            }
            uint32_t err = 0;
            if (bad(hipMemcpy(found.data(), d_found, 4 * (size_t)nb, hipMemcpyDeviceToHost)) ||
                bad(hipMemcpy(joined.data(), d_joined, 4 * (size_t)nb, hipMemcpyDeviceToHost)) ||
                bad(hipMemcpy(min_key.data(), d_min, 8 * (size_t)nb, hipMemcpyDeviceToHost)) || bad(hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost)))
                return true;
            if (err) {
                D.rc = NFC_ERR_INTERNAL;
                return true;
            }
            for (uint32_t i = 0; i < nb; i++) sink(b0 + i, Verdict{plan.log2[i] == 0, found[i], counts[2 * i], counts[2 * i + 1], min_key[i], joined[i]}, prep[i]);
            S.n_batches++;
        }
        return true;
    }();
    S.ms_kernels = S.ms_count + S.ms_fill + S.ms_probe + D.ms_prelude;
    S.scratch_bytes = searched ? capacity * 16 : 0;
    return D.rc;
}

// ---- nested authentications ----
struct NestedLimits {
    Limits search;
    uint32_t first, count;   // count 0: all from first
};
bool nested_limits_of(const nfc_nested_config *c, NestedLimits &N) {
    N.first = N.count = 0;
    if (!c) return limits_of(nullptr, N.search);
    if (!limits_of(&c->search, N.search) || c->cand_first > NESTED_CANDS || c->reserved[0] || c->reserved[1]) return false;
    N.first = c->cand_first, N.count = c->cand_count;
    return true;
}
// the window of a trace with n_nt candidates: [first, end)
uint32_t window_end(const NestedLimits &N, uint32_t n_nt) {
    if (N.first >= n_nt) return N.first;
    return N.count ? (uint32_t)std::min<uint64_t>((uint64_t)N.first + N.count, n_nt) : n_nt;
}
// the records of one trace in ascending seed order, at most NESTED_CANDS (the kernel's rule) -> how many
uint32_t nested_records(const nfc_nested_trace &t, uint32_t parent, Prepared *out) {
    uint32_t n = 0;
    for (uint32_t seed = 0; seed < NESTED_SEEDS; seed++) {
        Prepared P;
        if (nested_candidate(t, parent, seed, P) && n < NESTED_CANDS) out[n++] = P;
    }
    return n;
}
// One nested trace's result from the verdicts of its searched candidates, in candidate order: the sums, the lowest key and its nt.
struct NestedFold {
    nfc_nested_result r;
    uint64_t min_key = ~0ull;
    bool overflow = false;
    Prepared best;
    explicit NestedFold(uint32_t n_nt) {
        memset(&r, 0, sizeof r);
        r.n_nt = n_nt;
    }
    void add(const Verdict &v, const Prepared &P) {
        r.n_searched++;
        r.n_odd += v.n_odd, r.n_even += v.n_even;
        if (v.overflow) {
            overflow = true;
            return;
        }
        r.n_verified = (uint32_t)std::min<uint64_t>((uint64_t)r.n_verified + v.n_found, 0xFFFFFFFFull);
        if (v.n_found && v.min_key < min_key) min_key = v.min_key, best = P;
    }
    nfc_nested_result done() {
        r.status = overflow ? NFC_KEY_OVERFLOW : r.n_verified == 0 ? NFC_KEY_NONE : r.n_verified == 1 ? NFC_KEY_OK : NFC_KEY_AMBIGUOUS;
        if (r.n_verified) {
            for (int i = 0; i < 6; i++) r.key[i] = (uint8_t)(min_key >> (8 * i));
            r.nt = best.nt;
            (void)verify(min_key, best, &r.nr);
        }
        return r;
    }
};
// `records` [n][NESTED_CANDS] and n_nt [n] -> the virtual traces of the windows, in order: their places in `records`
std::vector<uint32_t> virtual_traces(const NestedLimits &N, const uint32_t *n_nt, size_t n) {
    std::vector<uint32_t> map;
    for (size_t p = 0; p < n; p++)
        for (uint32_t c = N.first; c < window_end(N, n_nt[p]); c++) map.push_back((uint32_t)(p * NESTED_CANDS + c));
    return map;
}
// the folds of all traces, fed by either search's sink in virtual-trace order
struct NestedFolds {
    std::vector<NestedFold> f;
    NestedFolds(const uint32_t *n_nt, size_t n) {
        f.reserve(n);
        for (size_t p = 0; p < n; p++) f.emplace_back(n_nt[p]);
    }
    void add(uint32_t place, const Verdict &v, const Prepared &P) { f[place / NESTED_CANDS].add(v, P); }
    void done(nfc_nested_result *out) {
        for (size_t p = 0; p < f.size(); p++) out[p] = f[p].done();
    }
};
// the candidate launch for all traces; the records stay on the device (d_rec) and come down once, with the counts, for the host's side
bool launch_candidates(DeviceSearch &D, const nfc_nested_trace *traces, size_t n, Prepared *&d_rec, std::vector<Prepared> &rec, uint32_t *n_nt) {
    nfc_nested_trace *d_traces = nullptr;
    uint32_t *d_n = nullptr;   // [n] counts, then the error word
    rec.resize(n * NESTED_CANDS);
    if (!D.alloc(d_traces, sizeof(nfc_nested_trace) * n) || !D.alloc(d_rec, sizeof(Prepared) * rec.size()) || !D.alloc(d_n, 4 * (n + 1))) return false;
    if (D.bad(hipMemcpy(d_traces, traces, sizeof(nfc_nested_trace) * n, hipMemcpyHostToDevice)) ||
        D.bad(hipMemsetAsync(d_rec, 0, sizeof(Prepared) * rec.size(), 0)) || D.bad(hipMemsetAsync(d_n, 0, 4 * (n + 1), 0)))
        return false;
    if (!D.timed(D.ms_prelude, [&] { NFC_LAUNCH(k_nested_candidates, dim3((uint32_t)n), dim3(NESTED_BLOCK), 0, 0, d_traces, d_rec, d_n, d_n + n); }))
        return false;
    uint32_t err = 0;
    if (D.bad(hipMemcpy(n_nt, d_n, 4 * n, hipMemcpyDeviceToHost)) || D.bad(hipMemcpy(&err, d_n + n, 4, hipMemcpyDeviceToHost)) ||
        D.bad(hipMemcpy(rec.data(), d_rec, sizeof(Prepared) * rec.size(), hipMemcpyDeviceToHost)))
        return false;
    if (err) D.rc = NFC_ERR_INTERNAL;
    for (size_t p = 0; p < n; p++) n_nt[p] = std::min<uint32_t>(n_nt[p], NESTED_CANDS);
    return !err;
}
constexpr size_t NESTED_MAX_TRACES = (1ull << 32) / NESTED_CANDS;   // a record's place is 32 bits

bool key_type_ok(const nfc_auth_trace &t) { return t.key_type == 0x60 || t.key_type == 0x61; }

// nfc_find_auths (with_at) and nfc_find_reader_auths (without: the fourth frame is not looked at, at_enc and its ninth bits stay 0)
int find_first_auths(bool with_at, const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                     const uint8_t *par1, nfc_auth_trace *out, size_t cap, size_t *n_out) {
    const size_t tail = with_at ? 3 : 2;   // frames after the AUTH
    if (!n_out || (n && !frames) || (cap && !out)) return NFC_ERR_ARG;
    *n_out = 0;
    for (size_t i = 0; i < n; i++)
        if (frames[i].type != 0 && frames[i].type != 1) return NFC_ERR_ARG;
    auto bytes_of = [&](const nfc_raw_frame &r) { return (r.type ? bytes1 : bytes0) + r.byte_off; };
    auto par_of = [&](const nfc_raw_frame &r) { return (r.type ? par1 : par0) + r.byte_off; };
    auto is = [&](size_t i, int type, uint32_t n_bytes, uint32_t need) {
        const nfc_raw_frame &r = frames[i];
        if (r.type != type || (r.flags & NFC_RAW_CUT) || r.n_bytes != n_bytes || (r.flags & need) != need) return false;
        return (r.type ? bytes1 && par1 : bytes0 && par0);
    };
    auto word = [](const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; };
    bool have_uid = false;
    uint32_t uid = 0;
    size_t found = 0;
    for (size_t i = 0; i < n; i++) {
        if (is(i, 1, 9, NFC_RAW_CRC_A_OK)) {
            const uint8_t *b = bytes_of(frames[i]);
            if (b[0] == 0x93 && b[1] == 0x70) have_uid = true, uid = word(b + 2);
            continue;
        }
        if (!have_uid || i + tail >= n || !is(i, 1, 4, NFC_RAW_CRC_A_OK)) continue;
        const uint8_t *a = bytes_of(frames[i]);
        if (a[0] != 0x60 && a[0] != 0x61) continue;
        if (!is(i + 1, 0, 4, NFC_RAW_PARITY_OK) || !is(i + 2, 1, 8, 0) || (with_at && !is(i + 3, 0, 4, 0))) continue;
        if (found < cap) {
            nfc_auth_trace &t = out[found];
            memset(&t, 0, sizeof t);
            const uint8_t *rb = bytes_of(frames[i + 2]), *rp = par_of(frames[i + 2]);
            t.uid = uid;
            t.nt = word(bytes_of(frames[i + 1]));
            t.nr_enc = word(rb);
            t.ar_enc = word(rb + 4);
            for (int k = 0; k < 8; k++) t.par |= (uint16_t)((rp[k] & 1u) << k);
            if (with_at) {
                const uint8_t *tp = par_of(frames[i + 3]);
                t.at_enc = word(bytes_of(frames[i + 3]));
                for (int k = 0; k < 4; k++) t.par |= (uint16_t)((tp[k] & 1u) << (8 + k));
            }
            t.key_type = a[0];
            t.block = a[1];
            t.frame = (uint32_t)i;
            t.idx = frames[i].idx;
        }
        found++;
    }
    *n_out = found;
    return NFC_OK;
}

// ---- reader pairs ----
bool pair_limits_of(const nfc_reader_key_config *c, Limits &L) {
    if (!c) return limits_of(nullptr, L);
    if (!limits_of(&c->search, L) || (c->flags & ~(uint32_t)NFC_RKEY_VERIFY_INLINE) || c->reserved[0] || c->reserved[1] || c->stage_capacity > LIMIT_STAGE)
        return false;
    if (c->stage_capacity) L.stage = c->stage_capacity;
    if (c->flags & NFC_RKEY_VERIFY_INLINE) L.stage = 0;
    return true;
}
bool pairs_ok(const nfc_reader_pair *pairs, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!key_type_ok(pairs[i].search) || !key_type_ok(pairs[i].check)) return false;
    return true;
}
void pair_result_of(nfc_reader_key_result &r, const Verdict &v, const PairRecord &R) {
    memset(&r, 0, sizeof r);
    r.n_odd = v.n_odd, r.n_even = v.n_even;
    if (v.overflow) {
        r.status = NFC_KEY_OVERFLOW;
        return;
    }
    r.n_candidates = v.n_found, r.n_joined = v.n_joined;
    r.status = v.n_found == 0 ? NFC_KEY_NONE : v.n_found == 1 ? NFC_KEY_OK : NFC_KEY_AMBIGUOUS;
    if (v.n_found) {
        for (int i = 0; i < 6; i++) r.key[i] = (uint8_t)(v.min_key >> (8 * i));
        (void)verify_pair(v.min_key, R, &r.nr_search, &r.nr_check);
    }
}

}  // namespace

extern "C" {

int nfc_find_auths(const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1,
                   nfc_auth_trace *out, size_t cap, size_t *n_out) {
    return find_first_auths(true, frames, n, bytes0, par0, bytes1, par1, out, cap, n_out);
}

int nfc_find_reader_auths(const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                          const uint8_t *par1, nfc_auth_trace *out, size_t cap, size_t *n_out) {
    return find_first_auths(false, frames, n, bytes0, par0, bytes1, par1, out, cap, n_out);
}

int nfc_host_recover_reader_keys(const nfc_reader_pair *pairs, size_t n, const nfc_reader_key_config *cfg, nfc_reader_key_result *out,
                                 nfc_key_stats *stats) {
    Limits L;
    if (!pair_limits_of(cfg, L) || (n && (!pairs || !out)) || !pairs_ok(pairs, n)) return NFC_ERR_ARG;
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    host_search<PairKind>(L, S, n, [&](size_t v) { return prepare_pair(pairs[v]); },
                          [&](size_t v, const Verdict &V, const PairRecord &R) { pair_result_of(out[v], V, R); });
    if (stats) *stats = S;
    return NFC_OK;
}

int nfc_recover_reader_keys_device(int device, const nfc_reader_pair *pairs, size_t n, const nfc_reader_key_config *cfg,
                                   nfc_reader_key_result *out, nfc_key_stats *stats) {
    Limits L;
    if (!pair_limits_of(cfg, L) || (n && (!pairs || !out)) || device < 0 || !pairs_ok(pairs, n)) return NFC_ERR_ARG;
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    if (stats) *stats = S;
    if (n == 0) return NFC_OK;
    const int rc = device_search<PairKind>(
        device, L, S,
        [&](DeviceSearch &D) {
            D.nv = n;
            return true;
        },
        [&](size_t v) { return prepare_pair(pairs[v]); }, [&](size_t v, const Verdict &V, const PairRecord &R) { pair_result_of(out[v], V, R); });
    if (stats) *stats = S;
    return rc;
}

int nfc_host_recover_keys(const nfc_auth_trace *traces, size_t n, const nfc_key_config *cfg, nfc_key_result *out, nfc_key_stats *stats) {
    Limits L;
    if (!limits_of(cfg, L) || (n && (!traces || !out))) return NFC_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!key_type_ok(traces[i])) return NFC_ERR_ARG;
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    host_search<FullKind>(L, S, n, [&](size_t v) { return prepare(traces[v]); }, [&](size_t v, const Verdict &V, const Prepared &P) { result_of(out[v], V, P); });
    if (stats) *stats = S;
    return NFC_OK;
}

int nfc_recover_keys_device(int device, const nfc_auth_trace *traces, size_t n, const nfc_key_config *cfg, nfc_key_result *out,
                            nfc_key_stats *stats) {
    Limits L;
    if (!limits_of(cfg, L) || (n && (!traces || !out)) || device < 0) return NFC_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!key_type_ok(traces[i])) return NFC_ERR_ARG;
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    if (stats) *stats = S;
    if (n == 0) return NFC_OK;
    const int rc = device_search<FullKind>(
        device, L, S,
        [&](DeviceSearch &D) {
            D.nv = n;
            return true;
        },
        [&](size_t v) { return prepare(traces[v]); }, [&](size_t v, const Verdict &V, const Prepared &P) { result_of(out[v], V, P); });
    if (stats) *stats = S;
    return rc;
}

int nfc_find_nested_auths(const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                          const uint8_t *par1, nfc_nested_trace *out, size_t cap, size_t *n_out) {
    if (!n_out || (n && !frames) || (cap && !out)) return NFC_ERR_ARG;
    *n_out = 0;
    for (size_t i = 0; i < n; i++)
        if (frames[i].type != 0 && frames[i].type != 1) return NFC_ERR_ARG;
    auto bytes_of = [&](const nfc_raw_frame &r) { return (r.type ? bytes1 : bytes0) + r.byte_off; };
    auto par_of = [&](const nfc_raw_frame &r) { return (r.type ? par1 : par0) + r.byte_off; };
    auto is = [&](size_t i, int type, uint32_t n_bytes, uint32_t need) {
        const nfc_raw_frame &r = frames[i];
        if (r.type != type || (r.flags & NFC_RAW_CUT) || r.n_bytes != n_bytes || (r.flags & need) != need) return false;
        return (r.type ? bytes1 && par1 : bytes0 && par0);
    };
    auto word = [](const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; };
    bool have_uid = false, session = false;   // session: a first authentication of this UID was seen
    uint32_t uid = 0;
    size_t found = 0;
    for (size_t i = 0; i < n; i++) {
        if (is(i, 1, 9, NFC_RAW_CRC_A_OK)) {
            const uint8_t *b = bytes_of(frames[i]);
            if (b[0] == 0x93 && b[1] == 0x70) have_uid = true, session = false, uid = word(b + 2);
            continue;
        }
        if (!have_uid || i + 3 >= n || !is(i, 1, 4, 0)) continue;
        const uint8_t *a = bytes_of(frames[i]);
        const bool plain = (frames[i].flags & NFC_RAW_CRC_A_OK) && (a[0] == 0x60 || a[0] == 0x61);
        if (plain) {   // nfc_find_auths' rule
            if (is(i + 1, 0, 4, NFC_RAW_PARITY_OK) && is(i + 2, 1, 8, 0) && is(i + 3, 0, 4, 0)) session = true;
            continue;
        }
        if (!session || !is(i + 1, 0, 4, 0) || !is(i + 2, 1, 8, 0) || !is(i + 3, 0, 4, 0)) continue;
        if (found < cap) {
            nfc_nested_trace &t = out[found];
            memset(&t, 0, sizeof t);
            const uint8_t *rb = bytes_of(frames[i + 2]), *rp = par_of(frames[i + 2]), *tp = par_of(frames[i + 3]), *np = par_of(frames[i + 1]);
            t.uid = uid;
            t.nt_enc = word(bytes_of(frames[i + 1]));
            t.nr_enc = word(rb);
            t.ar_enc = word(rb + 4);
            t.at_enc = word(bytes_of(frames[i + 3]));
            for (int k = 0; k < 8; k++) t.par |= (uint16_t)((rp[k] & 1u) << k);
            for (int k = 0; k < 4; k++) t.par |= (uint16_t)((tp[k] & 1u) << (8 + k));
            for (int k = 0; k < 4; k++) t.par |= (uint16_t)((np[k] & 1u) << (12 + k));
            t.key_type = 0;
            t.block = 0xFF;
            t.frame = (uint32_t)i;
            t.idx = frames[i].idx;
        }
        found++;
    }
    *n_out = found;
    return NFC_OK;
}

int nfc_host_nested_candidates(const nfc_nested_trace *trace, uint32_t *out_nt, size_t cap, size_t *n_out) {
    if (!trace || !n_out || (cap && !out_nt)) return NFC_ERR_ARG;
    Prepared rec[NESTED_CANDS];
    const uint32_t n = nested_records(*trace, 0, rec);
    for (uint32_t i = 0; i < n && i < cap; i++) out_nt[i] = rec[i].nt;
    *n_out = n;
    return NFC_OK;
}

int nfc_nested_candidates_device(int device, const nfc_nested_trace *traces, size_t n, uint32_t *out_nt, uint32_t *out_n) {
    if ((n && (!traces || !out_nt || !out_n)) || device < 0 || n > NESTED_MAX_TRACES) return NFC_ERR_ARG;
    if (n == 0) return NFC_OK;
    Limits L;
    (void)limits_of(nullptr, L);
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    std::vector<Prepared> rec;
    return device_search<FullKind>(
        device, L, S,
        [&](DeviceSearch &D) {   // the prelude alone: no record is searched
            Prepared *d_rec = nullptr;
            if (!launch_candidates(D, traces, n, d_rec, rec, out_n)) return false;
            for (size_t i = 0; i < rec.size(); i++) out_nt[i] = rec[i].nt;
            return true;
        },
        [&](size_t) { return Prepared{}; }, [&](size_t, const Verdict &, const Prepared &) {});
}

int nfc_host_recover_nested_keys(const nfc_nested_trace *traces, size_t n, const nfc_nested_config *cfg, nfc_nested_result *out,
                                 nfc_key_stats *stats) {
    NestedLimits N;
    if (!nested_limits_of(cfg, N) || (n && (!traces || !out)) || n > NESTED_MAX_TRACES) return NFC_ERR_ARG;
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    std::vector<Prepared> rec(n * NESTED_CANDS);
    std::vector<uint32_t> n_nt(n);
    for (size_t p = 0; p < n; p++) n_nt[p] = nested_records(traces[p], (uint32_t)p, rec.data() + p * NESTED_CANDS);
    const std::vector<uint32_t> map = virtual_traces(N, n_nt.data(), n);
    NestedFolds folds(n_nt.data(), n);
    host_search<FullKind>(N.search, S, map.size(), [&](size_t v) { return rec[map[v]]; }, [&](size_t v, const Verdict &V, const Prepared &P) { folds.add(map[v], V, P); });
    folds.done(out);
    if (stats) *stats = S;
    return NFC_OK;
}

int nfc_recover_nested_keys_device(int device, const nfc_nested_trace *traces, size_t n, const nfc_nested_config *cfg, nfc_nested_result *out,
                                   nfc_key_stats *stats) {
    NestedLimits N;
    if (!nested_limits_of(cfg, N) || (n && (!traces || !out)) || device < 0 || n > NESTED_MAX_TRACES) return NFC_ERR_ARG;
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    if (stats) *stats = S;
    if (n == 0) return NFC_OK;
    std::vector<Prepared> rec;   // the device's records, read back for the fold (key -> nt, nr); never sent up
    std::vector<uint32_t> n_nt(n), map;
    std::vector<NestedFolds> folds;   // (made once n_nt is known)
    const int rc = device_search<FullKind>(
        device, N.search, S,
        [&](DeviceSearch &D) {
            Prepared *d_rec = nullptr;
            if (!launch_candidates(D, traces, n, d_rec, rec, n_nt.data())) return false;
            map = virtual_traces(N, n_nt.data(), n);
            D.map = map.data(), D.nv = map.size(), D.d_records = d_rec;
            folds.emplace_back(n_nt.data(), n);
            return true;
        },
        [&](size_t v) { return rec[map[v]]; }, [&](size_t v, const Verdict &V, const Prepared &P) { folds[0].add(map[v], V, P); });
    if (rc == NFC_OK && !folds.empty()) folds[0].done(out);
    if (stats) *stats = S;
    return rc;
}

}  // extern "C"
