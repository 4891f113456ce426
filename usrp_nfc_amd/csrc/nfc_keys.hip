// nfc_keys.hip -- the host side of the key recovery (keys.hip.h states the method and holds the kernels, DESIGN.md 8h the layout):
// nfc_find_auths picks the first authentications out of a stream's frames, nfc_host_recover_keys is the CPU twin (sort and search for the
// join), nfc_recover_keys_device batches the traces, reads the exact counts, places every trace's table in the scratch and launches.
// The capacity rules live in ONE place (plan_batch) that both use, so their statuses and statistics agree by construction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/nfc_amd.h"
#include "launch_check.h"
#include "keys.hip.h"

static_assert(sizeof(nfc_auth_trace) == 40 && sizeof(nfc_key_result) == 24 && sizeof(nfc_key_config) == 32 && sizeof(nfc_key_stats) == 56,
              "the key recovery's public structures");

namespace {
using namespace nfc;
using namespace nfc::keys;

constexpr uint64_t DEFAULT_INITIAL = 1ull << 26, DEFAULT_MAX = 1ull << 28, LIMIT_MAX = 1ull << 32;
constexpr uint32_t DEFAULT_BATCH = 16, LIMIT_BATCH = 4096;

struct Limits {
    uint64_t initial, max;
    uint32_t max_batch;
    bool timing;
};
bool limits_of(const nfc_key_config *c, Limits &L) {
    L = Limits{DEFAULT_INITIAL, DEFAULT_MAX, DEFAULT_BATCH, false};
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

void result_of(nfc_key_result &r, bool overflow, uint32_t n_found, uint64_t min_key, uint32_t n_odd, uint32_t n_even, const Prepared &P) {
    memset(&r, 0, sizeof r);
    r.n_odd = n_odd, r.n_even = n_even;
    if (overflow) {
        r.status = NFC_KEY_OVERFLOW;
        return;
    }
    r.n_candidates = n_found;
    r.status = n_found == 0 ? NFC_KEY_NONE : n_found == 1 ? NFC_KEY_OK : NFC_KEY_AMBIGUOUS;
    if (n_found) {
        for (int i = 0; i < 6; i++) r.key[i] = (uint8_t)(min_key >> (8 * i));
        (void)verify(min_key, P, &r.nr);
    }
}

bool key_type_ok(const nfc_auth_trace &t) { return t.key_type == 0x60 || t.key_type == 0x61; }

}  // namespace

extern "C" {

int nfc_find_auths(const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1,
                   nfc_auth_trace *out, size_t cap, size_t *n_out) {
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
        if (!have_uid || i + 3 >= n || !is(i, 1, 4, NFC_RAW_CRC_A_OK)) continue;
        const uint8_t *a = bytes_of(frames[i]);
        if (a[0] != 0x60 && a[0] != 0x61) continue;
        if (!is(i + 1, 0, 4, NFC_RAW_PARITY_OK) || !is(i + 2, 1, 8, 0) || !is(i + 3, 0, 4, 0)) continue;
        if (found < cap) {
            nfc_auth_trace &t = out[found];
            memset(&t, 0, sizeof t);
            const uint8_t *rb = bytes_of(frames[i + 2]), *rp = par_of(frames[i + 2]), *tp = par_of(frames[i + 3]);
            t.uid = uid;
            t.nt = word(bytes_of(frames[i + 1]));
            t.nr_enc = word(rb);
            t.ar_enc = word(rb + 4);
            t.at_enc = word(bytes_of(frames[i + 3]));
            for (int k = 0; k < 8; k++) t.par |= (uint16_t)((rp[k] & 1u) << k);
            for (int k = 0; k < 4; k++) t.par |= (uint16_t)((tp[k] & 1u) << (8 + k));
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

int nfc_host_recover_keys(const nfc_auth_trace *traces, size_t n, const nfc_key_config *cfg, nfc_key_result *out, nfc_key_stats *stats) {
    Limits L;
    if (!limits_of(cfg, L) || (n && (!traces || !out))) return NFC_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!key_type_ok(traces[i])) return NFC_ERR_ARG;
    nfc_key_stats S;
    memset(&S, 0, sizeof S);
    uint64_t capacity = L.initial;
    std::vector<std::pair<uint64_t, uint64_t>> odd;   // (signature, sequence)
    std::vector<uint32_t> n_odd;
    for (size_t b0 = 0; b0 < n; b0 += L.max_batch) {
        const uint32_t nb = (uint32_t)std::min<size_t>(L.max_batch, n - b0);
        n_odd.assign(nb, 0);
        for (uint32_t i = 0; i < nb; i++) {
            const Prepared P = prepare(traces[b0 + i]);
            odd.clear();
            for (uint32_t w = 0; w < WINDOWS; w++) walk(w, P.ks_odd, [&](uint64_t seq) { odd.emplace_back(signature<0>(seq), seq); });
            n_odd[i] = (uint32_t)odd.size();
            const bool overflow = (1ull << table_log2(odd.size())) > L.max;
            if (!overflow) std::sort(odd.begin(), odd.end());
            uint32_t n_even = 0, n_found = 0;
            uint64_t min_key = ~0ull;
            for (uint32_t w = 0; w < WINDOWS; w++)
                n_even += walk(w, P.ks_even, [&](uint64_t seq) {
                    if (overflow) return;
                    const uint64_t sig = signature<1>(seq);
                    for (auto it = std::lower_bound(odd.begin(), odd.end(), std::make_pair(sig, (uint64_t)0)); it != odd.end() && it->first == sig; ++it) {
                        const uint64_t key = rollback(join_state(it->second, seq), P);
                        if (verify(key, P, nullptr)) {
                            if (n_found != 0xFFFFFFFFu) n_found++;
                            min_key = std::min(min_key, key);
                        }
                    }
                });
            result_of(out[b0 + i], overflow, n_found, min_key, n_odd[i], n_even, P);
        }
        account(plan_batch(n_odd.data(), nb, L.max), capacity, S);
        S.n_batches++;
    }
    S.scratch_bytes = n ? capacity * 16 : 0;
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
    if (hipSetDevice(device) != hipSuccess) return NFC_ERR_DEVICE;

    const uint32_t mb = (uint32_t)std::min<size_t>(L.max_batch, n);
    // the small per-batch arrays in one allocation: prep | place | counts [2 mb] | n_found [mb] | err [1] (padded) | min_key [mb]
    const size_t o_place = sizeof(Prepared) * mb, o_counts = o_place + sizeof(Place) * mb, o_found = o_counts + 8 * (size_t)mb,
                 o_err = o_found + 4 * (size_t)mb, o_min = (o_err + 4 + 7) & ~(size_t)7, small_bytes = o_min + 8 * (size_t)mb;
    uint8_t *small = nullptr;
    uint64_t *scratch = nullptr;
    uint64_t capacity = L.initial;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = NFC_OK;
    auto bad = [&](hipError_t e, int status = NFC_ERR_DEVICE) {
        if (e == hipSuccess) return false;
        rc = (e == hipErrorOutOfMemory) ? NFC_ERR_NOMEM : status;
        return true;
    };
    // one launch, timed by HIP events when asked
    auto timed = [&](double &ms, auto &&launch) {
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
    };
    std::vector<Prepared> prep(mb);
    std::vector<Place> place(mb);
    std::vector<uint32_t> counts(2 * (size_t)mb), n_odd(mb), found(mb);
    std::vector<uint64_t> min_key(mb);
    do {
        if (bad(hipMalloc((void **)&small, small_bytes)) || bad(hipMalloc((void **)&scratch, capacity * 16))) break;
        if (L.timing && (bad(hipEventCreate(&e0)) || bad(hipEventCreate(&e1)))) break;
        Prepared *d_prep = (Prepared *)small;
        Place *d_place = (Place *)(small + o_place);
        uint32_t *d_counts = (uint32_t *)(small + o_counts), *d_found = (uint32_t *)(small + o_found), *d_err = (uint32_t *)(small + o_err);
        unsigned long long *d_min = (unsigned long long *)(small + o_min);
        const dim3 block(KEYS_BLOCK);
        for (size_t b0 = 0; b0 < n && rc == NFC_OK; b0 += mb) {
            const uint32_t nb = (uint32_t)std::min<size_t>(mb, n - b0);
            for (uint32_t i = 0; i < nb; i++) prep[i] = prepare(traces[b0 + i]);
            // counts, found and err to 0, min_key to all ones
            if (bad(hipMemcpy(d_prep, prep.data(), sizeof(Prepared) * nb, hipMemcpyHostToDevice)) ||
                bad(hipMemsetAsync(d_counts, 0, o_min - o_counts, 0)) || bad(hipMemsetAsync(d_min, 0xFF, 8 * (size_t)mb, 0)))
                break;
            if (!timed(S.ms_count, [&] { NFC_LAUNCH(k_keys_count, dim3(WINDOWS / KEYS_BLOCK, 2, nb), block, 0, 0, d_prep, d_counts); })) break;
            if (bad(hipMemcpy(counts.data(), d_counts, 8 * (size_t)nb, hipMemcpyDeviceToHost))) break;   // (waits for the launch)
            for (uint32_t i = 0; i < nb; i++) n_odd[i] = counts[2 * i];
            const Plan plan = plan_batch(n_odd.data(), nb, L.max);
            for (const Group &g : plan.groups) {
                if (g.slots > capacity) {   // grow to fit: the old tables are not needed
                    (void)hipFree(scratch);
                    scratch = nullptr;
                    capacity = g.slots;
                    S.n_grown++;
                    if (bad(hipMalloc((void **)&scratch, capacity * 16))) break;
                }
                for (uint32_t i = 0; i < nb; i++) {
                    const bool in = i >= g.t0 && i < g.t1 && plan.log2[i];
                    place[i] = Place{in ? plan.off[i] : 0, in ? plan.log2[i] : 0u, 0u};
                }
                uint64_t *sig_tab = scratch, *seq_tab = scratch + capacity;
                if (bad(hipMemcpy(d_place, place.data(), sizeof(Place) * nb, hipMemcpyHostToDevice)) ||
                    bad(hipMemsetAsync(sig_tab, 0xFF, g.slots * 8, 0)))
                    break;
                const dim3 grid(WINDOWS / KEYS_BLOCK, 1, g.t1 - g.t0);
                if (!timed(S.ms_fill, [&] { NFC_LAUNCH(k_keys_fill_odd, grid, block, 0, 0, d_prep, d_place, g.t0, sig_tab, seq_tab, d_err); })) break;
                if (!timed(S.ms_probe, [&] { NFC_LAUNCH(k_keys_probe_even, grid, block, 0, 0, d_prep, d_place, g.t0, sig_tab, seq_tab, d_found, d_min); }))
                    break;
                if (bad(hipStreamSynchronize(0))) break;   // (the next group rewrites d_place and the tables)
            }
            if (rc != NFC_OK) break;
            uint32_t err = 0;
            if (bad(hipMemcpy(found.data(), d_found, 4 * (size_t)nb, hipMemcpyDeviceToHost)) ||
                bad(hipMemcpy(min_key.data(), d_min, 8 * (size_t)nb, hipMemcpyDeviceToHost)) || bad(hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost)))
                break;
            if (err) {
                rc = NFC_ERR_INTERNAL;
                break;
            }
            for (uint32_t i = 0; i < nb; i++) result_of(out[b0 + i], plan.log2[i] == 0, found[i], min_key[i], counts[2 * i], counts[2 * i + 1], prep[i]);
            S.n_batches++;
        }
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (scratch) (void)hipFree(scratch);
    if (small) (void)hipFree(small);
    S.ms_kernels = S.ms_count + S.ms_fill + S.ms_probe;
    S.scratch_bytes = capacity * 16;
    if (stats) *stats = S;
    return rc;
}

}  // extern "C"
