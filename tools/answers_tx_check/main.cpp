// answers_tx_check -- the host twin of the answers' transmission (include/nfc_amd.h: nfc_host_answers_tx; csrc/answers_tx.hip.h, DESIGN.md
// 8m) over answers made here: ragged streams with a cardless and an empty one among them, answers of every n_bits in both roles, pushes
// cut at every position class (inside an answer, at its S, at S + L, at S + L - 1, between idx and S, a zero-length push, a push of one
// sample, one answer across three pushes), and pending entries given by hand over pushes of a few hundred samples (carried through many
// pushes, waiting in front of one, ended before one, cut away by a command) -- rendered into heap blocks of EXACTLY the size the sizing call reports, so that a sample
// written past the layout's end, or a bit read past an answer's bytes, is a sanitizer finding.  A stand-alone host program: the way to
// run the twin's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined tools/answers_tx_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_answers_tx.hip -o answers_tx_check && ./answers_tx_check
// It touches no GPU.  Exit status 0: every rendering fits its block to the byte; the pieces' concatenation is the whole, the final
// pending entry none; a buffer one sample short is refused, nothing written and no pending entry advanced; every argument error is
// NFC_ERR_ARG with the argument's name.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nfc_amd.h"

static std::string g_error;
namespace nfc {
void note_call_error(const char *text) { g_error = text; }   // (the library's is in nfc_amd.hip, behind nfc_last_error)
}

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

struct Stream {
    int32_t role;
    std::vector<nfc_tx_answer> ans;   // idx absolute, byte_off in the stream's own bytes
    std::vector<uint8_t> air, par;
    uint64_t total;                   // received samples in all
    void answer(uint64_t idx, uint32_t n_bits, uint32_t &seed) {
        const uint32_t nb = n_bits <= 8 ? 1 : n_bits / 9;
        ans.push_back(nfc_tx_answer{idx, (uint32_t)air.size(), n_bits});
        for (uint32_t i = 0; i < nb; i++) air.push_back((uint8_t)(lcg(seed) >> 24)), par.push_back((uint8_t)(lcg(seed) >> 31));
    }
};

// one push: stream k receives [base[k], base[k] + n[k]); the answers whose idx lies in it are the push's.  The rendering in a block of
// exactly the reported size, appended per stream to out[k]; false on any failure.
static bool push(const std::vector<Stream> &S, const nfc_answers_tx_config &c, const std::vector<uint64_t> &base, const std::vector<uint32_t> &n,
                 std::vector<nfc_tx_pending> &pend, std::vector<std::vector<float>> &out) {
    const size_t K = S.size();
    std::vector<int32_t> role(K);
    std::vector<uint32_t> ans_off(K + 1, 0), byte_base(K + 1, 0);
    std::vector<nfc_tx_answer> ans;
    std::vector<uint8_t> air, par;
    for (size_t k = 0; k < K; k++) {
        role[k] = S[k].role;
        for (const nfc_tx_answer &a : S[k].ans)
            if (a.idx >= base[k] && a.idx < base[k] + n[k]) ans.push_back(a);
        air.insert(air.end(), S[k].air.begin(), S[k].air.end()), par.insert(par.end(), S[k].par.begin(), S[k].par.end());
        ans_off[k + 1] = (uint32_t)ans.size(), byte_base[k + 1] = (uint32_t)air.size();
    }
    std::vector<uint64_t> first(K);
    std::vector<uint32_t> ns(K);
    const std::vector<nfc_tx_pending> before = pend;
    auto call = [&](void *o, size_t cap) {
        return nfc_host_answers_tx(&c, K, role.data(), base.data(), n.data(), ans_off.data(), ans.data(), air.data(), par.data(), byte_base.data(), pend.data(), o,
                                   cap, first.data(), ns.data());
    };
    if (call(nullptr, 0) != NFC_OK || memcmp(before.data(), pend.data(), K * sizeof(nfc_tx_pending))) return false;   // sizing touches no pending entry
    const size_t need = (size_t)(first[K - 1] + ns[K - 1]);
    float *block = (float *)malloc(need * 8 + 1);   // (malloc, not a vector: the red zone starts at the last byte)
    bool ok = true;
    if (need) {   // one sample short: refused, nothing written, no pending entry advanced
        memset(block, 0x5A, need * 8);
        ok = call(block, need - 1) == NFC_ERR_ARG && g_error.find("cap_samples") != std::string::npos && !memcmp(before.data(), pend.data(), K * sizeof(nfc_tx_pending));
        for (size_t i = 0; i < need * 8; i++) ok = ok && ((uint8_t *)block)[i] == 0x5A;
    }
    ok = ok && call(block, need) == NFC_OK;
    for (size_t k = 0; ok && k < K; k++) {
        if (first[k] % c.align_samples) ok = false;
        out[k].insert(out[k].end(), block + 2 * first[k], block + 2 * (first[k] + ns[k]));
        const uint64_t end = k + 1 < K ? first[k + 1] : need;
        for (uint64_t g = first[k] + ns[k]; g < end; g++) ok = ok && block[2 * g] == 0.f && block[2 * g + 1] == 0.f;   // padding is (0, 0)
    }
    free(block);
    return ok;
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "answers_tx_check: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static nfc_answers_tx_config config(double rate, uint32_t num, uint32_t den, uint64_t delay, int carrier, uint32_t align) {
    nfc_answers_tx_config c;
    memset(&c, 0, sizeof c);
    c.samp_rate = rate, c.freq = 13.56e6, c.first_index = 1ull << 40, c.delay_samples = delay, c.rate_num = num, c.rate_den = den;
    c.carrier = carrier, c.amp = 0.5f, c.align_samples = align;
    return c;
}

int main() {
    uint32_t seed = 14443;
    // stream 0: a tag with every n_bits, 9 000 samples apart; 1: no card (its answers are nobody's); 2: a reader with every n_bits, closer
    // than its answers are long (cut); 3: a tag that hears nothing; 4: a reader with five answers
    std::vector<Stream> S(5);
    S[0].role = NFC_EMU_TAG, S[1].role = -1, S[2].role = NFC_EMU_READER, S[3].role = NFC_EMU_TAG, S[4].role = NFC_EMU_READER;
    std::vector<uint32_t> lens;
    for (uint32_t n = 1; n <= 8; n++) lens.push_back(n);
    for (uint32_t n = 9; n <= 162; n += 9) lens.push_back(n);
    uint64_t at = 500;
    for (uint32_t n : lens) S[0].answer(at, n, seed), at += 9000;
    S[0].total = at;
    S[1].answer(100, 18, seed), S[1].total = 4000;
    at = 10;
    for (uint32_t n : lens) S[2].answer(at, n, seed), at += 700;
    S[2].total = at + 9000;
    S[3].total = 12345;
    const uint32_t five[5] = {162, 7, 45, 81, 18};
    at = 1000;
    for (uint32_t n : five) S[4].answer(at, n, seed), at += 9000;
    S[4].total = at;
    int renders = 0;
    const struct { double rate; uint32_t num, den; } rates[] = {{2e6, 1, 1}, {5e6, 5, 2}, {0.8e6, 2, 5}, {13.56e6, 339, 50}};
    for (const auto &r : rates)
        for (int carrier = 0; carrier < 2; carrier++)
            for (uint32_t align : {1u, 64u}) {
                const uint64_t delay = 173;
                const nfc_answers_tx_config c = config(r.rate, r.num, r.den, delay, carrier, align);
                auto T = [&](uint64_t x) { return x * r.num / r.den; };
                auto rx_at = [&](uint64_t t) { return (t * r.den + r.num - 1) / r.num; };   // the first r with T(r) >= t
                const size_t K = S.size();
                std::vector<std::vector<float>> whole(K), parts(K);
                std::vector<nfc_tx_pending> pend(K), pend2(K);
                memset(pend.data(), 0, K * sizeof(nfc_tx_pending)), memset(pend2.data(), 0, K * sizeof(nfc_tx_pending));
                std::vector<uint64_t> base(K, 0);
                std::vector<uint32_t> n(K);
                for (size_t k = 0; k < K; k++) n[k] = (uint32_t)S[k].total;
                CHECK(push(S, c, base, n, pend, whole));
                for (size_t k = 0; k < K; k++) CHECK(pend[k].n_bits == 0 && whole[k].size() == (k == 1 ? 0 : 2 * T(S[k].total)));
                // in pieces: stream 4's first answer (162 bits) sets the cuts of every position class; the others are cut at the same r
                const uint64_t S0 = T(1000) + delay;
                const uint64_t L0 = (uint64_t)(3096.0 * r.rate / 2e6);   // (the answer's length within a percent: 164 pieces of 9.44 us)
                std::vector<uint64_t> cuts = {1001, rx_at(S0), rx_at(S0 + 10), rx_at(S0 + 10), rx_at(S0 + 10) + 1, rx_at(S0 + L0 / 2), 10001, 19001};
                // ... and a push boundary at every TX index within two percent of S + L: S + L - 1 and S + L are among them
                for (uint64_t e = S0 + L0 - L0 / 50; e <= S0 + L0 + L0 / 50; e++) cuts.push_back(rx_at(e));
                std::sort(cuts.begin(), cuts.end());
                uint64_t prev = 0;
                cuts.push_back(~0ull);
                for (uint64_t cut : cuts) {
                    for (size_t k = 0; k < K; k++) {
                        base[k] = std::min<uint64_t>(prev, S[k].total);
                        n[k] = (uint32_t)(std::min<uint64_t>(cut, S[k].total) - base[k]);
                    }
                    CHECK(push(S, c, base, n, pend2, parts));
                    prev = std::min<uint64_t>(cut, 1ull << 40);
                }
                for (size_t k = 0; k < K; k++) {
                    CHECK(parts[k].size() == whole[k].size());
                    CHECK(whole[k].empty() || memcmp(parts[k].data(), whole[k].data(), whole[k].size() * 4) == 0);
                    if (k != 1) CHECK(pend2[k].n_bits == 0 && pend2[k].start == 0);
                }
                renders++;
            }
    // pending entries given by hand (what nfc_multi_set_tx_state gives the device), over pushes of a few hundred samples (tests/
    // test_answers_tx_trips.py, scenarios 2 and 5): stream 0's entry of the longest shape is carried THROUGH pushes that bring no answer,
    // the same 64 bytes behind every one; stream 1's starts far behind the first pushes and waits untouched over idle samples; stream 2
    // is given one that ended before its push began, which is dropped; stream 3's starts behind the moment its only command closes, and
    // is cut away entirely by that command's answer
    int carried = 0, waited = 0;
    {
        std::vector<Stream> Q(4);
        Q[0].role = NFC_EMU_TAG, Q[1].role = NFC_EMU_READER, Q[2].role = NFC_EMU_TAG, Q[3].role = NFC_EMU_READER;
        const uint64_t cmd = 2500, delay = 173, future = 5000, away = 2600;
        Q[3].answer(cmd, 18, seed);
        const nfc_answers_tx_config c = config(2e6, 1, 1, delay, 0, 1);
        auto entry = [&](uint64_t start, uint32_t n_bits, uint32_t role) {
            nfc_tx_pending p;
            memset(&p, 0, sizeof p);
            p.start = start, p.n_bits = (uint16_t)n_bits, p.role = (uint8_t)role;
            for (uint32_t i = 0; i < (n_bits <= 8 ? 1 : n_bits / 9); i++) p.air[i] = (uint8_t)(lcg(seed) >> 24), p.par[i] = (uint8_t)(lcg(seed) >> 31);
            return p;
        };
        const size_t K = Q.size();
        std::vector<nfc_tx_pending> pend(K);
        memset(pend.data(), 0, K * sizeof(nfc_tx_pending));
        pend[0] = entry(37, 162, NFC_EMU_READER), pend[1] = entry(future, 45, NFC_EMU_TAG), pend[3] = entry(away, 27, NFC_EMU_READER);
        const nfc_tx_pending first0 = pend[0], first1 = pend[1], first3 = pend[3];
        std::vector<std::vector<float>> out(K);
        std::vector<uint64_t> base(K, 0);
        std::vector<uint32_t> n(K);
        bool dropped = false, cut_away = false;
        for (uint32_t p = 0; base[0] < 9000; p++) {
            for (size_t k = 0; k < K; k++) n[k] = 301 + 2 * ((37 * (uint32_t)k + 11 * p) % 100);
            const bool give = !dropped && base[2] > 400;   // an entry wholly in the past: [10, 10 + L) with L below 390 samples (11 pieces of 9.44 us)
            if (give) pend[2] = entry(10, 9, NFC_EMU_TAG);
            const size_t before2 = out[2].size(), before1 = out[1].size();
            CHECK(push(Q, c, base, n, pend, out));
            if (give) {
                CHECK(pend[2].n_bits == 0 && pend[2].start == 0);
                for (size_t i = before2; i < out[2].size(); i++) CHECK(out[2][i] == 0.f);
                dropped = true;
            }
            if (pend[0].n_bits) {
                CHECK(!memcmp(&pend[0], &first0, sizeof first0));
                carried++;
            }
            if (base[1] + n[1] <= future) {   // the span ends in front of the entry: untouched, every sample the reader's idle level
                CHECK(!memcmp(&pend[1], &first1, sizeof first1));
                for (size_t i = before1; i < out[1].size(); i += 2) CHECK(out[1][i] == 1.f && out[1][i + 1] == 0.f);
                waited++;
            }
            if (base[3] + n[3] <= cmd) CHECK(!memcmp(&pend[3], &first3, sizeof first3));
            else if (!cut_away) {   // the push that holds the command: the entry is gone, the command's own answer is what is pending
                CHECK(pend[3].start == cmd + delay && pend[3].n_bits == 18);
                cut_away = true;
            }
            for (size_t k = 0; k < K; k++) base[k] += n[k];
        }
        CHECK(carried >= 5 && waited >= 5 && dropped && cut_away);
        for (size_t k = 0; k < K; k++) CHECK(pend[k].n_bits == 0 && pend[k].start == 0 && out[k].size() == 2 * base[k]);
        // stream 3: idle up to the answer's start (the entry that was cut away owned [2600, 2673) and left no sample there)
        for (uint64_t t = 0; t < cmd + delay; t++) CHECK(out[3][2 * t] == 1.f);
        bool low = false;
        for (uint64_t t = cmd + delay; t < cmd + delay + 100; t++) low = low || out[3][2 * t] == 0.f;
        CHECK(low);   // (a Miller answer begins with a pause)
        // stream 1: idle up to the entry's start, then a tag's answer over the reader's idle level
        for (uint64_t t = 0; t < future; t++) CHECK(out[1][2 * t] == 1.f);
        low = false;
        for (uint64_t t = future; t < future + 100; t++) low = low || out[1][2 * t] == 0.f;
        CHECK(low);
    }
    // argument errors
    {
        const size_t K = S.size();
        std::vector<std::vector<float>> sink(K);
        std::vector<nfc_tx_pending> pend(K);
        memset(pend.data(), 0, K * sizeof(nfc_tx_pending));
        std::vector<uint64_t> base(K, 0);
        std::vector<uint32_t> n(K);
        for (size_t k = 0; k < K; k++) n[k] = (uint32_t)S[k].total;
        auto bad = [&](nfc_answers_tx_config c, const char *name) { return !push(S, c, base, n, pend, sink) && g_error.find(name) != std::string::npos; };
        nfc_answers_tx_config c = config(2e6, 1, 1, 0, 0, 8);
        c.rate_num = 0;
        CHECK(bad(c, "rate_num"));
        c = config(2e6, 1, 65537, 0, 0, 8);
        CHECK(bad(c, "rate_den"));
        c = config(0.0, 1, 1, 0, 0, 8);
        CHECK(bad(c, "samp_rate"));
        c = config(2e9, 1, 1, 0, 0, 8);
        CHECK(bad(c, "samp_rate"));
        c = config(2e6, 1, 1, 0, 0, 24);
        CHECK(bad(c, "align_samples"));
        c = config(2e6, 1, 1, 0, 0, 8);
        c.reserved[2] = 1;
        CHECK(bad(c, "reserved"));
        c = config(2e6, 1, 1, 0, 0, 8);
        std::vector<Stream> B = S;
        B[0].ans[3].n_bits = 10;
        std::swap(S, B);
        CHECK(bad(c, "n_bits"));
        S = B;
        B[4].ans[4].n_bits = 162;   // the stream's last answer: its bytes would come from beyond the stream's part
        std::swap(S, B);
        CHECK(bad(c, "byte_off"));
        std::swap(S, B);
        n[3] = (1u << 30) + 1;
        CHECK(bad(c, "span"));
    }
    printf("answers_tx_check ok: %d whole renderings and their pieces in blocks of the exact size, %zu streams; an entry carried through %d pushes, one waiting through %d\n",
           renders, S.size(), carried, waited);
    return 0;
}
