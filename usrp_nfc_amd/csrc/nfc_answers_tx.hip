// nfc_answers_tx.hip -- the CPU twin of nfc_multi_transmit_device (include/nfc_amd.h: nfc_host_answers_tx; answers_tx.hip.h, DESIGN.md
// 8m) in a translation unit of its own, so that tools/answers_tx_check can build it stand-alone under a sanitizer.  The device call is
// the multi-stream context's (nfc_multi.hip); both run schedule_stream and index the one table of run counts.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"
#include "answers_tx.hip.h"

namespace nfc {
void note_call_error(const char *text);   // nfc_amd.hip: what nfc_last_error(NULL) returns

namespace atx {
namespace {
int fail(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    note_call_error(buf);
    return NFC_ERR_ARG;
}

struct HostSrc {
    const nfc_tx_answer *ans;
    const uint8_t *a, *p;
    uint64_t idx(uint32_t j) const { return ans[j].idx; }
    uint32_t n_bits(uint32_t j) const { return ans[j].n_bits; }
    const uint8_t *air(uint32_t j) const { return a + ans[j].byte_off; }
    const uint8_t *par(uint32_t j) const { return p + ans[j].byte_off; }
};

// k_answers_tx_render's sample with the angle in double: within 1.5e-7 of amp of the device's
void put(float *out, uint64_t at, const Consts &C, uint64_t t, float lvl) {
    float re = lvl, im = 0.f;
    if (C.carrier) {
        const uint64_t ph = (C.first_index + t) * C.phase_inc;
        const double turn = (double)(uint32_t)(ph >> 40) * 5.9604644775390625e-08;
        const float cs = (float)cos(2.0 * M_PI * turn), sn = (float)sin(2.0 * M_PI * turn);
        re = lvl * (C.amp * cs);
        im = lvl * (C.amp * sn);
    }
    out[2 * at] = re, out[2 * at + 1] = im;
}
}  // namespace
}  // namespace atx
}  // namespace nfc

using namespace nfc;

extern "C" int nfc_host_answers_tx(const nfc_answers_tx_config *cfg, size_t K, const int32_t *role, const uint64_t *rx_base, const uint32_t *rx_n,
                                   const uint32_t *ans_off, const nfc_tx_answer *answers, const uint8_t *air_bytes, const uint8_t *par,
                                   const uint32_t *byte_base, nfc_tx_pending *pending, void *out, size_t cap_samples, uint64_t *first_sample,
                                   uint32_t *n_samples) {
    char msg[256];
    if (atx::config_fault(cfg, msg, sizeof msg)) return atx::fail("%s", msg);
    if (K > 65536) return atx::fail("K exceeds 65536");
    if (K == 0) return NFC_OK;
    if (!role || !rx_base || !rx_n || !ans_off || !byte_base || !pending || !first_sample || !n_samples)
        return atx::fail("role, rx_base, rx_n, ans_off, byte_base, pending, first_sample or n_samples is null");
    if (ans_off[0] != 0 || byte_base[0] != 0) return atx::fail("ans_off[0] and byte_base[0] must be 0");
    for (size_t k = 0; k < K; k++) {
        if (ans_off[k + 1] < ans_off[k]) return atx::fail("ans_off[%zu] is below the entry before it", k + 1);
        if (byte_base[k + 1] < byte_base[k]) return atx::fail("byte_base[%zu] is below the entry before it", k + 1);
        if (role[k] < -1 || role[k] > 1) return atx::fail("role[%zu] is none of -1, NFC_EMU_TAG, NFC_EMU_READER", k);
    }
    if (ans_off[K] && !answers) return atx::fail("answers is null");
    if (byte_base[K] && (!air_bytes || !par)) return atx::fail("air or par is null");
    for (size_t k = 0; k < K; k++) {
        const uint32_t part = byte_base[k + 1] - byte_base[k];
        for (uint32_t j = ans_off[k]; j < ans_off[k + 1]; j++) {
            const nfc_tx_answer &a = answers[j];
            if (!atx::n_bits_ok(a.n_bits)) return atx::fail("answers[%u].n_bits %u is neither 1 .. 8 nor a multiple of 9 up to %u", j, a.n_bits, atx::MAX_BITS);
            const uint32_t nb = air::frame_bytes(a.n_bits);
            if (a.byte_off > part || nb > part - a.byte_off)
                return atx::fail("answers[%u].byte_off: the answer's %u bytes leave stream %zu's part of air / par (%u bytes)", j, nb, k, part);
        }
        const nfc_tx_pending &p = pending[k];
        if (p.n_bits && (!atx::n_bits_ok(p.n_bits) || p.role > 1)) return atx::fail("pending[%zu]: n_bits %u or role %u outside the domain", k, p.n_bits, p.role);
    }
    const atx::Consts C = atx::make_consts(*cfg);
    // the layout
    std::vector<uint64_t> t0(K);
    uint64_t at = 0, need = 0;
    for (size_t k = 0; k < K; k++) {
        t0[k] = atx::tx_index(C, rx_base[k]);
        const uint64_t n = role[k] < 0 ? 0ull : atx::tx_index(C, rx_base[k] + rx_n[k]) - t0[k];
        if (n > atx::MAX_SPAN) return atx::fail("stream %zu: a span of %llu samples exceeds 2^30", k, (unsigned long long)n);
        first_sample[k] = at;
        n_samples[k] = (uint32_t)n;
        need = at + n;
        at += air::align_up(n, C.align);
    }
    if (!out) return NFC_OK;   // the sizing call
    if (need > cap_samples) return atx::fail("cap_samples: the layout needs %llu samples, %zu do not hold them", (unsigned long long)need, cap_samples);
    float *o = (float *)out;
    std::vector<atx::Span> spans;
    std::vector<uint32_t> ends(atx::MAX_RUNS);
    for (size_t k = 0; k < K; k++) {
        const uint64_t f0 = first_sample[k], n = n_samples[k];
        if (role[k] >= 0) {
            const uint32_t na = ans_off[k + 1] - ans_off[k];
            spans.assign((size_t)na + 1, atx::Span{});
            const atx::HostSrc src = {answers + ans_off[k], air_bytes + byte_base[k], par + byte_base[k]};
            const uint32_t ns = atx::schedule_stream(C, (uint32_t)role[k], t0[k], (uint32_t)n, pending + k, na, src, spans.data(), na + 1);
            const float idle = role[k] == NFC_EMU_READER ? 1.f : 0.f;
            uint64_t r = 0;   // the next sample of the span
            for (uint32_t j = 0; j < ns; j++) {
                const atx::Span &s = spans[j];
                for (; r < s.lo; r++) atx::put(o, f0 + r, C, t0[k] + r, idle);
                // the answer's run ends from its pieces, as the render kernel makes them
                const air::Bits B = {s.air, s.par, s.n_bits};
                const uint32_t np = air::n_pieces(s.role, s.n_bits);
                uint32_t pos = 0;
                for (uint32_t q = 0; q < np; q++) {
                    const air::Piece P = air::piece_of(C.pieces, s.role, B, q);
                    ends[2 * q] = ((pos + P.ca) << 1) | P.la;
                    ends[2 * q + 1] = ((pos + P.ca + P.cb) << 1) | P.lb;
                    pos += P.ca + P.cb;
                }
                for (; r < s.hi; r++) {
                    const uint32_t p = (uint32_t)((int64_t)r - s.s_rel);
                    uint32_t run = atx::find_run(ends.data(), 2 * np, p);
                    run = run < 2 * np ? run : 2 * np - 1;
                    atx::put(o, f0 + r, C, t0[k] + r, (float)(ends[run] & 1u));
                }
            }
            for (; r < n; r++) atx::put(o, f0 + r, C, t0[k] + r, idle);
        }
        if (k + 1 < K)   // the padding up to the next stream
            for (uint64_t g = f0 + n; g < first_sample[k + 1]; g++) o[2 * g] = 0.f, o[2 * g + 1] = 0.f;
    }
    return NFC_OK;
}
