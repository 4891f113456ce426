// nfc_air.hip -- the air interface's translation unit: the launches of air.hip.h's kernels, their twin on the CPU, and the C ABI of the
// rendering (include/nfc_amd.h: nfc_air_frame, nfc_air_config, nfc_host_air_render, nfc_air_render_device).  DESIGN.md 8l.
//
// One call: check every argument on the host; upload the frames, their bytes and whose they are; k_air_layout (a workgroup per stream,
// a lane per frame) and k_air_starts (one workgroup) lay the streams out; the host reads the K starts and lengths back, and only when
// they fit the caller's buffer k_air_render (a workgroup per frame) writes it.  No run table goes through HBM: a frame's runs are made
// from its bits twice, counted in the layout and scanned into LDS in the renderer (dynamic LDS, sized to the call's longest frame).
//
// THE DEVICE BUFFER of one call, every section on 256 bytes: frames [F], frame_stream [F], frame_off [K + 1], byte_base [K + 1], air, par,
// stream_seeds [K] (when given), empty (the streams without a frame) -- the inputs -- and rel_start [F], n_stream [K], first_sample [K],
// n_samples [K] -- what the layout kernels write, each followed by GUARD_BYTES of the guard word, which the call checks at its end.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"
#include "air.hip.h"
#include "dev_buf.h"
#include "launch_check.h"

static_assert(sizeof(nfc_air_frame) == 16, "nfc_air_frame is 16 bytes");
static_assert(sizeof(nfc_air_config) == 72, "nfc_air_config is 72 bytes");

namespace nfc {
void note_call_error(const char *text);   // nfc_amd.hip: what nfc_last_error(NULL) returns

namespace air {

constexpr uint32_t GUARD_WORD = 0x5AFEC0DEu, GUARD_BYTES = 16;

inline int fail(int code, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    note_call_error(buf);
    return code;
}

inline bool kind_ok(uint32_t k) { return k == NFC_IN_IQ_F32 || k == NFC_IN_IQ_I16 || k == NFC_IN_IQ_I8 || k == NFC_IN_IQ_U8; }

// every argument of the two calls but the output; F: the frames in all
inline int args_fault(const nfc_air_config *cfg, const nfc_air_frame *frames, const uint32_t *frame_off, const uint8_t *air, const uint8_t *par,
                      const uint32_t *byte_base, size_t K, const uint64_t *first_sample, const uint32_t *n_samples) {
    if (!cfg) return fail(NFC_ERR_ARG, "cfg is null");
    if (!kind_ok(cfg->out_kind)) return fail(NFC_ERR_ARG, "cfg.out_kind %u is none of NFC_IN_IQ_F32, NFC_IN_IQ_I16, NFC_IN_IQ_I8, NFC_IN_IQ_U8", cfg->out_kind);
    if (cfg->align_samples == 0 || (cfg->align_samples & (cfg->align_samples - 1)) || cfg->align_samples > (1u << 20))
        return fail(NFC_ERR_ARG, "cfg.align_samples %u is no power of two up to 2^20", cfg->align_samples);
    if (!(cfg->rate_msps > 0) || !(cfg->rate_msps <= MAX_RATE_MSPS)) return fail(NFC_ERR_ARG, "cfg.rate_msps must be above 0 and at most %g", MAX_RATE_MSPS);
    if (!std::isfinite(cfg->carrier_i) || !std::isfinite(cfg->carrier_q) || !std::isfinite(cfg->depth) || !std::isfinite(cfg->full_scale))
        return fail(NFC_ERR_ARG, "cfg.carrier_i, carrier_q, depth and full_scale must be finite");
    if (!std::isfinite(cfg->sigma) || cfg->sigma < 0) return fail(NFC_ERR_ARG, "cfg.sigma must be finite and not negative");
    if (cfg->tail > MAX_STREAM_SAMPLES) return fail(NFC_ERR_ARG, "cfg.tail exceeds 2^30");
    for (int i = 0; i < 4; i++)
        if (cfg->reserved[i]) return fail(NFC_ERR_ARG, "cfg.reserved must be 0");
    if (K > 65536) return fail(NFC_ERR_ARG, "K exceeds 65536");
    if (K == 0) return NFC_OK;
    if (!frame_off || !byte_base || !first_sample || !n_samples) return fail(NFC_ERR_ARG, "frame_off, byte_base, first_sample or n_samples is null");
    for (size_t k = 0; k < K; k++) {
        if (frame_off[k + 1] < frame_off[k]) return fail(NFC_ERR_ARG, "frame_off[%zu] is below the entry before it", k + 1);
        if (byte_base[k + 1] < byte_base[k]) return fail(NFC_ERR_ARG, "byte_base[%zu] is below the entry before it", k + 1);
    }
    if (frame_off[0] != 0 || byte_base[0] != 0) return fail(NFC_ERR_ARG, "frame_off[0] and byte_base[0] must be 0");
    if (frame_off[K] > 0x7FFFFFFFu) return fail(NFC_ERR_ARG, "frame_off: more than 2^31 frames");
    if (frame_off[K] && !frames) return fail(NFC_ERR_ARG, "frames is null");
    if (byte_base[K] && (!air || !par)) return fail(NFC_ERR_ARG, "air or par is null");
    for (size_t k = 0; k < K; k++) {
        const uint32_t part = byte_base[k + 1] - byte_base[k];
        for (uint32_t f = frame_off[k]; f < frame_off[k + 1]; f++) {
            const nfc_air_frame &fr = frames[f];
            if (fr.type > 1) return fail(NFC_ERR_ARG, "frames[%u].type is neither 0 nor 1", f);
            if (fr.flags || fr.reserved) return fail(NFC_ERR_ARG, "frames[%u]: flags and reserved must be 0", f);
            if (fr.n_bits > MAX_BITS || (fr.n_bits > 8 && fr.n_bits % 9)) return fail(NFC_ERR_ARG, "frames[%u].n_bits %u is neither 0 .. 8 nor a multiple of 9 up to %u", f, fr.n_bits, MAX_BITS);
            if (fr.idle_before > MAX_STREAM_SAMPLES) return fail(NFC_ERR_ARG, "frames[%u].idle_before exceeds 2^30", f);
            const uint32_t nb = frame_bytes(fr.n_bits);
            if (nb && (fr.byte_off > part || nb > part - fr.byte_off))
                return fail(NFC_ERR_ARG, "frames[%u].byte_off: the frame's %u bytes leave stream %zu's part of air / par (%u bytes)", f, nb, k, part);
        }
    }
    return NFC_OK;
}

// the need of a layout against the caller's room: nothing is rendered when it does not fit
inline int room_fault(const uint64_t *first_sample, const uint64_t *n_stream, size_t K, size_t cap_samples, bool rendering, uint64_t &need) {
    need = 0;
    for (size_t k = 0; k < K; k++) {
        if (n_stream[k] > MAX_STREAM_SAMPLES) return fail(NFC_ERR_ARG, "stream %zu has %llu samples: more than 2^30", k, (unsigned long long)n_stream[k]);
        need = first_sample[k] + n_stream[k];
    }
    if (rendering && need > cap_samples)
        return fail(NFC_ERR_ARG, "cap_samples: the layout needs %llu samples, %zu do not hold them", (unsigned long long)need, cap_samples);
    return NFC_OK;
}

inline void store_sample(uint8_t *out, uint32_t kind, uint64_t at, uint64_t v) {
    const uint32_t bps = bytes_per_sample(kind);
    memcpy(out + at * bps, &v, bps);   // (little endian: the sample's bytes are the low ones)
}

template <int KIND>
void launch_render(const RenderArgs &A, unsigned blocks, uint32_t max_bits, hipEvent_t e0, hipEvent_t e1) {
    const unsigned lds = 4u * render_lds_words(max_bits);   // (at most 20 KB: MAX_BITS)
    if (e0) NFC_LAUNCH_EXT(k_air_render<KIND>, dim3(blocks), dim3(RENDER_BLOCK), lds, nullptr, e0, e1, 0, A, max_bits);
    else NFC_LAUNCH(k_air_render<KIND>, dim3(blocks), dim3(RENDER_BLOCK), lds, nullptr, A, max_bits);
}

}  // namespace air
}  // namespace nfc

using namespace nfc;

extern "C" {

int nfc_host_air_render(const nfc_air_config *cfg, const nfc_air_frame *frames, const uint32_t *frame_off, const uint8_t *air_bytes, const uint8_t *par,
                        const uint32_t *byte_base, size_t K, void *out, size_t cap_samples, uint64_t *first_sample, uint32_t *n_samples) {
    if (const int rc = air::args_fault(cfg, frames, frame_off, air_bytes, par, byte_base, K, first_sample, n_samples)) return rc;
    if (K == 0) return NFC_OK;
    const air::Consts C = air::make_consts(*cfg);
    // the layout
    std::vector<uint64_t> n_stream(K);
    std::vector<uint32_t> len(frame_off[K]);
    uint64_t at = 0;
    for (size_t k = 0; k < K; k++) {
        uint64_t n = 0;
        for (uint32_t f = frame_off[k]; f < frame_off[k + 1]; f++) {
            const nfc_air_frame &fr = frames[f];
            const uint8_t *b = air_bytes + byte_base[k] + fr.byte_off, *p = par + byte_base[k] + fr.byte_off;
            len[f] = air::frame_samples(C, fr.type, air::Bits{b, p, fr.n_bits});
            n += (uint64_t)fr.idle_before + len[f];
        }
        n_stream[k] = n + C.tail;
        first_sample[k] = at;
        n_samples[k] = n_stream[k] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_stream[k];
        at += air::align_up(n_stream[k], C.align);
    }
    uint64_t need;
    if (const int rc = air::room_fault(first_sample, n_stream.data(), K, cap_samples, out != nullptr, need)) return rc;
    if (!out) return NFC_OK;   // the sizing call
    // the samples, one after the other
    uint8_t *o = (uint8_t *)out;
    const bool noisy = C.noisy != 0;
    for (size_t k = 0; k < K; k++) {
        const uint64_t first = first_sample[k], key = air::stream_key(C.seed, cfg->stream_seeds ? cfg->stream_seeds[k] : (uint64_t)k);
        uint32_t r = 0;   // the sample's index in the stream
        auto put = [&](uint32_t m, bool with_noise) {
            float si, sq;
            air::sample_iq(C, m, with_noise, key, r, si, sq);
            air::store_sample(o, C.kind, first + r, air::pack(C.kind, si, sq, C.full_scale));
            r++;
        };
        for (uint32_t f = frame_off[k]; f < frame_off[k + 1]; f++) {
            const nfc_air_frame &fr = frames[f];
            const air::Bits B = {air_bytes + byte_base[k] + fr.byte_off, par + byte_base[k] + fr.byte_off, fr.n_bits};
            for (uint32_t i = 0; i < fr.idle_before; i++) put(air::M_ONE, noisy);
            const uint32_t np = air::n_pieces(fr.type, fr.n_bits);
            for (uint32_t j = 0; j < np; j++) {
                const air::Piece P = air::piece_of(C, fr.type, B, j);
                const uint32_t ma = fr.type ? P.la : P.la ? air::M_LOADED : air::M_ONE, mb = fr.type ? P.lb : P.lb ? air::M_LOADED : air::M_ONE;
                for (uint32_t i = 0; i < P.ca; i++) put(ma, noisy);
                for (uint32_t i = 0; i < P.cb; i++) put(mb, noisy);
            }
        }
        for (uint32_t i = 0; i < C.tail; i++) put(air::M_ONE, noisy);
        if (k + 1 < K)   // the padding up to the next stream: idle carrier without noise
            while (first + r < first_sample[k + 1]) put(air::M_ONE, false);
    }
    return NFC_OK;
}

int nfc_air_render_device(int device, const nfc_air_config *cfg, const nfc_air_frame *frames, const uint32_t *frame_off, const uint8_t *air_bytes,
                          const uint8_t *par, const uint32_t *byte_base, size_t K, void *dev_out, size_t cap_samples, uint64_t *first_sample,
                          uint32_t *n_samples, float *kernel_ms) {
    if (const int rc = air::args_fault(cfg, frames, frame_off, air_bytes, par, byte_base, K, first_sample, n_samples)) return rc;
    if (device < 0) return air::fail(NFC_ERR_ARG, "device is negative");
    if ((uintptr_t)dev_out & 15u) return air::fail(NFC_ERR_ARG, "dev_out must be 16-byte aligned");
    if (!dev_out && cap_samples) return air::fail(NFC_ERR_ARG, "dev_out is null");
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.f;
    if (K == 0) return NFC_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return air::fail(NFC_ERR_DEVICE, "nfc_air_render_device: no HIP device, and this call has no CPU fallback");
    if (device >= ndev) return air::fail(NFC_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
    if (hipSetDevice(device) != hipSuccess) return air::fail(NFC_ERR_DEVICE, "hipSetDevice(%d) failed", device);
    const air::Consts C = air::make_consts(*cfg);
    const uint32_t F = frame_off[K], n_bytes = byte_base[K];
    std::vector<uint32_t> frame_stream(F), empty;
    uint32_t max_bits = 0;
    for (size_t k = 0; k < K; k++) {
        for (uint32_t f = frame_off[k]; f < frame_off[k + 1]; f++) frame_stream[f] = (uint32_t)k, max_bits = std::max<uint32_t>(max_bits, frames[f].n_bits);
        if (frame_off[k] == frame_off[k + 1]) empty.push_back((uint32_t)k);
    }
    // the sections
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t G = air::GUARD_BYTES;
    const size_t s_frames = (size_t)F * sizeof(nfc_air_frame), s_fs = (size_t)F * 4, s_off = (K + 1) * 4, s_seeds = cfg->stream_seeds ? K * 8 : 0, s_empty = empty.size() * 4;
    const size_t o_frames = 0, o_fs = o_frames + up(s_frames), o_foff = o_fs + up(s_fs), o_base = o_foff + up(s_off), o_air = o_base + up(s_off),
                 o_par = o_air + up(n_bytes), o_seeds = o_par + up(n_bytes), o_empty = o_seeds + up(s_seeds), in_bytes = o_empty + up(s_empty);
    const size_t s_rel = (size_t)F * 4, s_n64 = K * 8, s_first = K * 8, s_n32 = K * 4;
    const size_t o_rel = in_bytes, o_n64 = o_rel + up(s_rel + G), o_first = o_n64 + up(s_n64 + G), o_n32 = o_first + up(s_first + G), total = o_n32 + up(s_n32 + G);
    const size_t guard_at[4] = {o_rel + s_rel, o_n64 + s_n64, o_first + s_first, o_n32 + s_n32};
    auto bad = [](hipError_t e, const char *what) {
        return e == hipSuccess ? NFC_OK : air::fail(e == hipErrorOutOfMemory ? NFC_ERR_NOMEM : NFC_ERR_DEVICE, "nfc_air_render_device: %s: %s", what, hipGetErrorString(e));
    };
    LaunchError launch;
    LaunchScope scope(&launch);
    DevBuf buf;
    Event e[4];
    if (int rc = bad(buf.ensure(total), "hipMalloc")) return rc;
    uint8_t *d = buf.as<uint8_t>();
    auto upload = [&](size_t off, const void *src, size_t n) { return n ? hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) : hipSuccess; };
    if (int rc = bad(upload(o_frames, frames, s_frames), "upload")) return rc;
    if (int rc = bad(upload(o_fs, frame_stream.data(), s_fs), "upload")) return rc;
    if (int rc = bad(upload(o_foff, frame_off, s_off), "upload")) return rc;
    if (int rc = bad(upload(o_base, byte_base, s_off), "upload")) return rc;
    if (int rc = bad(upload(o_air, air_bytes, n_bytes), "upload")) return rc;
    if (int rc = bad(upload(o_par, par, n_bytes), "upload")) return rc;
    if (int rc = bad(upload(o_seeds, cfg->stream_seeds, s_seeds), "upload")) return rc;
    if (int rc = bad(upload(o_empty, empty.data(), s_empty), "upload")) return rc;
    if (int rc = bad(hipMemsetAsync(d + in_bytes, 0, total - in_bytes, 0), "memset")) return rc;
    for (size_t g : guard_at)
        if (int rc = bad(hipMemsetD32Async((hipDeviceptr_t)(d + g), (int)air::GUARD_WORD, G / 4, 0), "memset")) return rc;
    if (kernel_ms)
        for (Event &ev : e)
            if (int rc = bad(ev.create(), "event")) return rc;

    air::Input in = {(const nfc_air_frame *)(d + o_frames), (const uint32_t *)(d + o_foff), (const uint32_t *)(d + o_base), d + o_air, d + o_par, (uint32_t)K, F};
    air::LayoutArgs LA = {C, in, (uint32_t *)(d + o_rel), (uint64_t *)(d + o_n64)};
    NFC_LAUNCH_EXT(air::k_air_layout, dim3((unsigned)K), dim3(air::BLOCK), 0, nullptr, kernel_ms ? (hipEvent_t)e[0] : nullptr, nullptr, 0, LA);
    NFC_LAUNCH_EXT(air::k_air_starts, dim3(1), dim3(air::START_BLOCK), 0, nullptr, nullptr, kernel_ms ? (hipEvent_t)e[1] : nullptr, 0, (const uint64_t *)(d + o_n64),
                   (uint32_t)K, C.align, (uint64_t *)(d + o_first), (uint32_t *)(d + o_n32));
    if (launch.err != hipSuccess) return bad(launch.err, "launch");
    std::vector<uint64_t> n_stream(K);
    if (int rc = bad(hipMemcpy(n_stream.data(), d + o_n64, s_n64, hipMemcpyDeviceToHost), "download")) return rc;   // (the copy waits for the kernels)
    if (int rc = bad(hipMemcpy(first_sample, d + o_first, s_first, hipMemcpyDeviceToHost), "download")) return rc;
    if (int rc = bad(hipMemcpy(n_samples, d + o_n32, s_n32, hipMemcpyDeviceToHost), "download")) return rc;
    uint64_t need;
    if (const int rc = air::room_fault(first_sample, n_stream.data(), K, cap_samples, true, need)) return rc;

    air::RenderArgs RA = {C, in, (const uint32_t *)(d + o_fs), (const uint32_t *)(d + o_rel), (const uint64_t *)(d + o_first), (const uint32_t *)(d + o_n32),
                          cfg->stream_seeds ? (const uint64_t *)(d + o_seeds) : nullptr, (const uint32_t *)(d + o_empty), (uint8_t *)dev_out};
    const unsigned blocks = F + (unsigned)empty.size();
    const hipEvent_t r0 = kernel_ms ? (hipEvent_t)e[2] : nullptr, r1 = kernel_ms ? (hipEvent_t)e[3] : nullptr;
    switch (C.kind) {
    case NFC_IN_IQ_F32: air::launch_render<NFC_IN_IQ_F32>(RA, blocks, max_bits, r0, r1); break;
    case NFC_IN_IQ_I16: air::launch_render<NFC_IN_IQ_I16>(RA, blocks, max_bits, r0, r1); break;
    case NFC_IN_IQ_I8: air::launch_render<NFC_IN_IQ_I8>(RA, blocks, max_bits, r0, r1); break;
    default: air::launch_render<NFC_IN_IQ_U8>(RA, blocks, max_bits, r0, r1); break;
    }
    if (launch.err != hipSuccess) return bad(launch.err, "launch");
    uint32_t guards[4][4];
    for (int g = 0; g < 4; g++)
        if (int rc = bad(hipMemcpy(guards[g], d + guard_at[g], G, hipMemcpyDeviceToHost), "download")) return rc;   // (waits for the renderer)
    if (int rc = bad(hipDeviceSynchronize(), "kernel")) return rc;
    if (kernel_ms) {
        if (int rc = bad(hipEventElapsedTime(&kernel_ms[0], e[0], e[1]), "event")) return rc;
        if (int rc = bad(hipEventElapsedTime(&kernel_ms[1], e[2], e[3]), "event")) return rc;
    }
    for (int g = 0; g < 4; g++)
        for (int w = 0; w < 4; w++)
            if (guards[g][w] != air::GUARD_WORD) return air::fail(NFC_ERR_INTERNAL, "nfc_air_render_device: the guard word behind device section %d was overwritten", g);
    return NFC_OK;
}

}  // extern "C"
