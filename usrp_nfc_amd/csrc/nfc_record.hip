// nfc_record.hip -- the recording kernel, k_record_pcm16<KIND, TAP>, in a translation unit of its own: a float per sample -- the
// envelope the threshold kernels compute for the input kind (threshold.hip.h: env_of / envelope_at, the same device functions), or
// the real part of a complex64 sample -- to 16-bit PCM (record.hip.h: pcm16_of).  nfc_amd.hip launches it through rec::launch
// (nfc_record_pcm16_device).  The non-template kernels of threshold.hip.h are nfc_amd.hip's: here they are `static`
// (NFC_HDR_KERNEL_LINKAGE) and never launched.
//
// One element-wise streaming kernel, memory-bound by design: a lane turns 8 consecutive samples into one 16-byte store per trip of
// a grid-stride loop (64-bit indices; the grid is a few workgroups per CU, not one per 2048 samples), reading them as 16-byte loads
// -- four for fc32 (64 B), two for the 4-byte kinds, one for the 2-byte kinds.  The last n mod 8 samples are a scalar tail of the
// first workgroup.  Nothing is written beyond out[n).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#define NFC_HDR_KERNEL_LINKAGE static
#include "../../include/nfc_amd.h"
#include "launch_check.h"
#include "threshold.hip.h"
#include "record.hip.h"
#include "input_kind.h"

namespace nfc {
namespace rec {

constexpr int REC_BLOCK = 256;
constexpr int REC_WG_PER_CU = 8;
typedef uint32_t rec_u4 __attribute__((ext_vector_type(4)));

template <int KIND, int TAP>
__device__ __forceinline__ float rec_value(typename RawOf<KIND>::T raw, float arg) {
    if constexpr (TAP == TAP_REAL_PART) return raw.x;   // (complex_to_real, record.py:18; fc32 only)
    else return env_of<KIND>(raw, arg);
}

template <int KIND, int TAP, bool NT>
__global__ __launch_bounds__(REC_BLOCK) void k_record_pcm16(const void *__restrict__ in, uint64_t n, float arg, float gain, int16_t *__restrict__ out) {
    using Raw = typename RawOf<KIND>::T;
    constexpr int NV = (int)(8 * sizeof(Raw) / 16);   // 16-byte loads per trip
    const uint64_t groups = n >> 3;
    const uint64_t stride = (uint64_t)gridDim.x * REC_BLOCK;
    for (uint64_t g = (uint64_t)blockIdx.x * REC_BLOCK + threadIdx.x; g < groups; g += stride) {
        const rec_u4 *p = (const rec_u4 *)in + g * NV;
        rec_u4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) v[j] = NT ? __builtin_nontemporal_load(p + j) : p[j];
        Raw raw[8];
        __builtin_memcpy(raw, v, sizeof raw);
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t a = (uint16_t)pcm16_of(rec_value<KIND, TAP>(raw[2 * k], arg), gain);
            const uint32_t b = (uint16_t)pcm16_of(rec_value<KIND, TAP>(raw[2 * k + 1], arg), gain);
            w[k] = a | (b << 16);
        }
        ((rec_u4 *)out)[g] = (rec_u4){w[0], w[1], w[2], w[3]};
    }
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)(n & 7u)) {
        const uint64_t m = (groups << 3) + threadIdx.x;
        out[m] = pcm16_of(rec_value<KIND, TAP>(load_raw<KIND>(in, (size_t)m), arg), gain);
    }
}

using RecKernel = void (*)(const void *, uint64_t, float, float, int16_t *);

template <bool NT>
RecKernel kernel_of(int kind, int tap) {
    if (tap == TAP_REAL_PART) return k_record_pcm16<IN_IQ_F32, TAP_REAL_PART, NT>;
    return with_kind(kind, [](auto K) -> RecKernel { return k_record_pcm16<decltype(K)::value, TAP_ENVELOPE, NT>; });
}

void launch(int kind, int tap, const void *in, size_t n, float arg, float gain, void *out, int cus, bool nontemporal, hipStream_t stream,
            hipEvent_t e0, hipEvent_t e1) {
    RecKernel k = kernel_of<false>(kind, tap);
#ifdef NFC_TEST_HOOKS
    if (nontemporal) k = kernel_of<true>(kind, tap);   // (the load-policy A/B: the test build carries both forms)
#else
    (void)nontemporal;
#endif
    const uint64_t groups = (uint64_t)n >> 3;
    const uint64_t want = (groups + REC_BLOCK - 1) / REC_BLOCK;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)std::max(1, cus) * REC_WG_PER_CU));
    if (e0 || e1) NFC_LAUNCH_EXT(k, dim3(blocks), dim3(REC_BLOCK), 0, stream, e0, e1, 0, in, (uint64_t)n, arg, gain, (int16_t *)out);
    else NFC_LAUNCH(k, dim3(blocks), dim3(REC_BLOCK), 0, stream, in, (uint64_t)n, arg, gain, (int16_t *)out);
}

}  // namespace rec
}  // namespace nfc
