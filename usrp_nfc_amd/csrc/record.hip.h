// record.hip.h -- the float -> 16-bit PCM conversion of the recording path (include/nfc_amd.h: nfc_record_pcm16_device), shared by
// the kernel (nfc_record.hip) and its host twin (nfc_host_record_pcm16), and what nfc_amd.hip reaches of nfc_record.hip.
//
// The reference writes its recordings through GNU Radio's wavfile_sink (usrp_src.py:35-37: complex_to_mag_squared -> wavfile_sink;
// record.py:10-19: complex_to_real -> wavfile_sink), 16 bits, one channel.  That block multiplies by 0x7FFF, clamps to +-0x7FFF and
// rounds to nearest; it is third party and absent from the reference tree, so this boundary is UNPINNED, as wavfile_source's is
// (SURVEY.md 8c).  The conversion here, in this order:
//   v = fl(x * gain)                      one float32 product (the unit is compiled with -ffp-contract=off)
//   NaN -> 0
//   clamp to [-32767, 32767]              (+-Inf -> +-32767)
//   round to nearest, halves away from 0  (lroundf): t = trunc(v); v - t is exact; |v - t| >= 1/2 moves t one step away from zero.
//                                         Not floor(v + 0.5): fl(0.49999997 + 0.5) is 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nfc {

__host__ __device__ __forceinline__ int16_t pcm16_of(float x, float gain) {
    float v = x * gain;
    if (!(v == v)) v = 0.f;
    v = fminf(fmaxf(v, -32767.f), 32767.f);
    float t = truncf(v);
    if (fabsf(v - t) >= 0.5f) t += copysignf(1.f, v);
    return (int16_t)(int)t;
}

namespace rec {
enum : int { TAP_ENVELOPE = 0, TAP_REAL_PART = 1 };
// Enqueues k_record_pcm16<kind, tap> on `stream` for n samples (n > 0; in and out 16-byte aligned; arg: the kind's kernel argument as
// nfc_create encodes i16_scale).  nontemporal: the input loads carry the non-temporal hint (the A/B of tests/record_bench.py; the
// product passes false).  e0 / e1: events around the launch itself, or null.  The launch is noted as every launch is (launch_check.h).
void launch(int kind, int tap, const void *in, size_t n, float arg, float gain, void *out, int cus, bool nontemporal, hipStream_t stream,
            hipEvent_t e0, hipEvent_t e1);
}  // namespace rec

}  // namespace nfc
