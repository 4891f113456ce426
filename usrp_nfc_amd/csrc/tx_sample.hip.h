// tx_sample.hip.h -- one transmitted sample, the device function k_tx_render (tx.hip.h) and k_answers_tx_render (answers_tx.hip.h)
// share: a level, and with the carrier on the level times amp * exp(j 2 pi phase).  The phase of carrier index i is (i * inc) mod 2^64
// with inc = floor(frac(f / samp_rate) * 2^64); its top 24 bits select the angle, cos / sin by sincospif in fp32.  With the carrier off
// the sample is exactly (level, 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nfc {

__device__ __forceinline__ float2 tx_sample(uint64_t index, uint64_t phase_inc, float amp, int carrier, float lvl) {
    float re = lvl, im = 0.f;
    if (carrier) {
        const uint64_t ph = index * phase_inc;
        const float turn = (float)(uint32_t)(ph >> 40) * 5.9604644775390625e-08f;   // top 24 bits: [0, 1) exactly
        float sn, cs;
        sincospif(2.0f * turn, &sn, &cs);
        re = lvl * (amp * cs);
        im = lvl * (amp * sn);
    }
    return make_float2(re, im);
}

}  // namespace nfc
