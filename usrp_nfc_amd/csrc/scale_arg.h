// scale_arg.h -- the kernels' conversion argument for an input kind and the caller's i16_scale, on the host: shared by the
// translation units that create contexts (nfc_amd.hip: nfc_create, nfc_record_pcm16_device; nfc_multi.hip: nfc_multi_create).
#pragma once
#include <cmath>

#include "../../include/nfc_amd.h"

namespace nfc {

// The complex 8-bit kinds' kernel argument (threshold.hip.h: iq8_env).  scale: i16_scale, 2^-7 where it is not positive.  A power of
// two 2^k takes the integer route, -2^(2k), where every nonzero value of the definition is a normal float: the smallest nonzero square
// is 2^(2k) (sc8, |q| = 1) or 2^(2k-2) (cu8, |u - 127.5| = 1/2), so k >= -63 (sc8) or k >= -62 (cu8); above, the scale is at most
// 2^56, and the largest envelope, 2^15 2^(2k), is at most 2^127.  Any other scale takes the float route: the scale itself.
inline float iq8_kernel_arg(int kind, float i16_scale) {
    const float s = i16_scale > 0.f ? i16_scale : 0.0078125f;
    int e = 0;
    const float mant = frexpf(s, &e);   // s = mant 2^e, mant in [0.5, 1)
    const int k = e - 1, kmin = kind == NFC_IN_IQ_I8 ? -63 : -62;
    if (mant == 0.5f && k >= kmin && k <= 56) return -ldexpf(1.0f, 2 * k);
    return s;
}
// The kernels' conversion argument for an input kind and the caller's i16_scale (nfc_params.i16_scale) -- what nfc_create puts into the
// context and nfc_record_pcm16_device hands its kernel: the int16 kinds' scale, or -1 for sample / 32767 (threshold.hip.h: i16_to_float);
// the complex 8-bit kinds' route and scale (iq8_kernel_arg).  Returns null, or what is wrong with the scale.
inline const char *kernel_scale_arg(int kind, float i16_scale, float *arg) {
    // (complex int16: |I|, |Q| <= 2^15, so the envelope 2 (2^15 s)^2 stays finite -- and the kernels need no guard for it -- up to s = 2^48)
    if (kind == NFC_IN_IQ_I16 && i16_scale > 281474976710656.0f) return "i16_scale must be at most 2^48 for complex int16 input";
    // (complex 8-bit: |I|, |Q| <= 2^7 s -- sc8's -128, cu8's 127.5 --, so the envelope 2 (2^7 s)^2 stays finite up to s = 2^56)
    if ((kind == NFC_IN_IQ_I8 || kind == NFC_IN_IQ_U8) && i16_scale > 72057594037927936.0f) return "i16_scale must be at most 2^56 for complex 8-bit input";
    *arg = i16_scale > 0.f ? i16_scale : -1.0f;   // (0: GNU Radio's wavfile_source normalisation, sample / 32767; threshold.hip.h: i16_to_float)
    if (kind == NFC_IN_IQ_I8 || kind == NFC_IN_IQ_U8) *arg = iq8_kernel_arg(kind, i16_scale);   // (not the -1 above)
    return nullptr;
}

}  // namespace nfc
