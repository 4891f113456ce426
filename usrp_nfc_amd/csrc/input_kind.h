// input_kind.h -- what is a property of an input kind and not of a kernel, on the host: how many kinds there are, a sample's bytes,
// the kernels' conversion argument for the caller's i16_scale, and with_kind -- the one switch over the kinds in csrc/.  Shared by the
// translation units that create contexts or pick a kind's kernel (nfc_amd.hip, nfc_multi.hip, nfc_record.hip; kind_kernels.h).
// Included after threshold.hip.h, whose IN_* the kernels are instantiated with.
#pragma once
#include <cmath>
#include <cstddef>
#include <type_traits>
#include <utility>

#include "../../include/nfc_amd.h"

namespace nfc {

constexpr int N_KINDS = 7;
static_assert(IN_IQ_F32 == NFC_IN_IQ_F32 && IN_ENV_F32 == NFC_IN_ENV_F32 && IN_REAL_F32_SQ == NFC_IN_REAL_F32_SQ && IN_I16_SQ == NFC_IN_I16_SQ &&
                  IN_IQ_I16 == NFC_IN_IQ_I16 && IN_IQ_I8 == NFC_IN_IQ_I8 && IN_IQ_U8 == NFC_IN_IQ_U8 && IN_IQ_U8 == N_KINDS - 1,
              "the kernels' kinds are the header's, 0 .. N_KINDS - 1");

constexpr bool kind_valid(int kind) { return kind >= 0 && kind < N_KINDS; }
constexpr bool is_iq8(int kind) { return kind == IN_IQ_I8 || kind == IN_IQ_U8; }
// input bytes per sample (kind_valid(kind))
inline size_t kind_bytes(int kind) {
    static const size_t bps[N_KINDS] = {8, 4, 4, 2, 4, 2, 2};
    return bps[kind];
}

// f(std::integral_constant<int, KIND>{}) for the kind: where a kind chosen at run time picks a template's instantiation.
template <class F>
decltype(auto) with_kind(int kind, F &&f) {
    switch (kind) {
    case IN_IQ_F32: return std::forward<F>(f)(std::integral_constant<int, IN_IQ_F32>{});
    case IN_ENV_F32: return std::forward<F>(f)(std::integral_constant<int, IN_ENV_F32>{});
    case IN_REAL_F32_SQ: return std::forward<F>(f)(std::integral_constant<int, IN_REAL_F32_SQ>{});
    case IN_IQ_I16: return std::forward<F>(f)(std::integral_constant<int, IN_IQ_I16>{});
    case IN_IQ_I8: return std::forward<F>(f)(std::integral_constant<int, IN_IQ_I8>{});
    case IN_IQ_U8: return std::forward<F>(f)(std::integral_constant<int, IN_IQ_U8>{});
    default: return std::forward<F>(f)(std::integral_constant<int, IN_I16_SQ>{});
    }
}

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
