// kind_kernels.h -- the threshold-stage kernels of an input kind as one table of pointers, filled by the translation unit that owns
// the kind's instantiations: nfc_amd.hip for the four original kinds, nfc_iq16.hip for the complex int16 kind, nfc_iq8.hip for the
// complex 8-bit kinds -- so each unit's device code is what it is without the others' (tests/test_isa_audit.py pins nfc_amd.hip's).
// The host side launches through a context's table (host_context.h) and asks the runtime about its entries (nfc_create: LDS attribute,
// occupancy); which entry a launch takes is launch_threshold's choice (host_threshold.h), from the batch's plan and what the launch is for.
// The one optional form is eight rows per step: whether a kind has it is whether wg[1] is filled, and is decided here alone.
// Included after threshold.hip.h, threshold_lean.hip.h and threshold_wg.hip.h.
#pragma once
#include "input_kind.h"

namespace nfc {

using ThrKernel = void (*)(ThrArgs);
using SeqKernel = void (*)(SeqArgs);
using FillKernel = void (*)(const void *, uint32_t, float, int, float *, Carry *, EdgeCarryInit, uint8_t *, int, CertSummary *, StateInit,
                            uint32_t *, uint32_t, int);   // (k_fill)

struct KindKernels {
    ThrKernel thr[2];        // [gring]   k_threshold<KIND, 4, gring>
    ThrKernel lean[2];       // [blk16]   k_threshold_lean<KIND, 4, blk16>
    ThrKernel wg[2];         // [nr == 8] k_threshold_wg<KIND, nr>: pass 0, four or eight rows per step; [1] null where eight rows are not instantiated
    ThrKernel wg_ex;         //           k_threshold_wg<KIND, 4, true>: re-runs with failed rounds evaluated in place
    FillKernel fill;         // k_fill<KIND>
    SeqKernel seq;           // k_threshold_seq<KIND>
};

// Eight rows per step: fc32, sc16, sc8 and cu8 IQ and the float32 envelope -- what a capture at a rate that wants a window of thousands
// of samples arrives as.
template <int KIND>
constexpr bool has_nr8 = KIND == IN_IQ_F32 || KIND == IN_ENV_F32 || KIND == IN_IQ_I16 || is_iq8(KIND);

template <int KIND>
KindKernels make_kind_kernels() {
    KindKernels k{};
    k.thr[0] = k_threshold<KIND, 4, false>;
    k.thr[1] = k_threshold<KIND, 4, true>;
    k.lean[0] = k_threshold_lean<KIND, 4, false>;
    k.lean[1] = k_threshold_lean<KIND, 4, true>;
    k.wg[0] = k_threshold_wg<KIND, 4>;
    if constexpr (has_nr8<KIND>) k.wg[1] = k_threshold_wg<KIND, 8>;
    k.wg_ex = k_threshold_wg<KIND, 4, true>;
    k.fill = k_fill<KIND>;
    k.seq = k_threshold_seq<KIND>;
    return k;
}

namespace iq16 {
const KindKernels &kernels();           // nfc_iq16.hip: IN_IQ_I16
}
namespace iq8 {
const KindKernels &kernels(int kind);   // nfc_iq8.hip: IN_IQ_I8 or IN_IQ_U8
}

}  // namespace nfc
