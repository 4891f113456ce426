// iq8.h -- what nfc_amd.hip reaches of nfc_iq8.hip: the threshold-stage kernels of the complex 8-bit input kinds (NFC_IN_IQ_I8, sc8,
// and NFC_IN_IQ_U8, cu8), which live in a translation unit of their own as the complex int16 kind's do (iq16.h).  Each function takes
// the kind (IN_IQ_I8 or IN_IQ_U8) and returns that kind's instantiation; the host side launches them through these pointers
// (host_context.h) and asks the runtime about them (nfc_create: LDS attribute, occupancy).
#pragma once

#include "iq16.h"   // (the kernel pointer types)

namespace nfc {
namespace iq8 {
ThrKernel threshold_kernel(int kind, bool gring);   // k_threshold<kind, 4, gring>
ThrKernel lean_kernel(int kind, bool blk16);        // k_threshold_lean<kind, 4, blk16>
ThrKernel wg_kernel(int kind, int nr);              // k_threshold_wg<kind, nr>: pass 0, four or eight rows per step
ThrKernel wg_ex_kernel(int kind);                   // k_threshold_wg<kind, 4, true>: re-runs with failed rounds evaluated in place
FillKernel fill_kernel(int kind);                   // k_fill<kind>
SeqKernel seq_kernel(int kind);                     // k_threshold_seq<kind>
}  // namespace iq8
}  // namespace nfc
