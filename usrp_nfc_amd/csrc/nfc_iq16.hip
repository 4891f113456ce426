// nfc_iq16.hip -- the threshold-stage kernels of the complex int16 input kind (NFC_IN_IQ_I16, sc16: what a USRP sends over
// the wire, 4 bytes per sample), in a translation unit of their own.  Every instantiation for the kind lives here and only here;
// nfc_amd.hip launches them through the pointers of iq16.h.  The kernels are the shared templates of threshold*.hip.h: the
// loads are the 4-byte kinds' (one dword per sample), the conversion is threshold.hip.h's iq16_env.  The non-template kernels
// of those headers are nfc_amd.hip's: here they are `static` (NFC_HDR_KERNEL_LINKAGE) and never launched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#define NFC_HDR_KERNEL_LINKAGE static
#include "../../include/nfc_amd.h"
#include "launch_check.h"
#include "threshold.hip.h"
#include "threshold_lean.hip.h"
#include "threshold_wg.hip.h"
#include "iq16.h"

namespace nfc {
namespace iq16 {

ThrKernel threshold_kernel(bool gring) { return gring ? k_threshold<IN_IQ_I16, 4, true> : k_threshold<IN_IQ_I16, 4, false>; }
ThrKernel lean_kernel(bool blk16) { return blk16 ? k_threshold_lean<IN_IQ_I16, 4, true> : k_threshold_lean<IN_IQ_I16, 4, false>; }
// (eight rows per step as for fc32 IQ: a 10 Msps capture arrives as sc16 just as naturally.  The per-wave-counter form of the
// test build, NFC_WG_FLAGS, is not instantiated for this kind: the switch is ignored for it.)
ThrKernel wg_kernel(int nr) { return nr == 8 ? k_threshold_wg<IN_IQ_I16, 8> : k_threshold_wg<IN_IQ_I16, 4>; }
ThrKernel wg_ex_kernel() { return k_threshold_wg<IN_IQ_I16, 4, true>; }
FillKernel fill_kernel() { return k_fill<IN_IQ_I16>; }
SeqKernel seq_kernel() { return k_threshold_seq<IN_IQ_I16>; }

}  // namespace iq16
}  // namespace nfc
