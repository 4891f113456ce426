// nfc_iq16.hip -- the threshold-stage kernels of the complex int16 input kind (NFC_IN_IQ_I16, sc16: what a USRP sends over
// the wire, 4 bytes per sample), in a translation unit of their own.  Every instantiation for the kind lives here and only here;
// nfc_amd.hip launches them through the table of kind_kernels.h.  The kernels are the shared templates of threshold*.hip.h: the
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
#include "kind_kernels.h"

namespace nfc {
namespace iq16 {

// (eight rows per step as for fc32 IQ: a 10 Msps capture arrives as sc16 just as naturally)
const KindKernels &kernels() {
    static const KindKernels k = make_kind_kernels<IN_IQ_I16>();
    return k;
}

}  // namespace iq16
}  // namespace nfc
