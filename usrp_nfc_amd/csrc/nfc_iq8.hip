// nfc_iq8.hip -- the threshold-stage kernels of the complex 8-bit input kinds (NFC_IN_IQ_I8, sc8: a HackRF's samples, UHD's sc8;
// NFC_IN_IQ_U8, cu8: rtl_sdr's; 2 bytes per sample), in a translation unit of their own.  Every instantiation for the two kinds
// lives here and only here; nfc_amd.hip launches them through the tables of kind_kernels.h.  The kernels are the shared templates of
// threshold*.hip.h: the loads are the 2-byte kind's (one ushort per sample, zero-extended), the conversion is threshold.hip.h's
// iq8_env -- the integer or the float route, as the kernel argument says.  The non-template kernels of those headers are
// nfc_amd.hip's: here they are `static` (NFC_HDR_KERNEL_LINKAGE) and never launched.
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
namespace iq8 {

// (eight rows per step as for fc32 and sc16 IQ: a HackRF records at 8-20 Msps, where the window is thousands of samples long)
const KindKernels &kernels(int kind) {
    static const KindKernels i8 = make_kind_kernels<IN_IQ_I8>(), u8 = make_kind_kernels<IN_IQ_U8>();
    return kind == IN_IQ_I8 ? i8 : u8;
}

}  // namespace iq8
}  // namespace nfc
