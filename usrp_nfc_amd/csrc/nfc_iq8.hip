// nfc_iq8.hip -- the threshold-stage kernels of the complex 8-bit input kinds (NFC_IN_IQ_I8, sc8: a HackRF's samples, UHD's sc8;
// NFC_IN_IQ_U8, cu8: rtl_sdr's; 2 bytes per sample), in a translation unit of their own.  Every instantiation for the two kinds
// lives here and only here; nfc_amd.hip launches them through the pointers of iq8.h.  The kernels are the shared templates of
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
#include "iq8.h"

namespace nfc {
namespace iq8 {

template <int K>
ThrKernel threshold_of(bool gring) { return gring ? k_threshold<K, 4, true> : k_threshold<K, 4, false>; }
template <int K>
ThrKernel lean_of(bool blk16) { return blk16 ? k_threshold_lean<K, 4, true> : k_threshold_lean<K, 4, false>; }
// (eight rows per step as for fc32 and sc16 IQ: a HackRF records at 8-20 Msps, where the window is thousands of samples long.  The
// per-wave-counter form of the test build, NFC_WG_FLAGS, is not instantiated for these kinds: the switch is ignored for them.)
template <int K>
ThrKernel wg_of(int nr) { return nr == 8 ? k_threshold_wg<K, 8> : k_threshold_wg<K, 4>; }

ThrKernel threshold_kernel(int kind, bool gring) { return kind == IN_IQ_I8 ? threshold_of<IN_IQ_I8>(gring) : threshold_of<IN_IQ_U8>(gring); }
ThrKernel lean_kernel(int kind, bool blk16) { return kind == IN_IQ_I8 ? lean_of<IN_IQ_I8>(blk16) : lean_of<IN_IQ_U8>(blk16); }
ThrKernel wg_kernel(int kind, int nr) { return kind == IN_IQ_I8 ? wg_of<IN_IQ_I8>(nr) : wg_of<IN_IQ_U8>(nr); }
ThrKernel wg_ex_kernel(int kind) { return kind == IN_IQ_I8 ? k_threshold_wg<IN_IQ_I8, 4, true> : k_threshold_wg<IN_IQ_U8, 4, true>; }
FillKernel fill_kernel(int kind) { return kind == IN_IQ_I8 ? k_fill<IN_IQ_I8> : k_fill<IN_IQ_U8>; }
SeqKernel seq_kernel(int kind) { return kind == IN_IQ_I8 ? k_threshold_seq<IN_IQ_I8> : k_threshold_seq<IN_IQ_U8>; }

}  // namespace iq8
}  // namespace nfc
