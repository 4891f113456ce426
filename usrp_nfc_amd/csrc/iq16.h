// iq16.h -- what nfc_amd.hip reaches of nfc_iq16.hip: the threshold-stage kernels of the complex int16 input kind
// (NFC_IN_IQ_I16, sc16), which live in a translation unit of their own -- nfc_amd.hip's device code stays exactly what it is
// without them (tests/test_isa_audit.py pins its instantiations).  The host side launches them through these pointers
// (host_context.h) and asks the runtime about them (nfc_create: LDS attribute, occupancy).
#pragma once

namespace nfc {

using ThrKernel = void (*)(ThrArgs);
using SeqKernel = void (*)(SeqArgs);
using FillKernel = void (*)(const void *, uint32_t, float, int, float *, Carry *, EdgeCarryInit, uint8_t *, int, CertSummary *, StateInit,
                            uint32_t *, uint32_t, int);   // (k_fill)

namespace iq16 {
ThrKernel threshold_kernel(bool gring);   // k_threshold<IN_IQ_I16, 4, gring>
ThrKernel lean_kernel(bool blk16);        // k_threshold_lean<IN_IQ_I16, 4, blk16>
ThrKernel wg_kernel(int nr);              // k_threshold_wg<IN_IQ_I16, nr>: pass 0, four or eight rows per step
ThrKernel wg_ex_kernel();                 // k_threshold_wg<IN_IQ_I16, 4, true>: re-runs with failed rounds evaluated in place
FillKernel fill_kernel();                 // k_fill<IN_IQ_I16>
SeqKernel seq_kernel();                   // k_threshold_seq<IN_IQ_I16>
}  // namespace iq16

}  // namespace nfc
