// nfc_ctx_commands.hip -- the kernels of ctx_commands.hip.h in a translation unit of their own (that header says what they compute,
// DESIGN.md 8o why they have this form), their launch, and nfc_host_commands_segmented, their twin on the CPU.  nfc_amd.hip
// (nfc_track_commands, nfc_read_commands ...) reaches them through ctxcmd::launch.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"
#include "launch_check.h"
#define NFC_CTX_COMMANDS_KERNELS
#include "ctx_commands.hip.h"

namespace nfc {
namespace ctxcmd {

void launch(const Args &A, hipStream_t stream, const hipEvent_t *ev) {
    const uint32_t most = std::max(A.cap_fr0, A.cap_fr1);
    NFC_LAUNCH(k_ctx_merge, dim3(std::max(1u, (most + MG_THREADS - 1) / MG_THREADS), 2), dim3(MG_THREADS), 0, stream, A);
    NFC_LAUNCH(k_ctx_segments, dim3(1), dim3(SG_THREADS), 0, stream, A);
    if (ev) (void)hipEventRecord(ev[0], stream);
    NFC_LAUNCH(k_ctx_walk, dim3((A.cap_seg + THREADS - 1) / THREADS), dim3(THREADS), 0, stream, A);
    if (ev) (void)hipEventRecord(ev[1], stream);
    NFC_LAUNCH(k_ctx_resolve, dim3(1), dim3(THREADS), 0, stream, A);
    if (ev) (void)hipEventRecord(ev[2], stream);
}

namespace {
// the twin's accessor: frame m of the caller's merged list, its slot the sum of the raw n_bytes before it
struct HostFrames {
    const nfc_raw_frame *merged;
    const uint8_t *bytes0, *par0, *bytes1, *par1;
    const uint32_t *slots;
    uint32_t *cmd;
    uint8_t *data;
    uint16_t *enc;
    Frame get(uint32_t m) const {
        const nfc_raw_frame &r = merged[m];
        Frame f;
        f.type = r.type;
        f.flags = r.flags;
        f.n = (r.flags & NFC_RAW_CUT) ? 0u : r.n_bytes;
        f.slot = slots[m];
        const uint8_t *b = r.type ? bytes1 : bytes0, *p = r.type ? par1 : par0;
        f.bytes = f.n ? b + r.byte_off : nullptr;
        f.par = f.n ? p + r.byte_off : nullptr;
        return f;
    }
};
}  // namespace

}  // namespace ctxcmd
}  // namespace nfc

using namespace nfc;

extern "C" int nfc_host_commands_segmented(nfc_fsm_state *st, const nfc_fsm_key_table *table, const nfc_raw_frame *merged, size_t n,
                                           const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1, nfc_frame *out,
                                           uint8_t *data, uint16_t *enc, size_t cap, size_t *used, const uint32_t *segment_order, size_t n_order,
                                           nfc_ctx_command_counters *counters) {
    using namespace ctxcmd;
    static_assert(sizeof(nfc_frame) == 28, "nfc_frame is seven words");
    if (!st || fsmd::state_fault(*st) || (n && (!merged || !out)) || n > 0x7FFFFFFFull) return NFC_ERR_ARG;
    if (table && skeys::table_fault(*table)) return NFC_ERR_ARG;
    if (n_order && !segment_order) return NFC_ERR_ARG;
    // the slots, checked as nfc_host_commands_keyed checks them
    std::vector<uint32_t> slots(n + 1, 0u);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const nfc_raw_frame &r = merged[i];
        if (r.type != 0 && r.type != 1) return NFC_ERR_ARG;
        const size_t nb = (r.flags & NFC_RAW_CUT) ? 0 : r.n_bytes;
        const uint8_t *b = r.type ? bytes1 : bytes0, *p = r.type ? par1 : par0;
        if (nb && (!b || !p || !data || !enc)) return NFC_ERR_ARG;
        if (at + nb > cap || at + nb > 0xFFFFFFFFull) return NFC_ERR_ARG;
        slots[i] = (uint32_t)at;
        at += nb;
    }
    slots[n] = (uint32_t)at;
    // the segments
    std::vector<uint32_t> seg_start;
    if (n) seg_start.push_back(0u);
    for (size_t m = 1; m < n; m++) {
        const nfc_raw_frame &r = merged[m];
        const uint32_t nb = (r.flags & NFC_RAW_CUT) ? 0u : r.n_bytes;
        const uint32_t b0 = nb >= 1u ? (r.type ? bytes1 : bytes0)[r.byte_off] : 0u;
        if (is_cut(r.type, r.flags, nb, b0)) seg_start.push_back((uint32_t)m);
    }
    const size_t S = seg_start.size();
    seg_start.push_back((uint32_t)n);
    // the order of the speculative walks: every segment once
    std::vector<uint32_t> order;
    if (!segment_order) {
        for (size_t k = 0; k < S; k++) order.push_back((uint32_t)k);
    } else {
        std::vector<uint8_t> seen(S, 0);
        for (size_t j = 0; j < n_order; j++) {
            const uint32_t k = segment_order[j];
            if (k >= S) continue;
            if (seen[k]) return NFC_ERR_ARG;
            seen[k] = 1;
            order.push_back(k);
        }
        if (order.size() != S) return NFC_ERR_ARG;
    }
    const skeys::HostTable keys = {table};
    const HostFrames F = {merged, bytes0, par0, bytes1, par1, slots.data(), (uint32_t *)out, data, enc};
    fsmd::Machine M0;
    fsmd::machine_from_state(M0, *st);
    const int32_t assumed = M0.cur_key;
    std::vector<fsmd::Machine> sum(S);
    std::vector<uint32_t> meta(S, 0u);
    nfc_ctx_command_counters cn = {(uint32_t)S, 0u, 0u, 0u};
    for (const uint32_t k : order) {
        fsmd::Machine M = M0;
        if (k) speculative_start(M);
        walk(M, meta[k], F, seg_start[k], seg_start[k + 1], keys);
        if (k == 0) meta[k] = M_WROTE_KEY | M_WROTE_SESS | M_EXACT;
        else if (meta[k] & M_READ_KEY) cn.n_keydep_segments++;
        sum[k] = M;
    }
    // the resolve
    fsmd::Machine T = S ? sum[0] : M0;
    for (size_t k = 1; k < S; k++) {
        if (stands(meta[k], T.encrypted, T.cur_key, assumed)) {
            fsmd::Machine E = sum[k];
            compose(E, meta[k], T);
            T = E;
        } else {
            uint32_t unused = 0;
            walk(T, unused, F, seg_start[k], seg_start[k + 1], keys);
            cn.n_rerun_segments++;
            cn.n_rerun_frames += seg_start[k + 1] - seg_start[k];
        }
    }
    fsmd::machine_to_state(T, *st);
    if (used) *used = at;
    if (counters) *counters = cn;
    return NFC_OK;
}
