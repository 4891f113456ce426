// multi_commands.hip.h -- k_multi_commands: the protocol machine of fsm.hip.h, a lane per stream, over the frames the assembly kernels
// (nfc_frames.hip: launch_multi) left in the packed buffer; and what nfc_multi.hip reaches of nfc_commands.hip.
//
// 64 streams per workgroup, one wave, as k_multi (multi.hip.h).  The lane loads its stream's machine from the [word][stream] arrays,
// walks the stream's two raw-frame lists with two pointers -- by idx, type 0 first on a tie: the order of api._merge_frames -- runs
// every frame through fsmd::process_frame and stores the machine back.  No scan of its own: in the merged order stream k's commands
// start at frame_off[0][k] + frame_off[1][k] and its byte slots at byte_off[0][k] + byte_off[1][k], both in the table
// k_multi_frames_scan wrote; a frame's slot inside the stream is a running sum in the lane.  Lanes of one wave sit in different
// branches of the lookup and in or out of a session: accepted, as k_multi accepts it in its decoders.
//
// The buffer: the frames' part as frames::MultiLayout lays it out, then the sections of Layout, each on 16 bytes and followed by
// guard_bytes of the guard word.  Every range is cut to what the HOST laid out: the device's counts cannot write past a section.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nfc_amd.h"
#include "frames.hip.h"
#include "emu.hip.h"
#include "fsm.hip.h"

namespace nfc {
namespace commands {

enum { SEC_CMD_OFF, SEC_CBYTE_OFF, SEC_FLAGS, SEC_CMD, SEC_SRC, SEC_DATA, SEC_ENC, SEC_COUNT };
struct Layout {
    uint64_t at[SEC_COUNT], end[SEC_COUNT];   // section starts; where each section's guard starts
    uint64_t total_cmds, total_bytes;         // the HOST's totals (total_bytes: the room of both byte sections of the frames)
};
struct Args {
    frames::MultiArgs R;   // the frames' part: what launch_multi was given
    uint32_t *state;       // [fsmd::W_WORDS][K]
    Layout L;
    const uint32_t *sector_keys;   // [skeys::SLOTS][2][K] (sector_keys.h), or null: no stream of the context was ever given a sector key
};
constexpr int THREADS = 64;

// The EMULATING form: a stream that was given a card (nfc_multi_emulate) answers what it hears.  k_multi_commands_emu is
// k_multi_commands' walk with one step more per frame: after a command of the OTHER side's type the lane runs the card's emulator
// (emu.hip.h: replay_step) and passes the answer through its OWN machine's outgoing, so the machine has advanced before the next heard
// frame is decrypted -- which is why this cannot be a kernel behind the machine kernel.  A context launches it only while a stream holds a
// card; otherwise it launches k_multi_commands, whose text is not touched.
// The cards live on the device from push to push: memory [64][K] units of 16 bytes and nonces [64][K] words as emu.hip.h's DevCard
// reads them (lanes that serve the same block load neighbouring units), params [EP_WORDS][K], the emulators' state [emu::EW_WORDS][K].
// The answers go behind the commands' sections, each on 16 bytes and followed by the guard word: stream k's answers are records
// [cmd_off[k], cmd_off[k] + ans_n[k]) -- at most one per command, so the commands' own offsets place them and no scan is needed --, a
// record's bytes at 18 * its index in ans_plain / ans_air / ans_par.
enum { EP_PRESENT, EP_ROLE, EP_TAG_TYPE, EP_MODE, EP_N_RANDS, EP_WORDS };
enum { ESEC_N, ESEC_REC, ESEC_PLAIN, ESEC_AIR, ESEC_PAR, ESEC_SCRATCH, ESEC_COUNT };
constexpr uint32_t ANS_BYTES = 18;
struct EmuArgs {
    const uint32_t *mem, *rands, *params;
    uint32_t *state;
    uint64_t at[ESEC_COUNT], end[ESEC_COUNT];
};
void launch_emu(const Args &A, const EmuArgs &E, hipStream_t stream, hipEvent_t e0, hipEvent_t e1);

void launch(const Args &A, hipStream_t stream, hipEvent_t e0, hipEvent_t e1);
// streams [k0, k1): the state of nfc_fsm_state_init / the two keys (48 bits, byte 0 lowest)
void launch_init(uint32_t *state, uint32_t K, uint32_t k0, uint32_t k1, hipStream_t stream);
void launch_set_keys(uint32_t *state, uint32_t K, uint32_t k0, uint32_t k1, uint64_t key_a, uint64_t key_b, hipStream_t stream);
// one stream's machine to (set == 0) or from blob[0 .. W_WORDS)
void launch_io(uint32_t *state, uint32_t K, uint32_t k, int set, uint32_t *blob, hipStream_t stream);
// the sector key tables, [skeys::SLOTS][2][K]: streams [k0, k1) all get the skeys::WORDS words of `blob` (null: emptied); one stream's
// table to (set == 0) or from blob[0 .. skeys::WORDS).  Their only writers; k_multi_commands only reads them.
void launch_set_table(uint32_t *tables, uint32_t K, uint32_t k0, uint32_t k1, const uint32_t *blob, hipStream_t stream);
void launch_table_io(uint32_t *tables, uint32_t K, uint32_t k, int set, uint32_t *blob, hipStream_t stream);

#ifdef NFC_COMMANDS_KERNELS
// (three waves per SIMD, as before the sector key look-up: left alone the allocator takes 169 registers with it, one past the step)
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3))) void k_multi_commands(Args A) {
    const frames::MultiArgs &R = A.R;
    const Layout &L = A.L;
    uint8_t *__restrict__ buf = R.packed;
    if (blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < (uint32_t)SEC_COUNT * R.guard_bytes; i += THREADS) {
            const uint32_t s = i / R.guard_bytes, b = i % R.guard_bytes;
            buf[L.end[s] + b] = (uint8_t)(R.guard_word >> (8 * (b & 3u)));
        }
    const uint32_t K = R.K, k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= K) return;
    const size_t T = (size_t)K + 1;
    const uint64_t *__restrict__ tab = R.table;
    // the stream's raw frames per type, cut to the sections as the assembly cut them (named per type: no array a lane would index)
    uint32_t nfr0, nfr1;
    const nfc_raw_frame *rec0, *rec1;
    const uint8_t *rb0, *rb1, *rp0, *rp1;
    uint64_t room0, room1;   // bytes of the type's section from the stream's first on
#define NFC_STREAM_PART(t, nfr, rec, rb, rp, room)                                     \
    {                                                                                  \
        uint64_t fe = tab[(size_t)t * T + k + 1], fb = tab[(size_t)t * T + k];         \
        fe = fe < R.F.total_frames[t] ? fe : R.F.total_frames[t];                      \
        fb = fb < fe ? fb : fe;                                                        \
        uint64_t bb = tab[(size_t)(2 + t) * T + k];                                    \
        bb = bb < R.F.total_bytes[t] ? bb : R.F.total_bytes[t];                        \
        nfr = (uint32_t)(fe - fb);                                                     \
        rec = (const nfc_raw_frame *)(buf + R.F.at_fr[t]) + fb;                        \
        rb = buf + R.F.at_bytes[t] + bb;                                               \
        rp = buf + R.F.at_par[t] + bb;                                                 \
        room = R.F.total_bytes[t] - bb;                                                \
    }
    NFC_STREAM_PART(0, nfr0, rec0, rb0, rp0, room0)
    NFC_STREAM_PART(1, nfr1, rec1, rb1, rp1, room1)
#undef NFC_STREAM_PART
    const uint64_t c0 = tab[0 * T + k] + tab[1 * T + k], b0 = tab[2 * T + k] + tab[3 * T + k];
    uint64_t *cmd_off = (uint64_t *)(buf + L.at[SEC_CMD_OFF]), *cbyte_off = (uint64_t *)(buf + L.at[SEC_CBYTE_OFF]);
    cmd_off[k] = c0;
    cbyte_off[k] = b0;
    if (k == K - 1u) {
        cmd_off[K] = tab[0 * T + K] + tab[1 * T + K];
        cbyte_off[K] = tab[2 * T + K] + tab[3 * T + K];
    }
    fsmd::Machine M;
    fsmd::load_machine(M, A.state, K, k);
    const skeys::DeviceTable keys = {A.sector_keys, K, k};   // (two words of it are read at an AUTH command and at the nonce that follows)
    {   // what the slabs did not store is lost to the machine
        const uint32_t *c = R.counts + (size_t)k * R.cnt_words;
        if (c[R.cnt_pk0] > R.cap_packets || c[R.cnt_pk0 + 1] > R.cap_packets || c[R.cnt_bits0] > R.cap_bits || c[R.cnt_bits0 + 1] > R.cap_bits)
            M.flags |= NFC_FSM_LOST;
    }
    uint32_t *__restrict__ out_cmd = (uint32_t *)(buf + L.at[SEC_CMD]);
    uint32_t *__restrict__ out_src = (uint32_t *)(buf + L.at[SEC_SRC]);
    uint8_t *__restrict__ out_data = buf + L.at[SEC_DATA];
    uint16_t *__restrict__ out_enc = (uint16_t *)(buf + L.at[SEC_ENC]);
    uint32_t i0 = 0, i1 = 0, run = 0;
    while (i0 < nfr0 || i1 < nfr1) {
        int t;
        if (i1 >= nfr1) t = 0;
        else if (i0 >= nfr0) t = 1;
        else t = rec0[i0].idx <= rec1[i1].idx ? 0 : 1;
        const uint32_t i = t ? i1 : i0;
        const uint4 *q = (const uint4 *)(t ? rec1 + i1 : rec0 + i0);
        const uint4 q0 = q[0], q1 = q[1];
        uint32_t byte_off = q0.z, n = q1.x, flags = q1.y;
        const uint8_t *rbt = t ? rb1 : rb0, *rpt = t ? rp1 : rp0;
        const uint64_t roomt = t ? room1 : room0;
        const uint64_t c = c0 + i0 + i1;
        if (c >= L.total_cmds) break;   // (never: the host's total is the sum of the streams' frames)
        // (never: a frame's bytes lie inside its type's section, its slot inside the host's room)
        if ((uint64_t)byte_off + n > roomt || b0 + run + n > L.total_bytes) flags = NFC_RAW_CUT;
        if (flags & NFC_RAW_CUT) n = 0;
        const fsmd::Rec r = fsmd::process_frame(M, t, flags, n, rbt + byte_off, rpt + byte_off, out_data + b0 + run, out_enc + b0 + run, keys);
        uint32_t *w = out_cmd + c * (sizeof(nfc_frame) / 4);
        w[0] = (uint32_t)r.cmd;
        w[1] = (uint32_t)r.type;
        w[2] = run;
        w[3] = r.n_bytes | r.n_header << 16;
        w[4] = r.n_extra | r.n_crc << 16;
        w[5] = r.flags;
        w[6] = r.n_enc;
        out_src[c] = (uint32_t)t << 31 | i;
        run += n;
        if (t) i1++;
        else i0++;
    }
    ((uint32_t *)(buf + L.at[SEC_FLAGS]))[k] = M.flags;
    fsmd::store_machine(M, A.state, K, k);
}

__global__ __launch_bounds__(THREADS) void k_multi_commands_emu(Args A, EmuArgs E) {
    const frames::MultiArgs &R = A.R;
    const Layout &L = A.L;
    uint8_t *__restrict__ buf = R.packed;
    if (blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < (uint32_t)(SEC_COUNT + ESEC_COUNT) * R.guard_bytes; i += THREADS) {
            const uint32_t s = i / R.guard_bytes, b = i % R.guard_bytes;
            buf[(s < (uint32_t)SEC_COUNT ? L.end[s] : E.end[s - SEC_COUNT]) + b] = (uint8_t)(R.guard_word >> (8 * (b & 3u)));
        }
    const uint32_t K = R.K, k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= K) return;
    const size_t T = (size_t)K + 1;
    const uint64_t *__restrict__ tab = R.table;
    uint32_t nfr0, nfr1;
    const nfc_raw_frame *rec0, *rec1;
    const uint8_t *rb0, *rb1, *rp0, *rp1;
    uint64_t room0, room1;
#define NFC_STREAM_PART(t, nfr, rec, rb, rp, room)                                     \
    {                                                                                  \
        uint64_t fe = tab[(size_t)t * T + k + 1], fb = tab[(size_t)t * T + k];         \
        fe = fe < R.F.total_frames[t] ? fe : R.F.total_frames[t];                      \
        fb = fb < fe ? fb : fe;                                                        \
        uint64_t bb = tab[(size_t)(2 + t) * T + k];                                    \
        bb = bb < R.F.total_bytes[t] ? bb : R.F.total_bytes[t];                        \
        nfr = (uint32_t)(fe - fb);                                                     \
        rec = (const nfc_raw_frame *)(buf + R.F.at_fr[t]) + fb;                        \
        rb = buf + R.F.at_bytes[t] + bb;                                               \
        rp = buf + R.F.at_par[t] + bb;                                                 \
        room = R.F.total_bytes[t] - bb;                                                \
    }
    NFC_STREAM_PART(0, nfr0, rec0, rb0, rp0, room0)
    NFC_STREAM_PART(1, nfr1, rec1, rb1, rp1, room1)
#undef NFC_STREAM_PART
    const uint64_t c0 = tab[0 * T + k] + tab[1 * T + k], b0 = tab[2 * T + k] + tab[3 * T + k];
    uint64_t *cmd_off = (uint64_t *)(buf + L.at[SEC_CMD_OFF]), *cbyte_off = (uint64_t *)(buf + L.at[SEC_CBYTE_OFF]);
    cmd_off[k] = c0;
    cbyte_off[k] = b0;
    if (k == K - 1u) {
        cmd_off[K] = tab[0 * T + K] + tab[1 * T + K];
        cbyte_off[K] = tab[2 * T + K] + tab[3 * T + K];
    }
    fsmd::Machine M;
    fsmd::load_machine(M, A.state, K, k);
    const skeys::DeviceTable keys = {A.sector_keys, K, k};
    {
        const uint32_t *c = R.counts + (size_t)k * R.cnt_words;
        if (c[R.cnt_pk0] > R.cap_packets || c[R.cnt_pk0 + 1] > R.cap_packets || c[R.cnt_bits0] > R.cap_bits || c[R.cnt_bits0 + 1] > R.cap_bits)
            M.flags |= NFC_FSM_LOST;
    }
    // the stream's card, if it has one, and its emulator
    const bool present = E.params[(size_t)EP_PRESENT * K + k] != 0;
    const int role = (int)E.params[(size_t)EP_ROLE * K + k];
    const uint32_t n_rands = E.params[(size_t)EP_N_RANDS * K + k];
    const emu::DevCard C = {E.mem, E.rands, K, k, n_rands < emu::MAX_RANDS ? n_rands : emu::MAX_RANDS, (int32_t)E.params[(size_t)EP_TAG_TYPE * K + k],
                            (int32_t)E.params[(size_t)EP_MODE * K + k]};
    emu::State S;
    emu::load_state(S, E.state, K, k);
    uint32_t *__restrict__ out_cmd = (uint32_t *)(buf + L.at[SEC_CMD]);
    uint32_t *__restrict__ out_src = (uint32_t *)(buf + L.at[SEC_SRC]);
    uint8_t *__restrict__ out_data = buf + L.at[SEC_DATA];
    uint16_t *__restrict__ out_enc = (uint16_t *)(buf + L.at[SEC_ENC]);
    nfc_emu_answer *__restrict__ ans = (nfc_emu_answer *)(buf + E.at[ESEC_REC]);
    uint8_t *__restrict__ scratch = buf + E.at[ESEC_SCRATCH] + (size_t)k * emu::SCRATCH_BYTES;
    uint32_t i0 = 0, i1 = 0, run = 0, na = 0;
    while (i0 < nfr0 || i1 < nfr1) {
        int t;
        if (i1 >= nfr1) t = 0;
        else if (i0 >= nfr0) t = 1;
        else t = rec0[i0].idx <= rec1[i1].idx ? 0 : 1;
        const uint32_t i = t ? i1 : i0;
        const uint4 *q = (const uint4 *)(t ? rec1 + i1 : rec0 + i0);
        const uint4 q0 = q[0], q1 = q[1];
        uint32_t byte_off = q0.z, n = q1.x, flags = q1.y;
        const uint8_t *rbt = t ? rb1 : rb0, *rpt = t ? rp1 : rp0;
        const uint64_t roomt = t ? room1 : room0;
        const uint64_t c = c0 + i0 + i1;
        if (c >= L.total_cmds) break;
        if ((uint64_t)byte_off + n > roomt || b0 + run + n > L.total_bytes) flags = NFC_RAW_CUT;
        if (flags & NFC_RAW_CUT) n = 0;
        const fsmd::Rec r = fsmd::process_frame(M, t, flags, n, rbt + byte_off, rpt + byte_off, out_data + b0 + run, out_enc + b0 + run, keys);
        uint32_t *w = out_cmd + c * (sizeof(nfc_frame) / 4);
        w[0] = (uint32_t)r.cmd;
        w[1] = (uint32_t)r.type;
        w[2] = run;
        w[3] = r.n_bytes | r.n_header << 16;
        w[4] = r.n_extra | r.n_crc << 16;
        w[5] = r.flags;
        w[6] = r.n_enc;
        out_src[c] = (uint32_t)t << 31 | i;
        if (present && c0 + na < L.total_cmds) {   // (an answer per command at the most: c0 + na <= c)
            const uint64_t slot = (c0 + na) * ANS_BYTES;
            uint8_t *air = buf + E.at[ESEC_AIR] + slot, *par = buf + E.at[ESEC_PAR] + slot, *plain = buf + E.at[ESEC_PLAIN] + slot;
            emu::Ans a;
            const int cmd = emu::replay_step(S, C, role, M, keys, r, out_data + b0 + run, a, air, par, scratch);
            if (cmd >= 0) {
                bool differs = false;
                for (uint32_t j = 0; j < ANS_BYTES; j++) {
                    const uint32_t pb = j < a.n ? a.B.at(j) : 0u;
                    plain[j] = (uint8_t)pb;
                    differs = differs || pb != air[j];
                }
                nfc_emu_answer rec;
                rec.src = (uint32_t)(i0 + i1), rec.cmd = cmd, rec.byte_off = na * ANS_BYTES, rec.n_bytes = (uint16_t)a.n;
                rec.n_bits = (uint16_t)((cmd == fsmd::C_REQA || cmd == fsmd::C_WUPA) ? 7u : 9u * a.n);
                rec.flags = differs ? NFC_EMU_FRAME_ENCRYPTED : 0u, rec.reserved = 0;
                ans[c0 + na] = rec;
                na++;
            }
        }
        run += n;
        if (t) i1++;
        else i0++;
    }
    ((uint32_t *)(buf + E.at[ESEC_N]))[k] = na;
    ((uint32_t *)(buf + L.at[SEC_FLAGS]))[k] = M.flags;
    fsmd::store_machine(M, A.state, K, k);
    if (present) emu::store_state(S, E.state, K, k);
}

__global__ __launch_bounds__(256) void k_commands_init(uint32_t *state, uint32_t K, uint32_t k0, uint32_t k1) {
    const uint32_t k = k0 + blockIdx.x * 256 + threadIdx.x;
    if (k >= k1 || k >= K) return;
    fsmd::Machine M;
    fsmd::machine_init(M);
    fsmd::store_machine(M, state, K, k);
}
__global__ __launch_bounds__(256) void k_commands_set_keys(uint32_t *state, uint32_t K, uint32_t k0, uint32_t k1, uint64_t key_a, uint64_t key_b) {
    using namespace fsmd;
    const size_t k = (size_t)k0 + blockIdx.x * 256 + threadIdx.x;
    if (k >= k1 || k >= K) return;
    state[W_KA_LO * (size_t)K + k] = (uint32_t)key_a;
    state[W_KA_HI * (size_t)K + k] = (uint32_t)(key_a >> 32);
    state[W_KB_LO * (size_t)K + k] = (uint32_t)key_b;
    state[W_KB_HI * (size_t)K + k] = (uint32_t)(key_b >> 32);
}
__global__ __launch_bounds__(64) void k_commands_io(uint32_t *state, uint32_t K, uint32_t k, int set, uint32_t *blob) {
    const uint32_t w = threadIdx.x;
    if (w >= (uint32_t)fsmd::W_WORDS || k >= K) return;
    if (set) state[(size_t)w * K + k] = blob[w];
    else blob[w] = state[(size_t)w * K + k];
}
// a thread per (stream of [k0, k1) ∩ [0, K), word): neighbouring threads write neighbouring streams of one word
__global__ __launch_bounds__(256) void k_commands_set_table(uint32_t *tables, uint32_t K, uint32_t k0, uint32_t k1, const uint32_t *blob) {
    const size_t k = (size_t)k0 + blockIdx.x * 256 + threadIdx.x;
    const uint32_t w = blockIdx.y;
    if (k >= k1 || k >= K || w >= skeys::WORDS) return;
    tables[(size_t)w * K + k] = blob ? blob[w] : 0u;
}
__global__ __launch_bounds__(256) void k_commands_table_io(uint32_t *tables, uint32_t K, uint32_t k, int set, uint32_t *blob) {
    const uint32_t w = threadIdx.x;
    if (w >= skeys::WORDS || k >= K) return;
    if (set) tables[(size_t)w * K + k] = blob[w];
    else blob[w] = tables[(size_t)w * K + k];
}
#endif   // NFC_COMMANDS_KERNELS

}  // namespace commands
}  // namespace nfc
