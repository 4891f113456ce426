// nfc_emu.hip -- the emulators' translation unit: k_emulate_pairs, a lane per (tag, reader) pair over the closed loop of emu.hip.h, its
// twin on the CPU, and the C ABI of the emulation (include/nfc_amd.h: nfc_emu_*, nfc_host_emu_step, nfc_host_emulate_pairs,
// nfc_emulate_pairs_device).  DESIGN.md 8k.
//
// 64 pairs per workgroup, one wave, as k_multi_commands.  A lane keeps both emulators and both protocol machines in registers and walks
// its pair's whole transaction; lanes of one wave sit in different branches (a tag's lane answers while its neighbour's reader asks
// only when their cards differ: pairs of one kind of card stay in step).
//
// THE DEVICE BUFFER of one call, every section on 256 bytes:
//   mem          [64][K] units of 16 bytes: unit u of pair k's tag memory (an Ultralight fills four units).  A READR takes one unit;
//                lanes that read the same block -- whole-card reads in step -- load neighbouring units.  Whether that matters is not measured.
//   tag_rands    [64][K] words, reader_rands [64][K] words: nonce i of pair k
//   params       [K] PairParams
//   tables       [skeys::SLOTS][2][K] words (sector_keys.h: DeviceTable), only when a reader has a table
//   results, frames, plain, air, par, scratch: the outputs, pair-major (a pair's slab is its lane's alone), each followed by GUARD_BYTES
//                of the guard word, which the call checks after the kernel.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"
#include "dev_buf.h"
#include "emu.hip.h"
#include "launch_check.h"

static_assert(sizeof(nfc_emu_state) == 88, "nfc_emu_state is 88 bytes");
static_assert(sizeof(nfc_emu_card) == 64, "nfc_emu_card is 64 bytes");
static_assert(sizeof(nfc_emu_answer) == 24, "nfc_emu_answer is 24 bytes");
static_assert(sizeof(nfc_emu_frame) == 16 && sizeof(nfc_emu_pair_result) == 32 && sizeof(nfc_emu_config) == 32, "the transcript's records");

namespace nfc {
namespace emu {

constexpr int THREADS = 64;
constexpr uint32_t GUARD_WORD = 0x5AFEC0DEu, GUARD_BYTES = 16;
constexpr uint32_t MEM_UNITS = CLASSIC_BYTES / 16;

struct PairParams {   // 48 bytes
    int32_t tag_type, tag_mode, reader_mode;
    uint32_t n_tag_rands, n_reader_rands, cap_frames;   // cap_frames: the pair's own, at most the call's
    uint64_t key_a, key_b;   // the reader's
    uint64_t pad2;
};
struct PairArgs {
    const uint32_t *mem, *tag_rands, *reader_rands;
    const PairParams *params;
    const uint32_t *tables;   // or null: no reader of the call has one
    uint32_t K, link, rounds, cap_frames, cap_bytes;
    nfc_emu_pair_result *results;
    nfc_emu_frame *frames;
    uint8_t *plain, *air, *par, *scratch;
};

__global__ __launch_bounds__(THREADS) void k_emulate_pairs(PairArgs A) {
    const uint32_t K = A.K, k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= K) return;
    const PairParams P = A.params[k];
    const DevCard T = {A.mem, A.tag_rands, K, k, P.n_tag_rands < MAX_RANDS ? P.n_tag_rands : MAX_RANDS, P.tag_type, P.tag_mode};
    const DevReader R = {A.reader_rands, K, k, P.n_reader_rands < MAX_RANDS ? P.n_reader_rands : MAX_RANDS, P.reader_mode};
    const skeys::DeviceTable rtab = {A.tables, K, k};
    const Slab O = {A.frames + (size_t)k * A.cap_frames, A.plain + (size_t)k * A.cap_bytes, A.air + (size_t)k * A.cap_bytes,
                    A.par + (size_t)k * A.cap_bytes, P.cap_frames < A.cap_frames ? P.cap_frames : A.cap_frames, A.cap_bytes};
    nfc_emu_pair_result r;
    run_pair(T, R, P.key_a & ST_MASK, P.key_b & ST_MASK, rtab, A.link, A.rounds, O, A.scratch + (size_t)k * SCRATCH_BYTES, r);
    A.results[k] = r;
}

// ---- arguments ----
inline char *error_text() {
    static thread_local char msg[160] = "";
    return msg;
}
inline int arg_error(const char *what, const char *name = "", long long index = -1) {
    if (index >= 0) snprintf(error_text(), 160, "%s[%lld]%s", name, index, what);
    else snprintf(error_text(), 160, "%s%s", name, what);
    return NFC_ERR_ARG;
}
inline int pairs_fault(const nfc_emu_card *tags, const nfc_emu_card *readers, size_t n, const nfc_emu_config *cfg, nfc_emu_pair_result *results,
                       nfc_emu_frame *frames, uint8_t *plain, uint8_t *air, uint8_t *par) {
    if (!cfg) return arg_error("cfg is null");
    if (cfg->link != NFC_EMU_LINK_PLAIN && cfg->link != NFC_EMU_LINK_AIR) return arg_error("cfg.link must be NFC_EMU_LINK_PLAIN or NFC_EMU_LINK_AIR");
    if (cfg->rounds < 1 || cfg->rounds > 64) return arg_error("cfg.rounds must be 1 .. 64");
    if (cfg->cap_frames < 1 || cfg->cap_frames > (1u << 16)) return arg_error("cfg.cap_frames must be 1 .. 65536");
    if (cfg->cap_bytes < 1 || cfg->cap_bytes > (1u << 20)) return arg_error("cfg.cap_bytes must be 1 .. 2^20");
    for (int i = 0; i < 2; i++)
        if (cfg->reserved[i]) return arg_error("cfg.reserved must be 0");
    if (n > 65536) return arg_error("n exceeds 65536");
    if ((uint64_t)n * cfg->cap_bytes > (1ull << 30)) return arg_error("n * cfg.cap_bytes exceeds 2^30");
    if (n && (!tags || !readers || !results || !frames || !plain || !air || !par)) return arg_error("a null array");
    if (cfg->pair_cap_frames)
        for (size_t i = 0; i < n; i++)
            if (cfg->pair_cap_frames[i] < 1) return arg_error(" must be at least 1", "cfg.pair_cap_frames", (long long)i);
    for (size_t i = 0; i < n; i++) {
        if (const char *f = card_fault(tags[i], NFC_EMU_TAG)) return arg_error(f, "tags", (long long)i);
        if (const char *f = card_fault(readers[i], NFC_EMU_READER)) return arg_error(f, "readers", (long long)i);
    }
    return NFC_OK;
}
inline uint32_t pair_cap(const nfc_emu_config &c, size_t k) {
    return c.pair_cap_frames && c.pair_cap_frames[k] < c.cap_frames ? c.pair_cap_frames[k] : c.cap_frames;
}
inline HostCard host_card(const nfc_emu_card &c) {
    const HostCard h = {c.mem, c.rands, c.n_rands, c.role == NFC_EMU_TAG ? c.tag_type : -1, c.mode};
    return h;
}

}  // namespace emu
}  // namespace nfc

using namespace nfc;

extern "C" {

int nfc_emu_state_init(nfc_emu_state *st) {
    if (!st) return emu::arg_error("st is null");
    emu::State S;
    emu::state_init(S);
    memset(st, 0, sizeof *st);
    emu::state_to_public(S, *st);
    return NFC_OK;
}

const char *nfc_emu_last_error(void) { return emu::error_text(); }

int nfc_host_emu_step(const nfc_emu_card *card, nfc_emu_state *st, int cmd, const uint8_t *extra, size_t n_extra, int *cmd_out, uint8_t *frame_out,
                      size_t *n_out) {
    if (!card) return emu::arg_error("card is null");
    if (card->role != NFC_EMU_TAG && card->role != NFC_EMU_READER) return emu::arg_error("card.role must be NFC_EMU_TAG or NFC_EMU_READER");
    if (const char *f = emu::card_fault(*card, card->role)) return emu::arg_error(f, "card");
    if (!st) return emu::arg_error("st is null");
    if (const char *f = emu::state_fault(*st)) return emu::arg_error(f, "st: ");
    if (cmd >= fsmd::C_COUNT || cmd < NFC_CMD_PARITY_ERROR) return emu::arg_error("cmd is no command");
    if (n_extra > (size_t)fsmd::MAX_COMMAND_BYTES || (n_extra && !extra)) return emu::arg_error("extra holds at most 18 bytes");
    if (!cmd_out || !frame_out || !n_out) return emu::arg_error("cmd_out, frame_out or n_out is null");
    emu::State S;
    emu::state_from_public(S, *st);
    fsmd::Bytes B = {};   // (the extra bytes alone: the header's length is 0)
    for (size_t i = 0; i < n_extra; i++) B.put((uint32_t)i, extra[i]);
    const emu::HostCard C = emu::host_card(*card);
    const emu::Ans a = card->role == NFC_EMU_TAG ? emu::tag_step(S, C, cmd, B, 0u, (uint32_t)n_extra) : emu::reader_step(S, C, cmd, B, 0u, (uint32_t)n_extra);
    emu::state_to_public(S, *st);
    *cmd_out = a.cmd;
    *n_out = a.cmd < 0 ? 0 : a.n;
    for (uint32_t i = 0; i < (uint32_t)fsmd::MAX_COMMAND_BYTES; i++) frame_out[i] = (a.cmd >= 0 && i < a.n) ? (uint8_t)a.B.at(i) : (uint8_t)0;
    return NFC_OK;
}

int nfc_host_emulate(nfc_fsm_state *st, const nfc_fsm_key_table *table, const nfc_emu_card *card, nfc_emu_state *est, const nfc_raw_frame *merged,
                     size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1, nfc_frame *out, uint8_t *data,
                     uint16_t *enc, size_t cap, size_t *used, nfc_emu_answer *answers, uint8_t *ans_plain, uint8_t *ans_air, uint8_t *ans_par,
                     size_t *n_answers) {
    if (!st) return emu::arg_error("st is null");
    if (const char *f = fsmd::state_fault(*st)) return emu::arg_error(f, "st: ");
    if (table && skeys::table_fault(*table)) return emu::arg_error("table: present must be 0 or 1");
    if (!card) return emu::arg_error("card is null");
    if (card->role != NFC_EMU_TAG && card->role != NFC_EMU_READER) return emu::arg_error("card.role must be NFC_EMU_TAG or NFC_EMU_READER");
    if (const char *f = emu::card_fault(*card, card->role)) return emu::arg_error(f, "card");
    if (!est) return emu::arg_error("est is null");
    if (const char *f = emu::state_fault(*est)) return emu::arg_error(f, "est: ");
    if (n && (!merged || !out || !answers || !ans_plain || !ans_air || !ans_par)) return emu::arg_error("a null array");
    const skeys::HostTable keys = {table};
    const emu::HostCard C = emu::host_card(*card);
    fsmd::Machine M;
    fsmd::machine_from_state(M, *st);
    emu::State S;
    emu::state_from_public(S, *est);
    alignas(16) uint8_t scratch[emu::SCRATCH_BYTES];
    size_t at = 0, na = 0;
    for (size_t i = 0; i < n; i++) {
        const nfc_raw_frame &r = merged[i];
        if (r.type != 0 && r.type != 1) return emu::arg_error("merged: a frame's type is neither 0 nor 1");
        const bool cut = (r.flags & NFC_RAW_CUT) != 0;
        const size_t nb = cut ? 0 : r.n_bytes;
        const uint8_t *b = r.type ? bytes1 : bytes0, *p = r.type ? par1 : par0;
        if (nb && (!b || !p || !data || !enc)) return emu::arg_error("bytes, par, data or enc is null");
        if (at + nb > cap || at + nb > 0xFFFFFFFFull) return emu::arg_error("cap: the frames need more room");
        const fsmd::Rec rec = fsmd::process_frame(M, r.type, r.flags, (uint32_t)nb, b ? b + r.byte_off : nullptr, p ? p + r.byte_off : nullptr,
                                                  data ? data + at : nullptr, enc ? enc + at : nullptr, keys);
        nfc_frame &o = out[i];
        memset(&o, 0, sizeof o);
        o.cmd = rec.cmd, o.type = rec.type, o.byte_off = (uint32_t)at, o.flags = rec.flags;
        o.n_bytes = (uint16_t)rec.n_bytes, o.n_header = (uint16_t)rec.n_header, o.n_extra = (uint16_t)rec.n_extra;
        o.n_crc = (uint16_t)rec.n_crc, o.n_enc = (uint16_t)rec.n_enc;
        const size_t slot = na * (size_t)fsmd::MAX_COMMAND_BYTES;
        emu::Ans a;
        const int cmd = emu::replay_step(S, C, card->role, M, keys, rec, data ? data + at : nullptr, a, ans_air + slot, ans_par + slot, scratch);
        if (cmd >= 0) {
            nfc_emu_answer &w = answers[na];
            memset(&w, 0, sizeof w);
            bool differs = false;
            for (uint32_t j = 0; j < (uint32_t)fsmd::MAX_COMMAND_BYTES; j++) {
                ans_plain[slot + j] = j < a.n ? (uint8_t)a.B.at(j) : (uint8_t)0;
                differs = differs || ans_plain[slot + j] != ans_air[slot + j];
            }
            w.src = (uint32_t)i, w.cmd = cmd, w.byte_off = (uint32_t)slot, w.n_bytes = (uint16_t)a.n, w.n_bits = (uint16_t)((cmd == fsmd::C_REQA || cmd == fsmd::C_WUPA) ? 7u : 9u * a.n);
            w.flags = differs ? NFC_EMU_FRAME_ENCRYPTED : 0u;
            na++;
        }
        at += nb;
    }
    fsmd::machine_to_state(M, *st);
    emu::state_to_public(S, *est);
    if (used) *used = at;
    if (n_answers) *n_answers = na;
    return NFC_OK;
}

int nfc_host_emulate_pairs(const nfc_emu_card *tags, const nfc_emu_card *readers, size_t n, const nfc_emu_config *cfg, nfc_emu_pair_result *results,
                           nfc_emu_frame *frames, uint8_t *plain, uint8_t *air, uint8_t *par) {
    if (const int rc = emu::pairs_fault(tags, readers, n, cfg, results, frames, plain, air, par)) return rc;
    if (n == 0) return NFC_OK;
    memset(results, 0, n * sizeof *results);
    memset(frames, 0, n * cfg->cap_frames * sizeof *frames);
    memset(plain, 0, n * (size_t)cfg->cap_bytes);
    memset(air, 0, n * (size_t)cfg->cap_bytes);
    memset(par, 0, n * (size_t)cfg->cap_bytes);
    alignas(16) uint8_t scratch[emu::SCRATCH_BYTES];
    for (size_t k = 0; k < n; k++) {
        const emu::HostCard T = emu::host_card(tags[k]), R = emu::host_card(readers[k]);
        const skeys::HostTable rtab = {readers[k].table};
        const emu::Slab O = {frames + k * cfg->cap_frames, plain + k * (size_t)cfg->cap_bytes, air + k * (size_t)cfg->cap_bytes,
                             par + k * (size_t)cfg->cap_bytes, emu::pair_cap(*cfg, k), cfg->cap_bytes};
        memset(scratch, 0, sizeof scratch);
        emu::run_pair(T, R, fsmd::key_of(readers[k].key_a), fsmd::key_of(readers[k].key_b), rtab, cfg->link, cfg->rounds, O, scratch, results[k]);
    }
    return NFC_OK;
}

int nfc_emulate_pairs_device(int device, const nfc_emu_card *tags, const nfc_emu_card *readers, size_t n, const nfc_emu_config *cfg,
                             nfc_emu_pair_result *results, nfc_emu_frame *frames, uint8_t *plain, uint8_t *air, uint8_t *par, float *kernel_ms) {
    if (const int rc = emu::pairs_fault(tags, readers, n, cfg, results, frames, plain, air, par)) return rc;
    if (device < 0) return emu::arg_error("device is negative");
    if (kernel_ms) *kernel_ms = 0.f;
    if (n == 0) return NFC_OK;
    const size_t K = n;
    // the input image, built on the host
    bool any_table = false;
    for (size_t k = 0; k < K; k++) any_table = any_table || readers[k].table != nullptr;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_mem = 0, o_trands = o_mem + up((size_t)emu::MEM_UNITS * K * 16), o_rrands = o_trands + up((size_t)emu::MAX_RANDS * K * 4),
                 o_params = o_rrands + up((size_t)emu::MAX_RANDS * K * 4), o_tables = o_params + up(K * sizeof(emu::PairParams)),
                 in_bytes = o_tables + (any_table ? up((size_t)skeys::WORDS * K * 4) : 0);
    const size_t G = emu::GUARD_BYTES;
    const size_t s_res = K * sizeof(nfc_emu_pair_result), s_fr = K * cfg->cap_frames * sizeof(nfc_emu_frame), s_by = K * (size_t)cfg->cap_bytes,
                 s_scr = K * (size_t)emu::SCRATCH_BYTES;
    const size_t o_res = in_bytes, o_fr = o_res + up(s_res + G), o_plain = o_fr + up(s_fr + G), o_air = o_plain + up(s_by + G), o_par = o_air + up(s_by + G),
                 o_scr = o_par + up(s_by + G), total = o_scr + up(s_scr + G);
    std::vector<uint8_t> image(in_bytes, 0);
    {
        uint32_t *mem = (uint32_t *)(image.data() + o_mem), *tr = (uint32_t *)(image.data() + o_trands), *rr = (uint32_t *)(image.data() + o_rrands);
        emu::PairParams *pp = (emu::PairParams *)(image.data() + o_params);
        uint32_t *tb = any_table ? (uint32_t *)(image.data() + o_tables) : nullptr;
        for (size_t k = 0; k < K; k++) {
            const nfc_emu_card &t = tags[k], &r = readers[k];
            const emu::HostCard T = emu::host_card(t), R = emu::host_card(r);
            for (uint32_t i = 0; i < t.mem_len / 4; i++) mem[((size_t)(i >> 2) * K + k) * 4 + (i & 3)] = T.mem_word(i);
            for (uint32_t i = 0; i < t.n_rands; i++) tr[(size_t)i * K + k] = T.rand(i);
            for (uint32_t i = 0; i < r.n_rands; i++) rr[(size_t)i * K + k] = R.rand(i);
            emu::PairParams P = {};
            P.tag_type = t.tag_type, P.tag_mode = t.mode, P.reader_mode = r.mode, P.n_tag_rands = t.n_rands, P.n_reader_rands = r.n_rands, P.cap_frames = emu::pair_cap(*cfg, k);
            P.key_a = fsmd::key_of(r.key_a), P.key_b = fsmd::key_of(r.key_b);
            pp[k] = P;
            if (tb && r.table)
                for (uint32_t slot = 0; slot < skeys::SLOTS; slot++) {
                    uint64_t key = 0;
                    const bool has = skeys::HostTable{r.table}.get(slot, key);
                    tb[(size_t)slot * 2 * K + k] = has ? skeys::word_lo(key) : 0u;
                    tb[(size_t)slot * 2 * K + K + k] = skeys::word_hi(key, has);
                }
        }
    }
    if (hipSetDevice(device) != hipSuccess) return NFC_ERR_DEVICE;
    LaunchError launch;
    LaunchScope scope(&launch);
    DevBuf buf;
    Event e0, e1;
    const hipError_t ea = buf.ensure(total);
    if (ea != hipSuccess) return ea == hipErrorOutOfMemory ? NFC_ERR_NOMEM : NFC_ERR_DEVICE;
    uint8_t *d = buf.as<uint8_t>();
    if (hipMemcpy(d, image.data(), in_bytes, hipMemcpyHostToDevice) != hipSuccess) return NFC_ERR_DEVICE;
    if (hipMemsetAsync(d + in_bytes, 0, total - in_bytes, 0) != hipSuccess) return NFC_ERR_DEVICE;
    const size_t guard_at[6] = {o_res + s_res, o_fr + s_fr, o_plain + s_by, o_air + s_by, o_par + s_by, o_scr + s_scr};
    for (size_t g : guard_at)
        if (hipMemsetD32Async((hipDeviceptr_t)(d + g), (int)emu::GUARD_WORD, G / 4, 0) != hipSuccess) return NFC_ERR_DEVICE;
    emu::PairArgs A = {};
    A.mem = (const uint32_t *)(d + o_mem), A.tag_rands = (const uint32_t *)(d + o_trands), A.reader_rands = (const uint32_t *)(d + o_rrands);
    A.params = (const emu::PairParams *)(d + o_params);
    A.tables = any_table ? (const uint32_t *)(d + o_tables) : nullptr;
    A.K = (uint32_t)K, A.link = cfg->link, A.rounds = cfg->rounds, A.cap_frames = cfg->cap_frames, A.cap_bytes = cfg->cap_bytes;
    A.results = (nfc_emu_pair_result *)(d + o_res), A.frames = (nfc_emu_frame *)(d + o_fr);
    A.plain = d + o_plain, A.air = d + o_air, A.par = d + o_par, A.scratch = d + o_scr;
    const dim3 grid((unsigned)((K + emu::THREADS - 1) / emu::THREADS)), block(emu::THREADS);
    if (kernel_ms) {
        if (e0.create() != hipSuccess || e1.create() != hipSuccess) return NFC_ERR_DEVICE;
        NFC_LAUNCH_EXT(emu::k_emulate_pairs, grid, block, 0, 0, e0, e1, 0, A);
    } else {
        NFC_LAUNCH(emu::k_emulate_pairs, grid, block, 0, 0, A);
    }
    if (launch.err != hipSuccess) return NFC_ERR_DEVICE;
    uint32_t guards[6][4];
    if (hipMemcpy(results, d + o_res, s_res, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(frames, d + o_fr, s_fr, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(plain, d + o_plain, s_by, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(air, d + o_air, s_by, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(par, d + o_par, s_by, hipMemcpyDeviceToHost) != hipSuccess)
        return NFC_ERR_DEVICE;
    for (int g = 0; g < 6; g++)
        if (hipMemcpy(guards[g], d + guard_at[g], G, hipMemcpyDeviceToHost) != hipSuccess) return NFC_ERR_DEVICE;
    if (kernel_ms && hipEventElapsedTime(kernel_ms, e0, e1) != hipSuccess) return NFC_ERR_DEVICE;
    for (int g = 0; g < 6; g++)
        for (int w = 0; w < 4; w++)
            if (guards[g][w] != emu::GUARD_WORD) {
                snprintf(emu::error_text(), 160, "the guard word behind device section %d was overwritten", g);
                return NFC_ERR_INTERNAL;
            }
    return NFC_OK;
}

}  // extern "C"
