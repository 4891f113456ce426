// nfc_commands.hip -- k_multi_commands and its small companions in a translation unit of their own (multi_commands.hip.h says what
// they compute, DESIGN.md 8g why they have this form), and the C ABI of the protocol layer, all of it over the one machine of
// fsm.hip.h: the host machine (protocol.h: nfc_fsm -- nfc_fsm_create .. nfc_crc_a), its hand-over to and from the plain state, the
// sector key table, and nfc_host_commands, the kernel's twin.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstring>

#include "../../include/nfc_amd.h"
#include "launch_check.h"
#define NFC_COMMANDS_KERNELS
#include "multi_commands.hip.h"
#include "protocol.h"

static_assert(sizeof(nfc_fsm_state) == 88 && sizeof(nfc_fsm_state) % 8 == 0, "nfc_fsm_state is 88 bytes");
static_assert(sizeof(nfc_frame) == 28, "nfc_frame is seven words");
static_assert(sizeof(nfc_fsm_key_table) == 560, "nfc_fsm_key_table is 560 bytes");

namespace nfc {
namespace commands {

void launch(const Args &A, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const dim3 grid((A.R.K + THREADS - 1) / THREADS), block(THREADS);
    if (e0 || e1) NFC_LAUNCH_EXT(k_multi_commands, grid, block, 0, stream, e0, e1, 0, A);
    else NFC_LAUNCH(k_multi_commands, grid, block, 0, stream, A);
}
void launch_emu(const Args &A, const EmuArgs &E, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const dim3 grid((A.R.K + THREADS - 1) / THREADS), block(THREADS);
    if (e0 || e1) NFC_LAUNCH_EXT(k_multi_commands_emu, grid, block, 0, stream, e0, e1, 0, A, E);
    else NFC_LAUNCH(k_multi_commands_emu, grid, block, 0, stream, A, E);
}
void launch_init(uint32_t *state, uint32_t K, uint32_t k0, uint32_t k1, hipStream_t stream) {
    if (k1 <= k0) return;
    NFC_LAUNCH(k_commands_init, dim3((k1 - k0 + 255) / 256), dim3(256), 0, stream, state, K, k0, k1);
}
void launch_set_keys(uint32_t *state, uint32_t K, uint32_t k0, uint32_t k1, uint64_t key_a, uint64_t key_b, hipStream_t stream) {
    if (k1 <= k0) return;
    NFC_LAUNCH(k_commands_set_keys, dim3((k1 - k0 + 255) / 256), dim3(256), 0, stream, state, K, k0, k1, key_a, key_b);
}
void launch_io(uint32_t *state, uint32_t K, uint32_t k, int set, uint32_t *blob, hipStream_t stream) {
    NFC_LAUNCH(k_commands_io, dim3(1), dim3(64), 0, stream, state, K, k, set, blob);
}
void launch_set_table(uint32_t *tables, uint32_t K, uint32_t k0, uint32_t k1, const uint32_t *blob, hipStream_t stream) {
    if (k1 <= k0) return;
    NFC_LAUNCH(k_commands_set_table, dim3((k1 - k0 + 255) / 256, skeys::WORDS), dim3(256), 0, stream, tables, K, k0, k1, blob);
}
void launch_table_io(uint32_t *tables, uint32_t K, uint32_t k, int set, uint32_t *blob, hipStream_t stream) {
    static_assert(skeys::WORDS <= 256, "one block copies a table");
    NFC_LAUNCH(k_commands_table_io, dim3(1), dim3(256), 0, stream, tables, K, k, set, blob);
}

}  // namespace commands
}  // namespace nfc

using namespace nfc;

extern "C" {

// ---- the host machine: packets -> bytes -> commands ("next" row f1, host only: protocol.h) ----
int nfc_fsm_create(nfc_fsm **out) {
    if (!out) return NFC_ERR_ARG;
    *out = new nfc_fsm();
    return NFC_OK;
}
void nfc_fsm_destroy(nfc_fsm *f) { delete f; }
int nfc_fsm_reset(nfc_fsm *f) {   // (the table is emptied, both keys are FF..FF again)
    if (!f) return NFC_ERR_ARG;
    *f = nfc_fsm();
    return NFC_OK;
}
int nfc_fsm_process(nfc_fsm *f, const uint8_t *bits, size_t n_bits, int packet_type, nfc_frame *out, uint8_t *bytes_out, size_t bytes_cap,
                    uint16_t *enc_out) {
    if (!f || !out || !bytes_out || (n_bits && !bits) || (packet_type != 0 && packet_type != 1)) return NFC_ERR_ARG;
    if (n_bits > 0xFFFFFFFFull || bytes_cap < n_bits / 9 + 1) return NFC_ERR_ARG;
    fsm_process(*f, bits, n_bits, packet_type, out, bytes_out, enc_out);
    return NFC_OK;
}
int nfc_fsm_process_outgoing(nfc_fsm *f, const uint8_t *bits, size_t n_bits, int cmd, uint8_t *bits_out) {
    if (!f || (n_bits && (!bits || !bits_out)) || cmd < 0 || cmd >= fsmd::C_COUNT) return NFC_ERR_ARG;
    return fsm_process_outgoing(*f, bits, n_bits, cmd, bits_out);
}
int nfc_fsm_set_keys(nfc_fsm *f, const uint8_t key_a[6], const uint8_t key_b[6]) {
    if (!f || !key_a || !key_b) return NFC_ERR_ARG;
    f->key_a = fsmd::key_of(key_a);
    f->key_b = fsmd::key_of(key_b);
    return NFC_OK;
}
// (both batch forms pack their outputs: a frame's bytes and enc entries start where the longer of the previous frame's two ended)
int nfc_fsm_process_packets(nfc_fsm *f, const nfc_packet *packets, size_t n_packets, const uint8_t *bits0, const uint8_t *bits1,
                            nfc_frame *frames_out, uint8_t *bytes_out, size_t bytes_cap, size_t *bytes_used, uint16_t *enc_out) {
    if (!f || (n_packets && (!packets || !frames_out || !bytes_out))) return NFC_ERR_ARG;
    size_t used = 0;
    for (size_t i = 0; i < n_packets; i++) {
        const nfc_packet &p = packets[i];
        if (p.type != 0 && p.type != 1) return NFC_ERR_ARG;
        const uint8_t *bits = p.type ? bits1 : bits0;
        if (p.n_bits && !bits) return NFC_ERR_ARG;
        if (used + p.n_bits / 9 + 1 > bytes_cap) return NFC_ERR_ARG;
        fsm_process(*f, bits ? bits + p.bit_off : nullptr, p.n_bits, p.type, &frames_out[i], bytes_out + used, enc_out ? enc_out + used : nullptr);
        frames_out[i].byte_off = (uint32_t)used;
        used += frames_out[i].n_bytes > frames_out[i].n_enc ? frames_out[i].n_bytes : frames_out[i].n_enc;
    }
    if (bytes_used) *bytes_used = used;
    return NFC_OK;
}
int nfc_fsm_process_frames(nfc_fsm *f, const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                           const uint8_t *par1, nfc_frame *frames_out, uint8_t *bytes_out, size_t bytes_cap, size_t *bytes_used, uint16_t *enc_out) {
    if (!f || (n && (!frames || !frames_out || !bytes_out))) return NFC_ERR_ARG;
    size_t used = 0;
    for (size_t i = 0; i < n; i++) {
        const nfc_raw_frame &r = frames[i];
        if ((r.type != 0 && r.type != 1) || (r.flags & NFC_RAW_CUT)) return NFC_ERR_ARG;
        const uint8_t *b = r.type ? bytes1 : bytes0, *p = r.type ? par1 : par0;
        if (r.n_bytes && (!b || !p)) return NFC_ERR_ARG;
        // (the whole slot of n_bytes is written: a frame has no more bytes than its bits make)
        if (r.n_bytes > r.n_bits / 9 + 1 || used + r.n_bits / 9 + 1 > bytes_cap) return NFC_ERR_ARG;
        fsm_process_frame(*f, r.type, r.flags, r.n_bytes, b ? b + r.byte_off : nullptr, p ? p + r.byte_off : nullptr, &frames_out[i],
                          bytes_out + used, enc_out ? enc_out + used : nullptr);
        frames_out[i].byte_off = (uint32_t)used;
        used += frames_out[i].n_bytes > frames_out[i].n_enc ? frames_out[i].n_bytes : frames_out[i].n_enc;
    }
    if (bytes_used) *bytes_used = used;
    return NFC_OK;
}

int nfc_command_count(void) { return fsmd::C_COUNT; }
int nfc_command_get(int cmd, nfc_command_info *out) {
    static const char *const NAMES[fsmd::C_COUNT] = {"REQA",   "WUPA",   "ATQAUL", "ATQA1K", "ATQA1K", "ATQADS", "ANTI1R", "ANTI1U", "ANTI1G",
                                                     "SEL1R",  "SEL1U",  "SEL1K",  "ANTI2R", "ANTI2T", "AUTHA",  "AUTHB",  "RANDTA", "RANDRB",
                                                     "RANDTB", "SEL2R",  "SEL2T",  "READR",  "READT",  "HALT",   "WRITE",  "COMPW1", "COMPW2"};
    if (cmd < 0 || cmd >= fsmd::C_COUNT || !out) return NFC_ERR_ARG;
    const fsmd::Def c = fsmd::def_of(cmd);
    memset(out, 0, sizeof *out);
    strncpy(out->name, NAMES[cmd], sizeof out->name - 1);
    out->stage = c.stage();
    out->type = c.type();
    out->crc = c.crc();
    out->n_header = c.n_header();
    out->n_extra = c.n_extra();
    out->xor_check = c.xor_check();
    out->header[0] = (uint8_t)c.h0();
    out->header[1] = (uint8_t)c.h1;
    return NFC_OK;
}
int nfc_crc_a(const uint8_t *data, size_t n, uint8_t out[2]) {
    if ((n && !data) || !out) return NFC_ERR_ARG;
    const uint16_t c = crc_a(data, n);
    out[0] = (uint8_t)(c & 0xFF);
    out[1] = (uint8_t)(c >> 8);
    return NFC_OK;
}

// ---- the plain state, and the hand-over of a host machine to and from it ----
int nfc_fsm_state_init(nfc_fsm_state *st) {
    if (!st) return NFC_ERR_ARG;
    fsmd::Machine M;
    fsmd::machine_init(M);
    memset(st, 0, sizeof *st);
    fsmd::machine_to_state(M, *st);
    return NFC_OK;
}

int nfc_fsm_get_state(const nfc_fsm *f, nfc_fsm_state *st) {
    if (!f || !st) return NFC_ERR_ARG;
    if (f->uid.size() > fsmd::UID_CAP) return NFC_ERR_ARG;   // the plain state holds 32 UID bytes
    fsmd::Machine M = *f;   // (the Machine of it: the UID goes into its words)
    for (size_t i = 0; i < f->uid.size(); i++) fsmd::uid_put(M, (uint32_t)i, f->uid[i]);
    M.uid_len = (uint32_t)f->uid.size();
    memset(st, 0, sizeof *st);
    fsmd::machine_to_state(M, *st);
    return NFC_OK;
}

int nfc_fsm_set_state(nfc_fsm *f, const nfc_fsm_state *st) {
    if (!f || !st || fsmd::state_fault(*st)) return NFC_ERR_ARG;
    fsmd::Machine &M = *f;
    fsmd::machine_from_state(M, *st);
    f->uid.assign(st->uid, st->uid + st->uid_len);
    fsmd::uid_clear(M);   // (the holder is the vector; and the host machine keeps no flags)
    M.flags = 0;
    return NFC_OK;
}

int nfc_sector_of_block(int block) { return block < 0 || block > 255 ? -1 : (int)nfc::skeys::sector_of((uint32_t)block); }

int nfc_fsm_key_table_init(nfc_fsm_key_table *t) {
    if (!t) return NFC_ERR_ARG;
    memset(t, 0, sizeof *t);
    return NFC_OK;
}

int nfc_fsm_set_sector_key(nfc_fsm *f, int key_type, int sector, const uint8_t key[6]) {
    if (!f || (key_type != 0x60 && key_type != 0x61) || sector < 0 || sector >= (int)nfc::skeys::SECTORS) return NFC_ERR_ARG;
    const int t = key_type & 1;
    f->table.present[t][sector] = key ? 1 : 0;
    if (key) memcpy(f->table.key[t][sector], key, 6);
    else memset(f->table.key[t][sector], 0, 6);
    return NFC_OK;
}

int nfc_fsm_get_key_table(const nfc_fsm *f, nfc_fsm_key_table *t) {
    if (!f || !t) return NFC_ERR_ARG;
    *t = f->table;
    return NFC_OK;
}

int nfc_fsm_set_key_table(nfc_fsm *f, const nfc_fsm_key_table *t) {
    if (!f || !t || nfc::skeys::table_fault(*t)) return NFC_ERR_ARG;
    f->table = *t;
    return NFC_OK;
}

int nfc_host_commands(nfc_fsm_state *st, const nfc_raw_frame *merged, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                      const uint8_t *par1, nfc_frame *out, uint8_t *data, uint16_t *enc, size_t cap, size_t *used) {
    return nfc_host_commands_keyed(st, nullptr, merged, n, bytes0, par0, bytes1, par1, out, data, enc, cap, used);
}

int nfc_host_commands_keyed(nfc_fsm_state *st, const nfc_fsm_key_table *table, const nfc_raw_frame *merged, size_t n, const uint8_t *bytes0,
                            const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1, nfc_frame *out, uint8_t *data, uint16_t *enc,
                            size_t cap, size_t *used) {
    if (!st || fsmd::state_fault(*st) || (n && (!merged || !out))) return NFC_ERR_ARG;
    if (table && skeys::table_fault(*table)) return NFC_ERR_ARG;
    const skeys::HostTable keys = {table};
    fsmd::Machine M;   // (the kernel's UID holder, capped: this is its twin)
    fsmd::machine_from_state(M, *st);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const nfc_raw_frame &r = merged[i];
        if (r.type != 0 && r.type != 1) return NFC_ERR_ARG;
        const bool cut = (r.flags & NFC_RAW_CUT) != 0;
        const size_t nb = cut ? 0 : r.n_bytes;
        const uint8_t *b = r.type ? bytes1 : bytes0, *p = r.type ? par1 : par0;
        if (nb && (!b || !p || !data || !enc)) return NFC_ERR_ARG;
        if (at + nb > cap || at + nb > 0xFFFFFFFFull) return NFC_ERR_ARG;
        const fsmd::Rec rec = fsmd::process_frame(M, r.type, r.flags, (uint32_t)nb, b ? b + r.byte_off : nullptr, p ? p + r.byte_off : nullptr,
                                                  data ? data + at : nullptr, enc ? enc + at : nullptr, keys);
        nfc_frame &o = out[i];
        memset(&o, 0, sizeof o);
        o.cmd = rec.cmd;
        o.type = rec.type;
        o.byte_off = (uint32_t)at;
        o.n_bytes = (uint16_t)rec.n_bytes;
        o.n_header = (uint16_t)rec.n_header;
        o.n_extra = (uint16_t)rec.n_extra;
        o.n_crc = (uint16_t)rec.n_crc;
        o.flags = rec.flags;
        o.n_enc = (uint16_t)rec.n_enc;
        at += nb;
    }
    fsmd::machine_to_state(M, *st);
    if (used) *used = at;
    return NFC_OK;
}

}  // extern "C"
