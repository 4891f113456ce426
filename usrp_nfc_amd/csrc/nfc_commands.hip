// nfc_commands.hip -- k_multi_commands and its small companions in a translation unit of their own (multi_commands.hip.h says what
// they compute, DESIGN.md 8g why they have this form), and the host side of the restated machine (fsm.hip.h): nfc_host_commands, the
// kernel's twin, and the hand-over of a host machine (protocol.h: nfc_fsm) to and from the plain state.
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
static_assert((int)nfc::fsmd::C_COUNT == (int)nfc::CMD_COUNT && (int)nfc::fsmd::C_COMPW2 == (int)nfc::CMD_COMPW2, "one command order");

namespace nfc {
namespace commands {

void launch(const Args &A, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const dim3 grid((A.R.K + THREADS - 1) / THREADS), block(THREADS);
    if (e0 || e1) NFC_LAUNCH_EXT(k_multi_commands, grid, block, 0, stream, e0, e1, 0, A);
    else NFC_LAUNCH(k_multi_commands, grid, block, 0, stream, A);
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

namespace {
// the restated command table against protocol.h's, field by field, and the stage tables entry by entry
bool tables_agree() {
    using namespace nfc;
    for (int c = 0; c < CMD_COUNT; c++) {
        const CommandDef &h = COMMANDS[c];
        const fsmd::Def d = fsmd::def_of(c);
        if (d.stage() != h.stage || d.n_header() != h.n_header || d.type() != h.type || d.crc() != h.crc || d.n_extra() != h.n_extra ||
            d.xor_check() != h.xor_check || d.total() != h.total() || h.total() > fsmd::MAX_COMMAND_BYTES)
            return false;
        if ((h.n_header >= 1 && d.h0() != h.header[0]) || (h.n_header >= 2 && d.h1 != h.header[1])) return false;
    }
    for (int v = 0; v < 12; v++) {
        const uint32_t tw = fsmd::tag_stage(v), rw = fsmd::reader_stage(v);
        for (int k = 0; k < 4; k++) {
            const int want_t = v < 6 ? TAG_STAGE[v][k] : -1, want_r = (v < 8 && k < 3) ? READER_STAGE[v][k] : -1;
            const int got_t = (int)((tw >> (8 * k)) & 0xFFu), got_r = (int)((rw >> (8 * k)) & 0xFFu);
            if ((got_t == 0xFF ? -1 : got_t) != want_t || (got_r == 0xFF ? -1 : got_r) != want_r) return false;
        }
    }
    return true;
}
}  // namespace

extern "C" {

int nfc_fsm_state_init(nfc_fsm_state *st) {
    if (!st) return NFC_ERR_ARG;
    nfc::fsmd::Machine M;
    nfc::fsmd::machine_init(M);
    memset(st, 0, sizeof *st);
    nfc::fsmd::machine_to_state(M, *st);
    return NFC_OK;
}

int nfc_fsm_get_state(const nfc_fsm *f, nfc_fsm_state *st) {
    if (!f || !st) return NFC_ERR_ARG;
    if (f->uid.size() > nfc::fsmd::UID_CAP) return NFC_ERR_ARG;
    memset(st, 0, sizeof *st);
    st->cur_cmd = f->cur_cmd;
    st->tag_type = f->tag_type;
    st->encrypted = f->encrypted;
    st->cur_key = f->cur_key;
    st->cipher = f->cipher.st;
    memcpy(st->ar, f->cipher.ar, 4);
    memcpy(st->at, f->cipher.at, 4);
    memcpy(st->key_a, f->key_a, 6);
    memcpy(st->key_b, f->key_b, 6);
    st->uid_len = (uint32_t)f->uid.size();
    if (!f->uid.empty()) memcpy(st->uid, f->uid.data(), f->uid.size());
    return NFC_OK;
}

int nfc_fsm_set_state(nfc_fsm *f, const nfc_fsm_state *st) {
    if (!f || !st || nfc::fsmd::state_fault(*st)) return NFC_ERR_ARG;
    f->cur_cmd = st->cur_cmd;
    f->tag_type = st->tag_type;
    f->encrypted = st->encrypted;
    f->cipher.st = st->cipher;
    memcpy(f->cipher.ar, st->ar, 4);
    memcpy(f->cipher.at, st->at, 4);
    memcpy(f->key_a, st->key_a, 6);
    memcpy(f->key_b, st->key_b, 6);
    f->cur_key = st->cur_key;
    f->uid.assign(st->uid, st->uid + st->uid_len);
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
    using namespace nfc;
    static const bool agree = tables_agree();
    if (!agree) return NFC_ERR_INTERNAL;
    if (!st || fsmd::state_fault(*st) || (n && (!merged || !out))) return NFC_ERR_ARG;
    if (table && skeys::table_fault(*table)) return NFC_ERR_ARG;
    const skeys::HostTable keys = {table};
    fsmd::Machine M;
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
