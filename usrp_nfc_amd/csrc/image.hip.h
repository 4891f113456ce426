// image.hip.h -- a stream's commands -> the card's MEMORY IMAGE (include/nfc_amd.h: nfc_card_image), one text for host and
// device, written the way fsm.hip.h, emu.hip.h and ctx_commands.hip.h are: scalar state, NFC_HD, nothing a lane would index dynamically.
//
// The rule.  An image is 1 024 bytes `mem`, one source code per byte in `src` (0: unknown), a tag type, sticky flags and a TAIL: the
// summaries -- cmd, type, flags, first extra byte -- of the stream's last three commands.  A command is judged from its own record, its
// extra bytes, the three summaries before it and the tag type in effect (`classify`): the outcome is a PATCH of at most 16 bytes, flags
// to set, perhaps a tag type.  Patches are applied in stream order, the last one wins a byte, and a patch whose value differs from a byte
// that was already known sets NFC_IMG_CHANGED.
//   ATQA*                      the tag type; NFC_IMG_TAG_CHANGED when another one was set before
//   ANTI1U / ANTI2T / ANTI1G   bytes 0..3 / 4..8 / 0..4: what emu.hip.h's tag_step sends from `mem`
//   READT behind a READR       tag type 0: pages val .. val + 3 round the 64 bytes (val > 0x0F: nothing).  Any other tag type, none heard
//                              included: block val -- a data block whole; a trailer [6, 10) and, where the access bits IN THIS ANSWER let
//                              key B be read (emu.hip.h: access_bits_at, bits <= 2), [10, 16); never [0, 6): a card reads key A as zeros.
//                              val >= 64: nothing, NFC_IMG_BEYOND
//   RANDTB with AT_OK behind AUTHA / AUTHB, RANDTA, RANDRB with AR_OK
//                              the key the machine held for (key type, the AUTH's block) -- sector_keys.h's choose / resolve, the rule
//                              process_frame applies -- into [0, 6) / [10, 16) of the sector's trailer; sector >= 16: NFC_IMG_BEYOND
//   WRITE / COMPW1 / COMPW2    nothing, NFC_IMG_SAW_WRITE (applying writes is not built)
//   cmd < 0                    nothing; it is still "the command before"
// A READT or READR record has passed its CRC_A in the lookup (fsm.hip.h: compatible() refuses a Def with crc() whose CRC is wrong, and
// both Defs have it): nothing is checked again here.
//
// The kernel: k_multi_images, a workgroup of one wave per stream, behind k_multi_commands / k_multi_commands_emu in a tracked push.  The
// stream's image comes into LDS with one 16-byte load per lane and array, the commands are walked in tiles of 64 -- the stream's records
// are contiguous from cmd_off[k], so lane i takes command i of the tile and the loads of a tile are neighbours --, the summaries before
// a lane's command come from the lanes below it (a shuffle) or, for the first three, from the tail carried from the tile or push before.
// Within a tile the order is made exact through an OWNER TABLE in LDS: every patching lane takes atomicMax(owner[cell], lane + 1), after a
// barrier the owner of a cell -- the last command that patches it -- compares with the byte that was known and stores; after another
// barrier every other patcher compares its value with the winner's.  NFC_IMG_CHANGED is order-free: in a sequence old, p1 .. pn two
// neighbours differ iff some element differs from pn.  The image goes back with one 16-byte store per lane and array, and only when a
// command of this push patched or flagged anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nfc_amd.h"
#include "emu.hip.h"
#include "fsm.hip.h"
#include "multi_commands.hip.h"
#include "sector_keys.h"

namespace nfc {
namespace image {

using namespace fsmd;

constexpr uint32_t MEM_BYTES = NFC_IMG_BYTES, TAIL = NFC_IMG_TAIL;
static_assert(MEM_BYTES == emu::CLASSIC_BYTES && MEM_BYTES == 1024, "an image is a Classic 1K's memory");
static_assert(sizeof(nfc_image_cmd) == 16 && sizeof(nfc_image_info) == 16 && sizeof(nfc_card_image) == 2 * 1024 + 16 + 3 * 16, "the image's records are the header's");
using Sum = nfc_image_cmd;

// a summary as two words, for the shuffles: the flags are NFC_FRAME_* (eight bits), val a byte, type a bit
NFC_HD uint32_t pack(const Sum &s) { return (s.flags & 0xFFu) | (s.val & 0xFFu) << 8 | (s.type & 1u) << 16; }
NFC_HD Sum unpack(int32_t cmd, uint32_t w) {
    const Sum s = {cmd, (w >> 16) & 1u, w & 0xFFu, (w >> 8) & 0xFFu};
    return s;
}
NFC_HD Sum no_command() {   // what a tail holds where there was no command yet
    const Sum s = {NFC_CMD_UNKNOWN, 0u, 0u, 0u};
    return s;
}
// what a record leaves to the commands behind it.  x0: its first four extra bytes (extra_words)
NFC_HD Sum summary(int32_t cmd, int32_t type, uint32_t flags, uint32_t n_extra, uint32_t x0) {
    const Sum s = {cmd, (uint32_t)type & 1u, flags & 0xFFu, (cmd >= 0 && n_extra >= 1u) ? x0 & 0xFFu : 0u};
    return s;
}

// A patch: 16 values in four words, byte j of them for cell addr(j) where mask has bit j.  page < 16: an Ultralight's four pages from
// `page`, round the end; else the cells from `base` on.
struct Patch {
    uint32_t w0, w1, w2, w3;
    uint32_t mask, base, page, src;
    uint32_t set_flags;
    int32_t set_type;   // -2: none
    NFC_HD uint32_t addr(uint32_t j) const { return (page < 16u ? (((page + (j >> 2)) & 15u) << 2 | (j & 3u)) : base + j) & (MEM_BYTES - 1u); }
    NFC_HD uint32_t value(uint32_t j) const {
        const uint32_t q = j >> 2;
        const uint32_t w = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
        return (w >> (8u * (j & 3u))) & 0xFFu;
    }
};
// a READT's sixteen bytes as the card emu.hip.h's access decoding reads
struct AnswerCard {
    uint32_t w0, w1, w2, w3;
    NFC_HD uint32_t mem_word(uint32_t i) const {
        i &= 3u;
        return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3;
    }
};

// One command.  c: its summary; x0 .. x3: its first sixteen extra bytes, zeros behind those there are; n_extra: how many there are;
// p1, p2, p3: the summaries of the commands before it, p1 the nearest; tag_type: the one in effect (-1: none heard).
template <class Table>
NFC_HD Patch classify(const Sum &c, uint32_t n_extra, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, const Sum &p1, const Sum &p2, const Sum &p3,
                      int32_t tag_type, const Table &tab, uint64_t key_a, uint64_t key_b) {
    Patch P = {x0, x1, x2, x3, 0u, 0u, 16u, 0u, 0u, -2};
    switch (c.cmd) {
    case C_ATQAUL: P.set_type = 0; break;
    case C_ATQA1K: P.set_type = 1; break;
    case C_ATQA4K: P.set_type = 2; break;
    case C_ATQADS: P.set_type = 3; break;
    case C_ANTI1U:
        if (n_extra >= 4u) P.mask = 0x000Fu, P.base = 0u, P.src = NFC_IMG_SRC_ANTICOLL;
        break;
    case C_ANTI2T:
        if (n_extra >= 5u) P.mask = 0x001Fu, P.base = 4u, P.src = NFC_IMG_SRC_ANTICOLL;
        break;
    case C_ANTI1G:
        if (n_extra >= 5u) P.mask = 0x001Fu, P.base = 0u, P.src = NFC_IMG_SRC_ANTICOLL;
        break;
    case C_READT: {
        if (p1.cmd != C_READR || n_extra < 16u) break;
        const uint32_t val = p1.val;
        P.src = NFC_IMG_SRC_READ;
        if (tag_type == 0) {
            if (val <= 0x0Fu) P.mask = 0xFFFFu, P.page = val;
        } else if (val >= 64u) {
            P.set_flags |= NFC_IMG_BEYOND;
        } else if (val % 4u != 3u) {
            P.mask = 0xFFFFu, P.base = val * 16u;
        } else {
            emu::State S;
            S.flags = 0;
            const AnswerCard A = {x0, x1, x2, x3};
            const uint32_t bits = emu::access_bits_at(S, A, 6u, 3u);
            P.mask = bits <= 2u ? 0xFFC0u : 0x03C0u;
            P.base = val * 16u;
        }
        break;
    }
    case C_RANDTB: {
        if (!(c.flags & NFC_FRAME_AT_OK) || p1.cmd != C_RANDRB || !(p1.flags & NFC_FRAME_AR_OK) || p2.cmd != C_RANDTA ||
            (p3.cmd != C_AUTHA && p3.cmd != C_AUTHB))
            break;
        const uint32_t kt = p3.cmd == C_AUTHB ? 1u : 0u, sector = skeys::sector_of(p3.val);
        if (sector >= 16u) {
            P.set_flags |= NFC_IMG_BEYOND;
            break;
        }
        const uint64_t key = skeys::resolve(tab, skeys::choose(tab, kt, p3.val), key_a, key_b);
        P.w0 = (uint32_t)key, P.w1 = (uint32_t)(key >> 32) & 0xFFFFu, P.w2 = P.w3 = 0u;
        P.mask = 0x003Fu, P.base = (sector * 4u + 3u) * 16u + (kt ? 10u : 0u), P.src = NFC_IMG_SRC_KEY;
        break;
    }
    case C_WRITE: case C_COMPW1: case C_COMPW2: P.set_flags |= NFC_IMG_SAW_WRITE; break;
    default: break;
    }
    if (P.set_type >= 0 && tag_type >= 0 && tag_type != P.set_type) P.set_flags |= NFC_IMG_TAG_CHANGED;
    return P;
}
// The extra bytes of a record that may be read, for twin and kernel alike: none of a record that is no command, none where header and
// extra bytes do not fit the record's own n_bytes, none where the record's bytes [byte_off, byte_off + n_bytes) do not lie inside the
// `room` bytes its data has -- the stream's slots on the device, the caller's data_len on the host.  `outside`: that last case.  Only a
// record the machines never write gets there; the kernel then goes on with no extra bytes (it has nobody to refuse), the twin
// refuses the call with NFC_ERR_ARG.
NFC_HD uint32_t readable_extra(int32_t cmd, uint32_t n_header, uint32_t n_extra, uint32_t n_bytes, uint64_t byte_off, uint64_t room, bool &outside) {
    outside = false;
    if (cmd < 0 || n_extra == 0u || n_header + n_extra > n_bytes) return 0u;
    outside = byte_off + n_bytes > room;
    return outside ? 0u : n_extra;
}
// the commands whose extra bytes classify() reads beyond the first
NFC_HD bool reads_extra(int32_t cmd) { return cmd == C_ANTI1U || cmd == C_ANTI2T || cmd == C_ANTI1G || cmd == C_READT; }

// what is wrong with a caller's image, or null
inline const char *image_fault(const nfc_card_image &g) {
    if (g.info.tag_type < -1 || g.info.tag_type > 3) return "tag_type out of range";
    if (g.info.flags & ~(uint32_t)NFC_IMG_FLAGS_ALL) return "unknown flags";
    if (g.info.reserved != 0) return "reserved must be 0";
    uint32_t known = 0;
    for (uint32_t i = 0; i < MEM_BYTES; i++) {
        if (g.src[i] > NFC_IMG_SRC_KEY) return "src holds an unknown source code";
        known += g.src[i] != 0;
    }
    if (known != g.info.n_known) return "n_known is not the number of known bytes";
    for (uint32_t j = 0; j < TAIL; j++) {
        const Sum &s = g.tail[j];
        if (s.cmd < NFC_CMD_CUT || s.cmd >= C_COUNT || s.type > 1u || s.flags > 0xFFu || s.val > 0xFFu) return "tail entry out of range";
    }
    return nullptr;
}
inline void image_init(nfc_card_image &g) {
    memset(&g, 0, sizeof g);
    g.info.tag_type = -1;
    for (uint32_t j = 0; j < TAIL; j++) g.tail[j] = no_command();
}

// ---- the CPU twin: one image over n records and their data, in place ----
// data_len: the bytes `data` holds; a record whose slot lies outside them is the caller's mistake (false: nothing of it was applied)
template <class Table>
inline bool host_run(nfc_card_image &g, const nfc_frame *cmds, size_t n, const uint8_t *data, size_t data_len, const Table &tab, uint64_t key_a,
                     uint64_t key_b) {
    for (size_t i = 0; i < n; i++) {
        const nfc_frame &r = cmds[i];
        uint32_t x[4] = {0, 0, 0, 0};
        bool outside;
        const uint32_t ne = readable_extra(r.cmd, r.n_header, r.n_extra, r.n_bytes, r.byte_off, data ? data_len : 0u, outside), take = ne < 16u ? ne : 16u;
        if (outside) return false;
        if (take) {
            for (uint32_t j = 0; j < take; j++) x[j >> 2] |= (uint32_t)data[(size_t)r.byte_off + r.n_header + j] << (8u * (j & 3u));
        }
        const Sum c = summary(r.cmd, r.type, r.flags, ne, x[0]);
        const Patch P = classify(c, ne, x[0], x[1], x[2], x[3], g.tail[0], g.tail[1], g.tail[2], g.info.tag_type, tab, key_a, key_b);
        for (uint32_t j = 0; j < 16u; j++) {
            if (!((P.mask >> j) & 1u)) continue;
            const uint32_t a = P.addr(j), v = P.value(j);
            if (g.src[a] && g.mem[a] != v) g.info.flags |= NFC_IMG_CHANGED;
            g.info.n_known += g.src[a] == 0;
            g.mem[a] = (uint8_t)v;
            g.src[a] = (uint8_t)P.src;
        }
        g.info.flags |= P.set_flags;
        if (P.set_type >= 0) g.info.tag_type = P.set_type;
        g.tail[2] = g.tail[1], g.tail[1] = g.tail[0], g.tail[0] = c;
    }
    return true;
}

// ---- the device ----
// The images' buffer, persistent from push to push: mem [K][1024] | src [K][1024] | info [K] | tail [K][3], each section on 16 bytes and
// followed by the guard word (nfc_multi.hip lays it out and fills the guards once, with the initial images: k_images_init).
enum { ISEC_MEM, ISEC_SRC, ISEC_INFO, ISEC_TAIL, ISEC_COUNT };
struct Args {
    uint8_t *img;                 // the images' buffer
    uint64_t at[ISEC_COUNT];
    uint32_t K;
    const uint8_t *cmds;          // the tracked push's buffer (multi_commands.hip.h: Layout)
    commands::Layout L;
    const uint32_t *state;        // [fsmd::W_WORDS][K]: the machines, for their key A / key B
    const uint32_t *sector_keys;  // [skeys::SLOTS][2][K], or null
};
constexpr int THREADS = 64;

#ifdef NFC_IMAGE_KERNELS
// streams [k0, k1) to image_init's image; with guard_bytes != 0 block 0 also writes the guard word behind the four sections
struct InitArgs {
    uint8_t *img;
    uint64_t at[ISEC_COUNT], end[ISEC_COUNT];
    uint32_t K, k0, k1, guard_bytes, guard_word;
};
__global__ __launch_bounds__(256) void k_images_init(InitArgs I) {
    uint8_t *img = I.img;
    if (blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < (uint32_t)ISEC_COUNT * I.guard_bytes; i += 256u) {
            const uint32_t s = i / I.guard_bytes, b = i % I.guard_bytes;
            img[I.end[s] + b] = (uint8_t)(I.guard_word >> (8u * (b & 3u)));
        }
    // a thread per 16 bytes of a stream's mem and src; the first four of a stream also write its info and tail
    const uint32_t per = MEM_BYTES / 16u;
    const uint64_t n = (uint64_t)(I.k1 > I.k0 ? I.k1 - I.k0 : 0u) * per;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t k = I.k0 + (uint32_t)(i / per), u = (uint32_t)(i % per);
        if (k >= I.K) continue;
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        ((uint4 *)(img + I.at[ISEC_MEM]))[(size_t)k * per + u] = z;
        ((uint4 *)(img + I.at[ISEC_SRC]))[(size_t)k * per + u] = z;
        if (u == 0) ((uint4 *)(img + I.at[ISEC_INFO]))[k] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
        else if (u <= TAIL) ((uint4 *)(img + I.at[ISEC_TAIL]))[(size_t)k * TAIL + (u - 1u)] = make_uint4((uint32_t)NFC_CMD_UNKNOWN, 0u, 0u, 0u);
    }
}

// the summary j (1 .. 3) places before position p of a tile: a lane's below it, or the carried tail's
__device__ __forceinline__ Sum before(uint32_t p, uint32_t j, int32_t my_cmd, uint32_t my_w, const Sum &t1, const Sum &t2, const Sum &t3) {
    const int src = (int)p - (int)j;
    const int32_t cmd = __shfl(my_cmd, src < 0 ? 0 : src, THREADS);
    const uint32_t w = __shfl(my_w, src < 0 ? 0 : src, THREADS);
    if (src >= 0) return unpack(cmd, w);
    const uint32_t back = j - p;   // 1 .. 3
    return back == 1u ? t1 : back == 2u ? t2 : t3;
}

__global__ __launch_bounds__(THREADS) void k_multi_images(Args A) {
    __shared__ uint4 s_mem4[MEM_BYTES / 16], s_src4[MEM_BYTES / 16];
    __shared__ uint32_t s_owner[MEM_BYTES];
    __shared__ uint32_t s_flags;
    uint8_t *const s_mem = (uint8_t *)s_mem4, *const s_src = (uint8_t *)s_src4;
    const uint32_t K = A.K, k = blockIdx.x, lane = threadIdx.x;
    if (k >= K) return;
    const commands::Layout &L = A.L;
    // the stream's commands and byte slots, cut to what the host laid out
    const uint64_t *cmd_off = (const uint64_t *)(A.cmds + L.at[commands::SEC_CMD_OFF]), *cbyte_off = (const uint64_t *)(A.cmds + L.at[commands::SEC_CBYTE_OFF]);
    uint64_t c1 = cmd_off[k + 1], c0 = cmd_off[k], b1 = cbyte_off[k + 1], b0 = cbyte_off[k];
    c1 = c1 < L.total_cmds ? c1 : L.total_cmds;
    c0 = c0 < c1 ? c0 : c1;
    b1 = b1 < L.total_bytes ? b1 : L.total_bytes;
    b0 = b0 < b1 ? b0 : b1;
    const uint64_t n_cmds = c1 - c0, room = b1 - b0;
    if (n_cmds == 0) return;
    const uint32_t *__restrict__ rec = (const uint32_t *)(A.cmds + L.at[commands::SEC_CMD]);
    const uint8_t *__restrict__ data = A.cmds + L.at[commands::SEC_DATA] + b0;

    uint4 *g_mem = (uint4 *)(A.img + A.at[ISEC_MEM]) + (size_t)k * (MEM_BYTES / 16), *g_src = (uint4 *)(A.img + A.at[ISEC_SRC]) + (size_t)k * (MEM_BYTES / 16);
    uint4 *g_info = (uint4 *)(A.img + A.at[ISEC_INFO]) + k, *g_tail = (uint4 *)(A.img + A.at[ISEC_TAIL]) + (size_t)k * TAIL;
    s_mem4[lane] = g_mem[lane];
    s_src4[lane] = g_src[lane];
    for (uint32_t i = lane; i < MEM_BYTES; i += THREADS) s_owner[i] = 0u;
    if (lane == 0) s_flags = 0u;
    const uint4 info = *g_info;
    int32_t tag_type = (int32_t)info.x;   // the one in effect before the tile
    if (tag_type < -1 || tag_type > 3) tag_type = -1;
    Sum t1, t2, t3;
    {
        const uint4 a = g_tail[0], b = g_tail[1], c = g_tail[2];
        t1 = unpack((int32_t)a.x, (a.z & 0xFFu) | (a.w & 0xFFu) << 8 | (a.y & 1u) << 16);
        t2 = unpack((int32_t)b.x, (b.z & 0xFFu) | (b.w & 0xFFu) << 8 | (b.y & 1u) << 16);
        t3 = unpack((int32_t)c.x, (c.z & 0xFFu) | (c.w & 0xFFu) << 8 | (c.y & 1u) << 16);
    }
    const uint64_t key_a = (uint64_t)A.state[(size_t)W_KA_LO * K + k] | (uint64_t)(A.state[(size_t)W_KA_HI * K + k] & 0xFFFFu) << 32;
    const uint64_t key_b = (uint64_t)A.state[(size_t)W_KB_LO * K + k] | (uint64_t)(A.state[(size_t)W_KB_HI * K + k] & 0xFFFFu) << 32;
    const skeys::DeviceTable tab = {A.sector_keys, K, k};
    uint32_t my_flags = 0u;
    bool touched = false;   // (wave-uniform)
    __syncthreads();

    for (uint64_t base = 0; base < n_cmds; base += THREADS) {
        const uint32_t cnt = (uint32_t)(n_cmds - base < (uint64_t)THREADS ? n_cmds - base : (uint64_t)THREADS);
        const bool mine = lane < cnt;
        // the lane's record: seven words, neighbours' records behind one another
        int32_t cmd = NFC_CMD_UNKNOWN;
        uint32_t type = 0, byte_off = 0, n_bytes = 0, n_header = 0, n_extra = 0, flags = 0;
        if (mine) {
            const uint32_t *w = rec + (c0 + base + lane) * (sizeof(nfc_frame) / 4);
            cmd = (int32_t)w[0], type = w[1], byte_off = w[2];
            n_bytes = w[3] & 0xFFFFu, n_header = w[3] >> 16, n_extra = w[4] & 0xFFFFu, flags = w[5];
        }
        bool outside;   // (its extra bytes, inside the record's own bytes and the stream's slots)
        n_extra = readable_extra(cmd, n_header, n_extra, n_bytes, byte_off, room, outside);
        uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
        {
            const uint32_t take = n_extra == 0 ? 0u : reads_extra(cmd) ? (n_extra < 16u ? n_extra : 16u) : 1u;
            const uint8_t *d = data + byte_off + n_header;
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++) {
                const uint32_t b = j < take ? (uint32_t)d[j] << (8u * (j & 3u)) : 0u;
                if (j < 4u) x0 |= b;
                else if (j < 8u) x1 |= b;
                else if (j < 12u) x2 |= b;
                else x3 |= b;
            }
        }
        const Sum c = summary(cmd, (int32_t)type, flags, n_extra, x0);
        const uint32_t cw = pack(c);
        const Sum p1 = before(lane, 1u, c.cmd, cw, t1, t2, t3), p2 = before(lane, 2u, c.cmd, cw, t1, t2, t3), p3 = before(lane, 3u, c.cmd, cw, t1, t2, t3);
        // the tag type in effect: the nearest ATQA below the lane in this tile, else the one carried
        const bool atqa = mine && cmd >= C_ATQAUL && cmd <= C_ATQADS;
        const uint64_t atqas = __ballot(atqa);
        const int32_t atqa_type = cmd - C_ATQAUL;
        const uint64_t below = atqas & ((1ull << lane) - 1ull);
        const int near = below ? 63 - __builtin_clzll(below) : 0;
        const int32_t near_type = __shfl(atqa_type, near, THREADS);
        const int32_t in_effect = below ? near_type : tag_type;
        Patch P = classify(c, n_extra, x0, x1, x2, x3, p1, p2, p3, in_effect, tab, key_a, key_b);
        if (!mine) P.mask = 0u, P.set_flags = 0u, P.set_type = -2;
        my_flags |= P.set_flags;
        const bool any = __ballot(P.mask != 0u) != 0ull;
        touched = touched || any || __ballot(P.set_flags != 0u || P.set_type >= 0) != 0ull;
        if (any) {   // (wave-uniform: every lane meets the barriers)
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++)
                if ((P.mask >> j) & 1u) atomicMax(&s_owner[P.addr(j)], lane + 1u);
            __syncthreads();
            uint32_t own = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++)
                if ((P.mask >> j) & 1u) {
                    const uint32_t a = P.addr(j), v = P.value(j);
                    if (s_owner[a] == lane + 1u) {
                        own |= 1u << j;
                        if (s_src[a] != 0 && s_mem[a] != v) my_flags |= NFC_IMG_CHANGED;
                        s_mem[a] = (uint8_t)v;
                        s_src[a] = (uint8_t)P.src;
                    }
                }
            __syncthreads();
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++)
                if ((P.mask >> j) & 1u) {
                    const uint32_t a = P.addr(j);
                    if (!((own >> j) & 1u) && s_mem[a] != P.value(j)) my_flags |= NFC_IMG_CHANGED;
                }
            __syncthreads();
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++)
                if ((P.mask >> j) & 1u) s_owner[P.addr(j)] = 0u;
            __syncthreads();
        }
        // what the next tile, or the next push, finds before its first commands
        if (atqas) tag_type = __shfl(atqa_type, 63 - __builtin_clzll(atqas), THREADS);
        const Sum n1 = before(cnt, 1u, c.cmd, cw, t1, t2, t3), n2 = before(cnt, 2u, c.cmd, cw, t1, t2, t3), n3 = before(cnt, 3u, c.cmd, cw, t1, t2, t3);
        t1 = n1, t2 = n2, t3 = n3;
    }

    if (my_flags) atomicOr(&s_flags, my_flags);
    __syncthreads();
    if (lane < TAIL) {
        const Sum &t = lane == 0 ? t1 : lane == 1 ? t2 : t3;
        g_tail[lane] = make_uint4((uint32_t)t.cmd, t.type, t.flags, t.val);
    }
    if (!touched) return;
    const uint4 m4 = s_mem4[lane], s4 = s_src4[lane];
    g_mem[lane] = m4;
    g_src[lane] = s4;
    // the known bytes: sixteen source codes per lane, summed over the wave
    uint32_t known = 0;
    {
        const uint32_t w[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int b = 0; b < 4; b++) known += ((w[q] >> (8 * b)) & 0xFFu) != 0u;
    }
#pragma unroll
    for (int off = THREADS / 2; off > 0; off >>= 1) known += __shfl_xor(known, off, THREADS);
    if (lane == 0) *g_info = make_uint4((uint32_t)tag_type, info.y | s_flags, known, 0u);
}
#endif   // NFC_IMAGE_KERNELS

}  // namespace image
}  // namespace nfc
