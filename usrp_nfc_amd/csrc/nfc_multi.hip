// nfc_multi.hip -- the multi-stream context (nfc_multi, include/nfc_amd.h) in a translation unit of its own: K independent streams
// with one parameter set, decoded a lane per stream by k_multi<KIND> (multi.hip.h), and the C-ABI around it.  The non-template
// kernels of threshold.hip.h / edges.hip.h are nfc_amd.hip's: here they are `static` (NFC_HDR_KERNEL_LINKAGE) and never launched.
//
// A push: the streams' (first_sample, n) and the lane order go up in one copy, ONE launch walks every stream, one copy brings
// all counts and flags back to pinned memory, one wait.  Everything else stays in the per-stream slabs until it is read -- stream by
// stream from the slabs, or packed on the device and brought over in one copy: the decoder's arrays by nfc_multi_fetch
// (multi_fetch.hip.h), the frames by nfc_multi_fetch_frames (frames.hip.h), and with command tracking on the frames and the commands of
// every push (multi_commands.hip.h: three launches behind the push's own, nfc_multi_fetch_commands copies).
//
// Who owns what: the stream, the events and every block of device or pinned memory are members of nfc_multi of dev_buf.h's owning types --
// the blocks allocated once by nfc_multi_create in one vector (dev), the ones that grow by name -- so `delete m` releases the context,
// nfc_multi_destroy only waits for the stream first, and a create that fails half way leaves nothing behind.
//
// The host side below, in the file's order: the context; its growable buffers (dev_buf.h; grow) and the layout of the three packed
// ones (Sections: one rule, and the guard offsets the test build checks); the readers; the fetch; the frames; command tracking; the C-ABI.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define NFC_HDR_KERNEL_LINKAGE static
#include "../../include/nfc_amd.h"
#include "launch_check.h"
#include "dev_buf.h"
#include "decoder_tables.h"
#include "multi.hip.h"
#include "multi_fetch.hip.h"
#include "frames.hip.h"   // (the frame assembly kernels: nfc_frames.hip)
#include "multi_commands.hip.h"   // (the protocol machine a lane per stream: nfc_commands.hip)
#include "input_kind.h"
#define NFC_ANSWERS_TX_KERNELS
#include "answers_tx.hip.h"   // (the answers as TX samples: the schedule and render kernels; their twin is nfc_answers_tx.hip)
#define NFC_IMAGE_KERNELS
#include "image.hip.h"   // (the memory images: k_multi_images; its twin is nfc_image.hip)

using namespace nfc;
using namespace nfc::multi;

static_assert(sizeof(nfc_multi_config) == 64, "nfc_multi_config is 64 bytes");
static_assert(F_EDGES == NFC_MULTI_TRUNC_EDGES && F_SYMBOLS == NFC_MULTI_TRUNC_SYMBOLS && F_PACKETS == NFC_MULTI_TRUNC_PACKETS &&
                  F_BITS == NFC_MULTI_TRUNC_BITS && F_PENDING == NFC_MULTI_PENDING_OVERFLOW,
              "the kernel's flag bits are the header's");
static_assert(MF_EDGES == NFC_MULTI_FETCH_EDGES && MF_SYMBOLS == NFC_MULTI_FETCH_SYMBOLS && MF_PACKETS == NFC_MULTI_FETCH_PACKETS &&
                  MF_ARRAYS == NFC_MF_ARRAYS && sizeof(nfc_packet) == 24 && sizeof(nfc_multi_stats) == 64,
              "the fetch kernels' arrays and records are the header's");
static_assert(sizeof(nfc_multi_frames) == 144 && sizeof(nfc_multi_commands) == 264 && sizeof(nfc_frame) == 28, "the commands' structures are the header's");

namespace {
// a packed buffer: on the device, its pinned twin, and where the launches that last filled the device's left GUARD_BYTES of the guard
// word -- behind every section (Sections); empty: nowhere yet, or the buffer was replaced since
struct Packed {
    DevBuf d;
    PinBuf h;
    std::vector<uint64_t> guards;
};
}  // namespace

struct nfc_multi {
    nfc_params P;
    uint32_t K = 0, max_push = 0;
    int L = 0, mx = 0, nd = 0;
    float scale = 0.f;
    size_t bps = 0;   // input bytes per sample
    Caps C;
    Args A;           // everything of the launch that does not change from push to push
    Stream st;   // (before every buffer and event: members go in reverse order, the stream last)
    Event ev[2];
    int timing = 0;
    // allocated once, by nfc_multi_create
    std::vector<DevBuf> dev;   // every device block (alloc_plain, alloc_slab): the launch arguments and d_up, d_blob point into them
    PinBuf h_up;               // pinned: first_sample (u64) | n (u32) | order (u32), K each
    uint8_t *d_up = nullptr;
    PinBuf h_counts;           // pinned mirror of the counts
    uint8_t *d_blob = nullptr;   // one stream's state (k_multi_state_io) ...
    PinBuf h_blob;               // ... and its pinned twin
    size_t blob_bytes = 0;
    std::vector<std::pair<void *, size_t>> guards;   // (slab, row stride in bytes) -- rows end in GUARD_BYTES of the guard word
    std::vector<size_t> guard_row;                   // payload bytes per row
    // the streams
    std::vector<uint64_t> nseen, g0;   // samples consumed so far / before the last push, per stream
    std::vector<uint32_t> last_n;
    uint8_t canon[16];
    bool have_outputs = false;
    // grown when a call needs more (grow), released with the context
    PinBuf h_stage;   // nfc_multi_push: the host arrays packed ...
    DevBuf d_stage;   // ... and their place on the device
    PinBuf h_read;    // staging of the per-stream readers
    // the fetch (multi_fetch.hip.h): the packed buffer, the prefix tables, what the host copy holds
    Packed fetch;
    DevBuf d_ftable;   // [MF_ARRAYS][K + 1]
    PinBuf h_ftable;   // the same, followed by base[K]
    uint32_t fetched = 0;     // NFC_MULTI_FETCH_* bits the host copy serves; 0: none (a push, a reset)
    nfc_multi_fetched fout;
    // the frames (frames.hip.h, nfc_multi_fetch_frames): a packed buffer of their own -- a fetch and a frame fetch do not end each
    // other's pointers; the pinned one is followed by base[K]
    Packed frames;
    // command tracking (multi_commands.hip.h): the machines' words on the device and one machine's blob, allocated when tracking is
    // first asked for; the buffer every tracked push fills -- the frames' part, then the commands' sections -- and its pinned twin,
    // followed by base[K]
    enum CmdState { CMD_NONE, CMD_EMPTY, CMD_LAUNCHED };   // of the last push: not tracked (or reset since) / nothing stored / three launches
    bool track = false;
    DevBuf d_fsm, d_fsm_blob;
    PinBuf h_fsm_blob;
    // the sector key tables (sector_keys.h), [skeys::SLOTS][2][K] words, and one table's blob: there from the first
    // nfc_multi_set_sector_keys on, never before -- a null d_keys is "every table empty" to the kernel and to the calls
    DevBuf d_keys, d_keys_blob;
    PinBuf h_keys_blob;
    // emulation (multi_commands.hip.h: EmuArgs): the cards and the emulators' state, there from the first nfc_multi_emulate on, never
    // before; has_card mirrors params' PRESENT word, n_cards counts it: while it is 0 a tracked push launches k_multi_commands as ever
    DevBuf d_emu;
    size_t emu_mem = 0, emu_rands = 0, emu_params = 0, emu_state = 0;   // offsets into d_emu
    std::vector<uint8_t> has_card;
    uint32_t n_cards = 0;
    bool cmd_emulated = false;   // the last launched push ran the emulating form: its buffer holds the answers' sections
    commands::EmuArgs cmd_emu;
    nfc_multi_answers aout;
    // transmission (answers_tx.hip.h), there from the first nfc_multi_transmit_device / nfc_multi_set_tx_state on, never before: the
    // pending entries [K], one section with its guard; the buffer of one call -- the streams' records, the tile table, the span table, the
    // span counts -- and the pinned staging of the two the host makes.  card_role: -1 none, else the card's role (ensure_emu sizes it)
    std::vector<int8_t> card_role;
    Packed txpend, tx;
    PinBuf h_tx;
    Event evt[4];
    bool tx_done = false;   // the last push was transmitted
    Packed cmd;
    size_t cmd_bytes = 0;
    CmdState cmd_state = CMD_NONE;
    bool cmd_fetched = false, cmd_timed = false;
    frames::MultiLayout cmd_frlay;   // of the last push that stored anything, as cmd_lay, cmd_nfr and cmd_room
    commands::Layout cmd_lay;
    uint64_t cmd_nfr[2] = {0, 0}, cmd_room[2] = {0, 0};
    Event evc[4];
    nfc_multi_commands cout;
    // the memory images (image.hip.h), there from the first nfc_multi_track_images on, never before: the buffer of four sections with
    // their guards, persistent from push to push; its pinned twin, filled by nfc_multi_fetch_images; one image's staging
    bool track_img = false;
    Packed img;
    uint64_t img_at[image::ISEC_COUNT] = {0, 0, 0, 0};
    size_t img_bytes = 0;
    PinBuf h_img_one;
    bool img_fetched = false, img_timed = false;
    uint32_t img_launches = 0;   // of the last push
    Event evi[2];
    nfc_multi_images iout;
    nfc_multi_stats stats;
    std::string err;
    LaunchError launch_err;
};

namespace {
std::string g_multi_create_error;

int mfail(nfc_multi *m, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (m) m->err = buf;
    else g_multi_create_error = buf;
    return code;
}

#define MCHK(m, call)                                                                                                       \
    do {                                                                                                                    \
        hipError_t e__ = (call);                                                                                            \
        if (e__ != hipSuccess) return mfail((m), NFC_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

using MultiKernel = void (*)(Args);
MultiKernel kernel_of(int kind) {
    return with_kind(kind, [](auto K) -> MultiKernel { return k_multi<decltype(K)::value>; });
}

int launch_ok(nfc_multi *m) {
    LaunchError &le = launch_error();
    if (le.err == hipSuccess) return NFC_OK;
    const LaunchError e = le;
    le = LaunchError{};
    return mfail(m, NFC_ERR_DEVICE, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e.err), e.file, e.line);
}

// a block the context keeps for good (m->dev); null: the device has none of that size
void *alloc_once(nfc_multi *m, size_t bytes) {
    DevBuf b;
    if (b.ensure(bytes) != hipSuccess) return (void)hipGetLastError(), nullptr;
    m->dev.push_back(std::move(b));
    return m->dev.back().p;
}
// a slab of K rows, each `row` payload bytes and GUARD_BYTES of the guard word behind them
template <class T>
int alloc_slab(nfc_multi *m, T **out, size_t row_bytes) {
    const size_t stride = row_bytes + GUARD_BYTES, total = stride * m->K;
    if (!(*out = (T *)alloc_once(m, total)))
        return mfail(nullptr, NFC_ERR_NOMEM, "nfc_multi_create: no device memory for a slab of %zu bytes (n_streams %u)", total, m->K);
    m->guards.emplace_back(*out, stride);
    m->guard_row.push_back(row_bytes);
    return NFC_OK;
}
template <class T>
int alloc_plain(nfc_multi *m, T **out, size_t bytes) {
    if (!(*out = (T *)alloc_once(m, std::max<size_t>(bytes, 16))))
        return mfail(nullptr, NFC_ERR_NOMEM, "nfc_multi_create: no device memory for %zu bytes (n_streams %u)", bytes, m->K);
    return NFC_OK;
}

__global__ __launch_bounds__(256) void k_multi_guard_fill(uint8_t *slab, size_t stride, size_t row, uint32_t K) {
    const size_t words = (size_t)K * (GUARD_BYTES / 4), step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += step) {
        const size_t k = i / (GUARD_BYTES / 4), w = i % (GUARD_BYTES / 4);
        uint8_t *g = slab + k * stride + row + w * 4;
        for (int b = 0; b < 4; b++) g[b] = (uint8_t)(GUARD_WORD >> (8 * b));   // (a row's end is only as aligned as its entries)
    }
}
__global__ __launch_bounds__(256) void k_multi_guard_check(const uint8_t *slab, size_t stride, size_t row, uint32_t K, uint32_t *bad) {
    const size_t words = (size_t)K * (GUARD_BYTES / 4), step = (size_t)gridDim.x * 256;
    uint32_t mine = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += step) {
        const size_t k = i / (GUARD_BYTES / 4), w = i % (GUARD_BYTES / 4);
        const uint8_t *g = slab + k * stride + row + w * 4;
        for (int b = 0; b < 4; b++) mine += g[b] != (uint8_t)(GUARD_WORD >> (8 * b));
    }
    if (mine) atomicAdd(bad, mine);
}

size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// A buffer for `bytes` of the call `fn`: as it is when it holds them, otherwise released and allocated anew with half as much again (or,
// for what never changes its size, exactly).  Returns 0: as it was; 1: another buffer -- nothing of the old one's contents is there;
// NFC_ERR_NOMEM: the too-small buffer is gone and the context is otherwise as it was.
const char *memory_of(const DevBuf &) { return "device"; }
const char *memory_of(const PinBuf &) { return "pinned host"; }
template <class Buf>
int grow(nfc_multi *m, Buf &b, size_t bytes, const char *fn, bool headroom = true) {
    if (b.cap >= bytes) return 0;
    b.release();
    const size_t cap = headroom ? bytes + bytes / 2 + 4096 : bytes;
    if (b.ensure(cap) == hipSuccess) return 1;
    (void)hipGetLastError();
    return mfail(m, NFC_ERR_NOMEM, "%s: no %s memory for %zu bytes", fn, memory_of(b), cap);
}
// ... of a packed buffer's device side, for the launches that fill it: another buffer holds no guards
int grow_packed(nfc_multi *m, Packed &p, size_t bytes, const char *fn) {
    const int g = grow(m, p.d, bytes, fn);
    if (g) p.guards.clear();
    return g < 0 ? g : NFC_OK;
}

// The sections of a packed buffer, one after the other: each starts on 16 bytes and has GUARD_BYTES of the guard word behind its end.
// `at` is where the next one starts -- in the end the bytes used -- and `guards` every end so far.
struct Sections {
    size_t at;
    std::vector<uint64_t> guards;
    void place(uint64_t &sec_at, uint64_t &sec_end, size_t bytes) {
        sec_at = at;
        sec_end = at + bytes;
        guards.push_back(sec_end);
        at = up16(sec_end + GUARD_BYTES);
    }
};

// [k0, k1) of the calls that take one stream or, with -1, all of them
int stream_range(nfc_multi *m, int64_t stream, uint32_t &k0, uint32_t &k1) {
    if (stream < -1 || stream >= (int64_t)m->K) return mfail(m, NFC_ERR_ARG, "stream %lld out of range (n_streams %u)", (long long)stream, m->K);
    k0 = stream < 0 ? 0u : (uint32_t)stream;
    k1 = stream < 0 ? m->K : (uint32_t)stream + 1u;
    return NFC_OK;
}

// the records a packing kernel left with idx batch-local, `off` [K + 1] their offset table: the stream's base is added here, over the few
// records there are
template <class Rec>
void add_base(Rec *rec, const uint64_t *off, const uint64_t *base, uint32_t K) {
    for (uint32_t k = 0; k < K; k++)
        if (base[k])
            for (uint64_t i = off[k]; i < off[k + 1]; i++) rec[i].idx += base[k];
}

// [first, first + n) of a stream's row, n cut to what the slab stores and the caller's room
int read_row(nfc_multi *m, const char *fn, const void *slab, size_t stride_entries, size_t esz, uint32_t stream, size_t stored, size_t first, void *out,
             size_t cap, size_t *n_out) {
    size_t n = 0;
    if (first < stored) n = std::min(cap, stored - first);
    if (n && !out) return mfail(m, NFC_ERR_ARG, "null output");
    if (n) {
        if (grow(m, m->h_read, n * esz, fn) < 0) return NFC_ERR_NOMEM;
        m->stats.n_reads_device++;
        MCHK(m, hipMemcpyAsync(m->h_read.p, (const char *)slab + ((size_t)stream * stride_entries + first) * esz, n * esz, hipMemcpyDeviceToHost, m->st));
        MCHK(m, hipStreamSynchronize(m->st));
        memcpy(out, m->h_read.p, n * esz);
    }
    if (n_out) *n_out = n;
    return NFC_OK;
}

int check_stream(nfc_multi *m, uint32_t stream, bool outputs) {
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (outputs && !m->have_outputs) return mfail(m, NFC_ERR_STATE, "no completed push");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    return NFC_OK;
}

// ---- the fetch ----
const uint64_t *foff(const nfc_multi *m, int a) { return m->h_ftable.as<uint64_t>() + (size_t)a * ((size_t)m->K + 1); }

// whether the host copy of the last fetch serves the arrays `bit` stands for
bool served(const nfc_multi *m, uint32_t bit) { return (m->fetched & bit) != 0; }

// rows [first, first + n) of stream k's part of a packed byte array, n cut as read_row cuts it
int read_fetched(nfc_multi *m, int a, const uint8_t *section, uint32_t stream, size_t first, uint8_t *out, size_t cap, size_t *n_out) {
    const uint64_t *off = foff(m, a);
    const size_t stored = (size_t)(off[stream + 1] - off[stream]);
    size_t n = 0;
    if (first < stored) n = std::min(cap, stored - first);
    if (n && !out) return mfail(m, NFC_ERR_ARG, "null output");
    if (n) memcpy(out, section + off[stream] + first, n);
    if (n_out) *n_out = n;
    return NFC_OK;
}

// ---- the frames' packed buffer: totals (64 bytes) | table [4][K + 1] | records 0 | records 1 | bytes 0 | bytes 1 | par 0 | par 1 ----
// The host knows every stream's frame count from its mirror of the counts, not its byte count (that takes the close rows): the byte
// sections are laid out for the most the stored bits can give -- a frame has at most (n_bits + 1) / 9 bytes.  Returns the sections so far.
Sections frames_layout(const nfc_multi *m, frames::MultiLayout &F, uint64_t n_fr[2], uint64_t room[2]) {
    const size_t T = (size_t)m->K + 1;
    n_fr[0] = n_fr[1] = room[0] = room[1] = 0;
    for (uint32_t k = 0; k < m->K; k++) {
        const uint32_t *c = m->h_counts.as<uint32_t>() + (size_t)k * CNT_WORDS;
        for (int t = 0; t < 2; t++) {
            const uint64_t npk = std::min(c[CNT_PK0 + t], m->C.packets), bits = std::min(c[CNT_BITS0 + t], m->C.bits);
            n_fr[t] += npk;
            room[t] += npk ? (bits + npk) / 9 : 0;
        }
    }
    memset(&F, 0, sizeof F);
    Sections S{up16(frames::MULTI_HEADER_BYTES + 4 * T * 8), {}};
    for (int t = 0; t < 2; t++) {
        S.place(F.at_fr[t], F.end_fr[t], n_fr[t] * sizeof(nfc_raw_frame));
        F.total_frames[t] = n_fr[t];
        F.total_bytes[t] = room[t];
    }
    for (int t = 0; t < 2; t++) S.place(F.at_bytes[t], F.end_bytes[t], room[t]);
    for (int t = 0; t < 2; t++) S.place(F.at_par[t], F.end_par[t], room[t]);
    return S;
}
frames::MultiArgs frames_args(const nfc_multi *m, uint8_t *packed, const frames::MultiLayout &F) {
    frames::MultiArgs A;
    memset(&A, 0, sizeof A);
    for (int t = 0; t < 2; t++) {
        A.close[t] = m->A.O.close[t];
        A.bits[t] = m->A.O.bits[t];
    }
    A.counts = m->A.O.counts;
    A.cnt_words = CNT_WORDS, A.cnt_pk0 = CNT_PK0, A.cnt_bits0 = CNT_BITS0;
    A.cap_packets = m->C.packets, A.cap_bits = m->C.bits, A.s_packets = m->C.s_packets, A.s_bits = m->C.s_bits;
    A.K = m->K;
    A.table = (uint64_t *)(packed + frames::MULTI_HEADER_BYTES);
    A.packed = packed;
    A.guard_word = GUARD_WORD, A.guard_bytes = GUARD_BYTES;
    A.F = F;
    return A;
}
// what the caller gets of the frames' part of a host copy `h` (fetch_frames, fetch_commands): pointers, and idx in the stream's own count
void frames_view(const nfc_multi *m, uint8_t *h, const frames::MultiLayout &F, const uint64_t *base, bool stored, nfc_multi_frames &f) {
    const uint32_t K = m->K;
    const size_t T = (size_t)K + 1;
    uint64_t *tab = (uint64_t *)(h + frames::MULTI_HEADER_BYTES);
    if (stored) {
        for (int t = 0; t < 2; t++) {
            f.frames[t] = (const nfc_raw_frame *)(h + F.at_fr[t]);
            f.bytes[t] = h + F.at_bytes[t];
            f.par[t] = h + F.at_par[t];
            add_base((nfc_raw_frame *)(h + F.at_fr[t]), tab + (size_t)t * T, base, K);
        }
    } else {
        memset(tab, 0, 4 * T * 8);
    }
    for (int t = 0; t < 2; t++) {
        f.frame_off[t] = tab + (size_t)t * T;
        f.byte_off[t] = tab + (size_t)(2 + t) * T;
    }
    f.base = base;
}

// the header of a host copy `h` of the frames' part against what the host laid out
int check_frame_totals(nfc_multi *m, const char *fn, const uint8_t *h, const uint64_t n_fr[2], const uint64_t room[2]) {
    const uint64_t *dev_total = (const uint64_t *)h;
    for (int t = 0; t < 2; t++)
        if (dev_total[t] != n_fr[t] || dev_total[2 + t] > room[t])
            return mfail(m, NFC_ERR_INTERNAL, "%s: type %d: the device counts %llu frames and %llu bytes, the host %llu frames and room for %llu bytes", fn, t,
                         (unsigned long long)dev_total[t], (unsigned long long)dev_total[2 + t], (unsigned long long)n_fr[t], (unsigned long long)room[t]);
    return NFC_OK;
}

// ---- command tracking ----
// the machines' words, the blob of one machine and the events, when tracking, keys or a machine's state are first asked for: a context that
// never does allocates and launches what it always did
int ensure_fsm(nfc_multi *m, const char *fn) {
    if (m->d_fsm.p) return NFC_OK;
    if (grow(m, m->d_fsm_blob, 256, fn, false) < 0 || grow(m, m->h_fsm_blob, 256, fn, false) < 0) return NFC_ERR_NOMEM;
    for (Event &e : m->evc)
        if (e.create() != hipSuccess) {
            (void)hipGetLastError();
            return mfail(m, NFC_ERR_DEVICE, "hipEventCreate failed");
        }
    if (grow(m, m->d_fsm, (size_t)fsmd::W_WORDS * m->K * 4, fn, false) < 0) return NFC_ERR_NOMEM;   // (the last: with it everything is there)
    commands::launch_init(m->d_fsm.as<uint32_t>(), m->K, 0, m->K, m->st);
    return launch_ok(m);
}

// ---- emulation ----
// the emulators of streams [k0, k1) to nfc_emu_state_init's state: one strided copy of [EW_WORDS][k1 - k0] words, and a wait (the source is the caller's)
int emu_state_init_range(nfc_multi *m, uint32_t k0, uint32_t k1) {
    if (k1 <= k0) return NFC_OK;
    emu::State S;
    emu::state_init(S);
    const size_t n = k1 - k0;
    std::vector<uint32_t> img((size_t)emu::EW_WORDS * n);
    for (size_t k = 0; k < n; k++) emu::store_state(S, img.data(), n, k);
    uint32_t *state = (uint32_t *)(m->d_emu.as<uint8_t>() + m->emu_state);
    MCHK(m, hipMemcpy2DAsync(state + k0, (size_t)m->K * 4, img.data(), n * 4, n * 4, emu::EW_WORDS, hipMemcpyHostToDevice, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    return NFC_OK;
}
// the cards' buffer, zeroed (no stream has a card), and the emulators' state, at the first nfc_multi_emulate of a context
int ensure_emu(nfc_multi *m, const char *fn) {
    if (m->d_emu.p) return NFC_OK;
    const size_t K = m->K;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_rands = up(K * emu::CLASSIC_BYTES), o_params = o_rands + up(K * emu::MAX_RANDS * 4), o_state = o_params + up(K * commands::EP_WORDS * 4),
                 bytes = o_state + up(K * emu::EW_WORDS * 4);
    DevBuf fresh;
    if (fresh.ensure(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return mfail(m, NFC_ERR_NOMEM, "%s: no device memory for %zu bytes", fn, bytes);
    }
    MCHK(m, hipMemsetAsync(fresh.p, 0, fresh.cap, m->st));
    std::swap(m->d_emu, fresh);
    m->emu_mem = 0, m->emu_rands = o_rands, m->emu_params = o_params, m->emu_state = o_state;
    m->has_card.assign(K, 0);
    m->card_role.assign(K, -1);
    m->n_cards = 0;
    return emu_state_init_range(m, 0, m->K);
}

// the three launches of a tracked push, behind the push's own kernel and its counts; no host wait
int enqueue_commands(nfc_multi *m) {
    m->cmd_state = nfc_multi::CMD_NONE;
    m->cmd_fetched = false;
    if (int rc = ensure_fsm(m, "nfc_multi_push")) return rc;
    frames::MultiLayout F;
    Sections S = frames_layout(m, F, m->cmd_nfr, m->cmd_room);
    if (m->cmd_nfr[0] + m->cmd_nfr[1] == 0) {   // (the buffer, its layouts and its guards stay those of the last push that stored anything)
        m->cmd_state = nfc_multi::CMD_EMPTY;
        return NFC_OK;
    }
    m->cmd_frlay = F;
    const uint32_t K = m->K;
    const size_t T = (size_t)K + 1;
    commands::Layout &L = m->cmd_lay;
    memset(&L, 0, sizeof L);
    L.total_cmds = m->cmd_nfr[0] + m->cmd_nfr[1];
    L.total_bytes = m->cmd_room[0] + m->cmd_room[1];
    const size_t sizes[commands::SEC_COUNT] = {T * 8, T * 8, (size_t)K * 4, (size_t)L.total_cmds * sizeof(nfc_frame), (size_t)L.total_cmds * 4,
                                               (size_t)L.total_bytes, (size_t)L.total_bytes * 2};
    for (int s = 0; s < commands::SEC_COUNT; s++) S.place(L.at[s], L.end[s], sizes[s]);
    const bool emulating = m->n_cards > 0;
    commands::EmuArgs E;
    memset(&E, 0, sizeof E);
    if (emulating) {   // the answers behind the commands: at most one per command and 18 bytes each (READT is the longest), and a lane's scratch
        const size_t esizes[commands::ESEC_COUNT] = {(size_t)K * 4, (size_t)L.total_cmds * sizeof(nfc_emu_answer), (size_t)L.total_cmds * commands::ANS_BYTES,
                                                     (size_t)L.total_cmds * commands::ANS_BYTES, (size_t)L.total_cmds * commands::ANS_BYTES,
                                                     (size_t)K * emu::SCRATCH_BYTES};
        for (int s = 0; s < commands::ESEC_COUNT; s++) S.place(E.at[s], E.end[s], esizes[s]);
        uint8_t *e = m->d_emu.as<uint8_t>();
        E.mem = (const uint32_t *)(e + m->emu_mem), E.rands = (const uint32_t *)(e + m->emu_rands), E.params = (const uint32_t *)(e + m->emu_params);
        E.state = (uint32_t *)(e + m->emu_state);
    }
    const size_t bytes = S.at;
    if (int rc = grow_packed(m, m->cmd, bytes, "nfc_multi_push")) return rc;
    commands::Args A;
    A.R = frames_args(m, m->cmd.d.as<uint8_t>(), F);
    A.state = m->d_fsm.as<uint32_t>();
    A.L = L;
    A.sector_keys = m->d_keys.as<uint32_t>();
    const bool timed = m->timing != 0;
    frames::launch_multi(A.R, m->st, timed ? m->evc[0] : nullptr, timed ? m->evc[1] : nullptr);
    if (emulating) commands::launch_emu(A, E, m->st, timed ? m->evc[2] : nullptr, timed ? m->evc[3] : nullptr);
    else commands::launch(A, m->st, timed ? m->evc[2] : nullptr, timed ? m->evc[3] : nullptr);
    m->cmd_emulated = emulating;
    m->cmd_emu = E;
    m->cmd.guards = std::move(S.guards);
    m->cmd_timed = timed;
    m->cmd_bytes = bytes;
    if (int rc = launch_ok(m)) return rc;
    m->cmd_state = nfc_multi::CMD_LAUNCHED;
    m->stats.n_launches += 3;
    if (m->track_img) {   // the images behind the machines: a workgroup of one wave per stream
        image::Args I;
        memset(&I, 0, sizeof I);
        I.img = m->img.d.as<uint8_t>();
        for (int s = 0; s < image::ISEC_COUNT; s++) I.at[s] = m->img_at[s];
        I.K = K;
        I.cmds = m->cmd.d.as<uint8_t>();
        I.L = L;
        I.state = m->d_fsm.as<uint32_t>();
        I.sector_keys = m->d_keys.as<uint32_t>();
        if (timed) NFC_LAUNCH_EXT(image::k_multi_images, dim3(K), dim3(image::THREADS), 0, m->st, m->evi[0], m->evi[1], 0, I);
        else NFC_LAUNCH(image::k_multi_images, dim3(K), dim3(image::THREADS), 0, m->st, I);
        if (int rc = launch_ok(m)) return rc;
        m->img_timed = timed;
        m->img_launches = 4;
        m->img_fetched = false;
        m->stats.n_launches += 1;
    }
    return NFC_OK;
}

// ---- the memory images ----
// streams [k0, k1) to nfc_card_image_init's image (guards: the guard word behind the four sections too)
int images_init_range(nfc_multi *m, uint32_t k0, uint32_t k1, bool guards) {
    image::InitArgs I;
    memset(&I, 0, sizeof I);
    I.img = m->img.d.as<uint8_t>();
    for (int s = 0; s < image::ISEC_COUNT; s++) I.at[s] = m->img_at[s], I.end[s] = m->img.guards[s];
    I.K = m->K, I.k0 = k0, I.k1 = k1;
    I.guard_bytes = guards ? GUARD_BYTES : 0u, I.guard_word = GUARD_WORD;
    const size_t work = (size_t)(k1 > k0 ? k1 - k0 : 0u) * (image::MEM_BYTES / 16);
    NFC_LAUNCH(image::k_images_init, dim3((unsigned)std::max<size_t>(1, std::min<size_t>(4096, (work + 255) / 256))), dim3(256), 0, m->st, I);
    m->img_fetched = false;
    return launch_ok(m);
}
// the images' buffer, every image nfc_card_image_init's, at the first nfc_multi_track_images of a context
int ensure_images(nfc_multi *m, const char *fn) {
    if (m->img.d.p) return NFC_OK;
    const size_t K = m->K;
    for (Event &e : m->evi)
        if (e.create() != hipSuccess) {
            (void)hipGetLastError();
            return mfail(m, NFC_ERR_DEVICE, "hipEventCreate failed");
        }
    if (grow(m, m->h_img_one, sizeof(nfc_card_image), fn, false) < 0) return NFC_ERR_NOMEM;
    Sections S{0, {}};
    const size_t sizes[image::ISEC_COUNT] = {K * image::MEM_BYTES, K * image::MEM_BYTES, K * sizeof(nfc_image_info), K * image::TAIL * sizeof(nfc_image_cmd)};
    uint64_t at[image::ISEC_COUNT], end[image::ISEC_COUNT];
    for (int s = 0; s < image::ISEC_COUNT; s++) S.place(at[s], end[s], sizes[s]);
    if (grow(m, m->img.d, S.at, fn, false) < 0) return NFC_ERR_NOMEM;
    for (int s = 0; s < image::ISEC_COUNT; s++) m->img_at[s] = at[s];
    m->img.guards = std::move(S.guards);
    m->img_bytes = S.at;
    m->img_launches = 0;
    if (int rc = images_init_range(m, 0, m->K, true)) {
        m->img.d.release();
        m->img.guards.clear();
        return rc;
    }
    return NFC_OK;
}
// one stream's image between the device and the pinned staging: four copies, one per section
int image_io(nfc_multi *m, uint32_t k, bool set) {
    nfc_card_image *h = m->h_img_one.as<nfc_card_image>();
    uint8_t *d = m->img.d.as<uint8_t>();
    struct { void *host; uint8_t *dev; size_t n; } part[image::ISEC_COUNT] = {
        {h->mem, d + m->img_at[image::ISEC_MEM] + (size_t)k * image::MEM_BYTES, image::MEM_BYTES},
        {h->src, d + m->img_at[image::ISEC_SRC] + (size_t)k * image::MEM_BYTES, image::MEM_BYTES},
        {&h->info, d + m->img_at[image::ISEC_INFO] + (size_t)k * sizeof(nfc_image_info), sizeof(nfc_image_info)},
        {h->tail, d + m->img_at[image::ISEC_TAIL] + (size_t)k * image::TAIL * sizeof(nfc_image_cmd), image::TAIL * sizeof(nfc_image_cmd)}};
    for (auto &p : part) {
        if (set) MCHK(m, hipMemcpyAsync(p.dev, p.host, p.n, hipMemcpyHostToDevice, m->st));
        else MCHK(m, hipMemcpyAsync(p.host, p.dev, p.n, hipMemcpyDeviceToHost, m->st));
    }
    MCHK(m, hipStreamSynchronize(m->st));
    return NFC_OK;
}

// stream k's counts and flags of the last push, from the pinned mirror
void counts_of(const nfc_multi *m, uint32_t k, nfc_counts &o, uint32_t *flags) {
    const uint32_t *c = m->h_counts.as<uint32_t>() + (size_t)k * CNT_WORDS;
    o.n_samples = m->last_n[k];
    o.n_edges = c[CNT_EDGES];
    o.n_symbols[0] = c[CNT_SYM0];
    o.n_symbols[1] = c[CNT_SYM1];
    o.n_packets[0] = c[CNT_PK0];
    o.n_packets[1] = c[CNT_PK1];
    o.n_packet_bits[0] = c[CNT_PKBITS0];
    o.n_packet_bits[1] = c[CNT_PKBITS1];
    if (flags) *flags = c[CNT_FLAGS];
}

int state_io(nfc_multi *m, uint32_t k, int set) {
    NFC_LAUNCH(k_multi_state_io, dim3(1), dim3(256), 0, m->st, m->A.S, m->C, m->K, k, m->L, set, m->d_blob);
    return launch_ok(m);
}
}  // namespace

extern "C" {

const char *nfc_multi_last_error(const nfc_multi *m) { return m ? m->err.c_str() : g_multi_create_error.c_str(); }

void nfc_multi_destroy(nfc_multi *m) {
    if (!m) return;
    (void)hipSetDevice(m->P.device);
    if (m->st) (void)hipStreamSynchronize(m->st);
    delete m;   // (every buffer, the events and the stream are members that release themselves)
}

int nfc_multi_create(const nfc_params *p, const nfc_multi_config *c, nfc_multi **out) {
    if (!p || !c || !out) return mfail(nullptr, NFC_ERR_ARG, "null argument");
    *out = nullptr;
    if (!(p->samp_rate > 0)) return mfail(nullptr, NFC_ERR_ARG, "samp_rate must be positive");
    if (p->av_window < 1 || p->av_window > 30000) return mfail(nullptr, NFC_ERR_ARG, "av_window must be in [1, 30000]");
    if (p->max_len < 1 || p->max_len > 4000) return mfail(nullptr, NFC_ERR_ARG, "max_len must be in [1, 4000]");
    if (!kind_valid(p->input_kind)) return mfail(nullptr, NFC_ERR_ARG, "unknown input_kind");
    if (p->flags != 0) return mfail(nullptr, NFC_ERR_ARG, "nfc_params.flags must be 0 for a multi-stream context");
    if (p->chunk_samples != 0) return mfail(nullptr, NFC_ERR_ARG, "nfc_params.chunk_samples must be 0 for a multi-stream context");
    if (c->n_streams < 1 || c->n_streams > 65536) return mfail(nullptr, NFC_ERR_ARG, "n_streams must be in [1, 65536]");
    if (c->max_push_samples < 1 || c->max_push_samples > (1u << 24)) return mfail(nullptr, NFC_ERR_ARG, "max_push_samples must be in [1, 2^24]");
    for (int i = 0; i < 9; i++)
        if (c->reserved[i] != 0) return mfail(nullptr, NFC_ERR_ARG, "nfc_multi_config.reserved must be 0");
    // A caller's capacity is bounded so that a row stride (uint32, in entries: Caps) cannot wrap and rows of different streams
    // cannot overlap: 2^26 entries is four times what the longest push (2^24 samples) can produce of anything.
    {
        const struct { const char *name; uint32_t v; } caps[] = {{"cap_edges", c->cap_edges}, {"cap_symbols", c->cap_symbols}, {"cap_packets", c->cap_packets},
                                                                 {"cap_packet_bits", c->cap_packet_bits}, {"cap_pending_bits", c->cap_pending_bits}};
        for (const auto &cp : caps)
            if (cp.v > MAX_CAP) return mfail(nullptr, NFC_ERR_ARG, "%s = %u exceeds %u", cp.name, cp.v, MAX_CAP);
    }
    float scale_arg = 0.f;
    if (const char *bad = kernel_scale_arg(p->input_kind, p->i16_scale, &scale_arg)) return mfail(nullptr, NFC_ERR_ARG, "%s", bad);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return mfail(nullptr, NFC_ERR_DEVICE, "no HIP device: this library has no CPU fallback");
    if (p->device < 0 || p->device >= ndev) return mfail(nullptr, NFC_ERR_ARG, "device %d out of range (%d devices)", p->device, ndev);
    if (hipSetDevice(p->device) != hipSuccess) return mfail(nullptr, NFC_ERR_DEVICE, "hipSetDevice failed");

    std::unique_ptr<nfc_multi, void (*)(nfc_multi *)> owner(new nfc_multi(), nfc_multi_destroy);   // (a failure below: what there is waits, then goes)
    nfc_multi *const m = owner.get();
    m->P = *p;
    m->K = c->n_streams;
    m->max_push = c->max_push_samples;
    m->L = p->av_window;
    m->mx = p->max_len;
    m->nd = m->mx + 1;
    m->scale = scale_arg;
    m->bps = kind_bytes(p->input_kind);
    memset(&m->stats, 0, sizeof m->stats);
    memset(&m->fout, 0, sizeof m->fout);
    memset(&m->cout, 0, sizeof m->cout);
    const uint32_t K = m->K;
    // Capacities per stream and push.  Entries are 6-13 % of the samples on every capture of this tree's generators (the densest:
    // 0.133 edges and 0.10 symbols of one type per sample): a quarter of the samples is room to spare.  A non-empty packet takes a
    // start bit, a bit and the symbol that closes it: at most a third of the symbols close one -- a sixteenth of the samples.
    const uint32_t dflt = m->max_push / 4 + 64;
    Caps &C = m->C;
    C.edges = c->cap_edges ? c->cap_edges : dflt;
    C.symbols = c->cap_symbols ? c->cap_symbols : dflt;
    C.bits = c->cap_packet_bits ? c->cap_packet_bits : dflt;
    C.packets = c->cap_packets ? c->cap_packets : m->max_push / 16 + 16;
    C.pending = c->cap_pending_bits ? c->cap_pending_bits : 4096;
    // (row strides in entries: the guard behind a row is GUARD_BYTES whatever the entry size -- alloc_slab)
    C.s_epos = C.edges + GUARD_BYTES / 4;
    C.s_ecode = C.edges + GUARD_BYTES / 2;
    C.s_symbols = C.symbols + GUARD_BYTES;
    C.s_bits = C.bits + GUARD_BYTES;
    C.s_packets = C.packets + GUARD_BYTES / 8;
    C.s_pending = C.pending + GUARD_BYTES;

#define CRT(call)                                                                                              \
    do {                                                                                                       \
        hipError_t e__ = (call);                                                                               \
        if (e__ != hipSuccess) {                                                                               \
            const int rc__ = mfail(nullptr, e__ == hipErrorOutOfMemory ? NFC_ERR_NOMEM : NFC_ERR_DEVICE, "nfc_multi_create: %s failed: %s", #call, hipGetErrorString(e__)); \
            (void)hipGetLastError();                                                                           \
            return rc__;                                                                                       \
        }                                                                                                      \
    } while (0)
#define CRC(call)                      \
    do {                               \
        const int rc__ = (call);       \
        if (rc__) return rc__;         \
    } while (0)

    CRT(m->st.create());
    CRT(m->ev[0].create());
    CRT(m->ev[1].create());
    Args &A = m->A;
    memset(&A, 0, sizeof A);
    State &S = A.S;
    Out &O = A.O;
    CRC(alloc_plain(m, &S.ss, (size_t)K * 8));
    CRC(alloc_plain(m, &S.slot, (size_t)K * 4));
    CRC(alloc_plain(m, &S.filled, (size_t)K * 4));
    CRC(alloc_plain(m, &S.edge, (size_t)K * 4));
    CRC(alloc_plain(m, &S.dec, (size_t)K * 4));
    CRC(alloc_plain(m, &S.npend[0], (size_t)K * 4));
    CRC(alloc_plain(m, &S.npend[1], (size_t)K * 4));
    CRC(alloc_plain(m, &S.flags, (size_t)K * 4));
    CRC(alloc_plain(m, &S.ring, (size_t)K * 4 * (size_t)m->L));
    CRC(alloc_plain(m, &O.counts, (size_t)K * CNT_WORDS * 4));
    CRC(alloc_plain(m, &m->d_up, (size_t)K * 16));
    m->blob_bytes = sizeof(IoHeader) + (size_t)m->L * 4 + 2 * (size_t)C.pending;
    CRC(alloc_plain(m, &m->d_blob, m->blob_bytes));
    for (int t = 0; t < 2; t++) {
        CRC(alloc_slab(m, &S.pending[t], (size_t)C.pending));
        CRC(alloc_slab(m, &O.sym[t], (size_t)C.symbols));
        CRC(alloc_slab(m, &O.bits[t], (size_t)C.bits));
        CRC(alloc_slab(m, &O.close[t], (size_t)C.packets * 8));
    }
    CRC(alloc_slab(m, &O.epos, (size_t)C.edges * 4));
    CRC(alloc_slab(m, &O.ecode, (size_t)C.edges * 2));
    CRT(m->h_up.ensure((size_t)K * 16));
    CRT(m->h_counts.ensure((size_t)K * CNT_WORDS * 4));
    CRT(m->h_blob.ensure(m->blob_bytes));
    memset(m->h_counts.p, 0, (size_t)K * CNT_WORDS * 4);

    // decoder LUTs in the walking form: next state | out byte << 8 per (LUT row, state)
    {
        const DecoderTables t = build_tables(p->samp_rate, m->mx);
        std::vector<uint16_t> mils(t.miller_map.size() * 16), mans(t.manch_map.size() * 8);
        for (size_t i = 0; i < t.miller_map.size(); i++)
            for (int s = 0; s < 16; s++) mils[i * 16 + s] = (uint16_t)(((t.miller_map[i] >> (4 * s)) & 15u) | (t.miller_out[i * 16 + s] << 8));
        for (size_t i = 0; i < t.manch_map.size(); i++)
            for (int s = 0; s < 8; s++) mans[i * 8 + s] = (uint16_t)(((t.manch_map[i] >> (4 * s)) & 15u) | (t.manch_out[i * 8 + s] << 8));
        uint16_t *d_mil = nullptr, *d_man = nullptr;
        CRC(alloc_plain(m, &d_mil, mils.size() * 2));
        CRC(alloc_plain(m, &d_man, mans.size() * 2));
        CRT(hipMemcpy(d_mil, mils.data(), mils.size() * 2, hipMemcpyHostToDevice));
        CRT(hipMemcpy(d_man, mans.data(), mans.size() * 2, hipMemcpyHostToDevice));
        A.mil_step = d_mil;
        A.man_step = d_man;
        // the carried Miller state is published as the canonical state of its class, as nfc_get_state publishes it (decoder_tables.h)
        const MillerQuotient q = miller_quotient(t);
        for (int k = 0; k < 16; k++) m->canon[k] = q.ok ? q.canon[k] : (uint8_t)k;
    }
    A.first = (const uint64_t *)m->d_up;
    A.n = (const uint32_t *)(m->d_up + (size_t)K * 8);
    A.order = (const uint32_t *)(m->d_up + (size_t)K * 12);
    A.K = K;
    A.L = m->L;
    A.mx = m->mx;
    A.nd = m->nd;
    A.reader = p->enable_reader != 0;
    A.tag = p->enable_tag != 0;
    A.scale = m->scale;
    A.lo = p->lo_val;
    A.hi = p->hi_val;
    A.hi_plus = p->hi_val + 0.1;   // transition_sink.py:63
    {   // the products that decide a comparison against lo / hi without the division (nfc_create: the same bands)
        const double eps = std::ldexp(1.0, -48);
        A.lo_a = p->lo_val - std::fabs(p->lo_val) * eps;
        A.lo_b = p->lo_val + std::fabs(p->lo_val) * eps;
        A.hi_a = p->hi_val - std::fabs(p->hi_val) * eps;
        A.hi_b = p->hi_val + std::fabs(p->hi_val) * eps;
        auto sane = [](double v) { return v == 0 || (std::fabs(v) > 1e-100 && std::fabs(v) < 1e100); };
        A.bands_ok = sane(p->lo_val) && sane(p->hi_val) && std::isfinite(p->lo_val) && std::isfinite(p->hi_val);
    }
    A.C = C;
    m->nseen.assign(K, 0);
    m->g0.assign(K, 0);
    m->last_n.assign(K, 0);

    LaunchScope scope(&m->launch_err);
    for (size_t i = 0; i < m->guards.size(); i++)
        NFC_LAUNCH(k_multi_guard_fill, dim3(std::min<uint32_t>(1024, (K * 4 + 255) / 256)), dim3(256), 0, m->st, (uint8_t *)m->guards[i].first,
                   m->guards[i].second, m->guard_row[i], K);
    NFC_LAUNCH(k_multi_reset, dim3(1024), dim3(256), 0, m->st, S, K, 0u, K, m->L, O.counts);
    CRC(launch_ok(nullptr));
    CRT(hipStreamSynchronize(m->st));
#undef CRT
#undef CRC
    *out = owner.release();
    return NFC_OK;
}

int nfc_multi_push_device(nfc_multi *m, const void *dev_base, const uint64_t *first_sample, const uint32_t *n) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (!first_sample || !n) return mfail(m, NFC_ERR_ARG, "null first_sample / n");
    const uint32_t K = m->K;
    uint64_t total = 0;
    uint32_t nmax = 0, nmin = UINT32_MAX;
    for (uint32_t k = 0; k < K; k++) {
        if (n[k] > m->max_push) return mfail(m, NFC_ERR_ARG, "n[%u] = %u exceeds max_push_samples = %u", k, n[k], m->max_push);
        total += n[k];
        nmax = std::max(nmax, n[k]);
        nmin = std::min(nmin, n[k]);
    }
    if (total && !dev_base) return mfail(m, NFC_ERR_ARG, "null dev_base");
    if ((uintptr_t)dev_base & 15u) return mfail(m, NFC_ERR_ARG, "dev_base must be 16-byte aligned");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    m->fetched = 0;   // the host copy is the last push's
    uint64_t *hf = m->h_up.as<uint64_t>();
    uint32_t *hn = (uint32_t *)(m->h_up.as<uint8_t>() + (size_t)K * 8), *ho = (uint32_t *)(m->h_up.as<uint8_t>() + (size_t)K * 12);
    memcpy(hf, first_sample, (size_t)K * 8);
    memcpy(hn, n, (size_t)K * 4);
    // Lanes of a wave walk until the longest of their streams ends: streams go to lanes by length, longest first, in classes of
    // 512 samples and in the caller's order within a class (so streams of one length keep their neighbours, and the window rows
    // their consecutive addresses).  The public stream index stays the caller's: `order` only says which lane walks it.
    if ((nmax + 511) / 512 == (nmin + 511) / 512) {
        for (uint32_t k = 0; k < K; k++) ho[k] = k;
    } else {
        const uint32_t classes = (nmax + 511) / 512 + 1;
        std::vector<uint32_t> at(classes + 1, 0);
        for (uint32_t k = 0; k < K; k++) at[classes - 1 - (n[k] + 511) / 512 + 1]++;
        for (uint32_t i = 0; i < classes; i++) at[i + 1] += at[i];
        for (uint32_t k = 0; k < K; k++) ho[at[classes - 1 - (n[k] + 511) / 512]++] = k;
    }
    MCHK(m, hipMemcpyAsync(m->d_up, m->h_up.p, (size_t)K * 16, hipMemcpyHostToDevice, m->st));
    Args A = m->A;
    A.in = dev_base;
    const dim3 grid((K + MB - 1) / MB), block(MB);
    if (m->timing) NFC_LAUNCH_EXT(kernel_of(m->P.input_kind), grid, block, 0, m->st, m->ev[0], m->ev[1], 0, A);
    else NFC_LAUNCH(kernel_of(m->P.input_kind), grid, block, 0, m->st, A);
    MCHK(m, hipMemcpyAsync(m->h_counts.p, A.O.counts, (size_t)K * CNT_WORDS * 4, hipMemcpyDeviceToHost, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    if (int rc = launch_ok(m)) return rc;
    uint32_t cut = 0;
    for (uint32_t k = 0; k < K; k++) {
        m->g0[k] = m->nseen[k];
        m->nseen[k] += n[k];
        m->last_n[k] = n[k];
        cut += (m->h_counts.as<uint32_t>()[(size_t)k * CNT_WORDS + CNT_FLAGS] & 15u) != 0;
    }
    m->have_outputs = true;
    m->stats.ms_kernels = 0;
    if (m->timing) {
        float ms = 0.f;
        MCHK(m, hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
        m->stats.ms_kernels = ms;
    }
    m->stats.n_samples = total;
    m->stats.bytes_in = total * m->bps;
    m->stats.n_launches = 1;
    m->stats.n_streams_truncated = cut;
    m->stats.n_fetches = m->stats.n_reads_device = 0;
    m->tx_done = false;
    m->cmd_state = nfc_multi::CMD_NONE;
    m->cmd_fetched = false;
    m->img_launches = 0;
    if (m->track_img) m->img_fetched = false;
    if (m->track) return enqueue_commands(m);
    return NFC_OK;
}

int nfc_multi_push(nfc_multi *m, const void *const *host_ptrs, const uint32_t *n) {
    if (!m) return NFC_ERR_ARG;
    if (!host_ptrs || !n) return mfail(m, NFC_ERR_ARG, "null host_ptrs / n");
    const uint32_t K = m->K;
    uint64_t total = 0;
    for (uint32_t k = 0; k < K; k++) {
        if (n[k] > m->max_push) return mfail(m, NFC_ERR_ARG, "n[%u] = %u exceeds max_push_samples = %u", k, n[k], m->max_push);
        if (n[k] && !host_ptrs[k]) return mfail(m, NFC_ERR_ARG, "host_ptrs[%u] is null", k);
        total += n[k];
    }
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    const size_t bytes = (size_t)total * m->bps;
    if (grow(m, m->h_stage, bytes, "nfc_multi_push") < 0 || grow(m, m->d_stage, bytes, "nfc_multi_push") < 0) return NFC_ERR_NOMEM;
    std::vector<uint64_t> first(K);
    uint64_t at = 0;
    for (uint32_t k = 0; k < K; k++) {
        first[k] = at;
        if (n[k]) memcpy(m->h_stage.as<uint8_t>() + at * m->bps, host_ptrs[k], (size_t)n[k] * m->bps);
        at += n[k];
    }
    if (bytes) MCHK(m, hipMemcpyAsync(m->d_stage.p, m->h_stage.p, bytes, hipMemcpyHostToDevice, m->st));
    return nfc_multi_push_device(m, bytes ? m->d_stage.p : nullptr, first.data(), n);
}

int nfc_multi_get_counts(nfc_multi *m, uint32_t stream, nfc_counts *out, uint32_t *flags_out) {
    if (!m) return NFC_ERR_ARG;
    if (!out) return mfail(m, NFC_ERR_ARG, "null output");
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!m->have_outputs) return mfail(m, NFC_ERR_STATE, "no completed push");
    counts_of(m, stream, *out, flags_out);
    return NFC_OK;
}

int nfc_multi_get_counts_all(nfc_multi *m, nfc_counts *out, uint32_t *flags_out) {
    if (!m) return NFC_ERR_ARG;
    if (!out) return mfail(m, NFC_ERR_ARG, "null output");
    if (!m->have_outputs) return mfail(m, NFC_ERR_STATE, "no completed push");
    for (uint32_t k = 0; k < m->K; k++) counts_of(m, k, out[k], flags_out ? flags_out + k : nullptr);
    return NFC_OK;
}

int nfc_multi_fetch(nfc_multi *m, uint32_t what, nfc_multi_fetched *out) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (what == 0 || (what & ~(uint32_t)NFC_MULTI_FETCH_ALL)) return mfail(m, NFC_ERR_ARG, "what = %u: a non-empty set of NFC_MULTI_FETCH_* bits is expected", what);
    if (!m->have_outputs) return mfail(m, NFC_ERR_STATE, "no completed push");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    m->fetched = 0;
    const uint32_t K = m->K;
    const size_t T = (size_t)K + 1;
    if (grow(m, m->h_ftable, (MF_ARRAYS * T + K) * 8, "nfc_multi_fetch", false) < 0 || grow(m, m->d_ftable, MF_ARRAYS * T * 8, "nfc_multi_fetch", false) < 0)
        return NFC_ERR_NOMEM;
    // the same table the scan kernel forms, from the pinned mirror of the counts: it sizes the buffers and is the caller's off[]
    uint64_t *tab = m->h_ftable.as<uint64_t>(), *base = tab + MF_ARRAYS * T;
    Amounts run = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < K; k++) {
        const Amounts s = stored_amounts(m->h_counts.as<uint32_t>() + (size_t)k * CNT_WORDS, m->C, what);
        tab[0 * T + k] = run.a0;
        tab[1 * T + k] = run.a1;
        tab[2 * T + k] = run.a2;
        tab[3 * T + k] = run.a3;
        tab[4 * T + k] = run.a4;
        tab[5 * T + k] = run.a5;
        tab[6 * T + k] = run.a6;
#define X(f) run.f += s.f;
        MF_EACH(X)
#undef X
        base[k] = m->g0[k];
    }
    const uint64_t total[MF_ARRAYS] = {run.a0, run.a1, run.a2, run.a3, run.a4, run.a5, run.a6};
    for (int a = 0; a < MF_ARRAYS; a++) tab[a * T + K] = total[a];
    nfc_multi_fetched &f = m->fout;
    memset(&f, 0, sizeof f);
    f.what = what;
    f.n_streams = K;
    f.edge_code_nd = (uint32_t)m->nd;
    for (int a = 0; a < MF_ARRAYS; a++) f.off[a] = foff(m, a);
    f.base = base;
    uint64_t any = 0;
    for (int a = 0; a < MF_ARRAYS; a++) any |= total[a];
    if (any) {
        FetchLayout F;
        Sections S{MF_HEADER_BYTES, {}};
        S.place(F.at_epos, F.end_epos, (size_t)total[0] * 4);
        S.place(F.at_ecode, F.end_ecode, (size_t)total[0] * 2);
        S.place(F.at_sym0, F.end_sym0, (size_t)total[1]);
        S.place(F.at_sym1, F.end_sym1, (size_t)total[2]);
        S.place(F.at_pk0, F.end_pk0, (size_t)total[3] * sizeof(nfc_packet));
        S.place(F.at_pk1, F.end_pk1, (size_t)total[4] * sizeof(nfc_packet));
        S.place(F.at_bits0, F.end_bits0, (size_t)total[5]);
        S.place(F.at_bits1, F.end_bits1, (size_t)total[6]);
        F.total = run;
        const size_t bytes = S.at;
        if (grow(m, m->fetch.h, bytes, "nfc_multi_fetch") < 0) return NFC_ERR_NOMEM;
        if (int rc = grow_packed(m, m->fetch, bytes, "nfc_multi_fetch")) return rc;
        uint8_t *h = m->fetch.h.as<uint8_t>(), *d = m->fetch.d.as<uint8_t>();
        GatherArgs G;
        G.O = m->A.O;
        G.C = m->C;
        G.K = K;
        G.table = m->d_ftable.as<uint64_t>();
        G.packed = d;
        G.F = F;
        const unsigned wgs = std::min<unsigned>(MF_GATHER_MAX_WG, (K + MF_GATHER_THREADS / 64 - 1) / (MF_GATHER_THREADS / 64));
        if (m->timing) MCHK(m, hipEventRecord(m->ev[0], m->st));
        NFC_LAUNCH(k_multi_fetch_scan, dim3(1), dim3(MF_SCAN_THREADS), 0, m->st, (const uint32_t *)m->A.O.counts, m->C, K, what, m->d_ftable.as<uint64_t>(), d, F);
        NFC_LAUNCH(k_multi_fetch_gather, dim3(wgs), dim3(MF_GATHER_THREADS), 0, m->st, G);
        if (m->timing) MCHK(m, hipEventRecord(m->ev[1], m->st));
        m->fetch.guards = std::move(S.guards);
        MCHK(m, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, m->st));
        MCHK(m, hipStreamSynchronize(m->st));
        if (int rc = launch_ok(m)) return rc;
        const uint64_t *dev_total = (const uint64_t *)h;
        for (int a = 0; a < MF_ARRAYS; a++)
            if (dev_total[a] != total[a])
                return mfail(m, NFC_ERR_INTERNAL, "nfc_multi_fetch: the device's total of array %d is %llu, the host's %llu", a, (unsigned long long)dev_total[a],
                             (unsigned long long)total[a]);
        if (m->timing) {
            float ms = 0.f;
            MCHK(m, hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
            f.ms_kernels = ms;
        }
        f.n_launches = 2;
        f.bytes_copied = bytes;
        f.edge_pos = (const uint32_t *)(h + F.at_epos);
        f.edge_code = (const uint16_t *)(h + F.at_ecode);
        f.symbols[0] = h + F.at_sym0;
        f.symbols[1] = h + F.at_sym1;
        f.packets[0] = (const nfc_packet *)(h + F.at_pk0);
        f.packets[1] = (const nfc_packet *)(h + F.at_pk1);
        f.packet_bits[0] = h + F.at_bits0;
        f.packet_bits[1] = h + F.at_bits1;
        add_base((nfc_packet *)(h + F.at_pk0), foff(m, NFC_MF_PK0), base, K);   // (the gather left the packets' idx batch-local)
        add_base((nfc_packet *)(h + F.at_pk1), foff(m, NFC_MF_PK1), base, K);
    }
    m->fetched = what;
    m->stats.n_fetches++;
    if (out) *out = f;
    return NFC_OK;
}

// The frames of every stream's stored packets, assembled on the device into one packed buffer (frames.hip.h; frames_layout above: each
// section on 16 bytes with GUARD_BYTES of the guard word behind it); the device's table, which travels in the buffer, says where a
// stream's bytes are.
int nfc_multi_fetch_frames(nfc_multi *m, nfc_multi_frames *out) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (!m->have_outputs) return mfail(m, NFC_ERR_STATE, "no completed push");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    const uint32_t K = m->K;
    uint64_t n_fr[2], room[2];
    nfc_multi_frames f;
    memset(&f, 0, sizeof f);
    f.n_streams = K;
    frames::MultiLayout F;
    Sections S = frames_layout(m, F, n_fr, room);
    const size_t bytes = S.at;
    // (the pinned buffer always: the offset tables and base[] are handed out when nothing was stored, too)
    if (grow(m, m->frames.h, bytes + (size_t)K * 8, "nfc_multi_fetch_frames") < 0) return NFC_ERR_NOMEM;
    uint8_t *h = m->frames.h.as<uint8_t>();
    uint64_t *base = (uint64_t *)(h + bytes);
    for (uint32_t k = 0; k < K; k++) base[k] = m->g0[k];
    if (n_fr[0] + n_fr[1]) {
        if (int rc = grow_packed(m, m->frames, bytes, "nfc_multi_fetch_frames")) return rc;
        const frames::MultiArgs A = frames_args(m, m->frames.d.as<uint8_t>(), F);
        frames::launch_multi(A, m->st, m->timing ? m->ev[0] : nullptr, m->timing ? m->ev[1] : nullptr);
        m->frames.guards = std::move(S.guards);
        MCHK(m, hipMemcpyAsync(h, m->frames.d.p, bytes, hipMemcpyDeviceToHost, m->st));
        MCHK(m, hipStreamSynchronize(m->st));
        if (int rc = launch_ok(m)) return rc;
        if (int rc = check_frame_totals(m, "nfc_multi_fetch_frames", h, n_fr, room)) return rc;
        if (m->timing) {
            float ms = 0.f;
            MCHK(m, hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
            f.ms_kernels = ms;
        }
        f.n_launches = 2;
        f.bytes_copied = bytes;
    }
    frames_view(m, h, F, base, n_fr[0] + n_fr[1] != 0, f);
    if (out) *out = f;
    return NFC_OK;
}

int nfc_multi_read_edges(nfc_multi *m, uint32_t stream, size_t first, nfc_edge *out, size_t cap, size_t *n_out) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (int rc = check_stream(m, stream, true)) return rc;
    const size_t stored = std::min<size_t>(m->h_counts.as<uint32_t>()[(size_t)stream * CNT_WORDS + CNT_EDGES], m->C.edges);
    size_t n = 0;
    if (first < stored) n = std::min(cap, stored - first);
    if (n && !out) return mfail(m, NFC_ERR_ARG, "null output");
    if (n_out) *n_out = n;
    if (!n) return NFC_OK;
    const uint32_t *pos;
    const uint16_t *code;
    if (served(m, NFC_MULTI_FETCH_EDGES)) {
        const uint64_t at = foff(m, NFC_MF_EDGES)[stream] + first;
        pos = m->fout.edge_pos + at;
        code = m->fout.edge_code + at;
    } else {
        if (grow(m, m->h_read, n * 6 + 16, "nfc_multi_read_edges") < 0) return NFC_ERR_NOMEM;
        uint32_t *dpos = m->h_read.as<uint32_t>();
        uint16_t *dcode = (uint16_t *)(dpos + n);
        m->stats.n_reads_device++;
        MCHK(m, hipMemcpyAsync(dpos, m->A.O.epos + (size_t)stream * m->C.s_epos + first, n * 4, hipMemcpyDeviceToHost, m->st));
        MCHK(m, hipMemcpyAsync(dcode, m->A.O.ecode + (size_t)stream * m->C.s_ecode + first, n * 2, hipMemcpyDeviceToHost, m->st));
        MCHK(m, hipStreamSynchronize(m->st));
        pos = dpos;
        code = dcode;
    }
    const uint64_t g0 = m->g0[stream];
    for (size_t i = 0; i < n; i++) {   // edges.hip.h: edge_code, and back
        const uint32_t li = code[i] & 0x3FFFu;
        nfc_edge e;
        memset(&e, 0, sizeof e);
        e.idx = g0 + pos[i];
        e.d = (int32_t)(li % (uint32_t)m->nd);
        e.v = (int8_t)((int)(li / (uint32_t)m->nd) - 1);
        e.t = (int8_t)((int)(code[i] >> 14) - 1);
        out[i] = e;
    }
    return NFC_OK;
}

int nfc_multi_read_symbols(nfc_multi *m, uint32_t stream, int type, size_t first, uint8_t *out, size_t cap, size_t *n_out) {
    if (!m) return NFC_ERR_ARG;
    if (type < 0 || type > 1) return mfail(m, NFC_ERR_ARG, "type must be 0 or 1");
    if (int rc = check_stream(m, stream, true)) return rc;
    if (served(m, NFC_MULTI_FETCH_SYMBOLS)) return read_fetched(m, NFC_MF_SYM0 + type, m->fout.symbols[type], stream, first, out, cap, n_out);
    const size_t stored = std::min<size_t>(m->h_counts.as<uint32_t>()[(size_t)stream * CNT_WORDS + CNT_SYM0 + type], m->C.symbols);
    return read_row(m, "nfc_multi_read_symbols", m->A.O.sym[type], m->C.s_symbols, 1, stream, stored, first, out, cap, n_out);
}

int nfc_multi_read_packets(nfc_multi *m, uint32_t stream, int type, nfc_packet *out, size_t cap, size_t *n_out) {
    if (!m) return NFC_ERR_ARG;
    if (type < 0 || type > 1) return mfail(m, NFC_ERR_ARG, "type must be 0 or 1");
    if (int rc = check_stream(m, stream, true)) return rc;
    const size_t stored = std::min<size_t>(m->h_counts.as<uint32_t>()[(size_t)stream * CNT_WORDS + CNT_PK0 + type], m->C.packets);
    const size_t n = std::min(cap, stored);
    if (n && !out) return mfail(m, NFC_ERR_ARG, "null output");
    if (n_out) *n_out = n;
    if (!n) return NFC_OK;
    if (served(m, NFC_MULTI_FETCH_PACKETS)) {
        memcpy(out, m->fout.packets[type] + foff(m, NFC_MF_PK0 + type)[stream], n * sizeof(nfc_packet));
        return NFC_OK;
    }
    if (grow(m, m->h_read, n * 8, "nfc_multi_read_packets") < 0) return NFC_ERR_NOMEM;
    m->stats.n_reads_device++;
    MCHK(m, hipMemcpyAsync(m->h_read.p, m->A.O.close[type] + (size_t)stream * m->C.s_packets, n * 8, hipMemcpyDeviceToHost, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    const uint32_t *cl = m->h_read.as<uint32_t>();
    uint32_t prev = 0;
    for (size_t i = 0; i < n; i++) {
        nfc_packet p;
        p.idx = m->g0[stream] + cl[2 * i + 1];
        p.bit_off = prev;
        p.n_bits = cl[2 * i] - prev;
        p.type = type;
        out[i] = p;
        prev = cl[2 * i];
    }
    return NFC_OK;
}

int nfc_multi_read_packet_bits(nfc_multi *m, uint32_t stream, int type, size_t first, uint8_t *out, size_t cap, size_t *n_out) {
    if (!m) return NFC_ERR_ARG;
    if (type < 0 || type > 1) return mfail(m, NFC_ERR_ARG, "type must be 0 or 1");
    if (int rc = check_stream(m, stream, true)) return rc;
    if (served(m, NFC_MULTI_FETCH_PACKETS)) return read_fetched(m, NFC_MF_BITS0 + type, m->fout.packet_bits[type], stream, first, out, cap, n_out);
    const size_t stored = std::min<size_t>(m->h_counts.as<uint32_t>()[(size_t)stream * CNT_WORDS + CNT_BITS0 + type], m->C.bits);
    return read_row(m, "nfc_multi_read_packet_bits", m->A.O.bits[type], m->C.s_bits, 1, stream, stored, first, out, cap, n_out);
}

int nfc_multi_get_state(nfc_multi *m, uint32_t stream, nfc_state_header *h, float *ring, size_t ring_cap, uint8_t *pending, size_t pending_cap) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (!h) return mfail(m, NFC_ERR_ARG, "null header");
    if (int rc = check_stream(m, stream, false)) return rc;
    if (int rc = state_io(m, stream, 0)) return rc;
    MCHK(m, hipMemcpyAsync(m->h_blob.p, m->d_blob, m->blob_bytes, hipMemcpyDeviceToHost, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    const IoHeader *io = m->h_blob.as<const IoHeader>();
    memset(h, 0, sizeof *h);
    h->n_seen = m->nseen[stream];
    h->ss = io->ss;
    h->last_low = -1;
    h->filled = io->filled;
    h->stable = io->filled >= m->L;
    h->cur_state = (int32_t)(io->edge & 3u);
    h->last_bit = (int32_t)((io->edge >> 2) & 3u) - 1;
    h->dur = (int32_t)(io->edge >> 4);
    h->miller_state = m->canon[io->dec & 15u];
    h->manch_state = (int32_t)((io->dec >> 4) & 7u);
    h->pkt_started[0] = (int32_t)((io->dec >> 8) & 1u);
    h->pkt_started[1] = (int32_t)((io->dec >> 9) & 1u);
    h->n_pending_bits[0] = io->npend[0];
    h->n_pending_bits[1] = io->npend[1];
    h->av_window = m->L;
    const size_t p0 = io->npend[0], p1 = io->npend[1];
    if (ring && ring_cap < (size_t)m->L) return mfail(m, NFC_ERR_ARG, "ring buffer too small");
    if (pending && pending_cap < p0 + p1) return mfail(m, NFC_ERR_ARG, "pending-bit buffer too small");
    if (pending && (p0 > m->C.pending || p1 > m->C.pending))
        return mfail(m, NFC_ERR_STATE, "stream %u: an open packet outgrew cap_pending_bits (NFC_MULTI_PENDING_OVERFLOW): reset the stream", stream);
    const uint8_t *b = m->h_blob.as<uint8_t>() + sizeof(IoHeader);
    if (ring) memcpy(ring, b, (size_t)m->L * 4);
    b += (size_t)m->L * 4;
    if (pending && p0) memcpy(pending, b, p0);
    if (pending && p1) memcpy(pending + p0, b + m->C.pending, p1);
    return NFC_OK;
}

int nfc_multi_set_state(nfc_multi *m, uint32_t stream, const nfc_state_header *h, const float *ring, size_t ring_len, const uint8_t *pending,
                        size_t pending_len) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (!h || !ring) return mfail(m, NFC_ERR_ARG, "null header / ring");
    if (int rc = check_stream(m, stream, false)) return rc;
    if (h->av_window != m->L || ring_len != (size_t)m->L) return mfail(m, NFC_ERR_ARG, "state was taken with another av_window");
    if (h->dur < 0 || h->dur > m->mx || h->last_bit < -1 || h->last_bit > 1 || h->cur_state < 0 || h->cur_state > 2)
        return mfail(m, NFC_ERR_ARG, "edge-timing state out of range (dur %d, last_bit %d, cur_state %d)", h->dur, h->last_bit, h->cur_state);
    if (h->filled < 0 || h->filled > m->L || (h->stable != 0) != (h->filled == m->L)) return mfail(m, NFC_ERR_ARG, "filled / stable out of range");
    if (h->miller_state < 0 || h->miller_state > 15 || h->manch_state < 0 || h->manch_state > 7) return mfail(m, NFC_ERR_ARG, "decoder state out of range");
    const size_t p0 = h->n_pending_bits[0], p1 = h->n_pending_bits[1];
    if (p0 + p1 != pending_len || ((p0 + p1) && !pending)) return mfail(m, NFC_ERR_ARG, "pending bits do not match the header");
    if (p0 > m->C.pending || p1 > m->C.pending) return mfail(m, NFC_ERR_ARG, "pending bits exceed cap_pending_bits = %u", m->C.pending);
    MCHK(m, hipStreamSynchronize(m->st));
    memset(m->h_blob.p, 0, m->blob_bytes);
    IoHeader *io = m->h_blob.as<IoHeader>();
    io->ss = h->ss;
    io->filled = h->filled;
    // (the slot of the first stable sample while the window fills; of the next sample afterwards)
    io->slot = (uint32_t)((h->n_seen - (h->stable ? 0u : (uint64_t)h->filled)) % (uint64_t)m->L);
    io->edge = pack_edge(h->cur_state, h->last_bit, h->dur);
    io->dec = pack_dec(m->canon[h->miller_state], h->manch_state, h->pkt_started[0] != 0, h->pkt_started[1] != 0);
    io->npend[0] = (uint32_t)p0;
    io->npend[1] = (uint32_t)p1;
    io->flags = 0;
    uint8_t *b = m->h_blob.as<uint8_t>() + sizeof(IoHeader);
    memcpy(b, ring, (size_t)m->L * 4);
    b += (size_t)m->L * 4;
    if (p0) memcpy(b, pending, p0);
    if (p1) memcpy(b + m->C.pending, pending + p0, p1);
    MCHK(m, hipMemcpyAsync(m->d_blob, m->h_blob.p, m->blob_bytes, hipMemcpyHostToDevice, m->st));
    if (int rc = state_io(m, stream, 1)) return rc;
    // the stream's outputs of the last push are void: its counts go to 0 on the device as in the mirror (a later fetch scans them)
    m->fetched = 0;
    m->cmd_state = nfc_multi::CMD_NONE;   // (the commands of the last push go with its outputs; the machine itself is not touched)
    m->cmd_fetched = false;
    MCHK(m, hipMemsetAsync(m->A.O.counts + (size_t)stream * CNT_WORDS, 0, CNT_WORDS * 4, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    m->nseen[stream] = h->n_seen;
    m->g0[stream] = h->n_seen;
    m->last_n[stream] = 0;
    memset(m->h_counts.as<uint32_t>() + (size_t)stream * CNT_WORDS, 0, CNT_WORDS * 4);
    return NFC_OK;
}

int nfc_multi_reset(nfc_multi *m, int64_t stream) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    uint32_t k0, k1;
    if (int rc = stream_range(m, stream, k0, k1)) return rc;
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    m->fetched = 0;
    const size_t work = (size_t)(k1 - k0) * (size_t)m->L;
    NFC_LAUNCH(k_multi_reset, dim3((unsigned)std::min<size_t>(1024, (work + 255) / 256)), dim3(256), 0, m->st, m->A.S, m->K, k0, k1, m->L, m->A.O.counts);
    if (m->d_fsm.p) commands::launch_init(m->d_fsm.as<uint32_t>(), m->K, k0, k1, m->st);   // the machines too, keys included, as nfc_fsm_reset
    if (m->d_keys.p) commands::launch_set_table(m->d_keys.as<uint32_t>(), m->K, k0, k1, nullptr, m->st);   // ... and their sector keys
    if (m->d_emu.p)   // ... and the emulators: nfc_emu_state_init's state (the cards stay)
        if (int rc = emu_state_init_range(m, k0, k1)) return rc;
    if (m->txpend.d.p) MCHK(m, hipMemsetAsync(m->txpend.d.as<nfc_tx_pending>() + k0, 0, (size_t)(k1 - k0) * sizeof(nfc_tx_pending), m->st));   // ... and what they were still to transmit
    if (m->img.d.p)   // ... and their memory images, tails included
        if (int rc = images_init_range(m, k0, k1, false)) return rc;
    m->cmd_state = nfc_multi::CMD_NONE;
    m->cmd_fetched = false;
    if (int rc = launch_ok(m)) return rc;
    MCHK(m, hipStreamSynchronize(m->st));
    for (uint32_t k = k0; k < k1; k++) {
        m->nseen[k] = m->g0[k] = 0;
        m->last_n[k] = 0;
        memset(m->h_counts.as<uint32_t>() + (size_t)k * CNT_WORDS, 0, CNT_WORDS * 4);
    }
    if (stream < 0) m->have_outputs = false;
    return NFC_OK;
}

// ---- commands (multi_commands.hip.h) ----
int nfc_multi_track_commands(nfc_multi *m, int on) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (on) {
        if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
        if (int rc = ensure_fsm(m, "nfc_multi_track_commands")) return rc;
    }
    m->track = on != 0;
    return NFC_OK;
}

int nfc_multi_set_keys(nfc_multi *m, int64_t stream, const uint8_t key_a[6], const uint8_t key_b[6]) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    uint32_t k0, k1;
    if (int rc = stream_range(m, stream, k0, k1)) return rc;
    if (!key_a) return mfail(m, NFC_ERR_ARG, "key_a is null");
    if (!key_b) return mfail(m, NFC_ERR_ARG, "key_b is null");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_fsm(m, "nfc_multi_set_keys")) return rc;
    commands::launch_set_keys(m->d_fsm.as<uint32_t>(), m->K, k0, k1, fsmd::key_of(key_a), fsmd::key_of(key_b), m->st);
    return launch_ok(m);
}

// the tables' buffer, zeroed, and the blobs, at the first nfc_multi_set_sector_keys of a context
static int ensure_keys(nfc_multi *m, const char *fn) {
    if (m->d_keys.p) return NFC_OK;
    const size_t blob = (size_t)skeys::WORDS * 4, bytes = blob * m->K;
    if (grow(m, m->d_keys_blob, blob, fn, false) < 0 || grow(m, m->h_keys_blob, blob, fn, false) < 0) return NFC_ERR_NOMEM;
    DevBuf fresh;
    if (fresh.ensure(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return mfail(m, NFC_ERR_NOMEM, "%s: no device memory for %zu bytes", fn, bytes);
    }
    MCHK(m, hipMemsetAsync(fresh.p, 0, fresh.cap, m->st));
    std::swap(m->d_keys, fresh);   // (only a zeroed buffer is ever the context's)
    return NFC_OK;
}

int nfc_multi_set_sector_keys(nfc_multi *m, int64_t stream, const nfc_fsm_key_table *table) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    uint32_t k0, k1;
    if (int rc = stream_range(m, stream, k0, k1)) return rc;
    if (!table) return mfail(m, NFC_ERR_ARG, "table is null");
    if (const char *bad = skeys::table_fault(*table)) return mfail(m, NFC_ERR_ARG, "table: %s", bad);
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_keys(m, "nfc_multi_set_sector_keys")) return rc;
    MCHK(m, hipStreamSynchronize(m->st));   // (the blob may still be on its way from an earlier call)
    uint32_t *w = m->h_keys_blob.as<uint32_t>();
    const skeys::HostTable T = {table};
    for (uint32_t slot = 0; slot < skeys::SLOTS; slot++) {
        uint64_t key = 0;
        const bool have = T.get(slot, key);
        w[2 * slot] = have ? skeys::word_lo(key) : 0u;
        w[2 * slot + 1] = skeys::word_hi(key, have);
    }
    MCHK(m, hipMemcpyAsync(m->d_keys_blob.p, m->h_keys_blob.p, skeys::WORDS * 4, hipMemcpyHostToDevice, m->st));
    commands::launch_set_table(m->d_keys.as<uint32_t>(), m->K, k0, k1, m->d_keys_blob.as<uint32_t>(), m->st);
    if (int rc = launch_ok(m)) return rc;
    MCHK(m, hipStreamSynchronize(m->st));
    return NFC_OK;
}

int nfc_multi_get_sector_keys(nfc_multi *m, uint32_t stream, nfc_fsm_key_table *table) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!table) return mfail(m, NFC_ERR_ARG, "table is null");
    memset(table, 0, sizeof *table);
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (!m->d_keys.p) {   // no sector key was ever set: every table is empty and nothing is allocated for the question
        MCHK(m, hipStreamSynchronize(m->st));
        return NFC_OK;
    }
    commands::launch_table_io(m->d_keys.as<uint32_t>(), m->K, stream, 0, m->d_keys_blob.as<uint32_t>(), m->st);
    if (int rc = launch_ok(m)) return rc;
    MCHK(m, hipMemcpyAsync(m->h_keys_blob.p, m->d_keys_blob.p, skeys::WORDS * 4, hipMemcpyDeviceToHost, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    const uint32_t *w = m->h_keys_blob.as<uint32_t>();
    for (uint32_t slot = 0; slot < skeys::SLOTS; slot++) {
        if (!(w[2 * slot + 1] & skeys::PRESENT)) continue;
        const uint32_t type = slot / skeys::SECTORS, sec = slot % skeys::SECTORS;
        const uint64_t key = (uint64_t)w[2 * slot] | (uint64_t)(w[2 * slot + 1] & 0xFFFFu) << 32;
        table->present[type][sec] = 1;
        for (int i = 0; i < 6; i++) table->key[type][sec][i] = (uint8_t)(key >> (8 * i));
    }
    return NFC_OK;
}

int nfc_multi_get_fsm_state(nfc_multi *m, uint32_t stream, nfc_fsm_state *st) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!st) return mfail(m, NFC_ERR_ARG, "st is null");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_fsm(m, "nfc_multi_get_fsm_state")) return rc;
    commands::launch_io(m->d_fsm.as<uint32_t>(), m->K, stream, 0, m->d_fsm_blob.as<uint32_t>(), m->st);
    if (int rc = launch_ok(m)) return rc;
    MCHK(m, hipMemcpyAsync(m->h_fsm_blob.p, m->d_fsm_blob.p, fsmd::W_WORDS * 4, hipMemcpyDeviceToHost, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    fsmd::Machine M;
    fsmd::load_machine(M, m->h_fsm_blob.as<uint32_t>(), 1, 0);
    memset(st, 0, sizeof *st);
    fsmd::machine_to_state(M, *st);
    return NFC_OK;
}

int nfc_multi_set_fsm_state(nfc_multi *m, uint32_t stream, const nfc_fsm_state *st) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!st) return mfail(m, NFC_ERR_ARG, "st is null");
    if (const char *bad = fsmd::state_fault(*st)) return mfail(m, NFC_ERR_ARG, "st: %s", bad);
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_fsm(m, "nfc_multi_set_fsm_state")) return rc;
    MCHK(m, hipStreamSynchronize(m->st));   // (the blob may still be on its way from an earlier call)
    fsmd::Machine M;
    fsmd::machine_from_state(M, *st);
    fsmd::store_machine(M, m->h_fsm_blob.as<uint32_t>(), 1, 0);
    MCHK(m, hipMemcpyAsync(m->d_fsm_blob.p, m->h_fsm_blob.p, fsmd::W_WORDS * 4, hipMemcpyHostToDevice, m->st));
    commands::launch_io(m->d_fsm.as<uint32_t>(), m->K, stream, 1, m->d_fsm_blob.as<uint32_t>(), m->st);
    if (int rc = launch_ok(m)) return rc;
    MCHK(m, hipStreamSynchronize(m->st));
    m->cmd_fetched = false;   // (the pointers of a fetch end here; the last push's commands stay fetchable)
    return NFC_OK;
}

// One copy of the tracked push's buffer -- the frames' part and the commands' sections -- to pinned memory, one wait.  The pinned copy is
// followed by base[K].  With nothing stored there is no buffer: the tables are zeroed on the host and the machines' flags come from their words.
int nfc_multi_fetch_commands(nfc_multi *m, nfc_multi_commands *out) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (!m->have_outputs) return mfail(m, NFC_ERR_STATE, "no completed push");
    if (m->cmd_state == nfc_multi::CMD_NONE)
        return mfail(m, NFC_ERR_STATE, "command tracking was off at the last push (nfc_multi_track_commands), or a stream was reset or set since");
    if (m->cmd_fetched) {   // the same data: nothing is copied again and no machine is touched
        if (out) *out = m->cout;
        return NFC_OK;
    }
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    const uint32_t K = m->K;
    const size_t T = (size_t)K + 1;
    const bool stored = m->cmd_state == nfc_multi::CMD_LAUNCHED;
    // nothing stored: [64 bytes | table [4][T] | cmd_off [T] | cbyte_off [T] | flags [K]] on the host alone
    const size_t empty_tabs = up16(frames::MULTI_HEADER_BYTES + 4 * T * 8), empty_bytes = up16(empty_tabs + 2 * T * 8 + (size_t)K * 4);
    const size_t bytes = stored ? m->cmd_bytes : empty_bytes, host_bytes = bytes + (size_t)K * 8;
    if (grow(m, m->cmd.h, host_bytes, "nfc_multi_fetch_commands") < 0) return NFC_ERR_NOMEM;
    uint8_t *h = m->cmd.h.as<uint8_t>();
    uint64_t *base = (uint64_t *)(h + bytes);
    for (uint32_t k = 0; k < K; k++) base[k] = m->g0[k];
    nfc_multi_commands &c = m->cout;
    memset(&c, 0, sizeof c);
    c.n_streams = c.raw.n_streams = K;
    if (stored) {
        const commands::Layout &L = m->cmd_lay;
        MCHK(m, hipMemcpyAsync(h, m->cmd.d.p, bytes, hipMemcpyDeviceToHost, m->st));
        MCHK(m, hipStreamSynchronize(m->st));
        if (int rc = launch_ok(m)) return rc;
        const uint64_t *dev_total = (const uint64_t *)h;
        const uint64_t *cmd_off = (const uint64_t *)(h + L.at[commands::SEC_CMD_OFF]), *cbyte_off = (const uint64_t *)(h + L.at[commands::SEC_CBYTE_OFF]);
        if (int rc = check_frame_totals(m, "nfc_multi_fetch_commands", h, m->cmd_nfr, m->cmd_room)) return rc;
        if (cmd_off[K] != L.total_cmds || cbyte_off[K] != dev_total[2] + dev_total[3])
            return mfail(m, NFC_ERR_INTERNAL, "nfc_multi_fetch_commands: the device counts %llu commands over %llu bytes, the host %llu commands, the frames %llu bytes",
                         (unsigned long long)cmd_off[K], (unsigned long long)cbyte_off[K], (unsigned long long)L.total_cmds, (unsigned long long)(dev_total[2] + dev_total[3]));
        if (m->cmd_timed) {
            float ms = 0.f;
            MCHK(m, hipEventElapsedTime(&ms, m->evc[0], m->evc[3]));
            c.ms_kernels = ms;
            MCHK(m, hipEventElapsedTime(&ms, m->evc[2], m->evc[3]));
            c.ms_machine = ms;
        }
        c.n_launches = 3;
        c.bytes_copied = bytes;
        c.cmd_off = cmd_off;
        c.cbyte_off = cbyte_off;
        c.stream_flags = (const uint32_t *)(h + L.at[commands::SEC_FLAGS]);
        c.cmd = (const nfc_frame *)(h + L.at[commands::SEC_CMD]);
        c.src = (const uint32_t *)(h + L.at[commands::SEC_SRC]);
        c.data = h + L.at[commands::SEC_DATA];
        c.enc = (const uint16_t *)(h + L.at[commands::SEC_ENC]);
    } else {
        memset(h, 0, empty_bytes);
        uint32_t *flags = (uint32_t *)(h + empty_tabs + 2 * T * 8);
        MCHK(m, hipMemcpyAsync(flags, m->d_fsm.as<uint32_t>() + (size_t)fsmd::W_FLAGS * K, (size_t)K * 4, hipMemcpyDeviceToHost, m->st));
        MCHK(m, hipStreamSynchronize(m->st));
        c.bytes_copied = (size_t)K * 4;
        c.cmd_off = (const uint64_t *)(h + empty_tabs);
        c.cbyte_off = c.cmd_off + T;
        c.stream_flags = flags;
    }
    frames_view(m, h, m->cmd_frlay, base, stored, c.raw);
    m->cmd_fetched = true;
    if (out) *out = c;
    return NFC_OK;
}

// ---- the memory images (image.hip.h) ----
int nfc_multi_track_images(nfc_multi *m, int on) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (on) {
        if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
        if (int rc = ensure_fsm(m, "nfc_multi_track_images")) return rc;
        if (int rc = ensure_images(m, "nfc_multi_track_images")) return rc;
        m->track = true;   // images are made of commands
    }
    m->track_img = on != 0;
    return NFC_OK;
}

// One copy of the images' buffer to pinned memory, one wait.
int nfc_multi_fetch_images(nfc_multi *m, nfc_multi_images *out) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (!m->img.d.p) return mfail(m, NFC_ERR_STATE, "the memory images were never switched on (nfc_multi_track_images)");
    if (m->img_fetched) {   // the same data: no device call
        if (out) *out = m->iout;
        return NFC_OK;
    }
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (grow(m, m->img.h, m->img_bytes, "nfc_multi_fetch_images", false) < 0) return NFC_ERR_NOMEM;
    uint8_t *h = m->img.h.as<uint8_t>();
    MCHK(m, hipMemcpyAsync(h, m->img.d.p, m->img_bytes, hipMemcpyDeviceToHost, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    if (int rc = launch_ok(m)) return rc;
    nfc_multi_images &o = m->iout;
    memset(&o, 0, sizeof o);
    o.mem = h + m->img_at[image::ISEC_MEM];
    o.src = h + m->img_at[image::ISEC_SRC];
    o.info = (const nfc_image_info *)(h + m->img_at[image::ISEC_INFO]);
    o.tail = (const nfc_image_cmd *)(h + m->img_at[image::ISEC_TAIL]);
    o.n_streams = m->K;
    o.n_launches = m->img_launches;
    o.bytes_copied = m->img_bytes;
    if (m->img_launches && m->img_timed) {
        float ms = 0.f;
        MCHK(m, hipEventElapsedTime(&ms, m->evi[0], m->evi[1]));
        o.ms_kernel = ms;
    }
    m->img_fetched = true;
    if (out) *out = o;
    return NFC_OK;
}

int nfc_multi_get_image(nfc_multi *m, uint32_t stream, nfc_card_image *image) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!image) return mfail(m, NFC_ERR_ARG, "image is null");
    if (!m->img.d.p) return mfail(m, NFC_ERR_STATE, "the memory images were never switched on (nfc_multi_track_images)");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = image_io(m, stream, false)) return rc;
    if (int rc = launch_ok(m)) return rc;
    memcpy(image, m->h_img_one.p, sizeof *image);
    return NFC_OK;
}

int nfc_multi_set_image(nfc_multi *m, uint32_t stream, const nfc_card_image *image) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!image) return mfail(m, NFC_ERR_ARG, "image is null");
    if (const char *bad = image::image_fault(*image)) return mfail(m, NFC_ERR_ARG, "image: %s", bad);
    if (!m->img.d.p) return mfail(m, NFC_ERR_STATE, "the memory images were never switched on (nfc_multi_track_images)");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    MCHK(m, hipStreamSynchronize(m->st));   // (the staging may still be on its way from an earlier call)
    memcpy(m->h_img_one.p, image, sizeof *image);
    m->img_fetched = false;
    return image_io(m, stream, true);
}

// ---- emulation: a stream that answers (multi_commands.hip.h: k_multi_commands_emu) ----
int nfc_multi_emulate(nfc_multi *m, int64_t stream, const nfc_emu_card *card) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    uint32_t k0, k1;
    if (int rc = stream_range(m, stream, k0, k1)) return rc;
    if (card) {
        if (card->role != NFC_EMU_TAG && card->role != NFC_EMU_READER) return mfail(m, NFC_ERR_ARG, "card.role must be NFC_EMU_TAG or NFC_EMU_READER");
        if (const char *bad = emu::card_fault(*card, card->role)) return mfail(m, NFC_ERR_ARG, "card%s", bad);
    }
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (!card && !m->d_emu.p) return NFC_OK;   // nothing to take away, and nothing is allocated for it
    if (int rc = ensure_fsm(m, "nfc_multi_emulate")) return rc;
    if (int rc = ensure_emu(m, "nfc_multi_emulate")) return rc;
    MCHK(m, hipStreamSynchronize(m->st));
    // one stream's column of each array, as the host builds it: 64 units of memory, 64 nonces, the parameters
    std::vector<uint32_t> mem(emu::CLASSIC_BYTES / 4, 0), rands(emu::MAX_RANDS, 0), par(commands::EP_WORDS, 0);
    if (card) {
        const emu::HostCard H = {card->mem, card->rands, card->n_rands, card->role == NFC_EMU_TAG ? card->tag_type : -1, card->mode};
        if (card->role == NFC_EMU_TAG)
            for (uint32_t i = 0; i < card->mem_len / 4; i++) mem[i] = H.mem_word(i);
        for (uint32_t i = 0; i < card->n_rands; i++) rands[i] = H.rand(i);
        par[commands::EP_PRESENT] = 1, par[commands::EP_ROLE] = (uint32_t)card->role, par[commands::EP_TAG_TYPE] = (uint32_t)H.tag_type;
        par[commands::EP_MODE] = (uint32_t)card->mode, par[commands::EP_N_RANDS] = card->n_rands;
    }
    uint8_t *e = m->d_emu.as<uint8_t>();
    const size_t K = m->K;
    for (uint32_t k = k0; k < k1; k++) {
        MCHK(m, hipMemcpy2DAsync(e + m->emu_mem + (size_t)k * 16, K * 16, mem.data(), 16, 16, emu::CLASSIC_BYTES / 16, hipMemcpyHostToDevice, m->st));
        MCHK(m, hipMemcpy2DAsync(e + m->emu_rands + (size_t)k * 4, K * 4, rands.data(), 4, 4, emu::MAX_RANDS, hipMemcpyHostToDevice, m->st));
        MCHK(m, hipMemcpy2DAsync(e + m->emu_params + (size_t)k * 4, K * 4, par.data(), 4, 4, commands::EP_WORDS, hipMemcpyHostToDevice, m->st));
        m->n_cards += (card ? 1u : 0u) - (uint32_t)m->has_card[k];
        m->has_card[k] = card ? 1 : 0;
        m->card_role[k] = card ? (int8_t)card->role : (int8_t)-1;
    }
    if (m->txpend.d.p) MCHK(m, hipMemsetAsync(m->txpend.d.as<nfc_tx_pending>() + k0, 0, (size_t)(k1 - k0) * sizeof(nfc_tx_pending), m->st));   // (a new card has nothing pending)
    MCHK(m, hipStreamSynchronize(m->st));   // (the sources are this call's)
    if (int rc = emu_state_init_range(m, k0, k1)) return rc;   // a new card starts from the initial state
    if (card) m->track = true;   // answering implies tracking
    return NFC_OK;
}

static int emu_state_io(nfc_multi *m, uint32_t stream, int set, uint32_t *words) {
    uint32_t *state = (uint32_t *)(m->d_emu.as<uint8_t>() + m->emu_state) + stream;
    if (set) MCHK(m, hipMemcpy2DAsync(state, (size_t)m->K * 4, words, 4, 4, emu::EW_WORDS, hipMemcpyHostToDevice, m->st));
    else MCHK(m, hipMemcpy2DAsync(words, 4, state, (size_t)m->K * 4, 4, emu::EW_WORDS, hipMemcpyDeviceToHost, m->st));
    MCHK(m, hipStreamSynchronize(m->st));
    return NFC_OK;
}

int nfc_multi_get_emu_state(nfc_multi *m, uint32_t stream, nfc_emu_state *st) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!st) return mfail(m, NFC_ERR_ARG, "st is null");
    emu::State S;
    emu::state_init(S);
    if (m->d_emu.p) {
        if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
        uint32_t words[emu::EW_WORDS];
        if (int rc = emu_state_io(m, stream, 0, words)) return rc;
        emu::load_state(S, words, 1, 0);
    }
    memset(st, 0, sizeof *st);
    emu::state_to_public(S, *st);
    return NFC_OK;
}

int nfc_multi_set_emu_state(nfc_multi *m, uint32_t stream, const nfc_emu_state *st) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!st) return mfail(m, NFC_ERR_ARG, "st is null");
    if (const char *bad = emu::state_fault(*st)) return mfail(m, NFC_ERR_ARG, "st: %s", bad);
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_fsm(m, "nfc_multi_set_emu_state")) return rc;
    if (int rc = ensure_emu(m, "nfc_multi_set_emu_state")) return rc;
    emu::State S;
    emu::state_from_public(S, *st);
    uint32_t words[emu::EW_WORDS];
    emu::store_state(S, words, 1, 0);
    return emu_state_io(m, stream, 1, words);
}

// The answers of the last push: sections of the buffer nfc_multi_fetch_commands copies -- the SAME single copy; when the commands were
// fetched since the push, no device call at all.
int nfc_multi_fetch_answers(nfc_multi *m, nfc_multi_answers *out) {
    if (!m) return NFC_ERR_ARG;
    if (!out) return mfail(m, NFC_ERR_ARG, "out is null");
    nfc_multi_commands c;
    if (int rc = nfc_multi_fetch_commands(m, &c)) return rc;
    nfc_multi_answers &a = m->aout;
    memset(&a, 0, sizeof a);
    a.n_streams = m->K;
    a.cmd_off = c.cmd_off;
    if (m->cmd_state == nfc_multi::CMD_LAUNCHED && m->cmd_emulated) {
        const uint8_t *h = m->cmd.h.as<uint8_t>();
        const commands::EmuArgs &E = m->cmd_emu;
        a.emulated = 1;
        a.ans_n = (const uint32_t *)(h + E.at[commands::ESEC_N]);
        a.ans = (const nfc_emu_answer *)(h + E.at[commands::ESEC_REC]);
        a.plain = h + E.at[commands::ESEC_PLAIN], a.air = h + E.at[commands::ESEC_AIR], a.par = h + E.at[commands::ESEC_PAR];
        for (uint32_t k = 0; k < m->K; k++) {
            if ((uint64_t)a.ans_n[k] > c.cmd_off[k + 1] - c.cmd_off[k])
                return mfail(m, NFC_ERR_INTERNAL, "nfc_multi_fetch_answers: stream %u has %u answers to %llu commands", k, a.ans_n[k],
                             (unsigned long long)(c.cmd_off[k + 1] - c.cmd_off[k]));
            a.n_answers += a.ans_n[k];
        }
    }
    *out = a;
    return NFC_OK;
}

// ---- transmission: the answers of the last push as TX samples (answers_tx.hip.h) ----
// the pending entries, zeroed (no stream has one), with their guard: at the first call that needs them
static int ensure_txpend(nfc_multi *m, const char *fn) {
    if (m->txpend.d.p) return NFC_OK;
    const size_t bytes = (size_t)m->K * sizeof(nfc_tx_pending);
    DevBuf fresh;
    if (fresh.ensure(bytes + GUARD_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        return mfail(m, NFC_ERR_NOMEM, "%s: no device memory for %zu bytes", fn, bytes + GUARD_BYTES);
    }
    MCHK(m, hipMemsetAsync(fresh.p, 0, bytes, m->st));
    MCHK(m, hipMemsetD32Async((hipDeviceptr_t)(fresh.as<uint8_t>() + bytes), (int)GUARD_WORD, GUARD_BYTES / 4, m->st));
    std::swap(m->txpend.d, fresh);
    m->txpend.guards.assign(1, bytes);
    return NFC_OK;
}

static const char *tx_pending_fault(const nfc_tx_pending &p) {
    if (p.n_bits && !atx::n_bits_ok(p.n_bits)) return "n_bits is neither 0, 1 .. 8 nor a multiple of 9 up to 162";
    if (p.role > 1) return "role is neither NFC_EMU_TAG nor NFC_EMU_READER";
    if (p.reserved0 || p.reserved1) return "reserved must be 0";
    for (int i = 0; i < 12; i++)
        if (p.reserved2[i]) return "reserved must be 0";
    return nullptr;
}

int nfc_multi_get_tx_state(nfc_multi *m, uint32_t stream, nfc_tx_pending *st) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!st) return mfail(m, NFC_ERR_ARG, "st is null");
    memset(st, 0, sizeof *st);
    if (!m->txpend.d.p) return NFC_OK;   // nothing was ever transmitted or set: no stream has a pending entry
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    MCHK(m, hipStreamSynchronize(m->st));
    if (int rc = launch_ok(m)) return rc;
    MCHK(m, hipMemcpy(st, m->txpend.d.as<nfc_tx_pending>() + stream, sizeof *st, hipMemcpyDeviceToHost));
    return NFC_OK;
}

int nfc_multi_set_tx_state(nfc_multi *m, uint32_t stream, const nfc_tx_pending *st) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    if (stream >= m->K) return mfail(m, NFC_ERR_ARG, "stream %u out of range (n_streams %u)", stream, m->K);
    if (!st) return mfail(m, NFC_ERR_ARG, "st is null");
    if (const char *bad = tx_pending_fault(*st)) return mfail(m, NFC_ERR_ARG, "st: %s", bad);
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_txpend(m, "nfc_multi_set_tx_state")) return rc;
    nfc_tx_pending p;
    memset(&p, 0, sizeof p);
    if (st->n_bits) {   // (canonical: zero behind the answer's bytes, every byte zero without one)
        const uint32_t nb = air::frame_bytes(st->n_bits);
        p.start = st->start, p.n_bits = st->n_bits, p.role = st->role;
        memcpy(p.air, st->air, nb);
        memcpy(p.par, st->par, nb);
    }
    MCHK(m, hipStreamSynchronize(m->st));
    MCHK(m, hipMemcpy(m->txpend.d.as<nfc_tx_pending>() + stream, &p, sizeof p, hipMemcpyHostToDevice));
    return NFC_OK;
}

int nfc_multi_transmit_device(nfc_multi *m, const nfc_answers_tx_config *cfg, void *dev_out, size_t cap_samples, uint64_t *first_sample,
                              uint32_t *n_samples, float *kernel_ms) {
    if (!m) return NFC_ERR_ARG;
    LaunchScope scope(&m->launch_err);
    char msg[256];
    if (atx::config_fault(cfg, msg, sizeof msg)) return mfail(m, NFC_ERR_ARG, "%s", msg);
    if (!first_sample || !n_samples) return mfail(m, NFC_ERR_ARG, "first_sample or n_samples is null");
    if ((uintptr_t)dev_out & 31u) return mfail(m, NFC_ERR_ARG, "dev_out must be 32-byte aligned");
    if (!m->have_outputs) return mfail(m, NFC_ERR_STATE, "no completed push");
    if (!m->track || m->cmd_state == nfc_multi::CMD_NONE)
        return mfail(m, NFC_ERR_STATE, "command tracking was off at the last push (nfc_multi_track_commands), or a stream was reset or set since");
    if (m->n_cards == 0) return mfail(m, NFC_ERR_STATE, "no stream holds a card (nfc_multi_emulate)");
    if (m->tx_done) return mfail(m, NFC_ERR_STATE, "the last push was transmitted already: once per push");
    const uint32_t K = m->K;
    const atx::Consts C = atx::make_consts(*cfg);
    // the layout, from the push's own arguments
    const bool have_answers = m->cmd_state == nfc_multi::CMD_LAUNCHED && m->cmd_emulated;
    std::vector<atx::StreamIn> streams((size_t)K + 1);
    uint64_t at = 0, need = 0, n_span = 0;
    for (uint32_t k = 0; k < K; k++) {
        atx::StreamIn &S = streams[k];
        memset(&S, 0, sizeof S);
        S.role = m->has_card[k] ? (int32_t)m->card_role[k] : -1;
        S.rx_base = m->g0[k], S.rx_n = m->last_n[k];
        S.t0 = atx::tx_index(C, S.rx_base);
        const uint64_t n = S.role < 0 ? 0ull : atx::tx_index(C, S.rx_base + S.rx_n) - S.t0;
        if (n > atx::MAX_SPAN) return mfail(m, NFC_ERR_ARG, "stream %u: a span of %llu samples exceeds 2^30", k, (unsigned long long)n);
        S.first_sample = first_sample[k] = at;
        S.n_samples = n_samples[k] = (uint32_t)n;
        need = at + n;
        at += air::align_up(n, C.align);
        // room in the span table: an answer per command at the most, and the entry carried in
        uint64_t ncmd = 0;
        if (have_answers && S.role >= 0) {
            const uint32_t *c = m->h_counts.as<uint32_t>() + (size_t)k * CNT_WORDS;
            for (int t = 0; t < 2; t++) ncmd += std::min(c[CNT_PK0 + t], m->C.packets);
        }
        S.span_off = (uint32_t)n_span;
        S.span_cap = S.role < 0 ? 0u : (uint32_t)ncmd + 1u;
        n_span += S.span_cap;
    }
    memset(&streams[K], 0, sizeof(atx::StreamIn));
    streams[K].first_sample = need, streams[K].role = -1, streams[K].span_off = (uint32_t)n_span;
    if (need > cap_samples) return mfail(m, NFC_ERR_ARG, "cap_samples: the layout needs %llu samples, %zu do not hold them", (unsigned long long)need, cap_samples);
    if (need && !dev_out) return mfail(m, NFC_ERR_ARG, "dev_out is null");
    if (n_span > 0xFFFFFFFFull) return mfail(m, NFC_ERR_ARG, "more than 2^32 span records");
    if (hipSetDevice(m->P.device) != hipSuccess) return mfail(m, NFC_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_txpend(m, "nfc_multi_transmit_device")) return rc;
    // the call's sections: streams [K + 1] | tile_stream [n_tiles] | spans | n_spans [K]
    const uint64_t n_tiles = (need + atx::TILE - 1) / atx::TILE;
    if (n_tiles > 0x7FFFFFFFull) return mfail(m, NFC_ERR_ARG, "cap_samples: more than 2^31 tiles");
    Sections S{0, {}};
    uint64_t o_streams, o_tiles, o_spans, o_ns, e_streams, e_tiles, e_spans, e_ns;
    S.place(o_streams, e_streams, ((size_t)K + 1) * sizeof(atx::StreamIn));
    S.place(o_tiles, e_tiles, (size_t)n_tiles * 4);
    S.place(o_spans, e_spans, (size_t)n_span * sizeof(atx::Span));
    S.place(o_ns, e_ns, (size_t)K * 4);
    if (int rc = grow_packed(m, m->tx, S.at, "nfc_multi_transmit_device")) return rc;
    const size_t up_bytes = (size_t)o_spans;   // the two sections the host makes, guards and all
    if (grow(m, m->h_tx, up_bytes, "nfc_multi_transmit_device") < 0) return NFC_ERR_NOMEM;
    if (kernel_ms)
        for (Event &e : m->evt)
            if (!e && e.create() != hipSuccess) {
                (void)hipGetLastError();
                return mfail(m, NFC_ERR_DEVICE, "hipEventCreate failed");
            }
    uint8_t *h = m->h_tx.as<uint8_t>(), *d = m->tx.d.as<uint8_t>();
    memset(h, 0, up_bytes);
    memcpy(h + o_streams, streams.data(), ((size_t)K + 1) * sizeof(atx::StreamIn));
    {   // per tile the first stream whose part of the buffer, the padding behind it included, reaches into the tile
        uint32_t *tile = (uint32_t *)(h + o_tiles);
        uint32_t k = 0;
        for (uint64_t t = 0; t < n_tiles; t++) {
            while (k + 1 < K && streams[k + 1].first_sample <= t * atx::TILE) k++;
            tile[t] = k;
        }
    }
    MCHK(m, hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, m->st));
    atx::ScheduleArgs SA;
    memset(&SA, 0, sizeof SA);
    SA.C = C;
    if (have_answers) {
        const commands::Layout &L = m->cmd_lay;
        const commands::EmuArgs &E = m->cmd_emu;
        const frames::MultiLayout &F = m->cmd_frlay;
        atx::Tracked &T = SA.T;
        T.buf = m->cmd.d.as<uint8_t>();
        T.table = (const uint64_t *)(T.buf + frames::MULTI_HEADER_BYTES);
        for (int t = 0; t < 2; t++) T.at_fr[t] = F.at_fr[t], T.total_frames[t] = F.total_frames[t];
        T.at_cmd_off = L.at[commands::SEC_CMD_OFF], T.at_src = L.at[commands::SEC_SRC], T.total_cmds = L.total_cmds;
        T.at_ans_n = E.at[commands::ESEC_N], T.at_ans = E.at[commands::ESEC_REC], T.at_air = E.at[commands::ESEC_AIR], T.at_par = E.at[commands::ESEC_PAR];
    }
    SA.streams = (const atx::StreamIn *)(d + o_streams);
    SA.spans = (atx::Span *)(d + o_spans);
    SA.n_spans = (uint32_t *)(d + o_ns);
    SA.pending = m->txpend.d.as<nfc_tx_pending>();
    SA.K = K;
    SA.packed = d;
    SA.guard_at[0] = e_streams, SA.guard_at[1] = e_tiles, SA.guard_at[2] = e_spans, SA.guard_at[3] = e_ns;
    SA.guard_word = GUARD_WORD, SA.guard_bytes = GUARD_BYTES;
    const bool timed = kernel_ms != nullptr;
    NFC_LAUNCH_EXT(atx::k_answers_tx_schedule, dim3((K + atx::SCHED_BLOCK - 1) / atx::SCHED_BLOCK), dim3(atx::SCHED_BLOCK), 0, m->st,
                   timed ? (hipEvent_t)m->evt[0] : nullptr, timed ? (hipEvent_t)m->evt[1] : nullptr, 0, SA);
    m->tx.guards = std::move(S.guards);
    uint32_t launches = 1;
    if (n_tiles) {
        atx::RenderArgs RA;
        memset(&RA, 0, sizeof RA);
        RA.C = C;
        RA.streams = SA.streams, RA.tile_stream = (const uint32_t *)(d + o_tiles), RA.spans = SA.spans, RA.n_spans = SA.n_spans;
        RA.K = K, RA.total = need, RA.out = (float2 *)dev_out;
        NFC_LAUNCH_EXT(atx::k_answers_tx_render, dim3((unsigned)n_tiles), dim3(atx::BLOCK), 0, m->st, timed ? (hipEvent_t)m->evt[2] : nullptr,
                       timed ? (hipEvent_t)m->evt[3] : nullptr, 0, RA);
        launches++;
    }
    if (int rc = launch_ok(m)) return rc;
    m->tx_done = true;
    m->stats.n_launches += launches;
    if (timed) {
        kernel_ms[0] = kernel_ms[1] = 0.f;
        MCHK(m, hipStreamSynchronize(m->st));
        MCHK(m, hipEventElapsedTime(&kernel_ms[0], m->evt[0], m->evt[1]));
        if (n_tiles) MCHK(m, hipEventElapsedTime(&kernel_ms[1], m->evt[2], m->evt[3]));
    }
    return NFC_OK;
}

int nfc_multi_get_stats(nfc_multi *m, nfc_multi_stats *out) {
    if (!m) return NFC_ERR_ARG;
    if (!out) return mfail(m, NFC_ERR_ARG, "null output");
    *out = m->stats;
    return NFC_OK;
}

int nfc_multi_set_timing(nfc_multi *m, int on) {
    if (!m) return NFC_ERR_ARG;
    m->timing = on != 0;
    return NFC_OK;
}

}  // extern "C"

#ifdef NFC_TEST_HOOKS
// Test support, in the test build only and not part of the C-ABI: the damaged bytes among the guards behind every stream's row of
// every slab (0: intact).
// the damaged bytes among the guards of a packed buffer's device side; -1: a copy failed
static int packed_guards_damaged(nfc_multi *m, const Packed &p) {
    std::vector<uint8_t> g(p.guards.size() * GUARD_BYTES);
    for (size_t s = 0; s < p.guards.size(); s++)
        if (hipMemcpyAsync(g.data() + s * GUARD_BYTES, p.d.as<uint8_t>() + p.guards[s], GUARD_BYTES, hipMemcpyDeviceToHost, m->st) != hipSuccess) return -1;
    if (hipStreamSynchronize(m->st) != hipSuccess) return -1;
    int bad = 0;
    for (size_t i = 0; i < g.size(); i++) bad += g[i] != (uint8_t)(GUARD_WORD >> (8 * ((i % GUARD_BYTES) & 3)));
    return bad;
}
extern "C" int nfc_debug_multi_guards(nfc_multi *m) {
    if (!m || hipSetDevice(m->P.device) != hipSuccess) return -1;
    LaunchScope scope(&m->launch_err);
    DevBuf bad_word;   // (a word of its own: the state blob stays the state calls')
    if (bad_word.ensure(16) != hipSuccess) return -1;
    uint32_t *const bad = bad_word.as<uint32_t>();
    if (hipMemsetAsync(bad, 0, 4, m->st) != hipSuccess) return -1;
    for (size_t i = 0; i < m->guards.size(); i++)
        NFC_LAUNCH(k_multi_guard_check, dim3(std::min<uint32_t>(1024, (m->K * 4 + 255) / 256)), dim3(256), 0, m->st, (const uint8_t *)m->guards[i].first,
                   m->guards[i].second, m->guard_row[i], m->K, bad);
    uint32_t h = 0;
    if (launch_ok(m) || hipMemcpyAsync(m->h_blob.p, bad, 4, hipMemcpyDeviceToHost, m->st) != hipSuccess || hipStreamSynchronize(m->st) != hipSuccess) return -1;
    memcpy(&h, m->h_blob.p, 4);
    // ... and the guards behind the sections of the three packed buffers, where the launches that last filled each left them
    for (const Packed *p : {&m->fetch, &m->frames, &m->cmd, &m->txpend, &m->tx, &m->img}) {
        const int bad_bytes = packed_guards_damaged(m, *p);
        if (bad_bytes < 0) return -1;
        h += (uint32_t)bad_bytes;
    }
    return (int)h;
}
#endif   // NFC_TEST_HOOKS
