// host_context.h -- the test build's switches (Switches, read_switches), the context (nfc_ctx), the mirrored state block, launch helpers
// (the threshold kernels' own launch: host_threshold.h, launch_threshold)
// (part of nfc_amd.hip: included there, in this order, into one translation unit)
// Who owns what: every HIP resource of a context -- device and pinned buffers, events, its two streams -- is a member of nfc_ctx of one of
// dev_buf.h's owning types, so `delete c` is the whole release (nfc_destroy waits for the streams first) and a context that nfc_create could
// not finish releases what it had got.  A buffer added to the struct needs no second mention anywhere.
#pragma once


namespace {

std::string g_create_error;

}  // namespace

// totals layout (device scalars inside DevState)
enum : int {
    TOT_RUNS = 0,       // u32
    TOT_EDGES = 8,      // u32
    TOT_DECMAP = 16,    // DecMaps (24 bytes)
    TOT_SPEC = 40,      // u32: verdict of the speculative decode's check (decode.hip.h: dec_verify), 0 = every assumption that mattered held
    TOT_PKT0 = 72,      // PktCnt: per type, bits | closes << 32
    TOT_PKT1 = 80,
    TOT_LAST2 = 88,     // Last2 (8 bytes)
    TOT_NSYM = 96,      // u32[2]: symbols per packet type
    TOT_CERT = 104,     // CertSummary (24 bytes)
    TOT_FRAME = 128,    // FrameAgg (32 bytes): symbol counts, framing maps, bit / close counts of the batch
    TOT_BYTES = 160
};

// Everything the host mirrors after a batch, in one block so that one copy fetches it.
static_assert(sizeof(CertSummary) <= TOT_FRAME - TOT_CERT, "the verdict summary fits its slot of the totals");
struct DevState {
    Carry carry;
    EdgeCarry ecarry;
    DecCarry dcarry;
    uint8_t totals[TOT_BYTES];
    uint32_t seq[4];   // seq[0]: the batch the block belongs to, stamped by the batch's window fill (k_fill, or fill_rider behind pass 0): a mirror that
                       // does not carry the current number was not written by this batch's kernels
};

// what the threshold kernel of a batch submitted ahead may hold of a CU's 160 KB of LDS: the later stages of the batch before it run
// beside it (the writer stages 12 KB per workgroup, the speculative decode 25 KB)
constexpr size_t AHEAD_LDS_MAX = 96 * 1024;
// The one-wave kernels walk steps of STEP samples -- four rows of 64: what kind_kernels.h instantiates (8-row steps measured slower: 126
// VGPRs, four waves per SIMD) --, and k_threshold_lean takes them four at a time (four steps ahead, 104 registers: nfc_amd.hip, create_plan_device).
constexpr int LEAN_STEPS_AHEAD = 4;
constexpr int NRING = 4;   // window buffers: the carried one + one per batch that may be in flight (they rotate)
constexpr int NSUB = 3;    // batches that may be submitted and not yet waited for

namespace {
// The PRODUCT build reads no environment variable: which kernels a deployed process runs does not depend on what it inherited.
// Every switch below -- the ones that make a context misbehave on purpose or talk, and the ones that select between kernel
// forms that are all exact (the A/Bs of DESIGN.md, the tests that keep the less travelled forms exact) -- exists in the TEST
// build only (-DNFC_TEST_HOOKS: usrp_nfc_amd/libnfc_amd_hooks.so, build.py), and is read here, once per nfc_create (NFC_REC_NT: per call of
// nfc_record_pcm16_device).  README.md lists them.  A value is unset or what the variable parsed to; nfc_create clamps and applies it.
struct Switches {
    std::optional<std::string> debug_clk;
    std::optional<int> no_small, debug_bad_launch, debug_redo_submitted, debug, trace, trace_alloc, no_submit_ahead, wg, wg_rounds, wg_bulk, wg_rerun, wg_rowbal, wg_nr, wg_per_cu, wg_per_cu_ahead, wg_ex, lean, lean_rounds,
        lean_waves, edge_prefix, dec_spec, dec_runin, spin_wait, chunk_adapt, chunk_mult, fill_front;
    std::optional<double> lean_gfac, lean_gmin, eps;
    std::optional<unsigned long> own_prefix_max;
    std::optional<std::pair<int, int>> wg_lone;        // max,div
    std::optional<std::array<double, 3>> rowbal_f;     // NFC_WG_ROWBAL=a,b,c: the rows' factors (anything else: wg_rowbal, 0 / 1)
    std::optional<bool> ring_global;                   // NFC_RING=global / lds
};
inline Switches read_switches() {
    Switches s;
#ifdef NFC_TEST_HOOKS
    const struct { const char *name; std::optional<int> Switches::*at; } ints[] = {
        {"NFC_NO_SMALL", &Switches::no_small}, {"NFC_DEBUG_BAD_LAUNCH", &Switches::debug_bad_launch}, {"NFC_DEBUG_REDO_SUBMITTED", &Switches::debug_redo_submitted},
        {"NFC_DEBUG", &Switches::debug}, {"NFC_TRACE", &Switches::trace}, {"NFC_TRACE_ALLOC", &Switches::trace_alloc}, {"NFC_NO_SUBMIT_AHEAD", &Switches::no_submit_ahead},
        {"NFC_WG", &Switches::wg}, {"NFC_WG_ROUNDS", &Switches::wg_rounds}, {"NFC_WG_BULK", &Switches::wg_bulk},
        {"NFC_WG_RERUN", &Switches::wg_rerun}, {"NFC_WG_NR", &Switches::wg_nr}, {"NFC_WG_PER_CU", &Switches::wg_per_cu},
        {"NFC_WG_PER_CU_AHEAD", &Switches::wg_per_cu_ahead}, {"NFC_WG_EX", &Switches::wg_ex}, {"NFC_LEAN", &Switches::lean}, {"NFC_LEAN_ROUNDS", &Switches::lean_rounds},
        {"NFC_LEAN_WAVES", &Switches::lean_waves}, {"NFC_EDGE_PREFIX", &Switches::edge_prefix}, {"NFC_DEC_SPEC", &Switches::dec_spec}, {"NFC_DEC_RUNIN", &Switches::dec_runin},
        {"NFC_SPIN_WAIT", &Switches::spin_wait}, {"NFC_CHUNK_ADAPT", &Switches::chunk_adapt}, {"NFC_CHUNK_MULT", &Switches::chunk_mult}, {"NFC_FILL_FRONT", &Switches::fill_front}};
    const struct { const char *name; std::optional<double> Switches::*at; } reals[] = {
        {"NFC_LEAN_GFAC", &Switches::lean_gfac}, {"NFC_LEAN_GMIN", &Switches::lean_gmin}, {"NFC_EPS", &Switches::eps}};
    for (const auto &v : ints)
        if (const char *e = getenv(v.name)) s.*v.at = atoi(e);
    for (const auto &v : reals)
        if (const char *e = getenv(v.name)) s.*v.at = atof(e);
    if (const char *e = getenv("NFC_DEBUG_CLK")) s.debug_clk = e;
    if (const char *e = getenv("NFC_OWN_PREFIX_MAX")) s.own_prefix_max = strtoul(e, nullptr, 10);
    if (const char *e = getenv("NFC_WG_LONE")) {
        int a = 4, b = 64;
        if (sscanf(e, "%d,%d", &a, &b) >= 1) s.wg_lone = std::make_pair(a, b);
    }
    if (const char *e = getenv("NFC_WG_ROWBAL")) {   // 0: chunks of equal length (host_threshold.h: the cut by dispatch row); a,b,c: the rows' factors
        std::array<double, 3> f{0.0, 1.0, 1.0};
        if (sscanf(e, "%lf,%lf,%lf", &f[0], &f[1], &f[2]) >= 2 && f[0] > 0.5 && f[0] < 1.5 && f[1] > 0.5 && f[1] < 1.5 && f[2] > 0.5 && f[2] < 1.5)
            s.rowbal_f = f;
        else s.wg_rowbal = atoi(e);
    }
    if (const char *e = getenv("NFC_RING")) {
        if (strcmp(e, "global") == 0) s.ring_global = true;
        else if (strcmp(e, "lds") == 0) s.ring_global = false;
    }
#endif
    return s;
}
}  // namespace

struct nfc_ctx {
    nfc_params P;
    const KindKernels *kk = nullptr;   // the threshold-stage kernels of P.input_kind (kind_kernels.h)
    int L, mx, Lpad, wpb, twords;
    double factor;
    double hi_plus, lo_a, lo_b, hi_a, hi_b;
    int bands_ok, fast_ok, nfold, wave_slots, lds_per_slot;
    int C_min;   // the configured chunk length, or the smallest one thr_prepare chooses (a batch's own: ThrPlan.chunk, host_threshold.h)
    uint32_t ring_carried = 0;   // nfc_stats.ring_slots_carried of the last batch adopted
    // the decode stage's speculative form (decode.hip.h: k_dec_spec): on unless NFC_DEC_SPEC=0; run-in edges per thread (2 / 4 / 8);
    // after a batch whose check failed the next batches take the three-launch form (spec_off_left counts them down)
    bool dec_spec = true, dec_spec_now = false;
    int dec_runin = 2, spec_off_left = 0, spec_fail_streak = 0;   // (streak: speculative attempts that failed in a row: the back-off doubles)
    size_t dec_lds[3] = {0, 0, 0};   // dynamic LDS of k_dec_spec / k_dec_reduce / k_dec_apply: the stream's tables (decode.hip.h: dec_table_bytes), set with T
    // what the decode stage left for the readers: packet bits packed 32 to a word (the multi-launch stage) or a byte each (short
    // batches); symbol arrays not written yet (materialize_symbols: on the first nfc_read_symbols)
    bool bits_packed = false, sym_lazy = false, sym_own = false;
    FrameOut sym_P;
    uint32_t sym_n = 0, sym_tiles = 0;
    uint32_t decode_respeculated = 0;   // batches whose decode stage was repeated with the three-launch form (nfc_stats)
    int lean = 1, lean_rounds = 0, lean_slots = 0;   // pass 0 by k_threshold_lean (NFC_LEAN=0 turns it off), the longest superstep (NFC_LEAN_ROUNDS), resident waves
    int n_cus = 1;                                             // compute units of the device
    // ... the rows' chunk lengths over the equal cut's, all but the last row's, by workgroups per CU (measured: host_threshold.h); [0]: NFC_WG_ROWBAL=a,b,c
    double rowbal_f[5][3] = {{1, 1, 1}, {1, 1, 1}, {1.02, 1, 1}, {1.045, 1.004, 1}, {1.036, 1.015, 0.990}};
    bool rowbal_set = false;
    bool wg_rowbal = true;                                     // chunks cut by dispatch row (host_threshold.h: thr_prepare; NFC_WG_ROWBAL=0: the equal cut)
    // pass 0 by k_threshold_wg (a chunk per workgroup; NFC_WG=0 turns it off): it applies to this stream, rows of 64 samples per step (NFC_WG_NR),
    // resident workgroups (one batch at a time / for a batch submitted ahead), the longest superstep in rounds (NFC_WG_ROUNDS)
    int wg = 1, wg_ok = 0, wg_nr = 4, wg_slots = 0, wg_slots_ahead = 0, wg_rounds = 0;
    // batches still to be cut into fine_mult times as many chunks (after a batch that needed re-runs); NFC_CHUNK_ADAPT=0 turns it off
    int fine_left = 0, fine_adapt = 1, fine_mult = 4;
    size_t wg_lds = 0, wg_lds_base = 0, wg_lds_bulk_max = 0;   // dynamic LDS of k_threshold_wg: with the staging ring / without any staging / the most a whole chunk's planes may bring it to
    bool wg_bulk = true;                                       // a chunk's plane words leave when the chunk is done (NFC_WG_BULK=0: always the ring)
    int wg_lone_max = 4, wg_lone_div = 64;   // ... how many failing chunks still count as lone: at most this many, and at most one in wg_lone_div
    int wg_rerun_lone = 1;   // a lone failing chunk of a clean batch is re-run by k_threshold_wg, gave up or not (rerun_plan.h; NFC_WG_RERUN=0 in the test build: never)
    // re-runs by k_threshold_wg<KIND, 4, true> (failed rounds evaluated in place): where it applies, its LDS, up to how many failing chunks
    // of a round take it (more: k_threshold, whose one wave per chunk fills the machine where every chunk fails)
    int wg_ex_ok = 0, wg_ex_max = 0;
    size_t wg_ex_lds = 0;
    float lean_gfac = 1.3f, lean_gmin = 9.765625e-4f;   // drift allowance of the next superstep: max(gfac * B, gmin * ss)
    // the ring of a chunk in global memory instead of LDS (which batch takes it: thr_prepare)
    int gring_ok = 0, gring_force = 0, wave_slots_g = 0;   // long windows qualify (NFC_RING=lds|global overrides the choice)
    uint32_t own_prefix_max = OWN_PREFIX_MAX_TILES;   // tile counts up to this need no prefix launches (NFC_OWN_PREFIX_MAX overrides)
    int use_small = 1;   // short batches take the one-launch edge / decode / framing kernel (NFC_NO_SMALL=1 turns it off)
    double expect_ms = 0.3;   // how long the stamp of a batch has taken to appear lately (wait_for_stamp)
    bool spin_wait = true;   // a batch's end is seen in the mirror's stamp word, not waited for on the stream (NFC_SPIN_WAIT=0; host_threshold.h)
    uint64_t selmask;
    float eps;               // certification margin of the speculative pass, relative to the window sum (1 %; host_threshold.h: eps_adapt says why it stays there)
    float i16_scale;         // the kernels' conversion argument: the int16 kinds' scale, -1 for sample / 32767 (i16_to_float); the complex 8-bit
                             // kinds' route and scale (iq8_kernel_arg, threshold.hip.h: iq8_env)
    size_t in_bytes_per_sample;
    // (the streams come before every buffer and event of the context: members go in reverse order, so a stream outlives what was enqueued on it)
    hipStream_t st = nullptr;   // the stream in use: own_st, st_a for a batch submitted ahead, or the caller's (nfc_set_stream) -- not owned
    Stream own_st;              // the stream the context created
    Stream st_a;                // a submitted batch's threshold stage runs here (host_submit.h)
    Event ev[8];
    DevBuf d_gring;
    bool state_dirty = false, dirty_fill_ring = false;   // host-side carried values not yet on the device (push_state)
    float dirty_fill = 0.f;
    Carry dirty_carry;
    EdgeCarry dirty_ecarry;
    DecCarry dirty_dcarry;
    bool cert_pending = false;   // the first certification waits to share a launch with the edge writer (host_stages.h: k_certify_and_write)
    CertLaunch cert;
    // The window fill of a fresh stream's first batch leaves the head of the batch: pass 0 starts at once (ThrArgs.own_window) and the fill's
    // work rides with the edge stage's reduce pass, the first launch behind pass 0 (host_stages.h: k_edge_reduce_and_fill).  fill_can_ride:
    // the batch in work will launch that pass (process_batch); fill_front: never (NFC_FILL_FRONT=1 in the test build); the counters: batches
    // that took the new order / that were repeated with k_fill in front because their window's sum depends on the order (test build)
    bool fill_pending = false, fill_can_ride = false, fill_front = false;
    FillRider fill;
    uint32_t dbg_fill_rode = 0, dbg_fill_refront = 0;
    // the route the last batch's threshold stage took (run_threshold; the test build's nfc_debug_threshold_route): parallel attempts, spans
    // handed to the sequential kernel, the samples it took, and which exit sent the rest of the batch there (0 none: a parallel attempt
    // stood; 1 the sequential kernel was configured or the window is shorter than a step; 2 round >= 6; 3 left <= 4 * span)
    uint32_t route[4] = {0, 0, 0, 0};
    // debugging switches, read ONCE for nfc_create (read_switches: an inherited environment must not reach the per-launch path)
    bool dbg_bad_launch = false, dbg_redo_submitted = false, dbg_no_submit_ahead = false, dbg_any = false, dbg_clk = false, dbg_trace = false;
    std::string dbg_clk_path;
    uint32_t batch_seq = 0;   // stamped into the state block by every batch's first kernel, checked in the mirror
    int timing = 0;   // 0: no events, 1: the threshold kernels' own start / stop events, 2: + batch total and stages as stream markers (nfc_set_timing)
    Event kev[2 * 6];  // start/stop pairs around the first k_threshold launches of a batch
    int n_kev = 0;
    std::string err;
    LaunchError launch_err;   // the first launch of the batch in work that the runtime rejected (launch_check.h)

    // tables
    DevBuf d_mil_map, d_man_map, d_mil_out, d_man_out, d_qmil_map, d_qmil_step;
    uint8_t mil_q_of[16], mil_canon[16];   // Miller state -> class of the quotient machine (0xFF: none) / -> canonical state (decoder_tables.h)
    DecTables T;

    // carried state
    DevBuf d_state, d_ring[NRING];   // the window: the carried one, the one the batch in work writes, and -- with batches submitted
                                     // ahead (nfc_submit_device) -- the ones THOSE write; they rotate
    // pinned host mirror of d_state (mapped AND coherent, explicitly: the host watches the stamp word while the stream runs -- host_threshold.h:
    // wait_for_stamp); hs is the block of hs_pin as what it holds
    PinBuf hs_pin{hipHostMallocMapped | hipHostMallocCoherent};
    DevState *hs = nullptr;
    void *hs_dev = nullptr;        // the same memory as the device addresses it (kernels may fill the mirror themselves)
    PinBuf h_stage;                // pinned staging for nfc_get_state
    PinBuf h_pk_stage;             // pinned staging for the packet tables (pk_stage)
    PinBuf h_edge_stage;           // pinned staging for nfc_read_edges / nfc_read_edges_compact (two pieces)
    std::vector<uint64_t> edge_lut;    // per LUT row: the (d, v) half of an nfc_edge record
    PinBuf h_cflags;               // pinned mirror of the per-chunk flag sections
    int ring_cur = 0;
    // ---- a batch submitted ahead (nfc_submit_device / nfc_wait): its threshold stage runs on st_a beside the edge and
    // decode stages of the batch before it on st
    DevBuf d_neg_alt[NSUB - 1], d_pos_alt[NSUB - 1];   // planes of the batches whose edge stage is not enqueued yet (a set becomes
                                                       // d_neg / d_pos then, and the retired set takes its place in the pool)
    uint32_t alt_free = (1u << (NSUB - 1)) - 1u;       // which of them are free
    PinBuf hs_a[NSUB];                         // pinned snapshots of the state block taken right after a submitted batch's certification
    Event ev_a[NSUB], ev_b[NSUB];              // its threshold stage / its last stage done
    Event kev_sub[NSUB][2];                    // start / stop of its threshold kernel (nfc_set_timing >= 1)
    struct Submitted {
        const void *d_in = nullptr;
        uint32_t n = 0, seq = 0, nch = 0, chunk = 0;
        uint64_t g0 = 0;
        int slot = 0, planes = -1, ring_in = 0, timing = 0;   // (timing: nfc_set_timing's level when the batch was submitted)
        uint32_t allocs = 0;   // buffers (re)allocated on its behalf so far (nfc_stats.device_allocs)
        bool fast = false, b_enqueued = false, timed = false, spec = false;   // (spec: its decode stage ran in the speculative form)
    } sub[NSUB];
    int sub_count = 0;             // batches submitted and not yet waited for (sub[0] the oldest)
    uint32_t slot_next = 0;
    bool low_valid = false;        // Carry.low_nl / low_kl on the device describe the end of the last completed batch
    size_t lean_lds_per_cu = 0;
    size_t ahead_lds_per_cu = 0;   // LDS the threshold kernel of a batch submitted ahead holds per CU (the kernel that actually runs)
    uint32_t stamp_b = 0;          // the batch number the decode stage's last launch writes into the mirror (seq[1])
    bool in_wait = false;
    uint32_t dbg_fast_waits = 0;
    uint32_t stats_redo_submitted = 0;   // submitted batches that had to go through the synchronous path after all
    Carry h_carry;
    EdgeCarry h_ecarry;
    DecCarry h_dcarry;
    uint64_t nseen = 0;

    // batch buffers
    DevBuf d_certinfo;
    DevBuf d_in, d_neg, d_pos, d_ringout[2], d_touched[2], d_info[2], d_ringin, d_meta, d_ver, d_cflags, d_list;
    DevBuf d_ecode, d_epos, d_eidx;   // per entry: code, batch-local sample position (edges.hip.h); caller's own indices (nfc_push_edges)
    bool edges_from_host = false;
    std::vector<nfc_edge> h_pushed;   // the entries of the last nfc_push_edges, as nfc_read_edges hands them back
    DevBuf d_states, d_sym[2], d_bits[2], d_pending[2][2], d_close_end[2],
        d_close_idx[2];
    DevBuf d_partials, d_partials2, d_aggs, d_faggs;  // scan scratch
    DevBuf d_edge_rec;   // the edge stage's reduce pass to its writer: a record per writer thread (edges.hip.h: EdgeRec).  One buffer serves batches
                         // submitted ahead too: the edge stages of consecutive batches run one after the other on the main stream
    // the writer reads those records instead of scanning its tile where the tail is what the step waits for: one batch at a time.  The edge
    // stage of a batch that ran ahead runs beside the next batch's threshold kernel, which is bound by its bytes and sets the step: there the
    // records' 12.5 MB of traffic cost more than the writer's instructions (measured: profiles/edge_prefix_ab.txt) and the writer scans.
    // -1: that rule; the test build's NFC_EDGE_PREFIX=0 / 1: never / always
    int edge_prefix = -1;
    DevBuf d_spec;                           // per decode tile: its map, the state it assumed (decode.hip.h: DecSpec)
    DevBuf d_stage_bits[2], d_stage_cb[2], d_stage_ci[2], d_stage_q[2], d_stage_own;   // ... and what it stages for k_concat (TileStage)
    DevBuf d_pack;                           // nfc_get_state staging
    DevBuf d_gvtop;                          // per chunk: bound of the ring values (guard of the fp64 sums)
    DevBuf d_seqout;                         // sequential kernel: edge-timing state after its last sample
    uint32_t cap_edges = 0, cap_sym[2] = {0, 0};   // capacity estimates of the edge / symbol buffers
    // what the buffers behind those estimates are ALLOCATED for: at least the estimates, and room for a quarter of an entry per
    // sample (four times a clean capture's density; hovering load modulation doubles it) -- the estimates size the grids and follow
    // the stream, the allocations are made once per batch length (size_capacities)
    uint32_t alloc_edges = 0, alloc_sym[2] = {0, 0};
    uint64_t alloc_mark = 0;                       // devbuf_allocs() when the batch in work began
    uint64_t cap_edges_floor = 0, cap_sym_floor[2] = {0, 0};   // raised when an estimate proved too small for this batch
    double edge_rate = 0.125;                      // entries per sample seen lately (peak-hold with slow decay)
    double sym_rate[2] = {1.0, 2.0};               // symbols per entry, per type (start at the upper bounds)
    int pend_cur = 0;                               // which half of d_pending holds the open packets' bits
    RerunBook book;                                 // the rounds of the attempt in work (rerun_plan.h; reset per attempt, capacity kept)

    // last batch
    const void *last_in = nullptr;
    uint32_t last_n = 0, last_skip = 0;
    uint64_t last_g0 = 0;
    uint32_t n_edges = 0;
    uint32_t n_sym[2] = {0, 0}, n_close[2] = {0, 0}, n_bits[2] = {0, 0};
    bool have_outputs = false;
    nfc_stats stats;
    // lazily built packet lists
    std::vector<nfc_packet> pk[2];
    bool pk_ready[2] = {false, false};
    // lazily assembled frames (frames.hip.h; nfc_read_frames ...): records, bytes and parity bits per type, the four totals
    DevBuf d_fr_rec[2], d_fr_bytes[2], d_fr_par[2], d_fr_tot;
    bool frames_ready = false;
    uint64_t fr_frames[2] = {0, 0}, fr_bytes[2] = {0, 0};
    Event fr_ev[2];   // around the two launches (nfc_set_timing >= 1)
    float fr_ms = 0.f;
    bool fr_enqueued = false, fr_timed = false;   // the two launches of this batch are on the stream; the totals are not read yet
    frames::CtxArgs fr_args;                      // ... with these arguments
    // tracked commands (ctx_commands.hip.h; nfc_track_commands ...): nothing of it exists until the machine is first touched
    struct Commands {
        bool on = false;
        bool batch = false;        // tracking was on when the last batch completed
        bool launched = false;     // ... and it had closes: the six launches are on the stream
        bool timed = false, read = false;
        DevBuf d_state, d_keys, d_out, d_scratch;
        PinBuf h_out;
        size_t at_cmd = 0, at_src = 0, at_data = 0, at_enc = 0, out_bytes = 0;
        uint32_t cap_cmds = 0, cap_bytes = 0;
        Event ev[5];               // before the frames' scan, behind the assembly, the segment numbering, the walk, the resolve
    } cc;
};

namespace {

int fail(nfc_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

inline Carry *dC(nfc_ctx *c) { return &((DevState *)c->d_state.p)->carry; }
inline EdgeCarry *dE(nfc_ctx *c) { return &((DevState *)c->d_state.p)->ecarry; }
inline DecCarry *dD(nfc_ctx *c) { return &((DevState *)c->d_state.p)->dcarry; }
inline uint8_t *dT(nfc_ctx *c) { return ((DevState *)c->d_state.p)->totals; }

// one copy brings the whole mirrored block to pinned host memory
inline hipError_t mirror_async(nfc_ctx *c) {
    return hipMemcpyAsync(c->hs, c->d_state.p, sizeof(DevState), hipMemcpyDeviceToHost, c->st);
}
inline void adopt_mirror(nfc_ctx *c) {
    c->h_carry = c->hs->carry;
    carry_apply_fin(c->h_carry);
    c->h_ecarry = c->hs->ecarry;
    c->h_dcarry = c->hs->dcarry;
}
// carried state set from the host without a copy engine round trip: the values travel as kernel arguments
__global__ void k_set_state(DevState *d, Carry a, EdgeCarry b, DecCarry e, int zero_totals, float *fill_ring, int ring_len, float fill) {
    if (fill_ring)
        for (int i = threadIdx.x; i < ring_len; i += blockDim.x) fill_ring[i] = fill;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    d->carry = a;
    d->ecarry = b;
    d->dcarry = e;
    if (zero_totals)
        for (int i = 0; i < TOT_BYTES; i++) d->totals[i] = 0;
}
inline void launch_set_state(nfc_ctx *c, int zero_totals, bool fill_ring, float fill) {
    NFC_LAUNCH(k_set_state, dim3(1), dim3(256), 0, c->st, (DevState *)c->d_state.p, c->h_carry, c->h_ecarry, c->h_dcarry,
                       zero_totals, fill_ring ? c->d_ring[c->ring_cur].as<float>() : (float *)nullptr, fill_ring && fill != 0.f ? c->L : c->Lpad,
                       fill);
}
// The host values become the device state lazily: with the next batch's first launch (k_fill takes them along), or
// right away when something reads the device state first (flush_state).
inline void push_state(nfc_ctx *c, int zero_totals = 0, bool fill_ring = false, float fill = 0.f) {
    c->low_valid = false;   // (the LOW bookkeeping a submitted batch would read on the device is not part of what the host sets)
    if (zero_totals) {
        launch_set_state(c, zero_totals, fill_ring, fill);
        c->state_dirty = false;
        return;
    }
    c->state_dirty = true;
    c->dirty_fill_ring = c->dirty_fill_ring || fill_ring;
    if (fill_ring) c->dirty_fill = fill;
    // the values as of NOW (process_batch advances the host mirrors before the batch's first launch)
    c->dirty_carry = c->h_carry;
    c->dirty_ecarry = c->h_ecarry;
    c->dirty_dcarry = c->h_dcarry;
}
inline void flush_state(nfc_ctx *c) {
    if (!c->state_dirty) return;
    NFC_LAUNCH(k_set_state, dim3(1), dim3(256), 0, c->st, (DevState *)c->d_state.p, c->dirty_carry, c->dirty_ecarry, c->dirty_dcarry, 0,
                       c->dirty_fill_ring ? c->d_ring[c->ring_cur].as<float>() : (float *)nullptr,
                       c->dirty_fill_ring && c->dirty_fill != 0.f ? c->L : c->Lpad, c->dirty_fill);
    c->state_dirty = c->dirty_fill_ring = false;
}
// ring | pending bits (type 0, type 1) as one contiguous byte vector (nfc_get_state)
__global__ void k_pack_state(uint8_t *dst, const float *ring, int L, const uint8_t *p0, uint32_t n0, const uint8_t *p1, uint32_t n1) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    float *rd = (float *)dst;
    for (uint32_t i = tid; i < (uint32_t)L; i += nth) rd[i] = ring[i];
    uint8_t *pd = dst + (size_t)L * 4;
    for (uint32_t i = tid; i < n0; i += nth) pd[i] = p0[i];
    for (uint32_t i = tid; i < n1; i += nth) pd[n0 + i] = p1[i];
}

#define HIPCHK(c, call)                                                                              \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess)                                                                       \
            return fail((c), NFC_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// A kernel launch of this batch was rejected by the runtime (launch_check.h), or -- with_mirror -- the host's mirror of the
// state block was not written by this batch's kernels: nothing the host would read next can be trusted.
int batch_ok(nfc_ctx *c, bool with_mirror) {
    LaunchError &le = launch_error();
    if (le.err != hipSuccess) {
        const LaunchError e = le;
        le = LaunchError{};
        return fail(c, NFC_ERR_DEVICE, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e.err), e.file, e.line);
    }
    if (with_mirror && c->hs->seq[0] != c->batch_seq)
        return fail(c, NFC_ERR_DEVICE, "state mirror is stale (batch %u, mirror %u): a kernel of this batch did not run", c->batch_seq, c->hs->seq[0]);
    return NFC_OK;
}
#define BATCHCHK(c, with_mirror)                                   \
    do {                                                           \
        if (int rc__ = batch_ok((c), (with_mirror))) return rc__;  \
    } while (0)

// ride_cert0 (threshold_span: where pass 0 may start without it): chunk 0's verdict byte -- a fresh stream's fill is then not launched
// but left pending for the edge stage's reduce pass (true), any other stream's is launched as ever.
bool launch_fill_kind(nfc_ctx *c, const void *in, uint32_t n, int nchunks, int ring_idx = -1, const uint8_t *ride_cert0 = nullptr) {
    float *ring = c->d_ring[ring_idx < 0 ? c->ring_cur : ring_idx].as<float>();
    Carry *cr = dC(c);
    EdgeCarryInit eci{(int32_t *)dE(c), c->L % c->mx};
    uint8_t *ver = c->d_ver.as<uint8_t>();
    CertSummary *sum = (CertSummary *)(dT(c) + TOT_CERT);
    StateInit init;
    memset(&init, 0, sizeof init);
    int fresh = 0;
    if (c->state_dirty) {
        static_assert(offsetof(DevState, totals) <= sizeof init.words && offsetof(DevState, totals) % 4 == 0, "state head fits");
        DevState h;
        h.carry = c->dirty_carry;
        h.ecarry = c->dirty_ecarry;
        h.dcarry = c->dirty_dcarry;
        init.apply = 1;
        init.n_words = (int32_t)(offsetof(DevState, totals) / 4);
        memcpy(init.words, &h, offsetof(DevState, totals));
        init.dst = (uint32_t *)c->d_state.p;
        init.fill_ring = c->dirty_fill_ring ? 1 : 0;
        init.fill = c->dirty_fill;
        init.ring_len = c->Lpad;
        c->state_dirty = c->dirty_fill_ring = false;
        // (a stream that starts here with a whole window in the batch: k_fill's short form)
        fresh = h.carry.stable == 0 && h.carry.filled == 0 && n >= (uint32_t)c->L && (void *)cr == c->d_state.p;
    }
    uint32_t *const seq_dst = &((DevState *)c->d_state.p)->seq[0];
    if (fresh && ride_cert0) {
        c->fill = FillRider{c->L, nchunks, ring, cr, eci, ver, ride_cert0, sum, seq_dst, c->batch_seq, init};
        c->fill_pending = true;
        return true;
    }
    NFC_LAUNCH(c->kk->fill, dim3(1), dim3(FILL_BLOCK), (size_t)c->Lpad * 4, c->st, in, n, c->i16_scale, c->L, ring, cr, eci, ver, nchunks, sum, init,
               seq_dst, c->batch_seq, fresh);
    return false;
}
void launch_seq_kind(nfc_ctx *c, const SeqArgs &A) { NFC_LAUNCH(c->kk->seq, dim3(1), dim3(64), 0, c->st, A); }

int ceil_log2(int v) {
    int b = 0;
    while ((1 << b) < v) b++;
    return b;
}

double elapsed_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}


}  // namespace
