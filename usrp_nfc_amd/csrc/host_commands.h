// host_commands.h -- the host side of a single context's frames and tracked commands: the frames' two launches without their wait
// (enqueue_frames; nfc_amd.hip's ensure_frames reads the totals later), the protocol machine's words on the device, and track_batch,
// which every path that completes a batch calls where the host has learnt the batch's counts (ctx_commands.hip.h says what is launched).
#pragma once

namespace {

// the two launches of the last batch's frames, no wait: the totals stay on the device until somebody needs them (ensure_frames)
int enqueue_frames(nfc_ctx *c) {
    if (c->frames_ready || c->fr_enqueued) return NFC_OK;
    c->fr_ms = 0.f;
    if (!(c->n_close[0] || c->n_close[1])) return NFC_OK;   // (a batch that closed no packet launches nothing)
    frames::CtxArgs &A = c->fr_args;
    memset(&A, 0, sizeof A);
    HIPCHK(c, c->d_fr_tot.ensure(64));
    for (int t = 0; t < 2; t++) {
        // a frame has at most (n_bits + 1) / 9 bytes: the type's bits and one more per close bound the section
        const size_t byte_cap = ((size_t)c->n_bits[t] + c->n_close[t]) / 9 + 16;
        HIPCHK(c, c->d_fr_rec[t].ensure(((size_t)c->n_close[t] + 1) * sizeof(nfc_raw_frame)));
        HIPCHK(c, c->d_fr_bytes[t].ensure(byte_cap));
        HIPCHK(c, c->d_fr_par[t].ensure(byte_cap));
        A.close_end[t] = c->d_close_end[t].as<uint32_t>();
        A.close_idx[t] = c->d_close_idx[t].as<uint64_t>();
        A.n_close[t] = c->n_close[t];
        A.bits[t] = c->d_bits[t].p;
        A.records[t] = c->d_fr_rec[t].as<nfc_raw_frame>();
        A.bytes[t] = c->d_fr_bytes[t].as<uint8_t>();
        A.par[t] = c->d_fr_par[t].as<uint8_t>();
        A.byte_cap[t] = (uint32_t)std::min<size_t>(byte_cap, 0xFFFFFFFFu);
    }
    A.totals = c->d_fr_tot.as<uint64_t>();
    c->fr_timed = c->timing >= 1;
    if (c->fr_timed)
        for (auto &e : c->fr_ev) HIPCHK(c, e.create());
    frames::launch_ctx(A, c->bits_packed, c->st, c->fr_timed ? (hipEvent_t)c->fr_ev[0] : nullptr, c->fr_timed ? (hipEvent_t)c->fr_ev[1] : nullptr);
    c->fr_enqueued = true;
    return NFC_OK;
}

// ---- the machine's words on the device (fsm.hip.h: W_WORDS, one machine) ----
// to and from the device behind everything the stream holds: rare calls, a wait each
int cc_put_words(nfc_ctx *c, DevBuf &dst, const uint32_t *w, size_t words) {
    HIPCHK(c, hipMemcpyAsync(dst.p, w, words * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return NFC_OK;
}
int cc_get_words(nfc_ctx *c, const DevBuf &src, uint32_t *w, size_t words) {
    HIPCHK(c, hipMemcpyAsync(w, src.p, words * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return NFC_OK;
}
int cc_write_machine(nfc_ctx *c, const fsmd::Machine &M) {
    uint32_t w[fsmd::W_WORDS];
    fsmd::store_machine(M, w, 1, 0);
    return cc_put_words(c, c->cc.d_state, w, fsmd::W_WORDS);
}
// allocated, and set to nfc_fsm_state_init's state, by whoever touches the machine first
int cc_ensure_state(nfc_ctx *c) {
    if (c->cc.d_state.p) return NFC_OK;
    HIPCHK(c, c->cc.d_state.ensure(fsmd::W_WORDS * 4));
    fsmd::Machine M;
    fsmd::machine_init(M);
    return cc_write_machine(c, M);
}
int cc_read_machine(nfc_ctx *c, fsmd::Machine &M) {
    if (!c->cc.d_state.p) {
        fsmd::machine_init(M);
        return NFC_OK;
    }
    uint32_t w[fsmd::W_WORDS];
    if (int rc = cc_get_words(c, c->cc.d_state, w, fsmd::W_WORDS)) return rc;
    fsmd::load_machine(M, w, 1, 0);
    return NFC_OK;
}

inline size_t cc_up16(size_t v) { return (v + 15) & ~(size_t)15; }

// Where a batch completes: the host has just learnt its counts.  With tracking on, the frames' two launches and the four of
// ctx_commands.hip.h go onto the stream, no wait; sized by what the host knows -- the closes bound the frames, the bits the bytes.
int track_batch(nfc_ctx *c) {
    nfc_ctx::Commands &cc = c->cc;
    cc.batch = cc.on;
    cc.launched = cc.read = false;
    if (!cc.on) return NFC_OK;
    if (int rc = cc_ensure_state(c)) return rc;
    if (!(c->n_close[0] || c->n_close[1])) return NFC_OK;   // (no frames: nothing is launched, the machine stays)
    cc.timed = c->timing >= 1;
    if (cc.timed) {
        for (auto &e : cc.ev) HIPCHK(c, e.create());
        HIPCHK(c, hipEventRecord(cc.ev[0], c->st));
    }
    if (int rc = enqueue_frames(c)) return rc;
    if (cc.timed) HIPCHK(c, hipEventRecord(cc.ev[1], c->st));
    const frames::CtxArgs &R = c->fr_args;
    const uint64_t cmds = (uint64_t)R.n_close[0] + R.n_close[1], bytes = (uint64_t)R.byte_cap[0] + R.byte_cap[1];
    if (cmds > 0x7FFFFFFFull || bytes > 0xFFFFFFFFull) return fail(c, NFC_ERR_ARG, "batch too long for tracked commands: %llu frames, %llu bytes", (unsigned long long)cmds, (unsigned long long)bytes);
    cc.cap_cmds = (uint32_t)cmds;
    cc.cap_bytes = (uint32_t)bytes;
    const uint32_t cap_seg = R.n_close[1] + 1u;   // a segment per reader frame at the most, and the first
    // the output: counters | records | src | data | enc, one block, one copy
    cc.at_cmd = cc_up16(ctxcmd::H_WORDS * 4);
    cc.at_src = cc.at_cmd + cc_up16((size_t)cc.cap_cmds * sizeof(nfc_frame));
    cc.at_data = cc.at_src + cc_up16((size_t)cc.cap_cmds * 4);
    cc.at_enc = cc.at_data + cc_up16(cc.cap_bytes);
    cc.out_bytes = cc.at_enc + cc_up16((size_t)cc.cap_bytes * 2);
    HIPCHK(c, cc.d_out.ensure(cc.out_bytes));
    // scratch: slot | seg_start | summaries | meta | cut marks
    const size_t at_seg = cc_up16((size_t)cc.cap_cmds * 4), at_sum = at_seg + cc_up16(((size_t)cap_seg + 1) * 4);
    const size_t at_meta = at_sum + cc_up16((size_t)fsmd::W_WORDS * cap_seg * 4), at_cut = at_meta + cc_up16((size_t)cap_seg * 4);
    HIPCHK(c, cc.d_scratch.ensure(at_cut + cc_up16(cc.cap_cmds)));
    uint8_t *out = cc.d_out.as<uint8_t>(), *scr = cc.d_scratch.as<uint8_t>();
    ctxcmd::Args A;
    memset(&A, 0, sizeof A);
    A.rec0 = R.records[0], A.rec1 = R.records[1];
    A.bytes0 = R.bytes[0], A.bytes1 = R.bytes[1], A.par0 = R.par[0], A.par1 = R.par[1];
    A.totals = R.totals;
    A.cap_fr0 = R.n_close[0], A.cap_fr1 = R.n_close[1], A.cap_by0 = R.byte_cap[0], A.cap_by1 = R.byte_cap[1];
    A.state = cc.d_state.as<uint32_t>();
    A.sector_keys = cc.d_keys.as<uint32_t>();
    A.hdr = (uint32_t *)out;
    A.cmd = (uint32_t *)(out + cc.at_cmd);
    A.src = (uint32_t *)(out + cc.at_src);
    A.data = out + cc.at_data;
    A.enc = (uint16_t *)(out + cc.at_enc);
    A.cap_cmds = cc.cap_cmds, A.cap_bytes = cc.cap_bytes, A.cap_seg = cap_seg;
    A.slot = (uint32_t *)scr;
    A.seg_start = (uint32_t *)(scr + at_seg);
    A.sum = (uint32_t *)(scr + at_sum);
    A.meta = (uint32_t *)(scr + at_meta);
    A.cutf = scr + at_cut;
    const hipEvent_t ev[3] = {cc.ev[2], cc.ev[3], cc.ev[4]};
    ctxcmd::launch(A, c->st, cc.timed ? ev : nullptr);
    cc.launched = true;
    return NFC_OK;
}

}  // namespace
