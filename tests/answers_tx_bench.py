#!/usr/bin/env python3
"""What transmitting the answers of K emulated streams costs.  Kept under tests/ like air_bench.py (not collected by pytest).

  workload   K copies of the reader side of the 24-frame Classic capture (16 661 samples and 12 answers; the two-sided capture has
             39 269), every stream with the Classic tag card, pushed from ONE device copy of the capture (every stream's first_sample
             is 0); 2 Msps in and out, delay 86.43 us, carrier off; output 8 B x 16 661 x K
  leg A      the route a user had before: fetch_answers(), tx.encode_runs per answer, a run list per stream built in numpy (idle up to
             S, the answer's runs cut where the next command closed), tx.render_device per stream.  Measured at K = 1 024 only; the row
             of K = 16 384 repeats that per-stream figure (a 1 024-stream sample) and says so
  leg B      NfcMultiContext.transmit(out=buf, timed=True): the call's wall time and the two passes by HIP events
  leg C      the yardstick for the render pass, K = 1 024: k_tx_render, carrier off, writing the same number of bytes in the same process
  protocol   the legs alternate in one process, the order flipping every repeat, one warm-up of each excluded, `repeats` (>= 5) of each;
             min / median / max
  cross-check  every leg B repeat: the sha256 of eight streams' samples downloaded from the device buffer is that of the twin's
             (emulate.host_transmit fed the fetched answers of those streams)

    python tests/answers_tx_bench.py [--repeats N] [--ks 1024,16384] [--out profiles/answers_tx_bench.json]"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.emulate_bench import spread   # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
CHECKED, DELAY_US = 8, 86.43


def note(msg):
    print('[answers_tx_bench] ' + msg, file=sys.stderr, flush=True)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_list(an, idx, k, n_rx, delay):
    """leg A's run list of stream k: idle, then every answer's runs, cut where the next answered command closed"""
    from usrp_nfc_amd import tx
    runs, pos = [], 0
    for j in range(int(an.n[k])):
        s = int(idx[k][j]) + delay
        cut = int(idx[k][j + 1]) if j + 1 < int(an.n[k]) else n_rx
        if s >= cut:
            continue
        runs.append(tx.as_runs([(0, max(s - pos, 0) / 2.0)]))
        r = tx.encode_runs(tx.NFC_TX_MANCHESTER, an.bits(k, j))
        ends = np.cumsum((r['dur_us'] * 2.0).astype(np.int64))   # (2 samples a microsecond: binary_src's int(dur * mult))
        keep = min(len(r), int(np.searchsorted(ends, cut - s, 'left')) + 1)
        r = r[:keep].copy()
        if int(ends[keep - 1]) > cut - s:   # the run the cut falls in ends there
            r['dur_us'][-1] -= (int(ends[keep - 1]) - (cut - s)) / 2.0
        runs.append(r)
        pos = s + int(min(ends[keep - 1], cut - s))
    runs.append(tx.as_runs([(0, max(n_rx - pos, 0) / 2.0)]))
    return np.concatenate(runs)


def run(K, repeats, legA_from=None):
    from usrp_nfc_amd import api, emulate, synth, tx
    classic = [f for f in synth.frames_from_trace(os.path.join(GOLD, '1k_with_enc.out'))[0][:24] if f[0] == synth.READER]
    iq = synth.iq_from_profile(synth.modulation_profile(classic))
    n = len(iq) // 2
    card = emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_classic1k.json'), emulate.NFC_EMU_CARD)[0]
    src = api.DeviceBuffer(iq)
    out = api.DeviceBuffer(np.zeros(0, np.float32), nbytes=8 * n * K + 64)
    one = api.DeviceBuffer(np.zeros(0, np.float32), nbytes=8 * n + 64)
    checked = sorted({int(k) for k in np.linspace(0, K - 1, min(K, CHECKED))})
    kw = dict(samp_rate=2e6, delay_us=DELAY_US, align_samples=1)
    delay = int(DELAY_US * 2)
    t = {'A': [], 'B': []}
    sched, render, push_ms = [], [], []
    want = None
    try:
        with api.NfcMultiContext(K, n, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as m:
            m.emulate(card)
            for rep in range(repeats + 1):
                for leg in (('A', 'B') if rep % 2 == 0 else ('B', 'A')):
                    if leg == 'A' and legA_from is not None:
                        continue
                    m.reset()
                    t0 = time.perf_counter()
                    m.push_device(src, np.zeros(K, np.uint64), np.full(K, n, np.uint32))
                    push_ms.append((time.perf_counter() - t0) * 1e3)
                    if leg == 'A':
                        t0 = time.perf_counter()
                        cm, an = m.fetch_commands(), m.fetch_answers()
                        _, idx = emulate.tx_inputs(cm, an)
                        for k in range(K):
                            runs = run_list(an, idx, k, n, delay)
                            tx.render_device(runs, 2e6, one.ptr, n)
                        dt = time.perf_counter() - t0
                    else:
                        t0 = time.perf_counter()
                        tc = m.transmit(out=out, timed=True, **kw)
                        dt = time.perf_counter() - t0
                        if want is None:   # the twin, once: fed the fetched answers of the checked streams
                            cm, an = m.fetch_commands(), m.fetch_answers()
                            answers, idx = emulate.tx_inputs(cm, an)
                            twin = emulate.host_transmit([answers[k] for k in checked], [idx[k] for k in checked], [card.role] * len(checked),
                                                         [0] * len(checked), [n] * len(checked), **kw)[0]
                            want = sha(twin)
                        got = sha(np.concatenate([tc.download(k) for k in checked]))
                        if got != want:
                            raise SystemExit('K %d repeat %d: the device captures are not the twin\'s' % (K, rep))
                        if rep:
                            sched.append(tc.kernel_ms[0]), render.append(tc.kernel_ms[1])
                    if rep:
                        t[leg].append(dt)
        row = dict(K=K, samples_per_stream=n, answers_per_stream=12, bytes=8 * n * K, digest=want, streams_checked=checked,
                   push_ms=spread(push_ms[2:]), transmit_call_ms=spread(t['B'], 1e3), schedule_ms=spread(sched), render_ms=spread(render),
                   render_GBps=8.0 * n * K / float(np.median(render)) / 1e6, us_per_stream_B=spread(np.asarray(t['B']) / K, 1e6))
        if legA_from is None:
            row.update(us_per_stream_A=spread(np.asarray(t['A']) / K, 1e6), legA='measured on all %d streams' % K)
        else:
            row.update(us_per_stream_A=legA_from, legA='not run at this K: the per-stream figure of the 1 024-stream row')
        return row
    finally:
        src.free(), out.free(), one.free()


def yardstick(n_samples, repeats, render_ms_b):
    """k_tx_render, carrier off, on the same number of output bytes as leg B at K = 1 024"""
    from usrp_nfc_amd import api, synth, tx
    period = []
    for d, bits in synth.txn_frames():
        period += [(1, 150.0)] + tx.encode_bits(tx.NFC_TX_MILLER if d == synth.READER else tx.NFC_TX_MANCHESTER, bits)
    one = tx.as_runs(period)
    runs = np.tile(one, max(1, n_samples // tx.sample_count(one, 2e6)))
    n_tx = tx.sample_count(runs, 2e6)
    idle = tx.as_runs([(0, n_samples / 2.0)])   # ... and one idle run of that length: the fill alone
    buf = api.DeviceBuffer(np.zeros(0, np.float32), nbytes=8 * max(n_samples, n_tx) + 64)
    ms = {'tx_frames': [], 'tx_idle': []}
    try:
        for rep in range(repeats + 1):
            for leg in (('tx_frames', 'tx_idle') if rep % 2 == 0 else ('tx_idle', 'tx_frames')):
                _, dt = tx.render_device(runs if leg == 'tx_frames' else idle, 2e6, buf.ptr, max(n_samples, n_tx), timed=True)
                if rep:
                    ms[leg].append(dt)
    finally:
        buf.free()
    gb = {'tx_frames': 8.0 * n_tx / np.median(ms['tx_frames']) / 1e6, 'tx_idle': 8.0 * n_samples / np.median(ms['tx_idle']) / 1e6,
          'answers_tx_render': 8.0 * n_samples / render_ms_b / 1e6}
    return dict(samples=n_samples, tx_samples=n_tx, ms={k: spread(v) for k, v in ms.items()}, GBps=gb,
                render_fraction_of_tx_frames=gb['answers_tx_render'] / gb['tx_frames'], render_fraction_of_tx_idle=gb['answers_tx_render'] / gb['tx_idle'])


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    out_path = args[args.index('--out') + 1] if '--out' in args else None
    ks = [int(v) for v in args[args.index('--ks') + 1].split(',')] if '--ks' in args else [1024, 16384]
    if repeats < 5:
        raise SystemExit('--repeats: at least 5')
    rows, yard, leg_a = [], None, None
    for K in ks:
        note('K = %d' % K)
        rows.append(run(K, repeats, None if K <= 1024 else leg_a))
        note(json.dumps(rows[-1]))
        if K <= 1024:
            leg_a = rows[-1]['us_per_stream_A']
        if K == 1024:
            yard = yardstick(rows[-1]['samples_per_stream'] * K, repeats, rows[-1]['render_ms']['median'])
            note(json.dumps(yard))
    res = dict(bench='answers_tx_bench', repeats=repeats, rows=rows, yardstick=yard)
    print(json.dumps(res))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
