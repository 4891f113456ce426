#!/usr/bin/env python3
"""What rendering K whole-card reads to IQ captures costs on the host and on the GPU.  Kept under tests/ like emulate_bench.py
(not collected by pytest).

  inputs     K DIFFERENT Classic 1K cards read whole (emulate_bench.make_cards through emulate.pairs_host: 199 frames a card, about 3e5
             complex samples a card at 2 Msps); K = 1, 1 024 (fc32 and sc8) and 16 384 (sc8 only)
  leg A      the numpy route the tests use: per card synth.transaction_frames, modulation_profile, iq_from_profile (PCG64 normals),
             quantise_sc8 for sc8, and the upload; measured on at most 16 cards, stated per card
  leg B      the C twin on one core (nfc_host_air_render) and the upload of what it rendered; measured on at most 128 cards (the twin takes
             some 12 ms a card: at K = 16 384 minutes a repeat), stated per card
  leg C      nfc_air_render_device: the call's wall time, and its layout kernels and its render kernel by HIP events
  protocol   the legs alternate in one process, the order flipping every repeat, one warm-up of each excluded, `repeats` (>= 5) of each;
             min / median / max
  cross-check  every leg C repeat: the sha256 of eight streams' bytes downloaded from the device buffer is that of the twin's rendering
             of those streams ALONE under their stream seeds (a sample depends on its key alone); leg B's captures are the twin's by
             construction and leg A's are the yardstick itself
  yardstick  the project's own write-only kernel: k_tx_render with the carrier off writing the same number of bytes as leg C at
             K = 1 024, fc32, in the same call; k_air_render's bytes/s at sigma 0 as a fraction of it, and the sigma = 0.002 figure beside it

    python tests/air_bench.py [--repeats N] [--ks 1,1024,16384] [--out profiles/air_bench.json]"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.emulate_bench import make_cards, spread   # noqa: E402

A_CARDS, B_CARDS, CHECKED = 16, 128, 8


def note(msg):
    print('[air_bench] ' + msg, file=sys.stderr, flush=True)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def subset(tr, ks):
    from usrp_nfc_amd import emulate
    ks = np.asarray(ks)
    return emulate.Transcripts(tr.results[ks], tr.frames[ks], tr.plain[ks], tr.air[ks], tr.par[ks])


def run(K, kind, repeats, tr):
    from usrp_nfc_amd import air, api, synth
    name = {api.NFC_IN_IQ_F32: 'fc32', api.NFC_IN_IQ_I8: 'sc8'}[kind]
    fr = air.frames_of(tr)
    checked = sorted({int(k) for k in np.linspace(0, K - 1, min(K, CHECKED))})
    twin = air.host_render(subset(tr, checked), out_kind=kind, stream_seeds=checked)
    want = sha(np.concatenate([twin.download(i) for i in range(len(checked))]))
    nA, nB = min(K, A_CARDS), min(K, B_CARDS)
    trA, frB = [tr.transcript(k) for k in range(nA)], air.frames_of(subset(tr, np.arange(nB)))
    bps = 8 if kind == api.NFC_IN_IQ_F32 else 2
    stage = api.DeviceBuffer(np.zeros(0, np.uint8), nbytes=frB.bound_samples(8) * bps + 64)

    def leg_a():
        t0 = time.perf_counter()
        for t in trA:
            iq = synth.iq_from_profile(synth.modulation_profile(synth.transaction_frames(t)))
            stage.upload(synth.quantise_sc8(iq) if kind == api.NFC_IN_IQ_I8 else iq)
        return (time.perf_counter() - t0) / nA

    def leg_b():
        t0 = time.perf_counter()
        cap = air.host_render(frB, out_kind=kind)
        stage.upload(cap.download_used())
        return (time.perf_counter() - t0) / nB

    out = dict(K=K, kind=name, frames_per_card=199, cards_measured=dict(A=nA, B=nB, C=K), digest=want, streams_checked=checked)
    per_card = {'A': [], 'B': [], 'C': []}
    layout, render, samples = [], [], 0
    try:
        for rep in range(repeats + 1):
            for leg in (('A', 'B', 'C') if rep % 2 == 0 else ('C', 'B', 'A')):
                if leg == 'C':
                    cap = air.render_device(fr, out_kind=kind, timing=True)
                    try:
                        got = sha(np.concatenate([cap.download(k) for k in checked]))
                        if got != want or not cap.guard_intact():
                            raise SystemExit('K %d %s repeat %d: the device captures are not the twin\'s' % (K, name, rep))
                        dt, samples = cap.call_s / K, cap.used_samples
                        if rep:
                            layout.append(cap.kernel_ms[0]), render.append(cap.kernel_ms[1])
                    finally:
                        cap.free()
                else:
                    dt = leg_a() if leg == 'A' else leg_b()
                if rep:
                    per_card[leg].append(dt)
    finally:
        stage.free()
    out.update(samples=samples, bytes=samples * bps, us_per_card={k: spread(v, 1e6) for k, v in per_card.items()},
               device_call_ms=spread(np.asarray(per_card['C']) * K, 1e3), layout_ms=spread(layout), render_ms=spread(render),
               render_GBps=samples * bps / float(np.median(render)) / 1e6)
    return out


def yardstick(tr, repeats):
    """k_air_render at K = 1 024, fc32, sigma 0 and 0.002, against k_tx_render with the carrier off writing the same number of bytes, alternating."""
    from usrp_nfc_amd import air, api, synth, tx
    fr = air.frames_of(tr)
    _, n = air.sizes(fr)
    total = int(n.astype(np.uint64).sum())
    period = []
    for d, bits in synth.txn_frames():
        period += [(1, 150.0)] + tx.encode_bits(tx.NFC_TX_MILLER if d == synth.READER else tx.NFC_TX_MANCHESTER, bits)
    one = tx.as_runs(period)
    runs = np.tile(one, max(1, total // tx.sample_count(one, 2e6)))   # (whole periods: at most one period short of leg C's samples)
    n_tx = tx.sample_count(runs, 2e6)
    buf = api.DeviceBuffer(np.zeros(0, np.float32), nbytes=8 * max(total, n_tx) + 64)
    ms = {'tx': [], 'air_sigma0': [], 'air_sigma0.002': []}
    used = 0
    try:
        for rep in range(repeats + 1):
            for leg in (('tx', 'air_sigma0', 'air_sigma0.002') if rep % 2 == 0 else ('air_sigma0.002', 'air_sigma0', 'tx')):
                if leg == 'tx':
                    got, t = tx.render_device(runs, 2e6, buf.ptr, n_tx, timed=True)
                    if got != n_tx:
                        raise SystemExit('yardstick: k_tx_render wrote %d of %d samples' % (got, n_tx))
                else:
                    cap = air.render_device(fr, sigma=0.0 if leg == 'air_sigma0' else 0.002, timing=True)
                    t, used = cap.kernel_ms[1], cap.used_samples
                    cap.free()
                if rep:
                    ms[leg].append(t)
    finally:
        buf.free()
    gbps = {'tx': 8.0 * n_tx / np.median(ms['tx']) / 1e6, 'air_sigma0': 8.0 * used / np.median(ms['air_sigma0']) / 1e6,
            'air_sigma0.002': 8.0 * used / np.median(ms['air_sigma0.002']) / 1e6}
    return dict(K=len(fr), kind='fc32', tx_samples=n_tx, air_samples=used, ms={k: spread(v) for k, v in ms.items()}, GBps=gbps,
                air_sigma0_fraction_of_tx=gbps['air_sigma0'] / gbps['tx'], air_sigma0002_fraction_of_tx=gbps['air_sigma0.002'] / gbps['tx'])


def main():
    from usrp_nfc_amd import api, emulate
    args = sys.argv[1:]
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    out_path = args[args.index('--out') + 1] if '--out' in args else None
    ks = [int(v) for v in args[args.index('--ks') + 1].split(',')] if '--ks' in args else [1, 1024, 16384]
    if repeats < 5:
        raise SystemExit('--repeats: at least 5')
    rows, yard = [], None
    for K in ks:
        tags, readers = make_cards(K)
        tr = emulate.pairs_host(tags, readers, link=emulate.NFC_EMU_LINK_AIR, rounds=1, cap_frames=200, cap_bytes=1800)
        if not np.all(tr.results['n_frames'] == 199) or tr.results['flags'].any():
            raise SystemExit('K %d: a card was not read whole' % K)
        for kind in ((api.NFC_IN_IQ_F32, api.NFC_IN_IQ_I8) if K <= 1024 else (api.NFC_IN_IQ_I8,)):
            note('K = %d, kind %d' % (K, kind))
            rows.append(run(K, kind, repeats, tr))
            note(json.dumps(rows[-1]))
        if K == 1024:
            note('yardstick')
            yard = yardstick(tr, repeats)
            note(json.dumps(yard))
    res = dict(bench='air_bench', repeats=repeats, rate_msps=2.0, rows=rows, yardstick=yard)
    print(json.dumps(res))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
