#!/usr/bin/env python3
"""What K whole-card reads cost on one CPU core and on the GPU.  Kept under tests/ like keys_bench.py (not collected by
pytest).

  cards      K DIFFERENT Classic 1K cards -- the reference card's layout, every card with its own UID, data, sixteen key pairs and
             nonces -- each read whole by a reader with the card's key table: 199 frames a card, NFC_EMU_LINK_AIR, NFC_EMU_CARD, one
             round; K = 1, 1 024, 16 384
  leg A      the host twin on one core (nfc_host_emulate_pairs)
  leg B      nfc_emulate_pairs_device, transcripts fetched: the call's wall time, and the kernel alone by HIP events
  protocol   the legs alternate, the order flipping every repeat, one warm-up of each excluded, `repeats` (>= 5) of each; min / median / max
  cross-check  the sha256 over every output array of leg B is leg A's, every repeat; every pair has 199 frames and no flag
  tracked push  K copies of the reader side of the 24-frame Classic capture (12 frames the tag of the trace answered), K = 1 024, 16 384, in
             one multi-stream context: leg C a tracked push with no card (k_multi_commands), leg D the same with a tag card per stream
             (k_multi_commands_emu: every stream answers 12 frames), alternating through emulate(None) / emulate(card) outside the timed
             part; per leg the push's wall time up to the end of its launches, and ms_machine, the machine kernel alone by HIP events;
             cross-check: every stream's answers are stream 0's and stream 0's are the host twin's (nfc_host_emulate), by sha256

    python tests/emulate_bench.py [--repeats N] [--out profiles/emulate_bench.json]"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = [1, 1024, 16384]


def spread(times, scale=1.0):
    t = np.asarray(times) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[emulate_bench] ' + msg, file=sys.stderr, flush=True)


def make_cards(K, seed=7):
    from usrp_nfc_amd import emulate
    rng = np.random.Generator(np.random.PCG64(seed))
    tags, readers = [], []
    for k in range(K):
        mem = rng.integers(0, 256, 1024).astype(np.uint8)
        mem[0] = 0x04 + 4 * (k % 8)
        mem[4] = mem[0] ^ mem[1] ^ mem[2] ^ mem[3]
        for s in range(16):
            mem[(4 * s + 3) * 16 + 6:(4 * s + 3) * 16 + 10] = [0xFF, 0x07, 0x80, 0x69]   # the transport configuration
        table = {(0x60, s): bytes(mem[(4 * s + 3) * 16:(4 * s + 3) * 16 + 6].tolist()) for s in range(16)}
        tags.append(emulate.tag_card(emulate.CLASSIC1K, mem, rng.integers(0, 256, (16, 4))))
        readers.append(emulate.reader_card(rng.integers(0, 256, (16, 4)), table=table))
    return tags, readers


def digest(t):
    h = hashlib.sha256()
    for a in t.arrays():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run(K, repeats):
    from usrp_nfc_amd import emulate
    tags, readers = make_cards(K)
    kw = dict(link=emulate.NFC_EMU_LINK_AIR, rounds=1, cap_frames=200, cap_bytes=1800)
    legs = {'A': lambda: emulate.pairs_host(tags, readers, **kw), 'B': lambda: emulate.pairs_device(tags, readers, timing=True, **kw)}
    wall, kernel, want = {'A': [], 'B': []}, [], None
    for rep in range(repeats + 1):
        for name in (('A', 'B') if rep % 2 == 0 else ('B', 'A')):
            out = legs[name]()
            dt = out.call_s   # (the library call alone: marshalling 16 384 cards through ctypes is Python's time, the same for both legs)
            d = digest(out)
            want = want or d
            if d != want:
                raise SystemExit('K %d leg %s repeat %d: another digest than the first run' % (K, name, rep))
            if rep == 0:
                r = out.results
                if not (np.all(r['n_frames'] == 199) and not r['flags'].any() and not r['tag_flags'].any() and not r['reader_flags'].any()):
                    raise SystemExit('K %d: a card was not read whole' % K)
                continue
            wall[name].append(dt)
            if name == 'B':
                kernel.append(out.kernel_ms)
    return dict(K=K, frames_per_card=199, digest=want, host_ms=spread(wall['A'], 1e3), device_call_ms=spread(wall['B'], 1e3), kernel_ms=spread(kernel),
                host_us_per_card=float(np.median(wall['A'])) * 1e6 / K, device_us_per_card=float(np.median(wall['B'])) * 1e6 / K)


def run_tracked(K, repeats):
    from usrp_nfc_amd import api, emulate, fsm, synth
    gold = os.path.join(ROOT, 'tests', 'golden')
    frames = [f for f in synth.frames_from_trace(os.path.join(gold, '1k_with_enc.out'))[0][:24] if f[0] == synth.READER]
    iq = synth.iq_from_profile(synth.modulation_profile(frames))
    N = len(iq) // 2
    card = emulate.cards_from_json(os.path.join(gold, 'fx_emu_classic1k.json'))[0]
    buf = api.DeviceBuffer(iq)
    first, n = np.zeros(K, np.uint64), np.full(K, N, np.uint32)
    push, machine, want = {'C': [], 'D': []}, {'C': [], 'D': []}, None
    try:
        with api.NfcMultiContext(K, N, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, tag=False) as m:
            m.track_commands()
            m.set_timing(True)
            for rep in range(repeats + 1):
                for name in (('C', 'D') if rep % 2 == 0 else ('D', 'C')):
                    m.emulate(card if name == 'D' else None)
                    m.reset()
                    t0 = time.perf_counter()
                    m.push_device(buf, first, n)
                    m.fsm_state(0)   # (waits for the push's launches)
                    dt = time.perf_counter() - t0
                    cm, an = m.fetch_commands(copy=False), m.fetch_answers(copy=False)
                    if name == 'D':
                        rec = an.records.reshape(K, -1) if an.n_answers == 12 * K else None
                        if rec is None or an.n.tolist() != [12] * K or any(rec[k].tobytes() != rec[0].tobytes() for k in range(K)) or \
                                np.unique(an.air.reshape(K, -1), axis=0).shape[0] != 1:
                            raise SystemExit('K %d leg D: the streams do not answer alike' % K)
                        d = hashlib.sha256(an.answers_of(0)[0].tobytes() + an.answers_of(0)[2].tobytes()).hexdigest()
                        if want is None:
                            _, tw = emulate.host_emulate(card, emulate.state_init(), fsm.state_init(), cm.raw.frames_of(0))
                            want = hashlib.sha256(tw.records.tobytes() + tw.air[:18 * len(tw)].tobytes()).hexdigest()
                        if d != want:
                            raise SystemExit('K %d leg D: the answers are not the host twin\'s' % K)
                    elif an.emulated:
                        raise SystemExit('K %d leg C: answers without a card' % K)
                    if rep:
                        push[name].append(dt)
                        machine[name].append(cm.ms_machine)
    finally:
        buf.free()
    return dict(K=K, samples_per_capture=N, answers_per_stream=12, digest=want, push_ms={k: spread(v, 1e3) for k, v in push.items()},
                ms_machine={k: spread(v) for k, v in machine.items()})


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    out_path = args[args.index('--out') + 1] if '--out' in args else None
    if repeats < 5:
        raise SystemExit('--repeats: at least 5')
    rows = []
    for K in KS:
        note('K = %d' % K)
        rows.append(run(K, repeats))
        note(json.dumps(rows[-1]))
    tracked = []
    for K in (1024, 16384):
        note('tracked push, K = %d' % K)
        tracked.append(run_tracked(K, repeats))
        note(json.dumps(tracked[-1]))
    res = dict(bench='emulate_bench', repeats=repeats, link='AIR', mode='CARD', rows=rows, tracked_push=tracked)
    print(json.dumps(res))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
