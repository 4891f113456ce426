#!/usr/bin/env python3
"""Frames to commands for many streams: one host call per stream against the protocol machine on the GPU, in the same process.
Kept under tests/ like frames_bench.py (not collected by pytest).

  captures   K copies of the 24-frame Classic capture of tests/test_commands.py (a first authentication, four encrypted reads, a nested
             authentication, one more read; 39 269 complex samples, fc32), as overlapping ranges of one device buffer; K = 1 024, 16 384
  leg A      fetch_frames() + a loop of fsm.process_frames(frames_of(k), dispatch=False) over a fresh fsm per stream
  leg B      fetch_commands() + cmd_mask(READT) + plain_crc_ok_mask()
             both start from the same completed push (tracking on); microseconds per capture, bytes copied
  also       the push alone with tracking off and on (wall time; with tracking on up to the end of its three launches, which the push only
             enqueues: the read of one machine's state waits for them),
             the three launches' and the machine kernel's time by HIP events
  protocol   the legs alternate, the order flipping every repeat, warm-up excluded, `repeats` (>= 5) of each; min / median / max
  cross-check  the record fields (cmd, type, n_bytes, n_header, n_extra, n_crc, flags, n_enc) of every command of A and B are equal (sha256)

    python tests/commands_bench.py [--repeats N] [--out profiles/commands_bench.json]   every K, each in a child process under its own
                                                                                        time limit; stops at the first failure
    python tests/commands_bench.py --leg K [--repeats N]                                one K, one JSON line"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(1024, 240), (16384, 560)]   # (K, seconds allowed)
FIELDS = ['cmd', 'type', 'n_bytes', 'n_header', 'n_extra', 'n_crc', 'flags', 'n_enc']
READT = 22


def spread(times, scale=1.0):
    t = np.asarray(times) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[commands_bench] ' + msg, file=sys.stderr, flush=True)


def digest(table):
    h = hashlib.sha256()
    for name in FIELDS:
        h.update(np.ascontiguousarray(table[name]).tobytes())
    return h.hexdigest()


def leg(K, repeats):
    from usrp_nfc_amd import api, fsm, synth
    frames = synth.frames_from_trace(os.path.join(ROOT, 'tests', 'golden', '1k_with_enc.out'))[0][:24]
    iq = synth.iq_from_profile(synth.modulation_profile(frames))
    N = len(iq) // 2
    buf = api.DeviceBuffer(iq)
    first, n = np.zeros(K, np.uint64), np.full(K, N, np.uint32)
    multi = api.NfcMultiContext(K, N, samp_rate=2e6, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32)
    multi.set_timing(True)
    devnull = open(os.devnull, 'w')
    info = dict(a=[], b=[])

    def push(track):
        multi.track_commands(track)
        multi.reset()
        t0 = time.perf_counter()
        multi.push_device(buf, first, n)
        if track:
            multi.fsm_state(0)   # (a tracked push returns with its three launches enqueued: reading one machine waits for them)
        return time.perf_counter() - t0

    def run(which):
        t0 = time.perf_counter()
        if which == 'a':
            fr = multi.fetch_frames(copy=False)
            tables = []
            for k in range(K):
                tables.append(fsm.fsm(out=devnull).process_frames(fr.frames_of(k), dispatch=False)[0])
            out = np.concatenate(tables)
            info['a'].append((fr.ms_kernels, 0.0, fr.bytes_copied))
        else:
            cm = multi.fetch_commands(copy=False)
            reads, crc = cm.cmd_mask(READT), cm.plain_crc_ok_mask()
            out = (cm.cmd.copy(), int(reads.sum()), int(crc.sum()))
            info['b'].append((cm.ms_kernels, cm.ms_machine, cm.bytes_copied))
        return time.perf_counter() - t0, out

    push(True)   # warm-up, and the cross-check
    _, ta = run('a')
    _, (tb, n_reads, n_crc) = run('b')
    da = digest(ta)
    assert len(ta) == len(tb) == 24 * K and da == digest(tb), 'the commands of leg A and leg B differ'
    assert n_reads == 5 * K and n_crc == 14 * K
    note('K = %d: %d commands, digests equal' % (K, len(ta)))
    del ta, tb
    for v in info.values():
        del v[:]
    acc = dict(a=[], b=[], off=[], on=[])
    for i in range(repeats):
        acc['off'].append(push(False))
        acc['on'].append(push(True))
        for name in (('a', 'b') if i % 2 == 0 else ('b', 'a')):
            t, _ = run(name)
            acc[name].append(t)
    res = dict(K=K, samples_per_capture=N, commands_total=24 * K, repeats=repeats, digest=da,
               us_per_capture=dict(A=spread(acc['a'], 1e6 / K), B=spread(acc['b'], 1e6 / K)),
               bytes_copied=dict(A=int(info['a'][0][2]), B=int(info['b'][0][2])),
               ms_push=dict(tracking_off=spread(acc['off'], 1e3), tracking_on=spread(acc['on'], 1e3)),
               ms_kernels=dict(frames_of_A=spread([v[0] for v in info['a']]), three_launches_of_B=spread([v[0] for v in info['b']]),
                               machine_kernel=spread([v[1] for v in info['b']])),
               a_median_over_b_median=float(np.median(acc['a']) / np.median(acc['b'])))
    multi.close()
    buf.free()
    return res


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    if '--leg' in args:
        print(json.dumps(leg(int(args[args.index('--leg') + 1]), max(1, repeats))))
        return 0
    out = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'commands_bench.json')
    results = []
    for K, limit in CONFIGS:   # every GPU step under its own time limit; the first failure ends the run
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg', str(K), '--repeats', str(max(5, repeats))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
        if p.returncode != 0:
            print('commands_bench: %s ended with status %d: stopping' % (' '.join(cmd[4:]), p.returncode), file=sys.stderr)
            return p.returncode
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    rec = dict(what='frames to commands for K streams: fetch_frames() + a loop of fsm.process_frames over a fresh fsm per stream (A) against '
                    'fetch_commands() + cmd_mask + plain_crc_ok_mask (B), from the same tracked push; same process, alternating',
               workload='K copies of the first 24 frames of tests/golden/1k_with_enc.out rendered at 2 Msps (39 269 complex samples)', results=results)
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
