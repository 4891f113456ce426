#!/usr/bin/env python3
"""IQ to commands for ONE long stream: the host's protocol machine against the tracked commands of the context, in the same process.
Kept under tests/ like frames_bench.py (not collected by pytest), and measured its way.

  workloads  all        one batch of 1e8 samples of synth.workload('all') at 2 Msps (bench.py's default capture length: 68 142 frames)
             classic    one tile of bench.py's classic1k capture: 1e8 samples at 10 Msps, the Classic trace again and again
             worst      route (b) of tests/test_ctx_commands_host.py stretched: the 24-frame Classic prefix, cut off in mid-session, then
                        Ultralight transactions to 2e7 samples -- the segments behind the first are walked again by ONE lane for as long
                        as the machine stays in the session (it leaves it when ciphertext happens to decrypt to a HALT: the counters say when)
             never      classic with the wrong key A: the machine never leaves its first session, EVERYTHING behind it is walked again
             each resident in HBM, pushed anew from a reset context (and a reset machine) before every timed leg
    leg A    frames(), then fsm.process_frames(dispatch=False)                       (the route there was)
    leg B    the batch pushed by a tracking context, then commands(copy=False)
    leg C    B, then cmd_mask(READT) and plain_crc_ok_mask()
             wall time of what FOLLOWS the push's return (for B and C also the time tracking adds to the push itself), the bytes each
             brings over the link, and -- with nfc_set_timing(1) -- the kernels by HIP events: the frames' two, merged order + segment
             numbering, the speculative walk, the resolve, and all six
  protocol   the legs alternate, the order rotating every repeat, warm-up excluded, `repeats` (>= 5) of each; min / median / max
  cross-check  the records and plaintext of A and of B are equal (sha256 over every record field but byte_off, and the bytes per record)

    python tests/ctx_commands_bench.py [--repeats N] [--out profiles/ctx_commands_bench.json]   every workload, each in a child process
                                                                                  under its own time limit; stops at the first failure
    python tests/ctx_commands_bench.py --leg all | classic | worst | never [--repeats N]                 one workload, one JSON line"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WRONG_KEYS = ([0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], [0xFF] * 6)
CONFIGS = [(['all'], 420), (['classic'], 420), (['worst'], 300), (['never'], 420)]   # (leg, seconds allowed)
FIELDS = ('cmd', 'type', 'n_bytes', 'n_header', 'n_extra', 'n_crc', 'flags', 'n_enc')
READT = 22


def spread(times, scale=1.0):
    t = np.asarray(times, np.float64) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[ctx_commands_bench] ' + msg, file=sys.stderr, flush=True)


def digest(table, data):
    """Over what both routes promise: every record field but byte_off (the host machine packs its bytes, the tracked commands give a
    slot per frame) and every record's plaintext bytes."""
    h = hashlib.sha256()
    for f in FIELDS:
        h.update(np.ascontiguousarray(table[f]).tobytes())
    off, n = table['byte_off'].astype(np.int64), table['n_bytes'].astype(np.int64)
    idx = np.repeat(off - np.r_[0, np.cumsum(n)[:-1]], n) + np.arange(int(n.sum()))
    h.update(np.ascontiguousarray(data[idx]).tobytes())
    return h.hexdigest()


def workload(name):
    """-> (interleaved float32 IQ, samples, the context's parameters)"""
    from usrp_nfc_amd import synth
    if name == 'all':
        n = 100_000_000
        return synth.workload('all', n), n, dict(samp_rate=2e6, hi_val=1.1)
    if name in ('classic', 'never'):
        import bench
        n = bench.TILE
        return bench.make_capture_slice('classic1k', n, 0, 1)[1], n, bench.stream_params('classic1k')
    n = 20_000_000
    prefix = synth.frames_from_trace(os.path.join(ROOT, 'tests', 'golden', '1k_with_enc.out'))[0][:24]
    head = synth.modulation_profile(prefix, lead_in=3000, tail=0)
    m = np.ones(n, np.float32)
    m[:len(head)] = head
    period = synth.modulation_profile(synth.txn_frames(), lead_in=0, tail=0)
    body = n - len(head)
    m[len(head):] = np.tile(period, -(-body // len(period)))[:body]
    return synth.iq_from_profile(m), n, dict(samp_rate=2e6, hi_val=1.1)


def leg(name, repeats):
    from usrp_nfc_amd import api, fsm
    iq, n, params = workload(name)
    note('%s: workload generated' % name)
    buf = api.DeviceBuffer(iq)
    del iq
    plain = api.NfcContext(input_kind=api.NFC_IN_IQ_F32, **params)
    tracked = api.NfcContext(input_kind=api.NFC_IN_IQ_F32, **params)
    tracked.track_commands()
    tracked.set_timing(1)
    m = fsm.fsm(out=open(os.devnull, 'w'))
    keys = WRONG_KEYS if name == 'never' else None
    info = []

    def run(which):
        ctx = plain if which == 'a' else tracked
        ctx.reset()   # (the same batch every time, from a fresh stream and a fresh machine)
        m.reset()
        if keys:
            m.set_keys(*keys)
            if which != 'a':
                ctx.set_keys(*keys)
        t0 = time.perf_counter()
        ctx.push_device(buf, n)
        t1 = time.perf_counter()
        if which == 'a':
            fr = ctx.frames()
            table, data = m.process_frames(fr, dispatch=False)
            link = 32 + sum(32 * len(fr.records[t]) + 2 * len(fr.bytes[t]) for t in (0, 1))
            extra = None
        else:
            cm = ctx.commands(copy=False)
            table, data = cm.table, cm.data
            link = cm.bytes_copied
            extra = (int(cm.cmd_mask(READT).sum()), int(cm.plain_crc_ok_mask().sum())) if which == 'c' else None
            info.append(dict(cm.counters, ms_kernels=cm.ms_kernels, ms_frames=cm.ms_frames, ms_merge=cm.ms_merge, ms_walk=cm.ms_walk,
                             ms_resolve=cm.ms_resolve))
        t2 = time.perf_counter()
        return dict(push=t1 - t0, after=t2 - t1, digest=digest(table, data), link=int(link), n=len(table), extra=extra)

    ra = run('a')   # warm-up, and the cross-check
    rb = run('b')
    rc = run('c')
    assert ra['digest'] == rb['digest'] == rc['digest'], 'the commands of leg A and leg B differ'
    note('%s: %d frames, digests equal; %s' % (name, ra['n'], info[-1]))
    del info[:]
    acc = {k: dict(push=[], after=[]) for k in 'abc'}
    for i in range(repeats):
        for which in ('abc', 'bca', 'cab')[i % 3]:
            r = run(which)
            assert r['digest'] == ra['digest']
            acc[which]['push'].append(r['push'])
            acc[which]['after'].append(r['after'])
    counters = {k: info[0][k] for k in ('n_segments', 'n_rerun_segments', 'n_rerun_frames', 'n_keydep_segments')}
    kernels = {k: spread([v[k] for v in info]) for k in ('ms_kernels', 'ms_frames', 'ms_merge', 'ms_walk', 'ms_resolve')}
    res = dict(leg=name, samples=n, frames=ra['n'], repeats=repeats, counters=counters,
               ms_after_the_push={k.upper(): spread(acc[k]['after'], 1e3) for k in 'abc'},
               ms_push={k.upper(): spread(acc[k]['push'], 1e3) for k in 'abc'},
               bytes_over_the_link=dict(A=ra['link'], B=rb['link']), kernels=kernels,
               us_resolve_per_segment=kernels['ms_resolve']['median'] * 1e3 / max(1, counters['n_segments']),
               us_resolve_per_rerun_frame=(kernels['ms_resolve']['median'] * 1e3 / counters['n_rerun_frames']) if counters['n_rerun_frames'] else None,
               us_host_per_frame=float(np.median(acc['a']['after'])) * 1e6 / max(1, ra['n']),
               a_median_over_b_median=float(np.median(acc['a']['after']) / np.median(acc['b']['after'])),
               a_over_b_with_the_push=float(np.median(np.add(acc['a']['after'], acc['a']['push'])) / np.median(np.add(acc['b']['after'], acc['b']['push']))),
               masks=rc['extra'], digest=ra['digest'])
    plain.close()
    tracked.close()
    buf.free()
    return res


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    if '--leg' in args:
        print(json.dumps(leg(args[args.index('--leg') + 1], max(1, repeats))))
        return 0
    out = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'ctx_commands_bench.json')
    results = []
    for name, limit in CONFIGS:   # every GPU step under its own time limit; the first failure ends the run
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg'] + name + ['--repeats', str(max(5, repeats))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
        if p.returncode != 0:
            print('ctx_commands_bench: %s ended with status %d: stopping' % (' '.join(cmd[4:]), p.returncode), file=sys.stderr)
            return p.returncode
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    rec = dict(what='IQ to commands for one long stream: frames() + process_frames on the host (A) against a tracked batch + commands() (B) and '
                    'B + the vectorised masks (C); same process, alternating; times are what follows the return of the push',
               workloads='all: synth.workload("all", 1e8); classic: one 1e8-sample tile of bench.py classic1k; worst: the Classic prefix cut off '
                         'in mid-session, then Ultralight transactions to 2e7 samples; never: classic with the wrong key A', results=results)
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
