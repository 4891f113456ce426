#!/usr/bin/env python3
"""Packets to frames: the host's bit-by-bit way against the frames assembled on the GPU, in the same process.
Kept under tests/ like multi_fetch_bench.py (not collected by pytest).

  single     one batch of 1e8 samples of synth.workload('all'), resident in HBM, pushed anew from a reset context before every timed leg (the packet
             tables and the frames of a batch are built once and kept: a second read of the same batch would time a memcpy)
    leg A    packet_table + packet_bits of both types, then process_packets(dispatch=False)
    leg B    frames(), then process_frames(dispatch=False)
             wall time per batch of each leg, the bytes each brings over the link, and -- from the test build, with
             nfc_set_timing(1) -- the two frame kernels' time by HIP events
  multi      the captures of multi_fetch_bench.py (K captures of 32 768 samples, fc32), one push
    leg D    fetch(PACKETS) + packets_all()          (the best there was)
    leg F    fetch_frames() + crc_ok_mask()
             microseconds per capture, bytes copied, kernel time by HIP events
  protocol   the legs alternate, the order flipping every repeat, warm-up excluded, `repeats` (>= 5) of each; min / median / max
  cross-check  single: the frame tables and bytes of A and B are equal (sha256); multi: per stream the frames of F carry the
             n_bits of D's packets, and F's frames with a good CRC_A are those a host CRC over D's bits finds (64 sampled captures)

    python tests/frames_bench.py [--repeats N] [--out profiles/frames_bench.json]     every configuration, each in a child process
                                                                            under its own time limit; stops at the first failure
    python tests/frames_bench.py --leg single | --leg multi K [--repeats N]           one configuration, one JSON line"""
import ctypes as C
import hashlib
import json
import multiprocessing
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.multi_bench import N, PARAMS, capture   # noqa: E402  (the same workload)

N_SINGLE = 100_000_000
CONFIGS = [(['single'], 420), (['multi', '1024'], 300), (['multi', '16384'], 560)]   # (leg, seconds allowed)


def spread(times, scale=1.0):
    t = np.asarray(times) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[frames_bench] ' + msg, file=sys.stderr, flush=True)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def merged_packets(tabs):
    t = np.concatenate(tabs)
    return t[np.argsort(t['idx'], kind='stable')]


def leg_single(repeats):
    from usrp_nfc_amd import _lib, api, fsm, synth
    iq = synth.workload('all', N_SINGLE)
    note('single: workload generated')
    buf = api.DeviceBuffer(iq)
    del iq
    ctx = api.NfcContext(input_kind=api.NFC_IN_IQ_F32, **PARAMS)
    m = fsm.fsm(out=open(os.devnull, 'w'))

    def run(which):
        ctx.reset()   # (the same batch every time: a stream carried on would start each push from another state)
        ctx.push_device(buf, N_SINGLE)
        m.reset()
        t0 = time.perf_counter()
        if which == 'a':
            tabs = [ctx.packet_table(t) for t in (0, 1)]
            bits = [ctx.packet_bits(t) for t in (0, 1)]
            table, data = m.process_packets(merged_packets(tabs), bits[0], bits[1], dispatch=False)
            link = sum(12 * len(tabs[t]) + 4 * ((len(bits[t]) + 31) // 32) for t in (0, 1))
        else:
            fr = ctx.frames()
            table, data = m.process_frames(fr, dispatch=False)
            link = 32 + sum(32 * len(fr.records[t]) + 2 * len(fr.bytes[t]) for t in (0, 1))
        return time.perf_counter() - t0, sha(table, data), link, len(table)

    _, da, link_a, n_frames = run('a')   # warm-up, and the cross-check
    _, db, link_b, _ = run('b')
    assert da == db, 'the frame tables of leg A and leg B differ'
    note('single: %d frames, digests equal' % n_frames)
    acc = dict(a=[], b=[])
    for i in range(repeats):
        for name in (('a', 'b') if i % 2 == 0 else ('b', 'a')):
            t, d, _, _ = run(name)
            assert d == da
            acc[name].append(t)
    ctx.close()
    # the two kernels by HIP events: the test build keeps the figure (nfc_debug_frames_ms)
    hooks = _lib.hooks_path()
    ctx = api.NfcContext(input_kind=api.NFC_IN_IQ_F32, lib_path=hooks, **PARAMS)
    ctx.L.nfc_debug_frames_ms.restype = C.c_float
    ctx.L.nfc_debug_frames_ms.argtypes = [C.c_void_p]
    ctx.set_timing(1)
    ms = []
    for i in range(repeats + 1):
        ctx.push_device(buf, N_SINGLE)
        ctx.frame_counts()
        ms.append(float(ctx.L.nfc_debug_frames_ms(ctx.h)))
    ctx.close()
    buf.free()
    return dict(leg='single', samples=N_SINGLE, frames=n_frames, repeats=repeats, ms_per_batch=dict(A=spread(acc['a'], 1e3), B=spread(acc['b'], 1e3)),
                bytes_over_the_link=dict(A=int(link_a), B=int(link_b)), ms_frame_kernels=spread(ms[1:]),
                a_median_over_b_median=float(np.median(acc['a']) / np.median(acc['b'])), digest=da)


def leg_multi(K, repeats):
    from usrp_nfc_amd import api, fsm
    flat = np.empty(K * N * 2, np.float32)
    workers = max(1, min(16, int(os.environ.get('OMP_NUM_THREADS', '8'))))
    with multiprocessing.get_context('fork').Pool(workers) as pool:   # (generated before the GPU is opened, by processes that never open it)
        for k, x in enumerate(pool.imap(capture, [(k, 'fc32') for k in range(K)], chunksize=16)):
            flat[k * N * 2:(k + 1) * N * 2] = x
            if k % 2048 == 2047:
                note('multi: %d captures generated' % (k + 1))
    buf = api.DeviceBuffer(flat)
    del flat
    first = np.arange(K, dtype=np.uint64) * N
    n = np.full(K, N, np.uint32)
    multi = api.NfcMultiContext(K, N, input_kind=api.NFC_IN_IQ_F32, **PARAMS)
    multi.set_timing(True)
    info = dict(d=[], f=[])

    def run(which):
        multi.reset()
        multi.push_device(buf, first, n)
        t0 = time.perf_counter()
        if which == 'd':
            f = multi.fetch(api.NFC_MULTI_FETCH_PACKETS, copy=False)
            out = f.packets_all()
        else:
            f = multi.fetch_frames(copy=False)
            out = (f, f.crc_ok_mask())
        t = time.perf_counter() - t0
        info[which].append((f.ms_kernels, f.bytes_copied))
        assert int(multi.stats().n_reads_device) == 0
        return t, out

    # warm-up, and the cross-check on 64 sampled captures
    _, pk = run('d')
    _, (fr, mask) = run('f')
    sample = sorted(np.random.default_rng(5).choice(K, min(64, K), replace=False).tolist())
    n_frames = sum(len(a) for a in fr.frames)
    assert n_frames == sum(len(p) for p in pk)
    for k in sample:
        got = fr.frames_of(k)
        assert got.table['n_bits'].tolist() == [len(b) for _, b in pk[k]] and got.table['type'].tolist() == [t for t, _ in pk[k]]
        want = []
        for t, b in pk[k]:   # a host CRC over the packets' bits, for whole frames (n_bits % 9 == 0) with good parity
            a = np.array(b[:len(b) - len(b) % 9], np.uint8).reshape(-1, 9)
            data = (a[:, :8].astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=1).astype(np.uint8)
            par_ok = len(a) > 0 and len(b) % 9 in (0, 1) and not ((a[:, :8].sum(axis=1) & 1) == a[:, 8]).any()
            want.append(bool(par_ok and len(data) >= 2 and fsm.crc_a(data[:-2]) == data[-2:].tolist()))
        if all(len(b) % 9 in (0, 1) for _, b in pk[k]):
            assert got.crc_ok_mask().tolist() == want, 'stream %d: CRC verdicts differ from the host\'s' % k
    n_crc_ok = int(sum(int(a.sum()) for a in mask))
    note('multi: %d frames, %d with a good CRC_A, cross-check done' % (n_frames, n_crc_ok))
    del pk, fr, mask
    for v in info.values():
        del v[:]
    acc = dict(d=[], f=[])
    for i in range(repeats):
        for name in (('d', 'f') if i % 2 == 0 else ('f', 'd')):
            t, _ = run(name)
            acc[name].append(t)
    res = dict(leg='multi', K=K, samples_per_capture=N, repeats=repeats, frames_total=n_frames, frames_crc_ok=n_crc_ok,
               us_per_capture=dict(D=spread(acc['d'], 1e6 / K), F=spread(acc['f'], 1e6 / K)),
               bytes_copied=dict(D=int(info['d'][0][1]), F=int(info['f'][0][1])),
               ms_kernels=dict(D=spread([v[0] for v in info['d']]), F=spread([v[0] for v in info['f']])),
               d_median_over_f_median=float(np.median(acc['d']) / np.median(acc['f'])))
    multi.close()
    buf.free()
    return res


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    if '--leg' in args:
        i = args.index('--leg')
        res = leg_single(max(1, repeats)) if args[i + 1] == 'single' else leg_multi(int(args[i + 2]), max(1, repeats))
        print(json.dumps(res))
        return 0
    out = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'frames_bench.json')
    results = []
    for leg, limit in CONFIGS:   # every GPU step under its own time limit; the first failure ends the run
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg'] + leg + ['--repeats', str(max(5, repeats))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
        if p.returncode != 0:
            print('frames_bench: %s ended with status %d: stopping' % (' '.join(cmd[4:]), p.returncode), file=sys.stderr)
            return p.returncode
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    rec = dict(what='closed packets to frames: packet tables + bits + process_packets (A) against frames() + process_frames (B) on one 1e8-sample '
                    'batch; fetch(PACKETS) + packets_all() (D) against fetch_frames() + crc_ok_mask() (F) on K captures; same process, alternating',
               workload="single: synth.workload('all', 1e8); multi: synth.workload('all', 32768, seed=k)", results=results)
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
