#!/usr/bin/env python3
"""Many short captures: a loop over one NfcContext against one push of an NfcMultiContext, in the same call.
Kept under tests/ like record_bench.py (not collected by pytest).

  workload   K captures of 32 768 samples, synth.workload('all', 32768, seed=k), resident in ONE device buffer; fc32 for
             K = 64, 1 024, 16 384 and sc8 for K = 16 384
  leg A      the single-stream way: one NfcContext; per capture reset(), push_device() at its offset, counts()
  leg B      one push_device() of an NfcMultiContext over all K captures, then every stream's counts
  both once more with the packets of every capture read to the host
  protocol   A and B alternate in the same process, warm-up excluded, `repeats` (>= 5) of each; per leg the min / median / max of the
             wall time per capture and of Msamples/s; B's kernel time by HIP events (ms_kernels); the device-side bytes per sample
  acceptance B's slowest repeat is faster than A's fastest repeat (non-overlapping ranges within one call) at K = 1 024 and 16 384;
             at K = 64 whatever comes out is reported
  cross-check  A's and B's counts are equal for every capture, and the packets of 64 sampled captures digest equally: a fast wrong
             answer cannot be reported

    python tests/multi_bench.py [--repeats N] [--out profiles/multi_bench.json]     every configuration, each in a child process
                                                                                   under its own time limit; stops at the first failure
    python tests/multi_bench.py --leg K KIND [--repeats N]                         one configuration, one JSON line"""
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

N = 32768
CONFIGS = [(64, 'fc32', 240), (1024, 'fc32', 300), (16384, 'fc32', 560), (16384, 'sc8', 560)]   # (K, kind, seconds allowed)
PARAMS = dict(samp_rate=2e6, hi_val=1.1)


def digest(packets):
    h = hashlib.sha256()
    for t, bits in packets:
        h.update(bytes([t, 255]) + bytes(bits) + b'\xfe')
    return h.hexdigest()


def spread(times, K):
    t = np.asarray(times)
    return dict(us_per_capture=dict(min=float(t.min() / K * 1e6), median=float(np.median(t) / K * 1e6), max=float(t.max() / K * 1e6)),
                msamples_s=dict(min=float(K * N / t.max() / 1e6), median=float(K * N / np.median(t) / 1e6), max=float(K * N / t.min() / 1e6)),
                seconds=[float(v) for v in t])


def capture(job):
    from usrp_nfc_amd import synth
    k, kind_name = job
    iq = synth.workload('all', N, seed=k)
    return iq if kind_name == 'fc32' else synth.quantise_sc8(iq)


def leg(K, kind_name, repeats):
    from usrp_nfc_amd import _lib, api
    kind = {'fc32': api.NFC_IN_IQ_F32, 'sc8': api.NFC_IN_IQ_I8}[kind_name]
    per, bps = 2, {'fc32': 8, 'sc8': 2}[kind_name]
    dt = np.float32 if kind_name == 'fc32' else np.int8
    flat = np.empty(K * N * per, dt)
    # (the captures are generated on the host before the GPU is opened, in a few worker processes that never open it)
    workers = max(1, min(16, int(os.environ.get('OMP_NUM_THREADS', '8'))))
    with multiprocessing.get_context('fork').Pool(workers) as pool:
        for k, x in enumerate(pool.imap(capture, [(k, kind_name) for k in range(K)], chunksize=16)):
            flat[k * N * per:(k + 1) * N * per] = x
    buf = api.DeviceBuffer(flat)
    del flat
    first = np.arange(K, dtype=np.uint64) * N
    n = np.full(K, N, np.uint32)
    L = _lib.load()
    ctx = api.NfcContext(input_kind=kind, **PARAMS)
    multi = api.NfcMultiContext(K, N, input_kind=kind, **PARAMS)
    multi.set_timing(True)
    cnt, flg = _lib.Counts(), C.c_uint32(0)

    def run_a(with_packets):
        out, pk = [], []
        t0 = time.perf_counter()
        for k in range(K):
            ctx.reset()
            ctx.push_device(buf.ptr.value + k * N * bps, N)
            c = ctx.counts()
            out.append((int(c.n_edges), int(c.n_symbols[0]), int(c.n_symbols[1]), int(c.n_packets[0]), int(c.n_packets[1])))
            if with_packets:
                pk.append(ctx.packets())
        return time.perf_counter() - t0, out, pk

    def run_b(with_packets):
        out, pk = [], []
        t0 = time.perf_counter()
        multi.reset()
        multi.push_device(buf, first, n)
        for k in range(K):
            rc = L.nfc_multi_get_counts(multi.h, k, C.byref(cnt), C.byref(flg))
            assert rc == 0 and flg.value == 0, (k, rc, flg.value)
            out.append((int(cnt.n_edges), int(cnt.n_symbols[0]), int(cnt.n_symbols[1]), int(cnt.n_packets[0]), int(cnt.n_packets[1])))
            if with_packets:
                pk.append(multi.stream(k).packets())
        return time.perf_counter() - t0, out, pk

    # warm-up (buffers sized, kernels loaded), and the cross-check
    _, ca, pa = run_a(True)
    _, cb, pb = run_b(True)
    assert ca == cb, 'the counts of the two legs differ'
    sample = sorted(np.random.default_rng(5).choice(K, min(64, K), replace=False).tolist())
    assert [digest(pa[k]) for k in sample] == [digest(pb[k]) for k in sample], 'the packets of the two legs differ'
    n_packets = sum(len(p) for p in pb)
    del pa, pb
    acc = {k: [] for k in ('a_counts', 'b_counts', 'a_packets', 'b_packets')}
    ms_kernels = []
    for i in range(repeats):
        order = ['a_counts', 'b_counts', 'a_packets', 'b_packets']
        for name in (order if i % 2 == 0 else order[::-1]):   # (alternating, and the order flips every repeat)
            t, c, _ = (run_a if name[0] == 'a' else run_b)(name.endswith('packets'))
            assert c == ca
            acc[name].append(t)
            if name == 'b_counts':
                ms_kernels.append(float(multi.stats().ms_kernels))
    st = multi.stats()
    res = dict(K=K, kind=kind_name, samples_per_capture=N, repeats=repeats, packets_total=n_packets, streams_truncated=int(st.n_streams_truncated),
               launches_per_push=int(st.n_launches), legs={k: spread(v, K) for k, v in acc.items()},
               ms_kernels=dict(min=min(ms_kernels), median=float(np.median(ms_kernels)), max=max(ms_kernels)),
               kernel_msamples_s=float(K * N / (np.median(ms_kernels) * 1e-3) / 1e6),
               # input once, the window slot read and (an accepted sample) written once, 6 bytes per entry and a byte per symbol / bit
               device_bytes_per_sample=dict(input=bps, window_read=4, window_write_at_most=4,
                                            outputs=float(sum(6 * c[0] + c[1] + c[2] for c in ca)) / (K * N)))
    for what in ('counts', 'packets'):
        a, b = acc['a_' + what], acc['b_' + what]
        res['ratio_' + what] = dict(a_fastest_over_b_slowest=float(min(a) / max(b)), a_median_over_b_median=float(np.median(a) / np.median(b)))
    res['b_slowest_beats_a_fastest'] = bool(max(acc['b_counts']) < min(acc['a_counts']) and max(acc['b_packets']) < min(acc['a_packets']))
    ctx.close()
    multi.close()
    buf.free()
    return res


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    if '--leg' in args:
        i = args.index('--leg')
        print(json.dumps(leg(int(args[i + 1]), args[i + 2], max(1, repeats))))
        return 0
    out = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'multi_bench.json')
    results = []
    for K, kind, limit in CONFIGS:   # every GPU step under its own time limit; the first failure ends the run
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg', str(K), kind, '--repeats', str(max(5, repeats))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
        if p.returncode != 0:
            print('multi_bench: %s ended with status %d: stopping' % (' '.join(cmd[4:]), p.returncode), file=sys.stderr)
            return p.returncode
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    ok = all(r['b_slowest_beats_a_fastest'] for r in results if r['K'] >= 1024)
    rec = dict(what='one NfcContext looped over K captures (A) against one push of an NfcMultiContext (B), same process, alternating',
               workload="synth.workload('all', 32768, seed=k)", acceptance_b_slowest_beats_a_fastest_from_1024_streams=ok,
               box=os.uname().nodename, results=results)
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
