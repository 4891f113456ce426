#!/usr/bin/env python3
"""Reading a multi-stream push back: stream by stream from the device against one fetch, in the same call.
Kept under tests/ like multi_bench.py (not collected by pytest), with multi_bench.py's workloads.

  workload   K captures of 32 768 samples, synth.workload('all', 32768, seed=k), resident in ONE device buffer; fc32 for
             K = 64, 1 024, 16 384 and sc8 for K = 16 384
  leg A      the single-stream way: one NfcContext; per capture reset(), push_device() at its offset, packets()
  leg B      one push_device() of an NfcMultiContext, then every stream's packets() read from the device -- no fetch: the path
             there was before the fetch
  leg C      push, fetch(PACKETS), every stream's packets() -- served from the host copy
  leg D      push, fetch(PACKETS), packets_all()
  leg E      push and fetch(ALL) alone
  protocol   the legs alternate in the same process, warm-up excluded, `repeats` (>= 5) of each, the order flipping every repeat;
             per leg the min / median / max of the wall time per capture.  The read cost per stream of B, C and D is the leg's time
             less the time of a push alone (leg P: reset, push, nothing read), per capture.
  per fetch  the two kernels' time by HIP events, bytes_copied, the copy's GB/s (the fetch call's wall time less the kernels, beside
             the link's 57 GB/s), and the share of the slabs' bytes -- what a blind copy of the slabs would move -- that was copied
  acceptance at K = 1 024 and 16 384: C's slowest repeat is faster than B's fastest (non-overlapping ranges within one call), and D
             is no slower than C (medians); at K = 64 whatever comes out is reported
  cross-check  the counts of A, B, C and D are equal for every capture and the packets of 64 sampled captures digest equally

    python tests/multi_fetch_bench.py [--repeats N] [--out profiles/multi_fetch_bench.json]   every configuration, each in a child
                                                                            process under its own time limit; stops at the first failure
    python tests/multi_fetch_bench.py --leg K KIND [--repeats N]            one configuration, one JSON line"""
import json
import multiprocessing
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.multi_bench import N, PARAMS, capture, digest   # noqa: E402  (the same workload and digest)

CONFIGS = [(64, 'fc32', 240), (1024, 'fc32', 300), (16384, 'fc32', 560), (16384, 'sc8', 560)]   # (K, kind, seconds allowed)
LINK_GBS = 57.0


def spread(times, K):
    t = np.asarray(times)
    return dict(us_per_capture=dict(min=float(t.min() / K * 1e6), median=float(np.median(t) / K * 1e6), max=float(t.max() / K * 1e6)),
                seconds=[float(v) for v in t])


def leg(K, kind_name, repeats):
    from usrp_nfc_amd import api
    kind = {'fc32': api.NFC_IN_IQ_F32, 'sc8': api.NFC_IN_IQ_I8}[kind_name]
    per, bps = 2, {'fc32': 8, 'sc8': 2}[kind_name]
    dt = np.float32 if kind_name == 'fc32' else np.int8
    flat = np.empty(K * N * per, dt)
    workers = max(1, min(16, int(os.environ.get('OMP_NUM_THREADS', '8'))))
    with multiprocessing.get_context('fork').Pool(workers) as pool:   # (generated before the GPU is opened, by processes that never open it)
        for k, x in enumerate(pool.imap(capture, [(k, kind_name) for k in range(K)], chunksize=16)):
            flat[k * N * per:(k + 1) * N * per] = x
    buf = api.DeviceBuffer(flat)
    del flat
    first = np.arange(K, dtype=np.uint64) * N
    n = np.full(K, N, np.uint32)
    ctx = api.NfcContext(input_kind=kind, **PARAMS)
    multi = api.NfcMultiContext(K, N, input_kind=kind, **PARAMS)
    multi.set_timing(True)
    fetches = dict(packets=[], all=[])

    def counts_of(ca):
        return [tuple(r) for r in np.stack([ca['n_edges'], ca['n_symbols'][:, 0], ca['n_symbols'][:, 1], ca['n_packets'][:, 0],
                                            ca['n_packets'][:, 1]], axis=1).tolist()]

    def run_a():
        out, pk = [], []
        t0 = time.perf_counter()
        for k in range(K):
            ctx.reset()
            ctx.push_device(buf.ptr.value + k * N * bps, N)
            c = ctx.counts()
            out.append((int(c.n_edges), int(c.n_symbols[0]), int(c.n_symbols[1]), int(c.n_packets[0]), int(c.n_packets[1])))
            pk.append(ctx.packets())
        return time.perf_counter() - t0, out, pk

    def timed_fetch(what, key):
        t0 = time.perf_counter()
        f = multi.fetch(what, copy=False)
        fetches[key].append((time.perf_counter() - t0, f.ms_kernels, f.bytes_copied))
        return f

    def run_multi(how):
        t0 = time.perf_counter()
        multi.reset()
        multi.push_device(buf, first, n)
        pk = None
        if how == 'b':
            pk = [multi.stream(k).packets() for k in range(K)]
        elif how == 'c':
            timed_fetch(api.NFC_MULTI_FETCH_PACKETS, 'packets')
            pk = [multi.stream(k).packets() for k in range(K)]
        elif how == 'd':
            pk = timed_fetch(api.NFC_MULTI_FETCH_PACKETS, 'packets').packets_all()
        elif how == 'e':
            timed_fetch(api.NFC_MULTI_FETCH_ALL, 'all')
        t = time.perf_counter() - t0
        st = multi.stats()
        if how == 'b':
            assert int(st.n_fetches) == 0 and int(st.n_reads_device) > 0
        elif how in 'cde':
            assert int(st.n_fetches) == 1 and int(st.n_reads_device) == 0, (how, int(st.n_fetches), int(st.n_reads_device))
        return t, counts_of(multi.counts_all()), pk

    # warm-up (buffers sized, kernels loaded), and the cross-check
    _, ca, pa = run_a()
    sample = sorted(np.random.default_rng(5).choice(K, min(64, K), replace=False).tolist())
    want = [digest(pa[k]) for k in sample]
    n_packets = sum(len(p) for p in pa)
    del pa
    for how in 'bcd':
        _, c, pk = run_multi(how)
        assert c == ca, 'the counts of leg %s differ from the single context\'s' % how.upper()
        assert [digest(pk[k]) for k in sample] == want, 'the packets of leg %s differ from the single context\'s' % how.upper()
        del pk
    run_multi('e')
    run_multi('p')
    assert not np.any(multi.counts_all()['flags'])
    for v in fetches.values():
        del v[:]
    acc = {k: [] for k in 'abcdep'}
    for i in range(repeats):
        order = ['a', 'b', 'c', 'd', 'e', 'p']
        for name in (order if i % 2 == 0 else order[::-1]):   # (alternating, and the order flips every repeat)
            t, c, _ = run_a() if name == 'a' else run_multi(name)
            assert c == ca
            acc[name].append(t)
    # what a blind copy of the slabs would move: every row at its capacity (the defaults of nfc_multi_create)
    cap = N // 4 + 64
    cap_pk = N // 16 + 16
    slab = dict(packets=K * 2 * (cap_pk * 8 + cap), all=K * (cap * 6 + 2 * cap + 2 * cap_pk * 8 + 2 * cap))

    def fetch_record(key):
        wall, ms, nbytes = (np.array(v, float) for v in zip(*fetches[key]))
        copy_s = np.maximum(wall - ms * 1e-3, 1e-9)
        return dict(fetches=len(wall), bytes_copied=int(nbytes[0]), ms_kernels=dict(min=float(ms.min()), median=float(np.median(ms)), max=float(ms.max())),
                    ms_fetch_call=dict(min=float(wall.min() * 1e3), median=float(np.median(wall) * 1e3), max=float(wall.max() * 1e3)),
                    copy_gb_s_call_less_kernels=float(np.median(nbytes / copy_s) / 1e9), link_gb_s=LINK_GBS,
                    kernels_gb_s=float(np.median(nbytes / (ms * 1e-3)) / 1e9), slab_bytes_of_a_blind_copy=int(slab[key]),
                    share_of_the_slab_bytes=float(nbytes[0] / slab[key]))

    med = {k: float(np.median(v)) for k, v in acc.items()}
    res = dict(K=K, kind=kind_name, samples_per_capture=N, repeats=repeats, packets_total=n_packets, legs={k.upper(): spread(v, K) for k, v in acc.items()},
               fetch_packets=fetch_record('packets'), fetch_all=fetch_record('all'),
               read_us_per_stream={k.upper(): (med[k] - med['p']) / K * 1e6 for k in 'bcd'},
               read_us_per_stream_single_context=(med['a'] / K * 1e6),
               ratio_a_over_b=med['a'] / med['b'], ratio_a_over_c=med['a'] / med['c'], ratio_a_over_d=med['a'] / med['d'],
               c_slowest_beats_b_fastest=bool(max(acc['c']) < min(acc['b'])), d_no_slower_than_c=bool(med['d'] <= med['c']),
               b_fastest_over_c_slowest=float(min(acc['b']) / max(acc['c'])), c_median_over_d_median=med['c'] / med['d'])
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
    out = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'multi_fetch_bench.json')
    results = []
    for K, kind, limit in CONFIGS:   # every GPU step under its own time limit; the first failure ends the run
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg', str(K), kind, '--repeats', str(max(5, repeats))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
        if p.returncode != 0:
            print('multi_fetch_bench: %s ended with status %d: stopping' % (' '.join(cmd[4:]), p.returncode), file=sys.stderr)
            return p.returncode
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    ok = all(r['c_slowest_beats_b_fastest'] and r['d_no_slower_than_c'] for r in results if r['K'] >= 1024)
    rec = dict(what='reading one push of an NfcMultiContext back: every stream\'s packets() from the device (B), after one fetch (C), '
                    'packets_all() of the fetch (D), push and fetch(ALL) alone (E), a push alone (P); A: one NfcContext looped over the captures; '
                    'same process, alternating', workload="synth.workload('all', 32768, seed=k)",
               acceptance_c_slowest_beats_b_fastest_and_d_no_slower_than_c_from_1024_streams=ok, results=results)
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
