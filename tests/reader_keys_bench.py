#!/usr/bin/env python3
"""Key recovery from reader pairs: the CPU twin on one core against the GPU, the two forms of the probe against each other, and the full
64-bit search as the yardstick, in the same process.  Kept under tests/ like keys_bench.py (not collected by pytest).

  pairs      N pairs of first authentications made with the project's own machine (tests/test_keys_host.py: crafted_trace) from
             fixed-seed keys, uids and nonces, two sessions per key; N = 1, 16, 256
  leg A      keys.host_recover_reader(pairs): nfc_host_recover_reader_keys, one core (at N = 256 on the first 16 pairs only)
  leg B      keys.recover_reader(pairs, timing=True): the STAGED probe and its verify launch (the default)
  leg C      keys.recover_reader(pairs, timing=True, verify_inline=True): every candidate verified by the lane that found it
  leg D      keys.recover(searched sessions WITH their genuine {at}, timing=True): the existing full search, the yardstick
  protocol   the legs alternate, the order reversing every repeat, one warm-up of B, C and D excluded, five repeats of each;
             min / median / max
  cross-check  the sha256 of the result records of A, B and C are equal (over the pairs all ran); every key of B, C and D is the one
             the sessions were made with
  records    us per pair for every leg, the ratios A / B, B / D and C / B, ms_count / ms_fill / ms_probe per leg (ms_probe of B holds
             the verify launch), scratch bytes, batches, launches, and at N = 256 the distribution of n_odd, n_even and n_joined

    python tests/reader_keys_bench.py [--out profiles/reader_keys_bench.json]"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 5
HOST_MAX = 16


def spread(v, scale=1.0):
    t = np.asarray(v, np.float64) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[reader_keys_bench] ' + msg, file=sys.stderr, flush=True)


def make_pairs(n):
    """-> (pairs without {at}, the searched sessions with it, the keys)"""
    from tests.test_keys_host import crafted_trace
    from tests.test_reader_keys_host import pair_of, reader_side
    from usrp_nfc_amd import _lib
    rng = np.random.RandomState(4343)
    want, pairs, full = [], [], []
    r4 = lambda: rng.randint(0, 256, 4).tolist()
    for i in range(n):
        key, uid = rng.randint(0, 256, 6).tolist(), r4()
        a, b = crafted_trace(key, 0x60 + (i & 1), uid, r4(), r4()), crafted_trace(key, 0x60 + (i & 1), uid, r4(), r4())
        pairs.append(pair_of(reader_side(a), reader_side(b)))
        full.append(a)
        want.append(key)
    return np.array(pairs, _lib.READER_PAIR_DTYPE), np.array(full, _lib.AUTH_DTYPE), want


def main():
    from usrp_nfc_amd import keys
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    pairs, full, want = make_pairs(256)
    keys.recover_reader(pairs[:1])   # warm-up: the module load and the first launches
    keys.recover_reader(pairs[:1], verify_inline=True)
    keys.recover(full[:1])
    res = dict(repeats=REPEATS, configs=[])
    for n in (1, 16, 256):
        p, f, nh = pairs[:n], full[:n], min(n, HOST_MAX)
        t = dict(A=[], B=[], C=[], D=[])
        ks = dict(B=[], C=[], D=[])
        out, stats = {}, {}
        for rep in range(REPEATS):
            for leg in ('ABCD' if rep % 2 == 0 else 'DCBA'):
                t0 = time.perf_counter()
                if leg == 'A':
                    out[leg], _ = keys.host_recover_reader(p[:nh])
                    t[leg].append((time.perf_counter() - t0) / nh)
                    continue
                if leg == 'D':
                    out[leg], st = keys.recover(f, timing=True)
                else:
                    out[leg], st = keys.recover_reader(p, timing=True, verify_inline=(leg == 'C'))
                t[leg].append((time.perf_counter() - t0) / n)
                ks[leg].append((st.ms_count, st.ms_fill, st.ms_probe, st.ms_kernels))
                stats[leg] = st
            note('N %d repeat %d: twin %.0f, staged %.0f, in-lane %.0f, full search %.0f us per pair' % ((n, rep) + tuple(t[l][-1] * 1e6 for l in 'ABCD')))
        digest = {l: hashlib.sha256(out[l][:nh].tobytes()).hexdigest() for l in 'ABC'}
        assert digest['A'] == digest['B'] == digest['C'], 'the twin and the two GPU forms differ'
        assert out['B'].tobytes() == out['C'].tobytes(), 'the two GPU forms differ'
        for l in 'BCD':
            assert (out[l]['status'] == keys.NFC_KEY_OK).all() and out[l]['key'].tolist() == want[:n], 'a key was not recovered (leg %s)' % l
        med = {l: float(np.median(t[l])) for l in 'ABCD'}
        cfg = dict(n=n, n_host=nh, us_per_pair={l: spread(t[l], 1e6) for l in 'ABCD'},
                   ratio_twin_over_staged=med['A'] / med['B'], ratio_staged_over_full_search=med['B'] / med['D'], ratio_inline_over_staged=med['C'] / med['B'],
                   digest=digest['B'])
        for l, name in (('B', 'staged'), ('C', 'inline'), ('D', 'full_search')):
            k, st = np.array(ks[l]), stats[l]
            cfg[name] = dict(ms_count=spread(k[:, 0]), ms_fill=spread(k[:, 1]), ms_probe=spread(k[:, 2]), ms_kernels=spread(k[:, 3]),
                             scratch_bytes=int(st.scratch_bytes), n_batches=int(st.n_batches), n_grown=int(st.n_grown), n_launches=int(st.n_launches))
        if n == 256:
            for name in ('n_odd', 'n_even', 'n_joined'):
                v = out['B'][name]
                cfg[name] = dict(min=int(v.min()), median=float(np.median(v)), max=int(v.max()))
        res['configs'].append(cfg)
        print(json.dumps(cfg), flush=True)
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
