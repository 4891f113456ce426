#!/usr/bin/env python3
"""Key recovery: the CPU twin on one core against the GPU, in the same process.  Kept under tests/ like commands_bench.py (not collected
by pytest).

  traces     N first authentications made with the project's own machine (tests/test_keys_host.py: crafted_trace) from fixed-seed keys,
             uids and nonces; N = 1, 16, 256
  leg A      keys.host_recover(traces): nfc_host_recover_keys, one core (at N = 256 on the first 16 traces only: it is per-trace work)
  leg B      keys.recover(traces, timing=True): nfc_recover_keys_device
  protocol   the legs alternate, the order flipping every repeat, one warm-up of B excluded, five repeats of each; min / median / max
  cross-check  the sha256 of the result records of A and B are equal (over the traces both ran), and every key is the one the trace was made with
  records    us per authentication for both legs and their ratio, ms_kernels split by kernel, scratch bytes, batches, and at N = 256 the
             distribution of n_odd and n_even (min / median / max)

    python tests/keys_bench.py [--out profiles/keys_bench.json]"""
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
    print('[keys_bench] ' + msg, file=sys.stderr, flush=True)


def make_traces(n):
    from tests.test_keys_host import crafted_trace
    from usrp_nfc_amd import _lib
    rng = np.random.RandomState(4242)
    want, out = [], []
    for i in range(n):
        key = rng.randint(0, 256, 6).tolist()
        out.append(crafted_trace(key, 0x60 + (i & 1), rng.randint(0, 256, 4).tolist(), rng.randint(0, 256, 4).tolist(), rng.randint(0, 256, 4).tolist()))
        want.append(key)
    return np.array(out, _lib.AUTH_DTYPE), want


def main():
    from usrp_nfc_amd import keys
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    traces, want = make_traces(256)
    keys.recover(traces[:1])   # warm-up: the module load and the first launches
    res = dict(repeats=REPEATS, configs=[])
    for n in (1, 16, 256):
        t, nh = traces[:n], min(n, HOST_MAX)
        ta, tb, ks = [], [], []
        for rep in range(REPEATS):
            for leg in ('AB' if rep % 2 == 0 else 'BA'):
                t0 = time.perf_counter()
                if leg == 'A':
                    ra, _ = keys.host_recover(t[:nh])
                    ta.append((time.perf_counter() - t0) / nh)
                else:
                    rb, st = keys.recover(t, timing=True)
                    tb.append((time.perf_counter() - t0) / n)
                    ks.append((st.ms_count, st.ms_fill, st.ms_probe, st.ms_kernels))
            note('N %d repeat %d: host %.0f us, gpu %.0f us per authentication' % (n, rep, ta[-1] * 1e6, tb[-1] * 1e6))
        da, db = hashlib.sha256(ra.tobytes()).hexdigest(), hashlib.sha256(rb[:nh].tobytes()).hexdigest()
        assert da == db, 'the twin and the GPU differ'
        assert (rb['status'] == keys.NFC_KEY_OK).all() and rb['key'].tolist() == want[:n], 'a key was not recovered'
        k = np.array(ks)
        cfg = dict(n=n, n_host=nh, host_us_per_auth=spread(ta, 1e6), gpu_us_per_auth=spread(tb, 1e6),
                   ratio_host_over_gpu=float(np.median(ta) / np.median(tb)), ms_count=spread(k[:, 0]), ms_fill=spread(k[:, 1]), ms_probe=spread(k[:, 2]),
                   ms_kernels=spread(k[:, 3]), scratch_bytes=int(st.scratch_bytes), n_batches=int(st.n_batches), n_grown=int(st.n_grown),
                   n_launches=int(st.n_launches), digest=db)
        if n == 256:
            cfg['n_odd'] = dict(min=int(rb['n_odd'].min()), median=float(np.median(rb['n_odd'])), max=int(rb['n_odd'].max()))
            cfg['n_even'] = dict(min=int(rb['n_even'].min()), median=float(np.median(rb['n_even'])), max=int(rb['n_even'].max()))
            sizes = [1 << int(2 * v - 1).bit_length() for v in rb['n_odd'].tolist()]
            cfg['table_slots'] = dict(max=int(max(sizes)), largest_16_consecutive=int(max(sum(sizes[i:i + 16]) for i in range(0, 256, 16))))
        res['configs'].append(cfg)
        print(json.dumps(cfg), flush=True)
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
