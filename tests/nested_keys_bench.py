#!/usr/bin/env python3
"""Key recovery from nested authentications: what one costs on the GPU against 64 first-authentication searches, the whole golden card
against one nested trace, the CPU twin against the GPU on one window, and the headline benchmark on this tree against the parent
commit's.  Kept under tests/ like keys_bench.py (not collected by pytest).

  traces     the fifteen nested authentications of tests/golden/1k_with_enc.out (keys.find_nested_auths), and 64 first authentications
             made with the project's own machine (tests/keys_bench.py: make_traces)
  leg F      keys.recover(64 first authentications): the baseline -- its time per authentication, times 64, is what one nested
             authentication would cost if a candidate were exactly one ordinary search
  leg N      keys.recover_nested(golden nested trace 0, timing=True): all 64 candidates
  leg C      keys.recover_nested(all fifteen, timing=True): the card
  leg T / G  keys.host_recover_nested / keys.recover_nested on the two-candidate window [32, 34) of golden nested trace 0
  protocol   F, N, C alternate in one process, the order flipping every repeat, one warm-up of each excluded, five repeats; T, G the
             same; min / median / max
  cross-check  the sha256 of the result records: N equals C's first record, T equals G, every repeat gives the same digest; every
             golden key is FF FF FF FF FF FF with one verified candidate
  headline   with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 100 --warmup 20 --no-cpu-baseline
             --no-extras` as a child process in this tree and in DIR, alternating, --bench-repeats times each (default 3)

    python tests/nested_keys_bench.py [--out profiles/nested_keys_bench.json] [--parent DIR] [--bench-repeats K]"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 5
BENCH = ['bench.py', '--gpus', '1', '--steps', '100', '--warmup', '20', '--no-cpu-baseline', '--no-extras']


def spread(v, scale=1.0):
    t = np.asarray(v, np.float64) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[nested_keys_bench] ' + msg, file=sys.stderr, flush=True)


def digest(r):
    return hashlib.sha256(r.tobytes()).hexdigest()


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def headline(tree):
    """One run of the headline benchmark in `tree`, a child process with its own library -> (Msamples/s, ms per step)."""
    env = dict(os.environ)
    env.pop('NFC_AMD_LIB', None)
    out = subprocess.run([sys.executable] + BENCH, cwd=tree, env=env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    line = json.loads([l for l in out.split('\n') if l.startswith('{')][-1])
    return float(line['value']), float(line['ms_per_step'])


def main():
    from tests.keys_bench import make_traces
    from tests.test_keys_host import reference_frames
    from usrp_nfc_amd import keys
    out_path, parent, bench_repeats = arg('--out'), arg('--parent'), int(arg('--bench-repeats', 3))
    firsts, want = make_traces(64)
    nested = keys.find_nested_auths(reference_frames())
    assert len(nested) == 15
    res = dict(repeats=REPEATS)

    # ---- F, N, C ----
    legs = dict(F=lambda: keys.recover(firsts, timing=True), N=lambda: keys.recover_nested(nested[:1], timing=True),
                C=lambda: keys.recover_nested(nested, timing=True))
    for f in legs.values():
        f()   # warm-up: the module load, the first launches, the scratch's first allocation
    t, ms, dig, last = {k: [] for k in legs}, {k: [] for k in legs}, {k: set() for k in legs}, {}
    for rep in range(REPEATS):
        for leg in ('FNC' if rep % 2 == 0 else 'CNF'):
            t0 = time.perf_counter()
            r, st = legs[leg]()
            t[leg].append(time.perf_counter() - t0)
            ms[leg].append((st.ms_count, st.ms_fill, st.ms_probe, st.ms_kernels))
            dig[leg].add(digest(r))
            last[leg] = (r, st)
        note('repeat %d: 64 firsts %.1f ms, one nested %.1f ms, the card %.1f ms' % (rep, t['F'][-1] * 1e3, t['N'][-1] * 1e3, t['C'][-1] * 1e3))
    assert all(len(d) == 1 for d in dig.values()), 'a repeat gave other results'
    rf, rn, rc = last['F'][0], last['N'][0], last['C'][0]
    assert (rf['status'] == keys.NFC_KEY_OK).all() and rf['key'].tolist() == want, 'a first key was not recovered'
    assert digest(rn) == digest(rc[:1]), 'one nested trace alone and in the card differ'
    assert (rc['status'] == keys.NFC_KEY_OK).all() and (rc['key'] == 0xFF).all() and (rc['n_verified'] == 1).all() and (rc['n_searched'] == 64).all()

    def leg_record(k, per):
        m = np.array(ms[k])
        st = last[k][1]
        return dict(ms_per_call=spread(t[k], 1e3), ms_per_unit=spread(t[k], 1e3 / per), ms_count=spread(m[:, 0]), ms_fill=spread(m[:, 1]),
                    ms_probe=spread(m[:, 2]), ms_kernels=spread(m[:, 3]), ms_candidates=spread(m[:, 3] - m[:, 0] - m[:, 1] - m[:, 2]),
                    n_batches=int(st.n_batches), n_launches=int(st.n_launches), n_grown=int(st.n_grown), scratch_bytes=int(st.scratch_bytes),
                    digest=sorted(dig[k])[0])

    res['firsts_64'] = leg_record('F', 64)       # per unit: per first authentication
    res['nested_1'] = leg_record('N', 1)         # per unit: per nested authentication
    res['card_15'] = leg_record('C', 15)
    base = np.median(t["F"])                     # 64 x the per-authentication time of the first-authentication leg: that leg is 64 of them
    res['nested_over_64_firsts'] = float(np.median(t['N']) / base)
    res['card_per_nested_over_one_nested'] = float(np.median(t['C']) / 15 / np.median(t['N']))
    res['n_odd_per_candidate'] = dict(nested_1=float(rn['n_odd'][0]) / 64, firsts_median=float(np.median(rf['n_odd'])))
    print(json.dumps({k: res[k] for k in ('nested_over_64_firsts', 'card_per_nested_over_one_nested')}), flush=True)

    # ---- T, G ----
    win = dict(cand_first=32, cand_count=2)
    tt, tg, dt = [], [], set()
    keys.recover_nested(nested[:1], **win)
    for rep in range(REPEATS):
        for leg in ('TG' if rep % 2 == 0 else 'GT'):
            t0 = time.perf_counter()
            r, _ = (keys.host_recover_nested if leg == 'T' else keys.recover_nested)(nested[:1], **win)
            (tt if leg == 'T' else tg).append(time.perf_counter() - t0)
            dt.add(digest(r))
        note('window repeat %d: twin %.0f ms, gpu %.1f ms' % (rep, tt[-1] * 1e3, tg[-1] * 1e3))
    assert len(dt) == 1, 'the twin and the GPU differ'
    res['window_2'] = dict(twin_ms=spread(tt, 1e3), gpu_ms=spread(tg, 1e3), ratio_twin_over_gpu=float(np.median(tt) / np.median(tg)), digest=sorted(dt)[0])
    print(json.dumps(res['window_2']), flush=True)

    # ---- the headline benchmark, this tree and the parent's ----
    if parent:
        runs = dict(this=[], parent=[])
        for rep in range(bench_repeats):
            for which in (('this', 'parent') if rep % 2 == 0 else ('parent', 'this')):
                runs[which].append(headline(ROOT if which == 'this' else parent))
                note('bench.py %s: %.1f Msamples/s, %.4f ms per step' % (which, runs[which][-1][0], runs[which][-1][1]))
        res['headline'] = {k: dict(msamples_per_s=spread([v[0] for v in r]), ms_per_step=spread([v[1] for v in r])) for k, r in runs.items()}
        res['headline']['this_over_parent'] = float(np.median([v[0] for v in runs['this']]) / np.median([v[0] for v in runs['parent']]))
        print(json.dumps(res['headline']), flush=True)
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
