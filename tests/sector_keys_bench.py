#!/usr/bin/env python3
"""What a per-sector key table costs a tracked push: the same multi-key card with the two keys alone and with a table per
stream, in the same process.  Kept under tests/ like commands_bench.py (not collected by pytest).

  captures   K copies of card 1 of tests/test_sector_keys_host.py (AUTHA 4 under K0, nested AUTHA 8 under K1, nested AUTHB 12 under K2,
             nested AUTHA 5 under K0, a READ after each; 26 frames, 41 164 complex samples, fc32), as overlapping ranges of one device
             buffer; K = 1 024, 16 384
  leg A      reset, set_keys(K0, K2), a tracked push, fetch_commands() -- in a context that never sets a sector key (no table buffer)
  leg B      the same with every stream's table set (one broadcast after the reset, outside the timed part)
             per leg: the push's wall time up to the end of its three launches (the read of one machine's state waits for them), the three
             launches' and the machine kernel's time by HIP events, the READ answers with a good plaintext CRC per card, and the bytes of
             the table buffer (640 per stream, from the layout: the context has no allocation counter)
  protocol   the legs alternate, the order flipping every repeat, one warm-up of each excluded, `repeats` (>= 5) of each; min / median / max
  cross-check  per leg the record fields of every stream's commands are those of stream 0, and stream 0's are the CPU twin's
               (fsm.host_commands with the same keys and table) on its raw frames (sha256)
  --parent TREE   a checkout of the parent commit with its library built: after every K, leg A alone (it needs nothing new) runs from that
                  tree in a child process, and this tree's median ms_machine of A is reported against the parent's min .. max

    python tests/sector_keys_bench.py [--repeats N] [--parent TREE] [--out profiles/sector_keys_bench.json]
                          every K, each in a child process under its own time limit; stops at the first failure
    python tests/sector_keys_bench.py --leg K --iq FILE [--only-a] [--tree TREE] [--repeats N]      one K, one JSON line"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1024, 200), (16384, 400)]   # (K, seconds allowed per child)
FIELDS = ['cmd', 'type', 'n_bytes', 'n_header', 'n_extra', 'n_crc', 'flags', 'n_enc']
READT = 22
TABLE_BYTES_PER_STREAM = 640


def spread(times, scale=1.0):
    t = np.asarray(times) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[sector_keys_bench] ' + msg, file=sys.stderr, flush=True)


def digest(table):
    h = hashlib.sha256()
    for name in FIELDS:
        h.update(np.ascontiguousarray(table[name]).tobytes())
    return h.hexdigest()


def leg(K, repeats, iq, card, only_a):
    """card: dict(k0, k2, table) -- the two keys and the (key_type, sector) -> key table as lists."""
    from usrp_nfc_amd import api, fsm
    N = len(iq) // 2
    buf = api.DeviceBuffer(iq)
    first, n = np.zeros(K, np.uint64), np.full(K, N, np.uint32)
    table = {(int(t), int(s)): k for t, s, k in card['table']}
    legs = ('a',) if only_a else ('a', 'b')
    ctx = {name: api.NfcMultiContext(K, N, samp_rate=2e6, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) for name in legs}
    for m in ctx.values():
        m.set_timing(True)
        m.track_commands(True)

    def run(name):
        m = ctx[name]
        m.reset()
        m.set_keys(card['k0'], card['k2'])
        if name == 'b':
            m.set_sector_keys(table)
        t0 = time.perf_counter()
        m.push_device(buf, first, n)
        m.fsm_state(0)   # (a tracked push returns with its three launches enqueued: reading one machine waits for them)
        t_push = time.perf_counter() - t0
        cm = m.fetch_commands(copy=False)
        return t_push, cm

    want_reads = dict(a=None, b=4)
    digests, reads = {}, {}
    for name in legs:   # warm-up, and the cross-check
        _, cm = run(name)
        t = cm.cmd
        per = len(t) // K
        assert len(t) == per * K and per == 26, 'another number of commands than 26 per card'
        rows = np.stack([np.ascontiguousarray(t[f]).reshape(K, per) for f in FIELDS])
        assert (rows == rows[:, :1, :]).all(), 'the streams of leg %s differ' % name.upper()
        digests[name] = digest(t[:per])
        if not only_a:   # (the twin with a table is this tree's)
            st = fsm.state_init()
            st.key_a[:], st.key_b[:] = card['k0'], card['k2']
            twin = fsm.host_commands(st, cm.raw.frames_of(0), sector_keys=table if name == 'b' else None)[0]
            assert digest(twin) == digests[name], 'leg %s is not its CPU twin' % name.upper()
        reads[name] = int(((t['cmd'] == READT) & (t['n_crc'] == 2)).sum()) // K
        assert want_reads[name] in (None, reads[name]), 'leg %s reads %d of 4 blocks' % (name.upper(), reads[name])
        note('K = %d leg %s: %d commands, %d of 4 READ answers in plaintext, cross-check passed' % (K, name.upper(), len(t), reads[name]))
        del cm, t, rows
    acc = {name: dict(push=[], kernels=[], machine=[]) for name in legs}
    for i in range(repeats):
        for name in (legs if i % 2 == 0 else legs[::-1]):
            t_push, cm = run(name)
            acc[name]['push'].append(t_push * 1e3)
            acc[name]['kernels'].append(cm.ms_kernels)
            acc[name]['machine'].append(cm.ms_machine)
    res = dict(K=K, samples_per_capture=N, repeats=repeats, digest=digests, reads_in_plaintext_of_4=reads,
               table_bytes={name: (TABLE_BYTES_PER_STREAM * K if name == 'b' else 0) for name in legs},
               ms_push={name.upper(): spread(acc[name]['push']) for name in legs},
               ms_kernels={name.upper(): spread(acc[name]['kernels']) for name in legs},
               ms_machine={name.upper(): spread(acc[name]['machine']) for name in legs})
    for m in ctx.values():
        m.close()
    buf.free()
    return res


def child(K, limit, repeats, iq_path, tree=None):
    cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg', str(K), '--iq', iq_path, '--repeats', str(repeats)]
    if tree:
        cmd += ['--only-a', '--tree', os.path.abspath(tree)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
    if p.returncode != 0:
        print('sector_keys_bench: %s ended with status %d: stopping' % (' '.join(cmd[4:]), p.returncode), file=sys.stderr)
        return None, p.returncode
    return json.loads(p.stdout.decode().strip().splitlines()[-1]), 0


def main():
    args = sys.argv[1:]
    opt = lambda name, default=None: args[args.index(name) + 1] if name in args else default
    repeats = int(opt('--repeats', 5))
    if '--leg' in args:
        sys.path.insert(0, opt('--tree', ROOT))   # (the package of that tree; nothing of tests/ is imported here)
        with np.load(opt('--iq'), allow_pickle=False) as z:
            iq = z['iq']
            card = dict(k0=z['k0'].tolist(), k2=z['k2'].tolist(), table=[(int(r[0]), int(r[1]), r[2:].tolist()) for r in z['table']])
        print(json.dumps(leg(int(opt('--leg')), max(1, repeats), iq, card, '--only-a' in args)))
        return 0
    sys.path.insert(0, ROOT)
    from tests.test_sector_keys_host import K0, K2, TABLE_1, card
    from usrp_nfc_amd import synth
    out = opt('--out', os.path.join(ROOT, 'profiles', 'sector_keys_bench.json'))
    parent = opt('--parent')
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        iq_path = os.path.join(tmp, 'card1.npz')
        np.savez(iq_path, iq=synth.iq_from_profile(synth.modulation_profile(card(1)[0])), k0=np.array(K0), k2=np.array(K2),
                 table=np.array([[t, s] + list(k) for (t, s), k in sorted(TABLE_1.items())]))
        for K, limit in CONFIGS:   # every GPU step under its own time limit; the first failure ends the run
            r, rc = child(K, limit, max(5, repeats), iq_path)
            if rc:
                return rc
            if parent:
                p, rc = child(K, limit, max(5, repeats), iq_path, tree=parent)
                if rc:
                    return rc
                pa, a = p['ms_machine']['A'], r['ms_machine']['A']['median']
                r['parent_A'] = dict(ms_machine=pa, ms_push=p['ms_push']['A'], digest=p['digest']['a'],
                                     this_tree_median_inside_parent_min_max=bool(pa['min'] <= a <= pa['max']))
                assert p['digest']['a'] == r['digest']['a'], 'leg A of the parent gives other commands'
            results.append(r)
            print(json.dumps(r), flush=True)
    rec = dict(what='a tracked push + fetch_commands() of K copies of a card whose sectors have different keys: with set_keys alone (A, no table '
                    'buffer) against every stream holding the sector key table (B); same process, alternating; parent_A: leg A from a checkout '
                    'of the parent commit, in a child process of the same call',
               workload='K copies of card 1 of tests/test_sector_keys_host.py rendered at 2 Msps (41 164 complex samples, 26 frames)', results=results)
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
