#!/usr/bin/env python3
"""What rebuilding the cards on the GPU saves: K DIFFERENT Classic 1K cards read whole, their captures resident in HBM.
Kept under tests/ like commands_bench.py (not collected by pytest).

  captures   K cards of random memory and keys, each read whole by a reader that holds its key A table (emulate.pairs_device, 199 frames),
             rendered on the GPU to complex int8 at 2 Msps with no noise (Transcripts.render_device) into one device buffer; K = 1 024, 16 384
  leg A      a tracked push, fetch_commands(), the CPU twin (emulate.host_card_image) per stream on one core
  leg B      a tracked push with images, fetch_images()
             per leg: wall time from the push to the images on the host, and the bytes copied device -> host
  protocol   the legs alternate in one process, the order flipping every repeat, one warm-up of each excluded, `repeats` (>= 5) of each;
             min / median / max
  cross-check  every image of leg B equals leg A's twin image (sha256 over mem, src, info and tail of all streams), and holds the card
  kernels    with timing on: k_multi_images alone beside the machine kernel, by HIP events (medians)

    python tests/images_bench.py [--repeats N] [--only K] [--out profiles/images_bench.json]     every K (or one), each in a child process under its own limit
    python tests/images_bench.py --leg K [--repeats N]                                one K, one JSON line"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1024, 300), (16384, 600)]   # (K, seconds allowed per child)
FF = (0xFF,) * 6


def spread(times, scale=1.0):
    t = np.asarray(times) * scale
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()))


def note(msg):
    print('[images_bench] ' + msg, file=sys.stderr, flush=True)


def leg(K, repeats):
    sys.path.insert(0, ROOT)
    from tests import image_util as iu
    from usrp_nfc_amd import api, emulate
    mems = [iu.classic_mem(1000 + k) for k in range(K)]
    for m in mems:   # (a first UID byte of 0x88 is the cascade tag: such a card is not a single-size Classic)
        if m[0] == 0x88:
            m[0], m[4] = 0x89, m[4] ^ 0x01
    tables = [iu.key_a_table(m) for m in mems]
    tags = [emulate.tag_card(1, m, emulate.drawn_rands(k % 16)) for k, m in enumerate(mems)]
    readers = [emulate.reader_card(emulate.drawn_rands(100 + k % 16), table=t) for k, t in enumerate(tables)]
    trs = emulate.pairs_device(tags, readers)
    assert int(trs.results['n_frames'].min()) == 199 == int(trs.results['n_frames'].max())
    caps = trs.render_device(out_kind=api.NFC_IN_IQ_I8, sigma=0.0)
    N = int(caps.n_samples.max())
    note('K = %d: %d cards read and rendered, %d .. %d samples each, %.1f MiB of captures' %
         (K, K, int(caps.n_samples.min()), N, caps.used_samples * 2 / 2.0 ** 20))
    ctx = {}
    for name in ('a', 'b'):
        m = ctx[name] = api.NfcMultiContext(K, N, samp_rate=2e6, hi_val=1.1, input_kind=api.NFC_IN_IQ_I8)
        m.set_timing(True)
        m.track_commands(True)
        if name == 'b':
            m.track_images(True)

    def setup(m):
        m.reset()
        for k in range(K):
            m.set_sector_keys(tables[k], stream=k)

    def digest_images(recs):
        h = hashlib.sha256()
        for r in recs:
            h.update(r)
        return h.hexdigest()

    def run(name):
        m = ctx[name]
        setup(m)
        m.fsm_state(0)   # (the set-up is complete before the clock starts)
        t0 = time.perf_counter()
        caps.push_to(m)
        if name == 'a':
            cm = m.fetch_commands(copy=False)
            imgs = [emulate.host_card_image(*cm.commands_of(k)[:2], keys=(FF, FF, tables[k])) for k in range(K)]
            dt = time.perf_counter() - t0
            return dt, int(cm.bytes_copied), cm.ms_machine, 0.0, digest_images(i.rec.tobytes() for i in imgs), imgs
        im = m.fetch_images(copy=False)
        dt = time.perf_counter() - t0
        cm = m.fetch_commands(copy=False)   # (outside the clock: the machine kernel's time)
        return dt, int(im.bytes_copied), cm.ms_machine, im.ms_kernel, digest_images(im.image(k).rec.tobytes() for k in range(K)), im

    digests = {}
    for name in ('a', 'b'):   # warm-up, and the cross-check
        out = run(name)
        digests[name] = out[4]
        if name == 'b':
            im = out[5]
            assert im.n_known.tolist() == [1024] * K and im.flags.tolist() == [0] * K
            assert all(im.mem(k).tobytes() == mems[k].tobytes() for k in range(K)), 'an image is not its card'
    assert digests['a'] == digests['b'], 'the images of the GPU are not the twin\'s'
    note('K = %d: cross-check passed, every card rebuilt whole' % K)
    acc = {name: dict(wall=[], bytes=[], machine=[], images=[]) for name in ('a', 'b')}
    for i in range(repeats):
        for name in (('a', 'b') if i % 2 == 0 else ('b', 'a')):
            dt, nbytes, ms_machine, ms_images, dg, _ = run(name)
            assert dg == digests['a']
            acc[name]['wall'].append(dt * 1e3), acc[name]['bytes'].append(nbytes), acc[name]['machine'].append(ms_machine), acc[name]['images'].append(ms_images)
    a, b = np.median(acc['a']['wall']), np.median(acc['b']['wall'])
    res = dict(K=K, frames_per_card=199, samples_per_capture=N, repeats=repeats, digest=digests['a'],
               ms_wall={n.upper(): spread(acc[n]['wall']) for n in acc}, bytes_copied={n.upper(): int(acc[n]['bytes'][0]) for n in acc},
               ms_machine_kernel={n.upper(): spread(acc[n]['machine']) for n in acc}, ms_k_multi_images=spread(acc['b']['images']),
               us_per_card={'A': float(a) * 1e3 / K, 'B': float(b) * 1e3 / K}, verdict='B wins' if b < a else 'B LOSES')
    for m in ctx.values():
        m.close()
    caps.free()
    return res


def main():
    args = sys.argv[1:]
    opt = lambda name, default=None: args[args.index(name) + 1] if name in args else default
    repeats = max(5, int(opt('--repeats', 5)))
    if '--leg' in args:
        print(json.dumps(leg(int(opt('--leg')), repeats)))
        return 0
    out = opt('--out', os.path.join(ROOT, 'profiles', 'images_bench.json'))
    results = []
    only = opt('--only')
    for K, limit in [c for c in CONFIGS if only is None or c[0] == int(only)]:   # every GPU step under its own time limit; the first failure ends the run
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg', str(K), '--repeats', str(repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
        if p.returncode != 0:
            print('images_bench: %s ended with status %d: stopping' % (' '.join(cmd[4:]), p.returncode), file=sys.stderr)
            break
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    rec = dict(what='K different Classic 1K cards read whole, captures resident in HBM: a tracked push + fetch_commands() + the CPU twin per stream on '
                    'one core (A) against a tracked push with images + fetch_images() (B); same process, alternating; wall time from the push to '
                    'the images on the host',
               workload='K cards of random memory and keys, 199 frames each, rendered at 2 Msps to complex int8 without noise', results=results)
    if results:
        with open(out, 'w') as fh:
            json.dump(rec, fh, indent=1)
            fh.write('\n')
    return 0 if results and (only is not None or len(results) == len(CONFIGS)) else 1


if __name__ == '__main__':
    sys.exit(main())
