#!/usr/bin/env python3
"""Generate tests/golden/emu_reference.npz (not fx_*: the suite takes every fx_*.npz for a decoder case, tests/golden_util.py) by driving the reference's OWN emulators (tag.Tag, reader.Reader, behind its fsm where that matters).

Runs only where the reference tree exists; the test-suite never executes it -- it reads the file it wrote (tests/test_emulate_host.py).
The reference's modules are translated IN MEMORY by the machinery of make_fsm_golden.py (lib2to3, Python 2 division), with `tag`, `reader`
and `rand` added and `miller` (GNU Radio blocks the emulators import and never use) stubbed; the translated text is written nowhere.
The file holds inputs' seeds and recorded outputs alone.

THE FILE
  loop_text_1k / loop_text_ul     what the closed loop of usrp_nfc.py:116-136 (restated here: it lives in a GNU Radio top block) prints on the
                                  two card files for two rounds, utf-8
  replay_tag / replay_reader      the trace's frames of the other side played to the reference's Tag / Reader behind its fsm: per answer
                                  the bits it handed its callback, packed; *_off their offsets in bits, *_src the index of the heard frame
  rows (tests/emu_cards.py makes the cards and scripts from the seed): row_role (0 tag / 1 reader), row_seed, row_raise (the step at
  which the reference raised, -1 none), step_off; per step ans_cmd (command index, -1 none), ans_off / ans_bytes (its whole frame) and
  step_print (bit 0 ERROR WITH ONES, 1 TWOS, 2 THREES, 3 "ERROR, Unexpected command!!")

    python3 tests/golden/make_emu_golden.py      # rewrites tests/golden/emu_reference.npz"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, 'emu_reference.npz')

spec = importlib.util.spec_from_file_location('make_fsm_golden', os.path.join(HERE, 'make_fsm_golden.py'))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)   # (imports the reference's fsm, command, cipher, lfsr, utilities, packets, translated)
G.gate()


class _More(G._Finder):
    NAMES = ('rand', 'tag', 'reader')

    def find_spec(self, name, path=None, target=None):
        return importlib.util.spec_from_loader(name, self) if name in self.NAMES else None


sys.modules['miller'] = types.SimpleNamespace(miller_encoder=None)
_finder = _More()
sys.meta_path.insert(0, _finder)
try:
    import rand as _rand, reader as _reader, tag as _tag   # noqa: E401,F401
finally:
    sys.meta_path.remove(_finder)
R = dict(G.R, tag=_tag, reader=_reader)
CT, CS = R['command'].CommandType, R['command'].CommandStructure
INDEX = {id(getattr(CT, n)): i for i, n in enumerate(G.REF_COMMANDS)}

from tests import emu_cards   # noqa: E402
from usrp_nfc_amd import synth   # noqa: E402


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cards(name):
    ar = json.load(open(os.path.join(HERE, 'fx_emu_%s.json' % name)))
    t = next(d for d in ar if d['entry'] == 'tag')
    r = next((d for d in ar if d['entry'] == 'reader'), {})
    return t, r


def make(name, tag_cb=None, reader_cb=None):
    t, r = cards(name)
    null = lambda *a: None
    tag = R['tag'].Tag(tag_cb or null, R['command'].TagType.ULTRALIGHT if t.get('type') == 'ULTRALIGHT' else R['command'].TagType.CLASSIC1K,
                       list(t['mem']), [list(x) for x in t.get('rands', [])])
    reader = R['reader'].Reader(reader_cb or null, [list(x) for x in r.get('rands', [])] or [[1, 2, 3, 4]], r.get('keya', []), r.get('keyb', []))
    return tag, reader


def loop_text(name, rounds):
    tag, reader = make(name)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cmd = CT.REQA
        struct = CS.encode_command(cmd, [])
        s, ns, i = tag, reader, 0
        while i < rounds:
            ret = s.process_packet(cmd, struct)
            if not ret:
                cmd = CT.REQA
                struct = CS.encode_command(cmd, [])
                s, ns = tag, reader
                s.wake_up()
                i += 1
            else:
                cmd, struct = ret
                s, ns = ns, s
    return G.norm(buf.getvalue())


def replay(role):
    frames, _ = synth.frames_from_trace(os.path.join(HERE, '1k_with_enc.out'))
    sent = []
    tag, reader = make('classic1k', lambda bits: sent.append(list(bits)), lambda bits, finished=False: sent.append(list(bits)))
    emu = tag if role == 0 else reader
    m = R['fsm'].fsm(emu.process_packet)
    emu.set_encoder(m.process_outgoing)
    src, out = [], []
    with quiet():
        for i, (t, bits) in enumerate(frames[:199]):
            if t == role:
                continue
            n0 = len(sent)
            m.process_bits(list(bits) + [0] if len(bits) == 7 else list(bits), t)
            if len(sent) > n0:
                src.append(i)
                out.append([int(b) for b in sent[-1]])
    return src, out


def play(emu, steps):
    """-> per step (answer index or -1, its bytes, print bits), the step at which the reference raised"""
    res, raised = [], -1
    for k, (name, extra) in enumerate(steps):
        cmd = getattr(CT, name) if name else None
        struct = CS.encode_command(cmd, list(extra))
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                ret = emu.process_packet(cmd, struct)
        except Exception:
            raised = k
            break
        text = buf.getvalue()
        prints = sum(1 << b for b, s in enumerate(('ERROR WITH ONES', 'ERROR WITH TWOS', 'ERROR WITH THREES', 'ERROR, Unexpected command!!')) if s in text)
        res.append((INDEX[id(ret[0])], [int(b) for b in ret[1].all_bytes()], prints) if ret else (-1, [], prints))
    return res, raised


def main():
    z = {}
    for key, name in (('loop_text_1k', 'classic1k'), ('loop_text_ul', 'ultralight')):
        z[key] = np.frombuffer(loop_text(name, 2).encode('utf-8'), np.uint8)
    for role, key in ((0, 'replay_tag'), (1, 'replay_reader')):
        src, out = replay(role)
        z[key] = np.packbits(np.array([b for o in out for b in o], np.uint8))
        z[key + '_off'] = np.cumsum([0] + [len(o) for o in out]).astype(np.uint32)
        z[key + '_src'] = np.array(src, np.uint16)
        print('%s: %d answers' % (key, len(out)))
    rows = []
    null = lambda *a: None
    TT = R['command'].TagType
    for seed in range(emu_cards.N_TAG_ROWS):
        tag_type, mem, rands, steps = emu_cards.tag_row(seed)
        with quiet():
            emu = R['tag'].Tag(null, TT.ULTRALIGHT if tag_type == 0 else TT.CLASSIC1K, list(mem), [list(r) for r in rands])
        rows.append((0, seed, steps) + play(emu, steps))
    for seed in range(emu_cards.N_READER_ROWS):
        rands, steps = emu_cards.reader_row(seed)
        with quiet():
            emu = R['reader'].Reader(null, [list(r) for r in rands], [], [])
        rows.append((1, seed, steps) + play(emu, steps))
    # how many rows exercise each quirk
    name_of = lambda row, k: row[2][k][0]
    count = dict(
        authb=sum(any(name_of(r, k) == 'AUTHB' and a[0] >= 0 for k, a in enumerate(r[3])) for r in rows if r[0] == 0),
        read_refused=sum(any(name_of(r, k) == 'READR' and a[0] < 0 for k, a in enumerate(r[3])) for r in rows if r[0] == 0),
        read_answered=sum(any(a[0] == 22 for a in r[3]) for r in rows if r[0] == 0),
        trailer_read=sum(any(a[0] == 22 and r[2][k][1][0] % 4 == 3 for k, a in enumerate(r[3])) for r in rows if r[0] == 0 and r[2][0][0]),
        complement_print=sum(any(a[2] & 7 for a in r[3]) for r in rows),
        raised_tag=sum(r[4] >= 0 for r in rows if r[0] == 0), raised_reader=sum(r[4] >= 0 for r in rows if r[0] == 1),
        after_halt=sum(any(name_of(r, k) == 'REQA' and a[0] < 0 for k, a in enumerate(r[3])) for r in rows if r[0] == 0),
        reader_halt=sum(any(a[0] == 23 for a in r[3]) for r in rows if r[0] == 1),
    )
    print('rows per quirk: %s' % json.dumps(count))
    # ("ERROR, Unexpected command!!" is not among them: every tag-to-reader command of the table has a branch in reader.py:69-143, and
    # a frame that is no command raises before it: the print cannot be reached, and no row shows it)
    assert not any(a[2] & 8 for r in rows for a in r[3])
    assert all(v > 0 for v in count.values()), count
    z['row_role'] = np.array([r[0] for r in rows], np.uint8)
    z['row_seed'] = np.array([r[1] for r in rows], np.uint32)
    z['row_raise'] = np.array([r[4] for r in rows], np.int16)
    z['step_off'] = np.cumsum([0] + [len(r[3]) for r in rows]).astype(np.uint32)
    ans = [a for r in rows for a in r[3]]
    z['ans_cmd'] = np.array([a[0] for a in ans], np.int8)
    z['ans_off'] = np.cumsum([0] + [len(a[1]) for a in ans]).astype(np.uint32)
    z['ans_bytes'] = np.array([b for a in ans for b in a[1]], np.uint8)
    z['step_print'] = np.array([a[2] for a in ans], np.uint8)
    tmp = OUT + '.tmp'
    with zipfile.ZipFile(tmp, 'w', zipfile.ZIP_DEFLATED) as f:
        for name in sorted(z):
            info = zipfile.ZipInfo(name + '.npy', (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with f.open(info, 'w') as member:
                np.lib.format.write_array(member, np.asanyarray(z[name]), allow_pickle=False)
    os.replace(tmp, OUT)
    print('%s: %d bytes, %d rows, %d steps' % (os.path.basename(OUT), os.path.getsize(OUT), len(rows), len(ans)))


if __name__ == '__main__':
    main()
