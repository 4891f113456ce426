#!/usr/bin/env python3
"""Generate tests/golden/fx_fsm_fuzz.npz by driving the reference's OWN protocol machine (fsm.process_bits, fsm.process_outgoing) over
malformed frame sequences.

Runs only in the build container (needs /root/reference); the GPU box and the test-suite never execute it -- they read the file it
wrote (tests/test_fsm_fuzz.py).

IMPORT.  The reference's fsm, command, cipher, lfsr, utilities and packets are Python 2.  They are translated IN MEMORY -- lib2to3's
fixers, then every ast.Div rewritten to Python 2's division (floor for two ints) -- and exec'd into module objects through a finder
that lives for this run only.  The translated text is written nowhere; the fixture holds inputs and recorded outputs alone.

GATE.  The translated machine must print tests/golden/ultralight.out and 1k_with_enc.out from packets_from_trace exactly, with the one
normalisation `0X` -> `0x` (Python 2's format(v, '#04X') printed a lower-case prefix).  Otherwise nothing is written.

THE FILE (everything deduplicated: a frame or a text that occurs in many sequences is stored once).
  frame_type / frame_len / frame_off / frame_bits   the distinct frames: type, bit count, byte offset into the packed bits (np.packbits,
                                                    every frame starts on a byte)
  text_off / text_blob                              the distinct per-frame texts (utf-8), text 0 is ''
  seq_off                                           row r owns entries seq_off[r] .. seq_off[r + 1] of seq_frame / seq_text / seq_sess
  seq_frame / seq_text / seq_sess                   per frame: its frame id, the text the reference printed for it ('' from the frame at
                                                    which it raised on), whether the reference had a cipher installed when it arrived
  seq_raise                                         the index of the frame at which the reference raised, -1: none
  seq_keys                                          key A, key B (12 bytes)
  seq_family                                        FAMILIES index: what made the row
  seq_src / seq_seed                                GPU rows only (else -1 / 0): the row whose frames were rendered with
                                                    synth.iq_from_profile(synth.modulation_profile(frames), seed=seed) at 2 Msps and decoded
                                                    by oracle.c_oracle; the row's own frames are the oracle's packets
  n_seq / gpu_rows                                  rows 0 .. n_seq - 1 are the sequences, gpu_rows the 256 rendered ones behind them
  out_*                                             the outgoing route: scenarios of steps (heard: type, frame in; sent: command index,
                                                    frame in, frame out; the text the machine printed at the step, its callback silent),
                                                    out_raise the step at which the reference raised

    python3 tests/golden/make_fsm_golden.py      # rewrites tests/golden/fx_fsm_fuzz.npz, byte for byte the same"""
import ast
import contextlib
import importlib.abc
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

REF = '/root/reference/code'
REF_MODULES = ('fsm', 'command', 'cipher', 'lfsr', 'utilities', 'packets')
OUT = os.path.join(HERE, 'fx_fsm_fuzz.npz')
N_SEQ, N_GPU, MAX_SAMPLES, MAX_BYTES = 2000, 256, 48000, 385 * 1024
FAMILIES = ('probe', 'uid_len', 'no_session', 'nt_cut', 'nine_k_r', 'authb', 'nested_uid')
DIRECTED = (1, 2, 3, 4, 6)
GPU_RAISING = {1: 4, 2: 10, 3: 8, 4: 1, 6: 1, 0: 1, 5: 0}   # rows of the 256 on which the reference may raise, per family: 25 in all
FF = [0xFF] * 6
WRONG_KEYS = ([0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], FF)   # tests/test_commands_host.py
KEY_B = [0xB0, 0xB1, 0xB2, 0xB3, 0xB4, 0xB5]


# ---- the reference, translated in memory -----------------------------------------------------------------------------------------------
def _py2div(a, b):
    return a // b if isinstance(a, int) and isinstance(b, int) else a / b


class _Div(ast.NodeTransformer):
    def visit_BinOp(self, node):
        self.generic_visit(node)
        if isinstance(node.op, ast.Div):
            return ast.copy_location(ast.Call(ast.Name('_py2div', ast.Load()), [node.left, node.right], []), node)
        return node

    def visit_AugAssign(self, node):
        self.generic_visit(node)
        assert not isinstance(node.op, ast.Div), 'an augmented division: not translated'
        return node


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self):
        from lib2to3 import refactor
        self.tool = refactor.RefactoringTool(refactor.get_fixers_from_package('lib2to3.fixes'))

    def find_spec(self, name, path=None, target=None):
        return importlib.util.spec_from_loader(name, self) if name in REF_MODULES else None

    def exec_module(self, module):
        name = module.__name__
        src = open(os.path.join(REF, name + '.py')).read()
        tree = ast.fix_missing_locations(_Div().visit(ast.parse(str(self.tool.refactor_string(src, name)))))
        module.__dict__['_py2div'] = _py2div
        exec(compile(tree, '<reference %s, translated>' % name, 'exec'), module.__dict__)


def import_reference():
    assert not any(n in sys.modules for n in REF_MODULES)
    finder = _Finder()
    sys.meta_path.insert(0, finder)
    try:
        mods = [importlib.import_module(n) for n in REF_MODULES]
    finally:
        sys.meta_path.remove(finder)
    return dict(zip(REF_MODULES, mods))


R = import_reference()

from tests.test_frames import GOLD_1K, GOLD_UL, crafted_oracle_packets, packets_from_trace   # noqa: E402
from usrp_nfc_amd import synth   # noqa: E402

REF_COMMANDS = ['REQA', 'WUPA', 'ATQAUL', 'ATQA1K', 'ATQA4K', 'ATQADS', 'ANTI1R', 'ANTI1U', 'ANTI1G', 'SEL1R', 'SEL1U', 'SEL1K', 'ANTI2R', 'ANTI2T',
                'AUTHA', 'AUTHB', 'RANDTA', 'RANDRB', 'RANDTB', 'SEL2R', 'SEL2T', 'READR', 'READT', 'HALT', 'WRITE', 'COMPW1', 'COMPW2']   # csrc/protocol.h's order


def norm(text):
    return text.replace('0X', '0x')


def run_reference(packets, keys):
    """-> (texts per frame, in-session flags per frame, raise index)."""
    m = R['fsm'].fsm()
    m.set_keys(list(keys[0]), list(keys[1]))
    texts, sess, raised = [], [], -1
    for i, (t, bits) in enumerate(packets):
        sess.append(int(m._encryption is not None))
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                m.process_bits([int(b) for b in bits], int(t))
        except Exception:
            raised = i
            break
        texts.append(norm(buf.getvalue()))
    n = len(packets)
    return texts + [''] * (n - len(texts)), sess + [0] * (n - len(sess)), raised


def gate():
    for path in (GOLD_UL, GOLD_1K):
        packets, text = packets_from_trace(path)
        texts, _, raised = run_reference(packets, (FF, FF))
        assert raised == -1 and ''.join(texts).rstrip('\n') == text.rstrip('\n'), 'the translated machine does not print ' + path
    print('gate: the translated reference prints both golden traces')


# ---- sequences ---------------------------------------------------------------------------------------------------------------------------
def fb(data):
    return synth.frame_bits(list(data))


def crc(data):
    c = R['utilities'].CRC.calculate_crc(list(data))
    return list(data) + c


def mutate(rng, packets, n):
    p = [(t, list(b)) for t, b in packets]
    for _ in range(n):
        if not p:
            break
        op = int(rng.integers(0, 8))
        i = int(rng.integers(0, len(p)))
        t, b = p[i]
        if op == 0:     # a bit flipped
            b[int(rng.integers(0, len(b)))] ^= 1
        elif op == 1:   # a frame dropped
            del p[i]
        elif op == 2:   # doubled
            p.insert(i, (t, list(b)))
        elif op == 3:   # cut
            if len(b) > 1:
                p[i] = (t, b[:int(rng.integers(1, len(b)))])
        elif op == 4:   # lengthened
            p[i] = (t, b + rng.integers(0, 2, int(rng.integers(1, 13))).tolist())
        elif op == 5:   # its direction swapped
            p[i] = (1 - t, b)
        elif op == 6:   # a random frame inserted
            p.insert(i, (int(rng.integers(0, 2)), rng.integers(0, 2, int(rng.integers(1, 81))).tolist()))
        else:           # two frames exchanged
            j = int(rng.integers(0, len(p)))
            p[i], p[j] = p[j], p[i]
    return p


def resized(rng, bits, n):
    return bits[:n] if n <= len(bits) else bits + rng.integers(0, 2, n - len(bits)).tolist()


def build_sequences():
    rng = np.random.Generator(np.random.PCG64(0x14443A))
    classic = packets_from_trace(GOLD_1K)[0][:24]
    ul = packets_from_trace(GOLD_UL)[0]
    crafted = crafted_oracle_packets()
    keysets = [(FF, FF), WRONG_KEYS, (FF, KEY_B)]
    seqs = []   # (family, keys, packets)

    def add(family, keys, packets):
        seqs.append((family, keys, [(int(t), [int(x) for x in b]) for t, b in packets if len(b)]))   # (an empty packet is never handed over: packets.py:97)

    reqa, atqa1k, atqaul, anti1r, anti2r = classic[0], (0, fb([0x04, 0x00])), (0, fb([0x44, 0x00])), (1, fb([0x93, 0x20])), (1, fb([0x95, 0x20]))
    sel1k = classic[5]
    broken = lambda f: (f[0], f[1][:8] + [f[1][8] ^ 1] + f[1][9:])   # the first ninth bit wrong: a parity error

    # 1. a RANDTA arriving with a UID of 0, 3, 7 and 10 bytes: the anticollision is rewritten, the authentication and what follows stay
    u = [0x04, 0xBE, 0x6F, 0x5D, 0x22, 0x09, 0x29, 0x80]
    a1u = (0, fb([0x88] + u[:3] + [0x88 ^ u[0] ^ u[1] ^ u[2]]))
    a2t = (0, fb(u[3:7] + [u[3] ^ u[4] ^ u[5] ^ u[6]]))
    sel2r = (1, fb(crc([0x95, 0x70] + u[3:7] + [u[3] ^ u[4] ^ u[5] ^ u[6]])))
    heads = {
        0: [reqa, atqa1k, anti1r, broken(classic[3]), broken(classic[4]), sel1k],
        3: [reqa, atqa1k, anti1r, a1u, broken(classic[4]), sel1k],
        7: [reqa, atqa1k, anti1r, a1u, broken(classic[4]), sel1k, anti2r, a2t, sel2r, sel1k],
        10: [reqa, atqa1k, anti1r, a1u, broken(classic[4]), sel1k, anti2r, a2t, sel2r, a1u, sel1k],
    }
    heads['3u'] = [reqa, atqaul, anti1r, classic[3], classic[4], sel1k]   # an Ultralight's SEL1R keeps three of the four bytes
    for rep in range(6):
        for name, head in heads.items():
            for keys in keysets[:2] if rep % 2 else keysets[:1]:
                add(1, keys, mutate(rng, head + classic[6:], 0 if rep < 2 else 1))
    # 2. RANDRB / RANDTB with no session up
    for rep in range(12):
        nr = (1, fb(rng.integers(0, 256, 8).tolist()))
        at = (0, fb(rng.integers(0, 256, 4).tolist()))
        add(2, keysets[0], classic[:7] + [nr] + classic[8:12])                   # the tag nonce never came
        add(2, keysets[0], ul[:9] + [at] + ul[9:])                              # four tag bytes at stage 4
        add(2, keysets[rep % 3], mutate(rng, classic[:7] + [nr, at] + classic[10:], 1))
    # 3. an AUTH inside a session whose {nt} is cut to each length from 0 to 36 bits
    for keys in keysets[:2]:
        for n in range(37):
            add(3, keys, classic[:19] + [(0, classic[19][1][:n])] + classic[20:])
    for n in (0, 8, 9, 17, 18, 26, 27, 28, 34, 35, 36, 37, 44, 45):              # ... and lengthened behind the cut
        add(3, keysets[0], classic[:19] + [(0, resized(rng, classic[19][1][:min(n, 36)], n))] + classic[20:])
    # 4. frames of 9k + r bits for every r, in and out of a session
    for r in range(9):
        for k in (0, 1, 4, 8):
            n = 9 * k + r
            if n == 0:
                continue
            for i in (4, 6, 10, 13, 20):   # SEL1R, AUTHA, an encrypted READR, an encrypted READT, the nested {nr}{ar}
                add(4, keysets[(r + k + i) % 2], classic[:i] + [(classic[i][0], resized(rng, classic[i][1], n))] + classic[i + 1:])
            add(4, keysets[0], ul[:8] + [(ul[8][0], resized(rng, ul[8][1], n))] + ul[9:])
    # 6. a NESTED authentication under a UID that is not four bytes, in a session whose keystream is right: the on-air frames are made
    # with the reference's own cipher, so the AUTH decrypts and the reference returns.  Three bytes: the nonce register gets 24 bits, the
    # three plaintext bytes are a SEL2T, and a {nr}{ar} / {at} of ZEROS follows -- answers nothing may call right.  Seven bytes (an
    # encrypted ANTI1U makes the UID grow inside the session): 63 of the nested frame's bits are taken, twice; some rows end in a frame
    # shorter than the UID, where the reference raises.
    Cipher = R['cipher'].cipher
    par0 = lambda uid: [b for byte in uid for b in [(byte >> i) & 1 for i in range(8)] + [0]]
    plain_bits = lambda data: [(byte >> i) & 1 for byte in data for i in range(8)]

    def nested_nonce(key, uid, data, behind):
        """{nt} for the plaintext bytes `data` (as many as the UID has) under a fresh register keyed `key`, `behind` more bits on the air."""
        c = Cipher(list(key))
        pt, ub = fb(data), par0(uid)
        k = c.enc_bits([a ^ b for a, b in zip(pt, ub)], 1, 0, 1)
        return c, [a ^ b for a, b in zip(k, ub)] + list(behind)

    for rep in range(24):
        keys = keysets[rep % 3]
        nt, nr = rng.integers(0, 256, 4).tolist(), rng.integers(0, 256, 4).tolist()
        short = rep % 2 == 0
        uid = u[:3]
        head = [reqa, atqa1k, anti1r, a1u, broken(classic[4]), sel1k] if short else list(classic[:6])
        if not short:
            uid = [int(sum(b << i for i, b in enumerate(classic[3][1][9 * j:9 * j + 8]))) for j in range(4)]
        c = Cipher(list(keys[0]))
        c.set_tag_bits(plain_bits(uid), plain_bits(nt), 0)
        frames = head + [(1, fb(crc([0x60, 0x04]))), (0, fb(nt))]
        frames.append((1, c.enc_bits(fb(nr), 1) + c.enc_bits(fb(c.get_ar()))))
        frames.append((0, c.enc_bits(fb(c.get_at()))))
        if short:
            frames.append((1, c.enc_bits(fb(crc([0x61, 0x08])))))                                   # AUTHB, encrypted: key B from here
            c, nonce = nested_nonce(keys[1], uid, crc([0x00]), rng.integers(0, 2, 9).tolist())
            frames.append((0, nonce))
            frames.append((1, c.enc_bits(fb(nr + [0, 0, 0, 0]))))
            frames.append((0, c.enc_bits(fb([0, 0, 0, 0]))))
            frames.append((1, c.enc_bits(fb(crc([0x30, 0x08])))))
        else:
            more = rng.integers(0, 256, 3).tolist()
            frames.append((0, c.enc_bits(fb([0x88] + more + [0x88 ^ more[0] ^ more[1] ^ more[2]]))))   # ANTI1U, encrypted: the UID is seven bytes
            uid = uid + more
            frames.append((1, c.enc_bits(fb(crc([0x60, 0x08])))))
            for _ in range(2):
                c, nonce = nested_nonce(keys[0], uid, rng.integers(0, 256, 7).tolist(), rng.integers(0, 2, 9 + 9 * (rep % 3)).tolist())
                frames.append((0, nonce))
            if rep % 4 == 1:
                frames.append((1, rng.integers(0, 2, 36).tolist()))                               # shorter than the UID
        add(6, keys, frames)
    # 5. key A != key B with an AUTHB: the first authentication names key B, which is the card's
    authb = (1, fb(crc([0x61, 0x04])))
    for rep in range(150):
        add(5, (WRONG_KEYS[0], FF), mutate(rng, classic[:6] + [authb] + classic[7:], 0 if rep < 4 else int(rng.integers(1, 4))))
    # the crafted packets of test_frames.py: a window of them alone, and behind the start of a session
    for rep in range(150):
        at = int(rng.integers(0, len(crafted) - 14))
        win = crafted[at:at + 14]
        add(0, keysets[rep % 3], mutate(rng, win, int(rng.integers(0, 3))) if rep % 3 == 0 else mutate(rng, classic[:10 + rep % 3] + win[:10], int(rng.integers(0, 3))))
    # the probe's mix: one to three mutations of the Classic prefix or of the Ultralight transaction
    while len(seqs) < N_SEQ:
        i = len(seqs)
        base, keys = (ul, keysets[0]) if i % 5 == 0 else (classic, keysets[i % 3])
        add(0, keys, mutate(rng, base, int(rng.integers(1, 4))))
    return seqs[:N_SEQ]


# ---- the outgoing route ------------------------------------------------------------------------------------------------------------------
def build_outgoing():
    """Scenarios of an emulator in both roles over the plain frames of the Classic prefix: steps (kind, a, bits in, bits out), kind 0 a
    frame heard (a: its type), kind 1 a frame sent through process_outgoing (a: the command's index); the step at which the reference
    raised."""
    CT = R['command'].CommandType
    classic = packets_from_trace(GOLD_1K)[0][:24]
    seen = []
    monitor = R['fsm'].fsm(lambda cmd, st: seen.append((cmd, st)))
    with contextlib.redirect_stdout(io.StringIO()):
        for t, bits in classic:
            monitor.process_bits(list(bits), t)
    assert len(seen) == 24 and all(c is not None for c, _ in seen)
    plain = [(t, cmd, synth.frame_bits(st.all_bytes(), 7) + [0] if cmd.name() in ('REQA', 'WUPA') else synth.frame_bits(st.all_bytes()))
             for (t, _), (cmd, st) in zip(classic, seen)]
    index = {id(getattr(CT, n)): i for i, n in enumerate(REF_COMMANDS)}
    broken = lambda b: b[:8] + [b[8] ^ 1] + b[9:]
    u = [0x04, 0xBE, 0x6F, 0x5D]
    a1u = synth.frame_bits([0x88] + u[:3] + [0x88 ^ u[0] ^ u[1] ^ u[2]])
    a2t = synth.frame_bits([0x22, 0x09, 0x29, 0x80, 0x82])
    sel2r = synth.frame_bits([0x95, 0x70, 0x22, 0x09, 0x29, 0x80, 0x82, 0xD8, 0xBA])
    scenarios = []

    def run(role, edit):
        """edit(i, t, air, bits) -> a list of (t, air, cmd, bits) to play in place of frame i."""
        emu = R['fsm'].fsm(lambda cmd, st: None)
        steps, raised = [], -1
        for i, ((t, air), (_, cmd, bits)) in enumerate(zip(classic, plain)):
            for t2, air2, cmd2, bits2 in edit(i, t, list(air), list(bits), cmd):
                heard = t2 != role
                buf = io.StringIO()
                try:
                    with contextlib.redirect_stdout(buf):
                        if heard:
                            emu.process_bits(list(air2), t2)
                            step = (0, t2, list(air2), [])
                        else:
                            out = emu.process_outgoing(list(bits2), cmd2)
                            step = (1, index[id(cmd2)], list(bits2), [int(x) for x in out])
                    steps.append(step + (norm(buf.getvalue()),))   # what the machine printed with a silent callback: messages, ciphertext, AR / AT
                except Exception:
                    raised = len(steps)
                    steps.append(((0, t2, list(air2), []) if heard else (1, index[id(cmd2)], list(bits2), [])) + ('',))
                    break
            if raised >= 0:
                break
        scenarios.append((role, steps, raised))

    same = lambda i, t, air, bits, cmd: [(t, air, cmd, bits)]
    for role in (0, 1):
        run(role, same)
        # the UID the emulator holds when the tag nonce comes: the anticollision frames it HEARS are rewritten
        run(role, lambda i, t, air, bits, cmd: [(t, broken(air) if i in (3, 4) else air, cmd, bits)])                       # none
        run(role, lambda i, t, air, bits, cmd: [(t, a1u if i == 3 else broken(air) if i == 4 else air, cmd, bits)])         # three bytes (reader role)
        run(role, lambda i, t, air, bits, cmd: [(t, air, cmd, bits)] * (2 if i in (3, 4) else 1))                           # heard twice
        run(role, lambda i, t, air, bits, cmd: [(t, air, cmd, bits)] + ([(0, a2t, CT.ANTI2T, a2t), (1, sel2r, CT.SEL2R, sel2r)] if i == 4 else []))
        # the nonce frame cut (both authentications), with the prefix's UID and with none
        for at in (7, 19):
            for n in range(0, 37):
                if n in (0, 1, 8, 9, 10, 17, 18, 26, 27, 28, 34, 35, 36) or role == 0:
                    run(role, lambda i, t, air, bits, cmd, at=at, n=n: [(t, air[:n] if i == at else air, cmd, bits[:n] if i == at else bits)])
            for n in (9, 18, 27, 35, 36):
                run(role, lambda i, t, air, bits, cmd, at=at, n=n: [(t, broken(air) if i in (3, 4) else air[:n] if i == at else air, cmd, bits[:n] if i == at else bits)])
    return scenarios


# ---- packing -----------------------------------------------------------------------------------------------------------------------------
class Table(object):
    def __init__(self):
        self.frames, self.frame_id, self.texts, self.text_id = [], {}, [''], {'': 0}

    def frame(self, t, bits):
        key = (int(t), bytes(bytearray(bits)))
        if key not in self.frame_id:
            self.frame_id[key] = len(self.frames)
            self.frames.append((int(t), [int(b) for b in bits]))
        return self.frame_id[key]

    def text(self, s):
        if s not in self.text_id:
            self.text_id[s] = len(self.texts)
            self.texts.append(s)
        return self.text_id[s]

    def arrays(self):
        packed = [np.packbits(np.array(b, np.uint8)) for _, b in self.frames]
        blobs = [s.encode('utf-8') for s in self.texts]
        return dict(frame_type=np.array([t for t, _ in self.frames], np.uint8), frame_len=np.array([len(b) for _, b in self.frames], np.uint16),
                    frame_off=np.cumsum([0] + [len(p) for p in packed]).astype(np.uint32), frame_bits=np.concatenate(packed),
                    text_off=np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint32), text_blob=np.frombuffer(b''.join(blobs), np.uint8))


def main():
    gate()
    from oracle import c_oracle
    seqs = build_sequences()
    tab = Table()
    rows = []   # (family, keys, frame ids, text ids, sess, raised, src, seed)
    for family, keys, packets in seqs:
        texts, sess, raised = run_reference(packets, keys)
        rows.append((family, keys, [tab.frame(t, b) for t, b in packets], [tab.text(s) for s in texts], sess, raised, -1, 0))
    n_seq = len(rows)
    raising = sum(r[5] >= 0 for r in rows)
    print('%d sequences, the reference raised in %d; families %s' % (n_seq, raising, np.bincount([r[0] for r in rows], minlength=len(FAMILIES)).tolist()))

    # the GPU section: 256 sequences through the signal chain
    order = np.random.Generator(np.random.PCG64(256)).permutation(n_seq).tolist()
    order = [i for i in order if rows[i][0] in DIRECTED] + [i for i in order if rows[i][0] not in DIRECTED]   # the directed families first
    per_family = dict.fromkeys(range(len(FAMILIES)), 0)
    gpu, n_raise, raising_of = [], 0, dict.fromkeys(range(len(FAMILIES)), 0)
    for i in order:
        if len(gpu) == N_GPU:
            break
        family, keys, packets = seqs[i]
        if rows[i][0] in DIRECTED and per_family[family] >= 24:
            continue
        if not packets or (rows[i][5] >= 0 and raising_of[family] >= GPU_RAISING[family]):
            continue
        m = synth.modulation_profile(packets)
        if len(m) > MAX_SAMPLES:
            continue
        seed = 1000 + i
        o = c_oracle.COracle(hi_val=1.1)
        o.push_iq(synth.iq_from_profile(m, seed=seed))
        got = [(t, b) for t, b in o.packets() if b]
        o.close()
        texts, sess, raised = run_reference(got, keys)
        if raised >= 0 and raising_of[family] >= GPU_RAISING[family]:
            continue
        n_raise += int(raised >= 0)
        raising_of[family] += int(raised >= 0)
        per_family[family] += 1
        gpu.append(len(rows))
        rows.append((family, keys, [tab.frame(t, b) for t, b in got], [tab.text(s) for s in texts], sess, raised, i, seed))
    assert len(gpu) == N_GPU, len(gpu)
    print('GPU section: %d rows, the reference raised in %d; families %s' % (len(gpu), n_raise, [per_family[k] for k in range(len(FAMILIES))]))

    # the caps (conditions, re-asserted by tests/test_fsm_fuzz.py on the committed file)
    assert raising * 10 <= n_seq and n_raise * 10 <= N_GPU
    fam = np.bincount([r[0] for r in rows[:n_seq]], minlength=len(FAMILIES))
    assert all(fam[f] >= 8 and per_family[f] >= 8 for f in DIRECTED), (fam, per_family)   # in the sequences and in the 256
    seen = sum(len(r[2]) if r[5] < 0 else r[5] + 1 for r in rows[:n_seq])
    inside = sum(sum(r[4]) for r in rows[:n_seq])
    assert inside * 10 >= seen * 4, (inside, seen)
    print('frames the reference saw: %d, inside a session: %d (%.1f %%)' % (seen, inside, 100.0 * inside / seen))

    scen = build_outgoing()
    o_role, o_off, o_kind, o_a, o_in, o_out, o_raise, o_text = [], [0], [], [], [], [], [], []
    for role, steps, raised in scen:
        o_role.append(role)
        o_raise.append(raised)
        for kind, a, bits_in, bits_out, text in steps:
            o_text.append(tab.text(text))
            o_kind.append(kind)
            o_a.append(a)
            o_in.append(tab.frame(2 + kind, bits_in))      # (types 2 / 3: frames of the outgoing section, never a sequence's)
            o_out.append(tab.frame(4, bits_out))
        o_off.append(len(o_kind))
    print('outgoing route: %d scenarios, %d steps, the reference raised in %d' % (len(scen), len(o_kind), sum(r >= 0 for r in o_raise)))

    z = tab.arrays()
    z.update(seq_off=np.cumsum([0] + [len(r[2]) for r in rows]).astype(np.uint32),
             seq_frame=np.array([f for r in rows for f in r[2]], np.uint32), seq_text=np.array([t for r in rows for t in r[3]], np.uint32),
             seq_sess=np.array([s for r in rows for s in r[4]], np.uint8), seq_raise=np.array([r[5] for r in rows], np.int16),
             seq_keys=np.array([list(r[1][0]) + list(r[1][1]) for r in rows], np.uint8), seq_family=np.array([r[0] for r in rows], np.uint8),
             seq_src=np.array([r[6] for r in rows], np.int32), seq_seed=np.array([r[7] for r in rows], np.uint32),
             n_seq=np.array(n_seq, np.uint32), gpu_rows=np.array(gpu, np.uint32),
             out_role=np.array(o_role, np.uint8), out_off=np.array(o_off, np.uint32), out_kind=np.array(o_kind, np.uint8), out_a=np.array(o_a, np.uint8),
             out_in=np.array(o_in, np.uint32), out_text=np.array(o_text, np.uint32), out_out=np.array(o_out, np.uint32), out_raise=np.array(o_raise, np.int16))
    tmp = OUT + '.tmp'
    with zipfile.ZipFile(tmp, 'w', zipfile.ZIP_DEFLATED) as f:   # np.savez_compressed, with no clock in it: the same bytes every time
        for name in sorted(z):
            info = zipfile.ZipInfo(name + '.npy', (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with f.open(info, 'w') as member:
                np.lib.format.write_array(member, np.asanyarray(z[name]), allow_pickle=False)
    size = os.path.getsize(tmp)
    if size > MAX_BYTES:
        os.remove(tmp)
        raise SystemExit('%d bytes: larger than the largest fixture (%d); lower N_SEQ' % (size, MAX_BYTES))
    os.replace(tmp, OUT)
    print('%s: %d bytes, %d distinct frames, %d distinct texts' % (os.path.basename(OUT), size, len(tab.frames), len(tab.texts)))


if __name__ == '__main__':
    main()
