"""Commands for one long stream, a lane per transaction (csrc/ctx_commands.hip.h), on the CPU: nfc_host_commands_segmented -- the cuts,
the speculative walks and the resolve in the very text the kernels run -- against nfc_host_commands_keyed, the sequential twin, and
the host machine on the same raw frames.  Every comparison is for equality: the records, data and enc byte for byte, the 88 bytes of
the state afterwards.  tests/test_ctx_commands.py holds the GPU half and imports the inputs and helpers below.

THE CUT PREDICATE is pinned by exhaustion (test_a_cut_frame_forgets_where_the_machine_was): a reader frame of one byte, 0x26 or 0x52,
parity good, heard with encrypted == 0, gives the same record from every state and leaves the same state but for cur_key, st, ar, at,
the flags and the keys, none of which it touches.

THE ROUTES.  (a) a session that ends with an encrypted HALT, then a transaction: every guess holds.  (b) the 24-frame Classic prefix,
cut off in mid-session, then three Ultralight transactions: their REQAs are ciphertext to the machine, every later segment is walked
again.  (c) a transaction that authenticates with key B of sector 3 under a table whose key A differs, a HALT, then REQA, ATQA,
anticollision, SELECT, SAK, a 4-byte tag frame and an 8-byte reader frame: the tag frame is RANDTA by stage, no AUTH in its segment, and
the register it loads is keyed by the cur_key the transaction BEFORE left.  (d) a frame with NFC_RAW_CUT, which the twin accepts as
nfc_host_commands does -- a single context never makes one: its frames are assembled from bit arrays that are never truncated.
(e) a list without a cut, and an empty list."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests.golden_util import GOLDEN, Case
from tests.test_commands_host import (WRONG_KEYS, assert_commands_equal, classic_packets, host_machine, prefix_frames, run_host,
                                      state_bytes)
from tests.test_frames import GOLDEN_CASES, host_frames_of
from tests.test_fsm_fuzz import fixture, frames_of
from tests.test_keys_host import AUTHA, AUTHB, RANDRB, RANDTA, RANDTB
from tests.test_nested_keys_host import READR, READT, bytes_of, extend
from usrp_nfc_amd import _lib, api, fsm, synth
from usrp_nfc_amd.command import CommandType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 0x60, 0x61
HALT = 23
REQA_BITS = synth.frame_bits([0x26], 7) + [0]   # (a short frame as the packet tables hold it: tests/test_frames.py: packets_from_trace)
_rng = np.random.RandomState(9151)
KA, KB = _rng.randint(0, 256, 6).tolist(), _rng.randint(0, 256, 6).tolist()
UID = _rng.randint(0, 256, 4).tolist()
BLOCK12 = _rng.randint(0, 256, 16).tolist()
NR = _rng.randint(0, 256, 4).tolist()
TABLE_C = {(A, 3): KA, (B, 3): KB}   # block 12 lies in sector 3
_cache = {}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def crc(d):
    return list(d) + fsm.crc_a(list(d))


def select_packets(m, packets):
    """REQA .. SAK of a Classic 1K with UID, heard by the generating machine m."""
    for t, data in ((1, None), (0, [0x04, 0x00]), (1, [0x93, 0x20]), (0, UID + [UID[0] ^ UID[1] ^ UID[2] ^ UID[3]]),
                    (1, crc([0x93, 0x70] + UID + [UID[0] ^ UID[1] ^ UID[2] ^ UID[3]])), (0, crc([0x08]))):
        bits = REQA_BITS if data is None else synth.frame_bits(data)
        packets.append((t, bits))
        m.process_bits(bits, t)


def classic_txn(key_type, key, seed, halt=True):
    """One whole Classic transaction on block 12: select, AUTHA / AUTHB, the three nonce frames, a READ and -- halt -- an encrypted HALT.
    The ciphertext is what a machine keyed with `key` puts out (fsm.process_outgoing)."""
    m = fsm.fsm(out=io.StringIO())
    m.set_keys(key, key)
    by = CommandType.by_index
    packets = []
    select_packets(m, packets)

    def sent(t, data, cmd):
        packets.append((t, m.process_outgoing(synth.frame_bits(data), by(cmd))))

    auth = synth.frame_bits(crc([key_type, 12]))
    packets.append((1, auth))
    m.process_bits(auth, 1)
    sent(0, bytes_of(extend(seed)), RANDTA)
    sent(1, NR + list(m.get_state().ar), RANDRB)
    sent(0, list(m.get_state().at), RANDTB)
    sent(1, crc([0x30, 12]), READR)
    sent(0, crc(BLOCK12), READT)
    if halt:
        sent(1, crc([0x50, 0x00]), HALT)
    return packets


def nonce_by_stage_txn(key, seed):
    """REQA .. SAK, then a 4-byte tag frame and the 8-byte reader frame behind it, with NO AUTH command: the tag frame is RANDTA by
    stage.  The eight bytes are {nr}{ar} under `key`."""
    m = fsm.fsm(out=io.StringIO())
    m.set_keys(key, key)
    packets = []
    select_packets(m, packets)
    by = CommandType.by_index
    packets.append((0, m.process_outgoing(synth.frame_bits(bytes_of(extend(seed))), by(RANDTA))))
    packets.append((1, m.process_outgoing(synth.frame_bits(NR + list(m.get_state().ar)), by(RANDRB))))
    return packets


def ultralight_packets():
    """The Ultralight transaction as it is sent (synth.ULTRALIGHT_TXN), the REQA with its end bit as a packet table holds it."""
    return [(d, bits + [0] if len(bits) == 7 else bits) for d, bits in synth.txn_frames()]


def route_packets(name):
    if name == 'a':
        return classic_txn(A, KA, 0x3A17) + ultralight_packets()
    if name == 'b':
        return list(classic_packets()[0][:24]) + ultralight_packets() * 3
    if name == 'c':
        return classic_txn(B, KB, 0x9C42) + nonce_by_stage_txn(KB, 0x51E8)
    raise KeyError(name)


ROUTE_KEYS = {'a': ((KA, KA), None), 'b': (None, None), 'c': ((KA, [0x11] * 6), TABLE_C)}   # name -> ((key_a, key_b) or None, table)


def route(name):
    """-> (NfcFrames, (key_a, key_b) or None, sector table or None), made once and read-only."""
    if name not in _cache:
        fr = host_frames_of(route_packets(name))[0]
        for a in (fr.table,) + tuple(fr.bytes) + tuple(fr.par):
            a.setflags(write=False)
        _cache[name] = (fr,) + ROUTE_KEYS[name]
    return _cache[name]


# ---- helpers (shared with tests/test_ctx_commands.py) --------------------------------------------------------------------------------------
def keyed_state(keys=None):
    s = fsm.state_init()
    if keys:
        s.key_a[:], s.key_b[:] = keys[0], keys[1]
    return s


def copy_state(s):
    return _lib.FsmState.from_buffer_copy(state_bytes(s))


def orders(n):
    """segment_order for a list of n frames: ascending, reversed, a fixed shuffle (entries past the segment count are skipped)."""
    return (None, np.arange(n + 1, dtype=np.uint32)[::-1], np.random.RandomState(1234).permutation(n + 1).astype(np.uint32))


def assert_same(got, want):
    for g, w, what in zip(got[:3], want[:3], ('records', 'data', 'enc')):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


def segmented_equals_sequential(frames, keys=None, table=None, start=None, rows=None):
    """The twin in its three orders against nfc_host_commands_keyed on the same frames from the same state -> (the counters, the state)."""
    t = frames.table if rows is None else rows
    start = start if start is not None else keyed_state(keys)
    want_state = copy_state(start)
    want = fsm.host_commands(want_state, t, frames.bytes, frames.par, sector_keys=table)
    seen = []
    for order in orders(len(t)):
        st = copy_state(start)
        got = fsm.host_commands_segmented(st, t, frames.bytes, frames.par, sector_keys=table, segment_order=order)
        assert_same(got, want)
        assert state_bytes(st) == state_bytes(want_state)
        seen.append(got[3])
    assert seen[0] == seen[1] == seen[2]
    return seen[0], want_state


def segmented_equals_host_machine(frames, keys=None):
    m = host_machine(keys)
    want = run_host(m, frames)
    st = keyed_state(keys)
    got = fsm.host_commands_segmented(st, frames)
    assert_commands_equal(got[:3], want, frames.table['n_bytes'])
    assert state_bytes(st) == state_bytes(m.get_state())


# ---- 1. the cut predicate, by exhaustion ---------------------------------------------------------------------------------------------------
def test_a_cut_frame_forgets_where_the_machine_was():
    n_cmds = _lib.load().nfc_command_count()
    assert n_cmds == 27
    raw = np.zeros(1, _lib.RAW_FRAME_DTYPE)
    raw['type'], raw['n_bytes'], raw['n_bits'] = 1, 1, 8
    ciphers = (0, 0xFFFFFFFFFFFF, 0x123456789ABC)
    words = ([0, 0, 0, 0], [0xDE, 0xAD, 0xBE, 0xEF], [0xFF] * 4)
    n = 0
    for byte, cmd in ((0x26, 0), (0x52, 1)):
        data = [np.zeros(0, np.uint8), np.array([byte], np.uint8)]
        par = [np.zeros(0, np.uint8), np.array([1 - bin(byte).count('1') & 1], np.uint8)]
        for extra in (0, 1, 2, _lib.NFC_RAW_CRC_A_OK):
            raw['flags'] = _lib.NFC_RAW_PARITY_OK | extra
            first = None
            for cur_cmd in range(n_cmds):
                for tag_type in (-1, 0, 1, 2, 3):
                    for uid_len in (0, 4, 7):
                        for i, cur_key in enumerate((0, 1, 2, 45, 81)):
                            st = fsm.state_init()
                            st.cur_cmd, st.tag_type, st.encrypted, st.cur_key = cur_cmd, tag_type, 0, cur_key
                            st.cipher, st.flags = ciphers[i % 3], i % 4
                            st.ar[:], st.at[:] = words[i % 3], words[(i + 1) % 3]
                            st.key_a[:], st.key_b[:] = KA, KB
                            st.uid_len = uid_len
                            st.uid[:uid_len] = list(range(0x41, 0x41 + uid_len))
                            before = copy_state(st)
                            out = fsm.host_commands(st, raw, data, par)
                            rec = (out[0].tobytes(), out[1].tobytes(), out[2].tobytes())
                            first = first or rec
                            assert rec == first, (byte, extra, cur_cmd, tag_type, uid_len, cur_key)
                            assert int(out[0]['cmd'][0]) == cmd and int(out[0]['flags'][0]) == (extra & 3)
                            # the state: what the frame sets is set, what it does not touch is as it was
                            assert (st.cur_cmd, st.tag_type, st.encrypted, st.uid_len) == (cmd, -1, 0, 0) and not any(st.uid)
                            assert (st.cur_key, st.cipher, st.flags) == (before.cur_key, before.cipher, before.flags)
                            assert bytes(st.ar) == bytes(before.ar) and bytes(st.at) == bytes(before.at)
                            assert bytes(st.key_a) == bytes(before.key_a) and bytes(st.key_b) == bytes(before.key_b)
                            n += 1
    assert n == 2 * 4 * 27 * 5 * 3 * 5


def test_what_is_no_cut():
    """Beside the predicate: a frame that is cut in the stream's bits, one with a parity error, a tag frame and a longer frame open no
    segment -- and a REQA at frame 0 opens none either, segment 0 starts there anyway."""
    fr = host_frames_of([(1, REQA_BITS), (0, synth.frame_bits([0x26])), (1, synth.frame_bits([0x26, 0x00])), (1, REQA_BITS[:7] + [1]),
                         (1, synth.frame_bits([0x52], 7) + [0])])[0]
    t = fr.table.copy()
    assert t['n_bytes'].tolist() == [1, 1, 2, 1, 1] and not t['flags'][3] & _lib.NFC_RAW_PARITY_OK
    cn, _ = segmented_equals_sequential(fr)
    assert cn['n_segments'] == 2   # frame 0 and the WUPA
    t['flags'][4], t['n_bytes'][4] = _lib.NFC_RAW_CUT, 0
    cn, _ = segmented_equals_sequential(fr, rows=t)
    assert cn['n_segments'] == 1


# ---- 2. the twin against the sequential machine ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n, _ in GOLDEN_CASES])
def test_segmented_on_the_golden_packets(name):
    frames = host_frames_of(dict(GOLDEN_CASES)[name])[0]
    segmented_equals_sequential(frames)
    segmented_equals_host_machine(frames)


@pytest.mark.parametrize('keys', [None, WRONG_KEYS], ids=['right_key', 'wrong_key'])
def test_segmented_on_the_classic_trace(keys):
    frames = host_frames_of(classic_packets()[0])[0]
    cn, _ = segmented_equals_sequential(frames, keys)
    segmented_equals_host_machine(frames, keys)
    # 198 frames of one session, an encrypted HALT, a plain HALT, two REQAs: with the wrong key the session never ends for the machine
    assert cn == (dict(n_segments=3, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0) if keys is None else
                  dict(n_segments=3, n_rerun_segments=2, n_rerun_frames=2, n_keydep_segments=0))


@pytest.mark.parametrize('keys', [None, WRONG_KEYS], ids=['right_key', 'wrong_key'])
def test_segmented_on_the_classic_prefix(keys):
    cn, st = segmented_equals_sequential(prefix_frames(), keys)
    segmented_equals_host_machine(prefix_frames(), keys)
    assert cn['n_segments'] == 1 and st.encrypted != 0


def test_segmented_on_every_malformed_capture():
    rows = fixture()['rows']
    assert len(rows) >= 256
    total = dict(n_segments=0, n_rerun_segments=0, n_keydep_segments=0)
    for row in rows:
        cn, _ = segmented_equals_sequential(frames_of(row), row.keys)
        for k in total:
            total[k] += cn[k]
    assert total['n_segments'] > len(rows)   # (the captures hold cuts behind their first frame, or this shows nothing)


def test_route_a_every_guess_holds():
    frames, keys, table = route('a')
    cn, st = segmented_equals_sequential(frames, keys, table)
    segmented_equals_host_machine(frames, keys)
    t, _, _ = fsm.host_commands(keyed_state(keys), frames)
    assert t['cmd'][:13].tolist() == [0, 3, 6, 8, 9, 11, AUTHA, RANDTA, RANDRB, RANDTB, READR, READT, HALT]
    assert t['flags'][12] & fsm.FRAME_ENCRYPTED and t['flags'][8] & fsm.FRAME_AR_OK and t['flags'][9] & fsm.FRAME_AT_OK
    assert cn == dict(n_segments=2, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0)
    assert st.encrypted == 0 and st.cur_cmd == HALT


def test_route_b_every_later_segment_is_walked_again():
    frames, keys, table = route('b')
    cn, st = segmented_equals_sequential(frames, keys, table)
    segmented_equals_host_machine(frames, keys)
    assert len(frames.table) == 24 + 3 * 19
    assert cn == dict(n_segments=4, n_rerun_segments=3, n_rerun_frames=57, n_keydep_segments=0)
    assert st.encrypted != 0


def test_route_c_the_carried_cur_key():
    frames, keys, table = route('c')
    cn, st = segmented_equals_sequential(frames, keys, table)
    want = fsm.host_commands(keyed_state(keys), frames, sector_keys=table)
    t = want[0]
    assert t['cmd'].tolist() == [0, 3, 6, 8, 9, 11, AUTHB, RANDTA, RANDRB, RANDTB, READR, READT, HALT, 0, 3, 6, 8, 9, 11, RANDTA, RANDRB]
    assert t['flags'][8] & fsm.FRAME_AR_OK and t['flags'][20] & fsm.FRAME_AR_OK   # key B of the table, both times
    assert cn['n_segments'] == 2 and cn['n_keydep_segments'] >= 1 and cn['n_rerun_segments'] == 1 and cn['n_rerun_frames'] == 8
    assert st.cur_key == 2 + 40 + 3
    # the second transaction from a machine that assumes key A: another plaintext, no AR OK -- the route is taken
    assumed = keyed_state(keys)
    other = fsm.host_commands(assumed, frames.table[13:], frames.bytes, frames.par, sector_keys=table)
    o = int(other[0]['byte_off'][7])
    w = int(t['byte_off'][20])
    assert other[0]['cmd'][:7].tolist() == t['cmd'][13:20].tolist()
    assert not other[0]['flags'][7] & fsm.FRAME_AR_OK and other[1][o:o + 8].tolist() != want[1][w:w + 8].tolist()
    # ... and a batch that STARTS with the right cur_key carried in guesses right: nothing is walked again
    first = keyed_state(keys)
    fsm.host_commands(first, frames.table[:5], frames.bytes, frames.par, sector_keys=table)
    fsm.host_commands(first, frames.table[5:9], frames.bytes, frames.par, sector_keys=table)
    assert first.cur_key == 45
    cn2, _ = segmented_equals_sequential(frames, table=table, start=first, rows=frames.table[9:])
    assert cn2 == dict(n_segments=2, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=1)


def test_route_d_a_frame_whose_bits_were_cut():
    """NFC_RAW_CUT: accepted by the twin as by nfc_host_commands (NFC_CMD_CUT, NFC_FSM_LOST); a single context never makes one."""
    frames, keys, table = route('a')
    t = frames.table.copy()
    t['flags'][15], t['n_bytes'][15] = _lib.NFC_RAW_CUT, 0
    cn, st = segmented_equals_sequential(frames, keys, table, rows=t)
    got = fsm.host_commands_segmented(keyed_state(keys), t, frames.bytes, frames.par)
    assert int(got[0]['cmd'][15]) == _lib.NFC_CMD_CUT and st.flags == _lib.NFC_FSM_LOST and cn['n_segments'] == 2


def test_route_e_no_cut_and_nothing_at_all():
    frames = host_frames_of(ultralight_packets())[0]
    cn, _ = segmented_equals_sequential(frames, rows=frames.table[1:])
    assert cn == dict(n_segments=1, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0)
    start = keyed_state((KA, KB))
    start.cur_cmd, start.encrypted, start.cipher = 21, 1, 0x1234
    cn, st = segmented_equals_sequential(frames, start=start, rows=frames.table[:0])
    assert cn == dict(n_segments=0, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0)
    assert state_bytes(st) == state_bytes(start)


def test_segment_order_must_name_every_segment_once():
    frames, keys, table = route('b')
    for bad in ([0, 1, 2], [0, 1, 2, 2, 3], []):
        with pytest.raises(ValueError):
            fsm.host_commands_segmented(keyed_state(), frames, segment_order=bad)
    fsm.host_commands_segmented(keyed_state(), frames, segment_order=[3, 99, 1, 0, 2])
    bad = fsm.state_init()
    bad.cur_cmd = 27
    with pytest.raises(ValueError):
        fsm.host_commands_segmented(bad, frames)


# ---- 3. batches: the state carried between them --------------------------------------------------------------------------------------------
def in_batches(frames, keys, table, cuts):
    st = keyed_state(keys)
    t = frames.table
    edges = [0] + list(cuts) + [len(t)]
    rerun = 0
    for a, b in zip(edges[:-1], edges[1:]):
        want_state = copy_state(st)
        want = fsm.host_commands(want_state, t[a:b], frames.bytes, frames.par, sector_keys=table)
        got = fsm.host_commands_segmented(st, t[a:b], frames.bytes, frames.par, sector_keys=table)
        assert_same(got, want)
        assert state_bytes(st) == state_bytes(want_state)
        rerun += got[3]['n_rerun_segments']
    return st, rerun


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_routes_in_two_and_three_batches_at_every_frame_boundary(name):
    frames, keys, table = route(name)
    whole = keyed_state(keys)
    fsm.host_commands(whole, frames, sector_keys=table)
    n = len(frames.table)
    for c1 in range(1, n):
        st, _ = in_batches(frames, keys, table, (c1,))
        assert state_bytes(st) == state_bytes(whole), c1
        for c2 in range(c1 + 1, n):
            st, _ = in_batches(frames, keys, table, (c1, c2))
            assert state_bytes(st) == state_bytes(whole), (c1, c2)
    if name == 'b':   # a batch that starts inside the session starts encrypted from the carried machine: its first segment is exact
        st, rerun = in_batches(frames, keys, table, (12,))
        assert rerun == 3


# ---- 4. the stand-alone program under the sanitizers ---------------------------------------------------------------------------------------
def test_check_program_runs_clean_under_the_sanitizers(tmp_path):
    """tools/ctx_commands_check: the twin on routes (a) - (c) as this file renders them and on 10 000 random frame lists, built with
    -fsanitize=address,undefined as a program of its own."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    exe = str(tmp_path / 'ctx_commands_check')
    src = [os.path.join(ROOT, 'tools', 'ctx_commands_check', 'main.cpp'), os.path.join(ROOT, 'usrp_nfc_amd', 'csrc', 'nfc_ctx_commands.hip'),
           os.path.join(ROOT, 'usrp_nfc_amd', 'csrc', 'nfc_commands.hip')]
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                           '-fno-sanitize-recover=undefined', '-Wno-unused-function'] + src + ['-o', exe])
    path = str(tmp_path / 'routes.bin')
    with open(path, 'wb') as f:
        for name in ('a', 'b', 'c'):
            frames, keys, table = route(name)
            st = keyed_state(keys)
            from usrp_nfc_amd import keys as _keys
            kt = _keys.key_table(table) if table is not None else _lib.FsmKeyTable()
            t = np.ascontiguousarray(frames.table)
            f.write(np.array([len(t), len(frames.bytes[0]), len(frames.bytes[1])], '<u8').tobytes())
            f.write(state_bytes(st) + bytes(bytearray(kt)) + t.tobytes())
            for k in (0, 1):
                f.write(frames.bytes[k].tobytes() + frames.par[k].tobytes())
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'routes 3' in r.stdout and 'random lists 10000' in r.stdout and 'ok' in r.stdout


# ---- 5. declarations -------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_and_bound():
    names = ['nfc_track_commands', 'nfc_read_commands', 'nfc_set_fsm_keys', 'nfc_set_fsm_sector_keys', 'nfc_get_fsm_sector_keys',
             'nfc_get_fsm_state', 'nfc_set_fsm_state', 'nfc_host_commands_segmented']
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(getattr(L, n).argtypes for n in names)
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'nfc_amd.h')).read()
    assert all(n + '(' in header for n in names) and '#define NFC_AMD_ABI_VERSION 4' in header and _lib.ABI_VERSION == 4
    assert C.sizeof(_lib.CtxCommandCounters) == 16 and C.sizeof(_lib.CtxCommands) == 32 + 16 + 8 + 16 + 8 + 40 + 32
    assert C.sizeof(_lib.Stats) == 144   # nfc_stats is as it was: the new counters have a struct of their own
    for name in ('track_commands', 'set_keys', 'set_sector_keys', 'sector_keys', 'fsm_state', 'set_fsm_state', 'commands'):
        assert callable(getattr(api.NfcContext, name))
    assert callable(fsm.host_commands_segmented) and callable(api.NfcCommands.cmd_mask) and callable(api.NfcCommands.plain_crc_ok_mask)
