"""The protocol machine (csrc/fsm.hip.h, one text for host and device) in two of its holders on the CPU: nfc_host_commands -- the twin of
k_multi_commands, the UID in eight words, a slot per frame -- against the host machine (csrc/protocol.h: an unbounded UID, packed outputs)
through nfc_fsm_process_frames.  Both run the same text, so what these comparisons pin is what a holder adds; what the text computes is
pinned by tests/test_fsm_fuzz.py and tests/test_fsm_parent.py.  Also here: the hand-over of a machine through nfc_fsm_state,
the UID capacity, cut frames and fsm.dispatch.  Every comparison is for equality.  tests/test_commands.py holds the GPU half and uses
the helpers and the fixture below.

THE FIXTURE.  The first 24 frames of the Classic trace (tests/golden/1k_with_enc.out): a first authentication, four encrypted reads, a
NESTED authentication and one more read -- the smallest input that walks every CRYPTO1 route.  Rendered at 2 Msps they are 78 538
samples.  With key A = A0 .. A5 the same frames give no AR OK, 15 parity errors and one UNKNOWN."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from tests.golden_util import GOLDEN, Case
from tests.test_frames import GOLD_1K, GOLD_UL, GOLDEN_CASES, crafted_oracle_packets, host_frames_of, packets_from_trace
from usrp_nfc_amd import _lib, api, fsm, synth

PREFIX = 24
PREFIX_CMDS = [0, 3, 6, 8, 9, 11, 14, 16, 17, 18, 21, 22, 21, 22, 21, 22, 21, 22, 14, 16, 17, 18, 21, 22]
WRONG_KEYS = ([0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], [0xFF] * 6)
RECORD_FIELDS = ('cmd', 'type', 'n_bytes', 'n_header', 'n_extra', 'n_crc', 'flags', 'n_enc', 'pad')
_cache = {}


# ---- helpers (shared with tests/test_commands.py) ---------------------------------------------------------------------------------
def classic_packets():
    if 'classic' not in _cache:
        _cache['classic'] = packets_from_trace(GOLD_1K)
    return _cache['classic']   # (packets, text)


def host_machine(keys=None, out=None):
    m = fsm.fsm(out=out if out is not None else io.StringIO())
    if keys:
        m.set_keys(*keys)
    return m


def run_host(m, frames):
    """nfc_fsm_process_frames on an NfcFrames, with the enc entries process_frames does not return: (table, data, enc)."""
    t = np.ascontiguousarray(frames.table, _lib.RAW_FRAME_DTYPE)
    b = [np.ascontiguousarray(a, np.uint8) for a in frames.bytes]
    p = [np.ascontiguousarray(a, np.uint8) for a in frames.par]
    cap = int(t['n_bits'].sum()) // 9 + len(t) + 1
    out, buf, enc = np.zeros(len(t), fsm.FRAME_DTYPE), np.zeros(cap, np.uint8), np.zeros(cap, np.uint16)
    used = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    rc = m.L.nfc_fsm_process_frames(m._h, ptr(t), len(t), ptr(b[0]), ptr(p[0]), ptr(b[1]), ptr(p[1]), out.ctypes.data, buf.ctypes.data, buf.size,
                                    C.byref(used), enc.ctypes.data)
    assert rc == 0
    return out, buf[:used.value], enc[:used.value]


def assert_commands_equal(got, want, raw_n_bytes=None):
    """(table, data, enc) of the restated machine against the host machine's: every record field but byte_off (the host machine packs
    its bytes, the restatement gives every frame a slot of its raw n_bytes), the plaintext bytes and the enc entries per record; and
    the slots: byte_off the running sum of the raw n_bytes, zero behind what was written."""
    (gt, gd, ge), (wt, wd, we) = got, want
    assert len(gt) == len(wt)
    for name in RECORD_FIELDS:
        assert gt[name].tolist() == wt[name].tolist(), name
    at = 0
    for i, (g, w) in enumerate(zip(gt, wt)):
        go, wo, nb, ne = int(g['byte_off']), int(w['byte_off']), int(g['n_bytes']), int(g['n_enc'])
        assert gd[go:go + nb].tolist() == wd[wo:wo + nb].tolist(), ('bytes', i)
        assert ge[go:go + ne].tolist() == we[wo:wo + ne].tolist(), ('enc', i)
        if raw_n_bytes is not None:
            slot = int(raw_n_bytes[i])
            assert go == at and nb <= slot and ne <= slot
            assert not gd[go + nb:go + slot].any() and not ge[go + ne:go + slot].any(), ('the slot behind what was written', i)
            at += slot
    if raw_n_bytes is not None:
        assert len(gd) == len(ge) == at


def state_bytes(st):
    return bytes(bytearray(st))


def twin_against_host(frames, keys=None, cuts=()):
    """The twin and the host machine over the same frames, in pieces cut at `cuts` with the state carried over: both outputs, the
    states afterwards equal."""
    m = host_machine(keys)
    st = fsm.state_init()
    if keys:
        st.key_a[:], st.key_b[:] = keys[0], keys[1]
    table = frames.table
    edges = [0] + list(cuts) + [len(table)]
    for a, b in zip(edges[:-1], edges[1:]):
        part = table[a:b]
        want = run_host(m, api.NfcFrames([part[part['type'] == 0], part[part['type'] == 1]], frames.bytes, frames.par))
        got = fsm.host_commands(st, part, frames.bytes, frames.par)
        assert_commands_equal(got, want, part['n_bytes'])
        assert state_bytes(st) == state_bytes(m.get_state())
    return st


def prefix_frames():
    if 'prefix' not in _cache:
        _cache['prefix'] = host_frames_of(classic_packets()[0][:PREFIX])[0]
    return _cache['prefix']


def dispatched(table, data, enc):
    out = io.StringIO()
    fsm.dispatch(table, data, enc, out=out)
    return out.getvalue()


# ---- the fixture is what the file says it is ------------------------------------------------------------------------------------------
def test_fixture_prefix_walks_every_crypto1_route():
    packets, text = classic_packets()
    out = io.StringIO()
    table, _ = host_machine(out=out).process_frames(prefix_frames())
    got = out.getvalue()
    assert text.startswith(got) and len(got) < len(text)
    assert table['cmd'].tolist() == PREFIX_CMDS
    assert got.count('AR OK') == 2 and got.count('AT OK') == 2
    assert int(((table['flags'] & fsm.FRAME_ENCRYPTED) != 0).sum()) == 16 and int(prefix_frames().table['n_bytes'].max()) == 18
    out = io.StringIO()
    table, _ = host_machine(WRONG_KEYS, out=out).process_frames(prefix_frames())
    assert 'AR OK' not in out.getvalue()
    assert int((table['cmd'] == fsm.NFC_CMD_PARITY_ERROR).sum()) == 15 and int((table['cmd'] == fsm.NFC_CMD_UNKNOWN).sum()) == 1


# ---- 1. the twin against the host machine ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n, _ in GOLDEN_CASES])
def test_twin_on_the_golden_packets(name):
    twin_against_host(host_frames_of(dict(GOLDEN_CASES)[name])[0])


def test_twin_on_the_crafted_capture():
    frames = host_frames_of(crafted_oracle_packets())[0]
    st = twin_against_host(frames)
    assert not st.flags & _lib.NFC_FSM_UID_OVERFLOW


@pytest.mark.parametrize('keys', [None, WRONG_KEYS], ids=['right_key', 'wrong_key'])
def test_twin_on_the_classic_trace(keys):
    frames = host_frames_of(classic_packets()[0])[0]
    assert len(frames.table) == 202
    st = twin_against_host(frames, keys)
    assert st.flags == 0


@pytest.mark.parametrize('keys', [None, WRONG_KEYS], ids=['right_key', 'wrong_key'])
def test_twin_split_at_every_frame_boundary_of_the_prefix(keys):
    whole = twin_against_host(prefix_frames(), keys)
    for cut in range(1, PREFIX):
        assert state_bytes(twin_against_host(prefix_frames(), keys, cuts=(cut,))) == state_bytes(whole)
    assert state_bytes(twin_against_host(prefix_frames(), keys, cuts=tuple(range(1, PREFIX)))) == state_bytes(whole)


# ---- 2. the hand-over on the host -----------------------------------------------------------------------------------------------------
def test_state_hand_over_in_the_middle_of_a_session():
    frames = prefix_frames()
    table = frames.table
    part = lambda a, b: api.NfcFrames([table[a:b][table[a:b]['type'] == 0], table[a:b][table[a:b]['type'] == 1]], frames.bytes, frames.par)
    one = host_machine()
    run_host(one, part(0, 12))
    st = one.get_state()
    assert st.encrypted == 1 and st.uid_len == 4
    rest = run_host(one, part(12, PREFIX))
    two = host_machine()
    two.set_state(st)
    assert state_bytes(two.get_state()) == state_bytes(st)
    again = run_host(two, part(12, PREFIX))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rest, again))
    assert state_bytes(one.get_state()) == state_bytes(two.get_state())
    bad = fsm.state_init()
    bad.uid_len = 33
    with pytest.raises(ValueError):
        two.set_state(bad)


# ---- 3. the UID capacity ----------------------------------------------------------------------------------------------------------------
def test_uid_capacity_is_32_bytes():
    reqa = [(0x26 >> i) & 1 for i in range(7)] + [0]
    packets = [(1, reqa), (0, synth.frame_bits([0x04, 0x00]))]
    for i in range(9):
        uid = [0x10 + i, 0x20 + i, 0x30 + i, 0x40 + i]
        packets += [(1, synth.frame_bits([0x93, 0x20])), (0, synth.frame_bits(uid + [uid[0] ^ uid[1] ^ uid[2] ^ uid[3]]))]
    frames = host_frames_of(packets)[0]
    table = frames.table
    st = twin_against_host(api.NfcFrames([t[:9] for t in frames.records], frames.bytes, frames.par))   # through the eighth pair
    assert st.uid_len == 32 and st.flags == 0 and bytes(bytearray(st.uid))[-4:] == bytes([0x17, 0x27, 0x37, 0x47])
    m = host_machine()
    want = run_host(m, frames)
    assert want[0]['cmd'].tolist() == [0, 3] + [6, 8] * 9
    full = fsm.state_init()
    got = fsm.host_commands(full, table, frames.bytes, frames.par)
    assert got[0]['cmd'].tolist() == want[0]['cmd'].tolist()
    assert full.flags == _lib.NFC_FSM_UID_OVERFLOW and full.uid_len == 32 and state_bytes(full)[:80] == state_bytes(st)[:80]   # the append was not made
    with pytest.raises(ValueError):
        m.get_state()                     # the host UID holds 36 bytes: NFC_ERR_ARG
    st2 = _lib.FsmState()
    assert m.L.nfc_fsm_get_state(m._h, C.byref(st2)) == -1


# ---- 4. a cut frame ---------------------------------------------------------------------------------------------------------------------
def test_cut_frame_is_reported_and_leaves_the_machine_alone():
    frames = prefix_frames()
    table = frames.table[:13].copy()
    st = fsm.state_init()
    fsm.host_commands(st, table[:12], frames.bytes, frames.par)
    before = state_bytes(st)
    cut = table[12:13].copy()
    cut['flags'], cut['n_bytes'] = _lib.NFC_RAW_CUT, 0
    out, data, enc = fsm.host_commands(st, cut, frames.bytes, frames.par)
    assert out['cmd'].tolist() == [_lib.NFC_CMD_CUT] and out['n_bytes'].tolist() == [0] and out['n_enc'].tolist() == [0] and out['flags'].tolist() == [0]
    assert len(data) == len(enc) == 0
    assert st.flags == _lib.NFC_FSM_LOST
    st.flags = 0
    assert state_bytes(st) == before


# ---- 5. dispatch ------------------------------------------------------------------------------------------------------------------------
def test_dispatch_prints_the_classic_trace():
    packets, text = classic_packets()
    frames = host_frames_of(packets)[0]
    got = dispatched(*fsm.host_commands(fsm.state_init(), frames))
    assert got.rstrip('\n') == text.rstrip('\n')
    seen = []
    fsm.dispatch(*fsm.host_commands(fsm.state_init(), frames), out=io.StringIO(), callback=lambda cmd, s: seen.append(s.name()))
    assert len(seen) == 202


def test_dispatch_prints_the_ultralight_trace():
    frames = host_frames_of(Case('fx_ultralight_txn').packets)[0]
    table, data, enc = fsm.host_commands(fsm.state_init(), frames)
    assert len(table) == 19 and dispatched(table, data, enc).rstrip('\n') == open(GOLD_UL).read().rstrip('\n')


def test_the_machine_still_dispatches_through_the_module_function():
    out = io.StringIO()
    host_machine(out=out).process_frames(prefix_frames())
    assert out.getvalue() == dispatched(*run_host(host_machine(), prefix_frames()))


# ---- 6. declarations --------------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_and_bound():
    names = ['nfc_fsm_state_init', 'nfc_fsm_get_state', 'nfc_fsm_set_state', 'nfc_host_commands', 'nfc_multi_track_commands', 'nfc_multi_fetch_commands',
             'nfc_multi_set_keys', 'nfc_multi_get_fsm_state', 'nfc_multi_set_fsm_state']
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(getattr(L, n).argtypes for n in names)
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'nfc_amd.h')).read()
    assert all(n + '(' in header for n in names) and '#define NFC_AMD_ABI_VERSION 4' in header and _lib.ABI_VERSION == 4
    # the sizes the library asserts for its own structs (static_assert in csrc/nfc_commands.hip, nfc_multi.hip)
    assert C.sizeof(_lib.FsmState) == _lib.FSM_STATE_DTYPE.itemsize == 88 and C.sizeof(_lib.FsmState) % 8 == 0
    assert C.sizeof(_lib.MultiCommands) == C.sizeof(_lib.MultiFrames) + 120 == 264
    assert fsm.FRAME_DTYPE.itemsize == C.sizeof(_lib.Frame) == 28
    st = fsm.state_init()
    assert (st.cur_cmd, st.tag_type, st.encrypted, st.cur_key, st.cipher, st.uid_len, st.flags, st.reserved) == (0, -1, 0, 0, 0, 0, 0, 0)
    assert bytes(bytearray(st.key_a)) == bytes(bytearray(st.key_b)) == b'\xff' * 6
    assert state_bytes(host_machine().get_state()) == state_bytes(st)
    assert (_lib.NFC_CMD_CUT, _lib.NFC_FSM_LOST, _lib.NFC_FSM_UID_OVERFLOW) == (-3, 1, 2)
