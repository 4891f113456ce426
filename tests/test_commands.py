"""Commands on the GPU: the protocol machine, CRYPTO1 included, a lane per stream of a multi-stream context (include/nfc_amd.h:
nfc_multi_track_commands, nfc_multi_fetch_commands; csrc/multi_commands.hip.h, fsm.hip.h).  The kernel is pinned to the host machine
(nfc_fsm_process_frames) on the frames of the same push, and through it to the golden traces; tests/test_commands_host.py pins the
restatement itself on the CPU and holds the fixture and the helpers.  Every comparison is for equality.

THE THREE STREAMS: the 24-frame Classic capture (39 269 complex samples: 78 538 float32 values) with the default keys, the Ultralight
fixture (29 003 complex samples, 19 commands), and the Classic capture again with the wrong key A."""
import ctypes
import io
import os

import numpy as np
import pytest

from tests.golden_util import GOLDEN
from tests.test_commands_host import (GOLD_UL, PREFIX, PREFIX_CMDS, WRONG_KEYS, assert_commands_equal, classic_packets, dispatched, host_machine,
                                      run_host, state_bytes)
from usrp_nfc_amd import _lib, api, fsm, synth

pytestmark = pytest.mark.gpu
KEYS = (None, None, WRONG_KEYS)
PIECES = (20011, 7919, 0)
_cache = {}


def classic_iq():
    if 'classic' not in _cache:
        frames = synth.frames_from_trace(os.path.join(GOLDEN, '1k_with_enc.out'))[0][:PREFIX]
        _cache['classic'] = synth.iq_from_profile(synth.modulation_profile(frames))
        _cache['classic'].setflags(write=False)
    return _cache['classic']


def ultralight_iq():
    if 'ul' not in _cache:
        _cache['ul'] = np.load(os.path.join(GOLDEN, 'fx_ultralight_iq.npz'))['iq']
    return _cache['ul']


def three_streams():
    return [classic_iq(), ultralight_iq(), classic_iq()]


def context(K, max_push, **kw):
    return api.NfcMultiContext(K, max_push, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, **kw)


def tracked(K, max_push, keys=KEYS, **kw):
    m = context(K, max_push, **kw)
    m.track_commands()
    for k, ks in enumerate(keys):
        if ks:
            m.set_keys(*ks, stream=k)
    return m


def one_push():
    """The three streams in one push of a tracked context, once: per stream the (table, data, enc) the GPU gave, the host machine's on
    the same raw frames, and the state afterwards.  Shared by the tests that compare against it; nothing in it is changed."""
    if 'one_push' not in _cache:
        streams = three_streams()
        with tracked(3, max(len(s) for s in streams) // 2) as m:
            m.push(streams)
            cm = m.fetch_commands()
            _cache['one_push'] = dict(cm=cm, got=[tuple(a.copy() for a in cm.commands_of(k)) for k in range(3)],
                                      state=[state_bytes(m.fsm_state(k)) for k in range(3)], counts=m.counts_all(), n_launches=int(m.stats().n_launches))
    return _cache['one_push']


def concatenated(parts):
    """[(table, data, enc), ...] of consecutive pushes as one: the byte_offs moved behind each other."""
    tables, at = [], 0
    for t, d, _ in parts:
        t = t.copy()
        t['byte_off'] += at
        at += len(d)
        tables.append(t)
    return np.concatenate(tables), np.concatenate([d for _, d, _ in parts]), np.concatenate([e for _, _, e in parts])


def assert_same_commands(got, want):
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()


# ---- 7. three streams, one push -------------------------------------------------------------------------------------------------------
def test_three_streams_in_one_push_equal_the_host_machine():
    streams = three_streams()
    m = tracked(3, max(len(s) for s in streams) // 2, lib_path=_lib.hooks_path())
    guards = m.L.nfc_debug_multi_guards
    guards.argtypes = [ctypes.c_void_p]
    try:
        m.push(streams)
        cm = m.fetch_commands()
        assert guards(m.h) == 0
        fr = m.fetch_frames()
        assert guards(m.h) == 0
        assert cm.n_launches == 3 and cm.bytes_copied > 0 and int(m.stats().n_launches) == 4
        assert cm.stream_flags.tolist() == [0, 0, 0]
        for t in (0, 1):   # raw: what a fetch_frames() on the same push returns
            assert cm.raw.frames[t].tobytes() == fr.frames[t].tobytes() and cm.raw.bytes[t].tobytes() == fr.bytes[t].tobytes()
            assert cm.raw.par[t].tobytes() == fr.par[t].tobytes()
            assert cm.raw.frame_off[t].tolist() == fr.frame_off[t].tolist() and cm.raw.byte_off[t].tolist() == fr.byte_off[t].tolist()
        assert cm.raw.base.tolist() == fr.base.tolist()
        for k in range(3):
            raw = cm.raw.frames_of(k)
            got = cm.commands_of(k)
            assert_commands_equal(got, run_host(host_machine(KEYS[k]), raw), raw.table['n_bytes'])
            typ, idx = cm.src_of(k)   # src leads to the raw frames in stream order
            assert typ.tolist() == raw.table['type'].tolist()
            assert [int(raw.records[t][i]['idx']) for t, i in zip(typ.tolist(), idx.tolist())] == raw.table['idx'].tolist()
        assert cm.commands_of(0)[0]['cmd'].tolist() == PREFIX_CMDS
        assert classic_packets()[1].startswith(dispatched(*cm.commands_of(0))) and dispatched(*cm.commands_of(0)).count('AT OK') == 2
        assert dispatched(*cm.commands_of(1)).rstrip('\n') == open(GOLD_UL).read().rstrip('\n')
        wrong = cm.commands_of(2)[0]['cmd']
        assert int((wrong == fsm.NFC_CMD_PARITY_ERROR).sum()) == 15 and int((wrong == fsm.NFC_CMD_UNKNOWN).sum()) == 1
        assert cm.stream_of().tolist() == [0] * 24 + [1] * 19 + [2] * 24
        assert int(cm.cmd_mask(22)[:24].sum()) == 5 and cm.plain_crc_ok_mask().tolist() == ((cm.cmd['cmd'] >= 0) & (cm.cmd['n_crc'] == 2)).tolist()
        assert int(cm.plain_crc_ok_mask()[:24].sum()) == 14   # stream 0: AUTHA x 2, READR x 5, READT x 5, SEL1R, SEL1K
    finally:
        m.close()


# ---- 8. the same streams in ragged pieces -----------------------------------------------------------------------------------------------
def test_ragged_pieces_give_the_same_commands_and_state():
    streams = three_streams()
    lens = np.array([len(s) // 2 for s in streams])
    parts, done, j, empty_pushes = [[], [], []], np.zeros(3, np.int64), 0, 0
    with tracked(3, max(PIECES)) as m:
        while (done < lens).any():
            n = np.minimum(lens - done, [PIECES[(j + k) % 3] for k in range(3)])
            m.push([s[2 * a:2 * (a + b)] for s, a, b in zip(streams, done, n)])
            cm = m.fetch_commands()
            for k in range(3):
                parts[k].append(tuple(a.copy() for a in cm.commands_of(k)))
                empty_pushes += int(n[k] == 0)
                assert n[k] or len(parts[k][-1][0]) == 0
            done += n
            j += 1
        assert empty_pushes >= 3 and j >= 5
        want = one_push()
        for k in range(3):
            assert_same_commands(concatenated(parts[k]), want['got'][k])
            assert state_bytes(m.fsm_state(k)) == want['state'][k]
    for k in range(3):   # ... which is the host machine's state after the whole capture
        h = host_machine(KEYS[k])
        run_host(h, want['cm'].raw.frames_of(k))
        assert state_bytes(h.get_state()) == want['state'][k]


# ---- 9. 130 streams: three waves, the last one partly empty -----------------------------------------------------------------------------
def test_130_streams_of_different_lengths():
    K = 130
    caps = [classic_iq(), ultralight_iq()]
    starts = [0, len(caps[0]) // 2]
    which = [1 if k % 5 == 0 else 0 for k in range(K)]
    n = np.array([max(3000, (len(caps[w]) // 2) * (k + 1) // K) for k, w in enumerate(which)], np.uint32)
    first = np.array([starts[w] for w in which], np.uint64)
    buf = api.DeviceBuffer(np.concatenate(caps))
    try:
        with tracked(K, int(n.max()), keys=()) as m:
            m.push_device(buf, first, n)
            cm = m.fetch_commands()
            assert cm.cmd_off.tolist() == (cm.raw.frame_off[0] + cm.raw.frame_off[1]).tolist()
            assert cm.cbyte_off.tolist() == (cm.raw.byte_off[0] + cm.raw.byte_off[1]).tolist()
            counts = []
            for k in range(K):
                raw = cm.raw.frames_of(k)
                h = host_machine()
                assert_commands_equal(cm.commands_of(k), run_host(h, raw), raw.table['n_bytes'])
                assert state_bytes(m.fsm_state(k)) == state_bytes(h.get_state())
                counts.append(len(raw.table))
            assert cm.stream_flags.tolist() == [0] * K
            assert len(set(counts)) > 10 and max(counts) == 24 and counts[129] == 24   # sessions end at different frames
            enc_up = [m.fsm_state(k).encrypted for k in range(K) if which[k] == 0]
            assert 0 in enc_up and 1 in enc_up
    finally:
        buf.free()


# ---- 10. the hand-off both ways ---------------------------------------------------------------------------------------------------------
def test_hand_off_device_to_host_and_host_to_device():
    iq = classic_iq()
    cut = 20000   # complex samples (40 000 float32 values): 13 frames closed, the first session up
    with tracked(2, cut, keys=()) as m:
        m.push([iq[:2 * cut], None])
        cm = m.fetch_commands()
        head = cm.raw.frames_of(0)
        assert len(head.table) == 13 and len(cm.commands_of(1)[0]) == 0
        host = host_machine()
        run_host(host, head)
        st0 = m.fsm_state(0)
        assert st0.encrypted == 1 and state_bytes(st0) == state_bytes(host.get_state())
        # host to device: a fresh stream takes the host machine's state (and stream 0's signal state, which does not touch a machine)
        s0 = m.stream(0).get_state()
        m.stream(1).set_state(*s0)
        assert state_bytes(m.fsm_state(0)) == state_bytes(st0) and m.fsm_state(1).encrypted == 0
        m.set_fsm_state(1, host.get_state())
        assert state_bytes(m.fsm_state(1)) == state_bytes(st0)
        m.push([iq[2 * cut:], iq[2 * cut:]])
        cm = m.fetch_commands()
        rest = cm.commands_of(0)
        assert rest[0]['cmd'].tolist() == PREFIX_CMDS[13:]
        # device to host: a host machine continues from the device's state
        cont = host_machine()
        cont.set_state(st0)
        raw = cm.raw.frames_of(0)
        assert_commands_equal(rest, run_host(cont, raw), raw.table['n_bytes'])
        assert_same_commands(cm.commands_of(1), rest)
        assert state_bytes(m.fsm_state(0)) == state_bytes(m.fsm_state(1)) == state_bytes(cont.get_state())


# ---- 11. truncation -----------------------------------------------------------------------------------------------------------------------
def test_truncated_bit_slab_gives_a_cut_record_and_a_lost_stream():
    """cap_packet_bits = 900: the Classic capture closes 1 038 tag bits, its last tag frame ends behind the slab (the one before it at
    877); the Ultralight fixture's 806 and 392 bits fit.  Stream 2 is the same capture as stream 0, so it is cut in the same way: it is
    checked as stream 0 is, and stream 1 equals the untruncated push."""
    streams = three_streams()
    want = one_push()
    with tracked(3, max(len(s) for s in streams) // 2, cap_packet_bits=900) as m:
        m.push(streams)
        assert [bool(f & api.NFC_MULTI_TRUNC_BITS) for f in m.counts_all()['flags']] == [True, False, True]
        cm = m.fetch_commands()
        assert cm.stream_flags.tolist() == [_lib.NFC_FSM_LOST, 0, _lib.NFC_FSM_LOST]
        assert_same_commands(cm.commands_of(1), want['got'][1])
        for k in (0, 2):
            table, data, enc = cm.commands_of(k)
            full = want['got'][k]
            assert len(table) == 24 and table['cmd'][:23].tolist() == full[0]['cmd'][:23].tolist()
            assert table[:23].tobytes() == full[0][:23].tobytes()
            used = int(table['byte_off'][23])
            assert data[:used].tobytes() == full[1][:used].tobytes() and enc[:used].tobytes() == full[2][:used].tobytes()
            last = table[23]
            assert (int(last['cmd']), int(last['n_bytes']), int(last['n_enc']), int(last['type'])) == (_lib.NFC_CMD_CUT, 0, 0, 0)
            assert len(data) == used
            typ, idx = cm.src_of(k)
            assert int(cm.raw.frames_of(k).records[int(typ[23])][int(idx[23])]['flags']) == _lib.NFC_RAW_CUT
        m.push([None] * 3)                       # the flag is sticky: the next fetch still carries it
        cm = m.fetch_commands()
        assert cm.n_launches == 0 and len(cm.cmd) == 0 and cm.stream_flags.tolist() == [_lib.NFC_FSM_LOST, 0, _lib.NFC_FSM_LOST]
        m.reset(0)
        assert m.fsm_state(0).flags == 0 and state_bytes(m.fsm_state(0)) == state_bytes(fsm.state_init())
        m.push([None] * 3)
        assert m.fetch_commands().stream_flags.tolist() == [0, 0, _lib.NFC_FSM_LOST]


# ---- 12. tracking changes nothing else ------------------------------------------------------------------------------------------------------
def test_tracking_changes_no_other_output():
    streams = three_streams()
    res = []
    for on in (False, True):
        with context(3, max(len(s) for s in streams) // 2) as m:
            if on:
                m.track_commands()
            m.push(streams)
            launches = int(m.stats().n_launches)
            f = m.fetch(api.NFC_MULTI_FETCH_ALL)
            fr = m.fetch_frames()
            arrays = [f.edge_pos, f.edge_code] + f.symbols + f.packet_table + f.packet_bits + list(f.off) + fr.frames + fr.bytes + fr.par + fr.frame_off + fr.byte_off
            res.append((launches, m.counts_all().tobytes(), [np.asarray(a).tobytes() for a in arrays]))
    assert res[0][0] == 1 and res[1][0] == 4
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]


# ---- 13. call order and arguments -----------------------------------------------------------------------------------------------------------
def test_call_order_and_arguments():
    iq = classic_iq()
    with context(2, len(iq) // 2) as m:
        def status(fn, *args):
            return fn(m.h, *args), m.L.nfc_multi_last_error(m.h).decode()
        out = _lib.MultiCommands()
        m.track_commands()
        assert status(m.L.nfc_multi_fetch_commands, ctypes.byref(out))[0] == -4          # before any push
        m.track_commands(False)
        m.push([iq, None])
        assert int(m.stats().n_launches) == 1
        assert status(m.L.nfc_multi_fetch_commands, ctypes.byref(out))[0] == -4          # tracking was off at the last push
        m.track_commands()
        assert status(m.L.nfc_multi_fetch_commands, ctypes.byref(out))[0] == -4          # ... and switching it on does not change that
        m.push([iq, None])
        a = m.fetch_commands()
        state = state_bytes(m.fsm_state(0))
        b = m.fetch_commands()
        assert all(x.tobytes() == y.tobytes() for x, y in zip((a.cmd, a.data, a.enc, a.src, a.cmd_off, a.cbyte_off), (b.cmd, b.data, b.enc, b.src, b.cmd_off, b.cbyte_off)))
        assert state_bytes(m.fsm_state(0)) == state and len(a.cmd) == 24
        m.push([None, None])                                                             # all-zero lengths: nothing is launched
        assert int(m.stats().n_launches) == 1
        e = m.fetch_commands()
        assert e.n_launches == 0 and len(e.cmd) == 0 and e.cmd_off.tolist() == [0, 0, 0] and e.cbyte_off.tolist() == [0, 0, 0]
        assert state_bytes(m.fsm_state(0)) == state
        key = np.full(6, 0xFF, np.uint8)
        st = fsm.state_init()
        for rc, msg, name in (status(m.L.nfc_multi_set_keys, 2, key.ctypes.data, key.ctypes.data) + ('stream',),
                              status(m.L.nfc_multi_set_keys, -2, key.ctypes.data, key.ctypes.data) + ('stream',),
                              status(m.L.nfc_multi_set_keys, 0, None, key.ctypes.data) + ('key_a',),
                              status(m.L.nfc_multi_set_keys, 0, key.ctypes.data, None) + ('key_b',),
                              status(m.L.nfc_multi_get_fsm_state, 2, ctypes.byref(st)) + ('stream',),
                              status(m.L.nfc_multi_get_fsm_state, 0, None) + ('st',),
                              status(m.L.nfc_multi_set_fsm_state, 2, ctypes.byref(st)) + ('stream',),
                              status(m.L.nfc_multi_set_fsm_state, 0, None) + ('st',)):
            assert rc == -1 and name in msg, (rc, msg, name)
        st.uid_len = 33
        rc, msg = status(m.L.nfc_multi_set_fsm_state, 0, ctypes.byref(st))
        assert rc == -1 and 'uid_len' in msg
        with pytest.raises(api.NfcError):
            m.set_keys([1, 2, 3], [0xFF] * 6)
        assert state_bytes(m.fsm_state(0)) == state


# ---- 14. decode_many --------------------------------------------------------------------------------------------------------------------------
def test_decode_many_attaches_the_commands(tmp_path):
    from usrp_nfc_amd import decoder
    paths = []
    for name, iq in (('classic.fc32', classic_iq()), ('ultralight.fc32', ultralight_iq())):
        paths.append(str(tmp_path / name))
        np.asarray(iq, np.float32).tofile(paths[-1])
    quiet = lambda: fsm.fsm(out=io.StringIO())
    plain = decoder.decode_many(paths, fsm_factory=quiet, max_push_samples=15000)
    backs = decoder.decode_many(paths, fsm_factory=quiet, max_push_samples=15000, commands=True)
    assert not hasattr(plain[0], 'commands')
    texts = [''.join(dispatched(*c) for c in b.commands) for b in backs]
    assert classic_packets()[1].startswith(texts[0]) and texts[0].count('AR OK') == 2 and sum(len(c[0]) for c in backs[0].commands) == 24
    assert texts[1].rstrip('\n') == open(GOLD_UL).read().rstrip('\n')
    assert [b.packets for b in backs] == [b.packets for b in plain]
    wrong = decoder.decode_many(paths, fsm_factory=quiet, max_push_samples=15000, commands=True, keys=[WRONG_KEYS, ([0xFF] * 6, [0xFF] * 6)])
    table = np.concatenate([c[0] for c in wrong[0].commands])
    assert int((table['cmd'] == fsm.NFC_CMD_PARITY_ERROR).sum()) == 15
    assert ''.join(dispatched(*c) for c in wrong[1].commands) == texts[1]
