"""The per-sector key table on the GPU (include/nfc_amd.h: nfc_multi_set_sector_keys, nfc_multi_get_sector_keys; csrc/sector_keys.h,
multi_commands.hip.h): k_multi_commands with a table per stream against its CPU twin nfc_host_commands_keyed on the raw
frames of the same push, from IQ.  tests/test_sector_keys_host.py pins the twin to the host machine on the CPU and holds the cards (made
without the table) and the helpers.  Every comparison is for equality.

THE CAPTURES: card 1 (26 frames, 41 164 complex samples), the 4K card 2 (14 frames, 19 643), the golden Classic prefix and the
Ultralight fixture of tests/test_commands.py."""
import ctypes
import io

import numpy as np
import pytest

from tests.test_commands import PIECES, assert_same_commands, classic_iq, concatenated, context, one_push, three_streams, ultralight_iq
from tests.test_commands_host import state_bytes
from tests.test_sector_keys_host import (A, B, BLOCKS, K0, K1, K2, TABLE_1, TABLE_2, WRONG, card, flag_count, keyed_state, read_answers)
from usrp_nfc_amd import _lib, api, fsm, keys, synth

pytestmark = pytest.mark.gpu
_cache = {}
kb = lambda k: bytes(bytearray(k))
ALL_BLOCKS = [BLOCKS[4], BLOCKS[8], BLOCKS[12], BLOCKS[5]]


def card_iq(which):
    if which not in _cache:
        _cache[which] = synth.iq_from_profile(synth.modulation_profile(card(which)[0]))
        _cache[which].setflags(write=False)
    return _cache[which]


def frame_start(which, i):
    """The complex sample at which frame i of the card's capture starts; the frame before it ends 300 samples (150 us) earlier."""
    return len(synth.modulation_profile(card(which)[0][:i], tail=0))


def twin(raw, table=None, pair=None):
    s = keyed_state(pair)
    return fsm.host_commands(s, raw, sector_keys=table), state_bytes(s)


def card_1_in_one_push():
    """Card 1 alone in one push with TABLE_1 and the default keys, once: its (table, data, enc) and the state afterwards."""
    if 'one' not in _cache:
        iq = card_iq(1)
        with context(1, len(iq) // 2) as m:
            m.track_commands()
            m.set_sector_keys(TABLE_1)
            m.push([iq])
            got = tuple(a.copy() for a in m.fetch_commands().commands_of(0))
            _cache['one'] = (got, state_bytes(m.fsm_state(0)))
    return _cache['one']


# ---- 9. 130 streams in one push ---------------------------------------------------------------------------------------------------------
def test_130_streams_with_a_table_each_equal_the_twin():
    K = 130
    caps = [card_iq(1), card_iq(2), classic_iq(), ultralight_iq()]
    starts = np.concatenate([[0], np.cumsum([len(c) // 2 for c in caps])[:-1]])
    which = [k % 4 for k in range(K)]
    wrong_k1 = dict(TABLE_1, **{})
    wrong_k1[(A, 2)] = WRONG
    tables = [None if k == 0 else wrong_k1 if k == 4 else (TABLE_1, TABLE_2, TABLE_1, TABLE_2)[w] for k, w in enumerate(which)]
    buf = api.DeviceBuffer(np.concatenate(caps))
    try:
        with context(K, max(len(c) // 2 for c in caps), lib_path=_lib.hooks_path()) as m:
            guards = m.L.nfc_debug_multi_guards
            guards.argtypes = [ctypes.c_void_p]
            m.track_commands()
            for k, t in enumerate(tables):
                if t is not None:
                    m.set_sector_keys(t, stream=k)
            m.push_device(buf, np.array([starts[w] for w in which], np.uint64), np.array([len(caps[w]) // 2 for w in which], np.uint32))
            cm = m.fetch_commands()
            assert guards(m.h) == 0
            want_flags = []
            for k in range(K):
                raw = cm.raw.frames_of(k)
                want, want_state = twin(raw, tables[k])
                assert_same_commands(cm.commands_of(k), want)
                assert state_bytes(m.fsm_state(k)) == want_state, k
                want_flags.append(0)
            assert cm.stream_flags.tolist() == want_flags
            assert m.sector_keys(0) == {} and m.sector_keys(129) == {k: kb(v) for k, v in TABLE_2.items()}
            assert m.sector_keys(4) == {k: kb(v) for k, v in wrong_k1.items()}
            # what the streams gave: the whole card with the right table (the last lane of the third workgroup is a card 2, 128 a card 1) ...
            for k in (8, 64, 128):
                t, d, _ = cm.commands_of(k)
                assert read_answers(t, d) == ALL_BLOCKS and flag_count(t, fsm.FRAME_AT_OK) == 4
            t, _, _ = cm.commands_of(129)
            assert flag_count(t, fsm.FRAME_AT_OK) == 3 and m.fsm_state(129).tag_type == 2
            # ... the stream without a table: today's result, the twin with None, FF keys -- no authentication succeeds
            t, d, _ = cm.commands_of(0)
            assert_same_commands(cm.commands_of(0), twin(cm.raw.frames_of(0), None)[0])
            assert flag_count(t, fsm.FRAME_AT_OK) == 0 and read_answers(t, d) == []
            # ... and K1's slot wrong: sector 2 is lost, the rest of the card is read
            t, d, _ = cm.commands_of(4)
            assert BLOCKS[4] in read_answers(t, d) and BLOCKS[8] not in read_answers(t, d)
            # the golden prefix and the Ultralight capture do not care
            assert_same_commands(cm.commands_of(2), one_push()['got'][0])
            assert_same_commands(cm.commands_of(3), one_push()['got'][1])
    finally:
        buf.free()


# ---- 10. ragged pieces -------------------------------------------------------------------------------------------------------------------
def test_ragged_pieces_carry_the_choice_across_pushes():
    # streams 0 .. 2: the PIECES of tests/test_commands.py in rotation; none of their boundaries falls between an AUTH frame and its nonce
    # (card 1: 14 994 .. 15 294), so stream 3 is cut there by its piece length, and stream 4 between {nt} and {nr}{ar} (15 960 .. 16 260)
    # (60 samples before the next frame starts, 240 after the last one ended: a run without transitions closes a packet within 100)
    cut_auth, cut_nonce = frame_start(1, 9) - 60, frame_start(1, 10) - 60
    assert (cut_auth, cut_nonce) == (15234, 16200)
    streams = [card_iq(1), card_iq(2), card_iq(1), card_iq(1), card_iq(1)]
    tables = [TABLE_1, TABLE_2, TABLE_1, TABLE_1, TABLE_1]
    pieces = [None, None, None, cut_auth, cut_nonce]
    lens = np.array([len(s) // 2 for s in streams])
    K = len(streams)
    parts, done, j = [[] for _ in range(K)], np.zeros(K, np.int64), 0
    with context(K, max(PIECES)) as m:
        m.track_commands()
        for k, t in enumerate(tables):
            m.set_sector_keys(t, stream=k)
        while (done < lens).any():
            n = np.minimum(lens - done, [PIECES[(j + k) % 3] if pieces[k] is None else pieces[k] for k in range(K)])
            m.push([s[2 * a:2 * (a + b)] for s, a, b in zip(streams, done, n)])
            cm = m.fetch_commands()
            for k in range(K):
                parts[k].append(tuple(a.copy() for a in cm.commands_of(k)))
            done += n
            j += 1
        final = [state_bytes(m.fsm_state(k)) for k in range(K)]
    one, one_state = card_1_in_one_push()
    for k in (0, 2, 3, 4):
        assert_same_commands(concatenated(parts[k]), one)
        assert final[k] == one_state
    t, d, _ = concatenated(parts[1])
    assert flag_count(t, fsm.FRAME_AT_OK) == 3
    # an AUTH frame and its nonce frame in different pushes (stream 3), a nonce and its {nr}{ar} (stream 4)
    is_auth = lambda c: int(c) in (14, 15)
    split = [k for k in range(K) for a, b in zip(parts[k][:-1], parts[k][1:]) if len(a[0]) and len(b[0]) and is_auth(a[0]['cmd'][-1])]
    assert 3 in split
    assert any(len(a[0]) and len(b[0]) and int(a[0]['cmd'][-1]) == 16 and int(b[0]['cmd'][0]) == 17 for a, b in zip(parts[4][:-1], parts[4][1:]))


# ---- 11. a table set between two pushes; reset ---------------------------------------------------------------------------------------
def test_table_set_between_pushes_and_reset_of_one_stream():
    iq = card_iq(1)
    cut = frame_start(1, 8) - 60   # between READ 4's answer and the nested AUTH of block 8
    one, one_state = card_1_in_one_push()
    with context(3, len(iq) // 2) as m:
        m.track_commands()
        m.set_keys(K0, K2)
        m.push([iq[:2 * cut]] * 3)
        head = [tuple(a.copy() for a in m.fetch_commands().commands_of(k)) for k in range(3)]
        assert len(head[0][0]) == 8 and read_answers(head[0][0], head[0][1]) == [BLOCKS[4]]
        assert m.sector_keys(1) == {}
        m.set_sector_keys(TABLE_1)   # stream=None: every stream
        want_table = {k: kb(v) for k, v in TABLE_1.items()}
        assert [m.sector_keys(k) for k in range(3)] == [want_table] * 3
        m.push([iq[2 * cut:]] * 3)
        cm = m.fetch_commands()
        for k in range(3):
            got = concatenated([head[k], cm.commands_of(k)])
            assert_same_commands(got, one)
            st = m.fsm_state(k)
            assert list(st.key_a) == K0 and list(st.key_b) == K2 and st.cur_key == 2 + 1
        # the state but for the two keys is the one-push state
        st = m.fsm_state(0)
        st.key_a[:], st.key_b[:] = [0xFF] * 6, [0xFF] * 6
        assert state_bytes(st) == one_state
        m.reset(1)   # that stream's table and no other
        assert m.sector_keys(1) == {} and m.sector_keys(0) == want_table and m.sector_keys(2) == want_table
        assert state_bytes(m.fsm_state(1)) == state_bytes(fsm.state_init()) and list(m.fsm_state(0).key_a) == K0
        m.set_keys(K0, K2, stream=1)
        assert m.sector_keys(1) == {}   # set_keys does not touch a table
        m.set_fsm_state(2, fsm.state_init())
        assert m.sector_keys(2) == want_table   # ... nor does set_fsm_state
        m.push([iq] * 3)
        cm = m.fetch_commands()
        t, d, _ = cm.commands_of(1)   # without its table stream 1 reads sector 1 alone, twice
        assert read_answers(t, d) == [BLOCKS[4], BLOCKS[5]]
        t, d, _ = cm.commands_of(2)
        assert read_answers(t, d) == ALL_BLOCKS
        # arguments, before the device is touched
        def status(fn, *args):
            return fn(m.h, *args), m.L.nfc_multi_last_error(m.h).decode()
        tab, bad = keys.key_table(TABLE_1), _lib.FsmKeyTable()
        bad.present[0][3] = 7
        for rc, msg, name in (status(m.L.nfc_multi_set_sector_keys, 3, ctypes.byref(tab)) + ('stream',),
                              status(m.L.nfc_multi_set_sector_keys, -2, ctypes.byref(tab)) + ('stream',),
                              status(m.L.nfc_multi_set_sector_keys, 0, None) + ('table',),
                              status(m.L.nfc_multi_set_sector_keys, 0, ctypes.byref(bad)) + ('present',),
                              status(m.L.nfc_multi_get_sector_keys, 3, ctypes.byref(tab)) + ('stream',),
                              status(m.L.nfc_multi_get_sector_keys, 0, None) + ('table',)):
            assert rc == -1 and name in msg, (rc, msg, name)
        with pytest.raises(api.NfcError, match='sector'):
            m.set_sector_keys({(A, 40): K0})
        assert m.sector_keys(0) == want_table


# ---- 12. no table, no difference -------------------------------------------------------------------------------------------------------
def test_a_context_that_never_sets_a_sector_key_gives_the_golden_result():
    # (nfc_multi_stats has no allocation counter, so that half of the check is not made: the buffer's absence shows in sector_keys()
    # answering from the host, and in csrc/nfc_multi.hip: ensure_keys is reached from nfc_multi_set_sector_keys alone)
    streams = three_streams()
    want = one_push()
    with context(3, max(len(s) for s in streams) // 2) as m:
        m.track_commands()
        m.set_keys(*([0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], [0xFF] * 6), stream=2)
        m.push(streams)
        cm = m.fetch_commands()
        for k in range(3):
            assert_same_commands(cm.commands_of(k), want['got'][k])
            assert state_bytes(m.fsm_state(k)) == want['state'][k]
            assert m.sector_keys(k) == {}
        assert int(m.stats().n_launches) == want['n_launches'] and cm.n_launches == 3
        # an EMPTY table set on every stream: still the same, state included
        m.reset()
        m.set_keys(*([0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], [0xFF] * 6), stream=2)
        m.set_sector_keys({})
        m.push(streams)
        cm = m.fetch_commands()
        for k in range(3):
            assert_same_commands(cm.commands_of(k), want['got'][k])
            assert state_bytes(m.fsm_state(k)) == want['state'][k]


# ---- 13. from IQ to a decrypted card with no key given ---------------------------------------------------------------------------------
def test_decode_many_recovers_the_keys_and_reads_the_whole_card(tmp_path):
    """One first and three nested searches per file.  The inputs' condition -- every authentication of card 1 has exactly one verified key
    -- is tests/test_sector_keys_host.py::test_card_1_keys_are_unambiguous."""
    from usrp_nfc_amd import decoder
    paths = []
    for i in range(3):
        paths.append(str(tmp_path / ('card%d.fc32' % i)))
        np.asarray(card_iq(1), np.float32).tofile(paths[-1])
    got = decoder.decode_many(paths, commands=True, keys='recover', nested=True, max_push_samples=20011)
    want = decoder.decode_many(paths, commands=True, keys=(K0, K2, TABLE_1), max_push_samples=20011)
    one = card_1_in_one_push()[0]
    for g, w in zip(got, want):
        assert g.recovered_keys == {(A, 4): kb(K0), (A, 8): kb(K1), (B, 12): kb(K2), (A, 5): kb(K0)} and g.key_conflicts == {}
        assert len(g.commands) == len(w.commands) == 3
        for a, b in zip(g.commands, w.commands):
            assert_same_commands(a, b)
        t, d, e = concatenated(g.commands)
        assert_same_commands((t, d, e), one)
        assert read_answers(t, d) == ALL_BLOCKS and flag_count(t, fsm.FRAME_AT_OK) == 4 and flag_count(t, fsm.FRAME_AR_OK) == 4
        out = io.StringIO()
        fsm.dispatch(t, d, e, out=out)
        assert out.getvalue().count('COMMAND: READT') == 4
    # a per-source list of triples and pairs, and the two keys alone: sector 1 only
    mixed = decoder.decode_many(paths[:2], commands=True, keys=[(K0, K2, TABLE_1), (K0, K2)], max_push_samples=20011)
    assert_same_commands(concatenated(mixed[0].commands), one)
    t, d, _ = concatenated(mixed[1].commands)
    assert read_answers(t, d) == [BLOCKS[4], BLOCKS[5]]
