"""Commands on the GPU for ONE long stream, a lane per transaction (include/nfc_amd.h: nfc_track_commands, nfc_read_commands;
csrc/ctx_commands.hip.h).  The kernels are pinned to nfc_host_commands_keyed -- the sequential twin -- on the raw frames of the same
batch, read back with frames(): records, data and enc byte for byte, the machine's 88 bytes afterwards; and the four counters to
nfc_host_commands_segmented, the kernels' own text on the CPU.  tests/test_ctx_commands_host.py pins that twin and holds the inputs
and helpers.  Every comparison is for equality.

THE SHAPES.  The Ultralight fixture (29 003 samples, 19 commands) and the 24-frame Classic capture (39 269 samples) in one batch and in
pieces of 20 011, 7 919 and the rest, where the session spans batches.  200 (REQA, ATQA) pairs with one whole Ultralight transaction
among them: 201 segments -- four workgroups of the walk, four rounds of the resolve -- in one batch under 2^18 samples, through the
one-launch stage and through the multi-launch stages; 2 100 pairs, 4 201 frames: a second tile of the segment scan.  The routes of
the CPU file rendered to IQ.  The whole Classic trace twice in one batch: lanes of 200 frames."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.golden_util import GOLDEN
from tests.test_commands import PIECES, classic_iq, concatenated, ultralight_iq
from tests.test_commands_host import GOLD_UL, PREFIX_CMDS, WRONG_KEYS, classic_packets, dispatched, state_bytes
from tests.test_ctx_commands_host import REQA_BITS, assert_same, copy_state, keyed_state, route, route_packets
from usrp_nfc_amd import _lib, api, fsm, synth

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4   # nfc_status
_cache = {}


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def context(keys=None, table=None, track=True, **kw):
    c = api.NfcContext(samp_rate=2e6, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, **kw)
    if keys:
        c.set_keys(*keys)
    if table:
        c.set_sector_keys(table)
    if track:
        c.track_commands()
    return c


def iq_of(packets, **kw):
    """[(type, bits)] as the packet tables hold them -- a short frame with its end bit -- rendered to IQ."""
    frames = [(t, list(b[:7]) if t == 1 and len(b) == 8 else list(b)) for t, b in packets]
    return synth.iq_from_profile(synth.modulation_profile(frames, **kw))


def batch_equals_the_twins(c, state, table=None):
    """The batch c has just completed: its commands against the sequential twin on the batch's own raw frames from `state` (advanced in
    place), the counters against the segmented twin's, the machine's state against both.  -> (NfcCommands, NfcFrames)."""
    cm = c.commands()
    raw = c.frames()
    seg_state = copy_state(state)
    want = fsm.host_commands(state, raw, sector_keys=table)
    seg = fsm.host_commands_segmented(seg_state, raw, sector_keys=table)
    assert_same(cm.commands(), want)
    assert cm.counters == seg[3]
    assert state_bytes(c.fsm_state()) == state_bytes(state) == state_bytes(seg_state)
    assert cm.flags == state.flags and cm.n_commands == len(raw.table) and cm.n_bytes == int(raw.table['n_bytes'].sum())
    typ, idx = cm.src()   # src leads to the raw frames in stream order
    assert typ.tolist() == raw.table['type'].tolist()
    assert [int(raw.records[t][i]['idx']) for t, i in zip(typ.tolist(), idx.tolist())] == raw.table['idx'].tolist()
    return cm, raw


def one_batch(iq, keys=None, table=None, **kw):
    with context(keys, table, **kw) as c:
        c.push(iq)
        state = keyed_state(keys)
        cm, raw = batch_equals_the_twins(c, state, table)
        return cm, raw, state


# ---- 1. the two captures, one batch each ---------------------------------------------------------------------------------------------------
def test_ultralight_in_one_batch():
    cm, raw, _ = one_batch(ultralight_iq())
    assert len(ultralight_iq()) // 2 == 29003 and cm.n_commands == 19 and cm.n_launches == 6 and cm.bytes_copied > 0
    assert dispatched(*cm.commands()).rstrip('\n') == open(GOLD_UL).read().rstrip('\n')
    assert cm.counters == dict(n_segments=1, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0)
    assert int(cm.cmd_mask(22).sum()) == 4 and cm.plain_crc_ok_mask().tolist() == ((cm.table['cmd'] >= 0) & (cm.table['n_crc'] == 2)).tolist()


@pytest.mark.parametrize('keys', [None, WRONG_KEYS], ids=['right_key', 'wrong_key'])
def test_classic_in_one_batch(keys):
    cm, raw, state = one_batch(classic_iq(), keys)
    assert len(classic_iq()) // 2 == 39269 and cm.n_commands == 24
    if keys is None:
        assert cm.table['cmd'].tolist() == PREFIX_CMDS and classic_packets()[1].startswith(dispatched(*cm.commands()))
        assert dispatched(*cm.commands()).count('AT OK') == 2 and state.encrypted == 1
    else:
        wrong = cm.table['cmd']
        assert int((wrong == fsm.NFC_CMD_PARITY_ERROR).sum()) == 15 and int((wrong == fsm.NFC_CMD_UNKNOWN).sum()) == 1


def test_tracking_adds_six_launches_and_frames_adds_none():
    """What a call launches, counted by the test build (nfc_debug_launch_count): a tracked batch is the untracked batch's launches and
    six more -- the frames' two, which a frames() behind it then does not launch again, and the four of ctx_commands.hip.h.  A context
    that never tracks launches what it did: its frames() still launches its two."""
    L = _lib.load(_lib.hooks_path())
    count = L.nfc_debug_launch_count
    count.restype = C.c_uint64
    seen = {}
    for track in (False, True):
        with context(track=track, lib_path=_lib.hooks_path()) as c:
            a = count()
            c.push(ultralight_iq())
            b = count()
            want = c.frames()
            d = count()
            c.frames()
            assert count() == d
            seen[track] = (b - a, d - b, want)
            if track:
                assert_same(c.commands().commands(), fsm.host_commands(fsm.state_init(), want))
                assert count() == d
            else:
                with pytest.raises(api.NfcError) as e:
                    c.commands()
                assert '(status %d)' % ERR_STATE in str(e.value)   # tracking was off when the batch completed
    assert seen[True][0] == seen[False][0] + 6 and seen[True][1] == 0 and seen[False][1] == 2
    for t in (0, 1):
        assert seen[True][2].records[t].tobytes() == seen[False][2].records[t].tobytes()


# ---- 2. the same captures in pieces --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which,keys', [('ul', None), ('classic', None), ('classic', WRONG_KEYS)], ids=['ultralight', 'classic', 'classic_wrong_key'])
def test_pieces_give_the_single_batch(which, keys):
    iq = ultralight_iq() if which == 'ul' else classic_iq()
    whole, _, whole_state = one_batch(iq, keys)
    parts, at, j, encrypted_starts = [], 0, 0, 0
    n = len(iq) // 2
    with context(keys) as c:
        state = keyed_state(keys)
        while at < n:
            take = PIECES[j % 3] or n - at
            take = min(take, n - at)
            encrypted_starts += int(state.encrypted != 0)
            c.push(iq[2 * at:2 * (at + take)])
            cm, _ = batch_equals_the_twins(c, state)
            parts.append(cm.commands())
            at += take
            j += 1
    assert j == 3
    got = concatenated(parts)
    assert_same(got, whole.commands())
    assert state_bytes(state) == state_bytes(whole_state)
    if which == 'classic' and keys is None:
        assert encrypted_starts >= 1   # the session spans batches: a first segment starts encrypted from the carried machine


# ---- 3. more segments than a wave, a workgroup and a scan tile hold ---------------------------------------------------------------------------
def pairs_packets(n_pairs, ul_at):
    pair = [(1, REQA_BITS), (0, synth.frame_bits([0x44, 0x00]))]
    from tests.test_ctx_commands_host import ultralight_packets
    return pair * ul_at + ultralight_packets() + pair * (n_pairs - ul_at)


def pairs_iq(n_pairs, ul_at, **kw):
    key = ('pairs', n_pairs, ul_at)
    if key not in _cache:
        _cache[key] = iq_of(pairs_packets(n_pairs, ul_at), **kw)
        _cache[key].setflags(write=False)
    return _cache[key]


@pytest.mark.parametrize('no_small', [False, True], ids=['small_stage', 'multi_launch'])
def test_201_segments_in_one_batch(no_small, monkeypatch):
    iq = pairs_iq(200, 77, gap_us=120.0)
    assert len(iq) // 2 < 1 << 18
    kw = {}
    if no_small:
        monkeypatch.setenv('NFC_NO_SMALL', '1')   # (the test build: the multi-launch stages whatever the length)
        kw['lib_path'] = _lib.hooks_path()
    cm, raw, _ = one_batch(iq, **kw)
    assert cm.n_commands == 2 * 200 + 19
    assert cm.counters == dict(n_segments=201, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0)
    assert cm.table['cmd'][2 * 77:2 * 77 + 19].tolist() == [0, 2, 6, 7, 9, 10, 12, 13, 19, 20, 21, 22, 21, 22, 21, 22, 21, 22, 23]


def test_4201_frames_cross_a_tile_of_the_segment_scan():
    iq = pairs_iq(2100, 1500, gap_us=60.0)
    cm, raw, _ = one_batch(iq)
    assert cm.n_commands == 2 * 2100 + 19 > 4096
    assert cm.counters == dict(n_segments=2101, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0)


# ---- 4. the routes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_routes_rendered_to_iq(name):
    frames, keys, table = route(name)
    cm, raw, _ = one_batch(iq_of(route_packets(name)), keys, table)
    want = fsm.host_commands_segmented(keyed_state(keys), frames, sector_keys=table)
    assert cm.table['cmd'].tolist() == want[0]['cmd'].tolist() and cm.counters == want[3]   # the capture decodes to the frames it was rendered from
    assert cm.counters == {'a': dict(n_segments=2, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0),
                           'b': dict(n_segments=4, n_rerun_segments=3, n_rerun_frames=57, n_keydep_segments=0),
                           'c': dict(n_segments=2, n_rerun_segments=1, n_rerun_frames=8, n_keydep_segments=1)}[name]


def test_route_c_a_batch_that_starts_with_the_carried_cur_key():
    """The first transaction in one batch, the second in the next: the guess is the carried cur_key, and it is right."""
    frames, keys, table = route('c')
    packets = route_packets('c')
    with context(keys, table) as c:
        state = keyed_state(keys)
        c.push(iq_of(packets[:13]))
        batch_equals_the_twins(c, state, table)
        assert state.cur_key == 45 and c.sector_keys() == {k: bytes(v) for k, v in table.items()}
        c.push(iq_of(packets[13:]))
        cm, _ = batch_equals_the_twins(c, state, table)
        assert cm.counters == dict(n_segments=1, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0)
        assert cm.table['flags'][7] & fsm.FRAME_AR_OK


# ---- 5. long lanes -----------------------------------------------------------------------------------------------------------------------------
def test_the_classic_trace_twice_in_one_batch():
    packets = classic_packets()[0]
    cm, raw, state = one_batch(iq_of(list(packets) * 2))
    assert cm.n_commands == 404 and dispatched(*cm.commands()).count('AT OK') == 32
    assert cm.n_segments == 6 and cm.n_rerun_segments == 0   # (a trace ends HALT, HALT, REQA, REQA)
    assert int(np.diff(np.flatnonzero(np.r_[True, cm.cmd_mask(0)[1:], True])).max()) >= 199   # a lane walks a whole session


# ---- 6. the other ways a batch completes --------------------------------------------------------------------------------------------------------
def test_push_edges_is_tracked():
    with context(track=False) as src:
        src.push(classic_iq())
        edges = src.edges()
    want, _, want_state = one_batch(classic_iq())
    with context() as c:
        c.push_edges(edges)
        state = fsm.state_init()
        cm, _ = batch_equals_the_twins(c, state)
        assert_same(cm.commands(), want.commands())
        assert state_bytes(state) == state_bytes(want_state)


def test_two_batches_in_flight():
    iq = classic_iq()
    cut = 2 * 20011
    pieces = (iq[:cut], iq[cut:])
    sync = []
    with context() as c:
        state = fsm.state_init()
        for p in pieces:
            c.push(p)
            sync.append(batch_equals_the_twins(c, state)[0].commands())
    bufs = [api.DeviceBuffer(np.ascontiguousarray(p)) for p in pieces]
    try:
        with context() as c:
            state = fsm.state_init()
            for b, p in zip(bufs, pieces):
                c.submit_device(b, len(p) // 2)
            assert c.submitted() == 2
            for k in range(2):
                c.wait()
                cm, _ = batch_equals_the_twins(c, state)
                assert_same(cm.commands(), sync[k])
    finally:
        for b in bufs:
            b.free()


# ---- 7. errors, the machine's accessors -----------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    with context(track=False) as c:
        with pytest.raises(api.NfcError) as e:
            c.commands()
        assert '(status %d)' % ERR_STATE in str(e.value) and 'no completed batch' in str(e.value)
        assert state_bytes(c.fsm_state()) == state_bytes(fsm.state_init()) and c.sector_keys() == {}
        c.push(ultralight_iq())
        with pytest.raises(api.NfcError) as e:
            c.commands()
        assert '(status %d)' % ERR_STATE in str(e.value) and 'tracking was off' in str(e.value)
        bad = fsm.state_init()
        bad.tag_type = 4
        with pytest.raises(api.NfcError) as e:
            c.set_fsm_state(bad)
        assert '(status %d)' % ERR_ARG in str(e.value) and 'st: tag_type' in str(e.value)
        with pytest.raises(api.NfcError):
            c.set_keys([1, 2, 3])
        # the machine set, read back, reset
        st = fsm.state_init()
        st.cur_cmd, st.tag_type, st.cur_key, st.uid_len = 11, 1, 1, 4
        st.uid[:4] = [1, 2, 3, 4]
        c.set_fsm_state(st)
        assert state_bytes(c.fsm_state()) == state_bytes(st)
        c.set_keys([1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12])
        assert bytes(c.fsm_state().key_a) == bytes([1, 2, 3, 4, 5, 6]) and c.fsm_state().cur_cmd == 11
        c.set_sector_keys({(0x61, 39): [9] * 6})
        assert c.sector_keys() == {(0x61, 39): bytes([9] * 6)}
        c.reset()
        assert state_bytes(c.fsm_state()) == state_bytes(fsm.state_init()) and c.sector_keys() == {}
        # a batch without frames: tracked, nothing launched, the machine as it stands
        c.track_commands()
        c.push(np.zeros(2 * 4096, np.float32) + np.float32(0.35))
        cm = c.commands()
        assert (cm.n_commands, cm.n_launches, cm.bytes_copied, cm.flags) == (0, 0, 0, 0) and len(cm.table) == 0


def test_decoder_attaches_the_commands():
    from usrp_nfc_amd.decoder import decoder
    d = decoder(src=np.ascontiguousarray(classic_iq()).view(np.complex64), commands=True, keys=([0xFF] * 6, [0xFF] * 6), fsm=fsm.fsm(out=open(os.devnull, 'w')))
    back = d.run()
    d._trans.close()
    assert len(back.commands) == 1 and back.commands[0][0]['cmd'].tolist() == PREFIX_CMDS


def test_new_names_are_declared_and_bound():
    names = ['nfc_track_commands', 'nfc_read_commands', 'nfc_set_fsm_keys', 'nfc_set_fsm_sector_keys', 'nfc_get_fsm_sector_keys',
             'nfc_get_fsm_state', 'nfc_set_fsm_state', 'nfc_host_commands_segmented']
    assert set(names) <= set(_lib.SYMBOLS)
    for path in (None, _lib.hooks_path()):
        L = _lib.load(path)
        assert all(getattr(L, n).argtypes for n in names)
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'nfc_amd.h')).read()
    assert all(n + '(' in header for n in names) and '#define NFC_AMD_ABI_VERSION 4' in header
