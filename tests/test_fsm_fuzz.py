"""The protocol machine (csrc/fsm.hip.h) in its three holders -- the host machine behind fsm.fsm (csrc/protocol.h), the twin behind
fsm.host_commands, and k_multi_commands, a GPU lane per stream -- on MALFORMED traffic, against the reference's own fsm.process_bits / process_outgoing.

THE FIXTURE, tests/golden/fx_fsm_fuzz.npz, is written by tests/golden/make_fsm_golden.py, which runs the reference's machine itself (translated
to Python 3 in memory, gated on printing both golden traces): 2 000 seeded sequences -- the 24-frame Classic prefix, the Ultralight
transaction and the crafted packets of tests/test_frames.py with one to three mutations (a bit flipped, a frame dropped, doubled, cut,
lengthened, its direction swapped, a random frame inserted, two exchanged), and four directed families: a RANDTA arriving with a UID of
0, 3, 7 and 10 bytes; RANDRB / RANDTB with no session up; a nested {nt} cut to every length from 0 to 36 bits; frames of 9k + r bits for
every r in and out of a session; a NESTED authentication under a UID of three and of seven bytes inside a session whose keystream is
right (the frames made with the reference's own cipher), a {nr}{ar} / {at} of zeros behind it -- with the keys FF..FF, the wrong key A, key A != key B.  Per sequence it holds the frames, the text the
reference printed PER FRAME and the frame at which the reference raised an exception (-1: none).  256 more rows are sequences rendered to
IQ at 2 Msps and decoded by the C oracle: their frames are the oracle's packets, their text the reference's on those packets.

WHERE THE REFERENCE RAISES (a UID longer than the nonce, RANDRB / RANDTB with no session, an empty UID or a frame shorter than the UID in a
nested authentication) it has no behaviour: the comparison with its text stops at that frame, and what the project does from there on
 is pinned by tests/test_fsm_parent.py, whose recorded digests cover the whole sequence; the twin and kernel legs here compare holders.  Every comparison is for equality."""
import ctypes
import io
import os

import numpy as np
import pytest

from tests.golden_util import GOLDEN
from tests.test_commands import PIECES, concatenated
from tests.test_commands_host import WRONG_KEYS, assert_commands_equal, dispatched, host_machine, run_host, state_bytes
from tests.test_frames import host_frames_of
from usrp_nfc_amd import _lib, api, command, fsm, synth

FIXTURE = os.path.join(GOLDEN, 'fx_fsm_fuzz.npz')
FAMILIES = ('probe', 'uid_len', 'no_session', 'nt_cut', 'nine_k_r', 'authb', 'nested_uid')
DIRECTED = (1, 2, 3, 4, 6)
ALL_SECTORS = 40
_cache = {}


class Row(object):
    """One row of the fixture: packets [(type, [bits])], texts per frame, the in-session flags, raised, keys, family, src, seed."""


def fixture():
    if 'fx' not in _cache:
        z = np.load(FIXTURE)
        z = {k: z[k] for k in z.files}
        bits = np.unpackbits(z['frame_bits'])
        frames = [(int(t), bits[8 * int(o):8 * int(o) + int(n)].tolist()) for t, n, o in zip(z['frame_type'], z['frame_len'], z['frame_off'])]
        blob = z['text_blob'].tobytes()
        texts = [blob[a:b].decode('utf-8') for a, b in zip(z['text_off'][:-1], z['text_off'][1:])]
        rows = []
        for r in range(len(z['seq_raise'])):
            a, b = int(z['seq_off'][r]), int(z['seq_off'][r + 1])
            row = Row()
            row.index = r
            row.packets = [frames[i] for i in z['seq_frame'][a:b]]
            row.texts = [texts[i] for i in z['seq_text'][a:b]]
            row.sess = z['seq_sess'][a:b].tolist()
            row.raised = int(z['seq_raise'][r])
            row.keys = (z['seq_keys'][r][:6].tolist(), z['seq_keys'][r][6:].tolist())
            row.family, row.src, row.seed = int(z['seq_family'][r]), int(z['seq_src'][r]), int(z['seq_seed'][r])
            row.compared = len(row.packets) if row.raised < 0 else row.raised   # frames whose text the reference printed
            rows.append(row)
        scen = []
        for s in range(len(z['out_role'])):
            a, b = int(z['out_off'][s]), int(z['out_off'][s + 1])
            steps = [(int(z['out_kind'][i]), int(z['out_a'][i]), frames[int(z['out_in'][i])][1], frames[int(z['out_out'][i])][1], texts[int(z['out_text'][i])]) for i in range(a, b)]
            scen.append((int(z['out_role'][s]), steps, int(z['out_raise'][s])))
        n_seq = int(z['n_seq'])
        _cache['fx'] = dict(rows=rows, seqs=rows[:n_seq], gpu=[rows[int(i)] for i in z['gpu_rows']], outgoing=scen)
    return _cache['fx']


def normalise(text):
    """THE one normaliser: Python 2 printed format(v, '#04X') with a lower-case prefix, and the project prints no lists -- the two
    `MISMATCH BETWEEN READER...` lines are cut behind the word UID."""
    out = []
    for line in text.replace('0X', '0x').split('\n'):
        out.append(line[:line.index(' UID') + 4] if line.startswith('MISMATCH BETWEEN READER') else line)
    return '\n'.join(out)


def frames_of(row):
    if 'frames' not in row.__dict__:
        row.frames = host_frames_of(row.packets)[0]
    return row.frames


def host_result(row):
    """The host machine over the row's frames with the row's keys, once: (table, data, enc) and the state afterwards."""
    if 'host' not in row.__dict__:
        m = host_machine(row.keys)
        row.host = run_host(m, frames_of(row))
        row.host_state = state_bytes(m.get_state())
    return row.host


def full_table(keys):
    t = {}
    for s in range(ALL_SECTORS):
        t[(0x60, s)], t[(0x61, s)] = bytes(keys[0]), bytes(keys[1])
    return t


# ---- the fixture is what the file says it is ---------------------------------------------------------------------------------------------
def test_fixture_caps():
    fx = fixture()
    seqs, gpu = fx['seqs'], fx['gpu']
    assert len(seqs) == 2000 and len(gpu) == 256
    assert os.path.getsize(FIXTURE) <= 385 * 1024
    assert sum(r.raised >= 0 for r in seqs) * 10 <= len(seqs)          # the reference raises in at most 10 % of the sequences ...
    assert sum(r.raised >= 0 for r in gpu) * 10 <= len(gpu)            # ... and of the 256
    for section in (seqs, gpu):                                        # every directed family at least 8 times, in both sections
        fam = np.bincount([r.family for r in section], minlength=len(FAMILIES))
        assert all(fam[f] >= 8 for f in DIRECTED), fam.tolist()
    seen = sum(min(r.compared + 1, len(r.packets)) for r in seqs)
    inside = sum(sum(r.sess) for r in seqs)
    assert inside * 10 >= seen * 4, (inside, seen)                     # at least 40 % of all frames inside a session
    for r in gpu:
        src = seqs[r.src]
        assert r.keys == src.keys and r.family == src.family
        assert len(synth.modulation_profile(src.packets)) <= 48000     # complex samples
    keys = {tuple(r.keys[0] + r.keys[1]) for r in seqs}
    assert tuple([0xFF] * 12) in keys and tuple(WRONG_KEYS[0] + WRONG_KEYS[1]) in keys and any(k[:6] != k[6:] and k[6:] != (0xFF,) * 6 for k in keys)
    # the directed families are what their names say.  Every {nt} length is there (0 bits: the frame is gone, 23 frames) ...
    assert {len(r.packets[19][1]) for r in seqs if r.family == 3 and len(r.packets) == 24} >= set(range(1, 37))
    assert any(r.family == 3 and len(r.packets) == 23 for r in seqs)
    # ... UIDs of 0, 3, 7 and 10 bytes meet a first tag nonce: 0 and 3 start a session, at 7 and 10 the reference raises ...
    met = {}
    for row in (r for r in seqs if r.family == 1):
        m = host_machine(row.keys)
        for i, (t, bits) in enumerate(row.packets):
            before = m.get_state()
            st = m.process_bits(bits, t)
            if st is not None and st.name() == 'RANDTA' and not before.encrypted:
                met.setdefault(before.uid_len, set()).add((row.raised == i, m.get_state().encrypted))
                break
    assert set(met) >= {0, 3, 7, 10} and met[0] == met[3] == {(False, 1)} and met[7] == met[10] == {(True, 0)}, met
    # ... RANDRB / RANDTB without a session are frames at which the reference raises, in both sections ...
    assert all(sum(r.family == 2 and r.raised >= 0 for r in section) >= 8 for section in (seqs, gpu))
    # ... and a nested authentication meets UIDs of three and seven bytes (encrypted == 2: a session whose answers nothing equals)
    for section in (seqs, gpu):
        ends = {}
        for row in (r for r in section if r.family == 6):
            m = host_machine(row.keys)
            run_host(m, frames_of(row))
            st = m.get_state()
            ends.setdefault(st.uid_len, set()).add(st.encrypted)
            if st.uid_len == 3:
                assert 'ERROR WITH AR' in ''.join(row.texts) and 'ERROR WITH AT' in ''.join(row.texts) and row.raised < 0
        assert ends == {3: {2}, 7: {2}}, ends
    for r in (0, 1, 2, 3, 4, 5, 6, 7, 8):
        assert any(len(b) % 9 == r for row in seqs if row.family == 4 for _, b in row.packets)


# ---- 1. the host machine against the reference ---------------------------------------------------------------------------------------------
def reference_leg(rows):
    bad = []
    for row in rows:
        out = io.StringIO()
        m = host_machine(row.keys, out=out)
        for i, (t, bits) in enumerate(row.packets[:row.compared]):
            at = out.tell()
            m.process_bits(bits, t)
            got = out.getvalue()[at:]
            if normalise(got) != normalise(row.texts[i]):
                bad.append('row %d (%s) frame %d: the reference printed %r, the host machine %r' % (row.index, FAMILIES[row.family], i, row.texts[i], got))
                break
    assert not bad, '%d rows differ; the first: %s' % (len(bad), '\n'.join(bad[:5]))


def test_host_machine_prints_what_the_reference_printed():
    reference_leg(fixture()['rows'])   # the 2 000 sequences and the 256 oracle-decoded ones


def test_frame_route_prints_what_the_reference_printed():
    # nfc_fsm_process_frames -- what the twin and the kernel are compared with -- on the same rows
    for row in fixture()['rows']:
        table, data, enc = host_result(row)
        assert normalise(dispatched(table[:row.compared], data, enc)) == normalise(''.join(row.texts[:row.compared])), row.index


# ---- 2. the twin against the host machine ----------------------------------------------------------------------------------------------------
def twin_run(row, cuts=(), sector_keys=None, keys='row'):
    """fsm.host_commands over the row's frames in pieces cut at `cuts`, the state handed over: the concatenated (table, data, enc), the state."""
    frames = frames_of(row)
    st = fsm.state_init()
    if keys == 'row':
        st.key_a[:], st.key_b[:] = row.keys
    parts, edges = [], [0] + list(cuts) + [len(frames.table)]
    for a, b in zip(edges[:-1], edges[1:]):
        handed = _lib.FsmState.from_buffer_copy(state_bytes(st))   # the state goes through its plain bytes
        parts.append(fsm.host_commands(handed, frames.table[a:b], frames.bytes, frames.par, sector_keys=sector_keys))
        st = handed
    return concatenated(parts), st


def test_twin_equals_the_host_machine_on_every_sequence():
    for row in fixture()['rows']:
        frames = frames_of(row)
        want = host_result(row)
        got, st = twin_run(row)
        assert_commands_equal(got, want, frames.table['n_bytes'])
        assert state_bytes(st) == row.host_state, row.index
        if row.index % 16 == 0:   # split at every frame boundary, the state handed over
            got, st = twin_run(row, cuts=range(1, len(frames.table)))
            assert_commands_equal(got, want, frames.table['n_bytes'])
            assert state_bytes(st) == row.host_state, row.index
            m = host_machine(row.keys)
            parts = []
            for i in range(len(frames.table)):   # ... and the host machine's through get_state / set_state
                one = frames.table[i:i + 1]
                parts.append(run_host(m, api.NfcFrames([one[one['type'] == 0], one[one['type'] == 1]], frames.bytes, frames.par)))
                nxt = host_machine()
                nxt.set_state(m.get_state())
                m = nxt
            assert_commands_equal(got, concatenated(parts), frames.table['n_bytes'])
            assert state_bytes(m.get_state()) == row.host_state


# ---- 3. sector tables ------------------------------------------------------------------------------------------------------------------------
def fallback_key_used(table):
    """A first authentication's tag nonce with no AUTHA / AUTHB before it in the sequence: the register is loaded with set_keys' key A, which
    the table does not replace."""
    cmd, enc = table['cmd'], (table['flags'] & fsm.FRAME_ENCRYPTED) != 0
    auth = np.flatnonzero((cmd == 14) | (cmd == 15))
    first = np.flatnonzero((cmd == 16) & ~enc)
    return len(first) > 0 and (len(auth) == 0 or first[0] < auth[0])


def without_cur_key(state):
    st = _lib.FsmState.from_buffer_copy(state)
    st.cur_key = 0
    return state_bytes(st)


def test_sector_table_in_place_of_set_keys():
    n = differ = 0
    for row in fixture()['rows'][::3]:
        frames = frames_of(row)
        table = full_table(row.keys)
        m = host_machine()                       # (set_keys is NOT called: both keys stay FF..FF)
        m.set_sector_keys(table)
        want = run_host(m, frames)
        got, st = twin_run(row, sector_keys=table, keys=None)
        assert_commands_equal(got, want, frames.table['n_bytes'])
        assert state_bytes(st) == state_bytes(m.get_state()), row.index
        plain = host_result(row)
        if fallback_key_used(plain[0]) and row.keys[0] != [0xFF] * 6:
            differ += 1
            continue
        n += 1
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, plain)), row.index
        keyed = _lib.FsmState.from_buffer_copy(state_bytes(st))
        keyed.key_a[:], keyed.key_b[:] = row.keys   # the two keys of set_keys are part of the state; the table is not
        assert without_cur_key(state_bytes(keyed)) == without_cur_key(row.host_state), row.index
    assert n > 600 and differ < 40, (n, differ)


# ---- 4. the outgoing route -------------------------------------------------------------------------------------------------------------------
def test_process_outgoing_puts_out_what_the_reference_put_out():
    scen = fixture()['outgoing']
    assert len(scen) > 100 and {r for r, _, _ in scen} == {0, 1}
    sent, answers = 0, ''
    for s, (role, steps, raised) in enumerate(scen):
        out = io.StringIO()
        emu = fsm.fsm(callback=lambda cmd, st: None, out=out)
        for i, (kind, a, bits_in, bits_out, text) in enumerate(steps[:len(steps) if raised < 0 else raised]):
            if not bits_in:   # (a frame cut to nothing: the reference changed no state on it, or raised)
                continue
            at = out.tell()
            if kind == 0:
                emu.process_bits(bits_in, a)
            else:
                got = emu.process_outgoing(bits_in, command.CommandType.by_index(a))
                assert got == bits_out, 'scenario %d (role %d) step %d, command %d' % (s, role, i, a)
                sent += 1
            # what the machine printed with its callback silent: the ciphertext it heard, PARITY ERROR, AR / AT of a session process_outgoing started
            assert normalise(out.getvalue()[at:]) == normalise(text), 'scenario %d (role %d) step %d' % (s, role, i)
            answers += text
    assert sent > 500 and 'AR OK' in answers and 'AT OK' in answers


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def gpu_streams():
    """The 256 captures, rendered once per module from the stored bits and seeds (as tests/test_commands.py: classic_iq)."""
    if 'iq' not in _cache:
        fx = fixture()
        iq = []
        for row in fx['gpu']:
            a = synth.iq_from_profile(synth.modulation_profile(fx['seqs'][row.src].packets), seed=row.seed)
            a.setflags(write=False)
            iq.append(a)
        _cache['iq'] = iq
    return _cache['iq']


def tracked(rows, max_push, **kw):
    """A tracked context of one stream per (k, row): the stream's keys through set_keys, every third k's through set_sector_keys as well
    (the table serves every AUTH; a tag nonce that no AUTH preceded is keyed with set_keys' key A, as in the reference)."""
    m = api.NfcMultiContext(len(rows), max_push, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, **kw)
    m.track_commands()
    for j, (k, row) in enumerate(rows):
        m.set_keys(*row.keys, stream=j)
        if k % 3 == 2:
            m.set_sector_keys(full_table(row.keys), stream=j)
    return m


def host_for_stream(k, row):
    m = host_machine(row.keys)
    if k % 3 == 2:
        m.set_sector_keys(full_table(row.keys))
    return m


def gpu_one_push():
    """The 256 streams in one push of a tracked context on the hooks build, once; shared, nothing in it is changed."""
    if 'one_push' not in _cache:
        streams, rows = gpu_streams(), fixture()['gpu']
        m = tracked(list(enumerate(rows)), max(len(s) for s in streams) // 2, lib_path=_lib.hooks_path())
        guards = m.L.nfc_debug_multi_guards
        guards.argtypes = [ctypes.c_void_p]
        try:
            m.push(streams)
            cm = m.fetch_commands()
            g1 = guards(m.h)
            fr = m.fetch_frames()
            g2 = guards(m.h)
            _cache['one_push'] = dict(cm=cm, fr=fr, guards=(g1, g2), got=[tuple(a.copy() for a in cm.commands_of(k)) for k in range(len(rows))],
                                      state=[state_bytes(m.fsm_state(k)) for k in range(len(rows))])
        finally:
            m.close()
    return _cache['one_push']


@pytest.mark.gpu
def test_gpu_256_streams_in_one_push():
    rows, res = fixture()['gpu'], gpu_one_push()
    cm, fr = res['cm'], res['fr']
    assert res['guards'] == (0, 0)
    assert cm.stream_flags.tolist() == [0] * len(rows)
    assert sum(len(g[0]) for g in res['got']) == sum(len(r.packets) for r in rows) > 4000   # every oracle packet became a command
    assert sum(int(((g[0]['flags'] & fsm.FRAME_ENCRYPTED) != 0).sum()) for g in res['got']) > 1500   # ... a good part of them inside sessions
    for k, row in enumerate(rows):
        want_frames = frames_of(row)
        raw = fr.frames_of(k)
        for t in (0, 1):   # fetch_frames gives the fixture's oracle packets as frames (idx: the twin's is a list position)
            for name in ('byte_off', 'n_bytes', 'n_bits', 'flags', 'type', 'reserved'):
                assert raw.records[t][name].tolist() == want_frames.records[t][name].tolist(), (k, t, name)
            assert raw.bytes[t].tobytes() == want_frames.bytes[t].tobytes() and raw.par[t].tobytes() == want_frames.par[t].tobytes(), (k, t)
        assert raw.table['type'].tolist() == [t for t, _ in row.packets], k
        got = cm.commands_of(k)
        h = host_for_stream(k, row)
        assert_commands_equal(got, run_host(h, raw), raw.table['n_bytes'])
        st = fsm.state_init()
        st.key_a[:], st.key_b[:] = row.keys
        twin = fsm.host_commands(st, raw.table, raw.bytes, raw.par, sector_keys=full_table(row.keys) if k % 3 == 2 else None)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, twin)), k
        assert res['state'][k] == state_bytes(st) == state_bytes(h.get_state()), k
        # the reference's text, up to the frame where it raised
        table, data, enc = got
        text = dispatched(table[:row.compared], data, enc)
        assert normalise(text) == normalise(''.join(row.texts[:row.compared])), (k, row.index)


@pytest.mark.gpu
def test_gpu_three_ragged_pushes_equal_the_one_push():
    streams, rows, want = gpu_streams(), fixture()['gpu'], gpu_one_push()
    K = len(rows)
    lens = np.array([len(s) // 2 for s in streams])
    parts, done, empty = [[] for _ in range(K)], np.zeros(K, np.int64), 0
    # the first two pieces by the PIECES pattern (zero-length ones included), the third takes the rest
    sizes = [np.minimum(lens, [PIECES[k % 3] for k in range(K)])]
    sizes.append(np.minimum(lens - sizes[0], [PIECES[(1 + k) % 3] for k in range(K)]))
    sizes.append(lens - sizes[0] - sizes[1])
    with tracked(list(enumerate(rows)), int(max(n.max() for n in sizes))) as m:
        for n in sizes:
            m.push([s[2 * a:2 * (a + b)] for s, a, b in zip(streams, done, n)])
            cm = m.fetch_commands()
            for k in range(K):
                parts[k].append(tuple(a.copy() for a in cm.commands_of(k)))
                empty += int(n[k] == 0)
            done += n
        assert empty >= K // 3 and (done == lens).all()
        for k in range(K):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(concatenated(parts[k]), want['got'][k])), k
            assert state_bytes(m.fsm_state(k)) == want['state'][k], k


@pytest.mark.gpu
def test_gpu_hand_off_device_host_device_in_a_mutated_session():
    streams, rows, want = gpu_streams(), fixture()['gpu'], gpu_one_push()
    pick = []   # mutated sessions: four each of the short-UID, cut-{nt}, 9k + r and AUTHB families
    for family in (1, 3, 4, 5):
        pick += [k for k, row in enumerate(rows) if row.family == family and sum(row.sess) >= 8][:4]
    assert len(pick) == 16
    cut = 24000   # complex samples: the first session is up in the Classic captures
    with tracked([(k, rows[k]) for k in pick], max(cut, max(len(streams[k]) // 2 for k in pick) - cut)) as m:
        m.push([streams[k][:2 * cut] for k in pick])
        cm = m.fetch_commands()
        head = [tuple(a.copy() for a in cm.commands_of(j)) for j in range(16)]
        up = 0
        for j, k in enumerate(pick):   # device -> host machine -> device
            st = m.fsm_state(j)
            up += int(st.encrypted != 0)
            h = host_machine()
            h.set_state(st)
            assert state_bytes(h.get_state()) == state_bytes(st)
            m.set_fsm_state(j, h.get_state())
        assert up >= 8
        m.push([streams[k][2 * cut:] for k in pick])
        cm = m.fetch_commands()
        for j, k in enumerate(pick):
            tail = tuple(a.copy() for a in cm.commands_of(j))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(concatenated([head[j], tail]), want['got'][k])), k
            assert state_bytes(m.fsm_state(j)) == want['state'][k], k
