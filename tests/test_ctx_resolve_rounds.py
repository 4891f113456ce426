"""The single-stream resolve (csrc/ctx_commands.hip.h: k_ctx_resolve) where re-runs cross its rounds.  The speculative walk is one text
with the CPU twin; the resolve is not: the twin judges one summary at a time, the kernel a round of THREADS summaries by ballot and
shuffle, and carries four scalars from round to round -- c_enc, c_key, c_sess, c_flags.  It judges a round again behind every lane it
walks again, and rebuilds that lane's true machine from pieces: the end machine of the segment before, cur_key from the chain, the
session words from the last segment that wrote them, the flags from two ballots and the carry.  tests/test_ctx_commands.py keeps
every re-run in lanes 0 .. 2 of the first round and every capture of more than one round free of re-runs, key readers, session words
and flags.  Here the failures sit ON the lines.

THE LINES ARE READ, NOT REMEMBERED: constants() takes THREADS, the round's stride and the segment scan's tile out of the source text,
and place() turns a segment index into (round, lane): round r >= 1 holds segments (r - 1) * THREADS + 1 .. r * THREADS, segment 0 is
exact and in no round.  Every case asserts from them where its re-runs, key readers and writers fall, and that its frames stay inside one
tile of the segment scan (tests/test_ctx_commands.py: test_4201_frames crosses that one), so the only lines crossed are the resolve's.

THE BUILDING BLOCKS.  PAIR: a plain REQA and a two-byte ATQA; every pair behind frame 0 opens a segment.  open_session(key_type, key,
seed, p, close): a Classic transaction without its HALT, then p PAIRs heard INSIDE the session -- ciphertext to the machine, each a cut
by its raw frame: p segments that are walked again -- and, with close, the session's HALT, encrypted p pairs later.  (What a pair
decrypts to depends on the nonce: under about one seed in five some pair of 70 ends the session early for the machine.  The seeds
below are ones under which none does, and the counters held as literals say so.)
nonce_by_stage_closed(key, seed): a RANDTA by stage, which reads the cur_key an EARLIER transaction left, closed by an encrypted HALT.
overflow_txn(): REQA, ATQA and nine anticollision pairs, which raise NFC_FSM_UID_OVERFLOW.

THE CPU HALF re-derives what the twin counts from the sequential machine alone (plan(): the machine entering every segment, by
nfc_host_commands_keyed on the frames before it), pins the twin in three orders, and holds the counters as literals.  THE GPU HALF
renders the same frame lists to IQ, one tracked NfcContext per case, every batch through batch_equals_the_twins: records, data and enc
byte for byte, the 88 state bytes against both twins, the counters, the flags and src.  Every comparison is for equality.

WHAT EACH CARRY LOSES, tried once per line on an MI355X with that carry's update taken out of k_ctx_resolve.  Without c_enc, lane 0
of a later round stands where it must not: case 1 wherever a failure sits in lane 0 (60-10-5, 64-64-3, 127-3-2) and case 5's final
round of one lane that is walked again (S 66, 130).  Without c_key, the final cur_key is segment 0's in every test of case 2, and with
gap 70 the RANDRB behind the nonce by stage in round 2 is decrypted with the wrong key: the records differ.  Without c_flags, the
overflow raised in round 1 is gone from the batch's flags (case 4).  tests/test_ctx_commands.py passes under each of the three.
Without ANY update of c_sess the final cipher, ar and at are segment 0's, which routes (b) and (c) of that file see as well; with
c_sess updated in round 1 ONLY that file passes, and here every session written in a later round shows."""
import io
import os
import re

import numpy as np
import pytest

from tests.test_commands_host import state_bytes
from tests.test_ctx_commands_host import (A, AUTHA, AUTHB, B, HALT, KA, KB, RANDRB, RANDTA, REQA_BITS, TABLE_C, classic_txn,
                                          copy_state, crc, in_batches, keyed_state, nonce_by_stage_txn, segmented_equals_sequential)
from tests.test_frames import host_frames_of
from usrp_nfc_amd import _lib, fsm, synth
from usrp_nfc_amd.command import CommandType

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')
PAIR = [(1, REQA_BITS), (0, synth.frame_bits([0x04, 0x00]))]
KEYS_A = (KA, KA)
KEYS_C = (KA, [0x11] * 6)   # route (c)'s: key A right, key B only in the table
MAX_SAMPLES = 1 << 18
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- 0. the lines, from the source text ------------------------------------------------------------------------------------------------
class Constants(object):
    pass


def _number(text, name, pattern):
    m = re.search(pattern, text)
    assert m, 'ctx_commands.hip.h: no definition of %s matches %r any more' % (name, pattern)
    return int(m.group(1))


def constants():
    def read():
        text = open(os.path.join(CSRC, 'ctx_commands.hip.h')).read()
        c = Constants()
        c.THREADS = _number(text, 'THREADS', r'constexpr\s+int\s+THREADS\s*=\s*(\d+)\s*;')
        c.ROUND = _number(text, 'the stride of a resolve round', r'for\s*\(uint32_t\s+base\s*=\s*1\s*;\s*base\s*<\s*S\s*;\s*base\s*\+=\s*(\d+)\s*\)')
        c.SG_THREADS = _number(text, 'SG_THREADS', r'\bSG_THREADS\s*=\s*(\d+)\s*[,;]')
        c.SG_ITEMS = _number(text, 'SG_ITEMS', r'\bSG_ITEMS\s*=\s*(\d+)\s*[,;]')
        assert re.search(r'\bSG_TILE\s*=\s*SG_THREADS\s*\*\s*SG_ITEMS\s*;', text), 'ctx_commands.hip.h: SG_TILE is no longer SG_THREADS * SG_ITEMS'
        assert re.search(r'__launch_bounds__\(THREADS\)\s*void\s+k_ctx_resolve\b', text), 'ctx_commands.hip.h: k_ctx_resolve is no longer THREADS wide'
        c.SG_TILE = c.SG_THREADS * c.SG_ITEMS
        return c
    return cached('constants', read)


def place(k):
    """Segment k >= 1 -> (round, lane) of the resolve: round 1 holds segments 1 .. THREADS."""
    assert k >= 1
    return (k - 1) // constants().THREADS + 1, (k - 1) % constants().THREADS


def test_the_lines_are_read_from_the_source():
    c = constants()
    assert c.THREADS > 0 and c.ROUND == c.THREADS, 'a resolve round is no longer one lane per thread'
    assert c.SG_TILE > 0 and c.SG_THREADS % 64 == 0
    assert place(1) == (1, 0) and place(c.THREADS) == (1, c.THREADS - 1) and place(c.THREADS + 1) == (2, 0)
    with pytest.raises(AssertionError, match='NO_SUCH_NAME'):   # a pattern that no longer matches fails loudly
        _number('constexpr int THREADS = 64;', 'NO_SUCH_NAME', r'\bNO_SUCH_NAME\s*=\s*(\d+)')


# ---- the building blocks -----------------------------------------------------------------------------------------------------------------
def hearing(key, packets):
    """A machine keyed with `key` that has heard `packets`: where the machine that generated them stands."""
    m = fsm.fsm(out=io.StringIO())
    m.set_keys(key, key)
    for t, bits in packets:
        m.process_bits(bits, t)
    return m


def encrypted_halt(m):
    return [(1, m.process_outgoing(synth.frame_bits(crc([0x50, 0x00])), CommandType.by_index(HALT)))]


def open_session(key_type, key, seed, p, close):
    packets = classic_txn(key_type, key, seed, halt=False)
    m = hearing(key, packets)
    assert m.get_state().encrypted == 1
    for _ in range(p):
        for t, bits in PAIR:   # the generator hears them too: its cipher stays in step with the observer's
            packets.append((t, bits))
            m.process_bits(bits, t)
    if close:
        packets += encrypted_halt(m)
    return packets


def nonce_by_stage_closed(key, seed):
    packets = nonce_by_stage_txn(key, seed)
    m = hearing(key, packets)
    assert m.get_state().encrypted == 1
    return packets + encrypted_halt(m)


def overflow_txn():
    """tests/test_commands_host.py: test_uid_capacity_is_32_bytes -- the ninth anticollision answer does not fit the UID."""
    packets = list(PAIR)
    for i in range(9):
        uid = [0x10 + i, 0x20 + i, 0x30 + i, 0x40 + i]
        packets += [(1, synth.frame_bits([0x93, 0x20])), (0, synth.frame_bits(uid + [uid[0] ^ uid[1] ^ uid[2] ^ uid[3]]))]
    return packets


# ---- the cases: name -> (packets, keys, table) -------------------------------------------------------------------------------------------
EDGE = [(60, 10, 5), (63, 1, 70), (64, 64, 3), (127, 3, 2)]   # case 1: (a, p, q)
EDGE_SEEDS = {(60, 10, 5): 0x1000, (63, 1, 70): 0x1001, (64, 64, 3): 0x1002, (127, 3, 2): 0x1004}
EDGE_COUNTERS = {(60, 10, 5): (76, 10, 21), (63, 1, 70): (135, 1, 3), (64, 64, 3): (132, 64, 129), (127, 3, 2): (133, 3, 7)}
KEY_GAPS = [3, 70]                                             # case 2
LAST = [64, 65, 66, 129, 130]                                  # case 5: segments
SPLIT_CUTS = [10, 14, 15]                                      # case 6: the frame the second push starts with


def case_packets(name):
    kind, arg = name[0], name[1:]
    if kind == 'edge':
        a, p, q = arg
        return PAIR * a + open_session(A, KA, EDGE_SEEDS[arg], p, True) + PAIR * q, KEYS_A, None
    if kind == 'key':
        gap, = arg
        return (PAIR * 2 + classic_txn(B, KB, 0x9C42) + PAIR * gap + nonce_by_stage_closed(KB, 0x51E8) + nonce_by_stage_closed(KB, 0x0B6D)
                + PAIR * 3), KEYS_C, TABLE_C
    if kind == 'sess':
        with_reruns, = arg
        if not with_reruns:
            return PAIR * 5 + classic_txn(A, KA, 0x77A1) + PAIR * 140, KEYS_A, None
        return PAIR * 5 + classic_txn(A, KA, 0x77A1) + PAIR * 66 + open_session(A, KA, 0x1005, 3, True) + PAIR * 70, KEYS_A, None
    if kind == 'flags':
        return PAIR * 4 + overflow_txn() + PAIR * 66 + open_session(A, KA, 0x1007, 4, True) + PAIR * 2, KEYS_A, None
    if kind == 'carried_flags':
        return PAIR * 100 + open_session(A, KA, 0x1009, 2, True) + PAIR * 30, KEYS_A, None
    if kind == 'last':
        S, p = arg
        return PAIR * (S - 1 - p) + open_session(A, KA, 0x4000 + S, p, False), KEYS_A, None
    if kind == 'split':
        return PAIR * 2 + open_session(A, KA, 0x100A, 70, True) + PAIR * 3, KEYS_A, None
    if kind == 'reader_only':
        return [PAIR[0]] * 70, None, None
    if kind == 'tag_only':
        return [PAIR[1]] * 70, None, None
    raise KeyError(name)


def case(*name):
    """-> (packets, NfcFrames, keys, table), made once and read-only."""
    def make():
        packets, keys, table = case_packets(name)
        fr = host_frames_of(packets)[0]
        for a in (fr.table,) + tuple(fr.bytes) + tuple(fr.par):
            a.setflags(write=False)
        assert len(fr.table) == len(packets) < constants().SG_TILE   # one tile of the segment scan: the lines crossed are the resolve's
        return packets, fr, keys, table
    return cached(name, make)


# ---- what the resolve has to find, from the sequential machine alone ---------------------------------------------------------------------
def cuts_of(frames, rows=None):
    """The frames that open a segment, by the raw frame alone (ctxcmd::is_cut), frame 0 first."""
    t = frames.table if rows is None else rows
    starts = [0]
    for m in range(1, len(t)):
        r = t[m]
        if int(r['type']) == 1 and int(r['n_bytes']) == 1 and not int(r['flags']) & _lib.NFC_RAW_CUT and int(r['flags']) & _lib.NFC_RAW_PARITY_OK:
            if int(frames.bytes[1][int(r['byte_off'])]) in (0x26, 0x52):
                starts.append(m)
    return starts


class Plan(object):
    pass


def plan(frames, keys=None, table=None, start=None, rows=None):
    """Which segments the resolve must walk again and which read the carried cur_key, re-derived WITHOUT the twin: the machine entering
    segment k is nfc_host_commands_keyed's on the frames before it.  Segment k >= 1 is walked again iff that machine is inside a session,
    or the segment holds a RANDTA by stage in front of any AUTH of its own and the machine's cur_key is not the batch's carried one."""
    t = frames.table if rows is None else rows
    start = start if start is not None else keyed_state(keys)
    whole = copy_state(start)
    seq = fsm.host_commands(whole, t, frames.bytes, frames.par, sector_keys=table)[0]
    p = Plan()
    p.starts = cuts_of(frames, t)
    p.n_segments = len(p.starts) if len(t) else 0
    p.rerun, p.keydep, p.rerun_frames = [], [], 0
    edges = p.starts + [len(t)]
    for k in range(1, len(p.starts)):
        st = copy_state(start)
        fsm.host_commands(st, t[:edges[k]], frames.bytes, frames.par, sector_keys=table)
        cmds = seq['cmd'][edges[k]:edges[k + 1]].tolist()
        reads = False
        if st.encrypted == 0 and RANDTA in cmds:
            before = cmds[:cmds.index(RANDTA)]
            reads = AUTHA not in before and AUTHB not in before
        if reads:
            p.keydep.append(k)
        if st.encrypted != 0 or (reads and st.cur_key != start.cur_key):
            p.rerun.append(k)
            p.rerun_frames += edges[k + 1] - edges[k]
    p.final, p.table = whole, seq
    return p


def counters(n_segments, n_rerun_segments=0, n_rerun_frames=0, n_keydep_segments=0):
    return dict(n_segments=n_segments, n_rerun_segments=n_rerun_segments, n_rerun_frames=n_rerun_frames, n_keydep_segments=n_keydep_segments)


def twin_and_plan(name, want, start=None, rows=None):
    """The CPU half of a case: the twin in three orders against the sequential machine, its counters against the literal `want` and
    against the plan.  -> (the plan, the final state)."""
    packets, frames, keys, table = case(*name)
    cn, st = segmented_equals_sequential(frames, keys, table, start=start, rows=rows)
    p = plan(frames, keys, table, start=start, rows=rows)
    assert cn == want
    assert cn == counters(p.n_segments, len(p.rerun), p.rerun_frames, len(p.keydep))
    assert state_bytes(st) == state_bytes(p.final)
    return p, st


def session_words(st):
    return int(st.cipher), bytes(st.ar), bytes(st.at)


def assert_session_words_are_set(st):
    cipher, ar, at = session_words(st)
    assert cipher != 0 and any(ar) and any(at)


# ---- case 1: re-runs across a round edge (c_enc; a predecessor in the round before) --------------------------------------------------------
def check_edge(a, p, q):
    T = constants().THREADS
    S, rr, rf = EDGE_COUNTERS[(a, p, q)]
    pl, st = twin_and_plan(('edge', a, p, q), counters(S, rr, rf))
    assert pl.rerun == list(range(a + 1, a + p + 1)) and st.encrypted == 0
    first, last = place(a + 1), place(a + p)
    if (a, p, q) == (60, 10, 5):      # the failures straddle rounds 1 | 2: lane 0 of round 2 fails on the carried encrypted alone
        assert first == (1, T - 4) and last == (2, 5) and place(T + 1) == (2, 0) and a + 1 <= T < T + 1 <= a + p
    elif (a, p, q) == (63, 1, 70):    # the one failure is the last lane of round 1; rounds 2 and 3 stand
        assert first == last == (1, T - 1) and place(S - 1)[0] == 3
    elif (a, p, q) == (64, 64, 3):    # the session opens in the last lane of round 1: lane 0 of round 2 takes its cipher from the carried
                                      # session segment; every lane of round 2 is walked again; round 3 stands
        assert place(a) == (1, T - 1) and first == (2, 0) and last == (2, T - 1) and place(S - 1) == (3, 2)
    else:                             # the failures straddle rounds 2 | 3
        assert (a, p, q) == (127, 3, 2) and first == (2, T - 1) and last == (3, 1)
    return pl


@pytest.mark.parametrize('a,p,q', EDGE)
def test_reruns_across_a_round_edge_on_the_twin(a, p, q):
    check_edge(a, p, q)


# ---- case 2: cur_key from an earlier round, a round judged again behind a re-run -----------------------------------------------------------
def check_key(gap):
    T = constants().THREADS
    pl, st = twin_and_plan(('key', gap), counters(8 + gap, 2, 18, 2))
    writer, readers = 2, [3 + gap, 4 + gap]
    assert pl.rerun == pl.keydep == readers and st.cur_key == 2 + 40 + 3 and st.encrypted == 0
    assert AUTHB in pl.table['cmd'][pl.starts[writer]:pl.starts[writer + 1]].tolist()
    assert place(writer) == (1, 1)
    if gap == 3:       # writer and readers in round 1: the key comes from a lane below
        assert [place(k) for k in readers] == [(1, 5), (1, 6)]
    else:              # the writer in round 1, both readers in round 2: the carried key for the first, the re-run lane's for the second
        assert gap == 70 and [place(k) for k in readers] == [(2, 8), (2, 9)] and readers[0] > T
    rows = np.flatnonzero(pl.table['cmd'] == RANDRB)
    assert len(rows) == 3 and int((pl.table['flags'] & fsm.FRAME_AR_OK != 0).sum()) == 3
    for k in readers:   # what a wrong incoming key loses
        r = [m for m in rows.tolist() if pl.starts[k] <= m < pl.starts[k + 1]]
        assert len(r) == 1 and pl.table['flags'][r[0]] & fsm.FRAME_AR_OK
    return pl


def key_parts(gap):
    """The same capture as two batches, the first ending behind the AUTHB transaction: (frames of the first, frames from there on)."""
    packets, frames, keys, table = case('key', gap)
    first = 2 * 2 + len(classic_txn(B, KB, 0x9C42))
    return first, packets, frames, keys, table


def check_key_standing(gap):
    first, packets, frames, keys, table = key_parts(gap)
    start = keyed_state(keys)
    fsm.host_commands(start, frames.table[:first], frames.bytes, frames.par, sector_keys=table)
    assert start.cur_key == 45 and start.encrypted == 0
    pl, st = twin_and_plan(('key', gap), counters(5 + gap, 0, 0, 2), start=copy_state(start), rows=frames.table[first:])
    assert pl.keydep == [gap, gap + 1] and pl.rerun == [] and int((pl.table['flags'] & fsm.FRAME_AR_OK != 0).sum()) == 2
    if gap == 70:
        assert [place(k) for k in pl.keydep] == [(2, 5), (2, 6)]
    return pl


@pytest.mark.parametrize('gap', KEY_GAPS)
def test_cur_key_from_an_earlier_segment_on_the_twin(gap):
    check_key(gap)
    check_key_standing(gap)


# ---- case 3: session words held over rounds that write none (c_sess) ------------------------------------------------------------------------
def check_sess(with_reruns):
    T = constants().THREADS
    if not with_reruns:
        pl, st = twin_and_plan(('sess', False), counters(146))
        assert pl.rerun == [] and place(5) == (1, 4) and place(pl.n_segments - 1)[0] == 3   # written in round 1, two rounds that write none
    else:
        pl, st = twin_and_plan(('sess', True), counters(146, 3, 7))
        assert pl.rerun == [73, 74, 75] and place(72) == (2, 7) and 72 >= 70 > T and place(pl.n_segments - 1)[0] == 3
    assert st.encrypted == 0
    assert_session_words_are_set(st)
    # they are the words of the LAST session: the machine behind that session's HALT holds the same
    closed = pl.starts[76] if with_reruns else pl.starts[6]
    packets, frames, keys, table = case('sess', with_reruns)
    behind = keyed_state(keys)
    fsm.host_commands(behind, frames.table[:closed], frames.bytes, frames.par)
    assert pl.table['cmd'][closed - 1] == HALT and behind.encrypted == 0 and session_words(st) == session_words(behind)
    return pl, st


@pytest.mark.parametrize('with_reruns', [False, True], ids=['standing', 'reruns_in_round_2'])
def test_session_words_over_rounds_that_write_none_on_the_twin(with_reruns):
    check_sess(with_reruns)


# ---- case 4: flags carried into a re-run and out of the batch (c_flags) -----------------------------------------------------------------------
def check_flags():
    T = constants().THREADS
    pl, st = twin_and_plan(('flags',), counters(78, 4, 9))
    assert pl.rerun == [72, 73, 74, 75] and st.flags == _lib.NFC_FSM_UID_OVERFLOW and st.encrypted == 0
    assert place(4) == (1, 3) and place(72) == (2, 7) and 4 <= T < 72   # raised in round 1, the re-runs in round 2
    # the flag is that segment's alone
    packets, frames, keys, table = case('flags')
    before, behind = keyed_state(keys), keyed_state(keys)
    fsm.host_commands(before, frames.table[:pl.starts[4]], frames.bytes, frames.par)
    fsm.host_commands(behind, frames.table[:pl.starts[5]], frames.bytes, frames.par)
    assert before.flags == 0 and behind.flags == _lib.NFC_FSM_UID_OVERFLOW
    return pl


def carried_flags_start():
    start = keyed_state(KEYS_A)
    start.flags = _lib.NFC_FSM_LOST | _lib.NFC_FSM_UID_OVERFLOW
    return start


def check_carried_flags():
    pl, st = twin_and_plan(('carried_flags',), counters(133, 2, 5), start=carried_flags_start())
    assert pl.rerun == [101, 102] and place(101) == (2, 36) and pl.n_segments >= 130
    assert st.flags == _lib.NFC_FSM_LOST | _lib.NFC_FSM_UID_OVERFLOW and st.encrypted == 0
    return pl


def test_flags_into_a_rerun_and_out_of_the_batch_on_the_twin():
    check_flags()
    check_carried_flags()


# ---- case 5: the last round's edges ---------------------------------------------------------------------------------------------------------
def check_last(S, p):
    T = constants().THREADS
    pl, st = twin_and_plan(('last', S, p), counters(S, p, 2 * p))
    assert pl.n_segments == S and pl.rerun == ([S - 1] if p else []) and st.encrypted == 1
    assert_session_words_are_set(st)
    rnd, lane = place(S - 1)
    # S - 1 segments in the rounds: one lane short of a full round, exactly full rounds, a final round of one lane
    assert (S - 1) % T in (T - 1, 0, 1) and lane == (S - 2) % T and rnd == (S - 2) // T + 1
    assert {64: (1, T - 2), 65: (1, T - 1), 66: (2, 0), 129: (2, T - 1), 130: (3, 0)}[S] == (rnd, lane)
    return pl, st


@pytest.mark.parametrize('p', [0, 1], ids=['last_opens_a_session', 'last_is_walked_again'])
@pytest.mark.parametrize('S', LAST)
def test_the_last_rounds_edges_on_the_twin(S, p):
    check_last(S, p)


# ---- case 6: a batch that starts inside a session, many segments long -------------------------------------------------------------------------
@pytest.mark.parametrize('cut', SPLIT_CUTS)
def test_a_batch_that_starts_inside_a_session_on_the_twin(cut):
    T = constants().THREADS
    packets, frames, keys, table = case('split')
    twin_and_plan(('split',), counters(76, 70, 141))
    st, rerun = in_batches(frames, keys, table, (cut,))
    assert rerun == 70 and st.encrypted == 0
    # the second batch: its segment 0 ends encrypted, its segments 1 .. 70 are walked again -- lane 0 of round 1 on the INITIAL carry, then
    # through the edge of rounds 1 | 2
    start = keyed_state(keys)
    fsm.host_commands(start, frames.table[:cut], frames.bytes, frames.par)
    assert (start.encrypted != 0) == (cut > 13)   # (frame 10 is the AUTHA, frames 11 .. 13 are the nonces)
    pl, _ = twin_and_plan(('split',), counters(74, 70, 141), start=copy_state(start), rows=frames.table[cut:])
    assert pl.rerun == list(range(1, 71)) and place(1) == (1, 0) and place(70) == (2, 70 - T - 1) and T < 70


# ---- case 7: one type absent ------------------------------------------------------------------------------------------------------------------
def test_one_type_absent_on_the_twin():
    pl, _ = twin_and_plan(('reader_only',), counters(70))
    assert len(pl.table) == 70 and set(pl.table['type'].tolist()) == {1} and place(69)[0] == 2
    pl, _ = twin_and_plan(('tag_only',), counters(1))
    assert len(pl.table) == 70 and set(pl.table['type'].tolist()) == {0}


# ================================================================ the GPU half ================================================================
gpu = pytest.mark.gpu


def rendered(name, cuts=(), gap_us=60.0):
    """The case's packets as IQ, one capture per part (each with the idle lead of a capture of its own), read-only."""
    def make():
        from tests.test_ctx_commands import iq_of
        packets = case(*name)[0]
        edges = [0] + list(cuts) + [len(packets)]
        parts = [iq_of(packets[a:b], gap_us=gap_us) for a, b in zip(edges[:-1], edges[1:])]
        for iq in parts:
            iq.setflags(write=False)
            assert len(iq) // 2 < MAX_SAMPLES
        return parts
    return cached(('iq', name, tuple(cuts), gap_us), make)


def on_the_gpu(name, cuts=(), start=None, gap_us=60.0):
    """One tracked NfcContext over the case, a push per part; every batch through batch_equals_the_twins and against the twin on the
    frames the capture was rendered from.  -> [(NfcCommands, its batch's counters)], the final state."""
    from tests.test_ctx_commands import batch_equals_the_twins, context
    packets, frames, keys, table = case(*name)
    edges = [0] + list(cuts) + [len(packets)]
    out = []
    with context(keys, table) as c:
        state = copy_state(start) if start is not None else keyed_state(keys)
        if start is not None:
            c.set_fsm_state(start)
        crafted = copy_state(state)
        for iq, a, b in zip(rendered(name, cuts, gap_us), edges[:-1], edges[1:]):
            c.push(iq)
            cm, raw = batch_equals_the_twins(c, state, table)
            want = fsm.host_commands_segmented(crafted, frames.table[a:b], frames.bytes, frames.par, sector_keys=table)
            # the capture decoded to the frame list it was rendered from
            assert cm.table['cmd'].tolist() == want[0]['cmd'].tolist() and cm.counters == want[3]
            assert state_bytes(c.fsm_state()) == state_bytes(crafted)
            out.append(cm)
        return out, c.fsm_state()


@gpu
@pytest.mark.parametrize('a,p,q', EDGE)
def test_reruns_across_a_round_edge(a, p, q):
    check_edge(a, p, q)
    S, rr, rf = EDGE_COUNTERS[(a, p, q)]
    (cm,), st = on_the_gpu(('edge', a, p, q))
    assert cm.counters == counters(S, rr, rf) and st.encrypted == 0
    enc = (cm.table['flags'] & fsm.FRAME_ENCRYPTED) != 0
    halt = 2 * a + 12 + 2 * p   # (a pairs, the transaction's twelve frames, p pairs)
    assert enc[halt - 2 * p:halt + 1].all() and not enc[halt + 1:].any() and cm.table['cmd'][halt] == HALT   # the pairs in the session are ciphertext


@gpu
@pytest.mark.parametrize('gap', KEY_GAPS)
def test_cur_key_from_an_earlier_segment(gap):
    pl = check_key(gap)
    (cm,), st = on_the_gpu(('key', gap))
    assert cm.counters == counters(8 + gap, 2, 18, 2) and st.cur_key == 45
    rows = np.flatnonzero(cm.table['cmd'] == RANDRB)
    assert len(rows) == 3 and all(cm.table['flags'][m] & fsm.FRAME_AR_OK for m in rows.tolist())
    assert [sum(pl.starts[k] <= m < pl.starts[k + 1] for m in rows.tolist()) for k in (2, 3 + gap, 4 + gap)] == [1, 1, 1]


@gpu
@pytest.mark.parametrize('gap', KEY_GAPS)
def test_cur_key_carried_into_the_batch_stands(gap):
    check_key_standing(gap)
    first = key_parts(gap)[0]
    (cm0, cm), st = on_the_gpu(('key', gap), cuts=(first,))
    assert cm0.counters == counters(3) and cm.counters == counters(5 + gap, 0, 0, 2) and st.cur_key == 45
    rows = np.flatnonzero(cm.table['cmd'] == RANDRB)
    assert len(rows) == 2 and all(cm.table['flags'][m] & fsm.FRAME_AR_OK for m in rows.tolist())


@gpu
@pytest.mark.parametrize('with_reruns', [False, True], ids=['standing', 'reruns_in_round_2'])
def test_session_words_over_rounds_that_write_none(with_reruns):
    _, want = check_sess(with_reruns)
    (cm,), st = on_the_gpu(('sess', with_reruns))
    assert cm.counters == (counters(146, 3, 7) if with_reruns else counters(146))
    assert_session_words_are_set(st)
    assert int(st.cipher) == int(want.cipher) and bytes(st.ar) == bytes(want.ar) and bytes(st.at) == bytes(want.at)


@gpu
def test_flags_into_a_rerun_and_out_of_the_batch():
    check_flags()
    (cm,), st = on_the_gpu(('flags',))
    assert cm.counters == counters(78, 4, 9)
    assert cm.flags == st.flags == _lib.NFC_FSM_UID_OVERFLOW


@gpu
def test_flags_the_batch_was_entered_with():
    check_carried_flags()
    both = _lib.NFC_FSM_LOST | _lib.NFC_FSM_UID_OVERFLOW
    (cm,), st = on_the_gpu(('carried_flags',), start=carried_flags_start())
    assert cm.counters == counters(133, 2, 5) and cm.n_segments >= 130
    assert cm.flags == st.flags == both


@gpu
@pytest.mark.parametrize('p', [0, 1], ids=['last_opens_a_session', 'last_is_walked_again'])
@pytest.mark.parametrize('S', LAST)
def test_the_last_rounds_edges(S, p):
    _, want = check_last(S, p)
    (cm,), st = on_the_gpu(('last', S, p))
    assert cm.counters == counters(S, p, 2 * p) and st.encrypted == 1
    assert_session_words_are_set(st)
    assert session_words(st) == session_words(want)


@gpu
@pytest.mark.parametrize('cut', SPLIT_CUTS[1:])
def test_a_batch_that_starts_inside_a_session(cut):
    (cm0, cm), st = on_the_gpu(('split',), cuts=(cut,))
    assert cm0.counters == counters(3) and cm.counters == counters(74, 70, 141)
    assert cm.table['flags'][0] & fsm.FRAME_ENCRYPTED and st.encrypted == 0   # the push starts inside the session and ends outside it


@gpu
def test_one_type_absent():
    (cm,), _ = on_the_gpu(('reader_only',))
    assert cm.counters == counters(70) and cm.n_commands == 70 and set(cm.table['type'].tolist()) == {1}
    (cm,), _ = on_the_gpu(('tag_only',))
    assert cm.counters == counters(1) and cm.n_commands == 70 and set(cm.table['type'].tolist()) == {0}
