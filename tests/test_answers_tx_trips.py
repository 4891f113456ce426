"""The answer-transmit kernels where tiles, spans and pushes turn over: k_answers_tx_schedule, k_answers_tx_render (csrc/answers_tx.hip.h)
and the host layout of nfc_multi_transmit_device (csrc/nfc_multi.hip).  tests/test_answers_tx.py feeds them two cards'
answers in streams tens of thousands of samples long; here a tile meets many streams and many spans, every answer shape goes through the
block scan, runs of no samples are stepped over, an answer outlasts many pushes, waits in front of one, is cut by a command, and streams
and answers end on the edges of a tile.

EVERY SCENARIO IS A CPU TEST AND A GPU TEST OVER THE SAME INPUTS.  The CPU half asserts, from the constants READ out of answers_tx.hip.h
(constants()), that the input crosses the line it is there for, and that the twin (emulate.host_transmit) equals the numpy restatement of
the schedule (`_model`, tests/test_answers_tx_host.py) per stream: the twin shares schedule_stream's text with the kernel, so only that
equality makes it a yardstick at these inputs.  The GPU half holds the device against the twin: the same bytes in the buffer, the same
layout, the same pending entries, the sentinels behind the layout untouched, every guard word intact.

ANSWERS WITHOUT A CARD CRAFTED FOR THEM: a stream that holds a card and receives an unmodulated carrier answers nothing, and
set_tx_state(k, entry) gives it a pending entry of any shape, start and role, which the next transmit() schedules and renders as a span."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests.test_answers_tx import SENTINEL, _buffer, _context, _pend_bytes, _piece_cuts, _push_transmit  # noqa: F401
from tests.test_answers_tx_host import IDLE, N_BITS, _model, in_pieces, one_stream, pack, wave
from tests.test_emulate import _reader_side_streams, _replay_cards
from tests.test_second_trips import _number, expected_pushes
from usrp_nfc_amd import _lib, emulate, fsm, tx

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')
TAG, READER = emulate.NFC_EMU_TAG, emulate.NFC_EMU_READER
IN_RATE = 2e6
gpu = pytest.mark.gpu
_cache = {}


def cached(key, make):
    """made once, shared by the tests that need it, and left unchanged (a cache of this file's own: its keys are not another file's)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- 0. the thresholds, from the source text --------------------------------------------------------------------------------------------
class Constants(object):
    pass


def constants():
    def read():
        c = Constants()
        text = open(os.path.join(CSRC, 'answers_tx.hip.h')).read()
        c.BLOCK = _number(text, 'BLOCK', r'constexpr\s+int\s+BLOCK\s*=\s*(\d+)\s*,', 'answers_tx.hip.h')
        c.PER_THREAD = _number(text, 'PER_THREAD', r'\bPER_THREAD\s*=\s*(\d+)\s*,', 'answers_tx.hip.h')
        assert re.search(r'\bTILE\s*=\s*BLOCK\s*\*\s*PER_THREAD\s*;', text), 'answers_tx.hip.h: TILE is no longer BLOCK * PER_THREAD'
        c.TILE = c.BLOCK * c.PER_THREAD
        c.SCHED_BLOCK = _number(text, 'SCHED_BLOCK', r'constexpr\s+int\s+SCHED_BLOCK\s*=\s*(\d+)\s*;', 'answers_tx.hip.h')
        c.MAX_BITS = _number(text, 'MAX_BITS', r'constexpr\s+uint32_t\s+MAX_BITS\s*=\s*(\d+)\s*;', 'answers_tx.hip.h')
        c.ANS_BYTES = _number(text, 'ANS_BYTES', r'constexpr\s+uint32_t\s+ANS_BYTES\s*=\s*(\d+)\s*;', 'answers_tx.hip.h')
        # what the render kernel makes of them: a piece per lane in ONE trip, a reader's answer of n bits has n + 2 pieces
        assert re.search(r'MAX_PIECES\s*=\s*MAX_BITS\s*\+\s*2\b', text), 'answers_tx.hip.h: MAX_PIECES is no longer MAX_BITS + 2'
        return c
    return cached('answers_tx_constants', read)


def test_the_thresholds_are_read_from_the_sources():
    c = constants()
    got = {n: getattr(c, n) for n in ('BLOCK', 'PER_THREAD', 'TILE', 'SCHED_BLOCK', 'MAX_BITS', 'ANS_BYTES')}
    assert all(isinstance(v, int) and v > 0 for v in got.values()), got
    assert c.BLOCK % 64 == 0 and c.MAX_BITS == 9 * c.ANS_BYTES == max(N_BITS) and c.MAX_BITS + 2 <= c.BLOCK
    assert _lib.TX_PENDING_DTYPE['air'].shape == (c.ANS_BYTES,)


# ---- what both halves share -------------------------------------------------------------------------------------------------------------
def ratio(rate):
    r = Fraction(rate) / Fraction(IN_RATE)
    return r.numerator, r.denominator


def entry(start, role, bits):
    """a pending entry (nfc_tx_pending) of the answer `bits`, its air / par bytes as `pack` makes them"""
    e = np.zeros(1, _lib.TX_PENDING_DTYPE)
    _, air, par = pack([list(bits)])
    e['start'], e['n_bits'], e['role'] = int(start), len(bits), int(role)
    e['air'][0, :len(air)], e['par'][0, :len(par)] = air, par
    return e[0]


def random_bits(seed, n):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 2, n).tolist()


def model_wave(role, bits, rate):
    """`_model` of ONE answer at index 0 of a stream that ends with it (TX indices: ratio 1/1, no delay), made once per answer"""
    def make():
        n = len(wave(role, bits, rate))
        out = _model(role, [(0, bits)], n, rate)
        assert len(out) == n
        return out
    return cached(('wave', role, tuple(bits), rate), make)


def timeline(stream_role, items, t1, rate):
    """TX indices [0, t1) of a stream that only ever had pending entries, items (start, entry role, bits) that do not meet: the idle level
    of the STREAM's role, and `_model`'s samples of every entry from its start to the timeline's end"""
    out = np.full(t1, IDLE[stream_role], np.float32)
    for start, er, bits in items:
        w = model_wave(er, bits, rate)
        a, b = start, min(start + len(w), t1)
        if a < b:
            out[a:b] = w[:b - a]
    return out


def twin_idle(roles, base, n, pend, **kw):
    """the twin over a push in which no stream answered anything -> (samples, first, ns, pending)"""
    K = len(roles)
    return emulate.host_transmit([None] * K, [()] * K, roles, base, n, pend, **kw)


def spans_per_tile(first, spans, tile):
    """spans: per stream the [a, b) (stream-relative) its answers own -> the largest number of spans of ONE stream that one tile meets"""
    best = 0
    for f, sp in zip(first, spans):
        count = {}
        for a, b in sp:
            for t in range((int(f) + a) // tile, (int(f) + b - 1) // tile + 1):
                count[t] = count.get(t, 0) + 1
        best = max([best] + list(count.values()))
    return best


def streams_per_tile(first, ns, tile):
    count = {}
    for f, n in zip(first, ns):
        if n:
            for t in range(int(f) // tile, (int(f) + int(n) - 1) // tile + 1):
                count[t] = count.get(t, 0) + 1
    return max(count.values())


def _idle_iq(n):
    from usrp_nfc_amd import synth
    long = cached('idle_iq', lambda: synth.iq_from_profile(np.ones(40000, np.float32)))
    assert n <= len(long) // 2
    return long[:2 * n]


def _cards_of(roles):
    cards = _replay_cards()
    return [cards[0] if r == TAG else cards[2] for r in roles]


def _cap(n, kw):
    num, den = ratio(kw.get('samp_rate', IN_RATE))
    return sum(int(x) * num // den + 1 + kw.get('align_samples', 8) for x in n) + 64


def device_push(m, pieces, roles, pend, kw, idle=True):
    """one push and transmit on the device against the twin fed what the push brought: everything the GPU half asserts of one push
    -> (the layout's samples, first, ns, the pending entries afterwards)"""
    K = len(roles)
    got, first, ns, want, pend, an = _push_transmit(m, pieces, roles, pend, _cap([len(p) // 2 for p in pieces], kw), **kw)
    assert not idle or int(an.n.sum()) == 0   # (an unmodulated carrier is answered by nobody)
    if kw.get('carrier'):
        assert np.abs(got - want).max() <= 1.5e-7 * kw['amp']
    else:
        assert got.tobytes() == want.tobytes()
    assert _pend_bytes(m, K) == pend.tobytes()
    assert m.L.nfc_debug_multi_guards(m.h) == 0
    return got, first, ns, pend


def set_entries(m, pend):
    for k in range(len(pend)):
        m.set_tx_state(k, pend[k])
    assert _pend_bytes(m, len(pend)) == pend.tobytes()


def parts_of(got, first, ns):
    return [got[int(f):int(f) + int(n)] for f, n in zip(first, ns)]


# ---- 1. every shape, both roles, four rates (and one more with two of the nine counts at 0) ---------------------------------------------
SHAPE_RATES = [2e6, 4e6, 13.56e6, 0.5e6, 0.25e6]
LOW_RATES = (0.25e6,)


def shapes_case(rate):
    """K = 2 len(N_BITS) streams that receive an idle carrier, one per (shape, entry role), the stream's own role alternating against it"""
    def make():
        c, x = constants(), Constants()
        num, den = ratio(rate)
        x.kw = dict(samp_rate=rate, in_rate=IN_RATE, align_samples=1)
        x.K = 2 * len(N_BITS)
        x.entry_role = [k % 2 for k in range(x.K)]
        x.roles = [(k // 2 + k) % 2 for k in range(x.K)]
        x.bits = [random_bits(1000 + k, N_BITS[k // 2]) for k in range(x.K)]
        x.len = [len(model_wave(x.entry_role[k], x.bits[k], rate)) for k in range(x.K)]
        n_tx = [c.TILE + c.PER_THREAD + max(x.len) + 8 + 13 * (k % 5) for k in range(x.K)]
        x.n = [(t * den + num - 1) // num for t in n_tx]   # the fewest received samples that give the stream n_tx TX samples
        _, x.first, x.ns, _ = twin_idle(x.roles, [0] * x.K, x.n, None, **x.kw)
        assert all(int(a) >= b for a, b in zip(x.ns, n_tx))
        # the starts: at offset 0 of the stream, inside a tile, in the PER_THREAD samples before a tile's edge, in those behind it
        x.pos_class = [k % 4 for k in range(x.K)]
        x.start = []
        for k in range(x.K):
            want = [None, 300 + k, c.TILE - 1 - (k // 4) % c.PER_THREAD, (k // 4) % c.PER_THREAD][x.pos_class[k]]
            x.start.append(0 if want is None else (want - int(x.first[k])) % c.TILE)
        x.pend = np.array([entry(x.start[k], x.entry_role[k], x.bits[k]) for k in range(x.K)], _lib.TX_PENDING_DTYPE)
        return x
    return cached(('shapes', rate), make)


def zero_and_nonzero_counts(rate):
    """by the encoder and nfc_tx_sample_count: the durations of the runs of every answer shape -> (those with no sample, those with some)"""
    count = {}
    for enc in (tx.NFC_TX_MANCHESTER, tx.NFC_TX_MILLER):
        for n in N_BITS:
            runs = tx.encode_runs(enc, random_bits(n, n))
            for i in range(len(runs)):
                if float(runs[i]['dur_us']) not in count:
                    count[float(runs[i]['dur_us'])] = tx.sample_count(runs[i:i + 1], rate)
    assert len(count) <= 9   # (the nine durations of the pieces' runs)
    return sorted(d for d, n in count.items() if n == 0), sorted(d for d, n in count.items() if n > 0)


@pytest.mark.parametrize('rate', SHAPE_RATES)
def test_every_shape_in_both_roles_crosses_its_lines_and_the_twin_is_the_model(rate):
    c, x = constants(), shapes_case(rate)
    assert sorted(set(len(b) for b in x.bits)) == N_BITS and max(N_BITS) == c.MAX_BITS
    # a piece per lane: the shapes' piece counts (n + 1 for a tag's answer, n + 2 for a reader's) lie on both sides of the 64-lane edges
    pieces = sorted({len(b) + 1 + r for b, r in zip(x.bits, x.entry_role)})
    assert pieces[0] < 64 and any(64 < p <= 128 for p in pieces) and any(128 < p <= c.BLOCK for p in pieces) and pieces[-1] == c.MAX_BITS + 2
    # tag-encoded entries over a reader's idle level, Miller entries over a tag's, and both over their own
    assert {(x.entry_role[k], x.roles[k]) for k in range(x.K)} == {(TAG, TAG), (TAG, READER), (READER, TAG), (READER, READER)}
    none, some = zero_and_nonzero_counts(rate)
    if rate in LOW_RATES:
        assert none and some, (none, some)   # runs of no samples among runs of some
        runs = tx.encode_runs(tx.NFC_TX_MILLER, x.bits[x.K - 1])
        assert any(tx.sample_count(runs[i:i + 1], rate) == 0 for i in range(len(runs)))   # ... in the longest reader's answer
    else:
        assert not none
    if rate == max(SHAPE_RATES):   # the longest answer just fits the push: about 3 200 received samples
        assert max(x.len) > 0.9 * min(int(n) for n in x.ns) and 3000 < min(x.n) <= max(x.n) < 3400
    # where the answers begin
    tile_pos = [(int(x.first[k]) + x.start[k]) % c.TILE for k in range(x.K)]
    assert sum(s == 0 for s in x.start) >= x.K // 4
    assert any(c.PER_THREAD <= p < c.TILE - c.PER_THREAD for p in tile_pos)
    assert {p for p in tile_pos if p >= c.TILE - c.PER_THREAD} == set(range(c.TILE - c.PER_THREAD, c.TILE))
    assert {p for k, p in enumerate(tile_pos) if x.pos_class[k] == 3} == set(range(c.PER_THREAD))
    assert all(x.start[k] + x.len[k] <= int(x.ns[k]) for k in range(x.K))   # every answer ends inside its push
    out, first, ns, pend = twin_idle(x.roles, [0] * x.K, x.n, x.pend, **x.kw)
    assert not pend.tobytes().strip(b'\0') and not out.imag.any()
    for k, part in enumerate(parts_of(out, first, ns)):
        assert part.real.tobytes() == timeline(x.roles[k], [(x.start[k], x.entry_role[k], x.bits[k])], int(ns[k]), rate).tobytes(), k


@gpu
@pytest.mark.parametrize('rate', SHAPE_RATES)
def test_gpu_every_shape_in_both_roles(rate):
    x = shapes_case(rate)
    with _context(_cards_of(x.roles), max(x.n)) as m:
        set_entries(m, x.pend)
        got, first, ns, pend = device_push(m, [_idle_iq(n) for n in x.n], x.roles, x.pend, x.kw)
        assert not pend.tobytes().strip(b'\0')
        for k, part in enumerate(parts_of(got, first, ns)):
            assert part.real.tobytes() == timeline(x.roles[k], [(x.start[k], x.entry_role[k], x.bits[k])], int(ns[k]), rate).tobytes(), k


# ---- 2. streams shorter than a tile, answers longer than a push -----------------------------------------------------------------------
SHORT_K = (1, 63, 64, 65, 130)


def short_case(K, align):
    """K streams that begin with a pending entry of the longest shape and receive a few hundred samples of idle carrier a push, until
    nobody has anything pending"""
    def make():
        x = Constants()
        x.K, x.kw = K, dict(samp_rate=IN_RATE, in_rate=IN_RATE, align_samples=align)
        x.roles = [k % 2 for k in range(K)]
        x.entry_role = [(k // 2) % 2 for k in range(K)]
        x.bits = [random_bits(2000 + k % 8, max(N_BITS)) for k in range(K)]   # (eight answers among the streams: the model's waves are made once)
        x.start = [(7 * k) % 50 for k in range(K)]
        x.end = [x.start[k] + len(model_wave(x.entry_role[k], x.bits[k], IN_RATE)) for k in range(K)]
        x.pend = np.array([entry(x.start[k], x.entry_role[k], x.bits[k]) for k in range(K)], _lib.TX_PENDING_DTYPE)
        x.pushes, done = [], [0] * K
        while any(d < e for d, e in zip(done, x.end)):
            p = len(x.pushes)
            n = [301 + 2 * ((37 * k + 11 * p) % 100) for k in range(K)]   # ragged and odd
            if align == 1 and sum(n) % 4 == 0:
                n[-1] += 2
            x.pushes.append(n)
            done = [d + a for d, a in zip(done, n)]
        x.total = done
        return x
    return cached(('short', K, align), make)


def short_twin(x):
    """the twin push by push -> per push (samples, first, ns, pending afterwards)"""
    def run():
        out, pend, base = [], x.pend, [0] * x.K
        for n in x.pushes:
            out.append(twin_idle(x.roles, base, n, pend, **x.kw))
            pend, base = out[-1][3], [b + a for b, a in zip(base, n)]
        return out
    return cached(('short_twin', x.K, x.kw['align_samples']), run)


def short_whole(x, k):
    return timeline(x.roles[k], [(x.start[k], x.entry_role[k], x.bits[k])], x.total[k], IN_RATE)


@pytest.mark.parametrize('align', [1, 8])
@pytest.mark.parametrize('K', SHORT_K)
def test_answers_longer_than_the_pushes_of_short_streams_cross_their_lines_and_the_twin_is_the_model(K, align):
    c, x = constants(), short_case(K, align)
    assert SHORT_K == (1, c.SCHED_BLOCK - 1, c.SCHED_BLOCK, c.SCHED_BLOCK + 1, 2 * c.SCHED_BLOCK + 2)   # around the schedule's workgroup
    longest_push = max(max(n) for n in x.pushes)
    assert 300 < min(min(n) for n in x.pushes) and longest_push < c.TILE // 2 and all(a % 2 for n in x.pushes for a in n)
    assert all(e - s > 5 * longest_push for s, e in zip(x.start, x.end))   # the answer outlasts five pushes at the least
    runs, carried = short_twin(x), [0] * K
    before = x.pend
    for p, (out, first, ns, pend) in enumerate(runs):
        if K >= 3:
            assert streams_per_tile(first, ns, c.TILE) >= 3
        if align == 1:
            assert len(out) % 4 != 0 and len(out) == sum(x.pushes[p])   # the last thread of the layout stores sample by sample
        else:
            assert all(int(f) % align == 0 for f in first) and (K == 1 or len(out) > sum(x.pushes[p]))
        for k in range(K):   # an entry carried THROUGH a push that brought no answer is the same 64 bytes behind it
            if int(pend[k]['n_bits']):
                assert pend[k].tobytes() == before[k].tobytes() == x.pend[k].tobytes()
                carried[k] += 1
        before = pend
        assert (p == len(runs) - 1) == (not pend.tobytes().strip(b'\0'))   # pushed until nobody has anything pending, and no longer
    assert min(carried) >= 5
    for k in range(K):
        whole = np.concatenate([parts_of(*r[:3])[k] for r in runs])
        assert not whole.imag.any() and whole.real.tobytes() == short_whole(x, k).tobytes(), k


@gpu
@pytest.mark.parametrize('align', [1, 8])
@pytest.mark.parametrize('K', SHORT_K)
def test_gpu_answers_longer_than_the_pushes_of_short_streams(K, align):
    x = short_case(K, align)
    runs = short_twin(x)
    with _context(_cards_of(x.roles), max(max(n) for n in x.pushes)) as m:
        set_entries(m, x.pend)
        pend, parts = x.pend, [[] for _ in range(K)]
        for p, n in enumerate(x.pushes):
            got, first, ns, pend = device_push(m, [_idle_iq(a) for a in n], x.roles, pend, x.kw)
            assert pend.tobytes() == runs[p][3].tobytes() and got.tobytes() == runs[p][0].tobytes()
            for k, part in enumerate(parts_of(got, first, ns)):
                parts[k].append(part)
        assert not pend.tobytes().strip(b'\0')
        for k in range(K):
            assert np.concatenate(parts[k]).real.tobytes() == short_whole(x, k).tobytes(), k


# ---- 3. many spans per tile, and cuts: the two captures at a TX rate below the RX rate -------------------------------------------------
def captures():
    """the two reader-side captures with their cards, from the reference side alone: per stream the entries (idx, bits) of what the card
    answers -- the C oracle's frames with the closing indices of the reference's framing, through the emulator's host twin"""
    def make():
        x = Constants()
        x.streams, x.cards = _reader_side_streams(), _replay_cards()
        x.roles = [c.role for c in x.cards]
        x.n = [len(s) // 2 for s in x.streams]
        x.entries, x.frame_idx, x.names = [], [], []
        for k in range(3):
            if x.n[k] == 0:
                x.entries.append([]), x.frame_idx.append([]), x.names.append([])
                continue
            frames = expected_pushes([x.streams[k]])[0].frames
            (table, _, _), ans = emulate.host_emulate(x.cards[k], emulate.state_init(), fsm.state_init(), frames)
            idx = frames.table['idx'].astype(np.int64)
            x.entries.append([(int(idx[int(r['src'])]), ans.bits(j)) for j, r in enumerate(ans.records)])
            x.frame_idx.append(idx), x.names.append(table['cmd'].tolist())
        x.tail = [4000, 4000, 0]   # an unmodulated tail behind the captures: the tags' last answers, 18 bytes, outlast them
        return x
    return cached('captures', make)


CAPTURE_CASES = [(0.5e6, 86.43, 1), (0.8e6, 86.43, 8), (0.5e6, 400.0, 8), (0.8e6, 400.0, 1)]


def capture_kw(rate, delay_us, align):
    return dict(samp_rate=rate, in_rate=IN_RATE, delay_us=delay_us, align_samples=align)


def capture_spans(x, k, rate, kw, total):
    """by the model: per answer of stream k (S, L, the cut) in TX indices"""
    num, den = ratio(rate)
    delay = tx.answers_tx_config(**kw).delay_samples
    T = lambda r: r * num // den
    e = x.entries[k]
    return [(T(i) + delay, len(wave(x.roles[k], b, rate)), T(e[j + 1][0]) if j + 1 < len(e) else T(total)) for j, (i, b) in enumerate(e)]


def capture_whole(x, k, rate, kw):
    """the model of stream k's whole timeline, the tail included"""
    num, den = ratio(rate)
    return _model(x.roles[k], x.entries[k], x.n[k] + x.tail[k], rate, num, den, tx.answers_tx_config(**kw).delay_samples)


@pytest.mark.parametrize('rate,delay_us,align', CAPTURE_CASES)
def test_the_captures_at_a_lower_tx_rate_cross_their_lines_and_the_twin_is_the_model(rate, delay_us, align):
    c, x, kw = constants(), captures(), capture_kw(rate, delay_us, align)
    num, den = ratio(rate)
    assert (num, den) in ((1, 4), (2, 5)) and [len(e) for e in x.entries] == [12, 9, 0]
    # the layout of the whole push, and the spans the answers own by the model: some tile meets three spans of one stream at the least
    answers = [pack([b for _, b in e]) for e in x.entries]
    out, first, ns, pend = emulate.host_transmit(answers, [[i for i, _ in e] for e in x.entries], x.roles, [0] * 3, x.n, **kw)
    spans = [[(s, min(s + ln, cut)) for s, ln, cut in capture_spans(x, k, rate, kw, x.n[k]) if s < min(s + ln, cut)] for k in range(3)]
    assert spans_per_tile(first, spans, c.TILE) >= 3
    all_spans = [v for k in range(3) for v in capture_spans(x, k, rate, kw, x.n[k] + x.tail[k])]
    if delay_us > 100:   # an answer cut short by the next answered command, and one cut away entirely
        assert any(s < cut < s + ln for s, ln, cut in all_spans) and any(s >= cut for s, ln, cut in all_spans)
    for k in (0, 1):
        total = x.n[k] + x.tail[k]
        whole, pend = one_stream(x.roles[k], x.entries[k], 0, total, **kw)
        assert whole.real.tobytes() == capture_whole(x, k, rate, kw).tobytes() and not whole.imag.any() and int(pend[0]['n_bits']) == 0
        assert out[int(first[k]):int(first[k]) + int(ns[k])].tobytes() == whole[:int(ns[k])].tobytes()
        # in pieces: tests/test_answers_tx.py's cuts (an empty push among them), then the tail
        cuts = _piece_cuts(x.frame_idx[0], x.frame_idx[1], x.names[0])[k] + [x.n[k]]
        got, pend, sizes = in_pieces(x.roles[k], x.entries[k], cuts, total, **kw)
        assert got.tobytes() == whole.tobytes() and not pend.tobytes().strip(b'\0')
        assert k == 1 or 0 in sizes[:-1]   # (stream 0's empty push)


def _run_captures(m, x, kw, pieces_of_push, n_push, idle_last=True):
    """the pushes on the device, the tail last -> per stream the concatenation, and per push the streams' bases"""
    parts, pend, bases, at = [[] for _ in range(3)], None, [], [0, 0, 0]
    for p in range(n_push + 1):
        pieces = pieces_of_push(p) if p < n_push else [_idle_iq(t) for t in x.tail]
        got, first, ns, pend = device_push(m, pieces, x.roles, pend, kw, idle=p == n_push)
        bases.append(list(at))
        at = [a + len(q) // 2 for a, q in zip(at, pieces)]
        for k, part in enumerate(parts_of(got, first, ns)):
            parts[k].append(part)
    assert not pend.tobytes().strip(b'\0')
    return [np.concatenate(q) for q in parts], bases


def _cut_pieces(x, cuts):
    edges = [[0] + list(cu) + [n] for cu, n in zip(cuts, x.n)]
    n_push = max(len(e) for e in edges) - 1
    return (lambda p: [s[2 * e[p]:2 * e[p + 1]] if p + 1 < len(e) else s[:0] for s, e in zip(x.streams, edges)]), n_push


def _assert_fetched_idx(m, x):
    """the answered commands' idx the device fetched are the reference side's: both halves have the same inputs"""
    cm, an = m.fetch_commands(), m.fetch_answers()
    _, idx = emulate.tx_inputs(cm, an)
    assert [[int(i) for i in v] for v in idx] == [[i for i, _ in e] for e in x.entries]
    assert cm.commands_of(0)[0]['cmd'].tolist() == x.names[0]


@gpu
@pytest.mark.parametrize('rate,delay_us,align', CAPTURE_CASES)
def test_gpu_the_captures_at_a_lower_tx_rate_whole_and_in_pieces(rate, delay_us, align):
    x, kw = captures(), capture_kw(rate, delay_us, align)
    with _context(x.cards, max(x.n + x.tail)) as m:
        whole, _ = _run_captures(m, x, kw, lambda p: x.streams, 1)
        m.reset()
        m.push(x.streams)
        _assert_fetched_idx(m, x)
        m.reset()
        pieces_of_push, n_push = _cut_pieces(x, _piece_cuts(x.frame_idx[0], x.frame_idx[1], x.names[0]))
        assert n_push == 6
        in_parts, _ = _run_captures(m, x, kw, pieces_of_push, n_push)
    for k in (0, 1):
        assert whole[k].real.tobytes() == capture_whole(x, k, rate, kw).tobytes() and not whole[k].imag.any(), k
        assert in_parts[k].tobytes() == whole[k].tobytes(), k
    assert len(whole[2]) == 0


# ---- 4. tile edges ------------------------------------------------------------------------------------------------------------------
EDGE_ORDERS = [(1, 0, 2, 3), (0, 2, 1, 3), (3, 2, 0, 1), (2, 3, 1, 0)]
LAST_ON_EDGE, FIRST_ON_EDGE, SPAN_IN_TAIL = 'an answer ends on a tile\'s last sample', 'an answer begins on a tile\'s first', 'a span in a tile\'s last samples'
LAST_ON_FIRST = 'an answer ends on a tile\'s first sample'


def edge_case(order):
    """four idle streams of TILE - 1, TILE, TILE + 1 and 2 TILE + 3 samples in the order given, packed without padding, every one with a
    pending entry placed against a tile's edge; a second push of idle carrier finishes what the first left"""
    def make():
        c, x = constants(), Constants()
        lengths = (c.TILE - 1, c.TILE, c.TILE + 1, 2 * c.TILE + 3)
        x.kw = dict(samp_rate=IN_RATE, in_rate=IN_RATE, align_samples=1)
        x.K, x.n = 4, [lengths[i] for i in order]
        x.roles = [k % 2 for k in range(4)]
        x.entry_role = [(k + order[0]) % 2 for k in range(4)]
        x.bits = [random_bits(4000 + 10 * order[0] + k, (18, 45, 9, 27)[k]) for k in range(4)]
        first = np.cumsum([0] + x.n)
        x.start, x.what = [], []
        for k in range(4):
            f, n, ln = int(first[k]), x.n[k], len(wave(x.entry_role[k], x.bits[k], IN_RATE))
            edge = (f + c.TILE - 1) // c.TILE * c.TILE   # the first tile that begins inside the stream, if any does
            want = [SPAN_IN_TAIL, LAST_ON_EDGE, FIRST_ON_EDGE, LAST_ON_FIRST][(k + order[1]) % 4]
            over = 1 if want == LAST_ON_FIRST else 0   # the samples of the answer behind the edge
            if want == SPAN_IN_TAIL and (f + n) % c.TILE == 0:   # the stream ends where a tile ends: the span is the stream's last three samples
                x.start.append(n - (c.PER_THREAD - 1)), x.what.append(SPAN_IN_TAIL)
            elif want != FIRST_ON_EDGE and edge + c.TILE + over - ln >= f and edge + c.TILE + over <= f + n:
                x.start.append(edge + c.TILE + over - ln - f), x.what.append(LAST_ON_FIRST if over else LAST_ON_EDGE)
            elif want != FIRST_ON_EDGE and edge + over - ln >= f and edge + over <= f + n:
                x.start.append(edge + over - ln - f), x.what.append(LAST_ON_FIRST if over else LAST_ON_EDGE)
            else:
                assert f <= edge < f + n
                x.start.append(edge - f), x.what.append(FIRST_ON_EDGE)
        x.pend = np.array([entry(x.start[k], x.entry_role[k], x.bits[k]) for k in range(4)], _lib.TX_PENDING_DTYPE)
        x.pushes = [x.n, [1501, 1200, 1333, 1024]]
        return x
    return cached(('edges', order), make)


def edge_whole(x, k):
    return timeline(x.roles[k], [(x.start[k], x.entry_role[k], x.bits[k])], x.pushes[0][k] + x.pushes[1][k], IN_RATE)


def test_streams_and_answers_on_the_edges_of_a_tile_cross_their_lines_and_the_twin_is_the_model():
    c, seen, lengths_at = constants(), [], {}
    for order in EDGE_ORDERS:
        x = edge_case(order)
        assert sorted(x.n) == [c.TILE - 1, c.TILE, c.TILE + 1, 2 * c.TILE + 3]
        pend, base = x.pend, [0] * 4
        parts = [[] for _ in range(4)]
        for p, n in enumerate(x.pushes):
            out, first, ns, pend = twin_idle(x.roles, base, n, pend, **x.kw)
            if p == 0:
                assert first.tolist() == np.cumsum([0] + x.n)[:4].tolist() and ns.tolist() == x.n
                for k in range(4):
                    f, s, ln = int(first[k]), x.start[k], len(wave(x.entry_role[k], x.bits[k], IN_RATE))
                    lengths_at.setdefault(x.n[k], set()).add(f % c.TILE)
                    if x.what[k] in (LAST_ON_EDGE, LAST_ON_FIRST):
                        assert (f + s + ln) % c.TILE == (x.what[k] == LAST_ON_FIRST) and s >= 0 and s + ln <= x.n[k] and int(pend[k]['n_bits']) == 0
                    elif x.what[k] == FIRST_ON_EDGE:
                        assert (f + s) % c.TILE == 0 and 0 <= s < x.n[k]
                    else:   # the span is cut by the stream's end, which is a tile's: the rest of the answer waits for the next push
                        assert (f + x.n[k]) % c.TILE == 0 and 0 < x.n[k] - s < c.PER_THREAD and int(pend[k]['n_bits']) == len(x.bits[k])
                    seen.append(x.what[k])
            base = [b + a for b, a in zip(base, n)]
            for k, part in enumerate(parts_of(out, first, ns)):
                parts[k].append(part)
        assert not pend.tobytes().strip(b'\0')
        for k in range(4):
            assert np.concatenate(parts[k]).real.tobytes() == edge_whole(x, k).tobytes(), (order, k)
        assert FIRST_ON_EDGE in x.what and {LAST_ON_EDGE, LAST_ON_FIRST} & set(x.what)
    assert seen.count(SPAN_IN_TAIL) >= 2 and seen.count(LAST_ON_EDGE) >= 4 and seen.count(FIRST_ON_EDGE) >= 4 and seen.count(LAST_ON_FIRST) >= 2, seen
    assert all(len(v) >= 2 for v in lengths_at.values())   # every length begins at more than one offset of a tile


@gpu
@pytest.mark.parametrize('order', EDGE_ORDERS)
def test_gpu_streams_and_answers_on_the_edges_of_a_tile(order):
    x = edge_case(order)
    with _context(_cards_of(x.roles), max(max(n) for n in x.pushes)) as m:
        set_entries(m, x.pend)
        pend, parts = x.pend, [[] for _ in range(4)]
        for n in x.pushes:
            got, first, ns, pend = device_push(m, [_idle_iq(a) for a in n], x.roles, pend, x.kw)
            for k, part in enumerate(parts_of(got, first, ns)):
                parts[k].append(part)
        assert not pend.tobytes().strip(b'\0')
        for k in range(4):
            assert np.concatenate(parts[k]).real.tobytes() == edge_whole(x, k).tobytes(), k


# ---- 5. pending entries that wait, and that are cut -------------------------------------------------------------------------------------
WAIT_RATES = [2e6, 5e6, 0.8e6]


def waiting_case(rate):
    """four idle streams, two pushes.  Before the first: stream 0 gets an entry that starts behind the push's span, stream 1 one that
    starts exactly at its end.  Before the second: stream 2 gets an entry that ended before the push began, stream 3 one that began
    before it and ends in it."""
    def make():
        x = Constants()
        num, den = ratio(rate)
        T = lambda r: r * num // den
        x.kw = dict(samp_rate=rate, in_rate=IN_RATE, align_samples=8)
        x.roles, x.entry_role = [TAG, READER, TAG, READER], [READER, READER, TAG, TAG]
        x.pushes = [[2000, 1777, 2000, 1501], [6000, 5000, 3001, 4000]]
        x.bits = [random_bits(5000 + k, n) for k, n in enumerate((45, 162, 9, 36))]
        x.len = [len(wave(x.entry_role[k], x.bits[k], rate)) for k in range(4)]
        x.start = [T(2000) + 700, T(1777), 100, T(1501) - x.len[3] // 3]
        x.set_before = [(0, 1), (2, 3)]
        x.t0 = [[0] * 4, [T(n) for n in x.pushes[0]]]
        x.t1 = [T(a + b) for a, b in zip(*x.pushes)]
        return x
    return cached(('waiting', rate), make)


def waiting_model(x, k, rate):
    whole = timeline(x.roles[k], [(x.start[k], x.entry_role[k], x.bits[k])] if k != 2 else [], x.t1[k], rate)
    if k == 3:   # (set behind the first push: what the entry would have owned of that push went out as the idle level)
        whole[:x.t0[1][k]] = IDLE[x.roles[k]]
    return whole


def _waiting_run(x, push):
    """`push(p, n, pend)` -> (samples, first, ns, pending): the two pushes with the entries set in front of each"""
    pend, parts, after = np.zeros(4, _lib.TX_PENDING_DTYPE), [[] for _ in range(4)], []
    for p, n in enumerate(x.pushes):
        for k in x.set_before[p]:
            pend[k] = entry(x.start[k], x.entry_role[k], x.bits[k])
        set_bytes = pend.tobytes()
        out, first, ns, pend = push(p, n, pend)
        after.append((set_bytes, pend.copy()))
        for k, part in enumerate(parts_of(out, first, ns)):
            parts[k].append(part)
    return parts, after


def _assert_waiting(x, rate, parts, after):
    (set0, pend0), (set1, pend1) = after
    # the entries in the future own nothing of the first push and survive it untouched: every sample is the idle level
    assert pend0.tobytes() == set0 and [int(v) for v in pend0['n_bits']] == [45, 162, 0, 0]
    for k in range(4):
        assert parts[k][0].tobytes() == np.full(x.t0[1][k], IDLE[x.roles[k]], np.complex64).tobytes(), k
    # the second push renders them; the entry in the past is dropped and its bytes cleared
    assert set1 != bytes(len(set1)) and not pend1.tobytes().strip(b'\0')
    for k in range(4):
        whole = np.concatenate(parts[k])
        assert whole.real.tobytes() == waiting_model(x, k, rate).tobytes() and not whole.imag.any(), k
    assert parts[2][1].tobytes() == np.full(len(parts[2][1]), IDLE[TAG], np.complex64).tobytes()


@pytest.mark.parametrize('rate', WAIT_RATES)
def test_entries_in_the_future_and_in_the_past_cross_their_lines_and_the_twin_is_the_model(rate):
    x = waiting_case(rate)
    assert x.start[0] > x.t0[1][0] and x.start[1] == x.t0[1][1]                      # beyond the first push's span, and exactly at its end
    assert x.start[0] + x.len[0] < x.t1[0] and x.start[1] + x.len[1] < x.t1[1]       # the second push holds them whole
    assert x.start[2] + x.len[2] < x.t0[1][2]                                        # ended before the second push began
    assert x.start[3] < x.t0[1][3] < x.start[3] + x.len[3] < x.t1[3]                 # began before it, ends in it
    base = [[0] * 4, x.pushes[0]]
    parts, after = _waiting_run(x, lambda p, n, pend: twin_idle(x.roles, base[p], n, pend, **x.kw))
    _assert_waiting(x, rate, parts, after)


@gpu
@pytest.mark.parametrize('rate', WAIT_RATES)
def test_gpu_entries_in_the_future_and_in_the_past(rate):
    x = waiting_case(rate)
    with _context(_cards_of(x.roles), max(max(n) for n in x.pushes)) as m:
        def push(p, n, pend):
            set_entries(m, pend)
            return device_push(m, [_idle_iq(a) for a in n], x.roles, pend, x.kw)
        parts, after = _waiting_run(x, push)
    _assert_waiting(x, rate, parts, after)


CUT_RATES = [2e6, 0.8e6]


def cut_case(rate):
    """the two captures behind a pending entry each: stream 0's begins in front of the first answered command and is cut where that command
    closed; stream 1's begins where the first command closed, delay_samples behind it, and is cut away entirely"""
    def make():
        x = captures()
        y = Constants()
        num, den = ratio(rate)
        y.kw = capture_kw(rate, 86.43, 8)
        y.delay = tx.answers_tx_config(**y.kw).delay_samples
        first_idx = [e[0][0] for e in x.entries[:2]]
        y.at = [first_idx[0] - 1200, first_idx[1]]   # the r whose T(r) + delay is the entry's start: `_model` takes the entry as one more answer
        y.bits = [random_bits(5100, 162), random_bits(5101, 45)]
        y.start = [i * num // den + y.delay for i in y.at]
        y.pend = np.zeros(3, _lib.TX_PENDING_DTYPE)
        for k in (0, 1):
            y.pend[k] = entry(y.start[k], x.roles[k], y.bits[k])
        y.top = [i * num // den for i in first_idx]
        return y
    return cached(('cut', rate), make)


def cut_whole(x, y, k, rate):
    num, den = ratio(rate)
    return _model(x.roles[k], [(y.at[k], y.bits[k])] + x.entries[k], x.n[k] + x.tail[k], rate, num, den, y.delay)


@pytest.mark.parametrize('rate', CUT_RATES)
def test_an_entry_cut_by_the_first_answered_command_crosses_its_lines_and_the_twin_is_the_model(rate):
    x, y = captures(), cut_case(rate)
    ln = [len(wave(x.roles[k], y.bits[k], rate)) for k in (0, 1)]
    assert 0 < y.start[0] < y.top[0] < y.start[0] + ln[0]   # cut short: the command closes inside the entry
    assert y.start[1] >= y.top[1]                           # cut away: the entry would begin where the command closed, or behind
    for k in (0, 1):
        total = x.n[k] + x.tail[k]
        out, first, ns, pend = emulate.host_transmit([pack([b for _, b in x.entries[k]])], [[i for i, _ in x.entries[k]]], [x.roles[k]], [0], [total],
                                                     y.pend[k:k + 1], **y.kw)
        assert out.real.tobytes() == cut_whole(x, y, k, rate).tobytes() and int(pend[0]['n_bits']) == 0
        plain = _model(x.roles[k], x.entries[k], total, rate, *ratio(rate), y.delay)
        assert (out.real.tobytes() != plain.tobytes()) == (k == 0)   # what is cut away leaves no sample


@gpu
@pytest.mark.parametrize('rate', CUT_RATES)
def test_gpu_an_entry_cut_by_the_first_answered_command(rate):
    x, y = captures(), cut_case(rate)
    with _context(x.cards, max(x.n + x.tail)) as m:
        set_entries(m, y.pend)
        got, first, ns, pend = device_push(m, x.streams, x.roles, y.pend, y.kw, idle=False)
        _assert_fetched_idx(m, x)
        parts = parts_of(got, first, ns)
        got, first, ns, pend = device_push(m, [_idle_iq(t) for t in x.tail], x.roles, pend, y.kw)
        assert not pend.tobytes().strip(b'\0')
        for k in (0, 1):
            whole = np.concatenate([parts[k], parts_of(got, first, ns)[k]])
            assert whole.real.tobytes() == cut_whole(x, y, k, rate).tobytes(), k


# ---- 6. the carrier across pushes -----------------------------------------------------------------------------------------------------
CARRIER_RATE, FIRST_INDEX, AMP, FREQ = 13.56e6, (1 << 40) + 12345, 0.5, 13.56e6


def carrier_kw(carrier):
    return dict(samp_rate=CARRIER_RATE, in_rate=IN_RATE, delay_us=86.43, carrier=carrier, amp=AMP, freq=FREQ, first_index=FIRST_INDEX, align_samples=8)


def carrier_reference(levels):
    """the levels of a stream's TX timeline from index 0 -> the samples in float64, the angle from the 24 bits the kernel keeps of it"""
    inc = np.uint64(int((FREQ / CARRIER_RATE - np.floor(FREQ / CARRIER_RATE)) * 2.0 ** 64))
    with np.errstate(over='ignore'):
        ph = ((np.uint64(FIRST_INDEX) + np.arange(len(levels), dtype=np.uint64)) * inc) >> np.uint64(40)
    return levels.astype(np.float64) * AMP * np.exp(2j * np.pi * ph.astype(np.float64) / 2.0 ** 24)


def carrier_bases(x):
    cuts = _piece_cuts(x.frame_idx[0], x.frame_idx[1], x.names[0])
    return [[0] + cu + [n] for cu, n in zip(cuts, x.n)]


def test_the_carrier_across_pushes_crosses_its_lines_and_the_twin_is_within_the_bound_of_the_model():
    x = captures()
    num, den = ratio(CARRIER_RATE)
    assert (num, den) == (339, 50)
    edges = carrier_bases(x)
    for k in (0, 1):   # from the second push on t0 is not 0, and T(base) is a floor that drops a fraction
        assert all(b > 0 for b in edges[k][1:]) and any(b * num % den for b in edges[k][1:])
        total = x.n[k] + x.tail[k]
        levels = _model(x.roles[k], x.entries[k], total, CARRIER_RATE, num, den, tx.answers_tx_config(**carrier_kw(True)).delay_samples)
        got, pend, sizes = in_pieces(x.roles[k], x.entries[k], edges[k][1:], total, **carrier_kw(True))
        assert not pend.tobytes().strip(b'\0') and len(got) == len(levels)
        assert np.abs(got - carrier_reference(levels)).max() <= 1.5e-7 * AMP
        off, _, _ = in_pieces(x.roles[k], x.entries[k], edges[k][1:], total, **carrier_kw(False))
        assert off.real.tobytes() == levels.tobytes() and not off.imag.any()


@gpu
@pytest.mark.parametrize('carrier', [True, False])
def test_gpu_the_carrier_across_pushes(carrier):
    x, kw = captures(), carrier_kw(carrier)
    num, den = ratio(CARRIER_RATE)
    with _context(x.cards, max(x.n + x.tail)) as m:
        pieces_of_push, n_push = _cut_pieces(x, _piece_cuts(x.frame_idx[0], x.frame_idx[1], x.names[0]))
        whole, bases = _run_captures(m, x, kw, pieces_of_push, n_push)
    assert any(b[0] * num % den for b in bases[1:]) and any(b[1] * num % den for b in bases[1:])
    for k in (0, 1):
        levels = _model(x.roles[k], x.entries[k], x.n[k] + x.tail[k], CARRIER_RATE, num, den, tx.answers_tx_config(**kw).delay_samples)
        if carrier:
            assert np.abs(whole[k] - carrier_reference(levels)).max() <= 1.5e-7 * AMP, k
        else:
            assert whole[k].real.tobytes() == levels.tobytes() and not whole[k].imag.any(), k
    assert math.isclose(CARRIER_RATE / IN_RATE, num / den)
