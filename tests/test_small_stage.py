"""k_small_stage (csrc/small.hip.h), the one launch that every batch of at most SM_MAX_SAMPLES samples takes, where its loops,
capacities and tables turn over.  One workgroup walks the edge stage in trips of SM_BLOCK words, lists a trip's entries in rounds of
SM_EVCAP, walks the decoders in trips of SM_BLOCK * DEC_ITEMS entries and frames in the same pass; the per-item arithmetic is the
multi-launch stages', the orchestration is its own.  What survives in that form is a round that is not taken, a carry that is not
added from trip to trip, a clamp that is forgotten under an overflowing estimate, a table read from the wrong place.

EVERY CASE IS COMPARED FOR EQUALITY WITH TWO THINGS: the C oracle (tests/test_gpu_parity.py: check_vs_oracle -- val, transitions,
both symbol streams, packets, the pushes accumulated), and the same pushes through the multi-launch stages (NFC_NO_SMALL=1 in the
test build): per push the entries with their indices, the symbols, the packet tables with their closing indices, the packet bits
and val, and after the last push counts() and the get_state blob.  The product library runs with no switch: the batch length alone
selects the kernel.

THE THRESHOLDS ARE READ, NOT REMEMBERED (constants(): small.hip.h, decode.hip.h, host_context.h, host_stages.h), and every case
carries a `crosses` function that asserts, from the C oracle's output and those constants alone, that its input crosses the line it
is there for.  test_the_inputs_cross_their_lines runs all of them without a GPU; each GPU test runs its own first.  host_model()
restates size_capacities / update_estimates of host_stages.h, so "the first estimate overflows" is an assertion, not a hope.

WHAT THE max_len = 50 FLICKER DOES NOT DO.  The three-level flicker at max_len = 50 closes a handful of one-bit packets: nearly all of
its 79 000 reader symbols are non-bits, and no packet collects more than a few bits (flicker50_pieces asserts what is true of it,
and the pieces stay as cases).  A packet that stays open over hundreds of short pushes is long_frames(): a 700-byte reader frame
and a 700-byte tag frame, 6 300 bits each, pushed in pieces of 8 192 and 777 samples."""
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import py_oracle as po
from tests.golden_util import GOLDEN, Case as GoldenCase
from tests.test_gpu_parity import check_case, check_vs_oracle, run_gpu
from usrp_nfc_amd import _lib, api, synth

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')
ENV, IQ = api.NFC_IN_ENV_F32, api.NFC_IN_IQ_F32
LOW, MID, HIGH = np.float32(0.01), np.float32(0.25), np.float32(0.25 * 1.3)
LEVELS = np.array([LOW, MID, HIGH], np.float32)
FLICKER = dict(hi_val=1.1, av_window=500)   # the parameters of the flicker captures
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- 0. the thresholds, from the source text --------------------------------------------------------------------------------------------
class Constants(object):
    pass


def _match(text, name, pattern, where):
    m = re.search(pattern, text)
    assert m, '%s: no definition of %s matches %r any more' % (where, name, pattern)
    return m


def constants():
    def read():
        c = Constants()
        src = {f: open(os.path.join(CSRC, f)).read() for f in ('small.hip.h', 'decode.hip.h', 'host_context.h', 'host_stages.h')}
        for name in ('SM_BLOCK', 'SM_EVCAP'):
            setattr(c, name, int(_match(src['small.hip.h'], name, r'\b%s\s*=\s*(\d+)\s*[,;]' % name, 'small.hip.h').group(1)))
        c.SM_MAX_SAMPLES = 1 << int(_match(src['small.hip.h'], 'SM_MAX_SAMPLES', r'\bSM_MAX_SAMPLES\s*=\s*1u\s*<<\s*(\d+)\s*;', 'small.hip.h').group(1))
        _match(src['small.hip.h'], 'the trip', r'w0\s*<\s*A\.nwords;\s*w0\s*\+=\s*SM_BLOCK\b', 'small.hip.h')
        _match(src['small.hip.h'], 'the round', r'rbase\s*<\s*total;\s*rbase\s*\+=\s*SM_EVCAP\b', 'small.hip.h')
        _match(src['small.hip.h'], 'the decode trip', r'e0\s*<\s*ne;\s*e0\s*\+=\s*\(size_t\)SM_BLOCK\s*\*\s*DEC_ITEMS\b', 'small.hip.h')
        _match(src['small.hip.h'], 'the table placement', r'lds_tab\s*=\s*4\s*\*\s*A\.T\.nd\s*<=\s*DEC_LDS_ROWS\b', 'small.hip.h')
        _match(src['host_stages.h'], 'nd', r'A\.E\.nd\s*=\s*c->mx\s*\+\s*1\s*;', 'host_stages.h')
        _match(src['host_stages.h'], 'the path choice', r'c->use_small\s*&&\s*n\s*<=\s*SM_MAX_SAMPLES\b', 'host_stages.h')
        for name in ('DEC_ITEMS', 'DEC_LDS_ROWS'):
            setattr(c, name, int(_match(src['decode.hip.h'], name, r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, 'decode.hip.h').group(1)))
        c.EDGE_RATE = float(_match(src['host_context.h'], 'edge_rate', r'double\s+edge_rate\s*=\s*([0-9.]+)\s*;', 'host_context.h').group(1))
        m = _match(src['host_context.h'], 'sym_rate', r'double\s+sym_rate\[2\]\s*=\s*\{\s*([0-9.]+)\s*,\s*([0-9.]+)\s*\}\s*;', 'host_context.h')
        c.SYM_RATE = (float(m.group(1)), float(m.group(2)))
        hs = src['host_stages.h']
        m = _match(hs, 'cap_edges', r'\(double\)n\s*\*\s*c->edge_rate\s*\*\s*([0-9.]+)\)\s*\+\s*(\d+)\s*;', 'host_stages.h')
        c.EDGE_HEADROOM, c.EDGE_FLOOR = float(m.group(1)), int(m.group(2))
        m = _match(hs, 'alloc_edges', r'\(uint64_t\)n\s*/\s*(\d+)\s*\+\s*(\d+)\s*,', 'host_stages.h')
        c.ALLOC_DIV, c.ALLOC_FLOOR = int(m.group(1)), int(m.group(2))
        m = _match(hs, 'cap_sym', r'\(double\)c->cap_edges\s*\*\s*c->sym_rate\[t\]\s*\*\s*([0-9.]+)\)\s*\+\s*(\d+)\s*;', 'host_stages.h')
        c.SYM_HEADROOM, c.SYM_FLOOR = float(m.group(1)), int(m.group(2))
        _match(hs, 'the symbol bound', r'\(t\s*==\s*1\s*\?\s*2ull\s*:\s*1ull\)\s*\*\s*c->cap_edges\s*\+\s*16\s*;', 'host_stages.h')
        m = _match(hs, 'the edge rate update', r'c->edge_rate\s*=\s*std::max\(\{\(double\)c->n_edges\s*/\s*\(double\)n,\s*c->edge_rate\s*\*\s*([0-9.]+),\s*1\.0\s*/\s*(\d+)\}\);',
                   'host_stages.h')
        c.RATE_DECAY, c.RATE_MIN = float(m.group(1)), 1.0 / int(m.group(2))
        m = _match(hs, 'the symbol rate update', r'if\s*\(c->n_edges\)\s*c->sym_rate\[t\]\s*=\s*std::max\(\(double\)c->n_sym\[t\]\s*/\s*\(double\)c->n_edges,\s*c->sym_rate\[t\]\s*\*\s*([0-9.]+)\);',
                   'host_stages.h')
        c.SYM_DECAY = float(m.group(1))
        _match(hs, 'the fit', r'fit\s*=\s*ne\s*<=\s*c->cap_edges\s*&&\s*ns\[0\]\s*\+\s*2\s*<=\s*c->cap_sym\[0\]\s*&&\s*ns\[1\]\s*\+\s*2\s*<=\s*c->cap_sym\[1\]\s*;', 'host_stages.h')
        c.TRIP = c.SM_BLOCK * 64                 # samples of an edge trip
        c.DEC_TRIP = c.SM_BLOCK * c.DEC_ITEMS    # entries of a decode trip
        return c
    return cached('constants', read)


def test_the_thresholds_are_read_from_the_sources():
    c = constants()
    assert c.SM_BLOCK % 64 == 0 and c.SM_EVCAP > 0 and c.SM_MAX_SAMPLES > 4 * c.TRIP
    assert c.TRIP > 2 * c.SM_EVCAP, 'a trip of flicker no longer takes a third round'
    assert c.DEC_LDS_ROWS % 4 == 0 and c.DEC_ITEMS > 0
    assert 0 < c.EDGE_RATE < 1 and c.EDGE_HEADROOM > 1 and c.SYM_HEADROOM > 1 and 0 < c.RATE_DECAY < 1 and 0 < c.SYM_DECAY < 1
    with pytest.raises(AssertionError, match='NO_SUCH_NAME'):   # a pattern that no longer matches fails loudly
        _match('constexpr int SM_BLOCK = 256;', 'NO_SUCH_NAME', r'\bNO_SUCH_NAME\s*=\s*(\d+)', 'a text')


# ---- the oracle's view of a case, and the host's capacity arithmetic over it ------------------------------------------------------------
class Case(object):
    def __init__(self, name, x, params, cuts, crosses, kind=ENV):
        self.name, self.x, self.params, self.kind, self.crosses = name, x, params, kind, crosses
        self.n = len(x) // (2 if kind == IQ else 1)
        self.cuts = [0, self.n] if cuts is None else list(cuts)
        x.setflags(write=False)

    def piece(self, a, b):
        per = 2 if self.kind == IQ else 1
        return self.x[a * per:b * per]


def oracle_pushes(case):
    """The case's pushes through the C oracle: per push its entries (EDGE_DTYPE rows, global idx), symbol counts and packets."""
    def make():
        o = co.COracle(**case.params)
        try:
            out = []
            for a, b in zip(case.cuts[:-1], case.cuts[1:]):
                o.clear_outputs()
                (o.push_iq if case.kind == IQ else o.push_env)(case.piece(a, b))
                e = o.edges()
                assert ((e['idx'] >= a) & (e['idx'] < b)).all(), 'the oracle lists an entry with the push that holds its sample'
                out.append(dict(a=a, b=b, n=b - a, edges=e, ns=(len(o.symbols(0)), len(o.symbols(1))), sym=(o.symbols(0), o.symbols(1)), packets=o.packets()))
            return out
        finally:
            o.close()
    return cached(('oracle', case.name), make)


def host_model(case, c):
    """size_capacities / update_estimates of host_stages.h over the oracle's counts: per push None (nothing but window fill) or the
    estimates the FIRST run of the batch gets -- cap_edges, cap_sym[2], the entries allocated for -- and whether that run fits."""
    rate, sym, alloc, filled, rows = c.EDGE_RATE, list(c.SYM_RATE), 0, 0, []
    L = case.params.get('av_window', 2000)
    for p in oracle_pushes(case):
        n, ne, ns = p['n'], len(p['edges']), p['ns']
        skip = min(n, L - filled)
        filled += skip
        if skip == n:
            rows.append(None)
            continue
        cap = int(n * rate * c.EDGE_HEADROOM) + c.EDGE_FLOOR
        cap_sym = [min((2 if t == 1 else 1) * cap + 16, int(cap * sym[t] * c.SYM_HEADROOM) + c.SYM_FLOOR) for t in (0, 1)]
        alloc = max(alloc, n // c.ALLOC_DIV + c.ALLOC_FLOOR, cap)
        rows.append(dict(cap_edges=cap, cap_sym=cap_sym, alloc=alloc, skip=skip, n=n, ne=ne, ns=ns, edges_fit=ne <= cap,
                         sym_fit=ns[0] + 2 <= cap_sym[0] and ns[1] + 2 <= cap_sym[1]))
        rate = max(ne / n, rate * c.RATE_DECAY, c.RATE_MIN)
        if ne:
            sym = [max(ns[t] / ne, sym[t] * c.SYM_DECAY) for t in (0, 1)]
    return rows


def assert_no_repeat(case, c):
    """no capacity repeat: the case is about something else, and says so"""
    for i, r in enumerate(host_model(case, c)):
        assert r is None or (r['edges_fit'] and r['sym_fit']), '%s: push %d would repeat for capacity (%r)' % (case.name, i, r)


def assert_small(case, c, but=()):
    for i, p in enumerate(oracle_pushes(case)):
        assert (p['n'] <= c.SM_MAX_SAMPLES) == (i not in but), '%s: push %d has %d samples' % (case.name, i, p['n'])
    assert case.n <= c.SM_MAX_SAMPLES + 1, 'no capture is longer than SM_MAX_SAMPLES + 1'


def trip_counts(p, c):
    """entries per edge trip of a push (batch-local sample // TRIP)"""
    return np.bincount((p['edges']['idx'].astype(np.int64) - p['a']) // c.TRIP, minlength=(p['n'] + c.TRIP - 1) // c.TRIP)


def frame_states(edges, rate=2e6):
    """The reference's decoders and framing over the oracle's entries, entry by entry (oracle/py_oracle.py; as tests/test_decode_tiles.py's
    Ref): per entry and type the open packet's bit count AFTER the entry, -1 while no packet is open; and per closed packet
    (type, bits, the closing entry's place)."""
    sink = po.BitSink()
    mil, man = po.MillerDecoder(sink), po.ManchesterDecoder(sink)
    f = 1e6 / rate
    st, closed = np.zeros((len(edges), 2), np.int64), []
    for i, (d, v, t) in enumerate(zip(edges['d'].tolist(), edges['v'].tolist(), edges['t'].tolist())):
        dec = mil if t == 1 else (man if t == 0 else None)
        if dec is not None:
            dec.process_transition([(v, d * f)])
        while len(closed) < len(sink.packets):
            closed.append(i)
        for k, p in enumerate(sink.procs):
            st[i, k] = len(p.cur) if p.started else -1
    return st, closed, sink


def all_edges(case):
    return np.concatenate([p['edges'] for p in oracle_pushes(case)])


# ---- 1. rounds of the entry writer ----------------------------------------------------------------------------------------------------------
def flicker(n, a, b, seed):
    x = np.full(n, MID, np.float32)
    x[a:b] = LEVELS[np.random.default_rng(seed).integers(0, 3, b - a)]
    return x


def case_flicker_ml1(cut):
    """max_len = 1: every sample behind the window fill is an entry, a whole trip holds TRIP of them: TRIP / SM_EVCAP rounds"""
    c = constants()
    n = 4 * c.TRIP + 4321
    name = 'flicker_ml1_' + ('cut' if cut else 'whole')

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        full = [int(k) for p in oracle_pushes(case) for k in trip_counts(p, c)]
        assert full.count(c.TRIP) >= 2 and c.TRIP > 3 * c.SM_EVCAP, 'whole trips of an entry per sample: four rounds each'
        if cut:
            p = oracle_pushes(case)[1]
            assert p['a'] % 2 == 1 and p['a'] % 64 and trip_counts(p, c)[0] == c.TRIP and trip_counts(oracle_pushes(case)[0], c)[-1] > c.SM_EVCAP, 'cut at an odd sample inside a dense trip'
    return Case(name, flicker(n, 600, n - 2000, 11), dict(max_len=1, **FLICKER), [0, 2 * c.TRIP + 5003, n] if cut else None, crosses)


def crafted_trip(target):
    """Three trips and a ragged end at max_len = 50: a sparse one (the window fill, pulses), one that holds EXACTLY `target` entries --
    from `lead` samples into the trip LOW and HIGH alternate, every sample an entry, the rest of the trip idles with a heartbeat every
    max_len samples --, a sparse one.  -> (x, lead)"""
    c = constants()
    n, t0 = 3 * c.TRIP + 1001, c.TRIP
    params = dict(max_len=50, **FLICKER)

    def build(lead, dense):
        x = np.full(n, MID, np.float32)
        for s in (2000, 7000, 7100, 12000, 2 * c.TRIP + 300, 2 * c.TRIP + 5000, 2 * c.TRIP + 5030, 3 * c.TRIP + 100):
            x[s:s + 17] = LOW
            x[s + 40:s + 43] = HIGH
        x[t0 + lead:t0 + lead + dense:2] = LOW
        x[t0 + lead + 1:t0 + lead + dense:2] = HIGH
        return x

    def count(x):
        o = co.COracle(**params)
        o.push_env(x)
        idx = o.edges()['idx'].astype(np.int64)
        o.close()
        return idx[(idx >= t0) & (idx < t0 + c.TRIP)] - t0

    for lead in (37, 5, 59, 22, 45, 13, 51, 30):
        dense = max(2, target - c.TRIP // 50)
        for _ in range(16):
            x = build(lead, dense)
            got = count(x)
            if len(got) == target:
                if target >= 2 * c.SM_EVCAP and not straddles(got, c):
                    break
                return x, lead
            dense += target - len(got)
            if not 2 <= dense <= c.TRIP - lead:
                break
    raise AssertionError('no crafted trip of exactly %d entries' % target)


def straddles(local, c):
    """a 64-entry word of the trip has entries on both sides of the first round's end"""
    w = local // 64
    return w[c.SM_EVCAP - 1] == w[c.SM_EVCAP] and int((w == w[c.SM_EVCAP]).sum()) == 64


def case_crafted(spec):
    c = constants()
    target = {'evcap-1': c.SM_EVCAP - 1, 'evcap': c.SM_EVCAP, 'evcap+1': c.SM_EVCAP + 1, '2evcap': 2 * c.SM_EVCAP, '2evcap+1': 2 * c.SM_EVCAP + 1}[spec]
    x, lead = cached(('crafted', spec), lambda: crafted_trip(target))

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        p, = oracle_pushes(case)
        k = trip_counts(p, c)
        assert k[1] == target, 'the dense trip holds %d entries, not %d' % (k[1], target)
        assert 0 < k[0] < c.SM_EVCAP and 0 < k[2] < c.SM_EVCAP and k[3] > 0, 'a sparse trip before and behind: n_edges_all carries across trips'
        local = p['edges']['idx'].astype(np.int64) - c.TRIP
        local = local[(local >= 0) & (local < c.TRIP)]
        dense = np.bincount(local // 64, minlength=c.SM_BLOCK)
        assert dense[1] == 64 and dense[0] < 64 and dense[-1] <= 2, 'dense words first (from sample %d), idle words for the rest' % lead
        if target >= 2 * c.SM_EVCAP:
            assert straddles(local, c), 'one thread lists its 64 entries in two rounds'
    return Case('crafted_' + spec, x, dict(max_len=50, **FLICKER), None, crosses)


# ---- 2. time-outs over the orchestration's seams ------------------------------------------------------------------------------------------
RUN_SPECS = ((1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (3, 1))   # k, delta: runs of k * max_len + delta samples


def case_timeouts(max_len, mode):
    """LOW and HIGH runs of k * max_len + {-1, 0, 1} samples, each across a seam: mode 'trips' -- one push, the seams are the edge
    trips' (run_l2 carries the last two changes over them); mode 'pushes' -- a push per trip, cut at the same samples (the edge carry
    does), and a push in which nothing happens at all.  max_len = 1 has an entry per sample: a first push of 60 000 idle samples
    brings the estimate up to that, so the case is not about the capacity repeat."""
    c = constants()
    base = 60000 if max_len == 1 else 0
    lens = sorted(set(k * max_len + d for k, d in RUN_SPECS if k * max_len + d > 0))
    runs = [(ln, lv) for ln in lens for lv in (LOW, HIGH)]
    n = base + (len(runs) + 1) * c.TRIP + 777
    rng = np.random.default_rng(500 + max_len)
    x = (MID * (1 + 0.002 * rng.standard_normal(n))).astype(np.float32)
    seams, placed = [base + (i + 1) * c.TRIP for i in range(len(runs))], []
    for s, (ln, lv) in zip(seams, runs):
        start = s - max(1, ln // 2)
        x[start:start + ln] = lv
        placed.append((start, ln, s))
        x[s + 300:s + 303] = HIGH     # something else in every trip
        x[s + 340:s + 345] = LOW
    cuts, empty = None, None
    if mode == 'trips':
        cuts = [0, base, n] if base else None
    else:
        cuts = [0] + seams + [n]
        if max_len > 1:   # a push between two heartbeats of the idle tail: no entry at all
            o = co.COracle(max_len=max_len, **FLICKER)
            o.push_env(x)
            idx = o.edges()['idx'].astype(np.int64)
            o.close()
            tail = idx[idx > seams[-1] + 1000]
            i = int(np.flatnonzero(np.diff(tail) == max_len)[0])
            empty = (int(tail[i]) + 1, int(tail[i + 1]))
            cuts = sorted(set(cuts + list(empty)))

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        e = all_edges(case)
        idx, d = e['idx'].astype(np.int64), e['d'].astype(np.int64)
        for start, ln, s in placed:
            assert (case.x[start:start + ln] == case.x[start]).all() and case.x[start - 1] != case.x[start] and case.x[start + ln] != case.x[start]
            if ln >= 2:
                assert start < s < start + ln, 'the run starts in one trip / push and ends in the next'
            else:
                assert start == s - 1, 'a run of one sample: the trip\'s / push\'s last'
            k = int(np.searchsorted(idx, s))
            assert idx[k] <= start + ln and idx[k] - d[k] < s, 'the first entry behind the seam measures back across it'
        for p in oracle_pushes(case):
            if mode == 'trips' and p['a'] <= placed[0][2] < p['b']:
                assert p['b'] == case.n and all((s - p['a']) % c.TRIP == 0 for _, _, s in placed), 'the seams are trip edges of the push'
        if empty:
            p, = [p for p in oracle_pushes(case) if (p['a'], p['b']) == empty]
            assert len(p['edges']) == 0 and p['n'] == max_len - 1, 'a push without an entry: ne = 0, no decode trip'
    return Case('timeouts_%d_%s' % (max_len, mode), x, dict(max_len=max_len, **FLICKER), cuts, crosses)


# ---- 3. decode loop trips -------------------------------------------------------------------------------------------------------------------
DECODE_KINDS = {'reader': ('miller', dict(tag=False)), 'tag': ('manchester', dict(reader=False)), 'both': ('all', dict())}


def case_decode_trips(kind, spec):
    """A push whose entry count is exactly DEC_TRIP, DEC_TRIP + 1 or 2 DEC_TRIP + 1, cut out of a workload by the oracle's entry indices,
    with a packet open at every trip edge (at the push's end for one whole trip)."""
    c = constants()
    target = {'trip': c.DEC_TRIP, 'trip+1': c.DEC_TRIP + 1, '2trips+1': 2 * c.DEC_TRIP + 1}[spec]
    wl, flags = DECODE_KINDS[kind]
    params = dict(hi_val=1.1, **flags)
    want = [t for t in (0, 1) if (t == 0 and flags.get('tag', True)) or (t == 1 and flags.get('reader', True))]
    edge_ranks = [r for r in range(c.DEC_TRIP, target + 1, c.DEC_TRIP)]

    def prepare():
        iq = synth.workload(wl, c.SM_MAX_SAMPLES)
        o = co.COracle(**params)
        o.push_iq(iq)
        e = o.edges()
        o.close()
        st, _, _ = frame_states(e)
        is_open = (st[:, want] >= 0).any(axis=1)
        return iq, e['idx'].astype(np.int64), is_open
    iq, idx, is_open = cached(('decode', kind), prepare)
    r0 = next(r for r in range(200, len(idx) - target - 1) if all(is_open[r + k - 1] for k in edge_ranks) and idx[r] - idx[r - 1] > 1)
    cuts = [0, int(idx[r0 - 1]) + 1, int(idx[r0 + target - 1]) + 1, len(iq) // 2]

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        p = oracle_pushes(case)[1]
        assert len(p['edges']) == target, (len(p['edges']), target)
        st, _, _ = frame_states(np.concatenate([q['edges'] for q in oracle_pushes(case)[:2]]))
        first = len(oracle_pushes(case)[0]['edges'])
        for k in edge_ranks:
            assert (st[first + k - 1, want] >= 0).any(), 'a packet is open behind entry %d of the push' % k
        assert all(q['ns'][t] > 0 for q in oracle_pushes(case) for t in want)
    return Case('decode_%s_%s' % (kind, spec), iq, params, cuts, crosses, kind=IQ)


# ---- 4. capacity repeats ----------------------------------------------------------------------------------------------------------------------
def case_capacity(which):
    """(a) entries above the first estimate, below the allocation; (b) above the allocation; (c) the overflow in a LATER push of a stream
    whose estimate has decayed, a packet open with bits pending; (d) the symbols overflow and the entries do not.  A sparse push
    behind each."""
    c = constants()
    N = c.SM_MAX_SAMPLES
    if which in 'ab':
        x, cuts, params, at = flicker(N, 3000, 233000, 5), [0, 240000, N], dict(max_len=7 if which == 'a' else 1, **FLICKER), 0
    elif which == 'c':
        # 20 sparse pushes (a heartbeat per max_len samples, some reader traffic) let the estimate decay; the last of them opens a reader
        # packet -- a pause, a start bit, ones -- that the flicker's first non-bit closes in the overflowing push
        x = flicker(N, 30000, 233000, 5)
        env = synth.envelope_f32(synth.iq_from_profile(synth.modulation_profile([(synth.READER, synth.frame_bits([0xA5] * 60))], lead_in=0, tail=0), sigma=0.0))
        x[30000 - 700:30000] = env[:700]   # (a carrier of amplitude 0.5: the idle level, MID)
        x[250000 - 700:250000 - 700 + len(env)] = env   # ... and another that the overflowing push leaves open: what the REPEATED run carries on
        cuts, params, at = list(range(0, 30001, 1500)) + [250000, N], dict(max_len=50, **FLICKER), 20
    else:
        x = flicker(N, 28000, 233000, 5)
        cuts, params, at = list(range(0, 28001, 1000)) + [250000, N], dict(max_len=1, **FLICKER), 28

    def crosses(case, c):
        assert_small(case, c)
        rows = host_model(case, c)
        r = rows[at]
        for i, q in enumerate(rows):
            assert i == at or q is None or (q['edges_fit'] and q['sym_fit']), 'push %d repeats too: %r' % (i, q)
        assert rows[at + 1]['ne'] <= rows[at + 1]['n'] // (16 if which == 'c' else case.params['max_len']) + 2, 'a sparse push behind the repeat: heartbeats (c: a frame\'s rest)'
        if which == 'a':
            assert r['cap_edges'] < r['ne'] <= r['alloc'], r
        elif which == 'b':
            assert r['ne'] > r['alloc'] > r['cap_edges'], r
        elif which == 'c':
            assert r['cap_edges'] < r['ne'] and r['cap_edges'] < c.EDGE_FLOOR + r['n'] // 8, r   # (a low estimate: the sparse pushes' rate)
            st, _, _ = frame_states(all_edges(case)[:sum(len(p['edges']) for p in oracle_pushes(case)[:at])])
            assert st[-1, 1] > 0, 'a reader packet is open at the overflowing push, with bits pending'
            assert any(t == 1 and len(b) >= st[-1, 1] for t, b in oracle_pushes(case)[at]['packets']), '... and closes in it'
            # at the push's END a reader packet is open again, far behind the entries the first, truncated run saw: the pending bits and
            # the decoder states the next push starts from are the repeated run's
            e = oracle_pushes(case)[at]['edges']
            st, _, _ = frame_states(all_edges(case)[:sum(len(p['edges']) for p in oracle_pushes(case)[:at + 1])])
            assert st[-1, 1] >= 20 and e['idx'][r['cap_edges']] < 250000 - 700 - 10000, (st[-1], e['idx'][r['cap_edges']])
            assert any(t == 1 and len(b) >= 9 * 60 for t, b in oracle_pushes(case)[at + 1]['packets']), 'the packet closes in the sparse push behind'
        else:
            assert r['edges_fit'] and r['ns'][1] + 2 > r['cap_sym'][1] and r['ns'][0] + 2 <= r['cap_sym'][0], r
            # (the symbols are non-bits: the kernel's `nbits > cap_bits || ncl > cap_close` branch needs more than SYM_FLOOR BITS or
            # closes of one type in a batch of SM_MAX_SAMPLES samples, one per four samples -- DESIGN.md section 6 says why no capture does that)
            assert c.SYM_FLOOR * 4 >= c.SM_MAX_SAMPLES
    return Case('capacity_' + which, x, params, cuts, crosses)


# ---- 5. packets that stay open over short pushes -----------------------------------------------------------------------------------------
def case_flicker50_pieces(step):
    """The max_len = 50 three-level flicker in pieces.  Its packets are short (the module's docstring): what the pieces do cross is every
    carry of the kernel at hundreds of places of a dense stream, the decoders in the middle of their error states."""
    c = constants()
    N = c.SM_MAX_SAMPLES

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        ps = oracle_pushes(case)
        assert len(ps) == -(-N // step) and sum(len(p['edges']) for p in ps) > N // 4
        assert sum(1 for p in ps if p['ns'][1] > 0) > len(ps) // 2 and sum(len(p['packets']) for p in ps) >= 5
    return Case('flicker50_pieces_%d' % step, flicker(N, 3000, 233000, 5), dict(max_len=50, **FLICKER), list(range(0, N, step)) + [N], crosses)


LONG_BYTES = 700


def case_long_frames(step):
    """A 700-byte reader frame and a 700-byte tag frame (6 300 bits each) in pieces of `step` samples: the open packet's pending bits grow
    to many times what a push appends before a later push closes it."""
    def make():
        rng = np.random.default_rng(77)
        frames = [(d, synth.frame_bits(rng.integers(0, 256, LONG_BYTES).tolist(), 0)) for d in (synth.READER, synth.TAG)]
        iq = synth.iq_from_profile(synth.modulation_profile(frames, rate_msps=2.0, gap_us=100.0, lead_in=2500, tail=400))
        iq.setflags(write=False)
        return iq
    iq = cached('long_frames', make)
    n = len(iq) // 2

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        ps = oracle_pushes(case)
        for t in (0, 1):
            (k, bits), = [(i, b) for i, p in enumerate(ps) for ty, b in p['packets'] if ty == t and len(b) > 1000]
            assert len(bits) >= 9 * LONG_BYTES - 1   # (the framing drops the tag frame's last bit with its end-of-frame)
            # of the packet's bits at most ns[t] were appended in the push that closes it: the rest was pending when it began
            pending = len(bits) - ps[k]['ns'][t]
            assert pending >= 4 * max(p['ns'][t] for p in ps), 'pending bits several times what a push appends (%d against %d)' % (pending, max(p['ns'][t] for p in ps))
            assert k >= 8, 'open over many pushes'
    return Case('long_frames_%d' % step, iq, dict(hi_val=1.1), list(range(0, n, step)) + [n], crosses, kind=IQ)


# ---- 6. tables in LDS and in global memory -------------------------------------------------------------------------------------------------
def glitched_workload(max_len):
    """60 000 samples of the whole transaction, and in its idle gaps HIGH runs of max_len - 3 .. max_len samples that go straight into a
    pause: reader-route entries with v = 2 and the longest durations, the LAST rows of the Miller tables (li = (v + 1) (max_len + 1) + d).
    Those are the rows that do not fit when a table is one max_len too long for its LDS slot -- with the tag decoder on, the Manchester
    step table lies right behind the Miller one."""
    iq = synth.workload('all', 60000).copy()
    o = co.COracle(hi_val=1.1)
    o.push_iq(iq)
    e = o.edges()
    o.close()
    real = e['idx'][e['t'] >= 0].astype(np.int64)
    gaps = real[:-1][np.diff(real) > 250]   # (150 us between frames: 300 samples)
    assert len(gaps) >= 8
    for k, p in enumerate(gaps):   # (behind a reader frame HIGH is not seen before the time-out: the gaps behind tag frames give the entries)
        ln = max_len - (k // 3 + k) % 4
        iq[2 * (p + 40):2 * (p + 40 + ln)] *= np.float32(1.2)
        iq[2 * (p + 40 + ln):2 * (p + 46 + ln)] *= np.float32(0.1)
    iq.setflags(write=False)
    return iq


def case_tables(max_len, streamed):
    c = constants()
    iq = cached(('tables_iq', max_len), lambda: glitched_workload(max_len))
    n = len(iq) // 2

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        rows = 4 * (max_len + 1)
        assert (rows == c.DEC_LDS_ROWS) if max_len == 127 else (rows == c.DEC_LDS_ROWS + 4), 'the last table that fits LDS / the first that does not'
        pk = [t for p in oracle_pushes(case) for t, b in p['packets'] if len(b) >= 7]
        assert pk.count(0) >= 3 and pk.count(1) >= 3, 'frames in both directions'
        e = all_edges(case)
        last_rows = np.flatnonzero((e['t'] == 1) & (e['v'] == 2) & (e['d'] > max_len - 4))
        assert len(last_rows) >= 8 and set(e['d'][last_rows].tolist()) >= set(range(max_len - 2, max_len + 1)), 'reader-route entries in the Miller tables\' last rows'
        assert case.params.get('tag', True) and case.params.get('reader', True), 'both decoders: both tables staged'
    return Case('tables_%d_%s' % (max_len, 'streamed' if streamed else 'whole'), iq, dict(hi_val=1.1, max_len=max_len),
                list(range(0, n, 7777)) + [n] if streamed else None, crosses, kind=IQ)


# ---- 7. the length seam -----------------------------------------------------------------------------------------------------------------------
def case_length(delta):
    c = constants()
    iq = cached('length_iq', lambda: synth.workload('all', c.SM_MAX_SAMPLES + 1))
    n = c.SM_MAX_SAMPLES + delta

    def crosses(case, c):
        assert_small(case, c, but=(0,) if delta > 0 else ())
        assert_no_repeat(case, c)
        assert case.n - c.SM_MAX_SAMPLES == delta and len(oracle_pushes(case)[0]['packets']) > 20
    return Case('length_%+d' % delta, iq[:2 * n], dict(hi_val=1.1), None, crosses, kind=IQ)


TINY = (100, 65, 1, 63, 64, 65, 1, 1, 130, 1000, 777, 1733)


def case_tiny_pushes():
    """pushes of 1, 63, 64 and 65 samples and others that are no multiple of 64, on a flicker with an entry in nearly every one; the
    window (128 samples) fills inside the second push"""
    cuts = [0] + np.cumsum(TINY).tolist()

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        rows = host_model(case, c)
        assert rows[0] is None and 0 < rows[1]['skip'] < rows[1]['n'], 'the window fill ends inside a batch'
        assert {1, 63, 64, 65} <= set(p['n'] for p in oracle_pushes(case)[2:]) and any(p['n'] % 64 for p in oracle_pushes(case))
        assert sum(1 for p in oracle_pushes(case)[1:] if len(p['edges'])) >= len(TINY) - 3
    return Case('tiny_pushes', flicker(cuts[-1], 0, cuts[-1], 9), dict(hi_val=1.1, av_window=128, max_len=7), cuts, crosses)


# ---- 8. a capture recorded from the unmodified reference ---------------------------------------------------------------------------------
def case_fixture(cut):
    """tests/golden/fx_dense_small.npz (make_golden.py --dense-small): max_len = 1 flicker, whole and cut at an odd sample of its dense trip"""
    g = cached('fixture', lambda: GoldenCase('fx_dense_small'))

    def crosses(case, c):
        assert_small(case, c)
        assert_no_repeat(case, c)
        assert case.n <= 20000 and case.params['max_len'] == 1 and os.path.getsize(os.path.join(GOLDEN, 'fx_dense_small.npz')) <= 385032
        ps = oracle_pushes(case)
        assert trip_counts(ps[0], c)[0] > (1 if cut else 3) * c.SM_EVCAP, 'an aligned trip of more than SM_EVCAP entries'
        # the oracle against what the reference gave
        o = co.COracle(**case.params)
        o.push_env(case.x)
        assert o.transitions() == g.transitions and o.symbols(0).tolist() == g.sym_tag.tolist() and o.symbols(1).tolist() == g.sym_reader.tolist()
        assert o.packets() == g.packets
        o.close()
    return Case('fixture_' + ('cut' if cut else 'whole'), g.x.copy(), g.params, [0, 9001, len(g.x)] if cut else None, crosses)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
CASES = {}
for _cut in (False, True):
    CASES['flicker_ml1_' + ('cut' if _cut else 'whole')] = (case_flicker_ml1, (_cut,))
for _spec in ('evcap-1', 'evcap', 'evcap+1', '2evcap', '2evcap+1'):
    CASES['crafted_' + _spec] = (case_crafted, (_spec,))
for _ml in (1, 31, 32, 63, 64):
    for _mode in ('trips', 'pushes'):
        CASES['timeouts_%d_%s' % (_ml, _mode)] = (case_timeouts, (_ml, _mode))
for _kind in ('reader', 'tag', 'both'):
    for _spec in ('trip', 'trip+1', '2trips+1'):
        CASES['decode_%s_%s' % (_kind, _spec)] = (case_decode_trips, (_kind, _spec))
for _w in 'abcd':
    CASES['capacity_' + _w] = (case_capacity, (_w,))
for _step in (8192, 777):
    CASES['flicker50_pieces_%d' % _step] = (case_flicker50_pieces, (_step,))
    CASES['long_frames_%d' % _step] = (case_long_frames, (_step,))
for _ml in (127, 128):
    for _s in (False, True):
        CASES['tables_%d_%s' % (_ml, 'streamed' if _s else 'whole')] = (case_tables, (_ml, _s))
for _d in (-1, 0, 1):
    CASES['length_%+d' % _d] = (case_length, (_d,))
CASES['tiny_pushes'] = (case_tiny_pushes, ())
for _cut in (False, True):
    CASES['fixture_' + ('cut' if _cut else 'whole')] = (case_fixture, (_cut,))


def get_case(name):
    def make():
        f, args = CASES[name]
        case = f(*args)
        assert case.name == name
        return case
    return cached(('case', name), make)


def test_the_inputs_cross_their_lines():
    c = constants()
    for name in CASES:
        case = get_case(name)
        case.crosses(case, c)
        _cache.pop(('oracle', name), None)   # (the captures stay, the oracle's lists go: some hundred MB over all cases otherwise)


# ---- the GPU half -------------------------------------------------------------------------------------------------------------------------------
def run_pushes(case, flags=0, lib_path=None):
    """The case's pushes through one context: per push everything the readers give, and the context's state behind the last."""
    out = []
    with api.NfcContext(input_kind=case.kind, flags=flags, lib_path=lib_path, **case.params) as ctx:
        for a, b in zip(case.cuts[:-1], case.cuts[1:]):
            ctx.push(case.piece(a, b))
            k = ctx.counts()
            row = dict(edges=ctx.edges(), val=ctx.val(), allocs=int(ctx.stats().device_allocs),
                       counts=(int(k.n_samples), int(k.n_edges), tuple(k.n_symbols), tuple(k.n_packets), tuple(k.n_packet_bits)))
            for t in (0, 1):
                row['sym%d' % t], row['table%d' % t], row['bits%d' % t] = ctx.symbols(t), ctx.packet_table(t), ctx.packet_bits(t)
            out.append(row)
        blob = ctx.state_blob()
    return out, blob


def assert_same_pushes(got, want, what):
    (g, gblob), (w, wblob) = got, want
    assert len(g) == len(w)
    for i, (a, b) in enumerate(zip(g, w)):
        assert a['counts'] == b['counts'], '%s: counts of push %d: %r / %r' % (what, i, a['counts'], b['counts'])
        for key in ('edges', 'val', 'sym0', 'sym1', 'table0', 'table1', 'bits0', 'bits1'):
            if not np.array_equal(a[key], b[key]):
                bad = np.flatnonzero(a[key] != b[key])[:3] if len(a[key]) == len(b[key]) else 'lengths %d / %d' % (len(a[key]), len(b[key]))
                raise AssertionError('%s: %s of push %d differ at %s' % (what, key, i, bad))
    assert np.array_equal(gblob, wblob), '%s: the state behind the last push differs at bytes %s' % (what, np.flatnonzero(gblob != wblob)[:8] if len(gblob) == len(wblob) else 'lengths')


def check_small_stage(monkeypatch, name):
    """-> the product library's pushes (k_small_stage wherever a push is short enough)"""
    case = get_case(name)
    c = constants()
    case.crosses(case, c)
    check_vs_oracle(case.x, case.params, kind=case.kind, pushes=case.cuts)
    small = run_pushes(case)
    ps = oracle_pushes(case)
    for i, (row, p) in enumerate(zip(small[0], ps)):   # the entries' indices and every count, push by push
        assert np.array_equal(row['edges']['idx'], p['edges']['idx'].astype(np.uint64)), 'entry indices of push %d' % i
        assert row['counts'][:3] == (p['n'], len(p['edges']), p['ns']), 'counts of push %d' % i
        assert sorted(len(b) for _, b in p['packets']) == sorted(row['table0']['n_bits'].tolist() + row['table1']['n_bits'].tolist())
    monkeypatch.setenv('NFC_NO_SMALL', '1')   # (the test build, and the multi-launch stages whatever the length)
    assert_same_pushes(small, run_pushes(case, lib_path=_lib.hooks_path()), name + ': k_small_stage against the multi-launch stages')
    return small


ROUNDS = [n for n in CASES if n.startswith(('flicker_ml1_', 'crafted_'))]
TIMEOUTS = [n for n in CASES if n.startswith('timeouts_')]
DECODE = [n for n in CASES if n.startswith('decode_')]
TABLES = [n for n in CASES if n.startswith('tables_')]
LENGTHS = [n for n in CASES if n.startswith('length_')] + ['tiny_pushes']


@pytest.mark.gpu
@pytest.mark.parametrize('name', ROUNDS)
def test_rounds_of_the_entry_writer(monkeypatch, name):
    check_small_stage(monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', TIMEOUTS)
def test_time_outs_over_trip_and_push_seams(monkeypatch, name):
    check_small_stage(monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', DECODE)
def test_decode_loop_trips(monkeypatch, name):
    check_small_stage(monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize('which', 'abcd')
def test_capacity_repeats(monkeypatch, which):
    case = get_case('capacity_' + which)
    at = {'a': 0, 'b': 0, 'c': 20, 'd': 28}[which]
    small, _ = check_small_stage(monkeypatch, case.name)
    if which == 'b':
        assert small[at]['allocs'] > 0, 'entries beyond the allocation: the repeat grows the buffers'
    assert all(row['allocs'] == 0 for row in small[at + 1:]), 'the push behind the repeat finds room'


@pytest.mark.gpu
@pytest.mark.parametrize('step', [8192, 777])
def test_flicker_in_short_pushes(monkeypatch, step):
    check_small_stage(monkeypatch, 'flicker50_pieces_%d' % step)


@pytest.mark.gpu
@pytest.mark.parametrize('step', [8192, 777])
def test_packets_open_over_many_short_pushes(monkeypatch, step):
    case = get_case('long_frames_%d' % step)
    small, _ = check_small_stage(monkeypatch, case.name)
    # the closing indices, from the reference's framing over the oracle's entries
    e = cached('long_frames_edges', lambda: all_edges(case))
    _, closed, sink = cached('long_frames_ref', lambda: frame_states(e))
    want = sorted((int(e['idx'][i]), t, len(b)) for i, (t, b) in zip(closed, sink.packets))
    got = sorted((int(r['idx']), t, int(r['n_bits'])) for row in small for t in (0, 1) for r in row['table%d' % t])
    assert got == want and len(want) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize('name', TABLES)
def test_tables_in_lds_and_in_global_memory(monkeypatch, name):
    check_small_stage(monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', LENGTHS)
def test_the_length_seam(monkeypatch, name):
    check_small_stage(monkeypatch, name)


@pytest.mark.gpu
def test_no_edges_flag_on_a_short_dense_batch(monkeypatch):
    """NFC_FLAG_NO_EDGES: the threshold stage alone -- no entries, val as the oracle's, and the edge carry (last_bit, dur, the state
    behind the window fill) as it was, in k_small_stage's place as in the multi-launch stages'."""
    c = constants()
    x = flicker(20000, 600, 19000, 3)
    params = dict(max_len=7, **FLICKER)
    o = co.COracle(trace=True, **params)
    o.push_env(x)
    trace = o.trace()
    o.close()
    assert len(x) <= c.SM_MAX_SAMPLES

    def run(lib_path=None):
        with api.NfcContext(input_kind=ENV, flags=api.NFC_FLAG_NO_EDGES, lib_path=lib_path, **params) as ctx:
            ctx.push(x[:600])
            h0 = ctx.get_state()[0]
            carry0 = (h0.last_bit, h0.dur)
            ctx.push(x[600:])
            k, h1 = ctx.counts(), ctx.get_state()[0]
            assert (int(k.n_edges), tuple(k.n_symbols), tuple(k.n_packets)) == (0, (0, 0), (0, 0))
            assert (h1.last_bit, h1.dur) == carry0, 'the edge carry is untouched'
            return ctx.val(), ctx.state_blob()
    val, blob = run()
    assert np.array_equal(val, trace[100:])
    monkeypatch.setenv('NFC_NO_SMALL', '1')
    val2, blob2 = run(_lib.hooks_path())
    assert np.array_equal(val, val2) and np.array_equal(blob, blob2)


@pytest.mark.gpu
@pytest.mark.parametrize('cut', ['whole', 'cut'])
def test_reference_fixture_of_a_dense_short_capture(monkeypatch, cut):
    case = get_case('fixture_' + cut)
    check_small_stage(monkeypatch, case.name)
    monkeypatch.delenv('NFC_NO_SMALL')
    monkeypatch.delenv('NFC_AMD_LIB')
    check_case(GoldenCase('fx_dense_small'), run_gpu(case.x, case.params, pushes=case.cuts))
