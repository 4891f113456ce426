"""What a push CARRIES, against the reference, after every push: nfc_state_header.ss (transition_sink._sum) on its 8 bytes, the ring
as float32 bit patterns, filled / stable, cur_state, last_bit, dur and the pending bits (tests/state_util.py) -- beside what the push
EMITS (edges, symbols, packets), which is all the other GPU modules compare with the reference.

The captures are tests/test_carried_state_host.py's, where their properties are asserted on the C oracle alone: ordinary streams, and the
families R (a rounding residue in _sum after every push), Z (zeros in the first window: an exact sum, and no sequential span), P (an odd
value that stays J windows: one to six sequential prefixes, seams inside LOW and HIGH runs, the round >= 6 exit) and M (odd values
accepted in mid-stream).

THE ROUTE is read from the test build (nfc_debug_threshold_route: parallel attempts, spans and samples of the sequential kernel, the
exit) and held against what the documented rule asks for, computed from the REFERENCE's ring (test_carried_state_host.expected_route,
t_clear): soundness -- the sequential kernel took at least every span in which the reference's window holds odd values -- and
conservatism -- at most one span more, unless the rule's own exits hand it the rest of the batch.

Shapes: av_window 256 is the shortest window the parallel path takes, 2000 brings the workgroup kernel; pushes of 45 000 .. 57 000
samples (six prefixes of eight windows and more than four spans behind them), 120 000 for av_window 2000; NFC_NO_SMALL=1 takes the same
pushes through the multi-launch stages and lets batches run ahead.  The longest sequential replay is a whole push of family M."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import test_carried_state_host as host
from tests.golden_util import GOLDEN, Case
from tests.state_util import assert_state_is_the_references
from usrp_nfc_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
ENV = api.NFC_IN_ENV_F32


def route_of(ctx):
    out = (C.c_uint32 * 4)()
    ctx.L.nfc_debug_threshold_route.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    assert ctx.L.nfc_debug_threshold_route(ctx.h, out) == 0
    return dict(attempts=int(out[0]), spans=int(out[1]), samples=int(out[2]), exit=int(out[3]))


class Marks(object):
    """The oracle's outputs are never cleared (its trace is the helper's record of the LOW samples): a push's share is what came since the marks."""

    def __init__(self, o):
        self.o = o
        self.n = [0, 0, 0, 0]

    def take(self):
        o, n = self.o, self.n
        all_ = [o.transitions(), o.symbols(0).tolist(), o.symbols(1).tolist(), o.packets()]
        new = [a[k:] for a, k in zip(all_, n)]
        self.n = [len(a) for a in all_]
        return new


def assert_outputs(view, want, where):
    got = [view.transitions(), view.symbols(0).tolist(), view.symbols(1).tolist(), view.packets()]
    for name, g, w in zip(('transitions', 'symbols 0', 'symbols 1', 'packets'), got, want):
        assert len(g) == len(w), '%s: %d %s, the reference has %d' % (where, len(g), name, len(w))
        assert g == w, '%s: %s differ' % (where, name)


def assert_route(got, n, av_window, t_clear_in_batch, where, cap=True):
    """Soundness (hard) and, unless cap is off, the conservatism cap of the module's docstring."""
    span = host.span_of(av_window)
    lo, hi, exit_ = host.expected_route(n, av_window, t_clear_in_batch)
    print('%s: route %s; the rule: %d samples, exit %d (t_clear %d, span %d)' % (where, got, lo, exit_, t_clear_in_batch, span))
    assert got['samples'] >= lo, '%s: a parallel attempt stood over a span in which the reference\'s window holds odd values: %s, the rule asks %d' % (where, got, lo)
    if not cap:
        return got['samples'] > 0
    if got['samples'] != lo:   # one span more, and whatever the rule's exits make of that
        lo2, hi2, exit2 = host.expected_route(n, av_window, t_clear_in_batch + span if t_clear_in_batch > 0 else 1)
        assert got['samples'] == lo2 and got['exit'] == exit2, '%s: more than one span beyond the rule: %s, the rule asks %d (one span more: %d)' % (where, got, lo, lo2)
    else:
        assert got['exit'] == exit_, '%s: %s, the rule\'s exit is %d' % (where, got, exit_)
    return got['samples'] > 0


def t_clear_in(b, a, e, odd_from):
    """t_clear of the batch [a, e): where in it the reference's window is clear of the capture's odd values (0: it never holds any).
    Beyond the batch's end where the guard can vouch for no batch of the stream (test_carried_state_host.never_provable)."""
    if host.never_provable(b.params):
        return e - a + 1
    return b.route_clear - a if (odd_from < e and b.route_clear > a) else 0


def push_all(b, odd_from, monkeypatch=None, no_small=False, restore_at=None, kw=None, cap=True):
    """Every push of the capture through one context of the test build: outputs, state and route against the reference after each.
    restore_at: after that push the state blob goes into a fresh context, which takes the remaining pushes as well."""
    if no_small:
        monkeypatch.setenv('NFC_NO_SMALL', '1')
    o = co.COracle(trace=True, **b.params)
    marks = Marks(o)
    L = b.params['av_window']
    seq = []
    others = []
    with api.NfcContext(input_kind=ENV, chunk_samples=b.chunk_samples, lib_path=_lib.hooks_path(), **dict(b.params, **(kw or {}))) as ctx:
        for k, (a, e) in enumerate(zip(b.cuts[:-1], b.cuts[1:])):
            o.push_env(b.x[a:e])
            want = marks.take()
            for c in [ctx] + others:
                where = 'push %d%s' % (k, '' if c is ctx else ' (restored context)')
                c.push(b.x[a:e])
                assert_outputs(c, want, where)
                assert_state_is_the_references(c, o, where)
                r = route_of(c)
                used = assert_route(r, e - a, L, t_clear_in(b, a, e, odd_from), where, cap)
                assert int(c.stats().used_sequential) == int(used), where
                if c is ctx:
                    seq.append(r)
            if restore_at == k:
                fresh = api.NfcContext(input_kind=ENV, chunk_samples=b.chunk_samples, lib_path=_lib.hooks_path(), **b.params)
                fresh.set_state_blob(ctx.state_blob())
                assert_state_is_the_references(fresh, o, 'the restored context before its first push')
                others.append(fresh)
        for c in others:
            c.close()
    return seq


def submit_all(b, odd_from, monkeypatch, depth, meets_range=None):
    """The same pushes as batches submitted ahead, `depth` in flight (the multi-launch stages: a short batch never runs ahead).  The
    state is read whenever nothing is in flight: after every batch with depth 1 (a batch submitted on its own still takes the
    submitted-ahead route: its threshold stage is enqueued at once and vouched for in nfc_wait), after the last with more.
    -> redone_total, and what the rule makes it: a batch runs ahead when the batch before it took no sequential span, and is repeated
    when it meets odd values (meets_range(k): the batches that do, where that is not a matter of t_clear)."""
    monkeypatch.setenv('NFC_NO_SMALL', '1')
    o = co.COracle(trace=True, **b.params)
    marks = Marks(o)
    pieces = list(zip(b.cuts[:-1], b.cuts[1:]))
    bufs = [api.DeviceBuffer(np.ascontiguousarray(b.x[a:e])) for a, e in pieces]
    expect_redone, prev_seq = 0, True   # (the first batch fills the window: never ahead)
    with api.NfcContext(input_kind=ENV, chunk_samples=b.chunk_samples, lib_path=_lib.hooks_path(), **b.params) as ctx:
        nxt = 0
        for k, (a, e) in enumerate(pieces):
            while nxt < len(bufs) and nxt < k + depth:
                ctx.submit_device(bufs[nxt], pieces[nxt][1] - pieces[nxt][0])
                nxt += 1
            ctx.wait()
            o.push_env(b.x[a:e])
            assert_outputs(ctx, marks.take(), 'batch %d' % k)
            meets = meets_range(k) if meets_range else t_clear_in(b, a, e, odd_from) > 0
            if meets and not prev_seq:
                expect_redone += 1
            r = route_of(ctx)
            print('batch %d: route %s, ran_ahead %d, redone_total %d' % (k, r, ctx.stats().ran_ahead, ctx.stats().redone_total))
            assert int(ctx.stats().redone_total) == expect_redone, 'batch %d: redone_total %d, the route asks for %d' % (k, ctx.stats().redone_total, expect_redone)
            assert r['samples'] > 0 or not meets, 'batch %d met odd values and no sample went the sequential way' % k
            assert not (prev_seq and int(ctx.stats().ran_ahead)), 'batch %d ran ahead of a batch that took a sequential span' % k
            prev_seq = r['samples'] > 0
            if ctx.submitted() == 0:
                assert_state_is_the_references(ctx, o, 'batch %d' % k)
        got = int(ctx.stats().redone_total)
    for buf in bufs:
        buf.free()
    return got, expect_redone


# ---- 1. ordinary streams --------------------------------------------------------------------------------------------------------------
_ordinary = {}


def ordinary(name):
    if name not in _ordinary:
        if name == 'classic':
            from tests.test_commands_host import PREFIX
            frames = synth.frames_from_trace(os.path.join(GOLDEN, '1k_with_enc.out'))[0][:PREFIX]
            _ordinary[name] = (synth.envelope_f32(synth.iq_from_profile(synth.modulation_profile(frames))), dict(samp_rate=2e6, hi_val=1.1))
        else:
            c = Case(name)
            _ordinary[name] = (np.ascontiguousarray(c.x, np.float32), c.params)
        _ordinary[name][0].setflags(write=False)
    return _ordinary[name]


@pytest.mark.parametrize('pieces', ['one', '777', '8192', 'random'])
@pytest.mark.parametrize('name', ['fx_ultralight_txn', 'classic', 'fx_stress_dropout'])
def test_ordinary_streams(name, pieces):
    x, params = ordinary(name)
    n = len(x)
    if pieces == 'one':
        cuts = [0, n]
    elif pieces == 'random':
        cuts = [0] + sorted(set(np.random.default_rng(11).integers(1, n, 9).tolist())) + [n]
    else:
        cuts = list(range(0, n, int(pieces))) + [n]
    o = co.COracle(trace=True, **params)
    marks = Marks(o)
    with api.NfcContext(input_kind=ENV, **params) as ctx:
        for k, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
            ctx.push(x[a:e])
            o.push_env(x[a:e])
            want = marks.take()
            # (the state after EVERY push; the outputs where the pushes are few -- tests/test_gpu_parity.py streams the fixtures in such pieces)
            if len(cuts) <= 12:
                assert_outputs(ctx, want, '%s, push %d' % (name, k))
            assert_state_is_the_references(ctx, o, '%s, push %d of %d' % (name, k, len(cuts) - 1))
    assert len(o.packets()) > 3


@pytest.mark.parametrize('kind', sorted(api._KIND_DTYPE))
def test_every_kind_every_form_carries_the_references_state(monkeypatch, kind):
    # the seven forms of tests/test_gpu_parity.py::test_every_kind_every_form on its capture: after the single push the state is the
    # oracle's over api.host_envelope of the same raw samples, whichever kernel of the kind's table took the batch
    from tests import test_gpu_parity as gp
    raw = gp._every_kind_raw(kind)
    o = co.COracle(trace=True, **gp._EVERY_PARAMS)
    o.push_env(api.host_envelope(raw, kind))
    want = Marks(o).take()
    forms = [({}, 0), ({}, api.NFC_FLAG_FORCE_SEQUENTIAL), (dict(NFC_WG_NR='8'), 0), (dict(NFC_WG_NR='4'), 0), (dict(NFC_WG='0'), 0),
             (dict(NFC_LEAN='0'), 0), (dict(NFC_RING='global'), 0)]
    for env, flags in forms:
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        with api.NfcContext(input_kind=kind, flags=flags, chunk_samples=16384, **gp._EVERY_PARAMS) as ctx:
            ctx.push(raw)
            assert_outputs(ctx, want, '%s, flags %d' % (env, flags))
            assert_state_is_the_references(ctx, o, 'kind %d, %s, flags %d' % (kind, env, flags))
        for name in env:
            monkeypatch.delenv(name)


# ---- 2. families R and Z ----------------------------------------------------------------------------------------------------------------
def _rz(family, av_window):
    return host.family_r(av_window) if family == 'R' else host.family_z(av_window)


@pytest.mark.parametrize('av_window', [256, 2000])
@pytest.mark.parametrize('family', ['R', 'Z'])
def test_three_pushes_and_a_restored_context(family, av_window):
    # after each push ss is the reference's _sum -- for R with its residue, which fsum of the ring does not give (asserted on the host side);
    # the context restored from push 2's blob carries it on: nfc_set_state hands ss over and the next batch's preparation takes delta from it
    routes = push_all(_rz(family, av_window), 0, restore_at=1)
    # R replays one prefix; Z none at all: its zeros are multiples of every power of two, its sums provably exact (push_all holds the route to that)
    assert (routes[0]['samples'] > 0) == (family == 'R')


@pytest.mark.parametrize('family', ['R', 'Z'])
def test_three_pushes_through_the_multi_launch_stages(monkeypatch, family):
    push_all(_rz(family, 256), 0, monkeypatch, no_small=True)


def test_a_short_first_push_goes_sequential_as_a_whole():
    # fewer than four spans in the batch: the `left <= 4 * span` exit.  Family R's capture: family Z's needs no sequential span at all
    b = host.family_r(256, short=True)
    routes = push_all(b, 0)
    assert routes[0] == dict(attempts=1, spans=1, samples=b.cuts[1], exit=3), routes[0]


@pytest.mark.parametrize('depth', [1, 3])
@pytest.mark.parametrize('av_window', [256, 2000])
@pytest.mark.parametrize('family', ['R', 'Z'])
def test_three_batches_submitted_ahead(monkeypatch, family, av_window, depth):
    # depth 3: all three in flight, the state behind the last; depth 1: the state behind every batch
    got, want = submit_all(_rz(family, av_window), 0, monkeypatch, depth=depth)
    assert got == want == 0, 'redone_total %d, the route asks for %d' % (got, want)


# ---- 2b. family A: the batch that ran ahead is repeated ---------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [1, 3])
def test_a_batch_that_ran_ahead_and_brings_wide_range_is_repeated(monkeypatch, depth):
    # push 3 runs ahead (pushes 1 and 2 are flat: no sequential span; a stream's first two batches never run ahead), its level rises by 2^22: nfc_wait finds its sums not provably exact and
    # processes it again synchronously from the state before it -- redone_total grows by one (asserted batch by batch in submit_all),
    # sequential spans are taken, and outputs and state (depth 1: after every batch) are the reference's.  Push 4 waits for it.
    b = host.family_a()
    got, want = submit_all(b, 0, monkeypatch, depth=depth, meets_range=lambda k: k == 2)
    assert got == want == 1, 'redone_total %d, the route asks for %d' % (got, want)


def test_family_a_pushed_synchronously():
    b = host.family_a()
    routes = push_all(b, len(b.x), cap=False)   # (no odd VALUE anywhere: nothing for t_clear; the route is read, not capped)
    assert routes[0]['samples'] == 0 and routes[1]['samples'] == 0 and routes[2]['samples'] > 0, routes


@pytest.mark.parametrize('av_window', [256, 2000])
@pytest.mark.parametrize('family', ['R', 'Z'])
def test_stream_1_of_three_in_a_multi_context(family, av_window):
    # k_multi's literal loop: the state against the oracle directly, not by way of an nfc_ctx
    b = _rz(family, av_window)
    beside = [host.family_z(av_window) if family == 'R' else host.family_r(av_window), host.family_r(av_window)]
    o = co.COracle(trace=True, **b.params)
    marks = Marks(o)
    with api.NfcMultiContext(3, max(e - a for a, e in zip(b.cuts[:-1], b.cuts[1:])), input_kind=ENV, **b.params) as m:
        for k, (a, e) in enumerate(zip(b.cuts[:-1], b.cuts[1:])):
            m.push([beside[0].x[a:e], b.x[a:e], beside[1].x[a:e][:(e - a) // 2]])
            o.push_env(b.x[a:e])
            assert_outputs(m.stream(1), marks.take(), 'multi, push %d' % k)
            assert_state_is_the_references(m.stream(1), o, 'multi, push %d' % k)


# ---- 3. family P ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('J', host.P_JS)
def test_family_p(J):
    b = host.family_p(J)
    r = push_all(b, 0)[0]
    assert r['samples'] > 0   # (push_all: used_sequential == 1 with it)
    span = host.span_of(256)
    if J in (9, 17):
        assert r['samples'] >= {9: 2, 17: 3}[J] * span and r['exit'] == 0, r
    if J == 60:
        assert r == dict(attempts=7, spans=7, samples=b.cuts[1], exit=2), r


# ---- 4. family M ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('place', sorted(host.M_PLACES))
def test_family_m(place):
    b = host.family_m(place)
    routes = push_all(b, b.at)
    assert routes[b.push_of_burst]['samples'] > 0, 'the push that meets the burst'
    if place == 'end_of_push_1':
        assert routes[1]['samples'] > 0, 'the push that starts with odd values in the carried ring'


@pytest.mark.parametrize('place', sorted(host.M_PLACES))
def test_family_m_submitted_ahead(monkeypatch, place):
    b = host.family_m(place)
    # A batch that ran ahead and met the burst would be repeated synchronously (redone_total + 1).  At a lo_val that lets the burst be
    # accepted no batch runs ahead: each is the sequential kernel's (never_provable), and behind such a batch the next one waits for it.
    # So every batch is processed inside its nfc_wait, none is repeated, and outputs and state are the reference's
    got, want = submit_all(b, b.at, monkeypatch, depth=1)
    assert got == want == 0, 'redone_total %d, the route asks for %d' % (got, want)


# ---- 5. a primed window -----------------------------------------------------------------------------------------------------------------
def test_primed_window_then_an_overlap():
    # nfc_prime leaves the window full of `level`, its exact sum, idle state machines and _dur = 1.  The oracle reaches that state through its
    # public calls when it is pushed av_window samples of `level` and av_window % max_len == 1 (transition_sink.py:123 sets _dur to that
    # remainder): max_len 51 with av_window 256.  Then the same overlap into both, from family R's capture.
    b = host.family_r(256)
    params = dict(b.params, max_len=51)
    level = np.float32(0.3)
    o = co.COracle(trace=True, **params)
    o.push_env(np.full(256, level, np.float32))
    marks = Marks(o)
    marks.take()
    with api.NfcContext(input_kind=ENV, **params) as ctx:
        ctx.prime(256, float(level))
        assert_state_is_the_references(ctx, o, 'primed')
        for k, (a, e) in enumerate(zip(b.cuts[:-1], b.cuts[1:])):
            ctx.push(b.x[a:e])
            o.push_env(b.x[a:e])
            assert_outputs(ctx, marks.take(), 'primed, push %d' % k)
            assert_state_is_the_references(ctx, o, 'primed, push %d' % k)
