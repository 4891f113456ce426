"""The window fill off the head of a batch (csrc/host_threshold.h: threshold_span; threshold.hip.h: fill_rider).

A stream that nfc_reset has just started, and whose first batch holds a whole window, no longer launches k_fill in front of pass 0:
k_threshold_wg starts at once -- its chunk 0 takes the window from the batch's first av_window samples and sums it itself, every other
chunk runs with delta = 0 by value -- and k_fill's work rides as one workgroup of the edge stage's reduce pass, the first launch behind
pass 0.  Every other batch keeps k_fill in front.

Every case runs on the test build with NFC_NO_SMALL=1 (the multi-launch edge stage whatever the length), is compared with the C oracle
on edges, symbols and packets, and ASSERTS WHICH ORDER ITS BATCHES TOOK from the test build's counters (nfc_debug_fill_order: batches
whose fill rode behind pass 0, and how many of those were repeated with k_fill in front), so no case passes by falling back.  Where a
case has more than one push, the get_state blob behind every push equals the blob of the same pushes on a context that is forced to
the old order (NFC_FILL_FRONT=1).

av_window = 500: k_threshold_wg needs a window of at least one round (1 024 samples: nfc_create, wg_ok), so pass 0 of such a stream is
k_threshold_lean and the batch keeps k_fill in front.  The cases stay, compared with the oracle like the others, and assert THAT.  The
capacity repeat is therefore taken at av_window = 2 000 (the max_len = 1 flicker of tests/test_small_stage.py, generated the same way)."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests.golden_util import Case as GoldenCase
from usrp_nfc_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

IQ, ENV, PCM, SC8 = api.NFC_IN_IQ_F32, api.NFC_IN_ENV_F32, api.NFC_IN_I16_SQ, api.NFC_IN_IQ_I8
PER = {IQ: 2, ENV: 1, PCM: 1, SC8: 2}
PCM_SCALE = 32767.0 * 0.9   # (the carrier of the synthetic captures has amplitude 0.5)
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
        if isinstance(_cache[key], np.ndarray):
            _cache[key].setflags(write=False)
    return _cache[key]


def capture(name, n):
    return cached(('iq', name, n), lambda: synth.workload(name, n))


def as_kind(iq, kind):
    """The synthetic IQ as a caller of that input kind holds it."""
    if kind == IQ:
        return iq
    if kind == ENV:
        return synth.envelope_f32(iq)
    if kind == PCM:
        return np.clip(np.rint(np.sqrt(synth.envelope_f32(iq)) * np.float32(PCM_SCALE)), -32768, 32767).astype(np.int16)
    return synth.quantise_sc8(iq, 120.0)


def fill_order(ctx):
    """(batches whose window fill rode behind pass 0, those of them repeated with k_fill in front) of the context so far"""
    out = (C.c_uint32 * 2)()
    ctx.L.nfc_debug_fill_order.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    assert ctx.L.nfc_debug_fill_order(ctx.h, out) == 0
    return int(out[0]), int(out[1])


def oracle_of(x, kind, params):
    """The C oracle over the capture's envelope as the library converts that kind (api.host_envelope: the kernels' conversion, bit for bit)."""
    o = co.COracle(**params)
    o.push_env(np.ascontiguousarray(api.host_envelope(x, kind), np.float32))
    return dict(transitions=o.transitions(), sym0=o.symbols(0).tolist(), sym1=o.symbols(1).tolist(), packets=o.packets())


def run(monkeypatch, x, kind, params, cuts, front=False, start='reset', chunk_samples=0):
    """The pushes through one context of the test build: what the readers give, accumulated; per push the order counters, the stats and
    the state blob.  start: 'reset' (nfc_reset: the stream whose state rides with the batch's first launch), or a function of the context."""
    monkeypatch.setenv('NFC_NO_SMALL', '1')
    monkeypatch.setenv('NFC_FILL_FRONT', '1' if front else '0')
    per = PER[kind]
    tr, s0, s1, pk, rows = [], [], [], [], []
    with api.NfcContext(input_kind=kind, chunk_samples=chunk_samples, lib_path=_lib.hooks_path(), **params) as ctx:
        if start == 'reset':
            ctx.reset()
        else:
            start(ctx)
        for a, b in zip(cuts[:-1], cuts[1:]):
            ctx.push(x[a * per:b * per])
            tr += ctx.transitions()
            s0 += ctx.symbols(0).tolist()
            s1 += ctx.symbols(1).tolist()
            pk += ctx.packets()
            st = ctx.stats()
            rows.append(dict(order=fill_order(ctx), blob=ctx.state_blob(), rerun=int(st.chunks_rerun), seq=int(st.used_sequential),
                             passes=int(st.threshold_passes), allocs=int(st.device_allocs), chunks=int(st.n_chunks)))
    return dict(transitions=tr, sym0=s0, sym1=s1, packets=pk), rows


def assert_outputs(got, want):
    assert len(got['transitions']) == len(want['transitions'])
    assert got['transitions'] == want['transitions'], 'edges differ'
    assert got['sym0'] == want['sym0'] and got['sym1'] == want['sym1'], 'symbols differ'
    assert got['packets'] == want['packets'], 'packets differ'


def assert_blobs(rows, rows_front):
    for i, (a, b) in enumerate(zip(rows, rows_front)):
        assert b['order'] == (0, 0), 'NFC_FILL_FRONT=1 keeps k_fill in front'
        assert np.array_equal(a['blob'], b['blob']), 'the state behind push %d differs from the old order\'s at bytes %s' % (
            i, np.flatnonzero(a['blob'] != b['blob'])[:8] if len(a['blob']) == len(b['blob']) else 'lengths')


# ---- a fresh stream, the whole window in its first batch ------------------------------------------------------------------------------
# n: 2^18 + 1; 3e5 cut at an odd sample (the first push is the fresh one, the second continues the stream); a length that leaves the
# window's end inside a round of k_threshold_wg (2 000 = 1 024 + 976: chunk 0's first classified round is ragged at its head) AND the batch's
# end inside a step (ragged at the tail)
LENGTHS = {'2^18+1': [0, (1 << 18) + 1], '3e5_odd_cut': [0, 150001, 300000], 'ragged': [0, (1 << 18) + 1024 + 513]}


@pytest.mark.parametrize('kind', [IQ, ENV, PCM, SC8], ids=['fc32', 'env', 'pcm16', 'sc8'])
@pytest.mark.parametrize('length', sorted(LENGTHS))
@pytest.mark.parametrize('av_window', [2000, 500])
def test_fresh_stream_with_a_whole_window_in_its_first_batch(monkeypatch, kind, length, av_window):
    cuts = LENGTHS[length]
    x = as_kind(capture('all', cuts[-1]), kind)
    params = dict(hi_val=1.1, av_window=av_window)
    want = cached(('oracle', 'all', cuts[-1], kind, av_window), lambda: oracle_of(x, kind, params))
    got, rows = run(monkeypatch, x, kind, params, cuts)
    assert_outputs(got, want)
    assert len(got['packets']) > 20 and rows[0]['chunks'] >= 2
    # the first batch on the new order where pass 0 is k_threshold_wg (the module's docstring: not at av_window 500); never repeated, and
    # a continuing stream's batch never rides
    assert [r['order'] for r in rows] == [(1, 0) if av_window >= 1024 else (0, 0)] * len(rows)
    _, rows_front = run(monkeypatch, x, kind, params, cuts, front=True)
    assert_blobs(rows, rows_front)


def test_fresh_stream_cut_into_many_chunks(monkeypatch):
    # a configured chunk length of eight rounds: 33 workgroups in pass 0, chunk 0 one of many
    n = (1 << 18) + 1
    x = capture('all', n)
    params = dict(hi_val=1.1)
    want = cached(('oracle', 'all', n, IQ, 2000), lambda: oracle_of(x, IQ, params))
    got, rows = run(monkeypatch, x, IQ, params, [0, n], chunk_samples=8192)
    assert_outputs(got, want)
    assert rows[0]['order'] == (1, 0) and rows[0]['chunks'] == 33


# ---- a window whose sum is not provably independent of the order ------------------------------------------------------------------------
def test_window_not_provably_exact(monkeypatch):
    # the samples of fx_stress_dynrange (a float32 envelope whose first window spans more exponents than 52 bits hold) as the stream's
    # first window, ordinary traffic behind them: chunk 0 gives up on its own window, and where the reference's order gives another sum
    # than the parallel one the batch is repeated with k_fill in front -- the `inexact` path from there on is the old order's
    g = GoldenCase('fx_stress_dynrange')
    assert g.params['av_window'] == 2000 and len(g.x) > 2000
    x = np.concatenate([g.x, synth.envelope_f32(capture('all', 1 << 18))])
    want = oracle_of(x, ENV, g.params)
    got, rows = run(monkeypatch, x, ENV, g.params, [0, len(x)])
    assert_outputs(got, want)
    got_f, rows_front = run(monkeypatch, x, ENV, g.params, [0, len(x)], front=True)
    assert_outputs(got_f, want)
    assert rows[0]['order'][0] == 1, 'the batch started on the new order'
    assert rows[0]['order'][1] == 1 or rows[0]['rerun'] >= 1, 'chunk 0 gave up on its window (re-run from the carried state), or the batch was repeated'
    assert rows[0]['seq'] == rows_front[0]['seq'], 'the sequential replay is taken exactly where the old order takes it'
    assert_blobs(rows, rows_front)   # (the blob's header carries the sum as the reference's order left it)


# ---- batches that keep k_fill in front -----------------------------------------------------------------------------------------------------
def _primed(ctx):
    ctx.prime(1_000_000, 0.25)


def test_primed_stream_keeps_the_old_order(monkeypatch):
    n = (1 << 18) + 1
    x = capture('all', n)
    params = dict(hi_val=1.1)
    got, rows = run(monkeypatch, x, IQ, params, [0, n], start=_primed)
    assert rows[0]['order'] == (0, 0)
    _, rows_front = run(monkeypatch, x, IQ, params, [0, n], start=_primed, front=True)
    assert_blobs(rows, rows_front)
    assert len(got['packets']) > 20


def test_restored_state_keeps_the_old_order(monkeypatch):
    n = (1 << 18) + 1
    x = capture('all', 2 * n)
    params = dict(hi_val=1.1)
    want = cached(('oracle', 'all', 2 * n, IQ, 2000), lambda: oracle_of(x, IQ, params))
    first, rows1 = run(monkeypatch, x, IQ, params, [0, n])
    blob = rows1[0]['blob']
    rest, rows2 = run(monkeypatch, x[2 * n:], IQ, params, [0, n], start=lambda ctx: ctx.set_state_blob(blob))
    assert rows1[0]['order'] == (1, 0) and rows2[0]['order'] == (0, 0)
    assert_outputs({k: first[k] + rest[k] for k in first}, want)


def test_window_that_fills_across_two_pushes_keeps_the_old_order(monkeypatch):
    n = (1 << 18) + 1
    x = capture('all', n)
    params = dict(hi_val=1.1)
    want = cached(('oracle', 'all', n, IQ, 2000), lambda: oracle_of(x, IQ, params))
    got, rows = run(monkeypatch, x, IQ, params, [0, 1203, n])
    assert_outputs(got, want)
    assert [r['order'] for r in rows] == [(0, 0), (0, 0)]


# ---- the batches behind the fresh one -------------------------------------------------------------------------------------------------------
def test_second_and_third_batch_of_the_stream(monkeypatch):
    # three pushes, the state behind each against the old order's; the stress capture's level step (at sample 1e6) makes chunks of the
    # second push fail their certification: re-runs, and the end-of-batch state finalized a second time
    n = 2_000_000
    x = cached(('stress', n), lambda: synth.stress_workload(n))
    cuts = [0, 700_001, 1_400_000, n]
    params = dict(hi_val=1.1)
    want = cached(('oracle', 'stress', n), lambda: oracle_of(x, IQ, params))
    got, rows = run(monkeypatch, x, IQ, params, cuts)
    assert_outputs(got, want)
    assert [r['order'] for r in rows] == [(1, 0)] * 3, 'the first batch rode, the continuing ones never do'
    assert rows[1]['rerun'] >= 1 and rows[1]['passes'] >= 2, 'a certification failed in the second push: its state was finalized twice'
    _, rows_front = run(monkeypatch, x, IQ, params, cuts, front=True)
    assert_blobs(rows, rows_front)


# ---- a capacity repeat of the edge stage on the new order ----------------------------------------------------------------------------------
def test_capacity_repeat_on_the_new_order(monkeypatch):
    # max_len = 1 and three levels drawn per sample: an entry per sample, far beyond the first estimate AND the allocation -- the
    # edge stage is repeated (the buffers grow), and its reduce pass runs again without the rider
    LOW, MID, HIGH = np.float32(0.01), np.float32(0.25), np.float32(0.25 * 1.3)
    n = (1 << 18) + 4097
    x = np.full(n, MID, np.float32)
    x[3000:n - 29000] = np.array([LOW, MID, HIGH], np.float32)[np.random.default_rng(5).integers(0, 3, n - 32000)]
    params = dict(hi_val=1.1, av_window=2000, max_len=1)
    want = oracle_of(x, ENV, params)
    assert len(want['transitions']) > n // 2
    got, rows = run(monkeypatch, x, ENV, params, [0, n])
    assert_outputs(got, want)
    assert rows[0]['order'][0] == 1
    assert rows[0]['allocs'] > 0, 'entries beyond the allocation: the repeat grew the buffers'
    _, rows_front = run(monkeypatch, x, ENV, params, [0, n], front=True)
    assert_blobs(rows, rows_front)
