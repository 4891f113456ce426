"""The edge stage's reduce pass hands the writer its threads' prefixes (edges.hip.h: EdgeRec): with the record
(NFC_EDGE_PREFIX=1: what the product runs for a batch processed on its own) and with the writer's own block scans
(NFC_EDGE_PREFIX=0: what it runs for a batch that ran ahead) the stage must leave what the C oracle leaves -- edges,
both symbol streams, packets and counts, exactly.

Batches here exceed 2^18 samples (shorter ones take the one-launch kernel); a tile is 32 768 samples, a super 131 072."""
import numpy as np
import pytest

from oracle import c_oracle as co
from usrp_nfc_amd import api, synth

pytestmark = pytest.mark.gpu

TILE, SUPER = 32_768, 131_072
ENV, IQ = api.NFC_IN_ENV_F32, api.NFC_IN_IQ_F32
BOTH = pytest.mark.parametrize('edge_prefix', ['0', '1'])

_ORACLE = {}   # case -> what the oracle leaves for it (computed once, shared by both settings of the switch)


def _oracle(name, x, params, kind):
    if name not in _ORACLE:
        o = co.COracle(**params)
        (o.push_env if kind == ENV else o.push_iq)(x)
        types, lens, bits = o.packet_arrays()
        _ORACLE[name] = dict(edges=o.edges(), sym=[o.symbols(0), o.symbols(1)], packets=o.packets(),
                             n_packets=[int((types == t).sum()) for t in (0, 1)], n_bits=[int(lens[types == t].sum()) for t in (0, 1)])
        o.close()
    return _ORACLE[name]


class _Got(object):
    """What the pushes of one stream produced, concatenated; the counts summed."""

    def __init__(self):
        self.edges, self.sym, self.packets = [], [[], []], []
        self.n = dict(samples=0, edges=0, sym=[0, 0], packets=[0, 0], bits=[0, 0])

    def take(self, ctx):
        c = ctx.counts()
        self.edges.append(ctx.edges())
        for t in (0, 1):
            self.sym[t].append(ctx.symbols(t))
            self.n['sym'][t] += int(c.n_symbols[t])
            self.n['packets'][t] += int(c.n_packets[t])
            self.n['bits'][t] += int(c.n_packet_bits[t])
        self.packets += ctx.packets()
        self.n['samples'] += int(c.n_samples)
        self.n['edges'] += int(c.n_edges)


def _compare(got, ref, n_samples):
    e = np.concatenate(got.edges) if got.edges else np.zeros(0, ref['edges'].dtype)
    r = ref['edges']
    assert len(e) == len(r), 'edges: %d, the oracle has %d' % (len(e), len(r))
    for f in ('idx', 'd', 'v', 't'):
        bad = np.flatnonzero(e[f] != r[f])
        assert not len(bad), 'edge %d of %d: %s is %s, the oracle has %s' % (bad[0], len(r), f, e[f][bad[0]], r[f][bad[0]])
    for t in (0, 1):
        s = np.concatenate(got.sym[t]) if got.sym[t] else np.zeros(0, np.uint8)
        assert len(s) == len(ref['sym'][t]) and (s == ref['sym'][t]).all(), 'symbols of type %d differ' % t
    assert got.packets == ref['packets']
    assert got.n['samples'] == n_samples and got.n['edges'] == len(r)
    assert got.n['sym'] == [len(ref['sym'][0]), len(ref['sym'][1])]
    assert got.n['packets'] == ref['n_packets'] and got.n['bits'] == ref['n_bits']


def _check(name, x, params, kind, pushes=None):
    per = 2 if kind == IQ else 1
    n = len(x) // per
    ref = _oracle(name, x, params, kind)
    cuts = [0, n] if pushes is None else pushes
    got = _Got()
    with api.NfcContext(input_kind=kind, **params) as ctx:
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert b - a > 1 << 18   # (the multi-launch edge stage)
            ctx.push(x[a * per:b * per])
            got.take(ctx)
    _compare(got, ref, n)
    return ref


_CAPTURES = {}


def _capture(name, make):
    if name not in _CAPTURES:
        _CAPTURES[name] = make()
    return _CAPTURES[name]


def _case1():
    return synth.workload('all', 400_037)   # three supers and a bit: a short last tile, a partial last word, tiles that begin in a frame gap


def _idle(n, seed):
    rng = np.random.default_rng(seed)
    return (0.25 * (1 + 0.002 * rng.standard_normal(n))).astype(np.float32)


LOW, HIGH = np.float32(1e-6), np.float32(0.25 * 1.3)


def _burst(x, at, k, rng):
    """k samples of frame-like content: pauses of 5 samples and loaded stretches of 9, a few samples apart."""
    p = at
    while p < at + k:
        ln, lvl = (5, LOW) if rng.integers(0, 2) else (9, HIGH)
        x[p:p + ln] = lvl
        p += ln + int(rng.integers(4, 30))


@BOTH
def test_workload_short_last_tile(monkeypatch, edge_prefix):
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)
    iq = _capture('case1', _case1)
    ref = _check('case1', iq, dict(samp_rate=2e6, hi_val=1.1), IQ)
    assert len(ref['edges']) > 5000 and len(ref['packets']) > 10


@BOTH
def test_idle_carrier_between_frames(monkeypatch, edge_prefix):
    # whole tiles without a change: the time-outs of one idle run are counted across tile joins and across a super join
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)

    def make():
        period = synth.modulation_profile(synth.txn_frames(), rate_msps=2.0, lead_in=0, tail=0)
        assert len(period) < 40_000
        n = 300_000
        m = np.ones(n, np.float32)
        starts = [3000, SUPER + 3000]
        assert 3000 + len(period) < SUPER - 70_000   # the first gap: >= 70 000 idle samples, over three tile joins and sample 131 072
        starts.append(starts[1] + len(period) + 70_500)
        for s in starts:
            k = min(len(period), n - s)
            m[s:s + k] = period[:k]
        return synth.iq_from_profile(m, seed=21)

    ref = _check('idle_gaps', _capture('idle_gaps', make), dict(samp_rate=2e6, hi_val=1.1), IQ)
    assert len(ref['edges']) > 300_000 // 50 - 2000   # (the idle carrier's heart-beats)


@BOTH
def test_losses_of_signal_across_tile_and_super_joins(monkeypatch, edge_prefix):
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)

    def make():
        rng = np.random.default_rng(31)
        x = _idle(300_000, 31)
        for k in range(1, 9):   # LOW runs of 400 samples (eight time-outs) across every tile join, k = 4: the super join
            x[TILE * k - 200:TILE * k + 200] = LOW
            x[TILE * k + 200:TILE * k + 204] = HIGH
        x[SUPER * 2 - 399:SUPER * 2 + 1] = LOW   # ... and one that ends on the super's first sample
        for at in (10_000, 70_000, 140_000, 250_000):
            _burst(x, at, 3000, rng)
        return x

    _check('los', _capture('los', make), dict(samp_rate=2e6, hi_val=1.1), ENV)


@BOTH
@pytest.mark.parametrize('max_len', [20, 50])
def test_max_len_short_and_default(monkeypatch, edge_prefix, max_len):
    # max_len 20: a word's own time-outs are counted by walking its runs (word_agg); 50: by the stretches without a change
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)
    iq = _capture('all_300001', lambda: synth.workload('all', 300_001))
    _check('max_len_%d' % max_len, iq, dict(samp_rate=2e6, hi_val=1.1, max_len=max_len), IQ)


@BOTH
def test_max_len_250_long_window(monkeypatch, edge_prefix):
    # max_len >= 63: no time-out inside a word; a 10 000-sample window at 10 Msps (eight rows per step in the threshold kernel).
    # The smallest capture that fills the window and leaves two supers.
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)
    window, n = 10_000, 10_000 + 2 * SUPER

    def make():
        period = synth.modulation_profile(synth.txn_frames(), rate_msps=10.0, lead_in=0, tail=0)
        return synth.iq_from_profile(synth.tiled_profile(period, n, lead_in=window + 700), seed=11)

    _check('max_len_250', _capture('max_len_250', make), dict(samp_rate=1e7, hi_val=1.1, av_window=window, max_len=250), IQ)


def _two_push_stream():
    rng = np.random.default_rng(51)
    n = 2 * 270_000
    x = _idle(n, 51)
    for at in range(5000, n - 4000, 47_000):
        _burst(x, at, 2500, rng)
    return x


@BOTH
@pytest.mark.parametrize('cut', ['idle', 'low'])
def test_two_pushes_carry_the_run(monkeypatch, edge_prefix, cut):
    # the second push starts inside an idle run / inside a LOW run: dur_in, last_bit_in and state_in come carried, and the
    # time-outs of the carried run are counted from where it began
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)

    def make():
        x = _two_push_stream().copy()
        if cut == 'low':
            x[270_000 - 180:270_000 + 220] = LOW
            x[270_000 + 220:270_000 + 223] = HIGH
        else:
            x[270_000 - 3000:270_000 + 3000] = np.float32(0.25)
        return x

    x = _capture('two_push_' + cut, make)
    _check('two_push_' + cut, x, dict(samp_rate=2e6, hi_val=1.1), ENV, pushes=[0, 270_000, len(x)])


@BOTH
def test_first_stable_sample_inside_tile_0(monkeypatch, edge_prefix):
    # a fresh stream: the samples before the window has filled (skip) produce nothing, the first stable one lies inside tile 0
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)

    def make():
        rng = np.random.default_rng(52)
        x = _idle(270_000, 52)
        _burst(x, 4000, 3000, rng)   # over the first stable sample (5000)
        _burst(x, 100_000, 3000, rng)
        return x

    _check('skip_in_tile_0', _capture('skip_in_tile_0', make), dict(samp_rate=2e6, hi_val=1.1, av_window=5000), ENV)


@BOTH
def test_every_tile_walks_twice(monkeypatch, edge_prefix):
    # an idle carrier with max_len 8: 4 096 heart-beats per tile, more than the writer stages in one round
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)
    x = _capture('heart_beats', lambda: _idle(270_000, 61))
    ref = _check('heart_beats', x, dict(samp_rate=2e6, hi_val=1.1, max_len=8), ENV)
    assert len(ref['edges']) >= (270_000 - 2000) // 8 - 1


@BOTH
def test_workload_behind_the_prefix_launch(monkeypatch, edge_prefix):
    # more tiles than a workgroup folds itself: the single-workgroup prefix launch over the supers' aggregates
    monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)
    monkeypatch.setenv('NFC_OWN_PREFIX_MAX', '2')
    _check('case1', _capture('case1', _case1), dict(samp_rate=2e6, hi_val=1.1), IQ)


@pytest.mark.parametrize('edge_prefix', ['0', '1', None])
def test_batches_submitted_ahead_share_the_record_buffer(monkeypatch, edge_prefix):
    # three batches in flight, four rounds: the edge stages of consecutive batches run one after the other on the main stream, so
    # one record buffer serves them all -- every round must leave the single stream's outputs.  (None: the product library and its
    # own rule -- the record for the batches that do not run ahead, the scans for those that do.)
    if edge_prefix is not None:
        monkeypatch.setenv('NFC_EDGE_PREFIX', edge_prefix)
    part = _capture('case1', _case1)
    n1 = len(part) // 2
    iq = _capture('case1_x3', lambda: np.concatenate([part, part, part]))
    ref = _oracle('case1_x3', iq, dict(samp_rate=2e6, hi_val=1.1), IQ)
    buf = api.DeviceBuffer(part)
    with api.NfcContext(input_kind=IQ, samp_rate=2e6, hi_val=1.1) as ctx:
        for _ in range(4):
            ctx.reset()
            got = _Got()
            for _ in range(3):
                ctx.submit_device(buf, n1)
            assert ctx.submitted() == 3
            for _ in range(3):
                ctx.wait()
                got.take(ctx)
            assert ctx.submitted() == 0
            _compare(got, ref, 3 * n1)
    buf.free()
