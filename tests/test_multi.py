"""The multi-stream context: nfc_multi (include/nfc_amd.h), api.NfcMultiContext, decoder.decode_many.

K independent streams with one parameter set are decoded in ONE kernel launch per push, a GPU lane per stream (csrc/multi.hip.h).
The contract is parity with the single stream: stream k's outputs and state are an NfcContext's for the same samples, which is in
turn pinned to the reference.  So the expected values here are the UNMODIFIED reference's arrays stored in tests/golden/fx_*.npz,
the pinned C oracle on seeded inputs, and -- for the state interchange -- an NfcContext.  Every comparison is bit for bit; every
stream's flags must be 0 with the default capacities."""
import ctypes as C
import io
import os
import re
import subprocess
import wave

import numpy as np
import pytest

from oracle import c_oracle as co
from tests.golden_util import Case, load_npz
from usrp_nfc_amd import _lib, api, build, decoder as dec, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI_SYMBOLS = ['nfc_multi_create', 'nfc_multi_destroy', 'nfc_multi_last_error', 'nfc_multi_push_device', 'nfc_multi_push',
                 'nfc_multi_get_counts', 'nfc_multi_read_edges', 'nfc_multi_read_symbols', 'nfc_multi_read_packets',
                 'nfc_multi_read_packet_bits', 'nfc_multi_get_state', 'nfc_multi_set_state', 'nfc_multi_reset', 'nfc_multi_get_stats',
                 'nfc_multi_set_timing']
FLAGS = dict(NFC_MULTI_TRUNC_EDGES=1, NFC_MULTI_TRUNC_SYMBOLS=2, NFC_MULTI_TRUNC_PACKETS=4, NFC_MULTI_TRUNC_BITS=8,
             NFC_MULTI_PENDING_OVERFLOW=16)
PER = {api.NFC_IN_IQ_F32: 2, api.NFC_IN_ENV_F32: 1, api.NFC_IN_REAL_F32_SQ: 1, api.NFC_IN_I16_SQ: 1, api.NFC_IN_IQ_I16: 2,
       api.NFC_IN_IQ_I8: 2, api.NFC_IN_IQ_U8: 2}


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_header_and_binding(tmp_path):
    h = open(os.path.join(ROOT, 'include', 'nfc_amd.h')).read()
    # the section's fifteen functions (with its two structure types, seventeen new names): every one declared in the header and
    # bound in _lib, the ABI version untouched
    assert set(MULTI_SYMBOLS) <= set(_lib.SYMBOLS)
    for s in MULTI_SYMBOLS:
        assert re.search(r'\b%s\(' % s, h), s
    assert re.search(r'#define NFC_AMD_ABI_VERSION 4\b', h) and _lib.ABI_VERSION == 4
    for name, v in FLAGS.items():
        m = re.search(r'\b%s\s*=\s*(\d+)' % name, h)
        assert m and int(m.group(1)) == getattr(_lib, name) == getattr(api, name) == v, name
        assert name in api.__all__
    assert 'NfcMultiContext' in api.__all__
    # sizeof by the C compiler against the ctypes mirrors
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "nfc_amd.h"\nint main(void) { printf("%zu %zu\\n", sizeof(nfc_multi_config), '
                   'sizeof(nfc_multi_stats)); return 0; }\n')
    exe = str(tmp_path / 'sz')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', exe])
    a, b = (int(v) for v in subprocess.check_output([exe]).split())
    assert a == 64 == C.sizeof(_lib.MultiConfig)
    assert b == C.sizeof(_lib.MultiStats)


@pytest.mark.parametrize('kw, name', [
    (dict(flags=1), 'flags'),
    (dict(chunk_samples=4096), 'chunk_samples'),
    (dict(n_streams=0), 'n_streams'),
    (dict(n_streams=65537), 'n_streams'),
    (dict(max_push_samples=0), 'max_push_samples'),
    (dict(max_push_samples=(1 << 24) + 1), 'max_push_samples'),
    (dict(_reserved=1), 'reserved'),
    # a capacity whose row stride (uint32 entries) could wrap: bounded at 2^26 entries
    (dict(cap_edges=(1 << 26) + 1), 'cap_edges'),
    (dict(cap_symbols=0xFFFFFFF0), 'cap_symbols'),
    (dict(cap_packets=0xFFFFFFFF), 'cap_packets'),
    (dict(cap_packet_bits=1 << 31), 'cap_packet_bits'),
    (dict(cap_pending_bits=0xFFFFFFF0), 'cap_pending_bits'),
])
def test_rejected_arguments_name_the_argument(kw, name):
    # checked before the device is touched: the same message with and without a GPU
    args = dict(n_streams=4, max_push_samples=1000)
    args.update(kw)
    with pytest.raises(api.NfcError) as e:
        api.NfcMultiContext(**args)
    assert name in str(e.value) and 'status -1' in str(e.value)


def test_decode_many_refuses_mixed_kinds():
    with pytest.raises(ValueError):
        dec.decode_many([np.zeros(64, np.complex64), np.zeros(64, np.int16)])


@pytest.mark.skipif(os.path.exists('/dev/kfd'), reason='a GPU is present: create succeeds')
def test_create_fails_loudly_without_a_gpu():
    with pytest.raises(api.NfcError) as e:
        api.NfcMultiContext(4, 1000)
    assert 'no CPU fallback' in str(e.value)


def test_multi_translation_unit_isa(tmp_path):
    # csrc/nfc_multi.hip compiled for gfx950 as the product is: one kernel per input kind, none with scratch (the decoder LUTs are
    # in global memory, a lane's state in named scalars).  The register counts are printed, not asserted: DESIGN.md records them.
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-shared')]
    asm = str(tmp_path / 'nfc_multi.s')
    subprocess.check_call([hipcc] + flags + ['-S', '--cuda-device-only', os.path.join(build.CSRC, 'nfc_multi.hip'), '-o', asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    for k in range(7):
        nm = '_ZN3nfc5multi7k_multiILi%dEEEvNS0_4ArgsE' % k
        body = re.search(r'^%s:(.*?)\.end_amdhsa_kernel' % nm, text, re.S | re.M)
        assert body, nm
        body = body.group(1)
        assert re.search(r'\.amdhsa_private_segment_fixed_size 0\b', body), nm
        assert 'scratch_' not in body, nm
        print('k_multi<%d>: %s VGPRs, %s SGPRs' % (k, re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1),
                                                   re.search(r'\.amdhsa_next_free_sgpr (\d+)', body).group(1)))
    assert 'nfc_multi.hip' in build.SOURCES and {'nfc_multi.hip', 'multi.hip.h'} <= set(build.DEPS)


# ---- GPU: helpers -----------------------------------------------------------------------------------------------------------

def first_diff(a, b):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i, a[i], b[i]
    return (n, None, None) if len(a) != len(b) else None


def state_key(st):
    h, ring, pend = st
    return bytes(h), ring.tobytes(), pend[0].tobytes(), pend[1].tobytes()


def empty_result():
    return dict(transitions=[], sym_tag=[], sym_reader=[], packets=[], edge_idx=[])


def collect(view, r):
    e = view.edges()
    r['edge_idx'] += e['idx'].tolist()
    r['transitions'] += [((int(v), int(d) * view.factor), int(t)) for v, d, t in zip(e['v'], e['d'], e['t'])]
    r['sym_tag'] += view.symbols(0).tolist()
    r['sym_reader'] += view.symbols(1).tolist()
    r['packets'] += view.packets()


def run_multi(arrays, kind, params, cuts=None, device_push=False, **ctx_kw):
    """arrays[k]: stream k's samples; cuts[k]: its cut positions [0, ..., n_k] (default: one push).  Round r hands stream k its
    piece r, or nothing once it has run out.  -> (results per stream, end states per stream)"""
    per = PER[kind]
    K = len(arrays)
    lens = [len(a) // per for a in arrays]
    cuts = cuts or [[0, n] for n in lens]
    piece = max([b - a for c in cuts for a, b in zip(c[:-1], c[1:])] + [1])
    res = [empty_result() for _ in range(K)]
    with api.NfcMultiContext(K, piece, input_kind=kind, **dict(params, **ctx_kw)) as m:
        for r in range(max(len(c) for c in cuts) - 1):
            parts = []
            for k in range(K):
                a, b = (cuts[k][r], cuts[k][r + 1]) if r + 1 < len(cuts[k]) else (0, 0)
                parts.append(arrays[k][a * per:b * per])
            if device_push:   # one buffer, ragged unaligned offsets: a sample of padding in front of every piece
                flat, first, at = [], [], 0
                for k, p in enumerate(parts):
                    pad = 1 + (k % 3)
                    flat += [np.zeros(pad * per, p.dtype), p]
                    first.append(at + pad)
                    at += pad + len(p) // per
                buf = api.DeviceBuffer(np.concatenate(flat))
                try:
                    m.push_device(buf, first, [len(p) // per for p in parts])
                finally:
                    buf.free()
            else:
                m.push(parts)
            assert int(m.stats().n_streams_truncated) == 0 and int(m.stats().n_launches) == 1
            for k in range(K):
                v = m.stream(k)
                assert v.flags() == 0, (k, v.flags())
                assert int(v.counts().n_samples) == len(parts[k]) // per
                if not len(parts[k]):
                    c = v.counts()
                    assert (int(c.n_edges), list(c.n_symbols), list(c.n_packets)) == (0, [0, 0], [0, 0]), k
                    continue
                collect(v, res[k])
        states = [state_key(m.stream(k).get_state()) for k in range(K)]
    return res, states


def check_case(c, r, label=''):
    d = first_diff(r['transitions'], c.transitions)
    assert d is None, '%s %s: transition %s' % (label, c.name, d)
    assert r['sym_tag'] == c.sym_tag.tolist(), (label, c.name)
    assert r['sym_reader'] == c.sym_reader.tolist(), (label, c.name)
    assert r['packets'] == c.packets, (label, c.name)
    assert r['edge_idx'] == sorted(r['edge_idx']) and (not r['edge_idx'] or r['edge_idx'][-1] < len(c.x))


ENV_GROUP = ['fx_empty', 'fx_short_1500', 'fx_short_2000', 'fx_short_2001', 'fx_low_run_timeout', 'fx_nonfinite_fill', 'fx_nonfinite_inf',
             'fx_nonfinite_nan', 'fx_stress_dropout', 'fx_stress_dynrange', 'fx_stress_hover', 'fx_stress_uniform', 'fx_stress_zero_start']


def fixture_groups():
    """[(label, kind, params, [(Case, samples)])]: the contexts of the issue's list."""
    env = api.NFC_IN_ENV_F32
    groups = []
    cs = [Case(n) for n in ENV_GROUP]
    assert all(c.params == cs[0].params for c in cs) and cs[0].params['hi_val'] == 1.1
    assert min(len(c.x) for c in cs) == 0 and max(len(c.x) for c in cs) == 29383
    groups.append(('env-1.1', env, cs[0].params, [(c, c.x) for c in cs]))
    cs = [Case('fx_reqa_atqa'), Case('fx_ultralight_txn')]
    assert cs[0].params == cs[1].params and cs[0].params['hi_val'] == 1.09
    groups.append(('env-1.09', env, cs[0].params, [(c, c.x) for c in cs]))
    c = Case('fx_ultralight_rec16')
    groups.append(('pcm16', api.NFC_IN_I16_SQ, c.params, [(c, load_npz('fx_ultralight_rec16.npz')['pcm'])] * 3))
    for name in ('fx_window500_max30', 'fx_rate4_defaults', 'fx_rate4_scaled', 'fx_txn_reader_only', 'fx_txn_tag_only'):
        c = Case(name)
        groups.append((name, env, c.params, [(c, c.x)] * 70))   # copies: more than one wave runs
    c = Case('fx_ultralight_txn')
    groups.append(('fc32', api.NFC_IN_IQ_F32, c.params, [(c, load_npz('fx_ultralight_iq.npz')['iq'])] * 2))
    for case in ('inf', 'nan'):
        c = Case('fx_nonfinite_iq:' + case, prefix=case + '_', file='fx_nonfinite_iq')
        groups.append(('fc32-' + case, api.NFC_IN_IQ_F32, c.params, [(c, load_npz('fx_nonfinite_iq.npz')[case + '_iq'])] * 2))
    for name, key, kind in (('sc16', 'iq16', api.NFC_IN_IQ_I16), ('sc8', 'iq8', api.NFC_IN_IQ_I8), ('cu8', 'iq8', api.NFC_IN_IQ_U8)):
        c = Case('fx_ultralight_' + name)
        groups.append((name, kind, c.params, [(c, load_npz('fx_ultralight_%s.npz' % name)[key])] * 2))
    return groups


GROUP_IDS = ['env-1.1', 'env-1.09', 'pcm16', 'fx_window500_max30', 'fx_rate4_defaults', 'fx_rate4_scaled', 'fx_txn_reader_only',
             'fx_txn_tag_only', 'fc32', 'fc32-inf', 'fc32-nan', 'sc16', 'sc8', 'cu8']


def group_of(label):
    g = [g for g in fixture_groups() if g[0] == label]
    assert len(g) == 1
    return g[0]


# ---- GPU: parity ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('label', GROUP_IDS)
def test_reference_fixtures_as_ragged_streams_of_one_push(label):
    _, kind, params, items = group_of(label)
    res, _ = run_multi([x for _, x in items], kind, params)
    for (c, _), r in zip(items, res):
        check_case(c, r, label)


def piecing(lens, how, rng):
    cuts = []
    for k, n in enumerate(lens):
        c = [0]
        r = 0
        while c[-1] < n:
            if how == 777:
                step = 777
            else:
                step = int(rng.integers(0, 4097))
                if (r + k) % 5 == 2:
                    step = 0   # this push gives the stream nothing
            c.append(min(n, c[-1] + step))
            r += 1
        cuts.append(c)
    return cuts


@pytest.mark.gpu
@pytest.mark.parametrize('how', [777, 'random'])
@pytest.mark.parametrize('label', GROUP_IDS)
def test_reference_fixtures_pushed_in_pieces(label, how):
    _, kind, params, items = group_of(label)
    rng = np.random.default_rng(4242 + GROUP_IDS.index(label))
    order = rng.permutation(len(items))   # stream order and neighbours must not matter
    items = [items[i] for i in order]
    arrays = [x for _, x in items]
    whole, end_whole = run_multi(arrays, kind, params)
    cuts = piecing([len(a) // PER[kind] for a in arrays], how, rng)
    res, end = run_multi(arrays, kind, params, cuts=cuts, device_push=(how == 'random'))
    for k, ((c, _), r) in enumerate(zip(items, res)):
        check_case(c, r, '%s/%s' % (label, how))
        assert r == whole[k]
        assert end[k] == end_whole[k], (label, how, k, c.name)


def oracle_iq(iq, params):
    o = co.COracle(**params)
    o.push_iq(iq)
    return o


@pytest.mark.gpu
def test_a_thousand_ragged_streams_against_the_c_oracle():
    K = 1000
    rng = np.random.default_rng(7)
    lens = rng.integers(1, 40001, K)
    assert (lens < 2000).sum() >= 3
    names = ['all', 'miller', 'manchester', 'stress']
    iqs = [synth.workload(names[k % 4], int(lens[k]), seed=1000 + k) for k in range(K)]
    # one device buffer, ragged offsets: an odd number of pad samples in front of every stream (fc32: 8-byte alignment, no more)
    pads = 1 + 2 * rng.integers(0, 4, K)
    first = np.cumsum(np.concatenate([[0], (lens + pads)[:-1]])) + pads
    flat = np.zeros(2 * int((lens + pads).sum()), np.float32)
    for k in range(K):
        flat[2 * first[k]:2 * (first[k] + lens[k])] = iqs[k]
    assert (first % 2 == 1).sum() > 100
    params = dict(samp_rate=2e6, hi_val=1.1)
    buf = api.DeviceBuffer(flat)
    try:
        with api.NfcMultiContext(K, 40000, input_kind=api.NFC_IN_IQ_F32, **params) as m:
            m.push_device(buf, first, lens)
            assert int(m.stats().n_streams_truncated) == 0 and int(m.stats().n_samples) == int(lens.sum())
            n_pk = 0
            for k in range(K):
                v = m.stream(k)
                assert v.flags() == 0, k
                o = oracle_iq(iqs[k], params)
                d = first_diff(v.transitions(), o.transitions())
                assert d is None, 'stream %d (%s, %d samples): transition %s' % (k, names[k % 4], lens[k], d)
                assert np.array_equal(v.edges()['idx'], o.edges()['idx'].astype(np.uint64)), k
                assert v.symbols(0).tolist() == o.symbols(0).tolist() and v.symbols(1).tolist() == o.symbols(1).tolist(), k
                pk = v.packets()
                assert pk == o.packets(), k
                n_pk += len(pk)
            assert n_pk > 2000
    finally:
        buf.free()


@pytest.mark.gpu
def test_the_largest_stream_count():
    K, n = 65536, 2500
    base = [synth.workload(nm, n + 64, seed=77 + i) for i, nm in enumerate(['all', 'miller', 'manchester', 'stress'])]
    flat = np.concatenate(base)
    per_base = n + 64
    # stream k: workload k % 4, shifted by (k // 4) % 64 samples -- overlapping ranges of one small buffer
    kk = np.arange(K)
    first = (kk % 4) * per_base + (kk // 4) % 64
    params = dict(samp_rate=2e6, hi_val=1.1)
    buf = api.DeviceBuffer(flat)
    try:
        with api.NfcMultiContext(K, n, input_kind=api.NFC_IN_IQ_F32, **params) as m:
            m.push_device(buf, first, np.full(K, n))
            st = m.stats()
            assert int(st.n_streams_truncated) == 0 and int(st.n_samples) == K * n and int(st.n_launches) == 1
            want = {}
            for k in range(4 * 64):   # every distinct stream once through the oracle
                o = oracle_iq(flat[2 * first[k]:2 * (first[k] + n)], params)
                want[(k % 4, (k // 4) % 64)] = (o, len(o.edges()), len(o.symbols(0)), len(o.symbols(1)), len(o.packets()))
            for k in range(K):
                c, f = m.stream(k)._counts()
                w = want[(k % 4, (k // 4) % 64)]
                assert f == 0 and (int(c.n_edges), int(c.n_symbols[0]), int(c.n_symbols[1]), int(c.n_packets[0] + c.n_packets[1])) == w[1:], k
            for k in np.random.default_rng(9).choice(K, 256, replace=False):
                v, o = m.stream(int(k)), want[(k % 4, (k // 4) % 64)][0]
                assert v.transitions() == o.transitions() and v.packets() == o.packets(), k
                assert v.symbols(0).tolist() == o.symbols(0).tolist() and v.symbols(1).tolist() == o.symbols(1).tolist(), k
    finally:
        buf.free()


def single_run(x, kind, params, cuts):
    per = PER[kind]
    out = []
    with api.NfcContext(input_kind=kind, **params) as ctx:
        for a, b in zip(cuts[:-1], cuts[1:]):
            ctx.push(x[a * per:b * per])
            r = empty_result()
            collect_ctx(ctx, r)
            out.append(r)
        return out, state_key(ctx.get_state())


def collect_ctx(ctx, r):
    e = ctx.edges()
    r['edge_idx'] += e['idx'].tolist()
    r['transitions'] += ctx.transitions()
    r['sym_tag'] += ctx.symbols(0).tolist()
    r['sym_reader'] += ctx.symbols(1).tolist()
    r['packets'] += ctx.packets()


@pytest.mark.gpu
def test_state_interchange_with_a_single_context():
    c = Case('fx_ultralight_txn')
    kind, params, x = api.NFC_IN_ENV_F32, c.params, c.x
    n = len(x)
    # a cut inside a frame: an open packet with pending bits, decoders mid-symbol
    (ref_a, ref_b), ref_end = single_run(x, kind, params, [0, n // 2, n])
    cut = None
    for cand in range(n // 2, n // 2 + 4000):
        with api.NfcContext(input_kind=kind, **params) as probe:
            probe.push(x[:cand])
            h = probe.get_state()[0]
            if h.n_pending_bits[0] + h.n_pending_bits[1] >= 3 and (h.pkt_started[0] or h.pkt_started[1]):
                cut = cand
                break
    assert cut is not None
    (ref_a, ref_b), ref_end = single_run(x, kind, params, [0, cut, n])
    # multi -> single
    with api.NfcMultiContext(3, n, input_kind=kind, **params) as m, api.NfcContext(input_kind=kind, **params) as ctx:
        m.push([x[:100], x[:cut], np.zeros(0, np.float32)])
        a = empty_result()
        collect(m.stream(1), a)
        assert a == ref_a
        st = m.stream(1).get_state()
        assert st[0].n_seen == cut and len(st[2][0]) + len(st[2][1]) >= 3
        ctx.set_state(*st)
        ctx.push(x[cut:])
        b = empty_result()
        collect_ctx(ctx, b)
        assert b == ref_b and state_key(ctx.get_state()) == ref_end
    # single -> multi, into a stream that has seen something else; its neighbours go on undisturbed
    with api.NfcMultiContext(3, n, input_kind=kind, **params) as m, api.NfcContext(input_kind=kind, **params) as ctx:
        ctx.push(x[:cut])
        m.push([x[:cut], x[:777], x[:cut]])
        m.stream(1).set_state(*ctx.get_state())
        assert state_key(m.stream(1).get_state()) == state_key(ctx.get_state())
        m.push([x[cut:], x[cut:], np.zeros(0, np.float32)])
        for k in (0, 1):
            b = empty_result()
            collect(m.stream(k), b)
            assert b == ref_b, k
            assert state_key(m.stream(k).get_state()) == ref_end, k
        # reset(k) touches stream k only
        before = state_key(m.stream(2).get_state())
        m.stream(0).reset()
        with api.NfcContext(input_kind=kind, **params) as fresh:
            assert state_key(m.stream(0).get_state()) == state_key(fresh.get_state())
        assert state_key(m.stream(2).get_state()) == before and state_key(m.stream(1).get_state()) == ref_end
        m.push([x, np.zeros(0, np.float32), x[cut:]])
        r0, r2 = empty_result(), empty_result()
        collect(m.stream(0), r0)
        collect(m.stream(2), r2)
        check_case(c, r0, 'after reset')
        assert r2 == ref_b and state_key(m.stream(2).get_state()) == ref_end


@pytest.mark.gpu
def test_capacity_semantics():
    cu, ct = Case('fx_stress_uniform'), Case('fx_ultralight_txn')
    params = dict(cu.params, hi_val=1.09)   # one parameter set for both: the expected values are the single context's
    kind = api.NFC_IN_ENV_F32
    xs = [cu.x, ct.x, ct.x[:3000], cu.x]   # (stream 2: a score of idle time-outs, nothing more)
    n = max(len(x) for x in xs)
    with api.NfcMultiContext(4, n, input_kind=kind, **params) as big:
        big.push(xs)
        full = []
        for k in range(4):
            assert big.stream(k).flags() == 0
            r = empty_result()
            collect(big.stream(k), r)
            r['counts'] = bytes(big.stream(k).counts())
            for t in (0, 1):
                r['pk%d' % t], r['bits%d' % t] = big.stream(k).packet_table(t), big.stream(k).packet_bits(t)
            full.append(r)
        states = [big.stream(k).get_state() for k in range(4)]
        end = [state_key(st) for st in states]
    assert len(full[0]['transitions']) > 64 and len(full[1]['transitions']) > 64 and len(full[1]['packets']) > 4
    assert len(full[2]['transitions']) <= 64 and not many_packets(full[2])   # the neighbour that fits
    # the longest an open packet of stream k ever gets: every open packet ends as a packet or as the pending bits of the end state
    longest = [max([int(v) for t in (0, 1) for v in full[k]['pk%d' % t]['n_bits']] + [len(p) for p in states[k][2]] + [0]) for k in range(4)]
    many = [many_packets(full[k]) for k in range(4)]
    assert longest[1] > 8 and many[1] and longest[2] <= 8 and not many[2]
    hooks = _lib.hooks_path()   # (the guard check is test support: in the test build only)

    def check_stored(m, k, pending_room):
        """edges cut at 64, packets at 2 per type; everything else whole.  pending_room: no open packet outgrew its room."""
        v = m.stream(k)
        f = v.flags()
        assert f == (api.NFC_MULTI_TRUNC_EDGES | (api.NFC_MULTI_TRUNC_PACKETS if many[k] else 0)
                     | (0 if pending_room else api.NFC_MULTI_PENDING_OVERFLOW)), (k, f)
        assert bytes(v.counts()) == full[k]['counts'], k   # the true totals
        with pytest.raises(api.NfcError) as e:
            v.edges()
        assert 'NFC_MULTI_TRUNC_EDGES' in str(e.value)
        got = v.transitions(allow_truncated=True)
        assert len(got) == 64 and got == full[k]['transitions'][:64]
        assert v.edges(allow_truncated=True)['idx'].tolist() == full[k]['edge_idx'][:64]
        wide = m.stream(k, allow_truncated=True)
        assert wide.symbols(0).tolist() == full[k]['sym_tag'] and wide.symbols(1).tolist() == full[k]['sym_reader']   # (default room)
        if many[k] or not pending_room:
            with pytest.raises(api.NfcError) as e:
                v.packets()
            assert ('NFC_MULTI_TRUNC_PACKETS' in str(e.value)) == many[k]
            assert ('NFC_MULTI_PENDING_OVERFLOW' in str(e.value)) == (not pending_room)
        # the carried state does not depend on what was stored: header and window exactly, whatever the slabs held
        if pending_room:
            for t in (0, 1):
                assert np.array_equal(v.packet_table(t, allow_truncated=True), full[k]['pk%d' % t][:2]), (k, t)   # the stored prefix
                assert np.array_equal(v.packet_bits(t, allow_truncated=True), full[k]['bits%d' % t]), (k, t)
            assert state_key(v.get_state()) == end[k], k
        else:
            h = _lib.StateHeader()
            m._chk(m.L.nfc_multi_get_state(m.h, k, C.byref(h), None, 0, None, 0), 'nfc_multi_get_state')
            ring = np.zeros(h.av_window, np.float32)
            m._chk(m.L.nfc_multi_get_state(m.h, k, C.byref(h), ring.ctypes.data, ring.size, None, 0), 'nfc_multi_get_state')
            assert (bytes(h), ring.tobytes()) == end[k][:2], k

    def check_neighbour(m):
        # stream 2, in the same wave as the cut ones: whole, no flag, its state exact
        v = m.stream(2)
        assert v.flags() == 0
        r = empty_result()
        collect(v, r)
        assert all(r[key] == full[2][key] for key in r)
        assert state_key(v.get_state()) == end[2]

    # (a) edges and packets cut, the open packets' room the default: the stored prefixes and the whole state, for every stream
    with api.NfcMultiContext(4, n, input_kind=kind, cap_edges=64, cap_packets=2, lib_path=hooks, **params) as m:
        guards = m.L.nfc_debug_multi_guards
        guards.argtypes = [C.c_void_p]
        assert guards(m.h) == 0
        m.push(xs)
        assert guards(m.h) == 0   # the words behind every stream's row of every slab
        assert int(m.stats().n_streams_truncated) == 3
        for k in (0, 1, 3):
            check_stored(m, k, True)
        check_neighbour(m)
    # (b) and 8 bits of room for an open packet
    with api.NfcMultiContext(4, n, input_kind=kind, cap_edges=64, cap_packets=2, cap_pending_bits=8, lib_path=hooks, **params) as m:
        guards = m.L.nfc_debug_multi_guards
        guards.argtypes = [C.c_void_p]
        assert guards(m.h) == 0
        m.push(xs)
        assert guards(m.h) == 0
        assert int(m.stats().n_streams_truncated) == 3
        for k in (0, 1, 3):
            check_stored(m, k, longest[k] <= 8)
        check_neighbour(m)
        # a pending overflow is sticky until the stream is reset, and the reset clears it
        m.push([np.zeros(0, np.float32)] * 4)
        assert m.stream(1).flags() == api.NFC_MULTI_PENDING_OVERFLOW
        m.reset(1)
        assert m.stream(1).flags() == 0
        m.push([np.zeros(0, np.float32), ct.x[:3000], np.zeros(0, np.float32), np.zeros(0, np.float32)])
        assert m.stream(1).flags() == 0 and guards(m.h) == 0
        assert m.stream(2).flags() == 0 and state_key(m.stream(2).get_state()) == end[2]


@pytest.mark.gpu
@pytest.mark.parametrize('window', [1, 8, 15, 16])
def test_windows_around_the_fetch_ahead_threshold(window):
    # k_multi fetches 8 window slots ahead of the walk only where the window has 16 or more; a shorter one is read in step.  70 ragged
    # streams (two waves) in two pushes against the C oracle, on both sides of the threshold and at the shortest window there is.
    K = 70
    rng = np.random.default_rng(100 + window)
    lens = rng.integers(1, 5001, K)
    lens[:3] = [1, window, window + 1]
    names = ['all', 'miller', 'manchester', 'stress']
    iqs = [synth.workload(names[k % 4], int(lens[k]), seed=500 + k) for k in range(K)]
    params = dict(samp_rate=2e6, hi_val=1.1, av_window=window)
    cuts = [[0, int(rng.integers(0, n + 1)), int(n)] for n in lens]
    # (a window this short follows the signal: entries can outnumber a quarter of the samples, so the slabs get room for all)
    caps = dict(cap_edges=5064, cap_symbols=10200, cap_packet_bits=10200, cap_packets=5064, cap_pending_bits=10200)   # (at most an entry per sample, two symbols per entry)
    res, end = run_multi(iqs, api.NFC_IN_IQ_F32, params, cuts=cuts, **caps)
    for k in range(K):
        o = oracle_iq(iqs[k], params)
        d = first_diff(res[k]['transitions'], o.transitions())
        assert d is None, 'window %d, stream %d (%d samples, cut at %d): transition %s' % (window, k, lens[k], cuts[k][1], d)
        assert res[k]['edge_idx'] == o.edges()['idx'].tolist(), k
        assert res[k]['sym_tag'] == o.symbols(0).tolist() and res[k]['sym_reader'] == o.symbols(1).tolist(), k
        assert res[k]['packets'] == o.packets(), k
    # and the state carried over the cut is the uncut run's
    whole, end_whole = run_multi(iqs, api.NFC_IN_IQ_F32, params, **caps)
    assert whole == res and end_whole == end


def many_packets(r):
    return max(len(r['pk0']), len(r['pk1'])) > 2


def write_wav(path, pcm, rate=2000000):
    w = wave.open(path, 'wb')
    try:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm, '<i2').tobytes())
    finally:
        w.close()


@pytest.mark.gpu
def test_decode_many(tmp_path):
    from usrp_nfc_amd import fsm
    iq = load_npz('fx_ultralight_iq.npz')['iq']
    gold = open(os.path.join(ROOT, 'tests', 'golden', 'ultralight.out')).read().rstrip('\n')

    def compare(paths, want_gold=False, **kw):
        outs = []

        def factory():
            outs.append(io.StringIO())
            return fsm.fsm(out=outs[-1])

        backs = dec.decode_many(paths, fsm_factory=factory, **kw)
        assert len(backs) == len(paths) == len(outs)
        for p, b, o in zip(paths, backs, outs):
            out = io.StringIO()
            one = dec.decoder(src=p, fsm=fsm.fsm(out=out)).run()
            assert list(b.packets) == list(one.packets) and len(b.packets) > 10, p
            assert o.getvalue() == out.getvalue(), p
            if want_gold:
                assert o.getvalue().rstrip('\n') == gold, p
        return backs

    # eight recordings of the Ultralight transaction as raw complex64, ragged: trailing idle carrier of different lengths
    paths = []
    for i in range(8):
        p = str(tmp_path / ('cap%d.fc32' % i))
        tail = np.tile(iq[-2:], 100 * i)
        np.concatenate([iq, tail]).astype(np.float32).tofile(p)
        paths.append(p)
    compare(paths, want_gold=True)
    compare(paths[:3], want_gold=True, max_push_samples=5000)   # captures longer than a push are streamed in pieces
    # one call each for complex int16, complex uint8 and a 16-bit WAV
    p16 = str(tmp_path / 'a.sc16')
    load_npz('fx_ultralight_sc16.npz')['iq16'].tofile(p16)
    compare([p16, p16])
    pu8 = str(tmp_path / 'a.cu8')
    load_npz('fx_ultralight_cu8.npz')['iq8'].tofile(pu8)
    compare([pu8, pu8])
    pw = str(tmp_path / 'a.wav')
    write_wav(pw, load_npz('fx_ultralight_rec16.npz')['pcm'])
    compare([pw, pw], want_gold=True)
    with pytest.raises(ValueError):
        dec.decode_many([paths[0], pw])
