"""The fetch of a multi-stream context: nfc_multi_fetch / nfc_multi_get_counts_all (include/nfc_amd.h), api.NfcMultiContext.fetch,
api.NfcMultiFetch, and decoder.decode_many's use of it.

A fetch packs what every stream stored in the last push on the GPU (csrc/multi_fetch.hip.h: a scan of the stored amounts, a gather of
the slab rows), brings the packed buffer to the host in one copy and serves every later read of that push from host memory.  It must
change no result: the expected values are the UNMODIFIED reference's arrays in tests/golden/fx_*.npz and the pinned C oracle, and --
byte for byte -- what the per-stream readers return from the device without a fetch."""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import test_multi as tm
from tests.golden_util import Case, load_npz
from usrp_nfc_amd import _lib, api, build, decoder as dec, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = api.NFC_IN_ENV_F32
FETCH = dict(NFC_MULTI_FETCH_EDGES=1, NFC_MULTI_FETCH_SYMBOLS=2, NFC_MULTI_FETCH_PACKETS=4, NFC_MULTI_FETCH_ALL=7)
MF = dict(NFC_MF_EDGES=0, NFC_MF_SYM0=1, NFC_MF_SYM1=2, NFC_MF_PK0=3, NFC_MF_PK1=4, NFC_MF_BITS0=5, NFC_MF_BITS1=6, NFC_MF_ARRAYS=7)


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_header_and_binding(tmp_path):
    h = open(os.path.join(ROOT, 'include', 'nfc_amd.h')).read()
    for s in ('nfc_multi_fetch', 'nfc_multi_get_counts_all'):
        assert re.search(r'\b%s\(' % s, h) and s in _lib.SYMBOLS, s
    assert set(re.findall(r'\b(nfc_[a-z_0-9]+)\s*\(', h)) - {'nfc_ctx'} == set(_lib.SYMBOLS)   # test_host_abi's "declared == bound"
    assert re.search(r'#define NFC_AMD_ABI_VERSION 4\b', h) and _lib.ABI_VERSION == 4
    assert re.search(r'\(still 4,[^)]*nfc_multi_fetch', h)
    for name, v in list(FETCH.items()) + list(MF.items()):
        m = re.search(r'\b%s\b(?:\s*=\s*(\d+))?' % name, h)
        assert m, name
        assert getattr(_lib, name) == getattr(api, name) == v and name in api.__all__, name
    for name in ('NfcMultiFetch', 'COUNTS_DTYPE'):
        assert name in api.__all__
    # the values as the C compiler sees them, and the structures' sizes against the ctypes mirrors
    names = list(FETCH) + list(MF)
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfc_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu'
                   + ' %d' * len(names) + '\\n", sizeof(nfc_multi_fetched), sizeof(nfc_multi_stats), offsetof(nfc_multi_stats, n_fetches), '
                   'offsetof(nfc_multi_stats, n_reads_device), offsetof(nfc_multi_fetched, bytes_copied), sizeof(nfc_counts), '
                   + ', '.join(names) + '); return 0; }\n')
    exe = str(tmp_path / 'sz')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', exe])
    out = [int(v) for v in subprocess.check_output([exe]).split()]
    assert out[0] == C.sizeof(_lib.MultiFetched)
    assert out[1] == C.sizeof(_lib.MultiStats) == 64
    assert out[2] == _lib.MultiStats.n_fetches.offset and out[3] == _lib.MultiStats.n_reads_device.offset
    assert out[4] == _lib.MultiFetched.bytes_copied.offset
    assert out[5] == C.sizeof(_lib.Counts) == _lib.COUNTS_DTYPE.itemsize
    assert out[6:] == [dict(FETCH, **MF)[n] for n in names]


def test_fetch_kernels_isa(tmp_path):
    # csrc/nfc_multi.hip compiled for gfx950 as the product is: both fetch kernels are there, neither with scratch.  The register
    # counts are printed, not asserted: DESIGN.md records them.
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-shared')]
    asm = str(tmp_path / 'nfc_multi.s')
    subprocess.check_call([hipcc] + flags + ['-S', '--cuda-device-only', os.path.join(build.CSRC, 'nfc_multi.hip'), '-o', asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    for kernel in ('k_multi_fetch_scan', 'k_multi_fetch_gather'):
        nm = re.search(r'^(_ZN3nfc5multi\d+%sE\w*):' % kernel, text, re.M)
        assert nm, kernel
        body = re.search(r'^%s:(.*?)\.end_amdhsa_kernel' % re.escape(nm.group(1)), text, re.S | re.M)
        assert body, kernel
        body = body.group(1)
        assert re.search(r'\.amdhsa_private_segment_fixed_size 0\b', body), kernel
        assert 'scratch_' not in body, kernel
        print('%s: %s VGPRs, %s SGPRs, %s bytes of LDS' % (kernel, re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1),
                                                           re.search(r'\.amdhsa_next_free_sgpr (\d+)', body).group(1),
                                                           re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)))
        if kernel == 'k_multi_fetch_gather':   # no LDS in the gather; its copies' bodies are 16-byte loads and stores
            assert re.search(r'\.amdhsa_group_segment_fixed_size 0\b', body)
            assert 'global_load_dwordx4' in body and 'global_store_dwordx4' in body
    assert 'multi_fetch.hip.h' in build.DEPS


# ---- GPU: helpers -----------------------------------------------------------------------------------------------------------

def read_stream(v, allow=None):
    """Everything the per-stream readers give for one stream."""
    return dict(edges=v.edges(allow), sym=[v.symbols(t, allow) for t in (0, 1)], table=[v.packet_table(t, allow) for t in (0, 1)],
                bits=[v.packet_bits(t, allow) for t in (0, 1)], packets=v.packets(allow))


def fetched_stream(f, k, allow=None):
    """The same from a fetch."""
    return dict(edges=f.edges(k, allow), sym=[f.symbols_of(k, t, allow) for t in (0, 1)], table=[f.packet_table_of(k, t, allow) for t in (0, 1)],
                bits=[f.packet_bits_of(k, t, allow) for t in (0, 1)], packets=f.packets_of(k, allow))


def same(a, b):
    """Two such readings, byte for byte."""
    return (a['edges'].dtype == b['edges'].dtype and a['edges'].tobytes() == b['edges'].tobytes() and a['packets'] == b['packets']
            and all(a[key][t].dtype == b[key][t].dtype and a[key][t].tobytes() == b[key][t].tobytes() for key in ('sym', 'table', 'bits') for t in (0, 1)))


def as_result(r, factor):
    """A reading in test_multi's form (check_case)."""
    e = r['edges']
    return dict(transitions=[((int(v), int(d) * factor), int(t)) for v, d, t in zip(e['v'], e['d'], e['t'])], sym_tag=r['sym'][0].tolist(),
                sym_reader=r['sym'][1].tolist(), packets=list(r['packets']), edge_idx=e['idx'].tolist())


def add_result(acc, r):
    for key in acc:
        acc[key] += r[key]


def check_offsets(f, m):
    """off[a] is the exclusive prefix of what the readers would return, and off[a][K] the total."""
    cnt = m.counts_all()
    K = m.n_streams
    for a in range(api.NFC_MF_ARRAYS):
        assert f.off[a].shape == (K + 1,) and f.off[a][0] == 0 and np.all(np.diff(f.off[a].astype(np.int64)) >= 0), a
    assert np.array_equal(np.diff(f.off[api.NFC_MF_EDGES]), cnt['n_edges'])   # (default capacities: nothing cut)
    for t in (0, 1):
        assert np.array_equal(np.diff(f.off[api.NFC_MF_SYM0 + t]), cnt['n_symbols'][:, t])
        assert np.array_equal(np.diff(f.off[api.NFC_MF_PK0 + t]), cnt['n_packets'][:, t])
        # (a bit row holds the closed packets' bits and then those of a packet still open at the push's end)
        assert np.all(np.diff(f.off[api.NFC_MF_BITS0 + t]) >= cnt['n_packet_bits'][:, t])
        assert len(f.symbols[t]) == f.off[api.NFC_MF_SYM0 + t][K] and len(f.packet_table[t]) == f.off[api.NFC_MF_PK0 + t][K]
        assert len(f.packet_bits[t]) == f.off[api.NFC_MF_BITS0 + t][K]
    assert len(f.edge_pos) == len(f.edge_code) == f.off[api.NFC_MF_EDGES][K]


# ---- GPU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('what', [0, 8, 15, 1 << 31])
def test_bad_what_is_refused(what):
    with api.NfcMultiContext(2, 1000, input_kind=ENV) as m:
        m.push([np.zeros(100, np.float32)] * 2)
        with pytest.raises(api.NfcError) as e:
            m.fetch(what)
        assert 'what' in str(e.value) and 'status -1' in str(e.value)
        assert int(m.stats().n_fetches) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('label', ['env-1.1', 'env-1.09', 'sc8'])
def test_reference_fixtures_one_push_ragged(label):
    _, kind, params, items = tm.group_of(label)
    if label == 'env-1.1':
        # the condition on the inputs, from the golden counts alone: the packed symbol sections start streams at many different
        # offsets mod 16 (every head / tail length of the gather's copies), and some streams contribute nothing at all
        for key in ('sym_tag', 'sym_reader'):
            off = np.cumsum([0] + [len(getattr(c, key)) for c, _ in items])[:-1]
            assert len(set((off % 16).tolist())) >= 5, key
        assert sum(1 for c, _ in items if not len(c.tr_v) and not len(c.sym_tag) and not len(c.sym_reader) and not len(c.pk_len)) >= 4
        assert len(items) == 13
    K = len(items)
    piece = max(1, max(len(x) // tm.PER[kind] for _, x in items))
    with api.NfcMultiContext(K, piece, input_kind=kind, **params) as m:
        m.push([x for _, x in items])
        before = [read_stream(m.stream(k)) for k in range(K)]   # from the device, stream by stream
        assert int(m.stats().n_reads_device) > 0 and int(m.stats().n_fetches) == 0
        f = m.fetch()
        st = m.stats()
        assert int(st.n_fetches) == 1 and int(st.n_launches) == 1   # (n_launches stays the push's)
        assert f.what == api.NFC_MULTI_FETCH_ALL and f.n_streams == K and f.n_launches == 2 and f.bytes_copied > 0
        assert np.all(f.base == 0) and np.all(f.flags == 0)
        check_offsets(f, m)
        for k, (c, _) in enumerate(items):
            got = fetched_stream(f, k)
            tm.check_case(c, as_result(got, m.factor), label)
            assert same(got, before[k]), (label, k, c.name)
            assert same(read_stream(m.stream(k)), before[k]), (label, k, c.name)   # the readers, now from the host copy
        assert f.packets_all() == [b['packets'] for b in before]
        # the per-stream view numpy.split gives
        for t in (0, 1):
            parts = np.split(f.symbols[t], f.off[api.NFC_MF_SYM0 + t][1:-1].astype(np.int64))
            assert [p.tolist() for p in parts] == [b['sym'][t].tolist() for b in before]


SEAM_FIXTURES = ['fx_reqa_atqa', 'fx_short_1500', 'fx_stress_zero_start']
_seam = {}


def seam_cases():
    """The three fixtures and ONE parameter set for them (hi_val 1.1; fx_reqa_atqa was recorded with 1.09): the C oracle confirms,
    without a GPU, that every fixture's arrays are what the reference gives under it."""
    if not _seam:
        cs = [Case(n) for n in SEAM_FIXTURES]
        params = dict(cs[0].params, hi_val=1.1)
        for c in cs:
            assert dict(c.params, hi_val=1.1) == params
            o = co.COracle(**params)
            o.push_env(c.x)
            assert o.transitions() == c.transitions and o.packets() == c.packets, c.name
            assert o.symbols(0).tolist() == c.sym_tag.tolist() and o.symbols(1).tolist() == c.sym_reader.tolist(), c.name
        assert not len(cs[1].tr_v) and len(cs[0].pk_len) and len(cs[2].sym_tag)
        _seam['cases'], _seam['params'] = cs, params
        _seam['want'] = [dict(transitions=c.transitions, sym_tag=c.sym_tag.tolist(), sym_reader=c.sym_reader.tolist(), packets=c.packets) for c in cs]
    return _seam['cases'], _seam['params'], _seam['want']


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 63, 64, 65, 1023, 1025])
def test_stream_counts_around_the_scans_seams(K):
    # a scan thread takes ceil(K / 1024) consecutive streams, a wave 64 threads: one stream, a wave's last lane, the next wave's
    # first, the last thread alone with one stream, and the first K at which a thread takes two
    cs, params, want = seam_cases()
    n = max(len(c.x) for c in cs)
    with api.NfcMultiContext(K, n, input_kind=ENV, **params) as m:
        m.push([cs[k % 3].x for k in range(K)])
        f = m.fetch()
        check_offsets(f, m)
        stored = [[len(c.tr_v), len(c.sym_tag), len(c.sym_reader)] for c in cs]
        for a, j in ((api.NFC_MF_EDGES, 0), (api.NFC_MF_SYM0, 1), (api.NFC_MF_SYM1, 2)):
            assert int(f.off[a][K]) == sum(stored[k % 3][j] for k in range(K)), a
        for t in (0, 1):
            assert int(f.off[api.NFC_MF_PK0 + t][K]) == sum(sum(1 for p in cs[k % 3].pk_type if p == t) for k in range(K))
            assert int(f.off[api.NFC_MF_BITS0 + t][K]) >= sum(sum(int(n_) for p, n_ in zip(cs[k % 3].pk_type, cs[k % 3].pk_len) if p == t) for k in range(K))
            assert int(f.off[api.NFC_MF_BITS0 + t][K]) == int(np.diff(f.off[api.NFC_MF_BITS0 + t])[:3].sum()) * (K // 3) + int(np.diff(f.off[api.NFC_MF_BITS0 + t])[:K % 3].sum())
        pa = f.packets_all()
        for k in range(K):
            w = want[k % 3]
            got = as_result(dict(edges=f.edges(k), sym=[f.symbols_of(k, 0), f.symbols_of(k, 1)], packets=pa[k]), m.factor)
            assert got['transitions'] == w['transitions'] and got['packets'] == w['packets'], k
            assert got['sym_tag'] == w['sym_tag'] and got['sym_reader'] == w['sym_reader'], k
            assert got['edge_idx'] == sorted(got['edge_idx']), k
        assert f.packets_of(K - 1) == want[(K - 1) % 3]['packets'] and f.packets_of(0) == want[0]['packets']
        assert int(m.stats().n_reads_device) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('how', [777, 'random'])
def test_pieces_with_a_fetch_after_every_push(how):
    _, kind, params, items = tm.group_of('env-1.09')
    assert [c.name for c, _ in items] == ['fx_reqa_atqa', 'fx_ultralight_txn']
    rng = np.random.default_rng(99)
    arrays = [x for _, x in items]
    K = len(arrays)
    cuts = tm.piecing([len(a) for a in arrays], how, rng)
    piece = max(b - a for c in cuts for a, b in zip(c[:-1], c[1:]))
    acc = [tm.empty_result() for _ in range(K)]
    seen = np.zeros(K, np.uint64)
    with api.NfcMultiContext(K, piece, input_kind=kind, **params) as m:
        for r in range(max(len(c) for c in cuts) - 1):
            parts = []
            for k in range(K):
                a, b = (cuts[k][r], cuts[k][r + 1]) if r + 1 < len(cuts[k]) else (0, 0)
                parts.append(arrays[k][a:b])
            m.push(parts)
            f = m.fetch()
            assert np.array_equal(f.base, seen), r   # the stream's samples before this push
            seen += np.array([len(p) for p in parts], np.uint64)
            check_offsets(f, m)
            for k in range(K):
                got = fetched_stream(f, k)
                if not len(parts[k]):
                    assert not len(got['edges']) and not got['packets'] and not len(got['sym'][0]) and not len(got['sym'][1]), (r, k)
                add_result(acc[k], as_result(got, m.factor))
            assert int(m.stats().n_reads_device) == 0
        for (c, _), r in zip(items, acc):
            tm.check_case(c, r, 'pieces/%s' % how)
        assert seen.tolist() == [len(a) for a in arrays]
        # a push that gives every stream nothing: the fetch is all-empty and launches nothing
        m.push([np.zeros(0, np.float32)] * K)
        f = m.fetch()
        assert f.n_launches == 0 and f.bytes_copied == 0 and np.array_equal(f.base, seen)
        assert all(int(o[K]) == 0 for o in f.off) and not len(f.edge_pos) and not len(f.packet_table[0]) and not len(f.symbols[1])
        assert f.packets_all() == [[] for _ in range(K)] and not len(f.edges(1))
        assert int(m.stats().n_fetches) == 1 and not len(m.stream(1).edges()) and int(m.stats().n_reads_device) == 0


@pytest.mark.gpu
def test_served_from_the_host_and_never_stale():
    _, kind, params, items = tm.group_of('env-1.09')
    x0, x1 = items[0][1], items[1][1]
    first, second = [x0, x1, x1[:9000]], [x1[9000:20000], x0, x0[:3000]]   # (different samples in the second push)
    K, n = 3, len(x1)
    with api.NfcMultiContext(K, n, input_kind=kind, **params) as m, api.NfcMultiContext(K, n, input_kind=kind, **params) as twin:
        with pytest.raises(api.NfcError) as e:
            m.fetch()
        assert 'no completed push' in str(e.value) and 'status -4' in str(e.value)
        m.push(first)
        twin.push(first)
        want = [read_stream(twin.stream(k)) for k in range(K)]   # without a fetch: from the device
        assert int(twin.stats().n_reads_device) > 0 and int(twin.stats().n_fetches) == 0
        assert sum(len(w['packets']) for w in want) > 20
        # after fetch(ALL): every reader is served from the host copy
        m.fetch(api.NFC_MULTI_FETCH_ALL)
        got = [read_stream(m.stream(k)) for k in range(K)]
        assert int(m.stats().n_reads_device) == 0 and int(m.stats().n_fetches) == 1
        assert all(same(g, w) for g, w in zip(got, want))
        # (first / cap of the C readers keep their meaning on the host copy)
        got_n, out = C.c_size_t(0), np.zeros(5, np.uint8)
        m._chk(m.L.nfc_multi_read_symbols(m.h, 1, 0, 7, out.ctypes.data, out.size, C.byref(got_n)), 'nfc_multi_read_symbols')
        assert got_n.value == 5 and out.tolist() == want[1]['sym'][0][7:12].tolist()
        m._chk(m.L.nfc_multi_read_symbols(m.h, 1, 0, len(want[1]['sym'][0]) - 2, out.ctypes.data, out.size, C.byref(got_n)), 'nfc_multi_read_symbols')
        assert got_n.value == 2 and out[:2].tolist() == want[1]['sym'][0][-2:].tolist()
        eo = np.zeros(3, api.EDGE_DTYPE)
        m._chk(m.L.nfc_multi_read_edges(m.h, 1, 10, eo.ctypes.data, eo.size, C.byref(got_n)), 'nfc_multi_read_edges')
        assert got_n.value == 3 and eo.tobytes() == want[1]['edges'][10:13].tobytes()
        assert int(m.stats().n_reads_device) == 0
        # after fetch(PACKETS) alone: the packets from the host, the edges still from the device -- and counted
        m.fetch(api.NFC_MULTI_FETCH_PACKETS)
        assert int(m.stats().n_fetches) == 2
        assert [m.stream(k).packets() for k in range(K)] == [w['packets'] for w in want] and int(m.stats().n_reads_device) == 0
        e1 = m.stream(1).edges()
        assert e1.tobytes() == want[1]['edges'].tobytes() and int(m.stats().n_reads_device) == 1
        assert m.stream(1).symbols(0).tobytes() == want[1]['sym'][0].tobytes() and int(m.stats().n_reads_device) == 2
        # push -> fetch -> push of other samples -> read WITHOUT a fetch: the second push's results, from the device
        m.fetch()
        m.push(second)
        twin.push(second)
        assert int(m.stats().n_fetches) == 0 and int(m.stats().n_reads_device) == 0   # (both are counted since the last push)
        want2 = [read_stream(twin.stream(k)) for k in range(K)]
        assert not any(same(a, b) for a, b in zip(want, want2))
        got2 = [read_stream(m.stream(k)) for k in range(K)]
        assert all(same(g, w) for g, w in zip(got2, want2)) and int(m.stats().n_reads_device) > 0
        # push -> fetch -> reset(k): no reader sees the old copy
        f = m.fetch()
        assert all(same(fetched_stream(f, k), want2[k]) for k in range(K))
        reads = int(m.stats().n_reads_device)
        m.reset(1)
        v = m.stream(1)
        assert int(v.counts().n_edges) == 0 and not len(v.edges()) and not v.packets() and not len(v.symbols(0))
        assert same(read_stream(m.stream(0)), want2[0]) and same(read_stream(m.stream(2)), want2[2])
        assert int(m.stats().n_reads_device) > reads   # (the neighbours' reads went to the device again)
        f = m.fetch()   # and a fetch after the reset has nothing of stream 1
        assert not len(f.edges(1)) and not f.packets_of(1) and same(fetched_stream(f, 0), want2[0]) and same(fetched_stream(f, 2), want2[2])
        m.reset()
        with pytest.raises(api.NfcError) as e:
            m.fetch()
        assert 'no completed push' in str(e.value)


@pytest.mark.gpu
def test_truncated_streams_contribute_their_stored_prefix():
    # test_capacity_semantics's setup: edges cut at 64 and packets at 2 per type; stream 2 fits and sits in the same wave
    cu, ct = Case('fx_stress_uniform'), Case('fx_ultralight_txn')
    params = dict(cu.params, hi_val=1.09)
    xs = [cu.x, ct.x, ct.x[:3000], cu.x]
    n = max(len(x) for x in xs)
    oracle = []
    for x in xs:
        o = co.COracle(**params)
        o.push_env(x)
        oracle.append(o)
    assert all(len(oracle[k].edges()) > 64 for k in (0, 1, 3)) and len(oracle[2].edges()) <= 64
    hooks = _lib.hooks_path()
    with api.NfcMultiContext(4, n, input_kind=ENV, cap_edges=64, cap_packets=2, lib_path=hooks, **params) as m:
        guards = m.L.nfc_debug_multi_guards
        guards.argtypes = [C.c_void_p]
        m.push(xs)
        assert guards(m.h) == 0
        cnt = m.counts_all()
        before = [read_stream(m.stream(k), True) for k in range(4)]   # the stored prefixes, from the device
        many = [bool(np.any(cnt['n_packets'][k] > 2)) for k in range(4)]
        assert many[1] and not many[2]
        reads = int(m.stats().n_reads_device)   # (of `before`)
        f = m.fetch()
        assert guards(m.h) == 0   # the slabs' guards and those behind the packed buffer's sections
        assert np.array_equal(m.counts_all(), cnt)   # flags and true counts are untouched by the fetch
        for k in range(4):
            o = oracle[k]
            want_flags = 0 if k == 2 else api.NFC_MULTI_TRUNC_EDGES | (api.NFC_MULTI_TRUNC_PACKETS if many[k] else 0)
            assert int(f.flags[k]) == want_flags == m.stream(k).flags(), k
            assert int(cnt['n_edges'][k]) == len(o.edges()) and cnt['n_symbols'][k].tolist() == [len(o.symbols(0)), len(o.symbols(1))], k
            if k != 2:
                with pytest.raises(api.NfcError) as e:
                    f.edges(k)
                assert 'NFC_MULTI_TRUNC_EDGES' in str(e.value)
            got = fetched_stream(f, k, True)
            assert len(got['edges']) == min(64, len(o.edges())) == int(np.diff(f.off[api.NFC_MF_EDGES])[k])
            assert f.transitions(k, True) == o.transitions()[:64], k
            assert got['edges']['idx'].tolist() == o.edges()['idx'][:64].tolist(), k
            assert got['sym'][0].tolist() == o.symbols(0).tolist() and got['sym'][1].tolist() == o.symbols(1).tolist(), k   # (default room)
            for t in (0, 1):
                assert len(got['table'][t]) == min(2, int(cnt['n_packets'][k][t])), (k, t)
                assert got['bits'][t].tobytes() == before[k]['bits'][t].tobytes(), (k, t)   # what packet_bits(allow_truncated=True) gives
            assert same(got, before[k]), k
            assert same(read_stream(m.stream(k), True), before[k]), k   # and the readers on the host copy
        # the neighbour is whole
        assert f.packets_of(2) == oracle[2].packets() and f.transitions(2) == oracle[2].transitions()
        with pytest.raises(api.NfcError):
            f.packets_all()
        assert f.packets_all(True) == [b['packets'] for b in before]
        assert int(m.stats().n_reads_device) == reads and guards(m.h) == 0   # nothing was read from the device after the fetch


def packed_arrays(f, fr, cm):
    """Every array a fetch(), a fetch_frames() and a fetch_commands() hand out, in a fixed order."""
    out = list(f.off) + [f.base, f.edge_pos, f.edge_code] + f.symbols + f.packet_table + f.packet_bits
    for r in (fr, cm.raw):
        out += r.frame_off + r.byte_off + [r.base] + r.frames + r.bytes + r.par
    return out + [cm.cmd_off, cm.cbyte_off, cm.cmd, cm.src, cm.data, cm.enc, cm.stream_flags]


@pytest.mark.gpu
def test_packed_buffers_grow_between_two_pushes():
    """The three packed buffers -- the fetch's, the frames', the tracked push's -- are allocated for a small first push and must be
    replaced for the second, in the same context: every call of push 2 copies more than 1.5 x its push-1 bytes + 4096, the most a buffer
    sized for push 1 can hold.  Nothing of it may show: the guards hold after every call and push 2 reads byte for byte as in a context
    whose buffers were allocated once, at their final size.

    The streams: the Classic capture of tests/test_commands.py, TWICE in a row in each of the three (the third with the wrong key A).  One
    copy is not enough for the condition: the frames of all three whole captures pack into 3 424 bytes, fewer than the 4 096 alone.
    Push 1 is the first 4 000 samples of stream 0 (REQA and ATQA: a packet of each type), the first 2 500 of stream 1 (edges, no
    packet), nothing of stream 2; push 2 the remainder.  With these cuts the C oracle's counts give, push 1 -> push 2: the fetch 880 ->
    114 688 bytes, the frames 416 -> 6 944, the commands 720 -> 14 848."""
    from tests import test_commands as tc
    one = tc.classic_iq()
    x = np.concatenate([one, one])
    cuts = (4000, 2500, 0)
    first, second = [x[:2 * c] for c in cuts], [x[2 * c:] for c in cuts]
    hooks = _lib.hooks_path()

    def calls(m):
        guards = m.L.nfc_debug_multi_guards
        guards.argtypes = [C.c_void_p]
        got = []
        for call in (m.fetch, m.fetch_frames, m.fetch_commands):
            got.append(call())
            assert guards(m.h) == 0, call.__name__
        return got

    with tc.tracked(3, len(x) // 2, lib_path=hooks) as m, tc.tracked(3, len(x) // 2, lib_path=hooks) as twin:
        m.push(first)
        small = calls(m)
        cnt = m.counts_all()
        assert cnt['n_packets'][0].tolist() == [1, 1] and int(cnt['n_edges'][1]) > 0 and not cnt['n_packets'][1].any() and int(cnt['n_edges'][2]) == 0
        assert len(small[1].frames[0]) == len(small[1].frames[1]) == 1 and len(small[2].cmd) == 2
        m.push(second)
        large = calls(m)
        for a, b in zip(small, large):
            print('%s: %d -> %d bytes copied' % (type(a).__name__, a.bytes_copied, b.bytes_copied))
            assert a.bytes_copied > 0 and b.bytes_copied > 1.5 * a.bytes_copied + 4096, type(a).__name__
        assert large[0].base.tolist() == list(cuts) == large[1].base.tolist() == large[2].raw.base.tolist()
        twin.push(first)
        twin.push(second)
        want = calls(twin)
        assert len(want[2].cmd) == 3 * 48 - 2 and [w.n_launches for w in want] == [2, 2, 3] == [g.n_launches for g in large]
        for i, (g, w) in enumerate(zip(packed_arrays(*large), packed_arrays(*want))):
            assert len(g) and g.dtype == w.dtype and g.tobytes() == w.tobytes(), i
        m.reset(-1)
        m.push([x[:0]] * 3)
        f, fr, cm = calls(m)
        assert f.n_launches == fr.n_launches == cm.n_launches == 0
        assert all(not o.any() for o in f.off + fr.frame_off + fr.byte_off + cm.raw.frame_off + cm.raw.byte_off + [cm.cmd_off, cm.cbyte_off])
        assert all(not len(a) for a in [f.edge_pos, f.edge_code] + f.symbols + f.packet_table + f.packet_bits + fr.frames + fr.bytes + cm.raw.frames
                   + [cm.cmd, cm.src, cm.data, cm.enc])
        assert not f.base.any() and not fr.base.any() and cm.stream_flags.tolist() == [0, 0, 0]


def edge_codes(e, nd):
    """EDGE_DTYPE records -> the 16-bit codes the device keeps (edges.hip.h: edge_code)."""
    return (((e['v'].astype(np.int64) + 1) * nd + e['d']) | ((e['t'].astype(np.int64) + 1) << 14)).astype(np.uint16)


@pytest.mark.gpu
def test_the_largest_stream_count():
    K, n = 65536, 2500
    base = [synth.workload(nm, n + 64, seed=77 + i) for i, nm in enumerate(['all', 'miller', 'manchester', 'stress'])]
    flat = np.concatenate(base)
    per_base = n + 64
    kk = np.arange(K)
    first = (kk % 4) * per_base + (kk // 4) % 64
    cls = (kk % 4) * 64 + (kk // 4) % 64   # 256 distinct streams
    params = dict(samp_rate=2e6, hi_val=1.1)
    want = {}
    for k in range(4 * 64):   # every distinct stream once through the C oracle, in the packed form
        o = tm.oracle_iq(flat[2 * first[k]:2 * (first[k] + n)], params)
        e = o.edges()
        types, lens, bits = o.packet_arrays()
        w = dict(pos=e['idx'].astype(np.uint32), code=edge_codes(e, 51), sym=[o.symbols(0), o.symbols(1)], packets=o.packets(), table=[], bits=[])
        at = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        for t in (0, 1):
            sel = np.nonzero(types == t)[0]
            tab = np.zeros(len(sel), api.PACKET_DTYPE)
            tab['n_bits'] = lens[sel]
            tab['bit_off'] = np.concatenate([[0], np.cumsum(lens[sel])[:-1]]) if len(sel) else []
            tab['type'] = t
            w['table'].append(tab)
            w['bits'].append(np.concatenate([bits[at[i]:at[i + 1]] for i in sel]) if len(sel) else np.zeros(0, np.uint8))
        want[int(cls[k])] = w
    # (2 500 samples are 500 behind the window: these streams store edges and symbols of type 0 and close no packet -- the packet
    # sections are empty at this stream count; the other tests cover them)
    assert sum(len(w['pos']) for w in want.values()) > 2000 and sum(len(w['sym'][0]) for w in want.values()) > 500
    per_class = [want[c] for c in range(256)]

    def packed(get):
        parts = [get(w) for w in per_class]
        lens = np.array([len(p) for p in parts], np.int64)[cls]
        return np.concatenate([parts[c] for c in cls]), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)

    buf = api.DeviceBuffer(flat)
    try:
        with api.NfcMultiContext(K, n, input_kind=api.NFC_IN_IQ_F32, **params) as m:
            m.push_device(buf, first, np.full(K, n))
            f = m.fetch()
            assert int(m.stats().n_launches) == 1 and f.n_launches == 2 and np.all(f.flags == 0) and np.all(f.base == 0)
            for a, arr, get in ((api.NFC_MF_EDGES, f.edge_pos, lambda w: w['pos']), (api.NFC_MF_EDGES, f.edge_code, lambda w: w['code']),
                                (api.NFC_MF_SYM0, f.symbols[0], lambda w: w['sym'][0]), (api.NFC_MF_SYM1, f.symbols[1], lambda w: w['sym'][1])):
                exp, off = packed(get)
                assert np.array_equal(f.off[a], off), a
                assert arr.dtype == exp.dtype and np.array_equal(arr, exp), a
            for t in (0, 1):   # the bit rows: the closed packets' bits lead every stream's part (an open packet's may follow)
                exp, off = packed(lambda w: w['bits'][t])
                npb = np.diff(off).astype(np.int64)
                assert np.array_equal(npb, f.counts['n_packet_bits'][:, t]) and np.all(np.diff(f.off[api.NFC_MF_BITS0 + t]) >= npb)
                at = np.repeat(f.off[api.NFC_MF_BITS0 + t][:-1].astype(np.int64) - off[:-1].astype(np.int64), npb) + np.arange(len(exp))
                assert np.array_equal(f.packet_bits[t][at], exp), t
            for t in (0, 1):
                exp, off = packed(lambda w: w['table'][t])
                assert np.array_equal(f.off[api.NFC_MF_PK0 + t], off)
                got = f.packet_table[t]
                assert all(np.array_equal(got[key], exp[key]) for key in ('bit_off', 'n_bits', 'type')), t
                assert np.all(got['idx'] < n)
            pa = f.packets_all()
            assert all(pa[k] == per_class[cls[k]]['packets'] for k in range(K))
            # counts_all against the per-stream call
            ca = m.counts_all()
            assert ca.shape == (K,)
            for k in np.random.default_rng(9).choice(K, 256, replace=False):
                c, fl = m.stream(int(k))._counts()
                assert (int(c.n_samples), int(c.n_edges), list(c.n_symbols), list(c.n_packets), list(c.n_packet_bits)) == (
                    int(ca['n_samples'][k]), int(ca['n_edges'][k]), ca['n_symbols'][k].tolist(), ca['n_packets'][k].tolist(), ca['n_packet_bits'][k].tolist())
                assert fl == int(ca['flags'][k]) == 0 and int(ca['n_samples'][k]) == n
                w = per_class[cls[k]]
                assert int(ca['n_edges'][k]) == len(w['pos']) and ca['n_symbols'][k].tolist() == [len(w['sym'][0]), len(w['sym'][1])]
            assert int(m.stats().n_reads_device) == 0
    finally:
        buf.free()


@pytest.mark.gpu
def test_decode_many_fetches_once_per_push(tmp_path):
    from usrp_nfc_amd import fsm
    iq = load_npz('fx_ultralight_iq.npz')['iq']
    gold = open(os.path.join(ROOT, 'tests', 'golden', 'ultralight.out')).read().rstrip('\n')
    paths = []
    for i in range(4):   # recordings of the Ultralight transaction as raw complex64, ragged (test_decode_many's kind)
        p = str(tmp_path / ('cap%d.fc32' % i))
        np.concatenate([iq, np.tile(iq[-2:], 100 * i)]).astype(np.float32).tofile(p)
        paths.append(p)
    single = []
    for p in paths:
        out = io.StringIO()
        one = dec.decoder(src=p, fsm=fsm.fsm(out=out)).run()
        single.append((list(one.packets), out.getvalue()))
        assert out.getvalue().rstrip('\n') == gold and len(one.packets) > 10
    for kw, pushes in ((dict(), 1), (dict(max_push_samples=5000), None), (dict(keep=0), 1)):
        outs, stats = [], []

        def factory():
            outs.append(io.StringIO())
            return fsm.fsm(out=outs[-1])

        backs = dec.decode_many(paths, fsm_factory=factory, push_stats=stats, **kw)
        assert len(backs) == len(paths) == len(outs)
        for b, o, (pk, trace) in zip(backs, outs, single):
            assert o.getvalue() == trace   # the command trace is unchanged
            assert list(b.packets) == (pk if kw.get('keep') != 0 else [])   # (keep=0 keeps nothing, as before)
        # one fetch per push, and no read went to the device
        assert stats and all(s == (1, 0) for s in stats), stats
        assert len(stats) == (pushes or -(-(len(iq) // 2 + 300) // 5000))
