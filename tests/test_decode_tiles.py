"""The decode stage at its tile seams (decode.hip.h): tiles of DEC_TILE edges, decoder tables in dynamic LDS sized to the stream,
every tile's workgroup folding the aggregates of the tiles before it.

Every case feeds the stage directly (nfc_push_edges: one short launch chain, no threshold pass), under both of its forms -- the
speculative one (k_dec_spec, k_concat) and the three-launch one (k_dec_reduce, k_dec_apply, k_frame_write) -- and compares symbols,
packets, packet bits and the packets' closing indices with the reference's decoders and PacketProcessor as oracle/py_oracle.py
restates them, driven edge by edge.  The edge lists come from the C oracle's edge stage on synthetic captures; entries routed
nowhere (t = -1, what the reference's router drops) are put in front of them to move a frame to the place in a tile a case is
about.  The shapes (edges per tile, packet ends staged per tile, the tile count up to which a workgroup folds its predecessors
itself, the longest run-in) are read from the test build, never written down here."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import py_oracle as po
from usrp_nfc_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

FORMS = ['1', '0']   # NFC_DEC_SPEC: the speculative form / the three-launch form
RATE = 2e6
_cache = {}


def _dec_shapes(ctx):
    out = (C.c_uint32 * 6)()
    ctx.L.nfc_debug_dec_shapes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    assert ctx.L.nfc_debug_dec_shapes(ctx.h, out) == 0
    return tuple(int(v) for v in out)


def _all_shapes():
    if 'shapes' not in _cache:
        with api.NfcContext(lib_path=_lib.hooks_path()) as ctx:
            _cache['shapes'] = _dec_shapes(ctx)
    return _cache['shapes']


def shapes():
    """(edges per tile, own-prefix tile limit, packet ends staged per tile, LUT rows staged at most) of the test build."""
    return _all_shapes()[:4]


def runin_max():
    """The longest run-in the stage can be given (NFC_DEC_RUNIN), in edges."""
    return _all_shapes()[4]


def folded_itself(ctx):
    """Did the tiles of the context's last batch fold their predecessors themselves (False: the single-workgroup prefix launch ran)?"""
    return bool(_dec_shapes(ctx)[5])


def oracle_edges(iq, max_len=50):
    """What the reference's edge stage makes of a capture: rows of api.EDGE_DTYPE, idx = the row's number."""
    o = co.COracle(samp_rate=RATE, hi_val=1.1, max_len=max_len)
    o.push_iq(iq)
    e = o.edges()
    rows = np.zeros(len(e), api.EDGE_DTYPE)
    rows['d'], rows['v'], rows['t'] = e['d'], e['v'], e['t']
    return rows


def idle(n):
    """n entries the router drops (background.py:30-35: neither direction)."""
    rows = np.zeros(n, api.EDGE_DTYPE)
    rows['d'], rows['t'] = 50, -1
    return rows


def numbered(rows):
    rows = rows.copy()
    rows['idx'] = np.arange(len(rows), dtype=np.uint64) * 3 + 11   # (the caller's own indices: any increasing numbers)
    return rows


class Ref(object):
    """The reference's decoders and packet framing over a list of rows, edge by edge: per type the symbols, and per closed packet
    (type, bits, the row that closed it)."""

    def __init__(self, rows, reader=True, tag=True):
        self.sink = po.BitSink()
        self.mil = po.MillerDecoder(self.sink) if reader else None
        self.man = po.ManchesterDecoder(self.sink) if tag else None
        self.closed_by = []
        self.feed(rows)

    def feed(self, rows):
        f = 1e6 / RATE
        sink, closed_by = self.sink, self.closed_by
        base = getattr(self, 'n', 0)
        for i, (d, v, t) in enumerate(zip(rows['d'].tolist(), rows['v'].tolist(), rows['t'].tolist())):
            dec = self.mil if t == 1 else (self.man if t == 0 else None)
            if dec is None:
                continue
            dec.process_transition([(v, d * f)])
            while len(closed_by) < len(sink.packets):
                closed_by.append(base + i)
        self.n = base + len(rows)

    def state(self):
        """Everything the next edge's outcome depends on."""
        return ([sorted((k, v) for k, v in vars(d).items() if k != 'sink') if d else None for d in (self.mil, self.man)],
                [(p.started, list(p.cur)) for p in self.sink.procs])


def run_gpu(monkeypatch, form, rows, cuts=None, **ctx_kw):
    """The rows through nfc_push_edges in one or several calls: symbols per type, packets as (type, bits, closing idx) in stream
    order, and the stats of the last call."""
    monkeypatch.setenv('NFC_DEC_SPEC', form)
    cuts = cuts or [0, len(rows)]
    sym, pk, resp = {0: [], 1: []}, [], 0
    with api.NfcContext(samp_rate=RATE, hi_val=1.1, **ctx_kw) as ctx:
        for a, b in zip(cuts[:-1], cuts[1:]):
            ctx.push_edges(rows[a:b])
            for t in (0, 1):
                sym[t].append(ctx.symbols(t))
                tab, bits = ctx.packet_table(t), ctx.packet_bits(t)
                for p in tab:
                    o = int(p['bit_off'])
                    pk.append((int(p['idx']), t, bits[o:o + int(p['n_bits'])].tolist()))
            resp += int(ctx.stats().decode_respeculated)
            assert folded_itself(ctx)   # (every case but the one about it stays below the own-prefix limit)
    pk.sort(key=lambda r: r[0])
    return {t: np.concatenate(sym[t]) for t in (0, 1)}, pk, resp


def check(rows, ref, sym, pk):
    for t in (0, 1):
        assert sym[t].tolist() == ref.sink.symbols[t], 'symbols of type %d differ' % t
    want = [(int(rows['idx'][e]), t, bits) for (t, bits), e in zip(ref.sink.packets, ref.closed_by)]
    assert [(t, b) for _, t, b in pk] == [(t, b) for _, t, b in want], 'packets differ'
    assert [i for i, _, _ in pk] == [i for i, _, _ in want], 'closing indices differ'


def traffic(name, n_samples, max_len=50):
    key = ('traffic', name, n_samples, max_len)
    if key not in _cache:
        _cache[key] = oracle_edges(synth.workload(name, n_samples), max_len)
    return _cache[key]


def reference(key, rows, **kw):
    if key not in _cache:
        _cache[key] = Ref(rows, **kw)
    return _cache[key]


# ---- tile edges ---------------------------------------------------------------------------------------------------------------
def _edge_counts():
    return [('tile-1', -1, 1), ('tile', 0, 1), ('tile+1', 1, 1), ('2tiles+1', 1, 2), ('3tiles+1', 1, 3)]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name,plus,mult', _edge_counts())
def test_edge_counts_around_the_tile(monkeypatch, form, name, plus, mult):
    tile = shapes()[0]
    n = mult * tile + plus
    e = traffic('all', 400_000)
    assert len(e) >= n, len(e)
    rows = numbered(e[:n])
    ref = reference(('count', n), rows)
    sym, pk, _ = run_gpu(monkeypatch, form, rows)
    check(rows, ref, sym, pk)
    assert len(pk) > 10


# ---- frames across a tile boundary -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
def test_frames_straddle_the_first_two_seams(monkeypatch, form):
    # both directions' frames back to back: in the edge domain a seam lies inside a frame unless it falls exactly between two
    tile = shapes()[0]
    rows = numbered(traffic('all', 400_000)[:2 * tile + tile // 2])
    ref = reference('straddle', rows)
    closes = np.array(ref.closed_by)
    for seam in (tile, 2 * tile):   # a packet is open across each: the first packet end behind the seam is not the seam's own edge,
        nxt = closes[closes >= seam].min()   # and symbols of the same frame lie before the seam
        assert seam < nxt < seam + 400 and not np.any(closes == seam - 1), (seam, nxt)
    sym, pk, resp = run_gpu(monkeypatch, form, rows)
    check(rows, ref, sym, pk)
    assert resp == 0   # (frames far shorter than the run-in: nothing to repeat)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('where', ['first', 'last'])
def test_packet_closes_on_a_tiles_first_or_last_edge(monkeypatch, form, where):
    tile = shapes()[0]
    e = traffic('miller', 300_000)
    r0 = reference('close-probe', e[:tile])
    c = r0.closed_by[len(r0.closed_by) // 2]   # a packet end somewhere in the middle of the first tile's worth of traffic
    pad = (tile if where == 'first' else tile - 1) + tile - c   # ... moved to edge 2 tile (a tile's first) or 2 tile - 1 (a tile's last)
    rows = numbered(np.concatenate([idle(pad), e[:2 * tile]]))
    ref = reference(('close', where), rows)
    assert (2 * tile if where == 'first' else 2 * tile - 1) in ref.closed_by
    sym, pk, _ = run_gpu(monkeypatch, form, rows)
    check(rows, ref, sym, pk)


# ---- frames longer than the run-in ------------------------------------------------------------------------------------------------
def _long_frame(n_bytes, seed):
    """A short reader frame, one of n_bytes bytes, a short one: the rows, and the long frame's first and last row."""
    key = ('long', n_bytes, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        frames = [(synth.READER, synth.frame_bits([0x26], 7)), (synth.READER, synth.frame_bits(rng.integers(0, 256, n_bytes).tolist(), 0)),
                  (synth.READER, synth.frame_bits([0x26], 7))]
        e = oracle_edges(synth.iq_from_profile(synth.modulation_profile(frames, rate_msps=2.0, gap_us=150.0, lead_in=3000, tail=400)))
        r = Ref(e)
        assert [len(b) for _, b in r.sink.packets] == [8, 9 * n_bytes + 1, 8]
        _cache[key] = (e, r.closed_by[0], r.closed_by[1])   # (the row that ends a frame is the next frame's first)
    return _cache[key]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('runin', ['512', '2048'])
def test_a_frame_longer_than_the_run_in_takes_the_fall_back(monkeypatch, form, runin):
    tile = shapes()[0]
    e, first, last = _long_frame(250, 7)
    RUNIN_MAX = runin_max()
    assert RUNIN_MAX + 1000 < last - first < tile
    # ordinary traffic, then three such frames, each beginning 300 edges before the run-in of a seam (2, 4, 6 tiles) and ending
    # behind the seam: no frame gap within reach of those tiles
    parts, n = [traffic('miller', 300_000)[:tile]], tile
    for seam in (2 * tile, 4 * tile, 6 * tile):
        pad = seam - RUNIN_MAX - 300 - first - n
        parts += [idle(pad), e]
        n += pad + len(e)
        assert n - len(e) + first < seam - RUNIN_MAX and n - len(e) + last > seam + 500
    rows = numbered(np.concatenate(parts))
    ref = reference('long-seam', rows)
    monkeypatch.setenv('NFC_DEC_RUNIN', runin)
    sym, pk, resp = run_gpu(monkeypatch, form, rows)
    check(rows, ref, sym, pk)
    assert sum(len(b) > 2000 for _, _, b in pk) == 3
    assert resp == (1 if form == '1' else 0), resp   # the check failed, the stage ran again in the three-launch form: once


@pytest.mark.parametrize('form', FORMS)
def test_a_long_frame_inside_one_tile_needs_no_fall_back(monkeypatch, form):
    tile = shapes()[0]
    e, first, last = _long_frame(200, 8)   # longer than the longest run-in, shorter than a tile
    RUNIN_MAX = runin_max()
    assert RUNIN_MAX + 500 < last - first < tile - 400, (first, last)
    # ordinary traffic up to 67 edges before the seam between tiles 1 and 2 (its frame gaps lie within every run-in); the long
    # frame begins 100 edges behind that seam and ends inside tile 2; ordinary traffic again
    t = traffic('miller', 300_000)
    rows = numbered(np.concatenate([idle(tile + 100 - first), t[:tile], e, t[:tile]]))
    assert 2 * tile + 100 + (last - first) < 3 * tile
    ref = reference('long-inside', rows)
    monkeypatch.setenv('NFC_DEC_RUNIN', str(RUNIN_MAX))
    sym, pk, resp = run_gpu(monkeypatch, form, rows)
    check(rows, ref, sym, pk)
    assert sum(len(b) > 1500 for _, _, b in pk) == 1
    assert resp == 0, resp


# ---- table sizes and decoder sets ---------------------------------------------------------------------------------------------------
def _spec_bytes(rows, decoders):
    return decoders * (rows * 16 + (rows + 1) * 8)   # k_dec_spec per decoder: a walk table of 16-byte rows, a map table with the identity row


def _dec_lds(ctx, which):
    dyn, wgs = C.c_uint32(0), C.c_int(0)
    ctx.L.nfc_debug_dec_lds.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    assert ctx.L.nfc_debug_dec_lds(ctx.h, which, C.byref(dyn), C.byref(wgs)) == 0
    return int(dyn.value), int(wgs.value)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('max_len', [50, 127, 250])
@pytest.mark.parametrize('reader,tag', [(True, False), (False, True), (True, True)])
def test_table_sizes_and_decoder_sets(monkeypatch, form, max_len, reader, tag):
    tile, _, _, lds_rows = shapes()
    e = traffic('all', 400_000, max_len)
    rows = numbered(e[:2 * tile + 1])
    assert int(rows['d'].max()) == max_len   # the tables' last rows are looked up
    ref = reference(('tables', max_len, reader, tag), rows, reader=reader, tag=tag)
    sym, pk, _ = run_gpu(monkeypatch, form, rows, max_len=max_len, reader=reader, tag=tag)
    check(rows, ref, sym, pk)
    assert len(pk) > 5
    # what the launches ask for: the stream's 4 (max_len + 1) rows per decoder it runs, nothing beyond the staged limit
    n_rows = 4 * (max_len + 1)
    with api.NfcContext(samp_rate=RATE, hi_val=1.1, max_len=max_len, reader=reader, tag=tag, lib_path=_lib.hooks_path()) as ctx:
        got = [_dec_lds(ctx, k) for k in range(3)]
    decoders = int(reader) + int(tag)
    if n_rows > lds_rows:
        assert [g[0] for g in got] == [0, 0, 0]
    else:
        assert got[0][0] == _spec_bytes(n_rows, decoders)
        assert got[1][0] == n_rows * (16 * int(reader) + 8 * int(tag))
        assert got[2][0] == n_rows * (32 * int(reader) + 16 * int(tag))
        if decoders == 1:
            assert got[0][0] <= _spec_bytes(n_rows, 2) // 2
    assert all(g[1] >= 1 for g in got)
    if max_len == 50 and decoders == 1:
        # with the bench's tables LDS is not what limits k_dec_spec's workgroups on a CU: the one-decoder kernel's registers
        # give five; the 512 rows of both decoders it used to reserve gave five by LDS alone
        assert got[0][1] >= 5, got


# ---- more tiles than a workgroup folds by itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
def test_more_tiles_than_a_workgroup_folds_itself(monkeypatch, form):
    # own_prefix_max tiles and one edge: the single-workgroup prefix launch (scan_partials) takes over.  The capture is periodic and
    # every period ends in a frame gap, so the reference is one period's outcome repeated -- checked below, not assumed: the
    # decoders and the framing are in the same state after the first period and after the second.  (33.5 M rows, half a gigabyte:
    # 0.5 s per form on an MI355X box, most of it the host's copies.)
    tile, own_max, _, _ = shapes()
    n = own_max * tile + 1
    per = oracle_edges(synth.iq_from_profile(synth.modulation_profile(synth.txn_frames(), rate_msps=2.0, lead_in=0, tail=0)))
    per = per[1:]   # (the capture's first edge has no frame before it)
    P = len(per)
    r = Ref(per)
    s1, n_sym1, n_pk1 = r.state(), [len(s) for s in r.sink.symbols], len(r.sink.packets)
    r.feed(per)
    assert r.state() == s1
    reps = -(-n // P)
    rows = np.tile(per, reps)[:n]
    rows['idx'] = np.arange(n, dtype=np.uint64) * 3 + 11   # (numbered() in place: the list is half a gigabyte)
    r3 = Ref(per)
    r3.feed(per[:n - (reps - 1) * P])   # the last, cut period, entered in the state every period but the first is entered in
    want_sym = {}
    for t in (0, 1):
        first, second = r.sink.symbols[t][:n_sym1[t]], r.sink.symbols[t][n_sym1[t]:]
        last = r3.sink.symbols[t][n_sym1[t]:]
        want_sym[t] = np.concatenate([np.array(first, np.uint8), np.tile(np.array(second, np.uint8), reps - 2), np.array(last, np.uint8)])
    monkeypatch.setenv('NFC_DEC_SPEC', form)
    with api.NfcContext(samp_rate=RATE, hi_val=1.1) as ctx:
        ctx.push_edges(rows)
        assert not folded_itself(ctx)   # the prefix launch ran
        for t in (0, 1):
            assert np.array_equal(ctx.symbols(t), want_sym[t]), 'symbols of type %d differ' % t
        got = []
        for t in (0, 1):
            tab, bits = ctx.packet_table(t), ctx.packet_bits(t)
            got.append((tab, bits))
    # packets: period k's are period 2's with their closing rows moved by (k - 2) P
    pk2 = [(e, t, b) for (t, b), e in zip(r.sink.packets[n_pk1:], r.closed_by[n_pk1:])]
    pk1 = [(e, t, b) for (t, b), e in zip(r.sink.packets[:n_pk1], r.closed_by[:n_pk1])]
    pkl = [(e - P + (reps - 1) * P, t, b) for (t, b), e in zip(r3.sink.packets[n_pk1:], r3.closed_by[n_pk1:])]
    for t in (0, 1):
        tab, bits = got[t]
        a1 = [(e, b) for e, tt, b in pk1 if tt == t]
        a2 = [(e - P, b) for e, tt, b in pk2 if tt == t]
        al = [(e, b) for e, tt, b in pkl if tt == t]
        want_n = np.concatenate([np.array([len(b) for _, b in a1], np.int64), np.tile(np.array([len(b) for _, b in a2], np.int64), reps - 2),
                                 np.array([len(b) for _, b in al], np.int64)])
        e2 = np.array([e for e, _ in a2], np.int64)
        want_e = np.concatenate([np.array([e for e, _ in a1], np.int64),
                                 (e2[None, :] + (np.arange(1, reps - 1, dtype=np.int64) * P)[:, None]).ravel(),
                                 np.array([e for e, _ in al], np.int64)])
        want_bits = np.concatenate([np.array(sum((b for _, b in a1), []), np.uint8), np.tile(np.array(sum((b for _, b in a2), []), np.uint8), reps - 2),
                                    np.array(sum((b for _, b in al), []), np.uint8)])
        assert np.array_equal(tab['n_bits'].astype(np.int64), want_n), 'packet lengths of type %d differ' % t
        assert np.array_equal(tab['idx'].astype(np.int64), want_e * 3 + 11), 'closing indices of type %d differ' % t
        off = np.cumsum(want_n) - want_n
        at = np.repeat(tab['bit_off'].astype(np.int64) - off, want_n) + np.arange(len(want_bits), dtype=np.int64)
        assert np.array_equal(bits[at], want_bits), 'packet bits of type %d differ' % t
    assert len(got[0][0]) + len(got[1][0]) > own_max   # (several packets per tile)


# ---- more packet ends in a tile than it stages ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
def test_more_packet_ends_in_a_tile_than_it_stages(monkeypatch, form):
    # reader frames of ONE data bit, 40 us apart: a packet end every six or seven edges, more than a tile stages (asserted below
    # from the reference).  The speculative form must say so (dec_verify) and the three-launch form take the batch.
    tile, _, staged, _ = shapes()
    if 'tiny' not in _cache:
        frames = [(synth.READER, [k & 1]) for k in range(tile // 2)]
        _cache['tiny'] = oracle_edges(synth.iq_from_profile(synth.modulation_profile(frames, rate_msps=2.0, gap_us=40.0, lead_in=3000, tail=400)))
    rows = numbered(_cache['tiny'][:tile + tile // 2])
    ref = reference('tiny-ref', rows)
    closes = np.array(ref.closed_by)
    assert np.sum(closes < tile) > staged and len(ref.sink.packets) == len(closes)
    sym, pk, resp = run_gpu(monkeypatch, form, rows)
    check(rows, ref, sym, pk)
    assert resp == (1 if form == '1' else 0), resp
