"""Frames assembled on the GPU (include/nfc_amd.h: nfc_raw_frame; csrc/frames.hip.h, nfc_frames.hip): closed packets -> the repaired
frame end, the bytes, the parity bits, the parity and CRC_A verdicts.

The CPU suite pins the kernels' host twin (nfc_host_frames) to a numpy restatement of the reference (fsm.py:28-66, utilities.py:30-41)
and nfc_fsm_process_frames to nfc_fsm_process_packets; the GPU suite pins the kernels to the host twin, from every bit source.

THE CRAFTED CAPTURE is the smallest input on which every branch exists: for seed in 7, 8, 9, 10 and L in 1 .. 45, a reader and a tag
frame of L random bits, then per seed and direction a frame with a good CRC_A and one of 40 bytes.  334 720 samples in one push take
the multi-launch stages (bits packed 32 to a word), one seed alone (86 234 samples) the one-launch stage (a byte per bit).  Its
coverage -- every n_bits % 9, both values of the extra bit, both parity and both CRC outcomes, the bit offsets modulo 32, a packet of
300 bits or more -- is ASSERTED from the packets a decode returned, not assumed."""
import ctypes
import glob
import io
import os

import numpy as np
import pytest

from tests.golden_util import GOLDEN, Case
from usrp_nfc_amd import _lib, api, fsm, synth

RAW = _lib.RAW_FRAME_DTYPE
EXTRA, MANY, PAR_OK, CRC_OK, CUT = 1, 2, _lib.NFC_RAW_PARITY_OK, _lib.NFC_RAW_CRC_A_OK, _lib.NFC_RAW_CUT
GOLD_UL = os.path.join(GOLDEN, 'ultralight.out')
GOLD_1K = os.path.join(GOLDEN, '1k_with_enc.out')
SEEDS = (7, 8, 9, 10)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def crafted_frames(seeds=SEEDS):
    frames = []
    for seed in seeds:
        rng = np.random.Generator(np.random.PCG64(seed))
        for L in range(1, 46):
            for d in (synth.READER, synth.TAG):
                frames.append((d, rng.integers(0, 2, L).tolist()))
        for d in (synth.READER, synth.TAG):
            frames.append((d, synth.frame_bits([0x30, 0x04, 0x26, 0xEE])))
            frames.append((d, synth.frame_bits(list(range(40)))))
    return frames


_cache = {}


def crafted_iq(seeds=SEEDS):
    key = ('iq', tuple(seeds))
    if key not in _cache:
        _cache[key] = synth.iq_from_profile(synth.modulation_profile(crafted_frames(seeds)))
        _cache[key].setflags(write=False)
    return _cache[key]


def crafted_oracle_packets():
    """The crafted capture through the C restatement of the reference path (oracle/nfc_oracle.c): [(type, [bits]), ...]."""
    if 'oracle' not in _cache:
        from oracle import c_oracle
        o = c_oracle.COracle(hi_val=1.1)
        o.push_iq(crafted_iq())
        _cache['oracle'] = [(t, b) for t, b in o.packets() if b]
        o.close()
    return _cache['oracle']


def golden_packet_cases():
    """(name, packets) of every tests/golden/fx_*.npz that holds packets (a file of several cases: one per key prefix)."""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'fx_*.npz'))):
        name = os.path.basename(path)[:-4]
        keys = np.load(path).files
        for k in keys:
            if k.endswith('pk_type'):
                prefix = k[:-len('pk_type')]
                c = Case(name + ':' + prefix, prefix=prefix, file=name) if prefix else Case(name)
                out.append((name + (':' + prefix if prefix else ''), [(t, b) for t, b in c.packets if b]))
    return out


GOLDEN_CASES = golden_packet_cases()


def tables_of(packets):
    """[(type, bits), ...] in stream order -> per type the PACKET_DTYPE rows (idx: the place in the list) and the bit array."""
    rows, bits = ([], []), ([], [])
    for i, (t, b) in enumerate(packets):
        rows[t].append((i, len(bits[t]), len(b), t))
        bits[t].extend(b)
    return [np.array(rows[t], _lib.PACKET_DTYPE) for t in (0, 1)], [np.array(bits[t], np.uint8) for t in (0, 1)]


def merged(tabs):
    t = np.concatenate(tabs)
    return t[np.argsort(t['idx'], kind='stable')]


def host_frames_of(packets):
    tabs, bits = tables_of(packets)
    parts = [api.host_frames(tabs[t], bits[t], t) for t in (0, 1)]
    return api.NfcFrames([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]), tabs, bits


# ---- the reference, restated with numpy (fsm.py:28-66; utilities.py:30-41 through fsm.crc_a) ---------------------------------------
def ref_frame(bits, ptype):
    start = 1 if ptype == 0 else 0   # packets.py:24-28
    b, flags = list(bits), 0
    rem = len(b) % 9
    if rem == 8:
        b.append(start)
    elif rem == 1:
        if b[-1] != start:
            flags |= EXTRA
        b.pop()
    elif rem:
        flags |= MANY
        b = b[:len(b) - rem]
    a = np.array(b, np.uint8).reshape(-1, 9)
    data = (a[:, :8].astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=1).astype(np.uint8)
    par = a[:, 8].copy()
    if len(a) and not ((a[:, :8].sum(axis=1) & 1) == par).any():
        flags |= PAR_OK
        if len(data) >= 2 and fsm.crc_a(data[:-2]) == data[-2:].tolist():
            flags |= CRC_OK
    return flags, data, par


def check_against_restatement(frames, tabs, bits):
    for t in (0, 1):
        recs = frames.records[t]
        assert len(recs) == len(tabs[t])
        at = 0
        for r, p in zip(recs, tabs[t]):
            o = int(p['bit_off'])
            flags, data, par = ref_frame(bits[t][o:o + int(p['n_bits'])], t)
            assert (int(r['idx']), int(r['n_bits']), int(r['type']), int(r['reserved'])) == (int(p['idx']), int(p['n_bits']), t, 0)
            assert int(r['byte_off']) == at and int(r['n_bytes']) == len(data)
            assert int(r['flags']) == flags, (t, int(p['idx']), hex(int(r['flags'])), hex(flags))
            assert frames.bytes[t][at:at + len(data)].tolist() == data.tolist()
            assert frames.par[t][at:at + len(data)].tolist() == par.tolist()
            at += len(data)
        assert at == len(frames.bytes[t]) == len(frames.par[t])


def assert_coverage(tabs, bits, records):
    """What makes the crafted capture the crafted capture, read off the packets a decode returned."""
    for t in (0, 1):
        n, off, fl = tabs[t]['n_bits'].astype(np.int64), tabs[t]['bit_off'].astype(np.int64), records[t]['flags']
        assert set((n % 9).tolist()) == set(range(9)), 'every n_bits % 9'
        last = bits[t][(off + n - 1)[n % 9 == 1]]
        assert set(last.tolist()) == {0, 1}, 'both values of the extra bit'
        assert ((fl & PAR_OK) != 0).any() and ((fl & PAR_OK) == 0).any(), 'both parity outcomes'
        ok = (fl & PAR_OK) != 0
        assert ((fl[ok] & CRC_OK) != 0).any() and ((fl[ok] & CRC_OK) == 0).any(), 'both CRC outcomes'
        assert len(set((off % 32).tolist())) >= 24, 'bit offsets modulo 32'
    assert max(int(tabs[t]['n_bits'].max()) for t in (0, 1)) >= 300, 'a long packet'


def assert_frames_equal(got, want):
    for t in (0, 1):
        assert got.records[t].tobytes() == want.records[t].tobytes(), 'records of type %d' % t
        assert got.bytes[t].tobytes() == want.bytes[t].tobytes(), 'bytes of type %d' % t
        assert got.par[t].tobytes() == want.par[t].tobytes(), 'parity bits of type %d' % t
    assert got.table.tobytes() == want.table.tobytes()


# ---- CPU suite -----------------------------------------------------------------------------------------------------------------
def test_crafted_capture_covers_every_branch():
    packets = crafted_oracle_packets()
    assert len(crafted_iq()) // 2 > 1 << 18 > len(crafted_iq(SEEDS[:1])) // 2   # one push: the multi-launch stages; one seed: the one-launch stage
    assert len(packets) == 373
    frames, tabs, bits = host_frames_of(packets)
    assert_coverage(tabs, bits, frames.records)
    for t in (0, 1):
        assert np.bincount(tabs[t]['n_bits'] % 9, minlength=9).min() >= 15
        assert int(((frames.records[t]['flags'] & CRC_OK) != 0).sum()) == 4


def test_host_frames_on_the_crafted_packets():
    frames, tabs, bits = host_frames_of(crafted_oracle_packets())
    check_against_restatement(frames, tabs, bits)


@pytest.mark.parametrize('name', [n for n, _ in GOLDEN_CASES])
def test_host_frames_on_the_golden_packets(name):
    packets = dict(GOLDEN_CASES)[name]
    frames, tabs, bits = host_frames_of(packets)
    check_against_restatement(frames, tabs, bits)


def test_host_frames_rejects_what_it_cannot_do():
    tabs, bits = tables_of([(1, synth.frame_bits([0x26, 0x00]))])
    with pytest.raises(api.NfcError):
        api.host_frames(tabs[1], bits[1], 0)            # a row of another type
    with pytest.raises(api.NfcError):
        api.host_frames(tabs[1], bits[1][:5], 1)        # packets that reach behind the bit array
    recs, data, par = api.host_frames(tabs[1][:0], bits[1], 1)
    assert len(recs) == len(data) == len(par) == 0


def both_ways(packets, keys=None):
    """process_packets on the packets and process_frames on their host frames: (frames, bytes, enc-carrying trace text) of each."""
    frames, tabs, bits = host_frames_of(packets)
    res = []
    for use_frames in (False, True):
        out = io.StringIO()
        m = fsm.fsm(out=out)
        if keys:
            m.set_keys(*keys)
        if use_frames:
            table, data = m.process_frames(frames)
        else:
            table, data = m.process_packets(merged(tabs), bits[0], bits[1])
        # the state afterwards: one more frame of each direction through the old entry must come out the same
        tail = [m.process_bits(synth.frame_bits([0x30, 0x04, 0x26, 0xEE]), 1), m.process_bits(synth.frame_bits([0x04, 0xDA, 0x17]), 0)]
        res.append((table, data, out.getvalue(), [None if s is None else (s.name(), s.all_bytes()) for s in tail]))
    (t0, d0, x0, s0), (t1, d1, x1, s1) = res
    assert t0.tobytes() == t1.tobytes(), 'frame tables (cmd, split, flags, n_enc)'
    assert d0.tobytes() == d1.tobytes(), 'bytes'
    assert x0 == x1, 'dispatched trace text (messages, ciphertext lines, commands)'
    assert s0 == s1, 'state afterwards'
    return t1, x1


def packets_from_trace(path):
    frames, text = synth.frames_from_trace(path)
    return [(d, bits + [0] if len(bits) == 7 else bits) for d, bits in frames], text


def test_process_frames_ultralight_golden():
    packets = Case('fx_ultralight_txn').packets
    out = io.StringIO()
    frames, _, _ = host_frames_of(packets)
    table, _ = fsm.fsm(out=out).process_frames(frames)
    assert out.getvalue().rstrip('\n') == open(GOLD_UL).read().rstrip('\n')
    assert len(table) == 19 and (table['cmd'] >= 0).all()
    both_ways(packets)


def test_process_frames_classic_1k_with_crypto1():
    packets, text = packets_from_trace(GOLD_1K)
    out = io.StringIO()
    frames, _, _ = host_frames_of(packets)
    table, _ = fsm.fsm(out=out).process_frames(frames)
    assert out.getvalue().rstrip('\n') == text.rstrip('\n')
    assert len(table) == 202 and text.count('AR OK') == 16 and text.count('AT OK') == 16
    assert int(((table['flags'] & fsm.FRAME_ENCRYPTED) != 0).sum()) > 100
    both_ways(packets)


def test_process_frames_wrong_key():
    packets, _ = packets_from_trace(GOLD_1K)
    _, text = both_ways(packets, keys=([0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], [0xFF] * 6))
    assert 'AR OK' not in text and 'PARITY ERROR' in text


def test_process_frames_crafted():
    table, text = both_ways(crafted_oracle_packets())
    assert 'EXTRA ERROR' in text and 'MANY MORE ERROR' in text and 'PARITY ERROR' in text
    assert (table['cmd'] == fsm.NFC_CMD_PARITY_ERROR).any() and (table['cmd'] >= 0).any()


def test_process_frames_refuses_a_cut_frame():
    frames, _, _ = host_frames_of([(1, synth.frame_bits([0x26, 0x00]))])
    frames.table['flags'] |= CUT
    with pytest.raises(ValueError):
        fsm.fsm(out=io.StringIO()).process_frames(frames)


def test_new_names_are_declared_and_bound():
    names = ['nfc_get_frame_counts', 'nfc_read_frames', 'nfc_read_frame_bytes', 'nfc_multi_fetch_frames', 'nfc_host_frames', 'nfc_fsm_process_frames']
    assert set(names) <= set(_lib.SYMBOLS)
    assert RAW.itemsize == 32 and _lib.ABI_VERSION == 4


# ---- GPU suite -----------------------------------------------------------------------------------------------------------------
def frames_and_twin(ctx):
    """ctx.frames() and the host twin of the same context's packets: (frames, twin, tabs, bits)."""
    got = ctx.frames()
    tabs = [ctx.packet_table(t) for t in (0, 1)]
    bits = [ctx.packet_bits(t) for t in (0, 1)]
    parts = [api.host_frames(tabs[t], bits[t], t) for t in (0, 1)]
    want = api.NfcFrames([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts])
    nf, nb = ctx.frame_counts()
    c = ctx.counts()
    assert nf.tolist() == [len(tabs[0]), len(tabs[1])] == [int(c.n_packets[0]), int(c.n_packets[1])]
    assert nb.tolist() == [len(want.bytes[0]), len(want.bytes[1])]
    return got, want, tabs, bits


@pytest.fixture
def ctx():
    c = api.NfcContext(hi_val=1.1, input_kind=api.NFC_IN_IQ_F32)
    yield c
    c.close()


@pytest.mark.gpu
def test_gpu_crafted_in_one_push_packed_source(ctx):
    ctx.push(crafted_iq())
    got, want, tabs, bits = frames_and_twin(ctx)
    assert sum(len(t) for t in tabs) == 373
    assert_coverage(tabs, bits, got.records)
    assert_frames_equal(got, want)
    check_against_restatement(got, tabs, bits)


@pytest.mark.gpu
def test_gpu_first_seed_alone_small_stage_source(ctx):
    ctx.push(crafted_iq(SEEDS[:1]))
    got, want, tabs, bits = frames_and_twin(ctx)
    assert sum(len(t) for t in tabs) > 80 and set((np.concatenate(tabs)['n_bits'] % 9).tolist()) == set(range(9))
    assert_frames_equal(got, want)


@pytest.mark.gpu
def test_gpu_crafted_in_pieces_of_50001(ctx):
    iq = crafted_iq()
    n_frames, flags = 0, []
    for i in range(0, len(iq), 2 * 50001):   # cuts inside frames: the open packet's bits are carried into the next batch
        ctx.push(iq[i:i + 2 * 50001])
        got, want, tabs, bits = frames_and_twin(ctx)
        assert_frames_equal(got, want)
        n_frames += len(got.table)
        flags.append(got.table['flags'])
    assert n_frames == 373
    whole = host_frames_of(crafted_oracle_packets())[0].table['flags']
    assert np.concatenate(flags).tolist() == whole.tolist()


@pytest.mark.gpu
def test_gpu_submit_device_and_wait(ctx):
    iq = crafted_iq()
    buf = api.DeviceBuffer(iq)
    try:
        ctx.submit_device(buf, len(iq) // 2)
        ctx.wait()
        got, want, tabs, bits = frames_and_twin(ctx)
        assert len(got.table) == 373
        assert_frames_equal(got, want)
    finally:
        buf.free()


@pytest.mark.gpu
@pytest.mark.parametrize('tagname,rate', [('frames_0p5', 2e6), ('0p5', 2e6)])
def test_gpu_push_edges_on_the_decoder_vectors(tagname, rate):
    # the reference's decoder-only vectors as a caller's own transition list (nfc_push_edges: decode and framing alone), both routes,
    # in two calls: whole frames, and 6 000 random (cur, d) pairs with every error branch (packets of every odd length)
    z = np.load(os.path.join(GOLDEN, 'fx_decoder_vectors.npz'))
    parts = []
    for t, c in ((1, 'm'), (0, 't')):
        d = z['d' + c + '_' + tagname] if 'd' + c + '_' + tagname in z else z['d_' + tagname]
        e = np.zeros(len(d), _lib.EDGE_DTYPE)
        e['v'], e['d'], e['t'] = z['cur' + c + '_' + tagname], d, t
        parts.append(e)
    e = np.concatenate(parts)
    e['idx'] = np.arange(len(e), dtype=np.uint64)
    seen = 0
    with api.NfcContext(samp_rate=rate, hi_val=1.1) as c:
        for piece in (e[:len(e) // 3], e[len(e) // 3:]):
            c.push_edges(piece)
            got, want, tabs, bits = frames_and_twin(c)
            assert_frames_equal(got, want)
            check_against_restatement(got, tabs, bits)
            seen += len(got.table)
    assert seen > 0   # (not vacuous: the equalities above are the check)


@pytest.mark.gpu
def test_gpu_ultralight_iq_to_trace_through_frames(ctx):
    iq = np.load(os.path.join(GOLDEN, 'fx_ultralight_iq.npz'))['iq']
    ctx.push(iq)
    got, want, _, _ = frames_and_twin(ctx)
    assert_frames_equal(got, want)
    out = io.StringIO()
    table, _ = fsm.fsm(out=out).process_frames(got)
    assert out.getvalue().rstrip('\n') == open(GOLD_UL).read().rstrip('\n')
    assert len(table) == 19 and (table['cmd'] >= 0).all()
    assert got.crc_ok_mask().sum() > 0


@pytest.mark.gpu
def test_gpu_empty_batches_and_call_order(ctx):
    with pytest.raises(api.NfcError):
        ctx.frames()                                  # before any batch: NFC_ERR_STATE
    ctx.push(np.zeros(0, np.float32))                 # an empty batch
    nf, nb = ctx.frame_counts()
    assert nf.tolist() == [0, 0] and nb.tolist() == [0, 0] and len(ctx.frames().table) == 0
    ctx.push(synth.iq_from_profile(np.ones(5000, np.float32)))   # a batch with no packets
    nf, nb = ctx.frame_counts()
    assert nf.tolist() == [0, 0] and nb.tolist() == [0, 0] and len(ctx.frames().table) == 0


def _status(ctx):
    nf = np.zeros(2, np.uint64)
    return ctx.L.nfc_get_frame_counts(ctx.h, nf.ctypes.data, nf.ctypes.data)


@pytest.mark.gpu
def test_gpu_no_batch_is_a_state_error():
    c = api.NfcContext(hi_val=1.1, input_kind=api.NFC_IN_IQ_F32)
    try:
        assert _status(c) == -4                       # NFC_ERR_STATE
        got = C_size()
        assert c.L.nfc_read_frames(c.h, 0, None, 0, got) == -4
        assert c.L.nfc_read_frame_bytes(c.h, 0, 0, None, None, 0, got) == -4
    finally:
        c.close()


def C_size():
    return ctypes.byref(ctypes.c_size_t(0))


# ---- multi-stream ----------------------------------------------------------------------------------------------------------------
def multi_streams():
    """Five ragged streams: the four seeds of the crafted capture, each alone, and the Ultralight fixture."""
    s = [crafted_iq((seed,)) for seed in SEEDS]
    s.append(np.load(os.path.join(GOLDEN, 'fx_ultralight_iq.npz'))['iq'])
    return s


def twin_of_stream(st, allow_truncated=False):
    tabs = [st.packet_table(t, allow_truncated) if allow_truncated else st.packet_table(t) for t in (0, 1)]
    bits = [st.packet_bits(t, allow_truncated) if allow_truncated else st.packet_bits(t) for t in (0, 1)]
    parts = [api.host_frames(tabs[t], bits[t], t) for t in (0, 1)]
    return api.NfcFrames([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts])


def check_multi(m, K):
    fr = m.fetch_frames()
    assert m.stats().n_reads_device == 0
    mask = fr.crc_ok_mask()
    total = 0
    for k in range(K):
        got = fr.frames_of(k)
        total += len(got.table)
    assert m.stats().n_reads_device == 0             # fetch_frames and every accessor: host memory only
    for k in range(K):
        assert_frames_equal(fr.frames_of(k), twin_of_stream(m.stream(k)))
    for t in (0, 1):
        assert mask[t].tolist() == ((fr.frames[t]['flags'] & CRC_OK) != 0).tolist()
        assert len(fr.stream_of(t)) == len(fr.frames[t])
    return fr, total


@pytest.mark.gpu
def test_gpu_multi_one_push_and_in_pieces():
    streams = multi_streams()
    K, longest = len(streams), max(len(s) for s in streams) // 2
    with api.NfcMultiContext(K, longest, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as m:
        m.push(streams)
        fr, total = check_multi(m, K)
        assert fr.n_launches == 2 and fr.bytes_copied > 0
        single = [len(oracle_packets_of(k)) for k in range(K)]
        assert [len(fr.frames_of(k).table) for k in range(K)] == single and total == sum(single)
        assert fr.crc_ok_mask()[0].sum() >= 4 and fr.crc_ok_mask()[1].sum() >= 4
    piece = 30001
    with api.NfcMultiContext(K, piece, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as m:
        done, total = 0, 0
        while done < longest:
            m.push([s[2 * done:2 * (done + piece)] for s in streams])
            total += check_multi(m, K)[1]
            done += piece
        assert total == sum(single)


def oracle_packets_of(k):
    """Stream k of multi_streams() through the C restatement of the reference path, once."""
    if ('stream', k) not in _cache:
        from oracle import c_oracle
        o = c_oracle.COracle(hi_val=1.1)
        o.push_iq(multi_streams()[k])
        _cache[('stream', k)] = [(t, b) for t, b in o.packets() if b]
        o.close()
    return _cache[('stream', k)]


@pytest.mark.gpu
def test_gpu_multi_fetch_and_fetch_frames_keep_each_other():
    streams = multi_streams()
    K, longest = len(streams), max(len(s) for s in streams) // 2
    with api.NfcMultiContext(K, longest, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as m:
        m.push(streams)
        f = m.fetch(api.NFC_MULTI_FETCH_PACKETS, copy=False)
        before = [a.copy() for a in f.packet_table + f.packet_bits]
        fr = m.fetch_frames(copy=False)
        kept = [a.copy() for a in fr.frames + fr.bytes + fr.par]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(f.packet_table + f.packet_bits, before))   # the fetch's views survived
        assert m.stream(0).packet_table(0).tobytes() == f.packet_table_of(0, 0).tobytes() and m.stats().n_reads_device == 0   # and the readers' host copy
        m.fetch(api.NFC_MULTI_FETCH_ALL, copy=False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fr.frames + fr.bytes + fr.par, kept))      # the frames' views survived a fetch
        for k in range(K):
            assert_frames_equal(fr.frames_of(k), twin_of_stream(m.stream(k)))


@pytest.mark.gpu
def test_gpu_multi_before_a_push_and_with_nothing_stored():
    with api.NfcMultiContext(3, 4096, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as m:
        with pytest.raises(api.NfcError):
            m.fetch_frames()                          # no completed push: NFC_ERR_STATE
        m.push([synth.iq_from_profile(np.ones(4096, np.float32))] * 3)
        fr = m.fetch_frames()
        assert fr.n_launches == 0 and fr.bytes_copied == 0 and all(len(a) == 0 for a in fr.frames + fr.bytes + fr.par)
        assert all(o.tolist() == [0] * 4 for o in fr.frame_off + fr.byte_off)
        assert len(fr.frames_of(2).table) == 0


@pytest.mark.gpu
def test_gpu_multi_truncated_bit_slab_cuts_frames_and_nothing_else():
    streams = multi_streams()
    K, longest = len(streams), max(len(s) for s in streams) // 2
    cap_bits = 900   # the crafted streams close 1 400 bits and more per type, the Ultralight fixture 806 and 392 (the C oracle's counts)
    m = api.NfcMultiContext(K, longest, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, cap_packet_bits=cap_bits, lib_path=_lib.hooks_path())
    guards = m.L.nfc_debug_multi_guards
    guards.argtypes = [ctypes.c_void_p]
    try:
        m.push(streams)
        flags = m.counts_all()['flags']
        assert (flags[:4] & api.NFC_MULTI_TRUNC_BITS).all() and not flags[4] & api.NFC_MULTI_TRUNC_BITS
        fr = m.fetch_frames()
        assert guards(m.h) == 0   # the guard bytes behind every slab row and every packed section
        assert_frames_equal(fr.frames_of(4), twin_of_stream(m.stream(4)))   # the stream that was not cut
        whole = [host_frames_of(oracle_packets_of(k))[0] for k in range(4)]
        for k in range(4):
            got = fr.frames_of(k)
            for t in (0, 1):
                recs, ref = got.records[t], whole[k].records[t]
                assert len(recs) == len(ref) and recs['n_bits'].tolist() == ref['n_bits'].tolist()
                ends = np.cumsum(ref['n_bits'].astype(np.int64))
                cut = ends > cap_bits
                assert cut.any() and not cut.all()
                assert ((recs['flags'] & CUT) != 0).tolist() == cut.tolist()
                assert (recs['flags'][cut] == CUT).all() and (recs['n_bytes'][cut] == 0).all()
                keep = ~cut
                for name in ('byte_off', 'n_bytes', 'flags', 'type', 'reserved'):   # frames before the cut are exact (idx: the twin's is a list position)
                    assert recs[name][keep].tolist() == ref[name][keep].tolist(), name
                nb = int(ref['n_bytes'][keep].sum())
                assert len(got.bytes[t]) == nb and got.bytes[t].tobytes() == whole[k].bytes[t][:nb].tobytes()
                assert got.par[t].tobytes() == whole[k].par[t][:nb].tobytes()
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_decode_many_attaches_frames():
    from usrp_nfc_amd import decoder
    iq = np.load(os.path.join(GOLDEN, 'fx_ultralight_iq.npz'))['iq']
    srcs = [iq.view(np.complex64), crafted_iq(SEEDS[:1]).view(np.complex64)]
    plain = decoder.decode_many(srcs, fsm_factory=lambda: fsm.fsm(out=io.StringIO()), max_push_samples=40000)
    backs = decoder.decode_many(srcs, fsm_factory=lambda: fsm.fsm(out=io.StringIO()), max_push_samples=40000, frames=True)
    assert not hasattr(plain[0], 'frames')                     # the default leaves the backgrounds as they were
    for b, p in zip(backs, plain):
        assert b.packets == p.packets
        table = np.concatenate([f.table for f in b.frames])
        assert table['n_bits'].tolist() == [len(bits) for _, bits in b.packets] and table['type'].tolist() == [t for t, _ in b.packets]
    out = io.StringIO()
    m = fsm.fsm(out=out)
    for f in backs[0].frames:
        m.process_frames(f)
    assert out.getvalue().rstrip('\n') == open(GOLD_UL).read().rstrip('\n')
