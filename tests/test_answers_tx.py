"""What the streams of a multi-stream context answer, transmitted: nfc_multi_transmit_device (include/nfc_amd.h; csrc/answers_tx.hip.h,
DESIGN.md 8m) behind NfcMultiContext.transmit, against its twin on the CPU (nfc_host_answers_tx, which tests/test_answers_tx_host.py pins
to the reference's TX vectors and the encoders) fed the very answers the push produced: the same bytes, whole and in pieces."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_emulate import _replay_cards, _reader_side_streams
from usrp_nfc_amd import emulate, tx

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
SENTINEL = np.complex64(7 - 3j)
pytestmark = pytest.mark.gpu


def _roles(cards):
    return [None if c is None else c.role for c in cards]


def _context(cards, max_push, **kw):
    from usrp_nfc_amd import _lib, api
    m = api.NfcMultiContext(len(cards), max_push, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, lib_path=_lib.hooks_path(), **kw)
    m.emulate(cards)
    m.L.nfc_debug_multi_guards.argtypes = [ctypes.c_void_p]
    return m


def _buffer(m, samples):
    """a device buffer of `samples` complex64 and 64 sentinels behind them"""
    from usrp_nfc_amd import api
    return api.DeviceBuffer(np.full(samples + 64, SENTINEL, np.complex64), m.device)


def _push_transmit(m, pieces, roles, pending, cap, **kw):
    """one push of `pieces` (an interleaved float32 array per stream) and one transmit into a buffer of `cap` samples with sentinels behind
    -> (the device's layout, first_sample, n_samples, the twin's layout, the twin's pending)"""
    n = m.push(pieces)
    buf = _buffer(m, cap)
    try:
        tc = m.transmit(out=(buf.ptr, cap), **kw)
        cm, an = m.fetch_commands(), m.fetch_answers()
        got = buf.download().view(np.complex64)
    finally:
        buf.free()
    answers, idx = emulate.tx_inputs(cm, an)
    want, first, ns, pend = emulate.host_transmit(answers, idx, roles, cm.raw.base, n, pending, **kw)
    assert first.tolist() == tc.first_sample.tolist() and ns.tolist() == tc.n_samples.tolist()
    assert tc.total == len(want) <= cap
    assert (got[tc.total:] == SENTINEL).all()   # nothing beyond the layout is touched
    return got[:tc.total], first, ns, want, pend, an


def _pend_bytes(m, K):
    return b''.join(bytes(bytearray(m.tx_state(k))) for k in range(K))


def _cut(streams, cuts, p):
    edges = [[0] + list(c) + [len(s) // 2] for s, c in zip(streams, cuts)]
    return [s[2 * e[p]:2 * e[p + 1]] if p + 1 < len(e) else s[:0] for s, e in zip(streams, edges)], max(len(e) for e in edges) - 1


def _piece_cuts(idx0, idx1, names, delay=172):
    """tests/test_emulate.py's cuts of the three streams, from the two captures' frame idx and stream 0's command names: one inside an
    answer's interval, one between an idx and its S, and an empty push"""
    auth, nrar = names.index(14), names.index(17)
    cuts0 = sorted([int(idx0[auth]) + 60, int(idx0[nrar]) + 60, int(idx0[1]) + delay + 100, int(idx0[3]) + 20])
    cuts0.insert(2, cuts0[1])   # the empty push
    return [cuts0, [int(idx1[2]) + 60, int(idx1[4]) + delay + 33], []]


# ---- 7. device equals twin, whole and in pieces ----
def test_device_equals_the_twin_whole_and_in_pieces():
    from usrp_nfc_amd import synth
    streams, cards = _reader_side_streams(), _replay_cards()
    roles, kw = _roles(cards), dict(delay_us=86.43, samp_rate=2e6, align_samples=8)
    max_push = max(len(s) for s in streams) // 2
    cap = sum(len(s) // 2 for s in streams) + 64
    with _context(cards, max_push) as m:
        got, first, ns, want, pend, an = _push_transmit(m, streams, roles, None, cap, **kw)
        assert an.n.tolist() == [12, 9, 0]
        assert got.tobytes() == want.tobytes()
        assert ns.tolist() == [len(s) // 2 for s in streams]   # (stream 2 heard nothing and transmits nothing: no samples)
        assert m.L.nfc_debug_multi_guards(m.h) == 0
        assert _pend_bytes(m, 3) == pend.tobytes() and pend['n_bits'].tolist() == [162, 162, 0]   # both tags' last answers, 18 bytes, outlast their captures
        whole = [got[int(f):int(f) + int(n)] for f, n in zip(first, ns)]
        cm = m.fetch_commands()
        # ... so an unmodulated tail follows, in a push of its own: the answer is finished there and nothing is pending any more
        tail = [synth.iq_from_profile(np.ones(4000, np.float32)), synth.iq_from_profile(np.ones(4000, np.float32)), streams[2]]
        got, first, ns, want, pend, _ = _push_transmit(m, tail, roles, pend, cap, **kw)
        assert got.tobytes() == want.tobytes() and not pend.tobytes().strip(b'\0') and _pend_bytes(m, 3) == pend.tobytes()
        whole = [np.concatenate([w, got[int(f):int(f) + int(n)]]) for w, f, n in zip(whole, first, ns)]
        assert whole[0][len(streams[0]) // 2:].real.max() == 1.0   # (the rest of that answer)
        for k in (0, 1):   # twelve and nine answers are on the air: the tag's load modulation over an idle level of 0
            assert whole[k].real.max() == 1.0 and whole[k].real.min() == 0.0 and not whole[k].imag.any()
        # in pieces: tests/test_emulate.py's cuts, one inside an answer's interval, one between an idx and its S, and an empty push
        idx0, idx1 = (cm.raw.frames_of(k).table['idx'].astype(np.int64) for k in (0, 1))
        cuts = _piece_cuts(idx0, idx1, cm.commands_of(0)[0]['cmd'].tolist())
        m.reset()
        assert not _pend_bytes(m, 3).strip(b'\0')
        parts, pend, n_push = [[] for _ in streams], None, _cut(streams, cuts, 0)[1]
        seen_pending = 0
        for p in range(n_push):
            pieces, _ = _cut(streams, cuts, p)
            got, first, ns, want, pend, _ = _push_transmit(m, pieces, roles, pend, cap, **kw)
            assert got.tobytes() == want.tobytes(), p
            assert _pend_bytes(m, 3) == pend.tobytes(), p
            seen_pending += int((pend['n_bits'] != 0).sum())
            for k in range(3):
                parts[k].append(got[int(first[k]):int(first[k]) + int(ns[k])])
        assert seen_pending >= 3 and n_push == 6
        got, first, ns, want, pend, _ = _push_transmit(m, tail, roles, pend, cap, **kw)
        assert got.tobytes() == want.tobytes() and _pend_bytes(m, 3) == pend.tobytes()
        for k in range(3):
            parts[k].append(got[int(first[k]):int(first[k]) + int(ns[k])])
        for k in range(3):
            assert np.concatenate(parts[k]).tobytes() == whole[k].tobytes(), k
        assert not pend.tobytes().strip(b'\0')   # the final pending is none
        assert m.L.nfc_debug_multi_guards(m.h) == 0


def test_a_stream_that_hears_nothing_is_all_idle_level(tmp_path):
    # stream 2 of the three, the reader card, given an unmodulated carrier: every sample is the reader's idle level 1; the buffer is
    # the result's own, and a stream's real part goes to a WAV through the recording kernel
    import wave
    from usrp_nfc_amd import synth
    streams, cards = _reader_side_streams(), _replay_cards()
    streams[2] = synth.iq_from_profile(np.ones(5000, np.float32))
    with _context(cards, max(len(s) for s in streams) // 2) as m:
        m.push(streams)
        tc = m.transmit(delay_us=86.43)
        try:
            s2 = tc.download(2)
            assert len(s2) == 5000 and s2.tobytes() == np.ones(5000, np.complex64).tobytes()
            s0 = tc.download(0)
            assert s0.real.min() == 0.0 and s0.real.max() == 1.0 and all(int(f) % 8 == 0 for f in tc.first_sample)
            assert tc.record(0, str(tmp_path / 'tx.wav')) == len(s0)
            with wave.open(str(tmp_path / 'tx.wav')) as w:
                pcm = np.frombuffer(w.readframes(w.getnframes()), '<i2')
            assert w.getframerate() == 2000000 and pcm.tobytes() == (s0.real * 32767).astype('<i2').tobytes()
        finally:
            tc.free()


# ---- 8. across waves and tiles ----
@pytest.mark.parametrize('align,out_rate', [(1, 2e6), (8, 2e6), (1, 5e6), (8, 5e6)])
def test_130_ragged_streams_equal_the_twin(align, out_rate):
    base_streams, base_cards = _reader_side_streams()[:2], _replay_cards()[:2]
    K = 130
    streams = [base_streams[k % 2][:2 * (len(base_streams[k % 2]) // 2 - (k * 397) % 9000)] for k in range(K)]
    cards = [None if k % 3 == 2 else base_cards[k % 2] for k in range(K)]
    roles = _roles(cards)
    kw = dict(samp_rate=out_rate, in_rate=2e6, delay_us=86.43, align_samples=align)
    cap = int(sum(len(s) // 2 for s in streams) * out_rate / 2e6) + 8 * K + 64
    with _context(cards, max(len(s) for s in streams) // 2) as m:
        got, first, ns, want, pend, an = _push_transmit(m, streams, roles, None, cap, **kw)
        assert got.tobytes() == want.tobytes()
        assert int(an.n.sum()) > 300 and all(int(ns[k]) == 0 for k in range(2, K, 3)) and len({int(n) for n in ns}) > 40
        assert _pend_bytes(m, K) == pend.tobytes()
        assert m.L.nfc_debug_multi_guards(m.h) == 0
        assert sum(int(f) % 1024 != 0 for f, n in zip(first, ns) if n) > 40   # streams begin inside tiles: a tile meets two of them


# ---- 9. the carrier ----
def test_carrier_is_k_tx_render_s():
    streams, cards = _reader_side_streams(), _replay_cards()
    roles = _roles(cards)
    first_index, amp, freq = 1 << 40, 0.5, 13.56e6
    kw = dict(delay_us=86.43, samp_rate=2e6, carrier=True, amp=amp, freq=freq, first_index=first_index)
    cap = sum(len(s) // 2 for s in streams) + 64
    with _context(cards, max(len(s) for s in streams) // 2) as m:
        got, first, ns, want, pend, an = _push_transmit(m, streams, roles, None, cap, **kw)
        cm = m.fetch_commands()
        answers, idx = emulate.tx_inputs(cm, an)
        levels = emulate.host_transmit(answers, idx, roles, cm.raw.base, [len(s) // 2 for s in streams], **dict(kw, carrier=False))[0].real
        inc = np.uint64(int((freq / 2e6 - np.floor(freq / 2e6)) * 2.0 ** 64))
        for k in (0, 1):
            f, n = int(first[k]), int(ns[k])
            with np.errstate(over='ignore'):
                ph = ((np.uint64(first_index) + np.arange(n, dtype=np.uint64)) * inc) >> np.uint64(40)
            ref = levels[f:f + n].astype(np.float64) * amp * np.exp(2j * np.pi * ph.astype(np.float64) / 2.0 ** 24)
            assert np.abs(got[f:f + n] - ref).max() <= 1.5e-7 * amp
            assert np.abs(got[f:f + n] - want[f:f + n]).max() <= 1.5e-7 * amp   # the twin's angle in double
        # one answer's interval, bit for bit, against k_tx_render in the same process: one device function, one result
        j = 4
        s = int(idx[0][j]) + 172
        one = tx.render(tx.encode_runs(tx.NFC_TX_MANCHESTER, an.bits(0, j)), 2e6, carrier=True, freq=freq, amp=amp, first_index=first_index + s)
        own = min(len(one), int(idx[0][j + 1]) - s)   # (what the next answered command leaves of it)
        assert own > 100 and got[int(first[0]) + s:int(first[0]) + s + own].tobytes() == one[:own].tobytes()


# ---- 10. round trip in HBM ----
def test_round_trip_in_hbm():
    from usrp_nfc_amd import api, synth
    reader = emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_ultralight.json'), emulate.NFC_EMU_CARD)[1]
    capture = synth.iq_from_profile(synth.modulation_profile(synth.txn_frames(directions=(synth.TAG,)), gap_us=2500))
    n = len(capture) // 2
    kw = dict(delay_us=86.43, samp_rate=2e6, carrier=True, amp=0.5)
    with _context([reader], n) as m:
        m.push([capture])
        tc = m.transmit(**kw)
        try:
            cm, an = m.fetch_commands(), m.fetch_answers()
            answers, idx = emulate.tx_inputs(cm, an)
            n_ans = int(an.n[0])
            assert n_ans >= 1
            # through the twin's schedule: no answer is cut (the next answered command closes behind every answer's end)
            starts = [int(i) + 172 for i in idx[0]]
            lens = [tx.sample_count(tx.encode_runs(tx.NFC_TX_MILLER, an.bits(0, j)), 2e6) for j in range(n_ans)]
            assert all(starts[j] + lens[j] <= (int(idx[0][j + 1]) if j + 1 < n_ans else n) for j in range(n_ans))
            _, _, _, pend = emulate.host_transmit(answers, idx, [reader.role], cm.raw.base, [n], **kw)
            assert int(pend[0]['n_bits']) == 0
            # the stream's span of dev_out straight into a second context, from the device pointer
            with api.NfcMultiContext(1, n, samp_rate=2e6, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, reader=True, tag=False) as rx:
                rx.push_device(tc.wait().buf, tc.first_sample[:1], tc.n_samples[:1])
                fr = rx.fetch_frames()
        finally:
            tc.free()
        got = fr.frames[1]
        assert len(got) == n_ans and len(fr.frames[0]) == 0
        rec, _, air, par = an.answers_of(0)
        for j in range(n_ans):
            o, nb = int(rec[j]['byte_off']), int(rec[j]['n_bytes'])
            g0, gn = int(got[j]['byte_off']), int(got[j]['n_bytes'])
            assert gn == nb and fr.bytes[1][g0:g0 + gn].tolist() == air[o:o + nb].tolist(), j
            if int(rec[j]['n_bits']) != 7:
                assert fr.par[1][g0:g0 + gn].tolist() == par[o:o + nb].tolist(), j


# ---- 11. state and errors on the device ----
def test_state_and_errors():
    from usrp_nfc_amd import api, synth
    streams, cards = _reader_side_streams(), _replay_cards()
    roles, kw = _roles(cards), dict(delay_us=86.43, samp_rate=2e6, align_samples=8)
    cap = 2 * sum(len(s) // 2 for s in streams) + 64
    with _context(cards, max(len(s) for s in streams) // 2) as m:
        with pytest.raises(api.NfcError, match='status -4'):   # no completed push
            m.transmit(**kw)
        cm_idx = None
        m.push(streams)
        launches = int(m.stats().n_launches)
        buf = _buffer(m, cap)
        try:
            # argument errors come before the device is touched
            for bad, name in [(dict(align_samples=24), 'align_samples'), (dict(samp_rate=0.0), 'samp_rate'), (dict(samp_rate=2e9), 'samp_rate'),
                              (dict(samp_rate=1e6, in_rate=70001e6), 'rate_den'), (dict(samp_rate=70001.0, in_rate=1.0), 'rate_num'), (dict(_reserved=1), 'reserved')]:
                with pytest.raises(api.NfcError, match=name):
                    m.transmit(out=(buf.ptr, cap), **dict(kw, **bad))
            with pytest.raises(api.NfcError, match='dev_out'):
                m.transmit(out=(buf.ptr.value + 16, cap - 2), **kw)
            with pytest.raises(api.NfcError, match='cap_samples'):
                m.transmit(out=(buf.ptr, 1000), **kw)
            assert int(m.stats().n_launches) == launches
            assert (buf.download().view(np.complex64) == SENTINEL).all()
            m.transmit(out=(buf.ptr, cap), **kw)
            assert int(m.stats().n_launches) == launches + 2
            with pytest.raises(api.NfcError, match='status -4'):   # once per push
                m.transmit(out=(buf.ptr, cap), **kw)
        finally:
            buf.free()
        # a pending answer handed over: stream 0 is cut inside its second answer; stream 2, a reader given an idle carrier of the same
        # length, takes stream 0's pending entry and finishes that answer in its next span
        cm = m.fetch_commands()
        cm_idx = cm.raw.frames_of(0).table['idx'].astype(np.int64)
        cut = int(cm_idx[1]) + 172 + 100
        idle = synth.iq_from_profile(np.ones(len(streams[0]) // 2, np.float32))
        three = [streams[0], streams[1][:0], idle]
        m.reset()
        first_half = [s[:2 * cut] for s in three]
        got, first, ns, want, pend, _ = _push_transmit(m, first_half, roles, None, cap, **kw)
        assert got.tobytes() == want.tobytes()
        st0 = m.tx_state(0)
        assert int(st0.n_bits) == int(pend[0]['n_bits']) != 0 and int(st0.start) == int(cm_idx[1]) + 172 and int(m.tx_state(2).n_bits) == 0
        m.set_tx_state(2, st0)
        pend[2] = pend[0]
        assert _pend_bytes(m, 3) == pend.tobytes()
        got, first, ns, want, pend, _ = _push_transmit(m, [s[2 * cut:] for s in three], roles, pend, cap, **kw)
        assert got.tobytes() == want.tobytes()
        s2 = got[int(first[2]):int(first[2]) + int(ns[2])].real
        assert s2[:400].min() == 0.0 and s2[:400].max() == 1.0 and (s2[4000:] == 1.0).all()   # the rest of a tag's answer over a reader's idle level
        assert int(m.tx_state(2).n_bits) == 0
        # reset(k) clears the stream's pending entry
        m.reset()
        _push_transmit(m, first_half, roles, None, cap, **kw)
        assert int(m.tx_state(0).n_bits) != 0
        m.reset(0)
        assert int(m.tx_state(0).n_bits) == 0
        with pytest.raises(api.NfcError, match='status -4'):   # a reset since the push
            m.transmit(**kw)
        with pytest.raises(api.NfcError, match='n_bits'):
            bad = m.tx_state(0)
            bad.n_bits = 10
            m.set_tx_state(0, bad)
        # tracking off
        m.reset()
        m.track_commands(False)
        m.push(streams)
        with pytest.raises(api.NfcError, match='status -4'):
            m.transmit(**kw)
    with api.NfcMultiContext(1, 1000) as plain:   # no stream holds a card
        plain.track_commands()
        plain.push([np.zeros(2000, np.float32)])
        with pytest.raises(api.NfcError, match='status -4'):
            plain.transmit(**kw)
        assert int(plain.tx_state(0).n_bits) == 0


# ---- 12. untouched ----
def test_a_context_that_never_transmits_is_untouched():
    # PARENT: what the parent commit reports for this very context and push -- recorded from a run of the parent's library on the same
    # machine, in the same session, as the run of this test that first passed (launches, copies, the tracking buffer's size, live handles)
    from usrp_nfc_amd import _lib
    L = _lib.load(_lib.hooks_path())
    L.nfc_debug_live_resources.argtypes = [ctypes.POINTER(ctypes.c_uint64 * 4)]
    L.nfc_debug_live_resources.restype = None
    live = lambda: (lambda o: (L.nfc_debug_live_resources(ctypes.byref(o)), list(o))[1])((ctypes.c_uint64 * 4)())
    before = live()
    streams, cards = _reader_side_streams(), _replay_cards()
    with _context(cards, max(len(s) for s in streams) // 2) as m:
        m.push(streams)
        cm, an = m.fetch_commands(), m.fetch_answers()
        s = m.stats()
        got = dict(n_launches=int(s.n_launches), cmd_launches=int(cm.n_launches), n_fetches=int(s.n_fetches), n_reads_device=int(s.n_reads_device),
                   n_samples=int(s.n_samples), bytes_in=int(s.bytes_in), cmd_bytes_copied=int(cm.bytes_copied), n_answers=int(an.n_answers),
                   live=[int(a - b) for a, b in zip(live(), before)])
    print('untouched:', got)
    assert got == PARENT


PARENT = dict(n_launches=4, cmd_launches=3, n_fetches=0, n_reads_device=0, n_samples=30502, bytes_in=244016, cmd_bytes_copied=4768, n_answers=21, live=[29, 6, 6, 1])
