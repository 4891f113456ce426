"""What the streams answer as TX samples, on the CPU: nfc_host_answers_tx (include/nfc_amd.h; csrc/answers_tx.hip.h), the twin
of nfc_multi_transmit_device, behind emulate.host_transmit.  No GPU.  The yardsticks are the reference's own TX vectors
(tests/golden/fx_tx.json), the pinned encoders (nfc_tx_encode) with nfc_tx_sample_count's rule per run, and a restatement of the schedule
in numpy (`_model`)."""
import json
import os

import numpy as np
import pytest

from usrp_nfc_amd import _lib, emulate, tx

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
TAG, READER = emulate.NFC_EMU_TAG, emulate.NFC_EMU_READER
ENCODING = {TAG: tx.NFC_TX_MANCHESTER, READER: tx.NFC_TX_MILLER}
IDLE = {TAG: 0.0, READER: 1.0}
N_BITS = list(range(1, 9)) + list(range(9, 163, 9))


def pack(bit_lists):
    """answers as host_transmit takes them: (records, air, par) -- a short frame in the low bits of its first byte, else nine bits a byte"""
    rec = np.zeros(len(bit_lists), _lib.EMU_ANSWER_DTYPE)
    air, par = [], []
    for i, bits in enumerate(bit_lists):
        n = len(bits)
        rec[i]['byte_off'], rec[i]['n_bits'] = len(air), n
        if n <= 8:
            air.append(sum(b << j for j, b in enumerate(bits))), par.append(0)
            rec[i]['n_bytes'] = 1
        else:
            assert n % 9 == 0
            for q in range(n // 9):
                air.append(sum(bits[9 * q + j] << j for j in range(8))), par.append(bits[9 * q + 8])
            rec[i]['n_bytes'] = n // 9
    return rec, np.array(air, np.uint8), np.array(par, np.uint8)


def wave(role, bits, rate):
    """an answer's levels: nfc_tx_encode's runs, every run with the samples nfc_tx_sample_count gives it, laid end to end"""
    runs = tx.encode_runs(ENCODING[role], bits)
    return np.concatenate([np.full(tx.sample_count(runs[i:i + 1], rate), float(runs[i]['level']), np.float32) for i in range(len(runs))])


def _model(role, entries, n_rx, rate, num=1, den=1, delay=0):
    """the schedule restated: entries (idx, bits) in order over a stream that received n_rx samples -> the real parts of its TX timeline"""
    T = lambda r: r * num // den
    out = np.full(T(n_rx), IDLE[role], np.float32)
    for j, (idx, bits) in enumerate(entries):
        w, s = wave(role, bits, rate), T(idx) + delay
        cut = T(entries[j + 1][0]) if j + 1 < len(entries) else len(out)
        a, b = s, min(s + len(w), cut, len(out))
        if a < b:
            out[a:b] = w[:b - a]
    return out


def one_stream(role, entries, base, n, pending=None, **kw):
    """one push of one stream: the entries (idx, bits) -> (samples, pending)"""
    out, first, ns, pend = emulate.host_transmit([pack([b for _, b in entries])], [[i for i, _ in entries]], [role], [base], [n], pending, **kw)
    assert first.tolist() == [0] and len(out) == int(ns[0])
    return out, pend


def in_pieces(role, entries, cuts, total, **kw):
    """the stream pushed in pieces cut at `cuts`, pending carried through -> (the concatenation, the final pending, samples per piece)"""
    edges, parts, sizes, pend = [0] + list(cuts) + [total], [], [], None
    for a, b in zip(edges[:-1], edges[1:]):
        mine = [(i, bits) for i, bits in entries if a <= i < b]   # a frame that closed at sample idx belongs to the push that holds it
        out, pend = one_stream(role, mine, a, b - a, pend, **kw)
        parts.append(out), sizes.append(len(out))
    return np.concatenate(parts), pend, sizes


# ---- 1. the reference's own samples ----
def test_reference_vectors_come_out_as_one_answer_of_a_one_stream_push():
    cases = json.load(open(os.path.join(GOLD, 'fx_tx.json')))['cases']
    roles = {'manchester': TAG, 'miller': READER}
    seen = {TAG: 0, READER: 0}
    for c in cases:
        n = len(c['bits'])
        if c['encoding'] not in roles or not (1 <= n <= 8 or (n % 9 == 0 and 9 <= n <= 162)):
            continue
        role = roles[c['encoding']]
        want = np.concatenate([np.full(k, float(v), np.float32) for v, k in c['samples_rle']])
        idx, n_rx = 37, 37 + len(want) + 50
        out, pend = one_stream(role, [(idx, c['bits'])], 0, n_rx, samp_rate=c['samp_rate'], align_samples=1)
        assert out.imag.tobytes() == np.zeros(n_rx, np.float32).tobytes()
        assert out.real[idx:idx + len(want)].tobytes() == want.tobytes(), (c['encoding'], c['samp_rate'], n)
        rest = np.concatenate([out.real[:idx], out.real[idx + len(want):]])
        assert rest.tobytes() == np.full(len(rest), IDLE[role], np.float32).tobytes()
        assert int(pend[0]['n_bits']) == 0
        seen[role] += 1
    assert seen[TAG] >= 6 and seen[READER] >= 6 and seen[TAG] + seen[READER] >= 12


# ---- 2. every answer shape against the pinned encoders ----
@pytest.mark.parametrize('rate', [2e6, 4e6, 13.56e6])
@pytest.mark.parametrize('role', [TAG, READER])
def test_every_answer_shape_equals_the_pinned_encoders(role, rate):
    rng = np.random.Generator(np.random.PCG64(int(rate) + role))
    entries, at = [], 100
    for n in N_BITS:
        bits = rng.integers(0, 2, n).tolist()
        entries.append((at, bits))
        at += len(wave(role, bits, rate)) + 7   # the next command closes just behind this answer: uncut
    out, pend = one_stream(role, entries, 0, at + 10, samp_rate=rate, align_samples=1)
    assert out.real.tobytes() == _model(role, entries, at + 10, rate).tobytes()
    assert not out.imag.any() and int(pend[0]['n_bits']) == 0


# ---- 3. pieces equal the whole ----
def _five_answers(rate, num, den):
    rng = np.random.Generator(np.random.PCG64(3))
    shapes, entries, at = [162, 7, 45, 81, 18], [], 1000
    for n in shapes:
        entries.append((at, rng.integers(0, 2, n).tolist()))
        at += 9000
    return entries, at


@pytest.mark.parametrize('carrier', [False, True])
@pytest.mark.parametrize('num,den', [(1, 1), (5, 2), (2, 5)])
def test_pieces_equal_the_whole(num, den, carrier):
    rate, delay = 2e6 * num / den, 173
    kw = dict(samp_rate=rate, in_rate=2e6, delay_us=delay * 1e6 / rate + 1e-4, carrier=carrier, amp=0.5, first_index=1 << 40, align_samples=1)
    assert tx.answers_tx_config(**kw).delay_samples == delay and (tx.answers_tx_config(**kw).rate_num, tx.answers_tx_config(**kw).rate_den) == (num, den)
    entries, total = _five_answers(rate, num, den)
    T = lambda r: r * num // den
    whole, pend = one_stream(READER, entries, 0, total, **kw)
    assert int(pend[0]['n_bits']) == 0 and len(whole) == T(total)
    if not carrier:
        assert whole.real.tobytes() == _model(READER, entries, total, rate, num, den, delay).tobytes()
    else:   # the carrier in float64 (tests/test_tx.py's tolerance for the same arithmetic)
        lvl = _model(READER, entries, total, rate, num, den, delay).astype(np.float64)
        inc = int((13.56e6 / rate - np.floor(13.56e6 / rate)) * 2.0 ** 64)
        ph = np.array([(((1 << 40) + t) * inc % (1 << 64)) >> 40 for t in range(0, len(lvl), 97)], np.float64) / 2.0 ** 24
        ref = lvl[::97] * 0.5 * np.exp(2j * np.pi * ph)
        assert np.abs(whole[::97] - ref).max() <= 1.5e-7 * 0.5

    def rx_at(t):   # the first r with T(r) >= t: where a push must be cut for its span to end at TX index t
        r = (t * den + num - 1) // num
        assert T(r) >= t
        return r
    i0, i1 = entries[0][0], entries[1][0]
    S0, L0 = T(i0) + delay, len(wave(READER, entries[0][1], rate))
    S1 = T(i1) + delay
    cut_sets = {
        'inside an answer': [rx_at(S0 + L0 // 2)],
        'at S': [rx_at(S0)],
        'at S + L': [rx_at(S0 + L0)],
        'at S + L - 1': [rx_at(S0 + L0 - 1)],
        'between idx and S': [i1 + 1],
        'a zero-length push': [5000, 5000],
        'a push of one sample': [rx_at(S0 + 40), rx_at(S0 + 40) + 1],
        'one answer across three pushes': [rx_at(S0 + 10), rx_at(S0 + L0 // 2)],
        'many': [i0 + 1, rx_at(S0 + 3), i1 + 1, rx_at(S1 + 2), entries[4][0], entries[4][0] + 1],
    }
    assert T(i1 + 1) < S1   # (the cut named so really lies between idx and S)
    for name, cuts in cut_sets.items():
        got, pend, sizes = in_pieces(READER, entries, cuts, total, **kw)
        assert sum(sizes) == T(total), name   # the spans tile
        assert got.tobytes() == whole.tobytes(), name
        assert int(pend[0]['n_bits']) == 0 and not pend.tobytes().strip(b'\0'), name
    # ... and the entry carried from a cut inside an answer is that answer
    _, pend = one_stream(READER, entries[:1], 0, rx_at(S0 + L0 // 2), None, **kw)
    assert int(pend[0]['start']) == S0 and int(pend[0]['n_bits']) == 162 and int(pend[0]['role']) == READER
    assert pend[0]['air'].tolist() == pack([entries[0][1]])[1].tolist()


# ---- 4. one at a time ----
def test_a_stream_transmits_one_answer_at_a_time():
    rate = 2e6
    rng = np.random.Generator(np.random.PCG64(4))
    long_bits, short_bits = rng.integers(0, 2, 162).tolist(), rng.integers(0, 2, 18).tolist()
    L = len(wave(TAG, long_bits, rate))
    assert L > 600 + 100   # the first answer is longer than the 300 us between the two commands
    entries = [(1000, long_bits), (1600, short_bits)]
    out, _ = one_stream(TAG, entries, 0, 6000, samp_rate=rate, delay_us=50.0, align_samples=1)
    w0, w1 = wave(TAG, long_bits, rate), wave(TAG, short_bits, rate)
    assert out.real[1100:1600].tobytes() == w0[:500].tobytes()          # cut at T(idx_2)
    assert not out.real[1600:1700].any()                                # idle until S_2
    assert out.real[1700:1700 + len(w1)].tobytes() == w1.tobytes()      # the second is whole
    assert not out.real[1700 + len(w1):].any() and not out.real[:1100].any()
    # an answer whose S is not before its cut contributes nothing: the next command closed inside the delay
    out, _ = one_stream(TAG, [(1000, long_bits), (1050, short_bits)], 0, 6000, samp_rate=rate, delay_us=50.0, align_samples=1)
    assert out.real.tobytes() == _model(TAG, [(1050, short_bits)], 6000, rate, delay=100).tobytes()
    # two entries with equal idx: the earlier one is empty
    out, _ = one_stream(TAG, [(1000, long_bits), (1000, short_bits)], 0, 6000, samp_rate=rate, align_samples=1)
    assert out.real.tobytes() == _model(TAG, [(1000, short_bits)], 6000, rate).tobytes()


# ---- 5. layout, guards, errors ----
def _five_streams():
    rng = np.random.Generator(np.random.PCG64(5))
    bits = lambda n: rng.integers(0, 2, n).tolist()
    roles = [TAG, None, READER, TAG, READER]
    lists = [[(300, bits(45)), (2500, bits(7))], [(10, bits(9))], [(100, bits(162))], [], [(50, bits(18)), (900, bits(27)), (1300, bits(9))]]
    return roles, lists, [0, 40, 1000, 7, 0], [3001, 500, 4000, 0, 1777]


@pytest.mark.parametrize('align', [1, 64])
def test_layout_padding_and_a_block_of_the_exact_size(align):
    roles, lists, base, n = _five_streams()
    ans = [pack([b for _, b in l]) for l in lists]
    idx = [[base[k] + i for i, _ in l] for k, l in enumerate(lists)]
    kw = dict(samp_rate=2e6, align_samples=align, delay_us=10.0)
    out, first, ns, pend = emulate.host_transmit(ans, idx, roles, base, n, **kw)
    assert ns.tolist() == [3001, 0, 4000, 0, 1777] and all(int(f) % align == 0 for f in first)
    need = int(first[-1]) + int(ns[-1])
    assert len(out) == need and first.tolist() == sorted(first.tolist())
    sentinel = np.complex64(7 - 3j)
    block = np.full(need + 16, sentinel, np.complex64)
    again = emulate.host_transmit(ans, idx, roles, base, n, out=block, cap_samples=need, **kw)
    assert again[0].tobytes() == out.tobytes() and (block[need:] == sentinel).all()
    for k in range(5):
        f, m = int(first[k]), int(ns[k])
        if roles[k] is not None:
            entries = [(i - base[k], b) for i, b in zip(idx[k], [b for _, b in lists[k]])]
            want = _model(roles[k], [(i + base[k], b) for i, b in entries], base[k] + n[k], 2e6, delay=20)[base[k]:]
            assert out.real[f:f + m].tobytes() == want.tobytes(), k
        end = int(first[k + 1]) if k < 4 else need
        assert not out[f + m:end].any()   # padding is (0, 0)
    # the 162-bit answer of stream 2 reaches beyond its span? no: every pending entry is none here but where it must be
    assert [int(p['n_bits']) for p in pend] == [0, 0, 0, 0, 0]
    # one sample short: nothing rendered, pending as it was
    carried = np.zeros(5, _lib.TX_PENDING_DTYPE)
    carried[2]['start'], carried[2]['n_bits'], carried[2]['role'], carried[2]['air'][:2] = 1001, 18, READER, [0xA5, 0x3C]
    block[:] = sentinel
    with pytest.raises(ValueError, match='cap_samples') as e:
        emulate.host_transmit(ans, idx, roles, base, n, pending=carried, out=block, cap_samples=need - 1, **kw)
    assert (block == sentinel).all() and e.value.pending.tobytes() == carried.tobytes()


def test_argument_errors_name_the_argument():
    rec, air, par = pack([[1, 0, 1, 1, 0, 0, 1]])
    call = lambda **kw: emulate.host_transmit([(kw.pop('rec', rec), air, par)], [[5]], [kw.pop('role', TAG)], [0], [kw.pop('n', 1000)], **kw)
    call()

    def cfg(**fields):
        c = tx.answers_tx_config()
        for k, v in fields.items():
            setattr(c, k, v)
        return c
    for fields, name in [(dict(rate_num=0), 'rate_num'), (dict(rate_den=0), 'rate_den'), (dict(rate_num=65537), 'rate_num'), (dict(rate_den=1 << 20), 'rate_den'),
                         (dict(samp_rate=0.0), 'samp_rate'), (dict(samp_rate=2e9), 'samp_rate'), (dict(samp_rate=float('nan')), 'samp_rate'),
                         (dict(align_samples=24), 'align_samples'), (dict(align_samples=0), 'align_samples')]:
        with pytest.raises(ValueError, match=name):
            call(cfg=cfg(**fields))
    with pytest.raises(ValueError, match='reserved'):
        call(_reserved=1)
    with pytest.raises(ValueError, match='span'):
        call(n=(1 << 30) + 1)
    for n_bits in (0, 10, 171, 9 * 19):
        bad = rec.copy()
        bad['n_bits'] = n_bits
        with pytest.raises(ValueError, match='n_bits'):
            call(rec=bad)
    bad = rec.copy()
    bad['byte_off'] = 1
    with pytest.raises(ValueError, match='byte_off'):
        call(rec=bad)
    bad['byte_off'], bad['n_bits'] = 0, 18   # two bytes in a part of one
    with pytest.raises(ValueError, match='byte_off'):
        call(rec=bad)


def test_names_are_declared_and_bound():
    names = ['nfc_host_answers_tx', 'nfc_multi_transmit_device', 'nfc_multi_get_tx_state', 'nfc_multi_set_tx_state']
    assert set(names) <= set(_lib.SYMBOLS)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'nfc_amd.h')).read()
    for n in names + ['nfc_answers_tx_config', 'nfc_tx_pending', 'nfc_tx_answer']:
        assert n in header
    import ctypes
    assert ctypes.sizeof(_lib.AnswersTxConfig) == 64 and ctypes.sizeof(_lib.TxPending) == 64 == _lib.TX_PENDING_DTYPE.itemsize
    assert _lib.TX_ANSWER_DTYPE.itemsize == 16 and 'NFC_AMD_ABI_VERSION 4' in header


# ---- 6. the twin over a real transaction, through the CPU route only ----
def test_twelve_answers_of_the_classic_capture_on_the_timeline():
    from usrp_nfc_amd import fsm, synth
    frames = synth.frames_from_trace(os.path.join(GOLD, '1k_with_enc.out'))[0][:24]
    heard = emulate.frames_of_bits([f for f in frames if f[0] == synth.READER])   # what a tag hears of the 24-frame capture
    heard.table['idx'] = 4000 * (np.arange(len(heard.table), dtype=np.uint64) + 1)   # a command every 2 ms
    card = emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_classic1k.json'), emulate.NFC_EMU_CARD)[0]
    _, ans = emulate.host_emulate(card, emulate.state_init(), fsm.state_init(), heard)
    assert len(ans) == 12
    idx = heard.table['idx'][ans.records['src'].astype(np.int64)].astype(np.int64)
    n_rx, delay = int(idx[-1]) + 4000, 172
    out, first, ns, pend = emulate.host_transmit([(ans.records, ans.air[:18 * 12], ans.par[:18 * 12])], [idx], [TAG], [0], [n_rx], samp_rate=2e6,
                                                 delay_us=86.43, align_samples=1)
    assert int(ns[0]) == n_rx and int(pend[0]['n_bits']) == 0 and idx.tolist() == sorted(idx.tolist())
    covered = np.zeros(n_rx, bool)
    for j in range(12):
        runs = tx.encode_runs(tx.NFC_TX_MANCHESTER, ans.bits(j))
        w = np.concatenate([np.full(tx.sample_count(runs[i:i + 1], 2e6), float(runs[i]['level']), np.float32) for i in range(len(runs))])
        s = int(idx[j]) + delay
        assert len(w) > 0 and (j == 11 or s + len(w) <= int(idx[j + 1]))   # non-empty and uncut
        assert out.real[s:s + len(w)].tobytes() == w.tobytes(), j
        covered[s:s + len(w)] = True
    assert not out.real[~covered].any() and not out.imag.any()
