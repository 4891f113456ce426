#!/usr/bin/env python3
"""Generate the committed golden vectors by driving the UNMODIFIED reference.

Runs only in the build container (needs /root/reference); the GPU box and the
test-suite never execute it -- they read the .npz/.json files it wrote.

The reference's hot-path modules (transition_sink, miller, manchester, packets,
utilities) import unchanged under Python 3 once ``gnuradio`` and ``fsm`` are
stubbed.  No reference source text is stored: fixtures
hold inputs (float32 envelopes, pulse lists) and the outputs the reference
produced for them.

    python3 tests/golden/make_golden.py           # rewrites tests/golden/*.npz|json
"""
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

REF = '/root/reference/code'


def import_reference():
    g = types.ModuleType('gnuradio')
    gr = types.ModuleType('gnuradio.gr')
    bl = types.ModuleType('gnuradio.blocks')

    class sync_block(object):
        def __init__(self, name=None, in_sig=None, out_sig=None):
            pass

    gr.sync_block = sync_block
    g.gr = gr
    g.blocks = bl
    sys.modules.update({'gnuradio': g, 'gnuradio.gr': gr, 'gnuradio.blocks': bl})
    f = types.ModuleType('fsm')
    packets_seen = []

    class fsm(object):
        def __init__(self, callback=None):
            pass

        def process_bits(self, bits, packet_type):
            packets_seen.append((packet_type, list(bits)))

    f.fsm = fsm
    sys.modules['fsm'] = f
    sys.path.insert(0, REF)
    import transition_sink, miller, manchester, packets, utilities   # noqa: E401
    return transition_sink, miller, manchester, packets, utilities, packets_seen


TS, MIL, MAN, PK, UT, PACKETS = import_reference()

from usrp_nfc_amd import synth   # noqa: E402  (the build's own generator)


class Tap(object):
    """Sits where CombinedPacketProcessor sits; forwards to the real one."""

    def __init__(self):
        self.cpp = PK.CombinedPacketProcessor()
        self.sym = {0: [], 1: []}

    def append_bit(self, bit, ptype):
        self.sym[ptype].append(int(bit))
        self.cpp.append_bit(bit, ptype)


def run_reference(x, samp_rate=2e6, hi_val=1.1, lo_val=0.1, av_window=2000, max_len=50,
                  reader=True, tag=True, chunk=8192, rng=None):
    """x: float32 envelope.  Mirrors decoder.py:31-33 + background.py:37-52 synchronously."""
    del PACKETS[:]
    tap = Tap()
    rd = MIL.miller_decoder(tap) if reader else None
    tg = MAN.manchester_decoder(tap) if tag else None
    all_tr = []

    def route(transitions):            # background.run body, no thread
        all_tr.extend(transitions)
        a = []
        cur = PK.PacketType.TAG_TO_READER
        for val, t in transitions:
            if t == cur:
                a.append(val)
            else:
                disp(a, cur)
                a = [val]
                cur = t
        if a:
            disp(a, cur)

    def disp(a, t):                    # background.process_transitions
        if t == PK.PacketType.TAG_TO_READER and tg:
            tg.process_transition(a)
        elif t == PK.PacketType.READER_TO_TAG and rd:
            rd.process_transition(a)

    ts = TS.transition_sink(samp_rate, route, lo_val=lo_val, hi_val=hi_val,
                            av_window=av_window, max_len=max_len)
    x = np.asarray(x, dtype=np.float32)
    i = 0
    while i < len(x):
        k = chunk if rng is None else int(rng.integers(1, chunk + 1))
        i += ts.work([x[i:i + k]], None)
    return all_tr, tap.sym[0], tap.sym[1], list(PACKETS)


def pack(x, params, res):
    tr, sym_tag, sym_rd, pk = res
    out = {
        'x': np.asarray(x, np.float32),
        'params': np.array([params['samp_rate'], params['lo_val'], params['hi_val'],
                            params['av_window'], params['max_len'],
                            int(params['reader']), int(params['tag'])], np.float64),
        'tr_v': np.array([v for (v, d), t in tr], np.int8),
        'tr_us': np.array([d for (v, d), t in tr], np.float64),
        'tr_t': np.array([t for (v, d), t in tr], np.int8),
        'sym_tag': np.array(sym_tag, np.uint8),
        'sym_reader': np.array(sym_rd, np.uint8),
        'pk_type': np.array([t for t, b in pk], np.int8),
        'pk_len': np.array([len(b) for t, b in pk], np.int32),
        'pk_bits': np.array([bit for t, b in pk for bit in b], np.uint8),
    }
    return out


DEFAULTS = dict(samp_rate=2e6, lo_val=0.1, hi_val=1.1, av_window=2000, max_len=50, reader=True, tag=True)


def make_case(name, x, **over):
    p = dict(DEFAULTS)
    p.update(over)
    kw = dict(samp_rate=p['samp_rate'], hi_val=p['hi_val'], lo_val=p['lo_val'], av_window=p['av_window'],
              max_len=p['max_len'], reader=p['reader'], tag=p['tag'])
    a = run_reference(x, chunk=8192, **kw)
    b = run_reference(x, chunk=4096, rng=np.random.default_rng(7), **kw)
    c = run_reference(x, chunk=3, **kw) if len(x) <= 9000 else a
    assert a == b == c, 'reference is not chunk-invariant on %s' % name
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **pack(x, p, a))
    print('%-28s N=%6d transitions=%6d sym_tag=%5d sym_reader=%5d packets=%3d' %
          (name, len(x), len(a[0]), len(a[1]), len(a[2]), len(a[3])))
    return a


def envelope(m, sigma=0.002, seed=1, amp=0.5):
    iq = synth.iq_from_profile(np.asarray(m, np.float32), amp=amp, sigma=sigma, seed=seed)
    return synth.envelope_f32(iq), iq


def check_encoders():
    """The build's pulse generators must equal the reference encoders."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        bits = rng.integers(0, 2, int(rng.integers(1, 40))).tolist()
        assert synth.miller_pulses(bits) == MIL.miller_encoder.encode_bits(bits)
        assert synth.manchester_pulses(bits) == MAN.manchester_encoder.encode_bits(bits)
    # utilities.Convert.to_bit_ar(parity=True) (needs xrange)
    import builtins
    builtins.xrange = range
    for _ in range(50):
        data = rng.integers(0, 256, int(rng.integers(1, 12))).tolist()
        assert synth.frame_bits(data) == UT.Convert.to_bit_ar(data, True)
    print('encoders: build generators == reference encoders')


def main():
    check_encoders()
    rng = np.random.default_rng(20151)

    # 1. report section 4.3 worked example (decoder only) + REQA known answer (report 3.3)
    tap = Tap()
    md = MIL.miller_decoder(tap)
    example = [(0, 3), (1, 11), (0, 3), (1, 16), (0, 3), (1, 6)]
    md.process_transition(list(example))
    reqa_bits = synth.frame_bits([0x26], 7)
    tap2 = Tap()
    md2 = MIL.miller_decoder(tap2)
    md2.process_transition(MIL.miller_encoder.encode_bits(reqa_bits) + [(1, 25.0)])
    json.dump({
        'report_example': {'pulses': example, 'symbols': tap.sym[1], 'stage': md._get_cur_stage()},
        'reqa': {'bits': reqa_bits, 'pulses': MIL.miller_encoder.encode_bits(reqa_bits) + [[1, 25.0]],
                 'symbols': tap2.sym[1]},
        'constants_hex': {
            'FULL': float(UT.PulseLength.FULL).hex(), 'ZERO': float(UT.PulseLength.ZERO).hex(),
            'HALF': float(UT.PulseLength.HALF).hex(), 'ZERO_REM': float(UT.PulseLength.ZERO_REM).hex(),
            'ONE_REM': float(UT.PulseLength.ONE_REM).hex(), 'ONE_HALF': float(UT.PulseLength.ONE_HALF).hex(),
            'MAN_LO': float(UT.PulseLength.HALF - 1).hex(), 'MAN_MID': float(UT.PulseLength.HALF + 1).hex(),
            'MAN_HI': float(2 * UT.PulseLength.HALF + 1).hex(),
            'MIL_LO': float(UT.PulseLength.ZERO - 1.5).hex(), 'MIL_HI': float(2 * UT.PulseLength.FULL).hex(),
        },
        'error_codes': {k: getattr(UT.ErrorCode, k) for k in
                        ('NO_ERROR', 'TOO_SHORT', 'TOO_LONG', 'ENCODING', 'INTERNAL', 'WRONG_DUR', 'GENERAL')},
    }, open(os.path.join(HERE, 'fx_report_miller.json'), 'w'), indent=1)
    print('fx_report_miller.json: example ->', tap.sym[1], ' reqa ->', tap2.sym[1])

    # 2. decoder-only vectors: random (cur, d) lists at several factors
    dec = {}
    for factor in (1.0, 0.5, 0.25, 0.1):
        n = 6000
        # mix of plausible durations and arbitrary ones
        d = rng.integers(1, 51, n)
        cur_m = rng.integers(0, 3, n)
        cur_t = rng.integers(-1, 2, n)
        tapm, tapt = Tap(), Tap()
        MIL.miller_decoder(tapm).process_transition([(int(c), int(k) * factor) for c, k in zip(cur_m, d)])
        MAN.manchester_decoder(tapt).process_transition([(int(c), int(k) * factor) for c, k in zip(cur_t, d)])
        key = ('%g' % factor).replace('.', 'p')
        dec['d_' + key] = d.astype(np.int16)
        dec['curm_' + key] = cur_m.astype(np.int8)
        dec['curt_' + key] = cur_t.astype(np.int8)
        dec['symm_' + key] = np.array(tapm.sym[1], np.uint8)
        dec['symt_' + key] = np.array(tapt.sym[0], np.uint8)
    # frame-like sequences with timing jitter, so that the non-error branches are well covered
    for factor in (0.5, 0.25):
        rate = 1.0 / factor
        seq_m, seq_t = [], []
        for _ in range(60):
            bits = rng.integers(0, 2, int(rng.integers(4, 40))).tolist()
            for lvl, us in MIL.miller_encoder.encode_bits(bits):
                k = max(1, int(us * rate) + int(rng.integers(-1, 2)))
                seq_m.append((int(lvl), min(k, 50)))
            seq_m.append((1, 50))
            for lvl, us in MAN.manchester_encoder.encode_bits(bits):
                k = max(1, int(us * rate) + int(rng.integers(-1, 2)))
                seq_t.append((int(lvl), min(k, 50)))
            seq_t.append((0, 50))
        tapm, tapt = Tap(), Tap()
        MIL.miller_decoder(tapm).process_transition([(c, k * factor) for c, k in seq_m])
        MAN.manchester_decoder(tapt).process_transition([(c, k * factor) for c, k in seq_t])
        key = 'frames_' + ('%g' % factor).replace('.', 'p')
        dec['dm_' + key] = np.array([k for c, k in seq_m], np.int16)
        dec['curm_' + key] = np.array([c for c, k in seq_m], np.int8)
        dec['symm_' + key] = np.array(tapm.sym[1], np.uint8)
        dec['dt_' + key] = np.array([k for c, k in seq_t], np.int16)
        dec['curt_' + key] = np.array([c for c, k in seq_t], np.int8)
        dec['symt_' + key] = np.array(tapt.sym[0], np.uint8)
    np.savez_compressed(os.path.join(HERE, 'fx_decoder_vectors.npz'), **dec)
    print('fx_decoder_vectors.npz written (%d arrays)' % len(dec))

    # 3. REQA + ATQA through the whole path
    frames = synth.txn_frames(synth.ULTRALIGHT_TXN[:2])
    m = synth.modulation_profile(frames, gap_us=90.0, depth=0.12)
    x, _ = envelope(m, seed=11)
    make_case('fx_reqa_atqa', x, hi_val=1.09)

    # 4. the whole Ultralight transaction of outputs/ultralight.out
    frames = synth.txn_frames()
    m = synth.modulation_profile(frames, gap_us=90.0, depth=0.12)
    x, iq = envelope(m, seed=12)
    res = make_case('fx_ultralight_txn', x, hi_val=1.09)
    # the 19 packets must carry the bytes of outputs/ultralight.out
    want = [(d, synth.frame_bits(data, sb)) for d, _, data, sb in synth.ULTRALIGHT_TXN]
    got = res[3]
    assert len(got) == len(want) == 19, (len(got), len(want))
    for (gt, gb), (wt, wb) in zip(got, want):
        assert gt == wt
        # fsm._fix_ending territory (fsm.py:51-66): one closing bit may be extra or missing
        k = min(len(gb), len(wb))
        assert abs(len(gb) - len(wb)) <= 1 and gb[:k] == wb[:k], (gt, gb, wb)
    print('fx_ultralight_txn: 19 packets carry the bytes of outputs/ultralight.out')
    # same transaction given as IQ with uhd semantics (hi 1.1): envelope computed by the path under test
    np.savez_compressed(os.path.join(HERE, 'fx_ultralight_iq.npz'), iq=iq.astype(np.float32))

    # 5. reader-only / tag-only flags on the same input
    make_case('fx_txn_reader_only', x, hi_val=1.09, tag=False)
    make_case('fx_txn_tag_only', x, hi_val=1.09, reader=False)

    # 6. stress: tag bursts hovering at the hi threshold
    frames = synth.txn_frames([synth.ULTRALIGHT_TXN[i] for i in (1, 3, 11)])
    m = synth.modulation_profile(frames, gap_us=120.0, depth=0.0488)
    x, _ = envelope(m, seed=13)
    make_case('fx_stress_hover', x)

    # 7. stress: dropouts > max_len, level steps, and HIGH immediately followed by LOW (v = 2)
    frames = synth.txn_frames(synth.ULTRALIGHT_TXN[:6])
    m = synth.modulation_profile(frames, gap_us=100.0, depth=0.1).copy()
    m[5000:5400] *= 0.2          # partial loss (LOW for 400 samples)
    m[9000:9800] = 0.0           # total loss
    m[12000:] *= 1.3             # level step up
    m[15000:15020] = 1.3 * 1.12  # load modulation ...
    m[15020:15026] = 0.0         # ... straight into a reader pause
    m[16000:] *= 0.6             # level step down
    x, _ = envelope(m, seed=14)
    make_case('fx_stress_dropout', x)

    # 8. ss == 0 start (window filled with zeros), then signal
    m = np.concatenate([np.zeros(2600, np.float32), synth.modulation_profile(synth.txn_frames(synth.ULTRALIGHT_TXN[:2]), lead_in=500)])
    x, _ = envelope(m, sigma=0.0, seed=15)
    make_case('fx_stress_zero_start', x)

    # 9. ragged sizes: N < window, N == window, window + 1, and an empty input
    x, _ = envelope(np.ones(2001, np.float32), seed=16)
    make_case('fx_short_1500', x[:1500])
    make_case('fx_short_2000', x[:2000])
    make_case('fx_short_2001', x[:2001])
    make_case('fx_empty', x[:0])

    # 10. uniform noise (dense marginal decisions), and non-default constructor arguments
    x = rng.random(20000, dtype=np.float32)
    make_case('fx_stress_uniform', x)
    frames = synth.txn_frames(synth.ULTRALIGHT_TXN[:6])
    m = synth.modulation_profile(frames, rate_msps=4.0, gap_us=90.0, depth=0.12, lead_in=6000)
    x, _ = envelope(m, seed=17)
    make_case('fx_rate4_scaled', x, samp_rate=4e6, av_window=4000, max_len=100, hi_val=1.09)
    make_case('fx_rate4_defaults', x, samp_rate=4e6, hi_val=1.09)
    m = synth.modulation_profile(frames, rate_msps=2.0, gap_us=90.0, depth=0.12, lead_in=1000)
    x, _ = envelope(m, seed=18)
    make_case('fx_window500_max30', x, av_window=500, max_len=30, hi_val=1.05, lo_val=0.2)

    # 11. wide dynamic range inside the window: the reference's running sum is inexact here
    m = synth.modulation_profile(synth.txn_frames(synth.ULTRALIGHT_TXN[:4]), gap_us=90.0, depth=0.12)
    x, _ = envelope(m, seed=19)
    x = x.copy()
    x[:2000] *= np.float32(10.0) ** rng.uniform(-6, 3, 2000).astype(np.float32)
    make_case('fx_stress_dynrange', x)
    corners()


def corners():
    """Round 6: the two corners that were only checked GPU-vs-oracle (`python3 tests/golden/make_golden.py --corners`
    writes these alone, leaving the other vectors' files as they are)."""
    # 12. LOW runs that end exactly on a time-out (transition_sink.py:95-99: the run's last sample resets _current_state to 0,
    # so the next change reports v = last_bit = -1, and a HIGH sample right behind it is NOT ignored).  Runs of max_len + 1,
    # 2 max_len + 1 (on a time-out), max_len, max_len + 2, 3 max_len + 1, 1 and 10 max_len samples, each followed by HIGH samples.
    rng = np.random.default_rng(3)
    x = (0.25 * (1 + 0.004 * rng.standard_normal(12000))).astype(np.float32)
    for start, ln in ((3000, 51), (4000, 101), (5000, 50), (6000, 52), (7000, 151), (8000, 1), (9000, 500)):
        x[start:start + ln] = 1e-6
        x[start + ln:start + ln + 3] = 0.25 * 1.3
    x[10500:10505] = 0.25 * 1.3   # HIGH straight into LOW: v = 2
    x[10505:10510] = 1e-6
    res = make_case('fx_low_run_timeout', x)
    vs = [v for (v, d), t in res[0]]
    assert -1 in vs and 2 in vs, sorted(set(vs))
    print('fx_low_run_timeout: v values', sorted(set(vs)), ' v = -1 x', vs.count(-1))

    # 13. samples that are not finite (transition_sink.py:58-77).  -Inf: ratio = -inf, LOW.  +Inf while _current_state != 2:
    # ratio = +inf > hi, HIGH, not stored.  +Inf while _current_state == 2 (right behind a LOW sample): neither test holds, the
    # sample is ACCEPTED -- the window sum becomes +inf, every later finite sample has ratio 0 and is LOW; a second +Inf then
    # gives ratio inf / inf = NaN, is accepted too, and inf - inf = NaN poisons the sum for good: every comparison with NaN is
    # false, every sample after it is val 0.
    frames = synth.txn_frames()
    m = synth.modulation_profile(frames, gap_us=100.0, depth=0.12)
    x0, _ = envelope(m, seed=21)
    n = len(x0)
    assert n > 16000, n
    x = x0.copy()
    x[2500] = -np.inf            # idle carrier: LOW for one sample
    x[2600] = np.inf             # state 0: HIGH
    x[2601] = np.inf             # state 1: HIGH again
    k = n // 2
    x[k:k + 4] = 0.0             # a pause ...
    x[k + 4] = np.inf            # ... and +Inf in state 2: stored, the sum is +inf from here on
    x[k + 3000] = np.inf         # ratio NaN: accepted; prev is finite, the sum stays +inf
    x[k + 4 + 2000] = np.inf     # lands on the slot that holds the first +Inf: inf - inf = NaN
    res = make_case('fx_nonfinite_inf', x)
    xi = x
    # a NaN in the middle of a frame: val 0 from there to the end of the stream
    x = x0.copy()
    x[2500] = -np.inf
    x[n // 3] = np.nan
    res = make_case('fx_nonfinite_nan', x)
    xn = x
    assert all(v == 0 or i < 10 for i, v in enumerate([v for (v, d), t in res[0]][-50:]))
    # a NaN that arrives in the FILL phase (transition_sink.py:109-125: sum(ar) is NaN from the first stable sample on)
    x = x0.copy()
    x[1234] = np.nan
    make_case('fx_nonfinite_fill', x)
    # the same streams as fc32 IQ whose envelope fl(fl(I I) + fl(Q Q)) is the fixture's, bit for bit (NaN as NaN)
    def iq_of(env):
        iq = np.zeros(2 * len(env), np.float32)
        iq[0::2] = np.sqrt(env.astype(np.float64)).astype(np.float32)
        return iq
    out = {}
    for name, env in (('inf', xi), ('nan', xn)):
        iq = iq_of(np.where(np.isfinite(env), env, 0).astype(np.float32))
        bad = np.flatnonzero(~np.isfinite(env))
        # a non-finite envelope out of IQ: Inf * Inf = Inf, -Inf has no IQ form (a sum of squares) -> +Inf there; NaN: a NaN component
        e2 = synth.envelope_f32(iq)
        e2[bad] = np.where(np.isnan(env[bad]), np.nan, np.inf)
        iq[2 * bad] = np.where(np.isnan(env[bad]), np.nan, np.inf).astype(np.float32)
        iq[2 * bad + 1] = np.where(np.isnan(env[bad]), 1.0, -np.inf).astype(np.float32)   # (NaN, 1) and (Inf, -Inf)
        assert np.array_equal(synth.envelope_f32(iq), e2, equal_nan=True)
        p = dict(DEFAULTS)
        a = run_reference(e2, chunk=8192, **{k_: p[k_] for k_ in ('samp_rate', 'hi_val', 'lo_val', 'av_window', 'max_len', 'reader', 'tag')})
        z = pack(e2, p, a)
        out.update({name + '_iq': iq, **{name + '_' + k_: v for k_, v in z.items()}})
        print('fx_nonfinite_iq[%s]: N=%d transitions=%d' % (name, len(e2), len(a[0])))
    np.savez_compressed(os.path.join(HERE, 'fx_nonfinite_iq.npz'), **out)


def dense_small():
    """A short DENSE capture for the one-launch stage of short batches (`python3 tests/golden/make_golden.py --dense-small` writes it alone):
    max_len = 1, so every sample behind the window fill is an entry, and the samples flicker between a LOW, an accepted and a HIGH
    level from one to the next.  Pushed whole, its first 16 384 samples hold four times the 4 096 entries the entry writer of
    csrc/small.hip.h lists per round (tests/test_small_stage.py reads the constants and asserts that).  Three levels only: it compresses well."""
    n = 20000
    x = np.full(n, 0.25, np.float32)
    x[600:n - 1500] = np.array([0.01, 0.25, 0.25 * 1.3], np.float32)[np.random.default_rng(2015).integers(0, 3, n - 2100)]
    res = make_case('fx_dense_small', x, av_window=500, max_len=1)
    assert len(res[0]) == n - 501, len(res[0])   # (the sample that completes the window reports nothing: transition_sink.py:109-125)


if __name__ == '__main__':
    if '--corners' in sys.argv:
        corners()
    elif '--dense-small' in sys.argv:
        dense_small()
    else:
        main()
