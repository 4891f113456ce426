"""The air interface on the CPU (include/nfc_amd.h: nfc_host_air_render; csrc/air.hip.h): the twin of the rendering kernels
against synth.py, the yardstick.  With sigma 0 the twin's bytes are synth's, in all four IQ kinds; the noise is pinned by its definition
(a sample depends on its key alone) and by its statistics; what it renders decodes to the packets of the synth capture.  No GPU here:
tests/test_air.py pins the kernels to this twin."""
import os

import numpy as np
import pytest

from oracle import c_oracle as co
from tests.golden_util import GOLDEN
from usrp_nfc_amd import _lib, air, api, synth, tx

KINDS = (api.NFC_IN_IQ_F32, api.NFC_IN_IQ_I16, api.NFC_IN_IQ_I8, api.NFC_IN_IQ_U8)
QUANTISE = {api.NFC_IN_IQ_I16: synth.quantise_sc16, api.NFC_IN_IQ_I8: synth.quantise_sc8, api.NFC_IN_IQ_U8: synth.quantise_cu8}
REQA = [(synth.READER, synth.frame_bits([0x26], 7))]
_cache = {}


def ultralight():
    return synth.txn_frames()


def classic24():
    if 'classic' not in _cache:
        _cache['classic'] = synth.frames_from_trace(os.path.join(GOLDEN, '1k_with_enc.out'))[0]
    return _cache['classic'][:24]


def yardstick(frames, rate_msps=2.0, depth=0.08, **kw):
    return synth.iq_from_profile(synth.modulation_profile(frames, rate_msps=rate_msps, depth=depth, **kw), sigma=0)


# ---- the run lists: the claim the kernels' pieces rest on ----
def test_synth_pulse_lists_are_the_encoders_run_lists():
    classic = synth.frames_from_trace(os.path.join(GOLDEN, '1k_with_enc.out'))[0]
    assert len(classic) > 24
    for direction, bits in ultralight() + classic:
        if direction == synth.READER:
            assert synth.miller_pulses(bits) == tx.encode_bits(tx.NFC_TX_MILLER, bits)
        else:
            assert synth.manchester_pulses(bits) == tx.encode_bits(tx.NFC_TX_MANCHESTER, bits)


# ---- zero noise: synth's bytes ----
@pytest.mark.parametrize('rate', [2.0, 4.0, 10.0])
@pytest.mark.parametrize('depth', [0.08, 0.12])
@pytest.mark.parametrize('which', ['ultralight', 'classic24'])
def test_zero_noise_equals_synth_in_every_kind(which, depth, rate):
    frames = ultralight() if which == 'ultralight' else classic24()
    m = synth.modulation_profile(frames, rate_msps=rate, depth=depth)
    want = synth.iq_from_profile(m, sigma=0)
    first, n = air.sizes([frames], rate_msps=rate)
    assert first.tolist() == [0] and n.tolist() == [len(m)]
    if which == 'ultralight' and rate == 2.0:
        assert len(m) == 31283
    got = air.host_render([frames], sigma=0, depth=depth, rate_msps=rate)
    assert got.n_samples.tolist() == [len(m)] and np.array_equal(got.download(0), want)
    for kind, q in QUANTISE.items():
        cap = air.host_render([frames], out_kind=kind, sigma=0, depth=depth, rate_msps=rate)
        assert cap.download(0).dtype == q(want).dtype and np.array_equal(cap.download(0), q(want)), kind


# ---- the noise ----
def test_a_sample_depends_on_its_key_alone():
    a, b, c = ultralight()[:6], classic24()[:5], ultralight()[4:12]
    kw = dict(sigma=0.002, out_kind=api.NFC_IN_IQ_I16)
    three = air.host_render([a, b, c], stream_seeds=[11, 12, 13], **kw)
    alone = air.host_render([c], stream_seeds=[13], **kw)
    assert three.download(2).tobytes() == alone.download(0).tobytes()                       # not on K, not on where the stream lies
    assert int(three.first_sample[2]) > 0 and int(alone.first_sample[0]) == 0
    other = air.host_render([a, b, c], stream_seeds=[11, 12, 13], align_samples=64, **kw)   # another alignment: the same bytes
    assert other.first_sample.tolist() != three.first_sample.tolist() and all(int(f) % 64 == 0 for f in other.first_sample)
    for k in range(3):
        assert other.download(k).tobytes() == three.download(k).tobytes()
    default = air.host_render([a, b, c], **kw)                                              # stream k's seed is k
    assert default.download(1).tobytes() == air.host_render([a, b, c], stream_seeds=[0, 1, 2], **kw).download(1).tobytes()
    assert default.download(2).tobytes() != three.download(2).tobytes()
    assert air.host_render([c], stream_seeds=[13], seed=1, **kw).download(0).tobytes() != alone.download(0).tobytes()   # another seed
    # the padding between streams is idle carrier without noise
    pad = other.download_used().view(np.int16).reshape(-1, 2)[int(other.first_sample[0]) + int(other.n_samples[0]):int(other.first_sample[1])]
    idle = synth.quantise_sc16(np.array([np.float32(0.5 * np.cos(0.3)), np.float32(0.5 * np.sin(0.3))], np.float32))
    assert len(pad) > 0 and (pad == idle).all()


def test_noise_statistics():
    N, sigma = 1 << 20, 0.002
    cap = air.host_render([[]], sigma=sigma, lead_in=0, gap_us=0.0, tail=N, align_samples=1)
    assert cap.n_samples.tolist() == [N]
    x = cap.download(0)
    i = x[0::2].astype(np.float64) - float(np.float32(0.5 * np.cos(0.3)))
    q = x[1::2].astype(np.float64) - float(np.float32(0.5 * np.sin(0.3)))
    se = sigma / np.sqrt(N)
    print('mean I %.3g Q %.3g (se %.3g); std I %.6g Q %.6g; r %.4g' % (i.mean(), q.mean(), se, i.std(), q.std(), np.corrcoef(i, q)[0, 1]))
    assert abs(i.mean()) < 5 * se and abs(q.mean()) < 5 * se
    assert abs(i.std() / sigma - 1) < 0.01 and abs(q.std() / sigma - 1) < 0.01
    assert abs(np.corrcoef(i, q)[0, 1]) < 0.01


# ---- what it renders decodes ----
def _packets(iq):
    o = co.COracle(samp_rate=2e6, hi_val=1.1)
    try:
        o.push_iq(iq)
        return o.packets()
    finally:
        o.close()


def test_all_four_kinds_decode_to_the_packets_of_the_synth_capture():
    frames = ultralight()
    want = _packets(synth.iq_from_profile(synth.modulation_profile(frames, depth=0.08), sigma=0.002))
    assert len(want) == 19
    for kind in KINDS:
        x = air.host_render([frames], out_kind=kind, sigma=0.002, depth=0.08).download(0)
        if kind == api.NFC_IN_IQ_I16:
            x = api.host_i16_to_float(x)
        elif kind != api.NFC_IN_IQ_F32:
            x = api.host_iq8_to_float(x, kind)
        assert _packets(x) == want, kind


# ---- shapes ----
def test_ragged_streams_an_empty_one_in_the_middle():
    streams = [ultralight()[:3], [], REQA, classic24()[:2]]
    cap = air.host_render(streams, sigma=0, align_samples=16)
    gap = int(150.0 * 2.0)
    assert cap.n_samples[1] == gap + 400                       # a stream without frames: the tail alone
    assert all(int(f) % 16 == 0 for f in cap.first_sample) and cap.first_sample[0] == 0
    for k, fr in enumerate(streams):
        want = yardstick(fr) if fr else np.tile(yardstick([])[:2], gap + 400)
        assert np.array_equal(cap.download(k), want), k
    assert cap.used_samples == int(cap.first_sample[3]) + int(cap.n_samples[3])


def test_a_lone_reqa():
    cap = air.host_render([REQA], sigma=0)
    assert np.array_equal(cap.download(0), yardstick(REQA))
    fr = air.frames_of([REQA])
    assert fr.frames['n_bits'].tolist() == [7] and fr.air.tolist() == [0x26] and fr.frames['idle_before'].tolist() == [3000]


def test_a_frame_without_bits_no_idle_between_frames_and_no_tail():
    a, b = ultralight()[2], ultralight()[3]
    fr = air.frames_of([[a, b]], gap_us=0.0, lead_in=17, tail=0)
    assert fr.frames['idle_before'].tolist() == [17, 0] and fr.tail == 0
    cap = air.host_render(fr, sigma=0)
    assert np.array_equal(cap.download(0), yardstick([a, b], gap_us=0.0, lead_in=17, tail=0))
    # n_bits == 0 renders only its idle_before
    recs = np.zeros(3, air.AIR_FRAME_DTYPE)
    recs[0], recs[2] = fr.frames[0], fr.frames[1]
    recs[1]['type'], recs[1]['idle_before'] = 1, 5
    with_gap = air.AirFrames(recs, [0, 3], fr.air, fr.par, fr.byte_base, 0, 2.0)
    got = air.host_render(with_gap, sigma=0).download(0)
    idle, n_a = yardstick([])[:2], len(yardstick([a], gap_us=0.0, lead_in=17, tail=0))
    want = np.concatenate([yardstick([a], gap_us=0.0, lead_in=17, tail=0), np.tile(idle, 5), yardstick([b], gap_us=0.0, lead_in=0, tail=0)])
    assert len(got) == len(want) and n_a > 0 and np.array_equal(got, want)


# ---- errors: NFC_ERR_ARG, the argument by name ----
def _frames(**field):
    fr = air.frames_of([ultralight()[:4], REQA])
    for name, v in field.items():
        fr.frames[name][1] = v
    return fr


@pytest.mark.parametrize('make,name', [
    (lambda: air.host_render(_frames(), out_kind=api.NFC_IN_ENV_F32), 'out_kind'),
    (lambda: air.host_render(_frames(), align_samples=12), 'align_samples'),
    (lambda: air.host_render(_frames(), align_samples=0), 'align_samples'),
    (lambda: air.host_render(_frames(n_bits=10)), 'frames[1].n_bits'),
    (lambda: air.host_render(_frames(n_bits=9 * 257)), 'frames[1].n_bits'),
    (lambda: air.host_render(_frames(byte_off=10)), 'frames[1].byte_off'),
    (lambda: air.host_render(_frames(n_bits=9 * 12)), 'frames[1].byte_off'),
    (lambda: air.host_render(_frames(reserved=1)), 'reserved'),
    (lambda: air.host_render(_frames(flags=1)), 'flags'),
    (lambda: air.host_render(_frames(), _reserved=1), 'cfg.reserved'),
    (lambda: air.host_render([[]] * 65537), 'K exceeds 65536'),
])
def test_argument_errors_name_the_argument(make, name):
    with pytest.raises(ValueError) as e:
        make()
    assert name in str(e.value) and 'status -1' in str(e.value)


def test_a_capacity_that_is_too_small_reports_the_need_and_writes_nothing():
    frames = ultralight()
    with pytest.raises(ValueError) as e:
        air.host_render([frames], cap_samples=31282)
    assert 'cap_samples' in str(e.value) and '31283' in str(e.value)
    # through the library itself: the counts are the true need, the buffer is untouched
    import ctypes as C
    fr = air.frames_of([frames])
    cfg, _ = air._config(fr, api.NFC_IN_IQ_F32, 0.5, 0.3, 0.08, 0.002, 1, None, None, 1)
    out, first, n = np.full(2 * 31282, 7.0, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    rc = _lib.load().nfc_host_air_render(C.byref(cfg), fr.frames.ctypes.data, fr.frame_off.ctypes.data, fr.air.ctypes.data, fr.par.ctypes.data,
                                         fr.byte_base.ctypes.data, 1, out.ctypes.data, 31282, first.ctypes.data, n.ctypes.data)
    assert rc == -1 and n.tolist() == [31283] and (out == 7.0).all()
    assert air.host_render([frames], cap_samples=31283, align_samples=1).n_samples.tolist() == [31283]


def test_render_device_without_a_gpu_says_so():
    if _lib.load().nfc_device_count() > 0:
        pytest.skip('a GPU is present')
    with pytest.raises(air.AirError) as e:
        air.render_device([ultralight()])
    assert 'no HIP device' in str(e.value) and 'no CPU fallback' in str(e.value)
    # and the library itself, past the package's own check: NFC_ERR_DEVICE, not an abort
    import ctypes as C
    fr = air.frames_of([REQA])
    cfg, _ = air._config(fr, api.NFC_IN_IQ_F32, 0.5, 0.3, 0.08, 0.002, 1, None, None, 8)
    first, n = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    rc = _lib.load().nfc_air_render_device(0, C.byref(cfg), fr.frames.ctypes.data, fr.frame_off.ctypes.data, fr.air.ctypes.data, fr.par.ctypes.data,
                                           fr.byte_base.ctypes.data, 1, C.c_void_p(256), 1 << 20, first.ctypes.data, n.ctypes.data, None)   # (any pointer: the call must fail before touching it)
    assert rc == -2 and b'no HIP device' in _lib.load().nfc_last_error(None)
