"""Recording to a 16-bit WAV on the GPU: nfc_record_pcm16_device / nfc_host_record_pcm16 (include/nfc_amd.h), api.record_pcm16*,
the reference-named record module and decoder(dst=...).

The conversion (nfc_amd.h): v = fl(x * gain), NaN -> 0, clamp to [-32767, 32767], round to nearest with halves away from zero,
int16.  x is the envelope the threshold kernels compute for the input kind (bit-identical to api.host_envelope) or the real part
of a complex64 sample.  Pinned here: the host twins (C and numpy) against the definition written out, the kernel against the host
twin bit for bit for every kind, nothing written beyond out[n), and the round trip -- what decoder(src=IQ, dst=wav) records,
decoder(src=wav) decodes to what the UNMODIFIED reference gave for that recording (tests/golden/make_record_golden.py)."""
import ctypes as C
import io
import os
import re
import wave

import numpy as np
import pytest

from tests.golden_util import Case, load_json, load_npz
from usrp_nfc_amd import _lib, api, decoder as dec, record as rec_mod, synth, tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAINS = [32767.0, 1000.5, 2.0 ** 15]
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 4097, (1 << 20) + 3]
NFC_ERR_ARG = -1


def c_twin(x, gain):
    f = _lib.load().nfc_host_record_pcm16
    g = float(np.float32(gain))
    return np.array([f(v, g) for v in np.asarray(x, np.float32).tolist()], np.int16)


def read_wav(path):
    w = wave.open(path, 'rb')
    try:
        return (w.getnchannels(), w.getsampwidth(), w.getframerate()), np.frombuffer(w.readframes(w.getnframes()), '<i2')
    finally:
        w.close()


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_header_constants_and_symbols():
    h = open(os.path.join(ROOT, 'include', 'nfc_amd.h')).read()
    for name, v in (('NFC_REC_ENVELOPE', 0), ('NFC_REC_REAL_PART', 1)):
        m = re.search(r'\b%s\s*=\s*(\d+)' % name, h)
        assert m and int(m.group(1)) == getattr(_lib, name) == getattr(api, name) == v
        assert name in api.__all__
    assert 'UNPINNED' in h[h.index('recording: a float per sample'):h.index('nfc_record_tap;')]
    assert {'nfc_record_pcm16_device', 'nfc_host_record_pcm16'} <= set(_lib.SYMBOLS)
    assert re.search(r'#define NFC_AMD_ABI_VERSION 4\b', h) and _lib.ABI_VERSION == 4


def test_record_translation_unit_isa(tmp_path):
    # csrc/nfc_record.hip compiled for gfx950 as the product is: the eight instantiations (seven kinds, and fc32's real-part tap),
    # each with 16-byte loads and one 16-byte store per trip, no scratch, no LDS, at most 64 VGPRs
    import subprocess
    from usrp_nfc_amd import build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-shared')]
    asm = str(tmp_path / 'nfc_record.s')
    subprocess.check_call([hipcc] + flags + ['-S', '--cuda-device-only', os.path.join(build.CSRC, 'nfc_record.hip'), '-o', asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    names = ['_ZN3nfc3rec14k_record_pcm16ILi%dELi0ELb0EEEvPKvmffPs' % k for k in range(7)] + ['_ZN3nfc3rec14k_record_pcm16ILi0ELi1ELb0EEEvPKvmffPs']
    loads = {0: 4, 1: 2, 2: 2, 3: 1, 4: 2, 5: 1, 6: 1}
    for nm in names:
        body = re.search(r'^%s:(.*?)\.end_amdhsa_kernel' % nm, text, re.S | re.M)
        assert body, nm
        body = body.group(1)
        k = int(re.search(r'ILi(\d)E', nm).group(1))
        assert body.count('global_load_dwordx4') >= loads[k] and body.count('global_store_dwordx4') >= 1, nm
        assert 'scratch_' not in body and 'ds_' not in body, nm
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 64, nm
        assert re.search(r'\.amdhsa_group_segment_fixed_size 0\b', body) and re.search(r'\.amdhsa_private_segment_fixed_size 0\b', body), nm
    assert 'nfc_record.hip' in build.SOURCES and {'nfc_record.hip', 'record.hip.h'} <= set(build.DEPS)


def test_host_twins_on_the_boundary_table():
    # every k, k +- 0.5 and the floats one ulp inside those halves, k = 0 .. 32767, and their negatives, at gain 1; the expected
    # values follow from the definition: a half rounds away from zero, a float just inside it does not, 32767 is the ceiling
    k = np.arange(32768, dtype=np.int64)
    kf = k.astype(np.float32)
    up, dn = kf + np.float32(0.5), kf - np.float32(0.5)
    xs = [kf, up, np.nextafter(up, np.float32(-np.inf)), dn, np.nextafter(dn, np.float32(np.inf))]
    want = [k, np.minimum(k + 1, 32767), k, np.where(k >= 1, k, -1), np.where(k >= 1, k, 0)]
    assert all(a.dtype == np.float32 for a in xs)
    assert xs[2][0] == np.float32(0.49999997) and xs[4][0] == np.float32(-0.49999997)   # (fl(0.49999997 + 0.5) is 1: no adding of 0.5)
    x = np.concatenate(xs)
    w = np.concatenate(want)
    x, w = np.concatenate([x, -x]), np.concatenate([w, -w]).astype(np.int16)
    got = api.host_record_pcm16(x, 1.0)
    assert got.dtype == np.int16 and np.array_equal(got, w)
    assert np.array_equal(c_twin(x, 1.0), w)


def test_host_twins_on_special_values():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.array([0.49999997, -0.49999997, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, inf, -inf, nan, -nan, 32767.0,
                  32767.49, 32767.5, 32768.0, 40000.0, 1e10, 3.4e38, -32767.0, -32767.5, -32768.0, -40000.0, -1e10, -3.4e38], np.float32)
    want = np.array([0, 0, 0, 0, 0, 0, 0, 0, 32767, -32767, 0, 0, 32767, 32767, 32767, 32767, 32767, 32767, 32767, -32767, -32767, -32767,
                     -32767, -32767, -32767], np.int16)
    assert np.array_equal(api.host_record_pcm16(x, 1.0), want)
    assert np.array_equal(c_twin(x, 1.0), want)
    # the product is one float32 rounding, then the steps above: fl(0.5 * 32767) = 16383.5 -> 16384; 3.4e38 * 32767 overflows -> 32767
    x = np.array([0.5, -0.5, 1.0, 1.5e-5, 3.4e38, -3.4e38, nan, 1e-45], np.float32)
    assert api.host_record_pcm16(x).tolist() == [16384, -16384, 32767, 0, 32767, -32767, 0, 0]   # (default gain 32767)
    assert c_twin(x, 32767.0).tolist() == [16384, -16384, 32767, 0, 32767, -32767, 0, 0]


def test_host_twins_agree_on_random_floats():
    rng = np.random.default_rng(20)
    x = np.concatenate([rng.uniform(-1.2, 1.2, 500_000).astype(np.float32),
                        rng.integers(0, 1 << 32, 500_000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    for g in GAINS:
        a = api.host_record_pcm16(x, g)
        assert np.array_equal(a, c_twin(x, g)), g
        assert a.min() == -32767 and a.max() == 32767


def test_device_call_checks_its_arguments_before_the_device():
    L = _lib.load()
    ok, odd = C.c_void_p(0x10000), C.c_void_p(0x10008)   # (never dereferenced: every call below fails its checks first)
    f32, env, sc16, sc8, cu8 = api.NFC_IN_IQ_F32, api.NFC_IN_ENV_F32, api.NFC_IN_IQ_I16, api.NFC_IN_IQ_I8, api.NFC_IN_IQ_U8

    def call(tap=0, kind=f32, scale=0.0, src=ok, n=64, gain=32767.0, dst=ok):
        return L.nfc_record_pcm16_device(0, tap, kind, scale, src, n, gain, dst, None, None)

    assert call(tap=2) == NFC_ERR_ARG and call(tap=-1) == NFC_ERR_ARG
    assert b'tap' in L.nfc_last_error(None)
    assert call(kind=7) == NFC_ERR_ARG and call(kind=-1) == NFC_ERR_ARG
    for kind in (env, api.NFC_IN_REAL_F32_SQ, api.NFC_IN_I16_SQ, sc16, sc8, cu8):
        assert call(tap=api.NFC_REC_REAL_PART, kind=kind) == NFC_ERR_ARG, kind
    for g in (0.0, -1.0, float('nan'), float('inf'), -float('inf')):
        assert call(gain=g) == NFC_ERR_ARG, g
    assert b'gain' in L.nfc_last_error(None)
    assert call(n=(1 << 30) + 1) == NFC_ERR_ARG
    assert call(src=odd) == NFC_ERR_ARG and call(dst=odd) == NFC_ERR_ARG
    assert b'aligned' in L.nfc_last_error(None)
    assert call(src=None) == NFC_ERR_ARG and call(dst=None) == NFC_ERR_ARG
    assert call(kind=sc16, scale=2.0 ** 49) == NFC_ERR_ARG and b'2^48' in L.nfc_last_error(None)
    for kind in (sc8, cu8):
        assert call(kind=kind, scale=2.0 ** 57) == NFC_ERR_ARG and b'2^56' in L.nfc_last_error(None)
    # n == 0 is a successful no-op -- also with null pointers, also without a device
    assert L.nfc_record_pcm16_device(0, 0, f32, 0.0, None, 0, 32767.0, None, None, None) == 0
    with pytest.raises(api.NfcError, match='gain'):
        api.record_pcm16_device(0x10000, 64, 0x10000, f32, gain=0.0)
    # pointers in every form a caller holds them: an integer, a ctypes pointer (DeviceBuffer.ptr, a stream of nfc_stream_create), None
    with pytest.raises(api.NfcError, match='gain'):
        api.record_pcm16_device(ok, 64, C.c_void_p(0x20000), f32, gain=-1.0, stream=C.c_void_p(0x30000))
    with pytest.raises(api.NfcError, match='aligned'):
        api.record_pcm16_device(odd, 64, ok, f32)
    with pytest.raises(api.NfcError, match='null buffer'):
        api.record_pcm16_device(None, 64, ok, f32, stream=0)
    assert api.record_pcm16_device(None, 0, None, f32) is None


def test_record_writes_pcm_into_a_mono_16_bit_wav(tmp_path):
    rng = np.random.default_rng(3)
    pcm = rng.integers(-32768, 32768, 10_001).astype(np.int16)
    p = str(tmp_path / 'a.wav')
    with rec_mod.record(p, samp_rate=2.5e6 + 0.7) as r:
        assert r.write_pcm(pcm[:4000]) == 4000
        r.write_pcm(pcm[4000:4000])   # (an empty piece)
        r.write_pcm(pcm[4000:])
    fmt, frames = read_wav(p)
    assert fmt == (1, 2, 2500000) and np.array_equal(frames, pcm)   # rate int(samp_rate), record.py:17
    with pytest.raises(ValueError):
        r.write_pcm(pcm)   # closed
    r.close()   # (twice is fine)
    q = str(tmp_path / 'b.wav')
    r = rec_mod.record(q)
    r.write_pcm(pcm[:5])
    r.close()
    fmt, frames = read_wav(q)
    assert fmt == (1, 2, 2000000) and frames.tolist() == pcm[:5].tolist()
    assert open(q, 'rb').read(4) == b'RIFF'


def test_record_refuses_to_pass_the_riff_limit(tmp_path, monkeypatch):
    assert rec_mod.RIFF_LIMIT == (1 << 32) - 1 - 36
    monkeypatch.setattr(rec_mod, 'RIFF_LIMIT', 2 * 1000)
    p = str(tmp_path / 'a.wav')
    r = rec_mod.record(p)
    r.write_pcm(np.arange(600, dtype=np.int16))
    with pytest.raises(ValueError, match='4 GiB'):
        r.write_pcm(np.zeros(401, np.int16))   # would end at 2002 bytes: refused whole, nothing of it written
    r.write_pcm(np.full(400, 7, np.int16))       # exactly at the limit
    r.close()
    _, frames = read_wav(p)
    assert frames.tolist() == list(range(600)) + [7] * 400


def test_fixture_against_the_pinned_c_oracle():
    from oracle import c_oracle as co
    z = load_npz('fx_ultralight_rec16.npz')
    c = Case('fx_ultralight_rec16')
    pcm = z['pcm']
    iq = load_npz('fx_ultralight_iq.npz')['iq']
    assert pcm.dtype == np.int16 and len(pcm) == len(iq) // 2 == 29003
    assert np.array_equal(pcm, api.host_record_pcm16(api.host_envelope(iq, api.NFC_IN_IQ_F32), 32767.0))
    assert int(np.abs(pcm.astype(np.int32)).max()) == 10560   # nothing clipped
    x = api.host_envelope(pcm, api.NFC_IN_I16_SQ, 0.0)
    assert np.array_equal(x.view(np.uint32), c.x.view(np.uint32)) and c.params['hi_val'] == 1.09
    o = co.COracle(**c.params)
    o.push_env(x)
    assert o.transitions() == c.transitions and len(c.transitions) == 2101
    assert o.symbols(0).tolist() == c.sym_tag.tolist() and o.symbols(1).tolist() == c.sym_reader.tolist()
    assert o.packets() == c.packets and len(c.packets) == 19
    own = Case('fx_ultralight_txn')
    assert c.packets == own.packets and c.sym_tag.tolist() == own.sym_tag.tolist() and c.sym_reader.tolist() == own.sym_reader.tolist()


class _FakeContext(object):
    """Stands in for api.NfcContext on the CPU (as tests/test_gr_branch.py's does): records what the sink asks for."""
    made = []

    def __init__(self, **kw):
        self.kw, self.pushed, self.pushed_device = kw, [], []
        _FakeContext.made.append(self)

    def push(self, x):
        self.pushed.append(np.array(x, copy=True))

    def push_device(self, ptr, n):
        self.pushed_device.append(n)

    def transitions(self):
        return []

    def symbols(self, t):
        return np.zeros(0, np.uint8)

    def packets(self):
        return []

    def close(self):
        pass


def _forbid(name):
    def f(*a, **k):
        raise AssertionError('%s must not be called on this path' % name)
    return f


def test_default_path_is_unchanged_and_wav_sources_ignore_dst(tmp_path, monkeypatch):
    from usrp_nfc_amd import transition_sink as ts_mod
    if dec._gr is not None:
        pytest.skip('the offline decoder class is not the one in use where GNU Radio is importable')
    monkeypatch.setattr(api, 'NfcContext', _FakeContext)
    monkeypatch.setattr(api, 'record_pcm16_device', _forbid('record_pcm16_device'))
    monkeypatch.setattr(api, 'record_pcm16', _forbid('record_pcm16'))
    monkeypatch.setattr(api, 'DeviceBuffer', _forbid('DeviceBuffer'))
    monkeypatch.setattr(rec_mod, 'record', _forbid('record'))
    monkeypatch.setattr(ts_mod.transition_sink, 'push_device_now', _forbid('push_device_now'))
    calls = []
    plain = ts_mod.transition_sink.push_now
    monkeypatch.setattr(ts_mod.transition_sink, 'push_now', lambda self, x: (calls.append(len(x)), plain(self, x))[1])
    iq = np.arange(2 * 2500, dtype=np.float32)
    _FakeContext.made = []
    d = dec.decoder(src=iq.view(np.complex64), dst=None, batch=1000)
    assert d.run() is d._back
    ctx = _FakeContext.made[-1]
    assert calls == [2000, 2000, 1000] and ctx.pushed_device == []
    assert np.array_equal(np.concatenate(ctx.pushed), iq) and ctx.kw['input_kind'] == api.NFC_IN_IQ_F32 and ctx.kw['hi_val'] == 1.1
    # the WAV branch's kinds (int16 PCM, real float32, a .wav path): dst stays ignored, as the reference ignores it there
    pcm = np.arange(-1200, 1300, dtype=np.int16)
    wav_in = str(tmp_path / 'in.wav')
    with wave.open(wav_in, 'wb') as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(2000000)
        w.writeframes(pcm.tobytes())
    for src in (pcm, pcm.astype(np.float32), wav_in):
        out = str(tmp_path / 'out.wav')
        del calls[:]
        d = dec.decoder(src=src, dst=out, batch=1000, record_gain=1000.0)
        d.run()
        assert calls == [1000, 1000, 500] and _FakeContext.made[-1].pushed_device == []
        assert _FakeContext.made[-1].kw['hi_val'] == 1.09 and not os.path.exists(out)


class _FakeDeviceBuffer(object):
    """Stands in for api.DeviceBuffer on the CPU: host bytes behind the same methods."""
    live = 0

    def __init__(self, host_array, device=0, nbytes=None):
        a = np.ascontiguousarray(host_array)
        self.nbytes = max(a.nbytes, int(nbytes or 0))
        self.data = np.zeros(self.nbytes, np.uint8)
        self.upload(a)
        _FakeDeviceBuffer.live += 1

    def upload(self, host_array):
        a = np.ascontiguousarray(host_array)
        assert a.nbytes <= self.nbytes
        self.data[:a.nbytes] = a.view(np.uint8).reshape(-1)

    def download(self, nbytes=None):
        return self.data[:self.nbytes if nbytes is None else nbytes].copy()

    def free(self):
        _FakeDeviceBuffer.live -= 1


def test_decoder_dst_wiring_with_stand_ins(tmp_path, monkeypatch):
    # our side of decoder(dst=...): per batch one upload, push_device on that buffer, the record call on the SAME buffer with the
    # envelope tap and the kind's scale, the PCM appended; the file closed and the buffers freed when run() ends -- also when it raises
    if dec._gr is not None:
        pytest.skip('the offline decoder class is not the one in use where GNU Radio is importable')
    calls = []

    def fake_record(dev_ptr, n, out_ptr, kind, i16_scale=0.0, gain=32767.0, tap=api.NFC_REC_ENVELOPE, device=0, stream=None, timed=False):
        dt, per = api._KIND_DTYPE[kind]
        x = dev_ptr.data[:n * per * np.dtype(dt).itemsize].view(dt)
        out_ptr.upload(api.host_record_pcm16(api.host_envelope(x, kind, i16_scale), gain))
        calls.append((dev_ptr, n, kind, i16_scale, gain, tap))

    monkeypatch.setattr(api, 'NfcContext', _FakeContext)
    monkeypatch.setattr(api, 'DeviceBuffer', _FakeDeviceBuffer)
    monkeypatch.setattr(api, 'record_pcm16_device', fake_record)
    _FakeDeviceBuffer.live = 0
    iq = load_npz('fx_ultralight_iq.npz')['iq']
    fx = load_npz('fx_ultralight_rec16.npz')['pcm']
    p = str(tmp_path / 'a.wav')
    _FakeContext.made = []
    dec.decoder(src=iq.view(np.complex64), dst=p, batch=4097, samp_rate=2e6).run()
    ctx = _FakeContext.made[-1]
    assert ctx.pushed == [] and ctx.pushed_device == [4097] * 7 + [29003 - 7 * 4097] == [c[1] for c in calls]
    assert all(c[2:] == (api.NFC_IN_IQ_F32, 0.0, 32767.0, api.NFC_REC_ENVELOPE) for c in calls) and len({id(c[0]) for c in calls}) == 1
    fmt, frames = read_wav(p)
    assert fmt == (1, 2, 2000000) and np.array_equal(frames, fx) and _FakeDeviceBuffer.live == 0
    # cu8 with its scale and another gain
    q = synth.quantise_cu8(iq)
    del calls[:]
    dec.decoder(src=q.reshape(-1, 2), dst=p, batch=10_000, iq8_scale=0.01, record_gain=1000.5).run()
    assert [c[1:] for c in calls] == [(10_000, api.NFC_IN_IQ_U8, 0.01, 1000.5, api.NFC_REC_ENVELOPE)] * 2 + [(9003, api.NFC_IN_IQ_U8, 0.01, 1000.5, api.NFC_REC_ENVELOPE)]
    assert np.array_equal(read_wav(p)[1], api.host_record_pcm16(api.host_envelope(q, api.NFC_IN_IQ_U8, 0.01), 1000.5))
    # a run() that raises still closes the file (a complete header over what was written) and frees the buffers

    def failing(dev_ptr, n, *a, **k):
        if len(calls) == 2:
            raise RuntimeError('no more')
        fake_record(dev_ptr, n, *a, **k)

    monkeypatch.setattr(api, 'record_pcm16_device', failing)
    del calls[:]
    with pytest.raises(RuntimeError, match='no more'):
        dec.decoder(src=iq.view(np.complex64), dst=p, batch=10_000).run()
    assert np.array_equal(read_wav(p)[1], fx[:20_000]) and _FakeDeviceBuffer.live == 0


# ---- GPU --------------------------------------------------------------------------------------------------------------------

KIND_CASES = {   # name -> (kind, tap, scales)
    'fc32': (api.NFC_IN_IQ_F32, api.NFC_REC_ENVELOPE, [0.0]),
    'env': (api.NFC_IN_ENV_F32, api.NFC_REC_ENVELOPE, [0.0]),
    'real': (api.NFC_IN_REAL_F32_SQ, api.NFC_REC_ENVELOPE, [0.0]),
    'pcm': (api.NFC_IN_I16_SQ, api.NFC_REC_ENVELOPE, [0.0, 1.0 / 32768.0]),
    'sc16': (api.NFC_IN_IQ_I16, api.NFC_REC_ENVELOPE, [0.0, 1.0 / 32768.0]),
    'sc8': (api.NFC_IN_IQ_I8, api.NFC_REC_ENVELOPE, [2.0 ** -7, 1.0 / 100.0]),   # (a power of two: the integer route; 1/100: the float route)
    'cu8': (api.NFC_IN_IQ_U8, api.NFC_REC_ENVELOPE, [0.0, 1.0 / 100.0]),
    'fc32_real_part': (api.NFC_IN_IQ_F32, api.NFC_REC_REAL_PART, [0.0]),
}


def _random_input(kind, n, rng):
    dt, per = api._KIND_DTYPE[kind]
    if dt == np.float32:
        x = rng.normal(0.0, 0.6, n * per).astype(np.float32)
        if kind == api.NFC_IN_ENV_F32 and n:   # NaN, +-Inf, negatives (the normal draw), denormals, values that clip
            odd = np.array([np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 0.0, -0.0, 5.0, -5.0, 1.5 / 32767, 2.5 / 32767], np.float32)
            x[rng.integers(0, n, min(n, 64))] = odd[rng.integers(0, len(odd), min(n, 64))]
        return x
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, n * per).astype(dt)


def _capture(kind):
    iq = load_npz('fx_ultralight_iq.npz')['iq']
    return {api.NFC_IN_IQ_F32: lambda: iq, api.NFC_IN_ENV_F32: lambda: api.host_envelope(iq, api.NFC_IN_IQ_F32),
            api.NFC_IN_REAL_F32_SQ: lambda: np.ascontiguousarray(iq[0::2]), api.NFC_IN_I16_SQ: lambda: load_npz('fx_ultralight_rec16.npz')['pcm'],
            api.NFC_IN_IQ_I16: lambda: synth.quantise_sc16(iq), api.NFC_IN_IQ_I8: lambda: synth.quantise_sc8(iq),
            api.NFC_IN_IQ_U8: lambda: synth.quantise_cu8(iq)}[kind]()


def _want(x, kind, tap, scale, gain):
    if tap == api.NFC_REC_REAL_PART:
        return api.host_record_pcm16(np.asarray(x, np.float32)[0::2], gain)
    return api.host_record_pcm16(api.host_envelope(x, kind, scale), gain)


def _device_with_guards(x, kind, tap, scale, gain, stream=None, timed=False):
    """-> (pcm, ms): the kernel's output for x, written between two 16-byte guards that must survive."""
    per = api._KIND_DTYPE[kind][1]
    n = len(x) // per
    tail = 16 + (-2 * n) % 16 + 16   # (to a 16-byte boundary, then a whole guard)
    src = api.DeviceBuffer(x if n else np.zeros(8, np.uint8))
    dst = api.DeviceBuffer(np.full(16 + 2 * n + tail, 0xA5, np.uint8))
    try:
        ms = api.record_pcm16_device(src, n, dst.ptr.value + 16, kind, scale, gain, tap, stream=stream, timed=timed)
        if stream is not None:
            assert _lib.load().nfc_stream_sync(0, stream) == 0
        raw = dst.download()
    finally:
        src.free()
        dst.free()
    assert np.all(raw[:16] == 0xA5) and np.all(raw[16 + 2 * n:] == 0xA5), 'written outside out[0, %d)' % n
    return raw[16:16 + 2 * n].view(np.int16), ms


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KIND_CASES))
def test_device_equals_host_twin(name):
    kind, tap, scales = KIND_CASES[name]
    rng = np.random.default_rng(sorted(KIND_CASES).index(name))
    inputs = [_random_input(kind, n, rng) for n in LENGTHS] + [_capture(kind)]
    for x in inputs:
        for scale in scales:
            for gain in GAINS:
                got, _ = _device_with_guards(x, kind, tap, scale, gain)
                want = _want(x, kind, tap, scale, gain)
                assert len(got) == len(want)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (name, len(want), scale, gain, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    x = inputs[-1]   # the upload / convert / download form
    assert np.array_equal(api.record_pcm16(x, kind, scales[-1], 1000.5, tap), _want(x, kind, tap, scales[-1], 1000.5))
    assert len(api.record_pcm16(x[:0], kind, tap=tap)) == 0


@pytest.mark.gpu
def test_stream_form_and_kernel_time():
    L = _lib.load()
    st = C.c_void_p()
    assert L.nfc_stream_create(0, C.byref(st)) == 0
    try:
        rng = np.random.default_rng(9)
        for name in ('fc32', 'sc16', 'cu8', 'fc32_real_part'):
            kind, tap, scales = KIND_CASES[name]
            x = _random_input(kind, (1 << 20) + 3, rng)
            got, ms = _device_with_guards(x, kind, tap, scales[0], 32767.0, stream=st)   # enqueued; complete after nfc_stream_sync
            assert ms is None and np.array_equal(got, _want(x, kind, tap, scales[0], 32767.0)), name
            got, ms = _device_with_guards(x, kind, tap, scales[0], 32767.0, stream=st, timed=True)
            assert ms > 0 and np.array_equal(got, _want(x, kind, tap, scales[0], 32767.0)), name
        got, ms = _device_with_guards(x, kind, tap, 0.0, 32767.0, timed=True)   # the null stream, timed
        assert 0 < ms < 100
    finally:
        assert L.nfc_stream_destroy(0, st) == 0


def _run_decoder(src, dst=None, **kw):
    d = dec.decoder(src=src, dst=dst, **kw)
    d._back.transitions = []      # keep the raw transitions too
    d._trans._want_list = True
    b = d.run()
    return dict(transitions=b.transitions, sym_tag=list(b.symbols[0]), sym_reader=list(b.symbols[1]), packets=list(b.packets))


@pytest.mark.gpu
def test_decoder_dst_records_the_envelope_and_decodes_the_same(tmp_path):
    iq = load_npz('fx_ultralight_iq.npz')['iq']
    fx = load_npz('fx_ultralight_rec16.npz')['pcm']
    plain = _run_decoder(iq.view(np.complex64))
    assert len(plain['packets']) == 19 and len(plain['transitions']) > 2000
    for i, batch in enumerate((1 << 22, 10_000, 4097)):   # (4097 does not divide 29003; the last piece has 324 samples)
        p = str(tmp_path / ('rec%d.wav' % i))
        got = _run_decoder(iq.view(np.complex64), p, batch=batch)
        assert got == plain, batch   # recording does not disturb decoding
        fmt, frames = read_wav(p)
        assert fmt == (1, 2, 2000000) and np.array_equal(frames, fx), batch
    # a raw complex64 file as the source, another gain
    p32, p = str(tmp_path / 'cap.fc32'), str(tmp_path / 'g.wav')
    iq.astype('<f4').tofile(p32)
    assert _run_decoder(p32, p, batch=4097, record_gain=4096.0) == plain
    assert np.array_equal(read_wav(p)[1], api.host_record_pcm16(api.host_envelope(iq, api.NFC_IN_IQ_F32), 4096.0))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['sc16', 'sc8', 'cu8'])
def test_decoder_dst_with_integer_iq(tmp_path, name):
    kind = KIND_CASES[name][0]
    q = _capture(kind)
    other = 1.0 / 32768.0 if name == 'sc16' else 1.0 / 100.0
    for j, (scale, kw) in enumerate(((0.0, {}), (other, {'iq16_scale' if name == 'sc16' else 'iq8_scale': other}))):
        plain = _run_decoder(q.reshape(-1, 2), **kw)
        p = str(tmp_path / ('%s_%d.wav' % (name, j)))
        got = _run_decoder(q.reshape(-1, 2), p, batch=4097, record_gain=1000.5, **kw)
        assert got == plain and len(plain['packets']) > 10
        assert np.array_equal(read_wav(p)[1], api.host_record_pcm16(api.host_envelope(q, kind, scale), 1000.5)), scale


@pytest.mark.gpu
def test_wav_source_with_dst_writes_no_file(tmp_path):
    fx = load_npz('fx_ultralight_rec16.npz')['pcm']
    src, out = str(tmp_path / 'in.wav'), str(tmp_path / 'out.wav')
    with rec_mod.record(src) as r:
        r.write_pcm(fx)
    a = _run_decoder(src, out)
    assert a == _run_decoder(src) and len(a['packets']) == 19 and not os.path.exists(out)
    assert _run_decoder(fx, out) == a and not os.path.exists(out)


@pytest.mark.gpu
def test_round_trip_gives_the_reference_outputs(tmp_path):
    # decoder(src=IQ, dst=wav) then decoder(src=wav): the transitions, symbols and packets the unmodified reference produced from
    # that recording through its WAV branch (fx_ultralight_rec16), and the command trace of tests/golden/ultralight.out
    from usrp_nfc_amd import fsm
    c = Case('fx_ultralight_rec16')
    iq = load_npz('fx_ultralight_iq.npz')['iq']
    p = str(tmp_path / 'rec.wav')
    dec.decoder(src=iq.view(np.complex64), dst=p, batch=10_000).run()
    got = _run_decoder(p, batch=10_000)
    assert got['transitions'] == c.transitions
    assert got['sym_tag'] == c.sym_tag.tolist() and got['sym_reader'] == c.sym_reader.tolist()
    assert got['packets'] == c.packets and len(c.packets) == 19
    out = io.StringIO()
    m = fsm.fsm(out=out)
    for t, bits in got['packets']:
        m.process_bits(bits, t)
    gold = open(os.path.join(ROOT, 'tests', 'golden', 'ultralight.out')).read().rstrip('\n')
    assert out.getvalue().rstrip('\n') == gold


@pytest.mark.gpu
def test_transmit_side_is_recorded_from_device_memory(tmp_path):
    from oracle import c_oracle as co
    cases = load_json('fx_tx.json')['cases']
    c = max((c for c in cases if c['samp_rate'] == 2e6 and c['encoding'] == 'miller'), key=lambda c: sum(n for _, n in c['samples_rle']))
    runs = tx.as_runs([(1, 1500.0)] + [(l, float.fromhex(d)) for l, d in c['runs']] + [(1, 300.0)])   # an idle carrier round the frame
    iq = tx.render(runs, 2e6)   # carrier off: level + 0j
    n = len(iq)
    want = api.host_record_pcm16(iq.real.astype(np.float32), 32767.0)
    assert n > 3000 and set(want.tolist()) == {0, 32767}
    a, b = str(tmp_path / 'host.wav'), str(tmp_path / 'dev.wav')
    with rec_mod.record(a, 2e6) as r:     # from the host: complex64, in two pieces (one of them interleaved float32)
        assert r.write(iq[:1001]) == 1001
        assert r.write(iq[1001:].view(np.float32)) == n - 1001
    buf = api.DeviceBuffer(np.zeros(0, np.float32), nbytes=8 * n)
    try:                                   # from device memory: what k_tx_render left there, no host copy of the complex64
        got, _ = tx.render_device(runs, 2e6, buf.ptr, n)
        assert got == n
        with rec_mod.record(b, 2e6) as r:
            assert r.write_device(buf.ptr, n) == n
    finally:
        buf.free()
    for p in (a, b):
        fmt, frames = read_wav(p)
        assert fmt == (1, 2, 2000000) and np.array_equal(frames, want), p
    # another gain, carrier on: still the host twin of the real part
    iqc = tx.render(runs, 2e6, carrier=True, freq=13.56e6, amp=0.5)
    with rec_mod.record(a, 2e6, gain=1000.5) as r:
        r.write(iqc)
    assert np.array_equal(read_wav(a)[1], api.host_record_pcm16(iqc.real.astype(np.float32), 1000.5))
    # the recording decodes through the GPU path as the C oracle decodes the same PCM's envelope (the WAV branch: hi_val 1.09)
    g = _run_decoder(b)
    o = co.COracle(samp_rate=2e6, hi_val=1.09)
    o.push_env(api.host_envelope(want, api.NFC_IN_I16_SQ, 0.0))
    assert g['transitions'] == o.transitions() and len(g['transitions']) > 10
    assert g['sym_tag'] == o.symbols(0).tolist() and g['sym_reader'] == o.symbols(1).tolist()
    assert g['packets'] == o.packets()
