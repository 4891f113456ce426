"""Complex 8-bit IQ input: NFC_IN_IQ_I8 (sc8: two int8 per sample, I first -- a HackRF's samples) and NFC_IN_IQ_U8 (cu8: two
offset-binary bytes, I first -- an RTL-SDR's).  I and Q are converted, s = fl(q * scale) or s = fl((u - 127.5) * scale), and the
envelope is the fc32 kind's of the converted pair.  The property pinned here: an 8-bit capture gives outputs bit-identical to the fc32
kind run on the host-converted capture, and to the C oracle (and, on the committed fixtures, to the unmodified reference).  A power-of-two
scale takes the kernels' integer route (one dot product per sample), any other the float route (threshold.hip.h: iq8_env); both run
here.  The kinds' kernels live in a translation unit of their own, csrc/nfc_iq8.hip, audited here on the CPU like nfc_amd.hip's."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.golden_util import Case, load_npz
from usrp_nfc_amd import _lib, api, decoder as dec, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {'sc8': api.NFC_IN_IQ_I8, 'cu8': api.NFC_IN_IQ_U8}
QUANT = {api.NFC_IN_IQ_I8: synth.quantise_sc8, api.NFC_IN_IQ_U8: synth.quantise_cu8}
DTYPE = {api.NFC_IN_IQ_I8: np.int8, api.NFC_IN_IQ_U8: np.uint8}
POW2, NONPOW2 = [0.0, 2.0 ** -3], [1.0 / 100.0]
HOST_SCALES = [0.0, 2.0 ** -7, 2.0 ** -3, 1.0 / 100.0, 2.0 ** 56]


def all_pairs(kind):
    """Every one of the 65 536 byte pairs, interleaved (I = low byte of the index, Q = high byte)."""
    v = np.arange(65536, dtype=np.uint32)
    pairs = np.stack([v & 0xFF, v >> 8], axis=1).astype(np.uint8).reshape(-1)
    return pairs.view(DTYPE[kind])


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_iq8_translation_unit_isa_audit(tmp_path):
    from usrp_nfc_amd import build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-shared')]
    asm = str(tmp_path / 'nfc_iq8.s')
    subprocess.check_call([hipcc] + flags + ['-S', '--cuda-device-only', os.path.join(build.CSRC, 'nfc_iq8.hip'), '-o', asm],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'audit_lean_isa.py'), asm], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        m = re.match(r'(_ZN3nfc1[46]k_threshold_(?:lean|wg)\w+):', line)
        if m:
            got[m.group(1)] = line
    want = set()
    for k in (5, 6):
        want |= {'_ZN3nfc14k_threshold_wgILi%dELi4ELb0EEEvNS_7ThrArgsE' % k, '_ZN3nfc14k_threshold_wgILi%dELi8ELb0EEEvNS_7ThrArgsE' % k,
                 '_ZN3nfc14k_threshold_wgILi%dELi4ELb1EEEvNS_7ThrArgsE' % k, '_ZN3nfc16k_threshold_leanILi%dELi4ELb1EEEvNS_7ThrArgsE' % k,
                 '_ZN3nfc16k_threshold_leanILi%dELi4ELb0EEEvNS_7ThrArgsE' % k}
    assert set(got) == want, r.stdout
    assert all(l.endswith(' 0 findings') for l in got.values()), r.stdout
    # both routes are in every workgroup kernel: the integer route's dot products and the float route's packed multiplies
    text = open(asm).read()
    for k, dot in ((5, 'v_dot4c_i32_i8'), (6, 'v_dot4_u32_u8')):
        body = re.search(r'^_ZN3nfc14k_threshold_wgILi%dELi4ELb0EEEvNS_7ThrArgsE:(.*?)\.end_amdhsa_kernel' % k, text, re.S | re.M).group(1)
        assert dot in body and 'v_pk_mul_f32' in body, k


def test_header_enum_matches_ctypes():
    h = open(os.path.join(ROOT, 'include', 'nfc_amd.h')).read()
    for name, v in (('NFC_IN_IQ_I8', 5), ('NFC_IN_IQ_U8', 6)):
        m = re.search(r'\b%s\s*=\s*(\d+)' % name, h)
        assert m and int(m.group(1)) == getattr(_lib, name) == getattr(api, name) == v
        assert name in api.__all__
    assert api._KIND_DTYPE[api.NFC_IN_IQ_I8] == (np.int8, 2)
    assert api._KIND_DTYPE[api.NFC_IN_IQ_U8] == (np.uint8, 2)


def test_loader_maps_complex_8bit(tmp_path):
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, 2 * 1000).astype(np.uint8)
    for ext, kind in (('.cs8', api.NFC_IN_IQ_I8), ('.sc8', api.NFC_IN_IQ_I8), ('.ci8', api.NFC_IN_IQ_I8), ('.CS8', api.NFC_IN_IQ_I8),
                      ('.Sc8', api.NFC_IN_IQ_I8), ('.cu8', api.NFC_IN_IQ_U8), ('.CU8', api.NFC_IN_IQ_U8)):
        p = str(tmp_path / ('cap' + ext))
        raw.tofile(p)
        a, k, scale = dec._load_source(p, 0.0, 0.0, 1.0 / 100.0)
        assert k == kind and scale == 1.0 / 100.0 and dec._hi_val(k) == 1.1, ext
        assert a.dtype == DTYPE[kind] and np.array_equal(a.view(np.uint8), raw), ext
    for kind in KINDS.values():
        x = raw.view(DTYPE[kind])
        a, k, scale = dec._load_source(x.reshape(-1, 2), 0.0, 0.5, 0.25)
        assert k == kind and scale == 0.25 and a.dtype == DTYPE[kind] and np.array_equal(a, x)
    a, k, _ = dec._load_source(raw.view(np.int8), 0.0)   # a 1-D int8 array is not IQ: it stays a real recording
    assert k == api.NFC_IN_REAL_F32_SQ


def _converted(a, kind, scale):
    """The definition in float64, rounded once to float32 (q * s and (u - 127.5) * s are exact in float64)."""
    s = np.float64(np.float32(scale if scale > 0 else 2.0 ** -7))
    v = a.astype(np.float64) - (127.5 if kind == api.NFC_IN_IQ_U8 else 0.0)
    return (v * s).astype(np.float32)


@pytest.mark.parametrize('name', sorted(KINDS))
def test_host_envelope_on_every_byte_pair(name):
    kind = KINDS[name]
    pairs = all_pairs(kind)
    for s in HOST_SCALES:
        conv = _converted(pairs, kind, s)
        assert np.array_equal(api.host_iq8_to_float(pairs, kind, s).view(np.uint32), conv.view(np.uint32)), s
        env = api.host_envelope(pairs, kind, s)
        assert env.dtype == np.float32 and len(env) == 65536
        assert np.array_equal(env.view(np.uint32), api.host_envelope(conv, api.NFC_IN_IQ_F32).view(np.uint32)), s
        assert np.array_equal(api.host_envelope(pairs.reshape(-1, 2), kind, s).view(np.uint32), env.view(np.uint32))
        assert np.all(np.isfinite(env)) and np.all(env >= 0), s
        if s != 1.0 / 100.0:   # a power of two: the integer route's value, (2 I / s)^2 + (2 Q / s)^2 exactly, times s^2 / 4
            sc = np.float64(s if s > 0 else 2.0 ** -7)
            d = 2.0 * pairs.astype(np.float64) - (255.0 if kind == api.NFC_IN_IQ_U8 else 0.0)
            exact = (d[0::2] ** 2 + d[1::2] ** 2) * (sc * sc / 4.0)
            assert np.array_equal(env.astype(np.float64), exact), s
    assert env.max() <= np.float32(2.0 ** 127)   # 2^56: the largest scale accepted keeps the envelope finite


def test_quantisers_round_and_clip():
    v = np.array([0.5, -0.5, 1.5, -1.5, 2.5 / 127, 0.5 / 127, 0.0, -2.0], np.float32)
    q = synth.quantise_sc8(v)
    assert q.dtype == np.int8 and q.tolist() == [64, -64, 127, -128, 2, 0, 0, -128]
    u = synth.quantise_cu8(v)   # 127.5 + v * 127, ties to even
    assert u.dtype == np.uint8 and u.tolist() == [191, 64, 255, 0, 130, 128, 128, 0]
    # ties at full_scale 2: 127.5 + 0.5 = 128 (exact), 128.5 -> 128, 126.5 -> 126, 129.5 -> 130
    assert synth.quantise_cu8(np.array([0.25, 0.5, -0.5, 1.0], np.float32), 2.0).tolist() == [128, 128, 126, 130]
    assert synth.quantise_sc8(np.array([0.25, 0.75, -0.25, -0.75], np.float32), 2.0).tolist() == [0, 2, 0, -2]


@pytest.mark.parametrize('name', sorted(KINDS))
def test_scale_beyond_2_56_is_rejected(name):
    # (checked before nfc_create looks for a device: the same answer with and without a GPU)
    for bad in (2.0 ** 57, 2.0 ** 56 * (1 + 2.0 ** -23), float('inf')):
        with pytest.raises(api.NfcError, match='i16_scale'):
            api.NfcContext(input_kind=KINDS[name], i16_scale=bad)


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def _first_diff(a, b):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i, a[i], b[i]
    return (n, None, None) if len(a) != len(b) else None


def run_gpu(x, params, kind, pushes=None, flags=0, chunk_samples=0, i16_scale=0.0, val=True):
    ctx = api.NfcContext(input_kind=kind, flags=flags, chunk_samples=chunk_samples, i16_scale=i16_scale, **params)
    per = api._KIND_DTYPE[kind][1]
    n = len(x) // per
    cuts = [0, n] if pushes is None else pushes
    tr, s0, s1, pk, vv = [], [], [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ctx.push(x[a * per:b * per])
        tr += ctx.transitions()
        s0 += ctx.symbols(0).tolist()
        s1 += ctx.symbols(1).tolist()
        pk += ctx.packets()
        if val:
            vv += ctx.val().tolist()
    st = ctx.stats()
    ctx.close()
    return dict(transitions=tr, sym_tag=s0, sym_reader=s1, packets=pk, val=vv, stats=st)


def check_iq8(iq8, kind, params, scale=0.0, val=True, **kw):
    """8-bit IQ through the path == fc32 on the host-converted capture == the C oracle (push_iq of the converted floats)."""
    from oracle import c_oracle as co
    conv = api.host_iq8_to_float(iq8, kind, scale)
    r = run_gpu(iq8, params, kind, i16_scale=scale, val=val, **kw)
    f = run_gpu(conv, params, api.NFC_IN_IQ_F32, val=val, **kw)
    o = co.COracle(trace=val, **params)
    o.push_iq(conv)
    if val:
        L = params.get('av_window', 2000)
        d = _first_diff(r['val'][L:], o.trace().tolist())
        assert d is None, 'val %s' % (d,)
    d = _first_diff(r['transitions'], o.transitions())
    assert d is None, 'transition %s' % (d,)
    assert r['sym_tag'] == o.symbols(0).tolist()
    assert r['sym_reader'] == o.symbols(1).tolist()
    assert r['packets'] == o.packets()
    for k in ('transitions', 'sym_tag', 'sym_reader', 'packets', 'val'):
        assert r[k] == f[k], k
    return r


def _check_case(c, r):
    d = _first_diff(r['transitions'], c.transitions)
    assert d is None, 'transition %s' % (d,)
    assert r['sym_tag'] == c.sym_tag.tolist()
    assert r['sym_reader'] == c.sym_reader.tolist()
    assert r['packets'] == c.packets


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_reference_fixture(name):
    # the Ultralight transaction quantised to 8 bits; the outputs are the unmodified reference's on its envelope (make_iq8_golden.py)
    kind = KINDS[name]
    c = Case('fx_ultralight_%s' % name)
    iq8 = load_npz('fx_ultralight_%s.npz' % name)['iq8']
    assert iq8.dtype == DTYPE[kind] and len(iq8) == 2 * len(c.x) and c.params['hi_val'] == 1.1
    assert np.array_equal(api.host_envelope(iq8, kind).view(np.uint32), c.x.view(np.uint32))
    assert len(c.packets) > 10
    n = len(c.x)
    for kw in (dict(), dict(chunk_samples=256), dict(pushes=[0, 1001, 2000, 2001, 7001, n])):
        _check_case(c, check_iq8(iq8, kind, c.params, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_device_conversion_tap(name):
    # exactly av_window samples into a fresh context fill its ring with their envelopes (transition_sink.work's first window,
    # transition_sink.py:110-124): the ring read back is the kernels' conversion itself, which must be host_envelope's bit for bit
    kind = KINDS[name]
    pairs = all_pairs(kind)
    for s in (0.0, 2.0 ** -3, 2.0 ** -60, 1.0 / 100.0, 3.0):
        want = api.host_envelope(pairs, kind, s)
        for a in range(0, 65536, 30000):
            b = min(a + 30000, 65536)
            with api.NfcContext(input_kind=kind, i16_scale=s, hi_val=1.1, av_window=b - a) as ctx:
                ctx.push(pairs[2 * a:2 * b])
                _, ring, _ = ctx.get_state()
            assert np.array_equal(ring.view(np.uint32), want[a:b].view(np.uint32)), (s, a, _first_diff(ring.tolist(), want[a:b].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
@pytest.mark.parametrize('form', ['default', 'sequential', 'general', 'lean'])
def test_kernel_forms(monkeypatch, name, form):
    kind = KINDS[name]
    iq8 = QUANT[kind](synth.workload('all', 400_000))
    flags = 0
    if form == 'sequential':
        flags = api.NFC_FLAG_FORCE_SEQUENTIAL
    elif form == 'general':
        monkeypatch.setenv('NFC_LEAN', '0')
    elif form == 'lean':
        monkeypatch.setenv('NFC_WG', '0')
    for s in (POW2[0], NONPOW2[0]):
        r = check_iq8(iq8, kind, dict(hi_val=1.1), scale=s, flags=flags)
        assert len(r['packets']) > 10
        if form == 'sequential':
            assert r['stats'].used_sequential == 1
    check_iq8(iq8, kind, dict(hi_val=1.1), flags=flags, chunk_samples=0 if form == 'sequential' else 256,
              pushes=[0, 1001, 2000, 2001, 7001, 150_000, len(iq8) // 2])


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_eight_rows_per_step_at_10msps(monkeypatch, name):
    monkeypatch.setenv('NFC_WG_NR', '8')
    kind = KINDS[name]
    iq8 = QUANT[kind](synth.workload('all', 1_200_000, rate_msps=10.0))
    for s in (POW2[0], NONPOW2[0]):
        r = check_iq8(iq8, kind, dict(hi_val=1.1, samp_rate=1e7, av_window=10000, max_len=250), scale=s, chunk_samples=22528)
        assert len(r['transitions']) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_in_place_reruns_and_hovering(monkeypatch, name):
    # level steps behind losses of signal: failing chunks re-run by k_threshold_wg<KIND, 4, true>
    kind = KINDS[name]
    q = QUANT[kind]
    iq8 = q(synth.stress_workload(3_000_000, depth=0.08, sigma=0.002, every=250_000))
    r = check_iq8(iq8, kind, dict(hi_val=1.1), val=False)
    st = r['stats']
    assert st.used_sequential == 0 and st.chunks_rerun_in_place > 0, (st.chunks_rerun, st.chunks_rerun_in_place)
    # the capture whose loaded half bits hover at the HIGH threshold
    hov = q(synth.stress_workload(1_000_000))
    check_iq8(hov, kind, dict(hi_val=1.1), scale=NONPOW2[0])
    monkeypatch.setenv('NFC_WG_EX', '100000')   # (here the in-place form takes every failing chunk)
    r = check_iq8(hov, kind, dict(hi_val=1.1))
    assert r['stats'].chunks_rerun_in_place > 0


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_short_batches_and_scales(name):
    kind = KINDS[name]
    iq8 = QUANT[kind](synth.workload('all', 1 << 18))
    for s in POW2 + NONPOW2:   # (a batch of at most 2^18 samples: the edge, decode and framing stages in one launch)
        r = check_iq8(iq8, kind, dict(hi_val=1.1), scale=s)
        assert len(r['packets']) > 10, s
    for s in (POW2[1], NONPOW2[0]):   # ... cut anywhere, on both routes
        check_iq8(iq8, kind, dict(hi_val=1.1), scale=s, pushes=[0, 2000, 2001, 100_000, 1 << 18])
    api.NfcContext(input_kind=kind, i16_scale=2.0 ** 56).close()   # (the largest scale accepted)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_zeros_and_full_scale(name):
    # runs of zero bytes and of full-scale bytes longer than the window, at the start and in mid-stream: sc8's 0 is a zero sample
    # (the window sum reaches 0: transition_sink.py:58-62); cu8's 0 and 255 are its extremes, -127.5 and 127.5
    kind = KINDS[name]
    iq8 = QUANT[kind](synth.workload('all', 300_000)).reshape(-1, 2)
    lo, hi = (-128, 127) if kind == api.NFC_IN_IQ_I8 else (0, 255)
    iq8[:2500] = 0
    iq8[100_000:103_000] = 0
    iq8[150_000:150_040] = [hi, hi]
    iq8[150_040:150_080] = [lo, lo]
    iq8[200_000:200_010] = [lo, hi]
    iq8[250_000:253_000] = [hi, lo]
    iq8 = iq8.reshape(-1)
    for kw in (dict(), dict(chunk_samples=256), dict(pushes=[0, 2499, 2500, 2501, 100_001, 150_040, 300_000]),
               dict(flags=api.NFC_FLAG_FORCE_SEQUENTIAL), dict(scale=NONPOW2[0])):
        check_iq8(iq8, kind, dict(hi_val=1.1), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_batches_submitted_ahead(name):
    kind = KINDS[name]
    n = 2_000_000
    iq8 = QUANT[kind](synth.workload('miller', n))
    one = run_gpu(iq8, dict(hi_val=1.1), kind, val=False)
    cuts = [0, 400_000, 800_000, 1_200_000, 1_600_000, n]
    bufs = [api.DeviceBuffer(iq8[2 * a:2 * b]) for a, b in zip(cuts[:-1], cuts[1:])]
    lens = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    tr, s0, s1, pk, ahead = [], [], [], [], []
    with api.NfcContext(input_kind=kind, hi_val=1.1) as ctx:
        nxt = 0
        for k in range(len(bufs)):
            while nxt < len(bufs) and nxt < k + 2:
                ctx.submit_device(bufs[nxt], lens[nxt])
                nxt += 1
            ctx.wait()
            tr += ctx.transitions()
            s0 += ctx.symbols(0).tolist()
            s1 += ctx.symbols(1).tolist()
            pk += ctx.packets()
            ahead.append(int(ctx.stats().ran_ahead))
    for b in bufs:
        b.free()
    assert tr == one['transitions'] and pk == one['packets']
    assert s0 == one['sym_tag'] and s1 == one['sym_reader']
    assert sum(ahead) > 0, ahead


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_state_round_trip_prime_and_val(name):
    kind = KINDS[name]
    iq8 = QUANT[kind](synth.workload('all', 300_000))
    whole = run_gpu(iq8, dict(hi_val=1.1), kind)
    cut = 123_457
    with api.NfcContext(input_kind=kind, hi_val=1.1) as a:
        a.push(iq8[:2 * cut])
        tr, pk = a.transitions(), a.packets()
        blob = a.state_blob()
    with api.NfcContext(input_kind=kind, hi_val=1.1) as b:
        b.set_state_blob(blob)
        b.push(iq8[2 * cut:])
        tr += b.transitions()
        pk += b.packets()
    assert tr == whole['transitions'] and pk == whole['packets']
    # primed at the carrier level the capture starts with (api.host_envelope's units), the context converges within the overlap
    from usrp_nfc_amd import sharding
    level = sharding.carrier_level(api.host_envelope(iq8[:2 * 4096], kind))
    ov = 2 * sharding.shard_overlap(2e6, 2000)
    start = ov + 20_000
    with api.NfcContext(input_kind=kind, hi_val=1.1) as p:
        p.prime(start - ov, level)
        p.push(iq8[2 * (start - ov):2 * start])
        assert p.window_converged()
        p.push(iq8[2 * start:])
        assert p.val().tolist() == whole['val'][start:]
    with api.NfcContext(input_kind=kind, hi_val=1.1, flags=api.NFC_FLAG_NO_EDGES) as c:
        c.push(iq8)
        assert c.val().tolist() == whole['val']


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_four_time_shards_at_10msps(name):
    # test_sharding.py's four-shard run at 10 Msps with 8-bit input (nfc_prime's level from api.host_envelope): the concatenated
    # outputs are the oracle's over the whole capture
    import threading
    from oracle import c_oracle as co
    from tests.test_sharding import ThreadComm
    from usrp_nfc_amd import sharding
    kind = KINDS[name]
    world, n_per = 4, 700_000
    params = dict(samp_rate=10e6, hi_val=1.1, av_window=10000, max_len=250)
    gold = os.path.join(os.path.dirname(__file__), 'golden', '1k_with_enc.out')
    frames, _ = synth.frames_from_trace(gold)
    m = synth.tiled_profile(synth.modulation_profile(frames, rate_msps=10.0, lead_in=0, tail=0), world * n_per)
    m[:15000] = 1.0
    iq8 = QUANT[kind](synth.iq_from_profile(m, seed=11))
    overlap = sharding.shard_overlap(10e6, 10000)
    o = co.COracle(**params)
    o.push_iq(api.host_iq8_to_float(iq8, kind))
    shared = ThreadComm.Shared(world)
    results, errors = [None] * world, []

    def run(rank):
        try:
            lo = rank * n_per
            nov = overlap if rank else 0
            own = iq8[2 * lo:2 * (lo + n_per)]
            ov = iq8[2 * (lo - nov):2 * lo]
            ctx = api.NfcContext(input_kind=kind, **params)
            comm = ThreadComm(shared, rank)
            level = sharding.carrier_level(api.host_envelope(ov[:2 * 4096], kind)) if rank else 0.0
            redos = sharding.decode_shard(ctx, comm, lambda: ctx.push(ov), lambda: ctx.push(own), lo - nov, level)
            results[rank] = (redos, ctx.transitions(), ctx.packets())
            ctx.close()
        except Exception as e:   # noqa: BLE001 -- a failing rank must not leave the others waiting at the barrier
            errors.append((rank, repr(e)))
            shared.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    assert [t for _, tr, _ in results for t in tr] == o.transitions()
    assert [p for _, _, pk in results for p in pk] == o.packets()
    assert len(o.packets()) > 100
    assert [r[0] for r in results] == [0, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KINDS))
def test_decoder_and_sink(tmp_path, name):
    kind = KINDS[name]
    iq8 = load_npz('fx_ultralight_%s.npz' % name)['iq8']
    p8 = str(tmp_path / ('cap.' + ('cs8' if kind == api.NFC_IN_IQ_I8 else 'cu8')))
    p32 = str(tmp_path / 'cap.fc32')
    iq8.tofile(p8)
    conv = api.host_iq8_to_float(iq8, kind)
    conv.astype('<f4').tofile(p32)
    a = dec.decoder(p8, batch=10_000).run()
    b = dec.decoder(p32, batch=10_000).run()
    assert a.packets == b.packets and len(a.packets) > 10
    assert dec.decoder(iq8.reshape(-1, 2)).run().packets == b.packets
    assert dec.decoder(iq8.reshape(-1, 2), iq8_scale=1.0 / 100.0).run().packets == \
        dec.decoder(api.host_iq8_to_float(iq8, kind, 1.0 / 100.0).view(np.complex64)).run().packets
    # transition_sink.work(): items are I,Q pairs ((n, 2) bytes, what a CS8 / RTL-SDR source emits), the return value counts
    # items, and the concatenated callbacks are the fc32 kind's on the converted capture
    from usrp_nfc_amd.transition_sink import transition_sink
    got, want = [], []
    s8 = transition_sink(2e6, got.extend, hi_val=1.1, input_kind=kind, flush_ms=0, batch=1)
    s32 = transition_sink(2e6, want.extend, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, flush_ms=0, batch=1)
    pairs = iq8.reshape(-1, 2)
    for a0, b0 in ((0, 777), (777, 9000), (9000, len(pairs))):
        assert s8.work([pairs[a0:b0]], None) == b0 - a0
        s32.work([conv[2 * a0:2 * b0]], None)
    s8.close()
    s32.close()
    assert got == want and len(got) > 1000
