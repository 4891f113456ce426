"""Complex int16 IQ input (NFC_IN_IQ_I16, sc16: what a USRP sends over the wire).  A sample is two little-endian int16, I first;
I and Q are converted as the PCM kind converts a sample (i16_scale) and the envelope is the fc32 kind's of the converted pair.  The
property pinned here: an sc16 capture gives outputs bit-identical to the fc32 kind run on the host-converted capture, and to the
C oracle (and, on the committed fixture, to the unmodified reference).  The kind's kernels live in a translation unit of their own,
csrc/nfc_iq16.hip, audited here on the CPU like nfc_amd.hip's (tests/test_isa_audit.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.golden_util import Case, load_npz
from usrp_nfc_amd import _lib, api, decoder as dec, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [0.0, 2.0 ** -15, 1.0 / 20000.0]


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_iq16_translation_unit_isa_audit(tmp_path):
    from usrp_nfc_amd import build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-shared')]
    asm = str(tmp_path / 'nfc_iq16.s')
    subprocess.check_call([hipcc] + flags + ['-S', '--cuda-device-only', os.path.join(build.CSRC, 'nfc_iq16.hip'), '-o', asm],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'audit_lean_isa.py'), asm], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        m = re.match(r'(_ZN3nfc1[46]k_threshold_(?:lean|wg)\w+):', line)
        if m:
            got[m.group(1)] = line
    want = {'_ZN3nfc14k_threshold_wgILi4ELi4ELb0EEEvNS_7ThrArgsE', '_ZN3nfc14k_threshold_wgILi4ELi8ELb0EEEvNS_7ThrArgsE',
            '_ZN3nfc14k_threshold_wgILi4ELi4ELb1EEEvNS_7ThrArgsE', '_ZN3nfc16k_threshold_leanILi4ELi4ELb1EEEvNS_7ThrArgsE',
            '_ZN3nfc16k_threshold_leanILi4ELi4ELb0EEEvNS_7ThrArgsE'}
    assert set(got) == want, r.stdout
    assert all(l.endswith(' 0 findings') for l in got.values()), r.stdout


def test_header_enum_matches_ctypes():
    h = open(os.path.join(ROOT, 'include', 'nfc_amd.h')).read()
    m = re.search(r'\bNFC_IN_IQ_I16\s*=\s*(\d+)', h)
    assert m and int(m.group(1)) == _lib.NFC_IN_IQ_I16 == api.NFC_IN_IQ_I16 == 4
    assert api._KIND_DTYPE[api.NFC_IN_IQ_I16] == (np.int16, 2)


def test_loader_maps_complex_int16(tmp_path):
    rng = np.random.default_rng(5)
    iq16 = rng.integers(-32768, 32768, 2 * 1000).astype(np.int16)
    for ext in ('.sc16', '.cs16', '.ci16', '.SC16'):
        p = str(tmp_path / ('cap' + ext))
        iq16.astype('<i2').tofile(p)
        a, kind, scale = dec._load_source(p, 0.0, 1.0 / 20000.0)
        assert kind == api.NFC_IN_IQ_I16 and scale == 1.0 / 20000.0 and dec._hi_val(kind) == 1.1
        assert a.dtype == np.int16 and np.array_equal(a, iq16)
    a, kind, scale = dec._load_source(iq16.reshape(-1, 2), 0.0, 0.0)
    assert kind == api.NFC_IN_IQ_I16 and scale == 0.0 and np.array_equal(a, iq16)
    a, kind, scale = dec._load_source(iq16, 0.5, 0.0)   # a 1-D int16 array stays 16-bit PCM
    assert kind == api.NFC_IN_I16_SQ and scale == 0.5 and dec._hi_val(kind) == 1.09
    assert dec._hi_val(api.NFC_IN_IQ_F32) == 1.1


def test_host_envelope_is_the_fc32_envelope_of_the_converted_pair():
    rng = np.random.default_rng(6)
    tail = [0, 0, 32767, -32768, -32768, -32768, 32767, 32767, 1, -1]
    iq16 = np.concatenate([rng.integers(-32768, 32768, 20000), tail]).astype(np.int16)
    for s in SCALES:
        conv = api.host_i16_to_float(iq16, s)
        assert conv.dtype == np.float32
        env = api.host_envelope(iq16, api.NFC_IN_IQ_I16, s)
        assert env.dtype == np.float32 and len(env) == len(iq16) // 2
        assert np.array_equal(env.view(np.uint32), api.host_envelope(conv, api.NFC_IN_IQ_F32).view(np.uint32))
        assert np.array_equal(api.host_envelope(iq16.reshape(-1, 2), api.NFC_IN_IQ_I16, s).view(np.uint32), env.view(np.uint32))
        assert np.all(np.isfinite(env)) and np.all(env >= 0)
    # the other kinds, for the record: what the kernels square
    x = rng.standard_normal(100).astype(np.float32)
    assert np.array_equal(api.host_envelope(x, api.NFC_IN_ENV_F32), x)
    assert np.array_equal(api.host_envelope(x, api.NFC_IN_REAL_F32_SQ), x * x)
    assert np.array_equal(api.host_envelope(x, api.NFC_IN_IQ_F32), synth.envelope_f32(x))


@pytest.mark.parametrize('scale', SCALES)
def test_host_conversion_equals_the_kernels_on_every_int16(scale):
    L = _lib.load()
    v = np.arange(-32768, 32768, dtype=np.int32)
    want = np.array([L.nfc_host_i16_to_float(int(k), scale) for k in v], np.float32)
    assert np.array_equal(api.host_i16_to_float(v.astype(np.int16), scale).view(np.uint32), want.view(np.uint32))


def test_quantise_rounds_and_clips():
    q = synth.quantise_sc16(np.array([0.5, -0.5, 1.5, -1.5, 2.5 / 32767, 0.0], np.float32))
    assert q.dtype == np.int16
    assert q.tolist() == [16384, -16384, 32767, -32768, 2, 0]


def test_scale_beyond_2_48_is_rejected():
    # (checked before nfc_create looks for a device: the same answer with and without a GPU)
    with pytest.raises(api.NfcError, match='i16_scale'):
        api.NfcContext(input_kind=api.NFC_IN_IQ_I16, i16_scale=2.0 ** 49)
    with pytest.raises(api.NfcError, match='i16_scale'):
        api.NfcContext(input_kind=api.NFC_IN_IQ_I16, i16_scale=float('inf'))


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


def check_iq16(iq16, params, scale=0.0, val=True, **kw):
    """sc16 through the path == fc32 on the host-converted capture == the C oracle (push_iq of the converted floats)."""
    from oracle import c_oracle as co
    conv = api.host_i16_to_float(iq16, scale)
    r = run_gpu(iq16, params, api.NFC_IN_IQ_I16, i16_scale=scale, val=val, **kw)
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
def test_reference_fixture():
    # the Ultralight transaction quantised to sc16; the outputs are the unmodified reference's on its envelope (make_iq16_golden.py)
    c = Case('fx_ultralight_sc16')
    iq16 = load_npz('fx_ultralight_sc16.npz')['iq16']
    assert iq16.dtype == np.int16 and len(iq16) == 2 * len(c.x) and c.params['hi_val'] == 1.1
    assert np.array_equal(api.host_envelope(iq16, api.NFC_IN_IQ_I16).view(np.uint32), c.x.view(np.uint32))
    assert len(c.packets) > 10
    n = len(c.x)
    for kw in (dict(), dict(chunk_samples=256), dict(pushes=[0, 1001, 2000, 2001, 7001, n])):
        _check_case(c, check_iq16(iq16, c.params, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['sequential', 'general', 'lean'])
def test_kernel_forms(monkeypatch, form):
    iq16 = synth.quantise_sc16(synth.workload('all', 400_000))
    flags = 0
    if form == 'sequential':
        flags = api.NFC_FLAG_FORCE_SEQUENTIAL
    elif form == 'general':
        monkeypatch.setenv('NFC_LEAN', '0')
    else:
        monkeypatch.setenv('NFC_WG', '0')
    r = check_iq16(iq16, dict(hi_val=1.1), flags=flags)
    assert len(r['packets']) > 10
    if form == 'sequential':
        assert r['stats'].used_sequential == 1
    check_iq16(iq16, dict(hi_val=1.1), flags=flags, chunk_samples=0 if form == 'sequential' else 256,
               pushes=[0, 1001, 2000, 2001, 7001, 150_000, len(iq16) // 2])


@pytest.mark.gpu
def test_eight_rows_per_step_at_10msps(monkeypatch):
    monkeypatch.setenv('NFC_WG_NR', '8')
    iq16 = synth.quantise_sc16(synth.workload('all', 1_200_000, rate_msps=10.0))
    r = check_iq16(iq16, dict(hi_val=1.1, samp_rate=1e7, av_window=10000, max_len=250), chunk_samples=22528)
    assert len(r['transitions']) > 1000


@pytest.mark.gpu
def test_in_place_reruns_and_hovering(monkeypatch):
    # level steps behind losses of signal: failing chunks re-run by k_threshold_wg<IN_IQ_I16, 4, true>
    iq16 = synth.quantise_sc16(synth.stress_workload(3_000_000, depth=0.08, sigma=0.002, every=250_000))
    r = check_iq16(iq16, dict(hi_val=1.1), val=False)
    st = r['stats']
    assert st.used_sequential == 0 and st.chunks_rerun_in_place > 0, (st.chunks_rerun, st.chunks_rerun_in_place)
    # the capture whose loaded half bits hover at the HIGH threshold (five times the noise)
    hov = synth.quantise_sc16(synth.stress_workload(1_000_000))
    check_iq16(hov, dict(hi_val=1.1))
    monkeypatch.setenv('NFC_WG_EX', '100000')   # (the product sends a batch where every chunk fails to k_threshold: here the in-place form takes them)
    r = check_iq16(hov, dict(hi_val=1.1))
    assert r['stats'].chunks_rerun_in_place > 0


@pytest.mark.gpu
def test_short_batches_and_scales():
    iq16 = synth.quantise_sc16(synth.workload('all', 1 << 18))
    for s in SCALES:   # (a batch of at most 2^18 samples: the edge, decode and framing stages in one launch)
        r = check_iq16(iq16, dict(hi_val=1.1), scale=s)
        assert len(r['packets']) > 10, s
    # ... cut anywhere; with a scale that is not a power of two the pair's squares round differently: still the fc32 kind's
    check_iq16(iq16, dict(hi_val=1.1), scale=1.0 / 20000.0, pushes=[0, 2000, 2001, 100_000, 1 << 18])
    api.NfcContext(input_kind=api.NFC_IN_IQ_I16, i16_scale=2.0 ** 48).close()   # (the largest scale accepted)


@pytest.mark.gpu
def test_zeros_and_full_scale():
    # runs of I = Q = 0 longer than the window at the start and in mid-stream (the window sum reaches 0: transition_sink.py:58-62),
    # and samples at +-32767 / -32768
    iq16 = synth.quantise_sc16(synth.workload('all', 300_000)).reshape(-1, 2)
    iq16[:2500] = 0
    iq16[100_000:103_000] = 0
    iq16[150_000:150_040] = [32767, 32767]
    iq16[150_040:150_080] = [-32768, -32768]
    iq16[200_000:200_010] = [-32768, 32767]
    iq16 = iq16.reshape(-1)
    for kw in (dict(), dict(chunk_samples=256), dict(pushes=[0, 2499, 2500, 2501, 100_001, 150_040, 300_000]),
               dict(flags=api.NFC_FLAG_FORCE_SEQUENTIAL)):
        check_iq16(iq16, dict(hi_val=1.1), **kw)


@pytest.mark.gpu
def test_batches_submitted_ahead():
    n = 2_000_000
    iq16 = synth.quantise_sc16(synth.workload('miller', n))
    one = run_gpu(iq16, dict(hi_val=1.1), api.NFC_IN_IQ_I16, val=False)
    cuts = [0, 400_000, 800_000, 1_200_000, 1_600_000, n]
    bufs = [api.DeviceBuffer(iq16[2 * a:2 * b]) for a, b in zip(cuts[:-1], cuts[1:])]
    lens = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    tr, s0, s1, pk, ahead = [], [], [], [], []
    with api.NfcContext(input_kind=api.NFC_IN_IQ_I16, hi_val=1.1) as ctx:
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
def test_state_round_trip_prime_and_val():
    # what does not depend on the kind: the boundary state carried across contexts (get / set), nfc_prime (a level in envelope
    # units, here api.host_envelope's), and the per-sample classification (nfc_read_val), also with NFC_FLAG_NO_EDGES
    iq16 = synth.quantise_sc16(synth.workload('all', 300_000))
    whole = run_gpu(iq16, dict(hi_val=1.1), api.NFC_IN_IQ_I16)
    cut = 123_457
    with api.NfcContext(input_kind=api.NFC_IN_IQ_I16, hi_val=1.1) as a:
        a.push(iq16[:2 * cut])
        tr, pk = a.transitions(), a.packets()
        blob = a.state_blob()
    with api.NfcContext(input_kind=api.NFC_IN_IQ_I16, hi_val=1.1) as b:
        b.set_state_blob(blob)
        b.push(iq16[2 * cut:])
        tr += b.transitions()
        pk += b.packets()
    assert tr == whole['transitions'] and pk == whole['packets']
    # primed at the carrier level the capture starts with, the context must converge to the true state within the overlap
    from usrp_nfc_amd import sharding
    level = sharding.carrier_level(api.host_envelope(iq16[:2 * 4096], api.NFC_IN_IQ_I16))
    ov = 2 * sharding.shard_overlap(2e6, 2000)
    start = ov + 20_000
    with api.NfcContext(input_kind=api.NFC_IN_IQ_I16, hi_val=1.1) as p:
        p.prime(start - ov, level)
        p.push(iq16[2 * (start - ov):2 * start])
        assert p.window_converged()
        p.push(iq16[2 * start:])
        assert p.val().tolist() == whole['val'][start:]
    with api.NfcContext(input_kind=api.NFC_IN_IQ_I16, hi_val=1.1, flags=api.NFC_FLAG_NO_EDGES) as c:
        c.push(iq16)
        assert c.val().tolist() == whole['val']


@pytest.mark.gpu
def test_four_time_shards_at_10msps():
    # test_sharding.py's four-shard run at 10 Msps with sc16 input (nfc_prime's level from api.host_envelope): the concatenated
    # outputs are the oracle's over the whole capture
    import threading
    from oracle import c_oracle as co
    from tests.test_sharding import ThreadComm
    from usrp_nfc_amd import sharding
    world, n_per = 4, 700_000
    params = dict(samp_rate=10e6, hi_val=1.1, av_window=10000, max_len=250)
    gold = os.path.join(os.path.dirname(__file__), 'golden', '1k_with_enc.out')
    frames, _ = synth.frames_from_trace(gold)
    m = synth.tiled_profile(synth.modulation_profile(frames, rate_msps=10.0, lead_in=0, tail=0), world * n_per)
    m[:15000] = 1.0
    iq16 = synth.quantise_sc16(synth.iq_from_profile(m, seed=11))
    overlap = sharding.shard_overlap(10e6, 10000)
    o = co.COracle(**params)
    o.push_iq(api.host_i16_to_float(iq16))
    shared = ThreadComm.Shared(world)
    results, errors = [None] * world, []

    def run(rank):
        try:
            lo = rank * n_per
            nov = overlap if rank else 0
            own = iq16[2 * lo:2 * (lo + n_per)]
            ov = iq16[2 * (lo - nov):2 * lo]
            ctx = api.NfcContext(input_kind=api.NFC_IN_IQ_I16, **params)
            comm = ThreadComm(shared, rank)
            level = sharding.carrier_level(api.host_envelope(ov[:2 * 4096], api.NFC_IN_IQ_I16)) if rank else 0.0
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
def test_decoder_and_sink(tmp_path):
    iq16 = load_npz('fx_ultralight_sc16.npz')['iq16']
    p16 = str(tmp_path / 'cap.sc16')
    p32 = str(tmp_path / 'cap.fc32')
    iq16.astype('<i2').tofile(p16)
    api.host_i16_to_float(iq16).astype('<f4').tofile(p32)
    a = dec.decoder(p16, batch=10_000).run()
    b = dec.decoder(p32, batch=10_000).run()
    assert a.packets == b.packets and len(a.packets) > 10
    assert dec.decoder(iq16.reshape(-1, 2)).run().packets == b.packets
    # transition_sink.work(): items are I,Q pairs ((n, 2) int16, what uhd.usrp_source emits with cpu_format="sc16"), the return
    # value counts items, and the concatenated callbacks are the fc32 kind's on the converted capture
    from usrp_nfc_amd.transition_sink import transition_sink
    got, want = [], []
    s16 = transition_sink(2e6, got.extend, hi_val=1.1, input_kind=api.NFC_IN_IQ_I16, flush_ms=0, batch=1)
    s32 = transition_sink(2e6, want.extend, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, flush_ms=0, batch=1)
    pairs = iq16.reshape(-1, 2)
    conv = api.host_i16_to_float(iq16)
    for a0, b0 in ((0, 777), (777, 9000), (9000, len(pairs))):
        assert s16.work([pairs[a0:b0]], None) == b0 - a0
        s32.work([conv[2 * a0:2 * b0]], None)
    s16.close()
    s32.close()
    assert got == want and len(got) > 1000
