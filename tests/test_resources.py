"""Nothing leaks: the HIP resources the library's owning handles hold (csrc/dev_buf.h: device blocks, pinned blocks, events, streams --
nfc_debug_live_resources of the test build) are, after a lifecycle, what they were before it.  The library keeps no handle for the life
of the process, so the "before" is taken as it is, with no warm-up.  The counts are per library and cover the handles only: memory a
test gets through the pass-through calls (api.DeviceBuffer: nfc_device_alloc) is the caller's and not among them.

Every assertion that decides a case is an equality of the four counts; the two inequalities say that a living context is seen at all."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests.test_commands import classic_iq
from tests.test_keys_host import all_traces
from usrp_nfc_amd import _lib, api, keys, synth, tx

pytestmark = pytest.mark.gpu
DEVICE, PINNED, EVENTS, STREAMS = range(4)
N_LONG, N_SHORT = 300_000, 4096   # above 2^18: the multi-launch stages / the one-launch kernel of short batches
NFC_ERR_NOMEM = -3
_cache = {}


@pytest.fixture(autouse=True)
def hooks_build(monkeypatch):
    monkeypatch.setenv_plain('NFC_AMD_LIB', _lib.hooks_path())   # every call of this module goes to the one library that counts


def live():
    L = _lib.load(_lib.hooks_path())
    L.nfc_debug_live_resources.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.nfc_debug_live_resources.restype = None
    gc.collect()   # (a context an earlier test dropped without close() goes now, not in the middle of a lifecycle)
    out = (C.c_uint64 * 4)()
    L.nfc_debug_live_resources(C.byref(out))
    return list(out)


def capture():
    """300 000 samples of the whole Ultralight transaction, frames of both directions, interleaved float32 IQ."""
    if 'iq' not in _cache:
        _cache['iq'] = synth.workload('all', N_LONG)
        _cache['iq'].setflags(write=False)
    return _cache['iq']


def lifecycle(ctx, x, per):
    """One context end to end: a long batch and every reader, three batches ahead, a short batch, reset."""
    ctx.push(x)
    c = ctx.counts()
    assert int(c.n_samples) == N_LONG and int(c.n_edges) > 0 and int(c.n_packets[0]) > 0 and int(c.n_packets[1]) > 0   # (both directions)
    ctx.edges()
    ctx.edges_compact()
    for t in (0, 1):
        ctx.symbols(t)
        ctx.packet_table(t)
        ctx.packet_bits(t)
    ctx.packets()
    ctx.frames()
    ctx.get_state()
    third = N_LONG // 3 // 16 * 16   # (a device pointer is 16-byte aligned)
    buf = api.DeviceBuffer(x)
    try:
        for k in range(3):
            ctx.submit_device(buf.ptr.value + k * third * per * x.itemsize, third)
        assert ctx.submitted() == 3
        for k in range(3):
            ctx.wait()
    finally:
        buf.free()
    ctx.push(x[:N_SHORT * per])
    assert int(ctx.counts().n_samples) == N_SHORT
    ctx.reset()


def single_context(kind, x, per, **kw):
    before = live()
    ctx = api.NfcContext(input_kind=kind, **kw)
    try:
        alive = live()
        assert alive[DEVICE] > before[DEVICE] and alive[EVENTS] > before[EVENTS]
        lifecycle(ctx, x, per)
    finally:
        ctx.close()
    assert live() == before


def test_single_context_end_to_end():
    single_context(api.NFC_IN_IQ_F32, capture(), 2)


def test_single_context_of_an_int16_kind():
    single_context(api.NFC_IN_IQ_I16, synth.quantise_sc16(capture()), 2)   # (another kind's kernel table)


def test_multi_stream_context():
    iq = classic_iq()
    first, second = iq[:2 * 8192], iq[2 * 8192:4 * 8192]
    before = live()
    m = api.NfcMultiContext(4, 8192, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32)
    try:
        m.push([first] * 4)
        m.fetch(api.NFC_MULTI_FETCH_ALL)
        m.fetch_frames()
        m.track_commands()
        m.push([second] * 4)
        m.fetch_commands()
        m.set_sector_keys({(0x60, 15): (0xFF,) * 6})
        m.fsm_state(0)
    finally:
        m.close()
    assert live() == before


def test_create_that_cannot_get_its_memory():
    """65 536 streams of 2^24 samples: the second slab alone is beyond the device.  The runtime refuses the allocation; nothing is launched."""
    before = live()
    with pytest.raises(api.NfcError) as e:
        api.NfcMultiContext(65536, 1 << 24, av_window=16)
    assert '(status %d)' % NFC_ERR_NOMEM in str(e.value) and 'no device memory for a slab' in str(e.value)
    assert live() == before   # the stream, the events and the blocks it had got are gone


def test_one_shot_calls():
    before = live()
    results, _ = keys.recover(all_traces()[:1])
    assert int(results['status'][0]) == keys.NFC_KEY_OK
    assert live() == before

    runs = tx.encode_runs(tx.NFC_TX_MILLER, [1, 0, 1, 1, 0, 0, 1, 0])
    n = tx.sample_count(runs, 2e6)
    out = api.DeviceBuffer(np.zeros(0, np.float32), nbytes=max(8 * n, 32))
    try:
        got, ms = tx.render_device(runs, 2e6, out.ptr, n, timed=True)
        assert got == n and ms is not None
        assert live() == before

        pcm = api.DeviceBuffer(np.zeros(0, np.int16), nbytes=2 * n + 32)
        try:
            assert api.record_pcm16_device(out, n, pcm, api.NFC_IN_IQ_F32, timed=True) is not None
        finally:
            pcm.free()
        assert live() == before
    finally:
        out.free()
