"""The air interface on the GPU (nfc_air_render_device: csrc/nfc_air.hip over csrc/air.hip.h) against its twin on the CPU
(nfc_host_air_render, which tests/test_air_host.py pins to synth.py): the same bytes in every used byte of the device buffer, padding
included, the same layout; and the loop closed in HBM -- cards -> transcripts -> captures -> decode -> commands -- with nothing downloaded
between the rendering and the decode.  The device call itself checks the guard words behind its device sections."""
import os

import numpy as np
import pytest

from tests import emu_cards
from tests.golden_util import GOLDEN
from tests.test_air_host import REQA, classic24, ultralight
from tests.test_emulate import _pair
from usrp_nfc_amd import air, api, emulate, fsm

pytestmark = pytest.mark.gpu
KINDS = (api.NFC_IN_IQ_F32, api.NFC_IN_IQ_I16, api.NFC_IN_IQ_I8, api.NFC_IN_IQ_U8)
READT = [ultralight()[11]]   # one 18-byte READT
_cache = {}


def random_transcripts():
    """two random cards of tests/emu_cards.py -- a Classic with keys of its own, an Ultralight -- read on the host by a reader with the
    default keys, at most 24 frames kept"""
    if 'pairs' not in _cache:
        tags, readers = [], []
        for seed in (0, 5):
            tag_type, mem, rands, _ = emu_cards.tag_row(seed)
            tags.append(emulate.tag_card(tag_type, mem, rands or None))
            readers.append(emulate.reader_card(emu_cards.reader_row(seed)[0]))
        t = emulate.pairs_host(tags, readers, pair_cap_frames=[24, 24])
        _cache['pairs'] = [t.transcript(0), t.transcript(1)]
        assert 0 < len(_cache['pairs'][0]) <= 24 and 0 < len(_cache['pairs'][1]) <= 24
    return _cache['pairs']


def seven_streams():
    a, b = random_transcripts()
    return [ultralight(), classic24(), a, b, [], REQA, READT]


def assert_same(dev, host):
    assert dev.first_sample.tolist() == host.first_sample.tolist() and dev.n_samples.tolist() == host.n_samples.tolist()
    assert dev.guard_intact()
    got, want = dev.download_used(), host.download_used()
    assert len(got) == len(want) and len(got) > 0
    assert got.tobytes() == want.tobytes(), 'first differing byte %d' % int(np.nonzero(got != want)[0][0])


@pytest.mark.parametrize('align', [1, 8])
@pytest.mark.parametrize('rate', [2.0, 10.0])
@pytest.mark.parametrize('sigma', [0.0, 0.002])
@pytest.mark.parametrize('kind', KINDS)
def test_device_equals_the_twin_in_every_used_byte(kind, sigma, rate, align):
    fr = air.frames_of(seven_streams(), rate_msps=rate)
    kw = dict(out_kind=kind, sigma=sigma, align_samples=align, stream_seeds=[3, 1, 4, 1, 5, 9, 2])
    dev = air.render_device(fr, **kw)
    try:
        assert_same(dev, air.host_render(fr, **kw))
        assert int(dev.n_samples[4]) == int(150.0 * rate) + 400 and len(dev) == 7
    finally:
        dev.free()


def test_a_frame_longer_than_a_workgroup_s_span_behind_a_long_lead_in():
    fr = air.frames_of([READT, REQA], rate_msps=10.0, lead_in=70000)
    first, n = air.sizes(fr, align_samples=1)
    assert int(n[0]) > 70000 + 15000
    for kind in (api.NFC_IN_IQ_F32, api.NFC_IN_IQ_I8):
        dev = air.render_device(fr, out_kind=kind, align_samples=1, timing=True)
        try:
            assert_same(dev, air.host_render(fr, out_kind=kind, align_samples=1))
            assert dev.kernel_ms[0] > 0 and dev.kernel_ms[1] > 0
        finally:
            dev.free()


def test_device_errors_come_before_the_device_is_touched():
    fr = air.frames_of([ultralight()[:4]])
    with pytest.raises(ValueError) as e:
        air.render_device(fr, align_samples=3)
    assert 'align_samples' in str(e.value)
    with pytest.raises(ValueError) as e:
        air.render_device(fr, cap_samples=100)
    assert 'cap_samples' in str(e.value)


def assert_frames_equal(got, want):
    """two api.NfcFrames: the order of the types, every field of the records but idx (a sample index on one side, a place in the list on
    the other) and n_bits (the length of the PACKET as the decoder closed it, which ends a bit early or late where the frame's last bits
    leave no edge: the synth capture of the same frames decodes to the same lengths), the bytes and the ninth bits"""
    assert got.table['type'].tolist() == want.table['type'].tolist()
    for t in (0, 1):
        for name in ('byte_off', 'n_bytes', 'flags', 'type'):
            assert got.records[t][name].tolist() == want.records[t][name].tolist(), (t, name)
        assert got.bytes[t].tobytes() == want.bytes[t].tobytes() and got.par[t].tobytes() == want.par[t].tobytes()


def three_cards():
    rng = np.random.Generator(np.random.PCG64(3))
    classic = emulate.cards_from_json(os.path.join(GOLDEN, 'fx_emu_classic1k.json'))
    ul = emulate.cards_from_json(os.path.join(GOLDEN, 'fx_emu_ultralight.json'))
    rnd = _pair(2, rng)
    return [classic[0], ul[0], rnd[0]], [classic[1], ul[1], rnd[1]]


def test_the_loop_closed_in_hbm():
    tags, readers = three_cards()
    tr = emulate.pairs_device(tags, readers, pair_cap_frames=[24, 256, 24])
    assert [len(tr.transcript(k)) for k in range(3)] == [24, 19, 20]   # (the random card's reader has no key table: it gives up after 20 frames)
    cap = tr.render_device(out_kind=api.NFC_IN_IQ_I8, sigma=0.002)
    try:
        with api.NfcMultiContext(3, int(cap.n_samples.max()), hi_val=1.1, input_kind=api.NFC_IN_IQ_I8) as m:
            m.track_commands()
            cap.push_to(m)
            raw, cm = m.fetch_frames(), m.fetch_commands()
            for k in range(3):
                want = tr.transcript(k).nfc_frames()
                assert_frames_equal(raw.frames_of(k), want)
                for a, b in zip(cm.commands_of(k), fsm.host_commands(fsm.state_init(), raw.frames_of(k))):
                    assert a.tobytes() == b.tobytes()
            assert (cm.commands_of(0)[0]['cmd'] >= 0).all()
    finally:
        cap.free()
    # one stream in fc32 through a single context
    cap = tr.render_device(out_kind=api.NFC_IN_IQ_F32, sigma=0.002, align_samples=2)
    try:
        ptr, n = cap.context_args(1)
        with api.NfcContext(hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as c:
            c.push_device(ptr, n)
            assert_frames_equal(c.frames(), tr.transcript(1).nfc_frames())
    finally:
        cap.free()
