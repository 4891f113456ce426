"""The memory images on the GPU (k_multi_images, csrc/image.hip.h; nfc_multi_track_images / nfc_multi_fetch_images): every comparison is
for equality with the CPU twin (emulate.host_card_image, pinned by tests/test_images_host.py) over the commands the same push fetched.
THE TILE IS READ, NOT REMEMBERED: THREADS comes out of the source text, and the cases that sit on a tile's edge assert from it where
their commands fall."""
import hashlib
import os
import re

import numpy as np
import pytest

from tests import emu_cards
from tests import image_util as iu
from tests.test_fsm_fuzz import fixture, full_table, gpu_streams
from usrp_nfc_amd import _lib, air, api, emulate, fsm, keys
from usrp_nfc_amd.command import CommandType

pytestmark = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')
FF = (0xFF,) * 6
_cache = {}


def threads():
    m = re.search(r'constexpr int THREADS = (\d+);', open(os.path.join(CSRC, 'image.hip.h')).read())
    assert m, 'image.hip.h: no definition of THREADS any more'
    return int(m.group(1))


def context(K, max_push, **kw):
    return api.NfcMultiContext(K, int(max_push), hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, **kw)


def twin_of(cm, k, keys_k=None, image=None):
    t, d, _ = cm.commands_of(k)
    return emulate.host_card_image(t, d, keys=keys_k, image=image)


def digest(cm):
    h = hashlib.sha256()
    for a in (cm.cmd_off, cm.cbyte_off, cm.cmd, cm.src, cm.data, cm.enc, cm.stream_flags):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest(), cm.n_launches


# ---- the closed loop ----
def loop_cards():
    mems = [iu.classic_mem(21), iu.ultralight_mem(22), iu.classic_mem(23, {9: emu_cards.access([0, 0, 0, 3])})]
    types = [1, 0, 1]
    rands = [emulate.drawn_rands(5), None, emulate.drawn_rands(6)]
    tags = [emulate.tag_card(t, m, r) for t, m, r in zip(types, mems, rands)]
    readers = [iu.reader_for(m, 7 + k) if t else emulate.reader_card(emulate.drawn_rands(7 + k)) for k, (t, m) in enumerate(zip(types, mems))]
    return mems, types, rands, tags, readers


def test_closed_loop_card_to_capture_to_image_to_card():
    mems, types, rands, tags, readers = loop_cards()
    first = emulate.pairs_device(tags, readers)
    assert [len(first.transcript(k)) for k in (0, 2)] == [199, 199] and threads() * 3 < 199 <= threads() * 4   # four tiles of commands
    caps = first.render_device(sigma=0.0)
    try:
        tables = [keys.sector_table({(0x60, 4 * s): iu.key_a_table(m)[(0x60, s)] for s in range(16)})[0] if t else None for t, m in zip(types, mems)]
        with context(3, max(caps.n_samples), lib_path=_lib.hooks_path()) as m:
            guards = m.L.nfc_debug_multi_guards
            guards.argtypes = [api.C.c_void_p]
            m.track_images()
            for k, table in enumerate(tables):
                if table is not None:
                    m.set_sector_keys(table, stream=k)
            caps.push_to(m)
            assert int(m.stats().n_launches) == 5
            cm, im = m.fetch_commands(), m.fetch_images()
            assert guards(m.h) == 0
            assert im.n_launches == 4 and im.bytes_copied >= 3 * 2112
            again = m.fetch_images()   # no device call: the same data
            assert again.mem_all.tobytes() == im.mem_all.tobytes() and int(m.stats().n_launches) == 5
            for k in range(3):
                twin = twin_of(cm, k, (FF, FF, tables[k]))
                assert iu.images_equal(im, k, twin), k
                assert m.image(k) == twin, k
                size = 1024 if types[k] else 64
                assert (im.mem(k)[:size][im.known_mask(k)[:size]] == mems[k][im.known_mask(k)[:size]]).all()
            assert im.tag_type.tolist() == [1, 0, 1] and im.flags.tolist() == [0, 0, 0]
            assert im.n_known.tolist() == [1024, 64, 1024 - 6] and im.coverage().tolist() == [1.0, 1.0, (1024 - 6) / 1024.0]
            clones = [im.card(k, rands=rands[k]) for k in range(3)]
    finally:
        caps.free()
    second = emulate.pairs_device(clones, readers)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first.arrays(), second.arrays()))


# ---- hostile input ----
def test_images_equal_the_twin_on_the_fuzzed_captures():
    streams, rows = gpu_streams(), fixture()['gpu']
    with context(len(rows), max(len(s) for s in streams) // 2, lib_path=_lib.hooks_path()) as m:
        guards = m.L.nfc_debug_multi_guards
        guards.argtypes = [api.C.c_void_p]
        m.track_images()
        for k, row in enumerate(rows):
            m.set_keys(*row.keys, stream=k)
            if k % 3 == 2:
                m.set_sector_keys(full_table(row.keys), stream=k)
        m.push(streams)
        cm, im = m.fetch_commands(), m.fetch_images()
        assert guards(m.h) == 0
    known = 0
    for k, row in enumerate(rows):
        twin = twin_of(cm, k, (row.keys[0], row.keys[1], full_table(row.keys) if k % 3 == 2 else None))
        assert iu.images_equal(im, k, twin), (k, row.index)
        known += twin.n_known
    assert known > 256 and len(set(im.flags.tolist())) > 1   # (the captures do show memory, and some of them raise flags)


# ---- order inside and across tiles ----
def two_cards_one_uid():
    """Two Ultralights with one UID and different pages, read in turn -- A B A B ... -- in ONE stream: plain frames, so any list of them is
    a capture."""
    if 'ab' not in _cache:
        a = iu.ultralight_mem(31)
        b = iu.ultralight_mem(32)
        b[:9] = a[:9]
        reader = emulate.reader_card(emulate.drawn_rands(3))
        trs = emulate.pairs_host([emulate.tag_card(0, a), emulate.tag_card(0, b)], [reader, reader])
        _cache['ab'] = (a, b, [emulate.synth_frames(trs.transcript(k)) for k in (0, 1)])
    return _cache['ab']


def run_stream(frames, repeats=1):
    """frames rendered to one capture and pushed into a fresh context with images on, `repeats` times -> [(commands, fetched images)]"""
    caps = air.render_device([frames], sigma=0.0)
    out = []
    try:
        for _ in range(repeats):
            with context(1, int(caps.n_samples[0])) as m:
                m.track_images()
                caps.push_to(m)
                out.append((m.fetch_commands(), m.fetch_images()))
    finally:
        caps.free()
    return out


def edge_pad(T, fa, turns):
    """The number of REQA frames in front that puts a READR on the last command of a tile and its READT on the first of the next, from
    THREADS and the transaction alone: the transaction's READR places come from the CPU machine over its frames."""
    t, _, _ = fsm.host_commands(fsm.state_init(), emulate.frames_of_bits(fa))
    readr, readt = CommandType.READR.index, CommandType.READT.index
    places = [i for i in range(len(t) - 1) if int(t[i]['cmd']) == readr and int(t[i + 1]['cmd']) == readt]
    assert places
    return min((T - 1 - (turn * len(fa) + r)) % T for turn in range(turns) for r in places)


@pytest.mark.parametrize('edge', [False, True])
def test_last_wins_within_a_tile_and_across_its_edge(edge):
    T = threads()
    a, b, (fa, fb) = two_cards_one_uid()
    n = len(fa)
    assert len(fb) == n and fa[0][1] == fb[0][1]
    turns = (2 * T) // n + 2
    turns += turns % 2          # the last card read is B
    pad = edge_pad(T, fa, turns) if edge else 0
    assert 2 * n + pad <= T     # (A and B share tile 0 whole, pad included)
    frames = [fa[0]] * pad + [f for i in range(turns) for f in (fb if i % 2 else fa)]
    runs = run_stream(frames, repeats=20)
    cm, im = runs[0]
    t, d, _ = cm.commands_of(0)
    assert len(t) == len(frames) > 2 * T
    # where the reads of page 4 fall: both contents inside tile 0, and again on both sides of an edge
    readr, readt = CommandType.READR.index, CommandType.READT.index
    pairs = [i for i in range(1, len(t)) if int(t[i]['cmd']) == readt and int(t[i - 1]['cmd']) == readr]
    reads = [(i, d[int(t[i]['byte_off']):int(t[i]['byte_off']) + 16].tobytes()) for i in pairs if int(d[int(t[i - 1]['byte_off']) + 1]) == 4]
    assert len(reads) == turns
    assert {c for i, c in reads if i < T} == {a[16:32].tobytes(), b[16:32].tobytes()}
    assert any(i // T != j // T and ci != cj for (i, ci), (j, cj) in zip(reads, reads[1:]))
    if edge:   # ... and a READR is the last command of a tile, its READT the first of the next
        assert any(i % T == 0 for i in pairs)
    twin = twin_of(cm, 0)
    assert iu.images_equal(im, 0, twin)
    assert im.mem(0)[:64].tolist() == b.tolist() and int(im.flags[0]) == _lib.NFC_IMG_CHANGED and int(im.n_known[0]) == 64
    for cm_i, im_i in runs[1:]:   # deterministic: twenty fresh contexts, one result
        assert iu.images_equal(im_i, 0, twin)


# ---- pushes that cut chains ----
def test_pushes_cut_between_readr_and_readt_and_inside_an_authentication():
    mem = iu.classic_mem(41)
    table = keys.sector_table({(0x60, 4 * s): k for (_, s), k in iu.key_a_table(mem).items()})[0]
    trs = emulate.pairs_host([emulate.tag_card(1, mem, emulate.drawn_rands(2))], [iu.reader_for(mem)], pair_cap_frames=[40])
    caps = air.render_device(trs, sigma=0.0)
    try:
        n = int(caps.n_samples[0])

        def pushed(cuts):
            with context(1, n) as m:
                m.track_images()
                m.set_sector_keys(table)
                twin, counts, raw = emulate.CardImage(), [], None
                for lo, hi in zip([0] + cuts, cuts + [n]):
                    m.push_device(caps.buf, caps.first_sample + np.uint64(lo), np.array([hi - lo], np.uint32))
                    cm = m.fetch_commands()
                    twin_of(cm, 0, (FF, FF, table), twin)
                    counts.append(len(cm.commands_of(0)[0]))
                    raw = cm.raw.frames_of(0).table if not cuts else raw
                    full = cm.commands_of(0)[0].copy() if not cuts else None
                im = m.fetch_images()
                assert iu.images_equal(im, 0, twin)
                return im, counts, raw, full

        whole, counts, raw, t = pushed([])
        assert counts == [40] and int(whole.n_known[0]) > 100
        idx = raw['idx'].astype(np.int64)
        name = lambda i: CommandType.by_index(int(t[i]['cmd'])).name() if int(t[i]['cmd']) >= 0 else '?'
        readt = next(i for i in range(1, 40) if name(i) == 'READT' and name(i - 1) == 'READR')
        auth = next(i for i in range(40) if name(i) == 'AUTHA')
        assert [name(auth + j) for j in range(4)] == ['AUTHA', 'RANDTA', 'RANDRB', 'RANDTB']
        between = lambda i: int((idx[i - 1] + idx[i]) // 2)   # a sample behind command i - 1's close and before command i's
        for cuts, want in (([between(readt)], [readt, 40 - readt]),
                           ([between(auth + 1), between(auth + 2), between(auth + 3)], [auth + 1, 1, 1, 40 - auth - 3]),
                           ([between(auth + 2), between(readt)], [auth + 2, readt - auth - 2, 40 - readt])):
            im, counts, _, _ = pushed(cuts)
            assert counts == want, (cuts, counts)
            assert im.image(0) == whole.image(0), cuts
    finally:
        caps.free()


# ---- edges ----
def test_no_commands_exactly_one_tile_one_more_and_65_streams():
    T = threads()
    a, b, (fa, fb) = two_cards_one_uid()
    long = [f for i in range(2 * T // len(fa) + 2) for f in (fb if i % 2 else fa)]
    lists = [long[:T], long[:T], long[:T + 1]] + [fa if k % 2 else fb for k in range(62)]
    assert len(lists) == 65 == T + 1
    caps = air.render_device(lists, sigma=0.0)
    try:
        n = caps.n_samples.copy()
        n[0] = 0   # stream 0 hears nothing
        with context(65, int(n.max()), lib_path=_lib.hooks_path()) as m:
            guards = m.L.nfc_debug_multi_guards
            guards.argtypes = [api.C.c_void_p]
            m.track_images()
            m.push_device(caps.buf, caps.first_sample, n)
            cm, im = m.fetch_commands(), m.fetch_images()
            assert guards(m.h) == 0
            assert np.diff(cm.cmd_off).tolist()[:3] == [0, T, T + 1]
            for k in range(65):
                assert iu.images_equal(im, k, twin_of(cm, k)), k
            assert im.image(0) == emulate.CardImage()
            assert im.mem(63)[:64].tolist() == b.tolist() and im.mem(64)[:64].tolist() == a.tolist()   # (lists[3 + k]: fa for odd k)
            # a push in which nothing is stored launches nothing and leaves the images; a reset returns one stream's
            m.push_device(caps.buf, caps.first_sample, np.zeros(65, np.uint32))
            assert int(m.stats().n_launches) == 1
            m.reset(5)
            after = m.fetch_images()
            assert after.n_launches == 0 and after.image(5) == emulate.CardImage() and after.image(6) == im.image(6)
    finally:
        caps.free()


# ---- off by default ----
def test_off_by_default_and_commands_unchanged():
    a, b, (fa, fb) = two_cards_one_uid()
    caps = air.render_device([fa, fb], sigma=0.0)
    try:
        got = []
        for images in (False, True):
            with context(2, int(caps.n_samples.max())) as m:
                m.track_commands()
                if images:
                    m.track_images()
                else:
                    with pytest.raises(api.NfcError):
                        m.fetch_images()
                caps.push_to(m)
                got.append((int(m.stats().n_launches), digest(m.fetch_commands())))
        assert got[0][0] == 4 and got[1][0] == 5     # what a tracked push reported before; one launch more with images
        assert got[0][1] == got[1][1] and got[0][1][1] == 3
    finally:
        caps.free()


def test_arguments_are_checked_before_the_device():
    with context(2, 1024) as m:
        img = emulate.CardImage()
        with pytest.raises(api.NfcError):
            m.image(0)                      # never switched on
        m.track_images()
        assert m.image(1) == img
        with pytest.raises(api.NfcError):
            m.image(2)
        bad = img.copy()
        bad.rec['info']['flags'] = 16
        with pytest.raises(api.NfcError):
            m.set_image(0, bad)
        assert m.L.nfc_multi_get_image(m.h, 0, None) == -1 and m.L.nfc_multi_set_image(m.h, 0, None) == -1
        assert m.L.nfc_multi_track_images(None, 1) == -1 and m.L.nfc_multi_fetch_images(None, None) == -1
        t, d = iu.commands([('ATQA1K', []), ('READR', [9]), ('READT', list(range(16)))])
        given = emulate.host_card_image(t, d)
        m.set_image(1, given)
        assert m.image(1) == given and m.fetch_images().image(1) == given and m.image(0) == img


def test_decode_many_attaches_each_files_image():
    from usrp_nfc_amd.decoder import decode_many
    a, b, (fa, fb) = two_cards_one_uid()
    caps = air.render_device([fa, fb], sigma=0.0)
    try:
        iq = [caps.download(k).copy().view(np.complex64) for k in (0, 1)]
    finally:
        caps.free()
    backs = decode_many(iq, images=True)
    assert [bk.image.mem[:64].tolist() for bk in backs] == [a.tolist(), b.tolist()]
    assert [bk.image.n_known for bk in backs] == [64, 64] and [bk.image.flags for bk in backs] == [0, 0]
    assert not hasattr(backs[0], 'commands')


def test_decode_many_images_with_recovered_keys():
    """keys='recover': the untracked pass finds the keys, the context is reset, and the image is built in the tracked pass that holds the
    recovered table -- one first authentication and its sector's reads, under a key that is not the default"""
    from usrp_nfc_amd.decoder import decode_many
    assert decode_many([], images=True) == []
    mem = iu.classic_mem(51)
    trs = emulate.pairs_host([emulate.tag_card(1, mem, emulate.drawn_rands(4))], [iu.reader_for(mem)], pair_cap_frames=[18])
    caps = air.render_device(trs, sigma=0.0)
    try:
        iq = caps.download(0).copy().view(np.complex64)
    finally:
        caps.free()
    plain = decode_many([iq], images=True)[0]
    back = decode_many([iq], commands=True, images=True, keys='recover')[0]
    key = bytes(bytearray(mem[63 * 16:63 * 16 + 6].tolist()))
    assert {k: bytes(bytearray(v)) for k, v in back.recovered_keys.items()} == {(0x60, 60): key}
    img = back.image
    assert img.mem[63 * 16:63 * 16 + 6].tolist() == list(key) and (img.src[63 * 16:63 * 16 + 6] == _lib.NFC_IMG_SRC_KEY).all()
    sector = slice(60 * 16, 64 * 16)
    assert img.src[sector].all() and img.mem[sector].tolist() == mem[sector].tolist() and img.flags == 0
    assert plain.image.n_known == 5 and img.n_known == 5 + 64   # without the key: the anticollision answer alone
    twin = emulate.CardImage()
    for t, d, _ in back.commands:
        emulate.host_card_image(t, d, keys=(key, (0xFF,) * 6, {(0x60, 15): key}), image=twin)
    assert img == twin
