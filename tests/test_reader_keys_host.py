"""Key recovery from TWO reader-side authentications, without {at}, on the CPU: nfc_find_reader_auths and nfc_host_recover_reader_keys
(csrc/keys.hip.h, nfc_keys.hip), and keys.pair_reader_auths.  No GPU.  tests/test_reader_keys.py holds the GPU half and uses
the pairs and the twin's results below.  Every comparison is for equality.

THE PAIRS, in this order (all_pairs): the reference's own first authentication (tests/golden/1k_with_enc.out) searched, with a crafted
check session of key FF; the six keys of test_keys_host.CRAFTED, each with a second session of another nt and nr (pair 2: another UID
too; pair 3: the SAME nt and another nr); then four that must fail -- pair 3 with one bit of the check session's ar_enc flipped, with
one bit of the searched session's ar_enc flipped, with one ninth bit of the searched {nr} flipped, and pair 3's searched session twice.
The twin runs over them ONCE (twin_results); the capacity and batching cases run eleven more recoveries of half a second each."""
import ctypes as C
import os

import numpy as np

from tests.test_keys_host import CRAFTED, FF, crafted_trace, reference_frames, word
from usrp_nfc_amd import _lib, api, emulate, keys, synth

_rng = np.random.RandomState(20252)   # the second sessions' nonces
SECOND = [(_rng.randint(0, 256, 4).tolist(), _rng.randint(0, 256, 4).tolist()) for _ in CRAFTED]   # (nt, nr)
OTHER_UID = [0x12, 0x34, 0x56, 0x78]
N_GOOD = 1 + len(CRAFTED)
BAD_CHECK_AR_BIT, BAD_SEARCH_AR_BIT, BAD_NR_NINTH = 13, 13, 2   # (run through the twin: NONE, NONE with n_joined > 0, NONE)
_cache = {}


def reader_side(t):
    """A trace as nfc_find_reader_auths leaves it: no {at}, no ninth bits of it."""
    t = t.copy()
    t['at_enc'], t['par'] = 0, int(t['par']) & 0xFF
    return t


def pair_of(search, check):
    p = np.zeros(1, _lib.READER_PAIR_DTYPE)[0]
    p['search'], p['check'] = search, check
    return p


def all_pairs():
    if 'pairs' not in _cache:
        ref = keys.find_reader_auths(reference_frames())[0]
        pairs = [pair_of(ref, reader_side(crafted_trace(FF, 0x60, [0xCD, 0x76, 0x92, 0x74], [0x01, 0x20, 0x01, 0x45], [0] * 4, block=0x3C)))]
        for i, ((key, key_type, uid, nt, nr), (nt2, nr2)) in enumerate(zip(CRAFTED, SECOND)):
            uid2 = OTHER_UID if i == 1 else uid
            nt2 = nt if i == 2 else nt2
            pairs.append(pair_of(reader_side(crafted_trace(key, key_type, uid, nt, nr)), reader_side(crafted_trace(key, key_type, uid2, nt2, nr2))))
        good = pairs[3]
        for field, side, bit in (('ar_enc', 'check', BAD_CHECK_AR_BIT), ('ar_enc', 'search', BAD_SEARCH_AR_BIT), ('par', 'search', BAD_NR_NINTH)):
            bad = good.copy()
            bad[side][field] ^= 1 << bit
            pairs.append(bad)
        pairs.append(pair_of(good['search'], good['search']))
        p = np.array(pairs, _lib.READER_PAIR_DTYPE)
        p.setflags(write=False)
        _cache['pairs'] = p
    return _cache['pairs']


def twin_results():
    """The twin over all_pairs(), once: (results, stats).  Shared, never changed."""
    if 'twin' not in _cache:
        r, st = keys.host_recover_reader(all_pairs())
        r.setflags(write=False)
        _cache['twin'] = (r, st)
    return _cache['twin']


FIELDS = ('key', 'status', 'n_candidates', 'n_joined', 'n_odd', 'n_even', 'nr_search', 'nr_check')


def assert_same_results(got, want):
    for name in FIELDS:
        assert got[name].tolist() == want[name].tolist(), name


# ---- the searches -------------------------------------------------------------------------------------------------------------------
def test_reference_authentication_as_the_searched_session():
    p = all_pairs()[0]
    assert (int(p['search']['uid']), int(p['search']['nt'])) == (word([0xCD, 0x76, 0x92, 0x74]), word([0x0E, 0x61, 0x64, 0xD6]))
    assert (int(p['search']['nr_enc']), int(p['search']['ar_enc'])) == (word([0x78, 0x5A, 0x41, 0x80]), word([0x50, 0x04, 0x8F, 0x22]))
    assert int(p['search']['at_enc']) == 0 and int(p['search']['par']) >> 8 == 0
    r = twin_results()[0][0]
    assert int(r['status']) == keys.NFC_KEY_OK and r['key'].tolist() == FF and int(r['n_candidates']) == 1
    assert int(r['nr_search']) == word([0x15, 0x45, 0x90, 0xA8]) and int(r['nr_check']) == 0
    # what the CPU prototype of the method counted on this pair
    assert (int(r['n_odd']), int(r['n_even']), int(r['n_joined'])) == (446989, 634554, 67325)


def test_crafted_pairs_are_recovered():
    r, p = twin_results()[0], all_pairs()
    for i, c in enumerate(CRAFTED):
        g = r[1 + i]
        assert int(g['status']) == keys.NFC_KEY_OK and int(g['n_candidates']) == 1 and g['key'].tolist() == c[0], i
        assert (int(g['nr_search']), int(g['nr_check'])) == (word(c[4]), word(SECOND[i][1])), i
        assert int(g['n_joined']) > 0 and int(g['n_odd']) > 0 and int(g['n_even']) > 0
    assert int(p[2]['search']['uid']) != int(p[2]['check']['uid'])                                             # different UIDs
    assert int(p[3]['search']['nt']) == int(p[3]['check']['nt']) and int(p[3]['search']['nr_enc']) != int(p[3]['check']['nr_enc'])   # the same nt
    assert int(p[6]['search']['uid']) == int(p[6]['search']['nt'])


def test_pairs_that_cannot_give_a_key():
    r = twin_results()[0]
    for i in (N_GOOD, N_GOOD + 1, N_GOOD + 2):   # a wrong bit in either session, a wrong ninth bit: no candidate passes both
        assert int(r['status'][i]) == keys.NFC_KEY_NONE and int(r['n_candidates'][i]) == 0, i
        assert r['key'][i].tolist() == [0] * 6 and (int(r['nr_search'][i]), int(r['nr_check'][i])) == (0, 0)
    # the flipped keystream bit changes the lists, yet pairs still join (22 relations against 2^19.5 sequences a half)
    assert int(r['n_joined'][N_GOOD + 1]) > 0
    # the check session's flip leaves the search as it was
    assert [int(r[n][N_GOOD]) for n in ('n_odd', 'n_even', 'n_joined')] == [int(r[n][3]) for n in ('n_odd', 'n_even', 'n_joined')]
    # an identical pair: every register that fits the one session fits the other
    g = r[N_GOOD + 3]
    assert int(g['status']) == keys.NFC_KEY_AMBIGUOUS and int(g['n_candidates']) > 1
    assert int(g['nr_search']) == int(g['nr_check'])


# ---- finding and pairing ------------------------------------------------------------------------------------------------------------
def frames_without(frames, drop=(), replace=None, upto=None):
    """The frame list with rows dropped, one row's type swapped for a reader frame of the same bytes, or cut after `upto` rows."""
    table = frames.table.copy()
    bytes_, par = [b.copy() for b in frames.bytes], [p.copy() for p in frames.par]
    if replace is not None:   # the tag frame becomes a reader frame: its bytes go to the end of the reader's buffers
        r = table[replace]
        o, n = int(r['byte_off']), int(r['n_bytes'])
        table[replace]['byte_off'] = len(bytes_[1])
        bytes_[1] = np.concatenate([bytes_[1], bytes_[0][o:o + n]])
        par[1] = np.concatenate([par[1], par[0][o:o + n]])
        table[replace]['type'] = 1
    rows = table[[i for i in range(len(table) if upto is None else upto) if i not in drop]]
    return api.NfcFrames([rows[rows['type'] == 0], rows[rows['type'] == 1]], bytes_, par)


def test_find_reader_auths_needs_no_at():
    frames = reference_frames()
    full, got = keys.find_auths(frames), keys.find_reader_auths(frames)
    assert len(full) == len(got) == 1
    for name in _lib.AUTH_DTYPE.names:
        if name not in ('at_enc', 'par'):
            assert int(got[0][name]) == int(full[0][name]), name
    assert int(got[0]['at_enc']) == 0 and int(got[0]['par']) == int(full[0]['par']) & 0xFF
    f = int(full[0]['frame'])
    for other in (frames_without(frames, drop=(f + 3,)), frames_without(frames, replace=f + 3), frames_without(frames, upto=f + 3)):
        again = keys.find_reader_auths(other)
        assert len(again) == 1 and again[0].tobytes() == got[0].tobytes()
        assert len(keys.find_auths(other)) == 0
    assert len(keys.find_reader_auths(frames_without(frames, drop=(f + 2,)))) == 0
    assert len(keys.find_reader_auths(frames_without(frames, upto=f + 2))) == 0


def test_pair_reader_auths_groups_and_skips_identical_sessions():
    p = all_pairs()
    a, b = p[3]['search'].copy(), p[3]['check'].copy()          # one key, sector 1 (block 4)
    same_sector = b.copy()
    same_sector['block'] = 7
    other_sector = b.copy()
    other_sector['block'] = 8
    other_stream = b.copy()
    other_stream['stream'] = 1
    other_type = b.copy()
    other_type['key_type'] = 0x61
    c, d = p[4]['search'].copy(), p[4]['check'].copy()          # another card
    traces = np.array([a, a, other_sector, c, same_sector, other_stream, b, other_type, d], _lib.AUTH_DTYPE)
    pairs, rest = keys.pair_reader_auths(traces)
    # a's group: a, a (identical: skipped), same_sector (the first that differs), b (a third: unpaired)
    assert len(pairs) == 2
    assert pairs[0]['search'].tobytes() == a.tobytes() and pairs[0]['check'].tobytes() == same_sector.tobytes()
    assert pairs[1]['search'].tobytes() == c.tobytes() and pairs[1]['check'].tobytes() == d.tobytes()
    assert [r.tobytes() for r in rest] == [x.tobytes() for x in (a, other_sector, other_stream, b, other_type)]
    pairs, rest = keys.pair_reader_auths(np.array([a, a], _lib.AUTH_DTYPE))
    assert len(pairs) == 0 and len(rest) == 2
    pairs, rest = keys.pair_reader_auths(traces[:0])
    assert len(pairs) == 0 and len(rest) == 0


def test_recover_reader_streams_searches_what_is_left_and_merges():
    p = all_pairs()
    traces = []
    for stream, pair in ((0, p[3]), (2, p[4])):
        for side in ('search', 'check'):
            t = pair[side].copy()
            t['stream'] = stream
            traces.append(t)
    traces = np.array(traces, _lib.AUTH_DTYPE)
    known = bytes(range(6))
    found = [{}, {}, {(int(p[4]['search']['key_type']), int(p[4]['search']['block'])): known}]   # stream 2's key is there already: not searched
    out = keys.recover_reader_streams(traces, found, host=True)
    assert out == [{(int(p[3]['search']['key_type']), int(p[3]['search']['block'])): bytes(bytearray(CRAFTED[2][0]))}, {}, found[2]]
    assert found[0] == {}
    found[2] = {}
    out = keys.recover_reader_streams(traces[2:], found, host=True)
    assert out[2] == {(int(p[4]['search']['key_type']), int(p[4]['search']['block'])): bytes(bytearray(CRAFTED[3][0]))} and out[0] == {}


# ---- the emulators' closed loop with mismatched keys: where such sessions come from --------------------------------------------------
LOOP_KEYS = [[0x11, 0x22, 0x33, 0x44, 0x55, 0x66], [0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], [0xD3, 0xF7, 0xD3, 0xF7, 0xD3, 0xF7]]   # K_r per pair; K_t is FF x 6
LOOP_BLOCK = 0x3C   # the reader walks a Classic 1K from the last sector down: its first AUTH


def loop_cards(run, mode):
    """Three blank cards (keys FF x 6) and three readers keyed LOOP_KEYS, with the nonces of run `run`."""
    tags = [emulate.tag_card(emulate.CLASSIC1K, emulate.generate_1k(), emulate.drawn_rands(100 + 10 * k + run), mode) for k in range(3)]
    readers = [emulate.reader_card(emulate.drawn_rands(200 + 10 * k + run), key, key, None, mode) for k, key in enumerate(LOOP_KEYS)]
    return tags, readers


def loop_sessions(pairs_call, mode=_lib.NFC_EMU_CARD, link=_lib.NFC_EMU_LINK_AIR):
    """The loop run twice with different nonces -> per pair its two transcripts."""
    runs = [pairs_call(*loop_cards(run, mode), link=link) for run in (0, 1)]
    return [[r.transcript(k) for r in runs] for k in range(3)]


def loop_reader_traces(sessions):
    parts = []
    for k, trs in enumerate(sessions):
        for tr in trs:
            a = keys.find_reader_auths(tr.nfc_frames())
            a['stream'] = k
            parts.append(a)
    return np.concatenate(parts)


def capture_frames(trs, at):
    """One stream's frame list (type, on-air bits) for synth.modulation_profile: the two sessions one after the other; at[run] says
    what follows {nr}{ar} of session `run`: None nothing (the loop's own: the tag stays silent), else four noise bytes as a tag frame."""
    frames = []
    for tr, noise in zip(trs, at):
        frames += emulate.synth_frames(tr)
        if noise is not None:
            frames.append((synth.TAG, synth.frame_bits(noise)))
    return frames


CAPTURE_AT = [(None, None), ([0x5A, 0xC3, 0x0F, 0x96], [0x01, 0x02, 0x03, 0x04]), (None, [0xDE, 0xAD, 0xBE, 0xEF])]   # per stream: absent, noise, one of each


def test_closed_loop_with_mismatched_keys_gives_reader_sessions_and_their_keys():
    sessions = loop_sessions(emulate.pairs_host)
    for trs in sessions:
        for tr in trs:
            # on the AIR link a reader whose {nr}{ar} the tag cannot verify gets NO answer: the transcript ends with its 8-byte frame
            assert len(tr) == 9 and int(tr.frames[8]['type']) == synth.READER and int(tr.frames[8]['n_bits']) == 72
            assert tr.air(8).tolist() != tr.plain(8).tolist()
            fr = tr.nfc_frames()
            assert len(keys.find_auths(fr)) == 0 and len(keys.find_reader_auths(fr)) == 1
    traces = loop_reader_traces(sessions)
    assert traces['stream'].tolist() == [0, 0, 1, 1, 2, 2] and traces['block'].tolist() == [LOOP_BLOCK] * 6 and traces['key_type'].tolist() == [0x60] * 6
    pairs, rest = keys.pair_reader_auths(traces)
    assert len(pairs) == 3 and len(rest) == 0
    r, _ = keys.host_recover_reader(pairs)
    assert r['status'].tolist() == [keys.NFC_KEY_OK] * 3 and r['key'].tolist() == LOOP_KEYS and r['n_candidates'].tolist() == [1] * 3
    # the REFERENCE mode's loop puts the same frames on the air here; the PLAIN link carries no CRYPTO1 (plain bytes, whatever the keys)
    ref = loop_sessions(emulate.pairs_host, mode=_lib.NFC_EMU_REFERENCE)
    assert loop_reader_traces(ref).tobytes() == traces.tobytes()
    plain = loop_sessions(emulate.pairs_host, link=_lib.NFC_EMU_LINK_PLAIN)[0][0]
    f = int(keys.find_reader_auths(plain.nfc_frames())[0]['frame'])
    assert plain.air(f + 2).tolist() == plain.plain(f + 2).tolist()


def test_reader_pairs_switch_is_checked():
    from usrp_nfc_amd import decoder
    import pytest
    for kw in (dict(reader_pairs=True), dict(reader_pairs=True, commands=True), dict(nested=True)):
        with pytest.raises(ValueError):
            decoder.decode_many([], **kw)
    assert keys.reader_options(True, dict(max_batch=2)) == dict(max_batch=2)
    assert keys.reader_options(dict(stage_capacity=256), dict(max_batch=2)) == dict(max_batch=2, stage_capacity=256)
    with pytest.raises(TypeError):
        keys.reader_options(dict(cand_first=1), {})


# ---- capacity and batching ----------------------------------------------------------------------------------------------------------
def test_capacity_overflow_is_a_status_with_exact_counts():
    want = twin_results()[0][:1]
    r, st = keys.host_recover_reader(all_pairs()[:1], max_capacity=1 << 16)
    assert int(r['status'][0]) == keys.NFC_KEY_OVERFLOW and int(r['n_candidates'][0]) == 0 and r['key'][0].tolist() == [0] * 6
    assert (int(r['n_odd'][0]), int(r['n_even'][0]), int(r['n_joined'][0])) == (int(want['n_odd'][0]), int(want['n_even'][0]), 0)
    assert st.n_grown == 0 and st.n_batches == 1 and st.scratch_bytes == 16 << 16


def test_small_initial_capacity_grows_and_changes_nothing():
    want, st0 = twin_results()
    r, st = keys.host_recover_reader(all_pairs()[:1], initial_capacity=1 << 16)
    assert_same_results(r, want[:1])
    assert st.n_grown == 1 and st.scratch_bytes == 16 << 20   # 446 989 odd sequences: a table of 2^20 slots
    assert st0.n_grown == 0 and st0.n_batches == 1 and st0.scratch_bytes == 16 << 26


def test_batching_changes_nothing():
    want = twin_results()[0][2:7]
    for max_batch, n_batches in ((1, 5), (2, 3), (5, 1)):
        r, st = keys.host_recover_reader(all_pairs()[2:7], max_batch=max_batch)
        assert_same_results(r, want)
        assert st.n_batches == n_batches


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_and_bound():
    names = ['nfc_find_reader_auths', 'nfc_host_recover_reader_keys', 'nfc_recover_reader_keys_device']
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(getattr(L, n).argtypes for n in names)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'nfc_amd.h')).read()
    assert all(n + '(' in header for n in names) and '#define NFC_AMD_ABI_VERSION 4' in header and _lib.ABI_VERSION == 4
    assert all(n in header for n in ('nfc_reader_pair', 'nfc_reader_key_result', 'nfc_reader_key_config', 'NFC_RKEY_VERIFY_INLINE'))
    # the sizes the library asserts for its own structs (static_assert in csrc/nfc_keys.hip)
    assert _lib.READER_PAIR_DTYPE.itemsize == 80 and _lib.READER_KEY_RESULT_DTYPE.itemsize == 32 and C.sizeof(_lib.ReaderKeyConfig) == 48
    assert _lib.NFC_RKEY_VERIFY_INLINE == 1


def test_arguments_are_checked():
    L = _lib.load()
    p = all_pairs()[:1].copy()
    out = np.zeros(1, _lib.READER_KEY_RESULT_DTYPE)
    for side in ('search', 'check'):
        bad = p.copy()
        bad[side]['key_type'] = 0x30
        assert L.nfc_host_recover_reader_keys(bad.ctypes.data, 1, None, out.ctypes.data, None) == -1
    K = _lib.KeyConfig
    for cfg in (_lib.ReaderKeyConfig(K(1 << 20, 1 << 16, 0, 0), 0, 0), _lib.ReaderKeyConfig(K(0, 0, 5000, 0), 0, 0), _lib.ReaderKeyConfig(K(0, 0, 0, 2), 0, 0),
                _lib.ReaderKeyConfig(K(), (1 << 24) + 1, 0), _lib.ReaderKeyConfig(K(), 0, 2), _lib.ReaderKeyConfig(K(), 0, 0, (C.c_uint32 * 2)(0, 1))):
        assert L.nfc_host_recover_reader_keys(p.ctypes.data, 1, C.byref(cfg), out.ctypes.data, None) == -1
        assert L.nfc_recover_reader_keys_device(0, p.ctypes.data, 1, C.byref(cfg), out.ctypes.data, None) == -1   # (before the device is touched)
    assert L.nfc_host_recover_reader_keys(None, 1, None, out.ctypes.data, None) == -1
    assert L.nfc_recover_reader_keys_device(-1, p.ctypes.data, 1, None, out.ctypes.data, None) == -1
    r, st = keys.host_recover_reader(p[:0])
    assert len(r) == 0 and st.n_batches == 0 and st.scratch_bytes == 0
