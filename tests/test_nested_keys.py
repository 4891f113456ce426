"""Key recovery from nested authentications on the GPU: k_nested_candidates and the three search kernels over virtual traces
(csrc/keys.hip.h; nfc_recover_nested_keys_device, nfc_nested_candidates_device in nfc_keys.hip) against the CPU twin on the
traces of tests/test_nested_keys_host.py, then batching, the capacity rules and the route from IQ samples to every sector's key.  Every
comparison is for equality.

The twin costs half a second per candidate: it runs on two-candidate windows of the PAIR of golden nested traces 0 and 3, three times
in the file (twin_window), shared."""
import numpy as np
import pytest

from tests.test_commands import classic_iq, context
from tests.test_keys_host import FF, word
from tests.test_nested_keys_host import (all_nested, assert_same_nested, golden_candidates, golden_nested, golden_true_index, off_sequence_nested,
                                         printed)
from usrp_nfc_amd import decoder, fsm, keys

pytestmark = pytest.mark.gpu
PAIR = [0, 3]
_cache = {}
FFK = bytes(bytearray(FF))


def pair():
    return golden_nested()[PAIR]


def twin_window(first, **cfg):
    """The twin on the pair over the window [first, first + 2), once per configuration: (results, stats)."""
    key = (first, tuple(sorted(cfg.items())))
    if key not in _cache:
        r, st = keys.host_recover_nested(pair(), cand_first=first, cand_count=2, **cfg)
        r.setflags(write=False)
        _cache[key] = (r, st)
    return _cache[key]


def assert_same_stats(st, want):
    assert (st.n_batches, st.n_grown, st.scratch_bytes) == (want.n_batches, want.n_grown, want.scratch_bytes)


# ---- 1. the candidates kernel alone ------------------------------------------------------------------------------------------------
def test_candidates_kernel_equals_the_host():
    t = all_nested()
    assert len(t) == 19
    want_nt, want_n = keys.nested_candidates(t)
    got_nt, got_n = keys.nested_candidates(t, device=0)
    assert got_n.tolist() == want_n.tolist() and set(want_n.tolist()) <= {0, 64}
    assert got_nt.tolist() == want_nt.tolist()
    assert got_nt[:15].tolist() == golden_candidates()[0].tolist()
    nt, n = keys.nested_candidates(t[:0], device=0)
    assert nt.shape == (0, 64) and len(n) == 0


# ---- 2. a full search, in four batches and in one ------------------------------------------------------------------------------------
def test_full_search_of_a_golden_nested_trace():
    r16, st16 = keys.recover_nested(golden_nested()[:1], max_batch=16)
    r64, st64 = keys.recover_nested(golden_nested()[:1], max_batch=64, timing=True)
    assert r16.tobytes() == r64.tobytes()
    assert (st16.n_batches, st64.n_batches) == (4, 1)
    r = r64[0]
    assert int(r['status']) == keys.NFC_KEY_OK and r['key'].tolist() == FF
    assert (int(r['nt']), int(r['nr'])) == (printed(0, 'RANDTA')[0], word([0x01, 0x3A, 0x6B, 0xBA]))
    assert (int(r['n_verified']), int(r['n_nt']), int(r['n_searched'])) == (1, 64, 64)
    # the candidate launch is counted and timed: a count launch per batch, a fill and a probe per group, and one more
    assert st16.n_launches >= 1 + 3 * 4 and st64.n_launches >= 1 + 3 and st16.ms_kernels == 0
    assert st64.ms_kernels > st64.ms_count + st64.ms_fill + st64.ms_probe > 0


def test_a_nonce_off_the_sequence_gives_no_key_from_any_candidate():
    r, _ = keys.recover_nested(off_sequence_nested())
    r = r[0]
    assert int(r['status']) == keys.NFC_KEY_NONE and r['key'].tolist() == [0] * 6 and int(r['n_searched']) == int(r['n_nt']) and int(r['n_nt']) in (0, 64)


# ---- 3. device against twin on two-candidate windows -----------------------------------------------------------------------------------
def test_window_with_the_true_nonce_equals_the_twin():
    first = golden_true_index(0)
    assert first == 32 and golden_true_index(3) not in (32, 33)
    want, st_want = twin_window(first)
    got, st = keys.recover_nested(pair(), cand_first=first, cand_count=2)
    assert_same_nested(got, want)
    assert got.tobytes() == want.tobytes()
    assert_same_stats(st, st_want)
    assert got['status'].tolist() == [keys.NFC_KEY_OK, keys.NFC_KEY_NONE] and got['key'][0].tolist() == FF and got['n_searched'].tolist() == [2, 2]
    assert (st.n_batches, st.n_launches) == (1, 4)   # candidates, count, one group's fill and probe


def test_window_across_a_batch_boundary_equals_the_twin():
    # candidates 15 and 16 lie in different batches of a full search at max_batch 16; here max_batch 3 cuts the four virtual traces
    # (trace 0: 15, 16; trace 3: 15, 16) between the two candidates of the second trace
    assert golden_true_index(0) not in (15, 16) and golden_true_index(3) not in (15, 16)
    want, st_want = twin_window(15, max_batch=3)
    got, st = keys.recover_nested(pair(), cand_first=15, cand_count=2, max_batch=3)
    assert got.tobytes() == want.tobytes()
    assert_same_stats(st, st_want)
    assert st.n_batches == 2 and got['status'].tolist() == [keys.NFC_KEY_NONE] * 2 and got['n_searched'].tolist() == [2, 2]
    one, _ = keys.recover_nested(pair(), cand_first=15, cand_count=2)
    assert one.tobytes() == got.tobytes()


# ---- 4. capacity ---------------------------------------------------------------------------------------------------------------------
def test_overflow_of_one_candidate_and_growth():
    # window [32, 34): trace 0's odd lists are 323 637 and 855 195 long -- tables of 2^20 and 2^21 slots -- trace 3's 478 448 and 224 391,
    # 2^20 both.  max_capacity 2^20: trace 0's second candidate overflows, its first (the true nonce) is still searched and found
    whole, _ = twin_window(32)
    want, st_want = twin_window(32, max_capacity=1 << 20)
    got, st = keys.recover_nested(pair(), cand_first=32, cand_count=2, max_capacity=1 << 20)
    assert got.tobytes() == want.tobytes()
    assert_same_stats(st, st_want)
    assert int(got['status'][0]) == keys.NFC_KEY_OVERFLOW and got['key'][0].tolist() == FF and int(got['n_verified'][0]) == 1
    assert (int(got['n_odd'][0]), int(got['n_even'][0])) == (int(whole['n_odd'][0]), int(whole['n_even'][0]))
    assert got[1].tobytes() == whole[1].tobytes()   # the neighbour untouched
    # a small initial capacity grows and changes nothing
    grown, st = keys.recover_nested(pair(), cand_first=32, cand_count=2, initial_capacity=1 << 16)
    assert grown.tobytes() == whole.tobytes() and st.n_grown >= 1


# ---- 5. from IQ ----------------------------------------------------------------------------------------------------------------------
def test_three_streams_from_iq_to_every_sector_key():
    iq = classic_iq()
    with context(3, len(iq) // 2) as m:
        m.push([iq, iq, iq])
        fr = m.fetch_frames()
        assert len(fr.frames_of(0).table) == 24
        t = fr.nested_auths()
        assert t['stream'].tolist() == [0, 1, 2] and t['frame'].tolist() == [18] * 3
        for name in ('uid', 'nt_enc', 'nr_enc', 'ar_enc', 'at_enc', 'par'):
            assert t[name].tolist() == [int(golden_nested()[0][name])] * 3, name
        assert fr.auths()['stream'].tolist() == [0, 1, 2]
        assert m.recover_keys(nested=True) == [{(0x60, 0x3C): FFK, (0x60, 0x38): FFK}] * 3
        assert m.recover_keys() == [{(0x60, 0x3C): FFK}] * 3


# ---- 6. decode_many ------------------------------------------------------------------------------------------------------------------
def test_decode_many_recovers_nested_keys(tmp_path):
    iq = classic_iq()
    paths = []
    for i in range(2):
        p = str(tmp_path / ('capture%d.fc32' % i))
        np.asarray(iq, np.float32).tofile(p)
        paths.append(p)
    want = decoder.decode_many(paths, commands=True, keys=(FF, FF), max_push_samples=20011)
    got = decoder.decode_many(paths, commands=True, keys='recover', nested=True, max_push_samples=20011)
    plain = decoder.decode_many(paths, commands=True, keys='recover', max_push_samples=20011)
    for g, w, p in zip(got, want, plain):
        assert g.recovered_keys == {(0x60, 0x3C): FFK, (0x60, 0x38): FFK}
        assert p.recovered_keys == {(0x60, 0x3C): FFK}
        assert len(g.commands) == len(w.commands) == len(p.commands) == 2
        for a, b, c in zip(g.commands, w.commands, p.commands):
            assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(a, b, c))
        assert sum(int(((c[0]['flags'] & fsm.FRAME_AT_OK) != 0).sum()) for c in g.commands) == 2
    with pytest.raises(ValueError):
        decoder.decode_many(paths, commands=True, keys=(FF, FF), nested=True)
