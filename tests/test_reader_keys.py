"""Key recovery from two reader-side authentications on the GPU: nfc_recover_reader_keys_device (csrc/keys.hip.h: k_keys_count and
k_keys_fill_odd at the pair depth, k_keys_probe_even staged or in-lane, k_keys_verify_stage; nfc_keys.hip) against its CPU twin on the pairs
of tests/test_reader_keys_host.py -- the exact list sizes pin the walk, n_joined the join, key / status / candidates / both nr the
roll-back and the two verifications -- then batching, the capacity rules and the stage's full path; then where such sessions come from:
the emulators' closed loop with mismatched keys, three streams of rendered captures of it through NfcMultiContext.recover_keys, and
decode_many on such files.  Every comparison is for equality.
The search has one size, two halves of 2^20 windows per pair, so small means few pairs: at most eight per test."""
import numpy as np
import pytest

from tests.test_commands import context
from tests.test_commands_host import assert_commands_equal, host_machine, run_host
from tests.test_reader_keys_host import (CAPTURE_AT, LOOP_BLOCK, LOOP_KEYS, all_pairs, assert_same_results, capture_frames, loop_reader_traces,
                                         loop_sessions, twin_results)
from usrp_nfc_amd import _lib, decoder, emulate, fsm, keys, synth

pytestmark = pytest.mark.gpu
_cache = {}


def loop_captures():
    """Three rendered captures (synth), one per reader key of LOOP_KEYS: two sessions of the emulators' closed loop (the GPU's) each, the
    tag's {at} absent (stream 0), noise (stream 1), one of each (stream 2).  Made once, never changed."""
    if 'iq' not in _cache:
        sessions = loop_sessions(emulate.pairs_device)
        _cache['iq'] = [synth.iq_from_profile(synth.modulation_profile(capture_frames(trs, at)), seed=31 + k)
                        for k, (trs, at) in enumerate(zip(sessions, CAPTURE_AT))]
        for iq in _cache['iq']:
            iq.setflags(write=False)
    return _cache['iq']


WANT_KEYS = [{(0x60, LOOP_BLOCK): bytes(bytearray(k))} for k in LOOP_KEYS]


def test_gpu_equals_twin_field_for_field_on_the_good_pairs():
    want, st_twin = twin_results()
    got, st = keys.recover_reader(all_pairs()[:7], timing=True)
    assert_same_results(got, want[:7])
    assert got.tobytes() == want[:7].tobytes()
    # one batch of seven: a count launch, one group, its fill, its probe and its verify launch; the scratch is what the twin accounts
    assert (st.n_batches, st.n_launches, st.n_grown, st.scratch_bytes) == (1, 4, 0, st_twin.scratch_bytes)
    assert st.ms_count > 0 and st.ms_fill > 0 and st.ms_probe > 0 and abs(st.ms_kernels - (st.ms_count + st.ms_fill + st.ms_probe)) < 1e-9


def test_gpu_equals_twin_on_the_pairs_that_give_no_key():
    want = twin_results()[0]
    got, st = keys.recover_reader(all_pairs()[7:])
    assert_same_results(got, want[7:])
    assert got['status'].tolist() == [keys.NFC_KEY_NONE] * 3 + [keys.NFC_KEY_AMBIGUOUS]
    assert st.ms_kernels == 0   # (no events unless asked)


def test_batching_does_not_change_the_results():
    want = twin_results()[0]
    r, st = keys.recover_reader(all_pairs()[:0])
    assert len(r) == 0 and (st.n_batches, st.n_launches, st.scratch_bytes) == (0, 0, 0)   # n == 0 launches nothing
    r1, st1 = keys.recover_reader(all_pairs()[2:7], max_batch=1)
    r3, st3 = keys.recover_reader(all_pairs()[2:7], max_batch=3)   # two batches, the last one short
    assert (st1.n_batches, st1.n_launches, st3.n_batches, st3.n_launches) == (5, 20, 2, 8)
    assert r1.tobytes() == r3.tobytes()
    assert_same_results(r1, want[2:7])


def test_groups_growth_and_overflow():
    want = twin_results()[0]
    sizes = [1 << int(2 * n - 1).bit_length() for n in want['n_odd'].tolist()]
    # a max_capacity that holds the largest table of the five but not all of them: more than one group inside the one batch
    cap = max(sizes[2:7])
    assert sum(sizes[2:7]) > cap
    r, st = keys.recover_reader(all_pairs()[2:7], max_capacity=cap)
    assert_same_results(r, want[2:7])
    assert st.n_batches == 1 and st.n_launches > 4 and st.scratch_bytes <= 16 * cap
    r, st = keys.recover_reader(all_pairs()[:2], initial_capacity=1 << 16)
    assert_same_results(r, want[:2])
    assert st.n_grown == 1 and st.scratch_bytes == 16 * sum(sizes[:2])
    # the overflow is a status: nothing is searched, the counts are exact -- the twin's result
    tw, tw_st = keys.host_recover_reader(all_pairs()[:1], max_capacity=1 << 16)
    r, st = keys.recover_reader(all_pairs()[:1], max_capacity=1 << 16)
    assert r.tobytes() == tw.tobytes() and int(r['status'][0]) == keys.NFC_KEY_OVERFLOW
    assert (st.n_batches, st.n_launches, st.n_grown, st.scratch_bytes) == (1, 1, 0, tw_st.scratch_bytes)   # the count launch alone


def test_a_full_stage_and_the_in_lane_form_change_nothing():
    want = twin_results()[0]
    pairs = all_pairs()[[0, 3, 8, 10]]   # the reference pair, a crafted one, a flipped bit, the identical pair (hundreds verify)
    expect = want[[0, 3, 8, 10]]
    assert int(expect['n_joined'].min()) > 100 * 256
    small, st_small = keys.recover_reader(pairs, stage_capacity=256)   # the stage fills hundreds of times over: the rest verify in the lane
    inline, st_inline = keys.recover_reader(pairs, verify_inline=True)
    one, _ = keys.recover_reader(pairs, stage_capacity=1)
    for got in (small, inline, one):
        assert_same_results(got, expect)
    assert (st_small.n_launches, st_inline.n_launches) == (4, 3)   # no verify launch in the in-lane form


# ---- where such sessions come from: the emulators' closed loop, and captures of it ---------------------------------------------------
@pytest.mark.parametrize('mode', [_lib.NFC_EMU_CARD, _lib.NFC_EMU_REFERENCE])
def test_closed_loop_with_mismatched_keys_gives_every_reader_key(mode):
    # tags keyed FF x 6, readers keyed LOOP_KEYS, the AIR link, run twice with different nonces: a run holds ONE usable session per pair
    # (the tag does not answer a {nr}{ar} it cannot verify, and the reader's next round gets no card), so two runs make the pair
    sessions = loop_sessions(emulate.pairs_device, mode=mode)
    assert loop_reader_traces(sessions).tobytes() == loop_reader_traces(loop_sessions(emulate.pairs_host, mode=mode)).tobytes()
    pairs, rest = keys.pair_reader_auths(loop_reader_traces(sessions))
    assert len(pairs) == 3 and len(rest) == 0
    r, _ = keys.recover_reader(pairs)
    assert r['status'].tolist() == [keys.NFC_KEY_OK] * 3 and r['key'].tolist() == LOOP_KEYS and r['n_candidates'].tolist() == [1] * 3


def test_three_streams_from_iq_to_reader_keys_to_commands():
    streams = loop_captures()
    with context(3, max(len(s) for s in streams) // 2) as m:
        m.push(streams)
        fr = m.fetch_frames()
        # a noise {at} has the shape of one: find_auths takes those sessions, and the full search finds no key for them
        assert fr.auths()['stream'].tolist() == [1, 1, 2]
        ra = fr.reader_auths()
        assert ra['stream'].tolist() == [0, 0, 1, 1, 2, 2] and ra['block'].tolist() == [LOOP_BLOCK] * 6 and not ra['at_enc'].any()
        assert m.recover_keys() == [{}, {}, {}]
        found = m.recover_keys(reader_pairs=True)
        assert found == WANT_KEYS
        assert m.recover_keys(reader_pairs=dict(stage_capacity=256), max_batch=2) == WANT_KEYS
        assert m.recover_keys(nested=True, reader_pairs=True) == WANT_KEYS
        assert m.recover_keys(nested=True) == [{}, {}, {}]
        # the recovered keys into the machines as sector keys, then a tracked re-push of the same samples: the reader's side of both
        # sessions is genuine, and under its key {nr}{ar} decrypts to a right ar -- as on the host with that table, and not without it
        m.reset()
        m.track_commands()
        tables = [keys.sector_table(found[k])[0] for k in range(3)]
        for k in range(3):
            m.set_sector_keys(tables[k], stream=k)
        m.push(streams)
        cm = m.fetch_commands()
        for k in range(3):
            raw, got = cm.raw.frames_of(k), cm.commands_of(k)
            flags = got[0]['flags']
            # frame 8 is the first session's {nr}{ar}.  The machine, like the reference's, leaves the encrypted state only through a
            # frame it understands, and no {at} ever comes: what follows the first session is taken for ciphertext, the second AUTH
            # included, so ONE session decrypts per capture (the host comparison below pins the rest)
            assert flags[8] & fsm.FRAME_AR_OK and int(((flags & fsm.FRAME_AR_OK) != 0).sum()) == 1 and not (flags & fsm.FRAME_AR_ERROR).any()
            hm = host_machine()
            hm.set_sector_keys(tables[k])
            assert_commands_equal(got, run_host(hm, raw), raw.table['n_bytes'])
            assert not (run_host(host_machine(), raw)[0]['flags'] & fsm.FRAME_AR_OK).any()


def test_decode_many_recovers_reader_keys_itself(tmp_path):
    paths = []
    for i, iq in enumerate(loop_captures()[:2]):   # {at} absent, {at} noise
        p = str(tmp_path / ('reader%d.fc32' % i))
        np.asarray(iq, np.float32).tofile(p)
        paths.append(p)
    plain = decoder.decode_many(paths, commands=True, keys='recover', max_push_samples=20011)
    got = decoder.decode_many(paths, commands=True, keys='recover', reader_pairs=True, max_push_samples=20011)   # several pushes per source: the frames are joined
    for i, (g, w) in enumerate(zip(got, plain)):
        assert w.recovered_keys == {} and g.recovered_keys == WANT_KEYS[i] and g.key_conflicts == {}
        ok = lambda b: sum(int(((c[0]['flags'] & fsm.FRAME_AR_OK) != 0).sum()) for c in b.commands)
        assert (ok(g), ok(w)) == (1, 0)   # the first session's {nr}{ar}; the machine stays in that session (no {at} ends it)
