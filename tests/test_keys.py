"""Key recovery on the GPU: nfc_recover_keys_device (csrc/keys.hip.h: k_keys_count, k_keys_fill_odd, k_keys_probe_even; nfc_keys.hip)
against its CPU twin on the traces of tests/test_keys_host.py -- the exact list sizes pin the walk, key / status / candidates / nr the
join, the roll-back and the verification -- then batching, the capacity rules, and the route from IQ samples to recovered keys and
decrypted commands.  Every comparison is for equality."""
import numpy as np
import pytest

from tests.test_commands import classic_iq, context
from tests.test_commands_host import assert_commands_equal, host_machine, run_host
from tests.test_keys_host import FF, all_traces, assert_same_results, twin_results
from usrp_nfc_amd import decoder, fsm, keys

pytestmark = pytest.mark.gpu
_cache = {}


def gpu_results():
    """recover() over all_traces() with the defaults, once: (results, stats)."""
    if 'gpu' not in _cache:
        r, st = keys.recover(all_traces(), timing=True)
        r.setflags(write=False)
        _cache['gpu'] = (r, st)
    return _cache['gpu']


def test_gpu_equals_twin_field_for_field():
    (got, st), (want, st_twin) = gpu_results(), twin_results()
    assert_same_results(got, want)
    assert got.tobytes() == want.tobytes()
    # one batch of eight: a count launch, one group, its fill and probe; the scratch is what the twin accounts
    assert (st.n_batches, st.n_launches, st.n_grown, st.scratch_bytes) == (1, 3, 0, st_twin.scratch_bytes)
    assert st.ms_count > 0 and st.ms_fill > 0 and st.ms_probe > 0 and abs(st.ms_kernels - (st.ms_count + st.ms_fill + st.ms_probe)) < 1e-9


def test_batching_does_not_change_the_results():
    want = twin_results()[0]
    r, st = keys.recover(all_traces()[:0])
    assert len(r) == 0 and (st.n_batches, st.n_launches, st.scratch_bytes) == (0, 0, 0)   # n == 0 launches nothing
    r, st = keys.recover(all_traces()[:1])
    assert_same_results(r, want[:1])
    assert (st.n_batches, st.n_launches) == (1, 3) and st.ms_kernels == 0   # (no events unless asked)
    r2, st2 = keys.recover(all_traces()[3:8], max_batch=2)   # three batches, the last one short; the corrupted trace among them
    r5, st5 = keys.recover(all_traces()[3:8], max_batch=5)
    assert (st2.n_batches, st2.n_launches, st5.n_batches, st5.n_launches) == (3, 9, 1, 3)
    assert r2.tobytes() == r5.tobytes()
    assert_same_results(r2, want[3:8])


def test_growth_and_overflow():
    want = twin_results()[0]
    r, st = keys.recover(all_traces()[:2], initial_capacity=1 << 16)
    assert_same_results(r, want[:2])
    assert st.n_grown == 1 and st.scratch_bytes == 16 * sum(1 << int(2 * n - 1).bit_length() for n in want['n_odd'][:2].tolist())
    # the overflow is a status: nothing is searched, the counts are exact, the neighbour in the batch is untouched by it
    r, st = keys.recover(all_traces()[:1], max_capacity=1 << 16)
    assert int(r['status'][0]) == keys.NFC_KEY_OVERFLOW and int(r['n_candidates'][0]) == 0 and r['key'][0].tolist() == [0] * 6 and int(r['nr'][0]) == 0
    assert (int(r['n_odd'][0]), int(r['n_even'][0])) == (int(want['n_odd'][0]), int(want['n_even'][0]))
    assert (st.n_batches, st.n_launches, st.n_grown, st.scratch_bytes) == (1, 1, 0, 16 << 16)   # the count launch alone
    # one trace of a batch over the limit (2^21 slots hold the reference trace's table, not a table of 2^22), the others searched
    sizes = [1 << int(2 * n - 1).bit_length() for n in want['n_odd'].tolist()]
    big = [i for i, s in enumerate(sizes) if s > 1 << 21]
    r, st = keys.recover(all_traces(), max_capacity=1 << 21)
    for i in range(len(r)):
        if i in big:
            assert int(r['status'][i]) == keys.NFC_KEY_OVERFLOW and (int(r['n_odd'][i]), int(r['n_even'][i])) == (int(want['n_odd'][i]), int(want['n_even'][i]))
        else:
            assert_same_results(r[i:i + 1], want[i:i + 1])
    assert sizes[0] == 1 << 21 and st.scratch_bytes <= 16 << 21


def test_three_streams_from_iq_to_keys_to_commands():
    iq = classic_iq()
    streams = [iq, iq, iq]
    with context(3, len(iq) // 2) as m:
        m.push(streams)
        traces = m.fetch_frames().auths()
        assert traces['stream'].tolist() == [0, 1, 2] and traces['block'].tolist() == [0x3C] * 3 and traces['key_type'].tolist() == [0x60] * 3
        assert traces[0]['uid'] == all_traces()[0]['uid'] and traces[0]['nr_enc'] == all_traces()[0]['nr_enc'] and traces[0]['par'] == all_traces()[0]['par']
        found = m.recover_keys()
        assert found == [{(0x60, 0x3C): bytes(bytearray(FF))}] * 3
        # the recovered keys into the machines, then a tracked re-push: the sessions decrypt as they do on the host with the right key
        m.reset()
        m.track_commands()
        for k in range(3):
            m.set_keys(*keys.first_keys(found[k]), stream=k)
        m.push(streams)
        cm = m.fetch_commands()
        for k in range(3):
            raw = cm.raw.frames_of(k)
            got = cm.commands_of(k)
            flags = got[0]['flags']
            assert int(((flags & fsm.FRAME_AR_OK) != 0).sum()) == 2 and int(((flags & fsm.FRAME_AT_OK) != 0).sum()) == 2
            assert not (flags & (fsm.FRAME_AR_ERROR | fsm.FRAME_AT_ERROR)).any()
            assert_commands_equal(got, run_host(host_machine((FF, FF)), raw), raw.table['n_bytes'])


def test_decode_many_recovers_the_keys_itself(tmp_path):
    iq = classic_iq()
    paths = []
    for i in range(2):
        p = str(tmp_path / ('capture%d.fc32' % i))
        np.asarray(iq, np.float32).tofile(p)
        paths.append(p)
    want = decoder.decode_many(paths, commands=True, keys=(FF, FF), max_push_samples=20011)
    got = decoder.decode_many(paths, commands=True, keys='recover', max_push_samples=20011)   # two pushes per source: the frames are joined
    for g, w in zip(got, want):
        assert g.recovered_keys == {(0x60, 0x3C): bytes(bytearray(FF))}
        assert len(g.commands) == len(w.commands) == 2
        for a, b in zip(g.commands, w.commands):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert sum(int(((c[0]['flags'] & fsm.FRAME_AT_OK) != 0).sum()) for c in g.commands) == 2
    assert not hasattr(want[0], 'recovered_keys')
