"""Key recovery on the CPU: nfc_find_auths and nfc_host_recover_keys (csrc/keys.hip.h, nfc_keys.hip) on the reference's own
printed trace and on traces crafted with the project's machine.  No GPU.  tests/test_keys.py holds the GPU half and uses the traces and
the twin's results below.  Every comparison is for equality.

THE TRACES, in this order (all_traces): the one first authentication of tests/golden/1k_with_enc.out; six crafted ones -- key 0, key
all-ones, A0 .. A5, two fixed-seed random keys, and a random key with uid == nt; and the A0 .. A5 trace with one bit of ar_enc flipped.
The twin runs over them ONCE (twin_results); the capacity cases run two more recoveries: ten in the file."""
import ctypes as C
import io
import os

import numpy as np

from tests.test_frames import GOLD_1K, host_frames_of, packets_from_trace
from usrp_nfc_amd import _lib, fsm, keys, synth
from usrp_nfc_amd.command import CommandType

ATQA1K, SEL1R, AUTHA, AUTHB, RANDTA, RANDRB, RANDTB = 3, 9, 14, 15, 16, 17, 18   # indices of the command table
FF = [0xFF] * 6
_rng = np.random.RandomState(20251)   # the two random keys, their uids and nonces
CRAFTED = [   # (key, key_type, uid, nt, nr)
    ([0] * 6, 0x60, [0x01, 0x02, 0x03, 0x04], [0x11, 0x22, 0x33, 0x44], [0xDE, 0xAD, 0xBE, 0xEF]),
    (FF, 0x61, [0xCD, 0x76, 0x92, 0x74], [0x01, 0x20, 0x01, 0x45], [0x00, 0x00, 0x00, 0x00]),
    ([0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5], 0x60, [0x9C, 0x59, 0x9B, 0x32], [0x82, 0xA4, 0x16, 0x6C], [0xA1, 0xE4, 0x58, 0xCE]),
] + [(_rng.randint(0, 256, 6).tolist(), 0x60 + i, _rng.randint(0, 256, 4).tolist(), _rng.randint(0, 256, 4).tolist(), _rng.randint(0, 256, 4).tolist())
     for i in range(2)]
_k = _rng.randint(0, 256, 6).tolist()
_u = _rng.randint(0, 256, 4).tolist()
CRAFTED.append((_k, 0x60, _u, _u, _rng.randint(0, 256, 4).tolist()))   # uid == nt: nothing but the key goes into the register
CORRUPTED_FROM, CORRUPTED_BIT = 3, 13   # all_traces()[3] is the A0 .. A5 trace; bit 13 of its ar_enc
_cache = {}


def word(b):
    return int(b[0]) | int(b[1]) << 8 | int(b[2]) << 16 | int(b[3]) << 24


def crafted_trace(key, key_type, uid, nt, nr, block=0x04):
    """One first authentication made by the project's own machine and CRYPTO1 (fsm.process_bits / process_outgoing; csrc/protocol.h over csrc/fsm.hip.h):
    the tag type and the UID go in as heard frames, the AUTH too (it selects the key), then the machine ENCRYPTS what a tag and a reader
    would send -- nt, nr | suc64(nt), suc96(nt); the two answers are the machine's own (its state after nt)."""
    m = fsm.fsm(out=io.StringIO())
    m.set_keys(key, key)
    crc = lambda d: d + fsm.crc_a(d)
    m.process_bits(synth.frame_bits([0x04, 0x00]), 0)
    m.process_bits(synth.frame_bits(crc([0x93, 0x70] + uid + [uid[0] ^ uid[1] ^ uid[2] ^ uid[3]])), 1)
    m.process_bits(synth.frame_bits(crc([key_type, block])), 1)
    assert m.process_outgoing(synth.frame_bits(nt), CommandType.by_index(RANDTA)) == synth.frame_bits(nt)   # in the clear
    st = m.get_state()
    assert st.encrypted == 1 and st.cur_key == (key_type & 1)
    ar, at = list(st.ar), list(st.at)
    nr_ar = m.process_outgoing(synth.frame_bits(nr + ar), CommandType.by_index(RANDRB))
    at_enc = m.process_outgoing(synth.frame_bits(at), CommandType.by_index(RANDTB))

    def split(bits):
        a = np.array(bits, np.uint8).reshape(-1, 9)
        return (a[:, :8].astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=1).tolist(), a[:, 8].tolist()

    (rb, rp), (tb, tp) = split(nr_ar), split(at_enc)
    t = np.zeros(1, _lib.AUTH_DTYPE)[0]
    t['uid'], t['nt'], t['nr_enc'], t['ar_enc'], t['at_enc'] = word(uid), word(nt), word(rb), word(rb[4:]), word(tb)
    t['par'] = sum(p << i for i, p in enumerate(rp + tp))
    t['key_type'], t['block'] = key_type, block
    return t


def reference_frames():
    if 'frames' not in _cache:
        _cache['frames'] = host_frames_of(packets_from_trace(GOLD_1K)[0])[0]
    return _cache['frames']


def all_traces():
    if 'traces' not in _cache:
        ref = keys.find_auths(reference_frames())
        crafted = [crafted_trace(*c) for c in CRAFTED]
        bad = crafted[CORRUPTED_FROM - 1].copy()
        bad['ar_enc'] ^= 1 << CORRUPTED_BIT
        t = np.concatenate([ref[:1], np.array(crafted + [bad], _lib.AUTH_DTYPE)])
        t.setflags(write=False)
        _cache['traces'] = t
    return _cache['traces']


def expected_keys():
    return [FF] + [c[0] for c in CRAFTED]


def twin_results():
    """The twin over all_traces(), once: (results, stats).  Shared, never changed."""
    if 'twin' not in _cache:
        r, st = keys.host_recover(all_traces())
        r.setflags(write=False)
        _cache['twin'] = (r, st)
    return _cache['twin']


def assert_same_results(got, want):
    for name in ('key', 'status', 'n_candidates', 'n_odd', 'n_even', 'nr'):
        assert got[name].tolist() == want[name].tolist(), name


# ---- the reference's own trace ------------------------------------------------------------------------------------------------------
def test_reference_trace_first_authentication():
    a = keys.find_auths(reference_frames())
    t = a[0]
    assert (int(t['uid']), int(t['nt'])) == (word([0xCD, 0x76, 0x92, 0x74]), word([0x0E, 0x61, 0x64, 0xD6]))
    assert (int(t['nr_enc']), int(t['ar_enc']), int(t['at_enc'])) == (word([0x78, 0x5A, 0x41, 0x80]), word([0x50, 0x04, 0x8F, 0x22]), word([0xCE, 0xCA, 0x0D, 0x83]))
    # the ninth bits: '!' in the trace where the parity bit EQUALS the data parity -- 0x78 0x5A 0x41 0x80! 0x50! 0x04! 0x8F 0x22! / 0xCE! 0xCA! 0x0D! 0x83
    bang = [0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0]
    data = [0x78, 0x5A, 0x41, 0x80, 0x50, 0x04, 0x8F, 0x22, 0xCE, 0xCA, 0x0D, 0x83]
    assert int(t['par']) == sum((bin(d).count('1') & 1 if b else 1 - (bin(d).count('1') & 1)) << i for i, (d, b) in enumerate(zip(data, bang)))
    assert (int(t['key_type']), int(t['block']), int(t['stream'])) == (0x60, 0x3C, 0)
    r = twin_results()[0][0]
    assert int(r['status']) == keys.NFC_KEY_OK and r['key'].tolist() == FF and int(r['n_candidates']) == 1
    assert (int(r['n_odd']), int(r['n_even'])) == (661002, 599119)   # (what an independent prototype of the method counted on this trace)
    assert int(r['nr']) == word([0x15, 0x45, 0x90, 0xA8])            # (the trace's RANDRB: EXTRA 0x15 0x45 0x90 0xA8 ..)


def test_reference_trace_every_first_authentication_and_no_nested_one():
    frames = reference_frames()
    table, _ = fsm.fsm(out=io.StringIO()).process_frames(frames, dispatch=False)
    auth = np.nonzero((table['cmd'] == AUTHA) | (table['cmd'] == AUTHB))[0]
    first = [int(i) for i in auth if not table['flags'][i] & fsm.FRAME_ENCRYPTED]
    nested = [int(i) for i in auth if table['flags'][i] & fsm.FRAME_ENCRYPTED]
    # from the trace itself: an AUTH printed without a ciphertext line before it is a first authentication
    lines = packets_from_trace(GOLD_1K)[1].split('\n')
    plain = [i for i, l in enumerate(lines) if l.startswith('COMMAND: AUTH') and not lines[i - 1].startswith('0x')]
    a = keys.find_auths(frames)
    assert len(plain) == len(first) == len(a) == 1 and len(nested) == 15
    assert a['frame'].tolist() == first
    assert nested[0] == 18 and 18 not in a['frame'].tolist()   # the encrypted AUTHA that follows the first session's reads
    assert frames.table['idx'][a['frame']].tolist() == a['idx'].tolist()
    r = twin_results()[0][:len(a)]
    assert (r['status'] == keys.NFC_KEY_OK).all() and all(k.tolist() == FF for k in r['key'])


# ---- crafted traces -----------------------------------------------------------------------------------------------------------------
def test_crafted_traces_are_recovered():
    r = twin_results()[0]
    want = expected_keys()
    assert len(want) == 7
    for i, key in enumerate(want):
        assert int(r['status'][i]) == keys.NFC_KEY_OK and int(r['n_candidates'][i]) == 1, i
        assert r['key'][i].tolist() == key, i
    assert [int(r['nr'][1 + i]) for i in range(len(CRAFTED))] == [word(c[4]) for c in CRAFTED]
    assert int(all_traces()[6]['uid']) == int(all_traces()[6]['nt'])
    assert int((r['n_odd'] > 0).sum()) == len(r) and int((r['n_even'] > 0).sum()) == len(r)


def test_corrupted_trace_gives_none():
    # One flipped bit of ar_enc flips one keystream bit: 64 bits over-determine the 48-bit register, so in general no register gives them.
    # A chance solution needs a pair with equal 54-bit signatures (n_odd n_even / 2^54, about 2^-16) whose key also decrypts {nr} to four
    # right parity bits (2^-4): about 2^-20.  Bit 13 of this trace was checked: the twin finds none.
    r = twin_results()[0][-1]
    assert int(r['status']) == keys.NFC_KEY_NONE and int(r['n_candidates']) == 0 and r['key'].tolist() == [0] * 6 and int(r['nr']) == 0
    assert int(r['n_odd']) > 0 and int(r['n_even']) > 0


# ---- capacity -----------------------------------------------------------------------------------------------------------------------
def test_capacity_overflow_is_a_status_with_exact_counts():
    want = twin_results()[0][:1]
    r, st = keys.host_recover(all_traces()[:1], max_capacity=1 << 16)
    assert int(r['status'][0]) == keys.NFC_KEY_OVERFLOW and int(r['n_candidates'][0]) == 0 and r['key'][0].tolist() == [0] * 6
    assert (int(r['n_odd'][0]), int(r['n_even'][0])) == (int(want['n_odd'][0]), int(want['n_even'][0]))
    assert st.n_grown == 0 and st.n_batches == 1 and st.scratch_bytes == 16 << 16


def test_small_initial_capacity_grows_and_changes_nothing():
    want, st0 = twin_results()
    r, st = keys.host_recover(all_traces()[:1], initial_capacity=1 << 16)
    assert_same_results(r, want[:1])
    assert st.n_grown == 1 and st.scratch_bytes == 16 << 21   # 661 002 odd sequences: a table of 2^21 slots
    assert st0.n_grown == 0 and st0.n_batches == 1 and st0.scratch_bytes == 16 << 26


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_and_bound():
    names = ['nfc_find_auths', 'nfc_host_recover_keys', 'nfc_recover_keys_device']
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(getattr(L, n).argtypes for n in names)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'nfc_amd.h')).read()
    assert all(n + '(' in header for n in names) and '#define NFC_AMD_ABI_VERSION 4' in header and _lib.ABI_VERSION == 4
    assert all(n in header for n in ('nfc_auth_trace', 'nfc_key_result', 'nfc_key_config', 'nfc_key_stats', 'NFC_KEY_OK', 'NFC_KEY_NONE',
                                     'NFC_KEY_AMBIGUOUS', 'NFC_KEY_OVERFLOW', 'NFC_KEY_TIMING'))
    # the sizes the library asserts for its own structs (static_assert in csrc/nfc_keys.hip)
    assert _lib.AUTH_DTYPE.itemsize == 40 and _lib.KEY_RESULT_DTYPE.itemsize == 24
    assert C.sizeof(_lib.KeyConfig) == 32 and C.sizeof(_lib.KeyStats) == 56
    assert (_lib.NFC_KEY_OK, _lib.NFC_KEY_NONE, _lib.NFC_KEY_AMBIGUOUS, _lib.NFC_KEY_OVERFLOW) == (0, 1, 2, 3)


def test_arguments_are_checked():
    L = _lib.load()
    t = all_traces()[:1].copy()
    out = np.zeros(1, _lib.KEY_RESULT_DTYPE)
    bad = t.copy()
    bad['key_type'] = 0x30
    assert L.nfc_host_recover_keys(bad.ctypes.data, 1, None, out.ctypes.data, None) == -1
    for cfg in (_lib.KeyConfig(1 << 20, 1 << 16, 0, 0), _lib.KeyConfig(0, 1 << 33, 0, 0), _lib.KeyConfig(0, 0, 5000, 0), _lib.KeyConfig(0, 0, 0, 2)):
        assert L.nfc_host_recover_keys(t.ctypes.data, 1, C.byref(cfg), out.ctypes.data, None) == -1
        assert L.nfc_recover_keys_device(0, t.ctypes.data, 1, C.byref(cfg), out.ctypes.data, None) == -1   # (before the device is touched)
    r, st = keys.host_recover(t[:0])
    assert len(r) == 0 and st.n_batches == 0 and st.scratch_bytes == 0
