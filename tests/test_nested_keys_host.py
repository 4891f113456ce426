"""Key recovery from NESTED authentications on the CPU: nfc_find_nested_auths, nfc_host_nested_candidates, nfc_host_recover_nested_keys
and keys.label_auths (csrc/keys.hip.h, nfc_keys.hip) on the reference's own printed trace -- one first and fifteen nested
authentications -- and on traces crafted with the project's machine.  No GPU.  tests/test_nested_keys.py holds the GPU half and uses the
traces below.  Every comparison is for equality.

The twin costs a quarter of a second per candidate, so it only ever searches windows of at most two candidates: eight searches in the file."""
import ctypes as C
import io
import os

import numpy as np

from tests.test_frames import GOLD_1K, host_frames_of, packets_from_trace
from tests.test_keys_host import AUTHA, AUTHB, FF, RANDRB, RANDTA, RANDTB, reference_frames, word
from usrp_nfc_amd import _lib, fsm, keys, synth
from usrp_nfc_amd.command import CommandType

READR, READT = 21, 22   # indices of the command table
_rng = np.random.RandomState(20252)
KEY_A, KEY_B = _rng.randint(0, 256, 6).tolist(), _rng.randint(0, 256, 6).tolist()
UID = _rng.randint(0, 256, 4).tolist()
NT1, NR1, NR2 = (_rng.randint(0, 256, 4).tolist() for _ in range(3))
SEED2 = int(_rng.randint(0, 1 << 16))
BLOCK_DATA = _rng.randint(0, 256, 16).tolist()
_cache = {}


# ---- the nonce sequence and the ten tests, restated with numpy ------------------------------------------------------------------------
def extend(seed):
    """The 32 nonce bits from the first 16: b[k + 16] = b[k] ^ b[k + 2] ^ b[k + 3] ^ b[k + 5]; seed: an array of 16-bit seeds."""
    x = np.asarray(seed, np.uint64) & np.uint64(0xFFFF)
    for k in range(16):
        k = np.uint64(k)
        bit = ((x >> k) ^ (x >> (k + np.uint64(2))) ^ (x >> (k + np.uint64(3))) ^ (x >> (k + np.uint64(5)))) & np.uint64(1)
        x = x | (bit << (k + np.uint64(16)))
    return x


def advance(x, ticks):
    """The nonce register `ticks` clocks on: a 32-bit window over the same sequence."""
    x = np.asarray(x, np.uint64)
    for _ in range(ticks):
        bit = ((x >> np.uint64(16)) ^ (x >> np.uint64(18)) ^ (x >> np.uint64(19)) ^ (x >> np.uint64(21))) & np.uint64(1)
        x = (x >> np.uint64(1)) | (bit << np.uint64(31))
    return x


def on_sequence(nt):
    return int(extend(int(nt) & 0xFFFF)) == int(nt)


def byte_parity(x, b):
    v = (np.asarray(x, np.uint64) >> np.uint64(8 * b)) & np.uint64(0xFF)
    p = np.zeros_like(v)
    for i in range(8):
        p ^= (v >> np.uint64(i)) & np.uint64(1)
    return p


def numpy_candidates(t, stages=None):
    """The ten ninth-bit tests over all 65 536 seeds: ninth_received ^ ks_bit == 1 ^ parity(plaintext byte), with the keystream bit of the
    NEXT data bit -- ks1 = {nt} ^ nt, ks2 = {ar} ^ suc64(nt), ks3 = {at} ^ suc96(nt).  stages: a list that gets the number of seeds left
    after the {nt} tests, after the {ar} tests and after the {at} tests."""
    nt = extend(np.arange(1 << 16))
    ar = advance(nt, 64)
    at = advance(ar, 32)
    ks1, ks2, ks3 = np.uint64(int(t['nt_enc'])) ^ nt, np.uint64(int(t['ar_enc'])) ^ ar, np.uint64(int(t['at_enc'])) ^ at
    par = int(t['par'])
    bit = lambda x, i: (x >> np.uint64(i)) & np.uint64(1)
    ok = np.ones(1 << 16, bool)
    counts = []
    for first, ks, pt in ((12, ks1, nt), (4, ks2, ar), (8, ks3, at)):
        for b in range(3):
            ok &= (np.uint64((par >> (first + b)) & 1) ^ bit(ks, 8 * b + 8)) == (np.uint64(1) ^ byte_parity(pt, b))
        if first == 4:
            ok &= (np.uint64((par >> 7) & 1) ^ bit(ks3, 0)) == (np.uint64(1) ^ byte_parity(ar, 3))
        counts.append(int(ok.sum()))
    if stages is not None:
        stages.extend(counts)
    return nt[ok].astype(np.uint32)


# ---- CRYPTO1's filter, restated: what encrypts a nested tag nonce (the machine's emulator side does not make that frame) -------------
def _fa(a, b, c, d):
    return ((a | b) ^ (a & d)) ^ (c & ((a ^ b) | d))


def _fb(a, b, c, d):
    return ((a & b) | c) ^ ((a ^ b) & (c | d))


def _fc(a, b, c, d, e):
    return (a | ((b | e) & (d ^ e))) ^ ((a ^ (b & d)) & ((c ^ d) | (b & e)))


def _filter(st):
    b = lambda i: (st >> i) & 1
    return _fc(_fa(b(9), b(11), b(13), b(15)), _fb(b(17), b(19), b(21), b(23)), _fb(b(25), b(27), b(29), b(31)), _fa(b(33), b(35), b(37), b(39)),
               _fb(b(41), b(43), b(45), b(47)))


_TAPS = sum(1 << t for t in (0, 5, 9, 10, 12, 14, 15, 17, 19, 24, 25, 27, 29, 35, 39, 41, 42, 43))


def nested_nonce_bits(key, uid, nt):
    """{nt} with its ninth bits as a card sends it in a nested authentication: the register holds the new key, every nonce bit is
    encrypted with the filter's output and uid ^ nt goes in; a ninth bit takes the keystream bit of the next data bit."""
    st = sum(int(k) << (8 * i) for i, k in enumerate(key))
    out = []
    for i in range(4):
        x = nt[i] ^ uid[i]
        for k in range(8):
            out.append(((nt[i] >> k) & 1) ^ _filter(st))
            st = (st >> 1) | (((bin(st & _TAPS).count('1') ^ (x >> k)) & 1) << 47)
        out.append((1 - (bin(nt[i]).count('1') & 1)) ^ _filter(st))
    return out


# ---- traces --------------------------------------------------------------------------------------------------------------------------
def golden_nested():
    if 'golden' not in _cache:
        t = keys.find_nested_auths(reference_frames())
        t.setflags(write=False)
        _cache['golden'] = t
    return _cache['golden']


def golden_candidates():
    if 'cands' not in _cache:
        _cache['cands'] = keys.nested_candidates(golden_nested())
    return _cache['cands']


def printed(lines_after, what):
    """The EXTRA bytes printed after every encrypted `what` (RANDTA / RANDRB) of the trace, as words, in order."""
    lines = packets_from_trace(GOLD_1K)[1].split('\n')
    out = []
    for i, l in enumerate(lines):
        if l == 'COMMAND: ' + what and lines[i - 1 - lines_after].startswith('0x'):
            out.append(word([int(v, 16) for v in lines[i + 1].split()[1:5]]))
    return out


def golden_true_index(i):
    """Where the printed plaintext nt of golden nested trace i lies in its candidate list."""
    return golden_candidates()[0][i].tolist().index(printed(0, 'RANDTA')[i])


def two_key_packets(nt2, read=True):
    """One card, two keys, made with the project's machine as tests/test_keys_host.py's crafted_trace makes a first authentication: AUTHA
    on block 4 under KEY_A, then -- encrypted -- AUTHB on block 8 under KEY_B with the nested nonce nt2, then an encrypted READ of block 8
    and its answer.  The machine encrypts every frame but {nt2}, which nested_nonce_bits states.  -> packets (type, bits)."""
    m = fsm.fsm(out=io.StringIO())
    m.set_keys(KEY_A, KEY_B)
    crc = lambda d: d + fsm.crc_a(d)
    by = CommandType.by_index
    packets = [(0, synth.frame_bits([0x04, 0x00])), (1, synth.frame_bits(crc([0x93, 0x70] + UID + [UID[0] ^ UID[1] ^ UID[2] ^ UID[3]]))),
               (1, synth.frame_bits(crc([0x60, 4])))]
    for t, bits in packets:
        m.process_bits(bits, t)
    packets.append((0, m.process_outgoing(synth.frame_bits(NT1), by(RANDTA))))
    packets.append((1, m.process_outgoing(synth.frame_bits(NR1 + list(m.get_state().ar)), by(RANDRB))))
    packets.append((0, m.process_outgoing(synth.frame_bits(list(m.get_state().at)), by(RANDTB))))
    packets.append((1, m.process_outgoing(synth.frame_bits(crc([0x61, 8])), by(AUTHB))))
    st = m.get_state()
    st.cur_key = 1   # (a heard AUTHB selects key B; the emulator side leaves the choice to its caller)
    m.set_state(st)
    m.process_outgoing(synth.frame_bits(nt2), by(RANDTA))   # the new register: KEY_B, uid ^ nt2; what it returns is not what a card sends
    packets.append((0, nested_nonce_bits(KEY_B, UID, nt2)))
    packets.append((1, m.process_outgoing(synth.frame_bits(NR2 + list(m.get_state().ar)), by(RANDRB))))
    packets.append((0, m.process_outgoing(synth.frame_bits(list(m.get_state().at)), by(RANDTB))))
    if read:
        packets.append((1, m.process_outgoing(synth.frame_bits(crc([0x30, 8])), by(READR))))
        packets.append((0, m.process_outgoing(synth.frame_bits(crc(BLOCK_DATA)), by(READT))))
    return packets


def bytes_of(x):
    return [(int(x) >> (8 * i)) & 0xFF for i in range(4)]


def two_key_frames():
    if 'two' not in _cache:
        _cache['two'] = host_frames_of(two_key_packets(bytes_of(extend(SEED2))))[0]
    return _cache['two']


def off_sequence_nested():
    """The same card with a nested nonce that is not on the sequence (bit 31 of the right one flipped): its nested trace."""
    if 'off' not in _cache:
        nt = int(extend(SEED2)) ^ (1 << 31)
        assert not on_sequence(nt)
        t = keys.find_nested_auths(host_frames_of(two_key_packets(bytes_of(nt)))[0])
        assert len(t) == 1
        _cache['off'] = t
    return _cache['off']


def damaged_nested():
    """Golden nested trace 0 with bit 5 of nt_enc flipped, and with bit 13 of ar_enc flipped."""
    a, b = golden_nested()[:1].copy(), golden_nested()[:1].copy()
    a['nt_enc'] ^= 1 << 5
    b['ar_enc'] ^= 1 << 13
    return a, b


def all_nested():
    """Every nested trace of the two test files: the fifteen golden ones, the crafted one, the off-sequence one, the two damaged ones."""
    return np.concatenate([golden_nested(), keys.find_nested_auths(two_key_frames()), off_sequence_nested()] + list(damaged_nested()))


def assert_same_nested(got, want):
    for name in ('key', 'status', 'n_verified', 'n_nt', 'n_searched', 'nt', 'nr', 'n_odd', 'n_even'):
        assert got[name].tolist() == want[name].tolist(), name


# ---- 1. the golden trace: finding ----------------------------------------------------------------------------------------------------
def test_golden_trace_nested_authentications_are_found():
    frames = reference_frames()
    table, _ = fsm.fsm(out=io.StringIO()).process_frames(frames, dispatch=False)
    auth = np.nonzero((table['cmd'] == AUTHA) | (table['cmd'] == AUTHB))[0]
    nested = [int(i) for i in auth if table['flags'][i] & fsm.FRAME_ENCRYPTED]
    t = golden_nested()
    assert len(t) == 15 and t['frame'].tolist() == nested and nested[0] == 18
    assert len(keys.find_auths(frames)) == 1
    assert frames.table['idx'][t['frame']].tolist() == t['idx'].tolist()
    assert t['uid'].tolist() == [word([0xCD, 0x76, 0x92, 0x74])] * 15 and t['stream'].tolist() == [0] * 15
    assert t['key_type'].tolist() == [0] * 15 and t['block'].tolist() == [0xFF] * 15
    t0 = t[0]
    assert int(t0['nt_enc']) == word([0x70, 0xBD, 0xED, 0x81])
    assert (int(t0['nr_enc']), int(t0['ar_enc']), int(t0['at_enc'])) == (word([0xFC, 0x1A, 0x1A, 0x1D]), word([0x7D, 0x90, 0x7E, 0x24]), word([0x87, 0x4D, 0xFF, 0x8A]))
    # the ninth bits: '!' where the parity bit EQUALS the data parity -- 0x70! 0xBD 0xED! 0x81 / 0xFC! 0x1A 0x1A! 0x1D! 0x7D! 0x90 0x7E! 0x24! /
    # 0x87 0x4D 0xFF! 0x8A (lines 112, 117 and 123 of the trace); bits 0 .. 7 {nr}{ar}, 8 .. 11 {at}, 12 .. 15 {nt}
    lines = open(GOLD_1K).read().split('\n')
    toks = lines[116].split() + lines[122].split() + lines[111].split()
    assert [x.rstrip('!') for x in toks] == ['0xFC', '0x1A', '0x1A', '0x1D', '0x7D', '0x90', '0x7E', '0x24', '0x87', '0x4D', '0xFF', '0x8A', '0x70', '0xBD', '0xED', '0x81']
    ones = lambda x: bin(int(x.rstrip('!'), 16)).count('1') & 1
    assert int(t0['par']) == sum((ones(x) if x.endswith('!') else 1 - ones(x)) << i for i, x in enumerate(toks))


# ---- 2. candidates -------------------------------------------------------------------------------------------------------------------
def test_golden_trace_has_64_candidates_each_and_the_printed_nonce_among_them():
    nt, n = golden_candidates()
    want_nt = printed(0, 'RANDTA')
    assert len(want_nt) == 15 and want_nt[0] == word([0x8F, 0x82, 0x69, 0x9E])
    assert n.tolist() == [64] * 15
    for i, t in enumerate(golden_nested()):
        c = nt[i]
        seeds = (c & 0xFFFF).tolist()
        assert seeds == sorted(set(seeds)) and all(on_sequence(x) for x in c.tolist())
        assert want_nt[i] in c.tolist() and on_sequence(want_nt[i])
        stages = []
        assert c.tolist() == numpy_candidates(t, stages).tolist()
        assert stages == [8192, 512, 64]   # three, four and three independent linear tests: rank 10 of 16


def test_labels_of_the_whole_golden_card():
    # with every key known (FF FF FF FF FF FF, as the window recoveries find) every nested AUTH command decrypts: sixteen sectors
    frames = reference_frames()
    firsts, nested = keys.find_auths(frames), keys.find_nested_auths(frames)
    fr, nr = np.zeros(1, _lib.KEY_RESULT_DTYPE), np.zeros(15, _lib.NESTED_RESULT_DTYPE)
    fr['key'], nr['key'] = 0xFF, 0xFF
    found = keys.label_auths(frames, firsts, fr, nested, nr)
    assert found == {(0x60, b): bytes(bytearray(FF)) for b in range(0, 0x40, 4)}
    assert nested['key_type'].tolist() == [0x60] * 15 and nested['block'].tolist() == list(range(0x38, -1, -4))
    # one key in the middle missing: its own sector and the label of the one after it are lost, the rest stays
    nr['status'][4] = keys.NFC_KEY_NONE
    again = keys.find_nested_auths(frames)
    found = keys.label_auths(frames, firsts, fr, again, nr)
    assert sorted(b for _, b in found) == sorted(set(range(0, 0x40, 4)) - {0x28, 0x24})
    assert (int(again[4]['block']), int(again[5]['block']), int(again[6]['block'])) == (0x28, 0xFF, 0x20)


# ---- 3. recovery on a window ---------------------------------------------------------------------------------------------------------
def golden_window_results():
    """The twin on golden nested traces 0 and 14, each on the one-candidate window of its printed nt: [(result, stats), ...]."""
    if 'win' not in _cache:
        _cache['win'] = [keys.host_recover_nested(golden_nested()[i:i + 1], cand_first=golden_true_index(i), cand_count=1) for i in (0, 14)]
    return _cache['win']


def test_golden_trace_recovery_on_the_window_of_the_true_nonce():
    want_nt, want_nr = printed(0, 'RANDTA'), printed(1, 'RANDRB')[1:]   # (the first authentication's {nr}{ar} is ciphertext too)
    assert want_nr[0] == word([0x01, 0x3A, 0x6B, 0xBA]) and len(want_nr) == 15
    for i, (r, st) in zip((0, 14), golden_window_results()):
        r = r[0]
        assert int(r['status']) == keys.NFC_KEY_OK and r['key'].tolist() == FF
        assert (int(r['nt']), int(r['nr'])) == (want_nt[i], want_nr[i])
        assert (int(r['n_verified']), int(r['n_nt']), int(r['n_searched'])) == (1, 64, 1)
        assert int(r['n_odd']) > 0 and int(r['n_even']) > 0 and (st.n_batches, st.n_launches) == (1, 0)


def test_a_window_without_the_true_nonce_gives_none():
    i = golden_true_index(0)
    r, _ = keys.host_recover_nested(golden_nested()[:1], cand_first=(i + 1) % 64, cand_count=1)
    r = r[0]
    assert int(r['status']) == keys.NFC_KEY_NONE and r['key'].tolist() == [0] * 6 and (int(r['nt']), int(r['nr']), int(r['n_verified'])) == (0, 0, 0)
    assert (int(r['n_nt']), int(r['n_searched'])) == (64, 1)
    # a window behind the list searches nothing
    r, st = keys.host_recover_nested(golden_nested()[:2], cand_first=64)
    assert r['status'].tolist() == [keys.NFC_KEY_NONE] * 2 and r['n_searched'].tolist() == [0, 0] and r['n_nt'].tolist() == [64, 64]
    assert (st.n_batches, st.scratch_bytes) == (0, 0)


# ---- 4. two keys on one card ---------------------------------------------------------------------------------------------------------
def test_two_keys_on_one_card():
    assert KEY_A != KEY_B
    frames = two_key_frames()
    firsts, nested = keys.find_auths(frames), keys.find_nested_auths(frames)
    assert len(firsts) == 1 and len(nested) == 1 and int(nested[0]['frame']) == 6 and (int(nested[0]['key_type']), int(nested[0]['block'])) == (0, 0xFF)
    nt2 = int(extend(SEED2))
    c, n = keys.nested_candidates(nested)
    assert int(n[0]) == 64 and c[0].tolist() == numpy_candidates(nested[0]).tolist()
    i = c[0].tolist().index(nt2)
    fr, _ = keys.host_recover(firsts)
    nr, _ = keys.host_recover_nested(nested, cand_first=i, cand_count=1)
    assert int(fr['status'][0]) == keys.NFC_KEY_OK and fr['key'][0].tolist() == KEY_A
    assert int(nr['status'][0]) == keys.NFC_KEY_OK and nr['key'][0].tolist() == KEY_B
    assert (int(nr['nt'][0]), int(nr['nr'][0]), int(nr['n_verified'][0])) == (nt2, word(NR2), 1)
    found = keys.label_auths(frames, firsts, fr, nested, nr)
    assert found == {(0x60, 4): bytes(bytearray(KEY_A)), (0x61, 8): bytes(bytearray(KEY_B))}
    assert (int(nested[0]['key_type']), int(nested[0]['block'])) == (0x61, 8)
    # with both keys set the machine decrypts the READ behind the nested authentication
    m = fsm.fsm(out=io.StringIO())
    m.set_keys(*keys.first_keys(found))
    table, data = m.process_frames(frames, dispatch=False)
    assert int(((table['flags'] & fsm.FRAME_AR_OK) != 0).sum()) == 2 and int(((table['flags'] & fsm.FRAME_AT_OK) != 0).sum()) == 2
    assert table['cmd'].tolist()[-2:] == [READR, READT]
    o = int(table['byte_off'][-1])
    assert data[o:o + 16].tolist() == BLOCK_DATA
    # a nested authentication whose predecessor's key is not known stays unlabelled
    none = fr.copy()
    none['status'] = keys.NFC_KEY_NONE
    again = keys.find_nested_auths(frames)
    assert keys.label_auths(frames, firsts, none, again, nr) == {} and (int(again[0]['key_type']), int(again[0]['block'])) == (0, 0xFF)


# ---- 5. damage -----------------------------------------------------------------------------------------------------------------------
def test_damaged_traces_give_no_key():
    bad_nt, bad_ar = damaged_nested()
    i = golden_true_index(0)
    # {nt}: the candidates are other ones or none; the true nonce's keystream no longer fits
    (_, n), = [keys.nested_candidates(bad_nt)]
    assert int(n[0]) in (0, 64)
    r, _ = keys.host_recover_nested(bad_nt, cand_first=i, cand_count=1)
    assert int(r['status'][0]) == keys.NFC_KEY_NONE and int(r['n_nt'][0]) == int(n[0]) and r['key'][0].tolist() == [0] * 6
    # {ar}: bit 13 is no bit the ten tests read, so the true nonce is still a candidate at the same place; 64 keystream bits with one
    # flipped over-determine the register (tests/test_keys_host.py: test_corrupted_trace_gives_none)
    c, n = keys.nested_candidates(bad_ar)
    assert int(n[0]) == 64 and c[0].tolist() == golden_candidates()[0][0].tolist()
    r, _ = keys.host_recover_nested(bad_ar, cand_first=i, cand_count=1)
    assert int(r['status'][0]) == keys.NFC_KEY_NONE and (int(r['n_nt'][0]), int(r['n_searched'][0])) == (64, 1) and r['key'][0].tolist() == [0] * 6


def test_a_nonce_off_the_sequence_gives_no_wrong_key():
    t = off_sequence_nested()
    _, n = keys.nested_candidates(t)
    assert int(n[0]) in (0, 64)
    r, _ = keys.host_recover_nested(t, cand_first=0, cand_count=2)
    assert int(r['n_nt'][0]) == int(n[0]) and int(r['status'][0]) == keys.NFC_KEY_NONE and r['key'][0].tolist() == [0] * 6
    assert int(r['n_searched'][0]) == (2 if int(n[0]) else 0)


# ---- 6. ABI and arguments --------------------------------------------------------------------------------------------------------------
NAMES = ['nfc_find_nested_auths', 'nfc_host_nested_candidates', 'nfc_nested_candidates_device', 'nfc_host_recover_nested_keys',
         'nfc_recover_nested_keys_device']


def test_new_names_are_declared_and_bound():
    assert set(NAMES) <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(getattr(L, n).argtypes for n in NAMES)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'nfc_amd.h')).read()
    assert all(n + '(' in header for n in NAMES) and '#define NFC_AMD_ABI_VERSION 4' in header and _lib.ABI_VERSION == 4 and L.nfc_abi_version() == 4
    assert all(n in header for n in ('nfc_nested_trace', 'nfc_nested_result', 'nfc_nested_config'))
    assert _lib.NESTED_DTYPE.itemsize == 40 and _lib.NESTED_RESULT_DTYPE.itemsize == 48 and C.sizeof(_lib.NestedConfig) == 48
    assert _lib.NESTED_DTYPE.names == tuple(n if n != 'nt' else 'nt_enc' for n in _lib.AUTH_DTYPE.names)
    assert [_lib.NESTED_DTYPE.fields[n][1] for n in _lib.NESTED_DTYPE.names] == [_lib.AUTH_DTYPE.fields[n][1] for n in _lib.AUTH_DTYPE.names]


def test_arguments_are_checked():
    L = _lib.load()
    t = golden_nested()[:1].copy()
    out = np.zeros(1, _lib.NESTED_RESULT_DTYPE)
    K = _lib.KeyConfig
    bad = [_lib.NestedConfig(K(), 65, 0), _lib.NestedConfig(K(), 0, 0, (C.c_uint32 * 2)(1, 0)), _lib.NestedConfig(K(), 0, 0, (C.c_uint32 * 2)(0, 1)),
           _lib.NestedConfig(K(1 << 20, 1 << 16, 0, 0)), _lib.NestedConfig(K(0, 1 << 33, 0, 0)), _lib.NestedConfig(K(0, 0, 5000, 0)),
           _lib.NestedConfig(K(0, 0, 0, 2)), _lib.NestedConfig(K(0, 0, 0, 0, (C.c_uint32 * 2)(0, 1)))]
    for cfg in bad:
        assert L.nfc_host_recover_nested_keys(t.ctypes.data, 1, C.byref(cfg), out.ctypes.data, None) == -1
        assert L.nfc_recover_nested_keys_device(0, t.ctypes.data, 1, C.byref(cfg), out.ctypes.data, None) == -1   # (before the device is touched)
    assert L.nfc_host_recover_nested_keys(None, 1, None, out.ctypes.data, None) == -1
    assert L.nfc_recover_nested_keys_device(-1, t.ctypes.data, 1, None, out.ctypes.data, None) == -1
    n = C.c_size_t(7)
    assert L.nfc_host_nested_candidates(None, None, 0, C.byref(n)) == -1
    assert L.nfc_host_nested_candidates(t.ctypes.data, None, 0, C.byref(n)) == 0 and n.value == 64   # (cap 0: the count alone)
    # n == 0 launches nothing and touches no device: this test runs without one
    r, st = keys.host_recover_nested(t[:0])
    assert len(r) == 0 and (st.n_batches, st.n_launches, st.scratch_bytes) == (0, 0, 0)
    r, st = keys.recover_nested(t[:0], device=0)
    assert len(r) == 0 and (st.n_batches, st.n_launches, st.scratch_bytes) == (0, 0, 0)
    nt, cnt = keys.nested_candidates(t[:0], device=0)
    assert nt.shape == (0, 64) and len(cnt) == 0
