"""The per-sector key table of the protocol machines on the CPU (include/nfc_amd.h: nfc_fsm_key_table; csrc/sector_keys.h):
the host machine (csrc/protocol.h over csrc/fsm.hip.h), the kernel's twin nfc_host_commands_keyed (the same text, the capped UID) and the Python layers, on cards
whose sectors have DIFFERENT keys.  No GPU.  tests/test_sector_keys.py holds the GPU half and uses the cards and helpers below.  Every
comparison is for equality.

THE CARDS are made without the table: the project's own machine, re-keyed by hand with set_keys(K_i, K_i) before every authentication,
encrypts every frame through process_outgoing, and nested_nonce_bits states {nt} -- the way two_key_packets of
tests/test_nested_keys_host.py makes its card, with nothing but behaviour the suite pinned before the table existed.
  CARD 1 (1K)  AUTHA 4 under K0 (first) READ 4 / nested AUTHA 8 under K1 READ 8 / nested AUTHB 12 under K2 READ 12 / nested AUTHA 5
               (sector 1 again: K0) READ 5.  26 frames.
  CARD 2 (4K)  ATQA 4K, AUTHA 144 under K3 (first), nested AUTHA 159 (the same sector 33: K3), nested AUTHA 160 (sector 34: K4).
The nonce seeds are constants: with them every authentication of card 1 has exactly one verified key (test_card_1_keys_are_unambiguous),
which the GPU half's recovery test relies on."""
import ctypes as C
import io

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from tests.test_commands_host import assert_commands_equal, host_machine, prefix_frames, run_host, state_bytes
from tests.test_frames import host_frames_of
from tests.golden_util import Case
from tests.test_keys_host import AUTHA, AUTHB, RANDRB, RANDTA, RANDTB
from tests.test_nested_keys_host import READR, READT, bytes_of, extend, nested_nonce_bits
from usrp_nfc_amd import _lib, api, fsm, keys, synth
from usrp_nfc_amd.command import CommandType

A, B = 0x60, 0x61
_rng = np.random.RandomState(8240)
K0, K1, K2, K3, K4, WRONG = (_rng.randint(0, 256, 6).tolist() for _ in range(6))
UID = _rng.randint(0, 256, 4).tolist()
BLOCKS = {b: _rng.randint(0, 256, 16).tolist() for b in (4, 8, 12, 5)}
NRS = [_rng.randint(0, 256, 4).tolist() for _ in range(4)]
SEEDS_1 = (0x3A17, 0x9C42, 0x51E8, 0xD06B)   # the 16-bit seeds of card 1's four tag nonces (first, then the three nested ones)
SEEDS_2 = (0x1234, 0xBEEF, 0x7A5C)
CARD_1 = ((A, 4, K0), (A, 8, K1), (B, 12, K2), (A, 5, K0))       # (key_type, block, key) per authentication, a READ after each
CARD_2 = ((A, 144, K3), (A, 159, K3), (A, 160, K4))              # no READs
TABLE_1 = {(A, 1): K0, (A, 2): K1, (B, 3): K2}
TABLE_2 = {(A, 33): K3, (A, 34): K4}
_cache = {}


# ---- the cards, made without the feature ---------------------------------------------------------------------------------------------
def card_packets(auths, seeds, atqa=(0x04, 0x00), reads=True, plain=None):
    """-> packets (type, bits) as they are on the air.  plain: a list that gets (type, plain bits with parity, command index, what the
    generating machine's process_outgoing returned) per packet, the last two None for a frame the machine only heard -- what an emulator
    would hand to process_outgoing, and what it should get back.  The generating machine is told ATQA 1K whatever `atqa` says: its
    emulator side only encrypts for that tag type, and CRYPTO1 does not depend on the answer."""
    m = fsm.fsm(out=io.StringIO())
    crc = lambda d: list(d) + fsm.crc_a(list(d))
    by = CommandType.by_index
    plain = plain if plain is not None else []
    packets = []

    def heard(t, data):
        bits = synth.frame_bits(data)
        plain.append((t, bits, None, None))
        packets.append((t, bits))
        return bits

    def sent(t, data, cmd):
        bits = synth.frame_bits(data)
        out = m.process_outgoing(bits, by(cmd))
        plain.append((t, bits, cmd, out))
        packets.append((t, out))

    heard(0, list(atqa))
    m.process_bits(synth.frame_bits([0x04, 0x00]), 0)
    m.process_bits(heard(1, crc([0x93, 0x70] + UID + [UID[0] ^ UID[1] ^ UID[2] ^ UID[3]])), 1)
    for i, ((key_type, block, key), seed) in enumerate(zip(auths, seeds)):
        nt = bytes_of(extend(seed))
        auth = crc([key_type, block])
        m.set_keys(key, key)
        if i == 0:
            m.process_bits(heard(1, auth), 1)
            sent(0, nt, RANDTA)
        else:
            sent(1, auth, AUTHA if key_type == A else AUTHB)
            bits = synth.frame_bits(nt)
            plain.append((0, bits, RANDTA, m.process_outgoing(bits, by(RANDTA))))   # the new register: key, uid ^ nt; what it returns is not what a card sends
            packets.append((0, nested_nonce_bits(key, UID, nt)))
        sent(1, NRS[i] + list(m.get_state().ar), RANDRB)
        sent(0, list(m.get_state().at), RANDTB)
        if reads:
            sent(1, crc([0x30, block]), READR)
            sent(0, crc(BLOCKS[block]), READT)
    return packets


def card(which):
    """(packets, NfcFrames) of card 1 / 2, made once."""
    if which not in _cache:
        p = card_packets(CARD_1, SEEDS_1) if which == 1 else card_packets(CARD_2, SEEDS_2, atqa=(0x02, 0x00), reads=False)
        fr = host_frames_of(p)[0]
        for a in (fr.table,) + tuple(fr.bytes) + tuple(fr.par):
            a.setflags(write=False)
        _cache[which] = (p, fr)
    return _cache[which]


def ultralight_frames():
    if 'ul' not in _cache:
        _cache['ul'] = host_frames_of(Case('fx_ultralight_txn').packets)[0]
    return _cache['ul']


def keyed_machine(table=None, pair=None):
    m = host_machine(pair)
    if table is not None:
        m.set_sector_keys(table)
    return m


def keyed_state(pair=None):
    s = fsm.state_init()
    if pair:
        s.key_a[:], s.key_b[:] = pair[0], pair[1]
    return s


def read_answers(table, data):
    """The plaintext of every READT record with a good CRC: [(16 bytes)] in order."""
    out = []
    for f in table[(table['cmd'] == READT) & (table['n_crc'] == 2)]:
        o = int(f['byte_off'])
        out.append(data[o:o + 16].tolist())
    return out


def flag_count(table, bit):
    return int(((table['flags'] & bit) != 0).sum())


def twin_and_host(frames, table, pair, cuts):
    """nfc_host_commands_keyed against nfc_fsm_process_frames with the same table and keys over slices of the frames, the state handed
    on: every record, the bytes, the enc entries and the state after every slice are equal.  -> the twin's final state."""
    m, s = keyed_machine(table, pair), keyed_state(pair)
    t = frames.table
    edges = [0] + sorted(set(cuts)) + [len(t)]
    for a, b in zip(edges[:-1], edges[1:]):
        part = t[a:b]
        want = run_host(m, api.NfcFrames([part[part['type'] == 0], part[part['type'] == 1]], frames.bytes, frames.par))
        got = fsm.host_commands(s, part, frames.bytes, frames.par, sector_keys=table)
        assert_commands_equal(got, want, part['n_bytes'])
        assert state_bytes(s) == state_bytes(m.get_state())
    return s


def auth_and_nonce_cuts(frames, table):
    """Where a slice ends between an AUTH frame and its nonce, and between the nonce and {nr}{ar}: the frame indices to cut BEFORE."""
    t, _, _ = fsm.host_commands(keyed_state(), frames, sector_keys=table)
    auth = np.nonzero((t['cmd'] == AUTHA) | (t['cmd'] == AUTHB))[0]
    return sorted((auth + 1).tolist() + (auth + 2).tolist())


# ---- 1. the failing test: one key A and one key B lose the card, the table reads all of it ------------------------------------------
def test_the_table_decrypts_a_card_whose_sectors_have_different_keys():
    _, frames = card(1)
    assert len(frames.table) == 26
    # today's machine: K0 opens sector 1, the nested AUTHA of block 8 is keyed with K0 again and the session is lost
    m = host_machine((K0, K2))
    t, d = m.process_frames(frames, dispatch=False)
    assert t['cmd'][:9].tolist() == [3, 9, AUTHA, RANDTA, RANDRB, RANDTB, READR, READT, AUTHA]
    # (sectors 2 and 3 are lost: frames 8 .. 19.  The command in flight stays AUTHA while nothing is recognised, so every frame is taken
    # for a nested nonce under K0 -- and the nonce of the fourth authentication, sector 1 again, IS one: the session comes back for it)
    assert read_answers(t, d) == [BLOCKS[4], BLOCKS[5]]
    assert flag_count(t[8:20], fsm.FRAME_AT_OK | fsm.FRAME_AR_OK) == 0 and not (t['cmd'][9:20] == READT).any()
    assert flag_count(t, fsm.FRAME_AT_OK) == 2 and flag_count(t, fsm.FRAME_AR_OK) == 2
    # with the table every READ answer is the plaintext block with a good CRC
    out = io.StringIO()
    m = host_machine((K0, K2), out=out)
    m.set_sector_keys(TABLE_1)
    assert m.sector_keys() == {k: bytes(bytearray(v)) for k, v in TABLE_1.items()}
    t, d = m.process_frames(frames)
    assert read_answers(t, d) == [BLOCKS[4], BLOCKS[8], BLOCKS[12], BLOCKS[5]]
    assert flag_count(t, fsm.FRAME_AR_OK) == 4 and flag_count(t, fsm.FRAME_AT_OK) == 4
    assert flag_count(t, fsm.FRAME_AR_ERROR | fsm.FRAME_AT_ERROR) == 0 and (t['cmd'] >= 0).all()
    text = out.getvalue()
    assert text.count('AR OK') == 4 and text.count('AT OK') == 4 and text.count('COMMAND: READT') == 4
    for block, data in BLOCKS.items():   # the four blocks, as the reference's traces print a READ answer
        assert 'COMMAND: READT\nEXTRA: ' + ''.join('0x%02X ' % v for v in data) + '\n' in text, block
    # the same through the twin and fsm.dispatch, with the DEFAULT two keys: the table alone carries the card
    tt, td, te = fsm.host_commands(keyed_state(), frames, sector_keys=TABLE_1)
    assert read_answers(tt, td) == [BLOCKS[4], BLOCKS[8], BLOCKS[12], BLOCKS[5]]
    shown = io.StringIO()
    fsm.dispatch(tt, td, te, out=shown)
    assert shown.getvalue() == text


# ---- 2. the sector mapping ---------------------------------------------------------------------------------------------------------
def test_sector_of_every_block():
    for block in range(256):
        want = block >> 2 if block < 128 else 32 + ((block - 128) >> 4)
        assert keys.sector_of(block) == want == _lib.load().nfc_sector_of_block(block)
    assert max(keys.sector_of(b) for b in range(256)) == 39
    assert _lib.load().nfc_sector_of_block(-1) == -1 and _lib.load().nfc_sector_of_block(256) == -1
    with pytest.raises(ValueError):
        keys.sector_of(256)


def test_4k_card_blocks_144_and_159_share_a_slot_and_160_does_not():
    assert keys.sector_of(144) == keys.sector_of(159) == 33 and keys.sector_of(160) == 34
    _, frames = card(2)
    s = keyed_state()
    t, _, _ = fsm.host_commands(s, frames, sector_keys=TABLE_2)
    assert s.tag_type == 2 and flag_count(t, fsm.FRAME_AT_OK) == 3 and flag_count(t, fsm.FRAME_AR_OK) == 3
    assert s.cur_key == 2 + 34
    # the slot of sector 33 alone: 144 and 159 authenticate, 160 falls back to the default key A and fails
    t, _, _ = fsm.host_commands(keyed_state(), frames, sector_keys={(A, 33): K3})
    assert flag_count(t, fsm.FRAME_AT_OK) == 2 and flag_count(t[:-4], fsm.FRAME_AT_OK) == 2
    # the slot of sector 34 alone with K3 as key A: the same three, the other way round
    t, _, _ = fsm.host_commands(keyed_state((K3, K3)), frames, sector_keys={(A, 34): K4})
    assert flag_count(t, fsm.FRAME_AT_OK) == 3


# ---- 3. an empty table changes nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['classic', 'ultralight'])
def test_an_empty_table_is_no_table(name):
    frames = prefix_frames() if name == 'classic' else ultralight_frames()
    t = frames.table
    for cut in [None] + list(range(1, min(30, len(t)))):
        edges = [0, len(t)] if cut is None else [0, cut, len(t)]
        states = [keyed_state() for _ in range(3)]
        for a, b in zip(edges[:-1], edges[1:]):
            want = fsm.host_commands(states[0], t[a:b], frames.bytes, frames.par)
            for s, table in ((states[1], {}), (states[2], _lib.FsmKeyTable())):
                got = fsm.host_commands(s, t[a:b], frames.bytes, frames.par, sector_keys=table)
                for g, w in zip(got, want):
                    assert g.tobytes() == w.tobytes()
                assert state_bytes(s) == state_bytes(states[0])
    # ... and for the host machine, against a machine that never saw a table
    m, e = host_machine(), keyed_machine({})
    for g, w in zip(run_host(e, frames), run_host(m, frames)):
        assert g.tobytes() == w.tobytes()
    assert state_bytes(e.get_state()) == state_bytes(m.get_state()) and e.get_state().cur_key in (0, 1)


def test_host_commands_is_host_commands_keyed_with_null():
    L, (_, frames) = _lib.load(), card(1)
    t = np.ascontiguousarray(frames.table, _lib.RAW_FRAME_DTYPE)
    outs = []
    for keyed in (False, True):
        s, cap = keyed_state((K0, K2)), int(t['n_bytes'].sum()) + 1
        out, buf, enc, used = np.zeros(len(t), fsm.FRAME_DTYPE), np.zeros(cap, np.uint8), np.zeros(cap, np.uint16), C.c_size_t(0)
        args = (t.ctypes.data, len(t), frames.bytes[0].ctypes.data, frames.par[0].ctypes.data, frames.bytes[1].ctypes.data, frames.par[1].ctypes.data,
                out.ctypes.data, buf.ctypes.data, enc.ctypes.data, cap, C.byref(used))
        rc = L.nfc_host_commands_keyed(C.byref(s), None, *args) if keyed else L.nfc_host_commands(C.byref(s), *args)
        assert rc == 0
        outs.append((out.tobytes(), buf.tobytes(), enc.tobytes(), used.value, state_bytes(s)))
    assert outs[0] == outs[1]


# ---- 4. the twin equals the host machine --------------------------------------------------------------------------------------------
def test_twin_equals_host_machine_cut_between_auth_nonce_and_answer():
    for which, table, pair in ((1, TABLE_1, (K0, K2)), (1, TABLE_1, None), (2, TABLE_2, None), (1, None, (K0, K2)), (2, {(A, 33): K3}, (K4, K4))):
        _, frames = card(which)
        cuts = auth_and_nonce_cuts(frames, TABLE_1 if which == 1 else TABLE_2)
        assert len(cuts) == (8 if which == 1 else 6)
        whole = twin_and_host(frames, table, pair, [])
        for c in cuts:   # one cut at a time: the choice is carried by the state alone
            assert state_bytes(twin_and_host(frames, table, pair, [c])) == state_bytes(whole)
        assert state_bytes(twin_and_host(frames, table, pair, cuts)) == state_bytes(whole)
    # the choice IS in the state between the AUTH frame and the nonce: 2 + slot of (A, sector 2)
    _, frames = card(1)
    s = keyed_state()
    fsm.host_commands(s, frames.table[:9], frames.bytes, frames.par, sector_keys=TABLE_1)
    assert s.cur_cmd == AUTHA and s.cur_key == 2 + 2
    # a slot emptied between the AUTH frame and the nonce falls back to the key A / B of its type: here to the right key, K1
    s.key_a[:] = K1
    t, d, _ = fsm.host_commands(s, frames.table[9:15], frames.bytes, frames.par, sector_keys={(A, 1): K0})
    assert flag_count(t, fsm.FRAME_AT_OK) == 1 and read_answers(t, d) == [BLOCKS[8]]


_slot = st.sampled_from(['right', 'wrong', 'absent'])


@settings(max_examples=60, deadline=None)
@given(which=st.sampled_from([1, 2]), picks=st.lists(_slot, min_size=3, max_size=3), default_right=st.booleans(),
       cuts=st.sets(st.integers(1, 25), max_size=6))
def test_twin_equals_host_machine_on_random_tables(which, picks, default_right, cuts):
    _, frames = card(which)
    right = TABLE_1 if which == 1 else TABLE_2
    table = {}
    for (slot, key), pick in zip(sorted(right.items()), picks):
        if pick != 'absent':
            table[slot] = key if pick == 'right' else WRONG
    pair = ((K0, K2) if which == 1 else (K3, K3)) if default_right else (WRONG, WRONG)
    twin_and_host(frames, table, pair, [c for c in cuts if c < len(frames.table)])


# ---- 5. state and table hygiene ------------------------------------------------------------------------------------------------------
def test_table_round_trip_reset_and_set_keys():
    m = host_machine()
    assert m.sector_keys() == {}
    m.set_sector_keys(TABLE_1)
    m.set_sector_key(B, 39, K4)
    want = {k: bytes(bytearray(v)) for k, v in list(TABLE_1.items()) + [((B, 39), K4)]}
    assert m.sector_keys() == want
    m.set_keys(K3, K4)
    st0 = m.get_state()
    m.set_state(st0)
    assert m.sector_keys() == want and list(m.get_state().key_a) == K3   # set_keys and set_state leave the table
    m.set_sector_key(A, 1, None)
    del want[(A, 1)]
    assert m.sector_keys() == want
    t = keys.key_table(want)
    m2 = host_machine()
    m2.set_sector_keys(t)
    assert m2.sector_keys() == want and keys.table_dict(t) == want
    m.reset()
    assert m.sector_keys() == {} and list(m.get_state().key_a) == [0xFF] * 6
    m2.set_sector_keys(None)
    assert m2.sector_keys() == {}


def test_bad_arguments_are_rejected_by_name():
    L, m = _lib.load(), host_machine()
    key = (C.c_uint8 * 6)(*K0)
    assert L.nfc_fsm_set_sector_key(m._h, 0x60, 40, key) == -1 and L.nfc_fsm_set_sector_key(m._h, 0x60, -1, key) == -1
    assert L.nfc_fsm_set_sector_key(m._h, 0x62, 0, key) == -1 and L.nfc_fsm_set_sector_key(m._h, 0, 0, key) == -1
    assert L.nfc_fsm_set_sector_key(m._h, 0x61, 39, key) == 0
    bad = _lib.FsmKeyTable()
    bad.present[1][7] = 2
    assert L.nfc_fsm_set_key_table(m._h, C.byref(bad)) == -1 and m.sector_keys() == {(B, 39): bytes(bytearray(K0))}
    s = keyed_state()
    assert L.nfc_host_commands_keyed(C.byref(s), C.byref(bad), None, 0, None, None, None, None, None, None, None, 0, None) == -1
    for call, word in ((lambda: m.set_sector_keys(bad), 'present'), (lambda: m.set_sector_key(A, 40, K0), 'sector'),
                       (lambda: m.set_sector_key(0x62, 0, K0), 'key_type'), (lambda: m.set_sector_keys({(A, 0): K0[:5]}), 'key'),
                       (lambda: fsm.host_commands(s, card(1)[1], sector_keys={(1, 0): K0}), 'key_type')):
        with pytest.raises(ValueError, match=word):
            call()


def test_cur_key_out_of_range_is_rejected():
    m, L = host_machine(), _lib.load()
    for v, ok in ((0, True), (1, True), (2, True), (81, True), (82, False), (-1, False), (1 << 20, False)):
        s = keyed_state()
        s.cur_key = v
        assert (L.nfc_fsm_set_state(m._h, C.byref(s)) == 0) == ok
        assert (L.nfc_host_commands_keyed(C.byref(s), None, None, 0, None, None, None, None, None, None, None, 0, None) == 0) == ok
        if ok:
            assert m.get_state().cur_key == v


def test_key_table_size_matches_the_c_compiler(tmp_path):
    import subprocess
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfc_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(nfc_fsm_key_table), '
                   'offsetof(nfc_fsm_key_table, present), sizeof(nfc_fsm_state)); return 0; }\n')
    exe = tmp_path / 'size'
    include = str(__import__('pathlib').Path(__file__).resolve().parents[1] / 'include')
    subprocess.check_call(['gcc', '-I', include, str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.FsmKeyTable), _lib.FsmKeyTable.present.offset, C.sizeof(_lib.FsmState)] == [560, 480, 88]
    assert _lib.KEY_TABLE_DTYPE.itemsize == 560 and _lib.KEY_TABLE_DTYPE.fields['present'][1] == 480
    t = keys.key_table(TABLE_1)
    rec = np.frombuffer(bytes(bytearray(t)), _lib.KEY_TABLE_DTYPE)[0]
    assert rec['present'][0, 1] == 1 and rec['key'][1, 3].tolist() == K2 and int(rec['present'].sum()) == 3


# ---- 6. sector_table ------------------------------------------------------------------------------------------------------------------
def test_sector_table_keeps_the_lower_block_and_reports_the_other():
    kb = lambda k: bytes(bytearray(k))
    found = {(A, 4): kb(K0), (A, 8): kb(K1), (B, 12): kb(K2), (A, 5): kb(K0)}
    assert keys.sector_table(found) == ({(A, 1): kb(K0), (A, 2): kb(K1), (B, 3): kb(K2)}, {})
    found = {(A, 6): kb(K1), (A, 4): kb(K0), (A, 5): kb(K0), (B, 4): kb(K2), (A, 130): kb(K3), (A, 143): kb(K4)}
    table, conflicts = keys.sector_table(found)
    assert table == {(A, 1): kb(K0), (B, 1): kb(K2), (A, 32): kb(K3)} and conflicts == {(A, 6): kb(K1), (A, 143): kb(K4)}
    assert keys.sector_table({}) == ({}, {})


def test_decode_many_takes_pairs_and_triples_of_keys():
    from usrp_nfc_amd.decoder import _per_source_keys
    ff = [0xFF] * 6
    assert _per_source_keys((K0, K2), 3) == [(K0, K2)] * 3 and _per_source_keys((K0, K2, TABLE_1), 2) == [(K0, K2, TABLE_1)] * 2
    assert _per_source_keys([(K0, K2, TABLE_1), (ff, ff)], 2) == [(K0, K2, TABLE_1), (ff, ff)]
    assert _per_source_keys([(K0, K2), (ff, ff), (K1, K1)], 3) == [(K0, K2), (ff, ff), (K1, K1)]   # three pairs are not a triple
    assert _per_source_keys((np.array(K0), bytes(bytearray(K2))), 1)[0][1] == bytes(bytearray(K2))
    for bad in ([(K0, K2)], (K0, K2, TABLE_1, None), (K0[:5], K2)):
        with pytest.raises(ValueError):
            _per_source_keys(bad, 2)


# ---- 7. the emulator side ---------------------------------------------------------------------------------------------------------------
def test_process_outgoing_keys_its_sectors_from_the_table():
    plain = []
    packets = card_packets(CARD_1, SEEDS_1, plain=plain)
    assert packets == card(1)[0]
    e = fsm.fsm(out=io.StringIO())   # the emulator: the table and the DEFAULT two keys
    e.set_sector_keys(TABLE_1)
    stated_by_hand = 0
    for (t, bits, cmd, machine_out), (_, air) in zip(plain, packets):
        if cmd is None:   # heard, as the generator heard it
            e.process_bits(bits, t)
            continue
        assert e.process_outgoing(bits, CommandType.by_index(cmd)) == machine_out, cmd
        if air != machine_out:   # the nested nonces, which nested_nonce_bits states: a card sends them under the NEW key
            assert cmd == RANDTA and e.get_state().cur_key >= 2
            stated_by_hand += 1
    assert stated_by_hand == 3 and e.get_state().cur_key == 2 + 1 and list(e.get_state().key_a) == [0xFF] * 6
    # without the table the same emulator goes wrong at the second sector
    e = fsm.fsm(out=io.StringIO())
    outs = [e.process_bits(bits, t) if cmd is None else e.process_outgoing(bits, CommandType.by_index(cmd)) for t, bits, cmd, _ in plain]
    assert [o for o, (_, _, cmd, _) in zip(outs, plain) if cmd is not None] != [w for _, _, cmd, w in plain if cmd is not None]


# ---- the condition of the GPU half's recovery test, checked where it is cheap ----------------------------------------------------
def test_card_1_keys_are_unambiguous():
    """Every authentication of card 1 has exactly one verified key (NFC_KEY_OK): keys.host_recover on the first, keys.host_recover_nested
    on the two-candidate window that holds the true nonce of each nested one (half a second per candidate on one core)."""
    _, frames = card(1)
    firsts, nested = keys.find_auths(frames), keys.find_nested_auths(frames)
    assert len(firsts) == 1 and len(nested) == 3
    r, _ = keys.host_recover(firsts)
    assert int(r[0]['status']) == keys.NFC_KEY_OK and r[0]['key'].tolist() == K0 and int(r[0]['n_candidates']) == 1
    nt, n = keys.nested_candidates(nested)
    for i, ((_, _, key), seed) in enumerate(zip(CARD_1[1:], SEEDS_1[1:])):
        at = nt[i][:n[i]].tolist().index(int(extend(seed)))
        first = min(at, int(n[i]) - 2)
        r, _ = keys.host_recover_nested(nested[i:i + 1], cand_first=first, cand_count=2)
        assert int(r[0]['status']) == keys.NFC_KEY_OK and r[0]['key'].tolist() == key and int(r[0]['n_verified']) == 1, i


# ---- 8. the stand-alone program for the sanitizers holds THIS card -----------------------------------------------------------------
def test_sector_keys_check_embeds_card_1():
    """tools/sector_keys_check/main.cpp runs nfc_host_commands_keyed over card 1 under -fsanitize=address,undefined (built and run by
    hand, never through Python: its header says how).  Here only: the frames it embeds are the card's."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'sector_keys_check', 'main.cpp')).read()
    _, frames = card(1)
    for name, want in (('BYTES0', frames.bytes[0]), ('PAR0', frames.par[0]), ('BYTES1', frames.bytes[1]), ('PAR1', frames.par[1])):
        body = re.search(r'static const uint8_t %s\[(\d+)\] = \{(.*?)\};' % name, text, re.S)
        assert int(body.group(1)) == len(want) and [int(v, 16) for v in re.findall(r'0x[0-9A-F]{2}', body.group(2))] == want.tolist(), name
    rows = re.search(r'static const Row ROWS\[(\d+)\] = \{(.*?)\};', text, re.S)
    got = [[int(v, 0) for v in r.split(',')] for r in re.findall(r'\{([^{}]*)\},', rows.group(2))]
    t = frames.table
    assert got == [[int(r[f]) for f in ('idx', 'byte_off', 'n_bits', 'n_bytes', 'flags', 'type')] for r in t] and int(rows.group(1)) == len(t)
    for name, key in (('K0', K0), ('K1', K1), ('K2', K2), ('WRONG', WRONG)):
        assert '%s[6] = {%s}' % (name, ', '.join('0x%02X' % v for v in key)) in text
