"""The emulators on the host (csrc/emu.hip.h behind nfc_host_emu_step and nfc_host_emulate_pairs): no GPU.

Goldens: the reference's own traces outputs/1k_with_enc.out and outputs/ultralight.out (tests/golden/), which its closed loop on
data/classic1k.json / data/ultralight.json (tests/golden/fx_emu_*.json: the two card files, as data) reproduces -- frames 2 to 199 of
the Classic trace (with the seeding REQA: 1 to 199 of 202; the last three are the real reader's repeated HALT and two REQAs) and all 19
of the Ultralight's.  Everything is bit-exact."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

from usrp_nfc_amd import _lib, command, emulate, fsm, keys, synth

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
CT = command.CommandType
REF, CARD = emulate.NFC_EMU_REFERENCE, emulate.NFC_EMU_CARD
PLAIN, AIR = emulate.NFC_EMU_LINK_PLAIN, emulate.NFC_EMU_LINK_AIR


def cards(name, mode):
    return emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_%s.json' % name), mode)


def packets_of(frames):
    """(type, bits) as the framing stage hands them over: a short frame arrives as its seven bits and the end bit"""
    return [(d, bits + [0] if len(bits) == 7 else bits) for d, bits in frames]


def monitor(packets, sector_keys=None):
    """What a monitor with default keys prints and decodes: (text, [(type, command, plain bytes)])"""
    out, seen = io.StringIO(), []
    m = fsm.fsm(out=out)
    if sector_keys:
        m.set_sector_keys(sector_keys)
    for t, bits in packets:
        st = m.process_bits(bits, t)
        seen.append((t, st.name() if st is not None else None, st.all_bytes() if st is not None else None))
    return out.getvalue(), seen


@pytest.fixture(scope='module')
def trace_1k():
    frames, text = synth.frames_from_trace(os.path.join(GOLD, '1k_with_enc.out'))
    assert len(frames) == 202
    mon_text, seen = monitor(packets_of(frames))
    assert mon_text.rstrip('\n') == text.rstrip('\n')   # (tests/test_protocol.py pins this: here it only guards the slicing below)
    return frames, seen


@pytest.fixture(scope='module')
def trace_ul():
    frames, text = synth.frames_from_trace(os.path.join(GOLD, 'ultralight.out'))
    assert len(frames) == 19
    return frames, text


# ---- 1. the PLAIN loop ----
@pytest.mark.parametrize('mode', [REF, CARD])
def test_plain_loop_sends_the_plain_frames_of_the_classic_trace(trace_1k, mode):
    frames, seen = trace_1k
    tag, reader = cards('classic1k', mode)
    T = emulate.pairs_host([tag], [reader], link=PLAIN, rounds=2, cap_frames=512, cap_bytes=4096).transcript(0)
    assert int(T.result['n_frames']) == 398 == len(T) and int(T.result['rounds']) == 2 and int(T.result['flags']) == 0
    for rnd in (0, 1):   # (both rounds: the reader starts over from its first nonce, reader.py:39)
        for i in range(199):
            f = T.frames[199 * rnd + i]
            t, name, data = seen[i]
            assert (int(f['type']), CT.by_index(int(f['cmd'])).name(), T.plain(199 * rnd + i).tolist()) == (t, name, data), (rnd, i)
            assert int(f['round']) == rnd and int(f['flags']) == (emulate._lib.NFC_EMU_FRAME_SEED if i == 0 else 0)
            assert T.air(199 * rnd + i).tolist() == data   # nothing is encrypted
    assert int(T.result['tag_flags']) == 0 and int(T.result['reader_flags']) == 0


@pytest.mark.parametrize('mode', [REF, CARD])
@pytest.mark.parametrize('link', [PLAIN, AIR])
def test_loop_on_the_ultralight_card_is_the_reference_s_trace(trace_ul, mode, link):
    frames, text = trace_ul
    tag, reader = cards('ultralight', mode)
    T = emulate.pairs_host([tag], [reader], link=link, rounds=2).transcript(0)
    assert int(T.result['n_frames']) == 38 and int(T.result['flags']) == 0
    got = synth.transaction_frames(T)
    assert got[:19] == frames and got[19:] == frames
    # 3. a monitor that hears the transcript prints ultralight.out whole
    mon_text, _ = monitor(packets_of(got[:19]))
    assert mon_text.rstrip('\n') == text.rstrip('\n')


# ---- 2. the AIR loop in CARD mode ----
def test_air_loop_card_mode_puts_the_classic_trace_on_the_air(trace_1k):
    frames, seen = trace_1k
    tag, reader = cards('classic1k', CARD)
    T = emulate.pairs_host([tag], [reader], link=AIR, rounds=1).transcript(0)
    assert int(T.result['n_frames']) == 199 == len(T) and int(T.result['flags']) == 0
    got = synth.transaction_frames(T)
    assert got == frames[:199]   # every ciphertext bit and every ninth bit, the fifteen nested {nt} included
    want_text, _ = monitor(packets_of(frames[:199]))
    got_text, _ = monitor(packets_of(got))
    assert got_text == want_text
    assert got_text.count('AR OK') == 16 and got_text.count('AT OK') == 16 and 'ERROR' not in got_text
    golden = open(os.path.join(GOLD, '1k_with_enc.out')).read().replace(' PROCESSING FINISHED\n', ' ')
    assert got_text.rstrip('\n') in golden   # frames 1 to 199 of the printed trace, character for character
    enc = [i for i in range(199) if int(T.frames[i]['flags']) & emulate._lib.NFC_EMU_FRAME_ENCRYPTED]
    assert len(enc) > 150 and enc[0] == 8   # {nr}{ar} of the first authentication is the first encrypted frame
    assert all(int(v) == 0 for v in (T.result['tag_flags'], T.result['reader_flags'], T.result['tag_fsm_flags'], T.result['reader_fsm_flags']))


# ---- 4. the AIR loop in REFERENCE mode ----
def test_air_loop_reference_mode_breaks_at_the_first_nested_nonce(trace_1k):
    frames, seen = trace_1k
    tag, reader = cards('classic1k', REF)
    T = emulate.pairs_host([tag], [reader], link=AIR, rounds=1).transcript(0)
    got = synth.transaction_frames(T)
    # equal to the trace through the first sector and the nested AUTHA; the twentieth frame is the second RANDTA
    assert len(T) == 20 and got[:19] == frames[:19] and CT.by_index(int(T.frames[19]['cmd'])).name() == 'RANDTA'
    assert got[19][0] == frames[19][0] == 0 and got[19][1] != frames[19][1]
    # ... which left under the OLD session's keystream, the quirk of fsm.py:96-99 that fsm.process_outgoing keeps (tests/test_protocol.py)
    emu = fsm.fsm(callback=lambda cmd, st: None, out=io.StringIO())
    for i, (t, bits) in enumerate(packets_of(frames[:19])):
        if t == 1:
            emu.process_bits(bits, t)
        else:
            emu.process_outgoing(synth.frame_bits(seen[i][2]), getattr(CT, seen[i][1]))
    assert emu.process_outgoing(synth.frame_bits(T.plain(19).tolist()), CT.RANDTA) == got[19][1]
    assert T.plain(19).tolist() == seen[19][2]   # (the plain nonce is the card's: only its encryption differs)
    # the reader's machine hears rubbish: a parity error, no answer, the reader stops
    assert int(T.result['reader_flags']) & emulate._lib.NFC_EMU_RAISED and int(T.result['tag_flags']) == 0
    mon_text, _ = monitor(packets_of(got))
    assert mon_text.endswith('PARITY ERROR\n')


# ---- 5. replay of the trace, command by command ----
@pytest.mark.parametrize('mode', [REF, CARD])
def test_replay_tag_and_reader_answer_the_trace_s_next_frame(trace_1k, mode):
    frames, seen = trace_1k
    tag, reader = cards('classic1k', mode)
    for role, card in ((0, tag), (1, reader)):
        st, answered = emulate.state_init(), 0
        for i in range(198):
            t, name, data = seen[i]
            if t == role:   # (its own side's frame: the other side's is what it hears)
                continue
            c = getattr(CT, name)
            extra = data[len(c.header()):len(data) - (2 if c.needs_crc() else 0)]
            cmd, frame = emulate.step(card, st, c.index, extra)
            if name == 'HALT':
                assert cmd is None
                continue
            assert cmd is not None and (CT.by_index(cmd).name(), frame) == (seen[i + 1][1], seen[i + 1][2]), (role, i)
            answered += 1
        assert answered == 99 and st.flags == 0


# ---- the quirks, one by one ----
def _selected_tag(mode, mem=None, rands=((1, 2, 3, 4), (5, 6, 7, 8))):
    mem = emulate.generate_1k() if mem is None else mem
    tag = emulate.tag_card(emulate.CLASSIC1K, mem, rands, mode)
    st = emulate.state_init()
    assert emulate.step(tag, st, CT.REQA.index)[0] == CT.ATQA1K.index
    assert emulate.step(tag, st, CT.ANTI1R.index) == (CT.ANTI1G.index, list(mem[:5]))
    assert emulate.step(tag, st, CT.SEL1R.index, mem[:5])[0] == CT.SEL1K.index and st.selected == 1
    return tag, st


def _access(c1, c2, c3):
    """the four access bytes of a trailer: nibble cX bit i is CX of block i"""
    return [((~c2 & 0xF) << 4) | (~c1 & 0xF), (c1 << 4) | (~c3 & 0xF), (c3 << 4) | c2, 0x69]


def _card_memory(seed, data_conds, trailer_conds):
    """1024 random bytes with sixteen distinct key pairs; block b of a sector has condition (C1 C2 C3 as a number) data_conds / trailer_conds [sector]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    mem = rng.integers(0, 256, 1024).astype(np.uint8)
    mem[4] = mem[0] ^ mem[1] ^ mem[2] ^ mem[3]   # BCC
    for s in range(16):
        conds = [data_conds[s][0], data_conds[s][1], data_conds[s][2], trailer_conds[s]]
        c1 = sum(((c >> 2) & 1) << i for i, c in enumerate(conds))
        c2 = sum(((c >> 1) & 1) << i for i, c in enumerate(conds))
        c3 = sum((c & 1) << i for i, c in enumerate(conds))
        mem[(4 * s + 3) * 16 + 6:(4 * s + 3) * 16 + 10] = _access(c1, c2, c3)
    return mem


def test_authb_is_served_with_key_a_in_reference_mode_and_with_key_b_in_card_mode():
    for mode, want in ((REF, 1), (CARD, 2)):
        tag, st = _selected_tag(mode)
        cmd, frame = emulate.step(tag, st, CT.AUTHB.index, [0x04])
        assert cmd == CT.RANDTA.index and frame == [1, 2, 3, 4] and st.auth_key == want and st.auth_prosp == 4 and st.auth == -1
        cmd, frame = emulate.step(tag, st, CT.RANDRB.index, [0] * 8)   # (the reader's answer is not checked, tag.py:367-370)
        assert cmd == CT.RANDTB.index and st.auth == 4 and frame == list(bytearray(st.at))
        assert st.rand_idx == 1


def test_key_b_conditions_apply_in_card_mode_only():
    # data condition 3 (C1 C2 C3 = 011): read with key B alone
    mem = _card_memory(3, [[3, 0, 0]] * 16, [1] * 16)
    for mode, auth, want in ((REF, CT.AUTHB, None), (CARD, CT.AUTHB, CT.READT.index), (CARD, CT.AUTHA, None)):
        tag, st = _selected_tag(mode, mem)
        emulate.step(tag, st, auth.index, [0x08])
        emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
        cmd, frame = emulate.step(tag, st, CT.READR.index, [0x08])
        assert cmd == want
        if want is not None:
            assert frame[:16] == mem[128:144].tolist() and frame[16:] == fsm.crc_a(frame[:16])
        assert emulate.step(tag, st, CT.READR.index, [0x09])[0] == CT.READT.index   # (condition 0: either key)
        assert emulate.step(tag, st, CT.READR.index, [0x0C])[0] is None                # another sector


def test_reference_mode_reads_the_access_bytes_at_the_auth_s_block_number():
    # tag.py:194-197,225-229: bytes 16 * block + 54.  An AUTH on a sector's SECOND block finds data bytes there, not the trailer's
    mem = _card_memory(5, [[0, 0, 0]] * 16, [1] * 16)
    mem[5 * 16 + 54:5 * 16 + 58] = _access(0xF, 0xF, 0xF)   # block 8, bytes 6 .. 9: condition 7 for every block -- never readable
    for mode, want in ((REF, None), (CARD, CT.READT.index)):
        tag, st = _selected_tag(mode, mem)
        emulate.step(tag, st, CT.AUTHA.index, [0x05])
        emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
        assert emulate.step(tag, st, CT.READR.index, [0x04])[0] == want
    # ... and one on block 61 .. 63 behind the memory's end: the reference raises
    tag, st = _selected_tag(REF, mem)
    emulate.step(tag, st, CT.AUTHA.index, [0x3D])
    emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
    assert emulate.step(tag, st, CT.READR.index, [0x3C])[0] is None and st.flags & _lib.NFC_EMU_RAISED


def test_trailer_reads_are_masked_and_broken_complements_are_flagged():
    mem = _card_memory(9, [[0, 0, 0]] * 16, [1] * 8 + [4] * 8)
    tag, st = _selected_tag(CARD, mem)
    for sector, shown_b in ((2, True), (12, False)):
        emulate.step(tag, st, CT.AUTHA.index, [4 * sector])
        emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
        cmd, frame = emulate.step(tag, st, CT.READR.index, [4 * sector + 3])
        t = mem[(4 * sector + 3) * 16:(4 * sector + 4) * 16].tolist()
        assert cmd == CT.READT.index and frame[:16] == [0] * 6 + t[6:10] + (t[10:] if shown_b else [0] * 6)
    assert st.flags == 0
    mem[3 * 16 + 6] ^= 0x01   # the complement of C1, block 0, of sector 0
    tag, st = _selected_tag(CARD, mem)
    emulate.step(tag, st, CT.AUTHA.index, [0])
    emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
    emulate.step(tag, st, CT.READR.index, [1])
    assert st.flags == _lib.NFC_EMU_ERR_ONES


def test_malformed_reader_scripts():
    mem = _card_memory(11, [[0, 0, 0]] * 16, [1] * 16)
    tag, st = _selected_tag(CARD, mem)
    assert emulate.step(tag, st, CT.READR.index, [0x01])[0] is None                      # no authentication yet
    assert emulate.step(tag, st, CT.RANDRB.index, [0] * 8)[0] is None and st.flags == _lib.NFC_EMU_RAISED   # RANDRB before any AUTH
    st.flags = 0
    assert emulate.step(tag, st, CT.SEL1R.index, [1, 2, 3, 4, 4])[0] is None             # SEL with a wrong UID: no answer, still selected
    assert emulate.step(tag, st, CT.WUPA.index)[0] == CT.ATQA1K.index and st.selected == 0   # WUPA in a session
    assert emulate.step(tag, st, CT.AUTHA.index, [0])[0] is None                         # not selected any more
    tag, st = _selected_tag(CARD, mem)
    assert emulate.step(tag, st, CT.HALT.index)[0] is None and st.halted == 1
    assert emulate.step(tag, st, CT.REQA.index)[0] is None                               # frames after HALT
    assert emulate.step(tag, st, CT.WUPA.index)[0] == CT.ATQA1K.index
    assert emulate.step(tag, st, -1, [1, 2, 3])[0] is None and st.flags == _lib.NFC_EMU_RAISED   # a frame the machine does not know
    assert emulate.step(tag, st, CT.ATQA1K.index)[0] is None                             # a tag's own direction: ignored silently


def test_reader_sends_halt_to_what_it_does_not_expect_and_flags_it():
    reader = emulate.reader_card([[9, 9, 9, 9]])
    st = emulate.state_init()
    assert emulate.step(reader, st, CT.ATQA1K.index)[0] == CT.ANTI1R.index and st.tag_type == 1
    cmd, frame = emulate.step(reader, st, CT.ANTI1G.index, [1, 2, 3, 4, 4])
    assert cmd == CT.SEL1R.index and frame[:7] == [0x93, 0x70, 1, 2, 3, 4, 4] and st.uid_len == 4
    assert emulate.step(reader, st, CT.COMPW2.index, [0] * 16)[0] is None and st.flags == 0   # a reader's own direction: ignored silently
    cmd, frame = emulate.step(reader, st, CT.ATQA4K.index)                                    # reader.py:75-78: a 4K is not read
    assert cmd == CT.HALT.index and frame == [0x50, 0x00, 0x57, 0xCD]
    assert st.uid_len == 0 and st.tag_type == -1 and st.rand_idx == 0 and st.flags == 0   # reader.py:45-46: HALT forgets the tag
    # eight UID bytes, then a nonce: more UID bits than nonce bits -- the reference raises
    for _ in range(2):
        emulate.step(reader, st, CT.ANTI1G.index, [1, 2, 3, 4, 4])
    assert st.uid_len == 8
    assert emulate.step(reader, st, CT.RANDTA.index, [1, 2, 3, 4])[0] is None and st.flags == _lib.NFC_EMU_RAISED
    for _ in range(7):
        emulate.step(reader, st, CT.ANTI1G.index, [1, 2, 3, 4, 4])
    assert st.uid_len == 32 and st.flags & _lib.NFC_EMU_UID_OVERFLOW


# ---- 7. / 8. sixteen key pairs, mixed access bits ----
@pytest.fixture(scope='module')
def keyed_card():
    data_conds = [[[0, 1, 2, 4, 6][(s + b) % 5] for b in range(3)] for s in range(16)]   # every condition key A may read under
    trailer_conds = [s % 8 for s in range(16)]                                            # all eight
    mem = _card_memory(21, data_conds, trailer_conds)
    rng = np.random.Generator(np.random.PCG64(22))
    tag = emulate.tag_card(emulate.CLASSIC1K, mem, rng.integers(0, 256, (16, 4)), CARD)
    table = {(0x60, s): bytes(mem[(4 * s + 3) * 16:(4 * s + 3) * 16 + 6].tolist()) for s in range(16)}
    reader = emulate.reader_card(rng.integers(0, 256, (5, 4)), key_a=[1, 2, 3, 4, 5, 6], table=table, mode=CARD)
    T = emulate.pairs_host([tag], [reader], link=AIR, rounds=1).transcript(0)
    return mem, table, trailer_conds, T


def test_card_with_sixteen_key_pairs_is_read_whole_and_decrypts_with_the_sector_table(keyed_card):
    mem, table, trailer_conds, T = keyed_card
    assert len({bytes(mem[(4 * s + 3) * 16:(4 * s + 3) * 16 + 6]) for s in range(16)}) == 16
    assert int(T.result['n_frames']) == 199 == len(T) and int(T.result['tag_flags']) == 0 and int(T.result['reader_flags']) == 0
    found = {(0x60, 4 * s): k for (_, s), k in table.items()}   # as a key recovery reports them: by block
    sector_keys, conflicts = keys.sector_table(found)
    assert not conflicts
    recs, data, enc = fsm.host_commands(fsm.state_init(), T.nfc_frames(), sector_keys=sector_keys)
    reads, asked = [], None
    for r in recs:
        name = CT.by_index(int(r['cmd'])).name() if int(r['cmd']) >= 0 else None
        body = data[int(r['byte_off']):int(r['byte_off']) + int(r['n_bytes'])].tolist()
        if name == 'READR':
            asked = body[1]
        elif name == 'READT':
            reads.append((asked, body[:16]))
    assert [b for b, _ in reads] == list(range(63, -1, -1))
    for block, got in reads:
        want = mem[16 * block:16 * block + 16].tolist()
        if block % 4 == 3:   # key A is never shown, key B where the condition lets key A read it
            want = [0] * 6 + want[6:10] + (want[10:] if trailer_conds[block // 4] <= 2 else [0] * 6)
        assert got == want, block
    assert sum(1 for r in recs if int(r['flags']) & fsm.FRAME_AR_OK) == 16 and sum(1 for r in recs if int(r['flags']) & fsm.FRAME_AT_OK) == 16
    # with the two default keys alone the monitor is lost at the first nonce
    recs2, _, _ = fsm.host_commands(fsm.state_init(), T.nfc_frames())
    assert not any(int(r['flags']) & fsm.FRAME_AR_OK for r in recs2)


def test_key_recovery_finds_the_first_key_of_an_emulated_card(keyed_card):
    mem, table, _, T = keyed_card
    traces = keys.find_auths(T.nfc_frames())
    assert len(traces) == 1 and int(traces[0]['block']) == 0x3C and int(traces[0]['key_type']) == 0x60
    res, _ = keys.host_recover(traces)
    assert int(res[0]['status']) == keys.NFC_KEY_OK and bytes(res[0]['key'].tolist()) == table[(0x60, 15)]


# ---- 9. state hand-over ----
def test_state_taken_mid_authentication_continues_identically():
    mem = _card_memory(31, [[0, 0, 0]] * 16, [1] * 16)
    tag, st = _selected_tag(CARD, mem)
    emulate.step(tag, st, CT.AUTHA.index, [0x10])
    fresh = emulate.state_init()
    C.memmove(C.byref(fresh), C.byref(st), C.sizeof(st))
    script = [(CT.RANDRB, [0] * 8), (CT.READR, [0x11]), (CT.READR, [0x13]), (CT.AUTHB, [0x20]), (CT.RANDRB, [1] * 8), (CT.READR, [0x21]), (CT.HALT, [])]
    for c, extra in script:
        assert emulate.step(tag, st, c.index, extra) == emulate.step(tag, fresh, c.index, extra)
        assert bytes(st) == bytes(fresh)
    assert st.halted == 1 and st.rand_idx == 0   # (two nonces, handed out in turn and from the first again)


# ---- 10. error paths ----
def test_argument_errors_name_the_argument():
    good_mem, rands = emulate.generate_1k(), [[1, 2, 3, 4]]
    reader = emulate.reader_card(rands)
    cases = [
        (emulate.tag_card(emulate.CLASSIC1K, good_mem[:1000], rands), reader, {}, 'tags[0].mem'),
        (emulate.tag_card(emulate.ULTRALIGHT, good_mem, None), reader, {}, 'tags[0].mem'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, None), reader, {}, 'tags[0].rands'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, [[1, 2, 3, 4]] * 65), reader, {}, 'tags[0].rands'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands), emulate.reader_card(None), {}, 'readers[0].rands'),
        (emulate.tag_card(2, good_mem, rands), reader, {}, 'tags[0].tag_type'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands, mode=2), reader, {}, 'tags[0].mode'),
        (reader, reader, {}, 'tags[0].role'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands), reader, dict(rounds=0), 'cfg.rounds'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands), reader, dict(rounds=65), 'cfg.rounds'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands), reader, dict(link=2), 'cfg.link'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands), reader, dict(cap_frames=0), 'cfg.cap_frames'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands), reader, dict(cap_bytes=0), 'cfg.cap_bytes'),
        (emulate.tag_card(emulate.CLASSIC1K, good_mem, rands), reader, dict(pair_cap_frames=[0]), 'cfg.pair_cap_frames[0]'),
    ]
    for tag, rd, kw, name in cases:
        for call in (emulate.pairs_host, emulate.pairs_device):   # (the device call checks before it touches a device: no GPU is needed to fail)
            with pytest.raises(ValueError, match=name.replace('[', r'\[').replace(']', r'\]').replace('.', r'\.')):
                call([tag], [rd], **kw)
    st = emulate.state_init()
    st.rand_idx = 64
    with pytest.raises(ValueError, match='rand_idx'):
        emulate.step(reader, st, CT.ATQA1K.index)
    with pytest.raises(ValueError, match='extra'):
        emulate.step(reader, emulate.state_init(), CT.ATQA1K.index, [0] * 19)
    with pytest.raises(ValueError, match='cmd'):
        emulate.step(reader, emulate.state_init(), 27)
    assert emulate.pairs_host([], []).results.size == 0


def test_a_slab_that_is_outgrown_keeps_true_counts():
    tag, reader = cards('classic1k', CARD)
    whole = emulate.pairs_host([tag], [reader], rounds=1).transcript(0)
    for kw, flag in ((dict(cap_frames=20), _lib.NFC_EMU_PAIR_CUT_FRAMES), (dict(cap_bytes=100), _lib.NFC_EMU_PAIR_CUT_BYTES),
                     (dict(pair_cap_frames=[20]), _lib.NFC_EMU_PAIR_CUT_FRAMES)):
        T = emulate.pairs_host([tag], [reader], rounds=1, **kw).transcript(0)
        assert int(T.result['n_frames']) == 199 and int(T.result['n_bytes']) == int(whole.result['n_bytes']) and int(T.result['flags']) == flag
        assert 0 < len(T) <= 20 and synth.transaction_frames(T) == synth.transaction_frames(whole)[:len(T)]


def test_names_are_declared_and_bound():
    names = ['nfc_emu_state_init', 'nfc_emu_last_error', 'nfc_host_emu_step', 'nfc_host_emulate_pairs', 'nfc_emulate_pairs_device']
    header = open(os.path.join(os.path.dirname(GOLD), '..', 'include', 'nfc_amd.h')).read()
    assert set(names) <= set(_lib.SYMBOLS) and all(n + '(' in header for n in names)
    assert C.sizeof(_lib.EmuState) == 88 and C.sizeof(_lib.EmuCard) == 64 and C.sizeof(_lib.EmuConfig) == 32
    assert _lib.EMU_FRAME_DTYPE.itemsize == 16 and _lib.EMU_RESULT_DTYPE.itemsize == 32


# ---- 11. the reference-named objects ----
def test_reference_named_objects_keep_the_reference_s_signatures():
    import inspect
    from usrp_nfc_amd import parser, rand, reader, tag
    def positional(f):   # what can be passed by position: exactly the reference's parameters (anything more is keyword-only)
        return [n for n, p in inspect.signature(f).parameters.items() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
    assert positional(tag.Tag.__init__) == ['self', 'callback', 'tag_type', 'memory', 'rands']
    assert positional(reader.Reader.__init__) == ['self', 'callback', 'rands', 'keya', 'keyb']
    assert positional(parser.Parser.__init__) == ['self', 'name'] and positional(parser.Parser.get_tag) == positional(parser.Parser.get_reader) == ['self', 'callback']
    assert positional(reader.Reader.process_packet) == ['self', 'cmd', 'struct'] and positional(tag.Tag.set_encoder) == ['self', 'encode']
    assert positional(rand.Rand.__init__) == ['self', 'rands']
    assert list(inspect.signature(tag.Tag.process_packet).parameters) == ['self', 'cmd', 'struct']
    assert list(inspect.signature(command.CommandStructure.encode_command).parameters) == ['cmd', 'bytes']
    for name in ('process_packet', 'set_encoder', 'wake_up', 'generate_1k', 'get_keys_from_mem'):
        assert callable(getattr(tag.Tag, name))
    mem = tag.Tag.generate_1k()
    assert len(mem) == 1024 and tag.Tag.get_keys_from_mem(mem) == ([0xFF] * 6, [0xFF] * 6) and mem == emulate.cards_from_json([])[0].mem.tolist()
    r = rand.Rand([[1, 2, 3, 4], [5, 6, 7, 8]])
    assert [r.get_next(), r.get_next(), r.get_next()] == [[1, 2, 3, 4], [5, 6, 7, 8], [1, 2, 3, 4]]
    r.reset()
    assert r.get_next() == [1, 2, 3, 4]
    assert rand.Rand(None).rands() == rand.Rand(None).rands() and len(rand.Rand(None).rands()) == 16   # drawn once, from a fixed seed
    st = command.CommandStructure.encode_command(CT.SEL1R, [0x88, 0x04, 0xBE, 0x6F, 0x5D])
    assert (st.name(), st.header(), st.crc()) == ('SEL1R', [0x93, 0x70], [0xA1, 0x8E])
    assert command.CommandStructure.encode_command(CT.REQA, []).all_bytes() == [0x26]
    assert command.CommandStructure.encode_command(None, [1, 2]).name() == 'UNKNOWN'
    p = parser.Parser(os.path.join(GOLD, 'fx_emu_classic1k.json'))
    assert isinstance(p.get_tag(None, out=io.StringIO()), tag.Tag) and isinstance(p.get_reader(None, out=io.StringIO()), reader.Reader)


@pytest.mark.parametrize('role', [0, 1])
def test_objects_behind_their_fsm_replay_the_trace(trace_1k, role):
    # decoder-less wiring, as background.py does it: fsm.fsm(emulator.process_packet) hears, emulator.set_encoder(fsm.process_outgoing)
    # sends.  The trace's frames of the OTHER side are played to it; what it puts on the air is the trace's next frame -- in the tag's
    # role but for the fifteen nested tag nonces, which the reference's hook sends under the old keystream (fsm.py:96-99)
    from usrp_nfc_amd import parser
    frames, seen = trace_1k
    sent, text = [], io.StringIO()
    p = parser.Parser(os.path.join(GOLD, 'fx_emu_classic1k.json'))
    emu = p.get_tag(lambda bits: sent.append(bits), out=text) if role == 0 else p.get_reader(lambda bits, finished: sent.append(bits), out=text)
    m = fsm.fsm(emu.process_packet, out=io.StringIO())
    emu.set_encoder(m.process_outgoing)
    answers, differ = 0, []
    for i, (t, bits) in enumerate(packets_of(frames[:199])):
        if t == role:
            continue
        n0 = len(sent)
        m.process_bits(bits, t)
        if seen[i][1] == 'HALT':
            assert len(sent) == n0
            continue
        assert len(sent) == n0 + 1, i
        answers += 1
        if sent[-1] != frames[i + 1][1]:
            differ.append(seen[i + 1][1])
    if role == 1:
        assert answers == 99 and not differ and emu.flags() == 0
        assert text.getvalue().count('READER OUTGOING') == 99 and text.getvalue().count('READER INCOMING') == 99
    else:   # (its machine keys the new session from the PLAIN nonce, so it stays in step: only what went on the air differs)
        assert answers == 99 and differ == ['RANDTA'] * 15 and emu.flags() == 0
        assert text.getvalue().count('TAG OUTGOING') == 99 and text.getvalue().count('INCOMING') == 100


# ---- 5. replay through the twin: a machine that hears one side answers as the other ----
def _heard(frames, role):
    """the frames a stream that decodes only the other side hears, and for each the trace's next frame (None behind the HALT)"""
    idx = [i for i in range(199) if frames[i][0] != role]
    return emulate.frames_of_bits([frames[i] for i in idx]), [frames[i + 1][1] if i + 1 < 199 and frames[i + 1][0] == role else None for i in idx]


@pytest.mark.parametrize('mode', [REF, CARD])
@pytest.mark.parametrize('role', [0, 1])
def test_replay_twin_answers_the_trace(trace_1k, role, mode):
    frames, seen = trace_1k
    card = cards('classic1k', mode)[role]
    heard, nxt = _heard(frames, role)
    est, st = emulate.state_init(), fsm.state_init()
    (recs, data, enc), ans = emulate.host_emulate(card, est, st, heard)
    assert len(recs) == (100 if role == 0 else 99) and len(ans) == 99 and est.flags == 0
    differ = [CT.by_index(int(r['cmd'])).name() for i, r in enumerate(ans.records) if ans.bits(i) != nxt[int(r['src'])]]
    # a tag in REFERENCE mode sends its fifteen nested nonces under the old keystream (fsm.py:96-99); everything else is the trace's
    assert differ == (['RANDTA'] * 15 if (role, mode) == (0, REF) else [])
    assert [CT.by_index(int(r['cmd'])).name() for r in recs] == [seen[i][1] for i in range(199) if frames[i][0] != role]   # the machine stayed in step
    if (role, mode) == (0, REF):   # ... and those fifteen are what the reference-named objects put on the air
        from usrp_nfc_amd import parser
        sent = []
        emu = parser.Parser(os.path.join(GOLD, 'fx_emu_classic1k.json')).get_tag(lambda bits: sent.append(bits), out=io.StringIO())
        m = fsm.fsm(emu.process_packet, out=io.StringIO())
        emu.set_encoder(m.process_outgoing)
        for t, bits in packets_of([f for f in frames[:199] if f[0] == 1]):
            m.process_bits(bits, t)
        assert sent == [ans.bits(i) for i in range(99)]


@pytest.mark.parametrize('role', [0, 1])
def test_replay_twin_in_pieces_continues_identically(trace_1k, role):
    frames, _ = trace_1k
    card = cards('classic1k', CARD)[role]
    heard, _ = _heard(frames, role)
    _, whole = emulate.host_emulate(card, emulate.state_init(), fsm.state_init(), heard)
    want = [whole.bits(i) for i in range(len(whole))]
    t = heard.table
    # cut between an AUTH and its nonce, between {nr}{ar} and {at}, and in the middle of the nested part
    for cut in (4, 5, 9, 30):
        est, st, got = emulate.state_init(), fsm.state_init(), []
        for part in (t[:cut], t[cut:]):
            _, a = emulate.host_emulate(card, est, st, part, heard.bytes, heard.par)
            got += [a.bits(i) for i in range(len(a))]
        assert got == want, cut


# ---- 6. the recorded reference: tests/golden/emu_reference.npz (make_emu_golden.py drove the reference's own Tag / Reader) ----
@pytest.fixture(scope='module')
def fx_emu():
    with np.load(os.path.join(GOLD, 'emu_reference.npz')) as z:   # (every array once: an NpzFile reads a member again at every access)
        return {k: z[k] for k in z.files}


def _recorded_bits(fx, key):
    bits, off = np.unpackbits(fx[key]), fx[key + '_off']
    return [bits[int(off[i]):int(off[i + 1])].tolist() for i in range(len(off) - 1)], fx[key + '_src'].tolist()


def test_fuzz_rows_twin_against_the_recorded_reference(fx_emu):
    from tests import emu_cards
    fx = fx_emu
    assert len(fx['row_role']) == emu_cards.N_TAG_ROWS + emu_cards.N_READER_ROWS
    prints = {1: _lib.NFC_EMU_ERR_ONES, 2: _lib.NFC_EMU_ERR_TWOS, 4: _lib.NFC_EMU_ERR_THREES, 8: _lib.NFC_EMU_UNEXPECTED}
    n_steps = n_raised = 0
    for r in range(len(fx['row_role'])):
        role, seed, raised = int(fx['row_role'][r]), int(fx['row_seed'][r]), int(fx['row_raise'][r])
        if role == 0:
            tag_type, mem, rands, steps = emu_cards.tag_row(seed)
            card = emulate.tag_card(tag_type, mem, rands or None, REF)
        else:
            rands, steps = emu_cards.reader_row(seed)
            card = emulate.reader_card(rands, mode=REF)
        st, s0 = emulate.state_init(), int(fx['step_off'][r])
        assert int(fx['step_off'][r + 1]) - s0 == (raised if raised >= 0 else len(steps))
        for k, (name, extra) in enumerate(steps):
            before = int(st.flags)
            cmd, frame = emulate.step(card, st, getattr(CT, name).index if name else -1, extra)
            new = int(st.flags) & ~before
            if k == raised:   # where the reference raises: no answer, the flag; the row ends
                assert cmd is None and new & _lib.NFC_EMU_RAISED, (r, k)
                n_raised += 1
                break
            a = s0 + k
            want = int(fx['ans_cmd'][a])
            assert (cmd if cmd is not None else -1) == want, (r, k, name, extra)
            assert frame == fx['ans_bytes'][int(fx['ans_off'][a]):int(fx['ans_off'][a + 1])].tolist(), (r, k)
            assert not int(st.flags) & _lib.NFC_EMU_RAISED, (r, k)
            for bit, flag in prints.items():   # a print of the reference is a flag here (sticky: a flag set earlier stays)
                if int(fx['step_print'][a]) & bit:
                    assert int(st.flags) & flag, (r, k)
                else:
                    assert not new & flag, (r, k)
            n_steps += 1
    assert n_steps == len(fx['ans_cmd']) and n_raised == int((fx['row_raise'] >= 0).sum()) > 50


@pytest.mark.parametrize('name,key,n', [('classic1k', 'loop_text_1k', 398), ('ultralight', 'loop_text_ul', 38)])
def test_plain_loop_prints_the_recorded_reference_text(fx_emu, name, key, n):
    # 1. emulate.run (usrp_nfc.py:116-136) over the reference-named objects, two rounds: the reference's printed text, and the PLAIN loop of
    # the twin sends exactly the frames that text shows going out
    from usrp_nfc_amd import parser
    want = bytes(fx_emu[key]).decode('utf-8')
    out = io.StringIO()
    p = parser.Parser(os.path.join(GOLD, 'fx_emu_%s.json' % name))
    tag, reader = p.get_tag(lambda bits: None, out=out), p.get_reader(lambda bits, finished=False: None, out=out)
    cmd = CT.REQA
    struct = command.CommandStructure.encode_command(cmd, [])
    s, ns, i = tag, reader, 0
    while i < 2:
        ret = s.process_packet(cmd, struct)
        if not ret:
            cmd = CT.REQA
            struct = command.CommandStructure.encode_command(cmd, [])
            s, ns = tag, reader
            s.wake_up()
            i += 1
        else:
            (cmd, struct), s, ns = ret, ns, s
    assert out.getvalue() == want
    T = emulate.pairs_host(list(emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_%s.json' % name), REF)[:1]),
                           [emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_%s.json' % name), REF)[1]], link=PLAIN, rounds=2, cap_frames=512,
                           cap_bytes=4096).transcript(0)
    assert len(T) == n
    sent = [blk.split('\n\n\n')[0] for blk in want.split('OUTGOING\n')[1:]]
    seeds = 0
    for i in range(n):
        if int(T.frames[i]['flags']) & _lib.NFC_EMU_FRAME_SEED:
            seeds += 1
            continue
        c = CT.by_index(int(T.frames[i]['cmd']))
        d = T.plain(i).tolist()
        n_crc = 2 if c.needs_crc() else 0
        st = command.CommandStructure(c.name(), d[:len(c.header())], d[len(c.header()):len(d) - n_crc], d[len(d) - n_crc:])
        assert st.text().rstrip('\n') == sent[i - seeds].rstrip('\n'), i
    assert seeds == 2 and len(sent) == n - 2


@pytest.mark.parametrize('role,key', [(0, 'replay_tag'), (1, 'replay_reader')])
def test_replay_in_reference_mode_is_the_recorded_reference(fx_emu, trace_1k, role, key):
    # 5. / 4. what the reference's Tag / Reader behind its fsm put on the air for the replayed trace: the twin's answers in REFERENCE mode, bit
    # for bit -- the fifteen nested tag nonces under the old keystream included -- and the frame at which the AIR loop breaks
    frames, _ = trace_1k
    want, src = _recorded_bits(fx_emu, key)
    assert len(want) == 99
    heard_idx = [i for i in range(199) if frames[i][0] != role]
    heard, nxt = _heard(frames, role)
    _, ans = emulate.host_emulate(cards('classic1k', REF)[role], emulate.state_init(), fsm.state_init(), heard)
    assert [heard_idx[int(r['src'])] for r in ans.records] == src
    assert [ans.bits(i) for i in range(len(ans))] == want
    differ = [i for i in range(99) if want[i] != nxt[int(ans.records[i]['src'])]]
    assert len(differ) == (15 if role == 0 else 0)
    if role == 0:
        T = emulate.pairs_host(*[[c] for c in cards('classic1k', REF)], link=AIR, rounds=1).transcript(0)
        assert T.bits(19) == want[src.index(18)] and differ[0] == src.index(18)


def test_create_json_writes_card_files_the_parser_reads(tmp_path, trace_ul):
    from usrp_nfc_amd import create_json, parser, tag
    paths = create_json.write(str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ['classic1k.json', 'ultralight.json']
    ref_1k = json.load(open(os.path.join(GOLD, 'fx_emu_classic1k.json')))
    ref_ul = json.load(open(os.path.join(GOLD, 'fx_emu_ultralight.json')))
    got_1k, got_ul = json.load(open(paths[0])), json.load(open(paths[1]))
    assert got_ul == ref_ul                                      # the Ultralight file is the reference's, entry for entry
    assert [sorted(d) for d in got_1k] == [sorted(d) for d in ref_1k] and got_1k[0]['mem'] == ref_1k[0]['mem'] == tag.Tag.generate_1k()
    assert [np.shape(d['rands']) for d in got_1k] == [np.shape(d['rands']) for d in ref_1k] == [(16, 4), (16, 4)]   # (the nonces are drawn here)
    frames, _ = trace_ul
    t, r = emulate.cards_from_json(paths[1])
    assert synth.transaction_frames(emulate.pairs_host([t], [r], link=AIR).transcript(0)) == frames
    t, r = emulate.cards_from_json(paths[0])
    res = emulate.pairs_host([t], [r], link=AIR).results[0]
    assert int(res['n_frames']) == 199 and int(res['flags']) == 0
    assert isinstance(parser.Parser(paths[0]).get_tag(None, out=io.StringIO()), tag.Tag)
