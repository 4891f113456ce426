"""The emulators on the GPU where only their CPU twin was tested (csrc/emu.hip.h in k_emulate_pairs, csrc/nfc_emu.hip, and in
k_multi_commands_emu, csrc/multi_commands.hip.h).  tests/test_emulate_host.py pins the twin to the reference in depth; the
kernels have their own text for the cards (DevCard, DevReader), the tables (skeys::DeviceTable, TrailerTable<DevCard>), the transposed
images and the per-lane slabs, and tests/test_emulate.py shows them well-formed cards and clean traffic only.

TWO HALVES, as tests/test_second_trips.py: the CPU half asserts on the twin that every input reaches the behaviour it is there for -- each
flag in its lane, the nonce index past 64, the shares of sessions that survive a mutation -- so a later change to a generator turns a
test red instead of emptying it; the GPU half pins the kernels to the twin.  Every comparison is for byte equality.  Everything is made
from seeds.

1. PAIRS: one call of K = 193 pairs (four workgroups, the last with one live lane) per link, the catalogue below between the mixed pairs
   of tests/test_emulate.py so that neighbours differ in card kind, mode and behaviour.  Nine rounds: five take the nonce index of a tag
   with 64 nonces past 64 (a whole card is 16 authentications; the count is the twin's), nine fill a reader's 32 UID bytes.
   WHAT THE CLOSED LOOP CANNOT REACH: reader_step only ever sends AUTHA, and only on a sector's FIRST block.  So no lane of k_emulate_pairs
   serves an AUTHB, reads under key B, or finds other access bytes in REFERENCE mode than in CARD mode (16 * block + 54 of a first block
   IS its trailer's); the lanes for those entries are there and are shown NOT to differ by mode.  The streams of part 3 hear AUTHB.
   NFC_EMU_PAIR_RUNAWAY is left out: every answer of reader_step either moves a counter that only moves one way (cur_addr down to 0 for a
   Classic, up to 0x0C for an Ultralight; the anticollision has no way back) or is a HALT, which a tag never answers, so a round is 199
   frames at the most and ROUND_STEPS = 1024 is out of reach for every card card_fault admits.
   cap_bytes is per call and the nine rounds need 16 000 of it, so NFC_EMU_PAIR_CUT_BYTES has a small call of its own.
2. STREAMS that answer, keyed per sector, on mutated sessions: the traffic is one side of the emulators' own closed loop over 32 pairs of
   tests/test_emulate.py's _pair(), 40 frames at the most, with 0 to 3 seeded mutations in the second half of the frames, rendered to
   IQ; 132 streams in one tracked context, the role by lane (Classic tag, Ultralight tag, reader, no card), every stream that holds or
   hears a Classic card keyed from its trailers.  One push, three ragged pushes, a hand-off into the mirrored slots of a second context.
   THE SHARE OF SESSIONS THAT SURVIVE is held up by drawing again, not by placement alone: see stream_specs().
3. The fuzz fixture of tests/test_fsm_fuzz.py through six kinds of card.
4. The streams of part 2 with a bit slab they outgrow: a push that ends in cut frames stores the emulator all the same.

THE COUNTS the CPU half measured (they are computed, and where they are literals below the CPU half holds them against the twin):
pairs, PLAIN / AIR, of 193 lanes: NFC_EMU_RAISED in 133 / 142, NFC_EMU_ERR_ONES in 4 / 2, NFC_EMU_UID_OVERFLOW in 133 / 0.  Most of the mixed pairs
have a block key A may not read: the tag's silence ends the round, the reader keeps its UID (it forgets the tag only when it sends HALT),
refuses the nonce from the second round on and has 32 UID bytes after eight.  On the AIR link a tag whose machine is left inside a
session hears every later REQA as ciphertext, so no round behind the broken one gets as far as the UID.
Streams (STREAM_COUNTS): 955 answers, 401 of them in cipher, 99 of 132 streams answering, NFC_EMU_RAISED in 39; of the 58 keyed Classic
streams 19 are clean and all bring a session up, 39 are mutated and 26 answer in cipher behind their first mutated frame.
Fixture (FIXTURE_COUNTS, FIXTURE_BY_KIND): 978 answers, 112 in cipher (111 of them a reader's), 253 of 256 streams answering, NFC_EMU_RAISED in 234."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.golden_util import GOLDEN
from tests.test_commands import PIECES, concatenated
from tests.test_commands_host import state_bytes
from tests.test_emulate import _access, _pair
from tests.test_emulate_host import _card_memory, _selected_tag
from tests.test_fsm_fuzz import fixture, frames_of, full_table, gpu_one_push, gpu_streams, tracked
from usrp_nfc_amd import _lib, api, command, emulate, fsm, synth

CT = command.CommandType
REF, CARD = emulate.NFC_EMU_REFERENCE, emulate.NFC_EMU_CARD
PLAIN, AIR = emulate.NFC_EMU_LINK_PLAIN, emulate.NFC_EMU_LINK_AIR
RAISED, ERR_ONES, UID_OVERFLOW = _lib.NFC_EMU_RAISED, _lib.NFC_EMU_ERR_ONES, _lib.NFC_EMU_UID_OVERFLOW
CUT_FRAMES, CUT_BYTES = _lib.NFC_EMU_PAIR_CUT_FRAMES, _lib.NFC_EMU_PAIR_CUT_BYTES
ENCRYPTED = _lib.NFC_EMU_FRAME_ENCRYPTED
ARRAYS = ('results', 'frames', 'plain', 'air', 'par')
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def names_of(T):
    return [CT.by_index(int(f['cmd'])).name() for f in T.frames]


# ---- 1. the pairs: the twin's catalogue ---------------------------------------------------------------------------------------------------
K_PAIRS = 3 * 64 + 1
SAME_AT = (0, 31, 63, 64, 100, 127, 128, K_PAIRS - 1)   # lane independence: these lanes' pairs are also run alone
CAPPED_PAIR, CAPPED_FRAMES = 'mixed_7', 20              # a mixed pair (Classic, CARD, a reader with a table) whose slab is outgrown by frames


def classic_memory(seed, data_conds, trailer_conds):
    mem = _card_memory(seed, data_conds, trailer_conds)
    mem[0] = 0x04 + 4 * (seed % 8)   # (not 0x88: the cascade tag is an Ultralight's)
    mem[4] = mem[0] ^ mem[1] ^ mem[2] ^ mem[3]
    return mem


def trailer_keys(mem):
    """keys A and B of every sector from the trailers, as set_sector_keys and reader_card take them"""
    t = {}
    for s in range(16):
        trailer = bytes(bytearray(mem[(4 * s + 3) * 16:(4 * s + 4) * 16].tolist()))
        t[(0x60, s)], t[(0x61, s)] = trailer[:6], trailer[10:]
    return t


def ultralight_memory(rng, bcc_error=0):
    mem = rng.integers(0, 256, 64).astype(np.uint8)
    mem[3] = 0x88 ^ mem[0] ^ mem[1] ^ mem[2] ^ bcc_error   # seven UID bytes: 0 .. 2 behind the cascade tag, 4 .. 7
    mem[8] = mem[4] ^ mem[5] ^ mem[6] ^ mem[7]
    return mem


class Entry(object):
    """One pair of the catalogue: the two cards and what the reader is made of (to make it again with or without its table)."""

    def __init__(self, name, tag, rands, key_a=(0xFF,) * 6, table=None, mode=CARD):
        self.name, self.tag, self.rands, self.key_a, self.table, self.mode = name, tag, rands, key_a, table, mode
        self.reader = emulate.reader_card(rands, key_a=key_a, table=table, mode=mode)


def catalogue():
    def make():
        rng = np.random.Generator(np.random.PCG64(1931))
        out = []

        def classic(name, mem, mode, n_tag=3, n_reader=2, reader_mode=None, key_a=None, table='a', tag_rands=None):
            keys = trailer_keys(mem)
            a_keys = {k: v for k, v in keys.items() if k[0] == 0x60}
            tag = emulate.tag_card(emulate.CLASSIC1K, mem, rng.integers(0, 256, (n_tag, 4)) if tag_rands is None else tag_rands, mode)
            out.append(Entry(name, tag, rng.integers(0, 256, (n_reader, 4)), key_a or keys[(0x60, 15)], a_keys if table == 'a' else table,
                             mode if reader_mode is None else reader_mode))

        for mode, m in ((REF, 'ref'), (CARD, 'card')):
            # key B only: block 1 of every sector under condition 3.  One reader has key A, one has key B in key A's place
            mem = classic_memory(101, [[0, 3, 0]] * 16, [1] * 16)
            classic('keyb_reader_a_' + m, mem, mode)
            classic('keyb_reader_b_' + m, mem, mode, key_a=trailer_keys(mem)[(0x61, 15)], table=None)
            # block 8, bytes 6 .. 9 say "never readable": where REFERENCE mode would look after an AUTH on block 5
            mem = classic_memory(5, [[0, 0, 0]] * 16, [1] * 16)
            mem[5 * 16 + 54:5 * 16 + 58] = _access([7, 7, 7, 7])
            classic('auth_block_' + m, mem, mode)
            # trailers under condition 4 (sectors 8 .. 15) and 1 (0 .. 7); the complement of C1 broken in sector 15's and in sector 0's
            mem = classic_memory(9, [[0, 0, 0]] * 16, [1] * 8 + [4] * 8)
            mem[63 * 16 + 6] ^= 0x01
            classic('trailer_15_' + m, mem, mode)
            mem = classic_memory(9, [[0, 0, 0]] * 16, [1] * 8 + [4] * 8)
            mem[3 * 16 + 6] ^= 0x01
            classic('trailer_0_' + m, mem, mode)
            # a CARD tag; the reader's table is wrong for sector 12 and right for the others, in both of the reader's modes
            mem = classic_memory(11, [[0, 0, 0]] * 16, [1] * 16)
            table = {k: v for k, v in trailer_keys(mem).items() if k[0] == 0x60}
            table[(0x60, 12)] = bytes(bytearray([1, 2, 3, 4, 5, 6]))
            classic('wrong_key_reader_' + m, mem, CARD, reader_mode=mode, table=table)
            if mode == CARD:   # ... and wrong for sector 15, the first one asked for, in the table and in key A
                table = dict(table)
                table[(0x60, 12)], table[(0x60, 15)] = trailer_keys(mem)[(0x60, 12)], bytes(bytearray([6, 5, 4, 3, 2, 1]))
                classic('wrong_first_key_card', mem, CARD, key_a=table[(0x60, 15)], table=table)
            # ... and with the right table: SideTable::reader_on decides whether it counts
            classic('table_reader_' + m, classic_memory(12, [[0, 0, 0]] * 16, [1] * 16), CARD, reader_mode=mode)
            out.append(Entry('ultralight_' + m, emulate.tag_card(emulate.ULTRALIGHT, ultralight_memory(rng), None, mode), rng.integers(0, 256, (1, 4)), mode=mode))
            out.append(Entry('ultralight_bcc_' + m, emulate.tag_card(emulate.ULTRALIGHT, ultralight_memory(rng, 0x10), None, mode),
                             rng.integers(0, 256, (1, 4)), mode=mode))
        # the nonce index: 64 nonces, and a twin with the first 63 of them
        mem, nonces = classic_memory(13, [[0, 0, 0]] * 16, [1] * 16), rng.integers(0, 256, (64, 4))
        reader_rands = rng.integers(0, 256, (64, 4))
        for n in (64, 63):
            classic('nonces_%d' % n, mem, CARD, tag_rands=nonces[:n])
            out[-1] = Entry(out[-1].name, out[-1].tag, reader_rands, out[-1].key_a, out[-1].table, CARD)
        assert len({e.name for e in out}) == len(out)
        return out
    return cached('catalogue', make)


def entry(name):
    return next(e for e in catalogue() if e.name == name)


def pair_lanes():
    """K_PAIRS (name, tag, reader): eight catalogue entries at SAME_AT, the others every fifth lane from lane 2, the mixed pairs of
    tests/test_emulate.py -- its 65 from its seed, and as many more as fill the call -- everywhere else, in their order."""
    def make():
        lanes = [None] * K_PAIRS
        pinned = ('keyb_reader_a_card', 'trailer_15_card', 'wrong_key_reader_card', 'nonces_64', 'ultralight_bcc_card', 'auth_block_ref',
                  'table_reader_ref', 'trailer_0_card')
        for at, name in zip(SAME_AT, pinned):
            lanes[at] = (name, entry(name).tag, entry(name).reader)
        at = 2
        for e in catalogue():
            if e.name in pinned:
                continue
            while lanes[at] is not None:
                at += 1
            lanes[at] = (e.name, e.tag, e.reader)
            at += 5
        rng, k = np.random.Generator(np.random.PCG64(65)), 0
        for at in range(K_PAIRS):
            if lanes[at] is None:
                lanes[at] = ('mixed_%d' % k,) + _pair(k, rng)
                k += 1
        assert k >= 65
        return lanes
    return cached('pair_lanes', make)


def lane_of(name):
    return next(i for i, l in enumerate(pair_lanes()) if l[0] == name)


def max_rands():
    text = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc', 'emu.hip.h')).read()
    m = re.search(r'constexpr\s+uint32_t\s+MAX_RANDS\s*=\s*(\d+)\s*,', text)
    assert m, 'emu.hip.h: no definition of MAX_RANDS matches any more'
    return int(m.group(1))


def rounds_needed():
    """From the twin's count: the rounds that take a 64-nonce tag's index past 64, and those that fill a reader's 32 UID bytes and one more."""
    def make():
        e = entry('nonces_64')
        T = emulate.pairs_host([e.tag], [e.reader], link=AIR, rounds=1).transcript(0)
        per_round = names_of(T).count('RANDTA')
        assert int(T.result['flags']) == 0 and per_round > 0
        wrap = max_rands() // per_round + 1
        return dict(per_round=per_round, wrap=wrap, uid=32 // 4 + 1, rounds=max(wrap, 32 // 4 + 1))
    return cached('rounds', make)


def pairs_kw(link):
    r = rounds_needed()['rounds']
    caps = np.full(K_PAIRS, 200 * r, np.uint32)
    caps[lane_of(CAPPED_PAIR)] = CAPPED_FRAMES
    return dict(link=link, rounds=r, cap_frames=200 * r, cap_bytes=1800 * r, pair_cap_frames=caps)


def pairs_twin(link):
    """the one call of K_PAIRS pairs on the twin, once per link; shared, nothing in it is changed"""
    def make():
        lanes = pair_lanes()
        host = emulate.pairs_host([l[1] for l in lanes], [l[2] for l in lanes], **pairs_kw(link))
        for a in host.arrays():
            a.setflags(write=False)
        return host
    return cached(('pairs_twin', link), make)


def same_arrays(a, b, what=''):
    for name, x, y in zip(ARRAYS, a.arrays(), b.arrays()):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)


def lane_arrays(T, k):
    return [a[k].tobytes() for a in T.arrays()]


def alone(call, link, k):
    """lane k's pair in a call of its own, with the call's configuration"""
    name, tag, reader = pair_lanes()[k]
    kw = pairs_kw(link)
    kw['pair_cap_frames'] = kw['pair_cap_frames'][k:k + 1]
    return call([tag], [reader], **kw)


def test_the_catalogue_is_what_its_names_say():
    # the memories, with the twin's single steps: what each card WOULD do if a reader asked
    mem = entry('keyb_reader_a_card').tag.mem
    for mode, auth, want in ((CARD, CT.AUTHB, CT.READT.index), (CARD, CT.AUTHA, None), (REF, CT.AUTHB, None)):
        tag, st = _selected_tag(mode, mem)
        emulate.step(tag, st, auth.index, [0x3C])
        emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
        assert emulate.step(tag, st, CT.READR.index, [0x3D])[0] == want       # block 1 of sector 15: key B alone
        assert emulate.step(tag, st, CT.READR.index, [0x3E])[0] == CT.READT.index
    mem = entry('auth_block_ref').tag.mem
    for mode, want in ((REF, None), (CARD, CT.READT.index)):
        tag, st = _selected_tag(mode, mem)
        emulate.step(tag, st, CT.AUTHA.index, [0x05])
        emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
        assert emulate.step(tag, st, CT.READR.index, [0x04])[0] == want
    for name, sector in (('trailer_15_card', 15), ('trailer_0_card', 0)):
        mem = entry(name).tag.mem
        tag, st = _selected_tag(CARD, mem)
        for s, shown_b in ((2, True), (12, False)):
            emulate.step(tag, st, CT.AUTHA.index, [4 * s])
            emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
            cmd, frame = emulate.step(tag, st, CT.READR.index, [4 * s + 3])
            t = mem[(4 * s + 3) * 16:(4 * s + 4) * 16].tolist()
            assert cmd == CT.READT.index and frame[:16] == [0] * 6 + t[6:10] + (t[10:] if shown_b else [0] * 6)
        assert st.flags == 0
        emulate.step(tag, st, CT.AUTHA.index, [4 * sector])
        emulate.step(tag, st, CT.RANDRB.index, [0] * 8)
        emulate.step(tag, st, CT.READR.index, [4 * sector + 1])
        assert st.flags == ERR_ONES
    for name in ('ultralight_card', 'ultralight_bcc_card'):
        mem = entry(name).tag.mem
        assert (int(mem[3]) == 0x88 ^ int(mem[0]) ^ int(mem[1]) ^ int(mem[2])) == (name == 'ultralight_card') and int(mem[8]) == int(mem[4] ^ mem[5] ^ mem[6] ^ mem[7])
    a, b = entry('nonces_64'), entry('nonces_63')
    assert len(a.tag.rands) == 64 == len(a.reader.rands) and len(b.tag.rands) == 63 and a.tag.rands[:63].tobytes() == b.tag.rands.tobytes()
    assert a.tag.mem.tobytes() == b.tag.mem.tobytes() and len({r.tobytes() for r in a.tag.rands}) == 64
    # the lanes: four workgroups, the last with one live lane; neighbours differ
    lanes = pair_lanes()
    assert len(lanes) == K_PAIRS > 192 and K_PAIRS % 64 == 1 and {l[0] for l in lanes} >= {e.name for e in catalogue()}
    assert sum(l[0].startswith('mixed_') for l in lanes) >= 65
    kind = [(l[1].tag_type, l[1].mode, l[2].mode, l[2].table is None) for l in lanes]
    assert sum(kind[i] != kind[i + 1] for i in range(K_PAIRS - 1)) >= 0.9 * (K_PAIRS - 1)
    for w in range(0, K_PAIRS - 1, 64):   # every full wave: both tag types, both modes on both sides, readers with and without a table
        assert len({k[0] for k in kind[w:w + 64]}) == 2 and len({k[1] for k in kind[w:w + 64]}) == 2 and len({k[2:] for k in kind[w:w + 64]}) == 4
    assert SAME_AT[0] == 0 and SAME_AT[-1] == K_PAIRS - 1 and {63, 64, 127, 128} < set(SAME_AT) and len(set(SAME_AT)) == 8


@pytest.mark.parametrize('link', [PLAIN, AIR])
def test_every_catalogue_entry_shows_in_its_lane_on_the_twin(link):
    host, r = pairs_twin(link), rounds_needed()
    res = host.results
    assert r['per_round'] == 16 and r['wrap'] == 5 and r['rounds'] == 9
    flags = lambda name, field: int(res[lane_of(name)][field])
    T = lambda name: host.transcript(lane_of(name))
    # no slab but the capped one is outgrown, and no round runs away
    capped = lane_of(CAPPED_PAIR)
    assert [k for k in range(K_PAIRS) if int(res[k]['flags'])] == [capped] and int(res[capped]['flags']) == CUT_FRAMES
    assert int(res[capped]['n_frames']) > CAPPED_FRAMES == len(host.transcript(capped))
    assert (res['rounds'] == r['rounds']).all() and int(res['n_frames'].max()) == 199 * r['rounds'] and int(res['n_bytes'].max()) <= 1800 * r['rounds']
    # key B only: the tag is silent at block 0x3D whichever key the reader holds -- the reader sends AUTHA and nothing else
    for m in ('ref', 'card'):
        for who in ('a', 'b'):
            t = T('keyb_reader_%s_%s' % (who, m))
            first = [n for n, f in zip(names_of(t), t.frames) if int(f['round']) == 0]
            if link == PLAIN or (who, m) == ('a', 'card'):
                assert first[-2:] == ['READT', 'READR'] and t.plain(len(first) - 1).tolist()[1] == 0x3D and 'AUTHB' not in names_of(t)
            else:   # REFERENCE keys its machine from sector 0's trailer, and key B is not key A: the tag hears rubbish for {nr}{ar}
                assert first[-1] == 'RANDRB' and flags('keyb_reader_%s_%s' % (who, m), 'tag_flags') & RAISED
    # ... and the round that ends there leaves the reader its UID: four more bytes a round, the nonce refused from the second round on
    # (more UID bits than nonce bits), the ninth round's bytes not taken.  On the AIR link the tag's machine stays inside its session
    # and hears every later REQA as ciphertext.
    if link == PLAIN:
        assert all(flags('keyb_reader_%s_%s' % (w, m), 'reader_flags') == RAISED | UID_OVERFLOW for w in ('a', 'b') for m in ('ref', 'card'))
    else:
        assert not any(int(v) & UID_OVERFLOW for v in res['reader_flags']) and flags('keyb_reader_a_card', 'tag_flags') == RAISED
    # the access bytes at the AUTH's block: the reader authenticates first blocks only, so the modes read the same bytes
    assert flags('auth_block_ref', 'tag_flags') == 0 or link == AIR
    if link == PLAIN:
        a, b = T('auth_block_ref'), T('auth_block_card')
        reads = lambda t: [(n, t.plain(i).tolist()) for i, n in enumerate(names_of(t)[:199]) if n in ('AUTHA', 'READR', 'READT')]
        assert len(a) == len(b) == 199 * r['rounds'] and reads(a) == reads(b) and len(reads(a)) == 16 + 2 * 64   # (the nonces are each pair's own)
    # flagged trailers: sector 15's is read in the first frames, sector 0's at the end of a whole card
    whole = ['trailer_%s_%s' % (s, m) for s in ('15', '0') for m in ('ref', 'card') if link == PLAIN or m == 'card']
    for name in whole:
        assert flags(name, 'tag_flags') == ERR_ONES and int(res[lane_of(name)]['n_frames']) == 199 * r['rounds']
        t = T(name)
        reads = {t.plain(i - 1).tolist()[1]: t.plain(i).tolist()[:16] for i in range(1, 199) if names_of(t)[i] == 'READT'}
        mem = pair_lanes()[lane_of(name)][1].mem
        assert len(reads) == 64
        for s in range(16):   # key A hidden; key B shown under condition 1, hidden under 4
            tr = mem[(4 * s + 3) * 16:(4 * s + 4) * 16].tolist()
            assert reads[4 * s + 3] == [0] * 6 + tr[6:10] + (tr[10:] if s < 8 else [0] * 6)
    assert {k for k in range(K_PAIRS) if int(res[k]['tag_flags']) & ERR_ONES} == {lane_of(n) for n in whole} and len(whole) == (4 if link == PLAIN else 2)
    # a reader whose keys are right for some sectors and wrong for others: the round ends where the wrong one is asked for
    if link == AIR:
        t = T('wrong_key_reader_card')
        first = [(n, t.plain(i).tolist()) for i, (n, f) in enumerate(zip(names_of(t), t.frames)) if int(f['round']) == 0]
        auths = [d[1] for n, d in first if n == 'AUTHA']
        # (a NESTED authentication: the tag's {nt} goes out under sector 12's key, and it is the reader's machine that hears rubbish)
        assert auths == [0x3C, 0x38, 0x34, 0x30] and first[-1][0] == 'RANDTA' and flags('wrong_key_reader_card', 'reader_flags') & RAISED
        t = T('wrong_first_key_card')   # the FIRST authentication: the nonce is plain, {nr}{ar} is rubbish to the tag, the tag stays silent
        assert [n for n, f in zip(names_of(t), t.frames) if int(f['round']) == 0][-3:] == ['AUTHA', 'RANDTA', 'RANDRB']
        assert flags('wrong_first_key_card', 'tag_flags') & RAISED and not flags('wrong_first_key_card', 'reader_flags') & RAISED
        assert int(res[lane_of('wrong_key_reader_card')]['n_frames']) > int(res[lane_of('wrong_key_reader_ref')]['n_frames'])
        # the same reader with the right table: in CARD mode the whole card, in REFERENCE mode the table does not count
        assert int(res[lane_of('table_reader_card')]['n_frames']) == 199 * r['rounds'] and flags('table_reader_card', 'reader_flags') == 0
        assert int(res[lane_of('table_reader_ref')]['n_frames']) < 199 and flags('table_reader_ref', 'reader_flags') & RAISED
    else:
        assert int(res[lane_of('wrong_key_reader_card')]['n_frames']) == 199 * r['rounds']
    # the nonce index: the transcripts part at authentication 63 (0-based), the round before the index wraps
    a, b = T('nonces_64'), T('nonces_63')
    assert len(a) == len(b) == 199 * r['rounds']
    differ = [i for i in range(len(a)) if a.plain(i).tolist() != b.plain(i).tolist()]
    nonce_frames = [i for i, n in enumerate(names_of(a)) if n == 'RANDTA']
    assert differ[0] == nonce_frames[63] and int(a.frames[differ[0]]['round']) == 63 // r['per_round'] == r['wrap'] - 2
    rands = entry('nonces_64').tag.rands
    assert [a.plain(i).tolist() for i in nonce_frames[:80]] == [rands[j % 64].tolist() for j in range(80)]
    assert int(a.frames[nonce_frames[64]]['round']) == r['wrap'] - 1 and [b.plain(i).tolist() for i in nonce_frames[63:65]] == rands[:2].tolist()
    # Ultralights: seven UID bytes; a wrong BCC passes the emulators and stops the reader's machine on the AIR link
    for m in ('ref', 'card'):
        t = T('ultralight_' + m)
        assert int(t.result['n_frames']) == 19 * r['rounds'] and names_of(t)[:19].count('READT') == 4 and int(t.result['reader_flags']) == 0
        uid = [t.plain(3).tolist()[1:4], t.plain(7).tolist()[:4]]
        mem = pair_lanes()[lane_of('ultralight_' + m)][1].mem.tolist()
        assert uid == [mem[0:3], mem[4:8]]
        bad = T('ultralight_bcc_' + m)
        assert (int(bad.result['n_frames']), int(bad.result['reader_flags'])) == ((19 * r['rounds'], 0) if link == PLAIN else (4 * r['rounds'], RAISED))
    raised = sum(1 for k in range(K_PAIRS) if (int(res[k]['tag_flags']) | int(res[k]['reader_flags'])) & RAISED)
    overflow = sum(1 for v in res['reader_flags'] if int(v) & UID_OVERFLOW)
    assert (raised, overflow) == PAIRS_FLAGGED[link], (raised, overflow)
    if link == AIR:
        assert any(int(f) & ENCRYPTED for f in host.frames[lane_of('table_reader_card')]['flags'])


PAIRS_FLAGGED = {PLAIN: (133, 133), AIR: (142, 0)}   # lanes with NFC_EMU_RAISED on either side, with NFC_EMU_UID_OVERFLOW (held against the twin above)


@pytest.mark.parametrize('link', [PLAIN, AIR])
def test_a_lane_of_the_twin_is_its_pair_alone(link):
    host = pairs_twin(link)
    for k in SAME_AT:
        assert lane_arrays(alone(emulate.pairs_host, link, k), 0) == lane_arrays(host, k), pair_lanes()[k][0]
    assert len({lane_arrays(host, k)[2] for k in SAME_AT}) == 8   # eight different transcripts


def without_tables(extra=None):
    """the call's tags with readers that have no table (extra: lane K - 1's reader keeps its own)"""
    lanes = pair_lanes()
    readers = [emulate.reader_card(l[2].rands, key_a=l[2].key_a, key_b=l[2].key_b, table=None, mode=l[2].mode) for l in lanes]
    if extra:
        readers[-1] = lanes[-1][2]
    return [l[1] for l in lanes], readers


NO_TABLE_KW = dict(link=AIR, rounds=2, cap_frames=400, cap_bytes=3600)


def test_no_table_call_on_the_twin_differs_in_the_last_lane_alone():
    tags, readers = without_tables()
    assert all(r.struct().table is None for r in readers) and pair_lanes()[-1][2].struct().table is not None and pair_lanes()[-1][2].mode == CARD
    none = emulate.pairs_host(tags, readers, **NO_TABLE_KW)
    one = emulate.pairs_host(*without_tables(True), **NO_TABLE_KW)
    assert all(lane_arrays(none, k) == lane_arrays(one, k) for k in range(K_PAIRS - 1))
    assert int(one.results[-1]['n_frames']) == 398 > int(none.results[-1]['n_frames'])
    with_tables = emulate.pairs_host(tags, [l[2] for l in pair_lanes()], **NO_TABLE_KW)
    assert sum(lane_arrays(none, k) != lane_arrays(with_tables, k) for k in range(K_PAIRS)) >= 30   # a table matters to many of these pairs


def small_call():
    """cap_bytes is per call: three pairs with 300 bytes each.  Lane 0 meets the byte limit first, lane 1 its own frame limit, lane 2 fits."""
    names = ('trailer_15_card', 'nonces_64', 'ultralight_card')
    return [entry(n).tag for n in names], [entry(n).reader for n in names], dict(link=AIR, rounds=1, cap_frames=64, cap_bytes=300, pair_cap_frames=[64, 10, 64])


def test_small_call_outgrows_a_slab_by_bytes_next_to_one_by_frames():
    tags, readers, kw = small_call()
    host = emulate.pairs_host(tags, readers, **kw)
    assert [int(v) for v in host.results['flags']] == [CUT_BYTES, CUT_FRAMES, 0]
    t = host.transcript(0)
    assert len(t) < 64 and int(t.frames['n_bytes'].sum()) <= 300 < int(t.frames['n_bytes'].sum()) + 18 and int(t.result['n_frames']) == 199
    assert len(host.transcript(1)) == 10 and len(host.transcript(2)) == 19


@pytest.mark.gpu
@pytest.mark.parametrize('link', [PLAIN, AIR])
def test_pairs_kernel_equals_the_twin_over_the_catalogue(link):
    lanes, host = pair_lanes(), pairs_twin(link)
    dev = emulate.pairs_device([l[1] for l in lanes], [l[2] for l in lanes], **pairs_kw(link))   # (raises unless the call's status is 0: guards included)
    same_arrays(host, dev)


@pytest.mark.gpu
@pytest.mark.parametrize('link', [PLAIN, AIR])
def test_a_lane_of_the_kernel_is_its_pair_alone(link):
    # the [i][K] + k indexing: a lane's slab and result from a K = 1 call, where every stride is 1
    lanes = pair_lanes()
    dev = emulate.pairs_device([l[1] for l in lanes], [l[2] for l in lanes], **pairs_kw(link))
    for k in SAME_AT:
        assert lane_arrays(alone(emulate.pairs_device, link, k), 0) == lane_arrays(dev, k), lanes[k][0]


@pytest.mark.gpu
def test_pairs_kernel_without_any_table_and_with_one_in_the_last_lane():
    none = emulate.pairs_device(*without_tables(), **NO_TABLE_KW)            # A.tables is null
    same_arrays(emulate.pairs_host(*without_tables(), **NO_TABLE_KW), none)
    one = emulate.pairs_device(*without_tables(True), **NO_TABLE_KW)
    same_arrays(emulate.pairs_host(*without_tables(True), **NO_TABLE_KW), one)
    assert all(lane_arrays(none, k) == lane_arrays(one, k) for k in range(K_PAIRS - 1))
    assert lane_arrays(none, K_PAIRS - 1) != lane_arrays(one, K_PAIRS - 1)


@pytest.mark.gpu
def test_pairs_kernel_outgrows_a_slab_by_bytes_next_to_one_by_frames():
    tags, readers, kw = small_call()
    same_arrays(emulate.pairs_host(tags, readers, **kw), emulate.pairs_device(tags, readers, **kw))


# ---- 2. streams that answer, keyed per sector, on mutated sessions ----------------------------------------------------------------------
N_STREAM_PAIRS = 32      # pairs of _pair(): 24 Classic, 8 Ultralight
K_STREAMS = 132          # three workgroups, the last with four live lanes; role k % 4
SIDE_FRAMES = 40
ROLE_CLASSIC_TAG, ROLE_ULTRALIGHT_TAG, ROLE_READER, ROLE_NONE = range(4)
MUTATIONS = ('flip', 'drop', 'double', 'cut', 'lengthen', 'exchange')
REDRAWS = 64


def mutate(frames, n_mut, rng):
    """n_mut seeded mutations of a frame list, placed in its second half (uniform placement leaves too few sessions alive behind the
    first mutated frame: the CPU half holds the share).  -> the new list."""
    out = [(t, list(b)) for t, b in frames]
    for _ in range(n_mut):
        n = len(out)
        i = n // 2 + int(rng.integers(n - n // 2))
        kind = MUTATIONS[int(rng.integers(len(MUTATIONS)))]
        t, b = out[i]
        if kind == 'flip':
            b[int(rng.integers(len(b)))] ^= 1
        elif kind == 'drop' and n > 2:
            del out[i]
        elif kind == 'double':
            out.insert(i, (t, list(b)))
        elif kind == 'cut' and len(b) > 1:
            del b[1 + int(rng.integers(len(b) - 1)):]
        elif kind == 'lengthen':
            b += [int(v) for v in rng.integers(0, 2, 1 + int(rng.integers(12)))]
        elif kind == 'exchange' and i + 1 < n:
            out[i], out[i + 1] = out[i + 1], out[i]
    return out


class Stream(object):
    """One stream of part 2: role, card (None: none), table (the heard Classic card's keys A and B, or None), frames (what it hears),
    clean (before the mutations), first_mutated (the first frame that differs from the clean list; None: the stream is clean)."""


def stream_specs():
    def make():
        rng = np.random.Generator(np.random.PCG64(2024))
        pairs = [_pair(p, rng) for p in range(N_STREAM_PAIRS)]
        loop = emulate.pairs_host([p[0] for p in pairs], [p[1] for p in pairs], link=AIR, rounds=1)
        sides = []
        for p in range(N_STREAM_PAIRS):
            both = emulate.synth_frames(loop.transcript(p))
            sides.append({synth.TAG: [f for f in both if f[0] == synth.TAG][:SIDE_FRAMES], synth.READER: [f for f in both if f[0] == synth.READER][:SIDE_FRAMES],
                          None: both[:SIDE_FRAMES]})
        classic = [p for p in range(N_STREAM_PAIRS) if pairs[p][0].tag_type == emulate.CLASSIC1K]
        ultralight = [p for p in range(N_STREAM_PAIRS) if pairs[p][0].tag_type == emulate.ULTRALIGHT]
        out = []
        for k in range(K_STREAMS):
            s, j = Stream(), k // 4
            s.role = k % 4
            s.pair = {ROLE_CLASSIC_TAG: classic[j % len(classic)], ROLE_ULTRALIGHT_TAG: ultralight[j % len(ultralight)], ROLE_READER: j % N_STREAM_PAIRS,
                      ROLE_NONE: (5 * j) % N_STREAM_PAIRS}[s.role]
            tag, reader = pairs[s.pair]
            s.card = {ROLE_CLASSIC_TAG: tag, ROLE_ULTRALIGHT_TAG: tag, ROLE_READER: reader, ROLE_NONE: None}[s.role]
            s.classic = tag.tag_type == emulate.CLASSIC1K
            s.table = trailer_keys(tag.mem) if s.classic else None
            s.clean = sides[s.pair][{ROLE_READER: synth.TAG, ROLE_NONE: None}.get(s.role, synth.READER)]
            s.n_mut = (j + j // 4) % 4
            # Placement in the second half alone does not keep half of the sessions: behind a frame that is flipped, dropped, doubled, cut or
            # exchanged inside a session the keystream is lost for good (the twin: 2 to 16 % of such streams answer in cipher again; 98 % behind a
            # lengthened one).  So two streams in three draw again, up to REDRAWS times, until the twin answers in cipher behind the first
            # mutated frame; every third keeps its first draw, whatever became of its session.
            draw = np.random.Generator(np.random.PCG64(7000 + k))
            for s.draws in range(1, REDRAWS + 1):
                s.frames = mutate(s.clean, s.n_mut, draw)
                differ = [i for i in range(max(len(s.frames), len(s.clean))) if i >= len(s.frames) or i >= len(s.clean) or s.frames[i] != s.clean[i]]
                s.first_mutated = differ[0] if differ else None
                if s.first_mutated is None or s.card is None or not s.classic or k % 3 == 0 or n_encrypted(stream_twin(s)[1], s.first_mutated):
                    break
            out.append(s)
        return out
    return cached('stream_specs', make)


def stream_iq():
    def make():
        out = []
        for s in stream_specs():
            a = synth.iq_from_profile(synth.modulation_profile(s.frames))
            a.setflags(write=False)
            out.append(a)
        return out
    return cached('stream_iq', make)


def stream_twin(s, frames=None, est=None, fst=None):
    """the replay twin over what stream s hears (frames: an api.NfcFrames in place of the generated list), with the stream's own table
    -> ((table, data, enc), answers, the emulator's state, the machine's state); without a card the machine alone and no answers"""
    frames = emulate.frames_of_bits(s.frames) if frames is None else frames
    est, fst = est or emulate.state_init(), fst or fsm.state_init()
    if s.card is None:
        return fsm.host_commands(fst, frames.table, frames.bytes, frames.par, sector_keys=s.table), None, est, fst
    cmds, ans = emulate.host_emulate(s.card, est, fst, frames, sector_keys=s.table)
    return cmds, ans, est, fst


def n_encrypted(ans, behind=0):
    return 0 if ans is None else int((((ans.records['flags'] & ENCRYPTED) != 0) & (ans.records['src'] >= behind)).sum())


STREAM_COUNTS = dict(answers=955, encrypted=401, answering=99, raised=39)   # what the twin gives over the K_STREAMS streams (held below)


def test_streams_reach_sessions_and_keep_them_behind_their_mutations():
    specs = stream_specs()
    assert len(specs) == K_STREAMS >= 130 and N_STREAM_PAIRS >= 24 and [sum(s.role == r for s in specs) for r in range(4)] == [K_STREAMS // 4] * 4
    assert all(s.classic for s in specs if s.role == ROLE_CLASSIC_TAG) and not any(s.classic for s in specs if s.role == ROLE_ULTRALIGHT_TAG)
    assert all(len(s.clean) <= SIDE_FRAMES for s in specs) and max(len(s.clean) for s in specs) == SIDE_FRAMES
    assert max(len(a) for a in stream_iq()) // 2 <= 100000   # complex samples (40 frames of a tag's side are mostly READT, 3 058 samples each)
    runs = [stream_twin(s) for s in specs]
    # every clean keyed Classic stream brings a session up; without its table a tag stream never does
    keyed = [k for k, s in enumerate(specs) if s.classic and s.card is not None]
    clean = [k for k in keyed if specs[k].first_mutated is None]
    mutated = [k for k in keyed if specs[k].first_mutated is not None]
    assert len(clean) >= 12 and len(mutated) >= 36 and {specs[k].role for k in clean} == {specs[k].role for k in mutated} == {ROLE_CLASSIC_TAG, ROLE_READER}
    assert all(n_encrypted(runs[k][1]) > 0 for k in clean)
    bare = 0
    for k in clean:
        s = specs[k]
        _, ans = emulate.host_emulate(s.card, emulate.state_init(), fsm.state_init(), emulate.frames_of_bits(s.frames))
        bare += n_encrypted(ans) if s.role == ROLE_CLASSIC_TAG else 0
    assert bare == 0
    # at least half of the mutated ones give an encrypted answer BEHIND their first mutated frame (among the streams that can encrypt at
    # all: a Classic tag, or a reader that hears one)
    alive = [k for k in mutated if n_encrypted(runs[k][1], specs[k].first_mutated) > 0]
    assert 2 * len(alive) >= len(mutated), (len(alive), len(mutated))
    assert (len(clean), len(mutated), len(alive)) == (19, 39, 26)
    # ... most of the mutations fall inside a session (a Classic session is up from the fifth heard frame on), some streams kept their
    # first draw, and the clean tag streams answer nested AUTHs in cipher: {nt} under the table's key for the new sector
    assert 2 * sum(specs[k].first_mutated >= 5 for k in mutated) >= len(mutated) and sum(specs[k].draws == 1 for k in mutated) >= 13
    nested = sum(int(((r[1].records['cmd'] == CT.RANDTA.index) & ((r[1].records['flags'] & ENCRYPTED) != 0)).sum()) for k, r in enumerate(runs)
                 if k in clean and specs[k].role == ROLE_CLASSIC_TAG)
    assert nested >= 10
    # both NFC_EMU_RAISED and 0 among the final emulator flags
    flags = [int(r[2].flags) for k, r in enumerate(runs) if specs[k].card is not None]
    assert 0 in flags and any(f & RAISED for f in flags)
    got = dict(answers=sum(len(r[1]) for r in runs if r[1] is not None), encrypted=sum(n_encrypted(r[1]) for r in runs),
               answering=sum(1 for r in runs if r[1] is not None and len(r[1])), raised=sum(1 for f in flags if f & RAISED))
    assert got == STREAM_COUNTS, got
    assert all(r[1] is None for k, r in enumerate(runs) if specs[k].role == ROLE_NONE)


def streams_context(specs, max_push, **kw):
    """a tracked context of one stream per spec: its table through set_sector_keys, its card through emulate"""
    m = api.NfcMultiContext(len(specs), max_push, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, **kw)
    m.track_commands()
    for j, s in enumerate(specs):
        if s.table is not None:
            m.set_sector_keys(s.table, stream=j)
        if s.card is not None:
            m.emulate(s.card, j)
    return m


def guards_of(m):
    g = m.L.nfc_debug_multi_guards
    g.argtypes = [ctypes.c_void_p]
    return g


def fetched(m, K):
    """the last push's commands and answers, per stream, as copies: (commands, answers, bits)"""
    cm, an = m.fetch_commands(), m.fetch_answers()
    cmds = [tuple(a.copy() for a in cm.commands_of(k)) for k in range(K)]
    answers = [tuple(a.copy() for a in an.answers_of(k)) for k in range(K)]
    bits = [[(int(r['cmd']), int(r['flags']), an.bits(k, i)) for i, r in enumerate(answers[k][0])] for k in range(K)]
    return cm, an, cmds, answers, bits


def states_of(m, K):
    return [(state_bytes(m.fsm_state(k)), state_bytes(m.emu_state(k))) for k in range(K)]


def streams_one_push():
    """The K_STREAMS streams in one push on the hooks build, once; shared, nothing in it is changed."""
    def make():
        specs, iq = stream_specs(), stream_iq()
        with streams_context(specs, max(len(a) for a in iq) // 2, lib_path=_lib.hooks_path()) as m:
            guards = guards_of(m)
            m.push(iq)
            cm = m.fetch_commands()
            g1 = guards(m.h)
            an = m.fetch_answers()
            g2 = guards(m.h)
            _, _, cmds, answers, bits = fetched(m, K_STREAMS)
            return dict(cm=cm, an=an, guards=(g1, g2), cmds=cmds, answers=answers, bits=bits, states=states_of(m, K_STREAMS),
                        raw=[cm.raw.frames_of(k) for k in range(K_STREAMS)])
    return cached('streams_one_push', make)


def assert_stream_equals_twin(s, raw, cmds, answers, states, what, est=None, fst=None):
    """what one stream gave on the device against the replay twin on the frames the push assembled: commands, answers, both states"""
    want_cmds, want, est, fst = stream_twin(s, raw, est, fst)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cmds, want_cmds)) and len(cmds[0]) == len(raw.table), what
    rec, plain, air, par = answers
    if s.card is None:
        assert len(rec) == 0, what
    else:
        n = 18 * len(rec)
        assert rec.tobytes() == want.records.tobytes(), what
        assert plain.tobytes() == want.plain[:n].tobytes() and air.tobytes() == want.air[:n].tobytes() and par.tobytes() == want.par[:n].tobytes(), what
    assert states == (state_bytes(fst), state_bytes(est)), what
    return want


@pytest.mark.gpu
def test_streams_in_one_push_equal_the_replay_twin():
    specs, res = stream_specs(), streams_one_push()
    assert res['guards'] == (0, 0) and res['an'].emulated
    n_enc = n_raised = 0
    for k, s in enumerate(specs):
        want = assert_stream_equals_twin(s, res['raw'][k], res['cmds'][k], res['answers'][k], res['states'][k], k)
        n_enc += n_encrypted(want)
        n_raised += int(bool(_lib.EmuState.from_buffer_copy(res['states'][k][1]).flags & RAISED))
    # the IQ route brings the same traffic as the CPU half's frame lists: sessions come up and break on the device as they do there
    assert n_enc >= STREAM_COUNTS['encrypted'] * 9 // 10 and n_raised >= STREAM_COUNTS['raised'] * 9 // 10, (n_enc, n_raised)
    assert res['an'].n.tolist() == [len(a[0]) for a in res['answers']] and sum(len(a[0]) for a in res['answers']) == res['an'].n_answers


def ragged_sizes(lens):
    """three pushes by the PIECES pattern, zero-length pieces included; the third takes the rest"""
    K = len(lens)
    sizes = [np.minimum(lens, [PIECES[k % 3] for k in range(K)])]
    sizes.append(np.minimum(lens - sizes[0], [PIECES[(1 + k) % 3] for k in range(K)]))
    sizes.append(lens - sizes[0] - sizes[1])
    return sizes


@pytest.mark.gpu
def test_streams_in_three_ragged_pushes_equal_the_one_push():
    specs, iq, want = stream_specs(), stream_iq(), streams_one_push()
    lens = np.array([len(a) // 2 for a in iq])
    sizes = ragged_sizes(lens)
    assert sum(int((n == 0).sum()) for n in sizes) >= K_STREAMS // 3
    parts, bits, done = [[] for _ in specs], [[] for _ in specs], np.zeros(K_STREAMS, np.int64)
    with streams_context(specs, int(max(n.max() for n in sizes))) as m:
        for n in sizes:
            m.push([a[2 * b:2 * (b + c)] for a, b, c in zip(iq, done, n)])
            _, _, cmds, _, got_bits = fetched(m, K_STREAMS)
            for k in range(K_STREAMS):
                parts[k].append(cmds[k])
                bits[k] += got_bits[k]
            done += n
        assert (done == lens).all()
        states = states_of(m, K_STREAMS)
    for k in range(K_STREAMS):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(concatenated(parts[k]), want['cmds'][k])), k
        assert bits[k] == want['bits'][k] and states[k] == want['states'][k], k


@pytest.mark.gpu
def test_streams_handed_to_other_slots_of_a_second_context_continue_identically():
    specs, iq, want = stream_specs(), stream_iq(), streams_one_push()
    # sixteen Classic streams, eight tags and eight readers, those that hear the most; cut behind the seventh heard frame
    pick = []
    for role in (ROLE_CLASSIC_TAG, ROLE_READER):
        of_role = [k for k, s in enumerate(specs) if s.role == role and s.classic and len(want['raw'][k].table) >= 10]
        pick += sorted(of_role, key=lambda k: (-len(want['raw'][k].table), k))[:8]
    assert len(pick) == 16
    picked = [specs[k] for k in pick]
    cut = [int(want['raw'][k].table['idx'][6]) + 60 for k in pick]
    K2 = 16
    slot = lambda j: K2 - 1 - j
    with streams_context(picked, max(cut)) as m:
        m.push([iq[k][:2 * c] for k, c in zip(pick, cut)])
        _, _, head, _, head_bits = fetched(m, 16)
        handed = [(m.stream(j).get_state(), m.fsm_state(j), m.emu_state(j), m.sector_keys(j)) for j in range(16)]
        assert sum(int(h[1].encrypted != 0) for h in handed) >= 8
        assert all(h[3] == picked[j].table for j, h in enumerate(handed))
    rest = [len(iq[k]) // 2 - c for k, c in zip(pick, cut)]
    with api.NfcMultiContext(K2, max(rest), hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as m2:
        m2.track_commands()
        for j in range(16):   # stream j into slot K' - 1 - j, with that slot's card: a mis-indexed [word][K] store would show
            signal, fst, est, table = handed[j]
            m2.emulate(picked[j].card, slot(j))
            m2.stream(slot(j)).set_state(*signal)
            m2.set_fsm_state(slot(j), fst)
            m2.set_emu_state(slot(j), est)
            m2.set_sector_keys(table, stream=slot(j))
        tails = [None] * K2
        for j, k in enumerate(pick):
            tails[slot(j)] = iq[k][2 * cut[j]:]
        m2.push(tails)
        _, _, tail, _, tail_bits = fetched(m2, K2)
        states = states_of(m2, K2)
    for j, k in enumerate(pick):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(concatenated([head[j], tail[slot(j)]]), want['cmds'][k])), k
        assert head_bits[j] + tail_bits[slot(j)] == want['bits'][k] and states[slot(j)] == want['states'][k], k
        assert len(head[j][0]) >= 7 and len(tail[slot(j)][0]) >= 3


# ---- 3. the fuzz fixture through cards --------------------------------------------------------------------------------------------------
def fixture_cards():
    """six kinds, cyclically by stream: the Classic golden tag and reader (CARD), the Ultralight golden tag and reader, the Classic tag and
    reader again (REFERENCE)"""
    def make():
        json_of = lambda name: os.path.join(GOLDEN, 'fx_emu_%s.json' % name)
        return list(emulate.cards_from_json(json_of('classic1k'), CARD)) + list(emulate.cards_from_json(json_of('ultralight'), CARD)) + \
            list(emulate.cards_from_json(json_of('classic1k'), REF))
    return cached('fixture_cards', make)


def fixture_twin(k, row, card, frames):
    """the replay twin over one fixture stream with stream k's keys (tests/test_fsm_fuzz.py: tracked) -> (commands, answers, est, fst)"""
    est, fst = emulate.state_init(), fsm.state_init()
    fst.key_a[:], fst.key_b[:] = row.keys
    table = full_table(row.keys) if k % 3 == 2 else None
    if card is None:
        return fsm.host_commands(fst, frames.table, frames.bytes, frames.par, sector_keys=table), None, est, fst
    cmds, ans = emulate.host_emulate(card, est, fst, frames, sector_keys=table)
    return cmds, ans, est, fst


# what the twin gives for the cyclic assignment with the streams' own keys ...
FIXTURE_COUNTS = dict(answers=978, encrypted=112, answering=253, raised=234, machine_differs=165)
# ... and per kind over ALL 256 rows with the default keys: (answers, encrypted answers, rows answered)
FIXTURE_BY_KIND = [(847, 11, 253), (1173, 200, 252), (688, 0, 253), (1182, 203, 252), (847, 11, 253), (1173, 200, 252)]


def test_fixture_rows_answer_through_the_six_cards():
    rows, cards = fixture()['gpu'], fixture_cards()
    assert len(rows) == 256 and [(c.role, c.tag_type if c.role == 0 else 1, c.mode) for c in cards] == [(0, 1, CARD), (1, 1, CARD), (0, 0, CARD), (1, 1, CARD), (0, 1, REF), (1, 1, REF)]
    runs = [fixture_twin(k, row, cards[k % 6], frames_of(row)) for k, row in enumerate(rows)]
    answering = sum(1 for r in runs if len(r[1]))
    reader_enc = sum(n_encrypted(r[1]) for k, r in enumerate(runs) if k % 2 == 1)
    assert answering * 10 >= 9 * len(rows) and reader_enc >= 30, (answering, reader_enc)
    for kind in range(6):   # NFC_EMU_RAISED and 0 for every kind
        flags = [int(r[2].flags) & RAISED for k, r in enumerate(runs) if k % 6 == kind]
        assert 0 in flags and RAISED in flags, kind
    # the answer passes through the machine: the streams whose COMMANDS a card changes
    differs = [k for k, row in enumerate(rows) if any(a.tobytes() != b.tobytes() for a, b in zip(runs[k][0], fixture_twin(k, row, None, frames_of(row))[0]))]
    got = dict(answers=sum(len(r[1]) for r in runs), encrypted=sum(n_encrypted(r[1]) for r in runs), answering=answering,
               raised=sum(1 for r in runs if int(r[2].flags) & RAISED), machine_differs=len(differs))
    assert got == FIXTURE_COUNTS, got
    by_kind = []
    for card in cards:
        answers = [emulate.host_emulate(card, emulate.state_init(), fsm.state_init(), frames_of(row))[1] for row in rows]
        by_kind.append((sum(len(a) for a in answers), sum(n_encrypted(a) for a in answers), sum(1 for a in answers if len(a))))
    assert by_kind == FIXTURE_BY_KIND and by_kind[4:] == by_kind[:2], by_kind   # (this traffic does not tell the two modes apart in what is counted)


@pytest.mark.gpu
def test_fixture_streams_with_cards_equal_the_replay_twin():
    """The 256 captures of tests/test_fsm_fuzz.py once more, every stream with a card.  These streams decode BOTH directions, so a stream hears
    the real device's answer behind its own.  165 of the 256 give other commands than the card-less push (on the twin: 33, 34, 5, 33, 31
    and 29 of the six kinds in their order): the card's answer has passed through the stream's machine first -- a tag's RANDTA or a
    reader's RANDRB has keyed a session before the recorded one arrives, and what follows decrypts differently.  All but five of the
    Ultralight tags are among the 91 others, and with them the streams whose answers stay in the anticollision.  Which stream is which
    is found with the twin, on the frames of the push."""
    streams, rows, cards, bare = gpu_streams(), fixture()['gpu'], fixture_cards(), gpu_one_push()
    with tracked(list(enumerate(rows)), max(len(a) for a in streams) // 2, lib_path=_lib.hooks_path()) as m:
        for k in range(len(rows)):
            m.emulate(cards[k % 6], k)
        guards = guards_of(m)
        m.push(streams)
        cm = m.fetch_commands()
        g1 = guards(m.h)
        an = m.fetch_answers()
        assert (g1, guards(m.h)) == (0, 0)
        _, _, cmds, answers, _ = fetched(m, len(rows))
        states = states_of(m, len(rows))
        raws = [cm.raw.frames_of(k) for k in range(len(rows))]
    same = n_answers = 0
    for k, row in enumerate(rows):
        want_cmds, want, est, fst = fixture_twin(k, row, cards[k % 6], raws[k])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(cmds[k], want_cmds)), k
        rec, plain, air, par = answers[k]
        n = 18 * len(rec)
        assert rec.tobytes() == want.records.tobytes(), k
        assert plain.tobytes() == want.plain[:n].tobytes() and air.tobytes() == want.air[:n].tobytes() and par.tobytes() == want.par[:n].tobytes(), k
        assert states[k] == (state_bytes(fst), state_bytes(est)), k
        n_answers += len(rec)
        # wherever the stream's own answers change nothing, the commands of the card-less push
        if all(a.tobytes() == b.tobytes() for a, b in zip(want_cmds, fixture_twin(k, row, None, raws[k])[0])):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(cmds[k], bare['got'][k])), k
            same += 1
    assert n_answers == FIXTURE_COUNTS['answers'] and len(rows) - same == FIXTURE_COUNTS['machine_differs']


# ---- 4. streams whose bit slab is outgrown: the push ends in cut frames ------------------------------------------------------------------
TRUNC_BITS = 300   # cap_packet_bits: a Classic session is up at bit 214 of what a tag hears, at bit 162 of what a reader hears


def truncated_pick():
    """the keyed Classic streams that hear more bits than the slab holds"""
    heard = lambda s: sum(len(b) + (1 if len(b) == 7 else 0) for _, b in s.frames)
    return [k for k, s in enumerate(stream_specs()) if s.classic and s.card is not None and heard(s) > TRUNC_BITS + 100]


def test_truncated_streams_outgrow_their_slab_inside_a_session():
    pick = truncated_pick()
    assert len(pick) >= 20 and {stream_specs()[k].role for k in pick} == {ROLE_CLASSIC_TAG, ROLE_READER}
    for k in pick:   # the frames that fit bring a session up: the emulator has left its initial state when the slab ends
        s = stream_specs()[k]
        fits, used = [], 0
        for t, b in s.frames:
            used += len(b) + (1 if len(b) == 7 else 0)
            if used > TRUNC_BITS:
                break
            fits.append((t, b))
        head = Stream()
        head.card, head.table, head.frames = s.card, s.table, fits
        _, ans, est, _ = stream_twin(head)
        assert state_bytes(est) != state_bytes(emulate.state_init()) and len(ans) >= 3, k


@pytest.mark.gpu
def test_streams_with_an_outgrown_bit_slab_equal_the_twin_and_keep_their_state():
    specs, iq, pick = stream_specs(), stream_iq(), truncated_pick()
    picked = [specs[k] for k in pick]
    with streams_context(picked, max(len(iq[k]) for k in pick) // 2, cap_packet_bits=TRUNC_BITS, lib_path=_lib.hooks_path()) as m:
        guards = guards_of(m)
        m.push([iq[k] for k in pick])
        trunc = [bool(f & api.NFC_MULTI_TRUNC_BITS) for f in m.counts_all()['flags']]
        cm, an, cmds, answers, _ = fetched(m, len(pick))
        assert guards(m.h) == 0
        states = states_of(m, len(pick))
        assert cm.stream_flags.tolist() == [_lib.NFC_FSM_LOST if t else 0 for t in trunc] and sum(trunc) >= 20
        ends_cut = 0
        for j, s in enumerate(picked):
            fst = fsm.state_init()
            fst.flags = _lib.NFC_FSM_LOST if trunc[j] else 0   # (sticky, and read by nothing: the kernel sets it before the first frame)
            assert_stream_equals_twin(s, cm.raw.frames_of(j), cmds[j], answers[j], states[j], pick[j], fst=fst)
            last_cut = len(cmds[j][0]) > 0 and int(cmds[j][0]['cmd'][-1]) == _lib.NFC_CMD_CUT
            ends_cut += int(last_cut and states[j][1] != state_bytes(emulate.state_init()))
        assert ends_cut >= 10, ends_cut   # pushes that END in a cut frame, behind answers that moved the emulator
