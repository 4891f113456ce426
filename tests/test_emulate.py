"""K cards read by K readers on the GPU, a lane per pair (nfc_emulate_pairs_device: csrc/nfc_emu.hip over csrc/emu.hip.h),
against its twin on the CPU (nfc_host_emulate_pairs, which tests/test_emulate_host.py pins to the reference's traces): the same bytes in
every output array.  The device call itself checks the guard words behind its device sections and fails when one was overwritten."""
import os

import numpy as np
import pytest

from usrp_nfc_amd import emulate

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
REF, CARD = emulate.NFC_EMU_REFERENCE, emulate.NFC_EMU_CARD


def _access(conds):
    c1 = sum(((c >> 2) & 1) << i for i, c in enumerate(conds))
    c2 = sum(((c >> 1) & 1) << i for i, c in enumerate(conds))
    c3 = sum((c & 1) << i for i, c in enumerate(conds))
    return [((~c2 & 0xF) << 4) | (~c1 & 0xF), (c1 << 4) | (~c3 & 0xF), (c3 << 4) | c2, 0x69]


def _pair(k, rng):
    """pair k of a mixed wave: Classic / Ultralight and CARD / REFERENCE by k, every card with its own UID, memory, keys and nonces"""
    mode = CARD if k % 3 else REF
    if k % 4 == 1:
        mem = rng.integers(0, 256, 64).astype(np.uint8)
        mem[3] = 0x88 ^ mem[0] ^ mem[1] ^ mem[2]
        mem[8] = mem[4] ^ mem[5] ^ mem[6] ^ mem[7]
        return emulate.tag_card(emulate.ULTRALIGHT, mem, None, mode), emulate.reader_card(rng.integers(0, 256, (1, 4)), mode=mode)
    mem = rng.integers(0, 256, 1024).astype(np.uint8)
    mem[0] = 0x04 + 4 * (k % 8)   # (not 0x88: the cascade tag is an Ultralight's)
    mem[4] = mem[0] ^ mem[1] ^ mem[2] ^ mem[3]
    for s in range(16):
        # data blocks under the conditions key A may read, one sector in seven with a block it may not; trailers under all eight
        conds = [[0, 1, 2, 4, 6][(k + s + b) % 5] for b in range(3)] + [(k + s) % 8]
        if (k + s) % 7 == 0:
            conds[1] = 3
        mem[(4 * s + 3) * 16 + 6:(4 * s + 3) * 16 + 10] = _access(conds)
    table = {(0x60, s): bytes(mem[(4 * s + 3) * 16:(4 * s + 3) * 16 + 6].tolist()) for s in range(16)}
    tag = emulate.tag_card(emulate.CLASSIC1K, mem, rng.integers(0, 256, (1 + k % 7, 4)), mode)
    reader = emulate.reader_card(rng.integers(0, 256, (1 + k % 5, 4)), key_a=table[(0x60, 15)], table=table if k % 2 else None, mode=mode)
    return tag, reader


def _same(host, dev):
    for name, a, b in zip(('results', 'frames', 'plain', 'air', 'par'), host.arrays(), dev.arrays()):
        assert a.tobytes() == b.tobytes(), name


@pytest.mark.gpu
def test_one_pair_reads_the_reference_s_card_as_the_twin_does():
    tag, reader = emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_classic1k.json'), CARD)
    kw = dict(link=emulate.NFC_EMU_LINK_AIR, rounds=2, cap_frames=400, cap_bytes=3600)
    host, dev = emulate.pairs_host([tag], [reader], **kw), emulate.pairs_device([tag], [reader], **kw)
    assert int(host.results[0]['n_frames']) == 398 and int(host.results[0]['flags']) == 0
    _same(host, dev)


@pytest.mark.gpu
@pytest.mark.parametrize('link', [emulate.NFC_EMU_LINK_PLAIN, emulate.NFC_EMU_LINK_AIR])
def test_sixty_five_mixed_pairs_equal_the_twin_byte_for_byte(link):
    # two workgroups, the second with one live lane; Classic and Ultralight, CARD and REFERENCE in one wave; pair 5's slab holds 20 frames
    rng = np.random.Generator(np.random.PCG64(65))
    pairs = [_pair(k, rng) for k in range(65)]
    tags, readers = [p[0] for p in pairs], [p[1] for p in pairs]
    caps = np.full(65, 400, np.uint32)
    caps[5] = 20
    kw = dict(link=link, rounds=2, cap_frames=400, cap_bytes=3600, pair_cap_frames=caps)
    host, dev = emulate.pairs_host(tags, readers, **kw), emulate.pairs_device(tags, readers, **kw)
    _same(host, dev)
    r = host.results
    assert int(r[5]['flags']) & emulate._lib.NFC_EMU_PAIR_CUT_FRAMES and int(r[5]['n_frames']) > 20 and len(host.transcript(5)) == 20
    assert all(int(r[k]['n_frames']) == 38 for k in range(65) if k % 4 == 1)                      # every Ultralight: two rounds of 19
    assert len({int(v) for v in r['n_frames']}) > 3 and len({host.plain[k].tobytes() for k in range(65)}) == 65   # K DIFFERENT cards
    if link == emulate.NFC_EMU_LINK_AIR:
        assert any(int(f) & emulate._lib.NFC_EMU_FRAME_ENCRYPTED for f in host.frames[2]['flags'])


# ---- replay on the device: a stream that answers (nfc_multi_emulate, k_multi_commands_emu) against its twin nfc_host_emulate ----
def _reader_side_streams():
    """the 24-frame Classic capture of tests/test_commands.py and the Ultralight transaction, reader side only (what a tag hears), as IQ"""
    from usrp_nfc_amd import synth
    classic = [f for f in synth.frames_from_trace(os.path.join(GOLD, '1k_with_enc.out'))[0][:24] if f[0] == synth.READER]
    ul = synth.txn_frames(directions=(synth.READER,))
    return [synth.iq_from_profile(synth.modulation_profile(fr)) for fr in (classic, ul)] + [np.zeros(0, np.float32)]


def _replay_cards():
    tag_1k = emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_classic1k.json'), CARD)[0]
    tag_ul, reader = emulate.cards_from_json(os.path.join(GOLD, 'fx_emu_ultralight.json'), CARD)
    return [tag_1k, tag_ul, reader]   # roles tag, tag, reader


def _state_bytes(st):
    return bytes(bytearray(st))


def _push_pieces(m, streams, cuts):
    """push the streams cut at cuts[k] (sample positions), fetch after every push -> per stream the answers' bit lists, in order, and
    per push the (commands, answers) fetched"""
    from usrp_nfc_amd import api  # noqa: F401
    bits, fetched = [[] for _ in streams], []
    edges = [[0] + list(c) + [len(s) // 2] for s, c in zip(streams, cuts)]
    for p in range(max(len(e) for e in edges) - 1):
        m.push([s[2 * e[p]:2 * e[p + 1]] if p + 1 < len(e) else s[:0] for s, e in zip(streams, edges)])
        cm, an = m.fetch_commands(), m.fetch_answers()
        fetched.append((cm, an))
        for k in range(len(streams)):
            bits[k] += [an.bits(k, i) for i in range(int(an.n[k]))]
    return bits, fetched


@pytest.mark.gpu
def test_streams_that_answer_equal_the_replay_twin_whole_and_in_pieces():
    import ctypes
    from usrp_nfc_amd import _lib, api, fsm, synth
    streams, cards = _reader_side_streams(), _replay_cards()
    max_push = max(len(s) for s in streams) // 2

    def context():
        m = api.NfcMultiContext(3, max_push, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32, lib_path=_lib.hooks_path())
        m.emulate(cards)
        return m

    with context() as m:
        guards = m.L.nfc_debug_multi_guards
        guards.argtypes = [ctypes.c_void_p]
        whole_bits, [(cm, an)] = _push_pieces(m, streams, [[], [], []])
        assert guards(m.h) == 0   # the answers' sections included
        assert an.emulated and an.n.tolist() == [12, 9, 0] and an.n_answers == 21
        again = m.fetch_answers()   # the same data, nothing fetched again
        assert again.records.tobytes() == an.records.tobytes() and again.air.tobytes() == an.air.tobytes() and again.n.tolist() == an.n.tolist()
        # what the tag answers is what the real tag of the trace sent next: ciphertext, ninth bits, the nested nonce included
        frames = synth.frames_from_trace(os.path.join(GOLD, '1k_with_enc.out'))[0][:24]
        assert whole_bits[0] == [frames[i + 1][1] for i in range(23) if frames[i][0] == synth.READER and frames[i + 1][0] == synth.TAG]
        assert whole_bits[1] == [b for d, b in synth.txn_frames() if d == synth.TAG]
        cut_at = {}
        for k in range(3):   # the twin, stream by stream, on the very frames the push assembled
            raw = cm.raw.frames_of(k)
            est, fst = emulate.state_init(), fsm.state_init()
            (t, d, e), want = emulate.host_emulate(cards[k], est, fst, raw)
            got_t, got_d, got_e = cm.commands_of(k)
            assert got_t.tobytes() == t.tobytes() and got_d.tobytes() == d.tobytes() and got_e.tobytes() == e.tobytes()
            rec, plain, air, par = an.answers_of(k)
            assert rec.tobytes() == want.records.tobytes()
            n = 18 * len(rec)
            assert plain.tobytes() == want.plain[:n].tobytes() and air.tobytes() == want.air[:n].tobytes() and par.tobytes() == want.par[:n].tobytes()
            assert _state_bytes(m.fsm_state(k)) == _state_bytes(fst) and _state_bytes(m.emu_state(k)) == _state_bytes(est)
            cut_at[k] = raw.table['idx'].astype(np.int64)
        # in pieces: cut behind the AUTHA (before the nonce it asks for is used) and behind {nr}{ar} (before {at} would be heard)
        names = [c for c in cm.commands_of(0)[0]['cmd'].tolist()]
        auth, nrar = names.index(14), names.index(17)
        cuts = [[int(cut_at[0][auth]) + 60, int(cut_at[0][nrar]) + 60], [int(cut_at[1][2]) + 60], []]
        m.reset()
        assert _state_bytes(m.emu_state(0)) == _state_bytes(emulate.state_init())   # reset returns the emulator to its initial state
        piece_bits, fetched = _push_pieces(m, streams, cuts)
        assert piece_bits == whole_bits and len(fetched) == 3
        assert guards(m.h) == 0
        # a state handed over: stream 2 (a reader that heard nothing) takes stream 0's emulator
        m.set_emu_state(2, m.emu_state(0))
        assert _state_bytes(m.emu_state(2)) == _state_bytes(m.emu_state(0))
        m.emulate(None, 0)   # the card taken away: the stream decodes on and answers nothing
        m.reset()
        m.push(streams)
        an2 = m.fetch_answers()
        assert an2.n.tolist() == [0, 9, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('touched', [False, True])
def test_tracked_context_without_a_card_is_untouched(touched):
    # the digests were recorded from the host twin over the traces' own frames (tests/golden/emu_untouched.json): a tracked push with no
    # card -- in a context that never emulated, and in one that was given cards and had them taken away again -- gives those commands
    import json
    from tests import fsm_digests, test_commands
    from usrp_nfc_amd import api
    want = json.load(open(os.path.join(GOLD, 'emu_untouched.json')))
    streams = test_commands.three_streams()[:2]
    with api.NfcMultiContext(2, max(len(s) for s in streams) // 2, hi_val=1.1, input_kind=api.NFC_IN_IQ_F32) as m:
        m.track_commands()
        if touched:
            m.emulate(_replay_cards()[:2])
            m.emulate(None)
        m.push(streams)
        cm = m.fetch_commands()
        assert cm.n_launches == 3 and int(m.stats().n_launches) == 4
        assert not m.fetch_answers().emulated
        got = [fsm_digests.row_digest(*cm.commands_of(k), _state_bytes(m.fsm_state(k))) for k in range(2)]
    assert got == [want['classic24'], want['ultralight']]


@pytest.mark.gpu
def test_decode_many_attaches_every_file_s_answers(tmp_path):
    import io
    from usrp_nfc_amd import decoder, fsm, synth
    streams, cards = _reader_side_streams()[:2], _replay_cards()[:2]
    paths = []
    for name, iq in zip(('classic.fc32', 'ultralight.fc32'), streams):
        paths.append(str(tmp_path / name))
        np.asarray(iq, np.float32).tofile(paths[-1])
    quiet = lambda: fsm.fsm(out=io.StringIO())
    backs = decoder.decode_many(paths, fsm_factory=quiet, max_push_samples=15000, tag=False, emulate=cards)   # several pushes per file
    plain = decoder.decode_many(paths, fsm_factory=quiet, max_push_samples=15000, tag=False)
    assert not hasattr(plain[0], 'answers') and [b.packets for b in backs] == [b.packets for b in plain]
    frames = synth.frames_from_trace(os.path.join(GOLD, '1k_with_enc.out'))[0][:24]
    want = [[f[1] for f in frames if f[0] == synth.TAG], [b for d, b in synth.txn_frames() if d == synth.TAG]]
    for b, w in zip(backs, want):
        got = []
        for rec, _, air, par in b.answers:
            for r in rec:
                o, n = int(r['byte_off']), int(r['n_bytes'])
                got.append([bit for v, q in zip(air[o:o + n].tolist(), par[o:o + n].tolist()) for bit in [(v >> j) & 1 for j in range(8)] + [q & 1]])
        assert got == w
    with pytest.raises(ValueError, match='emulate'):
        decoder.decode_many(paths, emulate=cards[:1])
