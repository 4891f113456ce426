"""The memory image's CPU twin (nfc_host_card_image, emulate.host_card_image; csrc/image.hip.h): every rule of include/nfc_amd.h pinned on
a hand-made command list, the twin over the commands of emulated transactions against an independent statement in numpy, and command
lists cut into two and three calls at every boundary.  No GPU."""
import json

import numpy as np
import pytest

from tests import emu_cards
from tests import image_util as iu
from usrp_nfc_amd import _lib, emulate, fsm

READ, ANTICOLL, KEY = _lib.NFC_IMG_SRC_READ, _lib.NFC_IMG_SRC_ANTICOLL, _lib.NFC_IMG_SRC_KEY
F = iu.IMG_FLAGS
BLOCK = list(range(0x10, 0x20))


def run(rows, keys=None, image=None):
    return emulate.host_card_image(*iu.commands(rows), keys=keys, image=image)


def known(img):
    return np.nonzero(img.src)[0].tolist()


def test_a_fresh_image_knows_nothing():
    img = emulate.CardImage()
    assert img.tag_type == -1 and img.flags == 0 and img.n_known == 0 and not img.src.any() and not img.mem.any()
    assert img.tail['cmd'].tolist() == [-1, -1, -1]
    assert run([]) == img


@pytest.mark.parametrize('name,tag_type', [('ATQAUL', 0), ('ATQA1K', 1), ('ATQA4K', 2), ('ATQADS', 3)])
def test_an_atqa_sets_the_tag_type(name, tag_type):
    img = run([(name, [])])
    assert img.tag_type == tag_type and img.flags == 0 and img.n_known == 0


def test_tag_changed_only_when_another_type_was_set():
    assert run([('ATQA1K', []), ('REQA', []), ('ATQA1K', [])]).flags == 0
    img = run([('ATQA1K', []), ('REQA', []), ('ATQAUL', [])])
    assert img.flags == F['TAG_CHANGED'] and img.tag_type == 0


def test_anticollision_answers_patch_what_a_tag_sends():
    img = run([('ANTI1U', [1, 2, 3, 4])])
    assert known(img) == [0, 1, 2, 3] and img.mem[:4].tolist() == [1, 2, 3, 4] and set(img.src[:4]) == {ANTICOLL}
    img = run([('ANTI2T', [5, 6, 7, 8, 9])])
    assert known(img) == [4, 5, 6, 7, 8] and img.mem[4:9].tolist() == [5, 6, 7, 8, 9]
    img = run([('ANTI1G', [1, 2, 3, 4, 5])])
    assert known(img) == [0, 1, 2, 3, 4] and img.mem[:5].tolist() == [1, 2, 3, 4, 5] and img.n_known == 5


def test_a_data_block_is_taken_whole():
    img = run([('ATQA1K', []), ('READR', [9]), ('READT', BLOCK)])
    assert known(img) == list(range(144, 160)) and img.mem[144:160].tolist() == BLOCK and set(img.src[144:160]) == {READ} and img.flags == 0


def test_a_readt_not_preceded_by_a_readr_patches_nothing():
    assert run([('ATQA1K', []), ('READT', BLOCK)]).n_known == 0
    assert run([('ATQA1K', []), ('READR', [9]), ('HALT', []), ('READT', BLOCK)]).n_known == 0
    # a frame the machine did not know, a parity error and a cut frame still count as the command before
    for bad in (fsm.NFC_CMD_UNKNOWN, fsm.NFC_CMD_PARITY_ERROR, _lib.NFC_CMD_CUT):
        assert run([('ATQA1K', []), ('READR', [9]), (bad, [1, 2, 3] if bad == -1 else []), ('READT', BLOCK)]).n_known == 0


@pytest.mark.parametrize('conds,key_b_shown', [(0, True), (1, True), (2, True), (3, False), (4, False), (5, False), (6, False), (7, False)])
def test_trailer_rule_under_both_access_settings(conds, key_b_shown):
    """[0, 6) is never taken (a card reads key A as zeros), [6, 10) always, [10, 16) only where THIS answer's access bits show key B"""
    answer = [0] * 6 + emu_cards.access([0, 0, 0, conds]) + [0xB0 + i for i in range(6)]
    img = run([('ATQA1K', []), ('READR', [7]), ('READT', answer)])
    want = list(range(7 * 16 + 6, 7 * 16 + (16 if key_b_shown else 10)))
    assert known(img) == want and img.mem[want].tolist() == answer[6:6 + len(want)]


def test_ultralight_wrap_at_page_14():
    img = run([('ATQAUL', []), ('READR', [14]), ('READT', BLOCK)])
    assert known(img) == list(range(0, 8)) + list(range(56, 64))
    assert img.mem[56:64].tolist() == BLOCK[:8] and img.mem[0:8].tolist() == BLOCK[8:]
    assert run([('ATQAUL', []), ('READR', [0x10]), ('READT', BLOCK)]).n_known == 0   # val > 0x0F: nothing, and no flag
    assert run([('ATQAUL', []), ('READR', [0x10]), ('READT', BLOCK)]).flags == 0


def test_beyond():
    img = run([('ATQA1K', []), ('READR', [64]), ('READT', BLOCK)])
    assert img.n_known == 0 and img.flags == F['BEYOND']
    img = run([('ATQA1K', [])] + iu.auth(64))   # sector 16
    assert img.n_known == 0 and img.flags == F['BEYOND']


@pytest.mark.parametrize('rows', [[('WRITE', [4, 1, 2, 3, 4])], [('COMPW1', [4])], [('COMPW2', BLOCK)]])
def test_saw_write(rows):
    img = run([('ATQA1K', [])] + rows)
    assert img.n_known == 0 and img.flags == F['SAW_WRITE']


def test_changed_and_last_wins():
    other = [b ^ 0xFF for b in BLOCK]
    same = run([('ATQA1K', []), ('READR', [9]), ('READT', BLOCK), ('READR', [9]), ('READT', BLOCK)])
    assert same.flags == 0
    img = run([('ATQA1K', []), ('READR', [9]), ('READT', BLOCK), ('READR', [9]), ('READT', other)])
    assert img.flags == F['CHANGED'] and img.mem[144:160].tolist() == other and img.n_known == 16


def test_an_authentication_proves_the_key_the_machine_held():
    ka, kb = [0xA0 + i for i in range(6)], [0xB0 + i for i in range(6)]
    t5 = [0x50 + i for i in range(6)]
    keys = (ka, kb, {(0x60, 5): t5})
    img = run([('ATQA1K', [])] + iu.auth(4), keys=keys)   # sector 1: no slot, key A
    assert known(img) == list(range(112, 118)) and img.mem[112:118].tolist() == ka and set(img.src[112:118]) == {KEY}
    img = run(iu.auth(22), keys=keys)                      # sector 5: the table's slot
    assert img.mem[23 * 16:23 * 16 + 6].tolist() == t5 and img.n_known == 6
    img = run(iu.auth(22, key_b=True), keys=keys)          # key B: no slot of that type
    assert known(img) == list(range(23 * 16 + 10, 23 * 16 + 16)) and img.mem[23 * 16 + 10:23 * 16 + 16].tolist() == kb
    # a nested authentication's frames carry ENCRYPTED on every record: it counts as well
    nested = [(n, x, (f[0] if f else 0) | iu.ENC) for n, x, *f in iu.auth(8)]
    assert run(nested, keys=keys).n_known == 6
    # not proven: AT not OK, AR not OK, another command inside the chain
    assert run(iu.auth(4, ok=False), keys=keys).n_known == 0
    rows = iu.auth(4)
    rows[2] = ('RANDRB', [0] * 8, iu.ENC | fsm.FRAME_AR_ERROR)
    assert run(rows, keys=keys).n_known == 0
    rows = iu.auth(4)
    rows.insert(2, (fsm.NFC_CMD_UNKNOWN, [1]))
    assert run(rows, keys=keys).n_known == 0


def test_a_key_and_a_trailer_read_fill_one_trailer():
    ka = [0xA0 + i for i in range(6)]
    answer = [0] * 6 + [0xFF, 0x07, 0x80, 0x69] + [0xB0 + i for i in range(6)]
    img = run([('ATQA1K', [])] + iu.auth(4) + [('READR', [7]), ('READT', answer)], keys=(ka, ka))
    assert img.mem[112:128].tolist() == ka + answer[6:] and img.flags == 0
    assert img.src[112:128].tolist() == [KEY] * 6 + [READ] * 10


def test_arguments_are_checked():
    t, d = iu.commands([('ATQA1K', []), ('READR', [9]), ('READT', BLOCK)])
    with pytest.raises(ValueError):
        emulate.host_card_image(t, d[:-4])          # the READT's bytes lie outside data
    with pytest.raises(ValueError):
        emulate.host_card_image(t, d, keys=([1] * 5, [1] * 6))
    for field, value in (('tag_type', 4), ('flags', 16), ('n_known', 1), ('reserved', 1)):
        img = emulate.CardImage()
        img.rec['info'][field] = value
        with pytest.raises(ValueError):
            emulate.host_card_image(t, d, image=img)
    img = emulate.CardImage()
    img.rec['src'][5] = 4
    with pytest.raises(ValueError):
        emulate.host_card_image(t, d, image=img)
    L = _lib.load()
    assert L.nfc_card_image_init(None) == -1 and L.nfc_host_card_image(None, None, 0, None, 0, None, None, None) == -1


# ---- the twin over emulated transactions ----
def cards():
    out = []
    for seed in range(emu_cards.N_TAG_ROWS):
        tag_type, mem, rands, _ = emu_cards.tag_row(seed)
        out.append((tag_type, np.array(mem, np.uint8), rands))
    return out


def test_twin_over_the_cards_of_emu_cards():
    """Every card of tests/emu_cards.py read in CARD mode by a reader that holds its key A table.  What the image knows is exactly what
    the transcript showed, and equals the card there; every authenticated sector's key A sits in its trailer with source KEY."""
    cs = cards()
    tags = [emulate.tag_card(t, m, r or None) for t, m, r in cs]
    readers = [emulate.reader_card(emulate.drawn_rands(seed + 1), table=iu.key_a_table(m) if t else None) for seed, (t, m, r) in enumerate(cs)]
    trs = emulate.pairs_host(tags, readers)
    n_auth = n_ul = 0
    for k, (tag_type, mem, _) in enumerate(cs):
        table = iu.key_a_table(mem) if tag_type else None
        t, d = iu.transcript_commands(trs.transcript(k), table)
        img = emulate.host_card_image(t, d, keys=((0xFF,) * 6, (0xFF,) * 6, table))
        mask, val, auths = iu.shown(t, d, tag_type)
        full = np.zeros(1024, np.uint8)
        full[:len(mem)] = mem
        assert (val[mask] == full[mask]).all(), k            # (the statement itself: a card shows its memory)
        keys_at = np.zeros(1024, bool)
        for key_type, sector in auths:
            assert key_type == 0x60
            keys_at[(4 * sector + 3) * 16:(4 * sector + 3) * 16 + 6] = True
        assert ((img.src != 0) == (mask | keys_at)).all(), k   # nothing is known that the transcript never showed
        assert (img.mem[mask | keys_at] == full[mask | keys_at]).all(), k
        assert (img.src[keys_at] == KEY).all() and (img.src[mask & ~keys_at] != KEY).all(), k
        assert img.n_known == int((mask | keys_at).sum()) and img.tag_type == tag_type and not img.flags & ~F['CHANGED'], k
        assert auths or tag_type == 0, k   # (a reader that holds the card's keys gets through its first authentication at least)
        n_auth += len(auths)
        n_ul += tag_type == 0
    assert n_auth >= len(cs) - n_ul and n_ul == len(cs) // 6   # (both tag types are there: tag_row makes every sixth an Ultralight)


# ---- cuts ----
def _cut_case():
    mem = iu.classic_mem(7, {2: emu_cards.access([0, 0, 0, 3])})
    tr = emulate.pairs_host([emulate.tag_card(1, mem, emulate.drawn_rands(0))], [iu.reader_for(mem)]).transcript(0)
    table = iu.key_a_table(mem)
    t, d = iu.transcript_commands(tr, table)
    return t, d, ((0xFF,) * 6, (0xFF,) * 6, table)


def _pieces(t, d, cuts, keys):
    img = emulate.CardImage()
    for a, b in zip((0,) + cuts, cuts + (len(t),)):
        emulate.host_card_image(t[a:b], d, keys=keys, image=img)   # (byte_off stays relative to the whole data)
    return img


def test_two_calls_cut_at_every_boundary():
    t, d, keys = _cut_case()
    whole = emulate.host_card_image(t, d, keys=keys)
    assert whole.n_known > 900 and len(t) == 199
    for c in range(len(t) + 1):
        assert _pieces(t, d, (c,), keys) == whole, c


def test_three_calls_cut_at_every_boundary():
    """every pair of cuts a <= b over the 199 commands: 20 100 runs of three calls"""
    t, d, keys = _cut_case()
    whole = emulate.host_card_image(t, d, keys=keys).rec.tobytes()
    for a in range(len(t) + 1):
        for b in range(a, len(t) + 1):
            assert _pieces(t, d, (a, b), keys).rec.tobytes() == whole, (a, b)


def test_card_and_json_round_trip(tmp_path):
    t, d, keys = _cut_case()
    img = emulate.host_card_image(t, d, keys=keys)
    card = img.card(rands=emulate.drawn_rands(0))
    assert card.tag_type == 1 and card.mem.tolist() == img.mem.tolist()
    path = img.to_json(str(tmp_path / 'card.json'), rands=emulate.drawn_rands(0))
    assert json.load(open(path))[0]['mem'] == img.mem.tolist()
    tag, _ = emulate.cards_from_json(path)
    assert tag.mem.tolist() == img.mem.tolist() and tag.tag_type == 1
    ul = run([('ATQAUL', []), ('READR', [0]), ('READT', BLOCK)])
    assert ul.card().tag_type == 0 and len(ul.card().mem) == 64 and ul.entries()[0]['type'] == 'ULTRALIGHT'
    from usrp_nfc_amd.parser import Parser
    assert Parser(path).get_tag(None) is not None


def test_the_clone_answers_the_reader_as_the_card_did():
    """the twin's image alone, emulated against the same reader, gives the original's transcript: the premise of the closed loop on the GPU"""
    for mem, tag_type in ((iu.classic_mem(11), 1), (iu.ultralight_mem(12), 0), (iu.classic_mem(13, {5: emu_cards.access([0, 0, 0, 3])}), 1)):
        rands = emulate.drawn_rands(0) if tag_type else None
        reader = iu.reader_for(mem) if tag_type else emulate.reader_card(emulate.drawn_rands(1))
        table = iu.key_a_table(mem) if tag_type else None
        first = emulate.pairs_host([emulate.tag_card(tag_type, mem, rands)], [reader])
        t, d = iu.transcript_commands(first.transcript(0), table)
        img = emulate.host_card_image(t, d, keys=((0xFF,) * 6, (0xFF,) * 6, table))
        again = emulate.pairs_host([img.card(rands=rands)], [reader])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first.arrays(), again.arrays())), tag_type
