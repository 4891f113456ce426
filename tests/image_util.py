"""Helpers of the memory-image tests (tests/test_images_host.py, tests/test_images.py; not collected by pytest): hand-made command
lists, the cards of the closed loop, and an independent statement in numpy of what a transcript showed of a card."""
import numpy as np

from usrp_nfc_amd import _lib, emulate, fsm
from usrp_nfc_amd.command import CommandType

AR_OK, AT_OK, ENC = fsm.FRAME_AR_OK, fsm.FRAME_AT_OK, fsm.FRAME_ENCRYPTED


def commands(rows):
    """rows of (command name or a negative NFC_CMD_*, extra bytes, flags) -> (FRAME_DTYPE table, data): records as the machine writes them
    -- header | extra | CRC in the slot, the header and CRC bytes filled with 0xEE, which the image never reads."""
    t = np.zeros(len(rows), fsm.FRAME_DTYPE)
    data = []
    for i, row in enumerate(rows):
        name, extra = row[0], list(row[1])
        flags = row[2] if len(row) > 2 else 0
        if isinstance(name, int):
            t[i] = (name, 0, len(data), len(extra) if name == fsm.NFC_CMD_UNKNOWN else 0, 0, len(extra) if name == fsm.NFC_CMD_UNKNOWN else 0, 0, flags, 0, 0)
            data += extra
            continue
        c = getattr(CommandType, name)
        nh, ncrc = len(c.header()), 2 if c.needs_crc() else 0
        t[i] = (c.index, c.packet_type(), len(data), nh + len(extra) + ncrc, nh, len(extra), ncrc, flags, 0, 0)
        data += [0xEE] * nh + extra + [0xEE] * ncrc
    return t, np.array(data, np.uint8)


def auth(block, key_b=False, ok=True):
    """the four commands of an authentication that the machine verified (ok) or not"""
    return [('AUTHB' if key_b else 'AUTHA', [block]), ('RANDTA', [1, 2, 3, 4]), ('RANDRB', [0] * 8, ENC | (AR_OK if ok else fsm.FRAME_AR_ERROR)),
            ('RANDTB', [5, 6, 7, 8], ENC | (AT_OK if ok else fsm.FRAME_AT_ERROR))]


def classic_mem(seed, trailers=None):
    """A Classic 1K's memory: random data blocks, a consistent UID, every trailer key A | FF 07 80 69 | key B with random keys;
    trailers: sector -> the four access bytes in its place."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mem = rng.integers(0, 256, 1024).astype(np.uint8)
    mem[4] = mem[0] ^ mem[1] ^ mem[2] ^ mem[3]
    for s in range(16):
        mem[(4 * s + 3) * 16 + 6:(4 * s + 3) * 16 + 10] = (trailers or {}).get(s, [0xFF, 0x07, 0x80, 0x69])
    return mem


def ultralight_mem(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    mem = rng.integers(0, 256, 64).astype(np.uint8)
    mem[3] = 0x88 ^ mem[0] ^ mem[1] ^ mem[2]
    mem[8] = mem[4] ^ mem[5] ^ mem[6] ^ mem[7]
    return mem


def key_a_table(mem):
    """(key_type, sector) -> key A of every sector's trailer: what a reader that knows the card holds"""
    return {(0x60, s): bytes(bytearray(mem[(4 * s + 3) * 16:(4 * s + 3) * 16 + 6].tolist())) for s in range(16)}


def reader_for(mem, seed=1):
    return emulate.reader_card(emulate.drawn_rands(seed), table=key_a_table(mem))


def shown(table, data, tag_type):
    """What the plain records of a transcript showed, stated without the image's text: -> (mask, values) over 1 024 bytes for every byte
    an anticollision answer or a READT behind a READR carried, a trailer's bytes [6, 10) and, where its access bits show key B, [10, 16);
    and the list of (key_type, sector) of every authentication that ended in AT_OK."""
    idx = {n: getattr(CommandType, n).index for n in ('ANTI1U', 'ANTI1G', 'ANTI2T', 'READR', 'READT', 'AUTHA', 'AUTHB', 'RANDTB')}
    mask, val, auths = np.zeros(1024, bool), np.zeros(1024, np.uint8), []
    last_auth = None
    for i, f in enumerate(table):
        o = int(f['byte_off']) + int(f['n_header'])
        x = data[o:o + int(f['n_extra'])]
        c = int(f['cmd'])
        if c in (idx['AUTHA'], idx['AUTHB']):
            last_auth = (0x60 + (c == idx['AUTHB']), int(x[0]) // 4)
        elif c == idx['RANDTB'] and int(f['flags']) & AT_OK:
            auths.append(last_auth)
        elif c == idx['ANTI1U']:
            mask[0:4], val[0:4] = True, x[:4]
        elif c == idx['ANTI1G']:
            mask[0:5], val[0:5] = True, x[:5]
        elif c == idx['ANTI2T']:
            mask[4:9], val[4:9] = True, x[:5]
        elif c == idx['READT'] and i and int(table[i - 1]['cmd']) == idx['READR']:
            p = table[i - 1]
            b = int(data[int(p['byte_off']) + int(p['n_header'])])
            if tag_type == 0:
                for j in range(16):
                    a = ((b + j // 4) % 16) * 4 + j % 4
                    mask[a], val[a] = True, x[j]
            elif b % 4 != 3:
                mask[16 * b:16 * b + 16], val[16 * b:16 * b + 16] = True, x
            else:
                c1 = (int(x[7]) >> 7) & 1   # the trailer's own condition bits C1 C2 C3 (block 3 of the sector)
                c2, c3 = (int(x[8]) >> 3) & 1, (int(x[8]) >> 7) & 1
                end = 16 if (c1 << 2 | c2 << 1 | c3) <= 2 else 10
                mask[16 * b + 6:16 * b + end], val[16 * b + 6:16 * b + end] = True, x[6:end]
    return mask, val, auths


def transcript_commands(tr, table=None, keys=None):
    """A transcript as the eavesdropper's machine decodes it on the CPU -> (FRAME_DTYPE table, data)."""
    st = fsm.state_init()
    if keys is not None:
        for i in range(6):
            st.key_a[i], st.key_b[i] = keys[0][i], keys[1][i]
    t, d, _ = fsm.host_commands(st, tr.nfc_frames(), sector_keys=table)
    return t, d


def images_equal(fetched, k, image):
    """stream k of an api.NfcMultiImages against an emulate.CardImage, byte for byte: mem, src, info and tail"""
    return fetched.image(k).rec.tobytes() == image.rec.tobytes()


IMG_FLAGS = dict(TAG_CHANGED=_lib.NFC_IMG_TAG_CHANGED, CHANGED=_lib.NFC_IMG_CHANGED, BEYOND=_lib.NFC_IMG_BEYOND, SAW_WRITE=_lib.NFC_IMG_SAW_WRITE)
