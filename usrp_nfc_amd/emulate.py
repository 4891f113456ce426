"""Emulated tags and readers (include/nfc_amd.h: nfc_emu_*, csrc/emu.hip.h): the reference's tag.py and reader.py as two
machines, and its closed loop (usrp_nfc.py:116-136) for K (tag, reader) pairs at once -- on the GPU a lane per pair (``pairs_device``),
on one CPU core its twin (``pairs_host``).  Both return a ``Transcripts``: per pair every frame that went on the air, plain and as sent.

A card is made with ``tag_card`` / ``reader_card`` (or ``cards_from_json`` from one of the reference's JSON files) and carries its mode:
NFC_EMU_REFERENCE is the reference with its quirks, NFC_EMU_CARD what a MIFARE Classic does where the reference differs.  ``step`` is one
machine's answer to one heard command, on the host.  There is no fall-back from the GPU call to the host twin."""
import ctypes as C
import json
import random
import time

import numpy as np

from . import _lib
from . import keys as _keys
from ._lib import (EMU_FRAME_DTYPE, EMU_RESULT_DTYPE, NFC_EMU_CARD, NFC_EMU_LINK_AIR, NFC_EMU_LINK_PLAIN, NFC_EMU_READER,  # noqa: F401
                   NFC_EMU_REFERENCE, NFC_EMU_TAG)

ULTRALIGHT, CLASSIC1K = 0, 1


class EmulationError(RuntimeError):
    pass


def _fail(name, rc):
    msg = _lib.load().nfc_emu_last_error()
    text = '%s status %d: %s' % (name, rc, (msg or b'').decode())
    raise (ValueError if rc == -1 else EmulationError)(text)


class Card(object):
    """What a machine emulates (nfc_emu_card).  Keeps its arrays alive for as long as its C structure is in use."""

    def __init__(self, role, tag_type=CLASSIC1K, mode=NFC_EMU_CARD, mem=None, rands=None, key_a=(0xFF,) * 6, key_b=(0xFF,) * 6, table=None):
        self.role, self.tag_type, self.mode = int(role), int(tag_type), int(mode)
        self.mem = np.ascontiguousarray([] if mem is None else mem, np.uint8).reshape(-1)
        r = np.ascontiguousarray([] if rands is None else rands, np.uint8)
        if r.size % 4:
            raise ValueError('rands: every nonce is four bytes')
        self.rands = r.reshape(-1, 4)
        self.key_a, self.key_b = list(bytearray(key_a)), list(bytearray(key_b))
        if len(self.key_a) != 6 or len(self.key_b) != 6:
            raise ValueError('key_a / key_b: a key is six bytes')
        self.table = None if table is None else _keys.key_table(table)

    def struct(self):
        """the nfc_emu_card over this object's arrays (made once: a card is not changed after it is made)"""
        if getattr(self, '_c', None) is not None:
            return self._c
        c = self._c = _lib.EmuCard()
        c.role, c.tag_type, c.mode, c.mem_len = self.role, self.tag_type, self.mode, self.mem.size
        c.mem = self.mem.ctypes.data if self.mem.size else None
        c.rands = self.rands.ctypes.data if self.rands.size else None
        c.n_rands = len(self.rands)
        for i in range(6):
            c.key_a[i], c.key_b[i] = self.key_a[i], self.key_b[i]
        c.table = C.addressof(self.table) if self.table is not None else None
        return c


def tag_card(tag_type, mem, rands=None, mode=NFC_EMU_CARD):
    """A tag: tag_type ULTRALIGHT (64 bytes of memory) or CLASSIC1K (1024 bytes and 1 .. 64 four-byte nonces)."""
    return Card(NFC_EMU_TAG, tag_type, mode, mem, rands)


def reader_card(rands, key_a=(0xFF,) * 6, key_b=(0xFF,) * 6, table=None, mode=NFC_EMU_CARD):
    """A reader: 1 .. 64 four-byte nonces, its two keys and (CARD mode) a sector key table as keys.key_table takes it."""
    return Card(NFC_EMU_READER, CLASSIC1K, mode, None, rands, key_a, key_b, table)


def drawn_rands(seed=0, n=16):
    """What stands in for the reference's `random` fallback (rand.py:33-40, Rand(None)): n four-byte nonces drawn ONCE from a generator
    seeded with `seed`.  A stated deviation: the reference reseeds on every reset, so its sequence repeats too, but from the clock."""
    rng = random.Random(seed)
    return [[rng.randint(0, 255) for _ in range(4)] for _ in range(n)]


def cards_from_json(source, mode=NFC_EMU_CARD, seed=0):
    """(tag, reader) from one of the reference's card files (parser.py:12-59: a list of entries, `entry` tag / reader; `type`, `mem`, `rands`
    for a tag, `rands`, `keya`, `keyb` for a reader), a path or the parsed list.  As Parser does it: without a reader entry the reader
    has the default keys, without a tag entry the tag is Tag.generate_1k's card; nonces that are missing are drawn_rands(seed)."""
    ar = source if isinstance(source, list) else json.load(open(source))
    tag_d = next((d for d in ar if d.get('entry', '') == 'tag'), None)
    reader_d = next((d for d in ar if d.get('entry', '') == 'reader'), {})
    if tag_d is None:
        tag = tag_card(CLASSIC1K, generate_1k(), drawn_rands(seed), mode)
    else:
        ul = tag_d.get('type', '') == 'ULTRALIGHT'
        tag = tag_card(ULTRALIGHT if ul else CLASSIC1K, tag_d.get('mem', []), tag_d.get('rands') or (None if ul else drawn_rands(seed)), mode)
    reader = reader_card(reader_d.get('rands') or drawn_rands(seed + 1), reader_d.get('keya') or (0xFF,) * 6, reader_d.get('keyb') or (0xFF,) * 6, None, mode)
    return tag, reader


def generate_1k():
    """Tag.generate_1k (tag.py:34-49): the memory of a blank Classic 1K with the reference card's manufacturer block."""
    zero, trailer = [0x00] * 16, [0xFF] * 6 + [0xFF, 0x07, 0x80, 0x69] + [0xFF] * 6
    block0 = [0xCD, 0x76, 0x92, 0x74, 0x5D, 0x88, 0x04, 0x00, 0x85, 0x00, 0x00, 0x00, 0x04, 0x13, 0x45, 0x01]
    return block0 + zero * 2 + trailer + (zero * 3 + trailer) * 15


class CardImage(object):
    """A card as it was heard (nfc_card_image; include/nfc_amd.h says how commands patch it): `rec`, one CARD_IMAGE_DTYPE record.  mem / src:
    views of its 1 024 bytes and their source codes (0: never shown); tag_type (-1: no ATQA heard), flags (NFC_IMG_*), n_known; tail: the
    summaries of the stream's last three commands, with which a later call continues mid-chain."""

    def __init__(self, rec=None):
        if rec is None:
            rec = np.zeros((), _lib.CARD_IMAGE_DTYPE)
            if _lib.load().nfc_card_image_init(rec.ctypes.data) != 0:
                raise EmulationError('nfc_card_image_init failed')
        self.rec = np.array(rec, _lib.CARD_IMAGE_DTYPE).reshape(())

    mem = property(lambda self: self.rec['mem'])
    src = property(lambda self: self.rec['src'])
    tail = property(lambda self: self.rec['tail'])
    tag_type = property(lambda self: int(self.rec['info']['tag_type']))
    flags = property(lambda self: int(self.rec['info']['flags']))
    n_known = property(lambda self: int(self.rec['info']['n_known']))

    def copy(self):
        return CardImage(self.rec.copy())

    def __eq__(self, other):
        return isinstance(other, CardImage) and self.rec.tobytes() == other.rec.tobytes()

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def known_mask(self):
        return self.src != 0

    def size(self):
        """bytes of the card's memory: 64 for an Ultralight, else 1 024"""
        return 64 if self.tag_type == ULTRALIGHT else _lib.NFC_IMG_BYTES

    def card(self, rands=None, mode=NFC_EMU_CARD):
        """The image as a tag to emulate (tag_card), unknown bytes as zeros; a Classic without `rands` gets drawn_rands()."""
        ul = self.tag_type == ULTRALIGHT
        return tag_card(ULTRALIGHT if ul else CLASSIC1K, self.mem[:self.size()].copy(), rands if (rands is not None or ul) else drawn_rands(), mode)

    def entries(self, rands=None):
        """The image as the entries of one of the reference's card files (parser.Parser reads them, create_json writes them)."""
        tag = {'entry': 'tag', 'type': 'ULTRALIGHT' if self.tag_type == ULTRALIGHT else 'CLASSIC1K', 'mem': self.mem[:self.size()].tolist()}
        if rands is not None:
            tag['rands'] = [list(map(int, r)) for r in rands]
        return [tag]

    def to_json(self, path, rands=None):
        with open(path, 'w') as f:
            json.dump(self.entries(rands), f)
        return path


def host_card_image(commands, data, keys=None, image=None):
    """The CPU twin of the image kernel (nfc_host_card_image): a stream's command records (fsm.FRAME_DTYPE, as fsm.host_commands and
    NfcMultiCommands.commands_of give them) and their data advance `image` in place (None: a fresh CardImage) -> the image.
    keys: (key_a, key_b) or (key_a, key_b, table) -- the machine's two keys and its sector table, as decode_many takes them; None: FF..FF."""
    from . import fsm as _fsm
    img = CardImage() if image is None else image
    t = np.ascontiguousarray(commands, _fsm.FRAME_DTYPE)
    d = np.ascontiguousarray(data, np.uint8).reshape(-1)
    keys = ((0xFF,) * 6, (0xFF,) * 6) if keys is None else keys
    ka, kb = (np.ascontiguousarray(list(bytearray(k)), np.uint8) for k in keys[:2])
    if ka.size != 6 or kb.size != 6:
        raise ValueError('host_card_image: a key is six bytes')
    table = _keys.key_table(keys[2]) if len(keys) > 2 and keys[2] is not None else None
    rc = _lib.load().nfc_host_card_image(img.rec.ctypes.data, t.ctypes.data if len(t) else None, len(t), d.ctypes.data if d.size else None, d.size,
                                         ka.ctypes.data, kb.ctypes.data, None if table is None else C.byref(table))
    if rc != 0:
        raise (ValueError if rc == -1 else EmulationError)('nfc_host_card_image status %d' % rc)
    return img


def state_init():
    st = _lib.EmuState()
    rc = _lib.load().nfc_emu_state_init(C.byref(st))
    if rc != 0:
        _fail('nfc_emu_state_init', rc)
    return st


def step(card, state, cmd, extra=()):
    """One heard command through one machine on the host (nfc_host_emu_step): cmd a command index (command.CommandType.X.index), or -1
    for a frame the protocol machine did not know / -2 for a parity error; `state` an _lib.EmuState, advanced in place.
    -> (answer's command index or None, its plain frame's bytes: header | extra | CRC_A)."""
    e = np.ascontiguousarray(list(extra), np.uint8)
    out, n, cmd_out = np.zeros(18, np.uint8), C.c_size_t(0), C.c_int(0)
    c = card.struct()
    rc = _lib.load().nfc_host_emu_step(C.byref(c), C.byref(state), int(cmd), e.ctypes.data if e.size else None, e.size, C.byref(cmd_out),
                                       out.ctypes.data, C.byref(n))
    if rc != 0:
        _fail('nfc_host_emu_step', rc)
    return (None, []) if cmd_out.value < 0 else (cmd_out.value, out[:n.value].tolist())


class Answers(object):
    """What a replay answered (host_emulate): `records` EMU_ANSWER_DTYPE, `plain` / `air` / `par` indexed by a record's byte_off."""

    def __init__(self, records, plain, air, par):
        self.records, self.plain, self.air, self.par = records, plain, air, par

    def __len__(self):
        return len(self.records)

    def plain_of(self, i):
        r = self.records[i]
        return self.plain[int(r['byte_off']):int(r['byte_off']) + int(r['n_bytes'])]

    def bits(self, i):
        """Answer i as the bit list the reference's emulator hands binary_src.set_bits (what tx.encode takes)."""
        r = self.records[i]
        o, n = int(r['byte_off']), int(r['n_bytes'])
        out = []
        for v, q in zip(self.air[o:o + n].tolist(), self.par[o:o + n].tolist()):
            out += [(v >> j) & 1 for j in range(8)] + [q & 1]
        return out


def host_emulate(card, emu_state, fsm_state, frames, data=None, par=None, sector_keys=None):
    """Replay on the host (nfc_host_emulate): fsm.host_commands with `card`'s emulator behind the machine -- after every command of the
    other side's type the emulator answers, and the answer passes through the same machine's process_outgoing in the card's mode.
    emu_state (an _lib.EmuState) and fsm_state (an _lib.FsmState) are advanced in place.  -> ((table, data, enc), Answers)."""
    from . import fsm as _fsm
    if data is None:
        frames, data, par = frames.table, frames.bytes, frames.par
    t = np.ascontiguousarray(frames, _lib.RAW_FRAME_DTYPE)
    b = [np.ascontiguousarray(a, np.uint8) for a in data]
    p = [np.ascontiguousarray(a, np.uint8) for a in par]
    n, cap = len(t), int(t['n_bytes'].sum()) + 1
    out, buf, enc = np.zeros(n, _fsm.FRAME_DTYPE), np.zeros(cap, np.uint8), np.zeros(cap, np.uint16)
    ans = np.zeros(max(n, 1), _lib.EMU_ANSWER_DTYPE)
    ap, aa, aq = (np.zeros(18 * max(n, 1), np.uint8) for _ in range(3))
    used, n_ans = C.c_size_t(0), C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    keyed = None if sector_keys is None else C.byref(_keys.key_table(sector_keys))
    c = card.struct()
    rc = _lib.load().nfc_host_emulate(C.byref(fsm_state), keyed, C.byref(c), C.byref(emu_state), ptr(t), n, ptr(b[0]), ptr(p[0]), ptr(b[1]), ptr(p[1]),
                                      out.ctypes.data, buf.ctypes.data, enc.ctypes.data, cap, C.byref(used), ans.ctypes.data, ap.ctypes.data,
                                      aa.ctypes.data, aq.ctypes.data, C.byref(n_ans))
    if rc != 0:
        _fail('nfc_host_emulate', rc)
    return (out, buf[:used.value], enc[:used.value]), Answers(ans[:n_ans.value], ap, aa, aq)


def tx_inputs(commands, answers):
    """What fetch_commands() and fetch_answers() brought of one push, as host_transmit takes it: per stream (records, air, par) of its
    answers and, per answer, the idx of the raw frame of the command it answers (commands.raw and commands.src) -> (answers, frames_idx)."""
    out, idx = [], []
    raw = commands.raw
    for k in range(answers.n_streams):
        rec, _, air, par = answers.answers_of(k)
        out.append((rec, air, par))
        if len(rec) == 0:
            idx.append(np.zeros(0, np.uint64))
            continue
        t, i = commands.src_of(k)
        t, i = t[rec['src'].astype(np.int64)], i[rec['src'].astype(np.int64)]
        idx.append(np.array([raw.frames[int(a)][int(raw.frame_off[int(a)][k]) + int(b)]['idx'] for a, b in zip(t, i)], np.uint64))
    return out, idx


def host_transmit(answers, frames_idx, roles, rx_base, rx_n, pending=None, out=None, cap_samples=None, **kw):
    """The CPU twin of NfcMultiContext.transmit (nfc_host_answers_tx), one push of K streams.  answers[k]: (records, air, par) of stream
    k's answers -- records with byte_off and n_bits (EMU_ANSWER_DTYPE: what answers_of(k) and host_emulate's Answers hold), their bytes in
    air / par -- or None; frames_idx[k]: per answer the idx of the answered command's raw frame, in the stream's own sample count;
    roles[k]: NFC_EMU_TAG, NFC_EMU_READER or None (no card); the push gave stream k the samples [rx_base[k], rx_base[k] + rx_n[k]).
    pending: the TX_PENDING_DTYPE array an earlier call returned (None: no stream has a pending answer).  kw: transmit's keywords.
    out: a complex64 array to render into (cap_samples: how much of it the call may use, default all of it); None: one of the needed
    size.  -> (samples, first_sample, n_samples, pending): the layout's complex64 samples and the advanced pending entries."""
    from . import tx
    K = len(roles)
    cfg = kw.pop('cfg', None) or tx.answers_tx_config(**kw)   # (cfg: an _lib.AnswersTxConfig made by hand, in place of the keywords)
    role = np.array([-1 if r is None else int(r) for r in roles], np.int32)
    base, n = np.ascontiguousarray(rx_base, np.uint64), np.ascontiguousarray(rx_n, np.uint32)
    if base.size != K or n.size != K or len(answers) != K or len(frames_idx) != K:
        raise ValueError('host_transmit: one entry per stream in answers, frames_idx, roles, rx_base and rx_n')
    ans_off, byte_base = np.zeros(K + 1, np.uint32), np.zeros(K + 1, np.uint32)
    recs, airs, pars = [], [], []
    for k in range(K):
        rec, air, par = answers[k] if answers[k] is not None else (np.zeros(0, _lib.EMU_ANSWER_DTYPE), [], [])
        air, par = np.ascontiguousarray(air, np.uint8).reshape(-1), np.ascontiguousarray(par, np.uint8).reshape(-1)
        r = np.zeros(len(rec), _lib.TX_ANSWER_DTYPE)
        if len(rec):
            r['idx'], r['byte_off'], r['n_bits'] = np.asarray(frames_idx[k], np.uint64), rec['byte_off'], rec['n_bits']
        recs.append(r), airs.append(air), pars.append(par)
        ans_off[k + 1], byte_base[k + 1] = ans_off[k] + len(r), byte_base[k] + max(air.size, par.size)
        if air.size != par.size:
            raise ValueError('host_transmit: stream %d: air and par differ in length' % k)
    rec = np.concatenate(recs) if K else np.zeros(0, _lib.TX_ANSWER_DTYPE)
    air = np.concatenate(airs + [np.zeros(1, np.uint8)])
    par = np.concatenate(pars + [np.zeros(1, np.uint8)])
    pend = np.zeros(K, _lib.TX_PENDING_DTYPE) if pending is None else np.array(pending, _lib.TX_PENDING_DTYPE)
    if pend.shape != (K,):
        raise ValueError('host_transmit: pending has one entry per stream')
    first, ns = np.zeros(K, np.uint64), np.zeros(K, np.uint32)
    L = _lib.load()
    ptr = lambda a: a.ctypes.data if a.size else None
    call = lambda o, cap: L.nfc_host_answers_tx(C.byref(cfg), K, ptr(role), ptr(base), ptr(n), ans_off.ctypes.data, ptr(rec), air.ctypes.data, par.ctypes.data,
                                                byte_base.ctypes.data, ptr(pend), o, int(cap), ptr(first), ptr(ns))
    rc = call(None, 0)
    if rc != 0:
        _tx_fail(rc, pend)
    need = int(first[-1]) + int(ns[-1]) if K else 0
    if out is None:
        out = np.zeros(max(need, 1), np.complex64)
        cap_samples = need
    elif cap_samples is None:
        cap_samples = out.size
    if out.dtype != np.complex64 or not out.flags['C_CONTIGUOUS'] or cap_samples > out.size:
        raise ValueError('host_transmit: out is a contiguous complex64 array of at least cap_samples entries')
    rc = call(out.ctypes.data, cap_samples)
    if rc != 0:
        _tx_fail(rc, pend)
    return out[:need], first, ns, pend


def _tx_fail(rc, pending):
    msg = _lib.load().nfc_last_error(None)
    e = (ValueError if rc == -1 else EmulationError)('nfc_host_answers_tx status %d: %s' % (rc, (msg or b'').decode()))
    e.pending = pending   # the entries as the failed call left them
    raise e


def synth_frames(transcript):
    """(type, on-air bits) per stored frame: synth.transaction_frames"""
    return [(int(f['type']), transcript.bits(i)) for i, f in enumerate(transcript.frames)]


def frames_of_bits(frames):
    """A list of (type, on-air data bits) -- synth.frames_from_trace, synth.transaction_frames -- as the frames an eavesdropper's decode
    would assemble from it (api.NfcFrames), through the frame assembly's host twin; a short frame with the end bit the framing stage hands
    over behind it.  A frame's idx is its place in the list."""
    from . import api
    recs, data, par = [], [], []
    for t in (0, 1):
        rows, bits = [], []
        for i, (ft, b) in enumerate(frames):
            if int(ft) == t:
                b = list(b) + [0] if len(b) == 7 else list(b)
                rows.append((i, len(bits), len(b), t))
                bits += b
        r, d, p = api.host_frames(np.array(rows, _lib.PACKET_DTYPE), np.array(bits, np.uint8), t)
        recs.append(r), data.append(d), par.append(p)
    return api.NfcFrames(recs, data, par)


class Transcript(object):
    """One pair's transcript: `frames` the stored EMU_FRAME_DTYPE records, `result` its EMU_RESULT_DTYPE record (true counts, flags)."""

    def __init__(self, result, frames, plain, air, par):
        self.result = result
        n = min(int(result['n_frames']), len(frames))
        if int(result['flags']) & (_lib.NFC_EMU_PAIR_CUT_FRAMES | _lib.NFC_EMU_PAIR_CUT_BYTES):   # what lies before the first frame that did not fit
            used = 0
            for i in range(n):
                if int(frames[i]['n_bits']) == 0 or int(frames[i]['byte_off']) != used:
                    n = i
                    break
                used += int(frames[i]['n_bytes'])
        self.frames, self._plain, self._air, self._par = frames[:n], plain, air, par

    def __len__(self):
        return len(self.frames)

    def _slice(self, a, i):
        f = self.frames[i]
        return a[int(f['byte_off']):int(f['byte_off']) + int(f['n_bytes'])]

    def plain(self, i):
        return self._slice(self._plain, i)

    def air(self, i):
        return self._slice(self._air, i)

    def par(self, i):
        return self._slice(self._par, i)

    def nfc_frames(self):
        """The transcript as an eavesdropper's frames (api.NfcFrames: what fsm.host_commands, keys.find_auths and the monitors take)."""
        return frames_of_bits(synth_frames(self))

    def bits(self, i):
        """Frame i as the bit list the reference's emulator hands binary_src.set_bits (what tx.encode takes): nine bits per byte, least
        significant first and the ninth behind them; a short frame its seven bits."""
        b, p = self.air(i), self.par(i)
        if int(self.frames[i]['n_bits']) == 7:
            return [(int(b[0]) >> j) & 1 for j in range(7)]
        out = []
        for v, q in zip(b.tolist(), p.tolist()):
            out += [(v >> j) & 1 for j in range(8)] + [q & 1]
        return out


class Transcripts(object):
    def __init__(self, results, frames, plain, air, par, kernel_ms=None):
        self.results, self.frames, self.plain, self.air, self.par, self.kernel_ms = results, frames, plain, air, par, kernel_ms
        self.call_s = None

    def __len__(self):
        return len(self.results)

    def transcript(self, k):
        return Transcript(self.results[k], self.frames[k], self.plain[k], self.air[k], self.par[k])

    def arrays(self):
        """Every output array, for a byte-for-byte comparison of two calls."""
        return self.results, self.frames, self.plain, self.air, self.par

    def render_device(self, **kw):
        """What an eavesdropper's radio would have recorded of the K transactions, rendered on the GPU into one device buffer
        (air.render_device, its keywords) -> air.AirCaptures, ready for NfcMultiContext.push_device."""
        from . import air
        return air.render_device(self, **kw)


def _pairs(call, name, tags, readers, link, rounds, cap_frames, cap_bytes, pair_cap_frames, extra=()):
    tags, readers = list(tags), list(readers)
    if len(tags) != len(readers):
        raise ValueError('tags and readers: a pair is one of each')
    n = len(tags)
    ta, ra = (_lib.EmuCard * max(n, 1))(), (_lib.EmuCard * max(n, 1))()
    for i in range(n):
        ta[i], ra[i] = tags[i].struct(), readers[i].struct()
    cfg = _lib.EmuConfig(int(link), int(rounds), int(cap_frames), int(cap_bytes))
    if pair_cap_frames is not None:
        caps = np.ascontiguousarray(pair_cap_frames, np.uint32)
        if caps.shape != (n,):
            raise ValueError('pair_cap_frames: one entry per pair')
        cfg.pair_cap_frames = caps.ctypes.data if n else None
    res = np.zeros(n, EMU_RESULT_DTYPE)
    fr = np.zeros((n, int(cap_frames)), EMU_FRAME_DTYPE)
    plain, air, par = (np.zeros((n, int(cap_bytes)), np.uint8) for _ in range(3))
    t0 = time.perf_counter()
    rc = call(ta, ra, n, C.byref(cfg), res.ctypes.data, fr.ctypes.data, plain.ctypes.data, air.ctypes.data, par.ctypes.data, *extra)
    dt = time.perf_counter() - t0
    if rc != 0:
        _fail(name, rc)
    out = Transcripts(res, fr, plain, air, par)
    out.call_s = dt   # the library call alone, without the marshalling of the cards
    return out


def pairs_host(tags, readers, link=NFC_EMU_LINK_AIR, rounds=1, cap_frames=256, cap_bytes=2048, pair_cap_frames=None):
    """K cards read by K readers on one CPU core (nfc_host_emulate_pairs): the twin of pairs_device, the same bytes."""
    return _pairs(_lib.load().nfc_host_emulate_pairs, 'nfc_host_emulate_pairs', tags, readers, link, rounds, cap_frames, cap_bytes, pair_cap_frames)


def pairs_device(tags, readers, link=NFC_EMU_LINK_AIR, rounds=1, cap_frames=256, cap_bytes=2048, pair_cap_frames=None, device=0, timing=False):
    """K cards read by K readers on the GPU, a lane per pair (nfc_emulate_pairs_device).  timing: the kernel's duration -> .kernel_ms."""
    L = _lib.load()
    ms = C.c_float(0)
    out = _pairs(lambda *a: L.nfc_emulate_pairs_device(int(device), *a), 'nfc_emulate_pairs_device', tags, readers, link, rounds, cap_frames, cap_bytes,
                 pair_cap_frames, (C.byref(ms) if timing else None,))
    out.kernel_ms = ms.value if timing else None
    return out
