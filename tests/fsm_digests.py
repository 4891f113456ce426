"""Truncated SHA-256 digests of what the protocol machine makes of a sequence -- what commit 8370f3e's host machine (the separate
csrc/protocol.h of that time) produced on the rows of tests/golden/fx_fsm_fuzz.npz, on its outgoing scenarios and on a family of UIDs
grown past 32 bytes (tests/golden/fx_fsm_parent.json, written by tests/golden/make_fsm_parent_digests.py AT THAT COMMIT).  The maker
and tests/test_fsm_parent.py share everything here: the byte string of a row and the legs that produce one.

A row's byte string is independent of the route that produced it: every nfc_frame field but byte_off (the packet and frame routes pack
the bytes, the twin and the kernel give every frame a slot) as little-endian columns, then per record bytes[:n_bytes] and enc[:n_enc],
then the 88 bytes of the nfc_fsm_state afterwards -- or NO_STATE where nfc_fsm_get_state refuses (a UID longer than 32 bytes)."""
import ctypes as C
import hashlib

import numpy as np

from usrp_nfc_amd import _lib, command, fsm, synth

HEX = 10                                   # hexadecimal digits kept of a row's SHA-256
NO_STATE = b'no state: the UID is longer than 32 bytes'
FIELDS = ('cmd', 'type', 'n_bytes', 'n_header', 'n_extra', 'n_crc', 'flags', 'n_enc', 'pad')


def records_bytes(table, data, enc):
    table = np.ascontiguousarray(table, fsm.FRAME_DTYPE)
    parts = [np.ascontiguousarray(table[name]).tobytes() for name in FIELDS]
    for f in table:
        o = int(f['byte_off'])
        parts.append(np.ascontiguousarray(data[o:o + int(f['n_bytes'])], np.uint8).tobytes())
        parts.append(np.ascontiguousarray(enc[o:o + int(f['n_enc'])], '<u2').tobytes())
    return b''.join(parts)


def digest(*parts):
    return hashlib.sha256(b''.join(parts)).hexdigest()[:HEX]


def row_digest(table, data, enc, state):
    """state: the 88 bytes, or None where there is none to be had."""
    return digest(records_bytes(table, data, enc), NO_STATE if state is None else bytes(state))


def state_of(m):
    st = _lib.FsmState()
    return bytes(bytearray(st)) if m.L.nfc_fsm_get_state(m._h, C.byref(st)) == 0 else None


def machine(keys=None, table=None):
    m = fsm.fsm(callback=lambda cmd, st: None)
    if keys:
        m.set_keys(*keys)
    if table:
        m.set_sector_keys(table)
    return m


def one_packet(m, bits, ptype):
    """nfc_fsm_process on one packet: (the record, its bytes, its enc entries)."""
    b = np.ascontiguousarray(bits, np.uint8)
    frame = np.zeros(1, fsm.FRAME_DTYPE)
    data, enc = np.zeros(b.size // 9 + 1, np.uint8), np.zeros(b.size // 9 + 1, np.uint16)
    rc = m.L.nfc_fsm_process(m._h, b.ctypes.data if b.size else None, b.size, int(ptype), frame.ctypes.data_as(C.POINTER(_lib.Frame)), data.ctypes.data,
                             data.size, enc.ctypes.data)
    assert rc == 0
    return frame, data[:int(frame['n_bytes'][0])], enc[:int(frame['n_enc'][0])]


def packet_route(m, packets):
    """The packets one by one through nfc_fsm_process: (table, data, enc), packed."""
    recs, data, enc, at = [], [], [], 0
    for t, bits in packets:
        f, d, e = one_packet(m, bits, t)
        f['byte_off'] = at
        n = max(len(d), len(e))
        recs.append(f)
        data.append(np.concatenate([d, np.zeros(n - len(d), np.uint8)]))
        enc.append(np.concatenate([e, np.zeros(n - len(e), np.uint16)]))
        at += n
    if not recs:
        return np.zeros(0, fsm.FRAME_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.uint16)
    return np.concatenate(recs), np.concatenate(data), np.concatenate(enc)


def packet_digest(packets, keys=None, table=None):
    m = machine(keys, table)
    return row_digest(*packet_route(m, packets), state=state_of(m))


def outgoing_digest(steps):
    """One scenario of the fixture through ALL its steps (kind 0: a frame heard, a its type; kind 1: a frame sent, a its command): the record
    or the bits put out per step, the state afterwards."""
    m = machine()
    parts = []
    for kind, a, bits_in, _, _ in steps:
        if kind == 0:
            parts.append(b'H' + records_bytes(*one_packet(m, bits_in, a)))
        else:
            parts.append(b'S' + bytes(bytearray(m.process_outgoing(bits_in, command.CommandType.by_index(a)))))
    state = state_of(m)
    return digest(b'|'.join(parts), NO_STATE if state is None else state)


def long_uid_family():
    """UIDs grown past 32 bytes: nine and ten ANTI1R / ANTI1G and ANTI2R / ANTI2T pairs of distinct bytes behind REQA, ATQA1K; then a SEL2R that
    names the last four bytes or four others, an AUTHA and a tag nonce.  -> [(name, packets)]"""
    def with_crc(data):
        return list(data) + fsm.crc_a(data)

    def with_bcc(u):
        return list(u) + [u[0] ^ u[1] ^ u[2] ^ u[3]]

    reqa = [(0x26 >> i) & 1 for i in range(7)] + [0]
    out = []
    for name, ask in (('anti1', [0x93, 0x20]), ('anti2', [0x95, 0x20])):
        for pairs in (9, 10):
            for same in (True, False):
                packets = [(1, reqa), (0, synth.frame_bits([0x04, 0x00]))]
                for i in range(pairs):
                    uid = [0x10 + i, 0x20 + i, 0x30 + i, 0x40 + i]
                    packets += [(1, synth.frame_bits(ask)), (0, synth.frame_bits(with_bcc(uid)))]
                sel = uid if same else [0xA1, 0xB2, 0xC3, 0xD4]
                packets += [(1, synth.frame_bits(with_crc([0x95, 0x70] + with_bcc(sel)))), (1, synth.frame_bits(with_crc([0x60, 0x04]))),
                            (0, synth.frame_bits([0x01, 0x02, 0x03, 0x04]))]
                out.append(('%s_%d_%s' % (name, pairs, 'same' if same else 'other'), packets))
    return out


def long_uid_cmds(name):
    kind, pairs, _ = name.split('_')
    return [0, 3] + ([12, 13] if kind == 'anti2' else [6, 8]) * int(pairs) + [19, 14, 16]


def long_uid_digest(packets, route):
    """route(m, packets) -> (table, data, enc).  The commands are the ones meant, the SEL2R flags a mismatch exactly where it names other bytes,
    nothing has a state to give, and the tag nonce started no session: a REQA behind it is heard in the clear."""
    m = machine()
    table, data, enc = route(m, packets)
    d = row_digest(table, data, enc, state_of(m))
    assert state_of(m) is None
    f, _, _ = one_packet(m, packets[0][1], 1)
    assert int(f['cmd'][0]) == 0 and int(f['flags'][0]) == 0, 'a session was started'
    return d, table
