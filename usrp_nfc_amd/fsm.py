"""fsm.process_bits of the reference (fsm.py:218-238) -- "next" rows f1 and f3 of SURVEY.md section 8.

`fsm(callback)` keeps the reference's constructor and `process_bits(bits, packet_type)` entry point, so
`background` / `CombinedPacketProcessor` hand packets to it unchanged; frame repair, parity, CRC_A, command lookup
and UID tracking run in the shared library (csrc/fsm.hip.h, the host machine over it: csrc/protocol.h).  `process_packets` is the batch form for the
packet tables a GPU batch produces.  MIFARE Classic sessions are decrypted (CRYPTO1: cipher.py, lfsr.py) with the
keys of set_keys (default FF..FF), nested authentications included; as in the reference, the ciphertext of every
frame of a session is printed before its decoded command.  A card whose sectors have different keys takes a table
(set_sector_keys: (key_type, sector) -> key; include/nfc_amd.h): every AUTHA / AUTHB looks its block's
sector up there and falls back to the two keys of set_keys where the table has no entry."""
import ctypes as C
import sys

import numpy as np

from . import _lib
from . import keys as _keys
from .command import CommandStructure, CommandType

NFC_CMD_UNKNOWN, NFC_CMD_PARITY_ERROR = -1, -2
FRAME_EXTRA_ERROR, FRAME_MANY_MORE_ERROR, FRAME_UID_MISMATCH, FRAME_ENCRYPTED = 1, 2, 4, 8
FRAME_AR_OK, FRAME_AR_ERROR, FRAME_AT_OK, FRAME_AT_ERROR = 16, 32, 64, 128
_SEL2R = 19   # csrc/fsm.hip.h: C_SEL2R
FRAME_DTYPE = np.dtype([('cmd', '<i4'), ('type', '<i4'), ('byte_off', '<u4'), ('n_bytes', '<u2'), ('n_header', '<u2'),
                        ('n_extra', '<u2'), ('n_crc', '<u2'), ('flags', '<u4'), ('n_enc', '<u2'), ('pad', '<u2')])


def _messages(flags, out):
    if flags & FRAME_EXTRA_ERROR:
        out.write('EXTRA ERROR\n')
    if flags & FRAME_MANY_MORE_ERROR:
        out.write('MANY MORE ERROR\n')


def _structure(cmd_index, n_header, n_extra, data):
    cmd = CommandType.by_index(cmd_index)
    if cmd is None:
        return None, CommandStructure('UNKNOWN', [], data)
    return cmd, CommandStructure(cmd.name(), data[:n_header], data[n_header:n_header + n_extra], data[n_header + n_extra:])


def dispatch(table, data, enc, out=None, callback=None):
    """Print or forward the records of a frame table exactly as the machine does while it processes them: `table` FRAME_DTYPE records,
    `data` / `enc` the byte and ciphertext arrays their byte_off indexes (fsm.process_frames' outputs, host_commands', or one
    stream's part of an NfcMultiCommands: ``dispatch(*cmds.commands_of(k))``).  out: where the messages go (default sys.stdout);
    callback(cmd, struct): default struct.display(out).  It uses no machine state.  -> the CommandStructures (None: a parity error)."""
    out = out or sys.stdout
    callback = callback or (lambda cmd, struct: struct.display(out))
    res = []
    for f in table:
        o = int(f['byte_off'])
        res.append(_dispatch_one(f, data[o:o + int(f['n_bytes'])].tolist(), enc[o:o + int(f['n_enc'])], out, callback))
    return res


def _dispatch_one(f, data, enc, out, callback):
    flags = int(f['flags'])
    _messages(flags, out)
    if flags & FRAME_ENCRYPTED:   # fsm._print_enc (fsm.py:113-131): what was on the air, '!' where the parity bit equals the data parity
        out.write(''.join('0x%02X%s ' % (int(e) & 0xFF, '!' if int(e) & 0x100 else '') for e in enc) + '\n')
    if int(f['cmd']) == NFC_CMD_PARITY_ERROR:
        out.write('PARITY ERROR\n')
        return None
    if int(f['cmd']) == _lib.NFC_CMD_CUT:   # (only the GPU machine of a multi-stream context makes these: the frame's bits were not stored)
        out.write('CUT\n')
        return None
    if flags & FRAME_UID_MISMATCH:   # fsm.py:184,192: the two lines, without the lists the reference prints behind them
        out.write('MISMATCH BETWEEN READER_TAG UID#2\n' if int(f['cmd']) == _SEL2R else 'MISMATCH BETWEEN READER-TAG UID\n')
    for bit, msg in ((FRAME_AR_OK, 'AR OK'), (FRAME_AR_ERROR, 'ERROR WITH AR'), (FRAME_AT_OK, 'AT OK'), (FRAME_AT_ERROR, 'ERROR WITH AT')):
        if flags & bit:
            out.write(msg + '\n')
    cmd, st = _structure(int(f['cmd']), int(f['n_header']), int(f['n_extra']), data)
    callback(cmd, st)
    return st


def state_init():
    """The nfc_fsm_state a reset leaves (nfc_fsm_state_init): REQA in flight, no tag, both keys FF..FF."""
    st = _lib.FsmState()
    if _lib.load().nfc_fsm_state_init(C.byref(st)) != 0:
        raise RuntimeError('nfc_fsm_state_init failed')
    return st


def host_commands(state, frames, data=None, par=None, sector_keys=None):
    """The GPU machine's twin on the CPU (nfc_host_commands_keyed): `frames` as process_frames takes them, `state` an _lib.FsmState that
    is advanced in place, sector_keys the stream's key table (keys.key_table's argument; None: none -- nfc_host_commands).
    -> (table, data, enc): every frame owns a slot of its raw n_bytes entries in data and enc."""
    if data is None:
        frames, data, par = frames.table, frames.bytes, frames.par
    t = np.ascontiguousarray(frames, _lib.RAW_FRAME_DTYPE)
    b = [np.ascontiguousarray(a, np.uint8) for a in data]
    p = [np.ascontiguousarray(a, np.uint8) for a in par]
    cap = int(t['n_bytes'].sum()) + 1
    out, buf, enc = np.zeros(len(t), FRAME_DTYPE), np.zeros(cap, np.uint8), np.zeros(cap, np.uint16)
    used = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    keyed = None if sector_keys is None else C.byref(_keys.key_table(sector_keys))
    rc = _lib.load().nfc_host_commands_keyed(C.byref(state), keyed, ptr(t), len(t), ptr(b[0]), ptr(p[0]), ptr(b[1]), ptr(p[1]), out.ctypes.data,
                                             buf.ctypes.data, enc.ctypes.data, cap, C.byref(used))
    if rc != 0:
        raise ValueError('nfc_host_commands_keyed status %d' % rc)
    return out, buf[:used.value], enc[:used.value]


def host_commands_segmented(state, frames, data=None, par=None, sector_keys=None, segment_order=None):
    """host_commands computed the way a tracked NfcContext computes it on the GPU (nfc_host_commands_segmented, csrc/ctx_commands.hip.h):
    the frames cut into segments at every plain REQA / WUPA, every segment walked speculatively -- in the order `segment_order` names,
    entries at or past the segment count skipped, None: ascending -- and a resolve that walks again what was guessed wrong.
    -> (table, data, enc, counters): host_commands' outputs, bit for bit, and a dict of n_segments, n_rerun_segments, n_rerun_frames,
    n_keydep_segments."""
    if data is None:
        frames, data, par = frames.table, frames.bytes, frames.par
    t = np.ascontiguousarray(frames, _lib.RAW_FRAME_DTYPE)
    b = [np.ascontiguousarray(a, np.uint8) for a in data]
    p = [np.ascontiguousarray(a, np.uint8) for a in par]
    cap = int(t['n_bytes'].sum()) + 1
    out, buf, enc = np.zeros(len(t), FRAME_DTYPE), np.zeros(cap, np.uint8), np.zeros(cap, np.uint16)
    used = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    keyed = None if sector_keys is None else C.byref(_keys.key_table(sector_keys))
    order = None if segment_order is None else np.ascontiguousarray(segment_order, np.uint32)
    cn = _lib.CtxCommandCounters()
    rc = _lib.load().nfc_host_commands_segmented(C.byref(state), keyed, ptr(t), len(t), ptr(b[0]), ptr(p[0]), ptr(b[1]), ptr(p[1]), out.ctypes.data,
                                                 buf.ctypes.data, enc.ctypes.data, cap, C.byref(used),
                                                 None if order is None else (order if order.size else np.zeros(1, np.uint32)).ctypes.data,
                                                 0 if order is None else len(order), C.byref(cn))
    if rc != 0:
        raise ValueError('nfc_host_commands_segmented status %d' % rc)
    return out, buf[:used.value], enc[:used.value], {k: int(getattr(cn, k)) for k, _ in _lib.CtxCommandCounters._fields_}


class fsm(object):
    def __init__(self, callback=None, out=None):
        self.L = _lib.load()
        self._h = C.c_void_p()
        if self.L.nfc_fsm_create(C.byref(self._h)) != 0:
            raise RuntimeError('nfc_fsm_create failed')
        self._out = out or sys.stdout
        self._callback = callback if callback else self._display

    def __del__(self):
        if getattr(self, '_h', None):
            self.L.nfc_fsm_destroy(self._h)
            self._h = None

    def reset(self):
        self.L.nfc_fsm_reset(self._h)

    def _display(self, cmd, struct):
        struct.display(self._out)

    def set_keys(self, key_a=(0xFF,) * 6, key_b=(0xFF,) * 6):
        """Sector keys of a MIFARE Classic tag (fsm.set_keys, fsm.py:157-160)."""
        a = np.ascontiguousarray(key_a, np.uint8)
        b = np.ascontiguousarray(key_b, np.uint8)
        if a.size != 6 or b.size != 6 or self.L.nfc_fsm_set_keys(self._h, a.ctypes.data, b.ctypes.data) != 0:
            raise ValueError('keys are six bytes each')

    def set_sector_keys(self, table=None):
        """The per-sector key table (nfc_fsm_set_key_table): a dict (key_type, sector) -> six key bytes, key_type 0x60 / 0x61, or an
        _lib.FsmKeyTable; None or {} empties it.  An AUTHA / AUTHB on a block whose sector has an entry is keyed with it, every other
        one with set_keys' two keys.  reset() empties the table; set_keys and set_state leave it alone."""
        if self.L.nfc_fsm_set_key_table(self._h, C.byref(_keys.key_table(table))) != 0:
            raise ValueError('nfc_fsm_set_key_table failed')

    def set_sector_key(self, key_type, sector, key):
        """One slot of the table (nfc_fsm_set_sector_key): key None clears it."""
        _keys.key_table({(key_type, sector): key})   # (names what is wrong)
        k = None if key is None else np.ascontiguousarray(list(bytearray(key)), np.uint8)
        if self.L.nfc_fsm_set_sector_key(self._h, int(key_type), int(sector), None if k is None else k.ctypes.data) != 0:
            raise ValueError('nfc_fsm_set_sector_key failed')

    def sector_keys(self):
        """The table as the dict (key_type, sector) -> six key bytes of its present slots (nfc_fsm_get_key_table)."""
        t = _lib.FsmKeyTable()
        if self.L.nfc_fsm_get_key_table(self._h, C.byref(t)) != 0:
            raise ValueError('nfc_fsm_get_key_table failed')
        return _keys.table_dict(t)

    def get_state(self):
        """The machine as a plain nfc_fsm_state (nfc_fsm_get_state) -- what NfcMultiContext.set_fsm_state takes.  ValueError when the
        UID is longer than the 32 bytes the plain state holds."""
        st = _lib.FsmState()
        if self.L.nfc_fsm_get_state(self._h, C.byref(st)) != 0:
            raise ValueError('nfc_fsm_get_state: the UID is longer than 32 bytes')
        return st

    def set_state(self, st):
        """Continue from a plain nfc_fsm_state (NfcMultiContext.fsm_state(k), another machine's get_state())."""
        if self.L.nfc_fsm_set_state(self._h, C.byref(st)) != 0:
            raise ValueError('nfc_fsm_set_state: a field of the state is out of range')

    def _dispatch(self, f, data, enc=()):
        return _dispatch_one(f, data, enc, self._out, self._callback)

    def process_bits(self, bits, packet_type):
        """One closed packet (fsm.py:218).  Returns the CommandStructure, or None on a parity error."""
        b = np.ascontiguousarray(bits, np.uint8)
        frame = np.zeros(1, FRAME_DTYPE)
        data = np.zeros(b.size // 9 + 1, np.uint8)
        enc = np.zeros(b.size // 9 + 1, np.uint16)
        rc = self.L.nfc_fsm_process(self._h, b.ctypes.data, b.size, int(packet_type), frame.ctypes.data_as(C.POINTER(_lib.Frame)),
                                    data.ctypes.data, data.size, enc.ctypes.data)
        if rc != 0:
            raise ValueError('nfc_fsm_process status %d' % rc)
        f = frame[0]
        return self._dispatch(f, data[:int(f['n_bytes'])].tolist(), enc[:int(f['n_enc'])])

    def process_outgoing(self, bits, cmd):
        """A frame an emulator is about to send (fsm.process_outgoing, fsm.py:68-112; the encoder hook of packets.py:88-90):
        `bits` with parity as the encoders take them, `cmd` the CommandType it is.  Returns the bits to put on the air --
        encrypted while a MIFARE Classic session is up.  With an Ultralight tag the frame goes through process_bits, as in the
        reference ("update state": the callback sees it)."""
        b = np.ascontiguousarray(bits, np.uint8)
        out = np.zeros(max(1, b.size), np.uint8)
        rc = self.L.nfc_fsm_process_outgoing(self._h, b.ctypes.data if b.size else None, b.size, int(cmd.index), out.ctypes.data)
        if rc == 1:
            self.process_bits(bits, cmd.packet_type())
            return list(bits)
        if rc != 0:
            raise ValueError('nfc_fsm_process_outgoing status %d' % rc)
        return [int(v) for v in out[:b.size]]

    def process_packets(self, table, bits0, bits1, dispatch=True):
        """A batch: `table` rows of nfc_packet (both types, in stream order) over the per-type bit arrays.
        Returns (frames, bytes) as numpy arrays; the callback sees every command in order (dispatch=False: only the
        arrays -- a caller that consumes the frame table itself)."""
        t = np.ascontiguousarray(table)
        b0 = np.ascontiguousarray(bits0, np.uint8)
        b1 = np.ascontiguousarray(bits1, np.uint8)
        frames = np.zeros(len(t), FRAME_DTYPE)
        data = np.zeros(int(t['n_bits'].sum()) // 9 + len(t) + 1, np.uint8)
        enc = np.zeros(data.size, np.uint16)
        used = C.c_size_t(0)
        rc = self.L.nfc_fsm_process_packets(self._h, t.ctypes.data, len(t), b0.ctypes.data if b0.size else None,
                                            b1.ctypes.data if b1.size else None, frames.ctypes.data, data.ctypes.data, data.size,
                                            C.byref(used), enc.ctypes.data)
        if rc != 0:
            raise ValueError('nfc_fsm_process_packets status %d' % rc)
        for f in (frames if dispatch else ()):
            o = int(f['byte_off'])
            self._dispatch(f, data[o:o + int(f['n_bytes'])].tolist(), enc[o:o + int(f['n_enc'])])
        return frames, data[:used.value]

    def process_frames(self, frames, data=None, par=None, dispatch=True):
        """process_packets over frames assembled on the GPU (NfcContext.frames(), NfcMultiFrames.frames_of(k), api.host_frames):
        `frames` an NfcFrames, or the merged RAW_FRAME_DTYPE table with data = (bytes0, bytes1) and par = (par0, par1).  Returns what
        process_packets returns on the packets the frames came from, and leaves the machine in the same state."""
        if data is None:
            frames, data, par = frames.table, frames.bytes, frames.par
        t = np.ascontiguousarray(frames, _lib.RAW_FRAME_DTYPE)
        b = [np.ascontiguousarray(a, np.uint8) for a in data]
        p = [np.ascontiguousarray(a, np.uint8) for a in par]
        out = np.zeros(len(t), FRAME_DTYPE)
        buf = np.zeros(int(t['n_bits'].sum()) // 9 + len(t) + 1, np.uint8)
        enc = np.zeros(buf.size, np.uint16)
        used = C.c_size_t(0)
        ptr = lambda a: a.ctypes.data if a.size else None
        rc = self.L.nfc_fsm_process_frames(self._h, ptr(t), len(t), ptr(b[0]), ptr(p[0]), ptr(b[1]), ptr(p[1]), out.ctypes.data,
                                           buf.ctypes.data, buf.size, C.byref(used), enc.ctypes.data)
        if rc != 0:
            raise ValueError('nfc_fsm_process_frames status %d' % rc)
        for f in (out if dispatch else ()):
            o = int(f['byte_off'])
            self._dispatch(f, buf[o:o + int(f['n_bytes'])].tolist(), enc[o:o + int(f['n_enc'])])
        return out, buf[:used.value]


def crc_a(data):
    """ISO 14443-3 type A CRC as [low, high] (utilities.CRC.calculate_crc, utilities.py:30-41)."""
    L = _lib.load()
    b = np.ascontiguousarray(data, np.uint8)
    out = np.zeros(2, np.uint8)
    if L.nfc_crc_a(b.ctypes.data if b.size else None, b.size, out.ctypes.data) != 0:
        raise ValueError('nfc_crc_a failed')
    return [int(out[0]), int(out[1])]
