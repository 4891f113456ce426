"""The reference's tag module (tag.py) over the tag machine of csrc/emu.hip.h (nfc_host_emu_step): ``Tag(callback, tag_type, memory,
rands)`` keeps the reference's constructor, ``process_packet(cmd, struct)``, ``set_encoder``, ``wake_up``, ``generate_1k``,
``get_keys_from_mem`` and its printed text.  An object of it is what ``decoder(..., emulator=)`` / ``background(..., emulator=)`` take:
``fsm.fsm(tag.process_packet)`` hears for it and ``tag.set_encoder(fsm.process_outgoing)`` encrypts what it sends.

mode: emulate.NFC_EMU_REFERENCE (the default: the reference with its quirks) or NFC_EMU_CARD (include/nfc_amd.h says what differs).
Where the reference raises the object answers nothing and ``flags()`` has NFC_EMU_RAISED."""
import sys

from . import emulate
from .command import CommandStructure, CommandType, PacketType, TagType
from .rand import Rand
from .utilities import Convert


class AuthKey:   # tag.py:27-30
    NONE = 0
    A = 1
    B = 2


class Tag(object):
    @staticmethod
    def generate_1k():
        return emulate.generate_1k()

    @staticmethod
    def get_keys_from_mem(mem):   # tag.py:52-57: the trailer of sector 0
        return (list(mem[48:54]), list(mem[58:64]))

    def __init__(self, callback=None, tag_type=TagType.ULTRALIGHT, memory=None, rands=None, *, mode=emulate.NFC_EMU_REFERENCE, out=None):
        """The reference's four arguments (tag.py:59); behind the `*`, by keyword only: the card's mode and where the text is printed."""
        if tag_type not in (TagType.ULTRALIGHT, TagType.CLASSIC1K):
            raise ValueError('tag_type: TAG TYPE UNSUPPORTED')
        self._tag_type, self._out = tag_type, out or sys.stdout
        self._random = Rand(rands) if tag_type == TagType.CLASSIC1K else None
        self._card = emulate.tag_card(tag_type, memory, self._random.rands() if self._random else None, mode)
        self._state = emulate.state_init()
        self._callback = callback if callback else self._display
        self._encode = None

    def _display(self, bits):
        self._out.write('%s\n' % (bits,))

    def wake_up(self):
        self._state.halted = 0

    def set_encoder(self, encode):
        self._encode = encode

    def state(self):
        """the machine's nfc_emu_state (an _lib.EmuState; assign to continue from another's)"""
        return self._state

    def flags(self):
        return int(self._state.flags)

    def process_packet(self, cmd, struct):
        if cmd is not None and cmd.packet_type() != PacketType.READER_TO_TAG:
            return None
        if cmd is not None:
            self._out.write('TAG INCOMING\n' if self._tag_type == TagType.ULTRALIGHT else 'INCOMING\n')   # tag.py:118,326
            struct.display(self._out)
        nxt, frame = emulate.step(self._card, self._state, cmd.index if cmd is not None else -1, struct.extra() if cmd is not None else [])
        if nxt is None:
            return None
        nxt = CommandType.by_index(nxt)
        n_crc = 2 if nxt.needs_crc() else 0
        st = CommandStructure(nxt.name(), nxt.header(), frame[len(nxt.header()):len(frame) - n_crc], frame[len(frame) - n_crc:])
        self._out.write('TAG OUTGOING\n')   # tag.py:100-108
        st.display(self._out)
        all_bits = Convert.to_bit_ar(st.all_bytes(), True)
        if self._encode:
            all_bits = self._encode(all_bits, nxt)
        self._callback(all_bits)
        return (nxt, st)
