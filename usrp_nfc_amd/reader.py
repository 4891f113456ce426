"""The reference's reader module (reader.py) over the reader machine of csrc/emu.hip.h (nfc_host_emu_step): ``Reader(callback, rands,
keya, keyb)`` keeps the reference's constructor, ``process_packet(cmd, struct)``, ``set_encoder`` and its printed text; the callback gets
``(bits, finished)``, finished with the HALT that ends a card.  As tag.Tag, it is what ``decoder(..., emulator=)`` takes.

The plain frames a reader sends do not depend on its keys (the answer to a tag nonce follows from the nonce alone): the keys are its
protocol machine's -- ``keys()`` gives them for ``fsm.set_keys``.  mode / table: for the closed loop on the device (emulate.reader_card)."""
import sys

from . import emulate
from .command import CommandStructure, CommandType, PacketType
from .rand import Rand
from .utilities import Convert


class Reader(object):
    def __init__(self, callback=None, rands=None, keya=None, keyb=None, *, mode=emulate.NFC_EMU_REFERENCE, table=None, out=None):
        """The reference's four arguments (reader.py:16); behind the `*`, by keyword only: the card's mode, its key table, where the text goes."""
        self._out = out or sys.stdout
        self._callback = callback if callback else self._display
        self._random = Rand(rands)
        self._keya, self._keyb = keya, keyb
        self._key = [0xFF] * 6 if not keya else list(keya)   # reader.py:25
        self._card = emulate.reader_card(self._random.rands(), self._key, list(keyb) if keyb else [0xFF] * 6, table, mode)
        self._state = emulate.state_init()
        self._encode = None

    def _display(self, bits, finished=False):
        self._out.write('%s %s\n' % (bits, finished))

    def keys(self):
        return list(self._card.key_a), list(self._card.key_b)

    def set_encoder(self, encode):
        self._encode = encode

    def state(self):
        return self._state

    def flags(self):
        return int(self._state.flags)

    def process_packet(self, cmd, struct):
        if cmd is not None and cmd.packet_type() != PacketType.TAG_TO_READER:
            return None
        if cmd is not None:
            self._out.write('READER INCOMING\n')   # reader.py:63-64
            struct.display(self._out)
        before = int(self._state.flags)
        nxt, frame = emulate.step(self._card, self._state, cmd.index if cmd is not None else -1, struct.extra() if cmd is not None else [])
        if int(self._state.flags) & ~before & emulate._lib.NFC_EMU_UNEXPECTED:
            self._out.write('ERROR, Unexpected command!!\n')   # reader.py:146
        if nxt is None:
            return None
        nxt = CommandType.by_index(nxt)
        n_crc = 2 if nxt.needs_crc() else 0
        st = CommandStructure(nxt.name(), nxt.header(), frame[len(nxt.header()):len(frame) - n_crc], frame[len(frame) - n_crc:])
        self._out.write('READER OUTGOING\n')   # reader.py:43-44
        st.display(self._out)
        all_bits = Convert.to_bit_ar(st.all_bytes(), True)
        if self._encode:
            all_bits = self._encode(all_bits, nxt)
        self._callback(all_bits, nxt.name() == 'HALT')
        return (nxt, st)
