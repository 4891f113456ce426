"""The reference's rand module (rand.py): the nonces an emulator hands out, in turn and from the first again after a reset.

``Rand(rands)`` keeps the reference's constructor.  Without a list the reference draws from `random`, reseeded from the clock on every
reset; here ``Rand(None)`` draws a fixed-length list ONCE from a generator seeded with `seed` (emulate.drawn_rands) and hands that down --
a stated deviation: the emulators behind tag.Tag / reader.Reader take a list of at most 64 nonces (include/nfc_amd.h)."""
from . import emulate


class Rand(object):
    def __init__(self, rands=None, *, seed=0, n=16):
        self._rands = [list(r) for r in rands] if rands else emulate.drawn_rands(seed, n)
        self._randll = len(self._rands)
        self.reset()

    def rands(self):
        """the whole list (what the emulator's card takes)"""
        return [list(r) for r in self._rands]

    def get_next(self):   # rand.py:23-27
        r = self._rands[self._index]
        self._index = (self._index + 1) % self._randll
        return list(r)

    def reset(self):      # rand.py:29-30
        self._index = 0
