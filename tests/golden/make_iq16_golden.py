#!/usr/bin/env python3
"""Generate tests/golden/fx_ultralight_sc16.npz by driving the UNMODIFIED reference (make_golden.run_reference).

The Ultralight transaction's IQ (fx_ultralight_iq.npz) quantised to complex int16 (synth.quantise_sc16), and what the
reference produced from its envelope: the pair converted as NFC_IN_IQ_I16 converts it (i16_scale 0: / 32767), then
fl(fl(I*I) + fl(Q*Q)) -- api.host_envelope -- with the UHD branch's hi_val 1.1 (decoder.py:23).  The file is a
golden_util.Case like the others (x = that envelope) plus the capture itself ('iq16', interleaved int16, I first).

Runs only where the reference is (as make_golden.py); the test-suite reads the .npz.

    python3 tests/golden/make_iq16_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg   # noqa: E402  (imports the reference)

from usrp_nfc_amd import api, synth   # noqa: E402


def main():
    iq = np.load(os.path.join(HERE, 'fx_ultralight_iq.npz'))['iq']
    iq16 = synth.quantise_sc16(iq)
    x = api.host_envelope(iq16, api.NFC_IN_IQ_I16, 0.0)
    p = dict(mg.DEFAULTS, hi_val=1.1)
    kw = dict(samp_rate=p['samp_rate'], hi_val=p['hi_val'], lo_val=p['lo_val'], av_window=p['av_window'],
              max_len=p['max_len'], reader=p['reader'], tag=p['tag'])
    a = mg.run_reference(x, chunk=8192, **kw)
    b = mg.run_reference(x, chunk=4096, rng=np.random.default_rng(7), **kw)
    assert a == b, 'reference is not chunk-invariant on the sc16 capture'
    out = mg.pack(x, p, a)
    out['iq16'] = iq16
    np.savez_compressed(os.path.join(HERE, 'fx_ultralight_sc16.npz'), **out)
    print('fx_ultralight_sc16: N=%d transitions=%d sym_tag=%d sym_reader=%d packets=%d' %
          (len(x), len(a[0]), len(a[1]), len(a[2]), len(a[3])))


if __name__ == '__main__':
    main()
