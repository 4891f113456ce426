#!/usr/bin/env python3
"""Generate tests/golden/fx_ultralight_sc8.npz and fx_ultralight_cu8.npz by driving the UNMODIFIED reference
(make_golden.run_reference).

The Ultralight transaction's IQ (fx_ultralight_iq.npz) quantised to complex int8 (synth.quantise_sc8) and to complex uint8
(synth.quantise_cu8), both at full_scale 127, and what the reference produced from each one's envelope: the pair converted as
NFC_IN_IQ_I8 / NFC_IN_IQ_U8 convert it (scale 0: 2^-7), then fl(fl(I*I) + fl(Q*Q)) -- api.host_envelope -- with the UHD branch's
hi_val 1.1 (decoder.py:23).  Each file is a golden_util.Case like the others (x = that envelope) plus the capture itself ('iq8',
interleaved, I first).  It also checks that fsm prints tests/golden/ultralight.out from each capture's packets.

Runs only where the reference is (as make_golden.py); the test-suite reads the .npz.

    python3 tests/golden/make_iq8_golden.py
"""
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg   # noqa: E402  (imports the reference)

from usrp_nfc_amd import api, fsm, synth   # noqa: E402

FULL_SCALE = 127.0


def fsm_trace(packets):
    out = io.StringIO()
    m = fsm.fsm(out=out)
    for t, bits in packets:
        m.process_bits(bits, t)
    return out.getvalue()


def main():
    iq = np.load(os.path.join(HERE, 'fx_ultralight_iq.npz'))['iq']
    gold = open(os.path.join(HERE, 'ultralight.out')).read().rstrip('\n')
    for name, kind, q in (('sc8', api.NFC_IN_IQ_I8, synth.quantise_sc8), ('cu8', api.NFC_IN_IQ_U8, synth.quantise_cu8)):
        iq8 = q(iq, FULL_SCALE)
        x = api.host_envelope(iq8, kind, 0.0)
        p = dict(mg.DEFAULTS, hi_val=1.1)
        kw = dict(samp_rate=p['samp_rate'], hi_val=p['hi_val'], lo_val=p['lo_val'], av_window=p['av_window'],
                  max_len=p['max_len'], reader=p['reader'], tag=p['tag'])
        a = mg.run_reference(x, chunk=8192, **kw)
        b = mg.run_reference(x, chunk=4096, rng=np.random.default_rng(7), **kw)
        assert a == b, 'reference is not chunk-invariant on the %s capture' % name
        out = mg.pack(x, p, a)
        out['iq8'] = iq8
        np.savez_compressed(os.path.join(HERE, 'fx_ultralight_%s.npz' % name), **out)
        same = fsm_trace(a[3]).rstrip('\n') == gold
        print('fx_ultralight_%s: N=%d transitions=%d sym_tag=%d sym_reader=%d packets=%d; fsm prints ultralight.out: %s' %
              (name, len(x), len(a[0]), len(a[1]), len(a[2]), len(a[3]), 'yes' if same else 'NO'))


if __name__ == '__main__':
    main()
