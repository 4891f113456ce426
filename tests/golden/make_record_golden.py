#!/usr/bin/env python3
"""Generate tests/golden/fx_ultralight_rec16.npz by driving the UNMODIFIED reference (make_golden.run_reference).

The Ultralight transaction's IQ (fx_ultralight_iq.npz) recorded as decoder(src=IQ, dst=wav) records it: the envelope
fl(fl(I*I) + fl(Q*Q)) (api.host_envelope) converted to 16-bit PCM at gain 32767 (api.host_record_pcm16: the conversion of
include/nfc_amd.h) -- 'pcm' -- and what the reference produced from that recording read back through its WAV branch
(decoder.py:25-29): s = fl(pcm / 32767), x = fl(s*s), hi_val 1.09.  The file is a golden_util.Case like the others (x = that
envelope) plus the PCM.  It also checks that the packets are the fc32 capture's own (fx_ultralight_txn) and that fsm prints
tests/golden/ultralight.out from them, and reports the other gains: 4096 and 512 keep every packet, 131068 clips and does not.

Runs only where the reference is (as make_golden.py); the test-suite reads the .npz.

    python3 tests/golden/make_record_golden.py
"""
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg   # noqa: E402  (imports the reference)

from usrp_nfc_amd import api, fsm   # noqa: E402


def fsm_trace(packets):
    out = io.StringIO()
    m = fsm.fsm(out=out)
    for t, bits in packets:
        m.process_bits(bits, t)
    return out.getvalue()


def main():
    iq = np.load(os.path.join(HERE, 'fx_ultralight_iq.npz'))['iq']
    gold = open(os.path.join(HERE, 'ultralight.out')).read().rstrip('\n')
    env = api.host_envelope(iq, api.NFC_IN_IQ_F32)
    p = dict(mg.DEFAULTS, hi_val=1.09)
    kw = dict(samp_rate=p['samp_rate'], hi_val=p['hi_val'], lo_val=p['lo_val'], av_window=p['av_window'],
              max_len=p['max_len'], reader=p['reader'], tag=p['tag'])
    own = mg.run_reference(env, chunk=8192, **dict(kw, hi_val=1.1))   # the fc32 capture itself (the UHD branch)
    for gain in (32767.0, 4096.0, 512.0, 131068.0):
        pcm = api.host_record_pcm16(env, gain)
        x = api.host_envelope(pcm, api.NFC_IN_I16_SQ, 0.0)
        a = mg.run_reference(x, chunk=8192, **kw)
        b = mg.run_reference(x, chunk=4096, rng=np.random.default_rng(7), **kw)
        assert a == b, 'reference is not chunk-invariant on the recording at gain %g' % gain
        clipped = int(np.count_nonzero(np.abs(pcm.astype(np.int32)) == 32767))
        print('gain %g: N=%d peak=%d clipped=%d transitions=%d sym_tag=%d sym_reader=%d packets=%d; packets and symbols of the fc32 '
              'capture: %s' % (gain, len(x), int(np.abs(pcm.astype(np.int32)).max()), clipped, len(a[0]), len(a[1]), len(a[2]), len(a[3]),
                               'yes' if (a[1], a[2], a[3]) == (own[1], own[2], own[3]) else 'NO'))
        if gain == 32767.0:
            assert (a[1], a[2], a[3]) == (own[1], own[2], own[3]), 'the default-gain recording does not decode like the capture'
            out = mg.pack(x, p, a)
            out['pcm'] = pcm
            np.savez_compressed(os.path.join(HERE, 'fx_ultralight_rec16.npz'), **out)
            print('fx_ultralight_rec16: fsm prints ultralight.out: %s' % ('yes' if fsm_trace(a[3]).rstrip('\n') == gold else 'NO'))


if __name__ == '__main__':
    main()
