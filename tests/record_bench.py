#!/usr/bin/env python3
"""The recording kernel (k_record_pcm16, nfc_record_pcm16_device) against the threshold launch that reads the same buffer, in the
same call.  Kept under tests/ like iq8_bench.py (not collected by pytest); prints one JSON line.

  kernels    BASELINE configs[1] (the synthetic `miller` workload, 1e8 samples at 2 Msps) as fc32, sc16, sc8 and cu8, resident in
             HBM; per kind, alternating within every step: the record kernel on one buffer ("same": event time, algorithmic
             bytes/s = (bytes_in + 2 n) / t), on four distinct buffers stepped round-robin ("cold": 4 x the capture is far beyond
             the 256 MiB Infinity Cache, so this is the kernel's share of the achievable HBM bandwidth), both once more with
             non-temporal input loads (the test build's NFC_REC_NT), and the unchanged threshold launch of the kind on the same
             buffer (nfc_set_timing(1), ms_threshold_kernel[0]).  fc32 also with the real-part tap.  The yardstick: fc32's record
             kernel moves 10 B/sample where the threshold launch moves 8, so launch x 10/8; the other kinds' threshold launch is
             instruction-bound, the record kernel should simply be faster
  decoder    decoder(src = the fc32 capture as an array).run() with dst on tmpfs and without: Msamples/s, and the parts of the
             difference measured by themselves per 2^22-sample batch -- the kernel (events), the PCM download, wave's write

    python tests/record_bench.py [samples] [steps] [decoder_samples]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usrp_nfc_amd import _lib, api, build as _build, decoder as dec, record as rec_mod, synth   # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
n_dec = int(float(sys.argv[3])) if len(sys.argv) > 3 else n
PARAMS = dict(samp_rate=2e6, hi_val=1.1, reader=True, tag=False)   # configs[1]: Miller only
COPY_TBS = 6.29   # the achievable copy bandwidth of one MI355X (read + write), TB/s
# name: (kind, bytes per sample, tap)
KINDS = {'fc32': (api.NFC_IN_IQ_F32, 8, api.NFC_REC_ENVELOPE), 'sc16': (api.NFC_IN_IQ_I16, 4, api.NFC_REC_ENVELOPE),
         'sc8': (api.NFC_IN_IQ_I8, 2, api.NFC_REC_ENVELOPE), 'cu8': (api.NFC_IN_IQ_U8, 2, api.NFC_REC_ENVELOPE),
         'fc32_real_part': (api.NFC_IN_IQ_F32, 8, api.NFC_REC_REAL_PART)}


def pieces(f, iq, dtype):
    out = np.empty(iq.size, dtype)
    for o in range(0, iq.size, 1 << 24):   # (in pieces: the float64 intermediate of the whole capture would be 1.6 GB)
        out[o:o + (1 << 24)] = f(iq[o:o + (1 << 24)])
    return out


def record_ms(L, kind, tap, src, out, nt):
    os.environ['NFC_REC_NT'] = '1' if nt else '0'   # (read per call by the test build; the product build has no such switch)
    ms = C.c_float(0)
    rc = L.nfc_record_pcm16_device(0, tap, kind, 0.0, src.ptr, n, 32767.0, out.ptr, None, C.byref(ms))
    assert rc == 0, L.nfc_last_error(None)
    return float(ms.value)


def kernels(name, x):
    kind, bps, tap = KINDS[name]
    Lp, Lh = _lib.load(), _lib.load(_build.SO_HOOKS)
    bufs = [api.DeviceBuffer(x) for _ in range(4)]
    out = api.DeviceBuffer(np.zeros(0, np.int16), nbytes=2 * n)
    ctx = api.NfcContext(input_kind=kind, **PARAMS)
    for _ in range(3):   # warm-up: buffers sized, kernels loaded
        ctx.push_device(bufs[0], n)
        ctx.sync()
        record_ms(Lp, kind, tap, bufs[0], out, False)
        record_ms(Lh, kind, tap, bufs[0], out, True)
        record_ms(Lh, kind, tap, bufs[0], out, False)
    forms = {'same': (Lp, False, False), 'cold': (Lp, False, True), 'same_test_build': (Lh, False, False), 'cold_test_build': (Lh, False, True),
             'same_nontemporal': (Lh, True, False), 'cold_nontemporal': (Lh, True, True)}
    acc = {k: [] for k in list(forms) + ['threshold']}
    for i in range(steps):
        order = list(forms) + ['threshold']
        for k in (order if i % 2 == 0 else order[::-1]):   # (alternating, and the order flips every step)
            if k == 'threshold':
                ctx.set_timing(1)
                ctx.push_device(bufs[0], n)
                ctx.sync()
                st = ctx.stats()
                acc[k].append(float(st.ms_threshold_kernel[0]))
                n_timed = int(st.n_threshold_timed)
                ctx.set_timing(0)
            else:
                L, nt, cold = forms[k]
                acc[k].append(record_ms(L, kind, tap, bufs[(i + 1) % 4 if cold else 0], out, nt))
    st = ctx.stats()
    res = dict(bytes_per_sample=bps, threshold_launch_ms_median=float(np.median(acc['threshold'])), threshold_launches_timed=n_timed,
               used_sequential=int(st.used_sequential), chunks_rerun=int(st.chunks_rerun))
    for k in forms:
        ms = float(np.median(acc[k]))
        tbs = (bps + 2) * n / (ms * 1e-3) / 1e12
        res[k] = dict(ms_median=ms, ms_min=float(np.min(acc[k])), algorithmic_TBs=tbs, share_of_copy_bandwidth=tbs / COPY_TBS)
    yard = res['threshold_launch_ms_median'] * (10.0 / 8.0 if bps == 8 else 1.0)
    res.update(yardstick_ms=yard, record_over_yardstick=res['same']['ms_median'] / yard, cold_over_yardstick=res['cold']['ms_median'] / yard,
               nontemporal_over_plain_same=res['same_nontemporal']['ms_median'] / res['same_test_build']['ms_median'],
               nontemporal_over_plain_cold=res['cold_nontemporal']['ms_median'] / res['cold_test_build']['ms_median'])
    ctx.close()
    for b in bufs + [out]:
        b.free()
    return res


def decoder_cost(iq):
    m = min(n_dec, len(iq) // 2)
    src = iq[:2 * m].view(np.complex64)
    tmp = '/dev/shm' if os.path.isdir('/dev/shm') else tempfile.gettempdir()
    path = os.path.join(tmp, 'record_bench_%d.wav' % os.getpid())
    batch = 1 << 22
    out = {}
    try:
        for rep in range(2):   # (the first round warms both paths up)
            for name, dst in (('plain', None), ('dst', path)):
                d = dec.decoder(src=src, dst=dst, reader=True, tag=False, keep=0, fsm=type('F', (), {'process_bits': lambda s, b, t: None})())
                t0 = time.perf_counter()
                d.run()
                out[name] = dict(seconds=time.perf_counter() - t0)
                out[name]['msamples_s'] = m / out[name]['seconds'] / 1e6
                d._trans.close()
        # the parts, per batch of 2^22 samples, by themselves
        b = min(batch, m)
        buf = api.DeviceBuffer(iq[:2 * b])
        pcm = api.DeviceBuffer(np.zeros(0, np.int16), nbytes=2 * b)
        kms, dl, wr = [], [], []
        for _ in range(8):
            kms.append(api.record_pcm16_device(buf, b, pcm, api.NFC_IN_IQ_F32, timed=True))
            t0 = time.perf_counter()
            host = pcm.download(2 * b).view(np.int16)
            dl.append((time.perf_counter() - t0) * 1e3)
            w = rec_mod.record(path)
            t0 = time.perf_counter()
            w.write_pcm(host)
            wr.append((time.perf_counter() - t0) * 1e3)
            w.close()
        buf.free()
        pcm.free()
        nb = (m + batch - 1) // batch
        out.update(samples=m, batch=batch, batches=nb, wav_on=tmp, extra_seconds=out['dst']['seconds'] - out['plain']['seconds'],
                   per_batch_ms=dict(record_kernel=float(np.median(kms)), pcm_download=float(np.median(dl)), wave_write=float(np.median(wr))),
                   msamples_ratio_dst_over_plain=out['dst']['msamples_s'] / out['plain']['msamples_s'])
    finally:
        if os.path.exists(path):
            os.remove(path)
    return out


def main():
    iq = synth.workload('miller', n)
    res = {}
    res['fc32'] = kernels('fc32', iq)
    res['fc32_real_part'] = kernels('fc32_real_part', iq)
    d = decoder_cost(iq)
    res['sc16'] = kernels('sc16', pieces(synth.quantise_sc16, iq, np.int16))
    res['sc8'] = kernels('sc8', pieces(synth.quantise_sc8, iq, np.int8))
    res['cu8'] = kernels('cu8', pieces(synth.quantise_cu8, iq, np.uint8))
    print(json.dumps(dict(what='k_record_pcm16 vs the threshold launch on the same buffer, same call', workload='miller', samples=n, steps=steps,
                          copy_bandwidth_TBs=COPY_TBS, kernels=res, decoder=d, box=os.uname().nodename)))


if __name__ == '__main__':
    main()
