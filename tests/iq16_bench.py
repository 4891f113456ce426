#!/usr/bin/env python3
"""Complex int16 input (NFC_IN_IQ_I16, sc16, 4 B/sample) against fc32 IQ (8 B/sample) on the same capture, in the same call.  Kept
under tests/ like tx_bench.py (not collected by pytest); prints one JSON line.

  resident   BASELINE configs[1] (the synthetic `miller` workload, 1e8 samples at 2 Msps) quantised to sc16, and its host-converted
             fc32 twin, both resident in HBM; timed steps of the two alternate (host clock around a synchronised step), the threshold
             launch from nfc_set_timing(1) events; output digests of the two kinds must be equal
  host_fed   pinned host samples -> uploads on a thread (a ring of device buffers) -> nfc_submit_device / nfc_wait (two in flight)
             -> edges (compact) and packets read back; the same loop for both kinds, at least `secs` seconds of streaming each

    python tests/iq16_bench.py [samples] [steps] [secs]"""
import ctypes as C
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usrp_nfc_amd import _lib, api, synth   # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
secs = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0
PARAMS = dict(samp_rate=2e6, hi_val=1.1, reader=True, tag=False)   # configs[1]: Miller only
KINDS = {'sc16': (api.NFC_IN_IQ_I16, 4), 'fc32': (api.NFC_IN_IQ_F32, 8)}


def capture():
    iq = synth.workload('miller', n)
    iq16 = np.empty(iq.size, np.int16)
    for o in range(0, iq.size, 1 << 24):   # (in pieces: the float64 intermediate of the whole capture would be 1.6 GB)
        iq16[o:o + (1 << 24)] = synth.quantise_sc16(iq[o:o + (1 << 24)])
    del iq
    return {'sc16': iq16, 'fc32': api.host_i16_to_float(iq16)}


def digest(ctx):
    m = hashlib.sha256()
    pos, code = ctx.edges_compact()
    for a in (pos, code, ctx.symbols(0), ctx.symbols(1), ctx.packet_table(0), ctx.packet_table(1), ctx.packet_bits(0), ctx.packet_bits(1)):
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()[:16], int(len(pos))


def resident(caps):
    bufs = {k: api.DeviceBuffer(caps[k]) for k in KINDS}
    ctxs = {k: api.NfcContext(input_kind=KINDS[k][0], **PARAMS) for k in KINDS}
    for k in KINDS:   # warm-up: buffers sized, kernels loaded
        for _ in range(3):
            ctxs[k].push_device(bufs[k], n)
        ctxs[k].sync()
    acc = {k: dict(ms=[], kernel_ms=[]) for k in KINDS}
    for i in range(steps):
        for k in (KINDS if i % 2 == 0 else list(KINDS)[::-1]):   # (alternating, and the order flips every step)
            ctx = ctxs[k]
            ctx.set_timing(1)
            t0 = time.perf_counter()
            ctx.push_device(bufs[k], n)
            ctx.sync()
            acc[k]['ms'].append((time.perf_counter() - t0) * 1e3)
            st = ctx.stats()
            acc[k]['kernel_ms'].extend(st.ms_threshold_kernel[j] for j in range(st.n_threshold_timed))
            ctx.set_timing(0)
    out = {}
    for k, (_, bps) in KINDS.items():
        ms = float(np.median(acc[k]['ms']))
        kms = float(np.median(acc[k]['kernel_ms']))
        dg, ne = digest(ctxs[k])
        st = ctxs[k].stats()
        out[k] = dict(ms_per_step_median=ms, ms_per_step_mean=float(np.mean(acc[k]['ms'])), ms_per_step_min=float(np.min(acc[k]['ms'])),
                      threshold_launch_ms_median=kms, bytes_per_sample=bps, frac_of_8TBps_step=bps * n / (ms * 1e-3) / 8e12,
                      frac_of_8TBps_threshold_launch=bps * n / (kms * 1e-3) / 8e12, digest=dg, edges=ne,
                      used_sequential=int(st.used_sequential), chunks_rerun=int(st.chunks_rerun))
        ctxs[k].close()
        bufs[k].free()
    out['step_ratio_sc16_over_fc32'] = out['sc16']['ms_per_step_median'] / out['fc32']['ms_per_step_median']
    out['launch_ratio_sc16_over_fc32'] = out['sc16']['threshold_launch_ms_median'] / out['fc32']['threshold_launch_ms_median']
    out['digests_equal'] = out['sc16']['digest'] == out['fc32']['digest']
    return out


def host_fed(x, kind, bps):
    L = _lib.load()
    per = api._KIND_DTYPE[kind][1]
    piece = 1 << 22
    pin = C.c_void_p()
    assert L.nfc_host_alloc_pinned(x.nbytes, C.byref(pin)) == 0
    C.memmove(pin, x.ctypes.data, x.nbytes)
    NB = 4
    bufs = [api.DeviceBuffer(np.zeros(0, np.float32), 0, nbytes=bps * piece) for _ in range(NB)]
    ctx = api.NfcContext(input_kind=kind, **PARAMS)
    outs = [(api.PinnedArray(piece // 4 + 65536, np.uint32), api.PinnedArray(piece // 4 + 65536, np.uint16)) for _ in range(2)]
    total = len(x) // per
    offs = [(o, min(piece, total - o)) for o in range(0, total, piece)]

    def one_pass(n_pieces):
        uploaded = [threading.Event() for _ in range(n_pieces)]
        free = [threading.Event() for _ in range(n_pieces)]   # piece k's buffer may be overwritten (its wait has returned)
        err = []

        def uploader():
            try:
                for k in range(n_pieces):
                    if k >= NB:
                        free[k - NB].wait()
                    o, m = offs[k % len(offs)]
                    assert L.nfc_device_upload(0, bufs[k % NB].ptr, pin.value + bps * o, bps * m) == 0
                    uploaded[k].set()
            except Exception as e:   # (the main thread must not wait for ever)
                err.append(e)
                for ev in uploaded:
                    ev.set()

        th = threading.Thread(target=uploader, daemon=True)
        t0 = time.perf_counter()
        th.start()
        done, n_edges, n_pk, n_bits, ahead, nxt = 0, 0, 0, 0, 0, 0
        for k in range(n_pieces):
            while nxt < n_pieces and nxt < k + 2:
                uploaded[nxt].wait()
                if err:
                    raise err[0]
                ctx.submit_device(bufs[nxt % NB], offs[nxt % len(offs)][1])
                nxt += 1
            ctx.wait()
            free[k].set()
            pos, code = ctx.edges_compact(out=(outs[k & 1][0].array, outs[k & 1][1].array))   # (the copy engine writes pinned arrays)
            n_edges += len(pos)
            tabs = [ctx.packet_table(t) for t in (0, 1)]
            bits = [ctx.packet_bits(t) for t in (0, 1)]
            n_pk += sum(len(t) for t in tabs)
            n_bits += sum(len(b) for b in bits)
            ahead += int(ctx.stats().ran_ahead)
            done += offs[k % len(offs)][1]
        th.join()
        dt = time.perf_counter() - t0
        return dict(msamples_s=done / dt / 1e6, GBs_in=bps * done / dt / 1e9, seconds=dt, samples=done, edges=n_edges, packets=n_pk, packet_bits=n_bits,
                    batches_ran_ahead=ahead, batches=n_pieces)

    one_pass(min(8, len(offs)))   # (the first batches size the context's buffers)
    r = one_pass(len(offs))
    while r['seconds'] < secs:   # (at least `secs` of streaming: the next pass longer by what the last one fell short, and 5 %)
        r = one_pass(int(np.ceil(r['batches'] * secs / r['seconds'] * 1.05)))
    ctx.close()
    for b in bufs:
        b.free()
    for a, b in outs:
        a.free()
        b.free()
    L.nfc_host_free_pinned(pin)
    r.update(bytes_per_sample=bps, piece_samples=piece)
    return r


def main():
    caps = capture()
    if 'trace' in sys.argv:   # (the kernel trace's run: resident sc16 steps only -- rocprofv3 --kernel-trace --stats -- python tests/iq16_bench.py N STEPS 0 trace)
        buf = api.DeviceBuffer(caps['sc16'])
        with api.NfcContext(input_kind=api.NFC_IN_IQ_I16, **PARAMS) as ctx:
            for _ in range(steps):
                ctx.push_device(buf, n)
            ctx.sync()
        buf.free()
        print(json.dumps(dict(trace='sc16 resident steps', samples=n, steps=steps)))
        return
    res = resident(caps)
    fed = {k: host_fed(caps[k], *KINDS[k]) for k in ('sc16', 'fc32')}
    fed['msamples_ratio_sc16_over_fc32'] = fed['sc16']['msamples_s'] / fed['fc32']['msamples_s']
    print(json.dumps(dict(what='sc16 (NFC_IN_IQ_I16) vs fc32 IQ, same capture, same call', workload='miller', samples=n, steps=steps,
                          resident=res, host_fed=fed, box=os.uname().nodename)))


if __name__ == '__main__':
    main()
