#!/usr/bin/env python3
"""Complex 8-bit input (NFC_IN_IQ_I8 sc8 and NFC_IN_IQ_U8 cu8, 2 B/sample) against sc16 (4 B/sample) and fc32 IQ (8 B/sample), in the same
call.  Kept under tests/ like iq16_bench.py (not collected by pytest); prints one JSON line.

  resident   BASELINE configs[1] (the synthetic `miller` workload, 1e8 samples at 2 Msps) quantised to sc8 and to cu8, each with its twins
             that carry the same converted values: sc8's sc16 twin (the same integers, i16_scale 2^-7) and fc32 twin, cu8's fc32 twin; all
             resident in HBM; timed steps alternate (host clock around a synchronised step), the threshold launch from nfc_set_timing(1)
             events; the output digests of twins must be equal.  sc8 / cu8 at the default scale run the integer route, and once more at
             scale 1/100 (the float route, against that scale's fc32 twin)
  host_fed   pinned host samples -> uploads on a thread (a ring of device buffers) -> nfc_submit_device / nfc_wait (two in flight)
             -> edges (compact) and packets read back; the same loop for sc8, sc16 and fc32 (4 Mi-sample pieces), at least `secs` seconds
             of streaming each; sc8 once more in 8 Mi-sample pieces (sc16's bytes per batch)
  nr8        the 10 Msps window (av_window 10000, max_len 250): sc8 with four against eight rows per step of the workgroup kernel
             (NFC_WG_NR, the test build), same call, alternating
  valu       VALU instructions per 64-sample row of each route in k_threshold_wg<KIND, 4> and <KIND, 8>, read from the ISA of nfc_iq8.hip

    python tests/iq8_bench.py [samples] [steps] [secs]"""
import ctypes as C
import hashlib
import json
import os
import re
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
# name: (kind, bytes per sample, scale)
KINDS = {'sc8': (api.NFC_IN_IQ_I8, 2, 0.0), 'cu8': (api.NFC_IN_IQ_U8, 2, 0.0), 'sc16': (api.NFC_IN_IQ_I16, 4, 2.0 ** -7),
         'fc32': (api.NFC_IN_IQ_F32, 8, 0.0), 'fc32_cu8': (api.NFC_IN_IQ_F32, 8, 0.0),
         'sc8_float': (api.NFC_IN_IQ_I8, 2, 0.01), 'fc32_float': (api.NFC_IN_IQ_F32, 8, 0.0)}
TWINS = [('sc8', 'sc16'), ('sc8', 'fc32'), ('cu8', 'fc32_cu8'), ('sc8_float', 'fc32_float')]


def capture():
    iq = synth.workload('miller', n)
    sc8 = np.empty(iq.size, np.int8)
    cu8 = np.empty(iq.size, np.uint8)
    for o in range(0, iq.size, 1 << 24):   # (in pieces: the float64 intermediate of the whole capture would be 1.6 GB)
        sc8[o:o + (1 << 24)] = synth.quantise_sc8(iq[o:o + (1 << 24)])
        cu8[o:o + (1 << 24)] = synth.quantise_cu8(iq[o:o + (1 << 24)])
    del iq
    return {'sc8': sc8, 'cu8': cu8, 'sc16': sc8.astype(np.int16), 'fc32': api.host_iq8_to_float(sc8, api.NFC_IN_IQ_I8),
            'fc32_cu8': api.host_iq8_to_float(cu8, api.NFC_IN_IQ_U8), 'sc8_float': sc8,
            'fc32_float': api.host_iq8_to_float(sc8, api.NFC_IN_IQ_I8, 0.01)}


def digest(ctx):
    m = hashlib.sha256()
    pos, code = ctx.edges_compact()
    for a in (pos, code, ctx.symbols(0), ctx.symbols(1), ctx.packet_table(0), ctx.packet_table(1), ctx.packet_bits(0), ctx.packet_bits(1)):
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()[:16], int(len(pos))


def resident(caps, names=tuple(KINDS)):
    bufs = {k: api.DeviceBuffer(caps[k]) for k in names}
    ctxs = {k: api.NfcContext(input_kind=KINDS[k][0], i16_scale=KINDS[k][2], **PARAMS) for k in names}
    for k in names:   # warm-up: buffers sized, kernels loaded
        for _ in range(3):
            ctxs[k].push_device(bufs[k], n)
        ctxs[k].sync()
    acc = {k: dict(ms=[], kernel_ms=[]) for k in names}
    for i in range(steps):
        for k in (names if i % 2 == 0 else list(names)[::-1]):   # (alternating, and the order flips every step)
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
    for k in names:
        bps = KINDS[k][1]
        ms = float(np.median(acc[k]['ms']))
        kms = float(np.median(acc[k]['kernel_ms']))
        dg, ne = digest(ctxs[k])
        st = ctxs[k].stats()
        out[k] = dict(ms_per_step_median=ms, ms_per_step_mean=float(np.mean(acc[k]['ms'])), ms_per_step_min=float(np.min(acc[k]['ms'])),
                      threshold_launch_ms_median=kms, bytes_per_sample=bps, scale=KINDS[k][2], digest=dg, edges=ne,
                      used_sequential=int(st.used_sequential), chunks_rerun=int(st.chunks_rerun))
        ctxs[k].close()
        bufs[k].free()
    for a, b in TWINS:
        out['step_ratio_%s_over_%s' % (a, b)] = out[a]['ms_per_step_median'] / out[b]['ms_per_step_median']
        out['launch_ratio_%s_over_%s' % (a, b)] = out[a]['threshold_launch_ms_median'] / out[b]['threshold_launch_ms_median']
        out['digests_equal_%s_%s' % (a, b)] = out[a]['digest'] == out[b]['digest']
    return out


def nr8():
    """sc8 at 10 Msps (av_window 10000): k_threshold_wg with four against eight rows per step, same call (the test build's NFC_WG_NR)."""
    from usrp_nfc_amd import build as _build
    m = 40_000_000
    x = synth.quantise_sc8(synth.workload('all', m, rate_msps=10.0))
    p = dict(samp_rate=10e6, hi_val=1.1, av_window=10000, max_len=250)
    buf = api.DeviceBuffer(x)
    ctxs = {}
    for nr in (4, 8):
        os.environ['NFC_WG_NR'] = str(nr)
        ctxs[nr] = api.NfcContext(input_kind=api.NFC_IN_IQ_I8, lib_path=_build.SO_HOOKS, **p)
    del os.environ['NFC_WG_NR']
    for c in ctxs.values():
        for _ in range(3):
            c.push_device(buf, m)
        c.sync()
    acc = {nr: dict(ms=[], kernel_ms=[]) for nr in ctxs}
    for i in range(steps):
        for nr in ((4, 8) if i % 2 == 0 else (8, 4)):
            c = ctxs[nr]
            c.set_timing(1)
            t0 = time.perf_counter()
            c.push_device(buf, m)
            c.sync()
            acc[nr]['ms'].append((time.perf_counter() - t0) * 1e3)
            st = c.stats()
            acc[nr]['kernel_ms'].extend(st.ms_threshold_kernel[j] for j in range(st.n_threshold_timed))
            c.set_timing(0)
    out = {}
    for nr, c in ctxs.items():
        out['nr%d' % nr] = dict(ms_per_step_median=float(np.median(acc[nr]['ms'])), threshold_launch_ms_median=float(np.median(acc[nr]['kernel_ms'])),
                                digest=digest(c)[0])
        c.close()
    buf.free()
    out['launch_ratio_nr8_over_nr4'] = out['nr8']['threshold_launch_ms_median'] / out['nr4']['threshold_launch_ms_median']
    out['step_ratio_nr8_over_nr4'] = out['nr8']['ms_per_step_median'] / out['nr4']['ms_per_step_median']
    out.update(samples=m, workload='all at 10 Msps', av_window=10000, max_len=250)
    return out


def route_valu(text, kind, nr):
    """VALU instructions per 64-sample row of each route of k_threshold_wg<kind, nr>: the blocks behind the regular round's take."""
    name = '_ZN3nfc14k_threshold_wgILi%dELi%dELb0EEEvNS_7ThrArgsE' % (kind, nr)
    body = re.search(r'^%s:(.*?)\.end_amdhsa_kernel' % name, text, re.S | re.M).group(1).split('\n')
    takes = [i for i, l in enumerate(body) if 's_waitcnt vmcnt(0)' in l and 'v_accvgpr_read_b32' in body[i + 1] and 'a0' in body[i + 1]]
    out = {}
    for t in takes:
        j = t
        while 'ASMEND' not in body[j]:
            j += 1
        blocks, cur = [], []
        for l in body[j + 1:j + 200]:
            if re.match(r'^(\.LBB|; %bb\.)', l):
                blocks.append(cur)
                cur = []
                if len(blocks) >= 4:
                    break
                continue
            code = l.split(';')[0].strip()
            if code:
                cur.append(code)
        got = {}
        for b in blocks:
            v = [c for c in b if c.startswith('v_')]
            if any(c.startswith('v_dot4') for c in v):
                got['integer'] = len(v) / nr
            elif any(c.startswith(('v_cvt_f32', 'v_pk_mul_f32')) for c in v) and 'float' not in got:
                got['float'] = len(v) / nr
        if len(got) == 2:
            out = got
    return out


def valu():
    import subprocess
    import tempfile
    from usrp_nfc_amd import build as _build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = [f for f in _build.FLAGS if f not in ('-fPIC', '-shared')]
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, 'nfc_iq8.s')
        subprocess.check_call([hipcc] + flags + ['-S', '--cuda-device-only', os.path.join(_build.CSRC, 'nfc_iq8.hip'), '-o', asm],
                              stderr=subprocess.DEVNULL)
        text = open(asm).read()
    return {'%s_wg%d' % (nm, nr): route_valu(text, k, nr) for nm, k in (('sc8', api.NFC_IN_IQ_I8), ('cu8', api.NFC_IN_IQ_U8)) for nr in (4, 8)}


def host_fed(x, kind, bps, scale=0.0, piece=1 << 22):
    L = _lib.load()
    per = api._KIND_DTYPE[kind][1]
    pin = C.c_void_p()
    assert L.nfc_host_alloc_pinned(x.nbytes, C.byref(pin)) == 0
    C.memmove(pin, x.ctypes.data, x.nbytes)
    NB = 4
    bufs = [api.DeviceBuffer(np.zeros(0, np.float32), 0, nbytes=bps * piece) for _ in range(NB)]
    ctx = api.NfcContext(input_kind=kind, i16_scale=scale, **PARAMS)
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
    if 'valu' in sys.argv:   # (the ISA only: no GPU)
        print(json.dumps(dict(valu_per_row=valu())))
        return
    caps = capture()
    if 'trace' in sys.argv:   # (the kernel trace's run: resident sc8 and cu8 steps -- rocprofv3 --kernel-trace --stats -- python tests/iq8_bench.py N STEPS 0 trace)
        for k in ('sc8', 'cu8'):
            buf = api.DeviceBuffer(caps[k])
            with api.NfcContext(input_kind=KINDS[k][0], **PARAMS) as ctx:
                for _ in range(steps):
                    ctx.push_device(buf, n)
                ctx.sync()
            buf.free()
        print(json.dumps(dict(trace='sc8 then cu8 resident steps', samples=n, steps=steps)))
        return
    res = resident(caps)
    fed = {k: host_fed(caps[k], KINDS[k][0], KINDS[k][1], KINDS[k][2]) for k in ('sc8', 'sc16', 'fc32')}
    fed['msamples_ratio_sc8_over_sc16'] = fed['sc8']['msamples_s'] / fed['sc16']['msamples_s']
    fed['msamples_ratio_sc8_over_fc32'] = fed['sc8']['msamples_s'] / fed['fc32']['msamples_s']
    # (the same bytes per batch as sc16's 4 Mi-sample pieces: whether sc8's rate is set by the link or by the batches)
    fed['sc8_pieces_8Mi'] = host_fed(caps['sc8'], *KINDS['sc8'], piece=1 << 23)
    del caps
    print(json.dumps(dict(what='sc8 / cu8 (NFC_IN_IQ_I8 / U8) vs sc16 and fc32 IQ, same capture, same call', workload='miller', samples=n,
                          steps=steps, resident=res, host_fed=fed, nr8=nr8(), valu_per_row=valu(), box=os.uname().nodename)))


if __name__ == '__main__':
    main()
