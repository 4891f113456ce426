"""The air interface (include/nfc_amd.h: nfc_air_*, csrc/air.hip.h): K ragged lists of on-air frames become K IQ captures in ONE
device buffer -- what an eavesdropper's radio would have recorded of K transactions, in any of the four IQ input kinds -- ready for
``NfcMultiContext.push_device`` without touching the host.  The stage between ``emulate.pairs_device`` and the decoder.

``frames_of`` packs an ``emulate.Transcripts``, a list of ``Transcript``s or a list of (direction, bits) lists (synth.frames_from_trace,
synth.txn_frames) into the arrays the library takes; ``render_device`` renders them on the GPU, ``host_render`` on one CPU core (the twin:
the same bytes); both return an ``AirCaptures``.  The signal is synth.py's (modulation_profile, iq_from_profile, quantise_*) with a
counter-based noise in the place of PCG64's normals: with sigma 0 the bytes are synth's.  There is no fall-back from the GPU call to the twin."""
import ctypes as C
import math

import numpy as np

from . import _lib, synth
from ._lib import AIR_FRAME_DTYPE, NFC_IN_IQ_F32, NFC_IN_IQ_I8, NFC_IN_IQ_I16, NFC_IN_IQ_U8

KIND_DTYPE = {NFC_IN_IQ_F32: np.float32, NFC_IN_IQ_I16: np.int16, NFC_IN_IQ_I8: np.int8, NFC_IN_IQ_U8: np.uint8}
FULL_SCALE = {NFC_IN_IQ_F32: 1.0, NFC_IN_IQ_I16: 32767.0, NFC_IN_IQ_I8: 127.0, NFC_IN_IQ_U8: 127.0}   # synth.quantise_*'s defaults
GUARD_BYTES, GUARD_BYTE = 16, 0xA5


class AirError(RuntimeError):
    pass


def _fail(name, rc):
    msg = _lib.load().nfc_last_error(None)
    text = '%s status %d: %s' % (name, rc, (msg or b'').decode())
    raise (ValueError if rc == -1 else AirError)(text)


class AirFrames(object):
    """K streams' frames as the library takes them: `frames` AIR_FRAME_DTYPE records, stream k's at frame_off[k] .. frame_off[k + 1]; their
    bytes and ninth bits in `air` / `par`, stream k's part at byte_base[k] .. byte_base[k + 1]; `tail` idle samples behind a stream's last
    frame; rate_msps the rate the idle counts were made for."""

    def __init__(self, frames, frame_off, air, par, byte_base, tail, rate_msps):
        self.frames = np.ascontiguousarray(frames, AIR_FRAME_DTYPE)
        self.frame_off = np.ascontiguousarray(frame_off, np.uint32)
        self.air, self.par = np.ascontiguousarray(air, np.uint8).reshape(-1), np.ascontiguousarray(par, np.uint8).reshape(-1)
        self.byte_base = np.ascontiguousarray(byte_base, np.uint32)
        self.tail, self.rate_msps = int(tail), float(rate_msps)

    def __len__(self):
        return len(self.frame_off) - 1

    def bound_samples(self, align_samples=1):
        """A cheap upper bound of the samples a rendering needs: idle + (n_bits + 2) * ceil(9.44 * rate) per frame, the tail and the
        alignment's padding per stream."""
        per_bit = int(math.ceil(synth.T_FULL * self.rate_msps))
        f = self.frames
        n = int(f['idle_before'].astype(np.uint64).sum()) + int(((f['n_bits'].astype(np.uint64) + 2) * per_bit).sum())
        return n + len(self) * (self.tail + int(align_samples) - 1)


def _pack_bits(bits):
    """on-air data bits -> (n_bits, bytes, ninth bits): up to eight bits a short frame in one byte, else nine bits a byte"""
    b = np.asarray(list(bits), np.uint8)
    if b.size and int(b.max()) > 1:
        raise ValueError('a bit is 0 or 1')
    if b.size <= 8:
        return b.size, [int((b.astype(np.uint32) << np.arange(b.size, dtype=np.uint32)).sum())] if b.size else [], [0] if b.size else []
    if b.size % 9:
        raise ValueError('a frame of %d bits: neither a short frame nor nine bits a byte' % b.size)
    rows = b.reshape(-1, 9)
    return b.size, (rows[:, :8].astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=1).tolist(), rows[:, 8].tolist()


def frames_of(source, rate_msps=2.0, gap_us=150.0, lead_in=3000, tail=400):
    """Pack an emulate.Transcripts, a list of emulate.Transcript or a list of (direction, bits) lists into an AirFrames.  The keywords mean
    what synth.modulation_profile means by them: a stream's first frame has lead_in idle samples in front, every later one
    int(gap_us * rate_msps), and behind the last frame lie that gap and `tail` more."""
    from . import emulate
    gap = int(gap_us * rate_msps)
    if isinstance(source, AirFrames):
        return source
    if isinstance(source, emulate.Transcripts):
        K, cap = source.frames.shape
        n = np.minimum(source.results['n_frames'].astype(np.int64), cap)
        cut = (source.results['flags'] & (_lib.NFC_EMU_PAIR_CUT_FRAMES | _lib.NFC_EMU_PAIR_CUT_BYTES)) != 0
        for k in np.nonzero(cut)[0]:   # (what lies before the first frame that did not fit: Transcript's own rule)
            n[k] = len(source.transcript(int(k)))
        keep = np.arange(cap)[None, :] < n[:, None]
        src = source.frames[keep]
        out = np.zeros(len(src), AIR_FRAME_DTYPE)
        out['type'], out['n_bits'], out['byte_off'] = src['type'], src['n_bits'], src['byte_off']
        frame_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
        out['idle_before'] = gap
        out['idle_before'][frame_off[:-1][n > 0]] = int(lead_in)
        byte_base = np.arange(K + 1, dtype=np.uint64) * source.air.shape[1]
        return AirFrames(out, frame_off, source.air, source.par, byte_base, gap + int(tail), rate_msps)
    recs, frame_off, air, par, byte_base = [], [0], [], [], [0]
    for stream in source:
        if isinstance(stream, emulate.Transcript):
            stream = emulate.synth_frames(stream)
        for i, (direction, bits) in enumerate(stream):
            nb, by, pa = _pack_bits(bits)
            recs.append((int(direction), 0, nb, len(air) - byte_base[-1], int(lead_in) if i == 0 else gap, 0))
            air += by
            par += pa
        frame_off.append(len(recs))
        byte_base.append(len(air))
    return AirFrames(np.array(recs, AIR_FRAME_DTYPE), frame_off, air, par, byte_base, gap + int(tail), rate_msps)


class AirCaptures(object):
    """K captures in one buffer: stream k's n_samples[k] samples start first_sample[k] samples behind its start.  `buf` is the
    api.DeviceBuffer of a render_device (free() releases it), `data` the bytes of a host_render; kernel_ms: (layout, render) of a
    timed render_device."""

    def __init__(self, kind, first_sample, n_samples, cap_samples, buf=None, data=None, kernel_ms=None, device=0):
        self.kind, self.first_sample, self.n_samples, self.cap_samples = int(kind), first_sample, n_samples, int(cap_samples)
        self.buf, self.data, self.kernel_ms, self.device = buf, data, kernel_ms, device
        self.bytes_per_sample = 2 * np.dtype(KIND_DTYPE[self.kind]).itemsize
        self.call_s = None

    def __len__(self):
        return len(self.n_samples)

    @property
    def used_samples(self):
        """the samples from the buffer's start to the end of the last stream: every byte of them is written"""
        return int(self.first_sample[-1]) + int(self.n_samples[-1]) if len(self) else 0

    def _bytes(self, first, n):
        lo, nb = int(first) * self.bytes_per_sample, int(n) * self.bytes_per_sample
        if self.data is not None:
            return self.data[lo:lo + nb]
        if self.buf is None or not self.buf.ptr:
            raise AirError('the captures were freed')
        out = np.zeros(nb, np.uint8)
        if nb and self.buf.L.nfc_device_download(self.device, out.ctypes.data, C.c_void_p(self.buf.ptr.value + lo), nb) != 0:
            raise AirError('nfc_device_download failed')
        return out

    def download(self, k):
        """Stream k's capture as NfcContext.push takes the kind: interleaved I, Q."""
        return self._bytes(self.first_sample[k], self.n_samples[k]).view(KIND_DTYPE[self.kind])

    def download_used(self):
        """Every written byte of the buffer, padding included (uint8)."""
        return self._bytes(0, self.used_samples)

    def guard_intact(self):
        """The bytes render_device put behind the buffer's cap_samples are what they were."""
        return bool((self._bytes(self.cap_samples, GUARD_BYTES // self.bytes_per_sample) == GUARD_BYTE).all()) if self.buf is not None else True

    def push_to(self, multi):
        """multi.push_device of the K captures, stream k to stream k."""
        if self.buf is None:
            raise AirError('push_to: captures of host_render are not in device memory')
        return multi.push_device(self.buf, self.first_sample, self.n_samples)

    def context_args(self, k):
        """(device address, n) for an NfcContext.push_device of stream k; its start must be 16-byte aligned (align_samples)."""
        if self.buf is None:
            raise AirError('context_args: captures of host_render are not in device memory')
        at = self.buf.ptr.value + int(self.first_sample[k]) * self.bytes_per_sample
        if at % 16:
            raise AirError('stream %d starts %d bytes past a 16-byte boundary: render with a larger align_samples' % (k, at % 16))
        return at, int(self.n_samples[k])

    def free(self):
        if self.buf is not None:
            self.buf.free()


def _config(fr, out_kind, amp, phase, depth, sigma, seed, stream_seeds, full_scale, align_samples, _reserved=0):
    cfg = _lib.AirConfig()
    cfg.rate_msps = fr.rate_msps
    cfg.carrier_i, cfg.carrier_q = np.float32(amp * np.cos(phase)), np.float32(amp * np.sin(phase))   # as synth.iq_from_profile computes them
    cfg.depth, cfg.sigma = float(depth), float(sigma)
    cfg.full_scale = float(FULL_SCALE.get(out_kind, 1.0) if full_scale is None else full_scale)
    cfg.out_kind, cfg.seed, cfg.tail, cfg.align_samples = int(out_kind), int(seed) & (2 ** 64 - 1), fr.tail, int(align_samples)
    cfg.reserved[0] = int(_reserved)   # (must be 0: the argument only lets a test see the library refuse it)
    seeds = None
    if stream_seeds is not None:
        seeds = np.ascontiguousarray(stream_seeds, np.uint64)
        if seeds.shape != (len(fr),):
            raise ValueError('stream_seeds: one entry per stream')
        cfg.stream_seeds = seeds.ctypes.data if len(fr) else None
    return cfg, seeds


def _ptr(a):
    return a.ctypes.data if a.size else None


def _render(call, name, source, layout, out_kind, amp, phase, depth, sigma, seed, stream_seeds, full_scale, align_samples, cap_samples, room, _reserved):
    import time
    fr = frames_of(source, **layout)
    cfg, seeds = _config(fr, out_kind, amp, phase, depth, sigma, seed, stream_seeds, full_scale, align_samples, _reserved)
    K = len(fr)
    cap = fr.bound_samples(align_samples) if cap_samples is None else int(cap_samples)
    first, n = np.zeros(K, np.uint64), np.zeros(K, np.uint32)
    out = room(cap)
    t0 = time.perf_counter()
    rc = call(C.byref(cfg), _ptr(fr.frames), _ptr(fr.frame_off), _ptr(fr.air), _ptr(fr.par), _ptr(fr.byte_base), K, out, cap, _ptr(first), _ptr(n))
    dt = time.perf_counter() - t0
    if rc != 0:
        _fail(name, rc)
    return first, n, cap, dt


def sizes(source, out_kind=NFC_IN_IQ_F32, align_samples=8, **layout):
    """The sizing call (nfc_host_air_render without an output): -> (first_sample, n_samples) of a rendering."""
    first, n, _, _ = _render(_lib.load().nfc_host_air_render, 'nfc_host_air_render', source, layout, out_kind, 0.5, 0.3, 0.08, 0.0, 0, None, None,
                             align_samples, 0, lambda cap: None, 0)
    return first, n


def host_render(source, out_kind=NFC_IN_IQ_F32, amp=0.5, phase=0.3, depth=0.08, sigma=0.002, seed=synth.SEED, stream_seeds=None, full_scale=None,
                align_samples=8, cap_samples=None, _reserved=0, **layout):
    """Render on one CPU core (nfc_host_air_render), the twin of render_device: the same bytes.  layout: frames_of's keywords."""
    bps = 2 * np.dtype(KIND_DTYPE.get(out_kind, np.float32)).itemsize   # (a kind that is none of the four: the library refuses it)
    held = []

    def room(cap):
        held.append(np.zeros(max(cap, 1) * bps, np.uint8))
        return held[0].ctypes.data

    first, n, cap, dt = _render(_lib.load().nfc_host_air_render, 'nfc_host_air_render', source, layout, out_kind, amp, phase, depth, sigma, seed,
                                stream_seeds, full_scale, align_samples, cap_samples, room, _reserved)
    out = AirCaptures(out_kind, first, n, cap, data=held[0])
    out.call_s = dt
    return out


def render_device(source, out_kind=NFC_IN_IQ_F32, amp=0.5, phase=0.3, depth=0.08, sigma=0.002, seed=synth.SEED, stream_seeds=None, full_scale=None,
                  align_samples=8, cap_samples=None, device=0, timing=False, _reserved=0, **layout):
    """Render on the GPU into one device buffer (nfc_air_render_device), a workgroup per frame.  timing: -> .kernel_ms = (layout, render).
    Raises without a GPU: there is no CPU fallback."""
    from . import api
    L = _lib.load()
    if L.nfc_device_count() <= 0:
        raise AirError('render_device: no HIP device, and the GPU rendering has no CPU fallback (host_render is the twin)')
    bps = 2 * np.dtype(KIND_DTYPE.get(out_kind, np.float32)).itemsize   # (a kind that is none of the four: the library refuses it)
    held, ms = [], (C.c_float * 2)()

    def room(cap):
        buf = api.DeviceBuffer(np.zeros(0, np.uint8), device, nbytes=max(cap, 1) * bps + GUARD_BYTES)
        held.append(buf)
        if L.nfc_device_fill(device, C.c_void_p(buf.ptr.value + cap * bps), GUARD_BYTE, GUARD_BYTES) != 0:
            raise AirError('nfc_device_fill failed')
        return buf.ptr

    try:
        first, n, cap, dt = _render(lambda *a: L.nfc_air_render_device(int(device), *a, C.byref(ms) if timing else None), 'nfc_air_render_device', source,
                                    layout, out_kind, amp, phase, depth, sigma, seed, stream_seeds, full_scale, align_samples, cap_samples, room, _reserved)
    except Exception:
        for b in held:
            b.free()
        raise
    out = AirCaptures(out_kind, first, n, cap, buf=held[0], kernel_ms=(float(ms[0]), float(ms[1])) if timing else None, device=device)
    out.call_s = dt
    return out
