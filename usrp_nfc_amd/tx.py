"""Transmit side over the C-ABI: encode_bits of the reference's three encoders
(miller.py:200-233, manchester.py:64-79, binary_src.py:17-20) and the device-side renderer that stands where
binary_src.work (binary_src.py:64-103) and multiplier (multiplier.py:18-22) stand in the reference's TX chain."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NFC_TX_MANCHESTER, NFC_TX_MILLER, NFC_TX_SAME, TX_RUN_DTYPE   # noqa: F401


def _check(rc, what):
    if rc != 0:
        msg = _lib.load().nfc_last_error(None)
        raise RuntimeError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else ''))


def encode_runs(encoding, bits):
    """-> structured array of nfc_tx_run (level, dur_us)."""
    L = _lib.load()
    b = np.ascontiguousarray(np.asarray(bits, dtype=np.uint8))
    cap = 3 * b.size + 8
    out = np.zeros(cap, TX_RUN_DTYPE)
    n = C.c_size_t(0)
    _check(L.nfc_tx_encode(int(encoding), b.ctypes.data, b.size, out.ctypes.data, cap, C.byref(n)), 'nfc_tx_encode')
    return out[:n.value]


def encode_bits(encoding, bits):
    """The reference's return type: a list of (level, microseconds) tuples."""
    r = encode_runs(encoding, bits)
    return [(int(l), float(d)) for l, d in zip(r['level'], r['dur_us'])]


def as_runs(pulses):
    """(level, us) tuples -> nfc_tx_run array."""
    r = np.zeros(len(pulses), TX_RUN_DTYPE)
    if len(pulses):
        r['level'] = [p[0] for p in pulses]
        r['dur_us'] = [p[1] for p in pulses]
    return r


def sample_count(runs, samp_rate):
    L = _lib.load()
    runs = np.ascontiguousarray(runs)
    n = C.c_uint64(0)
    _check(L.nfc_tx_sample_count(runs.ctypes.data, runs.size, float(samp_rate), C.byref(n)), 'nfc_tx_sample_count')
    return int(n.value)


def render_device(runs, samp_rate, dev_ptr, cap_samples, carrier=False, freq=13.56e6, amp=1.0, first_index=0, device=0,
                  timed=False):
    """Render into device memory (complex64).  -> (n_samples, kernel_ms or None)."""
    L = _lib.load()
    runs = np.ascontiguousarray(runs)
    n = C.c_size_t(0)
    ms = C.c_float(0)
    _check(L.nfc_tx_render_device(int(device), runs.ctypes.data, runs.size, float(samp_rate), 1 if carrier else 0, float(freq),
                                  float(amp), int(first_index), dev_ptr, int(cap_samples), C.byref(n),
                                  C.byref(ms) if timed else None), 'nfc_tx_render_device')
    return int(n.value), (float(ms.value) if timed else None)


def answers_tx_config(samp_rate=2e6, in_rate=None, delay_us=0.0, carrier=False, freq=13.56e6, amp=1.0, first_index=0, align_samples=8,
                      _reserved=0):
    """The nfc_answers_tx_config of NfcMultiContext.transmit / emulate.host_transmit: the ratio of the two rates from
    fractions.Fraction (in_rate None: the same rate, 1/1), delay_samples = int(delay_us * samp_rate / 1e6)."""
    from fractions import Fraction
    ratio = Fraction(1) if in_rate is None else Fraction(samp_rate) / Fraction(in_rate)
    if ratio.numerator >= 1 << 32 or ratio.denominator >= 1 << 32:
        raise ValueError('samp_rate / in_rate: neither term of the reduced ratio fits 32 bits')
    c = _lib.AnswersTxConfig(float(samp_rate), float(freq), int(first_index), int(delay_us * samp_rate / 1e6), ratio.numerator, ratio.denominator,
                             1 if carrier else 0, float(amp), int(align_samples))
    c.reserved[0] = int(_reserved)   # (must be 0: the argument only lets a test see the library refuse it)
    return c


class TxCaptures(object):
    """K TX captures in one device buffer (NfcMultiContext.transmit): stream k's complex64 samples are the n_samples[k] entries from
    first_sample[k] on.  `buf` is the device buffer, owned (and freed by free()) unless the caller gave it; kernel_ms: with timed=True the
    schedule and the render pass, by HIP events.  The rendering is only ENQUEUED on the context's stream: wait() completes it (download
    and record do so themselves); work of another stream or context that reads the buffer comes after a wait()."""

    def __init__(self, first_sample, n_samples, buf, owned, samp_rate, device=0, kernel_ms=None, multi=None):
        self.first_sample, self.n_samples, self.buf, self.owned = first_sample, n_samples, buf, owned
        self.samp_rate, self.device, self.kernel_ms, self._multi = float(samp_rate), int(device), kernel_ms, multi

    def wait(self):
        """Complete the rendering (nfc_multi_get_tx_state completes the context's stream before it reads)."""
        if self._multi is not None and getattr(self._multi, 'h', None):
            self._multi.tx_state(0)
        return self

    def __len__(self):
        return len(self.n_samples)

    @property
    def total(self):
        """samples of the layout: first_sample[K-1] + n_samples[K-1]"""
        return int(self.first_sample[-1]) + int(self.n_samples[-1]) if len(self.n_samples) else 0

    def ptr(self, k=None):
        """The device address of the buffer (k None) or of stream k's first sample."""
        from . import api
        base = api._as_pointer(self.buf).value or 0
        return C.c_void_p(base + (0 if k is None else 8 * int(self.first_sample[k])))

    def download(self, k=None):
        """Stream k's samples (k None: the whole layout, padding included) as a complex64 array."""
        first, n = (0, self.total) if k is None else (int(self.first_sample[k]), int(self.n_samples[k]))
        out = np.zeros(n, np.complex64)
        self.wait()
        if n and _lib.load().nfc_device_download(self.device, out.ctypes.data, C.c_void_p((self.ptr().value or 0) + 8 * first), 8 * n) != 0:
            raise RuntimeError('nfc_device_download failed')
        return out

    def record(self, k, path, gain=32767.0):
        """Stream k's real part as a 16-bit WAV, converted on the GPU (record.record(path).write_device).  Needs first_sample[k] on 16
        bytes: an even align_samples."""
        from . import record
        self.wait()
        with record.record(path, self.samp_rate, gain, self.device) as w:
            return w.write_device(self.ptr(k), int(self.n_samples[k]))

    def free(self):
        if self.owned and self.buf is not None:
            self.buf.free()
        self.buf = None


def render(runs, samp_rate, carrier=False, freq=13.56e6, amp=1.0, first_index=0, device=0):
    """Render on the GPU and bring the samples back: complex64 array."""
    from . import api
    n = sample_count(runs, samp_rate)
    buf = api.DeviceBuffer(np.zeros(0, np.float32), device, nbytes=max(8 * n, 32))
    try:
        got, _ = render_device(runs, samp_rate, buf.ptr, n, carrier, freq, amp, first_index, device)
        return buf.download(8 * got).view(np.complex64)
    finally:
        buf.free()
