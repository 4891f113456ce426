"""Drop-in for the reference's record module (record.py:10-19): the real part of a complex stream into a 16-bit mono WAV of
rate ``int(samp_rate)`` -- what the emulators keep of what they transmit (usrp_nfc.py:59-60,95-96).

* With GNU Radio importable ``record(dst, samp_rate)`` is the reference's ``gr.hier_block2``, ``complex_to_real -> wavfile_sink``.
* Without it (this image) ``record(dst, samp_rate, gain, device)`` is a writer: ``write(x)`` converts complex64 samples on the GPU
  (``nfc_record_pcm16_device`` with the real-part tap: v = fl(re * gain), NaN -> 0, clamp to +-32767, round to nearest with halves
  away from zero -- include/nfc_amd.h) and appends them; ``write_device(dev_ptr, n)`` does the same for samples already in device
  memory, e.g. ``record('tx.wav').write_device(buf.ptr, n)`` after ``tx.render_device`` keeps what k_tx_render left in HBM without
  a host copy of the complex64; ``write_pcm(int16 array)`` appends PCM that is already converted (decoder's ``dst`` uses it for
  the envelope tap).  ``close()`` finishes the header; the object is a context manager.
"""
import wave

import numpy

from . import api

try:  # (GNU Radio is not in the build image: this branch cannot be tested there)
    from gnuradio import blocks as _blocks
    from gnuradio import gr as _gr
except Exception:
    _gr = None
    _blocks = None

RIFF_LIMIT = (1 << 32) - 1 - 36   # data bytes a RIFF/WAVE file can hold: its 32-bit size field counts them and 36 bytes of header


if _gr is not None:

    class record(_gr.hier_block2):
        def __init__(self, dst, samp_rate=2e6):
            _gr.hier_block2.__init__(self, "record", _gr.io_signature(1, 1, _gr.sizeof_gr_complex), _gr.io_signature(0, 0, 0))
            self._re = _blocks.complex_to_real(1)
            self._sink = _blocks.wavfile_sink(dst, 1, int(samp_rate))
            self.connect(self, self._re, self._sink)

else:

    class record(object):
        def __init__(self, dst, samp_rate=2e6, gain=32767.0, device=0):
            self._gain = float(gain)
            self._device = int(device)
            self._bytes = 0
            self._w = wave.open(dst, 'wb')
            self._w.setnchannels(1)
            self._w.setsampwidth(2)
            self._w.setframerate(int(samp_rate))   # record.py:17

        def write_pcm(self, pcm):
            """Append int16 PCM that is already converted."""
            if self._w is None:
                raise ValueError('record: the file is closed')
            a = numpy.ascontiguousarray(pcm, dtype='<i2').reshape(-1)
            if self._bytes + a.nbytes > RIFF_LIMIT:   # (checked before the piece that would cross the limit is written)
                raise ValueError('record: %d more bytes after %d would pass the 4 GiB limit of a RIFF/WAVE file; start another file'
                                 % (a.nbytes, self._bytes))
            self._w.writeframesraw(a.tobytes())
            self._bytes += a.nbytes
            return len(a)

        def write_device(self, dev_ptr, n):
            """n complex64 samples resident in device memory (16-byte aligned): converted there, only the PCM comes to the host."""
            n = int(n)
            if n == 0:
                return 0
            out = api.DeviceBuffer(numpy.zeros(0, numpy.int16), self._device, nbytes=2 * n)
            try:
                api.record_pcm16_device(dev_ptr, n, out, api.NFC_IN_IQ_F32, gain=self._gain, tap=api.NFC_REC_REAL_PART, device=self._device)
                return self.write_pcm(out.download(2 * n).view(numpy.int16))
            finally:
                out.free()

        def write(self, x):
            """complex64 samples (or interleaved float32 I,Q) from the host."""
            a = numpy.asarray(x)
            a = a.astype(numpy.complex64, copy=False).view(numpy.float32) if numpy.iscomplexobj(a) else a
            a = numpy.ascontiguousarray(a, dtype=numpy.float32).reshape(-1)
            n = a.size // 2
            if n == 0:
                return 0
            buf = api.DeviceBuffer(a[:2 * n], self._device)
            try:
                return self.write_device(buf, n)
            finally:
                buf.free()

        def close(self):
            if getattr(self, '_w', None) is not None:
                self._w.close()
                self._w = None

        def __enter__(self):
            return self

        def __exit__(self, *a):
            self.close()

        __del__ = close
