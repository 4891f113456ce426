"""Python face of the C-ABI: one NfcContext = one stream, one NfcMultiContext = many streams decoded in one launch
(include/nfc_amd.h)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (COUNTS_DTYPE, EDGE_DTYPE, NFC_MF_ARRAYS, NFC_MF_BITS0, NFC_MF_BITS1, NFC_MF_EDGES, NFC_MF_PK0, NFC_MF_PK1, NFC_MF_SYM0,
                   NFC_MF_SYM1, NFC_MULTI_FETCH_ALL, NFC_MULTI_FETCH_EDGES, NFC_MULTI_FETCH_PACKETS, NFC_MULTI_FETCH_SYMBOLS,
                   NFC_FLAG_FORCE_SEQUENTIAL, NFC_FLAG_NO_EDGES, NFC_IN_ENV_F32, NFC_IN_I16_SQ,
                   NFC_IN_IQ_F32, NFC_IN_IQ_I8, NFC_IN_IQ_I16, NFC_IN_IQ_U8, NFC_IN_REAL_F32_SQ, NFC_MULTI_PENDING_OVERFLOW,
                   NFC_MULTI_TRUNC_BITS, NFC_MULTI_TRUNC_EDGES, NFC_MULTI_TRUNC_PACKETS, NFC_MULTI_TRUNC_SYMBOLS, NFC_REC_ENVELOPE,
                   NFC_RAW_CRC_A_OK, NFC_RAW_CUT, NFC_RAW_PARITY_OK, NFC_REC_REAL_PART, PACKET_DTYPE, RAW_FRAME_DTYPE, NFC_FSM_LOST,
                   NFC_FSM_UID_OVERFLOW, NFC_CMD_CUT)

__all__ = ['NfcContext', 'NfcError', 'DeviceBuffer', 'host_decode_lut', 'host_envelope', 'NFC_IN_IQ_F32', 'NFC_IN_ENV_F32',
           'NFC_IN_REAL_F32_SQ', 'NFC_IN_I16_SQ', 'NFC_IN_IQ_I16', 'NFC_IN_IQ_I8', 'NFC_IN_IQ_U8', 'NFC_FLAG_FORCE_SEQUENTIAL',
           'NFC_FLAG_NO_EDGES', 'NFC_REC_ENVELOPE', 'NFC_REC_REAL_PART', 'host_record_pcm16', 'record_pcm16_device', 'record_pcm16',
           'NfcMultiContext', 'NfcMultiStream', 'NFC_MULTI_TRUNC_EDGES', 'NFC_MULTI_TRUNC_SYMBOLS', 'NFC_MULTI_TRUNC_PACKETS',
           'NFC_MULTI_TRUNC_BITS', 'NFC_MULTI_PENDING_OVERFLOW', 'NfcMultiFetch', 'NFC_MULTI_FETCH_EDGES', 'NFC_MULTI_FETCH_SYMBOLS',
           'NFC_MULTI_FETCH_PACKETS', 'NFC_MULTI_FETCH_ALL', 'NFC_MF_EDGES', 'NFC_MF_SYM0', 'NFC_MF_SYM1', 'NFC_MF_PK0', 'NFC_MF_PK1',
           'NFC_MF_BITS0', 'NFC_MF_BITS1', 'NFC_MF_ARRAYS', 'COUNTS_DTYPE', 'COUNTS_FLAGS_DTYPE', 'NfcFrames', 'NfcMultiFrames', 'host_frames',
           'RAW_FRAME_DTYPE', 'NFC_RAW_PARITY_OK', 'NFC_RAW_CRC_A_OK', 'NFC_RAW_CUT', 'NfcMultiCommands', 'NFC_FSM_LOST', 'NFC_FSM_UID_OVERFLOW',
           'NFC_CMD_CUT', 'NfcMultiImages']

_KIND_DTYPE = {NFC_IN_IQ_F32: (np.float32, 2), NFC_IN_ENV_F32: (np.float32, 1),
               NFC_IN_REAL_F32_SQ: (np.float32, 1), NFC_IN_I16_SQ: (np.int16, 1), NFC_IN_IQ_I16: (np.int16, 2),
               NFC_IN_IQ_I8: (np.int8, 2), NFC_IN_IQ_U8: (np.uint8, 2)}


class NfcError(RuntimeError):
    pass


def _params(samp_rate, lo_val, hi_val, av_window, max_len, reader, tag, input_kind, device, i16_scale, flags,
            chunk_samples):
    return _lib.Params(float(samp_rate), float(lo_val), float(hi_val), int(av_window), int(max_len), int(bool(reader)),
                       int(bool(tag)), int(input_kind), int(device), float(i16_scale), int(flags), int(chunk_samples), 0)


class NfcContext(object):
    """Arguments mirror transition_sink.transition_sink (transition_sink.py:12) and
    background.background (background.py:17) of the reference."""

    def __init__(self, samp_rate=2e6, lo_val=0.1, hi_val=1.1, av_window=2000, max_len=50, reader=True, tag=True,
                 input_kind=NFC_IN_IQ_F32, device=0, i16_scale=0.0, flags=0, chunk_samples=0, lib_path=None):
        """lib_path: another build of libnfc_amd.so for this context (tests: the build with the test hooks, _lib.hooks_path())."""
        self.L = _lib.load(lib_path)
        self.h = C.c_void_p()
        self.input_kind = input_kind
        self.factor = 1e6 / samp_rate
        self.av_window = int(av_window)
        p = _params(samp_rate, lo_val, hi_val, av_window, max_len, reader, tag, input_kind, device, i16_scale, flags,
                    chunk_samples)
        rc = self.L.nfc_create(C.byref(p), C.byref(self.h))
        if rc != 0:
            raise NfcError('nfc_create: %s (status %d)' % (self.L.nfc_last_error(None).decode(), rc))

    def close(self):
        if getattr(self, 'h', None):
            self.L.nfc_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise NfcError('%s: %s (status %d)' % (what, self.L.nfc_last_error(self.h).decode(), rc))

    # -- input ---------------------------------------------------------------
    def push(self, samples):
        """Host array: float32 IQ interleaved / complex64, float32 envelope or real, int16 PCM, or complex int16 / int8 / uint8
        (sc16, sc8, cu8: I,Q interleaved -- 2n values -- or an (n, 2) array)."""
        dt, per = _KIND_DTYPE[self.input_kind]
        a = np.asarray(samples)
        if a.dtype == np.complex64 and per == 2:
            a = a.view(np.float32)
        a = np.ascontiguousarray(a, dtype=dt)
        n = a.size // per
        self._chk(self.L.nfc_push(self.h, a.ctypes.data, n), 'nfc_push')
        return n

    def push_device(self, dev_ptr, n):
        """Device pointer (int), n samples, 16-byte aligned."""
        ptr = dev_ptr.ptr if isinstance(dev_ptr, DeviceBuffer) else C.c_void_p(int(dev_ptr))
        self._chk(self.L.nfc_push_device(self.h, ptr, n), 'nfc_push_device')
        return n

    def submit_device(self, dev_ptr, n):
        """Enqueue a batch and return (nfc_submit_device); at most three in flight.  The buffer stays untouched until its wait()."""
        ptr = dev_ptr.ptr if isinstance(dev_ptr, DeviceBuffer) else C.c_void_p(int(dev_ptr))
        self._chk(self.L.nfc_submit_device(self.h, ptr, n), 'nfc_submit_device')
        return n

    def wait(self):
        """Complete the oldest submitted batch (nfc_wait): its outputs are then read like those of a push."""
        self._chk(self.L.nfc_wait(self.h), 'nfc_wait')

    def submitted(self):
        return int(self.L.nfc_submitted(self.h))

    # -- outputs of the last push -----------------------------------------------
    def push_edges(self, edges):
        """Transitions (EDGE_DTYPE rows: idx, d in samples, v, t) through the decode and framing stages alone (nfc_push_edges) --
        what background.append receives in the reference."""
        e = np.ascontiguousarray(edges, EDGE_DTYPE)
        self._chk(self.L.nfc_push_edges(self.h, e.ctypes.data if len(e) else None, len(e)), 'nfc_push_edges')

    def counts(self):
        c = _lib.Counts()
        self._chk(self.L.nfc_get_counts(self.h, C.byref(c)), 'nfc_get_counts')
        return c

    def stats(self):
        s = _lib.Stats()
        self._chk(self.L.nfc_get_stats(self.h, C.byref(s)), 'nfc_get_stats')
        return s

    def window_converged(self):
        """After a warm-up (prime + overlap): has every window slot taken an accepted sample since the prime?  (nfc_stats'
        ring_slots_carried of the last batch: slots whose value is still the one the batch started from.)"""
        st = self.stats()   # (a batch that needed the sequential prefix is not vouched for: its parallel rest counts from the prefix's end)
        return int(st.ring_slots_carried) == 0 and not int(st.used_sequential)

    def set_timing(self, level):
        """0: no HIP events (default), 1: threshold kernel durations (events attached to the launches), 2: + batch total and per-stage split (stream markers, a few us each)."""
        self._chk(self.L.nfc_set_timing(self.h, int(level)), 'nfc_set_timing')

    def _read(self, fn, total, dtype, *lead):
        out = np.zeros(int(total), dtype)
        got = C.c_size_t(0)
        if total:
            self._chk(fn(self.h, *lead, out.ctypes.data, out.size, C.byref(got)), fn.__name__)
            if got.value != out.size:
                raise NfcError('%s returned %d of %d items' % (fn.__name__, got.value, out.size))
        return out

    def edges(self):
        return self._read(self.L.nfc_read_edges, self.counts().n_edges, EDGE_DTYPE, 0)

    def edges_compact(self, out=None):
        """(pos, code) of the batch's transitions as the device keeps them (nfc_read_edges_compact): batch-local sample
        position, and ((v + 1) * (max_len + 1) + d) | (t + 1) << 14."""
        n = int(self.counts().n_edges)
        if out is not None:   # caller's arrays (pinned ones -- pinned_array -- are written by the copy engine in place)
            if len(out[0]) < n or len(out[1]) < n:
                raise NfcError('edges_compact: the output arrays hold %d entries, the batch has %d' % (min(len(out[0]), len(out[1])), n))
            pos, code = out[0][:n], out[1][:n]
        else:
            pos, code = np.zeros(n, np.uint32), np.zeros(n, np.uint16)
        got = C.c_size_t(0)
        if n:
            self._chk(self.L.nfc_read_edges_compact(self.h, 0, pos.ctypes.data, code.ctypes.data, n, C.byref(got)), 'nfc_read_edges_compact')
            if got.value != n:
                raise NfcError('nfc_read_edges_compact returned %d of %d items' % (got.value, n))
        return pos, code

    def transitions(self):
        """The list transition_sink hands to its callback: [((v, d*factor), t), ...]."""
        e = self.edges()
        f = self.factor
        return [((int(v), int(d) * f), int(t)) for v, d, t in zip(e['v'], e['d'], e['t'])]

    def symbols(self, ptype):
        return self._read(self.L.nfc_read_symbols, self.counts().n_symbols[ptype], np.uint8, ptype, 0)

    def packet_table(self, ptype):
        n = self.counts().n_packets[ptype]
        out = np.zeros(int(n), PACKET_DTYPE)
        got = C.c_size_t(0)
        if n:
            self._chk(self.L.nfc_read_packets(self.h, ptype, out.ctypes.data, out.size, C.byref(got)), 'nfc_read_packets')
        return out

    def packet_bits(self, ptype):
        """The per-type bit array the packet table's bit_off / n_bits index (nfc_read_packet_bits)."""
        tab = self.packet_table(ptype)
        if not len(tab):
            return np.zeros(0, np.uint8)
        bits = np.zeros(int((tab['bit_off'] + tab['n_bits']).max()), np.uint8)
        got = C.c_size_t(0)
        if bits.size:
            self._chk(self.L.nfc_read_packet_bits(self.h, ptype, 0, bits.ctypes.data, bits.size, C.byref(got)), 'nfc_read_packet_bits')
        return bits

    def packets(self):
        """Closed packets of both types in stream order: [(type, [bits]), ...] -- what
        CombinedPacketProcessor hands to fsm.process_bits (packets.py:96-98)."""
        items = []
        for t in (0, 1):
            tab = self.packet_table(t)
            if not len(tab):
                continue
            hi = int((tab['bit_off'] + tab['n_bits']).max())
            bits = np.zeros(hi, np.uint8)
            got = C.c_size_t(0)
            self._chk(self.L.nfc_read_packet_bits(self.h, t, 0, bits.ctypes.data, bits.size, C.byref(got)),
                      'nfc_read_packet_bits')
            for p in tab:
                o = int(p['bit_off'])
                items.append((int(p['idx']), t, bits[o:o + int(p['n_bits'])].tolist()))
        # one edge feeds one decoder, so closing indices of the two types never tie
        items.sort(key=lambda r: r[0])
        return [(t, b) for _, t, b in items]

    def frame_counts(self):
        """(n_frames[2], n_bytes[2]) of the last batch (nfc_get_frame_counts); the first frame call after a batch assembles them."""
        nf, nb = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
        self._chk(self.L.nfc_get_frame_counts(self.h, nf.ctypes.data, nb.ctypes.data), 'nfc_get_frame_counts')
        return nf, nb

    def frames(self):
        """The last batch's closed packets as frames assembled on the GPU -- repaired, nine bits to a byte, parity verdict, CRC_A
        (nfc_read_frames / nfc_read_frame_bytes) -> NfcFrames.  fsm.process_frames takes it."""
        nf, nb = self.frame_counts()
        recs, data, par = [], [], []
        got = C.c_size_t(0)
        for t in (0, 1):
            r, b, p = np.zeros(int(nf[t]), RAW_FRAME_DTYPE), np.zeros(int(nb[t]), np.uint8), np.zeros(int(nb[t]), np.uint8)
            if r.size:
                self._chk(self.L.nfc_read_frames(self.h, t, r.ctypes.data, r.size, C.byref(got)), 'nfc_read_frames')
            if b.size:
                self._chk(self.L.nfc_read_frame_bytes(self.h, t, 0, b.ctypes.data, p.ctypes.data, b.size, C.byref(got)), 'nfc_read_frame_bytes')
            recs.append(r), data.append(b), par.append(p)
        return NfcFrames(recs, data, par)

    def track_commands(self, on=True):
        """While on, every batch that completes also assembles its frames and runs the protocol machine over them on the GPU, CRYPTO1
        included, a lane per transaction (nfc_track_commands, csrc/ctx_commands.hip.h): six launches behind the batch's own, no host
        wait.  The machine's state stays on the device from batch to batch; commands() brings the last batch's commands to the host."""
        self._chk(self.L.nfc_track_commands(self.h, int(bool(on))), 'nfc_track_commands')

    def set_keys(self, key_a=(0xFF,) * 6, key_b=(0xFF,) * 6):
        """MIFARE Classic keys A / B of the context's machine, six bytes each, as fsm.set_keys (nfc_set_fsm_keys)."""
        a, b = np.ascontiguousarray(key_a, np.uint8), np.ascontiguousarray(key_b, np.uint8)
        if a.size != 6 or b.size != 6:
            raise NfcError('set_keys: key_a and key_b are six bytes each')
        self._chk(self.L.nfc_set_fsm_keys(self.h, a.ctypes.data, b.ctypes.data), 'nfc_set_fsm_keys')

    def set_sector_keys(self, table):
        """The per-sector key table of the context's machine, as fsm.set_sector_keys: a dict (key_type, sector) -> six key bytes or an
        _lib.FsmKeyTable; None or {} empties it (nfc_set_fsm_sector_keys).  The first call allocates the table's device buffer."""
        from . import keys
        try:
            t = keys.key_table(table)
        except ValueError as e:
            raise NfcError('set_sector_keys: %s' % e)
        self._chk(self.L.nfc_set_fsm_sector_keys(self.h, C.byref(t)), 'nfc_set_fsm_sector_keys')

    def sector_keys(self):
        """The machine's key table as the dict (key_type, sector) -> six key bytes of its present slots (nfc_get_fsm_sector_keys)."""
        from . import keys
        t = _lib.FsmKeyTable()
        self._chk(self.L.nfc_get_fsm_sector_keys(self.h, C.byref(t)), 'nfc_get_fsm_sector_keys')
        return keys.table_dict(t)

    def fsm_state(self):
        """The context's protocol machine as a plain nfc_fsm_state (an _lib.FsmState): what fsm.set_state takes."""
        st = _lib.FsmState()
        self._chk(self.L.nfc_get_fsm_state(self.h, C.byref(st)), 'nfc_get_fsm_state')
        return st

    def set_fsm_state(self, st):
        """The context's machine continues from `st` (fsm.get_state(), another context's fsm_state())."""
        self._chk(self.L.nfc_set_fsm_state(self.h, C.byref(st)), 'nfc_set_fsm_state')

    def commands(self, copy=True):
        """The commands of the last batch, tracked on the GPU (track_commands), in ONE copy (nfc_read_commands) -> NfcCommands.
        copy=False: views of the context's pinned memory, valid until the next batch completes, commands(), reset, set_fsm_state or
        close of this context."""
        c = _lib.CtxCommands()
        self._chk(self.L.nfc_read_commands(self.h, C.byref(c)), 'nfc_read_commands')
        return NfcCommands(c, copy)

    def val(self):
        return self._read(self.L.nfc_read_val, self.counts().n_samples, np.int8, 0)

    def reset(self):
        """Start a new stream (state of a fresh context), keeping the device buffers."""
        self._chk(self.L.nfc_reset(self.h), 'nfc_reset')

    def get_state(self):
        """(header, ring float32[av_window], [pending bits type 0, pending bits type 1])."""
        h = _lib.StateHeader()
        self._chk(self.L.nfc_get_state(self.h, C.byref(h), None, 0, None, 0), 'nfc_get_state')
        ring = np.zeros(h.av_window, np.float32)
        p0, p1 = int(h.n_pending_bits[0]), int(h.n_pending_bits[1])
        pend = np.zeros(p0 + p1, np.uint8)
        self._chk(self.L.nfc_get_state(self.h, C.byref(h), ring.ctypes.data, ring.size, pend.ctypes.data, pend.size),
                  'nfc_get_state')
        return h, ring, [pend[:p0].copy(), pend[p0:].copy()]

    def set_state(self, header, ring, pending=None):
        ring = np.ascontiguousarray(ring, np.float32)
        pend = np.zeros(0, np.uint8) if pending is None else np.ascontiguousarray(np.concatenate(pending), np.uint8)
        self._chk(self.L.nfc_set_state(self.h, C.byref(header), ring.ctypes.data, ring.size, pend.ctypes.data, pend.size),
                  'nfc_set_state')

    def state_blob(self):
        """Boundary state as one uint8 vector: header | ring | pending bits (for RCCL exchange)."""
        h, ring, pend = self.get_state()
        return np.concatenate([np.frombuffer(bytes(h), np.uint8), ring.view(np.uint8), pend[0], pend[1]])

    def export_state(self, dev_ptr, cap):
        """Boundary state into device memory (16-byte aligned), asynchronously: [u32 len | 12 B | state_blob() bytes]."""
        got = C.c_size_t(0)
        self._chk(self.L.nfc_export_state(self.h, C.c_void_p(int(dev_ptr)), int(cap), C.byref(got)), 'nfc_export_state')
        return got.value

    def sync(self):
        self._chk(self.L.nfc_sync(self.h), 'nfc_sync')

    def set_stream(self, stream):
        """Run on the caller's HIP stream (an integer hipStream_t, e.g. torch.cuda.current_stream().cuda_stream; 0 / None:
        the context's own again)."""
        h = int(stream or 0)
        if h == getattr(self, '_stream', 0):
            return   # (the switch waits for the stream it leaves: not something to repeat per batch)
        self._chk(self.L.nfc_set_stream(self.h, C.c_void_p(h)), 'nfc_set_stream')
        self._stream = h

    def set_state_blob(self, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        hs = C.sizeof(_lib.StateHeader)
        h = _lib.StateHeader.from_buffer_copy(blob[:hs].tobytes())
        rb = 4 * h.av_window
        ring = blob[hs:hs + rb].view(np.float32)
        p0, p1 = int(h.n_pending_bits[0]), int(h.n_pending_bits[1])
        pend = blob[hs + rb:hs + rb + p0 + p1]
        self.set_state(h, ring, [pend[:p0], pend[p0:]])

    def prime(self, start_index, level):
        """Speculative start for a time chunk that does not begin the stream: every ring slot at the
        estimated carrier level, idle state machine, decoders reset.  Pushing an overlap region that ends
        where the chunk starts then converges to the true boundary state (multi-GPU)."""
        self._chk(self.L.nfc_prime(self.h, int(start_index), float(np.float32(level))), 'nfc_prime')


_MULTI_FLAG_NAMES = ((NFC_MULTI_TRUNC_EDGES, 'NFC_MULTI_TRUNC_EDGES'), (NFC_MULTI_TRUNC_SYMBOLS, 'NFC_MULTI_TRUNC_SYMBOLS'),
                     (NFC_MULTI_TRUNC_PACKETS, 'NFC_MULTI_TRUNC_PACKETS'), (NFC_MULTI_TRUNC_BITS, 'NFC_MULTI_TRUNC_BITS'),
                     (NFC_MULTI_PENDING_OVERFLOW, 'NFC_MULTI_PENDING_OVERFLOW'))


COUNTS_FLAGS_DTYPE = np.dtype(COUNTS_DTYPE.descr + [('flags', '<u4')])   # NfcMultiContext.counts_all


def _flag_names(bits):
    return ' | '.join(nm for v, nm in _MULTI_FLAG_NAMES if bits & v)


def _trunc_mask(bit):
    """The flags that make an array of kind `bit` unreliable: its own, and for packets and their bits an overflowed open packet."""
    return bit | NFC_MULTI_PENDING_OVERFLOW if bit in (NFC_MULTI_TRUNC_PACKETS, NFC_MULTI_TRUNC_BITS) else bit


class NfcMultiContext(object):
    """n_streams independent streams with one parameter set, decoded in one kernel launch per push -- a GPU lane per stream
    (nfc_multi, include/nfc_amd.h).  The keywords are NfcContext's; cap_*: entries stored per stream and push (0: the defaults
    from max_push_samples).  Stream k's outputs and state are what an NfcContext with the same arguments gives for the same
    samples; ``stream(k)`` is the view that reads them."""

    def __init__(self, n_streams, max_push_samples, samp_rate=2e6, lo_val=0.1, hi_val=1.1, av_window=2000, max_len=50, reader=True,
                 tag=True, input_kind=NFC_IN_IQ_F32, device=0, i16_scale=0.0, flags=0, chunk_samples=0, cap_edges=0, cap_symbols=0,
                 cap_packets=0, cap_packet_bits=0, cap_pending_bits=0, lib_path=None, _reserved=0):
        self.L = _lib.load(lib_path)
        self.h = C.c_void_p()
        self.input_kind = input_kind
        self.factor = 1e6 / samp_rate
        self.av_window = int(av_window)
        self.device = int(device)
        p = _params(samp_rate, lo_val, hi_val, av_window, max_len, reader, tag, input_kind, device, i16_scale, flags, chunk_samples)
        c = _lib.MultiConfig(int(n_streams), int(max_push_samples), int(cap_edges), int(cap_symbols), int(cap_packets),
                             int(cap_packet_bits), int(cap_pending_bits))
        c.reserved[0] = int(_reserved)   # (must be 0: the argument only lets a test see the library refuse it)
        rc = self.L.nfc_multi_create(C.byref(p), C.byref(c), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise NfcError('nfc_multi_create: %s (status %d)' % (self.L.nfc_multi_last_error(None).decode(), rc))
        self.n_streams = int(n_streams)
        self.max_push_samples = int(max_push_samples)

    def close(self):
        if getattr(self, 'h', None):
            self.L.nfc_multi_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __len__(self):
        return self.n_streams

    def _chk(self, rc, what):
        if rc != 0:
            raise NfcError('%s: %s (status %d)' % (what, self.L.nfc_multi_last_error(self.h).decode(), rc))

    def push(self, arrays):
        """One host array per stream, in the layouts NfcContext.push takes for the kind; an empty array (or None) gives the stream
        nothing.  -> the samples consumed per stream."""
        if len(arrays) != self.n_streams:
            raise NfcError('push: %d arrays for %d streams' % (len(arrays), self.n_streams))
        dt, per = _KIND_DTYPE[self.input_kind]
        keep, ptrs, n = [], (C.c_void_p * self.n_streams)(), np.zeros(self.n_streams, np.uint32)
        for k, a in enumerate(arrays):
            a = np.zeros(0, dt) if a is None else np.asarray(a)
            if a.dtype == np.complex64 and per == 2:
                a = a.view(np.float32)
            a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
            keep.append(a)
            n[k] = a.size // per
            ptrs[k] = a.ctypes.data if n[k] else None
        self._chk(self.L.nfc_multi_push(self.h, ptrs, n.ctypes.data), 'nfc_multi_push')
        return n

    def push_device(self, buf_or_ptr, first_sample, n):
        """Stream k takes n[k] samples that start first_sample[k] samples behind the device pointer (16-byte aligned)."""
        first = np.ascontiguousarray(first_sample, np.uint64)
        n = np.ascontiguousarray(n, np.uint32)
        if first.size != self.n_streams or n.size != self.n_streams:
            raise NfcError('push_device: first_sample and n hold %d / %d entries for %d streams' % (first.size, n.size, self.n_streams))
        self._chk(self.L.nfc_multi_push_device(self.h, _as_pointer(buf_or_ptr), first.ctypes.data, n.ctypes.data), 'nfc_multi_push_device')
        return n

    def stream(self, k, allow_truncated=False):
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('stream %d out of range (n_streams %d)' % (k, self.n_streams))
        return NfcMultiStream(self, int(k), allow_truncated)

    def fetch(self, what=NFC_MULTI_FETCH_ALL, copy=True, allow_truncated=False):
        """Everything the streams stored in the last push, packed on the GPU and brought to the host in ONE copy (nfc_multi_fetch):
        -> NfcMultiFetch.  what: NFC_MULTI_FETCH_* bits (PACKETS: the packet tables and the bit arrays).  Until the next push the
        stream views read the arrays `what` covers from that host copy, without a device call.
        copy=True (default): the arrays are numpy copies and stay valid.  copy=False: they are views of the context's pinned
        memory, valid only until the next push, fetch, reset (of any stream), set_state or close of this context -- reading them
        afterwards reads freed or rewritten memory."""
        f = _lib.MultiFetched()
        self._chk(self.L.nfc_multi_fetch(self.h, int(what), C.byref(f)), 'nfc_multi_fetch')
        return NfcMultiFetch(self, f, copy, allow_truncated)

    def fetch_frames(self, copy=True):
        """Every stream's stored packets as frames assembled on the GPU -- bytes, parity bits, parity and CRC_A verdicts -- in ONE
        packed buffer and one copy (nfc_multi_fetch_frames) -> NfcMultiFrames.  It has buffers of its own: a fetch() made before stays
        readable, and the reverse.  copy=False: views of the context's pinned memory, valid until the next push, fetch_frames, reset,
        set_state or close of this context."""
        f = _lib.MultiFrames()
        self._chk(self.L.nfc_multi_fetch_frames(self.h, C.byref(f)), 'nfc_multi_fetch_frames')
        return NfcMultiFrames(f, copy)

    def track_commands(self, on=True):
        """While on, every push also assembles the frames and runs the protocol machine, CRYPTO1 included, a GPU lane per stream
        (nfc_multi_track_commands): three more launches behind the push's own, no host wait.  The machines' state stays on the device
        from push to push; fetch_commands() brings the last push's commands to the host."""
        self._chk(self.L.nfc_multi_track_commands(self.h, int(bool(on))), 'nfc_multi_track_commands')

    def set_keys(self, key_a=(0xFF,) * 6, key_b=(0xFF,) * 6, stream=None):
        """MIFARE Classic sector keys A / B of one stream's machine (default: of every stream's), six bytes each, as fsm.set_keys."""
        a, b = np.ascontiguousarray(key_a, np.uint8), np.ascontiguousarray(key_b, np.uint8)
        if a.size != 6 or b.size != 6:
            raise NfcError('set_keys: key_a and key_b are six bytes each')
        self._chk(self.L.nfc_multi_set_keys(self.h, -1 if stream is None else int(stream), a.ctypes.data, b.ctypes.data), 'nfc_multi_set_keys')

    def set_sector_keys(self, table, stream=None):
        """The per-sector key table of one stream's machine (default: of every stream's), as fsm.set_sector_keys: a dict
        (key_type, sector) -> six key bytes or an _lib.FsmKeyTable; None or {} empties it (nfc_multi_set_sector_keys).  The first call
        allocates the tables' device buffer, 640 bytes per stream; reset(k) empties stream k's table."""
        from . import keys
        try:
            t = keys.key_table(table)
        except ValueError as e:
            raise NfcError('set_sector_keys: %s' % e)
        self._chk(self.L.nfc_multi_set_sector_keys(self.h, -1 if stream is None else int(stream), C.byref(t)), 'nfc_multi_set_sector_keys')

    def sector_keys(self, k):
        """Stream k's key table as the dict (key_type, sector) -> six key bytes of its present slots (nfc_multi_get_sector_keys)."""
        from . import keys
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('sector_keys: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        t = _lib.FsmKeyTable()
        self._chk(self.L.nfc_multi_get_sector_keys(self.h, int(k), C.byref(t)), 'nfc_multi_get_sector_keys')
        return keys.table_dict(t)

    def recover_keys(self, nested=False, reader_pairs=False, **cfg):
        """The sector keys of the last push's first authentications: fetch_frames() + NfcMultiFrames.auths() + ONE keys.recover call on
        this context's device (cfg: keys.recover's).  -> per stream a dict (key_type, block) -> six key bytes (keys.keys_by_stream).
        nested=True: the nested authentications too (keys.recover_streams: one more call, keys.recover_nested, and keys.label_auths per
        stream), so the dicts also hold every later sector's key whose AUTH command could be decrypted.
        reader_pairs: True, or a dict of keys.recover_reader's OWN options (stage_capacity, verify_inline) -- the first authentications
        that are left without a key (no {at}, or a noise one) are paired and searched besides (keys.recover_reader_streams: ONE more
        call, with the same cfg)."""
        from . import keys
        if nested:
            fr = self.fetch_frames()
            have = (np.diff(fr.frame_off[0]) > 0) & (np.diff(fr.frame_off[1]) > 0)
            return keys.recover_streams([fr.frames_of(k) if have[k] else None for k in range(self.n_streams)], device=self.device,
                                        reader_pairs=reader_pairs, **cfg)
        fr = self.fetch_frames()
        traces = fr.auths()
        results, _ = keys.recover(traces, device=self.device, **cfg)
        found = keys.keys_by_stream(traces, results, self.n_streams)
        if reader_pairs:
            found = keys.recover_reader_streams(fr.reader_auths(), found, device=self.device, **keys.reader_options(reader_pairs, cfg))
        return found

    def fsm_state(self, k):
        """Stream k's protocol machine as a plain nfc_fsm_state (an _lib.FsmState): what fsm.set_state takes."""
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('fsm_state: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        st = _lib.FsmState()
        self._chk(self.L.nfc_multi_get_fsm_state(self.h, int(k), C.byref(st)), 'nfc_multi_get_fsm_state')
        return st

    def set_fsm_state(self, k, st):
        """Stream k's machine continues from `st` (fsm.get_state(), another stream's fsm_state())."""
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('set_fsm_state: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        self._chk(self.L.nfc_multi_set_fsm_state(self.h, int(k), C.byref(st)), 'nfc_multi_set_fsm_state')

    def fetch_commands(self, copy=True):
        """The commands of the last push, tracked on the GPU (track_commands), in ONE copy (nfc_multi_fetch_commands) -> NfcMultiCommands.
        copy=False: views of the context's pinned memory, valid until the next push, fetch_commands, reset, set_state, set_fsm_state or
        close of this context."""
        c = _lib.MultiCommands()
        self._chk(self.L.nfc_multi_fetch_commands(self.h, C.byref(c)), 'nfc_multi_fetch_commands')
        return NfcMultiCommands(c, copy)

    def track_images(self, on=True):
        """While on, every tracked push also rebuilds every stream's card from its commands (nfc_multi_track_images; it switches command
        tracking on): one launch more, k_multi_images, a wave per stream, no host wait.  The images stay on the device from push to
        push; fetch_images() brings them."""
        self._chk(self.L.nfc_multi_track_images(self.h, int(bool(on))), 'nfc_multi_track_images')

    def fetch_images(self, copy=True):
        """Every stream's memory image in ONE copy (nfc_multi_fetch_images) -> NfcMultiImages.  copy=False: views of the context's pinned
        memory, valid until the next fetch_images that copies, or close."""
        f = _lib.MultiImages()
        self._chk(self.L.nfc_multi_fetch_images(self.h, C.byref(f)), 'nfc_multi_fetch_images')
        return NfcMultiImages(f, copy)

    def image(self, k):
        """Stream k's image, tail included, as an emulate.CardImage (nfc_multi_get_image)."""
        from . import emulate
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('image: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        rec = np.zeros((), _lib.CARD_IMAGE_DTYPE)
        self._chk(self.L.nfc_multi_get_image(self.h, int(k), rec.ctypes.data), 'nfc_multi_get_image')
        return emulate.CardImage(rec)

    def set_image(self, k, image):
        """Stream k's image continues from `image` (an emulate.CardImage: host_card_image's, another stream's)."""
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('set_image: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        rec = np.ascontiguousarray(image.rec, _lib.CARD_IMAGE_DTYPE)
        self._chk(self.L.nfc_multi_set_image(self.h, int(k), rec.ctypes.data), 'nfc_multi_set_image')

    def emulate(self, cards, stream=-1):
        """Give stream `stream` a card (an emulate.Card; -1: every stream; a list: one per stream, None for none), or None to take it away
        (nfc_multi_emulate).  From then on a tracked push -- tracking is switched on -- runs the emulating form of the machine kernel: the
        stream answers what it hears, in the launch that decodes its commands; fetch_answers() brings the answers."""
        if isinstance(cards, (list, tuple)):
            if len(cards) != self.n_streams:
                raise NfcError('emulate: a list of cards has one entry per stream')
            for k, c in enumerate(cards):
                self.emulate(c, k)
            return
        c = None if cards is None else cards.struct()
        self._chk(self.L.nfc_multi_emulate(self.h, int(stream), None if c is None else C.byref(c)), 'nfc_multi_emulate')

    def fetch_answers(self, copy=True):
        """The answers of the last push (nfc_multi_fetch_answers): sections of the buffer fetch_commands() copies, so after a fetch of the
        commands, or a second call, no device call -> NfcMultiAnswers."""
        a = _lib.MultiAnswers()
        self._chk(self.L.nfc_multi_fetch_answers(self.h, C.byref(a)), 'nfc_multi_fetch_answers')
        return NfcMultiAnswers(a, copy)

    def emu_state(self, k):
        """Stream k's emulator as a plain nfc_emu_state (an _lib.EmuState)."""
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('emu_state: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        st = _lib.EmuState()
        self._chk(self.L.nfc_multi_get_emu_state(self.h, int(k), C.byref(st)), 'nfc_multi_get_emu_state')
        return st

    def set_emu_state(self, k, st):
        """Stream k's emulator continues from `st` (emulate.state_init(), another stream's emu_state())."""
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('set_emu_state: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        self._chk(self.L.nfc_multi_set_emu_state(self.h, int(k), C.byref(st)), 'nfc_multi_set_emu_state')

    def transmit(self, samp_rate=2e6, in_rate=None, delay_us=0.0, carrier=False, freq=13.56e6, amp=1.0, first_index=0, align_samples=8,
                 out=None, timed=False, _reserved=0):
        """What the streams that hold a card transmit for the last push, rendered on the GPU (nfc_multi_transmit_device): every answer as
        the reference's binary_src -> multiplier chain would send it, delay_us behind the moment the answered command closed, idle level
        elsewhere; an answer that reaches beyond the push's span is carried to the next transmit().  Once per push, enqueued behind the
        push's kernels with no host wait.  samp_rate: of the output, in_rate: of the input (None: the same).  out: a DeviceBuffer (or
        (pointer, cap_samples)) to render into, 32-byte aligned; None: a buffer of the needed size is allocated and owned by the result.
        timed: the two passes' durations -> .kernel_ms (waits).  -> tx.TxCaptures, whose wait() completes the rendering."""
        from . import tx
        cfg = tx.answers_tx_config(samp_rate, in_rate, delay_us, carrier, freq, amp, first_index, align_samples, _reserved)
        first, n = np.zeros(self.n_streams, np.uint64), np.zeros(self.n_streams, np.uint32)
        ms = (C.c_float * 2)()
        call = lambda ptr, cap: self.L.nfc_multi_transmit_device(self.h, C.byref(cfg), ptr, int(cap), first.ctypes.data, n.ctypes.data,
                                                                 C.byref(ms) if timed else None)
        buf, owned = out, False
        if out is None:   # the sizing call: a layout that does not fit renders nothing and reports the need
            rc = call(None, 0)
            if rc == 0:   # (nothing to render: no stream with a card was given a sample)
                return tx.TxCaptures(first, n, None, False, samp_rate, self.device, tuple(ms) if timed else None, self)
            if rc != -1 or b'cap_samples' not in self.L.nfc_multi_last_error(self.h):
                self._chk(rc, 'nfc_multi_transmit_device')
            cap = int(first[-1]) + int(n[-1])
            buf, owned = DeviceBuffer(np.zeros(0, np.float32), self.device, nbytes=max(8 * cap, 32)), True
            ptr = buf.ptr
        elif isinstance(out, DeviceBuffer):
            ptr, cap = out.ptr, out.nbytes // 8
        else:
            ptr, cap = _as_pointer(out[0]), int(out[1])
        rc = call(ptr, cap)
        if rc != 0 and owned:
            buf.free()
        self._chk(rc, 'nfc_multi_transmit_device')
        return tx.TxCaptures(first, n, buf if isinstance(buf, DeviceBuffer) else ptr, owned, samp_rate, self.device, tuple(ms) if timed else None, self)

    def tx_state(self, k):
        """Stream k's pending answer as a plain nfc_tx_pending (an _lib.TxPending; n_bits 0: none)."""
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('tx_state: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        st = _lib.TxPending()
        self._chk(self.L.nfc_multi_get_tx_state(self.h, int(k), C.byref(st)), 'nfc_multi_get_tx_state')
        return st

    def set_tx_state(self, k, st):
        """Stream k continues with the pending answer `st` (another stream's tx_state(), emulate.host_transmit's)."""
        if not 0 <= int(k) < self.n_streams:
            raise NfcError('set_tx_state: stream %d out of range (n_streams %d)' % (k, self.n_streams))
        if isinstance(st, np.void):
            st = _lib.TxPending.from_buffer_copy(st.tobytes())
        self._chk(self.L.nfc_multi_set_tx_state(self.h, int(k), C.byref(st)), 'nfc_multi_set_tx_state')

    def counts_all(self):
        """Every stream's counts and flags of the last push from one call: a COUNTS_FLAGS_DTYPE array of n_streams records."""
        cnt, flags = np.zeros(self.n_streams, COUNTS_DTYPE), np.zeros(self.n_streams, np.uint32)
        self._chk(self.L.nfc_multi_get_counts_all(self.h, cnt.ctypes.data, flags.ctypes.data), 'nfc_multi_get_counts_all')
        out = np.zeros(self.n_streams, COUNTS_FLAGS_DTYPE)
        for name in COUNTS_DTYPE.names:
            out[name] = cnt[name]
        out['flags'] = flags
        return out

    def reset(self, stream=-1):
        """A new stream in place of stream k (default: of every one), keeping the device buffers."""
        self._chk(self.L.nfc_multi_reset(self.h, int(stream)), 'nfc_multi_reset')

    def stats(self):
        s = _lib.MultiStats()
        self._chk(self.L.nfc_multi_get_stats(self.h, C.byref(s)), 'nfc_multi_get_stats')
        return s

    def set_timing(self, on):
        """HIP events around the push's launch: stats().ms_kernels."""
        self._chk(self.L.nfc_multi_set_timing(self.h, int(bool(on))), 'nfc_multi_set_timing')


class NfcMultiStream(object):
    """One stream of an NfcMultiContext: the reading side of an NfcContext (counts, edges, transitions, symbols, packets, state), so
    that background._deliver(view) works unchanged.  Reading an array that the stream's slab cut short raises NfcError naming the
    flag, unless allow_truncated: then what was stored -- the first cap_* entries -- comes back."""

    def __init__(self, multi, k, allow_truncated=False):
        self.m, self.k, self.allow_truncated = multi, k, allow_truncated
        self.factor = multi.factor

    def _counts(self):
        c, f = _lib.Counts(), C.c_uint32(0)
        self.m._chk(self.m.L.nfc_multi_get_counts(self.m.h, self.k, C.byref(c), C.byref(f)), 'nfc_multi_get_counts')
        return c, int(f.value)

    def counts(self):
        return self._counts()[0]

    def flags(self):
        return self._counts()[1]

    def _stored(self, field, ptype, bit, allow):
        """How many entries of the array to read (counts.field, [ptype]), from ONE counts call; a cut array raises unless allowed."""
        c, f = self._counts()
        bad = f & _trunc_mask(bit)
        if bad and not (self.allow_truncated if allow is None else allow):
            raise NfcError('stream %d: %s (pass allow_truncated=True for what was stored)' % (self.k, _flag_names(bad)))
        total = getattr(c, field)
        return int(total if ptype is None else total[ptype])

    def _read(self, fn, total, dtype, *lead):
        out = np.zeros(int(total), dtype)
        got = C.c_size_t(0)
        if total:
            self.m._chk(fn(self.m.h, self.k, *lead, out.ctypes.data, out.size, C.byref(got)), fn.__name__)
        return out[:got.value]

    def edges(self, allow_truncated=None):
        n = self._stored('n_edges', None, NFC_MULTI_TRUNC_EDGES, allow_truncated)
        return self._read(self.m.L.nfc_multi_read_edges, n, EDGE_DTYPE, 0)

    def transitions(self, allow_truncated=None):
        e = self.edges(allow_truncated)
        f = self.factor
        return [((int(v), int(d) * f), int(t)) for v, d, t in zip(e['v'], e['d'], e['t'])]

    def symbols(self, ptype, allow_truncated=None):
        n = self._stored('n_symbols', ptype, NFC_MULTI_TRUNC_SYMBOLS, allow_truncated)
        return self._read(self.m.L.nfc_multi_read_symbols, n, np.uint8, ptype, 0)

    def packet_table(self, ptype, allow_truncated=None):
        n = self._stored('n_packets', ptype, NFC_MULTI_TRUNC_PACKETS, allow_truncated)
        out = np.zeros(n, PACKET_DTYPE)
        got = C.c_size_t(0)
        if n:
            self.m._chk(self.m.L.nfc_multi_read_packets(self.m.h, self.k, ptype, out.ctypes.data, out.size, C.byref(got)), 'nfc_multi_read_packets')
        return out[:got.value]

    def packet_bits(self, ptype, allow_truncated=None):
        """The per-type bit array the packet table's bit_off / n_bits index."""
        n = self._stored('n_packet_bits', ptype, NFC_MULTI_TRUNC_BITS, allow_truncated)
        return self._read(self.m.L.nfc_multi_read_packet_bits, n, np.uint8, ptype, 0)

    def packets(self, allow_truncated=None):
        """Closed packets of both types in stream order: [(type, [bits]), ...] (NfcContext.packets)."""
        items = []
        for t in (0, 1):
            tab = self.packet_table(t, allow_truncated)
            if not len(tab):
                continue
            bits = self.packet_bits(t, allow_truncated)
            for p in tab:
                o = int(p['bit_off'])
                if o + int(p['n_bits']) <= len(bits):   # (a cut bit array: the packets it still holds whole)
                    items.append((int(p['idx']), t, bits[o:o + int(p['n_bits'])].tolist()))
        items.sort(key=lambda r: r[0])
        return [(t, b) for _, t, b in items]

    def get_state(self):
        """(header, ring float32[av_window], [pending bits type 0, pending bits type 1]) -- NfcContext.get_state's."""
        L, h = self.m.L, _lib.StateHeader()
        self.m._chk(L.nfc_multi_get_state(self.m.h, self.k, C.byref(h), None, 0, None, 0), 'nfc_multi_get_state')
        ring = np.zeros(h.av_window, np.float32)
        p0, p1 = int(h.n_pending_bits[0]), int(h.n_pending_bits[1])
        pend = np.zeros(p0 + p1, np.uint8)
        self.m._chk(L.nfc_multi_get_state(self.m.h, self.k, C.byref(h), ring.ctypes.data, ring.size, pend.ctypes.data, pend.size),
                    'nfc_multi_get_state')
        return h, ring, [pend[:p0].copy(), pend[p0:].copy()]

    def set_state(self, header, ring, pending=None):
        ring = np.ascontiguousarray(ring, np.float32)
        pend = np.zeros(0, np.uint8) if pending is None else np.ascontiguousarray(np.concatenate(pending), np.uint8)
        self.m._chk(self.m.L.nfc_multi_set_state(self.m.h, self.k, C.byref(header), ring.ctypes.data, ring.size, pend.ctypes.data, pend.size),
                    'nfc_multi_set_state')

    def reset(self):
        self.m.reset(self.k)


class NfcMultiFetch(object):
    """What every stream of an NfcMultiContext stored in its last push, in packed host arrays (NfcMultiContext.fetch).

    off[a] (a: NFC_MF_EDGES, NFC_MF_SYM0, NFC_MF_SYM1, NFC_MF_PK0, NFC_MF_PK1, NFC_MF_BITS0, NFC_MF_BITS1): n_streams + 1 offsets, stream
    k's entries of array a are [off[a][k], off[a][k + 1]) -- ``numpy.split(array, off[a][1:-1])`` is the per-stream view.  base[k]: the
    stream's sample count before the push.  edge_pos / edge_code: the edges as the device keeps them (``edges(k)`` expands them);
    symbols[t], packet_table[t] (PACKET_DTYPE, bit_off relative to the stream's own part of packet_bits[t]), packet_bits[t] (a stream's
    part is its bit row as stored: the closed packets' bits, then those of a packet still open at the push's end, which
    ``packet_bits_of`` leaves out as NfcMultiStream.packet_bits does).  Arrays the fetch did not ask for are empty.  counts: the
    COUNTS_FLAGS_DTYPE records of NfcMultiContext.counts_all.  flags[k]: the stream's NFC_MULTI_* flags; the per-stream accessors raise NfcError for an
    array its stream cut short unless allow_truncated (theirs, else the fetch's): then the stored prefix comes back.
    With fetch(copy=False) every array is a view of the context's pinned memory: see NfcMultiContext.fetch for how long it lives."""

    def __init__(self, multi, f, copy, allow_truncated=False):
        K = int(f.n_streams)
        self.what, self.n_streams, self.nd, self.factor = int(f.what), K, int(f.edge_code_nd), multi.factor
        self.n_launches, self.bytes_copied, self.ms_kernels = int(f.n_launches), int(f.bytes_copied), float(f.ms_kernels)
        self.allow_truncated = allow_truncated

        def arr(ptr, n, dtype):
            dtype = np.dtype(dtype)
            if not ptr or not n:
                return np.zeros(0, dtype)
            a = np.frombuffer((C.c_char * (int(n) * dtype.itemsize)).from_address(ptr), dtype)
            return a.copy() if copy else a

        self.off = [arr(f.off[a], K + 1, '<u8') for a in range(NFC_MF_ARRAYS)]
        tot = [int(o[K]) for o in self.off]
        self.base = arr(f.base, K, '<u8')
        self.edge_pos = arr(f.edge_pos, tot[NFC_MF_EDGES], '<u4')
        self.edge_code = arr(f.edge_code, tot[NFC_MF_EDGES], '<u2')
        self.symbols = [arr(f.symbols[t], tot[NFC_MF_SYM0 + t], np.uint8) for t in (0, 1)]
        self.packet_table = [arr(f.packets[t], tot[NFC_MF_PK0 + t], PACKET_DTYPE) for t in (0, 1)]
        self.packet_bits = [arr(f.packet_bits[t], tot[NFC_MF_BITS0 + t], np.uint8) for t in (0, 1)]
        self.counts = multi.counts_all()   # (the true totals, whatever was stored)
        self.flags = self.counts['flags']

    def _need(self, bit, name):
        if not self.what & bit:
            raise NfcError('this fetch did not ask for the %s (what = %d)' % (name, self.what))

    def _allowed(self, k, bit, allow):
        bad = int(self.flags[k]) & _trunc_mask(bit)
        if bad and not (self.allow_truncated if allow is None else allow):
            raise NfcError('stream %d: %s (pass allow_truncated=True for what was stored)' % (k, _flag_names(bad)))

    def _slice(self, a, array, k):
        return array[int(self.off[a][k]):int(self.off[a][k + 1])]

    def edges(self, k, allow_truncated=None):
        """Stream k's edges as an EDGE_DTYPE array: NfcMultiStream.edges()."""
        self._need(NFC_MULTI_FETCH_EDGES, 'edges')
        self._allowed(k, NFC_MULTI_TRUNC_EDGES, allow_truncated)
        pos, code = self._slice(NFC_MF_EDGES, self.edge_pos, k), self._slice(NFC_MF_EDGES, self.edge_code, k).astype(np.int32)
        out = np.zeros(len(pos), EDGE_DTYPE)
        li = code & 0x3FFF   # edges.hip.h: edge_code, and back
        out['idx'] = self.base[k] + pos.astype(np.uint64)
        out['d'] = li % self.nd
        out['v'] = li // self.nd - 1
        out['t'] = (code >> 14) - 1
        return out

    def transitions(self, k, allow_truncated=None):
        e = self.edges(k, allow_truncated)
        f = self.factor
        return [((int(v), int(d) * f), int(t)) for v, d, t in zip(e['v'], e['d'], e['t'])]

    def symbols_of(self, k, ptype, allow_truncated=None):
        self._need(NFC_MULTI_FETCH_SYMBOLS, 'symbols')
        self._allowed(k, NFC_MULTI_TRUNC_SYMBOLS, allow_truncated)
        return self._slice(NFC_MF_SYM0 + ptype, self.symbols[ptype], k)

    def packet_table_of(self, k, ptype, allow_truncated=None):
        self._need(NFC_MULTI_FETCH_PACKETS, 'packets')
        self._allowed(k, NFC_MULTI_TRUNC_PACKETS, allow_truncated)
        return self._slice(NFC_MF_PK0 + ptype, self.packet_table[ptype], k)

    def packet_bits_of(self, k, ptype, allow_truncated=None):
        self._need(NFC_MULTI_FETCH_PACKETS, 'packets')
        self._allowed(k, NFC_MULTI_TRUNC_BITS, allow_truncated)
        return self._slice(NFC_MF_BITS0 + ptype, self.packet_bits[ptype], k)[:int(self.counts['n_packet_bits'][k][ptype])]

    def packets_of(self, k, allow_truncated=None):
        """Stream k's closed packets of both types in stream order, [(type, [bits]), ...]: NfcMultiStream.packets(), with its rule for
        a cut bit array (the packets it still holds whole)."""
        items = []
        for t in (0, 1):
            tab = self.packet_table_of(k, t, allow_truncated)
            if not len(tab):
                continue
            bits = self.packet_bits_of(k, t, allow_truncated)
            for p in tab:
                o = int(p['bit_off'])
                if o + int(p['n_bits']) <= len(bits):
                    items.append((int(p['idx']), t, bits[o:o + int(p['n_bits'])].tolist()))
        items.sort(key=lambda r: r[0])
        return [(t, b) for _, t, b in items]

    def packets_all(self, allow_truncated=None):
        """[packets_of(k) for every stream], built from the packed arrays with numpy: no call into the library per stream."""
        self._need(NFC_MULTI_FETCH_PACKETS, 'packets')
        K = self.n_streams
        if not (self.allow_truncated if allow_truncated is None else allow_truncated):
            cut = np.nonzero(self.flags & (NFC_MULTI_TRUNC_PACKETS | NFC_MULTI_TRUNC_BITS | NFC_MULTI_PENDING_OVERFLOW))[0]
            if len(cut):
                raise NfcError('stream %d: %s (pass allow_truncated=True for what was stored)' % (int(cut[0]), _flag_names(int(self.flags[cut[0]]))))
        cols = []
        for t in (0, 1):
            tab = self.packet_table[t]
            if not len(tab):
                continue
            stream = np.repeat(np.arange(K, dtype=np.int64), np.diff(self.off[NFC_MF_PK0 + t]).astype(np.int64))
            bo = self.off[NFC_MF_BITS0 + t].astype(np.int64)
            a = bo[stream] + tab['bit_off'].astype(np.int64)
            b = a + tab['n_bits'].astype(np.int64)
            whole = b <= np.minimum(bo[stream + 1], bo[stream] + self.counts['n_packet_bits'][stream, t].astype(np.int64))   # (a cut bit array: the packets it still holds whole)
            cols.append((stream[whole], tab['idx'][whole].astype(np.int64), np.full(int(whole.sum()), t, np.int64), a[whole], b[whole]))
        out = [[] for _ in range(K)]
        if not cols:
            return out
        stream, idx, typ, a, b = (np.concatenate(c) for c in zip(*cols))
        order = np.lexsort((typ, idx, stream))   # per stream by the closing sample, type 0 first on a tie: packets_of's order
        bits = self.packet_bits
        for s, t, i, j in zip(stream[order].tolist(), typ[order].tolist(), a[order].tolist(), b[order].tolist()):
            out[s].append((t, bits[t][i:j].tolist()))
        return out


def _merge_frames(records):
    """Both types' RAW_FRAME_DTYPE records in stream order: by idx, type 0 first on a tie (a tie cannot happen: one edge feeds one decoder)."""
    t = np.concatenate(records) if len(records) else np.zeros(0, RAW_FRAME_DTYPE)
    return t[np.lexsort((t['type'], t['idx']))] if len(t) else t


class NfcFrames(object):
    """Frames of one stream: `records[t]` the RAW_FRAME_DTYPE records per type in the packet table's order, `table` both types merged
    by idx, `bytes[t]` / `par[t]` the data bytes and the ninth bits as received, indexed by a record's byte_off."""

    def __init__(self, records, data, par):
        self.records, self.bytes, self.par = list(records), list(data), list(par)
        self.table = _merge_frames(self.records)

    def data_of(self, rec):
        """The bytes of one record, as a numpy view."""
        o = int(rec['byte_off'])
        return self.bytes[int(rec['type'])][o:o + int(rec['n_bytes'])]

    def crc_ok_mask(self):
        return (self.table['flags'] & NFC_RAW_CRC_A_OK) != 0


class NfcMultiFrames(object):
    """What nfc_multi_fetch_frames packs: frames[t] (RAW_FRAME_DTYPE; byte_off relative to the stream's own part of bytes[t] / par[t],
    idx in the stream's own sample count), bytes[t], par[t]; frame_off[t] / byte_off[t]: n_streams + 1 offsets, stream k's frames of
    type t are frames[t][frame_off[t][k]:frame_off[t][k + 1]] and its bytes bytes[t][byte_off[t][k]:byte_off[t][k + 1]].  A frame whose
    bits the stream's slab cut carries NFC_RAW_CUT and no bytes."""

    def __init__(self, f, copy=True):
        K = int(f.n_streams)
        self.n_streams, self.n_launches, self.bytes_copied, self.ms_kernels = K, int(f.n_launches), int(f.bytes_copied), float(f.ms_kernels)

        def arr(ptr, n, dtype):
            dtype = np.dtype(dtype)
            if not ptr or not n:
                return np.zeros(0, dtype)
            a = np.frombuffer((C.c_char * (int(n) * dtype.itemsize)).from_address(ptr), dtype)
            return a.copy() if copy else a

        self.frame_off = [arr(f.frame_off[t], K + 1, '<u8') for t in (0, 1)]
        self.byte_off = [arr(f.byte_off[t], K + 1, '<u8') for t in (0, 1)]
        self.base = arr(f.base, K, '<u8')
        self.frames = [arr(f.frames[t], self.frame_off[t][K], RAW_FRAME_DTYPE) for t in (0, 1)]
        self.bytes = [arr(f.bytes[t], self.byte_off[t][K], np.uint8) for t in (0, 1)]
        self.par = [arr(f.par[t], self.byte_off[t][K], np.uint8) for t in (0, 1)]

    def frames_of(self, k):
        """Stream k's part as an NfcFrames of numpy views (no copy)."""
        recs, data, par = [], [], []
        for t in (0, 1):
            recs.append(self.frames[t][int(self.frame_off[t][k]):int(self.frame_off[t][k + 1])])
            a, b = int(self.byte_off[t][k]), int(self.byte_off[t][k + 1])
            data.append(self.bytes[t][a:b]), par.append(self.par[t][a:b])
        return NfcFrames(recs, data, par)

    def auths(self):
        """Every stream's first authentications (keys.find_auths per stream, in stream order) as ONE AUTH_DTYPE array, `stream` filled
        in and `idx` in the stream's own sample count: what keys.recover takes.  A loop over the streams that have frames of both types."""
        from . import keys
        parts = []
        for k in np.nonzero((np.diff(self.frame_off[0]) > 0) & (np.diff(self.frame_off[1]) > 0))[0]:
            a = keys.find_auths(self.frames_of(int(k)))
            a['stream'] = int(k)
            parts.append(a)
        return np.concatenate(parts) if parts else np.zeros(0, _lib.AUTH_DTYPE)

    def reader_auths(self):
        """Every stream's first authentications as far as the reader's {nr}{ar} (keys.find_reader_auths per stream, in stream order) as
        ONE AUTH_DTYPE array, `stream` filled in: what keys.pair_reader_auths and keys.recover_reader_streams take."""
        from . import keys
        parts = []
        for k in np.nonzero((np.diff(self.frame_off[0]) > 0) & (np.diff(self.frame_off[1]) > 0))[0]:
            a = keys.find_reader_auths(self.frames_of(int(k)))
            a['stream'] = int(k)
            parts.append(a)
        return np.concatenate(parts) if parts else np.zeros(0, _lib.AUTH_DTYPE)

    def nested_auths(self):
        """Every stream's nested authentications (keys.find_nested_auths per stream, in stream order) as ONE NESTED_DTYPE array, `stream`
        filled in: what keys.recover_nested takes."""
        from . import keys
        parts = []
        for k in np.nonzero((np.diff(self.frame_off[0]) > 0) & (np.diff(self.frame_off[1]) > 0))[0]:
            a = keys.find_nested_auths(self.frames_of(int(k)))
            a['stream'] = int(k)
            parts.append(a)
        return np.concatenate(parts) if parts else np.zeros(0, _lib.NESTED_DTYPE)

    def stream_of(self, ptype):
        """The stream every frame of frames[ptype] belongs to."""
        return np.repeat(np.arange(self.n_streams, dtype=np.int64), np.diff(self.frame_off[ptype]).astype(np.int64))

    def crc_ok_mask(self):
        """Per type, over ALL frames of frames[t]: parity held and the CRC_A matched."""
        return [(self.frames[t]['flags'] & NFC_RAW_CRC_A_OK) != 0 for t in (0, 1)]


class NfcMultiAnswers(object):
    """What the streams of a multi-stream context answered in the last push (nfc_multi_fetch_answers).  `n[k]` answers of stream k;
    answers_of(k) -> (records, plain, air, par): EMU_ANSWER_DTYPE records (src: the index of the command it answers among the stream's
    commands) and the stream's bytes, a record's at its byte_off -- numpy views of the fetched arrays (copies with copy=True)."""

    def __init__(self, a, copy=True):
        K = int(a.n_streams)
        self.n_streams, self.emulated, self.n_answers = K, bool(a.emulated), int(a.n_answers)

        def arr(ptr, n, dtype):
            dtype = np.dtype(dtype)
            if not ptr or n == 0:
                return np.zeros(0, dtype)
            v = np.frombuffer((C.c_uint8 * (n * dtype.itemsize)).from_address(ptr), dtype)
            return v.copy() if copy else v
        self.cmd_off = arr(a.cmd_off, K + 1, '<u8')
        total = int(self.cmd_off[K]) if len(self.cmd_off) else 0
        self.n = arr(a.ans_n, K, '<u4') if self.emulated else np.zeros(K, np.uint32)
        self.records = arr(a.ans, total, _lib.EMU_ANSWER_DTYPE) if self.emulated else np.zeros(0, _lib.EMU_ANSWER_DTYPE)
        self.plain, self.air, self.par = ((arr(p, 18 * total, 'u1') if self.emulated else np.zeros(0, np.uint8)) for p in (a.plain, a.air, a.par))

    def answers_of(self, k):
        if not self.emulated or int(self.n[k]) == 0:
            z = np.zeros(0, np.uint8)
            return np.zeros(0, _lib.EMU_ANSWER_DTYPE), z, z, z
        c0, n = int(self.cmd_off[k]), int(self.n[k])
        sl = slice(18 * c0, 18 * (c0 + n))
        return self.records[c0:c0 + n], self.plain[sl], self.air[sl], self.par[sl]

    def bits(self, k, i):
        """Answer i of stream k as the bit list the reference's emulator hands binary_src.set_bits (what tx.encode takes)."""
        rec, _, air, par = self.answers_of(k)
        o, n = int(rec[i]['byte_off']), int(rec[i]['n_bytes'])
        if int(rec[i]['n_bits']) == 7:
            return [(int(air[o]) >> j) & 1 for j in range(7)]
        out = []
        for v, q in zip(air[o:o + n].tolist(), par[o:o + n].tolist()):
            out += [(v >> j) & 1 for j in range(8)] + [q & 1]
        return out


class NfcMultiImages(object):
    """What nfc_multi_fetch_images brings: every stream's card as it was heard.  mem_all / src_all: [n_streams][1024] bytes and their source
    codes (_lib.NFC_IMG_SRC_*; 0: never shown); tag_type (-1: no ATQA heard), flags (_lib.NFC_IMG_*), n_known: one entry per stream; tail:
    [n_streams][3] IMAGE_CMD_DTYPE, the summaries of each stream's last three commands."""

    def __init__(self, f, copy=True):
        K = int(f.n_streams)
        self.n_streams, self.n_launches, self.bytes_copied, self.ms_kernel = K, int(f.n_launches), int(f.bytes_copied), float(f.ms_kernel)

        def arr(ptr, n, dtype):
            dtype = np.dtype(dtype)
            a = np.frombuffer((C.c_char * (int(n) * dtype.itemsize)).from_address(ptr), dtype)
            return a.copy() if copy else a
        self.mem_all = arr(f.mem, K * _lib.NFC_IMG_BYTES, np.uint8).reshape(K, _lib.NFC_IMG_BYTES)
        self.src_all = arr(f.src, K * _lib.NFC_IMG_BYTES, np.uint8).reshape(K, _lib.NFC_IMG_BYTES)
        self.info = arr(f.info, K, _lib.IMAGE_INFO_DTYPE)
        self.tail = arr(f.tail, K * _lib.NFC_IMG_TAIL, _lib.IMAGE_CMD_DTYPE).reshape(K, _lib.NFC_IMG_TAIL)
        self.tag_type, self.flags, self.n_known = self.info['tag_type'], self.info['flags'], self.info['n_known']

    def mem(self, k):
        return self.mem_all[k]

    def src(self, k):
        return self.src_all[k]

    def known_mask(self, k):
        return self.src_all[k] != 0

    def coverage(self):
        """Per stream: the known share of the card's memory (64 bytes for an Ultralight, else 1 024)."""
        size = np.where(self.tag_type == 0, 64, _lib.NFC_IMG_BYTES)
        return self.n_known.astype(np.float64) / size

    def image(self, k):
        """Stream k's image as an emulate.CardImage (a copy): what host_card_image gives and set_image takes."""
        from . import emulate
        rec = np.zeros((), _lib.CARD_IMAGE_DTYPE)
        rec['mem'], rec['src'], rec['info'], rec['tail'] = self.mem_all[k], self.src_all[k], self.info[k], self.tail[k]
        return emulate.CardImage(rec)

    def card(self, k, rands=None, mode=_lib.NFC_EMU_CARD):
        """Stream k's image as a tag to emulate (emulate.tag_card), unknown bytes as zeros."""
        return self.image(k).card(rands, mode)

    def to_json(self, k, path, rands=None):
        """Stream k's image as one of the reference's card files (parser.Parser reads it)."""
        return self.image(k).to_json(path, rands)


class NfcMultiCommands(object):
    """What nfc_multi_fetch_commands brings: every stream's commands of one push, found by the protocol machine on the GPU.
    cmd: fsm.FRAME_DTYPE records of ALL streams, stream k's are cmd[cmd_off[k]:cmd_off[k + 1]] in stream order (both directions merged);
    data / enc: the plaintext bytes and, inside a CRYPTO1 session, the on-air entries (byte | 0x100 where the parity bit equals the data
    parity), stream k's part data[cbyte_off[k]:cbyte_off[k + 1]], a record's byte_off relative to it; every frame owns a slot of its raw
    n_bytes entries in both, zero where nothing was written.  src: type << 31 | index among the stream's raw frames of that type.
    raw: the NfcMultiFrames of the same push.  stream_flags: NFC_FSM_LOST / NFC_FSM_UID_OVERFLOW per stream."""

    def __init__(self, c, copy=True):
        from .fsm import FRAME_DTYPE
        K = int(c.n_streams)
        self.n_streams, self.n_launches, self.bytes_copied = K, int(c.n_launches), int(c.bytes_copied)
        self.ms_kernels, self.ms_machine = float(c.ms_kernels), float(c.ms_machine)

        def arr(ptr, n, dtype):
            dtype = np.dtype(dtype)
            if not ptr or not n:
                return np.zeros(0, dtype)
            a = np.frombuffer((C.c_char * (int(n) * dtype.itemsize)).from_address(ptr), dtype)
            return a.copy() if copy else a

        self.raw = NfcMultiFrames(c.raw, copy)
        self.cmd_off, self.cbyte_off = arr(c.cmd_off, K + 1, '<u8'), arr(c.cbyte_off, K + 1, '<u8')
        self.cmd = arr(c.cmd, self.cmd_off[K], FRAME_DTYPE)
        self.src = arr(c.src, self.cmd_off[K], '<u4')
        self.data = arr(c.data, self.cbyte_off[K], np.uint8)
        self.enc = arr(c.enc, self.cbyte_off[K], '<u2')
        self.stream_flags = arr(c.stream_flags, K, '<u4')

    def commands_of(self, k):
        """Stream k's (table, data, enc) as numpy views: what fsm.dispatch takes."""
        a, b = int(self.cbyte_off[k]), int(self.cbyte_off[k + 1])
        return self.cmd[int(self.cmd_off[k]):int(self.cmd_off[k + 1])], self.data[a:b], self.enc[a:b]

    def src_of(self, k):
        """Per command of stream k: (type, index among the stream's raw frames of that type)."""
        s = self.src[int(self.cmd_off[k]):int(self.cmd_off[k + 1])]
        return (s >> 31).astype(np.int64), (s & 0x7FFFFFFF).astype(np.int64)

    def stream_of(self):
        """The stream every command of cmd belongs to."""
        return np.repeat(np.arange(self.n_streams, dtype=np.int64), np.diff(self.cmd_off).astype(np.int64))

    def cmd_mask(self, index):
        """Over ALL commands: true where the command is `index` (an index of the command table, or NFC_CMD_*)."""
        return self.cmd['cmd'] == int(index)

    def plain_crc_ok_mask(self):
        """Over ALL commands: true where the command's definition carries a CRC_A.  A command is only found when its CRC matches -- inside
        a session: the CRC of the PLAINTEXT -- so no byte is touched."""
        return (self.cmd['cmd'] >= 0) & (self.cmd['n_crc'] == 2)


class NfcCommands(object):
    """What nfc_read_commands brings: one batch's commands of a single context, found by the protocol machine on the GPU.
    table: fsm.FRAME_DTYPE records, both directions merged by idx; data / enc: the plaintext bytes and, inside a CRYPTO1 session, the
    on-air entries (byte | 0x100 where the parity bit equals the data parity), indexed by a record's byte_off; every frame owns a slot
    of its raw n_bytes entries in both.  flags: NFC_FSM_LOST / NFC_FSM_UID_OVERFLOW of the machine behind the batch.  The counters
    (n_segments, n_rerun_segments, n_rerun_frames, n_keydep_segments) say how the batch was spread over lanes.
    ``fsm.dispatch(*c.commands())`` prints the reference's trace."""

    def __init__(self, c, copy=True):
        from .fsm import FRAME_DTYPE
        n, nb = int(c.n_commands), int(c.n_bytes)
        self.n_commands, self.n_bytes, self.flags = n, nb, int(c.flags)
        self.n_launches, self.bytes_copied = int(c.n_launches), int(c.bytes_copied)
        self.ms_kernels, self.ms_frames, self.ms_merge = float(c.ms_kernels), float(c.ms_frames), float(c.ms_merge)
        self.ms_walk, self.ms_resolve = float(c.ms_walk), float(c.ms_resolve)
        self.counters = {k: int(getattr(c.counters, k)) for k, _ in _lib.CtxCommandCounters._fields_}
        for k, v in self.counters.items():
            setattr(self, k, v)

        def arr(ptr, count, dtype):
            dtype = np.dtype(dtype)
            if not ptr or not count:
                return np.zeros(0, dtype)
            a = np.frombuffer((C.c_char * (int(count) * dtype.itemsize)).from_address(ptr), dtype)
            return a.copy() if copy else a

        self.table = arr(c.cmd, n, FRAME_DTYPE)
        self._src = arr(c.src, n, '<u4')
        self.data = arr(c.data, nb, np.uint8)
        self.enc = arr(c.enc, nb, '<u2')

    def commands(self):
        """(table, data, enc): what fsm.dispatch takes."""
        return self.table, self.data, self.enc

    def src(self):
        """Per command: (type, index among the batch's raw frames of that type)."""
        return (self._src >> 31).astype(np.int64), (self._src & 0x7FFFFFFF).astype(np.int64)

    def cmd_mask(self, index):
        """True where the command is `index` (an index of the command table, or NFC_CMD_*)."""
        return self.table['cmd'] == int(index)

    def plain_crc_ok_mask(self):
        """True where the command's definition carries a CRC_A: a command is only found when its CRC matches -- inside a session the
        CRC of the PLAINTEXT -- so no byte is touched."""
        return (self.table['cmd'] >= 0) & (self.table['n_crc'] == 2)


def host_frames(table, bits, ptype):
    """The frame kernels' twin on the CPU (nfc_host_frames): the packets `table` (PACKET_DTYPE rows of ONE type) over that type's bit
    array, a byte per bit -> (records, bytes, par)."""
    L = _lib.load()
    t = np.ascontiguousarray(table, PACKET_DTYPE)
    b = np.ascontiguousarray(bits, np.uint8)
    if len(t) and int((t['bit_off'] + t['n_bits']).max()) > b.size:
        raise NfcError('the packets reach behind the bit array')
    cap = int(t['n_bits'].sum()) // 9 + len(t) + 1
    recs, data, par = np.zeros(len(t), RAW_FRAME_DTYPE), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    used = C.c_size_t(0)
    rc = L.nfc_host_frames(t.ctypes.data if len(t) else None, len(t), b.ctypes.data if b.size else None, int(ptype), recs.ctypes.data,
                           data.ctypes.data, par.ctypes.data, cap, C.byref(used))
    if rc != 0:
        raise NfcError('nfc_host_frames status %d' % rc)
    return recs, data[:used.value], par[:used.value]


class DeviceBuffer(object):
    """Input kept resident in HBM (nfc_device_alloc / nfc_device_upload) for NfcContext.push_device."""

    def __init__(self, host_array, device=0, nbytes=None):
        """nbytes: allocate that much (at least the array's size) -- room for a kernel to write into."""
        self.L = _lib.load()
        self.device = device
        a = np.ascontiguousarray(host_array)
        self.nbytes = max(a.nbytes, int(nbytes or 0))
        self.ptr = C.c_void_p()
        if self.L.nfc_device_alloc(device, self.nbytes, C.byref(self.ptr)) != 0:
            raise NfcError('nfc_device_alloc: %s' % self.L.nfc_last_error(None).decode())
        if a.nbytes and self.L.nfc_device_upload(device, self.ptr, a.ctypes.data, a.nbytes) != 0:
            raise NfcError('nfc_device_upload failed')

    def upload(self, host_array):
        """Overwrite the buffer's first bytes with a host array (nfc_device_upload)."""
        a = np.ascontiguousarray(host_array)
        if a.nbytes > self.nbytes:
            raise NfcError('DeviceBuffer.upload: %d bytes do not fit %d' % (a.nbytes, self.nbytes))
        if a.nbytes and self.L.nfc_device_upload(self.device, self.ptr, a.ctypes.data, a.nbytes) != 0:
            raise NfcError('nfc_device_upload failed')

    def download(self, nbytes=None):
        """The buffer's first nbytes (default: all) as a uint8 array (nfc_device_download)."""
        n = self.nbytes if nbytes is None else int(nbytes)
        out = np.zeros(n, np.uint8)
        if n and self.L.nfc_device_download(self.device, out.ctypes.data, self.ptr, n) != 0:
            raise NfcError('nfc_device_download failed')
        return out

    def free(self):
        if getattr(self, 'ptr', None):
            self.L.nfc_device_free(self.device, self.ptr)
            self.ptr = None

    __del__ = free


class PinnedArray(object):
    """A numpy array over pinned host memory (nfc_host_alloc_pinned): the copy engine reads and writes it directly."""

    def __init__(self, count, dtype):
        self.L = _lib.load()
        self.ptr = C.c_void_p()
        dt = np.dtype(dtype)
        nbytes = max(16, int(count) * dt.itemsize)
        if self.L.nfc_host_alloc_pinned(nbytes, C.byref(self.ptr)) != 0:
            raise NfcError('nfc_host_alloc_pinned failed')
        self.array = np.frombuffer((C.c_char * nbytes).from_address(self.ptr.value), dtype=dt, count=int(count))

    def free(self):
        if getattr(self, 'ptr', None):
            self.array = None
            self.L.nfc_host_free_pinned(self.ptr)
            self.ptr = None

    __del__ = free


def device_count():
    """HIP devices this process sees (nfc_device_count; 0 without a GPU)."""
    return int(_lib.load().nfc_device_count())


def host_i16_to_float(v, i16_scale=0.0):
    """int16 -> float32 as the kernels convert it (threshold.hip.h: i16_to_float): 0 -> fl(v / 32767), > 0 -> fl(v * i16_scale)."""
    v = np.asarray(v).astype(np.float32)
    if i16_scale > 0:
        return v * np.float32(i16_scale)
    return v / np.float32(32767.0)   # (IEEE float32 division: what the kernels' fma form equals for every int16)


def host_iq8_to_float(v, kind, scale=0.0):
    """Complex 8-bit -> float32, I and Q each, as nfc_amd.h defines it: sc8 fl(q * s), cu8 fl((u - 127.5) * s) (u - 127.5 is exact);
    s = scale where it is positive, else 2^-7."""
    s = np.float32(scale if scale > 0 else 2.0 ** -7)
    if kind == NFC_IN_IQ_I8:
        return np.asarray(v).astype(np.int8).astype(np.float32) * s
    u = np.asarray(v).astype(np.uint8).astype(np.float32)
    return (u - np.float32(127.5)) * s


def host_envelope(x, kind, i16_scale=0.0):
    """The envelope the kernels compute from a host array of input kind `kind`, as a numpy float32 copy (one value per sample):
    fl(fl(I*I) + fl(Q*Q)) for the IQ kinds -- complex int16 after converting I and Q as the PCM kind converts a sample, complex
    8-bit after host_iq8_to_float --, fl(s*s) for the real kinds, the samples themselves for the envelope kind.  What a time
    shard's carrier level (sharding.carrier_level) is computed from."""
    dt, per = _KIND_DTYPE[kind]
    a = np.asarray(x)
    if a.dtype == np.complex64 and per == 2:
        a = a.view(np.float32)
    a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
    if kind == NFC_IN_ENV_F32:
        return a.copy()
    if kind in (NFC_IN_I16_SQ, NFC_IN_IQ_I16):
        a = host_i16_to_float(a, i16_scale)
    if kind in (NFC_IN_IQ_I8, NFC_IN_IQ_U8):
        a = host_iq8_to_float(a, kind, i16_scale)
    if per == 1:
        return a * a
    i, q = a[0::2], a[1::2]
    return (i * i) + (q * q)


def host_record_pcm16(x, gain=32767.0):
    """float32 -> int16 PCM as the recording kernel converts it (nfc_amd.h, csrc/record.hip.h: pcm16_of): v = fl(x * gain), NaN -> 0,
    clamp to [-32767, 32767], round to nearest with halves away from zero.  The numpy twin of nfc_host_record_pcm16."""
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.asarray(x, dtype=np.float32) * np.float32(gain)
    v = np.where(np.isnan(v), np.float32(0), v)
    v = np.clip(v, np.float32(-32767), np.float32(32767))
    t = np.trunc(v)
    t = np.where(np.abs(v - t) >= np.float32(0.5), t + np.copysign(np.float32(1), v), t)   # (v - t is exact)
    return t.astype(np.int16)


def _as_pointer(p):
    """A DeviceBuffer, a ctypes pointer (DeviceBuffer.ptr, a stream of nfc_stream_create), an integer address or None -> c_void_p."""
    if isinstance(p, DeviceBuffer):
        return p.ptr
    if isinstance(p, C.c_void_p):
        return p
    return C.c_void_p(int(p or 0))


def record_pcm16_device(dev_ptr, n, out_ptr, kind, i16_scale=0.0, gain=32767.0, tap=NFC_REC_ENVELOPE, device=0, stream=None,
                        timed=False):
    """n samples of input kind `kind` at dev_ptr (device memory) -> n int16 PCM at out_ptr (device memory), both 16-byte aligned
    (nfc_record_pcm16_device).  tap: NFC_REC_ENVELOPE, the envelope the threshold kernels compute for the kind and i16_scale, or
    NFC_REC_REAL_PART, the real part of complex64.  stream: None, or an integer hipStream_t (the work is then only enqueued).
    -> the kernel's duration in ms when timed, else None."""
    L = _lib.load()
    src, dst, st = _as_pointer(dev_ptr), _as_pointer(out_ptr), _as_pointer(stream)
    ms = C.c_float(0)
    rc = L.nfc_record_pcm16_device(int(device), int(tap), int(kind), float(i16_scale), src, int(n), float(gain), dst, st,
                                   C.byref(ms) if timed else None)
    if rc != 0:
        raise NfcError('nfc_record_pcm16_device: %s (status %d)' % (L.nfc_last_error(None).decode(), rc))
    return float(ms.value) if timed else None


def record_pcm16(x, kind, i16_scale=0.0, gain=32767.0, tap=NFC_REC_ENVELOPE, device=0):
    """Upload a host array of input kind `kind`, convert it on the GPU, download: the int16 PCM, one value per sample."""
    dt, per = _KIND_DTYPE[kind]
    a = np.asarray(x)
    if a.dtype == np.complex64 and per == 2:
        a = a.view(np.float32)
    a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
    n = a.size // per
    if n == 0:
        return np.zeros(0, np.int16)
    src = DeviceBuffer(a[:n * per], device)
    dst = DeviceBuffer(np.zeros(0, np.int16), device, nbytes=2 * n)
    try:
        record_pcm16_device(src, n, dst, kind, i16_scale, gain, tap, device)
        return dst.download(2 * n).view(np.int16)
    finally:
        src.free()
        dst.free()


def host_decode_lut(ptype, cur, d, samp_rate=2e6, max_len=50):
    """Drive the decode kernels' duration LUTs sequentially on the host (no GPU)."""
    L = _lib.load()
    p = _params(samp_rate, 0.1, 1.1, 2000, max_len, True, True, NFC_IN_IQ_F32, 0, 0.0, 0, 0)
    cur = np.ascontiguousarray(cur, np.int8)
    d = np.ascontiguousarray(d, np.int32)
    out = np.zeros(2 * len(cur) + 1, np.uint8)
    got = C.c_size_t(0)
    rc = L.nfc_host_decode_lut(C.byref(p), ptype, cur.ctypes.data, d.ctypes.data, len(cur), out.ctypes.data, out.size,
                               C.byref(got))
    if rc != 0:
        raise NfcError('nfc_host_decode_lut status %d' % rc)
    return out[:got.value]
