"""The state a push CARRIES, compared with the reference's (oracle.c_oracle.COracle.state), field by field and bit for bit.

Shared by tests/test_carried_state.py (GPU) and tests/test_carried_state_host.py (the helper's own checks, on plain data)."""
import ctypes as C
import struct

import numpy as np


def ring_in_reference_order(ring, n_seen_at_slot0=0):
    """nfc_get_state's ring in the order of the reference's _buffer.  include/nfc_amd.h: ring[i] is the slot the samples with stream
    index = i (mod av_window) land on; the reference's _buffer[i] takes the samples with index = i (mod av_window) of a stream counted
    from 0 (transition_sink.py:109-125 fills slots 0 .. av_window - 1 in order, then _index starts at 0) -- the same order, so for a
    stream that began at index 0 the rotation is by nothing.  n_seen_at_slot0: the stream index the reference counted as 0."""
    ring = np.asarray(ring)
    return np.roll(ring, -(int(n_seen_at_slot0) % len(ring))) if len(ring) else ring


def last_low_of_trace(trace, first_index):
    """The stream index of the last sample the reference classified LOW (val -1), or -1.  trace: the oracle's per-sample tap from the
    stream's first STABLE sample on (COracle(trace=True), never cleared), first_index: that sample's stream index (av_window)."""
    at = np.flatnonzero(np.asarray(trace) == -1)
    return int(first_index + at[-1]) if len(at) else -1


def remembered_low(n_seen, cur_state, last_bit, dur):
    """What (cur_state, last_bit, dur) still say about the last LOW sample (csrc/host_threshold.h: thr_prepare's nl0 / kl0): its
    stream index while the reference is inside a LOW run (last_bit -1: the sample just seen) or right behind one (cur_state 2: dur
    samples back); None once a time-out has reset the state (transition_sink.py:95-99)."""
    if last_bit == -1:
        return n_seen - 1
    if cur_state == 2:
        return n_seen - dur - 1
    return None


def assert_state_is_the_references(ctx_or_stream, oracle, where, n_seen_at_slot0=0):
    """The carried state of an NfcContext (or an NfcMultiStream) against the oracle's after the same samples.

    ctx_or_stream: anything with get_state() -> (header, ring float32[av_window], [pending bits type 0, type 1]).
    oracle: a COracle(trace=True) that was pushed the same samples and whose trace was never cleared.
    where: names the case and the push in every message.

    Equal: n_seen, filled, stable, cur_state, last_bit, dur, n_pending_bits; ss on its 8 bytes (struct.pack('<d')); the ring as
    float32 bit patterns, slot by slot (the oracle's doubles all came from float32 samples, so the conversion back is exact); the
    pending bits of both types.

    last_low: include/nfc_amd.h documents it as NOT carried (always -1): what a successor needs of the last LOW sample follows from
    cur_state, last_bit and dur.  So the header's -1 is asserted, and the index those three fields imply (remembered_low) is compared
    with the last index of val -1 in the oracle's trace wherever the reference still remembers a LOW sample.

    Left out: miller_state and manch_state.  The short-batch stage stores a class representative of the Miller decoder's state
    (csrc/small.hip.h: canon -- states no later edge can tell apart share one code), which the reference has no name for; the open
    packets' bits and every emitted symbol, which those words determine together with the edges to come, are compared instead."""
    h, ring, pend = ctx_or_stream.get_state()
    s = oracle.state()
    for name, got, want in (('n_seen', h.n_seen, s['nseen']), ('filled', h.filled, s['filled']), ('stable', h.stable, s['stable']),
                            ('cur_state', h.cur_state, s['state']), ('last_bit', h.last_bit, s['last_bit']), ('dur', h.dur, s['dur']),
                            ('n_pending_bits[0]', h.n_pending_bits[0], len(s['open_bits'][0])),
                            ('n_pending_bits[1]', h.n_pending_bits[1], len(s['open_bits'][1]))):
        assert int(got) == int(want), '%s: %s is %d, the reference has %d' % (where, name, int(got), int(want))
    assert struct.pack('<d', h.ss) == struct.pack('<d', s['total']), '%s: ss is %s, the reference\'s _sum is %s (%+d units in the last place)' % (
        where, float(h.ss).hex(), s['total'].hex(), struct.unpack('<q', struct.pack('<d', h.ss))[0] - struct.unpack('<q', struct.pack('<d', s['total']))[0])
    want_ring = s['ring'].astype(np.float32)
    assert np.array_equal(want_ring.astype(np.float64), s['ring']), '%s: the reference\'s ring holds a value that is no float32' % where
    got_ring = ring_in_reference_order(np.ascontiguousarray(ring, np.float32), n_seen_at_slot0)
    assert len(got_ring) == len(want_ring), '%s: ring of %d slots, the reference has %d' % (where, len(got_ring), len(want_ring))
    bad = np.flatnonzero(got_ring.view(np.uint32) != want_ring.view(np.uint32))
    assert len(bad) == 0, '%s: ring differs in %d slots, first slot %d: %s, the reference has %s' % (
        where, len(bad), bad[0], float(got_ring[bad[0]]).hex(), float(want_ring[bad[0]]).hex())
    for t in (0, 1):
        assert np.asarray(pend[t]).tolist() == s['open_bits'][t].tolist(), '%s: pending bits of type %d are %s, the reference has %s' % (
            where, t, np.asarray(pend[t]).tolist(), s['open_bits'][t].tolist())
    assert int(h.last_low) == -1, '%s: last_low is %d, documented as always -1' % (where, int(h.last_low))
    if s['stable']:
        implied = remembered_low(int(h.n_seen), int(h.cur_state), int(h.last_bit), int(h.dur))
        if implied is not None:
            want_low = last_low_of_trace(oracle.trace(), n_seen_at_slot0 + oracle.av_window)
            assert implied == want_low, '%s: cur_state %d, last_bit %d, dur %d place the last LOW sample at %d, the reference\'s trace at %d' % (
                where, h.cur_state, h.last_bit, h.dur, implied, want_low)


class HostState(object):
    """get_state() over plain values: what the helper's own tests hand it (tests/test_carried_state_host.py)."""

    class Header(C.Structure):
        _fields_ = [('n_seen', C.c_uint64), ('ss', C.c_double), ('last_low', C.c_int64), ('filled', C.c_int32), ('stable', C.c_int32),
                    ('cur_state', C.c_int32), ('last_bit', C.c_int32), ('dur', C.c_int32), ('n_pending_bits', C.c_uint32 * 2)]

    def __init__(self, oracle_state):
        s = oracle_state
        self.h = self.Header(s['nseen'], s['total'], -1, s['filled'], s['stable'], s['state'], s['last_bit'], s['dur'],
                             (C.c_uint32 * 2)(len(s['open_bits'][0]), len(s['open_bits'][1])))
        self.ring = s['ring'].astype(np.float32)
        self.pend = [b.copy() for b in s['open_bits']]

    def get_state(self):
        return self.h, self.ring, self.pend
