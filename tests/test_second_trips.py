"""The frame, command and air kernels where their loops take a SECOND trip (csrc/nfc_frames.hip, csrc/multi_commands.hip.h,
csrc/air.hip.h).  Every one of them is a fixed-size workgroup that walks its input in tiles and carries a running sum from tile to tile,
or a fixed-size grid that strides over the streams; what survives in that form is a carry that is not added, a `prev` read across a tile
edge, a table slot rewritten in place, a tail thread whose range is empty.  The other suites stay below every one of those lines.

THE THRESHOLDS ARE READ, NOT REMEMBERED: constants() takes them out of the source text, and every test asserts from them that its input
crosses the line it is there for, so a later change of a constant turns a test red instead of emptying it.  The CPU half asserts all
of those input conditions on what the C oracle, synth.py and air.sizes give, and pins the air twin to synth.py at the new sizes; the
GPU half pins the kernels.  Every comparison is for equality.

CLOSES WITHOUT BITS (a start bit directly followed by a non-bit: the reference's packets.py:67-79 returns an empty list, which
k_frames_scan drops while it compacts) do occur in these inputs.  The oracles' sinks do not show them (packets.py:96-98: an empty
list never reaches the fsm, and oracle/py_oracle.py's BitSink and the C oracle's packet list leave it out in the same way), so
framing_of() replays the oracles' SYMBOL streams through the reference's PacketProcessor and counts every close.  The crafted capture
over 91 seeds closes 4 277 packets per type; 50 of the tag's are without bits, 47 of them in front of the first tile edge and 3 behind it.
The tiled decoder vectors close 5 840 and 13 097 in their long call, 816 and 8 908 of them without bits, on both sides of the edge for
both types.  The counts are literals below; test_the_inputs_cross_their_lines holds them against the replay."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import py_oracle as po
from tests import test_air
from tests.golden_util import GOLDEN
from tests.test_air_host import REQA, yardstick
from tests.test_commands_host import state_bytes
from tests.test_decode_tiles import Ref
from tests.test_frames import (CUT, SEEDS, assert_frames_equal, check_against_restatement, check_multi, crafted_frames, crafted_iq,
                               crafted_oracle_packets, frames_and_twin, host_frames_of, multi_streams, oracle_packets_of, twin_of_stream)
from usrp_nfc_amd import _lib, air, api, emulate, fsm, synth

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')
F32, I16, I8, U8 = api.NFC_IN_IQ_F32, api.NFC_IN_IQ_I16, api.NFC_IN_IQ_I8, api.NFC_IN_IQ_U8
QUANTISE = {F32: lambda x: x, I16: synth.quantise_sc16, I8: synth.quantise_sc8, U8: synth.quantise_cu8}
ATQA = (synth.TAG, synth.frame_bits([0x44, 0x00]))
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- 0. the thresholds, from the source text --------------------------------------------------------------------------------------------
class Constants(object):
    pass


def _number(text, name, pattern, where):
    m = re.search(pattern, text)
    assert m, '%s: no definition of %s matches %r any more' % (where, name, pattern)
    v = 1
    for g in m.groups():
        v *= int(g)
    return v


def constants():
    def read():
        c = Constants()
        frames = open(os.path.join(CSRC, 'nfc_frames.hip')).read()
        for name in ('FS_THREADS', 'FS_ITEMS', 'FA_THREADS', 'FA_MAX_WG'):
            setattr(c, name, _number(frames, name, r'\b%s\s*=\s*(\d+)\s*[,;]' % name, 'nfc_frames.hip'))
        assert re.search(r'\bFS_TILE\s*=\s*FS_THREADS\s*\*\s*FS_ITEMS\s*;', frames), 'nfc_frames.hip: FS_TILE is no longer FS_THREADS * FS_ITEMS'
        c.FS_TILE = c.FS_THREADS * c.FS_ITEMS
        # what the launches make of them: a wave per stream in k_multi_frames_assemble, FA_MAX_WG workgroups at the most
        assert re.search(r'A\.K\s*\+\s*FA_THREADS\s*/\s*64\s*-\s*1\)\s*/\s*\(FA_THREADS\s*/\s*64\)', frames), 'nfc_frames.hip: launch_multi no longer gives a wave a stream'
        c.FA_GRID_STREAMS = c.FA_MAX_WG * (c.FA_THREADS // 64)
        text = open(os.path.join(CSRC, 'air.hip.h')).read()
        for name in ('BLOCK', 'START_BLOCK', 'RENDER_BLOCK'):
            setattr(c, name, _number(text, name, r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, 'air.hip.h'))
        c.MAX_BITS = _number(text, 'MAX_BITS', r'constexpr\s+uint32_t\s+MAX_BITS\s*=\s*(\d+)\s*\*\s*(\d+)\s*;', 'air.hip.h')
        return c
    return cached('constants', read)


def test_the_thresholds_are_read_from_the_sources():
    c = constants()
    got = {n: getattr(c, n) for n in ('FS_THREADS', 'FS_ITEMS', 'FS_TILE', 'FA_THREADS', 'FA_MAX_WG', 'BLOCK', 'START_BLOCK', 'RENDER_BLOCK', 'MAX_BITS')}
    assert all(isinstance(v, int) and v > 0 for v in got.values()), got
    assert c.FS_THREADS % 64 == 0 and c.FA_THREADS % 64 == 0 and c.BLOCK % 64 == 0 and c.START_BLOCK % 64 == 0 and c.RENDER_BLOCK % 64 == 0
    assert c.MAX_BITS % 9 == 0
    with pytest.raises(AssertionError, match='NO_SUCH_NAME'):   # a pattern that no longer matches fails loudly
        _number('constexpr int BLOCK = 256;', 'NO_SUCH_NAME', r'\bNO_SUCH_NAME\s*=\s*(\d+)', 'a text')


# ---- 1. single context: more than a tile of closes per type ---------------------------------------------------------------------------
N_SEEDS = 91   # settled with the oracle: what a batch closes per type, whole and behind the cut, is asserted below
LONG_SEEDS = tuple(range(SEEDS[0], SEEDS[0] + N_SEEDS))
# per type: the closes of a batch (n_close, what k_frames_scan walks), those with bits (the frames), and the closes without bits in front
# of and behind the first tile edge (their place among the batch's closes)
CRAFTED_WHOLE = dict(closes=(4277, 4277), frames=(4227, 4277), empty_before_edge=(47, 0), empty_behind_edge=(3, 0))
CRAFTED_BEHIND_THE_CUT = dict(closes=(4232, 4231), frames=(4183, 4231), empty_before_edge=(47, 0), empty_behind_edge=(2, 0))


def long_crafted_iq():
    """The crafted capture of tests/test_frames.py over N_SEEDS seeds (not kept in that module's cache: some 60 MB)."""
    iq = synth.iq_from_profile(synth.modulation_profile(crafted_frames(LONG_SEEDS)))
    iq.setflags(write=False)
    return iq


def crafted_cut():
    """A complex-sample position inside the first seed's 40-byte reader frame: (cut, where that frame starts, where it ends)."""
    frames = crafted_frames(LONG_SEEDS[:1])
    i = max(j for j, (d, b) in enumerate(frames) if d == synth.READER and len(b) == 360)
    start = len(synth.modulation_profile(frames[:i], tail=0))
    return start + 2001, start, start + len(synth.modulation_profile(frames[i:i + 1], gap_us=0.0, lead_in=0, tail=0))


def framing_of(symbol_pushes):
    """Consecutive batches of one stream, each the two types' symbol streams (what the decoders hand to append_bit), through the
    reference's PacketProcessor as oracle/py_oracle.py restates it: per batch and type the bit count of EVERY close, 0 for a close
    without bits."""
    procs, out = [po.PacketProcessor(0), po.PacketProcessor(1)], []
    for symbols in symbol_pushes:
        row = []
        for t in (0, 1):
            done = [procs[t].append_bit(b) for b in np.asarray(symbols[t]).tolist()]
            row.append(np.array([len(d) for d in done if d is not None], np.int64))
        out.append(row)
    return out


def batch_summary(lengths, c):
    """framing_of's row of one batch in the form of the literals above"""
    empty = [np.nonzero(a == 0)[0] for a in lengths]
    return dict(closes=tuple(len(a) for a in lengths), frames=tuple(int((a > 0).sum()) for a in lengths),
                empty_before_edge=tuple(int((e < c.FS_TILE).sum()) for e in empty), empty_behind_edge=tuple(int((e >= c.FS_TILE).sum()) for e in empty))


def _oracle_pushes(parts):
    """Consecutive pushes of one stream through the C oracle: per push its packets [(type, bits), ...] and its symbols per type."""
    o = co.COracle(hi_val=1.1)
    try:
        out = []
        for p in parts:
            o.clear_outputs()
            o.push_iq(p)
            out.append((o.packets(), [o.symbols(0), o.symbols(1)]))
        return out
    finally:
        o.close()


def long_crafted_oracle():
    """-> dict(whole: the packets of the capture in one push, pieces: those of its two pieces; whole_closes, pieces_closes: framing_of
    their symbols)"""
    def make():
        iq, (cut, _, _) = long_crafted_iq(), crafted_cut()
        whole, pieces = _oracle_pushes([iq]), _oracle_pushes([iq[:2 * cut], iq[2 * cut:]])
        return dict(whole=whole[0][0], pieces=[p for p, _ in pieces], n=len(iq) // 2, whole_closes=framing_of([whole[0][1]])[0],
                    pieces_closes=framing_of([s for _, s in pieces]))
    return cached('long', make)


def frames_per_type(packets):
    """[(type, bits), ...] as the oracles' sinks list them -> the packets per type"""
    return [sum(1 for t, _ in packets if t == ty) for ty in (0, 1)]


def assert_second_scan_trip(batch, c):
    """what makes a batch (one of the literals' form) take k_frames_scan and k_frames_assemble past their first trips, with a ragged
    last tile and closes without bits to drop on both sides of the tile edge"""
    n_close, n_frames = batch['closes'], batch['frames']
    assert min(n_close) > c.FS_TILE, 'every type: a second tile of closes (the run carry, prev across the tile edge, wave_sum reused)'
    assert min(n_frames) > c.FS_TILE, 'every type: the carried frame count moves the records of the second tile'
    assert any(n % c.FS_ITEMS for n in n_close), 'a last thread with fewer than FS_ITEMS closes'
    assert any(n % c.FS_TILE < c.FS_TILE - c.FS_THREADS for n in n_close), 'tail threads without a close'
    assert min(n_frames) > c.FA_THREADS, 'workgroup 1 of k_frames_assemble runs for both types'
    assert any(a > 0 and b > 0 for a, b in zip(batch['empty_before_edge'], batch['empty_behind_edge'])), 'closes without bits on each side of the first tile edge'


# ---- the decoder vectors through nfc_push_edges ----
EDGE_REPS = 69
EDGE_FRAMES_PER_REP = (73, 61)        # one repetition: the random vector (13 and 1) and the frame vector (60 and 60)
# the two calls: the first ends inside the first whole reader frame; and the rest
EDGE_BATCHES = (dict(closes=(25, 151), frames=(13, 20), empty_before_edge=(12, 131), empty_behind_edge=(0, 0)),
                dict(closes=(5840, 13097), frames=(5024, 4189), empty_before_edge=(576, 2774), empty_behind_edge=(240, 6134)))


def _edge_rows(z, tagname):
    parts = []
    for t, c in ((1, 'm'), (0, 't')):
        d = z['d' + c + '_' + tagname] if 'd' + c + '_' + tagname in z else z['d_' + tagname]
        e = np.zeros(len(d), _lib.EDGE_DTYPE)
        e['v'], e['d'], e['t'] = z['cur' + c + '_' + tagname], d, t
        parts.append(e)
    return np.concatenate(parts)


def edge_repetition():
    """The 6 000 random (cur, d) pairs per route, every error branch among them, and the whole frames behind them: at 2 Msps."""
    z = np.load(os.path.join(GOLDEN, 'fx_decoder_vectors.npz'))
    return np.concatenate([_edge_rows(z, '0p5'), _edge_rows(z, 'frames_0p5')])


def edge_cut():
    """where the first of the two calls ends: a third into the reader's whole frames of the first repetition"""
    z = np.load(os.path.join(GOLDEN, 'fx_decoder_vectors.npz'))
    return len(_edge_rows(z, '0p5')) + len(z['dm_frames_0p5']) // 3


def tiled_edges():
    e = np.tile(edge_repetition(), EDGE_REPS)
    e['idx'] = np.arange(len(e), dtype=np.uint64) * 2 + 5   # fresh, ascending
    return e, edge_cut()


# ---- 2. the multi-stream captures -----------------------------------------------------------------------------------------------------
LEAD_IN = 2100   # (300 would keep a capture shorter, but does not fill the averaging window: the lone REQA then decodes to nothing)


def short_captures():
    """Eight distinct short fc32 captures: -> [(name, iq)]"""
    def make():
        txn = synth.ULTRALIGHT_TXN
        fb = lambda i: (txn[i][0], synth.frame_bits(txn[i][2], txn[i][3]))
        bad = list(txn[4][2])
        bad[-1] ^= 0x10   # SEL1R with a CRC_A that does not match
        iq = lambda frames: synth.iq_from_profile(synth.modulation_profile(frames, lead_in=LEAD_IN))
        caps = [('nothing', np.zeros(0, np.float32)),
                ('carrier', synth.iq_from_profile(np.ones(2500, np.float32))),
                ('reqa', iq([fb(0)])),
                ('reqa_atqa', iq([fb(0), fb(1)])),
                ('reader_only', iq([fb(i) for i in (0, 2, 4, 6)])),
                ('tag_only', iq([fb(i) for i in (1, 3, 5, 7)])),
                ('five_frames', iq([fb(i) for i in (0, 1, 2, 3, 10)])),
                ('bad_crc', iq([(synth.READER, synth.frame_bits(bad)), fb(5), fb(18)]))]
        for _, a in caps:
            a.setflags(write=False)
        return caps
    return cached('captures', make)


NOTHING, CARRIER, READER_ONLY, TAG_ONLY, BAD_CRC = 0, 1, 4, 5, 7


class Expected(object):
    """What one stream gives for one push, from the reference side alone: frames (an api.NfcFrames whose idx is the closing edge's sample
    index in the stream), its commands (table, data, enc), the machine's state afterwards, the closes (all, without bits) per type."""


def expected_pushes(parts):
    """Consecutive pushes `parts` of ONE stream -> [Expected per push].  The packets are the C oracle's; the closing indices come from
    the reference's decoders and framing as oracle/py_oracle.py restates them, driven edge by edge over the C oracle's edges (and must
    give the same packets); the frames are the host twin's, checked against the numpy restatement of the reference's fsm.py; the
    commands are the host machine's, its state carried from push to push."""
    o, ref, state, out = co.COracle(hi_val=1.1), None, fsm.state_init(), []
    try:
        for p in parts:
            o.clear_outputs()
            o.push_iq(p)
            packets, e = o.packets(), o.edges()
            rows = np.zeros(len(e), _lib.EDGE_DTYPE)
            rows['d'], rows['v'], rows['t'], rows['idx'] = e['d'], e['v'], e['t'], e['idx']
            if ref is None:
                ref = Ref(rows[:0])
            n0 = len(ref.sink.packets)
            ref.feed(rows)
            assert [(t, b) for t, b in ref.sink.packets[n0:]] == packets, 'the two oracles disagree on the packets'
            closing = [int(rows['idx'][i - (ref.n - len(rows))]) for i in ref.closed_by[n0:]]
            x = Expected()
            x.n_frames = frames_per_type(packets)
            kept = [(t, b, i) for (t, b), i in zip(packets, closing) if b]
            frames, tabs, bits = host_frames_of([(t, b) for t, b, _ in kept])
            check_against_restatement(frames, tabs, bits)
            for t in (0, 1):
                frames.records[t]['idx'] = [i for ty, _, i in kept if ty == t]
            x.frames = api.NfcFrames(frames.records, frames.bytes, frames.par)
            assert x.frames.table['idx'].tolist() == [i for _, _, i in kept], 'stream order'
            x.commands = fsm.host_commands(state, x.frames)
            x.state = state_bytes(state)
            out.append(x)
        return out
    finally:
        o.close()


def expected_of(a, b=None):
    """capture a alone in a fresh stream (b None), or capture b in the stream that took capture a before"""
    caps = short_captures()
    if b is None:
        return cached(('exp', a), lambda: expected_pushes([caps[a][1]])[0])
    return cached(('exp', a, b), lambda: expected_pushes([caps[a][1], caps[b][1]])[1])


def multi_sizes(c):
    """K of the two cases, from the constants: one stream more than the scan has threads; and eight streams more than the assembly's
    grid has waves, which is no multiple of the streams a scan thread then owns and leaves the scan's tail threads nothing."""
    K1 = c.FS_THREADS + 1
    K2 = c.FA_GRID_STREAMS + 8
    return K1, K2


def draw_which(K, c):
    rng = np.random.Generator(np.random.PCG64(K))
    which = rng.integers(0, len(short_captures()), K)
    pins = [0, K - 1] + ([c.FA_GRID_STREAMS] if K > c.FA_GRID_STREAMS else [])
    for j, k in enumerate(pins):
        which[k] = (READER_ONLY, BAD_CRC, TAG_ONLY)[j]
    return which


def assert_multi_crosses(K, which, c, first_push=True):
    per = -(-K // c.FS_THREADS)
    assert K > c.FS_THREADS and per >= 2, 'a scan thread owns consecutive streams and rewrites their slots in place'
    busy = -(-K // per)
    assert busy < c.FS_THREADS, 'thread FS_THREADS - 1 writes the totals from an empty range'
    if K > 2 * c.FS_THREADS:
        assert K > c.FA_GRID_STREAMS and K % per != 0 and c.FS_THREADS - busy >= 64, 'grid-stride second trip; a ragged last thread; idle waves'
        assert K - c.FA_GRID_STREAMS == 8
    nf = np.array([[len(expected_of(w).frames.records[t]) for t in (0, 1)] for w in range(len(short_captures()))])
    assert len({tuple(r) for r in nf.tolist()}) >= 6 and (nf[READER_ONLY] == [0, 4]).all() and (nf[TAG_ONLY] == [4, 0]).all(), 'the types\' tables differ'
    if first_push:
        pins = [0, K - 1] + ([c.FA_GRID_STREAMS] if K > c.FA_GRID_STREAMS else [])
        assert all(nf[which[k]].sum() > 0 for k in pins)
    sums = nf[which, 0][:busy * per - per].reshape(-1, per).sum(axis=1)
    assert len(set(sums.tolist())) >= 4, 'the sums the scan threads form differ from thread to thread'


def gather(per_capture, which, dtype):
    parts = [per_capture[w] for w in which.tolist()]
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def offsets(counts, which):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.uint64)[which])]).astype(np.uint64)


def assert_multi_frames(fr, exp, which):
    """fr: an api.NfcMultiFrames; exp[j]: the Expected of pushes[j]; which[k]: the j of stream k"""
    K = len(which)
    for t in (0, 1):
        frame_off = offsets([len(x.frames.records[t]) for x in exp], which)
        byte_off = offsets([len(x.frames.bytes[t]) for x in exp], which)
        assert fr.frame_off[t].tobytes() == frame_off.tobytes(), 'frame_off of type %d: first wrong entry %d' % (t, _first(fr.frame_off[t], frame_off))
        assert fr.byte_off[t].tobytes() == byte_off.tobytes(), 'byte_off of type %d: first wrong entry %d' % (t, _first(fr.byte_off[t], byte_off))
        assert len(fr.frames[t]) == int(frame_off[K]) and len(fr.bytes[t]) == len(fr.par[t]) == int(byte_off[K])   # the totals the call reports
        want = gather([x.frames.records[t] for x in exp], which, _lib.RAW_FRAME_DTYPE)
        assert fr.frames[t].tobytes() == want.tobytes(), 'records of type %d: stream %d' % (t, _stream_of(fr.frames[t], want, frame_off))
        want = gather([x.frames.bytes[t] for x in exp], which, np.uint8)
        assert fr.bytes[t].tobytes() == want.tobytes(), 'bytes of type %d: stream %d' % (t, _stream_of(fr.bytes[t], want, byte_off))
        want = gather([x.frames.par[t] for x in exp], which, np.uint8)
        assert fr.par[t].tobytes() == want.tobytes(), 'ninth bits of type %d: stream %d' % (t, _stream_of(fr.par[t], want, byte_off))
        mask = gather([(x.frames.records[t]['flags'] & _lib.NFC_RAW_CRC_A_OK) != 0 for x in exp], which, bool)
        assert fr.crc_ok_mask()[t].tolist() == mask.tolist()
    for k in range(K):   # ... which is, stream by stream, what the accessor hands out
        got, want = fr.frames_of(k), exp[which[k]].frames
        for t in (0, 1):
            assert got.records[t].tobytes() == want.records[t].tobytes() and got.bytes[t].tobytes() == want.bytes[t].tobytes(), (k, t)
            assert got.par[t].tobytes() == want.par[t].tobytes(), (k, t)


def _first(got, want):
    n = min(len(got), len(want))
    d = np.nonzero(np.asarray(got[:n]) != np.asarray(want[:n]))[0]
    return int(d[0]) if len(d) else n


def _stream_of(got, want, off):
    return int(np.searchsorted(off, _first(got, want), side='right')) - 1


def assert_multi_commands(cm, exp, which):
    K = len(which)
    cmd_off = offsets([len(x.commands[0]) for x in exp], which)
    cbyte_off = offsets([len(x.commands[1]) for x in exp], which)
    assert cm.cmd_off.tobytes() == cmd_off.tobytes(), 'cmd_off: first wrong entry %d' % _first(cm.cmd_off, cmd_off)
    assert cm.cbyte_off.tobytes() == cbyte_off.tobytes(), 'cbyte_off: first wrong entry %d' % _first(cm.cbyte_off, cbyte_off)
    for i, (name, dtype) in enumerate((('cmd', fsm.FRAME_DTYPE), ('data', np.uint8), ('enc', np.uint16))):
        want = gather([x.commands[i] for x in exp], which, dtype)
        got = getattr(cm, name)
        assert got.tobytes() == want.tobytes(), '%s: stream %d' % (name, _stream_of(got, want, cmd_off if i == 0 else cbyte_off))
    for k in range(K):
        for a, b in zip(cm.commands_of(k), exp[which[k]].commands):
            assert a.tobytes() == b.tobytes(), k
    assert cm.stream_flags.tolist() == [0] * K


def state_sample(K, c):
    """some 64 streams whose machine state is read back, a device call each: the ends, the scan's thread and the grid's edges, and a draw"""
    rng = np.random.Generator(np.random.PCG64(64))
    fixed = [0, 1, 2, K - 2, K - 1, c.FS_THREADS - 1, c.FS_THREADS] + [k for k in (c.FA_GRID_STREAMS - 1, c.FA_GRID_STREAMS, c.FA_GRID_STREAMS + 1) if k < K]
    return sorted(set(fixed + rng.integers(0, K, 54).tolist()))


# ---- 3. a stream with more than 64 stored frames of a type ------------------------------------------------------------------------------
def long_stream_cap_bits():
    """cap_packet_bits that cuts the whole crafted capture, as ONE stream, inside its third group of 64 frames of either type -- and
    the per-type index of the first frame it cuts"""
    ends = [np.cumsum(host_frames_of(crafted_oracle_packets())[0].records[t]['n_bits'].astype(np.int64)) for t in (0, 1)]
    cap = int(max(ends[0][150], ends[1][150]))
    return cap, [int(np.nonzero(e > cap)[0][0]) for e in ends], [len(e) for e in ends]


# ---- 4. the air kernels -------------------------------------------------------------------------------------------------------------------
READT = test_air.READT
AIR_LISTS = ([], REQA, REQA + [ATQA], READT)


def short_frame_streams(c):
    """streams of BLOCK - 1, BLOCK, BLOCK + 1 and 2 BLOCK + 1 short frames and one of 3: REQA, ATQA and one-byte frames of varying
    values, both directions"""
    def make():
        rng = np.random.Generator(np.random.PCG64(255))
        streams = []
        for n in (c.BLOCK - 1, c.BLOCK, c.BLOCK + 1, 2 * c.BLOCK + 1, 3):
            frames = []
            for i in range(n):
                pick = int(rng.integers(0, 4))
                frames.append(REQA[0] if pick == 0 else ATQA if pick == 1 else (synth.READER if pick == 2 else synth.TAG, synth.frame_bits([int(rng.integers(0, 256))])))
            streams.append(frames)
        return streams
    return cached('short_streams', make)


def short_frames_of(c, tail):
    """the AirFrames of short_frame_streams: a small lead-in, 20 idle samples between frames but NONE before every third frame, and
    (tail 0) nothing at all behind a stream's last frame"""
    fr = air.frames_of(short_frame_streams(c), rate_msps=2.0, gap_us=10.0, lead_in=40, tail=tail)
    fr.frames['idle_before'][np.arange(len(fr.frames)) % 3 == 2] = 0
    if tail == 0:
        fr.tail = 0
    return fr


def yardstick_of_stream(fr, streams, k):
    """synth.py's samples of stream k of an AirFrames made from `streams`: every frame behind its own idle_before, then the tail"""
    idle = fr.frames['idle_before'][int(fr.frame_off[k]):int(fr.frame_off[k + 1])].tolist()
    parts = [yardstick([f], rate_msps=fr.rate_msps, gap_us=0.0, lead_in=int(i), tail=0) for f, i in zip(streams[k], idle)]
    parts.append(np.tile(yardstick([])[:2], fr.tail))
    return np.concatenate(parts)


def longest_frames():
    """one frame of 256 bytes in each direction"""
    rng = np.random.Generator(np.random.PCG64(2304))
    return [(synth.READER, synth.frame_bits(rng.integers(0, 256, 256).tolist())), (synth.TAG, synth.frame_bits(rng.integers(0, 256, 256).tolist()))]


def many_air_streams(c):
    """-> (K, which, stream_seeds): START_BLOCK + 6 streams drawn from AIR_LISTS; without a frame: stream 0, stream K - 1 and the five
    around index START_BLOCK.  The seeds are drawn from 0 .. 199, so streams of the same list share a seed on both sides of START_BLOCK."""
    K = c.START_BLOCK + 6
    rng = np.random.Generator(np.random.PCG64(K))
    which = rng.integers(0, len(AIR_LISTS), K)
    which[[0, K - 1] + list(range(c.START_BLOCK - 2, c.START_BLOCK + 3))] = 0
    return K, which, rng.integers(0, 200, K).astype(np.uint64)


def assert_air_streams_cross(K, which, c):
    assert K > c.START_BLOCK, 'k_air_starts takes a second trip'
    assert which[0] == 0 and which[K - 1] == 0 and (which[c.START_BLOCK - 2:c.START_BLOCK + 3] == 0).all(), 'the pinned empty streams'
    assert all((which == j).sum() > 100 for j in range(len(AIR_LISTS)))
    assert (which[:c.START_BLOCK] != 0).any() and (which[c.START_BLOCK:] != 0).any()


def twin_seeds(which, seeds, c):
    """two streams of the same list with the same seed, one on each side of START_BLOCK"""
    for k2 in range(c.START_BLOCK, len(which)):
        for k1 in range(c.START_BLOCK):
            if which[k1] == which[k2] != 0 and seeds[k1] == seeds[k2]:
                return k1, k2
    raise AssertionError('no two streams share list and seed across START_BLOCK')


def air_expected(j):
    """list j of AIR_LISTS as the frames an eavesdropper's decode assembles, and the host machine's commands over them"""
    def make():
        frames = emulate.frames_of_bits(AIR_LISTS[j])
        return frames, fsm.host_commands(fsm.state_init(), frames)
    return cached(('air', j), make)


# ---- CPU suite ------------------------------------------------------------------------------------------------------------------------
def test_the_inputs_cross_their_lines():
    """Every input condition the GPU tests rest on, from the C oracle, synth.py and air.sizes: no GPU."""
    c = constants()
    # 1. the long crafted capture, whole and in its two pieces
    cut, start, end = crafted_cut()
    long = long_crafted_oracle()
    assert 2000 < cut - start < end - cut and 2 * cut < long['n'], 'the cut lies inside a frame'
    assert batch_summary(long['whole_closes'], c) == CRAFTED_WHOLE and tuple(frames_per_type(long['whole'])) == CRAFTED_WHOLE['frames']
    assert_second_scan_trip(CRAFTED_WHOLE, c)
    assert long['pieces'][0] + long['pieces'][1] == long['whole'], 'the pieces give the whole'
    assert batch_summary(long['pieces_closes'][1], c) == CRAFTED_BEHIND_THE_CUT and tuple(frames_per_type(long['pieces'][1])) == CRAFTED_BEHIND_THE_CUT['frames']
    assert_second_scan_trip(CRAFTED_BEHIND_THE_CUT, c)
    assert all(len(a) > 0 for a in long['pieces_closes'][0]), 'the batch behind the cut is not the stream\'s first'
    lens = [len(b) for _, b in long['whole']]
    assert len(set(lens)) > 40 and max(lens) >= 360, 'the frames vary'
    assert long['n'] * 8 < 64 << 20, 'the largest device buffer here'
    # 1b. the decoder vectors: a repetition ends in the state it began in, so every repetition closes what the first one closes
    rep = edge_repetition()
    ref = Ref(rep[:0])
    begin = ref.state()
    for _ in range(2):
        n0 = len(ref.sink.packets)
        ref.feed(rep)
        assert ref.state() == begin
        assert frames_per_type(ref.sink.packets[n0:]) == list(EDGE_FRAMES_PER_REP)
    e, ecut = tiled_edges()
    assert (np.diff(e['idx'].astype(np.int64)) > 0).all() and len(e) == EDGE_REPS * len(rep)
    ref = Ref(e[:ecut])
    assert ref.state()[1][1][0] and len(ref.state()[1][1][1]) > 0, 'the first call ends inside a packet'
    n0, sym0 = len(ref.sink.packets), [list(x) for x in ref.sink.symbols]
    ref.feed(e[ecut:])
    batches = framing_of([sym0, [ref.sink.symbols[t][len(sym0[t]):] for t in (0, 1)]])
    assert [batch_summary(b, c) for b in batches] == list(EDGE_BATCHES)
    assert [tuple(frames_per_type(p)) for p in (ref.sink.packets[:n0], ref.sink.packets[n0:])] == [b['frames'] for b in EDGE_BATCHES]
    assert tuple(EDGE_REPS * n for n in EDGE_FRAMES_PER_REP) == tuple(a + b for a, b in zip(*[b['frames'] for b in EDGE_BATCHES]))
    assert_second_scan_trip(EDGE_BATCHES[1], c)
    # 2. the short captures and the two K
    caps = short_captures()
    assert len(caps) == 8 and len(caps[NOTHING][1]) == 0 and max(len(a) for _, a in caps) // 2 < 6500
    exp = [expected_of(w) for w in range(len(caps))]
    assert [sum(x.n_frames) for x in exp] == [0, 0, 1, 2, 4, 4, 5, 3]
    assert exp[BAD_CRC].frames.crc_ok_mask().tolist() == [False, True, True]
    assert len({tuple(x.frames.table['n_bytes'].tolist()) for x in exp}) == 7   # (no frames, twice)
    K1, K2 = multi_sizes(c)
    for K in (K1, K2):
        which = draw_which(K, c)
        assert_multi_crosses(K, which, c)
        assert_multi_crosses(K, np.roll(which, 1), c, first_push=False)
        pairs = {(int(a), int(b)) for a, b in zip(which, np.roll(which, 1))}
        assert len(pairs) > 40   # the second push: nearly every capture behind nearly every other
    assert (K1, -(-K1 // c.FS_THREADS)) == (c.FS_THREADS + 1, 2) and -(-K2 // c.FS_THREADS) >= 3
    # a stream's second capture decodes as it does in a fresh stream (the frames; the indices move by the first one's length) ...
    two = expected_of(BAD_CRC, READER_ONLY)
    assert two.frames.table['flags'].tolist() == exp[READER_ONLY].frames.table['flags'].tolist()
    assert (two.frames.table['idx'] - exp[READER_ONLY].frames.table['idx']).tolist() == [len(caps[BAD_CRC][1]) // 2] * 4
    differ = [(a, b) for a, b in sorted(pairs) if expected_of(a, b).state != exp[b].state or expected_of(a, b).commands[0].tobytes() != exp[b].commands[0].tobytes()]
    assert len(differ) >= 8   # ... the machine does not: what it makes of a capture depends on the one before
    # 3. the long stream: the slab cut falls inside its third group of 64 frames
    cap, cut_at, n = long_stream_cap_bits()
    assert all(128 <= a < min(192, m) for a, m in zip(cut_at, n)) and min(n) > 128
    ul = [sum(len(b) for t, b in oracle_packets_of(4) if t == ty) for ty in (0, 1)]
    one = [sum(len(b) for t, b in oracle_packets_of(0) if t == ty) for ty in (0, 1)]
    assert max(ul + one) < cap, 'the neighbours fit the slab'
    # 4. the air inputs, from air.sizes
    fr = short_frames_of(c, 400)
    assert np.diff(fr.frame_off).tolist() == [c.BLOCK - 1, c.BLOCK, c.BLOCK + 1, 2 * c.BLOCK + 1, 3]
    assert (fr.frames['idle_before'] == 0).sum() > 400 and set(fr.frames['n_bits'].tolist()) == {7, 9, 18}
    first, n = air.sizes(fr, align_samples=1)
    assert first.tolist() == np.concatenate([[0], np.cumsum(n)[:-1]]).tolist() and (n % 8 != 0).any()
    assert short_frames_of(c, 0).tail == 0
    fr = air.frames_of([longest_frames()])
    assert fr.frames['n_bits'].tolist() == [c.MAX_BITS, c.MAX_BITS] and fr.frames['type'].tolist() == [1, 0]
    K, which, seeds = many_air_streams(c)
    assert_air_streams_cross(K, which, c)
    k1, k2 = twin_seeds(which, seeds, c)
    assert k1 < c.START_BLOCK <= k2
    fr = air.frames_of([AIR_LISTS[j] for j in which])
    for align in (1, 8):
        first, n = air.sizes(fr, out_kind=I8, align_samples=align)
        assert len(n) == K and (first % align == 0).all() and (np.diff(first.astype(np.int64)) >= n[:-1]).all()
        assert len(set(n.tolist())) == len(AIR_LISTS) and int(n[0]) == int(n[K - 1]) == int(n[c.START_BLOCK]) == 300 + 400
    assert int(n.max()) < 7000


@pytest.mark.parametrize('tail', [400, 0])
@pytest.mark.parametrize('align', [1, 8])
def test_air_twin_equals_synth_around_the_layout_trip(align, tail):
    c = constants()
    streams, fr = short_frame_streams(c), short_frames_of(c, tail)
    want = [yardstick_of_stream(fr, streams, k) for k in range(len(streams))]
    first, n = air.sizes(fr, align_samples=align)
    assert n.tolist() == [len(w) // 2 for w in want]
    for kind, q in QUANTISE.items():
        cap = air.host_render(fr, out_kind=kind, sigma=0, align_samples=align)
        assert cap.first_sample.tolist() == air.sizes(fr, out_kind=kind, align_samples=align)[0].tolist()
        for k in range(len(streams)):
            assert np.array_equal(cap.download(k), q(want[k])), (kind, k)


@pytest.mark.parametrize('rate', [2.0, 10.0])
def test_air_twin_equals_synth_on_the_longest_frame(rate):
    frames = longest_frames()
    want = yardstick(frames, rate_msps=rate)
    for kind, q in QUANTISE.items():
        cap = air.host_render([frames], out_kind=kind, sigma=0, rate_msps=rate)
        assert cap.n_samples.tolist() == [len(want) // 2] and np.array_equal(cap.download(0), q(want)), kind


def test_air_twin_equals_synth_on_the_lists_of_the_many_streams():
    for j, frames in enumerate(AIR_LISTS):
        want = yardstick(frames) if frames else np.tile(yardstick([])[:2], 300 + 400)
        for kind, q in QUANTISE.items():
            cap = air.host_render([frames], out_kind=kind, sigma=0)
            assert np.array_equal(cap.download(0), q(want)), (j, kind)


# ---- GPU suite ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def long_iq():
    yield long_crafted_iq()


@pytest.fixture
def ctx():
    c = api.NfcContext(hi_val=1.1, input_kind=F32)
    yield c
    c.close()


def _whole_flags():
    return cached('whole_flags', lambda: host_frames_of([(t, b) for t, b in long_crafted_oracle()['whole'] if b])[0].table['flags'].tolist())


@pytest.mark.gpu
def test_gpu_more_than_a_tile_of_closes_per_type_in_one_push(ctx, long_iq):
    c = constants()
    ctx.push(long_iq)
    got, want, tabs, bits = frames_and_twin(ctx)
    assert (len(tabs[0]), len(tabs[1])) == CRAFTED_WHOLE['frames']   # the capture the CPU half counted the closes of
    assert_second_scan_trip(CRAFTED_WHOLE, c)
    assert_frames_equal(got, want)
    check_against_restatement(got, tabs, bits)
    assert got.table['flags'].tolist() == _whole_flags()


@pytest.mark.gpu
def test_gpu_more_than_a_tile_of_closes_behind_a_cut_inside_a_frame(ctx, long_iq):
    c = constants()
    cut = crafted_cut()[0]
    flags, n_frames = [], []
    for piece in (long_iq[:2 * cut], long_iq[2 * cut:]):
        ctx.push(piece)
        got, want, tabs, bits = frames_and_twin(ctx)
        assert_frames_equal(got, want)
        check_against_restatement(got, tabs, bits)
        flags += got.table['flags'].tolist()
        n_frames.append((len(tabs[0]), len(tabs[1])))
    assert n_frames[1] == CRAFTED_BEHIND_THE_CUT['frames'] and tuple(a + b for a, b in zip(*n_frames)) == CRAFTED_WHOLE['frames']
    assert_second_scan_trip(CRAFTED_BEHIND_THE_CUT, c)   # the batch that starts with carried bits takes the second trip too
    assert flags == _whole_flags()


@pytest.mark.gpu
def test_gpu_push_edges_more_than_a_tile_of_closes_on_the_decoder_vectors():
    """As test_frames.py::test_gpu_push_edges_on_the_decoder_vectors, the random pairs and the whole frames repeated EDGE_REPS times in
    two calls.  Most closes of the random pairs are without bits: in the long call they lie on both sides of the first tile edge, for
    both types (EDGE_BATCHES)."""
    c = constants()
    e, cut = tiled_edges()
    with api.NfcContext(samp_rate=2e6, hi_val=1.1) as cx:
        for piece, batch in zip((e[:cut], e[cut:]), EDGE_BATCHES):
            cx.push_edges(piece)
            got, want, tabs, bits = frames_and_twin(cx)
            assert (len(tabs[0]), len(tabs[1])) == batch['frames']
            assert_frames_equal(got, want)
            check_against_restatement(got, tabs, bits)
    assert_second_scan_trip(EDGE_BATCHES[1], c)


def _hooks_multi(K, max_push, **kw):
    m = api.NfcMultiContext(K, max_push, hi_val=1.1, input_kind=F32, lib_path=_lib.hooks_path(), **kw)
    guards = m.L.nfc_debug_multi_guards
    guards.argtypes = [ctypes.c_void_p]
    return m, guards


def _capture_buffer():
    """the short captures in one array, each at an even sample (16 bytes): -> (array, first sample per capture, samples per capture)"""
    parts, first, n, at = [], [], [], 0
    for _, a in short_captures():
        first.append(at)
        n.append(len(a) // 2)
        parts.append(a)
        if n[-1] % 2:
            parts.append(np.zeros(2, np.float32))
        at += n[-1] + n[-1] % 2
    return np.concatenate(parts), np.array(first, np.uint64), np.array(n, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize('case', [0, 1])
def test_gpu_multi_frames_and_commands_past_the_scan_s_threads_and_the_grid(case):
    c = constants()
    K = multi_sizes(c)[case]
    which = draw_which(K, c)
    assert_multi_crosses(K, which, c)
    host, first, n = _capture_buffer()
    M = len(n)
    buf = api.DeviceBuffer(host)
    m, guards = _hooks_multi(K, int(n.max()))
    try:
        m.track_commands()
        sample = state_sample(K, c)
        # the first push: stream k takes capture which[k]
        exp = [expected_of(w) for w in range(M)]
        m.push_device(buf, first[which], n[which])
        fr, cm = m.fetch_frames(), m.fetch_commands()
        assert guards(m.h) == 0
        assert_multi_frames(fr, exp, which)
        assert_multi_commands(cm, exp, which)
        for k in sample:
            assert state_bytes(m.fsm_state(k)) == exp[which[k]].state, k
        # the second push, rotated by one: the tables are rebuilt, the machines go on from where they were
        then = np.roll(which, 1)
        assert_multi_crosses(K, then, c, first_push=False)
        pairs = sorted({(int(a), int(b)) for a, b in zip(which, then)})
        exp2 = [expected_of(a, b) for a, b in pairs]
        which2 = np.array([pairs.index((int(a), int(b))) for a, b in zip(which, then)])
        m.push_device(buf, first[then], n[then])
        fr, cm = m.fetch_frames(), m.fetch_commands()
        assert guards(m.h) == 0
        assert_multi_frames(fr, exp2, which2)
        assert_multi_commands(cm, exp2, which2)
        for k in sample:
            assert state_bytes(m.fsm_state(k)) == exp2[which2[k]].state, k
    finally:
        m.close()
        buf.free()


@pytest.mark.gpu
def test_gpu_multi_a_stream_with_three_groups_of_64_frames_whole_and_cut_in_the_third():
    streams = multi_streams() + [crafted_iq(SEEDS)]
    K, longest = len(streams), max(len(s) for s in streams) // 2
    cap_bits, cut_at, n_frames = long_stream_cap_bits()
    assert K == 6 and all(128 <= a < min(192, n) for a, n in zip(cut_at, n_frames))   # the j0 loop's third trip, for both types
    with api.NfcMultiContext(K, longest, hi_val=1.1, input_kind=F32) as m:
        m.push(streams)
        fr, total = check_multi(m, K)
        assert [len(r) for r in fr.frames_of(5).records] == n_frames and total == sum(len(oracle_packets_of(k)) for k in range(5)) + 373
    m, guards = _hooks_multi(K, longest, cap_packet_bits=cap_bits)
    try:
        m.push(streams)
        flags = m.counts_all()['flags']
        assert not (flags[:5] & api.NFC_MULTI_TRUNC_BITS).any() and flags[5] & api.NFC_MULTI_TRUNC_BITS
        fr = m.fetch_frames()
        assert guards(m.h) == 0
        for k in range(5):   # the neighbours are untouched
            assert_frames_equal(fr.frames_of(k), twin_of_stream(m.stream(k)))
        whole, got = host_frames_of(crafted_oracle_packets())[0], fr.frames_of(5)
        for t in (0, 1):
            recs, ref = got.records[t], whole.records[t]
            assert len(recs) == len(ref) and recs['n_bits'].tolist() == ref['n_bits'].tolist()
            cut = np.cumsum(ref['n_bits'].astype(np.int64)) > cap_bits
            assert int(np.nonzero(cut)[0][0]) == cut_at[t] and cut[cut_at[t]:].all()
            assert ((recs['flags'] & CUT) != 0).tolist() == cut.tolist()
            assert (recs['flags'][cut] == CUT).all() and (recs['n_bytes'][cut] == 0).all()
            keep = ~cut
            for name in ('byte_off', 'n_bytes', 'flags', 'type', 'reserved'):   # frames before the cut are exact (idx: the twin's is a list position)
                assert recs[name][keep].tolist() == ref[name][keep].tolist(), name
            nb = int(ref['n_bytes'][keep].sum())
            assert len(got.bytes[t]) == nb and got.bytes[t].tobytes() == whole.bytes[t][:nb].tobytes()
            assert got.par[t].tobytes() == whole.par[t][:nb].tobytes()
    finally:
        m.close()


def _device_equals_twin(fr, **kw):
    dev = air.render_device(fr, **kw)
    try:
        test_air.assert_same(dev, air.host_render(fr, **kw))
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize('tail', [400, 0])
@pytest.mark.parametrize('align', [1, 8])
@pytest.mark.parametrize('kind', [F32, U8])
def test_gpu_air_frame_counts_around_the_layout_trip(kind, align, tail):
    c = constants()
    fr = short_frames_of(c, tail)
    assert np.diff(fr.frame_off).tolist() == [c.BLOCK - 1, c.BLOCK, c.BLOCK + 1, 2 * c.BLOCK + 1, 3]
    _device_equals_twin(fr, out_kind=kind, sigma=0.002, align_samples=align, stream_seeds=[3, 1, 4, 1, 5])


@pytest.mark.gpu
@pytest.mark.parametrize('rate', [2.0, 10.0])
@pytest.mark.parametrize('kind', [F32, I16])
def test_gpu_air_the_longest_frame_in_each_direction(kind, rate):
    c = constants()
    fr = air.frames_of([longest_frames()], rate_msps=rate)
    assert fr.frames['n_bits'].tolist() == [c.MAX_BITS, c.MAX_BITS]   # the dynamic LDS at its largest, RENDER_BLOCK lanes over MAX_BITS + 2 pieces
    assert c.MAX_BITS + 2 > 2 * c.RENDER_BLOCK
    _device_equals_twin(fr, out_kind=kind, sigma=0.002)


@pytest.mark.gpu
def test_gpu_air_a_frame_longer_than_the_longest_is_refused_by_name():
    c = constants()
    frame = (synth.READER, synth.frame_bits(list(range(256)) + [7]))
    assert len(frame[1]) == c.MAX_BITS + 9
    with pytest.raises(ValueError) as e:
        air.render_device([[frame]])
    assert 'frames[0].n_bits' in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize('align', [8, 1])
@pytest.mark.parametrize('kind', [I8, F32])
def test_gpu_air_more_streams_than_the_start_scan_has_threads(kind, align):
    c = constants()
    K, which, seeds = many_air_streams(c)
    assert_air_streams_cross(K, which, c)
    fr = air.frames_of([AIR_LISTS[j] for j in which])
    kw = dict(out_kind=kind, sigma=0.002, align_samples=align, stream_seeds=seeds)
    dev = air.render_device(fr, **kw)
    try:
        test_air.assert_same(dev, air.host_render(fr, **kw))
        first, n = air.sizes(fr, out_kind=kind, align_samples=align)
        assert dev.first_sample.tolist() == first.tolist() and dev.n_samples.tolist() == n.tolist()
        k1, k2 = twin_seeds(which, seeds, c)   # the noise: the seed and the index alone, not K, not the place
        assert dev.download(k1).tobytes() == dev.download(k2).tobytes()
    finally:
        dev.free()


@pytest.mark.gpu
def test_gpu_air_the_loop_at_that_many_streams():
    c = constants()
    K, which, seeds = many_air_streams(c)
    assert_air_streams_cross(K, which, c)
    fr = air.frames_of([AIR_LISTS[j] for j in which])
    cap = air.render_device(fr, out_kind=I8, sigma=0.002, stream_seeds=seeds)
    try:
        with api.NfcMultiContext(K, int(cap.n_samples.max()), hi_val=1.1, input_kind=I8) as m:
            m.track_commands()
            cap.push_to(m)
            reads = int(m.stats().n_reads_device)
            raw, cm = m.fetch_frames(), m.fetch_commands()
            assert int(m.stats().n_reads_device) == reads   # nothing is downloaded between the rendering and the decode
            want = [air_expected(j) for j in range(len(AIR_LISTS))]
            for k in range(K):
                test_air.assert_frames_equal(raw.frames_of(k), want[which[k]][0])
                for a, b in zip(cm.commands_of(k), want[which[k]][1]):
                    assert a.tobytes() == b.tobytes(), k
            assert cm.cmd_off.tolist() == offsets([len(w[1][0]) for w in want], which).tolist()
            assert cm.stream_flags.tolist() == [0] * K
    finally:
        cap.free()


# ---- 5. streams that answer -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_streams_that_answer_past_the_scan_s_threads():
    """k_multi_commands_emu at K = FS_THREADS + 1: a tag card for every stream whose capture is the reader-only transaction, none for
    the others; as tests/test_emulate.py::test_streams_that_answer_equal_the_replay_twin_whole_and_in_pieces compares them."""
    c = constants()
    K = multi_sizes(c)[0]
    which = draw_which(K, c)
    assert_multi_crosses(K, which, c)
    answering = which == READER_ONLY
    assert answering[0] and not answering[K - 1] and 64 < answering.sum() < K - 64
    card = emulate.cards_from_json(os.path.join(GOLDEN, 'fx_emu_ultralight.json'), emulate.NFC_EMU_CARD)[0]
    exp = [expected_of(w) for w in range(len(short_captures()))]
    (wt, wd, we), want = emulate.host_emulate(card, emulate.state_init(), fsm.state_init(), exp[READER_ONLY].frames)
    assert len(want) == 4 and want.records['n_bits'].tolist() == [18, 45, 27, 45]   # ATQA, the two cascade levels' UIDs, the first SAK
    host, first, n = _capture_buffer()
    buf = api.DeviceBuffer(host)
    m, guards = _hooks_multi(K, int(n.max()))
    try:
        m.emulate([card if a else None for a in answering])
        m.push_device(buf, first[which], n[which])
        cm, an = m.fetch_commands(), m.fetch_answers()
        assert guards(m.h) == 0   # the answers' sections included
        assert an.emulated and an.n.tolist() == np.where(answering, len(want), 0).tolist() and an.n_answers == len(want) * int(answering.sum())
        assert_multi_frames(cm.raw, exp, which)
        assert cm.cmd_off.tolist() == offsets([len(x.commands[0]) for x in exp], which).tolist()
        with_card = np.nonzero(answering)[0]
        sample = sorted(set(with_card[[0, 1, -2, -1]].tolist() + with_card[np.linspace(0, len(with_card) - 1, 28).astype(int)].tolist()))
        assert len(sample) >= 28 and sample[-1] > c.FS_THREADS // 2
        for k in sample:   # the twin on the very frames the push assembled
            est, fst = emulate.state_init(), fsm.state_init()
            (t, d, e), ans = emulate.host_emulate(card, est, fst, cm.raw.frames_of(k))
            got_t, got_d, got_e = cm.commands_of(k)
            assert got_t.tobytes() == t.tobytes() == wt.tobytes() and got_d.tobytes() == d.tobytes() and got_e.tobytes() == e.tobytes(), k
            rec, plain, air_bytes, par = an.answers_of(k)
            assert rec.tobytes() == ans.records.tobytes() == want.records.tobytes(), k
            nb = 18 * len(rec)
            assert plain.tobytes() == ans.plain[:nb].tobytes() and air_bytes.tobytes() == ans.air[:nb].tobytes() and par.tobytes() == ans.par[:nb].tobytes(), k
            assert plain.tobytes() == want.plain[:nb].tobytes() and air_bytes.tobytes() == want.air[:nb].tobytes(), k
            assert state_bytes(m.fsm_state(k)) == state_bytes(fst) and state_bytes(m.emu_state(k)) == state_bytes(est), k
        for k in np.nonzero(~answering)[0].tolist():   # a stream without a card decodes on and answers nothing
            assert len(an.answers_of(k)[0]) == 0
            for a, b in zip(cm.commands_of(k), exp[which[k]].commands):
                assert a.tobytes() == b.tobytes(), k
    finally:
        m.close()
        buf.free()
