"""Time sharding across ranks (usrp_nfc_amd/sharding.py): world_size-2 runs on CPU with an oracle-backed engine (the protocol
is host logic) over gloo and over the package's own TCP carrier, and the same boundary hand-off on one GPU."""
import os
import pickle
import socket

import numpy as np
import pytest

from oracle import py_oracle as po
from usrp_nfc_amd import sharding, synth

N_PER = 36000
OVERLAP = 24000


def capture(world):
    m = synth.tiled_profile(synth.modulation_profile(synth.txn_frames(), lead_in=0, tail=0), world * N_PER)
    iq = synth.iq_from_profile(m, seed=77)
    return synth.envelope_f32(iq), iq


class OracleEngine(object):
    """The CPU restatement behind the engine interface decode_shard expects (test stand-in for NfcContext)."""

    def __init__(self, hi_val=1.1):
        self.hi = hi_val
        self.reset()

    state_bytes = 65536   # room for the pickled state below in an exchange slot

    @property
    def av_window(self):
        return self.ts.length

    def reset(self):
        self.sink = po.BitSink()
        self.router = po.Router(po.MillerDecoder(self.sink), po.ManchesterDecoder(self.sink))
        self.out = []
        self.ts = po.TransitionSink(2e6, self._cb, hi_val=self.hi)

    def _cb(self, lst):
        self.out.extend(lst)
        self.router.append(lst)

    def prime(self, start_index, level):
        self.reset()
        ts = self.ts
        L = ts.length
        ts.ring = [float(np.float32(level))] * L
        ts.total = float(np.sum(np.full(L, np.float32(level), np.float32).astype(np.float64)))
        ts.filled, ts.stable = L, True
        ts.index = start_index % L
        ts.dur, ts.last_bit, ts.state = 1, 0, 0

    def push(self, x):
        self.out = []
        self.sink.packets = []
        self.sink.symbols = [[], []]
        po.drive_sink(self.ts, x, 8192)

    def _state(self):
        ts, md, mn = self.ts, self.router.reader_dec, self.router.tag_dec
        L = ts.length
        ring = [ts.ring[(ts.index + i) % L] for i in range(L)]   # oldest first: independent of the rotation
        return (ring, ts.total, ts.dur, ts.last_bit, ts.state,
                (md.prev if md.started else 0, md.started, md.stage()), (mn.prev_set, mn.prev),
                [(p.started, list(p.cur)) for p in self.sink.procs])

    def state_blob(self):
        return np.frombuffer(pickle.dumps(self._state(), protocol=4), np.uint8)

    def set_state_blob(self, blob):
        ring, total, dur, lb, st, mil, man, procs = pickle.loads(bytes(blob))
        ts = self.ts
        L = ts.length
        for i in range(L):
            ts.ring[(ts.index + i) % L] = ring[i]
        ts.total, ts.dur, ts.last_bit, ts.state = total, dur, lb, st
        md, mn = self.router.reader_dec, self.router.tag_dec
        md.prev, md.started = mil[0], mil[1]
        md.set_stage(mil[2])
        mn.prev_set, mn.prev = man
        for p, (s, c) in zip(self.sink.procs, procs):
            p.started, p.cur = s, list(c)


def _worker(rank, world, port, wrong_level, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        x, _ = capture(world)
        lo = rank * N_PER
        own = x[lo:lo + N_PER]
        nov = 64 if wrong_level else OVERLAP          # sabotage: an overlap far too short to converge
        ov = x[lo - nov:lo] if rank else x[:0]
        eng = OracleEngine()
        from tests.dist_util import GlooComm
        comm = GlooComm(dist)
        level = sharding.carrier_level(ov[:4096]) if rank else 0.0
        redos = sharding.decode_shard(eng, comm, lambda: eng.push(ov), lambda: eng.push(own), lo - len(ov), level)
        res = [None] * world
        dist.all_gather_object(res, (redos, eng.out, eng.sink.packets))
        if rank == 0:
            q.put(res)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize('wrong_level', [False, True])
def test_two_ranks_gloo(wrong_level):
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, wrong_level, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x, _ = capture(world)
    ref = po.run_path(x, hi_val=1.1)
    got_tr = [t for _, tr, _ in res for t in tr]
    got_pk = [p for _, _, pk in res for p in pk]
    assert got_tr == ref['transitions']
    assert got_pk == ref['packets']
    if wrong_level:
        assert res[1][0] == 1      # the speculation was sabotaged: exactly one re-decode, result still exact
    else:
        assert res[1][0] == 0      # the overlap speculation hit the true boundary state


def _worker_tcp(rank, world, port, wrong_level, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['RANK'], os.environ['WORLD_SIZE'] = str(rank), str(world)
    from usrp_nfc_amd import comm as cm
    comm = cm.HostComm(tag='t%d' % port)
    try:
        x, _ = capture(world)
        lo = rank * N_PER
        own = x[lo:lo + N_PER]
        nov = 64 if wrong_level else OVERLAP
        ov = x[lo - nov:lo] if rank else x[:0]
        eng = OracleEngine()
        level = sharding.carrier_level(ov[:4096]) if rank else 0.0
        redos = sharding.decode_shard(eng, comm, lambda: eng.push(ov), lambda: eng.push(own), lo - len(ov), level)
        assert comm.max_over_ranks(float(rank)) == float(world - 1)
        res = comm.gather_objects((redos, eng.out, eng.sink.packets))
        if rank == 0:
            q.put(res)
    finally:
        comm.close()


@pytest.mark.parametrize('wrong_level', [False, True])
def test_three_ranks_tcp(wrong_level):
    # the package's own torch-free carrier (usrp_nfc_amd/comm.py: HostComm), three ranks: the middle rank's sabotage shows
    # that a re-decode of rank 1 leaves rank 2's comparison to be evaluated against the corrected end state
    import multiprocessing as mp
    world = 3
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_tcp, args=(r, world, port, wrong_level, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x, _ = capture(world)
    ref = po.run_path(x, hi_val=1.1)
    import json
    plain = lambda v: json.loads(json.dumps(v))   # (HostComm gathers JSON: tuples arrive as lists)
    assert [t for _, tr, _ in res for t in tr] == plain(ref['transitions'])
    assert [p for _, _, pk in res for p in pk] == plain(ref['packets'])
    assert res[0][0] == 0
    if wrong_level:
        assert res[1][0] == 1 and res[2][0] >= 1
    else:
        assert res[1][0] == 0 and res[2][0] == 0


def test_shard_overlap_rule():
    assert sharding.shard_overlap(2e6, 2000) == 38400       # 16 * 2000 + 2 * 3097, to the next multiple of 256
    assert sharding.shard_overlap(10e6, 10000) == 190976
    assert sharding.shard_overlap(2e6, 2000) % 256 == 0


@pytest.mark.gpu
def test_boundary_handoff_on_gpu():
    from oracle import c_oracle as co
    from usrp_nfc_amd import api
    world = 3
    _, iq = capture(world)
    o = co.COracle(hi_val=1.1)
    o.push_iq(iq)
    edges, packets = [], []
    prev_end = None
    for r in range(world):
        lo = r * N_PER
        own = iq[2 * lo:2 * (lo + N_PER)]
        ctx = api.NfcContext(hi_val=1.1)
        if r == 0:
            ctx.reset()
        else:
            ov = iq[2 * (lo - OVERLAP):2 * lo]
            ctx.prime(lo - OVERLAP, sharding.carrier_level(synth.envelope_f32(ov[:8192])))
            ctx.push(ov)
            spec = ctx.state_blob()
            assert np.array_equal(spec, prev_end), 'speculated boundary state differs from the true one'
            # and the explicit hand-off gives the same decode
            ctx2 = api.NfcContext(hi_val=1.1)
            ctx2.set_state_blob(prev_end)
            ctx2.push(own)
            alt = (ctx2.transitions(), ctx2.packets())
            ctx2.close()
        ctx.push(own)
        tr, pk = ctx.transitions(), ctx.packets()
        if r:
            assert alt == (tr, pk)
        edges += tr
        packets += pk
        prev_end = ctx.state_blob()
        ctx.close()
    assert edges == o.transitions()
    assert packets == o.packets()


@pytest.mark.gpu
def test_export_state_matches_state_blob():
    # the device-resident form of the boundary state (what goes into the RCCL all-gather) is byte for byte the
    # host blob, behind a 16-byte length prefix; a slot that is too small gets the prefix only
    from usrp_nfc_amd import api
    _, iq = capture(1)
    ctx = api.NfcContext(hi_val=1.1)
    ctx.push(iq[:2 * 30011])          # ends inside a frame: pending packet bits are part of the state
    blob = ctx.state_blob()
    cap = sharding.slot_bytes(ctx.av_window)
    buf = api.DeviceBuffer(np.zeros(cap, np.uint8), 0)
    n = ctx.export_state(buf.ptr.value, cap)
    ctx.sync()
    assert n == blob.size
    got = buf.download(cap)
    assert int(got[:4].view('<u4')[0]) == blob.size and not got[4:16].any()
    assert np.array_equal(got[16:16 + n], blob)
    small = api.DeviceBuffer(np.full(64, 255, np.uint8), 0)
    assert ctx.export_state(small.ptr.value, 64) == blob.size
    ctx.sync()
    got = small.download(64)
    assert int(got[:4].view('<u4')[0]) == blob.size and (got[16:] == 255).all()
    ctx.close()


@pytest.mark.gpu
def test_context_on_the_callers_stream():
    # nfc_set_stream: the context enqueues on the caller's HIP stream, so a consumer the caller puts on that stream next
    # (here a device-to-host copy of the exported boundary state; in bench.py the RCCL all-gather) needs no host wait in between
    import ctypes as C
    from oracle import c_oracle as co
    from usrp_nfc_amd import api, _lib
    L = _lib.load()
    _, iq = capture(1)
    o = co.COracle(hi_val=1.1)
    o.push_iq(iq)
    side = C.c_void_p()
    assert L.nfc_stream_create(0, C.byref(side)) == 0
    ctx = api.NfcContext(hi_val=1.1)
    cap = sharding.slot_bytes(ctx.av_window)
    slot = api.DeviceBuffer(np.zeros(cap, np.uint8), 0)
    pinned = C.c_void_p()
    assert L.nfc_host_alloc_pinned(cap, C.byref(pinned)) == 0
    ctx.set_stream(side.value)
    ctx.push(iq)
    tr, pk = ctx.transitions(), ctx.packets()
    n = ctx.export_state(slot.ptr.value, cap)                                   # asynchronous, on `side`
    assert L.nfc_device_download_async(0, pinned, slot.ptr, cap, side) == 0      # ordered behind it by the stream alone
    assert L.nfc_stream_sync(0, side) == 0
    got = np.frombuffer((C.c_uint8 * cap).from_address(pinned.value), np.uint8).copy()
    assert tr == o.transitions() and pk == o.packets()
    blob = ctx.state_blob()
    assert n == blob.size and np.array_equal(got[16:16 + n], blob)
    ctx.set_stream(None)   # back on its own stream
    ctx.reset()
    ctx.push(iq)
    assert ctx.transitions() == o.transitions()
    ctx.close()
    L.nfc_host_free_pinned(pinned)
    L.nfc_stream_destroy(0, side)


@pytest.mark.gpu
def test_rccl_exchange_one_rank():
    # the ctypes binding of librccl (usrp_nfc_amd/comm.py): communicator of one rank, the all-gather of the boundary frames out
    # of the device buffer nfc_export_state fills, the scalar all-reduce behind barrier / max_over_ranks
    from oracle import c_oracle as co
    from usrp_nfc_amd import api, comm as cm
    os.environ.setdefault('MASTER_PORT', str(_free_port()))
    comm = cm.RcclComm(0, rank=0, world=1, tag='t1')
    try:
        _, iq = capture(1)
        ctx = api.NfcContext(hi_val=1.1)
        n = len(iq) // 2
        buf = api.DeviceBuffer(iq, 0)
        redos = sharding.decode_shard(ctx, comm, lambda: None, lambda: ctx.push_device(buf, n), 0, 0.0, force_exchange=True)
        assert redos == 0
        o = co.COracle(hi_val=1.1)
        o.push_iq(iq)
        assert ctx.transitions() == o.transitions() and ctx.packets() == o.packets()
        pairs = comm.exchange()
        assert len(pairs) == 1 and pairs[0][0].size == 0 and np.array_equal(pairs[0][1], ctx.state_blob())
        assert comm.max_over_ranks(3.25) == 3.25
        comm.barrier()
        ctx.set_stream(None)
        ctx.close()
    finally:
        comm.close()


@pytest.mark.gpu
def test_bench_spawns_two_ranks_on_one_gpu():
    # `python bench.py --gpus 2` without a launcher: the parent spawns the ranks itself; on a one-GPU box they share the device
    # and carry the boundary states over TCP (NFC_BENCH_BACKEND=host)
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NFC_BENCH_BACKEND='host')
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--samples', '2e6', '--steps', '3', '--warmup', '1',
                        '--full', '--no-cpu-baseline', '--no-extras'], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['n_gpus'] == 2 and line['config']['exchange'] == 'host' and line['config']['boundary_redos'] == 0
    assert line['parity']['edges_equal'] and line['parity']['packets_equal']
    # EVERY rank's shard against the oracle's cut of the whole capture (rank 0 regenerates it), not only rank 0's
    sh = line['parity']['sharded']
    assert sh['ranks_equal'] == [True, True] and sh['all_equal'] and min(sh['n_edges']) > 1000
    assert line['config']['rccl_ranks_seen'] is None   # (the TCP carrier: no RCCL communicator)


@pytest.mark.gpu
def test_bench_eight_ranks_of_configs4_on_one_gpu():
    # BASELINE.json configs[4] in miniature: `bench.py --gpus 8 --workload classic1k` (the -t all decode of the MIFARE Classic 1K
    # capture at 10 Msps, av_window 10000), eight ranks sharing this box's one GPU, boundary states over TCP; EVERY rank's shard
    # against the oracle's cut of the one stream over the whole capture
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NFC_BENCH_BACKEND='host')
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '8', '--workload', 'classic1k', '--samples', '2e7', '--steps', '2',
                        '--warmup', '1', '--full', '--no-cpu-baseline', '--no-extras'], capture_output=True, text=True, timeout=1500, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['n_gpus'] == 8 and line['config']['exchange'] == 'host'
    assert 'configs[3]/[4]' in line['config']['workload'] and line['config']['samples_per_gpu'] == 20_000_000
    sh = line['parity']['sharded']
    assert sh['ranks_equal'] == [True] * 8 and sh['all_equal'] and min(sh['n_edges']) > 1000
    assert line['parity']['edges_equal'] and line['parity']['packets_equal']


def test_bench_checks_a_tiled_capture_at_full_size():
    # configs[4] at its real size must not lose its all-rank parity to the regeneration cap: a tiled capture (every rank's chunk is
    # the same tile again and again) is checked whatever its length; a generated one beyond the cap says it was skipped
    import bench
    assert bench.SHARDED_PARITY_CAP < 8 * bench.default_samples('classic1k')
    skipped = bench.sharded_parity('miller', 10 ** 9, 8, bench.decoder_flags('miller'), [None] * 8)
    assert 'skipped' in skipped
    import inspect
    src = inspect.getsource(bench.sharded_parity)
    assert 'not tiled' in src and "workload == 'classic1k' and n > TILE" in src


@pytest.mark.gpu
@pytest.mark.parametrize('sabotage', [-1, 1])
def test_two_processes_rccl(sabotage):
    # BASELINE.json configs[4]'s exchange for real: two PROCESSES, one GPU each, the boundary states all-gathered by RCCL between
    # the devices (comm.RcclComm over ncclAllGather); each rank's decode against the oracle's cut of the whole capture.  Needs two
    # visible devices (RCCL refuses two ranks on one): skipped on a one-GPU box.  The ranks are fresh child processes.
    import json
    import subprocess
    import sys
    from usrp_nfc_amd import api
    if api.device_count() < 2:
        pytest.skip('two GPUs needed for two RCCL ranks (%d visible)' % api.device_count())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   NFC_TEST_SABOTAGE=str(sabotage), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, 'tests', 'rccl_rank.py')], env=env, cwd=root,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, out[-2000:] + err[-2000:]
        outs.append(json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1]))
    for r, o in enumerate(outs):
        assert o['rank'] == r and o['ranks_seen'] == 2 and o['device'] == r
        assert o['got'] == o['want'], 'rank %d differs from the oracle: %r' % (r, o)
        assert o['got']['n_edges'] > 1000
    assert outs[0]['redos'] == 0
    assert outs[1]['redos'] == (1 if sabotage == 1 else 0)


class ThreadComm(object):
    """Test infrastructure: the ranks of one job as threads of this process (one NfcContext each, all on GPU 0), the boundary
    frames gathered through shared memory behind a barrier -- the host-staged path of decode_shard with real contexts."""
    device_slots = False

    class Shared(object):
        def __init__(self, world):
            import threading
            self.world = world
            self.barrier = threading.Barrier(world)
            self.frames = [None] * world

    def __init__(self, shared, rank):
        self.sh, self.rank, self.world = shared, rank, shared.world
        self.half = 0

    def bind(self, av_window, state_bytes=None):
        self.half = sharding.slot_bytes(av_window)
        self._slots = [np.zeros(0, np.uint8), np.zeros(0, np.uint8)]

    def stream_handle(self):
        return None

    def put(self, slot, blob):
        self._slots[slot] = np.array(blob, np.uint8, copy=True)

    def exchange(self):
        self.sh.frames[self.rank] = (self._slots[0].copy(), self._slots[1].copy())
        self.sh.barrier.wait()
        pairs = list(self.sh.frames)
        self.sh.barrier.wait()
        return pairs


@pytest.mark.gpu
@pytest.mark.parametrize('sabotage', [None, 2])
def test_classic1k_10msps_four_shards_on_gpu(sabotage):
    # BASELINE.json configs[4] in miniature: the MIFARE Classic 1K transaction at 10 Msps (av_window 10000, max_len 250) cut into
    # four time shards with the derived overlap, every shard decoded by a real NfcContext from its speculated boundary state, the
    # states exchanged and verified (decode_shard); concatenated outputs against the C oracle over the whole capture.  With a
    # sabotaged (far too short) overlap on one rank its speculation must be caught and that shard re-decoded from the true state.
    import threading
    from oracle import c_oracle as co
    from usrp_nfc_amd import api
    world, n_per = 4, 700_000
    params = dict(samp_rate=10e6, hi_val=1.1, av_window=10000, max_len=250)
    gold = os.path.join(os.path.dirname(__file__), 'golden', '1k_with_enc.out')
    frames, _ = synth.frames_from_trace(gold)
    m = synth.tiled_profile(synth.modulation_profile(frames, rate_msps=10.0, lead_in=0, tail=0), world * n_per)
    m[:15000] = 1.0   # idle lead-in that covers the window
    iq = synth.iq_from_profile(m, seed=11)
    overlap = sharding.shard_overlap(10e6, 10000)
    assert overlap == 190976
    o = co.COracle(**params)
    o.push_iq(iq)
    shared = ThreadComm.Shared(world)
    results, errors = [None] * world, []

    def run(rank):
        try:
            lo = rank * n_per
            nov = (512 if sabotage == rank else overlap) if rank else 0
            own = iq[2 * lo:2 * (lo + n_per)]
            ov = iq[2 * (lo - nov):2 * lo]
            ctx = api.NfcContext(input_kind=api.NFC_IN_IQ_F32, **params)
            comm = ThreadComm(shared, rank)
            level = sharding.carrier_level(synth.envelope_f32(ov[:2 * 4096])) if rank else 0.0
            redos = sharding.decode_shard(ctx, comm, lambda: ctx.push(ov), lambda: ctx.push(own), lo - nov, level)
            results[rank] = (redos, ctx.transitions(), ctx.packets(), ctx.stats().used_sequential)
            ctx.close()
        except Exception as e:   # noqa: BLE001 -- a failing rank must not leave the others waiting at the barrier
            errors.append((rank, repr(e)))
            shared.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    assert [t for _, tr, _, _ in results for t in tr] == o.transitions()
    assert [p for _, _, pk, _ in results for p in pk] == o.packets()
    assert len(o.packets()) > 100
    redos = [r[0] for r in results]
    if sabotage is None:
        assert redos == [0, 0, 0, 0]
    else:
        assert redos[sabotage] == 1 and redos[0] == 0


def test_overlap_schedule_stops_at_the_first_converged_try():
    """decode_shard's measured warm-up: tries the schedule shortest first, primes each try at its own start with its own level,
    stops when the engine says every window slot has been rewritten, and leaves the length it ended on in engine.overlap_used."""
    assert sharding.overlap_schedule(2e6, 2000, 10**6) == [38400, 70400, 134400, 262400, 518400]
    assert sharding.overlap_schedule(2e6, 2000, 80000) == [38400, 70400]
    assert sharding.overlap_schedule(2e6, 2000, 1000) == [1000]
    assert sharding.overlap_schedule(2e6, 2000, 0) == []

    class Engine(object):
        def __init__(self, converges_at):
            self.calls, self.at = [], converges_at

        def prime(self, start, level):
            self.calls.append(('prime', start, level))

        def window_converged(self):
            return self.calls[-1][1] >= self.at

    class Rank1(object):
        rank, world, device_slots = 1, 1, False   # (world 1: no exchange -- only the warm-up is under test)

    for at, want in ((0, 100), (200, 200), (10**9, 400)):
        e = Engine(at)
        sharding.decode_shard(e, Rank1(), lambda nov: e.calls.append(('ov', nov)), lambda: e.calls.append(('own',)), None,
                              [1.0, 2.0, 3.0], overlap_steps=[100, 200, 400], shard_start=5000)
        tries = [100, 200, 400][:[100, 200, 400].index(want) + 1]
        assert e.calls == [c for k, nov in enumerate(tries) for c in (('prime', 5000 - nov, float(k + 1)), ('ov', nov))] + [('own',)]
        assert e.overlap_used == want


@pytest.mark.gpu
@pytest.mark.parametrize('measured,kind', [(True, 'train'), (False, 'train'), (True, 'dense')])
def test_overlap_is_measured_not_assumed(measured, kind):
    # A capture on which NO fixed number of warm-up windows is enough: for 40 windows before the shard boundary the reader sends a
    # pause every 100 samples -- a period that divides the 2000-sample window, so the same 20 x ~30 window slots are rejected on
    # every pass and keep the values they had before the train.  A warm-up that starts inside the train leaves the primed level in
    # those slots (nfc_stats.ring_slots_carried says how many); decode_shard's measured schedule (16, 32, 64 windows) goes on until
    # the count is zero and gets the boundary state exactly -- no re-decode; the fixed 16 windows are caught by the exchange and
    # pay the re-decode.  Either way the outputs equal the oracle's over the whole capture.
    # 'dense': frames back to back with 50 us gaps (a third of the usual) and no train -- the first try converges, no re-decode.
    import threading
    from oracle import c_oracle as co
    from usrp_nfc_amd import api
    world, n_per, L = 2, 400_000, 2000
    m = synth.tiled_profile(synth.modulation_profile(synth.txn_frames(), gap_us=50.0 if kind == 'dense' else 150.0, lead_in=0, tail=0),
                            world * n_per)
    if kind == 'train':
        train = np.ones(40 * L + 1000, np.float32)
        train.reshape(-1, 100)[:, 10:40] = 0.0
        m[n_per - 40 * L:n_per + 1000] = train
    iq = synth.iq_from_profile(m, seed=5)
    o = co.COracle()
    o.push_iq(iq)
    steps = sharding.overlap_schedule(2e6, L, n_per)[:3] if measured else None
    fixed = sharding.shard_overlap(2e6, L)
    shared = ThreadComm.Shared(world)
    results, errors = [None] * world, []

    def run(rank):
        try:
            lo = rank * n_per
            own = iq[2 * lo:2 * (lo + n_per)]
            ctx = api.NfcContext(input_kind=api.NFC_IN_IQ_F32)
            comm = ThreadComm(shared, rank)
            level_at = lambda nov: sharding.carrier_level(synth.envelope_f32(iq[2 * (lo - nov):2 * (lo - nov + 4096)]))
            carried = []

            def push_overlap(nov=fixed):
                ctx.push(iq[2 * (lo - nov):2 * lo])
                carried.append(int(ctx.stats().ring_slots_carried))
            if rank and measured:
                redos = sharding.decode_shard(ctx, comm, push_overlap, lambda: ctx.push(own), None, [level_at(s) for s in steps],
                                              overlap_steps=steps, shard_start=lo)
            else:
                redos = sharding.decode_shard(ctx, comm, push_overlap, lambda: ctx.push(own), lo - fixed, level_at(fixed) if rank else 0.0)
            results[rank] = (redos, ctx.transitions(), ctx.packets(), carried, getattr(ctx, 'overlap_used', None))
            ctx.close()
        except Exception as e:   # noqa: BLE001
            errors.append((rank, repr(e)))
            shared.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    assert [t for r in results for t in r[1]] == o.transitions()
    assert [p for r in results for p in r[2]] == o.packets()
    redos, carried, used = [r[0] for r in results], results[1][3], results[1][4]
    if kind == 'dense':
        assert carried == [0] and used == steps[0] and redos == [0, 0]
    elif measured:
        assert len(carried) == 3 and carried[0] > 300 and carried[1] > 300 and carried[2] == 0, carried
        assert used == steps[2] and redos == [0, 0]
    else:
        assert carried[0] > 300 and redos == [0, 1]


def test_bench_capture_slices_agree_on_the_samples_they_share():
    # bench.py: a rank's warm-up samples are the END of its predecessor's chunk, bit for bit, whatever length of the schedule is
    # used (the longest is generated, the shorter ones are its tail); the schedule follows the workload's rate and window.
    import bench
    assert bench.overlap_steps('miller', 100_000_000) == [38400, 70400, 134400]
    assert bench.overlap_steps('classic1k', 1_000_000_000) == [190976, 350976, 670976]
    assert bench.overlap_steps('miller', 50_000) == [38400]
    assert bench.overlap_steps('miller', 10_000) == [9984]
    n = 300_000
    ov1, own1 = bench.make_capture_slice('miller', n, 1, 3)
    ov0, own0 = bench.make_capture_slice('miller', n, 0, 3)
    assert len(ov0) == 0 and len(own0) == 2 * n and len(own1) == 2 * n
    assert len(ov1) == 2 * bench.overlap_steps('miller', n)[-1]
    assert np.array_equal(ov1, own0[-len(ov1):])
    ov2, _ = bench.make_capture_slice('miller', n, 2, 3)
    assert np.array_equal(ov2, own1[-len(ov2):])


def test_bench_parity_legs_of_an_eight_gpu_run_fit_the_drivers_clock():
    # `python bench.py --gpus 8 --steps K --warmup W --full` (no --workload) has to fit a 1 800 s limit.  Beside the GPU work that
    # run checks EVERY rank against the pinned C oracle on rank 0's host (bench.sharded_parity): the 8 x 1e8-sample Miller capture is
    # REGENERATED shard by shard and decoded by one core, then configs[4]'s 8 x 1e9-sample tiled capture is decoded tile by tile.  Both
    # legs are linear in the sample count: timed here at a fraction of the size, extrapolated, and held against a budget that leaves
    # the GPU legs the larger part of the limit -- so that the first real SCALE run does not die on a timeout.
    import time
    import bench
    flags = bench.decoder_flags('miller')
    n_small, world = 10_000_000, 8
    t0 = time.perf_counter()
    out = bench.sharded_parity('miller', n_small, world, flags, [None] * world)
    t_gen = time.perf_counter() - t0
    assert 'ranks_equal' in out and len(out['ranks_equal']) == world and min(out['n_edges']) > 1000
    full_generated = t_gen * (100_000_000 / n_small)
    # the tiled capture: one rank's share in miniature (the tile again and again), eight ranks of 1e9 samples in the real run
    # (the tile is generated ONCE, then decoded again and again: two sizes give the cost per tile)
    ts = []
    for tiles in (2, 4):
        t0 = time.perf_counter()
        out4 = bench.sharded_parity('classic1k', tiles * bench.TILE, 1, bench.decoder_flags('classic1k'), [None])
        ts.append(time.perf_counter() - t0)
        assert 'ranks_equal' in out4 and out4['n_edges'][0] > 1000
    per_tile = max(0.0, (ts[1] - ts[0]) / 2.0)
    full_tiled = ts[0] + per_tile * (8 * 1_000_000_000 / bench.TILE - 2)
    assert 8 * 100_000_000 <= bench.SHARDED_PARITY_CAP   # (the default run's generated capture is not skipped)
    # this container's cores are slower than the GPU host's; even so both legs together stay under a third of the driver's limit
    assert full_generated + full_tiled < 600.0, (full_generated, full_tiled)
