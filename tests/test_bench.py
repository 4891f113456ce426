"""bench.py's plain run and --dump-outputs: the plain line carries the headline only, and what the timed path computed in its
last step is written out so that two builds can be compared output for output (the C oracle on the same seeded capture here)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_arrays(workload, n):
    import bench
    from oracle import c_oracle as co
    _, iq = bench.make_capture_slice(workload, n, 0, 1)
    o = co.COracle(**bench.stream_params(workload), **bench.decoder_flags(workload))
    o.push_iq(iq)
    types, lens, bits = o.packet_arrays()
    return o, types, lens, bits


def check_dump(d, o, types, lens, bits):
    names = ('edges', 'symbols_tag', 'symbols_reader', 'packets', 'packet_bits')
    got = {k: np.load(os.path.join(d, k + '.npy')) for k in names + ('counts',) if os.path.exists(os.path.join(d, k + '.npy'))}
    # every file holds something: an empty output (a decoder the workload does not run) is left out, its count is 0
    assert all(len(v) for v in got.values())
    assert [k for k in names if k not in got] == [k for k, c in zip(names, got['counts']) if c == 0]
    shapes = {'edges': ((0, 4), np.float64), 'packets': ((0, 3), np.float64)}
    got.update({k: np.zeros(*shapes.get(k, ((0,), np.float32))) for k in names if k not in got})
    e = o.edges()
    assert got['edges'].dtype == np.float64 and got['packet_bits'].dtype == np.float32
    assert np.array_equal(got['edges'], np.stack([e['idx'], e['d'], e['v'], e['t']], axis=1).astype(np.float64))
    assert np.array_equal(got['symbols_tag'], o.symbols(0)) and np.array_equal(got['symbols_reader'], o.symbols(1))
    assert np.array_equal(got['packets'][:, 1], types) and np.array_equal(got['packets'][:, 2], lens)
    assert np.array_equal(got['packet_bits'], bits)
    assert got['counts'].tolist() == [len(e), len(o.symbols(0)), len(o.symbols(1)), len(types), len(bits)]
    return got


class StandIn(object):
    """A context that hands out the C oracle's outputs the way NfcContext does (a packet table and a bit array per type)."""

    def __init__(self, o, types, lens, bits):
        self.o, self.types, self.lens, self.bits = o, types, lens, bits
        self.close = np.cumsum(np.arange(1, len(types) + 1))   # (closing edge indices, increasing in stream order)
        self.offs = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)

    def edges(self):
        return self.o.edges()

    def symbols(self, t):
        return self.o.symbols(t)

    def packet_table(self, t):
        from usrp_nfc_amd._lib import PACKET_DTYPE
        m = self.types == t
        tab = np.zeros(int(m.sum()), PACKET_DTYPE)
        tab['idx'], tab['n_bits'], tab['type'] = self.close[m], self.lens[m], t
        tab['bit_off'] = np.concatenate([[0], np.cumsum(self.lens[m])])[:-1]
        return tab

    def packet_bits(self, t):
        m = self.types == t
        return np.concatenate([self.bits[a:a + k] for a, k in zip(self.offs[m], self.lens[m])] or [np.zeros(0, np.uint8)]).astype(np.uint8)


def test_dump_outputs_layout_and_size(tmp_path):
    import bench
    o, types, lens, bits = oracle_arrays('all', 3_000_000)
    assert set(types.tolist()) == {0, 1}
    ctx = StandIn(o, types, lens, bits)
    bench.dump_outputs(ctx, str(tmp_path))
    got = check_dump(str(tmp_path), o, types, lens, bits)
    assert np.array_equal(got['packets'][:, 0], ctx.close)
    # the same directory again, now a Miller-only decode: the tag symbols of the first dump must not stay behind
    o, types, lens, bits = oracle_arrays('miller', 2_000_000)
    bench.dump_outputs(StandIn(o, types, lens, bits), str(tmp_path))
    check_dump(str(tmp_path), o, types, lens, bits)
    assert not (tmp_path / 'symbols_tag.npy').exists()
    # the caps keep a dump of any size under 64 MB
    widths = {'edges': 4 * 8, 'symbols_tag': 4, 'symbols_reader': 4, 'packets': 3 * 8, 'packet_bits': 4}
    assert sum(bench.DUMP_CAPS[k] * w for k, w in widths.items()) <= 64 << 20


def test_dump_outputs_samples_rows_beyond_a_cap(tmp_path, monkeypatch):
    # the 1e8-sample headline always takes this path (6.6 M edges, 4 M reader symbols): caps lowered here to reach it on a small capture
    import bench
    o, types, lens, bits = oracle_arrays('all', 3_000_000)
    caps = {'edges': 5000, 'symbols_tag': 3000, 'symbols_reader': 2000, 'packets': 500, 'packet_bits': 4000}
    for k, v in caps.items():
        monkeypatch.setitem(bench.DUMP_CAPS, k, v)
    full = {}
    bench.dump_outputs(StandIn(o, types, lens, bits), str(tmp_path / 'a'))
    bench.dump_outputs(StandIn(o, types, lens, bits), str(tmp_path / 'b'))
    e = o.edges()
    full['edges'] = np.stack([e['idx'], e['d'], e['v'], e['t']], axis=1).astype(np.float64)
    full['symbols_tag'], full['symbols_reader'] = o.symbols(0).astype(np.float32), o.symbols(1).astype(np.float32)
    counts = np.load(str(tmp_path / 'a' / 'counts.npy'))
    assert counts.tolist() == [len(e), len(o.symbols(0)), len(o.symbols(1)), len(types), len(bits)]
    for k, cap in caps.items():
        x, y = np.load(str(tmp_path / 'a' / (k + '.npy'))), np.load(str(tmp_path / 'b' / (k + '.npy')))
        assert len(x) == cap < counts[list(caps).index(k)] and np.array_equal(x, y), k   # (a fixed sample: the same rows every time)
    # the sampled rows are rows of the full array, in their order: edges by their increasing sample index, symbols as a subsequence
    x = np.load(str(tmp_path / 'a' / 'edges.npy'))
    assert np.all(np.diff(x[:, 0]) > 0) and np.array_equal(x, full['edges'][np.searchsorted(full['edges'][:, 0], x[:, 0])])
    for k in ('symbols_tag', 'symbols_reader'):
        rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(len(full[k]), caps[k], replace=False))
        assert np.array_equal(np.load(str(tmp_path / 'a' / (k + '.npy'))), full[k][rows])


def test_full_run_dumps_only_the_headline(tmp_path, monkeypatch):
    # --full runs other configurations after the headline (rank_main): only the headline's call may write DIR
    import bench
    from usrp_nfc_amd import api
    calls = []

    def run_config(a, workload, n, steps, warmup, rank, world, local, comm, backend, want_parity, chunk=0, kind='iq', dump_dir=None):
        calls.append((workload, kind, dump_dir))
        return {'ms_per_step': 1.0, 'value': 1.0, 'config': {'time_chunks': 1}, 'roofline': {}}, np.zeros(2, np.float32), {}
    monkeypatch.setattr(bench, 'run_config', run_config)
    monkeypatch.setattr(bench, 'end_to_end', lambda *args: {'value': 1.0, 'link_GBs_in': 1.0})
    monkeypatch.setattr(bench, 'stress_config', lambda *args: {'ms_per_step': 1.0})
    monkeypatch.setattr(api, 'device_count', lambda: 1)
    for v in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'NFC_BENCH_FORCE_EXCHANGE'):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--no-cpu-baseline', '--dump-outputs', str(tmp_path)])
    bench.rank_main(bench.parse())
    assert calls[0] == ('miller', 'iq', str(tmp_path))
    assert len(calls) == 5 and all(d is None for _, _, d in calls[1:]), calls


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    n = 2_000_000
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--samples', '%d' % n, '--steps', '3', '--warmup', '1',
                        '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['value'] > 0 and line['higher_is_better'] is True
    assert line['unit'] == 'Msamples/s' and line['metric'].startswith('IQ Msamples/s') and line['dtype']
    for k in ('roofline', 'parity', 'cpu_baseline', 'submitted_ahead', 'other_configs', 'stress'):
        assert k not in line, k
    # every timed step is a fresh stream over the same capture: the last one decodes what the oracle decodes
    o, types, lens, bits = oracle_arrays('miller', n)
    got = check_dump(str(tmp_path), o, types, lens, bits)
    assert not os.path.exists(str(tmp_path / 'symbols_tag.npy'))   # (Miller only: no tag decoder, no file)
    assert line['config']['edges_per_gpu'] == len(got['edges']) and np.all(np.diff(got['packets'][:, 0]) > 0)
