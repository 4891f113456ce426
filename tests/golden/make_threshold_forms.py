#!/usr/bin/env python3
"""Which kernel form the threshold stage sends a batch down, as nfc_stats shows it: the scenarios of tests/test_threshold_forms.py and
the recorder of tests/golden/fx_threshold_forms.json.

    python3 tests/golden/make_threshold_forms.py            record (on a GPU, at the commit whose selection is to be pinned)
    python3 tests/golden/make_threshold_forms.py --check    compare with the committed file instead of writing it

Every form is exact, so parity with the oracle cannot tell a batch that took another form than it used to.  The tuple
(n_chunks, chunk_samples, threshold_passes, chunks_rerun, chunks_rerun_in_place, used_sequential, ran_ahead) of every batch can: chunk
lengths are given explicitly, so nothing in it depends on the device's size.  The file in the tree was recorded at a3b8d4f, the last
commit whose launches were chosen through per-batch members of the context; the recorder refuses a scenario whose tuples do not show
the form it is there for (SHOWS)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fx_threshold_forms.json')
FIELDS = ('n_chunks', 'chunk_samples', 'threshold_passes', 'chunks_rerun', 'chunks_rerun_in_place', 'used_sequential', 'ran_ahead')

N = 200_000
# the level-step stream: 64 chunks of three four-row rounds; a window of 1500 samples lets a chunk be that short (a chunk holds two windows)
STEPS = dict(stream='steps', params=dict(hi_val=1.1, av_window=1500), chunk=3072)
# eight batches of 25 000 samples, two in flight.  The first fills the window and the second follows it synchronously (the LOW bookkeeping
# on the device is valid after a batch that started stable), so the third is the first that runs ahead; the hook of (k) sends every third
# batch that ran ahead through the synchronous path again.  Batches of this size take the one-launch stages and do not run ahead: off.
AHEAD = dict(stream='all', params=dict(hi_val=1.1, av_window=2000), chunk=4096, cuts=list(range(0, N + 1, 25_000)))
SCENARIOS = {
    'a_default_four_rows': dict(stream='all', params=dict(hi_val=1.1, av_window=2000), chunk=4096, env={}),
    'b_eight_rows': dict(stream='all', params=dict(hi_val=1.1, av_window=2560), chunk=6144, env=dict(NFC_WG_NR='8')),
    'c_staging_ring_only': dict(stream='all', params=dict(hi_val=1.1, av_window=2000), chunk=4096, env=dict(NFC_WG_BULK='0')),
    'd_lean': dict(stream='all', params=dict(hi_val=1.1, av_window=2000), chunk=4096, env=dict(NFC_WG='0')),
    'e_general': dict(stream='all', params=dict(hi_val=1.1, av_window=2000), chunk=4096, env=dict(NFC_LEAN='0')),
    'f_global_ring': dict(stream='all', params=dict(hi_val=1.1, av_window=2000), chunk=4096, env=dict(NFC_RING='global')),
    'g_reruns_in_place': dict(STEPS, env={}),
    # (every failing chunk counts as a lone one: the workgroup kernel re-runs it once, the general kernel what it gives up on)
    'h_reruns_lone_and_general': dict(STEPS, env=dict(NFC_WG_EX='0', NFC_WG_LONE='64,1')),
    'i_reruns_general_only': dict(STEPS, env=dict(NFC_WG_EX='0', NFC_WG_RERUN='0')),
    'j_submitted_ahead': dict(AHEAD, env=dict(NFC_NO_SMALL='1')),
    'k_submitted_ahead_redone': dict(AHEAD, env=dict(NFC_NO_SMALL='1', NFC_DEBUG_REDO_SUBMITTED='1')),
}


def _col(rows, name):
    return [r[FIELDS.index(name)] for r in rows]


# what a scenario's tuples must show for the record to pin anything
SHOWS = {
    'a_default_four_rows': lambda t: t == [[49, 4096, 1, 0, 0, 0, 0]],
    'b_eight_rows': lambda t: t == [[33, 6144, 1, 0, 0, 0, 0]],
    'c_staging_ring_only': lambda t: t == [[49, 4096, 1, 0, 0, 0, 0]],
    'd_lean': lambda t: t == [[49, 4096, 1, 0, 0, 0, 0]],
    'e_general': lambda t: _col(t, 'n_chunks') == [49] and _col(t, 'used_sequential') == [0],
    'f_global_ring': lambda t: _col(t, 'n_chunks') == [49] and _col(t, 'used_sequential') == [0],
    'g_reruns_in_place': lambda t: _col(t, 'n_chunks') == [64] and _col(t, 'chunk_samples') == [3072] and t[0][4] > 0 and t[0][5] == 0,
    'h_reruns_lone_and_general': lambda t: _col(t, 'n_chunks') == [64] and t[0][3] > 0 and t[0][4] == 0 and t[0][5] == 0,
    'i_reruns_general_only': lambda t: _col(t, 'n_chunks') == [64] and t[0][3] > 0 and t[0][4] == 0 and t[0][5] == 0,
    'j_submitted_ahead': lambda t: _col(t, 'ran_ahead') == [0, 0, 1, 1, 1, 1, 1, 1] and _col(t, 'used_sequential') == [0] * 8,
    'k_submitted_ahead_redone': lambda t: _col(t, 'ran_ahead')[:2] == [0, 0] and 2 <= sum(_col(t, 'ran_ahead')) < 6 and _col(t, 'used_sequential') == [0] * 8,
}

_STREAMS = {}


def stream(name):
    """'all': the reader's and the tag's frames (usrp_nfc_amd.synth); 'steps': tests.test_gpu_parity._wg_torture -- LOW runs around the
    multiples of max_len, HIGH bursts behind them, and level steps of a few percent, which make chunks fail their certification."""
    if name not in _STREAMS:
        from usrp_nfc_amd import synth
        if name == 'all':
            _STREAMS[name] = synth.workload('all', N)
        else:
            from tests.test_gpu_parity import _wg_torture
            _STREAMS[name] = _wg_torture(77, 64 * 3072)
    return _STREAMS[name]


def run(name, setenv, delenv):
    """One scenario.  setenv / delenv: how a switch is set for the contexts created here and taken back (a switch brings the test
    build of the library).  Returns the tuple of every batch and (transitions, packets) of the whole stream."""
    from usrp_nfc_amd import api
    s = SCENARIOS[name]
    iq = stream(s['stream'])
    for k, v in s['env'].items():
        setenv(k, v)
    try:
        tuples, tr, pk = [], [], []
        with api.NfcContext(input_kind=api.NFC_IN_IQ_F32, chunk_samples=s['chunk'], **s['params']) as ctx:
            def take():
                tr.extend(ctx.transitions())
                pk.extend(ctx.packets())
                st = ctx.stats()
                tuples.append([int(getattr(st, f)) for f in FIELDS])
            if 'cuts' not in s:
                ctx.push(iq)
                take()
            else:
                cuts = s['cuts']
                bufs = [api.DeviceBuffer(iq[2 * a:2 * b]) for a, b in zip(cuts[:-1], cuts[1:])]
                nxt = 0
                for k in range(len(bufs)):
                    while nxt < len(bufs) and nxt < k + 2:
                        ctx.submit_device(bufs[nxt], cuts[nxt + 1] - cuts[nxt])
                        nxt += 1
                    ctx.wait()
                    take()
        return tuples, tr, pk
    finally:
        for k in s['env']:
            delenv(k)


def main():
    from usrp_nfc_amd import _lib

    def setenv(k, v):
        os.environ['NFC_AMD_LIB'] = _lib.hooks_path()
        os.environ[k] = v

    def delenv(k):
        os.environ.pop(k, None)
        os.environ.pop('NFC_AMD_LIB', None)

    got, silent = {}, []
    for name in sorted(SCENARIOS):
        got[name] = run(name, setenv, delenv)[0]
        if not SHOWS[name](got[name]):
            silent.append(name)
        print('%-28s %s%s' % (name, got[name], '   <-- does not show its form' if name in silent else ''))
        sys.stdout.flush()
    if got['h_reruns_lone_and_general'] == got['i_reruns_general_only']:   # (the workgroup kernel's re-runs change the rounds that follow)
        silent.append('h_reruns_lone_and_general')
    if silent:
        sys.exit('nothing written: %s would pin nothing' % silent)
    if '--check' in sys.argv:
        want = json.load(open(OUT))['scenarios']
        bad = [n for n in got if got[n] != want.get(n)]
        print('differs from %s: %s' % (OUT, bad) if bad else 'equal to %s' % OUT)
        sys.exit(1 if bad else 0)
    out = OUT
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    with open(out, 'w') as f:   # (a scenario per line)
        f.write('{"fields": %s,\n "scenarios": {\n' % json.dumps(list(FIELDS)))
        f.write(',\n'.join('  %s: %s' % (json.dumps(n), json.dumps(got[n])) for n in sorted(got)))
        f.write('\n }}\n')
    print('wrote %s' % out)


if __name__ == '__main__':
    main()
