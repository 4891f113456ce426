"""The one protocol machine (csrc/fsm.hip.h) against what the project's first host machine made of the same traffic.

Until commit 8370f3e csrc/protocol.h held a protocol machine of its own -- vectors, a bit list per frame -- and csrc/fsm.hip.h restated it for
host and device; tests compared the two.  Now protocol.h is a shell over fsm.hip.h, and that comparison would compare a text with itself.  So
what the separate machine computed was recorded before it was deleted: tests/golden/fx_fsm_parent.json (tests/golden/make_fsm_parent_digests.py,
run at that commit; tests/fsm_digests.py defines the byte strings) holds a truncated SHA-256 per row of tests/golden/fx_fsm_fuzz.npz over the
WHOLE sequence -- past the frame where the reference raised and tests/test_fsm_fuzz.py stops comparing text -- and the state afterwards.
Every route through the machine reproduces them; every comparison is for equality."""
import json
import os

import pytest

from tests import fsm_digests as fd
from tests import test_fsm_fuzz as fz
from tests.golden_util import GOLDEN
from tests.test_commands_host import run_host, state_bytes
from tests.test_frames import host_frames_of
from usrp_nfc_amd import _lib

_cache = {}


def parent():
    if 'p' not in _cache:
        with open(os.path.join(GOLDEN, 'fx_fsm_parent.json')) as f:
            p = json.load(f)
        n = p['hex_digits_per_row']
        for leg in ('packets', 'table', 'gpu', 'outgoing'):
            p[leg] = [p[leg][i:i + n] for i in range(0, len(p[leg]), n)]
        _cache['p'] = p
    return _cache['p']


def differing(got, want):
    got = list(got)
    assert len(got) == len(want)
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


def test_the_fixture_is_the_parents():
    p = parent()
    assert '8370f3e' in p['made_by'] and p['n_rows'] == len(fz.fixture()['rows']) == len(p['packets']) == 2256
    assert len(p['table']) == 752 and len(p['outgoing']) == len(fz.fixture()['outgoing']) and len(p['long_uid']) == 8
    assert os.path.getsize(os.path.join(GOLDEN, 'fx_fsm_parent.json')) < 64 * 1024


def test_packet_route_reproduces_the_parent():
    assert differing((fd.packet_digest(r.packets, keys=r.keys) for r in fz.fixture()['rows']), parent()['packets']) == []


def test_frame_route_reproduces_the_parent():
    got = []
    for row in fz.fixture()['rows']:
        m = fd.machine(row.keys)
        got.append(fd.row_digest(*run_host(m, fz.frames_of(row)), state=fd.state_of(m)))
    assert differing(got, parent()['packets']) == []


def test_twin_reproduces_the_parent():
    got, overflow = [], 0
    for row in fz.fixture()['rows']:
        (table, data, enc), st = fz.twin_run(row)
        overflow += int(bool(st.flags & _lib.NFC_FSM_UID_OVERFLOW))
        got.append(fd.row_digest(table, data, enc, state_bytes(st)))
    assert overflow == 0   # (no fuzz row grows a UID past the twin's 32 bytes: the long-UID family below is the host machine's alone)
    assert differing(got, parent()['packets']) == []


def test_table_leg_reproduces_the_parent():
    rows = fz.fixture()['rows'][::3]
    assert differing((fd.packet_digest(r.packets, table=fz.full_table(r.keys)) for r in rows), parent()['table']) == []
    got = []
    for row in rows:   # ... and the twin with the table, no keys set
        (table, data, enc), st = fz.twin_run(row, sector_keys=fz.full_table(row.keys), keys=None)
        got.append(fd.row_digest(table, data, enc, state_bytes(st)))
    assert differing(got, parent()['table']) == []


def test_gpu_rows_with_their_streams_keys_reproduce_the_parent():
    """The 256 oracle-decoded rows with the key set-up of their GPU streams (test_fsm_fuzz.tracked): set_keys, every third also the full table."""
    got, twin = [], []
    for k, row in enumerate(fz.fixture()['gpu']):
        keyed = fz.full_table(row.keys) if k % 3 == 2 else None
        got.append(fd.packet_digest(row.packets, keys=row.keys, table=keyed))
        (table, data, enc), st = fz.twin_run(row, sector_keys=keyed)
        twin.append(fd.row_digest(table, data, enc, state_bytes(st)))
    assert differing(got, parent()['gpu']) == [] and differing(twin, parent()['gpu']) == []


def test_outgoing_scenarios_reproduce_the_parent():
    assert differing((fd.outgoing_digest(steps) for _, steps, _ in fz.fixture()['outgoing']), parent()['outgoing']) == []


def frame_route(m, packets):
    return run_host(m, host_frames_of(packets)[0])


@pytest.mark.parametrize('route', [fd.packet_route, frame_route], ids=['packets', 'frames'])
def test_long_uids_reproduce_the_parent(route):
    """The host machine's UID is unbounded and follows the reference past 32 bytes (the twin and the kernel stop there and say so)."""
    want = parent()['long_uid']
    for name, packets in fd.long_uid_family():
        d, table = fd.long_uid_digest(packets, route)
        assert table['cmd'].tolist() == fd.long_uid_cmds(name), name
        assert bool(int(table['flags'][-3]) & 4) == name.endswith('other'), name   # the SEL2R: UID_MISMATCH where it names other bytes
        assert d == want[name], name


def test_fsm_check_embeds_the_classic_prefix():
    """tools/fsm_check/main.cpp runs the host machine's routes under -fsanitize=address,undefined (a stand-alone program: nothing loaded into
    python is): its packets are the 24-frame prefix of the Classic trace, eight bits to a byte."""
    import re
    from tests.test_commands_host import PREFIX, classic_packets
    text = open(os.path.join(os.path.dirname(GOLDEN), '..', 'tools', 'fsm_check', 'main.cpp')).read()
    body = text[text.index('BITS[206] = {'):]
    got = [int(v, 16) for v in re.findall(r'0x([0-9A-F]{2})', body[:body.index('};')])]
    want, rows = [], []
    for t, bits in classic_packets()[0][:PREFIX]:
        rows.append('{%d, %d, %d}' % (t, len(bits), len(want)))
        want += [sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8)]
    assert got == want and all(r in re.sub(r'\s+', ' ', text) for r in rows)


@pytest.mark.gpu
def test_gpu_256_streams_reproduce_the_parent():
    """The cached one push of tests/test_fsm_fuzz.py: every stream's records, bytes, enc entries and state are the parent host machine's on
    the row's packets -- with set_keys, and for every third stream the full table as well (tracked())."""
    res = fz.gpu_one_push()
    got = [fd.row_digest(table, data, enc, state) for (table, data, enc), state in zip(res['got'], res['state'])]
    assert differing(got, parent()['gpu']) == []
