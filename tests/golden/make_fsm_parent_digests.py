#!/usr/bin/env python3
"""Freezes what the host machine of commit 8370f3e -- the last one with a protocol machine of its own in csrc/protocol.h, beside the
one in csrc/fsm.hip.h -- made of every sequence of tests/golden/fx_fsm_fuzz.npz, PAST the frame where the reference raised, as
truncated SHA-256 digests (tests/golden/fx_fsm_parent.json; tests/fsm_digests.py defines the byte strings and the legs).

Run on a checkout of THAT commit with this file and tests/fsm_digests.py added:
    python3 tests/golden/make_fsm_parent_digests.py
The commit named in the file is the checkout's own HEAD, and the run refuses a library that is not built from it: NFC_AMD_LIB must be
unset (the in-tree library is rebuilt whenever a source is newer) and csrc/ and include/ must be HEAD's, unmodified."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import fsm_digests as fd   # noqa: E402
from tests import test_fsm_fuzz as fz   # noqa: E402


def main():
    git = lambda *a: subprocess.run(('git', '-C', ROOT) + a, stdout=subprocess.PIPE, check=False)
    assert 'NFC_AMD_LIB' not in os.environ, 'the library must be the one this checkout builds'
    assert git('diff', '--quiet', 'HEAD', '--', 'usrp_nfc_amd/csrc', 'usrp_nfc_amd/build.py', 'include').returncode == 0, 'the sources are not HEAD\'s'
    commit = git('rev-parse', '--short=7', 'HEAD').stdout.decode().strip()
    fx = fz.fixture()
    rows = fx['rows']
    out = {'made_by': 'the host machine (csrc/protocol.h) of commit %s, through nfc_fsm_process / nfc_fsm_process_outgoing' % commit,
           'hex_digits_per_row': fd.HEX, 'n_rows': len(rows)}
    out['packets'] = ''.join(fd.packet_digest(r.packets, keys=r.keys) for r in rows)
    out['table'] = ''.join(fd.packet_digest(r.packets, table=fz.full_table(r.keys)) for r in rows[::3])
    # the 256 oracle-decoded rows with the key set-up their streams have on the GPU (tests/test_fsm_fuzz.py: tracked())
    out['gpu'] = ''.join(fd.packet_digest(r.packets, keys=r.keys, table=fz.full_table(r.keys) if k % 3 == 2 else None) for k, r in enumerate(fx['gpu']))
    out['outgoing'] =''.join(fd.outgoing_digest(steps) for _, steps, _ in fx['outgoing'])
    out['long_uid'] = {}
    for name, packets in fd.long_uid_family():
        d, table = fd.long_uid_digest(packets, fd.packet_route)
        assert table['cmd'].tolist() == fd.long_uid_cmds(name), (name, table['cmd'].tolist())
        assert bool(int(table['flags'][-3]) & 4) == name.endswith('other'), name
        out['long_uid'][name] = d
    path = os.path.join(HERE, 'fx_fsm_parent.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d rows, %d table rows, %d scenarios, %d long UIDs: %d bytes' % (len(rows), len(rows[::3]), len(fx['outgoing']), len(out['long_uid']),
                                                                           os.path.getsize(path)))


if __name__ == '__main__':
    main()
