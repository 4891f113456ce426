"""The reference's create_json module (create_json.py): writes the two card files its emulators read -- `classic1k.json`, a tag entry
(type CLASSIC1K, the memory of Tag.generate_1k, sixteen nonces) and a reader entry (sixteen nonces), and `ultralight.json`, a tag entry of
type ULTRALIGHT -- in the format parser.Parser takes (parser.py:12-16).

The Classic memory is Tag.generate_1k's, the Ultralight's sixty-four bytes are what the four READ answers of the reference's own trace
show (synth.ULTRALIGHT_TXN: outputs/ultralight.out).  The NONCES are this project's: emulate.drawn_rands draws them from a seeded generator,
where the reference's file lists sixteen recorded ones -- those are data of the reference and live in tests/golden/fx_emu_classic1k.json,
not in program text.  The reference runs at import; here the work is `write(directory)`, and running the module calls it on '.'."""
import json
import os

from . import emulate, synth


def ultralight_memory():
    """pages 0 .. 15 as the trace's four READ answers (of pages 0, 4, 8, 12) give them"""
    reads = [data[:16] for _, name, data, _ in synth.ULTRALIGHT_TXN if name == 'READT']
    assert len(reads) == 4
    return [b for r in reads for b in r]


def classic1k_entries(tag_seed=0, reader_seed=1):
    return [{'entry': 'tag', 'rands': emulate.drawn_rands(tag_seed), 'type': 'CLASSIC1K', 'mem': emulate.generate_1k()},
            {'entry': 'reader', 'rands': emulate.drawn_rands(reader_seed)}]


def ultralight_entries():
    return [{'entry': 'tag', 'type': 'ULTRALIGHT', 'mem': ultralight_memory()}]


def write(directory='.'):
    """-> the two paths written"""
    paths = []
    for name, ar in (('classic1k.json', classic1k_entries()), ('ultralight.json', ultralight_entries())):
        paths.append(os.path.join(directory, name))
        with open(paths[-1], 'w') as f:
            json.dump(ar, f)
    return paths


if __name__ == '__main__':
    write()
