"""Random cards and malformed scripts for the emulators' fuzz rows, made from a seed alone -- tests/golden/make_emu_golden.py plays them to
the reference's Tag / Reader and records what they answer, tests/test_emulate_host.py plays the same rows to the twin.  (Not collected by
pytest.)  A step is (command name, extra bytes): what `process_packet(cmd, struct)` is handed."""
import numpy as np

N_TAG_ROWS, N_READER_ROWS = 240, 120


def access(conds):
    """the four access bytes of a trailer for conditions C1 C2 C3 (as a number) of blocks 0 .. 3"""
    c1 = sum(((c >> 2) & 1) << i for i, c in enumerate(conds))
    c2 = sum(((c >> 1) & 1) << i for i, c in enumerate(conds))
    c3 = sum((c & 1) << i for i, c in enumerate(conds))
    return [((~c2 & 0xF) << 4) | (~c1 & 0xF), (c1 << 4) | (~c3 & 0xF), (c3 << 4) | c2, 0x69]


def tag_row(seed):
    """-> (tag_type, mem, rands, steps): a random card -- memory, access bits drawn from all eight conditions (one trailer in eight with
    a broken complement), distinct keys, 1 .. 8 nonces -- and a reader's script with what a reader should not do mixed in."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    ul = seed % 6 == 5
    if ul:
        mem = rng.integers(0, 256, 64).tolist()
        mem[3] = 0x88 ^ mem[0] ^ mem[1] ^ mem[2]
        mem[8] = mem[4] ^ mem[5] ^ mem[6] ^ mem[7]
        steps = [('REQA', []), ('ANTI1R', []), ('SEL1R', [0x88] + mem[:4] if rng.integers(0, 6) else [0x88] + mem[1:5]), ('ANTI2R', []),
                 ('SEL2R', mem[4:9] if rng.integers(0, 6) else mem[3:8])]
        for _ in range(int(rng.integers(2, 8))):
            pick = int(rng.integers(0, 10))
            steps.append(('READR', [int(rng.integers(0, 20))]) if pick < 6 else ('HALT', []) if pick == 6 else ('REQA', []) if pick == 7 else
                         ('WUPA', []) if pick == 8 else ('ANTI2R', []))
        return 0, mem, [], steps
    mem = rng.integers(0, 256, 1024).tolist()
    mem[4] = mem[0] ^ mem[1] ^ mem[2] ^ mem[3]
    for s in range(16):
        a = access(rng.integers(0, 8, 4).tolist())
        if rng.integers(0, 8) == 0:
            a[int(rng.integers(0, 3))] ^= 1 << int(rng.integers(0, 8))
        mem[(4 * s + 3) * 16 + 6:(4 * s + 3) * 16 + 10] = a
    rands = rng.integers(0, 256, (int(rng.integers(1, 9)), 4)).tolist()
    steps = [('REQA', []), ('ANTI1R', [])]
    steps.append(('SEL1R', mem[:5] if rng.integers(0, 8) else rng.integers(0, 256, 5).tolist()))   # SEL with a wrong UID
    for _ in range(int(rng.integers(4, 14))):
        pick = int(rng.integers(0, 20))
        block = int(rng.integers(0, 64)) if rng.integers(0, 4) else 4 * int(rng.integers(0, 16))
        if pick < 5:
            steps += [('AUTHA' if rng.integers(0, 3) else 'AUTHB', [block]), ('RANDRB', rng.integers(0, 256, 8).tolist())]
            sector = block // 4
            for _ in range(int(rng.integers(1, 5))):   # READR inside the sector, and now and then outside it
                steps.append(('READR', [4 * sector + int(rng.integers(0, 4)) if rng.integers(0, 5) else int(rng.integers(0, 80))]))
        elif pick < 9:
            steps.append(('READR', [block]))
        elif pick == 9:
            steps.append(('RANDRB', rng.integers(0, 256, 8).tolist()))
        elif pick == 10:
            steps.append(('HALT', []))
        elif pick == 11:
            steps.append(('WUPA', []))     # WUPA in a session
        elif pick == 12:
            steps.append(('REQA', []))
        elif pick == 13:
            steps.append(('SEL2R', rng.integers(0, 256, 5).tolist()))
        elif pick == 14:
            steps += [('ANTI1R', []), ('SEL1R', mem[:5])]
        elif pick == 15:
            steps.append(('AUTHB', [block]))
        elif pick == 16:
            steps.append(('ATQA1K', []))   # a tag's own direction
        elif pick == 17:
            steps.append((None, rng.integers(0, 256, 3).tolist()))   # a frame the machine does not know
        else:
            steps.append(('ANTI2R', []))
    return 1, mem, rands, steps


def reader_row(seed):
    """-> (rands, steps): a reader's nonces and a tag's script: a card that is read as it should be, cut short and mixed with frames a tag
    would not send there.  At most seven UID frames (the reader's UID holds 32 bytes: a narrowing)."""
    rng = np.random.Generator(np.random.PCG64(5000 + seed))
    rands = rng.integers(0, 256, (int(rng.integers(1, 6)), 4)).tolist()
    uid = rng.integers(0, 256, 4).tolist()
    bcc = uid[0] ^ uid[1] ^ uid[2] ^ uid[3]
    steps, uid_frames = [], 0
    if seed % 4 == 3:
        steps = [('ATQAUL', []), ('ANTI1U', uid), ('SEL1U', []), ('ANTI2T', uid + [bcc]), ('SEL2T', [])]
        uid_frames = 2
        for _ in range(int(rng.integers(1, 6))):
            steps.append(('READT', rng.integers(0, 256, 16).tolist()))
    else:
        steps = [('ATQA1K' if rng.integers(0, 8) else ('ATQA4K' if rng.integers(0, 2) else 'ATQADS'), []), ('ANTI1G', uid + [bcc]), ('SEL1K', [])]
        uid_frames = 1
        for _ in range(int(rng.integers(1, 4))):
            steps += [('RANDTA', rng.integers(0, 256, 4).tolist()), ('RANDTB', rng.integers(0, 256, 4).tolist())]
            for _ in range(int(rng.integers(1, 6))):
                steps.append(('READT', rng.integers(0, 256, 16).tolist()))
    for _ in range(int(rng.integers(0, 5))):
        at = int(rng.integers(0, len(steps) + 1))
        pick = int(rng.integers(0, 8))
        if pick == 0 and uid_frames < 7:
            steps.insert(at, ('ANTI1G', uid + [bcc]))
            uid_frames += 1
        elif pick == 1:
            steps.insert(at, ('READR', [3]))          # a reader's own direction
        elif pick == 2:
            steps.insert(at, ('READT', rng.integers(0, 256, 16).tolist()))
        elif pick == 3:
            steps.insert(at, ('SEL2T', []))
        elif pick == 4:
            steps.insert(at, ('ATQAUL', []))
        elif pick == 5:
            steps.insert(at, (None, rng.integers(0, 256, 2).tolist()))
        elif pick == 6:
            steps.insert(at, ('RANDTB', rng.integers(0, 256, 4).tolist()))
        elif at < len(steps):
            del steps[at]
    return rands, steps
