"""MIFARE Classic key recovery from sniffed authentications (include/nfc_amd.h: nfc_find_auths, nfc_recover_keys_device,
nfc_host_recover_keys and their nested counterparts; csrc/keys.hip.h states the method, DESIGN.md 8h and 8i the layout).

``find_auths(frames)`` picks the first authentications out of one stream's frames, ``recover(traces)`` searches their keys on the GPU,
``host_recover(traces)`` is the same search on one CPU core.  Both return ``(results, stats)``: a KEY_RESULT_DTYPE record per trace and
the call's _lib.KeyStats.  There is no fall-back from one to the other.

Every later authentication of a session is NESTED, its tag nonce encrypted: ``find_nested_auths(frames)`` finds them by shape,
``nested_candidates(traces)`` lists the 64 (or 0) plaintext nonces each can have, ``recover_nested(traces)`` / ``host_recover_nested``
search one key per candidate and report a NESTED_RESULT_DTYPE record per trace, and ``label_auths`` decrypts the AUTH commands with the
recovered keys to say which sector each key belongs to.

WITHOUT {at} -- a stream that emulates a tag, a sniffer that hears the reader only -- one authentication is not enough and two are
(DESIGN.md 8n): ``find_reader_auths(frames)`` is find_auths less the {at} frame, ``pair_reader_auths(traces)`` pairs two sessions of
one (stream, uid, key type, sector), ``recover_reader(pairs)`` / ``host_recover_reader`` search a READER_KEY_RESULT_DTYPE record per
pair, and ``recover_reader_streams`` merges the keys into the per-stream dicts.

A card has a key A and a key B PER SECTOR: ``sector_of(block)`` is the mapping, ``sector_table(found)`` turns the recovered
``(key_type, block) -> key`` into the ``(key_type, sector) -> key`` table that the protocol machines take (fsm.set_sector_keys,
NfcMultiContext.set_sector_keys, fsm.host_commands(..., sector_keys=)), ``key_table`` / ``table_dict`` go between that dict and the C
structure (_lib.FsmKeyTable: nfc_fsm_key_table)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (AUTH_DTYPE, KEY_RESULT_DTYPE, NESTED_CANDS, NESTED_DTYPE, NESTED_RESULT_DTYPE, NFC_KEY_AMBIGUOUS,  # noqa: F401
                   NFC_KEY_NONE, NFC_KEY_OK, NFC_KEY_OVERFLOW, NFC_KEY_TIMING, NFC_RKEY_VERIFY_INLINE, READER_KEY_RESULT_DTYPE,
                   READER_PAIR_DTYPE)


class KeyRecoveryError(RuntimeError):
    pass


def _find(name, dtype, frames, per=4):
    L = _lib.load()
    t = np.ascontiguousarray(frames.table, _lib.RAW_FRAME_DTYPE)
    b = [np.ascontiguousarray(a, np.uint8) for a in frames.bytes]
    p = [np.ascontiguousarray(a, np.uint8) for a in frames.par]
    out = np.zeros(len(t) // per + 1, dtype)   # (an authentication is `per` frames)
    n = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    rc = getattr(L, name)(ptr(t), len(t), ptr(b[0]), ptr(p[0]), ptr(b[1]), ptr(p[1]), out.ctypes.data, len(out), C.byref(n))
    if rc != 0:
        raise KeyRecoveryError('%s status %d' % (name, rc))
    return out[:n.value]


def find_auths(frames):
    """The first authentications of one stream: `frames` an api.NfcFrames (NfcContext.frames(), NfcMultiFrames.frames_of(k),
    api.host_frames) -> AUTH_DTYPE records in stream order, `stream` 0."""
    return _find('nfc_find_auths', AUTH_DTYPE, frames)


def find_nested_auths(frames):
    """The nested authentications of one stream, found by shape with no keys (nfc_find_nested_auths) -> NESTED_DTYPE records in stream
    order, `stream` 0, key_type 0 and block 0xFF (label_auths fills them in)."""
    return _find('nfc_find_nested_auths', NESTED_DTYPE, frames)


def _config(initial_capacity=0, max_capacity=0, max_batch=0, timing=False):
    return _lib.KeyConfig(int(initial_capacity), int(max_capacity), int(max_batch), NFC_KEY_TIMING if timing else 0)


def _run(call, traces, cfg):
    t = np.ascontiguousarray(traces, AUTH_DTYPE).reshape(-1)
    out, stats = np.zeros(len(t), KEY_RESULT_DTYPE), _lib.KeyStats()
    rc = call(t.ctypes.data if len(t) else None, len(t), C.byref(_config(**cfg)), out.ctypes.data if len(t) else None, C.byref(stats))
    if rc != 0:
        raise KeyRecoveryError('key recovery failed with status %d' % rc)
    return out, stats


def recover(traces, device=0, **cfg):
    """Every trace's key on the GPU (nfc_recover_keys_device).  cfg: initial_capacity / max_capacity (table slots per group of traces,
    0: the defaults), max_batch (traces per count launch), timing (HIP events -> stats.ms_*)."""
    L = _lib.load()
    return _run(lambda *a: L.nfc_recover_keys_device(int(device), *a), traces, cfg)


def host_recover(traces, **cfg):
    """The CPU twin (nfc_host_recover_keys): the same results, statuses and capacity rules, no GPU."""
    return _run(_lib.load().nfc_host_recover_keys, traces, cfg)


def find_reader_auths(frames):
    """The first authentications of one stream as far as the READER's {nr}{ar} (nfc_find_reader_auths): find_auths' rule less the {at}
    frame, so a superset of find_auths' by `frame` -> AUTH_DTYPE records, at_enc and par bits 8 .. 11 zero."""
    return _find('nfc_find_reader_auths', AUTH_DTYPE, frames, per=3)


def pair_reader_auths(traces):
    """Pairs for recover_reader: the traces are grouped by (stream, uid, key_type, sector_of(block)) in order of first appearance, and
    per group the FIRST TWO sessions that differ in nt or nr_enc make one pair (search: the earlier) -- two identical sessions single
    nothing out and are never paired.  -> (READER_PAIR_DTYPE records, the unpaired traces as AUTH_DTYPE records, in order)."""
    t = np.ascontiguousarray(traces, AUTH_DTYPE).reshape(-1)
    groups = {}
    for i, a in enumerate(t):
        groups.setdefault((int(a['stream']), int(a['uid']), int(a['key_type']), sector_of(int(a['block']))), []).append(i)
    pairs, used = [], set()
    for idx in groups.values():
        first = t[idx[0]]
        other = next((j for j in idx[1:] if (int(t[j]['nt']), int(t[j]['nr_enc'])) != (int(first['nt']), int(first['nr_enc']))), None)
        if other is not None:
            pairs.append((idx[0], other))
            used.update((idx[0], other))
    out = np.zeros(len(pairs), READER_PAIR_DTYPE)
    for k, (a, b) in enumerate(pairs):
        out[k]['search'], out[k]['check'] = t[a], t[b]
    return out, t[[i for i in range(len(t)) if i not in used]]


def _run_reader(call, pairs, stage_capacity, verify_inline, cfg):
    p = np.ascontiguousarray(pairs, READER_PAIR_DTYPE).reshape(-1)
    out, stats = np.zeros(len(p), READER_KEY_RESULT_DTYPE), _lib.KeyStats()
    c = _lib.ReaderKeyConfig(_config(**cfg), int(stage_capacity), NFC_RKEY_VERIFY_INLINE if verify_inline else 0)
    rc = call(p.ctypes.data if len(p) else None, len(p), C.byref(c), out.ctypes.data if len(p) else None, C.byref(stats))
    if rc != 0:
        raise KeyRecoveryError('reader key recovery failed with status %d' % rc)
    return out, stats


def recover_reader(pairs, device=0, stage_capacity=0, verify_inline=False, **cfg):
    """Every pair's key on the GPU (nfc_recover_reader_keys_device): two reader-side authentications of one key, no {at} needed.
    stage_capacity: joined candidates per pair handed to the verify launch (0: the default); verify_inline: no stage, the walking lane
    verifies (NFC_RKEY_VERIFY_INLINE).  cfg: recover's.  -> (READER_KEY_RESULT_DTYPE records, _lib.KeyStats)."""
    L = _lib.load()
    return _run_reader(lambda *a: L.nfc_recover_reader_keys_device(int(device), *a), pairs, stage_capacity, verify_inline, cfg)


def host_recover_reader(pairs, stage_capacity=0, verify_inline=False, **cfg):
    """The CPU twin (nfc_host_recover_reader_keys): the same results, statuses and capacity rules, about a second per pair on one core."""
    return _run_reader(_lib.load().nfc_host_recover_reader_keys, pairs, stage_capacity, verify_inline, cfg)


def reader_options(reader_pairs, cfg):
    """The keywords of the reader-pair call of a combined recovery: `cfg` (the search options every recovery call takes) and, where the
    `reader_pairs` switch is a dict and not just True, recover_reader's OWN options out of it (stage_capacity, verify_inline)."""
    own = dict(reader_pairs) if isinstance(reader_pairs, dict) else {}
    unknown = sorted(set(own) - {'stage_capacity', 'verify_inline'})
    if unknown:
        raise TypeError('reader_pairs: unknown options %s' % unknown)
    return dict(cfg, **own)


def recover_reader_streams(reader_traces, found, device=0, host=False, **cfg):
    """The reader-pair branch of a key recovery over several streams.  `reader_traces`: every stream's find_reader_auths records with
    `stream` filled in; `found`: per stream the dict (key_type, block) -> key that the full search already gave.  The sessions whose
    (key_type, block) has no key yet are paired (pair_reader_auths) and searched in ONE recover_reader call (host=True: the twin); a key
    found exactly (NFC_KEY_OK) goes into its stream's dict under the SEARCHED session's (key_type, block), an earlier entry winning.
    -> the new list of dicts (`found` is not changed)."""
    out = [dict(d) for d in found]
    t = np.ascontiguousarray(reader_traces, AUTH_DTYPE).reshape(-1)
    todo = [i for i, a in enumerate(t) if (int(a['key_type']), int(a['block'])) not in out[int(a['stream'])]]
    pairs, _ = pair_reader_auths(t[todo])
    if len(pairs):
        results, _ = host_recover_reader(pairs, **cfg) if host else recover_reader(pairs, device=device, **cfg)
        for p, r in zip(pairs, results):
            if int(r['status']) == NFC_KEY_OK:
                s = p['search']
                out[int(s['stream'])].setdefault((int(s['key_type']), int(s['block'])), bytes(bytearray(r['key'].tolist())))
    return out


def keys_by_stream(traces, results, n_streams):
    """Per stream a dict (key_type, block) -> six key bytes, of the traces whose key was found exactly (NFC_KEY_OK); the first
    authentication of a stream with that type and block wins."""
    out = [dict() for _ in range(n_streams)]
    for t, r in zip(traces, results):
        if int(r['status']) == NFC_KEY_OK:
            out[int(t['stream'])].setdefault((int(t['key_type']), int(t['block'])), bytes(bytearray(r['key'].tolist())))
    return out


def first_keys(found):
    """(key_a, key_b) for set_keys from one stream's dict of keys_by_stream: the first key found per type, the default FF..FF where none."""
    pair = []
    for kt in (0x60, 0x61):
        ks = [v for (t, _), v in found.items() if t == kt]
        pair.append(list(bytearray(ks[0])) if ks else [0xFF] * 6)
    return tuple(pair)


def sector_of(block):
    """The sector of a block (nfc_sector_of_block): blocks 0 .. 127 four to a sector, 128 .. 255 sixteen -> 0 .. 39."""
    s = _lib.load().nfc_sector_of_block(int(block))
    if s < 0:
        raise ValueError('block %r is outside 0 .. 255' % (block,))
    return s


def key_table(table=None):
    """An _lib.FsmKeyTable (nfc_fsm_key_table) from None (empty), another FsmKeyTable (a checked copy) or a dict
    (key_type, sector) -> six key bytes (None: that slot stays empty), key_type 0x60 / 0x61, sector 0 .. 39.  ValueError names what is wrong."""
    t = _lib.FsmKeyTable()
    if table is None:
        return t
    if isinstance(table, _lib.FsmKeyTable):
        C.memmove(C.byref(t), C.byref(table), C.sizeof(t))
        if any(p > 1 for row in t.present for p in row):
            raise ValueError('present: a byte of the table is neither 0 nor 1')
        return t
    for (key_type, sector), key in dict(table).items():
        if key_type not in (0x60, 0x61):
            raise ValueError('key_type %r is neither 0x60 nor 0x61' % (key_type,))
        if not 0 <= int(sector) < _lib.NFC_KEY_SECTORS:
            raise ValueError('sector %r is outside 0 .. %d' % (sector, _lib.NFC_KEY_SECTORS - 1))
        if key is None:
            continue
        k = list(bytearray(key))
        if len(k) != 6:
            raise ValueError('key: the key of (0x%02X, %d) is not six bytes' % (key_type, sector))
        t.present[key_type & 1][int(sector)] = 1
        for i in range(6):
            t.key[key_type & 1][int(sector)][i] = k[i]
    return t


def table_dict(table):
    """An _lib.FsmKeyTable as the dict (key_type, sector) -> six key bytes of its present slots."""
    return {(0x60 + t, s): bytes(bytearray(table.key[t][s])) for t in (0, 1) for s in range(_lib.NFC_KEY_SECTORS) if table.present[t][s]}


def sector_table(found):
    """A dict of recovered keys (key_type, block) -> key (keys_by_stream, label_auths, a background's ``recovered_keys``) as the machines'
    table: -> (table, conflicts), `table` the dict (key_type, sector) -> six key bytes.  Two blocks of one sector whose keys differ cannot
    both be right: the LOWER block's key is kept and the other entry comes back in `conflicts`, a dict (key_type, block) -> key."""
    table, conflicts = {}, {}
    for (key_type, block), key in sorted(found.items()):
        slot, key = (int(key_type), sector_of(block)), bytes(bytearray(key))
        if table.setdefault(slot, key) != key:
            conflicts[(int(key_type), int(block))] = key
    return table, conflicts


def nested_candidates(traces, device=None):
    """The candidate plaintext nonces of every nested trace, ascending in seed -> (nt [n][64] uint32, n [n] uint32; unused entries 0).
    device None: the host twin (nfc_host_nested_candidates), else the kernel's answer on that device (nfc_nested_candidates_device)."""
    L = _lib.load()
    t = np.ascontiguousarray(traces, NESTED_DTYPE).reshape(-1)
    nt, cnt = np.zeros((len(t), NESTED_CANDS), np.uint32), np.zeros(len(t), np.uint32)
    if device is None:
        for i in range(len(t)):
            n = C.c_size_t(0)
            rc = L.nfc_host_nested_candidates(t[i:i + 1].ctypes.data, nt[i].ctypes.data, NESTED_CANDS, C.byref(n))
            if rc != 0:
                raise KeyRecoveryError('nfc_host_nested_candidates status %d' % rc)
            cnt[i] = n.value
    else:
        ptr = lambda a: a.ctypes.data if a.size else None
        rc = L.nfc_nested_candidates_device(int(device), ptr(t), len(t), ptr(nt), ptr(cnt))
        if rc != 0:
            raise KeyRecoveryError('nfc_nested_candidates_device status %d' % rc)
    return nt, cnt


def _run_nested(call, traces, cand_first, cand_count, cfg):
    t = np.ascontiguousarray(traces, NESTED_DTYPE).reshape(-1)
    out, stats = np.zeros(len(t), NESTED_RESULT_DTYPE), _lib.KeyStats()
    c = _lib.NestedConfig(_config(**cfg), int(cand_first), int(cand_count))
    rc = call(t.ctypes.data if len(t) else None, len(t), C.byref(c), out.ctypes.data if len(t) else None, C.byref(stats))
    if rc != 0:
        raise KeyRecoveryError('nested key recovery failed with status %d' % rc)
    return out, stats


def recover_nested(traces, device=0, cand_first=0, cand_count=0, **cfg):
    """Every nested trace's key on the GPU (nfc_recover_nested_keys_device): one search per candidate nonce of the window
    [cand_first, cand_first + cand_count) of each trace's ascending list (cand_count 0: all from cand_first).  cfg: recover's; capacity
    and max_batch count (trace, candidate) pairs.  -> (NESTED_RESULT_DTYPE records, _lib.KeyStats)."""
    L = _lib.load()
    return _run_nested(lambda *a: L.nfc_recover_nested_keys_device(int(device), *a), traces, cand_first, cand_count, cfg)


def host_recover_nested(traces, cand_first=0, cand_count=0, **cfg):
    """The CPU twin (nfc_host_recover_nested_keys): a quarter of a second per candidate on one core, so give it a window."""
    return _run_nested(_lib.load().nfc_host_recover_nested_keys, traces, cand_first, cand_count, cfg)


def label_auths(frames, firsts, first_results, nested, nested_results):
    """Which sector every recovered key of ONE stream belongs to.  Host only.  The project's protocol machine runs once over `frames` (an
    api.NfcFrames), in slices: before the AUTH frame of every authentication whose key was recovered (status NFC_KEY_OK) both of its keys
    are set to that key.  A nested trace's AUTH command then decrypts under its PREDECESSOR's key, and where its CRC holds the trace's
    key_type and block are filled in (`nested` is written in place); one whose predecessor's key was not recovered stays unlabelled.
    -> dict (key_type, block) -> six key bytes over the firsts and the labelled nesteds with status OK; the first of a kind wins."""
    from . import fsm as _fsm
    import io
    auths = sorted([(int(t['frame']), False, i) for i, t in enumerate(firsts)] + [(int(t['frame']), True, i) for i, t in enumerate(nested)])
    m = _fsm.fsm(out=io.StringIO())
    table, found, at = frames.table, {}, 0
    key_bytes = lambda r: bytes(bytearray(r['key'].tolist()))

    def run(upto):   # the frames [at, upto) -> the record of the last one and its plaintext bytes
        out, buf = m.process_frames(table[at:upto], frames.bytes, frames.par, dispatch=False)
        if not len(out):
            return None, []
        o = int(out[-1]['byte_off'])
        return out[-1], buf[o:o + int(out[-1]['n_bytes'])].tolist()

    prev_ok = False   # the session's keystream is right up to here: the previous authentication's key is known
    for frame, is_nested, i in auths:
        run(frame)
        at = frame
        r = (nested_results if is_nested else first_results)[i]
        ok = int(r['status']) == NFC_KEY_OK
        if ok:
            m.set_keys(r['key'].tolist(), r['key'].tolist())
        rec, data = run(frame + 1)   # the AUTH frame itself; the nonce that follows takes the key that is set now
        at = frame + 1
        # (the machine names a frame AUTHA / AUTHB only where 60|61 blk crc decrypts with its CRC right)
        if is_nested and prev_ok and rec is not None and len(data) == 4 and data[0] in (0x60, 0x61) and int(rec['n_crc']) == 2:
            nested[i]['key_type'], nested[i]['block'] = data[0], data[1]
        t = (nested if is_nested else firsts)[i]
        if ok and int(t['key_type']) in (0x60, 0x61):
            found.setdefault((int(t['key_type']), int(t['block'])), key_bytes(r))
        prev_ok = ok
    return found


def recover_streams(frames_by_stream, device=0, reader_pairs=False, **cfg):
    """First AND nested authentications of several streams: `frames_by_stream` one api.NfcFrames (or None) per stream -> per stream the
    dict of label_auths.  ONE keys.recover call over all first authentications, ONE keys.recover_nested call over all nested ones (cfg:
    recover's), then label_auths per stream on the host.  reader_pairs (True, or a dict of recover_reader's own options, see
    reader_options): the first authentications that are left without a key -- no {at}, or a noise one -- are paired and searched
    besides (recover_reader_streams: ONE more call, the same cfg)."""
    firsts, nested = [], []
    for k, fr in enumerate(frames_by_stream):
        if fr is None:
            continue
        for find, parts in ((find_auths, firsts), (find_nested_auths, nested)):
            a = find(fr)
            a['stream'] = k
            parts.append(a)
    firsts = np.concatenate(firsts) if firsts else np.zeros(0, AUTH_DTYPE)
    nested = np.concatenate(nested) if nested else np.zeros(0, NESTED_DTYPE)
    first_results, _ = recover(firsts, device=device, **cfg)
    nested_results, _ = recover_nested(nested, device=device, **cfg)
    out = []
    for k, fr in enumerate(frames_by_stream):
        a, b = firsts['stream'] == k, nested['stream'] == k
        out.append(label_auths(fr, firsts[a], first_results[a], nested[b].copy(), nested_results[b]) if fr is not None and a.any() else {})
    if reader_pairs:
        parts = []
        for k, fr in enumerate(frames_by_stream):
            if fr is not None:
                a = find_reader_auths(fr)
                a['stream'] = k
                parts.append(a)
        out = recover_reader_streams(np.concatenate(parts) if parts else np.zeros(0, AUTH_DTYPE), out, device=device,
                                     **reader_options(reader_pairs, cfg))
    return out
