"""MIFARE Classic key recovery from sniffed first authentications (include/nfc_amd.h: nfc_find_auths, nfc_recover_keys_device,
nfc_host_recover_keys; csrc/keys.hip.h states the method, DESIGN.md 8h the layout).

``find_auths(frames)`` picks the first authentications out of one stream's frames, ``recover(traces)`` searches their keys on the GPU,
``host_recover(traces)`` is the same search on one CPU core.  Both return ``(results, stats)``: a KEY_RESULT_DTYPE record per trace and
the call's _lib.KeyStats.  There is no fall-back from one to the other."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (AUTH_DTYPE, KEY_RESULT_DTYPE, NFC_KEY_AMBIGUOUS, NFC_KEY_NONE, NFC_KEY_OK, NFC_KEY_OVERFLOW,  # noqa: F401
                   NFC_KEY_TIMING)


class KeyRecoveryError(RuntimeError):
    pass


def find_auths(frames):
    """The first authentications of one stream: `frames` an api.NfcFrames (NfcContext.frames(), NfcMultiFrames.frames_of(k),
    api.host_frames) -> AUTH_DTYPE records in stream order, `stream` 0."""
    L = _lib.load()
    t = np.ascontiguousarray(frames.table, _lib.RAW_FRAME_DTYPE)
    b = [np.ascontiguousarray(a, np.uint8) for a in frames.bytes]
    p = [np.ascontiguousarray(a, np.uint8) for a in frames.par]
    out = np.zeros(len(t) // 4 + 1, AUTH_DTYPE)   # (an authentication is four frames)
    n = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    rc = L.nfc_find_auths(ptr(t), len(t), ptr(b[0]), ptr(p[0]), ptr(b[1]), ptr(p[1]), out.ctypes.data, len(out), C.byref(n))
    if rc != 0:
        raise KeyRecoveryError('nfc_find_auths status %d' % rc)
    return out[:n.value]


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
