"""Drop-in for the reference's decoder module (decoder.py:15-33).

``decoder(src, dst, repeat, reader, tag, samp_rate, emulator)`` keeps the reference signature and
wiring: source -> envelope -> ``transition_sink(samp_rate, background.append, hi_val)`` with
``hi_val`` 1.1 for the UHD source (decoder.py:23) and 1.09 for a recording (decoder.py:29).

* With GNU Radio importable it is a ``gr.hier_block2`` built from the same blocks as the reference
  (``usrp_src`` / ``wavfile_source -> float_to_complex -> complex_to_mag_squared``), so
  ``usrp_nfc.py`` can ``self.connect(decoder(...))`` unchanged.
* Without GNU Radio (this image) ``src`` may be a 16-bit mono WAV path, a raw float32 file, a raw complex64 IQ
  file (``.fc32`` / ``.cfile`` / ``.iq``), a raw complex int16 IQ file (``.sc16`` / ``.cs16`` / ``.ci16``: what
  ``uhd_rx_cfile -s`` and ``rx_samples_to_file --type short`` record, I first), a raw complex int8 IQ file
  (``.cs8`` / ``.sc8`` / ``.ci8``: what ``hackrf_transfer -r`` records), a raw complex uint8 IQ file (``.cu8``: what
  ``rtl_sdr`` records), or a numpy array, and ``run()`` streams it through the GPU path offline: a real recording is
  squared like the reference's WAV branch (float_to_complex with Q = 0, then |.|^2), complex64 / interleaved IQ takes
  the UHD branch's |IQ|^2 -- complex int16 too (an int16 array of shape (n, 2)), converted on the GPU (``iq16_scale``),
  and complex int8 / uint8 (an int8 / uint8 array of shape (n, 2)), converted on the GPU (``iq8_scale``).
  ``dst`` (``usrp_nfc.py -o``): with an IQ source -- the stand-ins for the UHD branch, whose ``usrp_src`` writes its envelope to a
  16-bit mono WAV (usrp_src.py:35-37) -- ``run()`` also records the envelope |IQ|^2 to that WAV, converted on the GPU
  (``record_gain``; include/nfc_amd.h: nfc_record_pcm16_device) from the very buffer the batch is decoded from.  The file is what
  ``decoder(src=path)`` reads back.  With a recording as the source ``dst`` is ignored, as the reference ignores it
  (decoder.py:24-29 has no sink there).
"""
import wave

import numpy

from . import api
from . import keys as _keys
from .background import background
from .transition_sink import transition_sink

try:  # (GNU Radio is not in the build image: tests/test_gr_branch.py runs this branch against stand-ins)
    from gnuradio import blocks as _blocks
    from gnuradio import gr as _gr
except Exception:
    _gr = None
    _blocks = None


def _load_source(src, wav_scale, iq16_scale=0.0, iq8_scale=0.0):
    """-> (array, input_kind, i16_scale)"""
    if isinstance(src, numpy.ndarray):
        if src.dtype == numpy.complex64:
            return src.view(numpy.float32), api.NFC_IN_IQ_F32, 0.0
        if src.dtype == numpy.int16 and src.ndim == 2 and src.shape[1] == 2:   # complex int16, one row per sample
            return numpy.ascontiguousarray(src).reshape(-1), api.NFC_IN_IQ_I16, iq16_scale
        if src.dtype in (numpy.int8, numpy.uint8) and src.ndim == 2 and src.shape[1] == 2:   # complex int8 / uint8, one row per sample
            kind = api.NFC_IN_IQ_I8 if src.dtype == numpy.int8 else api.NFC_IN_IQ_U8
            return numpy.ascontiguousarray(src).reshape(-1), kind, iq8_scale
        if src.dtype == numpy.int16:
            return src, api.NFC_IN_I16_SQ, wav_scale
        return numpy.ascontiguousarray(src, numpy.float32), api.NFC_IN_REAL_F32_SQ, 0.0
    if str(src).lower().endswith('.wav'):
        w = wave.open(src, 'rb')
        try:
            if w.getnchannels() != 1 or w.getsampwidth() != 2:
                raise ValueError('expected a 16-bit mono WAV (usrp_src.py:36 writes those)')
            pcm = numpy.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
        finally:
            w.close()
        return pcm, api.NFC_IN_I16_SQ, wav_scale
    if str(src).lower().endswith(('.fc32', '.cfile', '.iq', '.c64')):   # raw interleaved complex64, as a UHD / file sink writes
        return numpy.fromfile(src, dtype=numpy.float32), api.NFC_IN_IQ_F32, 0.0
    if str(src).lower().endswith(('.sc16', '.cs16', '.ci16')):   # raw interleaved complex int16 (little-endian, I first)
        return numpy.fromfile(src, dtype='<i2').astype(numpy.int16, copy=False), api.NFC_IN_IQ_I16, iq16_scale
    if str(src).lower().endswith(('.cs8', '.sc8', '.ci8')):   # raw interleaved complex int8 (I first: a HackRF's samples)
        return numpy.fromfile(src, dtype=numpy.int8), api.NFC_IN_IQ_I8, iq8_scale
    if str(src).lower().endswith('.cu8'):   # raw interleaved complex uint8, offset binary (I first: an RTL-SDR's samples)
        return numpy.fromfile(src, dtype=numpy.uint8), api.NFC_IN_IQ_U8, iq8_scale
    return numpy.fromfile(src, dtype=numpy.float32), api.NFC_IN_REAL_F32_SQ, 0.0


def _hi_val(kind):
    """1.1 for IQ from the radio (the UHD branch, decoder.py:23), 1.09 for the WAV branch (decoder.py:29)."""
    return 1.1 if kind in _IQ_KINDS else 1.09


_IQ_KINDS = (api.NFC_IN_IQ_F32, api.NFC_IN_IQ_I16, api.NFC_IN_IQ_I8, api.NFC_IN_IQ_U8)
_SCALED_KINDS = (api.NFC_IN_I16_SQ, api.NFC_IN_IQ_I16, api.NFC_IN_IQ_I8, api.NFC_IN_IQ_U8)   # (the kinds i16_scale converts)
_RECORDED_KINDS = _IQ_KINDS + (api.NFC_IN_ENV_F32,)   # (the kinds `dst` records: the UHD branch's stand-ins and a ready envelope)


def _is_key(k):
    try:
        return len(k) == 6 and all(isinstance(v, (int, numpy.integer)) for v in k)
    except TypeError:
        return False


def _per_source_keys(keys, n):
    """decode_many's ``keys`` as one (key_a, key_b) or (key_a, key_b, table) per source."""
    one = lambda k: len(k) in (2, 3) and _is_key(k[0]) and _is_key(k[1])
    if one(keys):
        return [tuple(keys)] * n
    if len(keys) == n and all(one(k) for k in keys):
        return [tuple(k) for k in keys]
    raise ValueError('decode_many: keys is one (key_a, key_b) pair or (key_a, key_b, table) triple, or one of them per source')


def decode_many(sources, reader=True, tag=True, samp_rate=2e6, fsm_factory=None, keep=None, device=0, push_stats=None, frames=False, commands=False,
                keys=None, nested=False, emulate=None, reader_pairs=False, images=False, **sink_kwargs):
    """Decode many recordings at once: every source is a stream of one api.NfcMultiContext, a GPU lane each, one kernel launch per
    round of pieces (include/nfc_amd.h: nfc_multi) -- what a loop of ``decoder(src=s).run()`` does capture by capture.

    sources: paths or arrays as ``decoder(src=...)`` takes them, all of ONE input kind (mixed kinds raise ValueError).  hi_val is
    chosen as ``decoder`` chooses it.  sink_kwargs: ``lo_val`` / ``av_window`` / ``max_len`` (transition_sink's), ``wav_scale`` /
    ``iq16_scale`` / ``iq8_scale`` (decoder's), ``max_push_samples`` (default 2^18): the longest piece one stream gets per launch --
    longer captures are streamed in pieces.  fsm_factory: called once per source for its protocol machine (default: background's).
    After every push the streams' outputs come to the host in ONE fetch (api.NfcMultiContext.fetch: the packets, and the symbols
    unless ``keep`` is 0) and are delivered from that host copy.  push_stats: a list that gets one ``(n_fetches, n_reads_device)``
    per push, read from the context's statistics after the push's delivery (one fetch and no read from the device are expected).
    frames=True: after every push the streams' frames -- bytes, parity bits, parity and CRC_A verdicts, assembled on the GPU -- are
    fetched once more (api.NfcMultiContext.fetch_frames) and every source's part is appended to its background's ``frames``, a list
    with one api.NfcFrames per push that gave the source samples; the default leaves the backgrounds as they were.
    commands=True: the context tracks the commands on the GPU (api.NfcMultiContext.track_commands: the protocol machine, CRYPTO1
    included, a lane per source); after every push they are fetched once (fetch_commands) and every source's ``(table, data, enc)``
    -- what fsm.dispatch prints -- is appended to its background's ``commands``.  keys: ``(key_a, key_b)`` for all sources, or a list
    with one such pair per source (default: FF..FF); in place of a pair also a triple ``(key_a, key_b, table)``, `table` the sector keys
    as NfcMultiContext.set_sector_keys takes them ((key_type, sector) -> key).  Without the argument nothing changes.
    keys='recover': per group of sources one UNTRACKED pass first collects every source's frames across its pushes, ONE key recovery
    (usrp_nfc_amd.keys.recover) searches the keys of all their first authentications, the context is reset, every stream gets the first
    key found for type A and for type B (the default where none was found), and the tracked pass follows as above.  Every background
    gets ``recovered_keys``: (key_type, block) -> six key bytes.  The cost is the doubled push.
    nested=True (with keys='recover'): the nested authentications are searched too (usrp_nfc_amd.keys.recover_streams), and
    ``recovered_keys`` holds every sector key whose AUTH command could be decrypted and labelled.
    reader_pairs (with keys='recover'; True, or a dict of keys.recover_reader's own options): the first authentications the full search leaves without a key -- no {at}, or a noise
    one -- are paired and searched as reader pairs (usrp_nfc_amd.keys.recover_reader_streams), one more recovery call.
    emulate: a card per source (emulate.tag_card / reader_card; a list, None for a source that only listens; one card: for all) --
    every source's stream ANSWERS what it hears, on the GPU in the launch that decodes its commands (api.NfcMultiContext.emulate), and
    after every push each source's ``(records, plain, air, par)`` (NfcMultiAnswers.answers_of) is appended to its background's ``answers``.
    It implies the tracking of commands=True; give reader=/tag= so that a source decodes only the side it hears.
    With keys='recover' every stream gets ``first_keys(...)`` as its two keys AND ``keys.sector_table(recovered_keys)`` as its table
    (DESIGN.md 8j), so a card whose sectors have different keys is decrypted through every authentication whose key was found.  Two
    blocks of one sector with different keys: the lower block's is used and the others are the background's ``key_conflicts``, a dict
    (key_type, block) -> key (empty where there were none).
    images=True: the context also rebuilds every source's card from its commands on the GPU (api.NfcMultiContext.track_images, which
    implies the tracking; keys= are then allowed without commands=True) and, when a group is done, every background gets ``image``, an
    emulate.CardImage (None for a source that no group reached) -- ``image.card()`` is the tag to emulate, ``image.to_json(path)`` the reference's card file.  With
    keys='recover' the image is built in the tracked pass, which uses the recovered table.
    -> one ``background`` per source, in order: ``decode_many(srcs)[i].packets`` and its fsm's command trace are what
    ``decoder(src=srcs[i]).run()`` gives."""
    scales = {k: sink_kwargs.pop(k, 0.0) for k in ('wav_scale', 'iq16_scale', 'iq8_scale')}
    max_push = int(sink_kwargs.pop('max_push_samples', 1 << 18))
    sink = {k: sink_kwargs.pop(k) for k in ('lo_val', 'av_window', 'max_len') if k in sink_kwargs}
    if sink_kwargs:
        raise TypeError('decode_many: unexpected keyword arguments %s' % sorted(sink_kwargs))
    loaded = [_load_source(s, scales['wav_scale'], scales['iq16_scale'], scales['iq8_scale']) for s in sources]
    kinds = sorted(set(k for _, k, _ in loaded))
    if len(kinds) > 1:
        raise ValueError('decode_many: the sources are of different input kinds %s: decode each kind in a call of its own' % kinds)
    backs = [background(reader, tag, None, fsm=fsm_factory() if fsm_factory else None, keep=keep, samp_rate=samp_rate,
                        max_len=sink.get('max_len', 50), device=device, attached=True) for _ in loaded]
    if frames:
        for b in backs:
            b.frames = []
    if emulate is not None:   # a card per source (an emulate.Card, or None for a source that only listens), or one card for all
        cards = list(emulate) if isinstance(emulate, (list, tuple)) else [emulate] * len(loaded)
        if len(cards) != len(loaded):
            raise ValueError('decode_many: emulate is one card, or a list with one entry per source')
        for b in backs:
            b.answers = []
    if commands:
        for b in backs:
            b.commands = []
    if images:
        for b in backs:
            b.image = None
    per_source_keys = None
    recover = isinstance(keys, str) and keys == 'recover'
    if recover:
        if not (commands or images):
            raise ValueError('decode_many: keys are for commands=True')
        for b in backs:
            b.recovered_keys = {}
            b.key_conflicts = {}
    elif nested or reader_pairs:
        raise ValueError("decode_many: nested and reader_pairs are for keys='recover'")
    elif keys is not None:
        if not (commands or images):
            raise ValueError('decode_many: keys are for commands=True')
        per_source_keys = _per_source_keys(keys, len(loaded))
    if not loaded:
        return backs
    kind, scale = kinds[0], loaded[0][2]
    dt, per = api._KIND_DTYPE[kind]
    data = [numpy.ascontiguousarray(d, dtype=dt).reshape(-1) for d, _, _ in loaded]
    for g0 in range(0, len(data), 65536):   # (a context holds at most 65536 streams)
        group = data[g0:g0 + 65536]
        lens = numpy.array([len(d) // per for d in group], numpy.int64)
        starts = numpy.concatenate([[0], numpy.cumsum(lens)[:-1]]).astype(numpy.int64)
        piece = int(max(1, min(max_push, lens.max())))
        flat = numpy.concatenate([d[:n * per] for d, n in zip(group, lens)]) if lens.sum() else numpy.zeros(0, dt)
        buf = api.DeviceBuffer(flat, device, nbytes=max(16, flat.nbytes))
        try:
            with api.NfcMultiContext(len(group), piece, samp_rate=samp_rate, hi_val=_hi_val(kind), reader=reader, tag=tag, input_kind=kind,
                                     device=device, i16_scale=scale if kind in _SCALED_KINDS else 0.0, **sink) as m:
                if recover:
                    _recover_group_keys(m, buf, starts, lens, piece, backs[g0:g0 + len(group)], device, nested, reader_pairs)
                if commands or images:
                    m.track_commands(True)
                    if images:
                        m.track_images(True)
                    if recover:
                        for k, b in enumerate(backs[g0:g0 + len(group)]):
                            if b.recovered_keys:
                                m.set_keys(*_keys.first_keys(b.recovered_keys), stream=k)
                                table, b.key_conflicts = _keys.sector_table(b.recovered_keys)
                                m.set_sector_keys(table, stream=k)
                    if per_source_keys is not None:
                        mine = per_source_keys[g0:g0 + len(group)]
                        pairs, tables = [k[:2] for k in mine], [k[2] if len(k) == 3 else None for k in mine]
                        if all(numpy.array_equal(k, pairs[0]) for k in pairs):
                            m.set_keys(*pairs[0])
                        else:
                            for k in range(len(group)):
                                m.set_keys(*pairs[k], stream=k)
                        if all(t is tables[0] for t in tables):   # (no table anywhere: nothing is set and nothing allocated)
                            if tables[0] is not None:
                                m.set_sector_keys(tables[0])
                        else:
                            for k in range(len(group)):
                                if tables[k] is not None:
                                    m.set_sector_keys(tables[k], stream=k)
                if emulate is not None:   # (after the untracked recovery pass, which must not answer; implies tracking)
                    m.emulate(cards[g0:g0 + len(group)])
                done = numpy.zeros(len(group), numpy.int64)
                while True:
                    n = numpy.minimum(lens - done, piece)
                    if not n.any():
                        break
                    m.push_device(buf, starts + done, n)
                    done += n
                    m.fetch(api.NFC_MULTI_FETCH_PACKETS | (api.NFC_MULTI_FETCH_SYMBOLS if keep != 0 else 0), copy=False)
                    for k in numpy.nonzero(n)[0]:
                        backs[g0 + int(k)].deliver(m.stream(int(k)))
                    if frames:
                        fr = m.fetch_frames()
                        for k in numpy.nonzero(n)[0]:
                            backs[g0 + int(k)].frames.append(fr.frames_of(int(k)))
                    if commands:
                        cm = m.fetch_commands()
                        for k in numpy.nonzero(n)[0]:
                            backs[g0 + int(k)].commands.append(cm.commands_of(int(k)))
                    if emulate is not None:
                        an = m.fetch_answers()
                        for k in numpy.nonzero(n)[0]:
                            backs[g0 + int(k)].answers.append(an.answers_of(int(k)))
                    if push_stats is not None:
                        st = m.stats()
                        push_stats.append((int(st.n_fetches), int(st.n_reads_device)))
                if images:
                    im = m.fetch_images()
                    for k, b in enumerate(backs[g0:g0 + len(group)]):
                        b.image = im.image(k)
        finally:
            buf.free()
    return backs


def _joined_frames(parts):
    """[(NfcFrames, base), ...] of one stream's consecutive pushes as one NfcFrames: byte_offs moved behind each other, idx in the stream's
    whole sample count."""
    recs, data, par = [[], []], [[], []], [[], []]
    at = [0, 0]
    for fr, base in parts:
        for t in (0, 1):
            r = fr.records[t].copy()
            r['byte_off'] += at[t]
            r['idx'] += base
            at[t] += len(fr.bytes[t])
            recs[t].append(r), data[t].append(fr.bytes[t]), par[t].append(fr.par[t])
    cat = lambda xs, dt: numpy.concatenate(xs) if xs else numpy.zeros(0, dt)
    return api.NfcFrames([cat(recs[t], api.RAW_FRAME_DTYPE) for t in (0, 1)], [cat(data[t], numpy.uint8) for t in (0, 1)],
                         [cat(par[t], numpy.uint8) for t in (0, 1)])


def _recover_group_keys(m, buf, starts, lens, piece, backs, device, nested=False, reader_pairs=False):
    """The untracked pass of decode_many(keys='recover') over one group: every source's frames across its pushes, one recovery call for
    all of them, the context reset afterwards.  Fills every background's ``recovered_keys``."""
    parts = [[] for _ in backs]
    done = numpy.zeros(len(backs), numpy.int64)
    while True:
        n = numpy.minimum(lens - done, piece)
        if not n.any():
            break
        m.push_device(buf, starts + done, n)
        done += n
        fr = m.fetch_frames()
        for k in numpy.nonzero(n)[0]:
            parts[int(k)].append((fr.frames_of(int(k)), int(fr.base[k]) if len(fr.base) else 0))
    if nested:
        for b, found in zip(backs, _keys.recover_streams([_joined_frames(ps) if ps else None for ps in parts], device=device, reader_pairs=reader_pairs)):
            b.recovered_keys = found
        m.reset()
        return
    traces, reader_traces = [], []
    for k, ps in enumerate(parts):
        joined = _joined_frames(ps)
        for find, into in ((_keys.find_auths, traces),) + (((_keys.find_reader_auths, reader_traces),) if reader_pairs else ()):
            a = find(joined)
            a['stream'] = k
            into.append(a)
    traces = numpy.concatenate(traces) if traces else numpy.zeros(0, _keys.AUTH_DTYPE)
    results, _ = _keys.recover(traces, device=device)
    found_all = _keys.keys_by_stream(traces, results, len(backs))
    if reader_pairs and reader_traces:   # the sessions the full search left without a key, in pairs
        found_all = _keys.recover_reader_streams(numpy.concatenate(reader_traces), found_all, device=device, **_keys.reader_options(reader_pairs, {}))
    for b, found in zip(backs, found_all):
        b.recovered_keys = found
    m.reset()


if _gr is not None:

    class decoder(_gr.hier_block2):
        def __init__(self, src="uhd", dst=None, repeat=False, reader=True, tag=True, samp_rate=2e6, emulator=None):
            _gr.hier_block2.__init__(self, "decoder", _gr.io_signature(0, 0, 0), _gr.io_signature(0, 0, 0))
            if src == "uhd":
                import usrp_src   # the reference's own UHD source block (usrp_src.py)
                self._src = usrp_src.usrp_src(samp_rate=samp_rate, dst=dst)
                hi_val = 1.1
            else:
                self._wav = _blocks.wavfile_source(src, repeat)
                self._r2c = _blocks.float_to_complex(1)
                self._src = _blocks.complex_to_mag_squared(1)
                self.connect(self._wav, self._r2c, self._src)
                hi_val = 1.09
            self._back = background(reader, tag, emulator)
            self._trans = transition_sink(samp_rate, self._back.append, hi_val=hi_val)
            self.connect(self._src, self._trans)

else:

    class decoder(object):
        def __init__(self, src="uhd", dst=None, repeat=False, reader=True, tag=True, samp_rate=2e6, emulator=None,
                     wav_scale=0.0, fsm=None, batch=1 << 22, device=0, lo_val=0.1, av_window=2000, max_len=50, keep=None,
                     iq16_scale=0.0, iq8_scale=0.0, record_gain=32767.0, commands=False, keys=None):
            """commands=True: the context tracks the commands on the GPU (api.NfcContext.track_commands: the protocol machine, CRYPTO1
            included, a lane per transaction); after every batch they are read once and ``(table, data, enc)`` -- what fsm.dispatch
            prints -- is appended to the background's ``commands``, as decode_many(..., commands=True) does per file.  keys:
            ``(key_a, key_b)`` or ``(key_a, key_b, table)`` for the machine (default: FF..FF, no table).
            wav_scale: int16 PCM -> float.  0 (default): GNU Radio's wavfile_source normalisation, sample / 32767 (what the
            reference's WAV branch feeds the path, decoder.py:25; third party, unpinned: nfc_amd.h); > 0: sample * wav_scale.
            lo_val / av_window / max_len: transition_sink's keyword arguments (transition_sink.py:12), e.g. scaled with the rate.
            iq16_scale: complex int16 -> float, I and Q each, with wav_scale's meaning (0: / 32767; UHD's own sc16 -> fc32 scaling
            is third party and unpinned: nfc_amd.h).
            iq8_scale: complex int8 / uint8 -> float, I and Q each: sc8 q * s, cu8 (u - 127.5) * s with s = iq8_scale, or 2^-7 where
            it is not positive (the third-party 8-bit conversions are unpinned: nfc_amd.h).
            dst / record_gain: a 16-bit mono WAV that run() records the envelope to, pcm = round(envelope * record_gain) clamped to
            +-32767 (nfc_amd.h; 32767 is the inverse of wav_scale's default) -- IQ sources only, see the module's text."""
            if isinstance(src, str) and src == "uhd":
                raise RuntimeError('the UHD source needs GNU Radio + UHD; pass a recording or an array')
            data, kind, scale = _load_source(src, wav_scale, iq16_scale, iq8_scale)
            self._data = data
            self._per = 2 if kind in _IQ_KINDS else 1
            hi_val = _hi_val(kind)   # decoder.py:23 / :29
            self._back = background(reader, tag, emulator, fsm=fsm, keep=keep)
            self._trans = transition_sink(samp_rate, self._back.append, lo_val=lo_val, hi_val=hi_val, av_window=av_window, max_len=max_len,
                                          batch=batch, device=device, input_kind=kind, i16_scale=scale if kind in _SCALED_KINDS else 0.0)
            self._batch = int(batch)
            if keys is not None and not commands:
                raise ValueError('decoder: keys are for commands=True')
            self._commands = bool(commands)
            if self._commands:
                ctx = self._trans._ctx
                if keys is not None:
                    if len(keys) not in (2, 3) or not _is_key(keys[0]) or not _is_key(keys[1]):
                        raise ValueError('decoder: keys is a (key_a, key_b) pair or a (key_a, key_b, table) triple')
                    ctx.set_keys(keys[0], keys[1])
                    if len(keys) == 3:
                        ctx.set_sector_keys(keys[2])
                ctx.track_commands(True)
                self._back.commands = []
            self._dst = dst if (dst is not None and kind in _RECORDED_KINDS) else None
            self._rec = (kind, scale if kind in _SCALED_KINDS else 0.0, float(record_gain), int(device), samp_rate)

        def run(self):
            """Stream the source through the path (what ``tb.run()`` does in usrp_nfc.py:170)."""
            if self._dst is not None:
                return self._run_recording()
            step = self._batch * self._per
            for i in range(0, len(self._data), step):
                self._trans.push_now(self._data[i:i + step])
                self._keep_commands()
            return self._back

        def _keep_commands(self):
            if self._commands:
                self._back.commands.append(self._trans._ctx.commands().commands())

        def _run_recording(self):
            """run() with ``dst``: each batch is uploaded once, decoded from the device buffer (push_device) and converted to PCM by
            the record kernel from the same buffer; the PCM comes back and goes into the WAV."""
            from .record import record
            kind, scale, gain, device, samp_rate = self._rec
            data = numpy.ascontiguousarray(self._data, dtype=api._KIND_DTYPE[kind][0]).reshape(-1)
            step = self._batch * self._per
            wav = record(self._dst, samp_rate, gain, device)
            src = pcm = None
            try:
                nmax = min(step, len(data)) // self._per
                src = api.DeviceBuffer(numpy.zeros(0, data.dtype), device, nbytes=nmax * self._per * data.itemsize)
                pcm = api.DeviceBuffer(numpy.zeros(0, numpy.int16), device, nbytes=2 * nmax)
                for i in range(0, len(data), step):
                    piece = data[i:i + step]
                    n = len(piece) // self._per
                    if n == 0:
                        continue
                    src.upload(piece[:n * self._per])
                    self._trans.push_device_now(src, n)
                    self._keep_commands()
                    api.record_pcm16_device(src, n, pcm, kind, scale, gain, api.NFC_REC_ENVELOPE, device)
                    wav.write_pcm(pcm.download(2 * n).view(numpy.int16))
            finally:
                wav.close()
                for b in (src, pcm):
                    if b is not None:
                        b.free()
            return self._back

        @property
        def packets(self):
            return self._back.packets
