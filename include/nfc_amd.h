/*
 * nfc_amd.h -- C-ABI of the MI355X-native ISO-14443A IQ -> bit eavesdrop path.
 *
 * This is the drop-in boundary for the one hot path of giech/usrp_nfc:
 *
 *   envelope (gnuradio complex_to_mag_squared, decoder.py:27 / usrp_src.py:31)
 *   -> transition_sink   (transition_sink.py:10-125: gated running mean, lo/hi
 *                         ratio threshold with hysteresis, run-length timing)
 *   -> background router (background.py:30-52)
 *   -> miller_decoder / manchester_decoder (miller.py:13-197, manchester.py:13-61)
 *   -> PacketProcessor   (packets.py:57-98)
 *
 * The reference has no FFI of its own (it is pure Python on GNU Radio); the
 * functions below are what a ctypes binding placed inside the reference's
 * transition_sink.work()/background.append() would call.  INTEGRATION.md shows
 * that binding.  Plain C types only; every buffer is caller-allocated; every
 * function returns 0 on success or a negative nfc_status and leaves a message
 * for nfc_last_error().  A context is one stream; it is not thread-safe.  All
 * compute runs in hand-written HIP kernels on the selected device: there is no
 * CPU fallback, and nfc_create fails if no GPU is usable.
 */
#ifndef NFC_AMD_H
#define NFC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: nfc_stats grew (ran_ahead, redone_total, ring_slots_carried); i16_scale == 0 means sample / 32767 (GNU Radio's wavfile_source), not / 32768 */
/* 3: nfc_stats.reserved0 became decode_respeculated (same layout); the raw float32 envelope takes the fast threshold kernels */
/* 4: nfc_stats grew (device_allocs, tail_fused, chunks_rerun_in_place) */
/* (still 4, no structure changed: the input kinds NFC_IN_IQ_I16, NFC_IN_IQ_I8, NFC_IN_IQ_U8; nfc_record_pcm16_device, nfc_host_record_pcm16, nfc_record_tap) */
/* (still 4, only new types and functions: the multi-stream context nfc_multi, its configuration, statistics and functions) */
/* (still 4, only new names: nfc_multi_fetch, nfc_multi_fetched, nfc_multi_get_counts_all, NFC_MULTI_FETCH_*, NFC_MF_*; two reserved words
 *  of nfc_multi_stats are now n_fetches and n_reads_device, its size unchanged) */
/* (still 4, only new names: nfc_raw_frame, NFC_RAW_*, nfc_get_frame_counts, nfc_read_frames, nfc_read_frame_bytes, nfc_multi_frames,
 *  nfc_multi_fetch_frames, nfc_host_frames, nfc_fsm_process_frames) */
/* (still 4, only new names: nfc_fsm_state, NFC_FSM_*, NFC_CMD_CUT, nfc_fsm_state_init, nfc_fsm_get_state, nfc_fsm_set_state, nfc_host_commands,
 *  nfc_multi_commands, nfc_multi_track_commands, nfc_multi_fetch_commands, nfc_multi_set_keys, nfc_multi_get_fsm_state,
 *  nfc_multi_set_fsm_state) */
/* (still 4, only new names: nfc_auth_trace, nfc_key_result, nfc_key_config, nfc_key_stats, NFC_KEY_*, nfc_find_auths, nfc_host_recover_keys,
 *  nfc_recover_keys_device) */
/* (still 4, only new names: nfc_nested_trace, nfc_nested_result, nfc_nested_config, nfc_find_nested_auths, nfc_host_nested_candidates,
 *  nfc_nested_candidates_device, nfc_host_recover_nested_keys, nfc_recover_nested_keys_device) */
/* (still 4, only new names: nfc_fsm_key_table, NFC_KEY_SECTORS, nfc_sector_of_block, nfc_fsm_key_table_init, nfc_fsm_set_sector_key,
 *  nfc_fsm_get_key_table, nfc_fsm_set_key_table, nfc_host_commands_keyed, nfc_multi_set_sector_keys, nfc_multi_get_sector_keys;
 *  nfc_fsm_state.cur_key also takes 2 + slot of such a table, its layout unchanged) */
/* (still 4, only new names: nfc_emu_state, nfc_emu_card, nfc_emu_frame, nfc_emu_pair_result, nfc_emu_config, NFC_EMU_*, nfc_emu_state_init,
 *  nfc_emu_last_error, nfc_host_emu_step, nfc_host_emulate, nfc_emu_answer, nfc_host_emulate_pairs, nfc_emulate_pairs_device,
 *  nfc_multi_emulate, nfc_multi_fetch_answers, nfc_multi_answers, nfc_multi_get_emu_state, nfc_multi_set_emu_state) */
/* (still 4, only new names: nfc_air_frame, nfc_air_config, nfc_host_air_render, nfc_air_render_device) */
/* (still 4, only new names: nfc_reader_pair, nfc_reader_key_result, nfc_reader_key_config, NFC_RKEY_VERIFY_INLINE, nfc_find_reader_auths,
 *  nfc_host_recover_reader_keys, nfc_recover_reader_keys_device) */
/* (still 4, only new names: nfc_image_cmd, nfc_image_info, nfc_card_image, nfc_multi_images, NFC_IMG_*, nfc_card_image_init, nfc_host_card_image,
 *  nfc_multi_track_images, nfc_multi_fetch_images, nfc_multi_get_image, nfc_multi_set_image) */
#define NFC_AMD_ABI_VERSION 4

typedef enum {
    NFC_OK = 0,
    NFC_ERR_ARG = -1,      /* bad parameter */
    NFC_ERR_DEVICE = -2,   /* HIP runtime error / no device */
    NFC_ERR_NOMEM = -3,
    NFC_ERR_STATE = -4,    /* call sequence error */
    NFC_ERR_INTERNAL = -5  /* a kernel reported an impossible condition */
} nfc_status;

/* What one input sample is (replaces the source side of decoder.py:21-29). */
typedef enum {
    NFC_IN_IQ_F32 = 0,      /* interleaved float32 I,Q; x = fl(fl(I*I)+fl(Q*Q))  (uhd branch, usrp_src.py:31) */
    NFC_IN_ENV_F32 = 1,     /* float32 envelope already computed; x = sample                                    */
    NFC_IN_REAL_F32_SQ = 2, /* float32 real sample, Q = 0; x = fl(s*s)              (wav branch, decoder.py:25-28) */
    NFC_IN_I16_SQ = 3,      /* int16 PCM; s = fl(pcm / 32767) (or fl(pcm * i16_scale)); x = fl(s*s)  (wavfile_source + wav branch) */
    NFC_IN_IQ_I16 = 4,      /* complex int16 (sc16): two little-endian int16 per sample, I first -- std::complex<int16_t>, UHD's sc16
                             * host buffers, 4 bytes per sample.  I and Q converted as the PCM kind converts a sample (i16_scale), THEN
                             * x = fl(fl(I*I)+fl(Q*Q)) -- the fc32 kind's envelope of the converted pair, bit for bit.  UHD's own
                             * sc16 -> fc32 conversion (what cpu_format="fc32", usrp_src.py:19-22, runs on the host) is third party
                             * and absent from the reference tree: that scaling is UNPINNED, as wavfile_source's is */
    NFC_IN_IQ_I8 = 5,       /* complex int8 (sc8): two int8 per sample, I first -- std::complex<int8_t>, a HackRF's only format
                             * (hackrf_transfer -r, SoapySDR CS8) and UHD's sc8, 2 bytes per sample.  s = fl(q * scale) for I and Q
                             * each, THEN x = fl(fl(I*I)+fl(Q*Q)) -- the fc32 kind's envelope of the converted pair, bit for bit */
    NFC_IN_IQ_U8 = 6        /* complex uint8 (cu8): two offset-binary bytes per sample, I first -- what rtl_sdr records, 2 bytes per
                             * sample.  s = fl((u - 127.5f) * scale) (u - 127.5 is exact), THEN x as for sc8.  The offset is fixed.
                             * Both 8-bit kinds: scale from i16_scale, see there.  The third-party conversions of such captures --
                             * UHD's sc8 -> fc32, gr-osmosdr's HackRF source and its RTL-SDR source (which subtracts 127.4) -- are
                             * absent from the reference tree: they are UNPINNED, as wavfile_source's scaling is */
} nfc_input_kind;

/* nfc_params.flags */
#define NFC_FLAG_FORCE_SEQUENTIAL 1u /* run the exact one-lane sequential kernel for the threshold stage (slow; testing) */
#define NFC_FLAG_NO_EDGES 2u         /* stop after the threshold stage (val codes only; profiling)                      */

/* Constructor arguments of transition_sink (transition_sink.py:12) and background (background.py:17). */
typedef struct {
    double samp_rate;      /* samples per second; durations are reported as d * 1e6 / samp_rate microseconds */
    double lo_val;         /* 0.1  */
    double hi_val;         /* 1.1 for IQ input (decoder.py:23), 1.09 for the WAV branch (decoder.py:29) */
    int32_t av_window;     /* 2000 */
    int32_t max_len;       /* 50   */
    int32_t enable_reader; /* Modified-Miller decoder present (background.py:20) */
    int32_t enable_tag;    /* Manchester decoder present      (background.py:21) */
    int32_t input_kind;    /* nfc_input_kind */
    int32_t device;        /* HIP device ordinal */
    float i16_scale;       /* NFC_IN_I16_SQ and NFC_IN_IQ_I16 (each of I, Q).  0: GNU Radio's wavfile_source normalisation, s = fl((float)pcm / 32767.0f) -- what
                            * decoder.py:25 feeds the path (gr-blocks wavfile_source_impl.cc divides 16-bit samples by 0x7FFF; GNU Radio
                            * is third party and absent from the reference tree, so this boundary is UNPINNED: SURVEY.md 8c).  > 0: s =
                            * fl((float)pcm * i16_scale) for a source normalised differently (1/32768 is a power of two; 1/32767 is not:
                            * fl(s*s) then rounds differently near the thresholds).  NFC_IN_IQ_I16: at most 2^48 (NFC_ERR_ARG beyond),
                            * which keeps every envelope finite.  NFC_IN_IQ_I8 / NFC_IN_IQ_U8 (each of I, Q): a value that is not
                            * positive means 2^-7 (exact, NOT / 32767); at most 2^56 (NFC_ERR_ARG beyond: |I|, |Q| <= 2^7 scale keeps
                            * every envelope finite) */
    uint32_t flags;
    int32_t chunk_samples; /* samples per time chunk of the threshold kernel; 0 -> default */
    int32_t reserved;
} nfc_params;

/* One entry of the list transition_sink hands to its callback
 * (transition_sink.py:89-90,97): ((v, d*factor), t) plus the sample index at
 * which the reference appended it. 16 bytes. */
typedef struct {
    uint64_t idx; /* 0-based sample index in the whole stream */
    int32_t d;    /* duration in samples, 1..max_len */
    int8_t v;     /* -1, 0, 1, 2 */
    int8_t t;     /* cur_state - 1: -1 idle, 0 tag->reader, 1 reader->tag */
    int16_t pad;
} nfc_edge;

/* A packet as PacketProcessor.append_bit returns it (packets.py:67-79). */
typedef struct {
    uint64_t idx;     /* sample index of the edge whose symbol closed the packet */
    uint64_t bit_off; /* offset of its first bit in the per-type packet bit array of this batch */
    uint32_t n_bits;
    int32_t type;     /* 0 TAG_TO_READER, 1 READER_TO_TAG (packets.py:19-20) */
} nfc_packet;

typedef struct {
    uint64_t n_samples;    /* samples in the last batch */
    uint64_t n_edges;      /* transitions produced by the last batch */
    uint64_t n_symbols[2]; /* symbols handed to append_bit per packet type (0 tag, 1 reader) */
    uint64_t n_packets[2]; /* closed, non-empty packets per type */
    uint64_t n_packet_bits[2];
} nfc_counts;

typedef struct {
    double ms_total;          /* device time of the last batch, all kernels (hipEvent) */
    double ms_threshold;      /* envelope + threshold kernel launches of the last batch */
    double ms_edges;          /* run-length / edge extraction */
    double ms_decode;         /* Miller / Manchester / framing */
    uint32_t threshold_passes; /* launches of the threshold kernel (2 = speculate + verify) */
    uint32_t chunks_rerun;    /* chunks re-evaluated after the verify pass */
    uint32_t used_sequential; /* 1 if the exact sequential kernel ran */
    uint32_t n_chunks;
    uint64_t bytes_in;        /* input bytes of the last batch */
    double ms_threshold_kernel[6]; /* hipEvent duration of each k_threshold launch of the last batch (first 6) */
    uint32_t n_threshold_timed;
    uint32_t chunk_samples;   /* time-chunk length the threshold kernel used for the last batch (the nominal one: where the chunks
                               * are cut by dispatch row -- nfc_plan_row_cut -- they are up to 4 % longer or shorter, and n_chunks counts them) */
    uint32_t ran_ahead;       /* 1: the last batch's threshold stage ran ahead of the batch before it (nfc_submit_device) */
    uint32_t redone_total;    /* submitted batches of this context that had to be processed again synchronously */
    uint32_t ring_slots_carried; /* window slots whose value at the end of the last batch is still the one the batch started from
                                  * (no sample landing on them was accepted): 0 after a warm-up (nfc_prime + overlap) means the
                                  * window no longer depends on the level it was primed with */
    uint32_t decode_respeculated; /* batches of this context whose decode stage was repeated in the three-launch form because a tile of the
                                   * speculative form (a run-in of the predecessor tile's last edges instead of a scan over all tiles)
                                   * had assumed a decoder state that the check found wrong: a frame longer than the run-in */
    uint32_t device_allocs;   /* device / pinned buffers (re)allocated while the last batch was submitted and processed: 0 in the steady state
                               * of a stream -- the buffers are sized when a stream's first batch of a length is seen, with room for four
                               * times the transition density of a clean capture, so a stream that turns dense does not pay hipMalloc */
    uint32_t tail_fused;      /* always 0, kept for the layout: until its removal the test build's fused tail (one launch for the edge, decode and framing stages) set it */
    uint32_t chunks_rerun_in_place; /* ... of chunks_rerun: re-runs by the workgroup kernel in the form that evaluates a failed round in place
                                     * (up to a machine-full of failing chunks per round), the rest by the one-wave exact kernel */
} nfc_stats;

/* Everything a successor time chunk needs from its predecessor:
 * fixed header; the ring (av_window float32) follows in the caller's buffer.
 * PINNED TO THE REFERENCE after every push (tests/test_carried_state.py, against the oracle's own state): n_seen, ss bit for bit -- the
 * residue of sums that rounded included --, the ring bit for bit, filled, stable, cur_state, last_bit, dur, n_pending_bits and the pending
 * bits.  Excepted: miller_state and manch_state (a short batch stores a class representative of the decoder's state, which the
 * reference has no name for; the symbols and packets they lead to are pinned), pkt_started, and last_low (not carried, below). */
typedef struct {
    uint64_t n_seen;       /* samples consumed so far */
    double ss;             /* transition_sink._sum */
    int64_t last_low;      /* always -1, kept for the layout; ignored by nfc_set_state.  What a successor needs of the last LOW sample
                            * follows from cur_state, last_bit and dur: n_seen - 1 while last_bit is -1, n_seen - dur - 1 while
                            * cur_state is 2, and nothing once a run-length time-out has reset the state */
    int32_t filled;        /* transition_sink._filled */
    int32_t stable;        /* work has been rebound to work_stable */
    int32_t cur_state;     /* transition_sink._current_state */
    int32_t last_bit;      /* transition_sink._last_bit */
    int32_t dur;           /* transition_sink._dur */
    int32_t miller_state;  /* (stage, has_started, prev) packed: stage | started<<2 | prev<<3 */
    int32_t manch_state;   /* prev_set | (prev+1)<<1 */
    int32_t pkt_started[2];
    uint32_t n_pending_bits[2]; /* PacketProcessor._cur lengths (bits stay on the device) */
    int32_t av_window;
    int32_t reserved;
} nfc_state_header;

int nfc_abi_version(void);
int nfc_device_count(void);

typedef struct nfc_ctx nfc_ctx; /* opaque; one per stream */

int nfc_create(const nfc_params *params, nfc_ctx **out);
void nfc_destroy(nfc_ctx *ctx);
const char *nfc_last_error(const nfc_ctx *ctx); /* ctx may be NULL: message of the last failed nfc_create */

/* transition_sink.work(): consume n samples (any n >= 0, any chunking gives the
 * same concatenated outputs).  Host buffer: staged to the device first.
 * One call takes at most 2^30 samples (positions inside a batch are 32-bit: NFC_ERR_ARG beyond; push a longer capture in pieces,
 * the stream index itself is 64-bit). */
int nfc_push(nfc_ctx *ctx, const void *host_samples, size_t n);
/* Same, input already in device memory (16-byte aligned). */
int nfc_push_device(nfc_ctx *ctx, const void *dev_samples, size_t n);
/* Wait for the device; outputs of the last push are complete after it. */
int nfc_sync(nfc_ctx *ctx);
/* The decode and framing stages alone, for a caller that already has transitions (what background.append receives,
 * background.py:27-28: entries as nfc_read_edges returns them -- v, d in samples, t the route -1 / 0 / 1; idx only labels
 * the packets): Modified-Miller / Manchester decoding and packet framing on the GPU with the context's decoder and framing
 * state carried on, results through nfc_read_symbols / nfc_read_packets.  The threshold state is not touched. */
int nfc_push_edges(nfc_ctx *ctx, const nfc_edge *host_edges, size_t n);
/* Batches submitted ahead.  nfc_submit_device enqueues a batch and returns; nfc_wait completes the OLDEST submitted batch,
 * after which its outputs are read as after nfc_push_device -- valid until the next nfc_submit_device / nfc_wait / nfc_push*.
 * At most three batches may be in flight, so the steady state of a stream is
 *     submit(0); submit(1);  loop k: submit(k + 2); wait(k); read the outputs of k
 * and the threshold stage of batch k + 1 runs on the GPU beside the edge and decode stages of batch k (which need nothing of
 * it, and leave it most of the machine's issue slots), with batch k + 2's queued right behind it.  The input buffer of a submitted batch must stay untouched until
 * its nfc_wait returns.  Results are identical to nfc_push_device's: what runs ahead is checked in nfc_wait (certification
 * verdict, exactness guard, buffer capacities) and a batch that fails a check is processed again synchronously from the
 * state before it.  A batch that does not qualify (window not full yet, a short batch, state just set from the host, ...)
 * is simply processed inside its nfc_wait.  No other call that touches the stream state is accepted while batches are in
 * flight (NFC_ERR_STATE).  No reference counterpart: the reference is one synchronous work() call after another. */
int nfc_submit_device(nfc_ctx *ctx, const void *dev_samples, size_t n);
int nfc_wait(nfc_ctx *ctx);
int nfc_submitted(nfc_ctx *ctx); /* batches submitted and not yet waited for (0 .. 3) */
/* Enqueue this context's work on the caller's HIP stream (hipStream_t; NULL: back to the context's own), so that what the
 * caller enqueues there next -- a collective on the exported boundary states -- needs no host wait in between. */
int nfc_set_stream(nfc_ctx *ctx, void *stream);

/* Outputs of the LAST push (valid until the next push). */
int nfc_get_counts(nfc_ctx *ctx, nfc_counts *out);
/* The transitions of the batch (transition_sink.py:89-90,97).  On the device an entry is its batch-local sample position
 * (u32) and a 16-bit code; nfc_read_edges fetches those and builds the 16-byte records on the host.  A caller that can use
 * the compact form directly (6 bytes per entry over the link instead of 16) reads it with nfc_read_edges_compact:
 *   pos   sample index in the batch (stream index = n_seen before the push + pos)
 *   code  ((v + 1) * (max_len + 1) + d) | (t + 1) << 14     -- v, d, t as in nfc_edge
 * (not after nfc_push_edges, whose entries keep the caller's own indices). */
int nfc_read_edges(nfc_ctx *ctx, size_t first, nfc_edge *out, size_t cap, size_t *n_out);
int nfc_read_edges_compact(nfc_ctx *ctx, size_t first, uint32_t *pos_out, uint16_t *code_out, size_t cap, size_t *n_out);
/* symbols handed to CombinedPacketProcessor.append_bit(bit, type): 0/1 or an ErrorCode (utilities.py:7-14) */
int nfc_read_symbols(nfc_ctx *ctx, int type, size_t first, uint8_t *out, size_t cap, size_t *n_out);
/* closed packets of one type in stream order, and their bits (one byte per bit) */
int nfc_read_packets(nfc_ctx *ctx, int type, nfc_packet *out, size_t cap, size_t *n_out);
int nfc_read_packet_bits(nfc_ctx *ctx, int type, size_t first, uint8_t *out, size_t cap, size_t *n_out);
/* per-sample classification of the last batch (-1 LOW, 0 accepted, +1 HIGH); debugging tap */
int nfc_read_val(nfc_ctx *ctx, size_t first, int8_t *out, size_t cap, size_t *n_out);

/* Boundary state for multi-GPU time sharding / restart.  ring holds av_window floats, in slot order: ring[i] is the slot that
 * the samples with stream index = i (mod av_window) land on -- for a stream counted from 0 the reference's _buffer[i]; pending_bits holds the
 * open packets' bits (PacketProcessor._cur), type 0 first, hdr->n_pending_bits[0] + [1] bytes.  ring and
 * pending_bits may be NULL in nfc_get_state to query the header (and the sizes) only. */
int nfc_get_state(nfc_ctx *ctx, nfc_state_header *hdr, float *ring, size_t ring_cap, uint8_t *pending_bits,
                  size_t pending_cap);
int nfc_set_state(nfc_ctx *ctx, const nfc_state_header *hdr, const float *ring, size_t ring_len,
                  const uint8_t *pending_bits, size_t pending_len);
/* The same state written to DEVICE memory (16-byte aligned), asynchronously on the context's stream, for a
 * boundary exchange that goes GPU to GPU (RCCL all-gather straight from this buffer):
 *   [u32 len | 12 zero bytes | nfc_state_header | ring | pending bits]   len = bytes behind the 16-byte prefix.
 * When 16 + len exceeds cap only the prefix is written (the reader sees len and can ask again with room).
 * nfc_sync() before another stream or library reads the buffer. */
int nfc_export_state(nfc_ctx *ctx, void *device_dst, size_t cap, size_t *len_out);
/* Back to the state of a freshly created context (a new stream), keeping the device buffers. */
int nfc_reset(nfc_ctx *ctx);
/* Speculative start for a time shard that does not begin the stream (multi-GPU sharding): the
 * window full of `level` (the unloaded-carrier estimate), its exact sum, idle state machines, decoders reset,
 * n_seen = start_index.  Pushing an overlap that ends where the shard starts then converges to the true
 * boundary state.  No host-side ring: the window is filled on the device. */
int nfc_prime(nfc_ctx *ctx, uint64_t start_index, float level);

int nfc_get_stats(nfc_ctx *ctx, nfc_stats *out);
/* How much of nfc_stats' timing is collected.  Default 0: no events (the ms_* fields stay 0).  1: the threshold
 * kernels' own launch durations (ms_threshold_kernel), from start / stop events attached to the launches themselves.
 * 2: also ms_total and the per-stage split, from events recorded as markers between the kernels -- each marker costs
 * the stream a few microseconds. */
int nfc_set_timing(nfc_ctx *ctx, int level);

/* ---- "next" row f1: closed packets -> bytes -> commands, on the host -------------------------
 * and row f3: the CRYPTO1 sessions of MIFARE Classic (cipher.py, lfsr.py, fsm.py:133-154).
 * fsm.process_bits (fsm.py:218-238): frame-end repair (fsm.py:49-66), decryption while a session is up, odd-parity strip and
 * check (fsm.py:28-47), command lookup by protocol stage and leading bytes with CRC_A / BCC checks
 * (command.py:44-67,166-199; utilities.py:26-46), header / extra / CRC split (command.py:245-253), tag type and
 * UID tracking (fsm.py:165-216).  No device work here -- but the machine is ONE text, csrc/fsm.hip.h, for this host machine (a shell over
 * it with an unbounded UID: csrc/protocol.h), for nfc_host_commands and for k_multi_commands, a GPU lane per stream (below).  A packet is
 * assembled into a frame by the text the frame kernels run (csrc/frames.hip.h) and then goes the frame's way: nfc_fsm_process_packets and
 * nfc_fsm_process_frames give the same records, bytes and enc entries.  Behind a record's n_bytes / n_enc the rest of the frame's room
 * in bytes_out / enc_out is written too (with zeros): the capacities asked for below cover it. */
enum {
    NFC_CMD_UNKNOWN = -1,       /* bytes that match no command: CommandStructure("UNKNOWN", [], bytes) */
    NFC_CMD_PARITY_ERROR = -2   /* "PARITY ERROR" (fsm.py:225-227): no bytes, nothing dispatched */
};
enum {
    NFC_FRAME_EXTRA_ERROR = 1,      /* "EXTRA ERROR" (fsm.py:61) */
    NFC_FRAME_MANY_MORE_ERROR = 2,  /* "MANY MORE ERROR" (fsm.py:65) */
    NFC_FRAME_UID_MISMATCH = 4,     /* "MISMATCH BETWEEN READER-TAG UID" / "... READER_TAG UID#2" at a SEL2R (fsm.py:184,192) */
    NFC_FRAME_ENCRYPTED = 8,        /* a CRYPTO1 session was up: the frame was decrypted first (fsm.py:133-154) */
    NFC_FRAME_AR_OK = 16, NFC_FRAME_AR_ERROR = 32,   /* reader answer vs suc64(nt): "AR OK" / "ERROR WITH AR" (fsm.py:203-208) */
    NFC_FRAME_AT_OK = 64, NFC_FRAME_AT_ERROR = 128   /* tag answer vs suc96(nt) (fsm.py:209-214) */
};
typedef struct nfc_frame {
    int32_t cmd;       /* index for nfc_command_info, or NFC_CMD_* */
    int32_t type;      /* 0 tag -> reader, 1 reader -> tag */
    uint32_t byte_off; /* nfc_fsm_process_packets: offset of the frame's bytes in the byte buffer */
    uint16_t n_bytes, n_header, n_extra, n_crc; /* bytes = header | extra | crc */
    uint32_t flags;    /* NFC_FRAME_* */
    uint16_t n_enc;    /* entries written to enc_out for this frame (what fsm._print_enc shows) */
    uint16_t pad;
} nfc_frame;
typedef struct nfc_command_info {
    char name[8];
    int32_t stage, type, crc, n_header, n_extra, xor_check;
    uint8_t header[2];
    uint8_t pad[2];
} nfc_command_info;
typedef struct nfc_fsm nfc_fsm; /* protocol state across packets: previous command, tag type, UID */

int nfc_fsm_create(nfc_fsm **out);
void nfc_fsm_destroy(nfc_fsm *f);
int nfc_fsm_reset(nfc_fsm *f);
/* one packet's bits (as nfc_read_packet_bits returns them); bytes_out needs n_bits / 9 + 1 bytes.  NFC_ERR_ARG also for a packet of
   2^32 bits or more (an nfc_packet counts its bits in 32) */
int nfc_fsm_process(nfc_fsm *f, const uint8_t *bits, size_t n_bits, int packet_type, nfc_frame *out, uint8_t *bytes_out,
                    size_t bytes_cap, uint16_t *enc_out /* NULL, or the same capacity: on-air byte | 0x100 if marked '!' */);
/* fsm.process_outgoing (fsm.py:68-112, wired at packets.py:88-90 as the emulator's encoder hook): a frame an emulator is about to
   send, bits with parity as the encoders take them; the machine follows it (tag type from an ATQA, the command in flight) and,
   while a MIFARE Classic session is up, encrypts it into bits_out (n_bits entries).  Returns 0, or 1 when the tag is an Ultralight:
   nothing was written, and the reference runs the frame through process_bits instead (the Python fsm does). */
int nfc_fsm_process_outgoing(nfc_fsm *f, const uint8_t *bits, size_t n_bits, int cmd, uint8_t *bits_out);
/* MIFARE Classic sector keys A / B (fsm.set_keys, fsm.py:157-160; both default to FF FF FF FF FF FF) */
int nfc_fsm_set_keys(nfc_fsm *f, const uint8_t key_a[6], const uint8_t key_b[6]);
/* a batch of packets in stream order: the rows of nfc_read_packets (both types merged by idx) over their bit arrays */
int nfc_fsm_process_packets(nfc_fsm *f, const nfc_packet *packets, size_t n_packets, const uint8_t *bits_type0,
                            const uint8_t *bits_type1, nfc_frame *frames_out, uint8_t *bytes_out, size_t bytes_cap,
                            size_t *bytes_used, uint16_t *enc_out /* NULL, or bytes_cap entries, indexed like bytes_out */);
int nfc_command_count(void);
int nfc_command_get(int cmd, nfc_command_info *out);
/* ISO 14443-3 type A CRC (utilities.py:30-41), low byte first */
int nfc_crc_a(const uint8_t *data, size_t n, uint8_t out[2]);

/* ---- "next" row f4: the transmit side as a device-side signal generator -------------------------
 * encode_bits of miller_encoder / manchester_encoder / binary_src.encoder (miller.py:200-233, manchester.py:64-79,
 * binary_src.py:17-20) on the host; binary_src.work (binary_src.py:64-103: int(dur * samp_rate / 1e6) samples per run,
 * complex64 level + 0j) and multiplier (multiplier.py:18-22: times A exp(j 2 pi f k / samp_rate)) as one kernel. */
typedef struct {
    int32_t level;  /* 0 / 1; 2 = binary_src's "temporary pause" marker (no samples) */
    int32_t pad;
    double dur_us;
} nfc_tx_run;
enum { NFC_TX_SAME = 0, NFC_TX_MANCHESTER = 1, NFC_TX_MILLER = 2 };
int nfc_tx_encode(int encoding, const uint8_t *bits, size_t n_bits, nfc_tx_run *out, size_t cap, size_t *n_out);
/* samples binary_src.work produces for the runs */
int nfc_tx_sample_count(const nfc_tx_run *runs, size_t n_runs, double samp_rate, uint64_t *n_samples);
/* renders the runs into dev_out (complex64, 32-byte aligned, cap_samples entries); carrier != 0 multiplies by the carrier,
 * sample k of this call having carrier index first_index + k.  kernel_ms (may be NULL): the kernel's duration by HIP events.
 * The carrier's phase is kept in 64-bit fixed point and its top 24 bits go into sincospif: a phase error of at most 3.7e-7 rad,
 * 1.5e-7 of the amplitude.  The reference's carrier is GNU Radio's sig_source_c -- third party, not under the reference tree:
 * parity at that boundary is unpinned (tx.hip.h states the arithmetic; tests/test_tx.py checks it against a float64
 * restatement within that tolerance). */
int nfc_tx_render_device(int device, const nfc_tx_run *runs, size_t n_runs, double samp_rate, int carrier, double freq,
                         float amp, uint64_t first_index, void *dev_out, size_t cap_samples, size_t *n_samples,
                         float *kernel_ms);

/* ---- recording: a float per sample -> 16-bit PCM on the device ---------------------------------------------------
 * What the reference writes through GNU Radio's wavfile_sink (16 bits, one channel): usrp_src.py:35-37 records the envelope
 * |IQ|^2 of the live capture (decoder(src="uhd", dst=path), usrp_nfc.py -o) -- the recording decoder(src=path) reads back --
 * and record.py:10-19 the real part of a complex stream (what the emulators transmit, usrp_nfc.py:59-60,95-96).
 * THE CONVERSION, for a float32 value x and a float32 gain, in this order:
 *   1. v = fl(x * gain): one float32 product (no contraction);
 *   2. NaN becomes 0;
 *   3. v is clamped to [-32767, 32767] (so +-Inf become +-32767);
 *   4. v is rounded to the nearest integer, halves away from zero (lroundf, exactly: 0.49999997 gives 0);
 *   5. the result is stored as little-endian int16.
 * gain must be finite and > 0 (NFC_ERR_ARG otherwise); 32767 is the inverse of NFC_IN_I16_SQ's default i16_scale = 0 (/ 32767).
 * Modelled on gr-blocks' wavfile_sink for 16 bits (times 0x7FFF, clamp to +-0x7FFF, round to nearest); GNU Radio is third party
 * and absent from the reference tree, so this boundary is UNPINNED, as wavfile_source's is.
 * x comes from one of two taps: */
typedef enum {
    NFC_REC_ENVELOPE = 0, /* the envelope the threshold kernels compute for input_kind and i16_scale (any nfc_input_kind; i16_scale as in
                           * nfc_params, with the same limits and NFC_ERR_ARG beyond them) */
    NFC_REC_REAL_PART = 1 /* the real part of an interleaved complex64 sample (complex_to_real, record.py:18): NFC_IN_IQ_F32 only,
                           * NFC_ERR_ARG with any other kind */
} nfc_record_tap;
/* Converts n samples at dev_samples (device memory, of input_kind) into n int16 at dev_pcm_out (device memory); both 16-byte
 * aligned (NFC_ERR_ARG otherwise).  No context: like nfc_tx_render_device.  stream == NULL: the result is complete when the call
 * returns.  A stream of nfc_stream_create: the kernel is only enqueued there and nfc_stream_sync completes it.  kernel_ms (NULL, or
 * the kernel's duration by HIP events) implies the wait.  n == 0 succeeds and does nothing; n > 2^30 is NFC_ERR_ARG (nfc_push's
 * per-call limit).  Every argument is checked before the device is touched.  Nothing is written beyond dev_pcm_out[n). */
int nfc_record_pcm16_device(int device, int tap, int input_kind, float i16_scale, const void *dev_samples, size_t n,
                            float gain, void *dev_pcm_out /* n int16 */, void *stream /* hipStream_t or NULL */,
                            float *kernel_ms /* NULL, or the kernel's duration by HIP events */);
/* steps 1-5 above on the host: the twin of the kernel's conversion, as nfc_host_i16_to_float is of the PCM kind's */
int16_t nfc_host_record_pcm16(float x, float gain);

/* ---- many independent streams in one launch: a lane per stream ------------------------------------------------------
 * A context (nfc_ctx) is one stream, and its kernels make one LONG stream fast.  A caller with many SHORT streams -- a directory of
 * recorded transactions, a rack of SDR channels that each deliver a few thousand samples per scheduler call -- pays a context's whole
 * launch sequence per stream and push.  nfc_multi holds K streams that share one nfc_params and carries every stream's state across
 * pushes; one push hands every stream its next piece, and ONE kernel launch walks them all, a GPU lane per stream running
 * transition_sink.py:55-99 literally (the fp64 window sum in the reference's own order), the routed decoder and the packet framing.
 * The reference has no counterpart (one flowgraph, one stream).  A push lasts as long as the longest stream's lane, however many
 * streams there are: measured with captures of 32 768 samples (README.md) it LOSES against a loop over an nfc_ctx at 64 streams (2 x
 * slower), wins 7 x at 1 024 and 51 x at 16 384, and pays from about 130 streams on (interpolated between those runs).
 *
 * PARITY.  After any sequence of pushes, stream k's outputs of the last push -- counts, edges with the 64-bit stream index in idx,
 * symbols per type, packets, packet bits -- and its state (the nfc_get_state triple) equal those of an nfc_ctx with the same
 * nfc_params after an nfc_push of the same samples; an nfc_ctx is in turn pinned to the reference, its outputs and -- after every push,
 * with the exceptions named at nfc_state_header -- its state; so is a stream's state here, directly (tests/test_carried_state.py).  The fill phase may span pushes.
 * n[k] == 0 leaves stream k untouched and its outputs empty.  A state exported here and imported into an nfc_ctx (or the other way)
 * continues identically.
 * INPUT.  All seven nfc_input_kinds, i16_scale and its limits as in nfc_create.  dev_base is 16-byte aligned; first_sample[k] is
 * arbitrary (a stream's start has the alignment of one sample, no more); the ranges of different streams may overlap.
 * REJECTED, with NFC_ERR_ARG, before the device is touched, the offending name in the message: a non-zero nfc_params.flags or
 * chunk_samples; n_streams or max_push_samples out of range; n[k] > max_push_samples; non-zero reserved fields; a cap_* above 2^26
 * entries (four times what the longest push can produce of anything).  Device memory the configuration cannot get: NFC_ERR_NOMEM.
 * CAPACITIES.  Outputs go to per-stream slabs sized at create, so a push never fails because a stream produced more than its slab
 * holds: the counts are the true totals, what is stored (and read) is the first cap_* entries, the stream's flag bits say which array
 * was cut, nfc_multi_stats.n_streams_truncated counts such streams, and the stream's carried state has advanced exactly -- it does
 * not depend on what was stored.  Defaults (a 0 in the configuration): max_push_samples / 4 + 64 edges, as many symbols per type and
 * packet bits per type, max_push_samples / 16 + 16 packets per type -- twice the densest capture of this tree's generators.  An open
 * packet longer than cap_pending_bits sets NFC_MULTI_PENDING_OVERFLOW on the stream: its packets are undefined until it is reset;
 * no other stream is affected.
 * There is no CPU fallback: create fails without a GPU.  The product build reads no environment variable.  Not thread-safe. */
typedef struct nfc_multi nfc_multi;            /* K streams, one parameter set; not thread-safe */
typedef struct {
    uint32_t n_streams;          /* 1 .. 65536 */
    uint32_t max_push_samples;   /* longest piece ONE stream gets in one push: 1 .. 2^24 */
    uint32_t cap_edges, cap_symbols, cap_packets, cap_packet_bits;  /* per stream and push; 0: default from max_push_samples */
    uint32_t cap_pending_bits;   /* bits of an open packet carried per stream; 0: 4096 */
    uint32_t reserved[9];        /* must be 0 */
} nfc_multi_config;              /* 64 bytes */
enum { NFC_MULTI_TRUNC_EDGES = 1, NFC_MULTI_TRUNC_SYMBOLS = 2, NFC_MULTI_TRUNC_PACKETS = 4, NFC_MULTI_TRUNC_BITS = 8,
       NFC_MULTI_PENDING_OVERFLOW = 16 /* sticky until the stream is reset */ };
typedef struct {
    double ms_kernels; uint64_t n_samples, bytes_in;
    uint32_t n_launches, n_streams_truncated;   /* of the push (a fetch does not touch them) */
    uint32_t n_fetches, n_reads_device;         /* since the last push: nfc_multi_fetch calls that succeeded; reader calls that went to the device */
    uint32_t reserved[6];
} nfc_multi_stats;               /* 64 bytes */

int  nfc_multi_create(const nfc_params *p, const nfc_multi_config *c, nfc_multi **out);
void nfc_multi_destroy(nfc_multi *m);
const char *nfc_multi_last_error(const nfc_multi *m);   /* m may be NULL: message of the last failed create */
/* stream k consumes n[k] samples (0 allowed) that start first_sample[k] SAMPLES behind dev_base; n and first_sample are host arrays of n_streams */
int nfc_multi_push_device(nfc_multi *m, const void *dev_base, const uint64_t *first_sample, const uint32_t *n);
int nfc_multi_push(nfc_multi *m, const void *const *host_ptrs, const uint32_t *n);   /* staged to the device, then the same */
/* Outputs of the LAST push, per stream; the readers return what the slab stores (at most cap_* entries, see CAPACITIES).  Each read is a
 * copy from the device and a wait, unless an nfc_multi_fetch (below) since the push covers the array: then it is host memory. */
int nfc_multi_get_counts(nfc_multi *m, uint32_t stream, nfc_counts *out, uint32_t *flags_out);
int nfc_multi_read_edges(nfc_multi *m, uint32_t stream, size_t first, nfc_edge *out, size_t cap, size_t *n_out);
int nfc_multi_read_symbols(nfc_multi *m, uint32_t stream, int type, size_t first, uint8_t *out, size_t cap, size_t *n_out);
int nfc_multi_read_packets(nfc_multi *m, uint32_t stream, int type, nfc_packet *out, size_t cap, size_t *n_out);
int nfc_multi_read_packet_bits(nfc_multi *m, uint32_t stream, int type, size_t first, uint8_t *out, size_t cap, size_t *n_out);
/* every stream's counts (and flags) of the last push in one call: the loop of nfc_multi_get_counts over host memory, no device work */
int nfc_multi_get_counts_all(nfc_multi *m, nfc_counts *out /* n_streams */, uint32_t *flags_out /* n_streams, may be NULL */);

/* ---- the fetch: every stream's outputs of the last push packed on the GPU, ONE copy to the host --------------------------------
 * A reader call above is a copy from the stream's slab row and a wait: a round trip per stream and array.  nfc_multi_fetch compacts what
 * EVERY stream stored in the last push into one packed device buffer (two kernel launches: a scan of the stored amounts, a gather of
 * the slab rows), brings that buffer to pinned host memory in one copy, and hands out pointers into it.  Until the next push the
 * readers above then serve the arrays the fetch covered from that host copy -- the same first / cap / n_out semantics, the same
 * bytes, no device call -- and take the device path (counted in nfc_multi_stats.n_reads_device) for arrays it did not cover.
 * STORED AMOUNT.  Stream k's part of an array is exactly what its reader returns with first = 0 and unlimited cap: min(count, cap_*)
 * entries (the bit rows: what nfc_multi_read_packet_bits returns).  A truncated stream contributes its stored prefix, a stream that
 * got n[k] == 0 in the push (or was reset since) nothing.
 * PACKING.  Tight, at entry granularity, no padding between streams: off[a] (n_streams + 1 entries) is the exclusive prefix of the
 * stored amounts of array a, stream k's entries are [off[a][k], off[a][k + 1]).  Arrays `what` does not ask for are empty: their off
 * is all zero and their pointers may be NULL (they are NULL too when no stream stored anything: n_launches == 0, nothing copied).
 * NFC_MULTI_FETCH_PACKETS stands for the packet tables AND the bit arrays of both types.
 * EDGES come as the two arrays the slabs hold: edge idx = base[k] + edge_pos, code & 0x3FFF = (v + 1) * edge_code_nd + d,
 * code >> 14 = t + 1 -- v, d, t as in nfc_edge.  packets[t] are nfc_packet records exactly as nfc_multi_read_packets gives them:
 * idx in the stream's own count of samples, bit_off relative to the stream's own part of packet_bits[t].
 * LIFETIME.  Every pointer in nfc_multi_fetched refers to pinned host memory owned by the context and is valid until the next
 * nfc_multi_push / _push_device, nfc_multi_fetch, nfc_multi_reset (of any stream), nfc_multi_set_state or nfc_multi_destroy of that
 * context; each of those also ends the readers' use of the host copy.
 * ERRORS.  what == 0 or bits outside NFC_MULTI_FETCH_ALL: NFC_ERR_ARG naming `what`; no completed push: NFC_ERR_STATE; buffers that
 * cannot be had: NFC_ERR_NOMEM, the context and its slabs intact (the readers go on from the device); totals of the device's scan that
 * differ from the host's: NFC_ERR_INTERNAL.  The buffers are sized from the amounts stored (grown geometrically), never for the
 * capacities.
 * COST, measured with captures of 32 768 samples (README.md, profiles/multi_fetch_bench.json): at 16 384 streams a fetch of everything
 * copies 271.4 MB (14.3 % of the slabs' room) in 7.09 ms, its two kernels taking 0.534 ms; reading every stream's packets costs 140.7 us per
 * stream from the device, 94.2 us through the per-stream Python view after a fetch and 56.5 us through NfcMultiFetch.packets_all(). */
enum { NFC_MULTI_FETCH_EDGES = 1, NFC_MULTI_FETCH_SYMBOLS = 2, NFC_MULTI_FETCH_PACKETS = 4 /* tables AND bit arrays, both types */,
       NFC_MULTI_FETCH_ALL = 7 };
enum { NFC_MF_EDGES = 0, NFC_MF_SYM0, NFC_MF_SYM1, NFC_MF_PK0, NFC_MF_PK1, NFC_MF_BITS0, NFC_MF_BITS1, NFC_MF_ARRAYS = 7 };
typedef struct {
    uint32_t what, n_streams;
    uint32_t edge_code_nd;               /* code & 0x3FFF = (v + 1) * nd + d, code >> 14 = t + 1 (edges.hip.h: edge_code) */
    uint32_t n_launches;                 /* of this fetch: 0 when nothing was stored at all */
    const uint64_t *off[NFC_MF_ARRAYS];  /* n_streams + 1 entries each: stream k's entries are [off[a][k], off[a][k+1]) of array a */
    const uint64_t *base;                /* n_streams: stream index of the push's first sample (edge idx = base[k] + pos) */
    const uint32_t *edge_pos;            /* batch-local sample position */
    const uint16_t *edge_code;
    const uint8_t  *symbols[2];
    const nfc_packet *packets[2];        /* exactly what nfc_multi_read_packets gives: bit_off relative to the stream's own bit row */
    const uint8_t  *packet_bits[2];
    uint64_t bytes_copied;               /* device -> host, of this fetch */
    double ms_kernels;                   /* with nfc_multi_set_timing(on): the fetch's launches by HIP events; else 0 */
    uint64_t reserved[4];
} nfc_multi_fetched;
int nfc_multi_fetch(nfc_multi *m, uint32_t what, nfc_multi_fetched *out /* may be NULL */);

/* ---- frames assembled on the GPU: closed packets -> bytes, parity verdict, CRC_A --------------------------------------------
 * The bit-level, packet-parallel part of fsm.process_bits, per closed non-empty packet: the frame-end repair (fsm.py:49-66), nine
 * bits to a byte plus the odd-parity check (fsm.py:28-47) and the ISO 14443-3 CRC_A (utilities.py:30-41).  Two kernel launches
 * (csrc/frames.hip.h, nfc_frames.hip): a scan over the packet closes gives every frame its place, then a lane per frame reads its
 * nine-bit fields from the bit array the decode stage left (packed 32 to a word, or a byte per bit) and writes the record, the bytes
 * and the parity bits.  Behind them the sequential protocol machine: nfc_fsm_process_frames on the host, or on the GPU -- for the many
 * streams of an nfc_multi a lane per stream (nfc_multi_fetch_commands below), for this one stream a lane per transaction
 * (nfc_track_commands / nfc_read_commands below).
 * REPAIR, with rem = n_bits % 9 and start_bit = (type == 0 ? 1 : 0):
 *   rem 0: nothing;  rem 8: the last byte's parity bit is start_bit;  rem 1: the last bit is dropped, NFC_FRAME_EXTRA_ERROR iff it
 *   differs from start_bit;  rem 2..7: rem bits are dropped, NFC_FRAME_MANY_MORE_ERROR.
 * bytes[type]: eight data bits, least significant first; par[type]: the ninth bit as received, a byte each; both indexed by byte_off.
 * They are stored for EVERY frame, parity errors included: a CRYPTO1 session checks parity after decryption and needs the on-air bits.
 * NFC_RAW_PARITY_OK: n_bytes > 0 and no byte has popcount(byte) & 1 == par (the negation of fsm.py:224-228's "PARITY ERROR");
 * NFC_RAW_CRC_A_OK: parity holds and the last two bytes are the CRC_A of those before them;
 * NFC_RAW_CUT (multi-stream only): the stream's bit slab was truncated before this packet's end: n_bytes is 0, nothing is written. */
enum { NFC_RAW_PARITY_OK = 0x100, NFC_RAW_CRC_A_OK = 0x200, NFC_RAW_CUT = 0x400 };  /* beside NFC_FRAME_EXTRA_ERROR (1), NFC_FRAME_MANY_MORE_ERROR (2): same values, same meaning */
typedef struct nfc_raw_frame {     /* 32 bytes; one per closed, non-empty packet, in the packet table's order */
    uint64_t idx;                  /* nfc_packet.idx */
    uint32_t byte_off;             /* first byte in bytes[type] / par[type] */
    uint32_t n_bits;               /* nfc_packet.n_bits, before the repair */
    uint32_t n_bytes;              /* after the repair: (n_bits + 1) / 9 when n_bits % 9 == 8, else n_bits / 9; may be 0 */
    uint32_t flags;
    int32_t  type;
    uint32_t reserved;             /* 0 */
} nfc_raw_frame;
/* Single context.  Assembly is lazy, like the symbol arrays: the first of these calls after a batch launches the two kernels on the
 * context's stream; a batch whose frames nobody reads launches nothing.  Valid exactly where nfc_read_packets is (after nfc_push_edges
 * too); NFC_ERR_STATE with no completed batch.  n_frames[t] == nfc_counts.n_packets[t].  Copies go through pinned staging. */
int nfc_get_frame_counts(nfc_ctx *ctx, uint64_t n_frames[2], uint64_t n_bytes[2]);
int nfc_read_frames(nfc_ctx *ctx, int type, nfc_raw_frame *out, size_t cap, size_t *n_out);
int nfc_read_frame_bytes(nfc_ctx *ctx, int type, size_t first, uint8_t *bytes_out, uint8_t *par_out /* may be NULL */, size_t cap, size_t *n_out);
/* The kernels' twin on the CPU (no GPU needed): the frames of n packets of ONE type (rows of nfc_read_packets; a row of another type is
 * NFC_ERR_ARG) over that type's bit array, a byte per bit.  out: n records; bytes / par: cap entries each (NFC_ERR_ARG when the frames
 * need more); *used: entries written. */
int nfc_host_frames(const nfc_packet *packets, size_t n, const uint8_t *bits, int type, nfc_raw_frame *out, uint8_t *bytes, uint8_t *par,
                    size_t cap, size_t *used);
/* nfc_fsm_process_packets over frames: `frames` holds both types merged by idx, as the rows of nfc_fsm_process_packets are; its outputs
 * and the machine's state afterwards are IDENTICAL to nfc_fsm_process_packets on the packets the frames came from, through CRYPTO1
 * sessions and nested authentications.  Outside a session it uses the assembled bytes and the parity and CRC verdicts; inside one
 * it decrypts bytes and par -- the route nfc_fsm_process takes once it has assembled its packet.  A frame with NFC_RAW_CUT is
 * NFC_ERR_ARG (its bits are not there), and so is one whose n_bytes exceeds n_bits / 9 + 1: all n_bytes entries of the frame's
 * room in bytes_out / enc_out are written, and that is the room the capacity check reserves. */
int nfc_fsm_process_frames(nfc_fsm *f, const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0,
                           const uint8_t *bytes1, const uint8_t *par1, nfc_frame *frames_out, uint8_t *bytes_out, size_t bytes_cap,
                           size_t *bytes_used, uint16_t *enc_out);
/* Multi-stream: the scan, the assembly of every stream's frames into ONE packed buffer, one copy and one wait.  Stream k's frames of
 * type t are frames[t][frame_off[t][k] .. frame_off[t][k + 1]) and its bytes bytes[t] / par[t][byte_off[t][k] .. byte_off[t][k + 1]);
 * a frame's byte_off is relative to the stream's own part, its idx is in the stream's own sample count (base[k] added on the host).
 * A stream contributes the packets its slab stores (at most cap_packets); a frame whose bits the slab cut carries NFC_RAW_CUT.
 * The call owns its buffers: it does not end the lifetime of an nfc_multi_fetch's pointers or the readers' host copy, and the reverse
 * holds too; nfc_multi_fetch, NFC_MULTI_FETCH_ALL and nfc_multi_stats are untouched.  The pointers live until the next nfc_multi_push /
 * _push_device, nfc_multi_fetch_frames, nfc_multi_reset, nfc_multi_set_state or nfc_multi_destroy.  No completed push: NFC_ERR_STATE;
 * nothing stored: no launch and no copy (n_launches == 0, NULL arrays); device totals that differ from the host's: NFC_ERR_INTERNAL.
 * COST, measured with captures of 32 768 samples (README.md, profiles/frames_bench.json): at 16 384 streams the call and a vectorised
 * CRC mask cost 0.105 us per capture (16.65 MB copied, the two kernels 0.727 ms) against 55.4 us for nfc_multi_fetch(PACKETS) and a
 * Python list of bits per packet; a single context's 1e8-sample batch: frames + nfc_fsm_process_frames 6.04 ms against 8.90 ms for
 * the packet tables, the bits and nfc_fsm_process_packets, the two kernels 0.100 ms. */
typedef struct {
    uint32_t n_streams, n_launches;
    const uint64_t *frame_off[2];        /* n_streams + 1 entries each */
    const uint64_t *byte_off[2];
    const uint64_t *base;                /* n_streams */
    const nfc_raw_frame *frames[2];
    const uint8_t *bytes[2], *par[2];
    uint64_t bytes_copied;               /* device -> host, of this call */
    double ms_kernels;                   /* with nfc_multi_set_timing(on): the two launches by HIP events; else 0 */
    uint64_t reserved[4];
} nfc_multi_frames;
int nfc_multi_fetch_frames(nfc_multi *m, nfc_multi_frames *out);

/* ---- commands on the GPU: the protocol machine, CRYPTO1 included, a lane per stream -----------------------------------------------
 * What nfc_fsm_process_frames does on the host -- command lookup by protocol stage and leading bytes, tag type and UID tracking, the
 * CRYPTO1 sessions of MIFARE Classic with nested authentications -- is sequential in ONE stream and independent across streams.  With
 * tracking on, every push of a multi-stream context assembles the frames (the two launches of nfc_multi_fetch_frames, into a buffer of
 * the tracking's own) and runs k_multi_commands behind them (csrc/multi_commands.hip.h): a lane per stream merges the stream's two frame
 * lists by idx (type 0 first on a tie), runs every frame through csrc/fsm.hip.h -- the one protocol machine, the text the host machine
 * behind nfc_fsm_* runs too -- and writes records, plaintext and enc entries.  The machines' state stays on the device from push to
 * push, so a session that spans pushes stays in step whether or not anybody fetches.
 * THE STATE is public and plain: nfc_fsm_state, 88 bytes.  A host machine hands itself over with nfc_fsm_get_state / nfc_fsm_set_state,
 * a stream with nfc_multi_get_fsm_state / nfc_multi_set_fsm_state; nfc_host_commands is the kernel's twin on the CPU.
 * UID CAPACITY.  The host machine's UID is an unbounded vector; here it holds 32 bytes (an Ultralight's is 7, the standard's longest
 * 10).  An append that would pass 32 is not made and sets the sticky NFC_FSM_UID_OVERFLOW: from there on that stream's commands are no
 * longer promised to equal the host machine's.  No other stream is affected; a reset clears the flag.
 * CUT FRAMES.  A frame with NFC_RAW_CUT gives a record with cmd == NFC_CMD_CUT and no bytes, does not touch the machine and sets the
 * sticky NFC_FSM_LOST: a session's keystream is out of step from here on.  A stream whose packet table or bit slab was truncated in a
 * push carries NFC_FSM_LOST too.
 * ONE FRAME OUT.  An nfc_frame record; the plaintext bytes (data) and, inside a session, the enc entries as nfc_fsm_process gives them
 * (on-air byte | 0x100 where the parity bit equals the data parity; n_enc of them, none outside a session), both indexed by the
 * record's byte_off.  Every frame owns a slot of its RAW n_bytes entries in both arrays (the nested-authentication route yields fewer
 * plaintext bytes than raw ones; a parity error none); entries of the slot that are not written are 0. */
enum { NFC_CMD_CUT = -3 };          /* beside NFC_CMD_UNKNOWN, NFC_CMD_PARITY_ERROR: the frame's bits were cut (NFC_RAW_CUT) */
enum { NFC_FSM_LOST = 1, NFC_FSM_UID_OVERFLOW = 2 };   /* nfc_fsm_state.flags, sticky until a reset */
typedef struct nfc_fsm_state {      /* 88 bytes */
    int32_t cur_cmd;                /* the command in flight (index for nfc_command_info) */
    int32_t tag_type;               /* -1 none, 0 Ultralight, 1 Classic 1K, 2 Classic 4K, 3 DESFire */
    int32_t encrypted;              /* a CRYPTO1 session is up: 1; 2: up, but its nonce register was not 32 bits (a UID that is not four
                                     * bytes under a nested tag nonce), so that no {ar} / {at} is ever reported as right */
    int32_t cur_key;                /* 0: key A, 1: key B, 2 + slot: that slot of the sector key table (below) */
    uint64_t cipher;                /* the 48-bit register; bit i is the i-th oldest bit */
    uint8_t ar[4], at[4];           /* the expected reader / tag answers */
    uint8_t key_a[6], key_b[6];
    uint32_t uid_len;               /* 0 .. 32 */
    uint8_t uid[32];                /* zero behind uid_len */
    uint32_t flags;                 /* NFC_FSM_* */
    uint32_t reserved;              /* 0 */
} nfc_fsm_state;
/* the state nfc_fsm_reset leaves: REQA in flight, no tag, both keys FF FF FF FF FF FF */
int nfc_fsm_state_init(nfc_fsm_state *st);
/* a host machine's state out and in.  get: NFC_ERR_ARG when the host UID is longer than 32 bytes; set: NFC_ERR_ARG for a field out of range */
int nfc_fsm_get_state(const nfc_fsm *f, nfc_fsm_state *st);
int nfc_fsm_set_state(nfc_fsm *f, const nfc_fsm_state *st);
/* The kernel's twin on the CPU (no GPU needed): nfc_fsm_process_frames' arguments, but on the plain state and with the slots described
 * above -- frame i's byte_off is the sum of the raw n_bytes before it; data / enc hold cap entries each (NFC_ERR_ARG when the frames
 * need more); *used: entries that belong to the frames.  A frame with NFC_RAW_CUT is accepted (NFC_CMD_CUT). */
int nfc_host_commands(nfc_fsm_state *st, const nfc_raw_frame *merged, size_t n, const uint8_t *bytes0, const uint8_t *par0,
                      const uint8_t *bytes1, const uint8_t *par1, nfc_frame *out, uint8_t *data, uint16_t *enc, size_t cap, size_t *used);
/* nfc_multi_track_commands(m, on): off at create.  While it is on, every nfc_multi_push / _push_device enqueues three launches before it
 * returns, after it has read the counts -- the frames scan, the frames assembly, k_multi_commands -- with no host wait: the machines
 * advance exactly once per push and stream.  A push in which nothing is stored launches nothing.  nfc_multi_fetch and
 * nfc_multi_fetch_frames keep their own buffers and lifetimes; a context that never switches tracking on launches what it always did.
 * nfc_multi_fetch_commands: ONE copy of the tracking's buffer to pinned memory, then one wait.
 *   raw            the frames of this push, exactly what nfc_multi_fetch_frames gives for it (its n_launches / bytes_copied / ms_kernels: 0)
 *   cmd_off        n_streams + 1: stream k's commands are cmd / src [cmd_off[k] .. cmd_off[k + 1]), in stream order (both types merged)
 *   cbyte_off      n_streams + 1: its slots are data / enc [cbyte_off[k] .. cbyte_off[k + 1]); a record's byte_off is relative to cbyte_off[k]
 *   src            per command: type << 31 | index among the stream's raw frames of that type (raw.frames[type][raw.frame_off[type][k] + index])
 *   stream_flags   n_streams: NFC_FSM_LOST, NFC_FSM_UID_OVERFLOW
 *   ms_kernels     with nfc_multi_set_timing(on): the three launches by HIP events, ms_machine the machine kernel alone; else 0
 * A second call before the next push returns the same data and touches no machine.  Tracking off at the last push, or no completed
 * push: NFC_ERR_STATE.  Device totals that differ from the host's: NFC_ERR_INTERNAL.  Nothing stored in the push: n_launches == 0, the
 * offsets all zero, NULL arrays but stream_flags.  The pointers live until the next nfc_multi_push / _push_device,
 * nfc_multi_fetch_commands, nfc_multi_reset, nfc_multi_set_state, nfc_multi_set_fsm_state or nfc_multi_destroy.
 * nfc_multi_set_keys: the sector keys of stream `stream` (-1: of every stream), as nfc_fsm_set_keys.  nfc_multi_get_fsm_state /
 * nfc_multi_set_fsm_state complete the device first.  nfc_multi_reset(stream) also returns that stream's machine to
 * nfc_fsm_state_init's state, keys included, as nfc_fsm_reset does; nfc_multi_set_state does not touch the machine.
 * Argument errors (a stream out of range, a null key or state, a state field out of range) are NFC_ERR_ARG, raised before the device is
 * touched, the argument's name in the message.
 * COST, measured with K copies of a 24-frame Classic capture of 39 269 samples (README.md, profiles/commands_bench.json): the call and two
 * vectorised masks cost 0.730 us per capture at 1 024 streams and 0.724 us at 16 384, against 93.27 / 94.07 us for nfc_multi_fetch_frames and
 * a host call per stream; tracking adds 0.32 ms / 1.05 ms to a push of 15.7 / 16.2 ms, the machine kernel alone 0.28 - 0.29 ms. */
typedef struct {
    nfc_multi_frames raw;
    const uint64_t *cmd_off, *cbyte_off;   /* n_streams + 1 entries each */
    const nfc_frame *cmd;
    const uint32_t *src;
    const uint8_t *data;
    const uint16_t *enc;
    const uint32_t *stream_flags;          /* n_streams */
    uint32_t n_streams, n_launches;        /* of the push: 3, or 0 when nothing was stored */
    uint64_t bytes_copied;                 /* device -> host, of this call */
    double ms_kernels, ms_machine;
    uint64_t reserved[4];
} nfc_multi_commands;
int nfc_multi_track_commands(nfc_multi *m, int on);
int nfc_multi_fetch_commands(nfc_multi *m, nfc_multi_commands *out);
int nfc_multi_set_keys(nfc_multi *m, int64_t stream /* -1: every stream */, const uint8_t key_a[6], const uint8_t key_b[6]);
int nfc_multi_get_fsm_state(nfc_multi *m, uint32_t stream, nfc_fsm_state *st);
int nfc_multi_set_fsm_state(nfc_multi *m, uint32_t stream, const nfc_fsm_state *st);

/* ---- a key per sector: the key table of the protocol machines ----------------------------------------------------------------------
 * A MIFARE Classic card has one key A and one key B PER SECTOR, 40 sectors at most: blocks 0 .. 127 lie four to a sector, blocks
 * 128 .. 255 sixteen (nfc_sector_of_block).  Beside its two keys every machine -- the host machine, nfc_host_commands_keyed, every
 * stream of a multi-stream context -- can hold a TABLE of 80 slots, slot = (key_type & 1) * 40 + sector, each empty or six key bytes.
 * When a machine recognises AUTHA / AUTHB it takes the block from the command's plaintext byte 1 (already decrypted under the running
 * session for a nested one) and chooses: the table's slot when it is present, else key A / key B exactly as without a table.  The
 * choice is nfc_fsm_state.cur_key (0 / 1: the machine's key A / B; 2 + slot: the table's slot), so it survives until the nonce frame
 * that loads the register, in a later call or push if need be; a slot emptied in between falls back to the key A / B of its type.
 * nfc_fsm_process_outgoing chooses the same way at an outgoing AUTHA / AUTHB (with no slot present it leaves cur_key to its caller, as
 * before).  AN EMPTY TABLE IS THE BEHAVIOUR WITHOUT ONE, bit for bit, state included.  The table is no part of nfc_fsm_state:
 * nfc_fsm_get_state / _set_state and nfc_multi_get_fsm_state / _set_fsm_state / nfc_multi_set_state leave it alone; nfc_fsm_reset and
 * nfc_multi_reset(stream) empty it (that stream's); nfc_fsm_set_keys / nfc_multi_set_keys do not touch it.
 * A `present` other than 0 or 1, a sector >= 40, a key_type other than 0x60 / 0x61 are NFC_ERR_ARG (nfc_multi_*: raised before the
 * device is touched, the argument's name in the message).
 * nfc_multi_set_sector_keys broadcasts ONE table to stream `stream` or to every stream; nfc_multi_get_sector_keys reads one stream's;
 * both complete the device first.  The device holds the tables in a buffer of 640 bytes per stream (40 MiB at 65 536 streams) that is
 * allocated, zeroed, by a context's FIRST nfc_multi_set_sector_keys: a context that never sets a sector key allocates nothing for it,
 * launches what it always did, and its nfc_multi_get_sector_keys gives an empty table.  No device memory: NFC_ERR_NOMEM, the context
 * as it was.
 * nfc_host_commands_keyed: nfc_host_commands with a table (NULL: an empty one -- then it IS nfc_host_commands); the CPU twin of
 * k_multi_commands for this path.
 * COST, measured with K copies of a 26-frame card of three keys in four authentications (41 164 samples; README.md,
 * profiles/sector_keys_bench.json): the machine kernel 0.275 ms with the two keys alone and 0.327 ms with a table per stream at 1 024
 * streams, 0.284 / 0.336 ms at 16 384 -- mostly the two sectors more that the lanes then decrypt; a push of 16.8 / 18.1 ms grows by
 * 0.05 - 0.07 ms.  With no table set the machine kernel is 1.3 % slower than it was before the table existed. */
#define NFC_KEY_SECTORS 40
typedef struct nfc_fsm_key_table {  /* 560 bytes */
    uint8_t key[2][NFC_KEY_SECTORS][6];     /* [key_type & 1][sector] */
    uint8_t present[2][NFC_KEY_SECTORS];    /* 0: empty, 1: key[..] holds the slot's key */
} nfc_fsm_key_table;
int nfc_sector_of_block(int block);         /* 0 .. 39 for block 0 .. 255; -1 outside */
int nfc_fsm_key_table_init(nfc_fsm_key_table *t);   /* every slot empty, every byte 0 */
int nfc_fsm_set_sector_key(nfc_fsm *f, int key_type /* 0x60, 0x61 */, int sector, const uint8_t key[6] /* NULL: clear the slot */);
int nfc_fsm_get_key_table(const nfc_fsm *f, nfc_fsm_key_table *t);
int nfc_fsm_set_key_table(nfc_fsm *f, const nfc_fsm_key_table *t);
int nfc_host_commands_keyed(nfc_fsm_state *st, const nfc_fsm_key_table *table, const nfc_raw_frame *merged, size_t n, const uint8_t *bytes0,
                            const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1, nfc_frame *out, uint8_t *data, uint16_t *enc,
                            size_t cap, size_t *used);
int nfc_multi_set_sector_keys(nfc_multi *m, int64_t stream /* -1: every stream */, const nfc_fsm_key_table *table);
int nfc_multi_get_sector_keys(nfc_multi *m, uint32_t stream, nfc_fsm_key_table *table);

/* ---- commands on the GPU for ONE long stream: a lane per transaction ----------------------------------------------------------------
 * A single context's frames go through the same machine (csrc/fsm.hip.h) on the device, although one stream is one sequence: a plain
 * REQA / WUPA heard outside a CRYPTO1 session leaves the machine in a state that does not depend on where it was, so a long capture is
 * thousands of transactions that can each be walked by a lane of their own (csrc/ctx_commands.hip.h).  "Outside a session"
 * is a guess until the transaction before has been walked: every segment -- from one such reader frame to the next -- is walked
 * speculatively, then one wave goes through the segments' summaries in order and walks again, from the true machine, every segment
 * whose guess was wrong.
 * nfc_track_commands(ctx, on): off at create.  While it is on, every batch that completes -- the return of nfc_push / nfc_push_device /
 * nfc_push_edges, nfc_wait for a submitted batch -- enqueues, with no further host wait, the frames' two launches (the context's own
 * lazy assembly: a later nfc_read_frames of that batch launches nothing more) and four launches behind them on the context's stream:
 * merged order and cuts, segment numbering, the speculative walk, the resolve.  The machine advances exactly once per batch whether or
 * not anybody reads.  A batch that closed no packet launches nothing.  A context that never turns tracking on allocates and launches
 * exactly what it did before.
 * nfc_read_commands: ONE copy to pinned memory, then one wait.  cmd / src / data / enc as in nfc_multi_commands for one stream: the
 * frames of both types merged by idx (type 0 first on a tie), src = type << 31 | index among the batch's raw frames of that type, a
 * record's byte_off into data / enc, a slot of the RAW n_bytes per frame.  A second call before the next batch returns the same data and
 * touches no machine.  No completed batch, or tracking off when the last batch completed: NFC_ERR_STATE.  A batch without frames:
 * n_launches == 0, n_commands == 0, NULL arrays.  The pointers live until the next batch completes, nfc_read_commands, nfc_reset,
 * nfc_set_fsm_state or nfc_destroy.
 * THE MACHINE: nfc_set_fsm_keys, nfc_set_fsm_sector_keys / nfc_get_fsm_sector_keys, nfc_get_fsm_state / nfc_set_fsm_state as their
 * nfc_multi_* namesakes for one stream; they complete the device first.  nfc_reset returns the machine to nfc_fsm_state_init's state
 * and empties the table.  The table's device buffer is allocated by the first nfc_set_fsm_sector_keys.  Argument errors are
 * NFC_ERR_ARG, raised before the device is touched, the argument's name in the message.
 * PROMISED: records, data, enc and the state afterwards equal nfc_host_commands_keyed's on the same raw frames, bit for bit, on every
 * input -- sessions that span batches, nested authentications, malformed traffic.
 * NOT PROMISED: more than one stream (nfc_multi_* is that); cuts anywhere but at a plain REQA / WUPA; speed on a capture that never
 * leaves a session: a REQA inside a session is ciphertext to the machine, the guess fails from there on, and ONE lane walks the rest
 * of the batch (n_rerun_frames says how much).
 * nfc_host_commands_segmented: the twin on the CPU (no GPU needed) -- nfc_host_commands_keyed's arguments and results, computed by
 * the kernels' own text: cuts, speculative walks in the order segment_order names (n_order entries; those below n_segments must name
 * every segment once, larger ones are skipped; NULL: ascending), resolve.  counters may be NULL. */
typedef struct nfc_ctx_command_counters {   /* 16 bytes */
    uint32_t n_segments;            /* 0 for no frames */
    uint32_t n_rerun_segments;      /* segments whose guess was wrong: walked again from the true machine */
    uint32_t n_rerun_frames;        /* ... and the frames in them */
    uint32_t n_keydep_segments;     /* speculative walks that read cur_key before writing it */
} nfc_ctx_command_counters;
typedef struct nfc_ctx_commands {
    const nfc_frame *cmd;
    const uint32_t *src;
    const uint8_t *data;
    const uint16_t *enc;
    uint64_t n_commands, n_bytes;
    uint32_t flags;                 /* NFC_FSM_* of the machine behind the batch */
    uint32_t n_launches;            /* of the batch's tracking: 6, or 0 for a batch without frames */
    nfc_ctx_command_counters counters;
    uint64_t bytes_copied;          /* device -> host, of this call */
    double ms_kernels;              /* with nfc_set_timing >= 1 when the batch completed: the six launches by HIP events; else all 0 */
    double ms_frames, ms_merge, ms_walk, ms_resolve;   /* ... the frames' two / merged order and segment numbering / the speculative walk / the resolve */
    uint64_t reserved[4];
} nfc_ctx_commands;
int nfc_track_commands(nfc_ctx *ctx, int on);
int nfc_read_commands(nfc_ctx *ctx, nfc_ctx_commands *out);
int nfc_set_fsm_keys(nfc_ctx *ctx, const uint8_t key_a[6], const uint8_t key_b[6]);
int nfc_set_fsm_sector_keys(nfc_ctx *ctx, const nfc_fsm_key_table *table /* NULL: an empty one */);
int nfc_get_fsm_sector_keys(nfc_ctx *ctx, nfc_fsm_key_table *table);
int nfc_get_fsm_state(nfc_ctx *ctx, nfc_fsm_state *st);
int nfc_set_fsm_state(nfc_ctx *ctx, const nfc_fsm_state *st);
int nfc_host_commands_segmented(nfc_fsm_state *st, const nfc_fsm_key_table *table, const nfc_raw_frame *merged, size_t n,
                                const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1, nfc_frame *out,
                                uint8_t *data, uint16_t *enc, size_t cap, size_t *used, const uint32_t *segment_order, size_t n_order,
                                nfc_ctx_command_counters *counters);

/* ---- key recovery: a MIFARE Classic sector key from one sniffed first authentication --------------------------------------------------
 * An eavesdropper who has no keys still sees everything the recovery needs: the UID (SEL1R), the tag nonce nt in the clear (RANDTA),
 * {nr}{ar} (RANDRB) and {at} (RANDTB).  ks2 = {ar} ^ suc64(nt) and ks3 = {at} ^ suc96(nt) are 64 known keystream bits of a free-running
 * 48-bit register; they determine it, and rolling it back over {nr} and uid ^ nt gives the key (csrc/keys.hip.h states the method,
 * DESIGN.md 8h the layout).  Independent across authentications: nfc_recover_keys_device runs a batch of traces per launch.
 * A 32-bit word of a frame has bit i = bit (i & 7) of byte (i >> 3) -- byte 0 lowest.  par: bit i the ninth bit, as received, of byte i of
 * {nr}{ar} (i = 0 .. 7) and of byte i - 8 of {at} (i = 8 .. 11).  40 bytes: five words, the parity bits, key type and block, stream and
 * frame as 32-bit counts and the 64-bit sample index at their natural widths.
 * NOT PROMISED: 7-byte UIDs.  (Without {at}: two authentications of one key, nfc_recover_reader_keys_device below.)  (Nested authentications, whose nt is encrypted, are not nfc_find_auths' but
 * nfc_find_nested_auths': the section below.) */
typedef struct nfc_auth_trace {
    uint32_t uid, nt, nr_enc, ar_enc, at_enc;
    uint16_t par;
    uint8_t key_type;              /* 0x60: key A, 0x61: key B */
    uint8_t block;
    uint32_t stream;               /* nfc_find_auths writes 0: the caller's to fill */
    uint32_t frame;                /* index of the AUTH frame in the merged order */
    uint64_t idx;                  /* nfc_raw_frame.idx of the AUTH frame */
} nfc_auth_trace;
enum { NFC_KEY_OK = 0,             /* exactly one verified candidate */
       NFC_KEY_NONE = 1,           /* no candidate passed the verification */
       NFC_KEY_AMBIGUOUS = 2,      /* more than one: the lowest key as a 48-bit integer (byte 0 lowest) is reported */
       NFC_KEY_OVERFLOW = 3 };     /* the trace's table does not fit max_capacity: nothing was searched, n_odd / n_even are exact */
typedef struct nfc_key_result {    /* 24 bytes */
    uint8_t key[6];
    uint8_t status;                /* NFC_KEY_* */
    uint8_t reserved;
    uint32_t n_candidates;         /* verified candidates, saturating */
    uint32_t n_odd, n_even;        /* the exact sizes of the two lists */
    uint32_t nr;                   /* the decrypted reader nonce under `key` (0 without a key) */
} nfc_key_result;
/* CAPACITY is counted in table slots (16 bytes each in device memory).  A trace needs a table of the smallest power of two that is at least
 * twice its odd list; the traces of a batch are searched in groups, in order, whose tables together fit max_capacity.  The scratch
 * starts at initial_capacity and grows to fit a group that needs more (nfc_key_stats.n_grown counts that), never beyond max_capacity; a
 * trace whose table alone exceeds max_capacity gets NFC_KEY_OVERFLOW -- nothing is truncated and nothing written past a table.
 * Defaults (a 0): initial_capacity 2^26 (1 GiB: sixteen tables of 2^22, DESIGN.md 8h says where that comes from), max_capacity 2^28,
 * max_batch 16.  initial_capacity above max_capacity, max_capacity above 2^32, max_batch above 4096, unknown flags or non-zero
 * reserved words are NFC_ERR_ARG. */
enum { NFC_KEY_TIMING = 1 };       /* nfc_key_config.flags: HIP events around every launch -> nfc_key_stats.ms_* (device call only) */
typedef struct nfc_key_config {    /* 32 bytes */
    uint64_t initial_capacity, max_capacity;
    uint32_t max_batch;            /* traces per count launch */
    uint32_t flags;
    uint32_t reserved[2];
} nfc_key_config;
typedef struct nfc_key_stats {     /* 56 bytes */
    double ms_kernels;             /* ms_count + ms_fill + ms_probe (the nested call: + its candidate launch); 0 without NFC_KEY_TIMING and from the host twin */
    double ms_count, ms_fill, ms_probe;
    uint64_t scratch_bytes;        /* the tables' scratch at the end of the call (the host twin: what the device call would hold) */
    uint32_t n_batches, n_grown;
    uint32_t n_launches, reserved;
} nfc_key_stats;
/* Host only.  `frames`: both types merged by idx, as nfc_fsm_process_frames takes them (type 0: tag, bytes0 / par0; type 1: reader).  A
 * first authentication is: the most recent reader frame 93 70 u0 u1 u2 u3 bcc crc with NFC_RAW_CRC_A_OK (4-byte UIDs only, as the
 * machine's set_tag); then, consecutive in the merged order and none NFC_RAW_CUT: a reader frame 60|61 blk crc with NFC_RAW_CRC_A_OK, a tag
 * frame of 4 bytes with NFC_RAW_PARITY_OK (nt), a reader frame of 8 bytes ({nr}{ar}), a tag frame of 4 bytes ({at}).  out: the first
 * `cap` of them; *n_out: how many there are. */
int nfc_find_auths(const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                   const uint8_t *par1, nfc_auth_trace *out, size_t cap, size_t *n_out);
/* The CPU twin (no GPU needed): the same header, the same capacity rules and statuses; the join is a sort of the odd list and a binary
 * search per even sequence.  cfg and stats may be NULL. */
int nfc_host_recover_keys(const nfc_auth_trace *traces, size_t n, const nfc_key_config *cfg, nfc_key_result *out, nfc_key_stats *stats);
/* No context, like nfc_record_pcm16_device: per batch one count launch and one read of the counts, then per group a fill and a probe
 * launch (csrc/keys.hip.h).  The results are complete when the call returns.  n == 0 launches nothing and touches no device.  Every
 * argument is checked before the device is touched.  There is no CPU fallback: without a usable device the call fails. */
int nfc_recover_keys_device(int device, const nfc_auth_trace *traces, size_t n, const nfc_key_config *cfg, nfc_key_result *out,
                            nfc_key_stats *stats);

/* ---- key recovery from NESTED authentications ---------------------------------------------------------------------------------------
 * Every authentication after a session's first one is nested: the AUTH command and the tag nonce arrive encrypted.  A genuine card draws
 * nt from a 16-bit LFSR, so there are 65 536 candidates; ten of the ninth bits of {nt}, {ar} and {at} are encrypted with keystream bits
 * that follow from the candidate alone, and 64 candidates pass them -- or none, when the nonce is off the sequence (a hardened card) or
 * a bit was misheard.  For ONE candidate a nested authentication is a first one with another nt: the search above runs once per
 * candidate (a VIRTUAL trace), and a key must besides reproduce the 32 keystream bits over {nt} and its four ninth bits (csrc/keys.hip.h,
 * DESIGN.md 8i).
 * nfc_nested_trace, 40 bytes in nfc_auth_trace's layout with nt_enc for nt.  par: bits 0 .. 11 as in nfc_auth_trace, bits 12 .. 15 the
 * ninth bits, as received, of {nt} bytes 0 .. 3.  key_type / block: 0 / 0xFF while the AUTH command is not known in plaintext (the
 * search reads neither).
 * NOT PROMISED: cards whose nested nonces are not on the 16-bit sequence (no candidates: NFC_KEY_NONE with n_nt 0), a nested {nt} without
 * {at} (the reader-pair search below takes first authentications only), 7-byte UIDs, a search that uses ks1 alone. */
typedef struct nfc_nested_trace {
    uint32_t uid, nt_enc, nr_enc, ar_enc, at_enc;
    uint16_t par;
    uint8_t key_type;              /* 0x60 / 0x61 once labelled, else 0 */
    uint8_t block;                 /* 0xFF until labelled */
    uint32_t stream;               /* nfc_find_nested_auths writes 0: the caller's to fill */
    uint32_t frame;                /* index of the encrypted AUTH frame in the merged order */
    uint64_t idx;                  /* nfc_raw_frame.idx of that frame */
} nfc_nested_trace;
/* status: NFC_KEY_OK / NONE / AMBIGUOUS over the verified (candidate, key) pairs of the searched candidates; AMBIGUOUS reports the
 * lowest key and the nt that goes with it.  NFC_KEY_OVERFLOW: the table of at least one searched candidate alone exceeds max_capacity
 * and that candidate was not searched; the OTHER candidates still were, and a key verified among them is reported -- status OVERFLOW
 * with key, nt, nr and n_verified set (n_verified 0 and a zero key: none was). */
typedef struct nfc_nested_result { /* 48 bytes */
    uint8_t key[6];
    uint8_t status;                /* NFC_KEY_* */
    uint8_t reserved;
    uint32_t n_verified;           /* verified (candidate, key) pairs, saturating */
    uint32_t n_nt;                 /* candidates the trace has: 0 or 64 */
    uint32_t n_searched;           /* how many of them the window held */
    uint32_t nt;                   /* the recovered plaintext tag nonce (0 without a key) */
    uint32_t nr;                   /* the decrypted reader nonce under `key` (0 without a key) */
    uint32_t reserved2;
    uint64_t n_odd, n_even;        /* the exact list sizes, summed over the searched candidates */
} nfc_nested_result;
/* search: as for first authentications, its limits and defaults; capacity and max_batch count VIRTUAL traces.  Per trace only the
 * candidates [cand_first, cand_first + cand_count) of its ascending list are searched (cand_count 0: all from cand_first): how several
 * devices share a card.  cand_first above 64 or a non-zero reserved word is NFC_ERR_ARG. */
typedef struct nfc_nested_config { /* 48 bytes */
    nfc_key_config search;
    uint32_t cand_first, cand_count;
    uint32_t reserved[2];
} nfc_nested_config;
/* Host only, nfc_find_auths' arguments.  A nested authentication comes after a first authentication (nfc_find_auths' rule) of the current
 * UID with no reader SELECT frame (93 70 .., NFC_RAW_CRC_A_OK) in between, and is four consecutive frames of the merged order, none
 * NFC_RAW_CUT: a reader frame of 4 bytes that is not itself a plain 60|61 blk crc with NFC_RAW_CRC_A_OK, a tag frame of 4 bytes ({nt}), a
 * reader frame of 8 bytes, a tag frame of 4 bytes.  No keys are needed: inside a session no other exchange has this shape. */
int nfc_find_nested_auths(const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                          const uint8_t *par1, nfc_nested_trace *out, size_t cap, size_t *n_out);
/* The candidate plaintext nonces of one trace in ascending seed order (the seed: bits 0 .. 15 of the nonce): *n_out is 0 or 64, the first
 * `cap` are written.  nfc_nested_candidates_device: the kernel's answer for n traces, out_nt [n][64] (unused entries 0) and out_n [n]. */
int nfc_host_nested_candidates(const nfc_nested_trace *trace, uint32_t *out_nt, size_t cap, size_t *n_out);
int nfc_nested_candidates_device(int device, const nfc_nested_trace *traces, size_t n, uint32_t *out_nt, uint32_t *out_n);
/* The CPU twin and the device call, as nfc_host_recover_keys / nfc_recover_keys_device: one candidate launch for all traces, then the
 * virtual traces (trace, candidate), in order, in batches of max_batch through the same capacity rules.  stats: n_launches counts the
 * candidate launch too, and with NFC_KEY_TIMING ms_kernels includes its time (ms_count + ms_fill + ms_probe is then less than
 * ms_kernels).  n == 0 launches nothing and touches no device; every argument is checked before the device is touched; no CPU
 * fallback.  cfg and stats may be NULL. */
int nfc_host_recover_nested_keys(const nfc_nested_trace *traces, size_t n, const nfc_nested_config *cfg, nfc_nested_result *out,
                                 nfc_key_stats *stats);
int nfc_recover_nested_keys_device(int device, const nfc_nested_trace *traces, size_t n, const nfc_nested_config *cfg,
                                   nfc_nested_result *out, nfc_key_stats *stats);

/* ---- key recovery from TWO reader-side authentications, without {at} (the "reader attack") ------------------------------------------
 * A stream that emulates a tag, or a sniffer that hears the reader only, gets nt and {nr}{ar} of a first authentication but no genuine
 * {at}.  ks2 = {ar} ^ suc64(nt) alone is 32 known keystream bits: about 2^16 registers fit ONE such authentication; a second one with
 * the same key and another nt or nr singles one out.  The search is the one above at half the depth (16 keystream bits per half, a
 * 22-bit signature: csrc/keys.hip.h); about 1e5 candidates join and each is checked against both sessions: the key must
 * decrypt {nr} to four right ninth bits, reproduce ar, and fit the four ninth bits of {ar} (the last under ks3 bit 0) -- in the SEARCHED
 * session, whose keystream started the search, and in the CHECK session.
 * PROMISED: pairs only; 4-byte UIDs; first authentications only (nt in the clear).  The two UIDs may differ: a UID enters only as
 * uid ^ nt.  at_enc and par bits 8 .. 11 of both traces are ignored.
 * NOT PROMISED: a single authentication without {at} (about 2^16 keys fit); a nested {nt} without {at}; 7-byte UIDs.
 * Two IDENTICAL sessions (same uid ^ nt, same {nr}{ar}) cannot single a key out: every register that fits the one fits the other, and
 * the result is NFC_KEY_AMBIGUOUS with n_candidates > 1 (keys.pair_reader_auths never pairs two such).
 * COST (MI355X, measured: profiles/reader_keys_bench.json): 1.60 ms per pair at 256 pairs and 1.68 ms at 16 (5.7 ms for a
 * single pair), against 214 ms for the twin on one core and 4.74 ms per authentication for the full search above on the same sessions
 * with their {at}; with NFC_RKEY_VERIFY_INLINE 3.31 ms and 3.67 ms.  Device memory: the tables as above plus max_batch x
 * stage_capacity x 8 bytes (32 MiB at the defaults). */
typedef struct nfc_reader_pair {   /* 80 bytes */
    nfc_auth_trace search, check;
} nfc_reader_pair;
typedef struct nfc_reader_key_result { /* 32 bytes */
    uint8_t key[6];
    uint8_t status;                /* NFC_KEY_*; AMBIGUOUS reports the lowest key; OVERFLOW as above: nothing searched, n_odd / n_even exact */
    uint8_t pad;
    uint32_t n_candidates;         /* joined candidates that passed both sessions, saturating */
    uint32_t n_joined;             /* pairs of sequences with equal signatures: what was verified */
    uint32_t n_odd, n_even;        /* the exact sizes of the two lists */
    uint32_t nr_search, nr_check;  /* the decrypted reader nonces of the two sessions under `key` (0 without a key) */
} nfc_reader_key_result;
/* search: as for first authentications, its limits and defaults; capacity counts table slots and max_batch pairs.  stage_capacity: the
 * joined candidates per pair that the probe launch hands to the verify launch (8 bytes each, max_batch sections); 0: the default,
 * 2^18.  A pair that joins more verifies the rest where they were found: the result does not depend on stage_capacity.  Above 2^24 is
 * NFC_ERR_ARG.  NFC_RKEY_VERIFY_INLINE: no stage and no verify launch, every candidate is verified by the lane that found it (the form
 * of the full search; kept for comparison).  Unknown flags or non-zero reserved words are NFC_ERR_ARG. */
enum { NFC_RKEY_VERIFY_INLINE = 1 };
typedef struct nfc_reader_key_config { /* 48 bytes */
    nfc_key_config search;
    uint32_t stage_capacity;
    uint32_t flags;
    uint32_t reserved[2];
} nfc_reader_key_config;
/* Host only, nfc_find_auths' arguments and rule LESS its fourth frame: the UID of the last NFC_RAW_CRC_A_OK 93 70 .., a plain
 * NFC_RAW_CRC_A_OK 60|61 blk crc, a tag frame of 4 bytes with NFC_RAW_PARITY_OK, a reader frame of 8 bytes, consecutive and none
 * NFC_RAW_CUT.  What follows is not looked at -- no {at}, a noise {at}, the end of the list -- so by `frame` the result is a superset
 * of nfc_find_auths'.  at_enc and par bits 8 .. 11 are written 0. */
int nfc_find_reader_auths(const nfc_raw_frame *frames, size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1,
                          const uint8_t *par1, nfc_auth_trace *out, size_t cap, size_t *n_out);
/* The CPU twin and the device call, as nfc_host_recover_keys / nfc_recover_keys_device: the same batching and capacity rules over
 * pairs, the same statuses and statistics by construction.  Per group a fill launch, a probe launch and -- unless
 * NFC_RKEY_VERIFY_INLINE -- a verify launch, whose time counts in ms_probe.  n == 0 launches nothing and touches no device; every
 * argument (key_type of all four traces included) is checked before the device is touched; no CPU fallback.  cfg and stats may be NULL. */
int nfc_host_recover_reader_keys(const nfc_reader_pair *pairs, size_t n, const nfc_reader_key_config *cfg, nfc_reader_key_result *out,
                                 nfc_key_stats *stats);
int nfc_recover_reader_keys_device(int device, const nfc_reader_pair *pairs, size_t n, const nfc_reader_key_config *cfg,
                                   nfc_reader_key_result *out, nfc_key_stats *stats);

/* ---- emulation: a tag machine and a reader machine, and K cards read by K readers with no signal at all ---------------------------
 * The reference's second half (tag.py, reader.py, the closed loop of usrp_nfc.py:116-136), one text for host and device
 * (csrc/emu.hip.h).  A TAG answers what it hears from its memory, its nonces and its access bits; a READER walks a card:
 * anticollision, then an Ultralight's pages or every sector of a Classic 1K from the last down, an authentication per sector.
 * WHAT IS EMULATED is an nfc_emu_card.  mem: exactly 64 bytes (Ultralight) or 1024 (Classic 1K) -- the reference's slices would
 * silently shorten an answer otherwise; a reader has none.  rands: four bytes each, handed out in turn and from the first again; a
 * Classic tag and every reader need 1 .. 64 of them (the reference's `random` fallback stays on the Python side).  key_a / key_b and
 * table: a reader's keys (a tag's come from its memory).  The reader's UID holds 32 bytes (NFC_EMU_UID_OVERFLOW beyond).
 * THE MODE travels in the card.  NFC_EMU_REFERENCE is the reference with its quirks: AUTHB served with key A and recorded as key A
 * (tag.py:364-366); both keys from the trailer of sector 0 whatever block is authenticated (tag.py:52-57); the access bytes read at
 * 16 * the AUTH's BLOCK number + 54 (tag.py:194-197,225-229), the trailer's only when the AUTH named the sector's first block; only
 * reads are served; the reader always uses key A (reader.py:25); a nested tag nonce leaves under the OLD session's keystream
 * (fsm.py:96-99).  NFC_EMU_CARD is what a MIFARE Classic does where that differs: the keys of the authenticated block's own sector,
 * AUTHB with key B and the access conditions that depend on it, a nested tag nonce under the NEW key's keystream while uid ^ nt is
 * fed in, a reader that takes its sector's key from `table` where the slot is filled (key_a / key_b otherwise).
 * Where the reference raises -- a frame it does not know, a parity error, RANDRB before any AUTH, more UID bits than nonce bits --
 * the machine gives no answer and sets the sticky NFC_EMU_RAISED; its prints are flags too.
 * ARGUMENT ERRORS are NFC_ERR_ARG, raised before the device is touched; nfc_emu_last_error() names the argument. */
enum { NFC_EMU_TAG = 0, NFC_EMU_READER = 1 };                 /* nfc_emu_card.role */
enum { NFC_EMU_REFERENCE = 0, NFC_EMU_CARD = 1 };             /* nfc_emu_card.mode */
enum { NFC_EMU_LINK_PLAIN = 0, NFC_EMU_LINK_AIR = 1 };        /* nfc_emu_config.link */
enum { NFC_EMU_RAISED = 1,                                     /* the reference raises here: no answer */
       NFC_EMU_UNEXPECTED = 2,                                 /* "ERROR, Unexpected command!!" (reader.py:146): HALT was sent */
       NFC_EMU_ERR_ONES = 4, NFC_EMU_ERR_TWOS = 8, NFC_EMU_ERR_THREES = 16,   /* "ERROR WITH ONES / TWOS / THREES" (tag.py:207-212) */
       NFC_EMU_UID_OVERFLOW = 32,                              /* the reader's UID would pass 32 bytes: not extended */
       NFC_EMU_FLAGS_ALL = 63 };
typedef struct nfc_emu_state {      /* 88 bytes; sticky flags apart, what tag.py / reader.py keep between two frames */
    int32_t halted, selected;       /* tag */
    int32_t auth;                   /* tag: the authenticated block (the AUTH's own number), -1 none */
    int32_t auth_key;               /* tag: 0 none, 1 key A, 2 key B (tag.py:27-30) */
    int32_t auth_prosp;             /* tag: the block of the AUTH in flight, -1 none */
    int32_t at_set;                 /* tag: `at` holds the answer of the AUTH in flight */
    uint8_t at[4];
    uint32_t rand_idx;              /* both: the next nonce */
    int32_t tag_type;               /* reader: -1 none, 0 .. 3 as nfc_fsm_state.tag_type */
    int32_t cur_addr, auth_addr;    /* reader */
    uint32_t uid_len;               /* reader: 0 .. 32 */
    uint8_t uid[32];
    uint32_t flags;                 /* NFC_EMU_* */
    uint32_t reserved;              /* 0 */
} nfc_emu_state;
typedef struct nfc_emu_card {       /* 64 bytes */
    int32_t role;                   /* NFC_EMU_TAG / NFC_EMU_READER */
    int32_t tag_type;               /* tag: 0 Ultralight, 1 Classic 1K; reader: ignored */
    int32_t mode;                   /* NFC_EMU_REFERENCE / NFC_EMU_CARD */
    uint32_t mem_len;
    const uint8_t *mem;
    const uint8_t *rands;           /* n_rands * 4 bytes */
    uint32_t n_rands;
    uint32_t reserved;              /* 0 */
    uint8_t key_a[6], key_b[6];     /* reader */
    uint32_t reserved2;             /* 0 */
    const nfc_fsm_key_table *table; /* reader, NFC_EMU_CARD: may be NULL */
} nfc_emu_card;
int nfc_emu_state_init(nfc_emu_state *st);
const char *nfc_emu_last_error(void);   /* of the calling thread's last failed nfc_*emu* call */
/* One step of one machine, host only: the heard command `cmd` (an index for nfc_command_info, or NFC_CMD_UNKNOWN / NFC_CMD_PARITY_ERROR)
 * with its extra bytes -> *cmd_out the answer's command (-1: none) and frame_out / *n_out its whole plain frame, header | extra | CRC_A
 * (frame_out holds 18 bytes).  What Tag.process_packet / Reader.process_packet do with (cmd, struct). */
int nfc_host_emu_step(const nfc_emu_card *card, nfc_emu_state *st, int cmd, const uint8_t *extra, size_t n_extra, int *cmd_out,
                      uint8_t *frame_out, size_t *n_out);
/* REPLAY, host only: nfc_host_commands_keyed with an emulator behind the machine, as tag_emulate / reader_emulate wire one
 * (usrp_nfc.py:35-100, packets.py:88-90).  After every command whose type is the OTHER side's (a tag card hears reader frames, a reader
 * card tag frames) the emulator of `card` runs, and its answer passes through the SAME machine's process_outgoing -- in the card's mode
 * -- so the machine has advanced before the next heard frame is decrypted.  `st` / `table` / the frames and out / data / enc / cap / used
 * are nfc_host_commands_keyed's; `est` is the emulator's state, advanced in place.  answers: one record per answer (at most n), src the
 * index of the command it answers; ans_plain / ans_air / ans_par: 18 * n entries each, an answer's plain bytes and what goes on the air
 * with its ninth bits at byte_off (an answer owns 18 entries, zeros behind its n_bytes).  A stream is meant to decode only the side it
 * hears; with both decoded the machine hears the real answer AND sends its own, as the reference's would.  On the device: nfc_multi_emulate,
 * below. */
typedef struct nfc_emu_answer {         /* 24 bytes */
    uint32_t src;                       /* index of the command (in `out`) this answers */
    int32_t cmd;                        /* index for nfc_command_info */
    uint32_t byte_off;
    uint16_t n_bytes;
    uint16_t n_bits;                    /* 9 * n_bytes; 7 for a short frame (no machine answers with one today) */
    uint32_t flags;                     /* NFC_EMU_FRAME_ENCRYPTED */
    uint32_t reserved;                  /* 0 */
} nfc_emu_answer;
int nfc_host_emulate(nfc_fsm_state *st, const nfc_fsm_key_table *table, const nfc_emu_card *card, nfc_emu_state *est, const nfc_raw_frame *merged,
                     size_t n, const uint8_t *bytes0, const uint8_t *par0, const uint8_t *bytes1, const uint8_t *par1, nfc_frame *out, uint8_t *data,
                     uint16_t *enc, size_t cap, size_t *used, nfc_emu_answer *answers, uint8_t *ans_plain, uint8_t *ans_air, uint8_t *ans_par,
                     size_t *n_answers);
/* REPLAY ON THE DEVICE: a stream of a multi-stream context that answers.  nfc_multi_emulate gives stream `stream` (-1: every stream)
 * a card -- a role per stream is allowed -- or, with NULL, takes it away; a card implies nfc_multi_track_commands(on).  From then on a
 * tracked push runs the EMULATING form of the machine kernel (csrc/multi_commands.hip.h: k_multi_commands_emu): the same walk, and after
 * every command whose type is the other side's the lane runs its emulator and passes the answer through its own machine's
 * process_outgoing, in the same launch that decodes the commands -- nfc_host_emulate is its twin, stream by stream.  Cards and the
 * emulators' state (nfc_emu_state; nfc_multi_get_emu_state / _set_emu_state) live on the device from push to push; a new card, and
 * nfc_multi_reset(stream), return the emulator to nfc_emu_state_init's state.  A reader card's key_a / key_b / table are NOT used here:
 * the stream's machine has its own (nfc_multi_set_keys, nfc_multi_set_sector_keys).  A context that never calls nfc_multi_emulate
 * allocates and launches exactly what it did; while no stream holds a card a tracked push launches k_multi_commands as ever.
 * nfc_multi_fetch_answers: the answers of the last push, as sections of the buffer nfc_multi_fetch_commands copies -- the same single
 * copy; after a fetch of the commands (or a second call) no device call.  Stream k's answers are records ans[cmd_off[k] ..
 * cmd_off[k] + ans_n[k]) (at most one answer per command, so the commands' offsets place them; there is no ans_off of its own); a
 * record's src is the index of the command it answers among the stream's commands, its bytes are plain / air / par[18 * (cmd_off[k] + j)
 * + i] for answer j.  emulated == 0: the last push ran without a card (or stored nothing): no answers, NULL arrays.  The sections are
 * on 16 bytes each and followed by the guard word; the test build's guard check covers them.  As in the reference, a stream is meant to
 * decode only the side it hears; with both decoded the machine hears the real answer and sends its own.
 * Errors as nfc_multi_set_keys': NFC_ERR_ARG before the device is touched, the argument's name in the message.
 * COST, measured with K copies of the reader side of a 24-frame Classic capture, 12 answers per stream (README.md,
 * profiles/emulate_bench.json): the machine kernel takes 0.509 ms with a card per stream against 0.025 ms without at 1 024 streams, 0.543
 * against 0.033 ms at 16 384; the push 7.75 against 7.28 ms and 9.09 against 8.29 ms. */
typedef struct nfc_multi_answers {
    uint32_t n_streams, emulated;
    uint64_t n_answers;
    const uint64_t *cmd_off;            /* n_streams + 1: as nfc_multi_commands.cmd_off */
    const uint32_t *ans_n;              /* n_streams */
    const nfc_emu_answer *ans;
    const uint8_t *plain, *air, *par;
    uint64_t reserved[4];
} nfc_multi_answers;
int nfc_multi_emulate(nfc_multi *m, int64_t stream /* -1: every stream */, const nfc_emu_card *card /* NULL: take the card away */);
int nfc_multi_fetch_answers(nfc_multi *m, nfc_multi_answers *out);
int nfc_multi_get_emu_state(nfc_multi *m, uint32_t stream, nfc_emu_state *st);
int nfc_multi_set_emu_state(nfc_multi *m, uint32_t stream, const nfc_emu_state *st);
/* THE CLOSED LOOP.  Pair i is tags[i] read by readers[i]: REQA, then every answer is the other side's next frame; after a frame that
 * gets no answer the loop sends REQA again and wakes the tag (usrp_nfc.py:125-131) -- `rounds` of those restarts, 1 .. 64.
 * NFC_EMU_LINK_PLAIN is emulate.run literally: command and structure are handed over, no protocol machine is involved, nothing is
 * encrypted.  NFC_EMU_LINK_AIR gives each side a protocol machine of its own, as tag_emulate / reader_emulate do: a frame leaves through
 * the sender's process_outgoing and arrives through the receiver's process_frame, so it is looked up by stage and decrypted there.  The
 * tag's machine has its two keys from the trailer of sector 0 and, in CARD mode, every trailer as its sector key table; the reader's has
 * key_a / key_b and, in CARD mode, `table`.  The loop's own REQA passes no machine (binary_src repeats it); in CARD mode the reader's
 * machine starts every round without a session, in REFERENCE mode it keeps what it had, as the reference's does.
 * THE TRANSCRIPT.  Pair i owns cap_frames records at frames + i * cap_frames and cap_bytes bytes at plain / air / par + i * cap_bytes:
 * per frame put on the air (the loop's REQAs included) its command, type, the plain bytes, and the on-air bytes with their ninth
 * bits in the form nfc_raw_frame's bytes / par have.  A short frame (REQA) has n_bits 7 and the ninth bit the frame-end repair assumes.
 * A pair that outgrows its slab keeps TRUE counts in its result, stores the frames before the first that did not fit and says so in
 * its flags; a round of more than 1024 frames is ended (NFC_EMU_PAIR_RUNAWAY).
 * nfc_host_emulate_pairs is the CPU twin of the kernel behind nfc_emulate_pairs_device (a lane per pair, csrc/nfc_emu.hip): the
 * same bytes in every output.  The device call checks every argument before the device is touched, returns complete results, and
 * fails with NFC_ERR_INTERNAL when a guard word behind one of its device sections was overwritten.  No CPU fallback.
 * n above 65 536, cap_frames above 2^16, cap_bytes above 2^20, n * cap_bytes above 2^30, a non-zero reserved word: NFC_ERR_ARG.
 * COST, measured with K different Classic 1K cards read whole, 199 frames each, AIR / CARD (README.md, profiles/emulate_bench.json): the
 * kernel takes 9.2 ms whatever K is (one lane's serial cipher clocks); per card the host twin costs 273 us against 9 753 us on the GPU
 * for ONE card (the GPU loses, 36 x), 308 us against 12.5 us at 1 024 cards and 3.71 us at 16 384 (the call: 61 ms, of it 9.2 the kernel). */
enum { NFC_EMU_FRAME_SEED = 1,          /* the loop's own REQA */
       NFC_EMU_FRAME_ENCRYPTED = 2 };   /* the on-air bytes differ from the plain ones */
typedef struct nfc_emu_frame {          /* 16 bytes */
    int16_t cmd;                        /* index for nfc_command_info */
    uint8_t type;                       /* 0 tag -> reader, 1 reader -> tag */
    uint8_t flags;                      /* NFC_EMU_FRAME_* */
    uint32_t byte_off;                  /* in the pair's part of plain / air / par */
    uint16_t n_bytes;
    uint16_t n_bits;                    /* on the air: 9 * n_bytes, or 7 for a short frame */
    uint32_t round;
} nfc_emu_frame;
enum { NFC_EMU_PAIR_CUT_FRAMES = 1, NFC_EMU_PAIR_CUT_BYTES = 2, NFC_EMU_PAIR_RUNAWAY = 4 };
typedef struct nfc_emu_pair_result {    /* 32 bytes */
    uint32_t n_frames, n_bytes;         /* the TRUE counts; stored: what fits before the first frame that did not */
    uint32_t flags;                     /* NFC_EMU_PAIR_* */
    uint32_t rounds;
    uint32_t tag_flags, reader_flags;   /* NFC_EMU_* of the two emulators */
    uint32_t tag_fsm_flags, reader_fsm_flags;   /* NFC_FSM_* of the two protocol machines (AIR) */
} nfc_emu_pair_result;
typedef struct nfc_emu_config {         /* 32 bytes */
    uint32_t link;                      /* NFC_EMU_LINK_* */
    uint32_t rounds;                    /* 1 .. 64 */
    uint32_t cap_frames, cap_bytes;     /* per pair; at least 1 */
    const uint32_t *pair_cap_frames;    /* NULL, or n entries, each at least 1 (NFC_ERR_ARG): pair i stores at most min(cap_frames, pair_cap_frames[i]) frames in its slab of cap_frames */
    uint32_t reserved[2];
} nfc_emu_config;
int nfc_host_emulate_pairs(const nfc_emu_card *tags, const nfc_emu_card *readers, size_t n, const nfc_emu_config *cfg,
                           nfc_emu_pair_result *results, nfc_emu_frame *frames, uint8_t *plain, uint8_t *air, uint8_t *par);
int nfc_emulate_pairs_device(int device, const nfc_emu_card *tags, const nfc_emu_card *readers, size_t n, const nfc_emu_config *cfg,
                             nfc_emu_pair_result *results, nfc_emu_frame *frames, uint8_t *plain, uint8_t *air, uint8_t *par,
                             float *kernel_ms /* NULL, or the kernel's duration by HIP events */);

/* ---- the air interface: K ragged lists of on-air frames -> K IQ captures in one device buffer (csrc/air.hip.h) ----------
 * What an eavesdropper's radio records of a transaction, in any of the four IQ input kinds, laid out for nfc_multi_push_device: the
 * stage between nfc_emulate_pairs_device and a multi-stream context.  The yardstick is synth.py -- with sigma 0 the bytes are those of
 * iq_from_profile over modulation_profile, through quantise_sc16 / _sc8 / _cu8 for the quantised kinds.
 * A STREAM's capture: per frame idle_before unmodulated samples, then the frame's runs; `tail` unmodulated samples behind the last frame.
 * A reader frame (type 1) has the runs of synth.miller_pulses, a tag frame (type 0) those of synth.manchester_pulses -- the lists
 * nfc_tx_encode gives -- and a run of d us has int(d * rate_msps) samples (NOT nfc_tx_sample_count's dur * samp_rate / 1e6).
 * A SAMPLE is I = fl(fl(carrier_i * m) + nI), Q = fl(fl(carrier_q * m) + nQ) in float32 without contraction, m = 1 when idle, the level
 * in a reader frame (0 in a pause), fl(1 + fl(depth) * level) in a tag frame.  The noise is counter-based: n = fl((float)(u0 + u1 + u2 +
 * u3 - 131070) * unit), unit = (float)(sigma / sqrt((65536^2 - 1) / 3)), u0 .. u3 the four 16-bit fields of ONE 64-bit hash of (seed,
 * the stream's seed, the sample's index in its stream, the component): SplitMix64 in counter form, stated in csrc/air.hip.h.  A
 * sample depends on nothing else -- not on K, on where the stream lies or on how the kernel tiles it.  sigma == 0 adds nothing.
 * The quantised kinds: rint in double of x * full_scale (NFC_IN_IQ_U8: of 127.5 + x * full_scale), clipped to the type's range, I first.
 * THE LAYOUT.  Streams are packed in stream order; first_sample[k] is rounded up to align_samples (a power of two, at most 2^20), and
 * the padding between two streams is idle carrier without noise: no byte of [0, first_sample[K-1] + n_samples[K-1]) is left unwritten.
 * A stream without frames is `tail` idle samples.
 * A frame's bits come from air / par, in the form nfc_raw_frame's bytes / par and an nfc_emu_frame transcript have, at byte_base[k] +
 * byte_off of stream k; frames[frame_off[k] .. frame_off[k+1]) are stream k's.  n_bits 1 .. 8: a short frame from the low bits of its
 * first byte; else a multiple of 9 up to 2304; 0: only idle_before is rendered.
 * nfc_host_air_render is the CPU twin of the kernels behind nfc_air_render_device: the same bytes.  With out == NULL it only fills
 * first_sample and n_samples: the sizing call.  The device call checks every argument before the device is touched; dev_out is device
 * memory, 16-byte aligned, of cap_samples samples; kernel_ms: NULL, or TWO floats, the layout kernels' and the render kernel's
 * duration by HIP events.  No CPU fallback: without a GPU it fails with NFC_ERR_DEVICE.
 * ERRORS are NFC_ERR_ARG with the argument's name in the message nfc_last_error gives for a NULL context: an out_kind that is no IQ
 * kind, an align_samples that is no power of two, a bad n_bits, a frame whose bytes leave its stream's part of air / par, a non-zero
 * flags or reserved word, K above 65 536, a type above 1, a rate_msps outside (0, 1000], an idle_before, tail or stream above 2^30
 * samples.  A layout that needs more than cap_samples renders nothing, fills first_sample and n_samples with the true need and is
 * NFC_ERR_ARG naming cap_samples, as nfc_tx_render_device's.  A guard word behind a device section the call allocates that was
 * overwritten: NFC_ERR_INTERNAL. */
typedef struct nfc_air_frame {          /* 16 bytes */
    uint8_t type;                       /* 0 tag -> reader, 1 reader -> tag */
    uint8_t flags;                      /* 0 */
    uint16_t n_bits;
    uint32_t byte_off;                  /* in the stream's part of air / par */
    uint32_t idle_before;               /* unmodulated samples in front of the frame */
    uint32_t reserved;
} nfc_air_frame;
typedef struct nfc_air_config {         /* 72 bytes */
    double rate_msps;                   /* samples per microsecond, used as it is */
    float carrier_i, carrier_q;         /* float32(amp cos phi), float32(amp sin phi) */
    float depth;                        /* of the tag's load modulation */
    float sigma;                        /* of the noise on I and on Q; 0: none */
    float full_scale;                   /* the quantised kinds: the integer value of 1.0 */
    uint32_t out_kind;                  /* NFC_IN_IQ_F32, NFC_IN_IQ_I16, NFC_IN_IQ_I8 or NFC_IN_IQ_U8 */
    uint64_t seed;
    const uint64_t *stream_seeds;       /* NULL: stream k's seed is k */
    uint32_t tail;                      /* idle samples behind a stream's last frame */
    uint32_t align_samples;             /* a power of two: every first_sample[k] is a multiple of it */
    uint32_t reserved[4];
} nfc_air_config;
int nfc_host_air_render(const nfc_air_config *cfg, const nfc_air_frame *frames, const uint32_t *frame_off /* [K + 1] */, const uint8_t *air,
                        const uint8_t *par, const uint32_t *byte_base /* [K + 1] */, size_t K, void *out, size_t cap_samples,
                        uint64_t *first_sample /* [K] */, uint32_t *n_samples /* [K] */);
int nfc_air_render_device(int device, const nfc_air_config *cfg, const nfc_air_frame *frames, const uint32_t *frame_off, const uint8_t *air,
                          const uint8_t *par, const uint32_t *byte_base, size_t K, void *dev_out, size_t cap_samples, uint64_t *first_sample,
                          uint32_t *n_samples, float *kernel_ms /* NULL, or two floats */);

/* ---- transmitting what the streams answer: K timed TX captures from one push (csrc/answers_tx.hip.h) ------------------
 * What tag_emulate / reader_emulate hand to binary_src -> multiplier -> the radio, for the answers of every stream of a tracked,
 * emulated push, rendered on the device from the tracking buffer: no answer byte goes through the host, no run table through HBM.
 * THE TWO TIMELINES.  r counts a stream's received samples since its last reset (a raw frame's idx as nfc_multi_fetch_commands gives
 * it); TX index T(r) = floor(r * rate_num / rate_den) in 64-bit integers (r * rate_num must stay below 2^64), rate_num / rate_den the
 * reduced ratio of output to input rate.  A push that gave a stream the samples [b, b + n) owns the TX span [T(b), T(b + n)): the spans
 * of consecutive pushes tile the TX timeline.
 * AN ANSWER's samples: its bits from air / par (n_bits 1 .. 8: a short frame from the low bits of its first byte; else a multiple of 9 up
 * to 162), the runs nfc_tx_encode gives for them -- NFC_TX_MANCHESTER for a tag card (idle level 0, usrp_nfc.py:75), NFC_TX_MILLER for
 * a reader card (idle level 1, usrp_nfc.py:45) -- and per run the samples nfc_tx_sample_count gives at samp_rate (binary_src.work's
 * rule, NOT the air interface's int(d * rate_msps)).  L: the answer's samples in all.
 * THE SCHEDULE of one stream and push: the pending entry carried in (if any), then the push's answers in order.  Entry j answers the
 * command whose raw frame closed at idx_j; it starts at S_j = T(idx_j) + delay_samples (a pending entry keeps its stored start), is cut
 * at C_j = T(idx_j+1), the moment the next answered command closed (never for the last entry), and owns [S_j, min(S_j + L_j, C_j)) --
 * which may be empty -- intersected with the push's span.  Every other sample of the span is the idle level.  Afterwards the stream's
 * pending entry is the last entry if its interval reaches beyond the span's end, else none: a stream carries at most one answer from
 * push to push, as long as it takes.  A push that is never transmitted drops its answers.
 * A SAMPLE is nfc_tx_render_device's: (level, 0) with the carrier off, else level * amp * exp(j 2 pi phase) with the phase of TX index
 * t taken from (first_index + t) * phase_inc in 64-bit fixed point (the device: sincospif of the top 24 bits, k_tx_render's own device
 * function; the twin: cos / sin in double, equal within 1.5e-7 of amp).  It depends on the stream's answers, the configuration and t
 * alone -- not on K, the stream's place, the tiling or how the pushes were cut.
 * THE LAYOUT is the air interface's: streams packed in stream order, first_sample[k] rounded up to align_samples, n_samples[k] =
 * T(b + n) - T(b), or 0 for a stream without a card, padding (0, 0); no byte of [0, first_sample[K-1] + n_samples[K-1]) is left
 * unwritten and none beyond is touched.  All sizes follow from the push's own arguments: no device read, no host wait.
 * NOT MODELLED: reader_emulate's REQA repeat after a HALT, tag_emulate's threshold / float-to-complex chain in front of the UHD sink;
 * ISO 14443-3 frame-delay conformance is not claimed (idx lies behind the frame's last pause by the decoder's timeout: DESIGN.md 8m).
 * ERRORS are NFC_ERR_ARG, raised before the device is touched, the argument's name in the message: a rate_num / rate_den outside
 * 1 .. 65 536, a samp_rate outside (0, 1e9], an align_samples that is no power of two (up to 2^20), a non-zero reserved word, a dev_out
 * that is not 32-byte aligned, a stream span above 2^30 samples; in the twin an n_bits outside the domain and bytes that leave the
 * stream's part.  A layout that needs more than cap_samples renders nothing, leaves every pending entry as it was, fills first_sample /
 * n_samples with the true need and is NFC_ERR_ARG naming cap_samples. */
typedef struct nfc_answers_tx_config {  /* 64 bytes */
    double samp_rate;                   /* of the output, Hz, in (0, 1e9] */
    double freq;                        /* of the carrier, Hz */
    uint64_t first_index;               /* carrier index of TX index 0 */
    uint64_t delay_samples;             /* from T(idx) to an answer's first sample */
    uint32_t rate_num, rate_den;        /* output rate : input rate, 1 .. 65 536 each */
    int32_t carrier;                    /* 0: (level, 0) */
    float amp;
    uint32_t align_samples;             /* a power of two: every first_sample[k] is a multiple of it */
    uint32_t reserved[3];               /* 0 */
} nfc_answers_tx_config;
typedef struct nfc_tx_pending {         /* 64 bytes, plain; n_bits == 0: none (then every byte is 0) */
    uint64_t start;                     /* S, a TX index */
    uint16_t n_bits;
    uint8_t role;                       /* NFC_EMU_TAG / NFC_EMU_READER: the encoding */
    uint8_t reserved0;
    uint32_t reserved1;
    uint8_t air[18], par[18];           /* zero behind the answer's bytes */
    uint8_t reserved2[12];
} nfc_tx_pending;
typedef struct nfc_tx_answer {          /* 16 bytes: the twin's input, one per answer */
    uint64_t idx;                       /* r of the answered command's raw frame */
    uint32_t byte_off;                  /* in the stream's part of air / par */
    uint32_t n_bits;
} nfc_tx_answer;
/* The CPU twin (no GPU needed).  role[k]: NFC_EMU_TAG, NFC_EMU_READER, or -1 for a stream without a card (no samples; its pending
 * entry is left alone); the push gave stream k the samples [rx_base[k], rx_base[k] + rx_n[k]); its answers are answers[ans_off[k] ..
 * ans_off[k + 1]), their bytes in air / par [byte_base[k] .. byte_base[k + 1]).  pending[K] is read and advanced in place.
 * out == NULL is the sizing call: it fills first_sample and n_samples and touches no pending entry. */
int nfc_host_answers_tx(const nfc_answers_tx_config *cfg, size_t K, const int32_t *role, const uint64_t *rx_base, const uint32_t *rx_n,
                        const uint32_t *ans_off /* [K + 1] */, const nfc_tx_answer *answers, const uint8_t *air, const uint8_t *par,
                        const uint32_t *byte_base /* [K + 1] */, nfc_tx_pending *pending /* [K] */, void *out, size_t cap_samples,
                        uint64_t *first_sample /* [K] */, uint32_t *n_samples /* [K] */);
/* Renders the last push's answers of every stream that holds a card into dev_out (complex64, cap_samples entries) and advances the
 * pending entries on the device: a schedule pass, a lane per stream, and a render pass over flat tiles of the packed output, enqueued
 * on the context's stream behind the machine kernel with no host wait.  kernel_ms: NULL, or TWO floats, the two passes' durations by
 * HIP events -- which implies the wait.  Once per push: a second call before the next push is NFC_ERR_STATE, as is a call with
 * tracking off, with no completed push (or a reset / set_state since), or with no stream holding a card.  A push in which nothing was
 * stored still renders: idle samples and whatever is pending.  The device sections of the call are followed by the guard word (the
 * test build's guard check covers them); a context that never calls this allocates and launches exactly what it did.
 * nfc_multi_get_tx_state / _set_tx_state: a stream's pending entry (set: NFC_ERR_ARG for an n_bits outside the domain, a role above 1,
 * a non-zero reserved byte); both complete the device first.  nfc_multi_reset(stream) and nfc_multi_emulate clear the stream's entry. */
int nfc_multi_transmit_device(nfc_multi *m, const nfc_answers_tx_config *cfg, void *dev_out, size_t cap_samples, uint64_t *first_sample,
                              uint32_t *n_samples, float *kernel_ms /* NULL, or two floats */);
int nfc_multi_get_tx_state(nfc_multi *m, uint32_t stream, nfc_tx_pending *st);
int nfc_multi_set_tx_state(nfc_multi *m, uint32_t stream, const nfc_tx_pending *st);

/* ---- the card rebuilt from what was heard: a memory image per stream -----------------------------------------------------------------
 * What an eavesdropper wants of a capture is the card.  An IMAGE belongs to one stream of a multi-stream context: 1 024 bytes `mem` (an
 * Ultralight uses the first 64), one source code per byte in `src` (0: never shown), a tag type (-1 until an ATQA is heard), sticky flags
 * and the count of known bytes.  It is built from the stream's command records in stream order -- nfc_frame and its `data` slot, as
 * k_multi_commands writes them -- by ONE text for host and device, csrc/image.hip.h:
 *   ATQA*                     set tag_type; another one than was set: NFC_IMG_TAG_CHANGED
 *   ANTI1U / ANTI2T / ANTI1G  bytes 0..3 / 4..8 / 0..4 (source ANTICOLL): the bytes an emulated tag sends from its memory
 *   READT                     only when the command IMMEDIATELY before it is a READR, whose first extra byte is the block / page `val`:
 *                             tag type 0: pages val .. val + 3, round the end of the 64 bytes (val > 0x0F: nothing).  Otherwise block val:
 *                             a data block whole; a trailer bytes [6, 10), and [10, 16) only where the access bits in this same answer
 *                             leave key B readable -- never [0, 6), which a card reads as zeros.  val >= 64: nothing, NFC_IMG_BEYOND
 *   RANDTB with AT_OK         behind AUTHA / AUTHB, RANDTA, RANDRB with AR_OK (either side of a nested authentication counts): the key
 *                             the machine held for (key type, sector of the AUTH's block) -- the table's slot where present, else key A /
 *                             key B, the rule of the key table above -- into [0, 6) (AUTHA) or [10, 16) (AUTHB) of that sector's trailer,
 *                             source KEY.  Sector >= 16: nothing, NFC_IMG_BEYOND
 *   WRITE / COMPW1 / COMPW2   nothing, NFC_IMG_SAW_WRITE: the image records what the card SAID and what the authentications proved;
 *                             applying writes is not built
 *   cmd < 0                   (UNKNOWN, PARITY_ERROR, NFC_CMD_CUT) nothing; the record still counts as "the command before"
 * Whatever is last in stream order wins a byte; a patch whose value differs from a byte that was already known sets NFC_IMG_CHANGED.
 * THE TAIL: beside the image its stream keeps the summaries of its last three commands -- cmd, type, flags, first extra byte --, tail[0]
 * the most recent, cmd NFC_CMD_UNKNOWN where there was none yet.  With it READR | READT and AUTH | nonce | {nr}{ar} | {at} may fall into
 * different pushes or calls: commands cut anywhere give the image of the whole.
 * nfc_host_card_image: the CPU twin (no GPU needed).  It advances `image` in place over n records; `data` holds data_len bytes, a record's
 * bytes at its byte_off; key_a / key_b and `table` (NULL: an empty one) are the machine's.  NFC_ERR_ARG: a null argument that is needed, an
 * image field out of range (tag_type, flags, a source code above 3, n_known other than the count of known bytes, a tail entry), a faulty
 * table, a record whose bytes lie outside data.
 * nfc_multi_track_images(m, on): off at create; on implies nfc_multi_track_commands(m, 1).  The images' buffer -- mem [K][1024] | src
 * [K][1024] | info [K] | tail [K][3], 2 112 bytes per stream, each section followed by the guard word -- is allocated, holding
 * nfc_card_image_init's images, by a context's FIRST call: a context that never switches it on allocates and launches what it always
 * did.  While it is on, a tracked push enqueues k_multi_images (csrc/image.hip.h) behind the machine kernel, a workgroup of one wave per
 * stream, with no host wait: four launches instead of three; a push in which nothing was stored launches nothing.  The images persist
 * on the device from push to push whether or not anybody fetches.  nfc_multi_fetch_commands is not affected.
 * nfc_multi_fetch_images: ONE copy of the buffer to pinned memory and one wait; a second call before the next push (or reset, or
 * nfc_multi_set_image) returns the same data and makes no device call.  Images never switched on: NFC_ERR_STATE.  ms_kernel: with
 * nfc_multi_set_timing(on), k_multi_images of the last push by HIP events, else 0.  The pointers live until the next
 * nfc_multi_fetch_images that copies, or nfc_multi_destroy.
 * nfc_multi_get_image / nfc_multi_set_image: one stream's image, tail included; both complete the device first, set checks the image as
 * the twin does.  nfc_multi_reset(stream) returns that stream's image and tail to nfc_card_image_init's.
 * Argument errors are NFC_ERR_ARG, raised before the device is touched.
 * COST: README.md, profiles/images_bench.json. */
#define NFC_IMG_BYTES 1024
#define NFC_IMG_TAIL 3
enum { NFC_IMG_SRC_UNKNOWN = 0, NFC_IMG_SRC_READ = 1, NFC_IMG_SRC_ANTICOLL = 2, NFC_IMG_SRC_KEY = 3 };   /* nfc_card_image.src */
enum { NFC_IMG_TAG_CHANGED = 1, NFC_IMG_CHANGED = 2, NFC_IMG_BEYOND = 4, NFC_IMG_SAW_WRITE = 8, NFC_IMG_FLAGS_ALL = 15 };   /* nfc_image_info.flags, sticky */
typedef struct nfc_image_cmd {      /* 16 bytes: what a command leaves to the three behind it */
    int32_t cmd;                    /* index for nfc_command_info, or NFC_CMD_* */
    uint32_t type, flags, val;      /* nfc_frame.type; NFC_FRAME_*; the first extra byte (0: none, or cmd < 0) */
} nfc_image_cmd;
typedef struct nfc_image_info {     /* 16 bytes */
    int32_t tag_type;               /* -1 none heard, 0 Ultralight, 1 Classic 1K, 2 Classic 4K, 3 DESFire */
    uint32_t flags;                 /* NFC_IMG_* */
    uint32_t n_known;               /* bytes of src that are not 0 */
    uint32_t reserved;              /* 0 */
} nfc_image_info;
typedef struct nfc_card_image {     /* 2 112 bytes */
    uint8_t mem[NFC_IMG_BYTES], src[NFC_IMG_BYTES];
    nfc_image_info info;
    nfc_image_cmd tail[NFC_IMG_TAIL];
} nfc_card_image;
typedef struct {
    const uint8_t *mem, *src;       /* [n_streams][1024] */
    const nfc_image_info *info;     /* [n_streams] */
    const nfc_image_cmd *tail;      /* [n_streams][3] */
    uint32_t n_streams, n_launches; /* of the last push: 4 with images, 0 when nothing was stored */
    uint64_t bytes_copied;          /* device -> host, of this call */
    double ms_kernel;
    uint64_t reserved[4];
} nfc_multi_images;
int nfc_card_image_init(nfc_card_image *image);   /* nothing known, no tag type, an empty tail */
int nfc_host_card_image(nfc_card_image *image, const nfc_frame *cmds, size_t n, const uint8_t *data, size_t data_len, const uint8_t key_a[6],
                        const uint8_t key_b[6], const nfc_fsm_key_table *table /* may be NULL */);
int nfc_multi_track_images(nfc_multi *m, int on);
int nfc_multi_fetch_images(nfc_multi *m, nfc_multi_images *out);
int nfc_multi_get_image(nfc_multi *m, uint32_t stream, nfc_card_image *image);
int nfc_multi_set_image(nfc_multi *m, uint32_t stream, const nfc_card_image *image);

/* one stream's boundary state, in the form an nfc_ctx exports and imports it */
int nfc_multi_get_state(nfc_multi *m, uint32_t stream, nfc_state_header *hdr, float *ring, size_t ring_cap, uint8_t *pending, size_t pending_cap);
int nfc_multi_set_state(nfc_multi *m, uint32_t stream, const nfc_state_header *hdr, const float *ring, size_t ring_len, const uint8_t *pending, size_t pending_len);
int nfc_multi_reset(nfc_multi *m, int64_t stream /* -1: every stream */);
int nfc_multi_get_stats(nfc_multi *m, nfc_multi_stats *out);
int nfc_multi_set_timing(nfc_multi *m, int on);   /* HIP events around the push's launches -> ms_kernels */

/* Device memory helpers so that a caller without HIP bindings (ctypes) can keep its input
 * resident in HBM and use nfc_push_device. */
int nfc_device_alloc(int device, size_t bytes, void **out);
int nfc_device_free(int device, void *p);
int nfc_device_upload(int device, void *dst, const void *src_host, size_t bytes);
int nfc_device_download(int device, void *dst_host, const void *src, size_t bytes);
/* The same for a caller that enqueues other libraries' work (an RCCL collective) next to a context's: a stream to share with
 * nfc_set_stream, a wait for it, a device-to-host copy on it, pinned host memory to copy into, a fill. */
int nfc_stream_create(int device, void **stream_out);
int nfc_stream_destroy(int device, void *stream);
int nfc_stream_sync(int device, void *stream);
int nfc_device_download_async(int device, void *dst_host, const void *src, size_t bytes, void *stream);
int nfc_device_fill(int device, void *dst, int byte_value, size_t bytes);
int nfc_host_alloc_pinned(size_t bytes, void **out);
int nfc_host_free_pinned(void *p);

/* Host-only helpers (no GPU needed): the duration LUTs the decode kernels use,
 * driven sequentially.  Used by the CPU test-suite to pin the tables to the
 * reference decoders' golden vectors.  type: 0 Manchester, 1 Miller. */
int nfc_host_decode_lut(const nfc_params *params, int type, const int8_t *cur, const int32_t *d, size_t n,
                        uint8_t *sym_out, size_t cap, size_t *n_out);
/* (type 2: Modified Miller through the decoder's QUOTIENT machine -- states that no sequence of transitions can tell apart are
 * one class, csrc/decoder_tables.h: miller_quotient -- which is what the speculative decode kernel walks: its state maps are
 * then 8 bytes.  Same symbols as type 1 by construction; the CPU suite checks it on the reference's decoder vectors.)
 * nfc_host_miller_classes: the class (0 .. n_classes - 1; 0xFF: a state no transition sequence reaches from the initial one)
 * and the canonical state of every one of the 16 Miller states (stage | has_started << 2 | prev << 3, miller.py:14-29).
 * The carried Miller state -- nfc_state_header.miller_state, the exported boundary state -- is always the canonical one:
 * `prev` reads 0 wherever the decoder cannot read it before writing it (miller.py:81 is its only read). */
int nfc_host_miller_classes(const nfc_params *params, uint8_t class_of[16], uint8_t canonical[16], int *n_classes);

/* The decoders themselves on the host, one transition at a time with any duration in microseconds (the walk the LUTs are
 * built from: csrc/decoder_tables.h), decoder state carried across calls in *state (0 before the first call; type 0
 * Manchester: manchester.py:30-61, type 1 Modified Miller: miller.py:153-197).  Behind usrp_nfc_amd.miller.miller_decoder /
 * manchester.manchester_decoder, the reference-named classes that keep `process_transition(list)`. */
int nfc_host_decode_steps(int type, const int8_t *cur, const double *dur_us, size_t n, int32_t *state, uint8_t *sym_out,
                          size_t cap, size_t *n_out);
/* the int16 -> float conversion of the NFC_IN_I16_SQ kernels, on the host (i16_scale as in nfc_params) */
float nfc_host_i16_to_float(int16_t pcm, float i16_scale);
/* How a batch of n samples is cut into the threshold stage's time chunks when the cut goes by dispatch row (csrc/chunk_cut.h; the
 * reference has no counterpart: its loop is one chunk, transition_sink.py:37-107 -- this is the parallel restatement's own geometry,
 * exposed so that the CPU suite can check it covers every sample exactly once).  C: the equal cut's chunk length, rs: samples per
 * round of the workgroup kernel (C a multiple of it), cus: compute units, rows: workgroups per CU (2 .. 4), factors: rows - 1 length
 * factors, max_len: longest chunk allowed (0: any).  out[0..3]: chunk length per row, out[4..7]: first sample per row, out[8]:
 * chunks per row, out[9]: chunks that begin inside the batch.  Returns 1 when the cut goes by row, 0 for the equal cut (the same
 * table with equal entries), negative on bad arguments.  Chunk c of row r = min(c / out[8], 3) covers
 * [out[4 + r] + (c - r * out[8]) * out[r], ... + out[r]) cut at n. */
int nfc_plan_row_cut(uint32_t n, uint32_t C, uint32_t rs, uint32_t cus, uint32_t rows, const double *factors, uint32_t max_len,
                     uint32_t out[10]);

#ifdef __cplusplus
}
#endif
#endif /* NFC_AMD_H */
