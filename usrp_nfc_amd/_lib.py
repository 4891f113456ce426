"""ctypes loader for libnfc_amd.so -- the C-ABI of include/nfc_amd.h.

There is no CPU implementation behind this package: if the shared library is
missing it is built with hipcc (usrp_nfc_amd/build.py); if that fails, or no GPU
is usable when a context is created, the caller gets an exception."""
import ctypes as C
import os

import numpy as np

from . import build as _build

NFC_IN_IQ_F32, NFC_IN_ENV_F32, NFC_IN_REAL_F32_SQ, NFC_IN_I16_SQ, NFC_IN_IQ_I16, NFC_IN_IQ_I8, NFC_IN_IQ_U8 = 0, 1, 2, 3, 4, 5, 6
NFC_FLAG_FORCE_SEQUENTIAL, NFC_FLAG_NO_EDGES = 1, 2
NFC_REC_ENVELOPE, NFC_REC_REAL_PART = 0, 1   # nfc_record_tap
ABI_VERSION = 4   # NFC_AMD_ABI_VERSION of the header these structures mirror
# per-stream flags of a multi-stream context (nfc_multi_get_counts)
NFC_MULTI_TRUNC_EDGES, NFC_MULTI_TRUNC_SYMBOLS, NFC_MULTI_TRUNC_PACKETS, NFC_MULTI_TRUNC_BITS, NFC_MULTI_PENDING_OVERFLOW = 1, 2, 4, 8, 16
# what nfc_multi_fetch brings to the host (PACKETS: the packet tables and the bit arrays), and its arrays in the order of off[]
NFC_MULTI_FETCH_EDGES, NFC_MULTI_FETCH_SYMBOLS, NFC_MULTI_FETCH_PACKETS, NFC_MULTI_FETCH_ALL = 1, 2, 4, 7
NFC_MF_EDGES, NFC_MF_SYM0, NFC_MF_SYM1, NFC_MF_PK0, NFC_MF_PK1, NFC_MF_BITS0, NFC_MF_BITS1, NFC_MF_ARRAYS = 0, 1, 2, 3, 4, 5, 6, 7


class Params(C.Structure):
    _fields_ = [('samp_rate', C.c_double), ('lo_val', C.c_double), ('hi_val', C.c_double),
                ('av_window', C.c_int32), ('max_len', C.c_int32), ('enable_reader', C.c_int32),
                ('enable_tag', C.c_int32), ('input_kind', C.c_int32), ('device', C.c_int32),
                ('i16_scale', C.c_float), ('flags', C.c_uint32), ('chunk_samples', C.c_int32),
                ('reserved', C.c_int32)]


class Counts(C.Structure):
    _fields_ = [('n_samples', C.c_uint64), ('n_edges', C.c_uint64), ('n_symbols', C.c_uint64 * 2),
                ('n_packets', C.c_uint64 * 2), ('n_packet_bits', C.c_uint64 * 2)]


class Stats(C.Structure):
    _fields_ = [('ms_total', C.c_double), ('ms_threshold', C.c_double), ('ms_edges', C.c_double),
                ('ms_decode', C.c_double), ('threshold_passes', C.c_uint32), ('chunks_rerun', C.c_uint32),
                ('used_sequential', C.c_uint32), ('n_chunks', C.c_uint32), ('bytes_in', C.c_uint64),
                ('ms_threshold_kernel', C.c_double * 6), ('n_threshold_timed', C.c_uint32), ('chunk_samples', C.c_uint32),
                ('ran_ahead', C.c_uint32), ('redone_total', C.c_uint32), ('ring_slots_carried', C.c_uint32), ('decode_respeculated', C.c_uint32),
                ('device_allocs', C.c_uint32), ('tail_fused', C.c_uint32), ('chunks_rerun_in_place', C.c_uint32)]


class MultiConfig(C.Structure):   # nfc_multi_config
    _fields_ = [('n_streams', C.c_uint32), ('max_push_samples', C.c_uint32), ('cap_edges', C.c_uint32), ('cap_symbols', C.c_uint32),
                ('cap_packets', C.c_uint32), ('cap_packet_bits', C.c_uint32), ('cap_pending_bits', C.c_uint32), ('reserved', C.c_uint32 * 9)]


class MultiStats(C.Structure):   # nfc_multi_stats
    _fields_ = [('ms_kernels', C.c_double), ('n_samples', C.c_uint64), ('bytes_in', C.c_uint64), ('n_launches', C.c_uint32),
                ('n_streams_truncated', C.c_uint32), ('n_fetches', C.c_uint32), ('n_reads_device', C.c_uint32), ('reserved', C.c_uint32 * 6)]


class MultiFetched(C.Structure):   # nfc_multi_fetched
    _fields_ = [('what', C.c_uint32), ('n_streams', C.c_uint32), ('edge_code_nd', C.c_uint32), ('n_launches', C.c_uint32),
                ('off', C.c_void_p * 7), ('base', C.c_void_p), ('edge_pos', C.c_void_p), ('edge_code', C.c_void_p),
                ('symbols', C.c_void_p * 2), ('packets', C.c_void_p * 2), ('packet_bits', C.c_void_p * 2), ('bytes_copied', C.c_uint64),
                ('ms_kernels', C.c_double), ('reserved', C.c_uint64 * 4)]


class MultiFrames(C.Structure):   # nfc_multi_frames
    _fields_ = [('n_streams', C.c_uint32), ('n_launches', C.c_uint32), ('frame_off', C.c_void_p * 2), ('byte_off', C.c_void_p * 2),
                ('base', C.c_void_p), ('frames', C.c_void_p * 2), ('bytes', C.c_void_p * 2), ('par', C.c_void_p * 2),
                ('bytes_copied', C.c_uint64), ('ms_kernels', C.c_double), ('reserved', C.c_uint64 * 4)]


class FsmState(C.Structure):   # nfc_fsm_state
    _fields_ = [('cur_cmd', C.c_int32), ('tag_type', C.c_int32), ('encrypted', C.c_int32), ('cur_key', C.c_int32), ('cipher', C.c_uint64),
                ('ar', C.c_uint8 * 4), ('at', C.c_uint8 * 4), ('key_a', C.c_uint8 * 6), ('key_b', C.c_uint8 * 6), ('uid_len', C.c_uint32),
                ('uid', C.c_uint8 * 32), ('flags', C.c_uint32), ('reserved', C.c_uint32)]


NFC_KEY_SECTORS = 40


class FsmKeyTable(C.Structure):   # nfc_fsm_key_table: key[key_type & 1][sector][6], present[key_type & 1][sector]
    _fields_ = [('key', C.c_uint8 * 6 * NFC_KEY_SECTORS * 2), ('present', C.c_uint8 * NFC_KEY_SECTORS * 2)]


class MultiCommands(C.Structure):   # nfc_multi_commands
    _fields_ = [('raw', MultiFrames), ('cmd_off', C.c_void_p), ('cbyte_off', C.c_void_p), ('cmd', C.c_void_p), ('src', C.c_void_p),
                ('data', C.c_void_p), ('enc', C.c_void_p), ('stream_flags', C.c_void_p), ('n_streams', C.c_uint32), ('n_launches', C.c_uint32),
                ('bytes_copied', C.c_uint64), ('ms_kernels', C.c_double), ('ms_machine', C.c_double), ('reserved', C.c_uint64 * 4)]


class CtxCommandCounters(C.Structure):   # nfc_ctx_command_counters
    _fields_ = [('n_segments', C.c_uint32), ('n_rerun_segments', C.c_uint32), ('n_rerun_frames', C.c_uint32), ('n_keydep_segments', C.c_uint32)]


class CtxCommands(C.Structure):   # nfc_ctx_commands
    _fields_ = [('cmd', C.c_void_p), ('src', C.c_void_p), ('data', C.c_void_p), ('enc', C.c_void_p), ('n_commands', C.c_uint64),
                ('n_bytes', C.c_uint64), ('flags', C.c_uint32), ('n_launches', C.c_uint32), ('counters', CtxCommandCounters),
                ('bytes_copied', C.c_uint64), ('ms_kernels', C.c_double), ('ms_frames', C.c_double), ('ms_merge', C.c_double), ('ms_walk', C.c_double),
                ('ms_resolve', C.c_double), ('reserved', C.c_uint64 * 4)]


class KeyConfig(C.Structure):   # nfc_key_config
    _fields_ = [('initial_capacity', C.c_uint64), ('max_capacity', C.c_uint64), ('max_batch', C.c_uint32), ('flags', C.c_uint32),
                ('reserved', C.c_uint32 * 2)]


class KeyStats(C.Structure):   # nfc_key_stats
    _fields_ = [('ms_kernels', C.c_double), ('ms_count', C.c_double), ('ms_fill', C.c_double), ('ms_probe', C.c_double),
                ('scratch_bytes', C.c_uint64), ('n_batches', C.c_uint32), ('n_grown', C.c_uint32), ('n_launches', C.c_uint32),
                ('reserved', C.c_uint32)]


class NestedConfig(C.Structure):   # nfc_nested_config
    _fields_ = [('search', KeyConfig), ('cand_first', C.c_uint32), ('cand_count', C.c_uint32), ('reserved', C.c_uint32 * 2)]


class ReaderKeyConfig(C.Structure):   # nfc_reader_key_config
    _fields_ = [('search', KeyConfig), ('stage_capacity', C.c_uint32), ('flags', C.c_uint32), ('reserved', C.c_uint32 * 2)]


class EmuState(C.Structure):   # nfc_emu_state
    _fields_ = [('halted', C.c_int32), ('selected', C.c_int32), ('auth', C.c_int32), ('auth_key', C.c_int32), ('auth_prosp', C.c_int32),
                ('at_set', C.c_int32), ('at', C.c_uint8 * 4), ('rand_idx', C.c_uint32), ('tag_type', C.c_int32), ('cur_addr', C.c_int32),
                ('auth_addr', C.c_int32), ('uid_len', C.c_uint32), ('uid', C.c_uint8 * 32), ('flags', C.c_uint32), ('reserved', C.c_uint32)]


class EmuCard(C.Structure):   # nfc_emu_card
    _fields_ = [('role', C.c_int32), ('tag_type', C.c_int32), ('mode', C.c_int32), ('mem_len', C.c_uint32), ('mem', C.c_void_p),
                ('rands', C.c_void_p), ('n_rands', C.c_uint32), ('reserved', C.c_uint32), ('key_a', C.c_uint8 * 6), ('key_b', C.c_uint8 * 6),
                ('reserved2', C.c_uint32), ('table', C.c_void_p)]


class MultiAnswers(C.Structure):   # nfc_multi_answers
    _fields_ = [('n_streams', C.c_uint32), ('emulated', C.c_uint32), ('n_answers', C.c_uint64), ('cmd_off', C.c_void_p), ('ans_n', C.c_void_p),
                ('ans', C.c_void_p), ('plain', C.c_void_p), ('air', C.c_void_p), ('par', C.c_void_p), ('reserved', C.c_uint64 * 4)]


class EmuConfig(C.Structure):   # nfc_emu_config
    _fields_ = [('link', C.c_uint32), ('rounds', C.c_uint32), ('cap_frames', C.c_uint32), ('cap_bytes', C.c_uint32), ('pair_cap_frames', C.c_void_p),
                ('reserved', C.c_uint32 * 2)]


class AirConfig(C.Structure):   # nfc_air_config
    _fields_ = [('rate_msps', C.c_double), ('carrier_i', C.c_float), ('carrier_q', C.c_float), ('depth', C.c_float), ('sigma', C.c_float),
                ('full_scale', C.c_float), ('out_kind', C.c_uint32), ('seed', C.c_uint64), ('stream_seeds', C.c_void_p), ('tail', C.c_uint32),
                ('align_samples', C.c_uint32), ('reserved', C.c_uint32 * 4)]


class AnswersTxConfig(C.Structure):   # nfc_answers_tx_config
    _fields_ = [('samp_rate', C.c_double), ('freq', C.c_double), ('first_index', C.c_uint64), ('delay_samples', C.c_uint64), ('rate_num', C.c_uint32),
                ('rate_den', C.c_uint32), ('carrier', C.c_int32), ('amp', C.c_float), ('align_samples', C.c_uint32), ('reserved', C.c_uint32 * 3)]


class TxPending(C.Structure):   # nfc_tx_pending
    _fields_ = [('start', C.c_uint64), ('n_bits', C.c_uint16), ('role', C.c_uint8), ('reserved0', C.c_uint8), ('reserved1', C.c_uint32),
                ('air', C.c_uint8 * 18), ('par', C.c_uint8 * 18), ('reserved2', C.c_uint8 * 12)]


class MultiImages(C.Structure):   # nfc_multi_images
    _fields_ = [('mem', C.c_void_p), ('src', C.c_void_p), ('info', C.c_void_p), ('tail', C.c_void_p), ('n_streams', C.c_uint32),
                ('n_launches', C.c_uint32), ('bytes_copied', C.c_uint64), ('ms_kernel', C.c_double), ('reserved', C.c_uint64 * 4)]


# the memory images (nfc_image_cmd, nfc_image_info, nfc_card_image as records), a byte's source codes and an image's sticky flags
NFC_IMG_BYTES, NFC_IMG_TAIL = 1024, 3
NFC_IMG_SRC_UNKNOWN, NFC_IMG_SRC_READ, NFC_IMG_SRC_ANTICOLL, NFC_IMG_SRC_KEY = 0, 1, 2, 3
NFC_IMG_TAG_CHANGED, NFC_IMG_CHANGED, NFC_IMG_BEYOND, NFC_IMG_SAW_WRITE = 1, 2, 4, 8
IMAGE_CMD_DTYPE = np.dtype([('cmd', '<i4'), ('type', '<u4'), ('flags', '<u4'), ('val', '<u4')])
IMAGE_INFO_DTYPE = np.dtype([('tag_type', '<i4'), ('flags', '<u4'), ('n_known', '<u4'), ('reserved', '<u4')])
CARD_IMAGE_DTYPE = np.dtype([('mem', 'u1', (NFC_IMG_BYTES,)), ('src', 'u1', (NFC_IMG_BYTES,)), ('info', IMAGE_INFO_DTYPE),
                             ('tail', IMAGE_CMD_DTYPE, (NFC_IMG_TAIL,))])
TX_PENDING_DTYPE = np.dtype([('start', '<u8'), ('n_bits', '<u2'), ('role', 'u1'), ('reserved0', 'u1'), ('reserved1', '<u4'), ('air', 'u1', (18,)),
                             ('par', 'u1', (18,)), ('reserved2', 'u1', (12,))])   # nfc_tx_pending as a record
TX_ANSWER_DTYPE = np.dtype([('idx', '<u8'), ('byte_off', '<u4'), ('n_bits', '<u4')])   # nfc_tx_answer
AIR_FRAME_DTYPE = np.dtype([('type', 'u1'), ('flags', 'u1'), ('n_bits', '<u2'), ('byte_off', '<u4'), ('idle_before', '<u4'),
                            ('reserved', '<u4')])   # nfc_air_frame
NFC_EMU_TAG, NFC_EMU_READER = 0, 1
NFC_EMU_REFERENCE, NFC_EMU_CARD = 0, 1
NFC_EMU_LINK_PLAIN, NFC_EMU_LINK_AIR = 0, 1
NFC_EMU_RAISED, NFC_EMU_UNEXPECTED, NFC_EMU_ERR_ONES, NFC_EMU_ERR_TWOS, NFC_EMU_ERR_THREES, NFC_EMU_UID_OVERFLOW = 1, 2, 4, 8, 16, 32
NFC_EMU_FRAME_SEED, NFC_EMU_FRAME_ENCRYPTED = 1, 2
NFC_EMU_PAIR_CUT_FRAMES, NFC_EMU_PAIR_CUT_BYTES, NFC_EMU_PAIR_RUNAWAY = 1, 2, 4
EMU_FRAME_DTYPE = np.dtype([('cmd', '<i2'), ('type', 'u1'), ('flags', 'u1'), ('byte_off', '<u4'), ('n_bytes', '<u2'), ('n_bits', '<u2'),
                            ('round', '<u4')])   # nfc_emu_frame
EMU_ANSWER_DTYPE = np.dtype([('src', '<u4'), ('cmd', '<i4'), ('byte_off', '<u4'), ('n_bytes', '<u2'), ('n_bits', '<u2'), ('flags', '<u4'),
                             ('reserved', '<u4')])   # nfc_emu_answer
EMU_RESULT_DTYPE = np.dtype([('n_frames', '<u4'), ('n_bytes', '<u4'), ('flags', '<u4'), ('rounds', '<u4'), ('tag_flags', '<u4'),
                             ('reader_flags', '<u4'), ('tag_fsm_flags', '<u4'), ('reader_fsm_flags', '<u4')])   # nfc_emu_pair_result


class Frame(C.Structure):   # nfc_frame
    _fields_ = [('cmd', C.c_int32), ('type', C.c_int32), ('byte_off', C.c_uint32), ('n_bytes', C.c_uint16),
                ('n_header', C.c_uint16), ('n_extra', C.c_uint16), ('n_crc', C.c_uint16), ('flags', C.c_uint32),
                ('n_enc', C.c_uint16), ('pad', C.c_uint16)]


class CommandInfo(C.Structure):   # nfc_command_info
    _fields_ = [('name', C.c_char * 8), ('stage', C.c_int32), ('type', C.c_int32), ('crc', C.c_int32),
                ('n_header', C.c_int32), ('n_extra', C.c_int32), ('xor_check', C.c_int32), ('header', C.c_uint8 * 2),
                ('pad', C.c_uint8 * 2)]


class StateHeader(C.Structure):
    _fields_ = [('n_seen', C.c_uint64), ('ss', C.c_double), ('last_low', C.c_int64), ('filled', C.c_int32),
                ('stable', C.c_int32), ('cur_state', C.c_int32), ('last_bit', C.c_int32), ('dur', C.c_int32),
                ('miller_state', C.c_int32), ('manch_state', C.c_int32), ('pkt_started', C.c_int32 * 2),
                ('n_pending_bits', C.c_uint32 * 2), ('av_window', C.c_int32), ('reserved', C.c_int32)]


TX_RUN_DTYPE = np.dtype([('level', '<i4'), ('pad', '<i4'), ('dur_us', '<f8')])   # nfc_tx_run
NFC_TX_SAME, NFC_TX_MANCHESTER, NFC_TX_MILLER = 0, 1, 2
EDGE_DTYPE = np.dtype([('idx', '<u8'), ('d', '<i4'), ('v', 'i1'), ('t', 'i1'), ('pad', '<i2')])
PACKET_DTYPE = np.dtype([('idx', '<u8'), ('bit_off', '<u8'), ('n_bits', '<u4'), ('type', '<i4')])
# nfc_raw_frame: a frame as the GPU assembles it, and its flags beside FRAME_EXTRA_ERROR (1) / FRAME_MANY_MORE_ERROR (2)
RAW_FRAME_DTYPE = np.dtype([('idx', '<u8'), ('byte_off', '<u4'), ('n_bits', '<u4'), ('n_bytes', '<u4'), ('flags', '<u4'), ('type', '<i4'),
                            ('reserved', '<u4')])
NFC_RAW_PARITY_OK, NFC_RAW_CRC_A_OK, NFC_RAW_CUT = 0x100, 0x200, 0x400
# nfc_fsm_state as a record (FsmState is its ctypes form), its sticky flags, and the record of a frame whose bits were cut
FSM_STATE_DTYPE = np.dtype([('cur_cmd', '<i4'), ('tag_type', '<i4'), ('encrypted', '<i4'), ('cur_key', '<i4'), ('cipher', '<u8'), ('ar', 'u1', (4,)),
                            ('at', 'u1', (4,)), ('key_a', 'u1', (6,)), ('key_b', 'u1', (6,)), ('uid_len', '<u4'), ('uid', 'u1', (32,)), ('flags', '<u4'),
                            ('reserved', '<u4')])
NFC_FSM_LOST, NFC_FSM_UID_OVERFLOW = 1, 2
KEY_TABLE_DTYPE = np.dtype([('key', 'u1', (2, NFC_KEY_SECTORS, 6)), ('present', 'u1', (2, NFC_KEY_SECTORS))])   # nfc_fsm_key_table as a record
NFC_CMD_CUT = -3
# nfc_auth_trace: one sniffed first authentication (words: byte 0 lowest), and nfc_key_result with its statuses
AUTH_DTYPE = np.dtype([('uid', '<u4'), ('nt', '<u4'), ('nr_enc', '<u4'), ('ar_enc', '<u4'), ('at_enc', '<u4'), ('par', '<u2'), ('key_type', 'u1'),
                       ('block', 'u1'), ('stream', '<u4'), ('frame', '<u4'), ('idx', '<u8')])
KEY_RESULT_DTYPE = np.dtype([('key', 'u1', (6,)), ('status', 'u1'), ('reserved', 'u1'), ('n_candidates', '<u4'), ('n_odd', '<u4'), ('n_even', '<u4'),
                             ('nr', '<u4')])
# nfc_nested_trace: one sniffed nested authentication (nt_enc for nt; par bits 12 .. 15: the ninth bits of {nt}), and nfc_nested_result
NESTED_DTYPE = np.dtype([('uid', '<u4'), ('nt_enc', '<u4'), ('nr_enc', '<u4'), ('ar_enc', '<u4'), ('at_enc', '<u4'), ('par', '<u2'), ('key_type', 'u1'),
                         ('block', 'u1'), ('stream', '<u4'), ('frame', '<u4'), ('idx', '<u8')])
NESTED_RESULT_DTYPE = np.dtype([('key', 'u1', (6,)), ('status', 'u1'), ('reserved', 'u1'), ('n_verified', '<u4'), ('n_nt', '<u4'), ('n_searched', '<u4'),
                                ('nt', '<u4'), ('nr', '<u4'), ('reserved2', '<u4'), ('n_odd', '<u8'), ('n_even', '<u8')])
NESTED_CANDS = 64
NFC_KEY_OK, NFC_KEY_NONE, NFC_KEY_AMBIGUOUS, NFC_KEY_OVERFLOW = 0, 1, 2, 3
NFC_KEY_TIMING = 1
# nfc_reader_pair: two reader-side first authentications of one key (at_enc and par bits 8 .. 11 ignored), and nfc_reader_key_result
READER_PAIR_DTYPE = np.dtype([('search', AUTH_DTYPE), ('check', AUTH_DTYPE)])
READER_KEY_RESULT_DTYPE = np.dtype([('key', 'u1', (6,)), ('status', 'u1'), ('pad', 'u1'), ('n_candidates', '<u4'), ('n_joined', '<u4'), ('n_odd', '<u4'),
                                    ('n_even', '<u4'), ('nr_search', '<u4'), ('nr_check', '<u4')])
NFC_RKEY_VERIFY_INLINE = 1
COUNTS_DTYPE = np.dtype([('n_samples', '<u8'), ('n_edges', '<u8'), ('n_symbols', '<u8', (2,)), ('n_packets', '<u8', (2,)),
                         ('n_packet_bits', '<u8', (2,))])   # nfc_counts

# every symbol include/nfc_amd.h declares
SYMBOLS = ['nfc_abi_version', 'nfc_device_count', 'nfc_create', 'nfc_destroy', 'nfc_last_error', 'nfc_push',
           'nfc_push_device', 'nfc_submit_device', 'nfc_wait', 'nfc_submitted', 'nfc_push_edges', 'nfc_sync', 'nfc_set_stream', 'nfc_get_counts', 'nfc_read_edges', 'nfc_read_edges_compact', 'nfc_read_symbols', 'nfc_read_packets',
           'nfc_read_packet_bits', 'nfc_read_val', 'nfc_get_state', 'nfc_set_state', 'nfc_reset', 'nfc_prime', 'nfc_export_state', 'nfc_get_stats', 'nfc_set_timing',
           'nfc_device_alloc', 'nfc_device_free', 'nfc_device_upload', 'nfc_device_download', 'nfc_stream_create', 'nfc_stream_destroy',
           'nfc_stream_sync', 'nfc_device_download_async', 'nfc_device_fill', 'nfc_host_alloc_pinned', 'nfc_host_free_pinned', 'nfc_host_decode_lut', 'nfc_host_miller_classes', 'nfc_host_decode_steps', 'nfc_host_i16_to_float', 'nfc_plan_row_cut',
           'nfc_fsm_create', 'nfc_fsm_destroy', 'nfc_fsm_reset', 'nfc_fsm_process', 'nfc_fsm_process_packets', 'nfc_fsm_process_outgoing', 'nfc_fsm_set_keys',
           'nfc_command_count', 'nfc_command_get', 'nfc_crc_a', 'nfc_tx_encode', 'nfc_tx_sample_count', 'nfc_tx_render_device',
           'nfc_record_pcm16_device', 'nfc_host_record_pcm16',
           'nfc_multi_create', 'nfc_multi_destroy', 'nfc_multi_last_error', 'nfc_multi_push_device', 'nfc_multi_push', 'nfc_multi_get_counts',
           'nfc_multi_read_edges', 'nfc_multi_read_symbols', 'nfc_multi_read_packets', 'nfc_multi_read_packet_bits', 'nfc_multi_get_state',
           'nfc_multi_set_state', 'nfc_multi_reset', 'nfc_multi_get_stats', 'nfc_multi_set_timing', 'nfc_multi_fetch', 'nfc_multi_get_counts_all',
           'nfc_get_frame_counts', 'nfc_read_frames', 'nfc_read_frame_bytes', 'nfc_host_frames', 'nfc_fsm_process_frames', 'nfc_multi_fetch_frames',
           'nfc_fsm_state_init', 'nfc_fsm_get_state', 'nfc_fsm_set_state', 'nfc_host_commands', 'nfc_multi_track_commands', 'nfc_multi_fetch_commands',
           'nfc_multi_set_keys', 'nfc_multi_get_fsm_state', 'nfc_multi_set_fsm_state',
           'nfc_sector_of_block', 'nfc_fsm_key_table_init', 'nfc_fsm_set_sector_key', 'nfc_fsm_get_key_table', 'nfc_fsm_set_key_table',
           'nfc_host_commands_keyed', 'nfc_multi_set_sector_keys', 'nfc_multi_get_sector_keys',
           'nfc_track_commands', 'nfc_read_commands', 'nfc_set_fsm_keys', 'nfc_set_fsm_sector_keys', 'nfc_get_fsm_sector_keys', 'nfc_get_fsm_state',
           'nfc_set_fsm_state', 'nfc_host_commands_segmented',
           'nfc_find_auths', 'nfc_host_recover_keys', 'nfc_recover_keys_device',
           'nfc_find_nested_auths', 'nfc_host_nested_candidates', 'nfc_nested_candidates_device', 'nfc_host_recover_nested_keys',
           'nfc_recover_nested_keys_device',
           'nfc_find_reader_auths', 'nfc_host_recover_reader_keys', 'nfc_recover_reader_keys_device',
           'nfc_emu_state_init', 'nfc_emu_last_error', 'nfc_host_emu_step', 'nfc_host_emulate', 'nfc_multi_emulate', 'nfc_multi_fetch_answers', 'nfc_multi_get_emu_state',
           'nfc_multi_set_emu_state', 'nfc_host_emulate_pairs', 'nfc_emulate_pairs_device',
           'nfc_host_air_render', 'nfc_air_render_device',
           'nfc_host_answers_tx', 'nfc_multi_transmit_device', 'nfc_multi_get_tx_state', 'nfc_multi_set_tx_state',
           'nfc_card_image_init', 'nfc_host_card_image', 'nfc_multi_track_images', 'nfc_multi_fetch_images', 'nfc_multi_get_image', 'nfc_multi_set_image']

_libs = {}


def lib_path():
    return _build.SO


def hooks_path():
    """The test build (-DNFC_TEST_HOOKS), built on demand: the NFC_DEBUG_* / NFC_TRACE switches only exist there."""
    return _build.build(hooks=True)


def load(path=None):
    """Load (building if needed) the shared library and declare its prototypes.  path: another build of the same ABI (the
    test build, a kernel experiment); default: NFC_AMD_LIB, else the in-tree product library."""
    path = path or os.environ.get('NFC_AMD_LIB') or _build.build()
    if path in _libs:
        return _libs[path]
    L = C.CDLL(path)
    vp, sz, psz = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    L.nfc_abi_version.restype = C.c_int
    if L.nfc_abi_version() != ABI_VERSION:   # (the ctypes structures below are written for exactly this header)
        raise RuntimeError('%s has ABI version %d, this package binds version %d of include/nfc_amd.h' % (path, L.nfc_abi_version(), ABI_VERSION))
    L.nfc_device_count.restype = C.c_int
    L.nfc_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.nfc_destroy.argtypes = [vp]
    L.nfc_destroy.restype = None
    L.nfc_last_error.argtypes = [vp]
    L.nfc_last_error.restype = C.c_char_p
    L.nfc_push.argtypes = [vp, vp, sz]
    L.nfc_push_device.argtypes = [vp, vp, sz]
    L.nfc_submit_device.argtypes = [vp, vp, sz]
    L.nfc_wait.argtypes = [vp]
    L.nfc_submitted.argtypes = [vp]
    L.nfc_sync.argtypes = [vp]
    L.nfc_push_edges.argtypes = [vp, vp, sz]
    L.nfc_set_stream.argtypes = [vp, vp]
    L.nfc_get_counts.argtypes = [vp, C.POINTER(Counts)]
    L.nfc_read_edges.argtypes = [vp, sz, vp, sz, psz]
    L.nfc_read_edges_compact.argtypes = [vp, sz, vp, vp, sz, psz]
    L.nfc_read_symbols.argtypes = [vp, C.c_int, sz, vp, sz, psz]
    L.nfc_read_packets.argtypes = [vp, C.c_int, vp, sz, psz]
    L.nfc_read_packet_bits.argtypes = [vp, C.c_int, sz, vp, sz, psz]
    L.nfc_read_val.argtypes = [vp, sz, vp, sz, psz]
    L.nfc_get_state.argtypes = [vp, C.POINTER(StateHeader), vp, sz, vp, sz]
    L.nfc_set_state.argtypes = [vp, C.POINTER(StateHeader), vp, sz, vp, sz]
    L.nfc_reset.argtypes = [vp]
    L.nfc_export_state.argtypes = [vp, vp, sz, psz]
    L.nfc_sync.argtypes = [vp]
    L.nfc_prime.argtypes = [vp, C.c_uint64, C.c_float]
    L.nfc_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.nfc_set_timing.argtypes = [vp, C.c_int]
    L.nfc_device_alloc.argtypes = [C.c_int, sz, C.POINTER(vp)]
    L.nfc_device_free.argtypes = [C.c_int, vp]
    L.nfc_device_upload.argtypes = [C.c_int, vp, vp, sz]
    L.nfc_device_download.argtypes = [C.c_int, vp, vp, sz]
    L.nfc_stream_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.nfc_stream_destroy.argtypes = [C.c_int, vp]
    L.nfc_stream_sync.argtypes = [C.c_int, vp]
    L.nfc_device_download_async.argtypes = [C.c_int, vp, vp, sz, vp]
    L.nfc_device_fill.argtypes = [C.c_int, vp, C.c_int, sz]
    L.nfc_host_alloc_pinned.argtypes = [sz, C.POINTER(vp)]
    L.nfc_host_free_pinned.argtypes = [vp]
    L.nfc_host_decode_lut.argtypes = [C.POINTER(Params), C.c_int, vp, vp, sz, vp, sz, psz]
    L.nfc_host_miller_classes.argtypes = [C.POINTER(Params), vp, vp, C.POINTER(C.c_int)]
    L.nfc_host_decode_steps.argtypes = [C.c_int, vp, vp, sz, C.POINTER(C.c_int32), vp, sz, psz]
    L.nfc_host_i16_to_float.argtypes = [C.c_int16, C.c_float]
    L.nfc_host_i16_to_float.restype = C.c_float
    L.nfc_plan_row_cut.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32)]
    L.nfc_plan_row_cut.restype = C.c_int
    L.nfc_fsm_create.argtypes = [C.POINTER(vp)]
    L.nfc_fsm_destroy.argtypes = [vp]
    L.nfc_fsm_destroy.restype = None
    L.nfc_fsm_reset.argtypes = [vp]
    L.nfc_fsm_process.argtypes = [vp, vp, sz, C.c_int, C.POINTER(Frame), vp, sz, vp]
    L.nfc_fsm_process_packets.argtypes = [vp, vp, sz, vp, vp, vp, vp, sz, psz, vp]
    L.nfc_fsm_process_outgoing.argtypes = [vp, vp, sz, C.c_int, vp]
    L.nfc_fsm_set_keys.argtypes = [vp, vp, vp]
    L.nfc_command_count.restype = C.c_int
    L.nfc_command_get.argtypes = [C.c_int, C.POINTER(CommandInfo)]
    L.nfc_crc_a.argtypes = [vp, sz, vp]
    L.nfc_tx_encode.argtypes = [C.c_int, vp, sz, vp, sz, psz]
    L.nfc_tx_sample_count.argtypes = [vp, sz, C.c_double, C.POINTER(C.c_uint64)]
    L.nfc_tx_render_device.argtypes = [C.c_int, vp, sz, C.c_double, C.c_int, C.c_double, C.c_float, C.c_uint64, vp, sz, psz,
                                       C.POINTER(C.c_float)]
    L.nfc_record_pcm16_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, vp, sz, C.c_float, vp, vp, C.POINTER(C.c_float)]
    L.nfc_host_record_pcm16.argtypes = [C.c_float, C.c_float]
    L.nfc_host_record_pcm16.restype = C.c_int16
    u32 = C.c_uint32
    L.nfc_multi_create.argtypes = [C.POINTER(Params), C.POINTER(MultiConfig), C.POINTER(vp)]
    L.nfc_multi_destroy.argtypes = [vp]
    L.nfc_multi_destroy.restype = None
    L.nfc_multi_last_error.argtypes = [vp]
    L.nfc_multi_last_error.restype = C.c_char_p
    L.nfc_multi_push_device.argtypes = [vp, vp, vp, vp]
    L.nfc_multi_push.argtypes = [vp, vp, vp]
    L.nfc_multi_get_counts.argtypes = [vp, u32, C.POINTER(Counts), C.POINTER(u32)]
    L.nfc_multi_read_edges.argtypes = [vp, u32, sz, vp, sz, psz]
    L.nfc_multi_read_symbols.argtypes = [vp, u32, C.c_int, sz, vp, sz, psz]
    L.nfc_multi_read_packets.argtypes = [vp, u32, C.c_int, vp, sz, psz]
    L.nfc_multi_read_packet_bits.argtypes = [vp, u32, C.c_int, sz, vp, sz, psz]
    L.nfc_multi_get_state.argtypes = [vp, u32, C.POINTER(StateHeader), vp, sz, vp, sz]
    L.nfc_multi_set_state.argtypes = [vp, u32, C.POINTER(StateHeader), vp, sz, vp, sz]
    L.nfc_multi_reset.argtypes = [vp, C.c_int64]
    L.nfc_multi_get_stats.argtypes = [vp, C.POINTER(MultiStats)]
    L.nfc_multi_set_timing.argtypes = [vp, C.c_int]
    L.nfc_multi_fetch.argtypes = [vp, u32, C.POINTER(MultiFetched)]
    L.nfc_multi_get_counts_all.argtypes = [vp, vp, vp]
    L.nfc_get_frame_counts.argtypes = [vp, vp, vp]
    L.nfc_read_frames.argtypes = [vp, C.c_int, vp, sz, psz]
    L.nfc_read_frame_bytes.argtypes = [vp, C.c_int, sz, vp, vp, sz, psz]
    L.nfc_host_frames.argtypes = [vp, sz, vp, C.c_int, vp, vp, vp, sz, psz]
    L.nfc_fsm_process_frames.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, psz, vp]
    L.nfc_multi_fetch_frames.argtypes = [vp, C.POINTER(MultiFrames)]
    L.nfc_fsm_state_init.argtypes = [C.POINTER(FsmState)]
    L.nfc_fsm_get_state.argtypes = [vp, C.POINTER(FsmState)]
    L.nfc_fsm_set_state.argtypes = [vp, C.POINTER(FsmState)]
    L.nfc_host_commands.argtypes = [C.POINTER(FsmState), vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, psz]
    L.nfc_multi_track_commands.argtypes = [vp, C.c_int]
    L.nfc_multi_fetch_commands.argtypes = [vp, C.POINTER(MultiCommands)]
    L.nfc_multi_set_keys.argtypes = [vp, C.c_int64, vp, vp]
    L.nfc_multi_get_fsm_state.argtypes = [vp, u32, C.POINTER(FsmState)]
    L.nfc_multi_set_fsm_state.argtypes = [vp, u32, C.POINTER(FsmState)]
    L.nfc_sector_of_block.argtypes = [C.c_int]
    L.nfc_fsm_key_table_init.argtypes = [C.POINTER(FsmKeyTable)]
    L.nfc_fsm_set_sector_key.argtypes = [vp, C.c_int, C.c_int, vp]
    L.nfc_fsm_get_key_table.argtypes = [vp, C.POINTER(FsmKeyTable)]
    L.nfc_fsm_set_key_table.argtypes = [vp, C.POINTER(FsmKeyTable)]
    L.nfc_host_commands_keyed.argtypes = [C.POINTER(FsmState), C.POINTER(FsmKeyTable), vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, psz]
    L.nfc_multi_set_sector_keys.argtypes = [vp, C.c_int64, C.POINTER(FsmKeyTable)]
    L.nfc_multi_get_sector_keys.argtypes = [vp, u32, C.POINTER(FsmKeyTable)]
    L.nfc_track_commands.argtypes = [vp, C.c_int]
    L.nfc_read_commands.argtypes = [vp, C.POINTER(CtxCommands)]
    L.nfc_set_fsm_keys.argtypes = [vp, vp, vp]
    L.nfc_set_fsm_sector_keys.argtypes = [vp, C.POINTER(FsmKeyTable)]
    L.nfc_get_fsm_sector_keys.argtypes = [vp, C.POINTER(FsmKeyTable)]
    L.nfc_get_fsm_state.argtypes = [vp, C.POINTER(FsmState)]
    L.nfc_set_fsm_state.argtypes = [vp, C.POINTER(FsmState)]
    L.nfc_host_commands_segmented.argtypes = [C.POINTER(FsmState), C.POINTER(FsmKeyTable), vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, psz, vp, sz,
                                              C.POINTER(CtxCommandCounters)]
    L.nfc_find_auths.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, psz]
    L.nfc_host_recover_keys.argtypes = [vp, sz, C.POINTER(KeyConfig), vp, C.POINTER(KeyStats)]
    L.nfc_recover_keys_device.argtypes = [C.c_int, vp, sz, C.POINTER(KeyConfig), vp, C.POINTER(KeyStats)]
    L.nfc_find_nested_auths.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, psz]
    L.nfc_host_nested_candidates.argtypes = [vp, vp, sz, psz]
    L.nfc_nested_candidates_device.argtypes = [C.c_int, vp, sz, vp, vp]
    L.nfc_host_recover_nested_keys.argtypes = [vp, sz, C.POINTER(NestedConfig), vp, C.POINTER(KeyStats)]
    L.nfc_recover_nested_keys_device.argtypes = [C.c_int, vp, sz, C.POINTER(NestedConfig), vp, C.POINTER(KeyStats)]
    L.nfc_find_reader_auths.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, psz]
    L.nfc_host_recover_reader_keys.argtypes = [vp, sz, C.POINTER(ReaderKeyConfig), vp, C.POINTER(KeyStats)]
    L.nfc_recover_reader_keys_device.argtypes = [C.c_int, vp, sz, C.POINTER(ReaderKeyConfig), vp, C.POINTER(KeyStats)]
    L.nfc_emu_state_init.argtypes = [C.POINTER(EmuState)]
    L.nfc_emu_last_error.restype = C.c_char_p
    L.nfc_host_emu_step.argtypes = [C.POINTER(EmuCard), C.POINTER(EmuState), C.c_int, vp, sz, C.POINTER(C.c_int), vp, psz]
    L.nfc_host_emulate.argtypes = [C.POINTER(FsmState), C.POINTER(FsmKeyTable), C.POINTER(EmuCard), C.POINTER(EmuState), vp, sz, vp, vp, vp, vp, vp, vp, vp,
                                   sz, psz, vp, vp, vp, vp, psz]
    L.nfc_multi_emulate.argtypes = [vp, C.c_int64, C.POINTER(EmuCard)]
    L.nfc_multi_fetch_answers.argtypes = [vp, C.POINTER(MultiAnswers)]
    L.nfc_multi_get_emu_state.argtypes = [vp, u32, C.POINTER(EmuState)]
    L.nfc_multi_set_emu_state.argtypes = [vp, u32, C.POINTER(EmuState)]
    L.nfc_host_emulate_pairs.argtypes = [vp, vp, sz, C.POINTER(EmuConfig), vp, vp, vp, vp, vp]
    L.nfc_emulate_pairs_device.argtypes = [C.c_int, vp, vp, sz, C.POINTER(EmuConfig), vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.nfc_host_air_render.argtypes = [C.POINTER(AirConfig), vp, vp, vp, vp, vp, sz, vp, sz, vp, vp]
    L.nfc_air_render_device.argtypes = [C.c_int, C.POINTER(AirConfig), vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, C.POINTER(C.c_float * 2)]
    L.nfc_host_answers_tx.argtypes = [C.POINTER(AnswersTxConfig), sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]
    L.nfc_multi_transmit_device.argtypes = [vp, C.POINTER(AnswersTxConfig), vp, sz, vp, vp, C.POINTER(C.c_float * 2)]
    L.nfc_multi_get_tx_state.argtypes = [vp, u32, C.POINTER(TxPending)]
    L.nfc_multi_set_tx_state.argtypes = [vp, u32, C.POINTER(TxPending)]
    L.nfc_card_image_init.argtypes = [vp]
    L.nfc_host_card_image.argtypes = [vp, vp, sz, vp, sz, vp, vp, C.POINTER(FsmKeyTable)]
    L.nfc_multi_track_images.argtypes = [vp, C.c_int]
    L.nfc_multi_fetch_images.argtypes = [vp, C.POINTER(MultiImages)]
    L.nfc_multi_get_image.argtypes = [vp, u32, vp]
    L.nfc_multi_set_image.argtypes = [vp, u32, vp]
    for name in SYMBOLS:
        getattr(L, name)
    _libs[path] = L
    return L
