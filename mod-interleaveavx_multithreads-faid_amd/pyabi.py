"""ctypes view of the C ABI in include/lnsfaid.h.

This is plumbing for tests/, bench.py and __graft_entry__.py: it declares the structs and the
entry points of liblnsfaid.so (the HIP product library) one-to-one and adds no logic of its own.
The library is loaded from csrc/ next to this file; a missing library is a hard error (there is
no CPU fallback in the product path).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "liblnsfaid.so")

GROUP = 32
MSG_REGISTERS, MSG_HBM = 1, 2  # lnsfaid_select_message_store
ZERO_SHIFT_ON, ZERO_SHIFT_OFF, ZERO_SHIFT_LOOP, ZERO_SHIFT_STATIC, ZERO_SHIFT_WINDOWED = 1, 2, 3, 4, 5  # lnsfaid_select_zero_shift
STOP_GROUP, STOP_CODEWORD = 0, 1  # lnsfaid_set_early_stop
SHORTEN_TAIL, SHORTEN_HEAD = 0, 1  # lnsfaid_decode_burst / lnsfaid_encode_burst: where the known zeros of a shortened codeword sit
LINE_HARD, LINE_LLR4 = 0, 1  # lnsfaid_decode_line: one bit / one 4-bit LLR per transmitted code bit
LINE_CAPTURE_UNCORRECTABLE, LINE_CAPTURE_WRONG = 1, 2  # lnsfaid_line_capture_*: bits of select and of a record's flags


class Code(C.Structure):
    _fields_ = [
        ("n_var", C.c_int32),
        ("n_check", C.c_int32),
        ("n_edges", C.c_int32),
        ("z", C.c_int32),
        ("puncture_tail", C.c_int32),
        ("nb_degres", C.c_int32),
        ("deg", C.POINTER(C.c_int32)),
        ("deg_rows", C.POINTER(C.c_int32)),
        ("pos_vn", C.POINTER(C.c_uint16)),
    ]


class Cfg(C.Structure):
    _fields_ = [
        ("decode_method", C.c_int32),
        ("max_iteration", C.c_int32),
        ("factor_1", C.c_int32),
        ("factor_2", C.c_int32),
        ("floor_err_count", C.c_int32),
        ("floor_iter_thresh", C.c_int32),
        ("ef_elimination", C.c_int32),
        ("max_bf_iter", C.c_int32),
        ("bf_L0", C.c_int32),
        ("bf_L1", C.c_int32),
        ("bf_alpha", C.c_int32),
        ("bf_delta", C.c_int32),
        ("regular_col_weight", C.c_int32),
        ("hard2_threshold", C.c_int32),
        ("bf_vote_cap", C.c_int32),
        ("v2c_map", C.c_int8 * 8 * 4 * 6),
        ("v2c_map_ef", C.c_int8 * 8 * 4 * 6),
    ]


class GroupStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("bf_iterations", C.c_int32)]


class CodewordStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("bf_iterations", C.c_int32), ("unsatisfied", C.c_int32)]


class LineStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("bf_iterations", C.c_int32), ("unsatisfied", C.c_int32), ("corrected", C.c_int32)]


# every symbol include/lnsfaid.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "lnsfaid_code_50gpon": (C.c_int, [C.POINTER(Code), C.POINTER(C.c_uint16), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lnsfaid_cfg_default": (C.c_int, [C.POINTER(Cfg), C.c_int32, C.c_int32]),
    "lnsfaid_cfg_table_preset": (C.c_int, [C.POINTER(Cfg), C.c_int32]),
    "lnsfaid_cfg_ef_elimination": (C.c_int, [C.POINTER(Cfg), C.c_int32]),
    "lnsfaid_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Code), C.POINTER(Cfg), C.c_int32, C.c_size_t]),
    "lnsfaid_destroy": (None, [C.c_void_p]),
    "lnsfaid_set_cfg": (C.c_int, [C.c_void_p, C.POINTER(Cfg)]),
    "lnsfaid_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_set_early_stop": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_early_stop": (C.c_int, [C.c_void_p]),
    "lnsfaid_decode_codewords": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_codewords_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_count_errors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "lnsfaid_count_errors_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "lnsfaid_decode_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_packed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_codewords_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_codewords_packed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_count_errors_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "lnsfaid_count_errors_packed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "lnsfaid_pack_llr4": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "lnsfaid_unpack_bits": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "lnsfaid_pack_bits": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "lnsfaid_decode_line": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_line_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lnsfaid_line_from_fixinput": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]),
    "lnsfaid_line_to_llr4": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_int32, C.c_int32, C.c_size_t, C.c_void_p]),
    "lnsfaid_encode_line": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_encode_line_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_encode_line_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_burst": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "lnsfaid_decode_burst_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "lnsfaid_encode_burst": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_encode_burst_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_encode_burst_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p,
                                            C.c_void_p]),
    "lnsfaid_burst_to_llr4": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p]),
    "lnsfaid_burst_words": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lnsfaid_line_payload_random_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p]),
    "lnsfaid_line_payload_random_host": (C.c_int, [C.POINTER(Code), C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p]),
    "lnsfaid_line_bsc_threshold": (C.c_int, [C.c_double, C.POINTER(C.c_uint32)]),
    "lnsfaid_line_bsc_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_uint64)]),
    "lnsfaid_line_bsc_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_uint64)]),
    "lnsfaid_line_count_errors_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64),
                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_line_count_errors_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_line_awgn_table": (C.c_int, [C.c_double, C.c_double, C.c_void_p]),
    "lnsfaid_line_soft_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_uint64)]),
    "lnsfaid_line_soft_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_uint64)]),
    "lnsfaid_burst_payload_random_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p]),
    "lnsfaid_burst_payload_random_host": (C.c_int, [C.POINTER(Code), C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p]),
    "lnsfaid_burst_bsc_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "lnsfaid_burst_bsc_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "lnsfaid_burst_soft_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "lnsfaid_burst_soft_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "lnsfaid_burst_count_errors_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_burst_count_errors_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_line_markov_thresholds": (C.c_int, [C.c_double, C.c_double, C.c_void_p]),
    "lnsfaid_line_markov_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_line_markov_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_line_capture_words": (C.c_int, [C.POINTER(Code), C.c_int32, C.POINTER(C.c_uint32)]),
    "lnsfaid_line_capture_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_int32,
                                              C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_line_capture_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_int32,
                                            C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_frontend_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_size_t, C.c_int32,
                                          C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "lnsfaid_frontend_device_states": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_size_t, C.c_int32,
                                                 C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "lnsfaid_frontend_draws_per_group": (C.c_uint64, [C.c_void_p, C.c_int32]),
    "lnsfaid_frontend_set_interleave": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_demap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_float, C.c_void_p]),
    "lnsfaid_demap_packed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_float, C.c_void_p]),
    "lnsfaid_demap_host": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_float, C.c_void_p]),
    "lnsfaid_demap_packed_host": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_float, C.c_void_p]),
    "lnsfaid_prefec_errors_host": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_int32,
                                             C.POINTER(C.c_uint64)]),
    "lnsfaid_prefec_errors_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]),
    "lnsfaid_frontend_set_prefec": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_frontend_prefec_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]),
    "lnsfaid_capture_errors_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                                C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_capture_errors_host": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_frontend_sent_bits": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "lnsfaid_fec_status_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_fec_status_packed_host": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_fec_status_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_fec_status_packed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lnsfaid_frontend_set_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "lnsfaid_frontend_input_bits": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "lnsfaid_code_parity_inverse": (C.c_int, [C.POINTER(Code), C.c_void_p, C.c_size_t]),
    "lnsfaid_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lnsfaid_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lnsfaid_frontend_random_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]),
    "lnsfaid_io_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "lnsfaid_read_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "lnsfaid_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "lnsfaid_host_unregister": (C.c_int, [C.c_void_p]),
    "lnsfaid_comm_unique_id": (C.c_int, [C.c_void_p]),
    "lnsfaid_comm_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lnsfaid_comm_attach": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lnsfaid_comm_destroy": (C.c_int, [C.c_void_p]),
    "lnsfaid_allreduce_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "lnsfaid_select_kernel": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_kernel_rows_per_lane": (C.c_int, [C.c_void_p]),
    "lnsfaid_select_waves": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_frontend_set_exact": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_frontend_fastpath_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "lnsfaid_kernel_waves": (C.c_int, [C.c_void_p]),
    "lnsfaid_select_message_store": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_message_store": (C.c_int, [C.c_void_p]),
    "lnsfaid_select_zero_shift": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_zero_shift_groups": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    "lnsfaid_window_free": (C.c_int, [C.c_void_p]),
    "lnsfaid_select_edge_words": (C.c_int, [C.c_void_p, C.c_int32]),
    "lnsfaid_edge_words": (C.c_int, [C.c_void_p]),
    "lnsfaid_code_zero_shift_order": (C.c_int, [C.POINTER(Code), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lnsfaid_code_bf_walk": (C.c_int, [C.POINTER(Code), C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_int32)]),
    "lnsfaid_kernel_residency": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lnsfaid_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int32]),
    "lnsfaid_stream": (C.c_void_p, [C.c_void_p]),
    "lnsfaid_strerror": (C.c_char_p, [C.c_int]),
    "lnsfaid_last_hip_error": (C.c_char_p, []),
    "lnsfaid_version": (C.c_char_p, []),
}


def bind(lib, symbols):
    for name, (res, args) in symbols.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def load():
    """Load liblnsfaid.so (built by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(no CPU fallback exists in the product path)" % LIB_PATH)
        _lib = bind(C.CDLL(LIB_PATH), SYMBOLS)
    return _lib


class Code50GPON:
    """The built-in 50G-PON code, expanded to the Constants_SSE.h table format, with its buffers kept alive."""

    def __init__(self, lib=None):
        lib = lib or load()
        self.pos_vn = (C.c_uint16 * 70400)()
        self.deg = (C.c_int32 * 3)()
        self.deg_rows = (C.c_int32 * 3)()
        self.code = Code()
        rc = lib.lnsfaid_code_50gpon(C.byref(self.code), self.pos_vn, self.deg, self.deg_rows)
        if rc != 0:
            raise RuntimeError("lnsfaid_code_50gpon failed: %d" % rc)

    @property
    def N(self):
        return self.code.n_var

    @property
    def M(self):
        return self.code.n_check

    @property
    def K(self):
        return self.code.n_var - self.code.n_check


def code_zero_shift_order(code, lib=None):
    """lnsfaid_code_zero_shift_order (no GPU needed): per layer, the leading groups of four zero-shift edges and the edge order
    of the rotation-free tables as indices into the code's own row"""
    lib = lib or load()
    groups, order = (C.c_int32 * 32)(), (C.c_int32 * (32 * 24))()
    nbr = lib.lnsfaid_code_zero_shift_order(C.byref(code), groups, order)
    if nbr < 0:
        raise ValueError("lnsfaid_code_zero_shift_order failed: %d" % nbr)
    return list(groups[:nbr]), [[j for j in order[br * 24:br * 24 + 24] if j >= 0] for br in range(nbr)]


def code_bf_walk(code, col_weight, lib=None):
    """lnsfaid_code_bf_walk (no GPU needed): the syndrome walk tables (full, flipped, fixed) as uint32 arrays [layers][slots][8][2]
    and info = (hard plane offset, zero word offset, slots of `flipped`, fits, block columns of that weight)"""
    import numpy as np
    lib = lib or load()
    full, fixed = np.zeros((32, 24, 8, 2), np.uint32), np.zeros((32, 24, 8, 2), np.uint32)
    flipped = np.zeros((32 * 24 * 8 * 2,), np.uint32)  # at least [32][info[2]][8][2]
    info = (C.c_int32 * 5)()
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    nbr = lib.lnsfaid_code_bf_walk(C.byref(code), col_weight, u32(full), u32(flipped), u32(fixed), info)
    if nbr < 0:
        raise ValueError("lnsfaid_code_bf_walk failed: %d" % nbr)
    slots = info[2]
    return full[:nbr], flipped[:nbr * slots * 16].reshape(nbr, slots, 8, 2), fixed[:nbr], tuple(info)


def default_cfg(method, max_iter, lib=None):
    lib = lib or load()
    cfg = Cfg()
    rc = lib.lnsfaid_cfg_default(C.byref(cfg), method, max_iter)
    if rc != 0:
        raise ValueError("lnsfaid_cfg_default(%d, %d) failed: %d" % (method, max_iter, rc))
    return cfg


def pack_llr4(fix_input, lib=None):
    """lnsfaid_pack_llr4: int8 fixInput (values in [-8, 7]) -> uint8 llr4, two elements per byte"""
    import numpy as np
    lib = lib or load()
    fix_input = np.ascontiguousarray(fix_input, dtype=np.int8)
    out = np.empty(fix_input.size // 2, dtype=np.uint8)
    rc = lib.lnsfaid_pack_llr4(fix_input.ctypes.data, fix_input.size, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_pack_llr4 failed: %d" % rc)
    return out


def unpack_bits(bits, lib=None):
    """lnsfaid_unpack_bits: packed decisions (uint32 words) -> int8 0/1, one byte per bit"""
    import numpy as np
    lib = lib or load()
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    out = np.empty(bits.size * 32, dtype=np.int8)
    rc = lib.lnsfaid_unpack_bits(bits.ctypes.data, out.size, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_unpack_bits failed: %d" % rc)
    return out


def pack_bits(input_bits, lib=None):
    """lnsfaid_pack_bits: int8 0/1 message bits -> uint8, eight per byte, bit b of byte i = input_bits[8 i + b]"""
    import numpy as np
    lib = lib or load()
    input_bits = np.ascontiguousarray(input_bits, dtype=np.int8)
    out = np.empty(input_bits.size // 8, dtype=np.uint8)
    rc = lib.lnsfaid_pack_bits(input_bits.ctypes.data, input_bits.size, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_pack_bits failed: %d" % rc)
    return out


def line_stats_dtype():
    """numpy view of lnsfaid_line_stats"""
    import numpy as np
    return np.dtype([("iterations", np.int32), ("bf_iterations", np.int32), ("unsatisfied", np.int32), ("corrected", np.int32)])


def line_sizes(code, fmt):
    """(elements of `line` per codeword, their numpy type, payload words per codeword) for a Code struct and a format"""
    import numpy as np
    L, K = code.n_var - code.puncture_tail, code.n_var - code.n_check
    return (L // 32, np.uint32, K // 32) if fmt == LINE_HARD else (L // 2, np.uint8, K // 32)


def line_from_fixinput(code, fix_input, n_codewords, fmt, lib=None):
    """lnsfaid_line_from_fixinput: int8 fixInput of ceil(n_codewords / 32) groups -> line (uint32 words for LINE_HARD, uint8 for
    LINE_LLR4) of n_codewords codewords; code is a Code struct (Code50GPON().code)"""
    import numpy as np
    lib = lib or load()
    fix_input = np.ascontiguousarray(fix_input, dtype=np.int8)
    groups = (n_codewords + GROUP - 1) // GROUP
    if fix_input.size != groups * GROUP * code.n_var:
        raise ValueError("lnsfaid_line_from_fixinput: fix_input has %d bytes, not %d" % (fix_input.size, groups * GROUP * code.n_var))
    per, dtype, _ = line_sizes(code, fmt)
    out = np.empty(n_codewords * per, dtype=dtype)
    rc = lib.lnsfaid_line_from_fixinput(C.byref(code), fix_input.ctypes.data, n_codewords, fmt, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_line_from_fixinput failed: %d" % rc)
    return out


def line_to_llr4(code, line, fmt, magnitude, n_codewords, lib=None):
    """lnsfaid_line_to_llr4: line -> uint8 llr4 of ceil(n_codewords / 32) groups (what lnsfaid_decode_line* decodes)"""
    import numpy as np
    lib = lib or load()
    per, dtype, _ = line_sizes(code, fmt)
    line = np.ascontiguousarray(line, dtype=dtype)
    if line.size != n_codewords * per:
        raise ValueError("lnsfaid_line_to_llr4: line has %d elements, not %d" % (line.size, n_codewords * per))
    groups = (n_codewords + GROUP - 1) // GROUP
    out = np.empty(groups * GROUP * code.n_var // 2, dtype=np.uint8)
    rc = lib.lnsfaid_line_to_llr4(C.byref(code), line.ctypes.data, fmt, magnitude, n_codewords, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_line_to_llr4 failed: %d" % rc)
    return out


def code_parity_inverse(code, lib=None):
    """lnsfaid_code_parity_inverse: the compact B^-1 of a Code struct as uint8 [mb * mb * z / 8]; ValueError with the library's code
    (-2 for a singular parity part)"""
    import numpy as np
    lib = lib or load()
    mb = code.n_check // code.z
    circ = np.zeros(mb * mb * code.z // 8, dtype=np.uint8)
    rc = lib.lnsfaid_code_parity_inverse(C.byref(code), circ.ctypes.data, circ.size)
    if rc != 0:
        raise ValueError("lnsfaid_code_parity_inverse failed: %d" % rc)
    return circ


def encode_line_host(code, payload, n_codewords, with_bits=False, lib=None, circ=None):
    """lnsfaid_encode_line_host: payload uint32 [n_codewords, K / 32] -> (line uint32 [n_codewords, L / 32], the whole codewords
    uint32 [n_codewords, n_var / 32] or None); code is a Code struct.  B^-1 is derived with lnsfaid_code_parity_inverse unless the
    caller passes the `circ` of an earlier code_parity_inverse(code)."""
    import numpy as np
    lib = lib or load()
    if circ is None:
        circ = code_parity_inverse(code, lib)
    L, K = code.n_var - code.puncture_tail, code.n_var - code.n_check
    payload = np.ascontiguousarray(payload, dtype=np.uint32)
    if payload.size != n_codewords * (K // 32):
        raise ValueError("lnsfaid_encode_line_host: payload has %d words, not %d" % (payload.size, n_codewords * (K // 32)))
    line = np.empty((n_codewords, L // 32), dtype=np.uint32)
    bits = np.empty((n_codewords, code.n_var // 32), dtype=np.uint32) if with_bits else None
    rc = lib.lnsfaid_encode_line_host(C.byref(code), circ.ctypes.data, circ.size, payload.ctypes.data, n_codewords, line.ctypes.data,
                                      bits.ctypes.data if with_bits else None)
    if rc != 0:
        raise ValueError("lnsfaid_encode_line_host failed: %d" % rc)
    return line, bits


def _shortened(shortened, n_codewords):
    """None, or S_c in bits per codeword as a contiguous uint32 array (a host array in every form)"""
    import numpy as np
    if shortened is None:
        return None
    shortened = np.ascontiguousarray(shortened, dtype=np.uint32)
    if shortened.size != n_codewords:
        raise ValueError("shortened has %d entries, not %d" % (shortened.size, n_codewords))
    return shortened


def burst_words(code, shortened, n_codewords, lib=None):
    """lnsfaid_burst_words: (bits of the burst line, bits of the burst payload) of n_codewords codewords shortened by `shortened`
    (uint32 [n_codewords] in bits, or None for all zero); ValueError for an entry the rule refuses"""
    lib = lib or load()
    shortened = _shortened(shortened, n_codewords)
    lb, pb = C.c_uint64(0), C.c_uint64(0)
    rc = lib.lnsfaid_burst_words(C.byref(code), None if shortened is None else shortened.ctypes.data, n_codewords,
                                 C.cast(C.byref(lb), C.c_void_p), C.cast(C.byref(pb), C.c_void_p))
    if rc != 0:
        raise ValueError("lnsfaid_burst_words failed: %d" % rc)
    return lb.value, pb.value


def burst_to_llr4(code, line, fmt, magnitude, shortened, where, n_codewords, lib=None):
    """lnsfaid_burst_to_llr4: burst line (uint32 words for LINE_HARD, uint8 for LINE_LLR4) -> uint8 llr4 of ceil(n_codewords / 32)
    groups: what lnsfaid_decode_burst* decodes"""
    import numpy as np
    lib = lib or load()
    shortened = _shortened(shortened, n_codewords)
    line_bits, _ = burst_words(code, shortened, n_codewords, lib)
    line = np.ascontiguousarray(line, dtype=np.uint32 if fmt == LINE_HARD else np.uint8)
    if line.size != (line_bits // 32 if fmt == LINE_HARD else line_bits // 2):
        raise ValueError("lnsfaid_burst_to_llr4: line has %d elements for %d positions" % (line.size, line_bits))
    groups = (n_codewords + GROUP - 1) // GROUP
    out = np.empty(groups * GROUP * code.n_var // 2, dtype=np.uint8)
    rc = lib.lnsfaid_burst_to_llr4(C.byref(code), line.ctypes.data, fmt, magnitude, None if shortened is None else shortened.ctypes.data,
                                   where, n_codewords, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_burst_to_llr4 failed: %d" % rc)
    return out


def encode_burst_host(code, payload, shortened, where, n_codewords, with_bits=False, lib=None, circ=None):
    """lnsfaid_encode_burst_host: burst payload (flat uint32) -> (burst line, flat uint32 in the LINE_HARD format, the whole mother
    codewords uint32 [n_codewords, n_var / 32] or None).  circ as encode_line_host"""
    import numpy as np
    lib = lib or load()
    if circ is None:
        circ = code_parity_inverse(code, lib)
    shortened = _shortened(shortened, n_codewords)
    line_bits, payload_bits = burst_words(code, shortened, n_codewords, lib)
    payload = np.ascontiguousarray(payload, dtype=np.uint32)
    if payload.size != payload_bits // 32:
        raise ValueError("lnsfaid_encode_burst_host: payload has %d words, not %d" % (payload.size, payload_bits // 32))
    line = np.empty(line_bits // 32, dtype=np.uint32)
    bits = np.empty((n_codewords, code.n_var // 32), dtype=np.uint32) if with_bits else None
    rc = lib.lnsfaid_encode_burst_host(C.byref(code), circ.ctypes.data, circ.size, payload.ctypes.data,
                                       None if shortened is None else shortened.ctypes.data, where, n_codewords, line.ctypes.data,
                                       bits.ctypes.data if with_bits else None)
    if rc != 0:
        raise ValueError("lnsfaid_encode_burst_host failed: %d" % rc)
    return line, bits


def line_bsc_threshold(p, lib=None):
    """lnsfaid_line_bsc_threshold: floor(p * 2^32) for 0 <= p < 1; ValueError otherwise"""
    lib = lib or load()
    t = C.c_uint32()
    rc = lib.lnsfaid_line_bsc_threshold(float(p), C.byref(t))
    if rc != 0:
        raise ValueError("lnsfaid_line_bsc_threshold(%r) failed: %d" % (p, rc))
    return t.value


def line_payload_random_host(code, key, first_codeword, n_codewords, lib=None):
    """lnsfaid_line_payload_random_host: the payload uint32 [n_codewords, K / 32] of codewords first_codeword .. of stream `key`;
    code is a Code struct"""
    import numpy as np
    lib = lib or load()
    out = np.empty((n_codewords, (code.n_var - code.n_check) // 32), dtype=np.uint32)
    rc = lib.lnsfaid_line_payload_random_host(C.byref(code), key, first_codeword, n_codewords, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_line_payload_random_host failed: %d" % rc)
    return out


def line_bsc_host(code, line, n_codewords, key, first_codeword, threshold, in_place=False, total=0, lib=None):
    """lnsfaid_line_bsc_host: line uint32 [n_codewords, L / 32] (LINE_HARD) through the binary symmetric channel of stream `key`.
    Returns (line out, flips uint32 [n_codewords], total + the positions inverted); in_place writes into `line` itself"""
    import numpy as np
    lib = lib or load()
    per = (code.n_var - code.puncture_tail) // 32
    if not in_place:
        line = np.ascontiguousarray(line, dtype=np.uint32)
    if line.dtype != np.uint32 or not line.flags.c_contiguous or line.size != n_codewords * per:
        raise ValueError("lnsfaid_line_bsc_host: line must be contiguous uint32 with %d words" % (n_codewords * per))
    out = line if in_place else np.empty_like(line)
    flips = np.zeros(n_codewords, dtype=np.uint32)
    t = C.c_uint64(total)
    rc = lib.lnsfaid_line_bsc_host(C.byref(code), line.ctypes.data, n_codewords, key, first_codeword, threshold, out.ctypes.data,
                                   flips.ctypes.data, C.byref(t))
    if rc != 0:
        raise ValueError("lnsfaid_line_bsc_host failed: %d" % rc)
    return out, flips, t.value


def _soft_table(table):
    """fourteen thresholds as a contiguous uint32 array (the library checks their order)"""
    import numpy as np
    table = np.ascontiguousarray(table, dtype=np.uint32)
    if table.size != 14:
        raise ValueError("a soft-channel table has 14 thresholds, not %d" % table.size)
    return table


def line_awgn_table(sigma, scale, lib=None):
    """lnsfaid_line_awgn_table: the uint32 [14] thresholds of +-1 + N(0, sigma^2) behind the 4-bit quantiser at `scale`; ValueError
    for a sigma or scale that is not finite and positive"""
    import numpy as np
    lib = lib or load()
    table = np.zeros(14, dtype=np.uint32)
    rc = lib.lnsfaid_line_awgn_table(float(sigma), float(scale), table.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_line_awgn_table(%r, %r) failed: %d" % (sigma, scale, rc))
    return table


def line_soft_host(code, line, n_codewords, key, first_codeword, table, total=0, lib=None):
    """lnsfaid_line_soft_host: line uint32 [n_codewords, L / 32] (LINE_HARD) through the soft channel of stream `key` and `table`.
    Returns (llr4 uint8 [n_codewords, L / 2] (LINE_LLR4), flips uint32 [n_codewords], total + the flips of the call)"""
    import numpy as np
    lib = lib or load()
    L = code.n_var - code.puncture_tail
    line = np.ascontiguousarray(line, dtype=np.uint32)
    if line.size != n_codewords * (L // 32):
        raise ValueError("lnsfaid_line_soft_host: line has %d words, not %d" % (line.size, n_codewords * (L // 32)))
    table = _soft_table(table)
    out = np.empty((n_codewords, L // 2), dtype=np.uint8)
    flips = np.zeros(n_codewords, dtype=np.uint32)
    t = C.c_uint64(total)
    rc = lib.lnsfaid_line_soft_host(C.byref(code), line.ctypes.data, n_codewords, key, first_codeword, table.ctypes.data, out.ctypes.data,
                                    flips.ctypes.data, C.byref(t))
    if rc != 0:
        raise ValueError("lnsfaid_line_soft_host failed: %d" % rc)
    return out, flips, t.value


def _markov_t(t):
    """{ t_idle, t_after, t_start } as a contiguous uint32 array (the library checks their order)"""
    import numpy as np
    t = np.ascontiguousarray(t, dtype=np.uint32)
    if t.size != 3:
        raise ValueError("an error-propagation channel has 3 thresholds, not %d" % t.size)
    return t


def line_markov_thresholds(ber, propagation, lib=None):
    """lnsfaid_line_markov_thresholds: uint32 [3] { t_idle, t_after, t_start } of the stationary chain with marginal error
    probability `ber` and P(error | error before) = `propagation`; ValueError unless 0 <= ber <= propagation < 1"""
    import numpy as np
    lib = lib or load()
    t = np.zeros(3, dtype=np.uint32)
    rc = lib.lnsfaid_line_markov_thresholds(float(ber), float(propagation), t.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_line_markov_thresholds(%r, %r) failed: %d" % (ber, propagation, rc))
    return t


def line_markov_host(code, line, n_codewords, key, first_codeword, t, total=0, total_runs=0, lib=None):
    """lnsfaid_line_markov_host: line uint32 [n_codewords, L / 32] (LINE_HARD) through the error-propagation channel of stream `key`
    and thresholds `t`.  Returns (line out, flips uint32 [n_codewords], runs uint32 [n_codewords], total + the positions inverted,
    total_runs + the runs of the call)"""
    import numpy as np
    lib = lib or load()
    per = (code.n_var - code.puncture_tail) // 32
    line = np.ascontiguousarray(line, dtype=np.uint32)
    if line.size != n_codewords * per:
        raise ValueError("lnsfaid_line_markov_host: line has %d words, not %d" % (line.size, n_codewords * per))
    t = _markov_t(t)
    out = np.empty_like(line)
    flips = np.zeros(n_codewords, dtype=np.uint32)
    runs = np.zeros(n_codewords, dtype=np.uint32)
    tf, tr = C.c_uint64(total), C.c_uint64(total_runs)
    rc = lib.lnsfaid_line_markov_host(C.byref(code), line.ctypes.data, n_codewords, key, first_codeword, t.ctypes.data, out.ctypes.data,
                                      flips.ctypes.data, runs.ctypes.data, C.byref(tf), C.byref(tr))
    if rc != 0:
        raise ValueError("lnsfaid_line_markov_host failed: %d" % rc)
    return out, flips, runs, tf.value, tr.value


def line_count_errors_host(code, payload, sent, stats, n_codewords, errors=True, fec=None, vs_sent=None, lib=None):
    """lnsfaid_line_count_errors_host: payload / sent uint32 payload streams (sent None: all-zero), stats a line_stats_dtype() array or
    None.  errors / fec / vs_sent: True, four numbers the call adds to, or None / False for a NULL pointer.  Returns the three as
    lists or None"""
    import numpy as np
    lib = lib or load()
    kw = (code.n_var - code.n_check) // 32
    payload = np.ascontiguousarray(payload, dtype=np.uint32)
    sent = None if sent is None else np.ascontiguousarray(sent, dtype=np.uint32)
    stats = None if stats is None else np.ascontiguousarray(stats, dtype=line_stats_dtype())
    if payload.size != n_codewords * kw or (sent is not None and sent.size != payload.size) or (stats is not None and stats.size != n_codewords):
        raise ValueError("lnsfaid_line_count_errors_host: buffer sizes do not fit %d codewords" % n_codewords)
    e, f, v = _fec_counters(errors), _fec_counters(fec), _fec_counters(vs_sent)
    rc = lib.lnsfaid_line_count_errors_host(C.byref(code), payload.ctypes.data, None if sent is None else sent.ctypes.data,
                                            None if stats is None else stats.ctypes.data, n_codewords, e, f, v)
    if rc != 0:
        raise ValueError("lnsfaid_line_count_errors_host failed: %d" % rc)
    return tuple(list(x) if x is not None else None for x in (e, f, v))


def _sptr(shortened):
    return None if shortened is None else shortened.ctypes.data


def burst_payload_random_host(code, key, first_codeword, shortened, where, n_codewords, lib=None):
    """lnsfaid_burst_payload_random_host: the burst payload (flat uint32, (K - S_c) / 32 words per codeword) of codewords
    first_codeword .. of stream `key`: the line payload of each codeword with the known words dropped"""
    import numpy as np
    lib = lib or load()
    shortened = _shortened(shortened, n_codewords)
    _, payload_bits = burst_words(code, shortened, n_codewords, lib)
    out = np.empty(payload_bits // 32, dtype=np.uint32)
    rc = lib.lnsfaid_burst_payload_random_host(C.byref(code), key, first_codeword, _sptr(shortened), where, n_codewords, out.ctypes.data)
    if rc != 0:
        raise ValueError("lnsfaid_burst_payload_random_host failed: %d" % rc)
    return out


def burst_bsc_host(code, line, shortened, where, n_codewords, key, first_codeword, threshold, in_place=False, total=0, lib=None):
    """lnsfaid_burst_bsc_host: burst line (flat uint32, LINE_HARD) through the binary symmetric channel of stream `key`, the draws
    indexed by mother position.  Returns (line out, flips uint32 [n_codewords], total + the positions inverted); in_place writes into
    `line` itself"""
    import numpy as np
    lib = lib or load()
    shortened = _shortened(shortened, n_codewords)
    line_bits, _ = burst_words(code, shortened, n_codewords, lib)
    if not in_place:
        line = np.ascontiguousarray(line, dtype=np.uint32)
    if line.dtype != np.uint32 or not line.flags.c_contiguous or line.size != line_bits // 32:
        raise ValueError("lnsfaid_burst_bsc_host: line must be contiguous uint32 with %d words" % (line_bits // 32))
    out = line if in_place else np.empty_like(line)
    flips = np.zeros(n_codewords, dtype=np.uint32)
    t = C.c_uint64(total)
    rc = lib.lnsfaid_burst_bsc_host(C.byref(code), line.ctypes.data, _sptr(shortened), where, n_codewords, key, first_codeword, threshold,
                                    out.ctypes.data, flips.ctypes.data, C.byref(t))
    if rc != 0:
        raise ValueError("lnsfaid_burst_bsc_host failed: %d" % rc)
    return out, flips, t.value


def burst_soft_host(code, line, shortened, where, n_codewords, key, first_codeword, table, total=0, lib=None):
    """lnsfaid_burst_soft_host: burst line (flat uint32, LINE_HARD) through the soft channel of stream `key` and `table`.  Returns
    (llr4 burst line, flat uint8 (LINE_LLR4), flips uint32 [n_codewords], total + the flips of the call)"""
    import numpy as np
    lib = lib or load()
    shortened = _shortened(shortened, n_codewords)
    line_bits, _ = burst_words(code, shortened, n_codewords, lib)
    line = np.ascontiguousarray(line, dtype=np.uint32)
    if line.size != line_bits // 32:
        raise ValueError("lnsfaid_burst_soft_host: line has %d words, not %d" % (line.size, line_bits // 32))
    table = _soft_table(table)
    out = np.empty(line_bits // 2, dtype=np.uint8)
    flips = np.zeros(n_codewords, dtype=np.uint32)
    t = C.c_uint64(total)
    rc = lib.lnsfaid_burst_soft_host(C.byref(code), line.ctypes.data, _sptr(shortened), where, n_codewords, key, first_codeword,
                                     table.ctypes.data, out.ctypes.data, flips.ctypes.data, C.byref(t))
    if rc != 0:
        raise ValueError("lnsfaid_burst_soft_host failed: %d" % rc)
    return out, flips, t.value


def burst_count_errors_host(code, payload, sent, stats, short_ones, shortened, n_codewords, errors=True, fec=None, vs_sent=None, lib=None):
    """lnsfaid_burst_count_errors_host: payload / sent burst payloads (flat uint32; sent None: all-zero), stats a line_stats_dtype()
    array or None, short_ones uint32 [n_codewords] or None (zeros).  errors / fec / vs_sent and the result as line_count_errors_host;
    a codeword with short_ones > 0 counts as failed"""
    import numpy as np
    lib = lib or load()
    shortened = _shortened(shortened, n_codewords)
    _, payload_bits = burst_words(code, shortened, n_codewords, lib)
    payload = np.ascontiguousarray(payload, dtype=np.uint32)
    sent = None if sent is None else np.ascontiguousarray(sent, dtype=np.uint32)
    stats = None if stats is None else np.ascontiguousarray(stats, dtype=line_stats_dtype())
    short_ones = None if short_ones is None else np.ascontiguousarray(short_ones, dtype=np.uint32)
    if (payload.size != payload_bits // 32 or (sent is not None and sent.size != payload.size)
            or (stats is not None and stats.size != n_codewords) or (short_ones is not None and short_ones.size != n_codewords)):
        raise ValueError("lnsfaid_burst_count_errors_host: buffer sizes do not fit %d codewords" % n_codewords)
    e, f, v = _fec_counters(errors), _fec_counters(fec), _fec_counters(vs_sent)
    rc = lib.lnsfaid_burst_count_errors_host(C.byref(code), payload.ctypes.data, None if sent is None else sent.ctypes.data,
                                             None if stats is None else stats.ctypes.data,
                                             None if short_ones is None else short_ones.ctypes.data, _sptr(shortened), n_codewords, e, f, v)
    if rc != 0:
        raise ValueError("lnsfaid_burst_count_errors_host failed: %d" % rc)
    return tuple(list(x) if x is not None else None for x in (e, f, v))


def line_failure_dtype():
    """numpy view of lnsfaid_line_failure"""
    import numpy as np
    return np.dtype([("codeword", np.uint64), ("index", np.uint32), ("flags", np.uint32), ("unsatisfied", np.uint32),
                     ("wrong_payload", np.uint32), ("wrong_parity", np.uint32), ("channel_errors", np.uint32)])


def line_capture_words(code, fmt, lib=None):
    """lnsfaid_line_capture_words: 32-bit words of one record's payload for a Code struct and a line format"""
    lib = lib or load()
    w = C.c_uint32()
    rc = lib.lnsfaid_line_capture_words(C.byref(code), fmt, C.byref(w))
    if rc != 0:
        raise ValueError("lnsfaid_line_capture_words failed: %d" % rc)
    return w.value


def line_capture_split(code, fmt, payload):
    """payload uint32 [stored, W] -> its four sections {"line", "bits", "error", "syndrome"}, each uint32 [stored, words]"""
    L, N, M = code.n_var - code.puncture_tail, code.n_var, code.n_check
    lw = L // 8 if fmt == LINE_LLR4 else L // 32
    cuts = [0, lw, lw + N // 32, lw + 2 * (N // 32), lw + 2 * (N // 32) + M // 32]
    return {name: payload[:, cuts[i]:cuts[i + 1]] for i, name in enumerate(("line", "bits", "error", "syndrome"))}


def line_capture_positions(words):
    """one record's `error` or `syndrome` section (uint32 words) -> the ascending list of its set bits: wrong positions / unsatisfied
    rows of pos_vn"""
    import numpy as np
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return np.flatnonzero(bits).tolist()


def _line_capture(fn, what, code, fmt, n_codewords, capacity, lib):
    """runs fn(records pointer, payload pointer, found, stored) on buffers of min(capacity, n_codewords) slots"""
    import numpy as np
    W = line_capture_words(code, fmt, lib)
    slots = min(capacity, n_codewords)
    records = np.zeros(slots, dtype=line_failure_dtype())
    payload = np.zeros((slots, W), dtype=np.uint32)
    found, stored = C.c_uint64(), C.c_uint64()
    rc = fn(records.ctypes.data if slots else None, payload.ctypes.data if slots else None, C.byref(found), C.byref(stored))
    if rc != 0:
        raise ValueError("%s failed: %d" % (what, rc))
    return found.value, records[:stored.value], line_capture_split(code, fmt, payload[:stored.value])


def line_capture_host(code, line, fmt, bits, sent, n_codewords, first_codeword=0, select=1, skip=0, capacity=256, lib=None):
    """lnsfaid_line_capture_host: line as decode_line takes it or None, bits / sent uint32 [n_codewords, N / 32] (sent None: no sent word
    is known).  Returns (found, records as a structured numpy array, {"line", "bits", "error", "syndrome"} uint32 [stored, words])"""
    import numpy as np
    lib = lib or load()
    per, dtype, _ = line_sizes(code, fmt)
    arrs = []
    for name, a, dt, size in (("line", line, dtype, n_codewords * per), ("bits", bits, np.uint32, n_codewords * (code.n_var // 32)),
                              ("sent", sent, np.uint32, n_codewords * (code.n_var // 32))):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != size:
                raise ValueError("lnsfaid_line_capture_host: %s has %d elements, not %d" % (name, a.size, size))
        arrs.append(a)
    ptr = [a.ctypes.data if a is not None else None for a in arrs]
    return _line_capture(lambda r, p, f, s: lib.lnsfaid_line_capture_host(C.byref(code), ptr[0], fmt, ptr[1], ptr[2], n_codewords, first_codeword,
                                                                          select, skip, capacity, r, p, f, s),
                         "lnsfaid_line_capture_host", code, fmt, n_codewords, capacity, lib)


def _demap_host(fn_name, packed, n_var, n_check, interleave, rx, n_groups, mod_type, scale, lib):
    import numpy as np
    lib = lib or load()
    rx = np.ascontiguousarray(rx, dtype=np.float32)
    floats = n_groups * GROUP * n_var * (1 if mod_type == 1 else 2) // max(mod_type, 1)
    if rx.size != floats:
        raise ValueError("%s: rx has %d floats, %d groups of mod_type %d take %d" % (fn_name, rx.size, n_groups, mod_type, floats))
    out = np.empty(n_groups * GROUP * n_var // (2 if packed else 1), dtype=np.uint8 if packed else np.int8)
    rc = getattr(lib, fn_name)(n_var, n_check, interleave, rx.ctypes.data, n_groups, mod_type, scale, out.ctypes.data)
    if rc != 0:
        raise ValueError("%s failed: %d" % (fn_name, rc))
    return out


def demap_host(n_var, n_check, interleave, rx, n_groups, mod_type, scale, lib=None):
    """lnsfaid_demap_host: received symbols (float32, the rx format of include/lnsfaid.h) -> int8 fixInput"""
    return _demap_host("lnsfaid_demap_host", False, n_var, n_check, interleave, rx, n_groups, mod_type, scale, lib)


def demap_packed_host(n_var, n_check, interleave, rx, n_groups, mod_type, scale, lib=None):
    """lnsfaid_demap_packed_host: received symbols -> uint8 llr4, two elements per byte"""
    return _demap_host("lnsfaid_demap_packed_host", True, n_var, n_check, interleave, rx, n_groups, mod_type, scale, lib)


PREFEC_INFO, PREFEC_CODEWORD = 1, 2


def prefec_errors_host(n_var, n_check, interleave, rx, n_groups, mod_type, sent, scope, lib=None, out=None):
    """lnsfaid_prefec_errors_host: received symbols (float32, the rx format of include/lnsfaid.h) against the sent bits (int8, the
    encoder's output layout, or None for the all-zero codeword) -> [TestFrame, ModErrorFrame, ModErrorBits, ModErrorSymbol], added
    to `out` (four numbers) when it is given"""
    import numpy as np
    lib = lib or load()
    rx = np.ascontiguousarray(rx, dtype=np.float32)
    floats = n_groups * GROUP * n_var * (1 if mod_type == 1 else 2) // max(mod_type, 1)
    if rx.size != floats:
        raise ValueError("lnsfaid_prefec_errors_host: rx has %d floats, %d groups of mod_type %d take %d" % (rx.size, n_groups, mod_type, floats))
    if sent is not None:
        sent = np.ascontiguousarray(sent, dtype=np.int8)
        if sent.size != n_groups * GROUP * n_var:
            raise ValueError("lnsfaid_prefec_errors_host: sent has %d bytes, not %d" % (sent.size, n_groups * GROUP * n_var))
    counters = (C.c_uint64 * 4)(*([0, 0, 0, 0] if out is None else [int(x) for x in out]))
    rc = lib.lnsfaid_prefec_errors_host(n_var, n_check, interleave, rx.ctypes.data, n_groups, mod_type,
                                        sent.ctypes.data if sent is not None else None, scope, counters)
    if rc != 0:
        raise ValueError("lnsfaid_prefec_errors_host failed: %d" % rc)
    return list(counters)


def error_record_dtype():
    """numpy view of lnsfaid_error_record"""
    import numpy as np
    return np.dtype([("codeword", np.uint32), ("info_errors", np.uint32), ("parity_errors", np.uint32), ("reserved", np.uint32)])


def _capture(fn, what, n_var, n_groups, capacity, counters):
    """runs fn(records pointer, payload pointer, found, stored, out) on buffers of min(capacity, 32 n_groups) slots"""
    import numpy as np
    slots = min(capacity, GROUP * n_groups)
    records = np.zeros(slots, dtype=error_record_dtype())
    payload = np.zeros((slots, 3, n_var), dtype=np.int8)
    found, stored = C.c_uint64(), C.c_uint64()
    out = None
    if counters is not False and counters is not None:
        out = (C.c_uint64 * 4)(*([0, 0, 0, 0] if counters is True else [int(x) for x in counters]))
    rc = fn(records.ctypes.data if slots else None, payload.ctypes.data if slots else None, C.byref(found), C.byref(stored), out)
    if rc != 0:
        raise ValueError("%s failed: %d" % (what, rc))
    res = (found.value, records[:stored.value], payload[:stored.value])
    return res + (list(out),) if out is not None else res


def capture_errors_host(n_var, n_check, fix_input, decoded, sent, n_groups, skip=0, capacity=256, counters=False, lib=None):
    """lnsfaid_capture_errors_host: fix_input / sent int8 in the encoder's output layout or None, decoded int8 [n_groups * 32][n_var].
    Returns (found, records as a structured numpy array, payload int8 [stored, 3, n_var][, counters]); counters: True, or four
    numbers the call adds to"""
    import numpy as np
    lib = lib or load()
    size = n_groups * GROUP * n_var
    arrs = []
    for name, a in (("fix_input", fix_input), ("decoded", decoded), ("sent", sent)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.int8)
            if a.size != size:
                raise ValueError("lnsfaid_capture_errors_host: %s has %d bytes, not %d" % (name, a.size, size))
        arrs.append(a)
    ptr = [a.ctypes.data if a is not None else None for a in arrs]
    return _capture(lambda r, p, f, s, o: lib.lnsfaid_capture_errors_host(n_var, n_check, ptr[0], ptr[1], ptr[2], n_groups, skip, capacity,
                                                                          r, p, f, s, o),
                    "lnsfaid_capture_errors_host", n_var, n_groups, capacity, counters)


def fec_record_dtype():
    """numpy view of lnsfaid_fec_record"""
    import numpy as np
    return np.dtype([("unsatisfied", np.uint32), ("corrected", np.uint32)])


def _fec_counters(v):
    """None / False: not asked for; True: start from zero; four numbers: the call adds to them"""
    if v is None or v is False:
        return None
    return (C.c_uint64 * 4)(*([0, 0, 0, 0] if v is True else [int(x) for x in v]))


def _fec_status_host(fn_name, packed, code, fix, decided, sent, n_groups, records, out, vs_sent, lib):
    import numpy as np
    lib = lib or load()
    n_var = code.n_var
    sizes = (n_groups * GROUP * n_var // (2 if packed else 1), n_groups * GROUP * n_var // (32 if packed else 1), n_groups * GROUP * n_var)
    types = (np.uint8, np.uint32, np.int8) if packed else (np.int8, np.int8, np.int8)
    arrs = []
    for name, a, size, t in zip(("fix_input", "decisions", "sent"), (fix, decided, sent), sizes, types):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=t)
            if a.size != size:
                raise ValueError("%s: %s has %d elements, not %d" % (fn_name, name, a.size, size))
        arrs.append(a)
    ptr = [a.ctypes.data if a is not None else None for a in arrs]
    rec = np.zeros(n_groups * GROUP, dtype=fec_record_dtype()) if records else None
    o, v = _fec_counters(out), _fec_counters(vs_sent)
    rc = getattr(lib, fn_name)(C.byref(code), ptr[0], ptr[1], ptr[2], n_groups, rec.ctypes.data if records else None, o, v)
    if rc != 0:
        raise ValueError("%s failed: %d" % (fn_name, rc))
    return rec, (list(o) if o is not None else None), (list(v) if v is not None else None)


def fec_status_host(code, fix_input, decoded, sent, n_groups, records=True, out=True, vs_sent=None, lib=None):
    """lnsfaid_fec_status_host: code a Code struct (Code50GPON().code); fix_input / sent int8 in the encoder's output layout or None,
    decoded int8 [n_groups * 32][n_var].  Returns (records as a structured numpy array or None, out or None, vs_sent or None); out /
    vs_sent: True, four numbers the call adds to, or None / False for a NULL pointer"""
    return _fec_status_host("lnsfaid_fec_status_host", False, code, fix_input, decoded, sent, n_groups, records, out, vs_sent, lib)


def fec_status_packed_host(code, llr4, bits, sent, n_groups, records=True, out=True, vs_sent=None, lib=None):
    """lnsfaid_fec_status_packed_host: llr4 uint8 (pack_llr4) or None, bits uint32 (the packed decisions), sent int8 or None"""
    return _fec_status_host("lnsfaid_fec_status_packed_host", True, code, llr4, bits, sent, n_groups, records, out, vs_sent, lib)


class Decoder:
    """Thin RAII wrapper over lnsfaid_create / lnsfaid_decode* / lnsfaid_destroy."""

    def __init__(self, code50, cfg, device=0, max_groups=64, lib=None):
        self.lib = lib or load()
        self.code50 = code50
        self.device = device
        self.ctx = C.c_void_p()
        rc = self.lib.lnsfaid_create(C.byref(self.ctx), C.byref(code50.code), C.byref(cfg), device, max_groups)
        if rc != 0:
            raise RuntimeError("lnsfaid_create failed: %d (%s; hip: %s)" % (
                rc, self.lib.lnsfaid_strerror(rc).decode(), self.lib.lnsfaid_last_hip_error().decode()))

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d (%s; hip: %s)" % (
                what, rc, self.lib.lnsfaid_strerror(rc).decode(), self.lib.lnsfaid_last_hip_error().decode()))

    def set_cfg(self, cfg):
        self._check(self.lib.lnsfaid_set_cfg(self.ctx, C.byref(cfg)), "lnsfaid_set_cfg")

    def decode(self, fix_input, n_groups):
        """fix_input: numpy int8 array, reference layout. Returns (decodedBits int8 array, stats array)."""
        import numpy as np
        N = self.code50.N
        assert fix_input.dtype == np.int8 and fix_input.size == n_groups * GROUP * N and fix_input.flags.c_contiguous
        out = np.empty(n_groups * GROUP * N, dtype=np.int8)
        stats = np.zeros((n_groups, 2), dtype=np.int32)
        self._check(self.lib.lnsfaid_decode(self.ctx, fix_input.ctypes.data, n_groups, out.ctypes.data,
                                            stats.ctypes.data), "lnsfaid_decode")
        return out, stats

    def set_early_stop(self, rule):
        """STOP_GROUP (default) or STOP_CODEWORD (lnsfaid_set_early_stop)"""
        self._check(self.lib.lnsfaid_set_early_stop(self.ctx, rule), "lnsfaid_set_early_stop")

    def early_stop(self):
        return self.lib.lnsfaid_early_stop(self.ctx)

    def decode_codewords(self, fix_input, n_groups, with_stats=True):
        """lnsfaid_decode_codewords: (decodedBits int8 array, [n_groups * 32, 3] int32 array of iterations / bf_iterations /
        unsatisfied, or None)"""
        import numpy as np
        N = self.code50.N
        assert fix_input.dtype == np.int8 and fix_input.size == n_groups * GROUP * N and fix_input.flags.c_contiguous
        out = np.empty(n_groups * GROUP * N, dtype=np.int8)
        cw = np.zeros((n_groups * GROUP, 3), dtype=np.int32) if with_stats else None
        self._check(self.lib.lnsfaid_decode_codewords(self.ctx, fix_input.ctypes.data, n_groups, out.ctypes.data,
                                                      cw.ctypes.data if with_stats else None), "lnsfaid_decode_codewords")
        return out, cw

    def decode_codewords_device(self, d_fix_ptr, n_groups, d_out_ptr, d_cw_stats_ptr=None):
        self._check(self.lib.lnsfaid_decode_codewords_device(self.ctx, d_fix_ptr, n_groups, d_out_ptr, d_cw_stats_ptr),
                    "lnsfaid_decode_codewords_device")

    def decode_device(self, d_fix_ptr, n_groups, d_out_ptr, d_stats_ptr=None):
        self._check(self.lib.lnsfaid_decode_device(self.ctx, d_fix_ptr, n_groups, d_out_ptr, d_stats_ptr),
                    "lnsfaid_decode_device")

    def count_errors(self, decoded, input_bits, n_groups):
        out = (C.c_uint64 * 4)()
        ip = input_bits.ctypes.data if input_bits is not None else None
        self._check(self.lib.lnsfaid_count_errors(self.ctx, decoded.ctypes.data, ip, n_groups, out), "lnsfaid_count_errors")
        return list(out)

    def count_errors_device(self, d_decoded_ptr, d_input_ptr, n_groups):
        out = (C.c_uint64 * 4)()
        self._check(self.lib.lnsfaid_count_errors_device(self.ctx, d_decoded_ptr, d_input_ptr, n_groups, out),
                    "lnsfaid_count_errors_device")
        return list(out)

    def decode_packed(self, llr4, n_groups):
        """lnsfaid_decode_packed: llr4 uint8 array (pack_llr4).  Returns (packed decisions uint32 array, stats array)."""
        import numpy as np
        N = self.code50.N
        assert llr4.dtype == np.uint8 and llr4.size == n_groups * GROUP * N // 2 and llr4.flags.c_contiguous
        out = np.empty(n_groups * GROUP * N // 32, dtype=np.uint32)
        stats = np.zeros((n_groups, 2), dtype=np.int32)
        self._check(self.lib.lnsfaid_decode_packed(self.ctx, llr4.ctypes.data, n_groups, out.ctypes.data, stats.ctypes.data),
                    "lnsfaid_decode_packed")
        return out, stats

    def decode_codewords_packed(self, llr4, n_groups, with_stats=True):
        """lnsfaid_decode_codewords_packed: (packed decisions uint32 array, [n_groups * 32, 3] int32 array or None)"""
        import numpy as np
        N = self.code50.N
        assert llr4.dtype == np.uint8 and llr4.size == n_groups * GROUP * N // 2 and llr4.flags.c_contiguous
        out = np.empty(n_groups * GROUP * N // 32, dtype=np.uint32)
        cw = np.zeros((n_groups * GROUP, 3), dtype=np.int32) if with_stats else None
        self._check(self.lib.lnsfaid_decode_codewords_packed(self.ctx, llr4.ctypes.data, n_groups, out.ctypes.data,
                                                             cw.ctypes.data if with_stats else None), "lnsfaid_decode_codewords_packed")
        return out, cw

    def decode_packed_device(self, d_llr4_ptr, n_groups, d_bits_ptr, d_stats_ptr=None):
        self._check(self.lib.lnsfaid_decode_packed_device(self.ctx, d_llr4_ptr, n_groups, d_bits_ptr, d_stats_ptr),
                    "lnsfaid_decode_packed_device")

    def decode_codewords_packed_device(self, d_llr4_ptr, n_groups, d_bits_ptr, d_cw_stats_ptr=None):
        self._check(self.lib.lnsfaid_decode_codewords_packed_device(self.ctx, d_llr4_ptr, n_groups, d_bits_ptr, d_cw_stats_ptr),
                    "lnsfaid_decode_codewords_packed_device")

    def decode_line(self, line, fmt, n_codewords, magnitude=4, with_bits=False, with_stats=True):
        """lnsfaid_decode_line: line uint32 words (LINE_HARD) or uint8 (LINE_LLR4), any number of codewords.  Returns (payload
        uint32 [n_codewords, K / 32], packed decisions uint32 [n_codewords, n_var / 32] or None, lnsfaid_line_stats array or None)"""
        import numpy as np
        code = self.code50.code
        per, dtype, k_words = line_sizes(code, fmt)
        assert line.dtype == dtype and line.size == n_codewords * per and line.flags.c_contiguous
        payload = np.empty((n_codewords, k_words), dtype=np.uint32)
        bits = np.empty((n_codewords, code.n_var // 32), dtype=np.uint32) if with_bits else None
        stats = np.zeros(n_codewords, dtype=line_stats_dtype()) if with_stats else None
        self._check(self.lib.lnsfaid_decode_line(self.ctx, line.ctypes.data, fmt, magnitude, n_codewords, payload.ctypes.data,
                                                 bits.ctypes.data if with_bits else None, stats.ctypes.data if with_stats else None),
                    "lnsfaid_decode_line")
        return payload, bits, stats

    def decode_line_device(self, d_line_ptr, fmt, n_codewords, d_payload_ptr, d_bits_ptr=None, d_stats_ptr=None, magnitude=4):
        self._check(self.lib.lnsfaid_decode_line_device(self.ctx, d_line_ptr, fmt, magnitude, n_codewords, d_payload_ptr, d_bits_ptr,
                                                        d_stats_ptr), "lnsfaid_decode_line_device")

    def encode_line(self, payload, n_codewords, with_bits=False):
        """lnsfaid_encode_line: payload uint32 [n_codewords, K / 32] (the payload of decode_line).  Returns (line uint32
        [n_codewords, L / 32] in the LINE_HARD format, the whole codewords uint32 [n_codewords, n_var / 32] or None)"""
        import numpy as np
        code = self.code50.code
        L, K = code.n_var - code.puncture_tail, code.n_var - code.n_check
        assert payload.dtype == np.uint32 and payload.size == n_codewords * (K // 32) and payload.flags.c_contiguous
        line = np.empty((n_codewords, L // 32), dtype=np.uint32)
        bits = np.empty((n_codewords, code.n_var // 32), dtype=np.uint32) if with_bits else None
        self._check(self.lib.lnsfaid_encode_line(self.ctx, payload.ctypes.data, n_codewords, line.ctypes.data,
                                                 bits.ctypes.data if with_bits else None), "lnsfaid_encode_line")
        return line, bits

    def encode_line_device(self, d_payload_ptr, n_codewords, d_line_ptr, d_bits_ptr=None):
        self._check(self.lib.lnsfaid_encode_line_device(self.ctx, d_payload_ptr, n_codewords, d_line_ptr, d_bits_ptr),
                    "lnsfaid_encode_line_device")

    def decode_burst(self, line, fmt, shortened, where, n_codewords, magnitude=4, with_bits=False, with_stats=True, with_ones=True):
        """lnsfaid_decode_burst: burst line, flat uint32 words (LINE_HARD) or uint8 (LINE_LLR4); shortened uint32 [n_codewords] in
        bits or None.  Returns (burst payload, flat uint32; packed decisions uint32 [n_codewords, n_var / 32] or None;
        lnsfaid_line_stats array or None; short_ones uint32 [n_codewords] or None)"""
        import numpy as np
        code = self.code50.code
        shortened = _shortened(shortened, n_codewords)
        line_bits, payload_bits = burst_words(code, shortened, n_codewords, self.lib)
        assert line.dtype == (np.uint32 if fmt == LINE_HARD else np.uint8) and line.flags.c_contiguous
        assert line.size == (line_bits // 32 if fmt == LINE_HARD else line_bits // 2)
        payload = np.empty(payload_bits // 32, dtype=np.uint32)
        bits = np.empty((n_codewords, code.n_var // 32), dtype=np.uint32) if with_bits else None
        stats = np.zeros(n_codewords, dtype=line_stats_dtype()) if with_stats else None
        ones = np.zeros(n_codewords, dtype=np.uint32) if with_ones else None
        self._check(self.lib.lnsfaid_decode_burst(self.ctx, line.ctypes.data, fmt, magnitude,
                                                  None if shortened is None else shortened.ctypes.data, where, n_codewords,
                                                  payload.ctypes.data, bits.ctypes.data if with_bits else None,
                                                  stats.ctypes.data if with_stats else None, ones.ctypes.data if with_ones else None),
                    "lnsfaid_decode_burst")
        return payload, bits, stats, ones

    def decode_burst_device(self, d_line_ptr, fmt, shortened, where, n_codewords, d_payload_ptr, d_bits_ptr=None, d_stats_ptr=None,
                            d_short_ones_ptr=None, magnitude=4):
        """lnsfaid_decode_burst_device: device pointers, but `shortened` is a host array (uint32 [n_codewords], bits) or None"""
        shortened = _shortened(shortened, n_codewords)
        self._check(self.lib.lnsfaid_decode_burst_device(self.ctx, d_line_ptr, fmt, magnitude,
                                                         None if shortened is None else shortened.ctypes.data, where, n_codewords,
                                                         d_payload_ptr, d_bits_ptr, d_stats_ptr, d_short_ones_ptr),
                    "lnsfaid_decode_burst_device")

    def encode_burst(self, payload, shortened, where, n_codewords, with_bits=False):
        """lnsfaid_encode_burst: burst payload (flat uint32, the payload of decode_burst).  Returns (burst line, flat uint32 in the
        LINE_HARD format, the whole mother codewords uint32 [n_codewords, n_var / 32] or None)"""
        import numpy as np
        code = self.code50.code
        shortened = _shortened(shortened, n_codewords)
        line_bits, payload_bits = burst_words(code, shortened, n_codewords, self.lib)
        assert payload.dtype == np.uint32 and payload.size == payload_bits // 32 and payload.flags.c_contiguous
        line = np.empty(line_bits // 32, dtype=np.uint32)
        bits = np.empty((n_codewords, code.n_var // 32), dtype=np.uint32) if with_bits else None
        self._check(self.lib.lnsfaid_encode_burst(self.ctx, payload.ctypes.data, None if shortened is None else shortened.ctypes.data,
                                                  where, n_codewords, line.ctypes.data, bits.ctypes.data if with_bits else None),
                    "lnsfaid_encode_burst")
        return line, bits

    def encode_burst_device(self, d_payload_ptr, shortened, where, n_codewords, d_line_ptr, d_bits_ptr=None):
        """lnsfaid_encode_burst_device: device pointers, `shortened` a host array or None"""
        shortened = _shortened(shortened, n_codewords)
        self._check(self.lib.lnsfaid_encode_burst_device(self.ctx, d_payload_ptr, None if shortened is None else shortened.ctypes.data,
                                                         where, n_codewords, d_line_ptr, d_bits_ptr), "lnsfaid_encode_burst_device")

    def line_payload_random_device(self, key, first_codeword, n_codewords, d_payload_ptr):
        """lnsfaid_line_payload_random_device: the payload of codewords first_codeword .. of stream `key` into a device buffer"""
        self._check(self.lib.lnsfaid_line_payload_random_device(self.ctx, key, first_codeword, n_codewords, d_payload_ptr),
                    "lnsfaid_line_payload_random_device")

    def line_bsc_device(self, d_line_in_ptr, n_codewords, key, first_codeword, threshold, d_line_out_ptr, d_flips_ptr=None, total=0):
        """lnsfaid_line_bsc_device: LINE_HARD words through the binary symmetric channel of stream `key` (d_line_out_ptr may equal
        d_line_in_ptr).  Returns total + the positions inverted"""
        t = C.c_uint64(total)
        self._check(self.lib.lnsfaid_line_bsc_device(self.ctx, d_line_in_ptr, n_codewords, key, first_codeword, threshold, d_line_out_ptr,
                                                     d_flips_ptr, C.byref(t)), "lnsfaid_line_bsc_device")
        return t.value

    def line_soft_device(self, d_line_in_ptr, n_codewords, key, first_codeword, table, d_llr4_out_ptr, d_flips_ptr=None, total=0):
        """lnsfaid_line_soft_device: LINE_HARD words through the soft channel of stream `key` and `table` (14 thresholds, host side)
        into LINE_LLR4 bytes.  Returns total + the flips of the call"""
        table = _soft_table(table)
        t = C.c_uint64(total)
        self._check(self.lib.lnsfaid_line_soft_device(self.ctx, d_line_in_ptr, n_codewords, key, first_codeword, table.ctypes.data,
                                                      d_llr4_out_ptr, d_flips_ptr, C.byref(t)), "lnsfaid_line_soft_device")
        return t.value

    def line_markov_device(self, d_line_in_ptr, n_codewords, key, first_codeword, t, d_line_out_ptr, d_flips_ptr=None, d_runs_ptr=None,
                           total=0, total_runs=0):
        """lnsfaid_line_markov_device: LINE_HARD words through the error-propagation channel of stream `key` and thresholds `t`
        ({ t_idle, t_after, t_start }, host side; d_line_out_ptr may equal d_line_in_ptr).  Returns (total + the positions inverted,
        total_runs + the runs of the call)"""
        t = _markov_t(t)
        tf, tr = C.c_uint64(total), C.c_uint64(total_runs)
        self._check(self.lib.lnsfaid_line_markov_device(self.ctx, d_line_in_ptr, n_codewords, key, first_codeword, t.ctypes.data,
                                                        d_line_out_ptr, d_flips_ptr, d_runs_ptr, C.byref(tf), C.byref(tr)),
                    "lnsfaid_line_markov_device")
        return tf.value, tr.value

    def line_count_errors_device(self, d_payload_ptr, d_sent_ptr, d_stats_ptr, n_codewords, errors=True, fec=None, vs_sent=None):
        """lnsfaid_line_count_errors_device: device pointers (d_sent_ptr None: all-zero payload; d_stats_ptr the lnsfaid_line_stats of
        decode_line_device, or None).  errors / fec / vs_sent and the result as line_count_errors_host"""
        e, f, v = _fec_counters(errors), _fec_counters(fec), _fec_counters(vs_sent)
        self._check(self.lib.lnsfaid_line_count_errors_device(self.ctx, d_payload_ptr, d_sent_ptr, d_stats_ptr, n_codewords, e, f, v),
                    "lnsfaid_line_count_errors_device")
        return tuple(list(x) if x is not None else None for x in (e, f, v))

    def burst_payload_random_device(self, key, first_codeword, shortened, where, n_codewords, d_payload_ptr):
        """lnsfaid_burst_payload_random_device: the burst payload of codewords first_codeword .. of stream `key` into a device buffer;
        `shortened` a host array (uint32 [n_codewords], bits) or None"""
        shortened = _shortened(shortened, n_codewords)
        self._check(self.lib.lnsfaid_burst_payload_random_device(self.ctx, key, first_codeword, _sptr(shortened), where, n_codewords,
                                                                 d_payload_ptr), "lnsfaid_burst_payload_random_device")

    def burst_bsc_device(self, d_line_in_ptr, shortened, where, n_codewords, key, first_codeword, threshold, d_line_out_ptr,
                         d_flips_ptr=None, total=0):
        """lnsfaid_burst_bsc_device: a LINE_HARD burst line through the binary symmetric channel of stream `key` (d_line_out_ptr may
        equal d_line_in_ptr).  Returns total + the positions inverted"""
        shortened = _shortened(shortened, n_codewords)
        t = C.c_uint64(total)
        self._check(self.lib.lnsfaid_burst_bsc_device(self.ctx, d_line_in_ptr, _sptr(shortened), where, n_codewords, key, first_codeword,
                                                      threshold, d_line_out_ptr, d_flips_ptr, C.byref(t)), "lnsfaid_burst_bsc_device")
        return t.value

    def burst_soft_device(self, d_line_in_ptr, shortened, where, n_codewords, key, first_codeword, table, d_llr4_out_ptr,
                          d_flips_ptr=None, total=0):
        """lnsfaid_burst_soft_device: a LINE_HARD burst line through the soft channel of stream `key` and `table` (14 thresholds, host
        side) into a LINE_LLR4 burst line.  Returns total + the flips of the call"""
        shortened = _shortened(shortened, n_codewords)
        table = _soft_table(table)
        t = C.c_uint64(total)
        self._check(self.lib.lnsfaid_burst_soft_device(self.ctx, d_line_in_ptr, _sptr(shortened), where, n_codewords, key, first_codeword,
                                                       table.ctypes.data, d_llr4_out_ptr, d_flips_ptr, C.byref(t)),
                    "lnsfaid_burst_soft_device")
        return t.value

    def burst_count_errors_device(self, d_payload_ptr, d_sent_ptr, d_stats_ptr, d_short_ones_ptr, shortened, n_codewords, errors=True,
                                  fec=None, vs_sent=None):
        """lnsfaid_burst_count_errors_device: device pointers to burst payloads (d_sent_ptr None: all-zero), to the lnsfaid_line_stats
        and the short_ones of decode_burst_device (either None); `shortened` a host array or None.  errors / fec / vs_sent and the
        result as line_count_errors_host"""
        shortened = _shortened(shortened, n_codewords)
        e, f, v = _fec_counters(errors), _fec_counters(fec), _fec_counters(vs_sent)
        self._check(self.lib.lnsfaid_burst_count_errors_device(self.ctx, d_payload_ptr, d_sent_ptr, d_stats_ptr, d_short_ones_ptr,
                                                               _sptr(shortened), n_codewords, e, f, v),
                    "lnsfaid_burst_count_errors_device")
        return tuple(list(x) if x is not None else None for x in (e, f, v))

    def count_errors_packed(self, bits, msg, n_groups):
        """lnsfaid_count_errors_packed: bits uint32 (decode_packed), msg uint8 (pack_bits) or None for the all-zero codeword"""
        out = (C.c_uint64 * 4)()
        mp = msg.ctypes.data if msg is not None else None
        self._check(self.lib.lnsfaid_count_errors_packed(self.ctx, bits.ctypes.data, mp, n_groups, out), "lnsfaid_count_errors_packed")
        return list(out)

    def count_errors_packed_device(self, d_bits_ptr, d_msg_ptr, n_groups):
        out = (C.c_uint64 * 4)()
        self._check(self.lib.lnsfaid_count_errors_packed_device(self.ctx, d_bits_ptr, d_msg_ptr, n_groups, out),
                    "lnsfaid_count_errors_packed_device")
        return list(out)

    def demap_device(self, d_rx_ptr, n_groups, mod_type, scale, d_fix_ptr):
        """lnsfaid_demap_device: received symbols on the device -> int8 fixInput (InterleaveModType: the context's)"""
        self._check(self.lib.lnsfaid_demap_device(self.ctx, d_rx_ptr, n_groups, mod_type, scale, d_fix_ptr), "lnsfaid_demap_device")

    def demap_packed_device(self, d_rx_ptr, n_groups, mod_type, scale, d_llr4_ptr):
        self._check(self.lib.lnsfaid_demap_packed_device(self.ctx, d_rx_ptr, n_groups, mod_type, scale, d_llr4_ptr),
                    "lnsfaid_demap_packed_device")

    def prefec_errors_device(self, d_rx_ptr, n_groups, mod_type, d_sent_ptr, scope, out=None):
        """lnsfaid_prefec_errors_device: symbols and sent bits on the device (d_sent_ptr None: the all-zero codeword) ->
        [TestFrame, ModErrorFrame, ModErrorBits, ModErrorSymbol], added to `out` when it is given"""
        counters = (C.c_uint64 * 4)(*([0, 0, 0, 0] if out is None else [int(x) for x in out]))
        self._check(self.lib.lnsfaid_prefec_errors_device(self.ctx, d_rx_ptr, n_groups, mod_type, d_sent_ptr, scope, counters),
                    "lnsfaid_prefec_errors_device")
        return list(counters)

    def frontend_set_prefec(self, scope):
        """lnsfaid_frontend_set_prefec: 0 = off, PREFEC_INFO / PREFEC_CODEWORD = count in every later front-end call"""
        self._check(self.lib.lnsfaid_frontend_set_prefec(self.ctx, scope), "lnsfaid_frontend_set_prefec")

    def frontend_prefec_counters(self, reset=False, out=None):
        """lnsfaid_frontend_prefec_counters: the accumulator of the fused counting, added to `out` when it is given"""
        counters = (C.c_uint64 * 4)(*([0, 0, 0, 0] if out is None else [int(x) for x in out]))
        self._check(self.lib.lnsfaid_frontend_prefec_counters(self.ctx, counters, 1 if reset else 0), "lnsfaid_frontend_prefec_counters")
        return list(counters)

    def capture_errors_device(self, d_fix_ptr, d_dec_ptr, d_sent_ptr, n_groups, skip=0, capacity=256, counters=False):
        """lnsfaid_capture_errors_device: device pointers (d_fix_ptr / d_sent_ptr may be None).  Returns (found, records as a
        structured numpy array, payload int8 [stored, 3, n_var][, counters]); counters: True, or four numbers the call adds to"""
        try:
            return _capture(lambda r, p, f, s, o: self.lib.lnsfaid_capture_errors_device(self.ctx, d_fix_ptr, d_dec_ptr, d_sent_ptr, n_groups,
                                                                                         skip, capacity, r, p, f, s, o),
                            "lnsfaid_capture_errors_device", self.code50.N, n_groups, capacity, counters)
        except ValueError as e:
            raise RuntimeError("%s (hip: %s)" % (e, self.lib.lnsfaid_last_hip_error().decode()))

    def line_capture_device(self, d_line_ptr, fmt, d_bits_ptr, d_sent_ptr, n_codewords, first_codeword=0, select=1, skip=0, capacity=256):
        """lnsfaid_line_capture_device: device pointers (d_line_ptr / d_sent_ptr may be None).  The result as line_capture_host"""
        try:
            return _line_capture(lambda r, p, f, s: self.lib.lnsfaid_line_capture_device(self.ctx, d_line_ptr, fmt, d_bits_ptr, d_sent_ptr,
                                                                                         n_codewords, first_codeword, select, skip, capacity,
                                                                                         r, p, f, s),
                                 "lnsfaid_line_capture_device", self.code50.code, fmt, n_codewords, capacity, self.lib)
        except ValueError as e:
            raise RuntimeError("%s (hip: %s)" % (e, self.lib.lnsfaid_last_hip_error().decode()))

    def _fec_status_device(self, fn_name, d_fix_ptr, d_dec_ptr, d_sent_ptr, n_groups, records, out, vs_sent, d_records_ptr):
        import numpy as np
        rec = None
        if records and d_records_ptr is None:
            import torch
            rec = torch.zeros(max(n_groups, 1) * GROUP * 2, dtype=torch.int32, device="cuda:%d" % self.device)
            torch.cuda.synchronize()  # the zero fill runs on torch's stream, the call on the context's
            d_records_ptr = rec.data_ptr()
        o, v = _fec_counters(out), _fec_counters(vs_sent)
        self._check(getattr(self.lib, fn_name)(self.ctx, d_fix_ptr, d_dec_ptr, d_sent_ptr, n_groups, d_records_ptr, o, v), fn_name)
        if rec is not None:
            # complete on the context's stream: the call has waited for it
            rec = rec.cpu().numpy().view(np.uint32)[:n_groups * GROUP * 2].copy().view(fec_record_dtype())
        return rec, (list(o) if o is not None else None), (list(v) if v is not None else None)

    def fec_status_device(self, d_fix_ptr, d_dec_ptr, d_sent_ptr, n_groups, records=True, out=True, vs_sent=None, d_records_ptr=None):
        """lnsfaid_fec_status_device: device pointers (d_fix_ptr / d_sent_ptr may be None).  Returns (records, out, vs_sent) like
        fec_status_host; records=True stages them through a torch buffer and returns a structured numpy array, d_records_ptr hands the
        call a device buffer of the caller's instead (records is then returned as None)"""
        return self._fec_status_device("lnsfaid_fec_status_device", d_fix_ptr, d_dec_ptr, d_sent_ptr, n_groups, records, out, vs_sent,
                                       d_records_ptr)

    def fec_status_packed_device(self, d_llr4_ptr, d_bits_ptr, d_sent_ptr, n_groups, records=True, out=True, vs_sent=None,
                                 d_records_ptr=None):
        """lnsfaid_fec_status_packed_device: d_llr4_ptr (or None) / d_bits_ptr in the packed decode I/O formats, d_sent_ptr int8"""
        return self._fec_status_device("lnsfaid_fec_status_packed_device", d_llr4_ptr, d_bits_ptr, d_sent_ptr, n_groups, records, out,
                                       vs_sent, d_records_ptr)

    def frontend_sent_bits(self):
        """lnsfaid_frontend_sent_bits: device pointer of the frames set_frames / random_frames left, None while none are set"""
        p = C.c_void_p()
        self._check(self.lib.lnsfaid_frontend_sent_bits(self.ctx, C.byref(p)), "lnsfaid_frontend_sent_bits")
        return p.value

    def encode(self, info, n_groups):
        """info: numpy int8 0/1, [32][K] per group.  Returns the encoder output, [32][K] then [32][M] per group."""
        import numpy as np
        K, N = self.code50.K, self.code50.N
        assert info.dtype == np.int8 and info.size == n_groups * GROUP * K and info.flags.c_contiguous
        out = np.empty(n_groups * GROUP * N, dtype=np.int8)
        self._check(self.lib.lnsfaid_encode(self.ctx, info.ctypes.data, n_groups, out.ctypes.data), "lnsfaid_encode")
        return out

    def encode_device(self, d_in_ptr, n_groups, d_out_ptr):
        self._check(self.lib.lnsfaid_encode_device(self.ctx, d_in_ptr, n_groups, d_out_ptr), "lnsfaid_encode_device")

    def random_frames(self, keys):
        """lnsfaid_frontend_random_frames: one uint64 key per stream"""
        buf = (C.c_uint64 * len(keys))(*[int(k) for k in keys])
        self._check(self.lib.lnsfaid_frontend_random_frames(self.ctx, buf, len(keys)), "lnsfaid_frontend_random_frames")

    def comm_init(self, n_ranks, rank, comm_id):
        self._check(self.lib.lnsfaid_comm_init(self.ctx, n_ranks, rank, comm_id), "lnsfaid_comm_init")

    def allreduce_counters(self, counters):
        buf = (C.c_uint64 * 4)(*[int(c) for c in counters])
        self._check(self.lib.lnsfaid_allreduce_counters(self.ctx, buf), "lnsfaid_allreduce_counters")
        return list(buf)

    def select_kernel(self, rows_per_lane):
        self._check(self.lib.lnsfaid_select_kernel(self.ctx, rows_per_lane), "lnsfaid_select_kernel")

    def rows_per_lane(self):
        return self.lib.lnsfaid_kernel_rows_per_lane(self.ctx)

    def select_waves(self, waves_per_codeword):
        self._check(self.lib.lnsfaid_select_waves(self.ctx, waves_per_codeword), "lnsfaid_select_waves")

    def kernel_waves(self):
        return self.lib.lnsfaid_kernel_waves(self.ctx)

    def select_message_store(self, where):
        """0 default, MSG_REGISTERS, MSG_HBM (lnsfaid_select_message_store)"""
        self._check(self.lib.lnsfaid_select_message_store(self.ctx, where), "lnsfaid_select_message_store")

    def message_store(self):
        return self.lib.lnsfaid_message_store(self.ctx)

    def select_zero_shift(self, mode):
        """0 default, ZERO_SHIFT_ON, ZERO_SHIFT_OFF, ZERO_SHIFT_LOOP, ZERO_SHIFT_STATIC, ZERO_SHIFT_WINDOWED (lnsfaid_select_zero_shift)"""
        self._check(self.lib.lnsfaid_select_zero_shift(self.ctx, mode), "lnsfaid_select_zero_shift")

    def zero_shift_groups(self, n_layers=32):
        """(the next decode launches the rotation-free kernel, its rotation-free groups per layer)"""
        zg = (C.c_int32 * n_layers)()
        on = self.lib.lnsfaid_zero_shift_groups(self.ctx, zg, n_layers)
        self._check(min(on, 0), "lnsfaid_zero_shift_groups")
        return on >= 1, list(zg)

    def static_layers(self):
        """the next decode launches the layer-static kernel (lnsfaid_kernel4s.hip)"""
        on = self.lib.lnsfaid_zero_shift_groups(self.ctx, None, 0)
        self._check(min(on, 0), "lnsfaid_zero_shift_groups")
        return on == 2

    def window_free(self):
        """the next decode launches the layer-static kernel's window-free form (lnsfaid_kernel4w.hip)"""
        on = self.lib.lnsfaid_window_free(self.ctx)
        self._check(min(on, 0), "lnsfaid_window_free")
        return on == 1

    def select_edge_words(self, on):
        """True (default): the edge-word twin where the window-free form applies; False: lnsfaid_kernel4w.hip (lnsfaid_select_edge_words)"""
        self._check(self.lib.lnsfaid_select_edge_words(self.ctx, 1 if on else 0), "lnsfaid_select_edge_words")

    def edge_words(self):
        """the next decode launches the window-free form's edge-word twin (lnsfaid_kernel4e.hip)"""
        on = self.lib.lnsfaid_edge_words(self.ctx)
        self._check(min(on, 0), "lnsfaid_edge_words")
        return on == 1

    def kernel_residency(self):
        """(workgroups per CU of the selected kernel, what its LDS alone allows)"""
        wg, lim = C.c_int32(), C.c_int32()
        self._check(self.lib.lnsfaid_kernel_residency(self.ctx, C.byref(wg), C.byref(lim)), "lnsfaid_kernel_residency")
        return wg.value, lim.value

    def kernel_time(self, reset=False):
        ms = C.c_double()
        n = C.c_uint64()
        self._check(self.lib.lnsfaid_kernel_time(self.ctx, C.byref(ms), C.byref(n), 1 if reset else 0), "lnsfaid_kernel_time")
        return ms.value, n.value

    def close(self):
        if self.ctx:
            self.lib.lnsfaid_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
