"""ctypes binding of libtezip_hip.so (the C ABI declared in include/tezip_hip.h).

This is the whole Python <-> native boundary: plain pointers and sizes.  Arguments may be
numpy arrays (host memory) or torch CUDA tensors (device memory; only `.data_ptr()` is
used).  There is NO CPU fallback: if the library is missing or no GPU is usable the calls
raise.

Streams: work on device buffers is enqueued on the context's stream and is complete only after
`Context.synchronize()`.  When torch produces or consumes those buffers either create the
context on a torch stream (`s = torch.cuda.Stream(); Context(dev, stream=s.cuda_stream)` and run
the torch side under `torch.cuda.stream(s)`) or synchronise both sides explicitly (bench.py and
tezip_amd.dist.HipEngine do the latter).  torch's DEFAULT stream has the handle 0, which the C ABI
reads as "make your own stream": such a context does not share anything with torch.  A process that hands the library torch's
streams or tensors imports torch BEFORE the first Context is made (bench.py does): the library then binds to the HIP runtime torch has
loaded; the other way round the process holds two runtimes, and torch's finds no device."""
import ctypes as C
import os
import threading

import numpy as np

from .ssim import SSIM_DTYPE   # tz_frame_ssim as a numpy record (24 bytes)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libtezip_hip.so")

TZ_OK = 0
TZ_NBINS = 2111
HUFFR_NTOK = 8          # TZ_HUFFR_NTOK: repeat tokens behind the literals of a tz_huffr_* code
TZ_MAX_TABLE = 1021
MODES = {"abs": 0, "rel": 1, "absrel": 2, "pwrel": 3}
QUANTISERS = ("greedy", "lattice")   # tz_set_quantiser: 0 = compress.py:23-70, 1 = TZ-QL1 (tezip_amd/lattice.py)

_SIGS = {
    "tz_version": (C.c_int, []),
    "tz_build_info": (C.c_char_p, []),
    "tz_strerror": (C.c_char_p, [C.c_int]),
    "tz_last_error": (C.c_char_p, [C.c_void_p]),
    "tz_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "tz_ctx_destroy": (C.c_int, [C.c_void_p]),
    "tz_ctx_synchronize": (C.c_int, [C.c_void_p]),
    "tz_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "tz_model_load": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tz_model_prepare": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "tz_predict_c0": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tz_predict_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_predict_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_set_conv_impl": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_scan_fault_inject": (C.c_int, [C.c_void_p, C.c_uint, C.c_uint]),
    "tz_pool_held": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "tz_set_contract": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_get_contract": (C.c_int, [C.c_void_p]),
    "tz_rollout_contract": (C.c_int, [C.c_void_p]),
    "tz_act_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tz_rollout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                             C.c_void_p, C.c_void_p]),
    "tz_rollout_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_rollout_closed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                    C.c_void_p]),
    "tz_rollout_loop": (C.c_int, [C.c_void_p]),
    "tz_rollout_closed_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_ulonglong,
                                           C.c_void_p]),
    "tz_rollout_closed_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_loop_frame_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "tz_loop_search_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "tz_rollout_decode_closed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_int, C.c_void_p]),
    "tz_set_pred_select": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_get_pred_select": (C.c_int, [C.c_void_p]),
    "tz_pred_modes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "tz_put_pred_modes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "tz_set_pred_motion": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_get_pred_motion": (C.c_int, [C.c_void_p]),
    "tz_pred_vectors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "tz_put_pred_vectors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "tz_range_restart": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "tz_rollout_decode_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]),
    "tz_undelta_carry": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_int16)]),
    "tz_decode_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_encode_quality": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_encode_digests": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_bound_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]),
    "tz_bound_err": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "tz_frame_digests": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "tz_ssim_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_encode_ssim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_decoded_digests": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_frames_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "tz_frames_put": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_frames_fence": (C.c_int, [C.c_void_p]),
    "tz_frames_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_payload_begin": (C.c_int, [C.c_void_p, C.c_size_t]),
    "tz_payload_put": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_decoded_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_payload_get": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_set_payload_deferred": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_set_payload_channels": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_get_payload_channels": (C.c_int, [C.c_void_p]),
    "tz_set_delta_stride": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_get_delta_stride": (C.c_int, [C.c_void_p]),
    "tz_set_delta_plane": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_get_delta_plane": (C.c_int, [C.c_void_p]),
    "tz_spatial_delta_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_spatial_undelta_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_set_frame_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "tz_get_frame_bounds": (C.c_int, [C.c_void_p]),
    "tz_error_bound_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_set_bound_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "tz_get_bound_map": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tz_error_bound_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_lattice_bound_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_map_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_encode_map_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_set_quantiser": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_get_quantiser": (C.c_int, [C.c_void_p]),
    "tz_lattice_bound": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_double, C.c_double]),
    "tz_lattice_bound_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_spatial_delta_stride": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_spatial_undelta_stride": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_undelta_carry_stride": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_spatial_delta_gray": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int16, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_reconstruct_gray": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    "tz_payload_wait": (C.c_int, [C.c_void_p]),
    "tz_get_predictions": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tz_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                            C.POINTER(C.c_int), C.c_void_p]),
    "tz_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "tz_host_free": (C.c_int, [C.c_void_p]),
    "tz_encode_delta": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]),
    "tz_encode_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_encode_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_int16, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_decode_delta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tz_delta_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_error_bound": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_double, C.c_double]),
    "tz_spatial_delta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int16, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_byte_shuffle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tz_byte_unshuffle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tz_build_table": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "tz_remap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_unmap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_spatial_undelta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int16, C.c_void_p]),
    "tz_reconstruct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p]),
    "tz_window_sse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tz_huff_lengths": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_huff_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tz_huff_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "tz_huff_get": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_huff_begin": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "tz_huff_put": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_huff_decode": (C.c_int, [C.c_void_p]),
    "tz_huff_encode_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "tz_huff_decode_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    "tz_huffr_lengths": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tz_huffr_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tz_huffr_counts_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tz_huffr_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "tz_huffr_get": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_huffr_begin": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "tz_huffr_put": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_huffr_decode": (C.c_int, [C.c_void_p]),
    "tz_huffr_encode_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "tz_huffd_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tz_huffd_counts_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tz_huffd_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "tz_huffd_get": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_huffd_begin": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tz_huffd_put": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_huffd_decode": (C.c_int, [C.c_void_p]),
    "tz_huffd_encode_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "tz_huffd_decode_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    "tz_huffr_decode_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    "tz_size_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]),
    "tz_size_count_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "tz_size_bits_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]),
    "tz_sdelta_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]),
    "tz_size_count_plane_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_int)]),
    "tz_size_bits_plane_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]),
    "tz_keys_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_keys_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "tz_keys_get": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_keys_begin": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_keys_put": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_keys_decode": (C.c_int, [C.c_void_p]),
    "tz_keys_residual_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_keys_unresidual_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_keys_gray": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tz_keysg_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "tz_keysg_get": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_keysg_begin": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_keysg_put": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "tz_keysg_decode": (C.c_int, [C.c_void_p]),
    "tz_keysg_residual_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_keysg_unresidual_buf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tz_timer_start": (C.c_int, [C.c_void_p]),
    "tz_timer_stop": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "tz_prof_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "tz_prof_count": (C.c_int, []),
    "tz_prof_name": (C.c_char_p, [C.c_int]),
    "tz_prof_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "tz_prof_reset": (C.c_int, [C.c_void_p]),
}
EXPORTS = sorted(_SIGS)


class FrameQuality(C.Structure):
    """tz_frame_quality: one record of tz_encode_quality (16 bytes)."""
    _fields_ = [("sse", C.c_ulonglong), ("max_abs", C.c_uint), ("n_changed", C.c_uint)]


QUALITY_DTYPE = np.dtype([("sse", "<u8"), ("max_abs", "<u4"), ("n_changed", "<u4")])   # the same layout as a numpy record
# tz_map_record (16 bytes): one frame of tz_map_check / tz_encode_map_check
MAP_DTYPE = np.dtype([("violations", "<u8"), ("max_excess", "<u4"), ("reserved", "<u4")])
# tz_size_record (64 bytes): one candidate of tz_size_probe
SIZE_DTYPE = np.dtype([("n", "<u8"), ("stream_words", "<u8"), ("bytes", "<u8"), ("cost_bits", "<u8", (3,)), ("A", "<i4"), ("base", "<i4"),
                       ("dist", "<i4"), ("table_len", "<i4")])
SIZE_CODERS = {"huff": 0, "huffr": 1, "huffd": 2}   # the `coder` argument of tz_size_probe
SIZE_BINS, SIZE_BIAS = 4096, 1024                   # TZ_SIZE_BINS, TZ_SIZE_BIAS: the literal bins of the size seams

_LIB = None


class TezipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("tezip_hip status %d: %s" % (status, message))
        self.status = status


def load():
    """Load libtezip_hip.so; raises if it has not been built (python -m tezip_amd.build)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -m tezip_amd.build` "
                              "(there is no CPU fallback)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIB = lib
        if diagnostic_defines(lib) and not os.environ.get("TEZIP_ALLOW_DIAGNOSTIC_BUILD"):
            _LIB = None
            raise ImportError("%s is a MEASUREMENT build (%s; compiled with TEZIP_DEFINES): its kernels are ablated or "
                              "instrumented and must not serve jobs, tests or the bench.  Rebuild with `python -m "
                              "tezip_amd.build` (TEZIP_DEFINES unset), or set TEZIP_ALLOW_DIAGNOSTIC_BUILD=1 in a "
                              "measurement script." % (LIB_PATH, " ".join(diagnostic_defines(lib))))
    return _LIB


def build_info(lib=None):
    return (lib or load()).tz_build_info().decode()


def diagnostic_defines(lib=None):
    """The diagnostic switches the loaded library was compiled with (tz_build_info), [] for a product build."""
    return build_info(lib).split("defines:", 1)[1].split()


def pad8(v):
    return (v + 7) // 8 * 8


def range_restart(key_mask, warm_up, first):
    """tz_range_restart (host only): the frame a decoder restarts its rollout at to reproduce frame `first`."""
    km = np.ascontiguousarray(key_mask, np.uint8)
    r = C.c_int(0)
    rc = load().tz_range_restart(km.ctypes.data, int(km.size), int(warm_up), int(first), C.byref(r))
    if rc != TZ_OK:
        raise TezipError(rc, "tz_range_restart: first=%d outside a %d-frame mask, or warm_up=%d < 0" % (first, km.size, warm_up))
    return r.value


def _numel(x):
    return int(x.numel()) if hasattr(x, "numel") else int(np.asarray(x).size)


def _dist(dist):
    """The match-distance argument of a tz_huffd_* call; the other families' calls have none."""
    return () if dist is None else (int(dist),)


class _Pinned:
    """Owner of one tz_host_alloc block (freed when the last numpy view goes away)."""

    def __init__(self, lib, ptr, nbytes):
        self.lib, self.ptr = lib, ptr
        self.__array_interface__ = {"data": (ptr, False), "shape": (nbytes,), "typestr": "|u1", "version": 3}

    def __del__(self):
        try:
            self.lib.tz_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


def pinned_empty(shape, dtype):
    """numpy array in page-locked host memory (tz_host_alloc): the library DMAs such buffers
    directly and overlaps the transfers with the predictor.  Needs a GPU (raises otherwise)."""
    lib = load()
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    p = C.c_void_p()
    rc = lib.tz_host_alloc(max(nbytes, 16), C.byref(p))
    if rc != TZ_OK:
        raise TezipError(rc, lib.tz_strerror(rc).decode() + " (tz_host_alloc)")
    owner = _Pinned(lib, p.value, max(nbytes, 16))
    return np.asarray(owner)[:nbytes].view(dtype).reshape(shape)


def pinned_copy(arr):
    out = pinned_empty(arr.shape, arr.dtype)
    out[...] = arr
    return out


class _ResultPool:
    """Recycled host buffers for the big results (payload, decoded frames).  A fresh np.empty costs a
    page fault per 4 KB while the staging threads fill it (126 MB payload of cfg3: 10 ms, as long as
    everything the GPU does in tz_encode); a block that comes back when the caller drops the array
    has its pages already.  (Page-locked blocks would save 1-2 ms more per call but cost 85 ms per
    500 MB the first time; callers who want that pass their own pinned_empty buffer.)  The MAX_FREE /
    MAX_FREE_BYTES most recently returned blocks are kept.  TEZIP_RESULT_POOL=0 turns the pool off."""
    MIN_BYTES, MAX_FREE, MAX_FREE_BYTES = 1 << 20, 6, 3 << 30

    def __init__(self):
        self.free = []                       # [uint8 base arrays], newest last
        self.lock = threading.RLock()        # (a finaliser may run inside empty())
        self.on = os.environ.get("TEZIP_RESULT_POOL", "1") != "0"

    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if not self.on or nbytes < self.MIN_BYTES:
            return np.empty(shape, dtype)
        base = None
        with self.lock:
            best = None
            for i, b in enumerate(self.free):
                if nbytes <= b.size <= 2 * nbytes and (best is None or b.size < self.free[best].size):
                    best = i
            if best is not None:
                base = self.free.pop(best)
        if base is None:
            base = np.empty((nbytes + (1 << 21) - 1) >> 21 << 21, np.uint8)
        return np.asarray(_Pooled(self, base))[:nbytes].view(dtype).reshape(shape)

    def give(self, base):
        with self.lock:
            self.free.append(base)
            while len(self.free) > self.MAX_FREE or sum(b.size for b in self.free) > self.MAX_FREE_BYTES:
                self.free.pop(0)


class _Pooled:
    """Owner of a pooled block: the arrays handed out are views of it; when the last one goes, the block
    returns to the pool."""

    def __init__(self, pool, base):
        self.pool, self.base = pool, base
        self.__array_interface__ = {"data": (base.ctypes.data, False), "shape": (base.size,), "typestr": "|u1", "version": 3}

    def __del__(self):
        try:
            self.pool.give(self.base)
        except Exception:
            pass


_RESULTS = _ResultPool()


def _ptr(x, dtype=None):
    """Pointer of a numpy array (host) or torch tensor (device or host)."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        if dtype is not None and x.dtype != dtype:
            raise TypeError("expected %s, got %s" % (dtype, x.dtype))
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr()
    raise TypeError("unsupported buffer type %r" % type(x))


def _bounds(bound):
    """-b values -> (b0, b1) of the C ABI (b1 is absrel's rel bound, 0 for the other modes)."""
    return float(bound[0]), float(bound[1]) if len(bound) > 1 else 0.0


def _carry(carry, stride):
    """The carry argument of a tz_*_stride seam: `stride` int16 elements on the host (a scalar serves stride 1)."""
    c = np.ascontiguousarray(np.atleast_1d(np.asarray(carry)).astype(np.int16))
    if c.size != int(stride):
        raise ValueError("the carry holds %d elements, the stride is %d" % (c.size, int(stride)))
    return c


def _payload_out(out, n):
    """An encoder's payload output -> the buffer passed on and returned: "resident" keeps the payload in the context
    (payload_get) and is None, None is a new host array of n int16, anything else a host or device buffer."""
    if isinstance(out, str) and out == "resident":
        return None
    return _RESULTS.empty(n, np.int16) if out is None else out


class Context:
    """One context per GPU/process (tz_ctx)."""

    def __init__(self, device=0, stream=None):
        """stream: a hipStream_t handle as an int (a torch.cuda.Stream's .cuda_stream), or None / 0 for a stream of the
        context's own (see the module docstring)."""
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.tz_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != TZ_OK:
            raise TezipError(rc, self.lib.tz_strerror(rc).decode() + " (tz_ctx_create; a MI355X is required)")
        self.h = h
        self.channels = 3

    def close(self):
        if getattr(self, "h", None):
            self.lib.tz_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def _ck(self, rc):
        if rc != TZ_OK:
            msg = self.lib.tz_last_error(self.h).decode() or self.lib.tz_strerror(rc).decode()
            raise TezipError(rc, msg)

    def synchronize(self):
        self._ck(self.lib.tz_ctx_synchronize(self.h))

    # ---- model
    def load_model(self, config, weights):
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        shapes = config.weight_shapes()
        if len(ws) != len(shapes) or any(tuple(w.shape) != s for w, (_, s) in zip(ws, shapes)):
            raise ValueError("weight list does not match the model (prednet.py:210-227 order)")
        ptrs = (C.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        st = np.array(config.stack_sizes, dtype=np.int32)
        rs = np.array(config.R_stack_sizes, dtype=np.int32)
        self._ck(self.lib.tz_model_load(self.h, config.nb_layers, st.ctypes.data, rs.ctypes.data,
                                        C.cast(ptrs, C.c_void_p)))
        self.config = config

    def prepare(self, hp, wp, max_batch=1):
        self._ck(self.lib.tz_model_prepare(self.h, hp, wp, max_batch))
        self.hp, self.wp = hp, wp

    def predict_c0(self):
        out = np.empty((self.hp, self.wp, 3), np.float32)
        self._ck(self.lib.tz_predict_c0(self.h, out.ctypes.data))
        return out

    def predict_next(self, frames, out=None):
        n = frames.shape[0]
        if out is None:
            out = np.empty((n, self.hp, self.wp, 3), np.float32)
        self._ck(self.lib.tz_predict_next(self.h, _ptr(frames, np.float32), n, _ptr(out, np.float32)))
        return out

    def predict_tap(self, kind, level):
        st, rs = self.config.stack_sizes, self.config.R_stack_sizes
        ch = 2 * st[level] if kind == 0 else rs[level]
        out = np.empty((self.hp >> level, self.wp >> level, ch), np.float32)
        self._ck(self.lib.tz_predict_tap(self.h, kind, level, out.ctypes.data))
        return out

    def act_probe(self, x, check_reciprocal=False):
        """Diagnostic: (hard_sigmoid(x), tanh(x)) as the kernels compute them; check_reciprocal adds the count of
        float32 d in [4, 2^27] whose division-free 1 - 2/d differs from the division (must be 0)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        hs, th = np.empty_like(x), np.empty_like(x)
        bad = C.c_ulonglong(0)
        self._ck(self.lib.tz_act_probe(self.h, x.ctypes.data, x.size, hs.ctypes.data, th.ctypes.data,
                                       C.byref(bad) if check_reciprocal else None))
        return (hs, th, int(bad.value)) if check_reciprocal else (hs, th)

    def set_conv_impl(self, lds_dma, lat=None):
        """Diagnostic: 1 = LDS-DMA convolution kernels where they apply (default), 0 = the general kernel.
        lat: None = k_convlat where the cost model picks it (default), "never", "always"."""
        code = {None: 0, "never": 1, "always": 2}[lat]
        self._ck(self.lib.tz_set_conv_impl(self.h, int(bool(lds_dma)) | (code << 1)))

    def set_contract(self, contract):
        """Arithmetic contract of the predictor: 1 = TZ-PA1 (direct fmaf chains), 2 = TZ-PA2 (Winograd chains on the
        same-resolution sources of levels >= 1).  Encoder and decoder must agree."""
        self._ck(self.lib.tz_set_contract(self.h, int(contract)))

    def get_contract(self):
        return int(self.lib.tz_get_contract(self.h))

    def rollout_contract(self):
        """The contract the resident prediction stack was made under (the stamp tz_rollout / tz_rollout_decode left)."""
        rc = int(self.lib.tz_rollout_contract(self.h))
        if rc < 0:
            self._ck(rc)
        return rc

    def scan_fault_inject(self, epoch_skew=0, poll_limit=0):
        """Diagnostic: make the inverse scan's bounded wait expire (see tz_scan_fault_inject); (0, 0) = normal."""
        self._ck(self.lib.tz_scan_fault_inject(self.h, int(epoch_skew), int(poll_limit)))

    def pool_held(self):
        """Diagnostic: (blocks of the device scratch pool handed out right now, blocks the pool holds); 0 between calls."""
        blocks = C.c_int(0)
        held = int(self.lib.tz_pool_held(self.h, C.byref(blocks)))
        if held < 0:
            self._ck(held)
        return held, int(blocks.value)

    # ---- rollout + encode / decode
    @staticmethod
    def _check_stack(x, what):
        if len(x.shape) != 4 or x.shape[3] != 3:  # compress.py:114: grayscale is expanded to 3 channels first
            raise ValueError("%s must be a (nt, H, W, 3) uint8 stack, got shape %r" % (what, tuple(x.shape)))

    # streaming ingestion / delivery (tz_frames_* / tz_payload_get)
    def frames_begin(self, nt, h, w):
        self._ck(self.lib.tz_frames_begin(self.h, nt, h, w))
        self._staged = (nt, h, w)

    def frames_put(self, first, frames):
        self._check_stack(frames, "frames")
        self._ck(self.lib.tz_frames_put(self.h, int(first), int(frames.shape[0]), _ptr(frames, np.uint8)))

    def frames_fence(self):
        self._ck(self.lib.tz_frames_fence(self.h))

    def frames_get(self, first, count, out=None):
        nt, h, w = self._shape
        if out is None:
            out = np.empty((count, h, w, 3), np.uint8)
        self._ck(self.lib.tz_frames_get(self.h, int(first), int(count), _ptr(out)))
        return out

    def payload_begin(self, count):
        self._ck(self.lib.tz_payload_begin(self.h, int(count)))

    def payload_put(self, offset, piece):
        self._ck(self.lib.tz_payload_put(self.h, int(offset), _numel(piece), _ptr(piece, np.int16)))

    def decoded_get(self, first, count, out=None):
        nt, h, w = self._shape
        if out is None:
            out = np.empty((count, h, w, 3), np.uint8)
        self._ck(self.lib.tz_decoded_get(self.h, int(first), int(count), _ptr(out)))
        return out

    def payload_get(self, offset, count, out=None):
        if out is None:
            out = np.empty(count, np.int16)
        self._ck(self.lib.tz_payload_get(self.h, int(offset), int(count), _ptr(out)))
        return out

    def rollout(self, frames, warm_up, window, threshold=0.0, want_mse=False):
        """frames: (nt,H,W,3) uint8 stack (host or device), or None after frames_begin / frames_put."""
        if frames is None:
            nt, h, w = self._staged
        else:
            self._check_stack(frames, "frames")
            nt, h, w = frames.shape[:3]
        key = np.zeros(nt, np.uint8)
        mse = np.zeros(nt, np.float64) if want_mse else None
        self._ck(self.lib.tz_rollout(self.h, None if frames is None else _ptr(frames, np.uint8), nt, h, w, warm_up, int(window or 0),
                                     float(threshold or 0.0), key.ctypes.data, _ptr(mse)))
        self._shape = (nt, h, w)
        return key.astype(bool), mse

    def rollout_decode(self, key_frames, warm_up):
        """key_frames: the (nt,H,W,3) key stack, or None after frames_begin / frames_put."""
        if key_frames is None:
            nt, h, w = self._staged
        else:
            self._check_stack(key_frames, "key_frames")
            nt, h, w = key_frames.shape[:3]
        key = np.zeros(nt, np.uint8)
        self._ck(self.lib.tz_rollout_decode(self.h, None if key_frames is None else _ptr(key_frames, np.uint8), nt, h, w,
                                            warm_up, key.ctypes.data))
        self._shape = (nt, h, w)
        return key.astype(bool)

    def rollout_closed(self, frames, warm_up, window, mode="abs", bound=(0.0,)):
        """tz_rollout_closed (TZ-CL1, tezip_amd/closedloop.py): the rollout of the job (mode, bound) under the quantiser in force
        with the DECODED frame fed back; frames as for rollout.  Returns the key mask."""
        if frames is None:
            nt, h, w = self._staged
        else:
            self._check_stack(frames, "frames")
            nt, h, w = frames.shape[:3]
        b0, b1 = _bounds(bound)
        key = np.zeros(nt, np.uint8)
        self._ck(self.lib.tz_rollout_closed(self.h, None if frames is None else _ptr(frames, np.uint8), nt, h, w, warm_up, int(window or 0),
                                            MODES[mode], b0, b1, key.ctypes.data))
        self._shape = (nt, h, w)
        return key.astype(bool)

    def rollout_closed_frames(self, frames, warm_up, window, bounds=None, sse_limit=0):
        """tz_rollout_closed_frames (TZ-CLF1, tezip_amd/closedframes.py): the closed loop under one abs bound per frame -- `bounds`
        (nt numbers), or found inside the loop so that every frame's sse stays <= `sse_limit` (> 0); exactly one of the two.  Needs
        the lattice quantiser; frames as for rollout.  Returns the key mask; loop_frame_bounds() has the bounds of the job, which
        runs under set_frame_bounds of exactly those."""
        if frames is None:
            nt, h, w = self._staged
        else:
            self._check_stack(frames, "frames")
            nt, h, w = frames.shape[:3]
        b = None
        if bounds is not None:
            b = np.ascontiguousarray(bounds, np.float64)
            if b.shape != (nt,):
                raise ValueError("%d bounds for %d frames" % (b.size, nt))
        key = np.zeros(nt, np.uint8)
        self._ck(self.lib.tz_rollout_closed_frames(self.h, None if frames is None else _ptr(frames, np.uint8), nt, h, w, warm_up,
                                                   int(window or 0), None if b is None else b.ctypes.data, int(sse_limit), key.ctypes.data))
        self._shape = (nt, h, w)
        return key.astype(bool)

    def rollout_closed_map(self, frames, warm_up, window):
        """tz_rollout_closed_map (TZ-CLM1, tezip_amd/closedmap.py): the closed loop under the bound map in force (set_bound_map), one
        abs bound per pixel; with set_pred_select(True) the per-tile selection under that map.  Needs the lattice quantiser; frames
        as for rollout.  Returns the key mask; the job runs under the same map: encode("abs", [0.0], ...)."""
        if frames is None:
            nt, h, w = self._staged
        else:
            self._check_stack(frames, "frames")
            nt, h, w = frames.shape[:3]
        key = np.zeros(nt, np.uint8)
        self._ck(self.lib.tz_rollout_closed_map(self.h, None if frames is None else _ptr(frames, np.uint8), nt, h, w, warm_up,
                                                int(window or 0), key.ctypes.data))
        self._shape = (nt, h, w)
        return key.astype(bool)

    def loop_frame_bounds(self):
        """tz_loop_frame_bounds: (bounds float64[nt], sse uint64[nt]) of the resident rollout_closed_frames; sse is zero after
        given bounds."""
        nt = self._shape[0]
        bounds, sse = np.zeros(nt, np.float64), np.zeros(nt, np.uint64)
        rc = int(self.lib.tz_loop_frame_bounds(self.h, bounds.ctypes.data, sse.ctypes.data, nt))
        if rc < 0:
            self._ck(rc)
        return bounds, sse

    def loop_search_trace(self):
        """tz_loop_search_trace: uint64 (9, nt), the sse of every bisection round and frame; 2**64 - 1 where a round did not run."""
        nt = self._shape[0]
        out = np.zeros((9, nt), np.uint64)
        rc = int(self.lib.tz_loop_search_trace(self.h, out.ctypes.data, out.size))
        if rc < 0:
            self._ck(rc)
        return out

    def rollout_loop(self):
        """tz_rollout_loop: 1 when the resident predictions are a closed loop's, 0 after any other rollout."""
        rc = int(self.lib.tz_rollout_loop(self.h))
        if rc < 0:
            self._ck(rc)
        return rc

    def rollout_decode_closed(self, key_frames, warm_up, payload, table):
        """tz_rollout_decode_closed: the decoder of a closed-loop stream.  key_frames as for rollout_decode; payload None: the
        pieces staged with payload_begin / payload_put.  The decoded frames stay in the context (decoded_get); returns the
        key mask."""
        if key_frames is None:
            nt, h, w = self._staged
        else:
            self._check_stack(key_frames, "key_frames")
            nt, h, w = key_frames.shape[:3]
        n = nt * h * w * 3
        if payload is not None and _numel(payload) != n:
            raise ValueError("payload holds %d elements, expected %d" % (_numel(payload), n))
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        key = np.zeros(nt, np.uint8)
        self._ck(self.lib.tz_rollout_decode_closed(self.h, None if key_frames is None else _ptr(key_frames, np.uint8), nt, h, w, warm_up,
                                                   None if payload is None else _ptr(payload), n, _ptr(tb), tl, key.ctypes.data))
        self._shape = (nt, h, w)
        return key.astype(bool)

    def set_pred_select(self, on):
        """tz_set_pred_select (TZ-PS1, tezip_amd/predselect.py): rollout_closed / rollout_decode_closed choose per 16 x 16 tile
        between the network's prediction and the decoded frame in front.  Off by default."""
        self._ck(self.lib.tz_set_pred_select(self.h, int(bool(on))))

    def get_pred_select(self):
        return int(self.lib.tz_get_pred_select(self.h))

    def pred_modes(self):
        """tz_pred_modes: the modes of the resident rollout_closed under selection, uint8 (nt, ceil(H/16), ceil(W/16))."""
        nt, h, w = self._shape
        out = np.zeros((nt, (h + 15) // 16, (w + 15) // 16), np.uint8)
        self._ck(self.lib.tz_pred_modes(self.h, out.ctypes.data, out.size))
        return out

    def put_pred_modes(self, modes):
        """tz_put_pred_modes: the stored modes of a stream, ahead of rollout_decode_closed under selection."""
        m = np.ascontiguousarray(modes, np.uint8)
        self._ck(self.lib.tz_put_pred_modes(self.h, m.ctypes.data, m.size))

    def set_pred_motion(self, r):
        """tz_set_pred_motion (TZ-PM1, tezip_amd/predmotion.py): rollout_closed / rollout_decode_closed choose per 16 x 16 tile
        between the network's prediction and the decoded frame in front displaced by a vector of up to r = 7 pixels.  0 (the
        default): off.  Excludes set_pred_select(True)."""
        self._ck(self.lib.tz_set_pred_motion(self.h, int(r)))

    def get_pred_motion(self):
        return int(self.lib.tz_get_pred_motion(self.h))

    def pred_vectors(self):
        """tz_pred_vectors: the vectors of the resident rollout_closed under motion, int8 (nt, ceil(H/16), ceil(W/16), 2) of (dy, dx)."""
        nt, h, w = self._shape
        out = np.zeros((nt, (h + 15) // 16, (w + 15) // 16, 2), np.int8)
        self._ck(self.lib.tz_pred_vectors(self.h, out.ctypes.data, out.size))
        return out

    def put_pred_vectors(self, vectors):
        """tz_put_pred_vectors: the stored vectors of a stream, next to put_pred_modes, ahead of rollout_decode_closed under motion."""
        v = np.ascontiguousarray(vectors, np.int8)
        self._ck(self.lib.tz_put_pred_vectors(self.h, v.ctypes.data, v.size))

    def rollout_decode_range(self, key_frames, warm_up, first, count):
        """tz_rollout_decode for frames [first, first + count) only; key_frames as for rollout_decode.  Returns the key mask
        of the whole stack."""
        if key_frames is None:
            nt, h, w = self._staged
        else:
            self._check_stack(key_frames, "key_frames")
            nt, h, w = key_frames.shape[:3]
        key = np.zeros(nt, np.uint8)
        self._ck(self.lib.tz_rollout_decode_range(self.h, None if key_frames is None else _ptr(key_frames, np.uint8), nt, h, w,
                                                  warm_up, int(first), int(count), key.ctypes.data))
        self._shape = (nt, h, w)
        return key.astype(bool)

    def get_predictions(self, out=None):
        """out: a host or device buffer of nt*Hp*Wp*3 float32 (default: a new numpy array)."""
        nt, h, w = self._shape
        if out is None:
            out = np.empty((nt, pad8(h), pad8(w), 3), np.float32)
        elif _numel(out) != nt * pad8(h) * pad8(w) * 3:
            raise ValueError("prediction buffer holds %d elements, expected %d" % (_numel(out), nt * pad8(h) * pad8(w) * 3))
        self._ck(self.lib.tz_get_predictions(self.h, _ptr(out)))
        return out

    def byte_shuffle(self, x, out=None):
        n = _numel(x)
        if out is None:
            out = np.empty(2 * n, np.uint8)
        self._ck(self.lib.tz_byte_shuffle(self.h, _ptr(x), n, _ptr(out)))
        return out

    def byte_unshuffle(self, planes, out=None):
        n = _numel(planes) // 2
        if out is None:
            out = np.empty(n, np.int16)
        self._ck(self.lib.tz_byte_unshuffle(self.h, _ptr(planes), n, _ptr(out)))
        return out

    def encode(self, mode, bound, entropy=True, payload=None, want_delta=False, shuffle=False, delta_out=None):
        """shuffle=True (not a reference format): `payload` then holds the two byte planes of the
        int16 payload (same buffer size), see tz_byte_shuffle.  want_delta / delta_out (a host or
        device buffer of nt*H*W*3 int16): also return the quantised delta stack."""
        nt, h, w = self._shape
        b0, b1 = _bounds(bound)
        payload = _payload_out(payload, nt * h * w * self.channels)
        table = np.zeros(TZ_MAX_TABLE, np.int16)
        tlen = C.c_int(0)
        delta = delta_out if delta_out is not None else (np.empty((nt, h, w, 3), np.int16) if want_delta else None)
        if delta is not None and _numel(delta) != nt * h * w * 3:
            raise ValueError("delta buffer holds %d elements, expected %d" % (_numel(delta), nt * h * w * 3))
        self._ck(self.lib.tz_encode(self.h, MODES[mode], b0, b1, int(bool(entropy)) | (2 if shuffle else 0), _ptr(payload), table.ctypes.data,
                                    C.byref(tlen), _ptr(delta)))
        t = table[: tlen.value].copy() if tlen.value >= 0 else None
        return payload, t, delta

    def set_payload_channels(self, channels):
        """tz_set_payload_channels: 3 (the default) or 1 = the one-channel payload of a gray job (tezip_amd/graypayload.py):
        encode then refuses a stack with colour and yields nt*H*W elements, decode / decode_range / encode_quality /
        encode_digests take as many and still yield 3-channel frames."""
        self._ck(self.lib.tz_set_payload_channels(self.h, int(channels)))
        self.channels = int(channels)

    def get_payload_channels(self):
        return int(self.lib.tz_get_payload_channels(self.h))

    def set_delta_stride(self, mode):
        """tz_set_delta_stride: 0 (the default) = the reference's flat spatial delta, 1 = the spatial delta of the payload at
        the channel stride (tezip_amd/sdelta.py): encode / decode / decode_range / encode_quality / encode_ssim /
        encode_digests work on the strided payload; the sharded entry points and undelta_carry refuse."""
        self._ck(self.lib.tz_set_delta_stride(self.h, int(mode)))

    def get_delta_stride(self):
        return int(self.lib.tz_get_delta_stride(self.h))

    def set_delta_plane(self, on):
        """tz_set_delta_plane: 0 (the default) or 1 = the spatial delta of the payload is the 2-D one, TZ-SD2
        (tezip_amd/sdelta.py encode_plane): encode / decode / decode_range / encode_quality / encode_ssim / encode_digests work
        on the plane payload, a range decode takes no carry; the sharded entry points, the carries and size_probe refuse."""
        self._ck(self.lib.tz_set_delta_plane(self.h, int(on)))

    def get_delta_plane(self):
        return int(self.lib.tz_get_delta_plane(self.h))

    def set_frame_bounds(self, bounds):
        """tz_set_frame_bounds: one abs tolerance per frame of the encoder rollout (None or empty: clear).  While set, encode /
        encode_delta / bound_probe / size_probe take mode "abs", ignore its bound and quantise frame f as abs bounds[f] does;
        the sharded entry points refuse.  A NaN, infinite or negative entry raises and the setting stays as it was."""
        if bounds is None or len(bounds) == 0:
            self._ck(self.lib.tz_set_frame_bounds(self.h, None, 0))
            return
        b = np.ascontiguousarray(bounds, np.float64)
        self._ck(self.lib.tz_set_frame_bounds(self.h, b.ctypes.data, int(b.size)))

    def get_frame_bounds(self):
        return int(self.lib.tz_get_frame_bounds(self.h))

    def set_bound_map(self, bmap):
        """tz_set_bound_map: an H x W uint8 map of abs tolerances, one per pixel, for every frame the encoder quantises
        (TZ-BM1, tezip_amd/boundmap.py; None: clear).  While set, encode / encode_delta / bound_probe / sdelta_probe take mode
        "abs", ignore its bound and hold every sample to its pixel's entry; frame bounds, the sharded entry points and
        size_probe refuse."""
        if bmap is None:
            self._ck(self.lib.tz_set_bound_map(self.h, None, 0, 0))
            return
        m = np.ascontiguousarray(bmap)
        if m.dtype != np.uint8 or m.ndim != 2:
            raise ValueError("a bound map is a 2-D uint8 array, not %s%s" % (m.dtype, m.shape))
        self._ck(self.lib.tz_set_bound_map(self.h, m.ctypes.data, int(m.shape[0]), int(m.shape[1])))

    def get_bound_map(self):
        """tz_get_bound_map: (H, W) of the map in force, or None."""
        h, w = C.c_int(0), C.c_int(0)
        return (h.value, w.value) if self.lib.tz_get_bound_map(self.h, C.byref(h), C.byref(w)) == 1 else None

    def encode_map_check(self, payload="resident", table=None, shuffle=False):
        """tz_encode_map_check after set_bound_map + rollout + encode, arguments as encode_quality's: per frame (violations,
        max_excess) of what the payload decodes to against the originals under the map, as MAP_DTYPE[nt]."""
        nt, h, w = self._shape
        n = nt * h * w * self.channels
        resident = isinstance(payload, str) and payload == "resident"
        if not resident and _numel(payload) != n:
            raise ValueError("payload holds %d elements, expected %d" % (_numel(payload), n))
        out = np.zeros(nt, MAP_DTYPE)
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_encode_map_check(self.h, None if resident else _ptr(payload), n, _ptr(tb), tl, int(bool(shuffle)),
                                              out.ctypes.data))
        return out

    def map_check(self, orig, decoded, bmap, shape):
        """tz_map_check: k_map_check over two uint8 stacks of shape = (nframes, H, W) x 3 and an H x W map (host arrays or
        device tensors): MAP_DTYPE[nframes] (boundmap.check)."""
        n, h, w = (int(v) for v in shape)
        if not (_numel(orig) == _numel(decoded) == n * h * w * 3) or _numel(bmap) != h * w:
            raise ValueError("stacks of %d and %d elements and a map of %d, %d x %d x %d x 3 and %d x %d wanted"
                             % (_numel(orig), _numel(decoded), _numel(bmap), n, h, w, h, w))
        out = np.zeros(max(n, 0), MAP_DTYPE)
        self._ck(self.lib.tz_map_check(self.h, _ptr(orig), _ptr(decoded), _ptr(bmap), n, h, w, out.ctypes.data))
        return out

    def set_quantiser(self, quant):
        """tz_set_quantiser: "greedy" / 0 (the default) = the reference's quantiser, "lattice" / 1 = the lattice quantiser
        TZ-QL1 (tezip_amd/lattice.py) in encode / encode_delta / bound_probe / size_probe."""
        q = QUANTISERS.index(quant) if isinstance(quant, str) else int(quant)
        self._ck(self.lib.tz_set_quantiser(self.h, q))

    def get_quantiser(self):
        return int(self.lib.tz_get_quantiser(self.h))

    def set_payload_deferred(self, on=True):
        """tz_set_payload_deferred: encode(payload=<pinned host buffer>) returns with the device -> host transfer of
        the payload still running; payload_wait() completes it (it overlaps the next sequence's rollout)."""
        self._ck(self.lib.tz_set_payload_deferred(self.h, int(bool(on))))

    def payload_wait(self):
        self._ck(self.lib.tz_payload_wait(self.h))

    def encode_begin(self, mode, bound, entropy=True):
        """First phase of a window-sharded encode (tz_encode_begin): -> (hist uint64[2111] | None,
        first, last) where hist counts this shard's symbols taken without a carry and first / last
        are the edge elements of its quantised delta stack.  The symbols stay in the context."""
        b0, b1 = _bounds(bound)
        hist = np.zeros(TZ_NBINS, np.uint64) if entropy else None
        edge = np.zeros(2, np.int16)
        self._ck(self.lib.tz_encode_begin(self.h, MODES[mode], b0, b1, int(bool(entropy)),
                                          None if hist is None else hist.ctypes.data, edge.ctypes.data))
        return hist, int(edge[0]), int(edge[1])

    def encode_finish(self, carry, table, out=None):
        """Second phase (tz_encode_finish): carry = last delta element of the previous shard (None for
        the first shard), table = the table of the summed histogram (None: no remap).  out: host or
        device buffer, "resident" keeps the payload in the context (payload_get)."""
        nt, h, w = self._shape
        out = _payload_out(out, nt * h * w * 3)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_encode_finish(self.h, int(carry is not None), int(carry or 0), _ptr(tb),
                                           -1 if tb is None else len(tb), _ptr(out)))
        return out

    def stream_ptr(self):
        return self.lib.tz_ctx_stream(self.h)

    def encode_delta(self, mode, bound, out=None):
        nt, h, w = self._shape
        if out is None:
            out = np.empty((nt, h, w, 3), np.int16)
        b0, b1 = _bounds(bound)
        self._ck(self.lib.tz_encode_delta(self.h, MODES[mode], b0, b1, _ptr(out)))
        return out

    def decode_delta(self, delta, out=None):
        nt, h, w = self._shape
        if _numel(delta) != nt * h * w * 3:  # decompress.py:240: the reference's reshape raises
            raise ValueError("delta stack holds %d elements, expected %d" % (_numel(delta), nt * h * w * 3))
        if out is None:
            out = np.empty((nt, h, w, 3), np.uint8)
        self._ck(self.lib.tz_decode_delta(self.h, _ptr(delta), _ptr(out)))
        return out

    def decode(self, payload, table, out=None):
        """payload None: the pieces staged with payload_begin / payload_put.  out="resident": the
        frames stay in the context (decoded_get)."""
        nt, h, w = self._shape
        n = nt * h * w * self.channels
        if payload is not None and _numel(payload) != n:  # decompress.py:240: the reference's reshape raises
            raise ValueError("payload holds %d elements, expected %d" % (_numel(payload), n))
        resident = isinstance(out, str) and out == "resident"
        if resident:
            out = None
        elif out is None:
            out = _RESULTS.empty((nt, h, w, 3), np.uint8)
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_decode(self.h, None if payload is None else _ptr(payload), n, _ptr(tb), tl, _ptr(out)))
        return out

    def decode_range(self, payload, table, first, count, out=None):
        """tz_decode_range: frames [first, first + count) after rollout_decode_range.  payload: the WHOLE stream (or None
        after payload_begin / payload_put); out="resident" keeps the frames for decoded_get (sequence indices)."""
        nt, h, w = self._shape
        n = nt * h * w * self.channels
        if payload is not None and _numel(payload) != n:  # decompress.py:240: the reference's reshape raises
            raise ValueError("payload holds %d elements, expected %d" % (_numel(payload), n))
        resident = isinstance(out, str) and out == "resident"
        if resident:
            out = None
        elif out is None:
            out = _RESULTS.empty((int(count), h, w, 3), np.uint8)
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_decode_range(self.h, None if payload is None else _ptr(payload), n, _ptr(tb), tl, int(first),
                                          int(count), _ptr(out)))
        return out

    def encode_quality(self, payload="resident", table=None, shuffle=False):
        """tz_encode_quality after rollout + encode: per frame (sse, max_abs, n_changed) of what the payload decodes to
        against the originals, as a QUALITY_DTYPE record array of nt entries.  payload: "resident" (the payload of
        encode(..., payload="resident")) or a host / device buffer of nt*H*W*3 int16; table: the encode's table (None:
        no remap); shuffle: the payload holds byte planes."""
        nt, h, w = self._shape
        n = nt * h * w * self.channels
        resident = isinstance(payload, str) and payload == "resident"
        if not resident and _numel(payload) != n:
            raise ValueError("payload holds %d elements, expected %d" % (_numel(payload), n))
        out = np.zeros(nt, QUALITY_DTYPE)
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_encode_quality(self.h, None if resident else _ptr(payload), n, _ptr(tb), tl, int(bool(shuffle)),
                                            out.ctypes.data))
        return out

    # ---- the bound for a PSNR target (definition TZ-TPSNR-1: tezip_amd/target.py)
    def bound_probe(self, mode, bound):
        """tz_bound_probe after rollout: the QUALITY_DTYPE records (nt entries) that encode(mode, bound) + encode_quality
        would give, without a payload, in the payload layout in force (set_payload_channels(1): the one-channel job's, and
        a stack with colour is refused as encode refuses it).  Nothing of the context changes."""
        nt, h, w = self._shape
        b0, b1 = _bounds(bound)
        out = np.zeros(nt, QUALITY_DTYPE)
        self._ck(self.lib.tz_bound_probe(self.h, MODES[mode], b0, b1, out.ctypes.data))
        return out

    def bound_err(self, orig, delta, qdelta, nframes, frame_elems):
        """tz_bound_err: k_bound_err over three stacks of nframes x frame_elems elements (uint8, int16, int16; host arrays
        or device tensors): QUALITY_DTYPE[nframes].  After set_payload_channels(1): the one-channel form (target.errors_of
        with channels=1 on gray originals)."""
        n = int(nframes) * int(frame_elems)
        if not (_numel(orig) == _numel(delta) == _numel(qdelta) == n):
            raise ValueError("stacks hold %d, %d and %d elements, expected %d" % (_numel(orig), _numel(delta), _numel(qdelta), n))
        out = np.zeros(max(int(nframes), 0), QUALITY_DTYPE)
        self._ck(self.lib.tz_bound_err(self.h, _ptr(orig), _ptr(delta), _ptr(qdelta), int(nframes), int(frame_elems),
                                       out.ctypes.data))
        return out

    # ---- structural similarity (definition TZ-SSIM-1: tezip_amd/ssim.py)
    def encode_ssim(self, payload="resident", table=None, shuffle=False):
        """tz_encode_ssim after rollout + encode, arguments as encode_quality's: per frame (sum_q32, min_q32, windows,
        reserved) of what the payload decodes to against the originals, as a SSIM_DTYPE record array of nt entries."""
        nt, h, w = self._shape
        n = nt * h * w * self.channels
        resident = isinstance(payload, str) and payload == "resident"
        if not resident and _numel(payload) != n:
            raise ValueError("payload holds %d elements, expected %d" % (_numel(payload), n))
        out = np.zeros(nt, SSIM_DTYPE)
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_encode_ssim(self.h, None if resident else _ptr(payload), n, _ptr(tb), tl, int(bool(shuffle)),
                                         out.ctypes.data))
        return out

    def ssim_frames(self, a, b):
        """tz_ssim_frames of two uint8 stacks (nt, H, W, 3), host arrays or device tensors: SSIM_DTYPE[nt]."""
        if tuple(a.shape) != tuple(b.shape) or len(a.shape) != 4 or a.shape[3] != 3:
            raise ValueError("two stacks of one shape (nt, H, W, 3), got %r and %r" % (tuple(a.shape), tuple(b.shape)))
        nt, h, w = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, np.uint8)
        if isinstance(b, np.ndarray):
            b = np.ascontiguousarray(b, np.uint8)
        out = np.zeros(nt, SSIM_DTYPE)
        self._ck(self.lib.tz_ssim_frames(self.h, _ptr(a), _ptr(b), nt, h, w, out.ctypes.data))
        return out

    # ---- per-frame digests (tz_*_digests; format TZD64: tezip_amd/digest.py)
    def encode_digests(self, payload="resident", table=None, shuffle=False, original=True):
        """tz_encode_digests after rollout + encode, arguments as encode_quality's -> (decoded, original): uint64[nt] each,
        the digests of what the payload decodes to and of the resident source frames (None with original=False)."""
        nt, h, w = self._shape
        n = nt * h * w * self.channels
        resident = isinstance(payload, str) and payload == "resident"
        if not resident and _numel(payload) != n:
            raise ValueError("payload holds %d elements, expected %d" % (_numel(payload), n))
        dec = np.zeros(nt, np.uint64)
        org = np.zeros(nt, np.uint64) if original else None
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_encode_digests(self.h, None if resident else _ptr(payload), n, _ptr(tb), tl, int(bool(shuffle)),
                                            dec.ctypes.data, None if org is None else org.ctypes.data))
        return dec, org

    def frame_digests(self, frames, nframes=None, frame_bytes=None, out=None):
        """tz_frame_digests of a host array or device tensor of uint8: frames[0] is one frame, or give nframes and frame_bytes
        for a flat buffer.  out: uint64 host array or device tensor of int64 (the same 64 bits), default a new host array."""
        if nframes is None:
            nframes = int(frames.shape[0])
            frame_bytes = _numel(frames) // nframes if nframes else 0
        if _numel(frames) != int(nframes) * int(frame_bytes):
            raise ValueError("buffer holds %d bytes, expected %d frames of %d" % (_numel(frames), nframes, frame_bytes))
        if out is None:
            out = np.zeros(int(nframes), np.uint64)
        self._ck(self.lib.tz_frame_digests(self.h, _ptr(frames), int(nframes), int(frame_bytes), _ptr(out)))
        return out

    def decoded_digests(self, first, count):
        """tz_decoded_digests: uint64[count] of the frames decode(..., out="resident") / decode_range(..., out="resident")
        left in the context (sequence indices, as decoded_get)."""
        out = np.zeros(int(count), np.uint64)
        self._ck(self.lib.tz_decoded_digests(self.h, int(first), int(count), out.ctypes.data))
        return out

    # ---- the opt-in coded streams.  Private helpers behind the five families below: `fn` is the library's entry point, `ntok` the
    # repeat tokens behind the literals of `lengths` (the A the library is given is the number of literals), `dist` the match
    # distance where the entry point takes one (tz_huffd_*), `what` names a pred array in a message.
    def _stream_counts(self, fn, fn_buf, x, rows):
        """-> (uint64[rows][A + 8], base) of the resident payload, or of the int16 array x"""
        counts = np.zeros((rows, TZ_NBINS + HUFFR_NTOK), np.uint64)
        a, base = C.c_int(0), C.c_int(0)
        if x is None:
            self._ck(fn(self.h, counts.ctypes.data, C.byref(a), C.byref(base)))
        else:
            self._ck(fn_buf(self.h, _ptr(x), _numel(x), counts.ctypes.data, C.byref(a), C.byref(base)))
        return counts[:, : a.value + HUFFR_NTOK].copy(), base.value

    def _stream_encode(self, fn, lengths, base, ntok, dist=None):
        ln = np.ascontiguousarray(lengths, np.uint8)
        nbytes = C.c_size_t(0)
        self._ck(fn(self.h, ln.ctypes.data, int(ln.size) - ntok, int(base), *_dist(dist), C.byref(nbytes)))
        return int(nbytes.value)

    def _stream_get(self, fn, offset, count, out):
        if out is None:
            out = np.empty(count, np.uint8)
        self._ck(fn(self.h, int(offset), int(count), _ptr(out, np.uint8)))
        return out

    def _stream_begin(self, fn, nbytes, n, lengths, base, run, ntok, dist=None):
        ln = np.ascontiguousarray(lengths, np.uint8)
        self._ck(fn(self.h, int(nbytes), int(n), ln.ctypes.data, int(ln.size) - ntok, int(base), int(run), *_dist(dist)))

    def _stream_put(self, fn, offset, piece):
        self._ck(fn(self.h, int(offset), _numel(piece), _ptr(piece, np.uint8)))

    def _stream_encode_buf(self, fn, x, lengths, base, out, ntok, dist=None):
        ln = np.ascontiguousarray(lengths, np.uint8)
        n = _numel(x)
        if out is None:   # the most a stream can need: 12 bits per element, a pad word per chunk, the index
            out = np.empty(n * 3 // 2 + (n // 16384 + 1) * 8 + (n // 256 + 1) * 2 + 64, np.uint8)
        nbytes = C.c_size_t(0)
        self._ck(fn(self.h, _ptr(x), n, ln.ctypes.data, int(ln.size) - ntok, int(base), *_dist(dist), _ptr(out), _numel(out), C.byref(nbytes)))
        return out[: nbytes.value]

    def _stream_decode_buf(self, fn, stream, n, lengths, base, run, out, ntok, dist=None):
        ln = np.ascontiguousarray(lengths, np.uint8)
        if out is None:
            out = np.empty(n, np.int16)
        self._ck(fn(self.h, _ptr(stream), _numel(stream), int(n), ln.ctypes.data, int(ln.size) - ntok, int(base), int(run), *_dist(dist), _ptr(out)))
        return out

    @staticmethod
    def _key_args(idx, pred, lengths, what):
        ix, pr, ln = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(pred, np.uint8), np.ascontiguousarray(lengths, np.uint8)
        if pr.size != ix.size or ln.size != 256:
            raise ValueError("%d %s for %d key frames, %d code lengths (256 wanted)" % (pr.size, what, ix.size, ln.size))
        return ix, pr, ln

    def _keys_encode(self, fn, idx, pred, lengths, what):
        ix, pr, ln = self._key_args(idx, pred, lengths, what)
        nbytes = C.c_size_t(0)
        self._ck(fn(self.h, ix.ctypes.data, int(ix.size), pr.ctypes.data, ln.ctypes.data, C.byref(nbytes)))
        return int(nbytes.value)

    def _keys_begin(self, fn, nbytes, nt, h, w, idx, pred, lengths, what):
        ix, pr, ln = self._key_args(idx, pred, lengths, what)
        self._ck(fn(self.h, int(nbytes), int(nt), int(h), int(w), ix.ctypes.data, int(ix.size), pr.ctypes.data, ln.ctypes.data))
        self._keys_shape = (int(nt), int(h), int(w))

    def _keys_decode(self, fn):
        self._ck(fn(self.h))
        self._staged = self._shape = self._keys_shape

    # ---- opt-in Huffman coder (tz_huff_*; format: tezip_amd/huff.py)
    def huff_counts(self):
        """Counts of the resident payload -> (uint64[A], base): counts[s] of the value s + base."""
        counts = np.zeros(TZ_NBINS, np.uint64)
        a, base = C.c_int(0), C.c_int(0)
        self._ck(self.lib.tz_huff_counts(self.h, counts.ctypes.data, C.byref(a), C.byref(base)))
        return counts[: a.value].copy(), base.value

    def huff_encode(self, lengths, base):
        """Code the resident payload into the resident stream (index | bits); returns its size in bytes."""
        return self._stream_encode(self.lib.tz_huff_encode, lengths, base, 0)

    def huff_get(self, offset, count, out=None):
        return self._stream_get(self.lib.tz_huff_get, offset, count, out)

    def huff_begin(self, nbytes, n, lengths, base, run=256):
        self._stream_begin(self.lib.tz_huff_begin, nbytes, n, lengths, base, run, 0)

    def huff_put(self, offset, piece):
        self._stream_put(self.lib.tz_huff_put, offset, piece)

    def huff_decode(self):
        self._ck(self.lib.tz_huff_decode(self.h))

    def huff_encode_buf(self, x, lengths, base, out=None):
        """Stand-alone: int16 values (host or device) -> the coded stream (index | bits) as a uint8 array."""
        return self._stream_encode_buf(self.lib.tz_huff_encode_buf, x, lengths, base, out, 0)

    def huff_decode_buf(self, stream, n, lengths, base, run=256, out=None):
        return self._stream_decode_buf(self.lib.tz_huff_decode_buf, stream, n, lengths, base, run, out, 0)

    # ---- opt-in key-frame coder (tz_keys_*; format: tezip_amd/keycoder.py)
    def keys_counts(self, idx):
        """Counts of the residual values of the resident stack's frames `idx` under the four predictors -> uint32[k][4][256]."""
        ix = np.ascontiguousarray(idx, np.int32)
        counts = np.zeros((ix.size, 4, 256), np.uint32)
        self._ck(self.lib.tz_keys_counts(self.h, ix.ctypes.data, int(ix.size), counts.ctypes.data))
        return counts

    def keys_encode(self, idx, pred, lengths):
        """Code the frames `idx` of the resident stack into the resident key stream (index | bits); returns its size."""
        return self._keys_encode(self.lib.tz_keys_encode, idx, pred, lengths, "predictor ids")

    def keys_get(self, offset, count, out=None):
        return self._stream_get(self.lib.tz_keys_get, offset, count, out)

    def keys_begin(self, nbytes, nt, h, w, idx, pred, lengths):
        self._keys_begin(self.lib.tz_keys_begin, nbytes, nt, h, w, idx, pred, lengths, "predictor ids")

    def keys_put(self, offset, piece):
        self._stream_put(self.lib.tz_keys_put, offset, piece)

    def keys_decode(self):
        """-> the context's frame stack, as frames_begin + frames_put of the zero-except-keys stack leave it."""
        self._keys_decode(self.lib.tz_keys_decode)

    @staticmethod
    def _keys_symbols(pred, h, w, gray):
        """The pred array as uint8 and the symbols its frames have: h * w for a GRAY frame where `gray` says the bit counts."""
        pr = np.ascontiguousarray(pred, np.uint8)
        return pr, int(np.where(pr & 4, h * w, h * w * 3).sum()) if gray else int(pr.size) * h * w * 3

    def _keys_residual_buf(self, fn, frames, pred, out, what, gray):
        self._check_stack(frames, "frames")
        k, h, w = (int(v) for v in frames.shape[:3])
        pr, n = self._keys_symbols(pred, h, w, gray)
        if pr.size != k:
            raise ValueError("%d %s for %d frames" % (pr.size, what, k))
        if out is None:
            out = np.empty(n, np.int16)
        elif gray and _numel(out) != n:     # (the TZK1 wrapper never checked the room of `out`, and stays as it was)
            raise ValueError("%d symbols of room, %d wanted" % (_numel(out), n))
        self._ck(fn(self.h, _ptr(frames), k, h, w, pr.ctypes.data, _ptr(out)))
        return out

    def _keys_unresidual_buf(self, fn, sym, pred, h, w, out, gray):
        h, w = int(h), int(w)
        pr, n = self._keys_symbols(pred, h, w, gray)
        k = int(pr.size)
        if _numel(sym) != n:
            raise ValueError("%d symbols for %d frames of %d x %d%s" % (_numel(sym), k, h, w, ", %d wanted" % n if gray else " x 3"))
        if out is None:
            out = np.empty((k, h, w, 3), np.uint8)
        self._ck(fn(self.h, _ptr(sym), k, h, w, pr.ctypes.data, _ptr(out)))
        return out

    def keys_residual_buf(self, frames, pred, out=None):
        """Stand-alone: uint8 (k, H, W, 3) frames (host or device) -> their k * H * W * 3 int16 residual symbols."""
        return self._keys_residual_buf(self.lib.tz_keys_residual_buf, frames, pred, out, "predictor ids", False)

    def keys_unresidual_buf(self, sym, pred, h, w, out=None):
        return self._keys_unresidual_buf(self.lib.tz_keys_unresidual_buf, sym, pred, h, w, out, False)

    # ---- the same with gray key frames stored once (tz_keys_gray, tz_keysg_*; format: tezip_amd/keycoderg.py).  predg: pred
    # bytes, predictor id | 4 for a GRAY frame, which has h * w symbols instead of h * w * 3
    def keys_gray(self, idx):
        """bool[k]: the three channels of frame idx[k] of the resident stack are equal at every pixel."""
        ix = np.ascontiguousarray(idx, np.int32)
        gray = np.zeros(ix.size, np.uint8)
        self._ck(self.lib.tz_keys_gray(self.h, ix.ctypes.data, int(ix.size), gray.ctypes.data))
        return gray.astype(bool)

    def keysg_encode(self, idx, predg, lengths):
        """Code the frames `idx` of the resident stack into the resident key stream (index | bits); returns its size."""
        return self._keys_encode(self.lib.tz_keysg_encode, idx, predg, lengths, "pred bytes")

    def keysg_get(self, offset, count, out=None):
        return self._stream_get(self.lib.tz_keysg_get, offset, count, out)

    def keysg_begin(self, nbytes, nt, h, w, idx, predg, lengths):
        self._keys_begin(self.lib.tz_keysg_begin, nbytes, nt, h, w, idx, predg, lengths, "pred bytes")

    def keysg_put(self, offset, piece):
        self._stream_put(self.lib.tz_keysg_put, offset, piece)

    def keysg_decode(self):
        """-> the context's frame stack, as frames_begin + frames_put of the zero-except-keys stack leave it."""
        self._keys_decode(self.lib.tz_keysg_decode)

    def keysg_residual_buf(self, frames, predg, out=None):
        """Stand-alone: uint8 (k, H, W, 3) frames (host or device) -> their int16 residual symbols, H * W for a GRAY frame."""
        return self._keys_residual_buf(self.lib.tz_keysg_residual_buf, frames, predg, out, "pred bytes", True)

    def keysg_unresidual_buf(self, sym, predg, h, w, out=None):
        return self._keys_unresidual_buf(self.lib.tz_keysg_unresidual_buf, sym, predg, h, w, out, True)

    # ---- opt-in Huffman coder with repeat tokens (tz_huffr_*; format: tezip_amd/huffr.py).  `lengths` holds the A literals
    # and then the 8 tokens.
    def huffr_counts(self, x=None):
        """Token counts of the resident payload (or of the int16 array x) -> (uint64[A + 8], base): the literals s + base,
        then the repeat tokens T_0..T_7."""
        counts, base = self._stream_counts(self.lib.tz_huffr_counts, self.lib.tz_huffr_counts_buf, x, 1)
        return counts[0], base

    def huffr_encode(self, lengths, base):
        """Code the resident payload into the resident stream (index | bits); returns its size in bytes."""
        return self._stream_encode(self.lib.tz_huffr_encode, lengths, base, HUFFR_NTOK)

    def huffr_get(self, offset, count, out=None):
        return self._stream_get(self.lib.tz_huffr_get, offset, count, out)

    def huffr_begin(self, nbytes, n, lengths, base, run=256):
        self._stream_begin(self.lib.tz_huffr_begin, nbytes, n, lengths, base, run, HUFFR_NTOK)

    def huffr_put(self, offset, piece):
        self._stream_put(self.lib.tz_huffr_put, offset, piece)

    def huffr_decode(self):
        self._ck(self.lib.tz_huffr_decode(self.h))

    def huffr_encode_buf(self, x, lengths, base, out=None):
        """Stand-alone: int16 values (host or device) -> the coded stream (index | bits) as a uint8 array."""
        return self._stream_encode_buf(self.lib.tz_huffr_encode_buf, x, lengths, base, out, HUFFR_NTOK)

    def huffr_decode_buf(self, stream, n, lengths, base, run=256, out=None):
        return self._stream_decode_buf(self.lib.tz_huffr_decode_buf, stream, n, lengths, base, run, out, HUFFR_NTOK)

    # ---- opt-in Huffman coder that picks its match distance (tz_huffd_*; format: tezip_amd/huffd.py).  `lengths` holds the A
    # literals and then the 8 tokens for every distance; dist is 0 (no tokens), 1 or 3.
    def huffd_counts(self, x=None):
        """The three token histograms of the resident payload (or of the int16 array x), from one read of it ->
        (uint64[3][A + 8], base): row 0 without tokens, row 1 at match distance 1, row 2 at distance 3."""
        return self._stream_counts(self.lib.tz_huffd_counts, self.lib.tz_huffd_counts_buf, x, 3)

    def huffd_encode(self, lengths, base, dist):
        """Code the resident payload into the resident stream (index | bits) at the match distance dist; returns its size."""
        return self._stream_encode(self.lib.tz_huffd_encode, lengths, base, HUFFR_NTOK, dist)

    def huffd_get(self, offset, count, out=None):
        return self._stream_get(self.lib.tz_huffd_get, offset, count, out)

    def huffd_begin(self, nbytes, n, lengths, base, dist, run=256):
        self._stream_begin(self.lib.tz_huffd_begin, nbytes, n, lengths, base, run, HUFFR_NTOK, dist)

    def huffd_put(self, offset, piece):
        self._stream_put(self.lib.tz_huffd_put, offset, piece)

    def huffd_decode(self):
        self._ck(self.lib.tz_huffd_decode(self.h))

    def huffd_encode_buf(self, x, lengths, base, dist, out=None):
        """Stand-alone: int16 values (host or device) -> the coded stream (index | bits) as a uint8 array."""
        return self._stream_encode_buf(self.lib.tz_huffd_encode_buf, x, lengths, base, out, HUFFR_NTOK, dist)

    def huffd_decode_buf(self, stream, n, lengths, base, dist, run=256, out=None):
        return self._stream_decode_buf(self.lib.tz_huffd_decode_buf, stream, n, lengths, base, run, out, HUFFR_NTOK, dist)

    # ---- the bound for a compression-ratio target (definition TZ-TRATIO-1: tezip_amd/ratetarget.py)
    def size_probe(self, mode, bound, entropy=True, coder="huffd"):
        """tz_size_probe after rollout: one SIZE_DTYPE record of the stream that encode(mode, bound, entropy, payload="resident"),
        <coder>_counts, the choice of the code and <coder>_encode would leave, without a payload, in the payload layout in
        force.  Nothing of the context changes."""
        b0, b1 = _bounds(bound)
        out = np.zeros(1, SIZE_DTYPE)
        self._ck(self.lib.tz_size_probe(self.h, MODES[mode], b0, b1, int(bool(entropy)), SIZE_CODERS[coder], out.ctypes.data))
        return out[0]

    def size_count_buf(self, q, channels=3, stride=1, offset=True):
        """tz_size_count_buf: k_size_count over the int16 stack q (host array or device tensor) read in the layout (channels,
        stride) -> (uint64[3][SIZE_BINS + 8], bad): ratetarget.count_of."""
        counts = np.zeros((3, SIZE_BINS + HUFFR_NTOK), np.uint64)
        bad = C.c_int(0)
        self._ck(self.lib.tz_size_count_buf(self.h, _ptr(q), _numel(q), int(channels), int(stride), int(bool(offset)), counts.ctypes.data,
                                            C.byref(bad)))
        return counts, bool(bad.value)

    def size_bits_buf(self, q, lens, dist, channels=3, stride=1, offset=True):
        """tz_size_bits_buf: k_size_bits over q under the SIZE_BINS + 8 code lengths `lens` (by bin, then the tokens) at the match
        distance dist -> (words, bits, bad): ratetarget.bits_of."""
        ln = np.ascontiguousarray(lens, np.uint8)
        if ln.size != SIZE_BINS + HUFFR_NTOK:
            raise ValueError("%d code lengths, %d + %d wanted" % (ln.size, SIZE_BINS, HUFFR_NTOK))
        words, bits, bad = C.c_ulonglong(0), C.c_ulonglong(0), C.c_int(0)
        self._ck(self.lib.tz_size_bits_buf(self.h, _ptr(q), _numel(q), int(channels), int(stride), int(bool(offset)), ln.ctypes.data,
                                           int(dist), C.byref(words), C.byref(bits), C.byref(bad)))
        return int(words.value), int(bits.value), bool(bad.value)

    # ---- the payload's spatial delta by exact size (definition TZ-SDA1: tezip_amd/sdauto.py)
    def sdelta_probe(self, mode, bound, entropy=True, coder="huffd"):
        """tz_sdelta_probe after rollout: three SIZE_DTYPE records, the streams of the job under the flat (one channel: channel 0
        alone), channel-stride and plane payloads, from ONE quantiser run; n == 0: the layout is no candidate.  The context's
        own delta_stride / delta_plane are neither read nor changed."""
        b0, b1 = _bounds(bound)
        out = np.zeros(3, SIZE_DTYPE)
        self._ck(self.lib.tz_sdelta_probe(self.h, MODES[mode], b0, b1, int(bool(entropy)), SIZE_CODERS[coder], out.ctypes.data))
        return out

    def size_count_plane_buf(self, q, shape, channels=3, offset=True):
        """tz_size_count_plane_buf: k_size_count over the plane symbols (TZ-SD2) of the int16 stack q of `shape` = (nt, H, W) pixels
        of 3 elements, channels 3 or 1 (channel 0 alone) -> (uint64[3][SIZE_BINS + 8], bad): sdauto.count_of_plane."""
        nt, h, w = (int(v) for v in shape)
        if _numel(q) != nt * h * w * 3:
            raise ValueError("q holds %d elements, %d x %d x %d x 3 wanted" % (_numel(q), nt, h, w))
        counts = np.zeros((3, SIZE_BINS + HUFFR_NTOK), np.uint64)
        bad = C.c_int(0)
        self._ck(self.lib.tz_size_count_plane_buf(self.h, _ptr(q), nt, h, w, int(channels), int(bool(offset)), counts.ctypes.data,
                                                  C.byref(bad)))
        return counts, bool(bad.value)

    def size_bits_plane_buf(self, q, shape, lens, dist, channels=3, offset=True):
        """tz_size_bits_plane_buf: k_size_bits over the plane symbols of q -> (words, bits, bad): sdauto.bits_of_plane."""
        nt, h, w = (int(v) for v in shape)
        if _numel(q) != nt * h * w * 3:
            raise ValueError("q holds %d elements, %d x %d x %d x 3 wanted" % (_numel(q), nt, h, w))
        ln = np.ascontiguousarray(lens, np.uint8)
        if ln.size != SIZE_BINS + HUFFR_NTOK:
            raise ValueError("%d code lengths, %d + %d wanted" % (ln.size, SIZE_BINS, HUFFR_NTOK))
        words, bits, bad = C.c_ulonglong(0), C.c_ulonglong(0), C.c_int(0)
        self._ck(self.lib.tz_size_bits_plane_buf(self.h, _ptr(q), nt, h, w, int(channels), int(bool(offset)), ln.ctypes.data, int(dist),
                                                 C.byref(words), C.byref(bits), C.byref(bad)))
        return int(words.value), int(bits.value), bool(bad.value)

    # ---- operator seams
    def delta_encode(self, pred, orig, zero_mask=None, out=None):
        n, h, w = orig.shape[:3]
        if out is None:
            out = np.empty((n, h, w, 3), np.int16)
        zm = None if zero_mask is None else np.ascontiguousarray(zero_mask, np.uint8)
        self._ck(self.lib.tz_delta_encode(self.h, _ptr(pred), _ptr(orig), _ptr(zm), n, h, w, _ptr(out)))
        return out

    def error_bound(self, orig, diff, mode, bound, skip_mask=None):
        n, h, w = orig.shape[:3]
        b0, b1 = _bounds(bound)
        sk = None if skip_mask is None else np.ascontiguousarray(skip_mask, np.uint8)
        self._ck(self.lib.tz_error_bound(self.h, _ptr(orig), _ptr(diff), _ptr(sk), n, h, w, MODES[mode], b0, b1))
        return diff

    def error_bound_frames(self, orig, diff, bounds, skip_mask=None):
        """tz_error_bound_frames: error_bound in abs mode with bounds[f] for frame f (the seam of set_frame_bounds)."""
        n, h, w = orig.shape[:3]
        b = np.ascontiguousarray(bounds, np.float64)
        if b.size != n:
            raise ValueError("%d bounds for %d frames" % (b.size, n))
        sk = None if skip_mask is None else np.ascontiguousarray(skip_mask, np.uint8)
        self._ck(self.lib.tz_error_bound_frames(self.h, _ptr(orig), _ptr(diff), _ptr(sk), n, h, w, b.ctypes.data))
        return diff

    def lattice_bound(self, orig, diff, mode, bound, skip_mask=None):
        """tz_lattice_bound: the lattice quantiser TZ-QL1 per frame and channel, in place (error_bound's arguments)."""
        n, h, w = orig.shape[:3]
        b0, b1 = _bounds(bound)
        sk = None if skip_mask is None else np.ascontiguousarray(skip_mask, np.uint8)
        self._ck(self.lib.tz_lattice_bound(self.h, _ptr(orig), _ptr(diff), _ptr(sk), n, h, w, MODES[mode], b0, b1))
        return diff

    def lattice_bound_frames(self, orig, diff, bounds, skip_mask=None):
        """tz_lattice_bound_frames: lattice_bound in abs mode with bounds[f] for frame f."""
        n, h, w = orig.shape[:3]
        b = np.ascontiguousarray(bounds, np.float64)
        if b.size != n:
            raise ValueError("%d bounds for %d frames" % (b.size, n))
        sk = None if skip_mask is None else np.ascontiguousarray(skip_mask, np.uint8)
        self._ck(self.lib.tz_lattice_bound_frames(self.h, _ptr(orig), _ptr(diff), _ptr(sk), n, h, w, b.ctypes.data))
        return diff

    def error_bound_map(self, diff, bmap, shape, skip_mask=None):
        """tz_error_bound_map: the greedy walk under the H x W uint8 map bmap (TZ-BM1), in place on the int16 stack diff of
        shape = (nframes, H, W) x 3; no originals.  Host arrays or device tensors at any alignment."""
        n, h, w = (int(v) for v in shape)
        if _numel(diff) != n * h * w * 3 or _numel(bmap) != h * w:
            raise ValueError("diff holds %d elements and the map %d, %d x %d x %d x 3 and %d x %d wanted" % (_numel(diff), _numel(bmap), n, h, w, h, w))
        sk = None if skip_mask is None else np.ascontiguousarray(skip_mask, np.uint8)
        self._ck(self.lib.tz_error_bound_map(self.h, _ptr(diff), _ptr(sk), n, h, w, _ptr(bmap)))
        return diff

    def lattice_bound_map(self, diff, bmap, shape, skip_mask=None):
        """tz_lattice_bound_map: TZ-QL1 with e = bmap[pixel], arguments as error_bound_map's."""
        n, h, w = (int(v) for v in shape)
        if _numel(diff) != n * h * w * 3 or _numel(bmap) != h * w:
            raise ValueError("diff holds %d elements and the map %d, %d x %d x %d x 3 and %d x %d wanted" % (_numel(diff), _numel(bmap), n, h, w, h, w))
        sk = None if skip_mask is None else np.ascontiguousarray(skip_mask, np.uint8)
        self._ck(self.lib.tz_lattice_bound_map(self.h, _ptr(diff), _ptr(sk), n, h, w, _ptr(bmap)))
        return diff

    def spatial_delta(self, x, offset, carry=None, hist=None, out=None):
        n = int(np.prod(x.shape))
        if out is None:
            out = np.empty(n, np.int16)
        self._ck(self.lib.tz_spatial_delta(self.h, _ptr(x), n, int(carry is not None), int(carry or 0), int(offset),
                                           _ptr(out), _ptr(hist)))
        return out

    def build_table(self, hist):
        hist = np.ascontiguousarray(hist, np.uint64)
        table = np.zeros(TZ_MAX_TABLE, np.int16)
        tlen = C.c_int(0)
        self._ck(self.lib.tz_build_table(hist.ctypes.data, len(hist), table.ctypes.data, C.byref(tlen)))
        return table[: tlen.value].copy()

    def remap(self, x, table, out=None):
        n = int(np.prod(x.shape))
        if out is None:
            out = np.empty(n, np.int16)
        tb = np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_remap(self.h, _ptr(x), n, tb.ctypes.data, len(tb), _ptr(out)))
        return out

    def unmap(self, x, table, offset=True, out=None):
        n = int(np.prod(x.shape))
        if out is None:
            out = np.empty(n, np.int16)
        tb = np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_unmap(self.h, _ptr(x), n, tb.ctypes.data, len(tb), int(offset), _ptr(out)))
        return out

    def undelta_carry(self, payload, n0, table=None, staged=False):
        """tz_undelta_carry: the decoded element in front of payload[n0] (table None: no remap).  staged=True: the payload
        staged with payload_begin / payload_put."""
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        c = C.c_int16(0)
        self._ck(self.lib.tz_undelta_carry(self.h, None if staged else _ptr(payload), int(n0), _ptr(tb), tl, C.byref(c)))
        return int(c.value)

    def spatial_undelta(self, x, carry=None, out=None):
        n = int(np.prod(x.shape))
        if out is None:
            out = np.empty(n, np.int16)
        self._ck(self.lib.tz_spatial_undelta(self.h, _ptr(x), n, int(carry is not None), int(carry or 0), _ptr(out)))
        return out

    def spatial_delta_stride(self, x, stride, offset, carry=None, hist=None, out=None):
        """tz_spatial_delta_stride: out[i] = x[i - stride] - x[i] (tezip_amd/sdelta.py); carry: None or `stride` elements."""
        n = _numel(x)
        if out is None:
            out = np.empty(n, np.int16)
        cy = None if carry is None else _carry(carry, stride)
        self._ck(self.lib.tz_spatial_delta_stride(self.h, _ptr(x), n, int(stride), _ptr(cy), int(offset), _ptr(out), _ptr(hist)))
        return out

    def spatial_undelta_stride(self, x, stride, carry=None, out=None):
        """tz_spatial_undelta_stride: the inverse, x[i] = x[i - stride] - s[i]."""
        n = _numel(x)
        if out is None:
            out = np.empty(n, np.int16)
        cy = None if carry is None else _carry(carry, stride)
        self._ck(self.lib.tz_spatial_undelta_stride(self.h, _ptr(x), n, int(stride), _ptr(cy), _ptr(out)))
        return out

    def spatial_delta_plane(self, x, shape, offset, hist=None, out=None):
        """tz_spatial_delta_plane: TZ-SD2 (tezip_amd/sdelta.py encode_plane) of the int16 stack x of `shape` = (nt, H, W, C),
        host or device."""
        nt, h, w, c = (int(v) for v in shape)
        if out is None:
            out = np.empty(nt * h * w * c, np.int16)
        self._ck(self.lib.tz_spatial_delta_plane(self.h, _ptr(x), nt, h, w, c, int(offset), _ptr(out), _ptr(hist)))
        return out

    def spatial_undelta_plane(self, x, shape, table=None, out=None):
        """tz_spatial_undelta_plane: the inverse; table None: x holds the spatial delta as stored, else ranks under the table
        (with the 1600 offset)."""
        nt, h, w, c = (int(v) for v in shape)
        if out is None:
            out = np.empty(nt * h * w * c, np.int16)
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        self._ck(self.lib.tz_spatial_undelta_plane(self.h, _ptr(x), nt, h, w, c, _ptr(tb), tl, _ptr(out)))
        return out

    def undelta_carry_stride(self, payload, n0, stride, table=None, staged=False):
        """tz_undelta_carry_stride: the `stride` decoded elements in front of payload[n0] (n0 a positive multiple of stride)."""
        tl = -1 if table is None else len(table)
        tb = None if table is None else np.ascontiguousarray(table, np.int16)
        c = np.zeros(max(int(stride), 1), np.int16)
        self._ck(self.lib.tz_undelta_carry_stride(self.h, None if staged else _ptr(payload), int(n0), int(stride), _ptr(tb), tl,
                                                  c.ctypes.data))
        return c

    def spatial_delta_gray(self, x3, offset, carry=None, hist=None, out=None):
        """tz_spatial_delta_gray: spatial_delta over channel 0 of the interleaved int16 stack x3 (npix * 3 elements, host or
        device) -> npix elements."""
        npix = _numel(x3) // 3
        if _numel(x3) != npix * 3:
            raise ValueError("%d elements are not whole 3-channel pixels" % _numel(x3))
        if out is None:
            out = np.empty(npix, np.int16)
        self._ck(self.lib.tz_spatial_delta_gray(self.h, _ptr(x3), npix, int(carry is not None), int(carry or 0), int(offset),
                                                _ptr(out), _ptr(hist)))
        return out

    def reconstruct_gray(self, pred, key_frames, key_mask, diff1, out=None):
        """tz_reconstruct_gray: diff1 (n, H, W) holds one int16 delta per pixel; -> (n, H, W, 3) uint8, three equal channels."""
        n, h, w = diff1.shape[:3]
        if out is None:
            out = np.empty((n, h, w, 3), np.uint8)
        km = None if key_mask is None else np.ascontiguousarray(key_mask, np.uint8)
        self._ck(self.lib.tz_reconstruct_gray(self.h, _ptr(pred), _ptr(key_frames), _ptr(km), _ptr(diff1), n, h, w, _ptr(out)))
        return out

    def reconstruct(self, pred, key_frames, key_mask, diff, out=None):
        n, h, w = diff.shape[:3]
        if out is None:
            out = np.empty((n, h, w, 3), np.uint8)
        km = None if key_mask is None else np.ascontiguousarray(key_mask, np.uint8)
        self._ck(self.lib.tz_reconstruct(self.h, _ptr(pred), _ptr(key_frames), _ptr(km), _ptr(diff), n, h, w, _ptr(out)))
        return out

    def window_sse(self, orig, pred):
        n, h, w = orig.shape[:3]
        sse = np.zeros(n, np.float64)
        self._ck(self.lib.tz_window_sse(self.h, _ptr(orig), _ptr(pred), n, h, w, sse.ctypes.data))
        return sse

    # ---- timing
    def timer_start(self):
        self._ck(self.lib.tz_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float(0)
        self._ck(self.lib.tz_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def prof_enable(self, on=True):
        self._ck(self.lib.tz_prof_enable(self.h, int(on)))

    def prof_reset(self):
        self._ck(self.lib.tz_prof_reset(self.h))

    def prof_get(self):
        out = {}
        for i in range(self.lib.tz_prof_count()):
            ms, n = C.c_double(0), C.c_longlong(0)
            self._ck(self.lib.tz_prof_get(self.h, i, C.byref(ms), C.byref(n)))
            out[self.lib.tz_prof_name(i).decode()] = (ms.value, n.value)
        return out
