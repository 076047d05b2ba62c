"""ctypes binding of librvc_amd.so (include/rvc_amd.h) for torch tensors.

The library is the product: there is no CPU or PyTorch fallback.  If the shared object is
missing this module raises at import, and every wrapper raises ``NativeError`` with the
library's own message when a call fails.  Tensors are passed as raw device pointers
(``tensor.data_ptr()``).  A native call runs on the device of its tensors and on that device's current HIP stream:
``_call`` makes the device current for the call when it is not, so the caller no longer has to.  The tensors of
one call share a device, and a ``Decoder`` or ``MelTransform`` handle belongs to the device it was built for.
"""
from __future__ import annotations

import ctypes
import threading
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "librvc_amd.so")
# The ablation build (same sources with -DRVC_ABLATE: the RVC_* tuning switches and the kernels that leave work out) is only
# ever loaded when RVC_AMD_LIB names it -- tools/ablate_*.sh and the F(4,3) test's child process do.
if os.environ.get("RVC_AMD_LIB"):
    LIB_PATH = os.path.abspath(os.environ["RVC_AMD_LIB"])
    print(f"[rvc_amd] RVC_AMD_LIB: loading {LIB_PATH} instead of the product library", flush=True)


class NativeError(RuntimeError):
    pass


if not os.path.isfile(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950).  rvc_amd has no fallback path without its HIP library.")

_lib = ctypes.CDLL(LIB_PATH)


class DecoderConfig(ctypes.Structure):
    _fields_ = [
        ("kind", c_int), ("sample_rate", c_int), ("in_channels", c_int), ("upsample_initial_channel", c_int),
        ("gin_channels", c_int), ("n_ups", c_int), ("upsample_rates", c_int * 8), ("upsample_kernel_sizes", c_int * 8),
        ("n_res_kernels", c_int), ("res_kernel_sizes", c_int * 4), ("res_dilations", c_int * 4),
        ("n_res_dilations", c_int), ("weight_storage", c_int),
    ]


class DecoderNoise(ctypes.Structure):
    _fields_ = [("src_rand_dev", c_void_p), ("src_randn_dev", c_void_p), ("adain_randn_dev", c_void_p)]


# every symbol include/rvc_amd.h declares: (restype, argtypes)
SYMBOLS = {
    "rvc_abi_version": (c_int, []),
    "rvc_last_error": (c_char_p, []),
    "rvc_knn_index_aux_bytes": (c_int, [c_int64, c_int, POINTER(c_size_t)]),
    "rvc_knn_index_build": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_size_t, c_void_p]),
    "rvc_knn_set_mode": (c_int, [c_int]),
    "rvc_knn_rank_candidates": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p,
                                        c_void_p, c_void_p]),
    "rvc_knn_workspace_bytes": (c_int, [c_int64, c_int64, c_int, c_int, POINTER(c_size_t)]),
    "rvc_knn_search": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                               c_void_p, c_size_t, c_void_p]),
    "rvc_knn_blend": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p,
                              c_void_p]),
    "rvc_logmel_workspace_bytes": (c_int, [c_int, c_int64, POINTER(c_size_t)]),
    "rvc_logmel_rmvpe": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p, c_size_t, c_void_p]),
    "rvc_mel_create": (c_int, [c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_int, POINTER(c_void_p)]),
    "rvc_mel_destroy": (c_int, [c_void_p]),
    "rvc_mel_frames": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "rvc_mel_workspace_bytes": (c_int, [c_void_p, c_int, c_int64, POINTER(c_size_t)]),
    "rvc_mel_forward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_resample_poly_f64": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "rvc_filtfilt_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "rvc_filtfilt_order5": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_filtfilt_order5_terms": (c_int, [c_void_p, POINTER(c_int64)]),
    "rvc_bigru_workspace_bytes": (c_int, [c_int, POINTER(c_size_t)]),
    "rvc_bigru_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_size_t,
                                  c_void_p]),
    "rvc_bigru_status": (c_int, [c_void_p, c_int, POINTER(c_int), c_void_p]),
    "rvc_bigru_set_spin_limit": (c_int, [ctypes.c_uint]),
    "rvc_attention_workspace_bytes": (c_int, [c_int, c_int64, c_int, c_int, POINTER(c_size_t)]),
    "rvc_attention_qkv_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_float,
                                      c_void_p, c_size_t, c_void_p]),
    "rvc_bias_relu_add_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p]),
    "rvc_gate_tanh_sigmoid_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p]),
    "rvc_rownorm_gelu_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, ctypes.c_float, c_void_p]),
    "rvc_set_concurrency_hint": (c_int, [c_int]),
    "rvc_decoder_create": (c_int, [POINTER(DecoderConfig), POINTER(c_void_p)]),
    "rvc_decoder_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    "rvc_decoder_finalize": (c_int, [c_void_p]),
    "rvc_decoder_destroy": (c_int, [c_void_p]),
    "rvc_decoder_upp": (c_int, [c_void_p]),
    "rvc_decoder_workspace_bytes": (c_int, [c_void_p, c_int, c_int64, POINTER(c_size_t)]),
    "rvc_decoder_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(DecoderNoise), c_int, c_int64,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_decoder_window_margin": (c_int, [POINTER(DecoderConfig), POINTER(c_int)]),
    "rvc_decoder_forward_window": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(DecoderNoise), c_int, c_int64, c_int64,
                                           c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_decoder_set_tap": (c_int, [c_void_p, c_int, c_void_p]),
    "rvc_decoder_set_concurrency_hint": (c_int, [c_void_p, c_int]),
    "rvc_decoder_set_branch_parallel": (c_int, [c_void_p, c_int]),
    "rvc_posconv_bf16x3_weight_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "rvc_posconv_bf16x3_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_posconv_gelu_bf16x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "rvc_hubert_conv0_workspace_bytes": (c_int, [c_int, POINTER(c_size_t)]),
    "rvc_hubert_conv0_frames_bf16x3": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                               c_size_t, c_void_p, c_int64, c_void_p]),
    "rvc_conv1d_frames_bf16x3": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_int, c_int, c_void_p]),
    "rvc_conv1d_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_conv1d_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_int64, c_int, c_int, c_float, c_float, c_void_p]),
    "rvc_conv1d_wino_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_conv1d_wino_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                        c_int64, c_int, c_int, c_float, c_float, c_void_p]),
    "rvc_conv1d_winobf_weight_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "rvc_conv1d_winobf_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_conv1d_winobf_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_int64, c_int, c_int, c_float, c_float, c_void_p]),
    "rvc_resblock_bf16x3_weight_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "rvc_resblock_bf16x3_pack_weight": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rvc_resblock_bf16x3_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int,
                                            c_int, c_float, c_float, c_void_p]),
    "rvc_resblock_bf16w_weight_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "rvc_resblock_bf16w_pack_weight": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rvc_resblock_bf16w_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int,
                                           c_int, c_float, c_float, c_void_p]),
    "rvc_resblock_bf16x3_set_enabled": (c_int, [c_int]),
    "rvc_upsample_bf16x3_weight_bytes": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "rvc_upsample_bf16x3_pack_weight": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_upsample_bf16x3_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int,
                                            c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "rvc_conv1d_f16x2_weight_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "rvc_conv1d_f16x2_pack_weight": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rvc_conv1d_f16x2_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int,
                                         c_int, c_float, c_float, c_void_p]),
    "rvc_decoder_set_arithmetic": (c_int, [c_void_p, c_int]),
    "rvc_conv1d_bf16w_weight_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "rvc_conv1d_bf16w_pack_weight": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rvc_conv1d_bf16w_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int,
                                         c_int, c_float, c_float, c_void_p]),
    "rvc_gemm_bf16x3_weight_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "rvc_gemm_bf16x3_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_linear_bf16x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "rvc_conv1d_bf16x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int, c_int, c_int,
                                  c_void_p]),
    "rvc_split_rows_bf16x3": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "rvc_linear_bf16x3_presplit": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                           c_void_p]),
    "rvc_bias_residual_layernorm_bf16x3": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                                   c_int64, c_int64, c_int, c_void_p]),
    "rvc_conv2d_packed_floats": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "rvc_conv2d_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_conv2d_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "rvc_conv2d_bf16x3_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "rvc_conv2d_bf16x3_weight_bytes": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "rvc_conv2d_bf16x3_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rvc_conv2d_bf16x3_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "rvc_conv2d_bf16x3_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_void_p, c_size_t, c_void_p]),
    "rvc_conv2d_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rvc_comm_unique_id": (c_int, [c_void_p]),
    "rvc_comm_create": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "rvc_comm_destroy": (c_int, [c_void_p]),
    "rvc_comm_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), c_char_p, c_size_t]),
    "rvc_index_broadcast": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "rvc_checksum64": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    "rvc_glu_dwconv_silu_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "rvc_layernorm_rows_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int, c_void_p]),
    "rvc_groupnorm_workspace_bytes": (c_int, [c_int, c_int64, c_int, POINTER(c_size_t)]),
    "rvc_groupnorm_lrelu_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_int, c_int64, c_void_p,
                                        c_size_t, c_void_p]),
    "rvc_fcpe_decode_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "rvc_kmeans_workspace_bytes": (c_int, [c_int64, c_int64, c_int, POINTER(c_size_t)]),
    "rvc_kmeans_assign": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_kmeans_update": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "rvc_lfilter_order5_warmup": (c_int, [c_void_p, POINTER(c_int64)]),
    "rvc_lfilter_order5_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "rvc_frame_rms_frames": (c_int, [c_int64, c_int64, c_int64, POINTER(c_int64), POINTER(c_size_t)]),
    "rvc_frame_rms_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_size_t, c_void_p]),
    "rvc_slice_export_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p,
                                     c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "rvc_spectral_gate_params": (c_int, [c_int, POINTER(c_int), POINTER(c_int), POINTER(ctypes.c_double), c_void_p, c_void_p]),
    "rvc_spectral_gate_workspace_bytes": (c_int, [c_int64, c_int, c_int64, c_int64, POINTER(c_size_t)]),
    "rvc_spectral_gate_f32": (c_int, [c_void_p, c_int64, c_int, c_float, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_formant_shift_workspace_bytes": (c_int, [c_int64, c_int, POINTER(c_size_t)]),
    "rvc_formant_shift_f32": (c_int, [c_void_p, c_int64, c_int, ctypes.c_double, ctypes.c_double, c_int, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "rvc_mrstft_sums_workspace_bytes": (c_int, [c_int64, POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, POINTER(c_size_t)]),
    "rvc_mrstft_sums_f32": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, ctypes.c_double,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_si_sdr_sums_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "rvc_si_sdr_sums_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_mean_abs_diff_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "rvc_mean_abs_diff_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_sola_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "rvc_sola_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                             c_void_p]),
    "rvc_stream_window_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "rvc_fx_pointwise_f32": (c_int, [c_void_p, c_int64, c_int, c_double, c_double, c_double, c_double, c_void_p, c_void_p]),
    "rvc_fx_delay_f32": (c_int, [c_void_p, c_int64, c_int, c_double, c_double, c_double, c_void_p, c_void_p]),
    "rvc_fx_chorus_workspace_bytes": (c_int, [c_int64, c_double, POINTER(c_size_t)]),
    "rvc_fx_chorus_f32": (c_int, [c_void_p, c_int64, c_int, c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "rvc_fx_reverb_params": (c_int, [c_int, POINTER(c_int), POINTER(c_int)]),
    "rvc_fx_reverb_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "rvc_fx_reverb_f32": (c_int, [c_void_p, c_int64, c_int, c_double, c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "rvc_fx_ballistics": (c_int, [c_int, c_double, c_double, POINTER(c_double), POINTER(c_double)]),
    "rvc_fx_compressor_workspace_bytes": (c_int, [c_int64, c_int64, c_int, POINTER(c_size_t)]),
    "rvc_fx_compressor_f32": (c_int, [c_void_p, c_int64, c_int, c_double, c_double, c_double, c_double, c_int64, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "rvc_fx_limiter_f32": (c_int, [c_void_p, c_int64, c_int, c_double, c_double, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_spectral_features_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "rvc_spectral_features_f32": (c_int, [c_void_p, c_int64, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_size_t, c_void_p]),
    "rvc_melcep_workspace_bytes": (c_int, [c_int64, c_int, POINTER(c_size_t)]),
    "rvc_melcep_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_dtw_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "rvc_dtw_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rvc_frame_dist_sum_f64": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "rvc_f0_track_sums_f64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
}

for _name, (_res, _args) in SYMBOLS.items():
    _fn = getattr(_lib, _name)  # AttributeError here = the .so is stale
    _fn.restype = _res
    _fn.argtypes = _args

ABI_VERSION = 4
if _lib.rvc_abi_version() != ABI_VERSION:
    raise ImportError(f"librvc_amd.so ABI {_lib.rvc_abi_version()} != {ABI_VERSION}: rebuild it")


def _check(rc: int, what: str):
    if rc != 0:
        raise NativeError(f"{what}: {_lib.rvc_last_error().decode(errors='replace')}")


def _stream() -> int:
    """The current device's current stream, for code that calls `_lib` directly (the wrappers below go through `_call`)."""
    return torch.cuda.current_stream().cuda_stream


def _call(name: str, device: torch.device, *args, stream: bool = True) -> None:
    """The one path into every entry point that launches on, or sizes for, a device.  The library looks its per-device resources up
    by hipGetDevice (csrc/common.h), so `device` is made current for the call when it is not already; `device`'s current stream is
    appended as the trailing `void *stream` argument (stream=False: a size query, which takes none); a non-zero return raises
    NativeError with the library's message.  The device already being current, the common case, costs one index compare."""
    if device.index != torch.cuda.current_device():
        if device.type != "cuda" or device.index is None:
            raise NativeError(f"{name}: every tensor must live in HBM, got one on {device}")
        with torch.cuda.device(device):
            return _call(name, device, *args, stream=stream)
    if stream:
        args += (torch.cuda.current_stream(device.index).cuda_stream,)
    _check(getattr(_lib, name)(*args), name)


def _device(*tensors) -> torch.device:
    """The one device of a call's tensor arguments (None: an optional one that is absent)."""
    device = None
    for t in tensors:
        if t is None:
            continue
        if device is None:
            device = t.device
        elif t.device != device:
            raise NativeError(f"the tensors of one call must share a device, got {device} and {t.device}")
    return device


def _cuda_device(device=None) -> torch.device:
    """`device` with its index spelled out; None or a bare "cuda" is the current device."""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise NativeError(f"a HIP device is needed, got {device} (no CPU fallback)")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    """The address of an optional tensor: NULL when it is absent."""
    return t.data_ptr() if t is not None else None


def _host(w: torch.Tensor) -> torch.Tensor:
    """A weight as the contiguous fp32 host tensor the *_pack_weight / set_tensor entry points read."""
    return w.detach().float().cpu().contiguous()


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise NativeError(f"{name} must live in HBM (got a {t.device} tensor); the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise NativeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


class _Workspace:
    """Grow-only scratch buffer per (tag, device, stream) so steady-state calls allocate nothing.  Keyed by the current
    stream as well: utterances that are in flight on different streams must not share scratch memory."""

    def __init__(self):
        self._buf = {}
        self._lock = threading.Lock()

    def get(self, tag: str, nbytes: int, device) -> torch.Tensor:
        key = (tag, str(device), torch.cuda.current_stream(device).cuda_stream)
        with self._lock:
            buf = self._buf.get(key)
            if buf is None or buf.numel() < nbytes:
                buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
                self._buf[key] = buf
        return buf


_ws = _Workspace()


def _size(query: str, device, *dims) -> int:
    """What the size query `query`(*dims, &bytes) answers on `device` (some depend on its CU count)."""
    need = c_size_t()
    _call(query, device, *dims, ctypes.byref(need), stream=False)
    return need.value


def _workspace(tag: str, device, query: str, *dims) -> torch.Tensor:
    """The scratch buffer of (tag, device, device's current stream), at least as large as `query`(*dims) asks for."""
    return _ws.get(tag, _size(query, device, *dims), device)


def _pack_slab(stem: str, device, host: tuple, size_dims: tuple, pack_dims: tuple = None) -> torch.Tensor:
    """<stem>_weight_bytes(*size_dims) -> an int16 slab of that size on `device` -> <stem>_pack_weight(*host tensors, *pack_dims,
    slab): the host weights (None: an absent one) repacked into the fragment layout a kernel family reads."""
    device = _cuda_device(device)
    slab = torch.empty(_size(stem + "_weight_bytes", device, *size_dims) // 2, dtype=torch.int16, device=device)
    _call(stem + "_pack_weight", device, *(_ptr(w) for w in host), *(size_dims if pack_dims is None else pack_dims), slab.data_ptr())
    return slab


# ---- K1 ------------------------------------------------------------------------------------------
def knn_index_build(index: torch.Tensor) -> torch.Tensor:
    """The per-index aux blob of rvc_knn_index_build (||x||^2, fp16 copy, screening statistics) as an opaque uint8 tensor."""
    index = _dev_f32(index, "index")
    n, d = index.shape[0], index.shape[1]
    aux = torch.empty(_size("rvc_knn_index_aux_bytes", index.device, n, d), dtype=torch.uint8, device=index.device)
    _call("rvc_knn_index_build", index.device, index.data_ptr(), n, d, aux.data_ptr(), aux.numel())
    return aux


knn_index_norms = knn_index_build   # round-1 name: the blob starts with the row norms


def knn_set_mode(mode: int) -> None:
    """0 auto, 1 exact fp32 regimes only, 2 fp16-screened whenever the shape allows (test hook; results do not change)."""
    _check(_lib.rvc_knn_set_mode(int(mode)), "rvc_knn_set_mode")


def knn_search(index: torch.Tensor, aux: torch.Tensor, queries: torch.Tensor, k: int = 8):
    index, queries = _dev_f32(index, "index"), _dev_f32(queries, "queries")
    if not aux.is_cuda or aux.dtype != torch.uint8:
        raise NativeError("aux must be the uint8 HBM blob returned by knn_index_build")
    dev = _device(index, aux, queries)
    nq = queries.shape[0]
    d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    if nq == 0:
        return d2, ids
    ws = _workspace("knn", dev, "rvc_knn_workspace_bytes", index.shape[0], nq, index.shape[1], k)
    _call("rvc_knn_search", dev, index.data_ptr(), aux.data_ptr(), index.shape[0], index.shape[1], queries.data_ptr(), nq, k,
          d2.data_ptr(), ids.data_ptr(), ws.data_ptr(), ws.numel())
    return d2, ids


def knn_rank_candidates(index: torch.Tensor, aux: torch.Tensor, queries: torch.Tensor, cand: torch.Tensor, k: int = 8):
    """Exact top-k among the candidate rows cand [Q, cap] (int32, negative = empty) of each query."""
    index, queries = _dev_f32(index, "index"), _dev_f32(queries, "queries")
    if not cand.is_cuda or cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != queries.shape[0]:
        raise NativeError("cand must be an int32 HBM tensor [n_queries, cap]")
    cand = cand.contiguous()
    dev = _device(index, aux, queries, cand)
    nq = queries.shape[0]
    d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    _call("rvc_knn_rank_candidates", dev, index.data_ptr(), aux.data_ptr(), index.shape[0], index.shape[1], queries.data_ptr(), nq,
          cand.data_ptr(), cand.shape[1], k, d2.data_ptr(), ids.data_ptr())
    return d2, ids


def knn_blend(index: torch.Tensor, feats: torch.Tensor, d2: torch.Tensor, ids: torch.Tensor, index_rate: float):
    index, feats, d2 = _dev_f32(index, "index"), _dev_f32(feats, "feats"), _dev_f32(d2, "d2")
    ids = ids.contiguous()
    out = torch.empty_like(feats)
    _call("rvc_knn_blend", _device(index, feats, d2, ids), index.data_ptr(), index.shape[1], feats.data_ptr(), d2.data_ptr(),
          ids.data_ptr(), feats.shape[0], d2.shape[1], float(index_rate), out.data_ptr())
    return out


# ---- K16 -----------------------------------------------------------------------------------------
def kmeans_assign(x: torch.Tensor, centroids: torch.Tensor):
    """-> (ids int32 [n], d2 float32 [n]): the nearest centroid of every row of x and its squared distance (rvc_kmeans_assign)."""
    x, centroids = _dev_f32(x, "x"), _dev_f32(centroids, "centroids")
    if x.dim() != 2 or centroids.dim() != 2 or x.shape[1] != centroids.shape[1]:
        raise NativeError(f"x {tuple(x.shape)} and centroids {tuple(centroids.shape)} must be [n, d] and [k, d]")
    dev = _device(x, centroids)
    n, d = x.shape
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return ids, d2
    ws = _workspace("kmeans", dev, "rvc_kmeans_workspace_bytes", n, centroids.shape[0], d)
    _call("rvc_kmeans_assign", dev, x.data_ptr(), n, d, centroids.data_ptr(), centroids.shape[0], ids.data_ptr(), d2.data_ptr(),
          ws.data_ptr(), ws.numel())
    return ids, d2


def kmeans_update(x: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, old: torch.Tensor) -> torch.Tensor:
    """Centroid j <- the mean of rows order[offsets[j] : offsets[j + 1]] of x (float64 sums), or old[j] when it has no member
    (rvc_kmeans_update).  order: int32 [n], offsets: int64 [k + 1]."""
    x, old = _dev_f32(x, "x"), _dev_f32(old, "old")
    n, d = x.shape
    k = old.shape[0]
    if (not order.is_cuda or order.dtype != torch.int32 or order.numel() != n or not offsets.is_cuda
            or offsets.dtype != torch.int64 or offsets.numel() != k + 1 or old.shape[1] != d):
        raise NativeError("order must be an int32 HBM tensor [n], offsets an int64 HBM tensor [k + 1], old [k, d]")
    if n == 0:
        return old.clone()
    order, offsets = order.contiguous(), offsets.contiguous()
    dev = _device(x, order, offsets, old)
    out = torch.empty_like(old)
    ws = _workspace("kmeans", dev, "rvc_kmeans_workspace_bytes", n, k, d)
    _call("rvc_kmeans_update", dev, x.data_ptr(), n, d, order.data_ptr(), offsets.data_ptr(), k, old.data_ptr(), out.data_ptr(),
          ws.data_ptr(), ws.numel())
    return out


def knn_roofline_report(n_rows: int, n_queries: int, dim: int, seconds: float, peak_hbm_gbs: float,
                        peak_f32_tflops: float, peak_f16_tflops: float, traffic=None, traffic_source=None) -> dict:
    """SURVEY §8d's kNN roofline for one rvc_knn_search of (n_queries x n_rows) that took `seconds` (all launches of the
    search: query conversion, sample pass, bound, main pass, exact re-scoring).  §8d prices a pass over the index at
    n_rows * dim * 4 B (the fp32 rows the reference's algorithm reads) times ceil(Q / Qt) passes; the screened regime
    (Qt = 256) streams an fp16 copy, so the bytes it really moves per pass are half of that.  Since round 6 `frac` is the fraction of
    whatever BOUNDS the regime (see below); `hbm_frac_physical` and `frac_8d` carry the two HBM readings in every regime."""
    screened = n_queries > 64 and n_rows >= 16384 and dim % 256 == 0
    stream = n_queries <= 64
    q_tile = 256 if screened else (32 if stream else 128)
    passes = -(-n_queries // q_tile)
    bytes_8d = passes * n_rows * dim * 4.0
    bytes_moved = passes * n_rows * dim * (2.0 if screened else 4.0) + (8.0 * n_queries * dim * 4 if screened else 0.0)
    flops = 2.0 * n_queries * n_rows * dim
    mfma_peak = peak_f16_tflops if screened else peak_f32_tflops
    hbm_gbs = bytes_moved / seconds / 1e9
    mfma_tf = flops / seconds / 1e12
    # What bounds each regime decides which fraction is `frac`: the streaming regime (<= 64 queries, ONE pass over the fp32 rows) is
    # HBM-bound -- bytes / time / 8 TB/s; the screened regime (a 256 x 256 GEMM tile per block on the fp16 matrix cores, the index
    # mostly served from L2 / MALL) is bound by the matrix pipe's operand ingest -- its `frac` is the fp16 MFMA fraction, and the
    # HBM figures (physical bytes, and SURVEY 8d's formula on fp32 rows the kernel never reads) are footnotes.
    bound = "hbm" if stream else "mfma"
    out = {"kernel": ("knn_screen_kernel<false> (sample) + knn_select_kernel + knn_screen_kernel<true> (main, fp16 MFMA) + "
                      "knn_finalize_kernel (exact fp32 re-scoring)" if screened else
                      ("knn_direct_kernel" if stream else "knn_partial_kernel") + " + knn_finalize_kernel"),
           "regime": "fp16-screened, exact re-scoring" if screened else ("fp32 streaming" if stream else "fp32 GEMM"),
           "shape": f"{n_queries} queries x {n_rows} rows x {dim}", "bound": bound, "query_tile": q_tile, "passes": passes,
           "bytes_per_pass_8d": n_rows * dim * 4}
    if bound == "hbm":
        out.update({"achieved": round(hbm_gbs, 1), "peak": peak_hbm_gbs, "unit": "GB/s", "frac": round(hbm_gbs / peak_hbm_gbs, 4),
                    "frac_is": "physical: bytes the pass reads (n_rows x dim x 4) / search time / HBM peak"})
    else:
        out.update({"achieved": round(mfma_tf, 2), "peak": mfma_peak, "unit": "TFLOP/s", "frac": round(mfma_tf / mfma_peak, 4),
                    "frac_is": "2 x queries x rows x dim / search time / the dense " + ("fp16" if screened else "fp32") + " MFMA peak "
                               "(round 5 and earlier printed an HBM fraction here: now hbm_frac_physical / frac_8d)"})
    out.update({"bytes_moved_per_search": bytes_moved,
                "hbm_gbs_physical": round(hbm_gbs, 1), "hbm_frac_physical": round(hbm_gbs / peak_hbm_gbs, 4),
                "achieved_8d": round(bytes_8d / seconds / 1e9, 1), "frac_8d": round(bytes_8d / seconds / 1e9 / peak_hbm_gbs, 4),
                "frac_8d_is": "SURVEY 8d's formula (passes x n_rows x dim x 4 B / t / 8 TB/s): fp32 bytes the screened kernel never reads -- a footnote",
                "traffic": traffic, "traffic_source": traffic_source,   # measured HBM bytes per search (the caller's: profiles/pmc_knn_*.json)
                "mfma_tflops": round(mfma_tf, 2), "mfma_frac": round(mfma_tf / mfma_peak, 4),
                "mfma_peak_used": "fp16 dense 2500 TF" if screened else "fp32 157.3 TF",
                "avg_search_ms": round(seconds * 1e3, 4)})
    return out


# ---- K4 ------------------------------------------------------------------------------------------
def logmel_rmvpe(audio: torch.Tensor, pad_to: int = 32) -> tuple[torch.Tensor, int]:
    """audio [B, n] -> (log-mel [B, 128, T_padded], T) with the frame axis reflect-padded to a multiple of pad_to."""
    audio = _dev_f32(audio, "audio")
    b, n = audio.shape
    t = n // 160 + 1
    t_pad = pad_to * ((t - 1) // pad_to + 1) if pad_to > 1 else t
    mel = torch.empty((b, 128, t_pad), dtype=torch.float32, device=audio.device)
    ws = _workspace("logmel", audio.device, "rvc_logmel_workspace_bytes", b, n)
    _call("rvc_logmel_rmvpe", audio.device, audio.data_ptr(), b, n, mel.data_ptr(), t_pad, ws.data_ptr(), ws.numel())
    return mel, t


class MelTransform:
    """Handle on rvc_mel_*: STFT magnitude / log-mel for any (n_fft, hop, window, pad, mel matrix) on one device."""

    def __init__(self, n_fft: int, hop: int, win_length: int, pad: int, mel_matrix, mag_eps: float = 0.0, log_floor: float = 1e-5,
                 device=None):
        """device: where the handle's tables live and its forwards run (None: the current device)."""
        import numpy as np
        m = np.ascontiguousarray(mel_matrix, dtype=np.float32)
        if m.ndim != 2 or m.shape[1] != n_fft // 2 + 1:
            raise NativeError(f"mel matrix must be [n_mels, {n_fft // 2 + 1}], got {m.shape}")
        self.n_fft, self.hop, self.n_mels, self.bins = n_fft, hop, m.shape[0], n_fft // 2 + 1
        self.device = _cuda_device(device)
        self._h = c_void_p()
        with torch.cuda.device(self.device):   # rvc_mel_create allocates and uploads, and takes no stream
            _check(_lib.rvc_mel_create(n_fft, hop, win_length, pad, float(mag_eps), float(log_floor), m.ctypes.data, m.shape[0],
                                       ctypes.byref(self._h)), "rvc_mel_create")

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.rvc_mel_destroy(self._h)
            self._h = None

    def n_frames(self, n_samples: int) -> int:
        t = c_int64()
        _check(_lib.rvc_mel_frames(self._h, n_samples, ctypes.byref(t)), "rvc_mel_frames")
        return t.value

    def forward(self, audio: torch.Tensor, want_mel: bool = True, want_spec: bool = False):
        """audio [B, n] float32 on the handle's device -> (log-mel [B, n_mels, T] or None, magnitude [B, n_fft/2+1, T] or None)."""
        audio = _dev_f32(audio, "audio")
        dev = self.device
        if audio.device != dev:
            raise NativeError(f"MelTransform of {dev} got audio on {audio.device}")
        b, n = audio.shape
        t = self.n_frames(n)
        mel = torch.empty((b, self.n_mels, t), dtype=torch.float32, device=dev) if want_mel else None
        spec = torch.empty((b, self.bins, t), dtype=torch.float32, device=dev) if want_spec else None
        ws = _workspace("mel", dev, "rvc_mel_workspace_bytes", self._h, b, n)
        _call("rvc_mel_forward", dev, self._h, audio.data_ptr(), b, n, _ptr(mel), _ptr(spec), ws.data_ptr(), ws.numel())
        return mel, spec


def resample_poly(x: torch.Tensor, up: int, down: int, h: torch.Tensor) -> torch.Tensor:
    """x [n] float64 on the device, h the FIR (float64, device) -> ceil(n * up / down) samples (resample_poly convention)."""
    if not (x.is_cuda and x.dtype == torch.float64 and x.dim() == 1 and h.is_cuda and h.dtype == torch.float64):
        raise NativeError("resample_poly wants 1-D float64 HBM tensors")
    x, h = x.contiguous(), h.contiguous()
    n_out = -(-x.numel() * up // down)
    y = torch.empty(n_out, dtype=torch.float64, device=x.device)
    _call("rvc_resample_poly_f64", _device(x, h), x.data_ptr(), x.numel(), int(up), int(down), h.data_ptr(), h.numel(), y.data_ptr(), n_out)
    return y


# ---- K6 ------------------------------------------------------------------------------------------
_ff_coef_cache = {}


def _filtfilt_coef(b, a):
    import numpy as np
    from scipy import signal
    key = (tuple(b), tuple(a))
    if key not in _ff_coef_cache:
        b = np.asarray(b, dtype=np.float64)
        a = np.asarray(a, dtype=np.float64)
        if not (b.shape == (6,) and a.shape == (6,) and a[0] == 1.0):
            raise NativeError("filtfilt_order5 wants b[6], a[6] with a[0] == 1")
        _ff_coef_cache[key] = np.ascontiguousarray(np.concatenate([b, a, signal.lfilter_zi(b, a)]))
    return _ff_coef_cache[key]


def filtfilt_terms(b, a) -> int:
    """The length of the state table rvc_filtfilt_order5 keeps for these coefficients: the input samples in front of a chunk that
    its start state is summed over."""
    coef, terms = _filtfilt_coef(b, a), c_int64()
    _check(_lib.rvc_filtfilt_order5_terms(coef.ctypes.data, ctypes.byref(terms)), "rvc_filtfilt_order5_terms")
    return terms.value


def filtfilt_order5(x: torch.Tensor, b, a) -> torch.Tensor:
    """scipy.signal.filtfilt(b, a, x) for a 5th-order filter; x: 1-D float64 on the device.  Non-finite, unstable and too slow
    coefficient sets are refused by the library."""
    if not x.is_cuda or x.dtype != torch.float64 or x.dim() != 1:
        raise NativeError("filtfilt_order5 wants a 1-D float64 HBM tensor")
    x = x.contiguous()
    coef = _filtfilt_coef(b, a)
    y = torch.empty_like(x)
    ws = _workspace("filtfilt", x.device, "rvc_filtfilt_workspace_bytes", x.numel())
    _call("rvc_filtfilt_order5", x.device, x.data_ptr(), x.numel(), coef.ctypes.data, y.data_ptr(), ws.data_ptr(), ws.numel())
    return y


# ---- K17 -----------------------------------------------------------------------------------------
def _lfilter_coef(b, a):
    import numpy as np
    b = np.asarray(b, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    if b.shape != (6,) or a.shape != (6,):
        raise NativeError("lfilter_order5 wants b[6], a[6]")
    return np.ascontiguousarray(np.concatenate([b, a]))


def lfilter_warmup(b, a) -> int:
    """The warm-up (samples) rvc_lfilter_order5_f64 runs in front of every chunk for these coefficients."""
    coef, warm = _lfilter_coef(b, a), c_int64()
    _check(_lib.rvc_lfilter_order5_warmup(coef.ctypes.data, ctypes.byref(warm)), "rvc_lfilter_order5_warmup")
    return warm.value


def lfilter_order5(x: torch.Tensor, b, a) -> torch.Tensor:
    """scipy.signal.lfilter(b, a, x) (zero initial state) for a 5th-order filter; x: 1-D float64 on the device."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float64 or x.dim() != 1:
        raise NativeError("lfilter_order5 wants a 1-D float64 HBM tensor")
    x = x.contiguous()
    coef = _lfilter_coef(b, a)
    y = torch.empty_like(x)
    if x.numel() == 0:               # an empty tensor has no storage to point at; the coefficients are still checked
        lfilter_warmup(b, a)
        return y
    _call("rvc_lfilter_order5_f64", x.device, x.data_ptr(), x.numel(), coef.ctypes.data, y.data_ptr())
    return y


def frame_rms(x: torch.Tensor, frame_length: int, hop_length: int) -> torch.Tensor:
    """get_rms of the reference's slicer.py: x 1-D float64 on the device -> float64 [n_frames] on the device."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float64 or x.dim() != 1:
        raise NativeError("frame_rms wants a 1-D float64 HBM tensor")
    x = x.contiguous()
    n_frames, need = c_int64(), c_size_t()
    _check(_lib.rvc_frame_rms_frames(x.numel(), int(frame_length), int(hop_length), ctypes.byref(n_frames), ctypes.byref(need)),
           "rvc_frame_rms_frames")
    out = torch.empty(n_frames.value, dtype=torch.float64, device=x.device)
    ws = _ws.get("frame_rms", need.value, x.device)
    # an empty tensor has no storage: hand the library an address it never dereferences (n == 0 reads nothing)
    _call("rvc_frame_rms_f64", x.device, x.data_ptr() or ws.data_ptr(), x.numel(), int(frame_length), int(hop_length),
          out.data_ptr() or ws.data_ptr(), n_frames.value, ws.data_ptr(), ws.numel())
    return out


def slice_export(x: torch.Tensor, bounds, up: int, down: int, h: torch.Tensor):
    """Every slice of one file in one launch.  x: 1-D float64 on the device; bounds: [(start, end), ...] half-open sample ranges;
    h: the FIR of rvc_amd.lib.audio.resample_filter(up, down) on the device.
    -> (full float32 [sum len], lo float32 [sum ceil(len * up / down)], off_full, off_lo): the two packed device buffers and the
    n_seg + 1 offsets of every slice in each (Python lists)."""
    import numpy as np
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 1
            and torch.is_tensor(h) and h.is_cuda and h.dtype == torch.float64 and h.dim() == 1 and h.device == x.device):
        raise NativeError("slice_export wants 1-D float64 HBM tensors on one device")
    x, h = x.contiguous(), h.contiguous()
    try:
        tab = np.ascontiguousarray(np.asarray(bounds, dtype=np.int64).reshape(-1, 2))
    except (TypeError, ValueError, OverflowError) as e:
        raise NativeError(f"slice_export: bounds must be (start, end) integer pairs ({e})")
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise NativeError(f"slice_export: up = {up}, down = {down} must be at least 1")
    n_seg = tab.shape[0]
    length = np.maximum(tab[:, 1] - tab[:, 0], 0)                  # a refused table still gets buffers of a sane size
    off_full = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    off_lo = np.concatenate([[0], np.cumsum(-(-(length * up) // down))]).astype(np.int64)
    tables = torch.from_numpy(np.concatenate([tab.reshape(-1), off_full, off_lo])).to(x.device)
    full = torch.empty(int(off_full[-1]), dtype=torch.float32, device=x.device)
    lo = torch.empty(int(off_lo[-1]), dtype=torch.float32, device=x.device)
    seg_ptr = tables.data_ptr()
    _call("rvc_slice_export_f32", x.device, x.data_ptr() or seg_ptr, x.numel(), tab.ctypes.data, seg_ptr, seg_ptr + 16 * n_seg,
          seg_ptr + 16 * n_seg + 8 * (n_seg + 1), n_seg, up, down, h.data_ptr(), h.numel(),
          full.data_ptr() or seg_ptr, full.numel(), lo.data_ptr() or seg_ptr, lo.numel())
    return full, lo, off_full.tolist(), off_lo.tolist()


# ---- K18 -----------------------------------------------------------------------------------------
def spectral_gate_params(sr: int):
    """-> (nf, nt, b, freq_taps[nf + 1], time_taps[nt + 1]): the constants rvc_spectral_gate_f32 derives from `sr` on the host
    (float64) -- the half-widths of the mask smoothing filter, the smoother's coefficient and the filter's normalised 1-D factors
    by distance from the centre.  No device access."""
    import numpy as np
    nf, nt, b = c_int(), c_int(), ctypes.c_double()
    ft, tt = np.zeros(51, dtype=np.float64), np.zeros(51, dtype=np.float64)
    _check(_lib.rvc_spectral_gate_params(int(sr), ctypes.byref(nf), ctypes.byref(nt), ctypes.byref(b), ft.ctypes.data, tt.ctypes.data),
           "rvc_spectral_gate_params")
    return nf.value, nt.value, b.value, ft[:nf.value + 1].copy(), tt[:nt.value + 1].copy()


def spectral_gate(y: torch.Tensor, sr: int, prop_decrease: float = 1.0, chunk_size: int = 600000, padding: int = 30000) -> torch.Tensor:
    """The non-stationary spectral gate of include/rvc_amd.h (K18) over y: 1-D float32 on the device -> float32 [n] on the same
    device, enqueued on its current stream."""
    if not torch.is_tensor(y) or y.dim() != 1:
        raise NativeError("spectral_gate wants a 1-D float32 HBM tensor")
    y = _dev_f32(y, "y")
    out = torch.empty_like(y)
    n = y.numel()
    dims = (n, int(sr), int(chunk_size), int(padding))
    ws = _workspace("spectral_gate", y.device, "rvc_spectral_gate_workspace_bytes", *dims)
    # an empty tensor has no storage: hand the library an address it never dereferences (n == 0 touches nothing)
    _call("rvc_spectral_gate_f32", y.device, y.data_ptr() or ws.data_ptr(), n, int(sr), float(prop_decrease), int(chunk_size), int(padding),
          out.data_ptr() or ws.data_ptr(), ws.data_ptr(), ws.numel())
    return out


# ---- K19 -----------------------------------------------------------------------------------------
def formant_shift(x: torch.Tensor, sr: int, quefrency_s: float, distortion: float, group_frames: int = 0) -> torch.Tensor:
    """The formant shifter of include/rvc_amd.h (K19) over x: 1-D float32 on the device, at least 1024 samples -> float32 [n] on
    the same device, enqueued on its current stream."""
    if not torch.is_tensor(x) or x.dim() != 1:
        raise NativeError("formant_shift wants a 1-D float32 HBM tensor")
    x = _dev_f32(x, "x")
    n = x.numel()
    ws = _workspace("formant_shift", x.device, "rvc_formant_shift_workspace_bytes", n, int(group_frames))
    out = torch.empty_like(x)
    _call("rvc_formant_shift_f32", x.device, x.data_ptr(), n, int(sr), float(quefrency_s), float(distortion), int(group_frames),
          out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


# ---- K23 -----------------------------------------------------------------------------------------
def spectral_features(x: torch.Tensor, sr: int, roll_percent: float = 0.85, want_mag: bool = False, want_db: bool = False):
    """The analyzer's spectral features of include/rvc_amd.h (K23) over x: 1-D float32 on the device -> (cent, bw, rolloff, mag,
    db) on the same device, enqueued on its current stream.  The curves are float64 [F], F = 1 + n // 512; mag and db are
    float32 [F, 1025] (frame-major), or None where not asked for: a plane that is not wanted is never written."""
    if not torch.is_tensor(x) or x.dim() != 1:
        raise NativeError("spectral_features wants a 1-D float32 HBM tensor")
    x = _dev_f32(x, "x")
    n = x.numel()
    ws = _workspace("spectral_features", x.device, "rvc_spectral_features_workspace_bytes", n)
    frames = 1 + n // 512
    curves = torch.empty(3, frames, dtype=torch.float64, device=x.device)
    mag = torch.empty(frames, 1025, dtype=torch.float32, device=x.device) if want_mag else None
    db = torch.empty(frames, 1025, dtype=torch.float32, device=x.device) if want_db else None
    _call("rvc_spectral_features_f32", x.device, x.data_ptr(), n, int(sr), float(roll_percent), _ptr(mag), _ptr(db),
          curves[0].data_ptr(), curves[1].data_ptr(), curves[2].data_ptr(), ws.data_ptr(), ws.numel())
    return curves[0], curves[1], curves[2], mag, db


# ---- K24 -----------------------------------------------------------------------------------------
def melcep(x: torch.Tensor, sr: int, mel: torch.Tensor, n_coef: int) -> torch.Tensor:
    """rvc_melcep_f32 (K24): x 1-D float32 on the device at `sr`, mel float32 [n_mels, 513] on the same device -> the mel-cepstral
    coefficients c[1 .. n_coef] per 5 ms frame, float32 [1 + n // (sr // 200), n_coef]."""
    if not torch.is_tensor(x) or x.dim() != 1:
        raise NativeError("melcep wants a 1-D float32 HBM tensor")
    if not torch.is_tensor(mel) or mel.dim() != 2 or mel.shape[1] != 513:
        raise NativeError("melcep wants the mel filterbank as a float32 [n_mels, 513] HBM tensor")
    _device(x, mel)
    x, mel = _dev_f32(x, "x"), _dev_f32(mel, "mel")
    n, sr = x.numel(), int(sr)
    ws = _workspace("melcep", x.device, "rvc_melcep_workspace_bytes", n, sr)     # refuses n < 1 and a rate outside the rule
    out = torch.empty(1 + n // (sr // 200), int(n_coef), dtype=torch.float32, device=x.device)
    _call("rvc_melcep_f32", x.device, x.data_ptr(), n, sr, mel.data_ptr(), mel.shape[0], int(n_coef), out.data_ptr(), ws.data_ptr(),
          ws.numel())
    return out


def _features_pair(a: torch.Tensor, b: torch.Tensor, what: str):
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise NativeError(f"{what} wants two [frames, dim] float32 HBM tensors of one dim")
    _device(a, b)
    return _dev_f32(a, f"{what}: a"), _dev_f32(b, f"{what}: b")


def dtw(a: torch.Tensor, b: torch.Tensor, band: int = -1):
    """rvc_dtw_f64 (K24) -> (out, path) on the device: out float64 [2] = (the total cost, the path's length L), path int32
    [Ta + Tb - 1, 2] of which the first L rows are written.  band < 0: no band."""
    a, b = _features_pair(a, b, "dtw")
    ta, tb = a.shape[0], b.shape[0]
    ws = _workspace("dtw", a.device, "rvc_dtw_workspace_bytes", ta, tb)
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    path = torch.empty(ta + tb - 1, 2, dtype=torch.int32, device=a.device)
    _call("rvc_dtw_f64", a.device, a.data_ptr(), ta, b.data_ptr(), tb, a.shape[1], int(band), out.data_ptr(), path.data_ptr(),
          ws.data_ptr(), ws.numel())
    return out, path


def frame_dist_sum(a: torch.Tensor, b: torch.Tensor, frames: int) -> torch.Tensor:
    """rvc_frame_dist_sum_f64 (K24): the sum of the Euclidean distances of the first `frames` rows of a and b -> float64 [1]."""
    a, b = _features_pair(a, b, "frame_dist_sum")
    if frames > min(a.shape[0], b.shape[0]):
        raise NativeError(f"frame_dist_sum: frames = {frames} exceeds a length ({a.shape[0]}, {b.shape[0]})")
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    _call("rvc_frame_dist_sum_f64", a.device, a.data_ptr(), b.data_ptr(), int(frames), a.shape[1], out.data_ptr())
    return out


def f0_track_sums(f0_a: torch.Tensor, f0_b: torch.Tensor) -> torch.Tensor:
    """rvc_f0_track_sums_f64 (K24): two 1-D float64 contours of equal length on the device -> the twelve sums of include/rvc_amd.h,
    float64 [12]."""
    if not (torch.is_tensor(f0_a) and torch.is_tensor(f0_b)) or f0_a.dim() != 1 or f0_a.shape != f0_b.shape:
        raise NativeError("f0_track_sums wants two 1-D float64 HBM tensors of equal length")
    device = _device(f0_a, f0_b)
    if not f0_a.is_cuda or f0_a.dtype != torch.float64 or f0_b.dtype != torch.float64:
        raise NativeError("f0_track_sums wants float64 contours in HBM (no CPU fallback)")
    f0_a, f0_b = f0_a.contiguous(), f0_b.contiguous()
    out = torch.empty(12, dtype=torch.float64, device=device)
    _call("rvc_f0_track_sums_f64", device, f0_a.data_ptr(), f0_b.data_ptr(), f0_a.numel(), out.data_ptr())
    return out


# ---- K21 -----------------------------------------------------------------------------------------
def _vec_f32(t, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dim() != 1:
        raise NativeError(f"{name} must be a 1-D float32 HBM tensor")
    if not t.is_contiguous():   # an in/out argument cannot be replaced by a copy
        raise NativeError(f"{name} must be contiguous")
    return _dev_f32(t, name)


def stream_window(hist: torch.Tensor, block: torch.Tensor) -> torch.Tensor:
    """rvc_stream_window_f32 (K21): -> window = [hist | block], a new float32 tensor; `hist` (1-D float32 on the device, updated in
    place) then holds the window's last len(hist) samples.  One launch on the device's current stream."""
    hist, block = _vec_f32(hist, "hist"), _vec_f32(block, "block")
    dev = _device(hist, block)
    window = torch.empty(hist.numel() + block.numel(), dtype=torch.float32, device=dev)
    if window.numel() == 0:
        return window
    # an empty tensor has no storage: hand the library an address it never dereferences
    _call("rvc_stream_window_f32", dev, hist.data_ptr() or block.data_ptr(), hist.numel(), block.data_ptr() or hist.data_ptr(),
          block.numel(), window.data_ptr())
    return window


def sola(infer: torch.Tensor, buf: torch.Tensor, fade_in: torch.Tensor, search: int, block: int, offset: torch.Tensor = None):
    """rvc_sola_f32 (K21): infer [block + len(buf) + search], buf [xfade] (the saved tail, updated in place) and fade_in [xfade],
    1-D float32 on the device -> (out float32 [block], offset int32 [1] on the device: the chosen lag; pass `offset` to reuse one).
    Two launches on the device's current stream; nothing is read back."""
    infer, buf, fade_in = _vec_f32(infer, "infer"), _vec_f32(buf, "buf"), _vec_f32(fade_in, "fade_in")
    dev = _device(infer, buf, fade_in, offset)
    xfade, search, block = buf.numel(), int(search), int(block)
    if fade_in.numel() != xfade:
        raise NativeError(f"sola: fade_in has {fade_in.numel()} samples, buf {xfade}")
    if offset is None:
        offset = torch.empty(1, dtype=torch.int32, device=dev)
    elif not (offset.is_cuda and offset.dtype == torch.int32 and offset.numel() == 1):
        raise NativeError("sola: offset must be an int32 HBM tensor of one element")
    ws = _workspace("sola", dev, "rvc_sola_workspace_bytes", xfade, search)
    out = torch.empty(max(block, 0), dtype=torch.float32, device=dev)
    _call("rvc_sola_f32", dev, infer.data_ptr(), infer.numel(), buf.data_ptr(), fade_in.data_ptr(), xfade, search, block,
          out.data_ptr(), offset.data_ptr(), ws.data_ptr(), ws.numel())
    return out, offset


# ---- K22 -----------------------------------------------------------------------------------------
FX_GAIN, FX_DISTORTION, FX_BITCRUSH, FX_CLIPPING = 1, 2, 4, 8


def fx_reverb_params(sr: int):
    """-> (comb lengths [8], allpass lengths [4]) of rvc_fx_reverb_f32 at `sr`.  No device access."""
    comb, allpass = (c_int * 8)(), (c_int * 4)()
    _check(_lib.rvc_fx_reverb_params(int(sr), comb, allpass), "rvc_fx_reverb_params")
    return list(comb), list(allpass)


def fx_ballistics(sr: int, attack_ms: float, release_ms: float):
    """-> (c_attack, c_release) as rvc_fx_compressor_f32 derives them, in double.  No device access."""
    ca, cr = c_double(), c_double()
    _check(_lib.rvc_fx_ballistics(int(sr), float(attack_ms), float(release_ms), ctypes.byref(ca), ctypes.byref(cr)), "rvc_fx_ballistics")
    return ca.value, cr.value


def _fx_signal(x, what: str) -> torch.Tensor:
    if not torch.is_tensor(x) or x.dim() != 1:
        raise NativeError(f"{what} wants a 1-D float32 HBM tensor")
    return _dev_f32(x, "x")


def fx_pointwise(x: torch.Tensor, stages: int, gain_db: float = 0.0, drive_db: float = 0.0, bit_depth: float = 8.0,
                 clip_threshold_db: float = 0.0) -> torch.Tensor:
    """rvc_fx_pointwise_f32 (K22): the enabled stages of gain | distortion | bitcrush | clipping, in that order, in one launch."""
    x = _fx_signal(x, "fx_pointwise")
    out = torch.empty_like(x)
    _call("rvc_fx_pointwise_f32", x.device, x.data_ptr() or 1, x.numel(), int(stages), float(gain_db), float(drive_db), float(bit_depth),
          float(clip_threshold_db), out.data_ptr() or 1)   # an empty tensor has no storage: n == 0 touches nothing
    return out


def fx_delay(x: torch.Tensor, sr: int, delay_seconds: float, feedback: float, mix: float) -> torch.Tensor:
    """rvc_fx_delay_f32 (K22): one launch on the device's current stream."""
    x = _fx_signal(x, "fx_delay")
    out = torch.empty_like(x)
    _call("rvc_fx_delay_f32", x.device, x.data_ptr() or 1, x.numel(), int(sr), float(delay_seconds), float(feedback), float(mix),
          out.data_ptr() or 1)
    return out


def fx_chorus(x: torch.Tensor, sr: int, rate_hz: float, depth: float, centre_delay_ms: float, feedback: float, mix: float) -> torch.Tensor:
    """rvc_fx_chorus_f32 (K22): a gather for feedback 0, otherwise one workgroup walking the signal (slow)."""
    x = _fx_signal(x, "fx_chorus")
    out = torch.empty_like(x)
    ws = _workspace("fx_chorus", x.device, "rvc_fx_chorus_workspace_bytes", x.numel(), float(feedback))
    _call("rvc_fx_chorus_f32", x.device, x.data_ptr() or 1, x.numel(), int(sr), float(rate_hz), float(depth), float(centre_delay_ms),
          float(feedback), float(mix), out.data_ptr() or 1, ws.data_ptr(), ws.numel())
    return out


def fx_reverb(x: torch.Tensor, sr: int, room_size: float, damping: float, wet_level: float, dry_level: float, width: float,
              freeze_mode: float) -> torch.Tensor:
    """rvc_fx_reverb_f32 (K22): Freeverb's mono path, seven launches."""
    x = _fx_signal(x, "fx_reverb")
    out = torch.empty_like(x)
    ws = _workspace("fx_reverb", x.device, "rvc_fx_reverb_workspace_bytes", x.numel())
    _call("rvc_fx_reverb_f32", x.device, x.data_ptr() or 1, x.numel(), int(sr), float(room_size), float(damping), float(wet_level),
          float(dry_level), float(width), float(freeze_mode), out.data_ptr() or 1, ws.data_ptr(), ws.numel())
    return out


def fx_compressor(x: torch.Tensor, sr: int, threshold_db: float, ratio: float, attack_ms: float, release_ms: float,
                  chunk: int = 0) -> torch.Tensor:
    """rvc_fx_compressor_f32 (K22); `chunk` = 0 lets the library choose (the result does not depend on it)."""
    x = _fx_signal(x, "fx_compressor")
    out = torch.empty_like(x)
    ws = _workspace("fx_compressor", x.device, "rvc_fx_compressor_workspace_bytes", x.numel(), int(chunk), 0)
    _call("rvc_fx_compressor_f32", x.device, x.data_ptr() or 1, x.numel(), int(sr), float(threshold_db), float(ratio), float(attack_ms),
          float(release_ms), int(chunk), out.data_ptr() or 1, ws.data_ptr(), ws.numel())
    return out


def fx_limiter(x: torch.Tensor, sr: int, threshold_db: float, release_ms: float, chunk: int = 0) -> torch.Tensor:
    """rvc_fx_limiter_f32 (K22): two compressors, the make-up gain and the clamp."""
    x = _fx_signal(x, "fx_limiter")
    out = torch.empty_like(x)
    ws = _workspace("fx_limiter", x.device, "rvc_fx_compressor_workspace_bytes", x.numel(), int(chunk), 1)
    _call("rvc_fx_limiter_f32", x.device, x.data_ptr() or 1, x.numel(), int(sr), float(threshold_db), float(release_ms), int(chunk),
          out.data_ptr() or 1, ws.data_ptr(), ws.numel())
    return out


# ---- K5 ------------------------------------------------------------------------------------------
def _signal_pair(x: torch.Tensor, y: torch.Tensor, what: str):
    if x.dim() != 1 or y.dim() != 1 or x.shape != y.shape:
        raise NativeError(f"{what} wants two 1-D signals of equal length, got shapes {tuple(x.shape)} and {tuple(y.shape)}")
    _device(x, y)
    return _dev_f32(x, f"{what}: x"), _dev_f32(y, f"{what}: y")


def mrstft_sums(x: torch.Tensor, y: torch.Tensor, fft_sizes, hop_sizes, win_lengths, eps: float = 1e-8) -> torch.Tensor:
    """The multi-resolution STFT sums of include/rvc_amd.h (K20) of the prediction x and the target y (1-D float32 on the device)
    -> float64 [n_res, 4] on the device: sum (ymag - xmag)^2, sum ymag^2, sum |log xmag - log ymag| and the number of terms."""
    x, y = _signal_pair(x, y, "mrstft_sums")
    n_res = len(fft_sizes)
    if not (len(hop_sizes) == len(win_lengths) == n_res):
        raise NativeError("mrstft_sums: fft_sizes, hop_sizes and win_lengths must have one entry per resolution")
    arr = [(c_int * max(n_res, 1))(*[int(v) for v in vals]) for vals in (fft_sizes, hop_sizes, win_lengths)]
    ws = _workspace("mrstft_sums", x.device, "rvc_mrstft_sums_workspace_bytes", x.numel(), *arr, n_res)
    out = torch.empty(max(n_res, 1), 4, dtype=torch.float64, device=x.device)
    _call("rvc_mrstft_sums_f32", x.device, x.data_ptr(), y.data_ptr(), x.numel(), *arr, n_res, float(eps), out.data_ptr(),
          ws.data_ptr(), ws.numel())
    return out


def si_sdr_sums(preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The five SI-SDR sums of include/rvc_amd.h (K20) -> float64 [5] on the device: sum p, sum t, and of the centred signals
    sum pc tc, sum tc^2, sum pc^2."""
    preds, target = _signal_pair(preds, target, "si_sdr_sums")
    ws = _workspace("si_sdr_sums", preds.device, "rvc_si_sdr_sums_workspace_bytes", preds.numel())
    out = torch.empty(5, dtype=torch.float64, device=preds.device)
    _call("rvc_si_sdr_sums_f32", preds.device, preds.data_ptr(), target.data_ptr(), preds.numel(), out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def mean_abs_diff_sum(a: torch.Tensor, b: torch.Tensor, min_t: int) -> torch.Tensor:
    """sum |a[r, c] - b[r, c]| over the first min_t columns of two float32 matrices on the device with as many rows (each may be
    a column slice of a wider matrix: the row stride is passed on) -> float64 [1] on the device (K20)."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise NativeError(f"mean_abs_diff_sum wants two matrices with as many rows, got shapes {tuple(a.shape)} and {tuple(b.shape)}")
    if min_t > min(a.shape[1], b.shape[1]):
        raise NativeError(f"mean_abs_diff_sum: min_t = {min_t} exceeds a width ({a.shape[1]}, {b.shape[1]})")
    _device(a, b)
    a, b = (t if t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] else
            _dev_f32(t, "mean_abs_diff_sum: matrix") for t in (a, b))
    rows = a.shape[0]
    ws = _workspace("mean_abs_diff", a.device, "rvc_mean_abs_diff_workspace_bytes", rows, int(min_t))
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    _call("rvc_mean_abs_diff_f32", a.device, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), rows, int(min_t), out.data_ptr(),
          ws.data_ptr(), ws.numel())
    return out


def bigru_forward(gi: torch.Tensor, whh_t: torch.Tensor, bhh: torch.Tensor, multi_cu: bool = True) -> torch.Tensor:
    """gi [B,T,2,768] (input projections) -> [B,T,512]; see include/rvc_amd.h."""
    gi, whh_t, bhh = _dev_f32(gi, "gi"), _dev_f32(whh_t, "whh_t"), _dev_f32(bhh, "bhh")
    dev = _device(gi, whh_t, bhh)
    b, t = gi.shape[0], gi.shape[1]
    out = torch.empty((b, t, 512), dtype=torch.float32, device=dev)
    ws = _workspace("bigru", dev, "rvc_bigru_workspace_bytes", b) if multi_cu else None
    _call("rvc_bigru_forward", dev, gi.data_ptr(), whh_t.data_ptr(), bhh.data_ptr(), out.data_ptr(), b, t, 256, _ptr(ws),
          ws.numel() if multi_cu else 0)
    return out


def bigru_redone(batch: int = 1, device=None) -> int:
    """How many (batch item, direction) sequences of the last multi-workgroup forward on the current stream's workspace
    had to be recomputed by the single-workgroup kernel (synchronises the stream)."""
    device = _cuda_device(device)
    ws = _workspace("bigru", device, "rvc_bigru_workspace_bytes", batch)
    n = c_int()
    _call("rvc_bigru_status", device, ws.data_ptr(), batch, ctypes.byref(n))
    return n.value


def bigru_set_spin_limit(polls: int) -> None:
    _check(_lib.rvc_bigru_set_spin_limit(int(polls)), "rvc_bigru_set_spin_limit")


# ---- HuBERT attention -------------------------------------------------------------------------------
def _is_f32_hbm(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def attention_qkv(qkv: torch.Tensor, n_heads: int, scale: float, emb_rel_k: torch.Tensor = None,
                  emb_rel_v: torch.Tensor = None) -> torch.Tensor:
    """qkv [B, T, 3 * n_heads * d] (fused projection output, d = 64 or 96) -> softmax(q k^T * scale [+ rel]) v [+ rel]
    as [B, T, n_heads * d].  emb_rel_k / emb_rel_v [21, d]: the TextEncoder's relative-position embeddings."""
    if not (_is_f32_hbm(qkv) and qkv.dim() == 3):
        raise NativeError("attention_qkv wants a contiguous float32 HBM tensor [B, T, 3 * n_heads * d]")
    b, t, c = qkv.shape
    hd = c // (3 * n_heads)
    rel = (emb_rel_k, emb_rel_v) if emb_rel_k is not None else (None, None)
    if rel[0] is not None and not all(e is not None and _is_f32_hbm(e) and tuple(e.shape) == (21, hd) for e in rel):
        raise NativeError(f"attention_qkv wants emb_rel_k and emb_rel_v as contiguous float32 HBM tensors [21, {hd}]")
    dev = _device(qkv, *rel)
    out = torch.empty(b, t, n_heads * hd, dtype=torch.float32, device=dev)
    ws = _workspace("attention", dev, "rvc_attention_workspace_bytes", b, t, n_heads, hd)
    _call("rvc_attention_qkv_f32", dev, qkv.data_ptr(), _ptr(rel[0]), _ptr(rel[1]), out.data_ptr(), b, t, n_heads, hd, float(scale),
          ws.data_ptr(), ws.numel())
    return out


# ---- RMVPE U-Net conv epilogue ------------------------------------------------------------------------
def bias_relu_add_(x: torch.Tensor, bias: torch.Tensor = None, res: torch.Tensor = None, relu: bool = True) -> torch.Tensor:
    """In place: x = relu(x + bias[c]) + res for x [B, C, ...] (contiguous, trailing extent a multiple of 4)."""
    if not (_is_f32_hbm(x) and x.dim() >= 3):
        raise NativeError("bias_relu_add_ wants a contiguous float32 HBM tensor [B, C, ...]")
    b, c = x.shape[0], x.shape[1]
    inner = x.numel() // (b * c)
    if res is not None and not (_is_f32_hbm(res) and res.shape == x.shape):
        raise NativeError("bias_relu_add_ wants res as a contiguous float32 HBM tensor of x's shape")
    _call("rvc_bias_relu_add_f32", _device(x, bias, res), x.data_ptr(), _ptr(bias), _ptr(res), x.data_ptr(), b, c, inner, int(relu))
    return x


def rownorm_gelu_(x: torch.Tensor, gamma: torch.Tensor = None, beta: torch.Tensor = None, eps: float = 1e-5) -> torch.Tensor:
    """In place: x = gelu(group_norm(x, num_groups = channels)) for x [B, C, L] (fp32, HBM, contiguous)."""
    if not (_is_f32_hbm(x) and x.dim() == 3):
        raise NativeError("rownorm_gelu_ wants a contiguous float32 HBM tensor [B, C, L]")
    b, c, length = x.shape
    _call("rvc_rownorm_gelu_f32", _device(x, gamma, beta), x.data_ptr(), _ptr(gamma), _ptr(beta), x.data_ptr(), b, c, length, float(eps))
    return x


def gate_tanh_sigmoid(x: torch.Tensor) -> torch.Tensor:
    """x [B, 2H, T] -> tanh(x[:, :H]) * sigmoid(x[:, H:]) [B, H, T]"""
    if not (_is_f32_hbm(x) and x.dim() == 3 and x.shape[1] % 2 == 0):
        raise NativeError("gate_tanh_sigmoid wants a contiguous float32 HBM tensor [B, 2H, T]")
    b, c2, t = x.shape
    out = torch.empty(b, c2 // 2, t, dtype=torch.float32, device=x.device)
    _call("rvc_gate_tanh_sigmoid_f32", x.device, x.data_ptr(), out.data_ptr(), b, c2 // 2, t)
    return out


def set_concurrency_hint(utterances_in_flight: int) -> None:
    _check(_lib.rvc_set_concurrency_hint(int(utterances_in_flight)), "rvc_set_concurrency_hint")


# ---- multi-GPU: RCCL index broadcast + device checksum ----------------------------------------------
COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(_lib.rvc_comm_unique_id(buf), "rvc_comm_unique_id")
    return buf.raw


class Comm:
    """RCCL communicator of the job (one rank per GPU), created collectively from rank 0's 128-byte id."""

    def __init__(self, unique_id: bytes, n_ranks: int, rank: int):
        if len(unique_id) != COMM_ID_BYTES:
            raise NativeError(f"Comm wants the {COMM_ID_BYTES}-byte id of comm_unique_id, got {len(unique_id)} bytes")
        self._h = c_void_p()
        _check(_lib.rvc_comm_create(ctypes.create_string_buffer(unique_id, COMM_ID_BYTES), int(n_ranks), int(rank),
                                    ctypes.byref(self._h)), "rvc_comm_create")

    def info(self) -> dict:
        n, r, v = c_int(), c_int(), c_int()
        path = ctypes.create_string_buffer(512)
        _check(_lib.rvc_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(v), path, 512), "rvc_comm_info")
        return {"n_ranks": n.value, "rank": r.value, "rccl_version": v.value, "library": path.value.decode()}

    def broadcast_(self, t: torch.Tensor, root: int = 0) -> torch.Tensor:
        """In-place broadcast of a contiguous HBM tensor's bytes from ``root`` on the current stream of the tensor's device."""
        if not t.is_cuda or not t.is_contiguous():
            raise NativeError("Comm.broadcast_ wants a contiguous HBM tensor")
        _call("rvc_index_broadcast", t.device, self._h, t.data_ptr(), t.numel() * t.element_size(), int(root))
        return t

    def destroy(self):
        h, self._h = self._h, None
        if h:
            _check(_lib.rvc_comm_destroy(h), "rvc_comm_destroy")

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.rvc_comm_destroy(self._h)
            self._h = None


def checksum64(t: torch.Tensor) -> torch.Tensor:
    """[2] int64 device tensor: (sum of 32-bit words, sum of (i+1)*word_i) mod 2^64 of the tensor's bytes, computed in HBM."""
    if not t.is_cuda or not t.is_contiguous():
        raise NativeError("checksum64 wants a contiguous HBM tensor")
    out = torch.empty(2, dtype=torch.int64, device=t.device)
    _call("rvc_checksum64", t.device, t.data_ptr(), t.numel() * t.element_size(), out.data_ptr())
    return out


# ---- conv1d: fp32 direct (unit-test entry), Winograd fp32 / bf16x3, and K3d / K3h, the square direct form (C = 128 / 256) of
# ---- csrc/convbf1.hip on two operand formats -- one body, the entry point chosen by name ------------------------------------
def conv1d_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    w = _host(w)
    packed = torch.empty(w.numel(), dtype=torch.float32, device=device)
    _call("rvc_conv1d_pack_weight", packed.device, w.data_ptr(), w.shape[0], w.shape[1], w.shape[2], packed.data_ptr())
    return packed


def conv1d_wino_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    w = _host(w)
    c_out, c_in, k = w.shape
    u = torch.empty(3 * ((k + 2) // 3) * c_in * c_out, dtype=torch.float32, device=device)
    _call("rvc_conv1d_wino_pack_weight", u.device, w.data_ptr(), c_out, c_in, k, u.data_ptr())
    return u


def conv1d_winobf_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    w = _host(w)
    return _pack_slab("rvc_conv1d_winobf", device, (w,), tuple(w.shape))


def _conv1d_square_pack(stem: str, w: torch.Tensor, device) -> torch.Tensor:
    w = _host(w)
    c, c_in, k = w.shape
    if c != c_in:
        raise NativeError(f"{stem[4:]}: a square conv expected, got {tuple(w.shape)}")
    return _pack_slab(stem, device, (w,), (c, k))


def conv1d_bf16w_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    """nn.Conv1d weight [c, c, k] -> one-term direct-form fragment slab on the device (the taps ROUNDED to bf16)."""
    return _conv1d_square_pack("rvc_conv1d_bf16w", w, device)


def conv1d_f16x2_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    """nn.Conv1d weight [c, c, k] -> fp16 (hi, lo * 2^11) direct-form fragment slab on the device; raises for a tap that is
    non-finite or beyond +-65504."""
    return _conv1d_square_pack("rvc_conv1d_f16x2", w, device)


def _conv1d(name: str, x, w_packed, bias, c_out, k, dilation, slope_in, res, acc, out_scale, out):
    """y = out_scale * (conv_d(leaky(x, slope_in)) + bias [+ res] [+ acc]) for x [B, C, L] in HBM through the entry point `name`.
    c_out None: a square direct-form kernel, which takes one channel count and refuses y aliasing x."""
    x = _dev_f32(x, "x")
    b, c_in, length = x.shape
    square = c_out is None
    y = out if out is not None else torch.empty((b, c_in if square else c_out, length), dtype=torch.float32, device=x.device)
    if square and y.data_ptr() == x.data_ptr():
        raise NativeError(f"{name[4:-8]}: x and y must not alias")
    _call(name, _device(x, w_packed, bias, res, acc, y), x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(res), _ptr(acc), y.data_ptr(),
          b, *((c_in,) if square else (c_in, c_out)), length, k, dilation, float(slope_in), float(out_scale))
    return y


def conv1d_forward(x, w_packed, bias, c_out, k, dilation=1, slope_in=1.0, res=None, acc=None, out_scale=1.0):
    return _conv1d("rvc_conv1d_forward", x, w_packed, bias, c_out, k, dilation, slope_in, res, acc, out_scale, None)


def conv1d_forward_into(x, w_packed, bias, c_out, k, dilation=1, slope_in=1.0, res=None, acc=None, out_scale=1.0, out=None):
    return _conv1d("rvc_conv1d_forward", x, w_packed, bias, c_out, k, dilation, slope_in, res, acc, out_scale, out)


def conv1d_wino_forward(x, u_packed, bias, c_out, k, dilation=1, slope_in=1.0, res=None, acc=None, out_scale=1.0, out=None):
    return _conv1d("rvc_conv1d_wino_forward", x, u_packed, bias, c_out, k, dilation, slope_in, res, acc, out_scale, out)


def conv1d_winobf_forward(x, u_packed, bias, c_out, k, dilation=1, slope_in=1.0, res=None, acc=None, out_scale=1.0, out=None):
    return _conv1d("rvc_conv1d_winobf_forward", x, u_packed, bias, c_out, k, dilation, slope_in, res, acc, out_scale, out)


def conv1d_bf16w_forward(x, u_packed, bias, k, dilation=1, slope_in=1.0, res=None, acc=None, out_scale=1.0, out=None):
    """C = 128 / 256 (K3d: the taps rounded to bf16)."""
    return _conv1d("rvc_conv1d_bf16w_forward", x, u_packed, bias, None, k, dilation, slope_in, res, acc, out_scale, out)


def conv1d_f16x2_forward(x, u_packed, bias, k, dilation=1, slope_in=1.0, res=None, acc=None, out_scale=1.0, out=None):
    """C = 128 / 256 (K3h: fp32 taps on error-corrected fp16 pairs)."""
    return _conv1d("rvc_conv1d_f16x2_forward", x, u_packed, bias, None, k, dilation, slope_in, res, acc, out_scale, out)


# ---- K3f: fused ResBlock pair (dilated conv -> conv + residual) on the bf16 matrix cores -------------------------
def resblock_bf16x3_pack_weight(w1: torch.Tensor, w2: torch.Tensor, device, bf16_taps: bool = False) -> torch.Tensor:
    """The two nn.Conv1d weights [c, c, k] of one ResBlock dilation -> fragment slab on the device.  bf16_taps: the taps rounded to
    bf16 (BASELINE cfg 4's weight storage), one fragment per group instead of three -- for resblock_bf16x3_forward(bf16_taps=True)."""
    w1, w2 = _host(w1), _host(w2)
    c, c_in, k = w1.shape
    if c != c_in or w2.shape != w1.shape:
        raise NativeError(f"resblock pair: square convs of one shape expected, got {tuple(w1.shape)} and {tuple(w2.shape)}")
    return _pack_slab("rvc_resblock_bf16w" if bf16_taps else "rvc_resblock_bf16x3", device, (w1, w2), (c, k))


def resblock_bf16x3_forward(x, u_packed, b1, b2, k, dilation=1, slope=0.1, acc=None, out_scale=1.0, out=None, bf16_taps: bool = False):
    """y = out_scale * (conv2(leaky(conv1_d(leaky(x)) + b1)) + b2 + x [+ acc]) for x [B, C, L] in HBM (residuals.py:75-86).
    bf16_taps: u_packed holds one-term fragments of bf16-valued taps (three products per multiply-add; hifigan_mrf.py:13-83 at cfg 4)."""
    x = _dev_f32(x, "x")
    b, c, length = x.shape
    y = out if out is not None else torch.empty_like(x)
    if y.data_ptr() == x.data_ptr():
        raise NativeError("resblock pair: x and y must not alias")
    _call("rvc_resblock_bf16w_forward" if bf16_taps else "rvc_resblock_bf16x3_forward", _device(x, u_packed, b1, b2, acc, y),
          x.data_ptr(), u_packed.data_ptr(), _ptr(b1), _ptr(b2), _ptr(acc), y.data_ptr(), b, c, length, k, dilation, float(slope),
          float(out_scale))
    return y


# ---- K3u: upsampling step (polyphase ConvTranspose1d + folded noise conv) on the bf16 matrix cores -----------------
def upsample_bf16x3_pack_weight(up_w: torch.Tensor, noise_w, bias, rate: int, nc_stride: int, device):
    """ConvTranspose1d weight [c_in, c_out, ksize] (+ the noise conv's weight [c_out, 1, nc_k] or None, + the summed bias [c_out] or None)
    -> (fragment slab, noise weights [c_out, nc_k] or None, bias or None) on the device, the triple `upsample_bf16x3_forward` takes."""
    up_w = _host(up_w)
    c_in, c_out, ksize = up_w.shape
    nw = _host(noise_w).reshape(c_out, -1).contiguous() if noise_w is not None else None
    nc_k = nw.shape[1] if nw is not None else 0
    b = _host(bias) if bias is not None else None
    u = _pack_slab("rvc_upsample_bf16x3", device, (up_w, nw, b), (c_in, c_out, rate, ksize, nc_k, nc_stride))
    return u, (nw.to(device) if nw is not None else None), (b.to(device) if b is not None else None)


def upsample_bf16x3_forward(x, har, packed, c_out, rate, ksize, pad, nc_stride=1, nc_pad=0, slope=0.1):
    """y [B, c_out, (L - 1) rate - 2 pad + ksize] = bias + conv_transpose1d(leaky(x)) + noise_conv(har) for x [B, c_in, L], har [B, Lh]."""
    u, nw, bias = packed
    x = _dev_f32(x, "x")
    b, c_in, length = x.shape
    l_out = (length - 1) * rate - 2 * pad + ksize
    y = torch.empty((b, c_out, l_out), dtype=torch.float32, device=x.device)
    if har is not None:
        har = _dev_f32(har, "har")
    _call("rvc_upsample_bf16x3_forward", _device(x, har, u, bias), x.data_ptr(), _ptr(har), har.shape[-1] if har is not None else 0,
          u.data_ptr(), _ptr(bias), y.data_ptr(), b, c_in, c_out, length, rate, ksize, pad, nw.shape[1] if nw is not None else 0,
          nc_stride, nc_pad, float(slope))
    return y


def resblock_bf16x3_set_enabled(enabled: bool) -> None:
    """Process-wide: decoder handles finalized while this is off keep their narrow ResBlock stages on the unfused kernels."""
    _check(_lib.rvc_resblock_bf16x3_set_enabled(1 if enabled else 0), "rvc_resblock_bf16x3_set_enabled")


# ---- K11: fp32 GEMM / strided conv1d as exact bf16x3 splits on the bf16 matrix cores ----------------------------
def gemm_bf16x3_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    """nn.Linear weight [out, in] or nn.Conv1d weight [c_out, c_in, taps] -> fragment slab on the device."""
    w = _host(w)
    taps = w.shape[2] if w.dim() == 3 else 1
    m, k_total = w.shape[0], w.shape[1] * taps
    return _pack_slab("rvc_gemm_bf16x3", device, (w,), (m, k_total), (m, k_total, taps))


def linear_bf16x3(x: torch.Tensor, a_packed: torch.Tensor, bias, out_features: int, act: str = "none", res=None) -> torch.Tensor:
    """y = act(x W^T + b) + res for x [..., in] (fp32, HBM, contiguous)."""
    x = _dev_f32(x, "x")
    in_features = x.shape[-1]
    n_rows = x.numel() // in_features
    y = torch.empty(x.shape[:-1] + (out_features,), dtype=torch.float32, device=x.device)
    if res is not None:
        res = _dev_f32(res, "res")
        if res.shape != y.shape:
            raise NativeError(f"linear_bf16x3: res {tuple(res.shape)} must have the result's shape {tuple(y.shape)}")
    _call("rvc_linear_bf16x3", _device(x, a_packed, bias, res), x.data_ptr(), a_packed.data_ptr(), _ptr(bias), _ptr(res), y.data_ptr(),
          n_rows, in_features, out_features, {"none": 0, "gelu": 1}[act])
    return y


# ---- K15: FCPE between its GEMMs (csrc/fcpe.hip) -------------------------------------------------------------------------
def glu_dwconv_silu(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """silu(depthwise_conv_K(x[:, :C] * sigmoid(x[:, C:]))) along the rows of x [n_rows, 2C]; w [C, K] (K odd, <= 31), bias [C]."""
    x, w, bias = _dev_f32(x, "x"), _dev_f32(w, "w"), _dev_f32(bias, "bias")
    n_rows, c = x.shape[0], x.shape[1] // 2
    y = torch.empty((n_rows, c), dtype=torch.float32, device=x.device)
    _call("rvc_glu_dwconv_silu_f32", _device(x, w, bias), x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), n_rows, c, w.shape[1])
    return y


def layernorm_rows(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """nn.LayerNorm over the last axis of x [..., F] (F a multiple of 64, <= 1024)."""
    x, gamma, beta = _dev_f32(x, "x"), _dev_f32(gamma, "gamma"), _dev_f32(beta, "beta")
    f = x.shape[-1]
    y = torch.empty_like(x)
    _call("rvc_layernorm_rows_f32", _device(x, gamma, beta), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), y.data_ptr(),
          x.numel() // f, f)
    return y


def groupnorm_lrelu(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float = 1e-5,
                    slope: float = 0.01) -> torch.Tensor:
    """leaky_relu(nn.GroupNorm(groups, C)(x), slope) for channel-major x [C, L]."""
    x = _dev_f32(x, "x")
    c, length = x.shape
    ws = _workspace("groupnorm", x.device, "rvc_groupnorm_workspace_bytes", c, length, groups)
    y = torch.empty_like(x)
    gamma, beta = _dev_f32(gamma, "gamma"), _dev_f32(beta, "beta")
    _call("rvc_groupnorm_lrelu_f32", _device(x, gamma, beta), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), groups, float(eps),
          float(slope), y.data_ptr(), c, length, ws.data_ptr(), ws.numel())
    return y


def fcpe_decode(logits: torch.Tensor, cent_table: torch.Tensor, out_dims: int, threshold: float, f0_min: float,
                want_latent: bool = False):
    """logits [n_rows, ld >= out_dims] -> (f0 [n_rows] fp32 in Hz, 0 = unvoiced; latent [n_rows, out_dims] or None)."""
    logits, cent_table = _dev_f32(logits, "logits"), _dev_f32(cent_table, "cent_table")
    n_rows, ld = logits.shape
    if cent_table.numel() != out_dims:
        raise NativeError(f"cent_table has {cent_table.numel()} entries, out_dims is {out_dims}")
    dev = _device(logits, cent_table)
    f0 = torch.empty(n_rows, dtype=torch.float32, device=dev)
    latent = torch.empty((n_rows, out_dims), dtype=torch.float32, device=dev) if want_latent else None
    _call("rvc_fcpe_decode_f32", dev, logits.data_ptr(), cent_table.data_ptr(), out_dims, ld, float(threshold), float(f0_min),
          f0.data_ptr(), _ptr(latent), n_rows)
    return f0, latent


# ---- K12: HuBERT's transformer GEMMs with both operands pre-split (csrc/linbf.hip) ---------------------------------------
def rows_padded(n_rows: int, tile: int = 128) -> int:
    return -(-n_rows // tile) * tile


def planes_empty(n_rows: int, features: int, device) -> torch.Tensor:
    """Uninitialised [3][rows_padded][features] bf16 planes (the padding rows are never read into a stored result)."""
    return torch.empty((3, rows_padded(n_rows), features), dtype=torch.bfloat16, device=device)


def split_rows_bf16x3(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [n_rows, k] -> three bf16 planes whose sum is x exactly."""
    x = _dev_f32(x, "x")
    n_rows, k = x.shape
    xs = out if out is not None else planes_empty(n_rows, k, x.device)
    _call("rvc_split_rows_bf16x3", _device(x, xs), x.data_ptr(), xs.data_ptr(), n_rows, xs.shape[1], k)
    return xs


def linear_bf16x3_presplit(xs: torch.Tensor, a_packed: torch.Tensor, bias, n_rows: int, out_features: int, mode: str = "f32",
                           k_parts: int = 1, out: torch.Tensor | None = None) -> torch.Tensor:
    """mode "f32": y [n_rows, out] = x W^T + b; "gelu_planes": planes of gelu(x W^T + b); "parts": [k_parts, n_rows, out] partial sums."""
    _, n_pad, in_features = xs.shape
    m = {"f32": 0, "gelu_planes": 1, "parts": 2, "gelu_f32": 3}[mode]
    if m in (0, 3):
        y = out if out is not None else torch.empty((n_rows, out_features), dtype=torch.float32, device=xs.device)
    elif m == 1:
        # (the output planes share n_rows_padded with the input planes: sized by xs, not by n_rows, or a caller whose planes are
        # longer than rows_padded(n_rows) would have planes 1 and 2 written past the end)
        y = out if out is not None else torch.empty((3, n_pad, out_features), dtype=torch.bfloat16, device=xs.device)
    else:
        y = out if out is not None else torch.empty((k_parts, n_rows, out_features), dtype=torch.float32, device=xs.device)
    _call("rvc_linear_bf16x3_presplit", _device(xs, a_packed, bias, y), xs.data_ptr(), a_packed.data_ptr(), _ptr(bias),
          y.data_ptr() if m != 1 else None, y.data_ptr() if m == 1 else None, n_rows, n_pad, in_features, out_features, m, k_parts)
    return y


def posconv_bf16x3_pack_weight(w: torch.Tensor, groups: int, device) -> torch.Tensor:
    """conv.weight [D, D / groups, taps] (weight norm folded) -> K14's fragment slab in HBM."""
    w = _host(w)
    return _pack_slab("rvc_posconv_bf16x3", device, (w,), (w.shape[0], groups, w.shape[2]))


def posconv_gelu_bf16x3(x: torch.Tensor, a_packed: torch.Tensor, bias, groups: int, taps: int, padding: int) -> torch.Tensor:
    """gelu(grouped Conv1d over the frames of x [T, D], output frames 0 .. T - 1) -> [T, D] fp32."""
    x = _dev_f32(x, "x")
    t, d = x.shape
    y = torch.empty_like(x)
    _call("rvc_posconv_gelu_bf16x3", _device(x, a_packed, bias), x.data_ptr(), a_packed.data_ptr(), _ptr(bias), y.data_ptr(), t, d, groups,
          taps, padding)
    return y


def hubert_conv0_frames_bf16x3(wav: torch.Tensor, w: torch.Tensor, gamma, beta, eps: float, stride: int = 5) -> tuple[torch.Tensor, int]:
    """HuBERT's first feature-extractor layer (Conv1d(1, C, 10, stride 5) -> GroupNorm(C, C) -> GELU) of ONE clip wav [n] ->
    (time-major planes [3, frames_padded, C], frames)."""
    wav = _dev_f32(wav, "wav")
    w2 = _dev_f32(w.reshape(w.shape[0], -1), "w")
    dev = _device(wav, w2, gamma, beta)
    c, taps = w2.shape
    n = wav.numel()
    frames = (n - taps) // stride + 1
    ys = planes_empty(frames, c, dev)
    ws = _workspace("hubert_conv0", dev, "rvc_hubert_conv0_workspace_bytes", c)
    _call("rvc_hubert_conv0_frames_bf16x3", dev, wav.data_ptr(), n, w2.data_ptr(), c, taps, stride, _ptr(gamma), _ptr(beta), float(eps),
          ws.data_ptr(), ws.numel(), ys.data_ptr(), ys.shape[1])
    return ys, frames


def conv1d_frames_bf16x3(xs: torch.Tensor, n_frames_in: int, a_packed: torch.Tensor, bias, out_channels: int, taps: int, stride: int,
                         mode: str = "gelu_planes") -> tuple[torch.Tensor, int]:
    """nn.Conv1d(C, out, taps, stride, no padding) (+ GELU) over time-major planes xs [3, frames_in_padded, C] ->
    (planes [3, frames_out_padded, out] or fp32 [frames_out, out], frames_out).  a_packed: gemm_bf16x3_pack_weight of
    conv.weight.permute(0, 2, 1).reshape(out, taps * C)."""
    _, n_pad_in, c = xs.shape
    m = {"f32": 0, "gelu_planes": 1, "gelu_f32": 3}[mode]
    frames = (n_frames_in - taps) // stride + 1
    if frames <= 0:
        raise NativeError("conv1d_frames_bf16x3: the input is shorter than one window")
    y = planes_empty(frames, out_channels, xs.device) if m == 1 else torch.empty((frames, out_channels), dtype=torch.float32, device=xs.device)
    _call("rvc_conv1d_frames_bf16x3", _device(xs, a_packed, bias), xs.data_ptr(), n_frames_in, n_pad_in, c, taps, stride, a_packed.data_ptr(),
          _ptr(bias), y.data_ptr() if m != 1 else None, y.data_ptr() if m == 1 else None, rows_padded(frames), out_channels, m)
    return y, frames


def bias_residual_layernorm_bf16x3(parts: torch.Tensor, bias, res, gamma, beta, eps: float, want_planes: bool = True,
                                   y: torch.Tensor | None = None, ys: torch.Tensor | None = None):
    """LayerNorm(sum(parts) + bias + res) -> (fp32 [n_rows, m], planes or None)."""
    n_parts, n_rows, m = parts.shape
    y = y if y is not None else torch.empty((n_rows, m), dtype=torch.float32, device=parts.device)
    if want_planes and ys is None:
        ys = planes_empty(n_rows, m, parts.device)
    _call("rvc_bias_residual_layernorm_bf16x3", _device(parts, bias, res, gamma, beta, y, ys), parts.data_ptr(), n_parts, _ptr(bias),
          _ptr(res), _ptr(gamma), _ptr(beta), float(eps), y.data_ptr(), _ptr(ys), n_rows, ys.shape[1] if ys is not None else n_rows, m)
    return y, ys


def conv1d_bf16x3(x: torch.Tensor, a_packed: torch.Tensor, bias, c_out: int, k: int, stride: int = 1, padding: int = 0,
                  act: str = "none") -> torch.Tensor:
    """nn.Conv1d(c_in, c_out, k, stride, padding) + activation for x [batch, c_in, L] (fp32, HBM, contiguous)."""
    x = _dev_f32(x, "x")
    b, c_in, l_in = x.shape
    l_out = max((l_in + 2 * padding - k) // stride + 1, 0)
    y = torch.empty((b, c_out, l_out), dtype=torch.float32, device=x.device)
    if y.numel() == 0:   # an input shorter than one window: an empty result, and no call with an empty tensor's NULL pointer
        return y
    _call("rvc_conv1d_bf16x3", _device(x, a_packed, bias), x.data_ptr(), a_packed.data_ptr(), _ptr(bias), y.data_ptr(), b, c_in, c_out, l_in,
          k, stride, padding, {"none": 0, "gelu": 1}[act])
    return y


# ---- K10 / K10b: conv2d 3x3 / 1x1 of the RMVPE U-Net, in fp32 and as exact bf16x3 products on the bf16 matrix cores ----------
def conv2d_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    """torch conv2d weight [C_out, C_in, kh, kw] (3x3 or 1x1) -> packed taps in HBM."""
    w = _host(w)
    device = _cuda_device(device)
    out = torch.empty(_size("rvc_conv2d_packed_floats", device, *w.shape), dtype=torch.float32, device=device)
    _call("rvc_conv2d_pack_weight", device, w.data_ptr(), *w.shape, out.data_ptr())
    return out


def conv2d_supported(c_in: int, width: int) -> bool:
    return c_in % 8 == 0 and 4 <= width <= 128 and width & (width - 1) == 0


def conv2d_bf16x3_supported(c_in: int, c_out: int, height: int, width: int) -> bool:
    return bool(_lib.rvc_conv2d_bf16x3_supported(c_in, c_out, height, width))


def conv2d_bf16x3_packable(c_in: int, c_out: int) -> bool:
    m_pad = (c_out + 31) // 32 * 32
    return c_in % 16 == 0 and (m_pad in (32, 64) or m_pad % 128 == 0)


def conv2d_bf16x3_pack_weight(w: torch.Tensor, device) -> torch.Tensor:
    """torch conv2d weight [C_out, C_in, 3, 3] -> bf16x3 tap fragments in HBM (int16 words)."""
    w = _host(w)
    return _pack_slab("rvc_conv2d_bf16x3", device, (w,), tuple(w.shape))


def _conv2d(stem: str, x, w_packed, bias, c_out, taps: tuple, relu, res, out):
    """<stem>_forward with the scratch <stem>_workspace_bytes asks for (none at all for most shapes); taps: (kh, kw), or () for the
    entry point that is 3x3 only."""
    x = _dev_f32(x, "x")
    b, c_in, h, wd = x.shape
    y = out if out is not None else torch.empty((b, c_out, h, wd), dtype=torch.float32, device=x.device)
    dev = _device(x, w_packed, bias, res, y)
    need = _size(stem + "_workspace_bytes", dev, b, c_in, c_out, h, wd, *taps)
    ws = _ws.get("conv2d", need, dev) if need else None
    _call(stem + "_forward", dev, x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(res), y.data_ptr(), b, c_in, c_out, h, wd, *taps,
          1 if relu else 0, _ptr(ws), need)
    return y


def conv2d_forward(x, w_packed, bias, c_out, ksize=3, relu=False, res=None, out=None):
    """y = act(conv2d(x, w, padding=ksize // 2) + bias) + res  (x [B, C_in, H, W] float32 on the device)."""
    return _conv2d("rvc_conv2d", x, w_packed, bias, c_out, (ksize, ksize), relu, res, out)


def conv2d_bf16x3_forward(x, u, bias, c_out, relu=False, res=None, out=None):
    """y = act(conv2d(x, w, padding=1) + bias) + res  (x [B, C_in, H, W] float32 on the device; u from conv2d_bf16x3_pack_weight)."""
    return _conv2d("rvc_conv2d_bf16x3", x, u, bias, c_out, (), relu, res, out)


# ---- K2/K3 -----------------------------------------------------------------------------------------
DEC_KINDS = {"HiFi-GAN": 0, "MRF HiFi-GAN": 1, "RefineGAN": 2}
DEC_ARITHMETIC = {"exact": 0, "fp16x2": 1}


def _decoder_config(vocoder, sr, *, in_channels=192, upsample_initial_channel=512, gin_channels=256,
                    upsample_rates=(12, 10, 2, 2), upsample_kernel_sizes=(24, 20, 4, 4), res_kernel_sizes=(3, 7, 11),
                    res_dilations=(1, 3, 5), weight_storage: str = "f32") -> DecoderConfig:
    cfg = DecoderConfig()
    cfg.kind = DEC_KINDS[vocoder]
    cfg.sample_rate = sr
    cfg.in_channels = in_channels
    cfg.upsample_initial_channel = upsample_initial_channel
    cfg.gin_channels = gin_channels
    cfg.n_ups = len(upsample_rates)
    for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
        cfg.upsample_rates[i] = int(u)
        cfg.upsample_kernel_sizes[i] = int(k)
    cfg.n_res_kernels = len(res_kernel_sizes)
    for i, k in enumerate(res_kernel_sizes):
        cfg.res_kernel_sizes[i] = int(k)
    cfg.weight_storage = {"f32": 0, "bf16": 1}[weight_storage]
    cfg.n_res_dilations = len(res_dilations)
    for i, d in enumerate(res_dilations):
        cfg.res_dilations[i] = int(d)
    return cfg


def _window_margin(cfg: DecoderConfig) -> int:
    frames = c_int()
    _check(_lib.rvc_decoder_window_margin(ctypes.byref(cfg), ctypes.byref(frames)), "rvc_decoder_window_margin")
    return frames.value


def decoder_window_margin(vocoder: str, sr: int = 48000, **config) -> int:
    """rvc_decoder_window_margin for a vocoder configuration (Decoder's keyword arguments): input frames on each side that an
    output frame depends on; -1 for RefineGAN (not covered).  A host computation: needs no device."""
    return _window_margin(_decoder_config(vocoder, sr, **config))


class Decoder:
    """Handle on the library's vocoder: weights are repacked into one device's HBM once, forward() launches the chain there."""

    def __init__(self, vocoder: str, sr: int, folded_weights: dict, *, in_channels=192, upsample_initial_channel=512,
                 gin_channels=256, upsample_rates=(12, 10, 2, 2), upsample_kernel_sizes=(24, 20, 4, 4),
                 res_kernel_sizes=(3, 7, 11), res_dilations=(1, 3, 5), weight_storage: str = "f32",
                 arithmetic: str = "exact", device=None):
        """arithmetic: "exact" (default), or "fp16x2" -- the square 128- / 256-channel ResBlock convs on error-corrected fp16
        pairs (K3h): the fp32 result to ~2^-22 per product, faster; not with weight_storage="bf16".
        device: where the weights live and forward() runs (None: the current device)."""
        if not torch.cuda.is_available():
            raise NativeError("rvc_amd.Decoder needs a HIP device (no CPU fallback)")
        if arithmetic not in DEC_ARITHMETIC:
            raise NativeError(f"rvc_amd.Decoder: arithmetic must be one of {sorted(DEC_ARITHMETIC)}, got {arithmetic!r}")
        cfg = self._cfg = _decoder_config(vocoder, sr, in_channels=in_channels, upsample_initial_channel=upsample_initial_channel,
                                          gin_channels=gin_channels, upsample_rates=upsample_rates,
                                          upsample_kernel_sizes=upsample_kernel_sizes, res_kernel_sizes=res_kernel_sizes,
                                          res_dilations=res_dilations, weight_storage=weight_storage)
        self.device = _cuda_device(device)
        self._h = c_void_p()
        self.vocoder = vocoder
        _check(_lib.rvc_decoder_create(ctypes.byref(cfg), ctypes.byref(self._h)), "rvc_decoder_create")
        self.arithmetic = arithmetic
        if arithmetic != "exact":   # (the default handle makes exactly the calls it always made)
            _check(_lib.rvc_decoder_set_arithmetic(self._h, DEC_ARITHMETIC[arithmetic]), "rvc_decoder_set_arithmetic")
        for name, t in folded_weights.items():
            t = _host(t)
            shape = (c_int64 * t.dim())(*t.shape)
            _check(_lib.rvc_decoder_set_tensor(self._h, name.encode(), t.data_ptr(), shape, t.dim()),
                   f"rvc_decoder_set_tensor({name})")
        with torch.cuda.device(self.device):   # rvc_decoder_finalize allocates and uploads, and takes no stream
            _check(_lib.rvc_decoder_finalize(self._h), "rvc_decoder_finalize")
        self.upp = _lib.rvc_decoder_upp(self._h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:  # _lib is None during interpreter shutdown
            _lib.rvc_decoder_destroy(h)
            self._h = None

    def set_concurrency_hint(self, utterances_in_flight: int):
        _check(_lib.rvc_decoder_set_concurrency_hint(self._h, int(utterances_in_flight)), "rvc_decoder_set_concurrency_hint")

    def set_branch_parallel(self, side_streams: int):
        """ResBlock branches of a short stage on this many side streams of the handle (-1: one per branch after the first;
        0, the default: every launch on the caller's stream)."""
        _check(_lib.rvc_decoder_set_branch_parallel(self._h, int(side_streams)), "rvc_decoder_set_branch_parallel")

    def set_tap(self, stage: int, tap: torch.Tensor | None):
        _check(_lib.rvc_decoder_set_tap(self._h, stage, _ptr(tap)), "rvc_decoder_set_tap")

    def window_margin(self) -> int:
        """Input frames on each side that an output frame depends on (rvc_decoder_window_margin); -1: RefineGAN, not covered."""
        return _window_margin(self._cfg)

    def forward(self, z: torch.Tensor, f0: torch.Tensor, g: torch.Tensor, *, src_randn: torch.Tensor,
                src_rand: torch.Tensor | None = None, adain_randn: torch.Tensor | None = None,
                keep: tuple | None = None) -> torch.Tensor:
        """keep = (lo, hi) in frames: only the samples [lo * upp, hi * upp) of the waveform, from the same full-length inputs
        (rvc_decoder_forward_window: the conv stack runs over those frames plus window_margin() on each side)."""
        z, f0, g, src_randn = _dev_f32(z, "z"), _dev_f32(f0, "f0"), _dev_f32(g, "g"), _dev_f32(src_randn, "src_randn")
        src_rand = _dev_f32(src_rand, "src_rand") if src_rand is not None else None
        adain_randn = _dev_f32(adain_randn, "adain_randn") if adain_randn is not None else None
        dev = self.device
        if _device(z, f0, g, src_randn, src_rand, adain_randn) != dev:
            raise NativeError(f"Decoder of {dev} got tensors on {z.device}")
        b, _, t = z.shape
        noise = DecoderNoise(_ptr(src_rand), src_randn.data_ptr(), _ptr(adain_randn))
        ws = _workspace("decoder", dev, "rvc_decoder_workspace_bytes", self._h, b, t)
        if keep is not None:
            lo, hi = int(keep[0]), int(keep[1])
            out = torch.empty((b, 1, max(hi - lo, 0) * self.upp), dtype=torch.float32, device=dev)
            _call("rvc_decoder_forward_window", dev, self._h, z.data_ptr(), f0.data_ptr(), g.data_ptr(), ctypes.byref(noise), b, t,
                  lo, hi, out.data_ptr(), ws.data_ptr(), ws.numel())
            return out
        out = torch.empty((b, 1, t * self.upp), dtype=torch.float32, device=dev)
        _call("rvc_decoder_forward", dev, self._h, z.data_ptr(), f0.data_ptr(), g.data_ptr(), ctypes.byref(noise), b, t,
              out.data_ptr(), ws.data_ptr(), ws.numel())
        return out
