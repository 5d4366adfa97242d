"""ctypes binding of libvdx_hip.so (C-ABI declared in include/vdx.h).

The product path has no CPU fallback: if the library is missing or a symbol is absent,
loading raises.  Nothing here imports `oracle/`.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VDX_LIB_PATH") or os.path.join(_HERE, "libvdx_hip.so")   # override: dev/diagnostic builds


class GemmArgs(C.Structure):
    """Mirror of `vdx_gemm_args` (include/vdx.h)."""
    _fields_ = [
        ("a", C.c_void_p), ("a2", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
        ("bias2", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("mode", C.c_int32),
        ("c1", C.c_int32), ("c2", C.c_int32),
        ("lda", C.c_int32), ("lda2", C.c_int32), ("ldo", C.c_int32), ("ldr", C.c_int32),
        ("h_in", C.c_int32), ("w_in", C.c_int32), ("h_out", C.c_int32), ("w_out", C.c_int32),
        ("stride", C.c_int32), ("upsample", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32),
        ("rows_per_bias2", C.c_int32), ("ldb2", C.c_int32), ("epilogue", C.c_int32),
        ("row_begin", C.c_int32), ("row_end", C.c_int32),
        ("ksplit", C.c_int32), ("wset_rows", C.c_int32), ("workspace", C.c_void_p), ("wset_bias", C.c_void_p),
        ("workspace_bytes", C.c_size_t), ("pad_mode", C.c_int32),
    ]


class ClipPreprocessArgs(C.Structure):
    """Mirror of `vdx_clip_preprocess_args` (include/vdx.h)."""
    _fields_ = [
        ("frames", C.c_void_p), ("x_bounds", C.c_void_p), ("x_coeffs", C.c_void_p), ("y_bounds", C.c_void_p),
        ("y_coeffs", C.c_void_p), ("out", C.c_void_p), ("out_u8", C.c_void_p),
        ("frame_pitch", C.c_size_t), ("row_pitch", C.c_int32), ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("kx", C.c_int32), ("ky", C.c_int32), ("band", C.c_int32), ("span", C.c_int32), ("ldo", C.c_int32),
    ]


class TomeArgs(C.Structure):
    """Mirror of `vdx_tome_args` (include/vdx.h)."""
    _fields_ = [
        ("src_idx", C.c_void_p), ("dst_idx", C.c_void_p), ("inv", C.c_void_p), ("node_max", C.c_void_p),
        ("node_idx", C.c_void_p), ("slot", C.c_void_p), ("off", C.c_void_p), ("items", C.c_void_p),
        ("n_img", C.c_int32), ("S", C.c_int32), ("n_src", C.c_int32), ("n_dst", C.c_int32), ("r", C.c_int32), ("C", C.c_int32),
    ]


_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> (restype, argtypes): every symbol include/vdx.h declares
SIGNATURES = {
    "vdx_last_error": (C.c_char_p, []),
    "vdx_version": (_i, []),
    "vdx_build_flags": (_i, []),
    "vdx_gemm_f16": (_i, [C.POINTER(GemmArgs), _vp]),
    "vdx_gemm_plan": (_i, [C.POINTER(GemmArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vdx_gemm_kernel_name": (_i, [C.POINTER(GemmArgs), C.c_char_p, _sz]),
    "vdx_gemm_plan_ksplit": (_i, [C.POINTER(GemmArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "vdx_softmax_rows_f16": (_i, [_vp, _i, _i, _i, _f, _vp]),
    "vdx_rows_to_u8_frames": (_i, [_vp, _i, _sz, _vp, _vp]),
    "vdx_im2col_in_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "vdx_rows_to_ncfhw_f16": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "vdx_silu_f16": (_i, [_vp, _vp, _sz, _vp]),
    "vdx_groupnorm_workspace": (_sz, [_i, _i, _i, _i]),
    "vdx_groupnorm_f16": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _f, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "vdx_groupnorm_workspace_part": (_sz, [_i, _i, _i, _i, _i]),
    "vdx_groupnorm_part_f16": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _f, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "vdx_groupnorm_fold_linear_f16": (_i, [_vp, _i, _i, _vp, _vp, _f, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "vdx_groupnorm_stats_f16": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _f, _i, _i, _i, _vp, _i, C.POINTER(_sz), _vp]),
    "vdx_conv3x3_gn_supported": (_i, [_i, _i, _i]),
    "vdx_conv3x3_gn_preferred": (_i, [_i, _i, _i, _i, _i, _i]),
    "vdx_conv3x3_gn_f16": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "vdx_tconv_gn_supported": (_i, [_i, _i, _i]),
    "vdx_tconv_gn_preferred": (_i, [_i, _i, _i, _i, _i]),
    "vdx_tconv_gn_f16": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "vdx_layernorm_f16": (_i, [_vp, _i, _vp, _vp, _f, _i, _i, _vp, _i, _vp]),
    "vdx_flash_attn_f16": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "vdx_flash_attn_rows_f16": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "vdx_timestep_embedding_f16": (_i, [_vp, _vp, _i, _i, _vp]),
    "vdx_gelu_f16": (_i, [_vp, _vp, _sz, _vp]),
    "vdx_temporal_attn_f16": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "vdx_ff_block_supported": (_i, [_i]),
    "vdx_ff_block_pack_bytes": (_sz, [_i]),
    "vdx_ff_block_f16": (_i, [_vp, _i, _vp, _f, _vp, _i, _i, _i, _vp]),
    "vdx_ff_block_proj_pack_bytes": (_sz, [_i]),
    "vdx_ff_block_proj_f16": (_i, [_vp, _i, _vp, _f, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    "vdx_cross_attn_block_supported": (_i, [_i, _i]),
    "vdx_cross_attn_block_pack_bytes": (_sz, [_i]),
    "vdx_cross_attn_block_kv_bytes": (_sz, [_i]),
    "vdx_cross_attn_block_f16": (_i, [_vp, _i, _vp, _vp, _i, _f, _vp, _i, _i, _i, _i, _vp]),
    "vdx_temporal_attn_block_supported": (_i, [_i, _i]),
    "vdx_temporal_attn_block_wqkv_bytes": (_sz, [_i]),
    "vdx_temporal_attn_block_wo_bytes": (_sz, [_i]),
    "vdx_temporal_attn_block_f16": (_i, [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "vdx_temporal_attn_block2_supported": (_i, [_i, _i]),
    "vdx_temporal_attn_block2_pack_bytes": (_sz, [_i]),
    "vdx_temporal_attn_block2_f16": (_i, [_vp, _i, _vp, _f, _vp, _i, _i, _i, _i, _i, _vp]),
    "vdx_comm_unique_id": (_i, [_vp]),
    "vdx_comm_init": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "vdx_comm_destroy": (_i, [_vp]),
    "vdx_allgather_shard": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "vdx_halo_exchange": (_i, [_vp, _vp, _sz, _i, _vp, _sz, _i, _vp]),
    "vdx_ipc_export": (_i, [_vp, _vp, C.POINTER(_sz)]),
    "vdx_ipc_open": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "vdx_ipc_close": (_i, [_vp, _sz]),
    "vdx_peer_gather": (_i, [_vp, C.POINTER(_vp), _i, _sz, _vp]),
    "vdx_set_reserved_cus": (_i, [_i]),
    "vdx_reserved_cus": (_i, []),
    "vdx_persistent_grid_cus": (_i, []),
    "vdx_probe_mfma_f16": (_i, [_vp, _sz, _i, C.POINTER(C.c_double), _vp]),
    "vdx_probe_occupancy_hog": (_i, [_i, _i, _i, _vp]),
    "vdx_cfg_input_f16": (_i, [_vp, _vp, _f, _vp, _i, _i, _i, _vp]),
    "vdx_cfg_ddim_step_f16": (_i, [_vp, _vp, _vp, _f, _f, _f, _f, _f, _sz, _vp]),
    "vdx_ddim_step_f16": (_i, [_vp, _vp, _vp, _f, _f, _f, _f, _sz, _vp]),
    "vdx_cfg_dpm_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _sz, _vp]),
    "vdx_dpm_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _sz, _vp]),
    "vdx_blend_accumulate_f16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vdx_blend_finalize_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "vdx_clip_preprocess_u8": (_i, [C.POINTER(ClipPreprocessArgs), _vp]),
    "vdx_clip_vision_embed_f16": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _vp, _i, _vp]),
    "vdx_quick_gelu_f16": (_i, [_vp, _vp, _sz, _vp]),
    "vdx_clip_cosine_score_f16": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "vdx_resample_h_u8": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _sz, _i, _vp]),
    "vdx_resample_v_u8": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _sz, _i, _vp]),
    "vdx_frames_to_conv_in_u8": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "vdx_vae_posterior_f16": (_i, [_vp, _i, _i, _i, _vp, _i, _f, _vp, _sz, _sz, _vp]),
    "vdx_add_noise_f16": (_i, [_vp, _vp, _vp, _f, _f, _sz, _vp]),
    "vdx_lpips_stem_u8": (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    "vdx_relu_f16": (_i, [_vp, _vp, _sz, _vp]),
    "vdx_relu_maxpool_f16": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "vdx_im2col_f16": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "vdx_lpips_distance_f16": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "vdx_frame_stats_u8": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vdx_flow_grey_u8": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _vp]),
    "vdx_flow_corr1d_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp]),
    "vdx_flow_resize_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _f, _vp]),
    "vdx_flow_polyexp_f32": (_i, [_vp, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _vp, _vp]),
    "vdx_flow_update_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vdx_flow_abs_sum_f32": (_i, [_vp, _i, _sz, _vp, _vp, _vp]),
    "vdx_flow_remap_absdiff_u8": (_i, [_vp, _sz, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    # motion-compensated frame interpolation (no reference counterpart; vdx/interp.py, csrc/interp.hip)
    "vdx_interp_frames_u8": (_i, [_vp, _sz, _i, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    # full-reference clip comparison: SSE / SSIM / MS-SSIM (no reference counterpart; vdx/compare.py, csrc/compare.hip)
    "vdx_compare_tiles": (_i, [_i, _i]),
    "vdx_compare_ssim_scale_u8": (_i, [_vp, _sz, _i, _vp, _sz, _i, _i, _i, _i, C.POINTER(C.c_double), _vp, _vp, _vp]),
    "vdx_compare_ssim_scale_f32": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_double), _vp, _vp]),
    "vdx_compare_down2_u8": (_i, [_vp, _sz, _i, _vp, _sz, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vdx_compare_down2_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "vdx_compare_finalize": (_i, [_vp, _vp, _i, _i, C.c_double, _i, _vp, _vp, _vp]),
    # FreeInit's frequency mix (no reference counterpart; vdx/freeinit.py, csrc/freeinit.hip)
    "vdx_freeinit_workspace": (_sz, [_i, _i, _i, _i]),
    "vdx_freeinit_mix_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _vp]),
    # temporal co-denoising: window input and the fused whole-clip steps (no reference counterpart; vdx/codenoise.py, csrc/codenoise.hip)
    "vdx_cfg_input_window_f16": (_i, [_vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _vp]),
    "vdx_cofuse_cfg_ddim_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f, _f, _f, _i, _i, _i, _vp]),
    "vdx_cofuse_cfg_dpm_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i,
                                         _vp]),
    # spatially tiled co-denoising: a tile's input and the fused whole-clip steps over time x row x column windows (no reference
    # counterpart; vdx/codenoise.py, csrc/cotile.hip)
    "vdx_cfg_input_tile_f16": (_i, [_vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vdx_cotile_cfg_ddim_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _sz, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _f, _f, _f,
                                          _f, _f, _i, _i, _i, _i, _vp]),
    "vdx_cotile_cfg_dpm_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _sz, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _f,
                                         _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _vp]),
    # seamless looping: a ring window's input and the fused whole-clip steps over windows that wrap (no reference counterpart;
    # vdx/codenoise.py `loop_plan`, csrc/codenoise.hip, its RING flag)
    "vdx_cfg_input_loop_f16": (_i, [_vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _vp]),
    "vdx_coloop_cfg_ddim_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f, _f, _f, _i, _i, _i, _vp]),
    "vdx_coloop_cfg_dpm_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i,
                                         _vp]),
    # strided context windows: a strided window's input and the fused whole-clip steps over rows (off, s, L, d) (no reference
    # counterpart; vdx/codenoise.py `stride_plan`, csrc/codenoise.hip, its `costride_tab`)
    "vdx_cfg_input_stride_f16": (_i, [_vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "vdx_costride_cfg_ddim_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f, _f, _f, _i, _i, _i, _vp]),
    "vdx_costride_cfg_dpm_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _i, _i,
                                           _i, _vp]),
    # CFG rescale: the statistics pass and the fused steps, plain and co-fused (no reference counterpart; vdx/scheduler.py
    # `guidance_rescale`, csrc/rescale.hip)
    "vdx_cfg_rescale_rows": (_i, [_sz]),
    "vdx_cfg_rescale_stats_f16": (_i, [_vp, _sz, _f, _vp, _vp]),
    "vdx_cfg_rescale_ddim_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _sz, _vp]),
    "vdx_cfg_rescale_dpm_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _f, _f, _sz, _vp]),
    "vdx_cofuse_cfg_rescale_rows": (_i, [_i, _i]),
    "vdx_cofuse_cfg_rescale_stats_f16": (_i, [_vp, _sz, _vp, _vp, _vp, _i, _vp, _f, _vp, _i, _i, _i, _vp]),
    "vdx_cofuse_cfg_rescale_ddim_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _i,
                                                  _i, _i, _vp]),
    "vdx_cofuse_cfg_rescale_dpm_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f,
                                                 _f, _f, _f, _f, _i, _i, _i, _vp]),
    # dynamic thresholding with a mimic scale: the statistics pass (sums, histogram, select) and the fused steps, plain and
    # co-fused (no reference counterpart; vdx/scheduler.py `cfg_mimic`, csrc/dynthresh.hip)
    "vdx_cfg_mimic_ws_bytes": (_sz, [_i, _i, _i]),
    "vdx_cfg_mimic_stats_f16": (_i, [_vp, _i, _i, _i, _f, _f, _sz, _f, _vp, _i, _vp]),
    "vdx_cfg_mimic_ddim_step_f16": (_i, [_vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i, _i, _i, _vp]),
    "vdx_cfg_mimic_dpm_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _vp]),
    "vdx_cofuse_cfg_mimic_ws_bytes": (_sz, [_i, _i, _i]),
    "vdx_cofuse_cfg_mimic_stats_f16": (_i, [_vp, _sz, _vp, _vp, _vp, _i, _vp, _f, _f, _sz, _f, _vp, _i, _i, _i, _i, _vp]),
    "vdx_cofuse_cfg_mimic_ddim_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i, _i, _i, _vp]),
    "vdx_cofuse_cfg_mimic_dpm_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _i,
                                               _i, _i, _vp]),
    # masked video-to-video: the per-step select, the paste and the mask's two maps (no reference counterpart; vdx/inpaint.py,
    # csrc/inpaint.hip)
    "vdx_mask_renoise_f16": (_i, [_vp, _vp, _vp, _vp, _f, _f, _i, _i, _i, _i, _i, _i, _vp]),
    "vdx_mask_paste_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "vdx_mask_to_latent_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vdx_mask_composite_u8": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    # FreeU's skip filter and backbone scale (no reference counterpart; unet3d.py enable_freeu, csrc/freeu.hip)
    "vdx_freeu_filter_f16": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, C.c_double, _vp, _i, _vp]),
    "vdx_freeu_scale_f16": (_i, [_vp, _i, _sz, _i, _f, _vp]),
    # token merging around the spatial self-attention (no reference counterpart; unet3d.py enable_tome, vdx/tome.py, csrc/tome.hip)
    "vdx_tome_match_f16": (_i, [C.POINTER(TomeArgs), _vp, _i, _vp]),
    "vdx_tome_select_lds": (_sz, [_i, _i]),
    "vdx_tome_select": (_i, [C.POINTER(TomeArgs), _vp]),
    "vdx_tome_merge_f16": (_i, [C.POINTER(TomeArgs), _vp, _i, _vp, _i, _vp]),
    "vdx_tome_unmerge_add_f16": (_i, [C.POINTER(TomeArgs), _vp, _i, _vp, _i, _vp, _i, _vp]),
    # prompt travel: a window's per-frame text and K5's key / value blobs in one launch each (no reference counterpart; vdx/travel.py,
    # csrc/travel.hip)
    "vdx_text_travel_f16": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vdx_cross_attn_block_pack_kv_f16": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    # regional prompts: the per-pixel blend of the cross-attention sub-block's per-text results (no reference counterpart;
    # vdx/region.py, csrc/region.hip)
    "vdx_region_blend_f16": (_i, [C.POINTER(_vp), _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    # LoRA adapters merged into a weight in the diffusers layout (no reference counterpart; vdx/lora.py, csrc/lora.hip)
    "vdx_lora_merge_f16": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int32), C.POINTER(_f), _vp, _vp]),
    # prompt emphasis: per-token weights on the text encoder's output, mean restored (no reference counterpart; vdx/prompt.py,
    # csrc/prompt.hip)
    "vdx_prompt_weight_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    # Motion-JPEG decode (scoring.py:16, :110, :230, :272, :314 cv2.VideoCapture; cv2_shim.py:199-289 the writer)
    "vdx_mjpeg_workspace": (_sz, [_i, _i, _i, _i]),
    "vdx_mjpeg_entropy": (_i, [_vp, _sz, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vdx_mjpeg_idct": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vdx_mjpeg_color": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    # Motion-JPEG encode (fsdp_chunked_coherent.py:250-253 cv2.VideoWriter; cv2_shim.py VideoWriter.write the host path)
    "vdx_mjpeg_enc_workspace": (_sz, [_i, _i, _i, _i]),
    "vdx_mjpeg_enc_offsets": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "vdx_mjpeg_enc_color": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "vdx_mjpeg_enc_fdct": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "vdx_mjpeg_enc_entropy": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vdx_mjpeg_enc_pack": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    # animated GIF of a whole clip (no reference counterpart; vdx/gif.py, csrc/gif.hip)
    "vdx_gif_hist_u8": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _vp]),
    "vdx_gif_lut": (_i, [_vp, _i, _vp, _vp]),
    "vdx_gif_index_u8": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "vdx_gif_lzw_workspace": (_sz, [_i, _i, _i, _i]),
    "vdx_gif_lzw_offsets": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "vdx_gif_lzw": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vdx_gif_pack": (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    # the portable seeded noise generator (no reference counterpart; vdx/noise.py, csrc/noise.hip)
    "vdx_noise_f16": (_i, [_sz, _sz, _i, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), _f, _vp, _vp]),
    "vdx_noise_f32": (_i, [_sz, _sz, _i, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), _vp, _vp]),
    "vdx_noise_form": (_i, [_i, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]),
    # stochastic sampling: the one-buffer and co-fused steps with the generator's draw inside (no reference counterpart;
    # vdx/scheduler.py, csrc/dpm.hip, csrc/codenoise.hip, csrc/step_noise.h)
    "vdx_cfg_ddim_eta_step_f16": (_i, [_vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _sz, _sz, _i, _i, _i, _i, _i, _vp]),
    "vdx_ddim_eta_step_f16": (_i, [_vp, _vp, _vp, _f, _f, _f, _f, _f, _sz, _sz, _i, _i, _i, _i, _i, _vp]),
    "vdx_cfg_sde_dpm_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _f, _sz, _sz, _i, _i, _i, _i, _i, _vp]),
    "vdx_sde_dpm_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _sz, _sz, _i, _i, _i, _i, _i, _vp]),
    "vdx_cofuse_cfg_ddim_eta_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f, _f, _f, _f, _sz, _sz, _i, _i, _i,
                                              _vp]),
    "vdx_cofuse_cfg_sde_dpm_step_f16": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _f, _sz,
                                             _sz, _i, _i, _i, _vp]),
}

_lib = None


def source_sha() -> str:
    """sha256 over the kernel sources (csrc/*.hip, *.h, include/vdx.h): the identity of the build a profile was
    taken on.  `.git` does not travel to the GPU box, so profiles/ records this instead of a commit id."""
    import glob
    import hashlib
    hsh = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "vdx.h"))
    for f in files:
        hsh.update(os.path.basename(f).encode())
        hsh.update(open(f, "rb").read())
    return hsh.hexdigest()[:16]


class VdxError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the HIP library; raise loudly when it is not built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VdxError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the denoising path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    flags = lib.vdx_build_flags()
    if flags and os.environ.get("VDX_ALLOW_LAB_BUILD") != "1":
        # VDX_LIB_PATH must not slip a stamps / ablation build (timing-only code paths, some with wrong results) into the product
        raise VdxError(f"{LIB_PATH} was built with lab macros (vdx_build_flags() = {flags}): not a parity build. "
                       "Lab tools set VDX_ALLOW_LAB_BUILD=1; the product path never does.")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().vdx_last_error()
        raise VdxError(f"{what}: {msg.decode() if msg else 'error'} (rc={rc})")
