"""argtypes/restype table for every symbol declared in include/fsnet_hip.h.  The CPU test
suite checks this table against the header and against the built library's exports."""
import ctypes as C

P = C.c_void_p
I = C.c_int
L = C.c_int64
F = C.c_float
D = C.c_double

SIGNATURES = {
    "fs_abi_version": (C.c_int, []),
    "fs_target_arch": (C.c_char_p, []),
    "fs_debug_timestamp": (C.c_int, [P, P]),
    "fs_capture_position": (C.c_int, [P, P]),
    "fs_conv_igemm": (C.c_int, [P, I, P]),
    # two problems per launch (ABI 7): (args0, args1 | NULL, dtype, stream)
    "fs_conv_igemm2": (C.c_int, [P, P, I, P]),
    "fs_conv3x3_halo2": (C.c_int, [P, P, I, P]),
    "fs_conv3x3_halo2_plan": (C.c_int, [P, P, I, P]),
    "fs_conv3x3_s2d": (C.c_int, [P, I, P]),
    "fs_conv3x3_s2d2": (C.c_int, [P, P, I, P]),
    "fs_conv_stem2": (C.c_int, [P, P, I, P]),
    "fs_conv_wgrad2": (C.c_int, [P, P, I, P]),
    "fs_conv_wgrad2_plan": (C.c_int, [P, P, I, P]),
    "fs_bn_apply2": (C.c_int, [P, P, I, P]),
    "fs_bn_bwd_reduce2": (C.c_int, [P, P, I, P]),
    "fs_bn_bwd_apply2": (C.c_int, [P, P, I, P]),
    "fs_maxpool_fwd2": (C.c_int, [P, P, P, I, P, P, P, I, I, I, I, I, P]),
    "fs_maxpool_bwd2": (C.c_int, [P, P, P, P, I, P, P, P, P, I, I, I, I, I, P]),
    "fs_conv3x3_halo": (C.c_int, [P, I, P]),
    "fs_conv3x3_halo_plan": (C.c_int, [P, I, P]),
    "fs_conv1x1": (C.c_int, [P, I, P]),
    "fs_conv_stem": (C.c_int, [P, I, P]),
    "fs_conv_wgrad": (C.c_int, [P, I, P]),
    "fs_conv_wgrad_plan": (C.c_int, [P, I, P]),
    "fs_pack_weights": (C.c_int, [P, P, I, I, I, I, I, I, L, I, I, P]),
    "fs_sigmoid_head_fwd": (C.c_int, [P, P, L, I, P]),
    "fs_sigmoid_head_bwd": (C.c_int, [P, P, P, L, I, I, P]),
    "fs_distill_fwd": (C.c_int, [P, P, P, L, P, P]),
    "fs_distill_bwd": (C.c_int, [P, P, P, L, P, P, P, P]),
    # added under ABI 15: is_unscaled_distill over 1..4 scales (FsDistillUnscaledArgs)
    "fs_distill_unscaled_fwd": (C.c_int, [P, P]),
    "fs_distill_unscaled_bwd": (C.c_int, [P, P]),
    "fs_distill_unscaled_workspace_bytes": (C.c_int64, [I, P, I]),
    "fs_distill_unscaled_chunk": (C.c_int, []),
    "fs_resize_linear":(C.c_int, [P, P, I, I, I, I, I, P]),
    "fs_depth_eval": (C.c_int, [P, P, I, I, I, I, I, P, P, P]),
    # ABI 14: Kitti360FisheyeEvaluator._single_loss (kitti360_fisheye_eval.py:43-72) and _precompute (:97-145)
    "fs_depth_eval_masked": (C.c_int, [P, P, P, I, I, I, I, I, F, F, I, P, P, P]),
    "fs_lidar_mei_depth": (C.c_int, [P, P, L, P, P, I, I, I, P, P, P, L, P]),
    "fs_lidar_mei_depth_workspace_bytes": (C.c_int64, [I, I, I]),
    # ABI 15: project_depth_map / generate_depth_map(vel_depth=True) (monodepth_utils.py:368-458)
    "fs_lidar_pinhole_depth": (C.c_int, [P, P, L, P, I, I, I, P, P, L, P]),
    "fs_lidar_pinhole_depth_workspace_bytes": (C.c_int64, [I, I, I]),
    # added under ABI 15: generate_depth_map + the uint16 cast of nuscenes_unsupervised_eval.py:85-126, :198
    "fs_lidar_nusc_depth_u16": (C.c_int, [P, P, L, P, I, I, I, I, P, P, L, P]),
    "fs_lidar_nusc_depth_workspace_bytes": (C.c_int64, [I, I, I, I]),
    # added under ABI 15: compute_errors of kitti_supervised_eval.py:7-81 and the depth writer that feeds it
    "fs_depth_errors9": (C.c_int, [P, P, I, I, D, I, I, I, P, L, P, P]),
    "fs_depth_errors9_workspace_bytes": (C.c_int64, [I, I, I]),
    "fs_depth_quantize_u16": (C.c_int, [P, P, F, I, I, P]),
    # added under ABI 15: ResnetEncoderMatching.match_features + confidence / lowest cost (resnet_matching.py:83-173, 227-237)
    "fs_cost_volume": (C.c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "fs_postopt": (C.c_int, [P, P]),
    "fs_postopt_workspace_bytes": (C.c_int64, [I, I, I, I]),
    "fs_optflow_farneback": (C.c_int, [P, P]),
    "fs_optflow_workspace_bytes": (C.c_int64, [P]),
    "fs_optflow_level_image": (C.c_int, [P, I, P, P]),
    "fs_motion_mask": (C.c_int, [P, P]),
    "fs_augment_masks": (C.c_int, [P, P, P, P, P, I, I, I, I, I, P]),
    "fs_copy_multi": (C.c_int, [P, P, P, I, P]),
    "fs_zero_multi": (C.c_int, [P, P, I, P]),
    "fs_pack_tile_blocks": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "fs_pack_weights_multi": (C.c_int, [P, I, L, I, P]),
    "fs_nchw_to_nhwc": (C.c_int, [P, P, P, I, I, I, I, I, I, I, P]),
    "fs_bn_apply": (C.c_int, [P, I, P]),
    "fs_bn_finalize": (C.c_int, [P, P, P, P]),
    "fs_bn_bwd_reduce": (C.c_int, [P, I, P]),
    "fs_bn_bwd_apply": (C.c_int, [P, I, P]),
    "fs_maxpool_fwd": (C.c_int, [P, P, P, I, I, I, I, I, P]),
    "fs_maxpool_bwd": (C.c_int, [P, P, P, P, I, I, I, I, I, P]),
    "fs_upcat_pad_fwd": (C.c_int, [P, P, P, I, I, I, I, I, I, P]),
    "fs_upcat_pad_bwd": (C.c_int, [P, P, P, I, I, I, I, I, I, P]),
    "fs_upcat_pad_bwd_bn": (C.c_int, [P, P, P, I, I, I, I, I, P, P, P, P, P, I, P]),
    "fs_channel_sum": (C.c_int, [P, P, L, I, I, I, P]),
    "fs_channel_sum_multi": (C.c_int, [P, P, P, P, P, I, I, P]),
    "fs_depth_head_fwd": (C.c_int, [P, P, P, P, L, I, I, F, F, P]),
    "fs_depth_head_bwd": (C.c_int, [P, P, P, P, P, L, I, I, F, F, I, P]),
    "fs_depth_head_fwd_multi": (C.c_int, [P, P, I, I, F, F, P]),
    "fs_depth_head_bwd_multi": (C.c_int, [P, P, I, I, F, F, I, P]),
    "fs_pose_tail_fwd": (C.c_int, [P, P, P, P, I, I, I, I, I, F, P]),
    "fs_pose_tail_bwd": (C.c_int, [P, P, P, I, I, I, I, I, F, I, P]),
    "fs_photo_setup": (C.c_int, [P, P, P, P, I, P, I, P]),
    "fs_mei_lut": (C.c_int, [P, I, I, F, F, F, F, D, D, D, P]),
    "fs_mei_stage_mask": (C.c_int, [P, P, P, I, I, I, P]),
    "fs_mei_points": (C.c_int, [P, P, P, I, I, I, P]),
    "fs_photo_identity": (C.c_int, [P, P]),
    # added under ABI 15: the row-walking identity kernel and its strip height
    "fs_photo_identity_rows": (C.c_int, [P, P]),
    "fs_photo_identity_strip_rows": (C.c_int, []),
    "fs_photo_fused_fwd": (C.c_int, [P, P]),
    "fs_photo_fused_bwd": (C.c_int, [P, P]),
    "fs_photo_fused_bwd_tiles": (C.c_int64, [I, I]),
    "fs_photo_pose_grad": (C.c_int, [P, P, P, P, I, I, I, P]),
    # added under ABI 15: the chain over 1..4 temporal source frames (FsPhotoMultiArgs)
    "fs_photo_multi_setup": (C.c_int, [P, P, I, P, I, P, P]),
    "fs_photo_multi_identity": (C.c_int, [P, P]),
    "fs_photo_multi_fwd": (C.c_int, [P, P]),
    "fs_photo_multi_bwd": (C.c_int, [P, P]),
    "fs_photo_multi_bwd_tiles": (C.c_int64, [I, I]),
    "fs_photo_multi_pose_grad": (C.c_int, [P, P, P, I, I, I, I, P]),
    "fs_photo_multi_strip": (C.c_int, [I, P, P]),
    # added under ABI 15: the same chain on the fisheye ray tables (FsPhotoMeiMultiArgs)
    "fs_photo_mei_multi_setup": (C.c_int, [P, I, P, I, P, P]),
    "fs_photo_mei_multi_fwd": (C.c_int, [P, P]),
    "fs_photo_mei_multi_bwd": (C.c_int, [P, P]),
    "fs_augment_frames": (C.c_int, [P, P]),
    "fs_resize_frames": (C.c_int, [P, P]),
    "fs_augment_frames_masked": (C.c_int, [P, P, P]),
    "fs_resize_frames_masked": (C.c_int, [P, P, P]),
    # added under ABI 15: the same launches with an output window and a colour op list (FsAugExtArgs)
    "fs_augment_frames_ext": (C.c_int, [P, P]),
    "fs_resize_frames_ext": (C.c_int, [P, P]),
    "fs_augment_masks_ext": (C.c_int, [P, P, P, P, P, I, I, I, I, I, P]),
    "fs_color_pyramid": (C.c_int, [P, P, I, I, I, I, I, P]),
    # added under ABI 15: (img, outs[n], hs[n], ws[n], n, B, H, W, stream) — all levels from one read of the image
    "fs_color_pyramid_multi": (C.c_int, [P, P, P, P, I, I, I, I, P]),
    "fs_smooth_mean": (C.c_int, [P, P]),
    "fs_smooth_fwd": (C.c_int, [P, P]),
    "fs_smooth_bwd": (C.c_int, [P, P]),
    "fs_loss_finalize": (C.c_int, [P, P, P, P, P, P, P]),
    "fs_sumsq": (C.c_int, [P, L, P, P, P]),
    "fs_counter_incr": (C.c_int, [P, P]),
    "fs_adam_step": (C.c_int, [P, P, P, P, L, F, F, F, F, F, I, F, P, F, P, P, P]),
    # added under ABI 15: the update launch with a run table (runs, n_runs before the stream) — AdamW / Adam-L2, SGD
    "fs_adamw_step": (C.c_int, [P, P, P, P, L, F, F, F, F, F, I, I, F, P, F, P, P, P, I, P]),
    "fs_sgd_step": (C.c_int, [P, P, P, L, F, F, F, I, F, I, F, P, F, P, P, P, I, P]),
    # added under ABI 15: deformable convolution v1 / v2 (FsDcnArgs; deform_conv.py:54-223)
    "fs_dcn_fwd": (C.c_int, [P, I, P]),
    "fs_dcn_bwd_data": (C.c_int, [P, I, P]),
    "fs_dcn_bwd_weight": (C.c_int, [P, I, P]),
    "fs_dcn_workspace_bytes": (C.c_int64, [P, I]),
    "fs_dcn_tile": (C.c_int, [I, P, P]),
    "fs_dcn_fwd_channels": (C.c_int, [P, I]),
    # added under ABI 15: the DLA backbone's 2x2 max pool and Root concatenation (FsCatArgs; dla.py:167, 207-208)
    "fs_pool2_fwd": (C.c_int, [P, P, P, I, I, I, I, L, L, I, P]),
    "fs_pool2_bwd": (C.c_int, [P, P, P, P, I, I, I, I, L, L, I, P]),
    "fs_cat_fwd": (C.c_int, [P, I, P]),
    "fs_cat_bwd": (C.c_int, [P, I, P]),
    # added under ABI 15: the ConvNeXt backbone's launches (FsDwconv7Args, FsLayerNormArgs, FsScaleResidualArgs; convnext.py)
    "fs_dwconv7_fwd": (C.c_int, [P, I, P]),
    "fs_dwconv7_bwd_weight": (C.c_int, [P, I, P]),
    "fs_dwconv7_workspace_bytes": (C.c_int64, [I, I, I, I]),
    "fs_dwconv7_tile": (C.c_int, [I, P, P, P]),
    "fs_layernorm_fwd": (C.c_int, [P, I, P]),
    "fs_layernorm_bwd": (C.c_int, [P, I, P]),
    "fs_layernorm_workspace_bytes": (C.c_int64, [L, I]),
    "fs_gelu_fwd": (C.c_int, [P, P, L, I, P]),
    "fs_gelu_bwd": (C.c_int, [P, P, P, L, I, P]),
    "fs_scale_residual_fwd": (C.c_int, [P, I, P]),
    "fs_scale_residual_bwd": (C.c_int, [P, I, P]),
    "fs_scale_residual_workspace_bytes": (C.c_int64, [L, I]),
    "fs_bias_grad": (C.c_int, [P, P, P, L, L, I, I, I, I, I, P]),
    "fs_patch_gather": (C.c_int, [P, P, I, I, I, I, I, I, P]),
    "fs_patch_scatter": (C.c_int, [P, P, I, I, I, I, I, I, P]),
}


def declare(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
