"""ctypes binding of libdfnet_hip.so (include/dfnet_hip.h).

The library is the product: there is NO fallback.  If it is missing or fails to load,
importing callers get a RuntimeError telling them how to build it.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

LIB_PATH = os.environ.get("DFN_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdfnet_hip.so")

DFN_PREC_F16 = 0
DFN_PREC_F32 = 1
DFN_PREC_F16X3 = 2  # DFNet only: split-f16 (fp32-grade results at f16 MFMA rate)
DFN_NET_COARSE, DFN_NET_FINE = 0, 1   # dfn_nerfh_points_train_*: the network a training query on points evaluates
PRECISIONS = {"f16": DFN_PREC_F16, "fp16": DFN_PREC_F16, "f32": DFN_PREC_F32, "fp32": DFN_PREC_F32, "f16x3": DFN_PREC_F16X3}

COMP_TEST_TIME, COMP_STATIC_ONLY, COMP_WHITE_BKGD = 1, 2, 4
COMP_COARSE = 16   # typ == "coarse" (dfn_raw2outputs)
RENDER_LINDISP, RENDER_COARSE_F16 = 1, 2


class DfnError(RuntimeError):
    pass


class NerfhDesc(Structure):
    _fields_ = [("depth", c_int), ("width", c_int), ("multires", c_int), ("multires_views", c_int),
                ("hist_bin", c_int), ("dim_a", c_int), ("dim_t", c_int), ("n_vocab", c_int)]


class AdamTensor(Structure):
    """dfn_adam_tensor (include/dfnet_hip.h)"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("numel", c_size_t),
                ("step_size", c_float), ("bias_correction2_sqrt", c_float)]


class RenderMaps(Structure):
    """dfn_render_maps (include/dfnet_hip.h): optional per-ray outputs of the *_maps entries, NULL = not wanted"""
    _fields_ = [("depth", c_void_p), ("depth_static", c_void_p), ("beta", c_void_p), ("rgb_static", c_void_p),
                ("rgb_transient", c_void_p)]


class MapGrads(Structure):
    """dfn_map_grads (include/dfnet_hip.h): upstream gradients of the compositor's outputs, NULL = zero"""
    _fields_ = [("rgb", c_void_p), ("acc", c_void_p), ("depth", c_void_p), ("depth_static", c_void_p), ("disp", c_void_p),
                ("beta", c_void_p), ("rgb_static", c_void_p), ("rgb_transient", c_void_p)]


class Raw2OutputsGrads(Structure):
    """dfn_raw2outputs_grads (include/dfnet_hip.h): upstream gradients of what raw2outputs_NeRFW returns, NULL = zero"""
    _fields_ = [("rgb", c_void_p), ("disp", c_void_p), ("acc", c_void_p), ("weights", c_void_p), ("depth", c_void_p), ("beta", c_void_p)]


class TrainMapGrads(Structure):
    """dfn_train_map_grads (include/dfnet_hip.h): upstream gradients of every output of the training render, NULL = zero"""
    _fields_ = [("rgb", c_void_p), ("disp", c_void_p), ("acc", c_void_p), ("depth", c_void_p), ("beta", c_void_p), ("rgb0", c_void_p),
                ("disp0", c_void_p), ("acc0", c_void_p), ("depth0", c_void_p)]


class FrameMapsOut(Structure):
    """dfn_frame_maps_out (include/dfnet_hip.h): quantised planes of dfn_frame_post_maps, NULL = not wanted"""
    _fields_ = [("depth16", c_void_p), ("depth_static16", c_void_p), ("beta8", c_void_p), ("rgb_static8", c_void_p),
                ("rgb_transient8", c_void_p)]


MAP_NAMES = tuple(n for n, _ in RenderMaps._fields_)   # trailing shape: () for the first three, (3,) for the rgb_* maps


# name -> (restype, argtypes); mirrors include/dfnet_hip.h one to one
_P = c_void_p
SIGNATURES = {
    "dfn_last_error": (c_char_p, []),
    "dfn_abi_version": (c_int, []),
    "dfn_nerfh_create": (c_int, [POINTER(NerfhDesc), POINTER(c_void_p)]),
    "dfn_nerfh_destroy": (c_int, [_P]),
    "dfn_nerfh_set_param": (c_int, [_P, c_char_p, _P, c_size_t]),
    "dfn_nerfh_commit": (c_int, [_P]),
    "dfn_nerfh_recommit_device": (c_int, [_P, _P, _P]),
    "dfn_nerfh_packed_buffer": (c_int, [_P, c_int, POINTER(c_char_p), POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float)]),
    "dfn_nerfh_recommit_selfcheck": (c_int, [c_int]),
    "dfn_feature_cosine_state_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfn_feature_cosine_forward": (c_int, [_P, c_size_t, _P, c_size_t, _P, c_int, c_int, c_int, c_size_t, _P, _P, c_size_t, _P]),
    "dfn_feature_cosine_backward": (c_int, [_P, c_size_t, _P, c_size_t, _P, c_int, c_int, c_int, c_size_t, _P, _P, _P, c_size_t, _P]),
    "dfn_dm_loss_scratch_bytes": (c_size_t, []),
    "dfn_dm_loss_forward": (c_int, [_P, _P, c_size_t, _P, _P, c_int, _P, c_float, c_float, c_float, _P, _P, _P]),
    "dfn_dm_loss_backward": (c_int, [_P, _P, c_size_t, _P, _P, c_int, c_float, c_float, c_float, _P, _P, _P, _P, _P]),
    "dfn_nerfh_set_render_options": (c_int, [_P, c_int]),
    "dfn_nerfh_range_status": (c_int, [_P, POINTER(c_int), _P]),
    "dfn_nerfh_range_status_async": (c_int, [_P, _P, _P]),
    "dfn_ndc_rays": (c_int, [c_int, c_int, c_float, c_float, _P, _P, c_size_t, _P, _P, _P]),
    # models/ray_utils.py:27-44 and rendering.py:364-371 under autograd: the adjoints of ndc_rays and of viewdirs = d / |d|
    "dfn_ndc_rays_backward": (c_int, [c_int, c_int, c_float, c_float, _P, _P, c_size_t, _P, _P, _P, _P, _P]),
    "dfn_viewdirs_backward": (c_int, [_P, _P, c_size_t, c_int, _P, _P]),
    "dfn_sample_fine_opt": (c_int, [_P, c_size_t, c_int, c_int, c_float, c_float, c_int, _P, _P, _P, _P]),
    "dfn_raygen": (c_int, [c_int, c_int, c_float, _P, _P, _P, _P, _P]),
    "dfn_raygen_frames": (c_int, [c_int, c_int, c_int, c_float, _P, _P, _P, _P, _P]),
    "dfn_posenc": (c_int, [_P, c_size_t, c_int, c_int, _P, _P]),
    "dfn_mlp_coarse": (c_int, [_P, c_int, _P, _P, c_size_t, c_int, c_float, c_float, _P, _P]),
    "dfn_coarse_weights": (c_int, [_P, _P, c_size_t, c_int, _P, _P]),
    "dfn_sample_pdf": (c_int, [_P, _P, c_size_t, c_int, c_int, _P, _P, _P]),
    "dfn_sample_pdf_backward": (c_int, [_P, _P, c_size_t, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "dfn_sample_fine": (c_int, [_P, c_size_t, c_int, c_int, c_float, c_float, _P, _P, _P, _P]),
    "dfn_fine_bias_bytes": (c_size_t, [c_size_t]),
    "dfn_mlp_fine": (c_int, [_P, c_int, _P, _P, _P, _P, c_size_t, c_size_t, _P, c_int, _P, _P, _P]),
    "dfn_composite_fine": (c_int, [_P, _P, c_size_t, c_int, c_float, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "dfn_render_workspace_bytes": (c_size_t, [c_size_t, c_int, c_int]),
    "dfn_render_rays": (c_int, [_P, c_int, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float,
                                _P, _P, _P, _P, _P, c_size_t, _P]),
    "dfn_render_image": (c_int, [_P, c_int, _P, c_int, c_int, c_float, c_float, c_float, c_int, c_int, _P,
                                 _P, _P, _P, _P, c_size_t, _P]),
    "dfn_render_maps_workspace_bytes": (c_size_t, [c_size_t, c_int, c_int]),
    "dfn_render_rays_maps": (c_int, [_P, c_int, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float,
                                     _P, _P, _P, _P, _P, c_size_t, POINTER(RenderMaps), _P]),
    "dfn_render_image_maps": (c_int, [_P, c_int, _P, c_int, c_int, c_float, c_float, c_float, c_int, c_int, _P,
                                      _P, _P, _P, _P, c_size_t, POINTER(RenderMaps), _P]),
    "dfn_composite_fine_maps": (c_int, [_P, _P, c_size_t, c_int, c_float, POINTER(RenderMaps), _P]),
    "dfn_composite_fine_backward": (c_int, [_P, _P, _P, c_size_t, c_int, _P, _P]),
    "dfn_composite_fine_backward_maps": (c_int, [_P, _P, c_size_t, c_int, c_float, POINTER(MapGrads), _P, _P, _P]),
    # models/rendering.py:132-243 raw2outputs_NeRFW as a stage, forward and backward w.r.t. raw and z_vals
    "dfn_raw2outputs": (c_int, [_P, c_int, _P, _P, c_float, c_size_t, c_int, c_float, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "dfn_raw2outputs_backward": (c_int, [_P, c_int, _P, _P, c_float, c_size_t, c_int, c_float, c_int, POINTER(Raw2OutputsGrads), _P, _P,
                                         _P]),
    "dfn_mlp_fine_backward": (c_int, [_P, c_int, _P, _P, _P, _P, c_size_t, c_size_t, _P, c_int, _P, _P, _P, _P]),
    "dfn_mlp_fine_mask_bytes": (c_size_t, [c_size_t]),
    "dfn_mlp_fine_saving": (c_int, [_P, c_int, _P, _P, _P, _P, c_size_t, c_size_t, _P, c_int, _P, _P, _P, _P]),
    "dfn_mlp_fine_backward_saved": (c_int, [_P, c_int, _P, _P, _P, c_size_t, _P, c_int, _P, _P, _P, _P, _P]),
    "dfn_mlp_coarse_points": (c_int, [_P, c_int, _P, c_size_t, c_int, _P, _P]),
    "dfn_mlp_fine_points": (c_int, [_P, c_int, _P, _P, _P, c_size_t, c_size_t, c_int, _P, _P, _P]),
    "dfn_mlp_fine_points_backward": (c_int, [_P, c_int, _P, _P, _P, c_size_t, c_size_t, c_int, _P, _P, _P, _P]),
    "dfn_mlp_coarse_points_backward": (c_int, [_P, c_int, _P, c_size_t, c_int, _P, _P, _P]),
    "dfn_mlp_coarse_static_points": (c_int, [_P, c_int, _P, _P, c_size_t, c_int, _P, _P, _P]),
    "dfn_mlp_coarse_static_points_backward": (c_int, [_P, c_int, _P, _P, c_size_t, c_int, _P, _P, _P, _P]),
    "dfn_ray_grad_reduce": (c_int, [_P, _P, _P, c_size_t, c_int, c_int, _P, _P, _P, _P]),
    "dfn_raygen_backward": (c_int, [c_int, c_int, c_float, _P, _P, _P, _P]),
    "dfn_raygen_frames_backward": (c_int, [c_int, c_int, c_int, c_float, _P, _P, _P, _P]),
    "dfn_render_backward_workspace_bytes": (c_size_t, [c_size_t, c_int, c_int]),
    "dfn_render_rays_backward": (c_int, [_P, c_int, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float,
                                         _P, _P, _P, _P, _P, c_size_t, _P]),
    "dfn_render_image_backward": (c_int, [_P, c_int, _P, c_int, c_int, c_float, c_float, c_float, c_int, c_int, _P,
                                          _P, _P, _P, c_size_t, _P]),
    "dfn_upsample_bicubic": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "dfn_upsample_bicubic_frames": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "dfn_dfnet_create": (c_int, [c_int, c_int, POINTER(c_void_p)]),
    "dfn_dfnet_destroy": (c_int, [_P]),
    "dfn_dfnet_set_param": (c_int, [_P, c_char_p, _P, c_size_t]),
    "dfn_dfnet_commit": (c_int, [_P]),
    "dfn_dfnet_workspace_bytes": (c_size_t, [_P, c_int, c_int, c_int, c_int]),
    "dfn_dfnet_forward": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P,
                                  _P, c_size_t, _P]),
    "dfn_dfnet_forward_levels": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "dfn_upsample_bicubic_backward": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "dfn_upsample_bicubic_frames_backward": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "dfn_dfnet_backward_workspace_bytes": (c_size_t, [_P, c_int, c_int, c_int, c_int]),
    "dfn_dfnet_backward_input": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_size_t, _P]),
    "dfn_dfnet_backward_params_workspace_bytes": (c_size_t, [_P, c_int, c_int, c_int, c_int]),
    "dfn_dfnet_backward_params": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, POINTER(c_void_p), c_int, _P, c_size_t, _P]),
    "dfn_dfnet_forward_train": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P,
                                        c_size_t, _P]),
    "dfn_dfnet_backward_all_params": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                              POINTER(c_void_p), c_int, _P, c_size_t, _P]),
    "dfn_frame_prep_scratch_bytes": (c_size_t, []),
    "dfn_frame_prep": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "dfn_frame_post_scratch_bytes": (c_size_t, [c_int]),
    "dfn_frame_post": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "dfn_frame_post_maps_scratch_bytes": (c_size_t, [c_int]),
    "dfn_frame_post_maps": (c_int, [POINTER(RenderMaps), _P, c_int, c_int, c_int, c_int, c_float, c_float, POINTER(FrameMapsOut), _P, _P,
                                    _P, _P]),
    "dfn_dfnet_forward_train_pyramid": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "dfn_dfnet_triplet_pyramid_state_bytes": (c_size_t, [_P, c_int, c_int]),
    "dfn_dfnet_triplet_pyramid_forward": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, _P, _P, c_size_t, _P,
                                                  c_size_t, _P]),
    "dfn_dfnet_backward_all_params_triplet": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_int,
                                                      _P, c_int, _P, c_size_t, _P]),
    "dfn_triplet_loss_state_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfn_triplet_loss_forward": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, c_int, c_float, c_int, _P, _P, c_size_t, _P]),
    "dfn_triplet_loss_backward": (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P, c_size_t, _P]),
    "dfn_dfnet_refresh_train_params_device": (c_int, [_P, POINTER(c_void_p), c_int, c_int, _P]),
    "dfn_dfnet_refresh_pose_params_device": (c_int, [_P, POINTER(c_void_p), c_int, c_int, _P]),
    "dfn_nerfh_train_param_count": (c_int, []),
    "dfn_nerfh_train_param_name": (c_char_p, [c_int]),
    "dfn_nerfh_train_workspace_bytes": (c_size_t, [_P, c_size_t, c_int, c_int]),
    "dfn_nerfh_set_train_mode": (c_int, [_P, c_int]),
    "dfn_nerfh_train_backward_rays_scratch_bytes": (c_size_t, [c_size_t, c_int, c_int]),
    "dfn_nerfh_train_backward_rays": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, _P, c_float, _P, _P, _P, _P, c_float, _P, _P, _P,
                                      _P, c_size_t, _P, c_size_t, _P]),
    "dfn_nerfh_train_tables_selfcheck": (c_int, [_P]),
    "dfn_nerfh_train_forward": (c_int, [_P, POINTER(c_void_p), _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float,
                                        _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "dfn_nerfh_train_forward_v": (c_int, [_P, POINTER(c_void_p), _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float,
                                          _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "dfn_nerfh_train_backward_rays_v": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, _P, c_float, _P, _P, _P, _P, c_float, _P,
                                                _P, _P, _P, _P, c_size_t, _P, c_size_t, _P]),
    "dfn_nerfh_train_backward_rays_maps_v": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, _P, c_float, _P,
                                                     POINTER(TrainMapGrads), c_float, _P, _P, _P, _P, _P, c_size_t, _P, c_size_t, _P]),
    "dfn_nerfw_loss": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_int, c_float, c_float, _P, _P, _P, _P, _P]),
    "dfn_nerfh_train_backward": (c_int, [_P, POINTER(c_void_p), _P, c_size_t, c_size_t, c_int, c_int, _P, c_float, _P, _P, _P, _P,
                                         c_float, _P, POINTER(c_void_p), _P, c_size_t, _P]),
    "dfn_composite_coarse_train_backward_maps": (c_int, [_P, _P, _P, c_float, c_size_t, c_int, POINTER(TrainMapGrads), _P, _P]),
    "dfn_composite_fine_train_backward_maps": (c_int, [_P, _P, c_size_t, c_int, POINTER(TrainMapGrads), c_float, _P, _P, _P]),
    "dfn_nerfh_train_depths": (c_int, [_P, c_size_t, c_int, c_int, _P, _P, c_size_t, _P, _P, _P]),
    "dfn_nerfh_train_backward_maps": (c_int, [_P, POINTER(c_void_p), _P, c_size_t, c_size_t, c_int, c_int, _P, c_float, _P,
                                              POINTER(TrainMapGrads), c_float, _P, POINTER(c_void_p), _P, c_size_t, _P]),
    "dfn_nerfh_train_backward_rays_maps": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, _P, c_float, _P,
                                                   POINTER(TrainMapGrads), c_float, _P, _P, _P, _P, c_size_t, _P, c_size_t, _P]),
    "dfn_nerfh_points_train_workspace_bytes": (c_size_t, [_P, c_int, c_size_t, c_int]),
    "dfn_nerfh_points_train_forward": (c_int, [_P, c_int, POINTER(c_void_p), _P, _P, _P, c_size_t, c_size_t, c_int, _P, _P, c_size_t, _P]),
    "dfn_nerfh_points_train_backward": (c_int, [_P, c_int, POINTER(c_void_p), _P, c_size_t, c_size_t, c_int, _P, _P, POINTER(c_void_p),
                                                _P, c_size_t, _P]),
    "dfn_nerfh_generic_workspace_bytes": (c_size_t, [_P, c_size_t, c_int, c_int]),
    "dfn_nerfh_generic_render_rays": (c_int, [_P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float, _P, _P, _P, _P,
                                              _P, c_size_t, _P]),
    "dfn_nerfh_generic_render_rays_v": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float, _P, _P, _P, _P,
                                                _P, c_size_t, _P]),
    "dfn_nerfh_generic_render_rays_maps": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float, _P, _P, _P, _P,
                                                   _P, c_size_t, POINTER(RenderMaps), _P]),
    "dfn_nerfh_generic_backward_workspace_bytes": (c_size_t, [_P, c_size_t, c_int, c_int]),
    "dfn_nerfh_generic_render_rays_backward": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float, _P, _P, _P, _P, _P,
                                               c_size_t, _P]),
    "dfn_nerfh_generic_render_rays_backward_raw": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float, _P, _P, _P, _P,
                                                   _P, _P, c_size_t, _P]),
    "dfn_nerfh_generic_render_rays_backward_maps": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_size_t, c_int, c_int, c_float, c_float, _P, _P, _P,
                                                    _P, _P, _P, c_size_t, POINTER(MapGrads), _P]),
    "dfn_pose_orthogonalize": (c_int, [_P, c_int, _P, _P]),
    "dfn_pose_orthogonalize_backward": (c_int, [_P, _P, c_int, _P, _P]),
    "dfn_conv_wgrad_scratch_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "dfn_conv_wgrad": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "dfn_linear_forward": (c_int, [_P, c_int, c_int, _P, c_int, c_int, _P, c_int, c_int, _P, c_int, c_size_t, c_int, _P]),
    "dfn_linear_backward_input": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, c_size_t, _P]),
    "dfn_linear_backward_weight_scratch_bytes": (c_size_t, [c_int, c_int, c_size_t]),
    "dfn_linear_backward_weight": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, _P, _P, c_size_t, _P]),
    "dfn_adam_step": (c_int, [_P, c_int, c_double, c_double, c_double, c_double, _P]),
    # mesh export (isosurface.hip; the reference only declares the flags, models/options.py:69-70): grid points for the density query,
    # marching tetrahedra as count -> read totals -> emit
    "dfn_isosurface_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dfn_grid_points": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "dfn_isosurface_count": (c_int, [_P, c_int, c_int, c_int, c_float, _P, c_size_t, _P, _P]),
    "dfn_isosurface_emit": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_float, _P, c_size_t, _P, c_longlong, _P, c_longlong, _P]),
    "dfn_profile_enable": (c_int, [c_int]),
    "dfn_profile_read": (c_int, [c_int, POINTER(c_double), POINTER(c_int)]),
}

_lib = None


def load():
    """Load libdfnet_hip.so once and declare every prototype.  Raises if the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP library is the product and has no fallback. "
                "Build it with `make -C dfnet_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`).")
        # torch first: the library must bind to the HIP runtime torch has mapped (device pointers and streams are torch's); loading
        # it before torch maps the system libamdhip64 as a second runtime and torch then finds "No HIP GPUs" (seen when
        # `python __graft_entry__.py smoke` ran build() -> load() before the first `import torch`)
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = load().dfn_last_error()
        raise DfnError(f"{what or 'libdfnet_hip'} failed (status {rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a contiguous fp32 CUDA tensor (or None)."""
    if t is None:
        return None
    import torch
    if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32:
        raise ValueError(f"expected a contiguous fp32 CUDA tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")
    return c_void_p(t.data_ptr())


def current_stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)
