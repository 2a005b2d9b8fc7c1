"""ctypes binding of libpwc_hip.so (the C ABI declared in include/pwc_hip.h).

The library is the product: if it is missing or fails to load, every operator
raises -- there is no CPU or eager-PyTorch fallback for the hot path.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# PWC_HIP_LIB: alternative build of the same C ABI (kernel experiments); default = the in-tree library
LIB_PATH = os.environ.get("PWC_HIP_LIB") or os.path.join(_HERE, "libpwc_hip.so")

ABI_VERSION = 13
PWC_F32, PWC_F16 = 0, 1
FLAG_CORR_NORMALIZE = 1
FLAG_ACT_LEAKY = 2
FLAG_CONV_RESIDUAL = 4
FLAG_CONV_OUT_F32 = 8
FLAG_CONV_SPLIT_W = 16
FLAG_CONV_SPLIT2 = 32

# name -> (restype, argtypes); mirrors include/pwc_hip.h one to one
SIGNATURES = {
    "pwc_abi_version": (c_int, []),
    "pwc_experiment_mask": (c_int, []),
    "pwc_last_error": (c_char_p, []),
    "pwc_last_conv_kernel": (c_char_p, []),
    "pwc_set_option": (c_int, [c_char_p, c_int]),
    "pwc_get_option": (c_int, [c_char_p, ctypes.POINTER(c_int)]),
    "pwc_corr_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_uint, c_float,
                             c_int64, c_int64, c_int64, c_void_p]),
    "pwc_warp_corr81_preferred": (c_int, [c_int, c_int, c_int, c_int]),
    "pwc_warp_corr81_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_float,
                                    c_float, c_uint, c_float, c_int64, c_int64, c_int64, c_int64, c_void_p]),
    "pwc_corr_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_uint, c_void_p]),
    "pwc_warp_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_float, c_int, c_float, c_int, c_int64, c_int64, c_int64, c_void_p]),
    "pwc_warp_bwd_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "pwc_warp_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_float, c_int, c_float, c_int, c_void_p, c_int64, c_void_p]),
    "pwc_warp_corr81_bwd_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "pwc_warp_corr81_bwd": (c_int, [c_void_p] * 8 + [c_int, c_int, c_int, c_int, c_float, c_int, c_float, c_float, c_uint, c_float]
                            + [c_int64] * 5 + [c_void_p, c_int64, c_void_p]),
    "pwc_proxy_loss_workspace_bytes": (c_int64, [c_int] * 6),
    "pwc_proxy_loss_fwd_workspace_bytes": (c_int64, [c_int] * 6),
    "pwc_proxy_loss_fwd": (c_int, [c_void_p] * 4 + [c_int, c_void_p] + [c_int] * 6 + [c_float] * 3 + [c_int64] * 4
                           + [c_void_p, c_int64, c_void_p]),
    "pwc_proxy_loss_bwd": (c_int, [c_void_p] * 4 + [c_int, c_void_p, c_void_p] + [c_int] * 6 + [c_float] * 3 + [c_int64] * 4
                           + [c_void_p, c_int64, c_void_p]),
    "pwc_flow_warp_image_fwd": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_int64] * 3 + [c_void_p]),
    "pwc_sup_flow_loss_workspace_bytes": (c_int64, [c_int] * 6),
    "pwc_sup_flow_loss_fwd": (c_int, [c_void_p] * 3 + [c_int, c_int, c_void_p] + [c_int] * 5 + [c_double] + [c_int64] * 3
                              + [c_void_p, c_int64, c_void_p]),
    "pwc_sup_flow_loss_bwd": (c_int, [c_void_p] * 3 + [c_int, c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_double] + [c_int64] * 3
                              + [c_void_p, c_int64, c_void_p]),
    "pwc_sup_multiscale_loss_workspace_bytes": (c_int64, [c_int] * 4 + [c_void_p, c_int]),
    "pwc_sup_multiscale_loss_fwd": (c_int, [c_void_p] * 4 + [c_int] + [c_void_p] * 2 + [c_int] + [c_void_p] * 2 + [c_int] * 3
                                    + [c_double, c_float, c_float] + [c_int64] * 3 + [c_void_p, c_int64, c_void_p]),
    "pwc_sup_multiscale_loss_bwd": (c_int, [c_void_p] * 4 + [c_int] + [c_void_p] * 2 + [c_int] + [c_void_p] * 4 + [c_int] * 3
                                    + [c_double, c_float, c_float] + [c_int64] * 3 + [c_void_p, c_int64, c_void_p]),
    "pwc_fb_metrics_workspace_bytes": (c_int64, [c_int] * 3),
    "pwc_fb_metrics": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "pwc_epipolar_pairs": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_int64] * 2 + [c_void_p]),
    "pwc_epipolar_ransac_workspace_bytes": (c_int64, [c_int, c_int]),
    "pwc_epipolar_ransac": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_double] + [c_void_p] * 5
                            + [c_int64, c_void_p]),
    "pwc_epipolar_distance": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int64, c_void_p]),
    "pwc_epipolar_mask_workspace_bytes": (c_int64, [c_int] * 3),
    "pwc_epipolar_mask": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_double] * 3 + [c_int64, c_void_p, c_int64, c_void_p]),
    "pwc_epipolar_loss_workspace_bytes": (c_int64, [c_int] * 3),
    "pwc_epipolar_loss_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p] + [c_int] * 4
                              + [c_double] * 2 + [c_int64] * 2 + [c_void_p, c_int64, c_void_p]),
    "pwc_epipolar_loss_bwd": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p]
                              + [c_int] * 4 + [c_double] * 2 + [c_int64] * 2 + [c_void_p, c_int64, c_void_p]),
    "pwc_conv3x3_packed_bytes": (c_int64, [c_int, c_int, c_int]),
    "pwc_conv3x3_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "pwc_conv2d_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_uint, c_float,
                               c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "pwc_conv2d_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "pwc_conv3x3_f16_packed_bytes": (c_int64, [c_int, c_int]),
    "pwc_conv3x3_f16_packed_bytes_split": (c_int64, [c_int, c_int]),
    "pwc_conv3x3_f16_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "pwc_conv3x3_f16_pack_split": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "pwc_conv3x3_wino_packed_bytes": (c_int64, [c_int, c_int]),
    "pwc_conv3x3_wino_preferred": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "pwc_conv3x3_wino_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "pwc_conv3x3_wino_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_uint, c_float,
                             c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "pwc_conv3x3_wino_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "pwc_conv3x3_wino4_packed_bytes": (c_int64, [c_int, c_int]),
    "pwc_conv3x3_wino4_preferred": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "pwc_conv3x3_wino4_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "pwc_conv3x3_wino4_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_uint, c_float,
                                     c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "pwc_conv3x3_wino4_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "pwc_kitti_ingest_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "pwc_flow_upsample_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_void_p]),
    "pwc_pil_resize_ksize": (c_int, [c_int, c_int]),
    "pwc_pil_resize_supported": (c_int, [c_int] * 4),
    "pwc_pil_resize_frames_u8": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                         c_void_p, c_int64, c_int, c_void_p]),
    "pwc_pil_resize_planes_f32": (c_int, [c_void_p] * 2 + [c_int] * 6 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                          c_void_p, c_int64, c_void_p]),
    "pwc_pil_flow_eval_workspace_bytes": (c_int64, [c_int] * 3),
    "pwc_pil_flow_eval": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int64,
                                  c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "pwc_cv_resize_frames_u8": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p] * 5 + [c_int, c_int64, c_int, c_void_p]),
    "pwc_cv_resize_flow_f32": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p] * 4 + [c_float] * 3 + [c_int, c_int64, c_void_p]),
    "pwc_cv_warp_perspective_u8": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p, c_int, c_int64, c_int64, c_void_p]),
    "pwc_video_ingest_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_int64, c_void_p]),
    "pwc_kitti_score_workspace_bytes": (c_int64, [c_int] * 3),
    "pwc_kitti_score": (c_int, [c_void_p] + [c_int] * 7 + [c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                                c_void_p, c_void_p]),
    "pwc_flow_compare_workspace_bytes": (c_int64, [c_int] * 3),
    "pwc_flow_compare": (c_int, [c_void_p, c_void_p] + [c_int] * 3 + [c_int64, c_int64, ctypes.POINTER(c_float), c_int, c_void_p, c_void_p,
                                 c_int64, c_void_p, c_void_p]),
    "pwc_flow_stats_workspace_bytes": (c_int64, [c_int] * 3),
    "pwc_flow_stats": (c_int, [c_void_p] + [c_int] * 5 + [c_int64, c_int, c_float, c_float, c_void_p, c_int64, c_void_p, c_void_p]),
    "pwc_flow_color": (c_int, [c_void_p] + [c_int] * 5 + [c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "pwc_flow_quiver": (c_int, [c_void_p] + [c_int] * 5 + [c_int64, c_int, c_int, c_int, c_float, c_float, c_float, c_int, c_float,
                                c_void_p, c_int64, c_float] + [c_void_p] * 4),
    "pwc_vanishing_workspace_bytes": (c_int64, [c_int] * 4),
    "pwc_vanishing_point": (c_int, [c_void_p] + [c_int] * 6 + [c_double] + [c_int] * 3 + [c_void_p] * 4 + [c_int64, c_void_p]),
    "pwc_kitti_augment": (c_int, [c_void_p, c_void_p, c_int, c_void_p] + [c_int] * 5 + [c_void_p] * 6),
    "pwc_kitti_augment_full": (c_int, [c_void_p, c_void_p, c_int, c_void_p] + [c_int] * 5 + [c_void_p] * 6),
    "pwc_optim_chunk_elems": (c_int, []),
    "pwc_optim_workspace_bytes": (c_int64, [c_int64, c_int]),
    "pwc_optim_grad_sqsum": (c_int, [c_void_p] * 3 + [c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "pwc_optim_finish": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_double, c_void_p, c_void_p] + [c_double] * 3
                         + [c_void_p] * 3),
    "pwc_optim_adam_update": (c_int, [c_void_p] * 3 + [c_int64] * 3 + [c_int, c_int, c_void_p, c_int64] + [c_double] * 5
                              + [c_int, c_void_p]),
    "pwc_lattice_unsplit_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_void_p]),
    "pwc_conv2d_f16_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_uint, c_float, c_int64, c_int64, c_void_p]),
    "pwc_nchw_to_c8_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_int64, c_void_p]),
    "pwc_nchw_to_c8_f16_hilo": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_void_p]),
    "pwc_c8_f16_to_nchw": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_int64, c_void_p]),
    "pwc_image_conv_s2_c8_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                         c_int64, c_int64, c_void_p]),
    "pwc_pyramid1_f16_packed_bytes": (c_int64, []),
    "pwc_pyramid1_fused_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                       c_int64, c_int64, c_void_p]),
    "pwc_pyr1_wino_packed_bytes": (c_int64, []),
    "pwc_pyr1_wino_preferred": (c_int, [c_int, c_int, c_int]),
    "pwc_pyr1_wino_pack": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pwc_pyr1_wino_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int64, c_int64, c_void_p]),
    "pwc_pyr1_wino_pair_fwd": (c_int, [c_void_p] * 6 + [c_int, c_int, c_int, c_float, c_int64, c_int64, c_void_p]),
    "pwc_corr81_c8_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_uint, c_float,
                                  c_int64, c_int64, c_int64, c_void_p]),
    "pwc_warp_c8_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_float,
                                c_int64, c_int64, c_int64, c_void_p]),
    "pwc_level_entry_c8_f16": (c_int, [c_void_p] * 9 + [c_int, c_int, c_int, c_int, c_float, c_int, c_float] + [c_int64] * 7 + [c_void_p]),
    "pwc_level_corr81_c8_f16": (c_int, [c_void_p] * 9 + [c_int, c_int, c_int, c_int, c_float, c_int, c_float, c_float, c_uint, c_float]
                                + [c_int64] * 7 + [c_void_p]),
    "pwc_calib_lds_dma_read": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "pwc_upsample_entry_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int64, c_void_p]),
    "pwc_deconv4x4s2_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_void_p]),
    "pwc_head_upfeat_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_void_p]),
    "pwc_head_upfeat_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "pwc_head_upfeat_ws_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
}

_lib = None


class PwcHipError(RuntimeError):
    """Raised when libpwc_hip.so is unavailable or a call returns non-zero."""


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PwcHipError(
            "libpwc_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C opticalflow_amd/csrc`; the HIP path has no fallback" % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the host
        raise PwcHipError("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise PwcHipError("libpwc_hip.so does not export %s" % name) from e
        fn.restype = res
        fn.argtypes = args
    got = lib.pwc_abi_version()
    if got != ABI_VERSION:
        raise PwcHipError("libpwc_hip.so ABI %d, binding expects %d -- rebuild" % (got, ABI_VERSION))
    exp = lib.pwc_experiment_mask()
    if exp and not os.environ.get("PWC_HIP_LIB"):
        # a timing-experiment build (-DPWC_*_EXP: work skipped, results invalid) must never pass as the product
        raise PwcHipError("%s was built with timing-experiment switches (mask %d): results would be invalid -- rebuild it "
                          "(make -C opticalflow_amd/csrc) or select an experiment library explicitly with PWC_HIP_LIB" % (LIB_PATH, exp))
    _lib = lib
    return lib


def set_option(name: str, value: int) -> None:
    """pwc_set_option: flip a kernel-selection switch of the library at run time (see include/pwc_hip.h for the names)."""
    check(load().pwc_set_option(name.encode(), int(value)), "pwc_set_option(%s)" % name)


def get_option(name: str) -> int:
    v = c_int(0)
    check(load().pwc_get_option(name.encode(), ctypes.byref(v)), "pwc_get_option(%s)" % name)
    return v.value


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().pwc_last_error()
        raise PwcHipError("%s failed (code %d): %s" % (what, rc, msg.decode("utf-8", "replace") if msg else "?"))
