"""Tensor-level wrappers over the C ABI (device pointers + current HIP stream).

PyTorch is used only for device memory and streams; all arithmetic happens in
libpwc_hip.so.  Every wrapper validates what the kernels assume (device,
dtype, dense C/H/W planes, batch stride) *before* launching -- the reference
does no validation and silently assumes contiguous NCHW
(correlation_cuda_kernel.cu:341-360).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Tuple

import torch

from . import _lib
from ._args import (_bias_arg, _dtype_code, _f32_dense, _frames_dense, _kitti_gt_arg, _mask_arg, _out_arg, _packed_arg, _plane_dense, _ptr,
                    _query_bytes, _raw_frames_shape, _require_device, _scalar_arg, _scratch, _stream, _table_arg, _workspace_args, densify)
from ._lib import (FLAG_ACT_LEAKY, FLAG_CONV_RESIDUAL, FLAG_CORR_NORMALIZE, PWC_F32, PwcHipError, check)
from ._pipeline import pad64

def corr_output_shape(C: int, H: int, W: int, pad_size: int, kernel_size: int, max_displacement: int,
                      stride1: int, stride2: int) -> Tuple[int, int, int]:
    """Shape contract of the reference binding (correlation_cuda.cc:25-38)."""
    krad = (kernel_size - 1) // 2
    border = krad + max_displacement
    drad = max_displacement // stride2
    return ((2 * drad + 1) ** 2,
            int(math.ceil((H + 2 * pad_size - 2 * border) / float(stride1))),
            int(math.ceil((W + 2 * pad_size - 2 * border) / float(stride1))))


def correlation(in1: torch.Tensor, in2: torch.Tensor, pad_size: int = 4, kernel_size: int = 1,
                max_displacement: int = 4, stride1: int = 1, stride2: int = 1, corr_multiply: float = 1.0,
                normalize: bool = False, leaky_slope: Optional[float] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    if in1.shape != in2.shape or in1.dtype != in2.dtype or in1.device != in2.device:
        raise ValueError("correlation inputs differ: %s/%s vs %s/%s" % (tuple(in1.shape), in1.dtype, tuple(in2.shape), in2.dtype))
    bs1 = _plane_dense(in1, "input1")
    bs2 = _plane_dense(in2, "input2")
    B, C, H, W = in1.shape
    nch, oh, ow = corr_output_shape(C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    if oh <= 0 or ow <= 0:
        raise ValueError("correlation output would be empty (%d x %d)" % (oh, ow))
    out = _out_arg(out, (B, nch, oh, ow), in1.dtype, in1.device)
    bso = _plane_dense(out, "out")
    flags = (FLAG_CORR_NORMALIZE if normalize else 0) | (FLAG_ACT_LEAKY if leaky_slope is not None else 0)
    with torch.cuda.device(in1.device):
        rc = lib.pwc_corr_fwd(in1.data_ptr(), in2.data_ptr(), out.data_ptr(), B, C, H, W,
                              pad_size, kernel_size, max_displacement, stride1, stride2,
                              float(corr_multiply), _dtype_code(in1), flags, float(leaky_slope or 0.0),
                              bs1, bs2, bso, _stream(in1))
    check(rc, "pwc_corr_fwd")
    return out


def correlation_backward(in1: torch.Tensor, in2: torch.Tensor, grad_out: torch.Tensor, pad_size: int = 4,
                         kernel_size: int = 1, max_displacement: int = 4, stride1: int = 1, stride2: int = 1,
                         corr_multiply: float = 1.0, normalize: bool = False):
    lib = _lib.load()
    for name, t in (("input1", in1), ("input2", in2), ("grad_output", grad_out)):
        _plane_dense(t, name)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous for the backward kernel" % name)
    B, C, H, W = in1.shape
    g1 = torch.empty_like(in1)
    g2 = torch.empty_like(in2)
    with torch.cuda.device(in1.device):
        rc = lib.pwc_corr_bwd(in1.data_ptr(), in2.data_ptr(), grad_out.data_ptr(), g1.data_ptr(), g2.data_ptr(),
                              B, C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2,
                              float(corr_multiply), _dtype_code(in1), FLAG_CORR_NORMALIZE if normalize else 0,
                              _stream(in1))
    check(rc, "pwc_corr_bwd")
    return g1, g2


def warp_correlation_preferred(B: int, C: int, H: int, W: int) -> bool:
    """Whether the fused warp + correlation kernel beats warp() followed by correlation() for this geometry (rule in the library:
    not for maps of a few tiles, where the small-map correlation kernel wins)."""
    return bool(_lib.load().pwc_warp_corr81_preferred(B, C, H, W))


def warp_correlation(in1: torch.Tensor, x2: torch.Tensor, flo: torch.Tensor, flow_scale: float = 1.0,
                     align_corners: bool = False, mask_threshold: float = 0.9999, corr_multiply: float = 1.0,
                     normalize: bool = False, leaky_slope: Optional[float] = None,
                     out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """correlation(in1, warp(x2, flow_scale * flo)) for PWC-Net's configuration (pad 4, k 1, d 4, strides 1) in ONE kernel:
    the warped tensor is produced tile by tile in LDS and never written to HBM (PWCNet.py:212-213 etc.).  Bit-identical to
    warp() followed by correlation().  Returns None (nothing launched) when the geometry is outside the fused kernel
    (W % 4 != 0 or unaligned operands): call the two operators then."""
    lib = _lib.load()
    bs1, bs2, bsf = _plane_dense(in1, "in1"), _plane_dense(x2, "x2"), _plane_dense(flo, "flo")
    B, C, H, W = in1.shape
    if in1.dtype != torch.float32 or x2.shape != in1.shape or x2.dtype != in1.dtype or tuple(flo.shape) != (B, 2, H, W) \
            or flo.dtype != in1.dtype or x2.device != in1.device or flo.device != in1.device:
        raise ValueError("in1, x2 must be float32 [B,C,H,W] and flo [B,2,H,W] on one device")
    out = _out_arg(out, (B, 81, H, W), in1.dtype, in1.device)
    bso = _plane_dense(out, "out")
    flags = (FLAG_CORR_NORMALIZE if normalize else 0) | (FLAG_ACT_LEAKY if leaky_slope is not None else 0)
    with torch.cuda.device(in1.device):
        rc = lib.pwc_warp_corr81_fwd(in1.data_ptr(), x2.data_ptr(), flo.data_ptr(), out.data_ptr(), B, C, H, W,
                                     float(flow_scale), 1 if align_corners else 0, float(mask_threshold),
                                     float(corr_multiply), flags, float(leaky_slope or 0.0), bs1, bs2, bsf, bso, _stream(in1))
    if rc == -2:                               # PWC_EUNSUPPORTED: geometry outside the fused kernel
        return None
    check(rc, "pwc_warp_corr81_fwd")
    return out


def warp(x: torch.Tensor, flo: torch.Tensor, flow_scale: float = 1.0, align_corners: bool = False,
         mask_threshold: float = 0.9999, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    bsf = _plane_dense(flo, "flo")
    B, C, H, W = x.shape
    if tuple(flo.shape) != (B, 2, H, W) or flo.dtype != x.dtype or flo.device != x.device:
        raise ValueError("flo must be %s %s, got %s %s" % ((B, 2, H, W), x.dtype, tuple(flo.shape), flo.dtype))
    out = _out_arg(out, (B, C, H, W), x.dtype, x.device)
    bso = _plane_dense(out, "out")
    with torch.cuda.device(x.device):
        rc = lib.pwc_warp_fwd(x.data_ptr(), flo.data_ptr(), out.data_ptr(), B, C, H, W,
                              float(flow_scale), 1 if align_corners else 0, float(mask_threshold), _dtype_code(x),
                              bsx, bsf, bso, _stream(x))
    check(rc, "pwc_warp_fwd")
    return out


def warp_backward(x: torch.Tensor, flo: torch.Tensor, grad_out: torch.Tensor, flow_scale: float = 1.0,
                  align_corners: bool = False, mask_threshold: float = 0.9999, deterministic: bool = True):
    """(grad_x, grad_flo) of `warp` for contiguous float32 tensors.  deterministic (default): the scatter into grad_x
    accumulates 64-bit fixed-point integers in a scratch buffer (bit-reproducible); False: float atomics."""
    lib = _lib.load()
    for name, t in (("x", x), ("flo", flo), ("grad_out", grad_out)):
        _plane_dense(t, name)
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError("%s must be contiguous float32 for the backward kernel" % name)
    B, C, H, W = x.shape
    if tuple(flo.shape) != (B, 2, H, W) or tuple(grad_out.shape) != (B, C, H, W):
        raise ValueError("flo must be %s and grad_out %s" % ((B, 2, H, W), (B, C, H, W)))
    gx = torch.empty_like(x)
    gf = torch.empty_like(flo)
    ws, ws_bytes = None, 0
    if deterministic:
        ws, ws_bytes = _scratch(lib.pwc_warp_bwd_workspace_bytes(B, C, H, W), x.device)
    with torch.cuda.device(x.device):
        rc = lib.pwc_warp_bwd(x.data_ptr(), flo.data_ptr(), grad_out.data_ptr(), gx.data_ptr(), gf.data_ptr(),
                              B, C, H, W, float(flow_scale), 1 if align_corners else 0, float(mask_threshold),
                              _dtype_code(x), _ptr(ws), ws_bytes, _stream(x))
    check(rc, "pwc_warp_bwd")
    return gx, gf


class WarpFunction(torch.autograd.Function):
    """autograd wrapper of the fused warp: forward and backward both run HIP kernels (what autograd builds from
    PWCNet.py:141-177 in the reference's training scripts)."""

    @staticmethod
    def forward(ctx, x, flo, flow_scale=1.0, align_corners=False, mask_threshold=0.9999):
        x, flo = x.contiguous(), flo.contiguous()
        ctx.save_for_backward(x, flo)
        ctx.cfg = (flow_scale, align_corners, mask_threshold)
        return warp(x, flo, flow_scale, align_corners, mask_threshold)

    @staticmethod
    def backward(ctx, grad_out):
        x, flo = ctx.saved_tensors
        gx, gf = warp_backward(x, flo, grad_out.contiguous(), *ctx.cfg)
        return gx, gf, None, None, None


def warp_correlation_backward(c1: torch.Tensor, c2: torch.Tensor, flo: Optional[torch.Tensor], y: torch.Tensor,
                              grad_y: torch.Tensor, flow_scale: float = 1.0, align_corners: bool = False,
                              mask_threshold: float = 0.9999, corr_multiply: float = 1.0, normalize: bool = False,
                              leaky_slope: Optional[float] = 0.1, fused: bool = True):
    """(grad_c1, grad_c2, grad_flo) of y = act(correlation(c1, warp(c2, flow_scale * flo))) in PWC-Net's configuration (pad 4, k 1,
    d 4, strides 1; act = LeakyReLU(leaky_slope), None = no activation); flo None = no warp (level 6), grad_flo is then None.
    y is the forward's activated output (its sign is the LeakyReLU mask).  fused (default): one pass of pwc_warp_corr81_bwd,
    bit-reproducible.  Where that entry declines the geometry (PWC_EUNSUPPORTED), or with fused=False, the same gradients come
    from warp_fwd -> mask in torch -> corr_bwd -> warp_bwd (also deterministic; summation order differs)."""
    lib = _lib.load()
    B, C, H, W = c1.shape
    dev = c1.device
    c1, bs1 = _f32_dense(c1, "c1", (B, C, H, W), dev)
    c2, bs2 = _f32_dense(c2, "c2", (B, C, H, W), dev)
    y, bsy = _f32_dense(y, "y", (B, 81, H, W), dev)
    grad_y, bsg = _f32_dense(grad_y, "grad_y", (B, 81, H, W), dev)
    bsf = 0
    if flo is not None:
        flo, bsf = _f32_dense(flo, "flo", (B, 2, H, W), dev)
    if fused:
        g1 = torch.empty((B, C, H, W), dtype=torch.float32, device=c1.device)
        g2 = torch.empty_like(g1)
        gf = torch.empty((B, 2, H, W), dtype=torch.float32, device=c1.device) if flo is not None else None
        ws, ws_bytes = None, 0
        if flo is not None:
            ws, ws_bytes = _scratch(lib.pwc_warp_corr81_bwd_workspace_bytes(B, C, H, W), c1.device)
        flags = (FLAG_CORR_NORMALIZE if normalize else 0) | (FLAG_ACT_LEAKY if leaky_slope is not None else 0)
        with torch.cuda.device(c1.device):
            rc = lib.pwc_warp_corr81_bwd(c1.data_ptr(), c2.data_ptr(), _ptr(flo), y.data_ptr(),
                                         grad_y.data_ptr(), g1.data_ptr(), g2.data_ptr(), _ptr(gf),
                                         B, C, H, W, float(flow_scale), 1 if align_corners else 0, float(mask_threshold),
                                         float(corr_multiply), flags, float(leaky_slope or 0.0), bs1, bs2, bsf, bsy, bsg,
                                         _ptr(ws), ws_bytes, _stream(c1))
        if rc != -2:                               # PWC_EUNSUPPORTED: take the composition below
            check(rc, "pwc_warp_corr81_bwd")
            return g1, g2, gf
    g = grad_y if leaky_slope is None else torch.where(y > 0, grad_y, grad_y * leaky_slope)
    if flo is None:
        g1, g2 = correlation_backward(c1.contiguous(), c2.contiguous(), g.contiguous(), 4, 1, 4, 1, 1, corr_multiply, normalize)
        return g1, g2, None
    c2, flo = c2.contiguous(), flo.contiguous()
    w2 = warp(c2, flo, flow_scale, align_corners, mask_threshold)
    g1, gw2 = correlation_backward(c1.contiguous(), w2, g.contiguous(), 4, 1, 4, 1, 1, corr_multiply, normalize)
    g2, gf = warp_backward(c2, flo, gw2, flow_scale, align_corners, mask_threshold)
    return g1, g2, gf


class WarpCorrelationFunction(torch.autograd.Function):
    """autograd of one PWC-Net cost volume, act(corr(c1, warp(c2, flow_scale * flo))) (PWCNet.py:212-214, 226-228, 240-242,
    256-258; flo None: corr(c1, c2) of level 6, :197-198): forward = the fused forward kernel where the library prefers it (else
    warp + correlation), backward = pwc_warp_corr81_bwd.  Under torch.autocast the inputs are cast to float32 (the kernels are
    f32 only).  apply(c1, c2, flo, flow_scale, align_corners, mask_threshold, corr_multiply, normalize, leaky_slope)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, c1, c2, flo, flow_scale=1.0, align_corners=False, mask_threshold=0.9999, corr_multiply=1.0,
                normalize=False, leaky_slope=0.1):
        c1, c2 = c1.contiguous(), c2.contiguous()
        flo = flo.contiguous() if flo is not None else None
        B, C, H, W = c1.shape
        y = None
        if flo is not None:
            if warp_correlation_preferred(B, C, H, W):
                y = warp_correlation(c1, c2, flo, flow_scale, align_corners, mask_threshold, corr_multiply, normalize, leaky_slope)
            if y is None:
                y = correlation(c1, warp(c2, flo, flow_scale, align_corners, mask_threshold), 4, 1, 4, 1, 1, corr_multiply,
                                normalize, leaky_slope)
        else:
            y = correlation(c1, c2, 4, 1, 4, 1, 1, corr_multiply, normalize, leaky_slope)
        ctx.save_for_backward(c1, c2, flo, y)
        ctx.cfg = (flow_scale, align_corners, mask_threshold, corr_multiply, normalize, leaky_slope)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y):
        c1, c2, flo, y = ctx.saved_tensors
        g1, g2, gf = warp_correlation_backward(c1, c2, flo, y, grad_y.to(torch.float32).contiguous(), *ctx.cfg)
        return g1, g2, gf, None, None, None, None, None, None


def pack_conv3x3(weight: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] nn.Conv2d filter bank -> kernel-native packed buffer (device, float32)."""
    lib = _lib.load()
    if weight.dim() != 4 or weight.shape[2:] != (3, 3):
        raise ValueError("expected [Cout,Cin,3,3], got %s" % (tuple(weight.shape),))
    if not weight.is_cuda:
        raise PwcHipError("weights must be on the device")
    w = weight.detach().to(torch.float32).contiguous()
    cout, cin = w.shape[:2]
    nbytes = lib.pwc_conv3x3_packed_bytes(cin, cout, PWC_F32)
    if nbytes <= 0:
        raise PwcHipError("pwc_conv3x3_packed_bytes(%d,%d) = %d" % (cin, cout, nbytes))
    wp = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = lib.pwc_conv3x3_pack(w.data_ptr(), wp.data_ptr(), cin, cout, PWC_F32, _stream(w))
    check(rc, "pwc_conv3x3_pack")
    return wp


def conv3x3(x: torch.Tensor, wpacked: torch.Tensor, bias: torch.Tensor, cout: int, stride: int = 1,
            dilation: int = 1, leaky_slope: Optional[float] = 0.1, residual: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`workspace`: optional device scratch (any dtype, see conv3x3_workspace_bytes) enabling the split-K
    route for layers with few output tiles; without it the layer runs unsplit."""
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    B, cin, H, W = x.shape
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = _out_arg(out, (B, cout, ho, wo), x.dtype, x.device)
    bsy = _plane_dense(out, "out")
    _packed_arg(wpacked, lib.pwc_conv3x3_packed_bytes(cin, cout, PWC_F32), x.device, "weights")
    _bias_arg(bias, cout, x.device)
    flags = FLAG_ACT_LEAKY if leaky_slope is not None else 0
    res_ptr, bsr = 0, 0
    if residual is not None:
        if tuple(residual.shape) != tuple(out.shape) or residual.dtype != x.dtype:
            raise ValueError("residual must match the output")
        bsr = _plane_dense(residual, "residual")
        res_ptr = residual.data_ptr()
        flags |= FLAG_CONV_RESIDUAL
    ws_ptr, ws_bytes = _workspace_args(workspace, x)
    with torch.cuda.device(x.device):
        rc = lib.pwc_conv2d_fwd(x.data_ptr(), wpacked.data_ptr(), bias.data_ptr(), res_ptr, out.data_ptr(),
                                B, cin, H, W, cout, stride, dilation, _dtype_code(x), flags,
                                float(leaky_slope or 0.0), bsx, bsy, bsr, ws_ptr, ws_bytes, _stream(x))
    check(rc, "pwc_conv2d_fwd")
    return out


def conv3x3_wino_preferred(B: int, cin: int, H: int, W: int, cout: int, dilation: int = 1) -> bool:
    """Whether the Winograd route is expected to beat conv3x3 for this stride-1 layer (rule lives in the library)."""
    return bool(_lib.load().pwc_conv3x3_wino_preferred(B, cin, H, W, cout, dilation))


def pack_conv3x3_wino(weight: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] filter bank -> Winograd F(2x2,3x3) filters G g Gt in the kernel's LDS order (device, float32)."""
    lib = _lib.load()
    if weight.dim() != 4 or weight.shape[2:] != (3, 3):
        raise ValueError("expected [Cout,Cin,3,3], got %s" % (tuple(weight.shape),))
    if not weight.is_cuda:
        raise PwcHipError("weights must be on the device")
    w = weight.detach().to(torch.float32).contiguous()
    cout, cin = w.shape[:2]
    up = torch.empty(lib.pwc_conv3x3_wino_packed_bytes(cin, cout) // 4, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = lib.pwc_conv3x3_wino_pack(w.data_ptr(), up.data_ptr(), cin, cout, _stream(w))
    check(rc, "pwc_conv3x3_wino_pack")
    return up


def conv3x3_wino_workspace_bytes(B: int, cin: int, H: int, W: int, cout: int, dilation: int = 1) -> int:
    """Scratch bytes the split-K form of this layer wants (0 = it does not split)."""
    return _query_bytes(_lib.load().pwc_conv3x3_wino_workspace_bytes(B, cin, H, W, cout, dilation), "conv")


def conv3x3_wino(x: torch.Tensor, upacked: torch.Tensor, bias: torch.Tensor, cout: int, leaky_slope: Optional[float] = 0.1,
                 out: Optional[torch.Tensor] = None, dilation: int = 1, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 / stride 1 convolution (padding = dilation) + bias (+ LeakyReLU) by Winograd F(2x2,3x3) on the matrix cores (fp32)."""
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    B, cin, H, W = x.shape
    if x.dtype != torch.float32:
        raise ValueError("conv3x3_wino is fp32 only")
    out = _out_arg(out, (B, cout, H, W), x.dtype, x.device)
    bsy = _plane_dense(out, "out")
    _packed_arg(upacked, lib.pwc_conv3x3_wino_packed_bytes(cin, cout), x.device, "Winograd filters")
    _bias_arg(bias, cout, x.device)
    ws_ptr, ws_bytes = _workspace_args(workspace, x)
    with torch.cuda.device(x.device):
        rc = lib.pwc_conv3x3_wino_fwd(x.data_ptr(), upacked.data_ptr(), bias.data_ptr(), out.data_ptr(), B, cin, H, W, cout, dilation,
                                      FLAG_ACT_LEAKY if leaky_slope is not None else 0, float(leaky_slope or 0.0), bsx, bsy,
                                      ws_ptr, ws_bytes, _stream(x))
    check(rc, "pwc_conv3x3_wino_fwd")
    return out


def pyr1_wino_preferred(B: int, H: int, W: int) -> int:
    """Route of the 16 -> 16 layers on B images of H x W (option "pyr1_wino"; rule in the library): 0 = conv3x3, 1 = pyr1_wino layer by
    layer, 2 = two consecutive layers as one pyr1_wino_pair launch."""
    return int(_lib.load().pwc_pyr1_wino_preferred(B, H, W))


def pack_pyr1_wino(weight: torch.Tensor) -> torch.Tensor:
    """[16,16,3,3] filter bank -> G g Gt in the LDS order of pwc_pyr1_wino_fwd (device, float32, 16 KB)."""
    lib = _lib.load()
    if tuple(weight.shape) != (16, 16, 3, 3):
        raise ValueError("expected [16,16,3,3], got %s" % (tuple(weight.shape),))
    if not weight.is_cuda:
        raise PwcHipError("weights must be on the device")
    w = weight.detach().to(torch.float32).contiguous()
    up = torch.empty(lib.pwc_pyr1_wino_packed_bytes() // 4, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = lib.pwc_pyr1_wino_pack(w.data_ptr(), up.data_ptr(), _stream(w))
    check(rc, "pwc_pyr1_wino_pack")
    return up


def pyr1_wino(x: torch.Tensor, upacked: torch.Tensor, bias: torch.Tensor, leaky_slope: float = 0.1,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(16 -> 16, 3x3, pad 1) + bias + LeakyReLU by Winograd F(2x2,3x3) on the fp32 matrix cores (W % 4 == 0)."""
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    B, cin, H, W = x.shape
    if x.dtype != torch.float32 or cin != 16:
        raise ValueError("pyr1_wino takes float32 [B,16,H,W], got %s %s" % (x.dtype, tuple(x.shape)))
    out = _out_arg(out, (B, 16, H, W), x.dtype, x.device)
    bsy = _plane_dense(out, "out")
    _packed_arg(upacked, lib.pwc_pyr1_wino_packed_bytes(), x.device, "pack_pyr1_wino filters")
    _bias_arg(bias, 16, x.device)
    with torch.cuda.device(x.device):
        rc = lib.pwc_pyr1_wino_fwd(x.data_ptr(), upacked.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W, float(leaky_slope),
                                   bsx, bsy, _stream(x))
    check(rc, "pwc_pyr1_wino_fwd")
    return out


def pyr1_wino_pair(x: torch.Tensor, upacked1: torch.Tensor, bias1: torch.Tensor, upacked2: torch.Tensor, bias2: torch.Tensor,
                   leaky_slope: float = 0.1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two Conv2d(16 -> 16, 3x3, pad 1) + bias + LeakyReLU layers in one launch (the map between them stays in LDS); out is not x."""
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    B, cin, H, W = x.shape
    if x.dtype != torch.float32 or cin != 16:
        raise ValueError("pyr1_wino_pair takes float32 [B,16,H,W], got %s %s" % (x.dtype, tuple(x.shape)))
    out = _out_arg(out, (B, 16, H, W), x.dtype, x.device)
    bsy = _plane_dense(out, "out")
    need = lib.pwc_pyr1_wino_packed_bytes()
    for up, bias in ((upacked1, bias1), (upacked2, bias2)):
        _packed_arg(up, need, x.device, "pack_pyr1_wino filters")
        _bias_arg(bias, 16, x.device)
    with torch.cuda.device(x.device):
        rc = lib.pwc_pyr1_wino_pair_fwd(x.data_ptr(), upacked1.data_ptr(), bias1.data_ptr(), upacked2.data_ptr(), bias2.data_ptr(),
                                        out.data_ptr(), B, H, W, float(leaky_slope), bsx, bsy, _stream(x))
    check(rc, "pwc_pyr1_wino_pair_fwd")
    return out


def conv3x3_wino4_preferred(B: int, cin: int, H: int, W: int, cout: int, dilation: int = 1) -> bool:
    """Measured rule: does Winograd F(4x4,3x3) beat F(2x2,3x3) for this layer (large, well-filled maps, dilation 1)?"""
    return bool(_lib.load().pwc_conv3x3_wino4_preferred(B, cin, H, W, cout, dilation))


def pack_conv3x3_wino4(weight: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] float32 device tensor -> G g Gt of F(4x4,3x3) in the kernel's LDS order (4x the filter bytes)."""
    if not weight.is_cuda:
        raise PwcHipError("weight is on %s: the HIP path needs device tensors" % weight.device)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.dtype != torch.float32:
        raise ValueError("expected float32 [Cout,Cin,3,3], got %s %s" % (weight.dtype, tuple(weight.shape)))
    lib = _lib.load()
    cout, cin = weight.shape[:2]
    up = torch.empty((lib.pwc_conv3x3_wino4_packed_bytes(cin, cout) // 4,), dtype=torch.float32, device=weight.device)
    w = weight.contiguous()
    with torch.cuda.device(w.device):
        rc = lib.pwc_conv3x3_wino4_pack(w.data_ptr(), up.data_ptr(), cin, cout, _stream(w))
    check(rc, "pwc_conv3x3_wino4_pack")
    return up


def conv3x3_wino4_workspace_bytes(B: int, cin: int, H: int, W: int, cout: int) -> int:
    """Scratch bytes the tail split of this layer's F(4x4) launches wants (0 = no partial last round worth splitting)."""
    return _query_bytes(_lib.load().pwc_conv3x3_wino4_workspace_bytes(B, cin, H, W, cout), "conv")


def conv3x3_wino4(x: torch.Tensor, upacked: torch.Tensor, bias: torch.Tensor, cout: int, leaky_slope: Optional[float] = 0.1,
                  out: Optional[torch.Tensor] = None, split2: bool = False, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 / stride 1 / padding 1 convolution + bias (+ LeakyReLU) by Winograd F(4x4,3x3) on the matrix cores (fp32; W % 4 == 0).
    split2: the result is stored as its four pixel lattices, [4B, cout, H/2, W/2] with image 4b + 2(y & 1) + (x & 1) -- the input
    layout in which the next, twice-as-dilated layer is a dilation-1 convolution (lattice_unsplit is the inverse).
    workspace (conv3x3_wino4_workspace_bytes): lets a launch whose last round of workgroups would leave most CUs idle run that
    round's tiles as input-channel slices (same result up to the fp32 summation order of those tiles; deterministic)."""
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    B, cin, H, W = x.shape
    if x.dtype != torch.float32:
        raise ValueError("conv3x3_wino4 is fp32 only")
    oshape = (4 * B, cout, H // 2, W // 2) if split2 else (B, cout, H, W)
    if split2 and (H % 2 or W % 8):
        raise ValueError("split2 needs even H and W % 8 == 0")
    out = _out_arg(out, oshape, x.dtype, x.device)
    bsy = _plane_dense(out, "out")
    _packed_arg(upacked, lib.pwc_conv3x3_wino4_packed_bytes(cin, cout), x.device, "F(4x4,3x3) filters")
    _bias_arg(bias, cout, x.device)
    ws_ptr, ws_bytes = _workspace_args(workspace, x)
    with torch.cuda.device(x.device):
        rc = lib.pwc_conv3x3_wino4_fwd(x.data_ptr(), upacked.data_ptr(), bias.data_ptr(), out.data_ptr(), B, cin, H, W, cout, 1,
                                       (FLAG_ACT_LEAKY if leaky_slope is not None else 0) | (_lib.FLAG_CONV_SPLIT2 if split2 else 0),
                                       float(leaky_slope or 0.0), bsx, bsy, ws_ptr, ws_bytes, _stream(x))
    check(rc, "pwc_conv3x3_wino4_fwd")
    return out


def kitti_ingest(pairs_u8: torch.Tensor, mean, std, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 RGB pairs [n,2,H,W,3] on the device -> float32 [n,6,Hp,Wp] (Hp, Wp = H, W rounded up to multiples of 64): ToTensor +
    (v - mean) / std per channel, the two images concatenated along the channels, replicate padding (inference_kitti.py:53-63,175-178,
    208-210) as one kernel (C-ABI pwc_kitti_ingest_u8)."""
    if not pairs_u8.is_cuda or pairs_u8.dtype != torch.uint8 or pairs_u8.dim() != 5 or pairs_u8.shape[1] != 2 or pairs_u8.shape[4] != 3 \
            or not pairs_u8.is_contiguous():
        raise ValueError("pairs_u8 must be a contiguous uint8 device tensor [n,2,H,W,3]")
    n, _, H, W, _ = pairs_u8.shape
    Hp, Wp = pad64(H, W)[:2]
    out = _out_arg(out, (n, 6, Hp, Wp), torch.float32, pairs_u8.device)
    bso = _plane_dense(out, "out")
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    with torch.cuda.device(pairs_u8.device):
        rc = _lib.load().pwc_kitti_ingest_u8(pairs_u8.data_ptr(), out.data_ptr(), n, H, W, m3, s3, bso, _stream(pairs_u8))
    check(rc, "pwc_kitti_ingest_u8")
    return out


def flow_upsample(flow_q: torch.Tensor, crop_h: int, crop_w: int, out_h: int, out_w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n,2,Hq,Wq] -> [n,2,out_h,out_w]: crop to the top-left crop_h x crop_w, bilinear resize (align_corners=True), u * out_w / crop_w,
    v * out_h / crop_h -- `unpad` + `flow_resize` of inference_kitti.py:66-91 as one kernel (C-ABI pwc_flow_upsample_f32)."""
    if not flow_q.is_cuda or flow_q.dtype != torch.float32 or flow_q.dim() != 4 or flow_q.shape[1] != 2:
        raise ValueError("flow_q must be a float32 device tensor [n,2,Hq,Wq]")
    n, _, Hq, Wq = flow_q.shape
    bsq = _plane_dense(flow_q, "flow_q")
    out = _out_arg(out, (n, 2, out_h, out_w), torch.float32, flow_q.device, contiguous=True)
    with torch.cuda.device(flow_q.device):
        rc = _lib.load().pwc_flow_upsample_f32(flow_q.data_ptr(), out.data_ptr(), n, Hq, Wq, crop_h, crop_w, out_h, out_w, bsq, _stream(flow_q))
    check(rc, "pwc_flow_upsample_f32")
    return out


def pil_resize_supported(in_hw, out_hw) -> bool:
    """True when the Pillow-exact resize kernels take this geometry: any upscale and a downscale of at most 8 per axis, more only to
    an output shorter than a tile (16 rows, 64 columns) whose coefficient rows and source span still fit one (there is no fallback)."""
    (ih, iw), (oh, ow) = in_hw, out_hw
    if min(ih, iw, oh, ow) <= 0 or max(ih, iw, oh, ow) >= 2 ** 31:
        return False
    return bool(_lib.load().pwc_pil_resize_supported(int(ih), int(iw), int(oh), int(ow)))


def _pil_axis_arg(tab, out_size: int, coef_dtype, device, name: str) -> Tuple[int, int, int]:
    """(bounds, coefficients, ksize) of one axis as pil_resize makes them -> (bounds pointer, coefficient pointer, ksize)."""
    bounds, coef, ks = tab
    return (_table_arg(bounds, torch.int32, 2 * out_size, device, name + " bounds"),
            _table_arg(coef, coef_dtype, ks * out_size, device, name + " coefficients"), int(ks))


def pil_resize_frames(frames_u8: torch.Tensor, size: Tuple[int, int], xtab, ytab, lut: torch.Tensor, out: torch.Tensor,
                      out_u8: Optional[torch.Tensor] = None, group: Optional[int] = None) -> torch.Tensor:
    """uint8 RGB frames [n,H,W,3] -> out float32 [group, 3*ceil(n/group), h, w] (dense planes, free batch stride): Pillow's BILINEAR
    resize in its 8-bit fixed point, then lut[c][byte] (C-ABI pwc_pil_resize_frames_u8).  xtab / ytab: (bounds int32 [O,2],
    coefficients int32 [O,ksize], ksize) on the device; lut float32 [3,256]; out_u8: optional resized bytes [n,h,w,3]."""
    _require_device(frames_u8, "frames_u8")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise ValueError("frames_u8 must be a contiguous uint8 device tensor [n,H,W,3]")
    n, H, W, _ = frames_u8.shape
    h, w = size
    group = n if group is None else int(group)
    dev = frames_u8.device
    if group <= 0:
        raise ValueError("group must be positive")
    want = (min(group, n), 3 * ((n + group - 1) // group), h, w)
    if out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != want:
        raise ValueError("out must be float32 %s on %s, got %s %s on %s" % (want, dev, out.dtype, tuple(out.shape), out.device))
    bso = _plane_dense(out, "out")
    if out_u8 is not None and (out_u8.dtype != torch.uint8 or tuple(out_u8.shape) != (n, h, w, 3) or out_u8.device != dev
                               or not out_u8.is_contiguous()):
        raise ValueError("out_u8 must be a contiguous uint8 %s tensor on %s" % ((n, h, w, 3), dev))
    xb, xk, xks = _pil_axis_arg(xtab, w, torch.int32, dev, "x")
    yb, yk, yks = _pil_axis_arg(ytab, h, torch.int32, dev, "y")
    lp = _table_arg(lut, torch.float32, 768, dev, "lut")
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_pil_resize_frames_u8(frames_u8.data_ptr(), out.data_ptr(), _ptr(out_u8), n, H, W, h, w, xb, xk, xks,
                                                  yb, yk, yks, lp, bso, group, _stream(frames_u8))
    check(rc, "pwc_pil_resize_frames_u8")
    return out


def pil_resize_planes(x: torch.Tensor, size: Tuple[int, int], xtab, ytab, factors: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 planes [n,c,h,w] (dense planes, free batch stride) -> [n,c,H,W] as Pillow resizes mode "F" images (double accumulation
    in tap order, float32 between the passes), times factors[c] (float32 [c] on the device) when given (C-ABI
    pwc_pil_resize_planes_f32).  xtab / ytab: (bounds int32 [O,2], coefficients float64 [O,ksize], ksize) on the device."""
    if x.dtype != torch.float32:
        raise ValueError("x must be float32, got %s" % x.dtype)
    x = densify(x)
    bsx = _plane_dense(x, "x")
    n, c, h, w = x.shape
    H, W = size
    out = _out_arg(out, (n, c, H, W), torch.float32, x.device, contiguous=True)
    xb, xk, xks = _pil_axis_arg(xtab, W, torch.float64, x.device, "x")
    yb, yk, yks = _pil_axis_arg(ytab, H, torch.float64, x.device, "y")
    fp = None if factors is None else _table_arg(factors, torch.float32, c, x.device, "factors")
    with torch.cuda.device(x.device):
        rc = _lib.load().pwc_pil_resize_planes_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, H, W, xb, xk, xks, yb, yk, yks, fp, bsx,
                                                   _stream(x))
    check(rc, "pwc_pil_resize_planes_f32")
    return out


def pil_flow_eval_workspace_bytes(n: int, out_h: int, out_w: int) -> int:
    return _query_bytes(_lib.load().pwc_pil_flow_eval_workspace_bytes(n, out_h, out_w), "pil-flow-eval")


_EVAL_WS = {}
_GT_ORDERS = {"kitti": 1, "reference": 2}
_ENC_ORDERS = {"reference": 0, "kitti": 1}


def pil_flow_eval(x: torch.Tensor, size: Tuple[int, int], xtab, ytab, factors: Optional[torch.Tensor] = None,
                  gt: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, gt_order: str = "kitti",
                  enc_out: Optional[torch.Tensor] = None, enc_order: str = "reference", flow_out: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None):
    """float32 flow [n,2,h,w] (dense planes, free batch stride) resized to (H, W) as pil_resize_planes does (same tables, factors
    float32 [2] on the device or None) and, in the same launch, scored and / or encoded (C-ABI pwc_pil_flow_eval) -> (scores, totals).
    gt: torch.uint16 [n,H,W,3], samples {u, v, valid} with gt_order "kitti" or {valid, v, u} with "reference" (`valid` must be None),
    or float32 [n,2,H,W] with `valid` None / bool / uint8 [n,H,W] (gt_order concerns uint16 samples only).  scores: float32 [n,2] =
    per-sample (EPE, Fl in percent), NaN without a valid pixel; totals: int64 [n,3] = {bits of the fp64 sum of EPE, #valid, #outliers},
    a view of the head of the workspace, which is cached per (device, n, H, W) -- consume it before the next call of that shape.  Both
    are None without gt.  enc_out: contiguous torch.uint16 [n,H,W,3] (2-byte aligned is enough) that receives save_flow's samples,
    {1, v, u} with enc_order "reference" or {u, v, 1} with "kitti".  flow_out: contiguous float32 [n,2,H,W] that receives the resized
    flow itself.  At least one of gt / enc_out / flow_out is needed.  Device tensors only, no host synchronisation, bit-reproducible."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 2:
        raise ValueError("x must be a float32 tensor [n,2,h,w]")
    x = densify(x)
    bsx = _plane_dense(x, "x")
    n, _, h, w = x.shape
    H, W = (int(v) for v in size)
    dev = x.device
    if gt is None and enc_out is None and flow_out is None:
        raise ValueError("nothing requested: give gt, enc_out or flow_out")
    if gt_order not in _GT_ORDERS or enc_order not in _ENC_ORDERS:
        raise ValueError("gt_order / enc_order must be 'kitti' or 'reference', got %r / %r" % (gt_order, enc_order))
    kind = 0
    if gt is not None:
        kind, valid = _kitti_gt_arg(gt, valid, n, H, W, dev)
        if kind == 1:
            kind = _GT_ORDERS[gt_order]
    elif valid is not None:
        raise ValueError("valid goes with a float32 gt")
    if enc_out is not None and (enc_out.dtype != torch.uint16 or tuple(enc_out.shape) != (n, H, W, 3) or enc_out.device != dev
                                or not enc_out.is_contiguous()):
        raise ValueError("enc_out must be contiguous torch.uint16 %s on %s" % ((n, H, W, 3), dev))
    if flow_out is not None:
        _out_arg(flow_out, (n, 2, H, W), torch.float32, dev, contiguous=True)
    xb, xk, xks = _pil_axis_arg(xtab, W, torch.float64, dev, "x")
    yb, yk, yks = _pil_axis_arg(ytab, H, torch.float64, dev, "y")
    fp = None if factors is None else _table_arg(factors, torch.float32, 2, dev, "factors")
    ws, nb = None, 0
    with torch.cuda.device(dev):
        if gt is not None:
            out = _out_arg(out, (n, 2), torch.float32, dev, contiguous=True)
            nb = pil_flow_eval_workspace_bytes(n, H, W)
            key = (dev, n, H, W)
            ws = _EVAL_WS.get(key)
            if ws is None:
                ws = _EVAL_WS[key] = torch.empty(nb // 8, dtype=torch.int64, device=dev)
        rc = _lib.load().pwc_pil_flow_eval(x.data_ptr(), n, h, w, H, W, xb, xk, xks, yb, yk, yks, fp, bsx, _ptr(gt), kind, _ptr(valid),
                                           _ptr(flow_out), _ptr(enc_out), _ENC_ORDERS[enc_order], _ptr(ws), nb,
                                           _ptr(out) if gt is not None else None, _stream(x))
    check(rc, "pwc_pil_flow_eval")
    if gt is None:
        return None, None
    return out, ws[:3 * n].view(n, 3)


def _cv_axis_arg(tab, out_size: int, device, name: str) -> Tuple[int, int]:
    """(first taps int32 [O], weights float32 [O]) of one axis as cv_resize.axis_table makes them, on the device -> their pointers."""
    s0, fx = tab
    for t in (s0, fx):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("%s axis table must be device tensors" % name)
    return (_table_arg(s0, torch.int32, out_size, device, name + " first taps"),
            _table_arg(fx, torch.float32, out_size, device, name + " weights"))


def cv_resize_frames(frames_u8: torch.Tensor, size: Tuple[int, int], xtab, ytab, lut: torch.Tensor, out: torch.Tensor,
                     flip_channels: bool = True, group: Optional[int] = None) -> torch.Tensor:
    """uint8 frames [n,H,W,3] -> out float32 [group, 3*ceil(n/group), h, w] (dense planes, free batch stride): cv2.resize's INTER_LINEAR
    in its 11-bit fixed point, the channel order flipped when asked, then lut[c_out][byte] (C-ABI pwc_cv_resize_frames_u8).  xtab /
    ytab: (first taps int32 [O], weights float32 [O]) on the device; lut float32 [3,256] on the device, indexed by the output channel."""
    if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 \
            or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise ValueError("frames_u8 must be a contiguous uint8 device tensor [n,H,W,3]")
    n, H, W, _ = frames_u8.shape
    h, w = (int(v) for v in size)
    group = n if group is None else int(group)
    dev = frames_u8.device
    if group <= 0 or min(n, H, W, h, w) <= 0:
        raise ValueError("group and every size must be positive")
    want = (min(group, n), 3 * ((n + group - 1) // group), h, w)
    if not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != want:
        raise ValueError("out must be float32 %s on %s" % (want, dev))
    if not torch.is_tensor(lut) or not lut.is_cuda:
        raise ValueError("lut must be a float32 device tensor [3,256]")
    bso = _plane_dense(out, "out")
    xs, xf = _cv_axis_arg(xtab, w, dev, "x")
    ys, yf = _cv_axis_arg(ytab, h, dev, "y")
    lp = _table_arg(lut, torch.float32, 768, dev, "lut")
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_cv_resize_frames_u8(frames_u8.data_ptr(), out.data_ptr(), n, H, W, h, w, xs, xf, ys, yf, lp,
                                                 1 if flip_channels else 0, bso, group, _stream(frames_u8))
    check(rc, "pwc_cv_resize_frames_u8")
    return out


def cv_resize_flow(flow: torch.Tensor, size: Tuple[int, int], xtab, ytab, gain: float = 1.0, fu: float = 1.0, fv: float = 1.0,
                   hwc: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 flow [n,2,h,w] (dense planes, free batch stride) -> [n,2,H,W], or [n,H,W,2] with hwc: (flow * gain) resized as cv2.resize
    does float images (INTER_LINEAR, float32 passes), channel 0 times fu and channel 1 times fv (C-ABI pwc_cv_resize_flow_f32).
    xtab / ytab: (first taps int32 [O], weights float32 [O]) on the device."""
    if not torch.is_tensor(flow) or not flow.is_cuda or flow.dtype != torch.float32 or flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("flow must be a float32 device tensor [n,2,h,w]")
    n, _, h, w = flow.shape
    H, W = (int(v) for v in size)
    if min(n, h, w, H, W) <= 0:
        raise ValueError("every size must be positive")
    bss = _plane_dense(flow, "flow")
    out = _out_arg(out, (n, H, W, 2) if hwc else (n, 2, H, W), torch.float32, flow.device, contiguous=True)
    xs, xf = _cv_axis_arg(xtab, W, flow.device, "x")
    ys, yf = _cv_axis_arg(ytab, H, flow.device, "y")
    with torch.cuda.device(flow.device):
        rc = _lib.load().pwc_cv_resize_flow_f32(flow.data_ptr(), out.data_ptr(), n, h, w, H, W, xs, xf, ys, yf, float(gain), float(fu),
                                                float(fv), 1 if hwc else 0, bss, _stream(flow))
    check(rc, "pwc_cv_resize_flow_f32")
    return out


def cv_warp_perspective(frames_u8: torch.Tensor, mats: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """uint8 frames [n,H,W,3] -> out uint8 [n,h,w,3] (both dense frames, free batch strides): cv2.warpPerspective's INTER_LINEAR /
    BORDER_CONSTANT 0 with the INVERSE maps `mats`, float64 [9] (one for all frames) or [n,9] on the device (C-ABI
    pwc_cv_warp_perspective_u8)."""
    sbs = _frames_dense(frames_u8, "frames_u8")
    dbs = _frames_dense(out, "out")
    n, H, W, _ = frames_u8.shape
    dev = frames_u8.device
    if out.shape[0] != n or out.device != dev:
        raise ValueError("out must hold %d frames on %s" % (n, dev))
    h, w = out.shape[1:3]
    if not torch.is_tensor(mats) or mats.dim() not in (1, 2) or mats.shape[-1] != 9 or (mats.dim() == 2 and mats.shape[0] != n):
        raise ValueError("mats must be float64 [9] or [%d,9]" % n)
    mp = _table_arg(mats, torch.float64, 9 * (n if mats.dim() == 2 else 1), dev, "mats")
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_cv_warp_perspective_u8(frames_u8.data_ptr(), out.data_ptr(), n, H, W, h, w, mp, 9 if mats.dim() == 2 else 0,
                                                    sbs, dbs, _stream(frames_u8))
    check(rc, "pwc_cv_warp_perspective_u8")
    return out


def video_ingest(frames_u8: torch.Tensor, out: Optional[torch.Tensor] = None, bgr: bool = True) -> torch.Tensor:
    """Raw frames uint8 [n,H,W,3] on the device (dense frames, free batch stride: e.g. one slot of a larger buffer) -> float32
    [n,3,Hp,Wp] (Hp, Wp = H, W rounded up to multiples of 64): channel flip when `bgr`, byte / 255 as an IEEE division, HWC -> CHW and
    replicate padding at the bottom / right -- frame_to_tensor + pad_to_multiple_of_64 of pwc_extract_flow_video.py:27-42 as one kernel
    (C-ABI pwc_video_ingest_u8).  out: dense planes with a free batch stride.  Every argument is checked before the library loads."""
    n, H, W = _raw_frames_shape(frames_u8, "frames_u8")
    Hp, Wp = pad64(H, W)[:2]
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (n, 3, Hp, Wp):
            raise ValueError("out must be float32 %s, got %s %s" % ((n, 3, Hp, Wp), getattr(out, "dtype", type(out).__name__),
                                                                   tuple(getattr(out, "shape", ()))))
        if out.device != frames_u8.device:
            raise ValueError("out is on %s, frames_u8 on %s" % (out.device, frames_u8.device))
    _require_device(frames_u8, "frames_u8")
    sbs = _frames_dense(frames_u8, "frames_u8")
    out = _out_arg(out, (n, 3, Hp, Wp), torch.float32, frames_u8.device)
    bso = _plane_dense(out, "out")
    with torch.cuda.device(frames_u8.device):
        rc = _lib.load().pwc_video_ingest_u8(frames_u8.data_ptr(), out.data_ptr(), n, H, W, 1 if bgr else 0, sbs, bso, _stream(frames_u8))
    check(rc, "pwc_video_ingest_u8")
    return out


def kitti_score_workspace_bytes(n: int, out_h: int, out_w: int) -> int:
    return _query_bytes(_lib.load().pwc_kitti_score_workspace_bytes(n, out_h, out_w), "kitti-score")


_SCORE_WS = {}


def kitti_score(flow_q: torch.Tensor, crop_h: int, crop_w: int, out_h: int, out_w: int, gt: torch.Tensor,
                valid: Optional[torch.Tensor] = None, flow_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                raw: bool = False):
    """float32 [n,2] = per-sample (EPE, Fl-all in percent) of pwc_kitti_score: the quarter-resolution flow [n,2,Hq,Wq] is cropped and
    upsampled exactly as `flow_upsample` does and scored against the ground truth in the same pass (epe_metric / fl_all_metric of
    inference_kitti.py:94-128); NaN for a sample without a valid pixel.  gt: torch.uint16 [n,out_h,out_w,3] (the KITTI PNG samples, R G
    B; validity is the blue sample, `valid` must be None) or float32 [n,2,out_h,out_w] with `valid` None / bool or uint8 [n,out_h,out_w].
    flow_out: optional float32 [n,2,out_h,out_w] that also receives the full-resolution flow.  raw=True returns (out, sum_epe float64
    [n], n_valid int64 [n], n_outlier int64 [n]): views of the workspace, which is cached per (device, shape) -- consume them before the
    next call of that shape.  Device tensors only, no host synchronisation, bit-reproducible."""
    if not flow_q.is_cuda or flow_q.dtype != torch.float32 or flow_q.dim() != 4 or flow_q.shape[1] != 2:
        raise ValueError("flow_q must be a float32 device tensor [n,2,Hq,Wq]")
    n, _, Hq, Wq = flow_q.shape
    dev = flow_q.device
    bsq = _plane_dense(flow_q, "flow_q")
    out_h, out_w = int(out_h), int(out_w)
    kind, valid = _kitti_gt_arg(gt, valid, n, out_h, out_w, dev)
    if flow_out is not None and (tuple(flow_out.shape) != (n, 2, out_h, out_w) or flow_out.dtype != torch.float32 or flow_out.device != dev
                                 or not flow_out.is_contiguous()):
        raise ValueError("flow_out must be contiguous float32 %s on %s" % ((n, 2, out_h, out_w), dev))
    out = _out_arg(out, (n, 2), torch.float32, dev, contiguous=True)
    with torch.cuda.device(dev):
        nb = kitti_score_workspace_bytes(max(n, 1), max(out_h, 1), max(out_w, 1))
        key = (dev, n, out_h, out_w)
        ws = _SCORE_WS.get(key)
        if ws is None:
            ws = _SCORE_WS[key] = torch.empty(nb // 8, dtype=torch.int64, device=dev)
        rc = _lib.load().pwc_kitti_score(flow_q.data_ptr(), n, Hq, Wq, int(crop_h), int(crop_w), out_h, out_w, bsq, gt.data_ptr(), kind,
                                         _ptr(valid), _ptr(flow_out), ws.data_ptr(), nb, out.data_ptr(),
                                         _stream(flow_q))
    check(rc, "pwc_kitti_score")
    if raw:
        head = ws[:3 * n].view(n, 3)
        return out, head[:, 0].view(torch.float64), head[:, 1], head[:, 2]
    return out


# record layout of pwc_flow_compare (include/pwc_hip.h PWC_FC_*): one float64 row per sample, then the batch row
FLOW_COMPARE_MAX_TAUS = 8
FLOW_COMPARE_FIELDS = 44
FC_N, FC_P, FC_SUM_D2, FC_SUM_ABS_D, FC_SUM_A2, FC_SUM_B2, FC_SUM_ABS_A, FC_SUM_A, FC_SUM_B, FC_SUM_AB, FC_SUM_EPE = range(11)
FC_MAX_ABS, FC_EPE_MAX, FC_MIN_A, FC_MAX_A, FC_MIN_B, FC_MAX_B = range(11, 17)
FC_COUNT0 = 17
FC_L2, FC_MAE, FC_REL_L2, FC_REL_MAE, FC_PEARSON, FC_COSINE, FC_EPE_MEAN = range(25, 32)
FC_AGREE0 = 32
FC_MEAN_A, FC_STD_A, FC_MEAN_B, FC_STD_B = range(40, 44)


def flow_compare_workspace_bytes(n: int, H: int, W: int) -> int:
    return _query_bytes(_lib.load().pwc_flow_compare_workspace_bytes(n, H, W), "flow-compare")


def _compare_flow_arg(t: torch.Tensor, name: str) -> int:
    """One side of flow_compare: float32 device [n,2,H,W] with dense planes -> batch stride in elements."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 2:
        raise ValueError("%s must be a tensor [n,2,H,W], got %s" % (name, tuple(getattr(t, "shape", ()))))
    if t.dtype in (torch.float16, torch.bfloat16):
        raise TypeError("%s is %s: flow_compare reads float32 only (widen a half-precision flow with .float() first; the report "
                        "is defined on float32 values)" % (name, t.dtype))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    return _plane_dense(t, name)


def flow_compare_taus(taus) -> Tuple[float, ...]:
    """The thresholds of flow_compare as a tuple of Python floats, checked: 1..8 finite non-negative values."""
    taus = tuple(float(t) for t in taus)
    if not 1 <= len(taus) <= FLOW_COMPARE_MAX_TAUS:
        raise ValueError("flow_compare takes 1..%d thresholds, got %d" % (FLOW_COMPARE_MAX_TAUS, len(taus)))
    for t in taus:
        if not (t >= 0.0 and math.isfinite(t)):
            raise ValueError("thresholds must be finite and non-negative, got %r" % (t,))
    return taus


def flow_compare(a: torch.Tensor, b: torch.Tensor, taus=(0.25, 0.5, 1.0, 2.0), epe_map: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [n+1, FLOW_COMPARE_FIELDS] record of pwc_flow_compare: compare_flows / print_flow_stats of onnx_pth_compare.py for the
    float32 device flows a (the reference side) and b, [n,2,H,W] with dense planes and free batch strides.  Row s < n is sample s,
    row n the whole batch (the samples stacked along H); columns are the FC_* indices.  taus: 1..8 EPE thresholds (agreement is
    epe <= tau, compared in float32).  epe_map: optional contiguous float32 [n,H,W] that receives the per-pixel EPE.  workspace:
    optional device tensor of flow_compare_workspace_bytes(n, H, W) bytes, 8-byte aligned (allocated when absent).  Device tensors
    only, no host synchronisation, bit-reproducible, capturable in a graph when workspace and out are given."""
    bsa = _compare_flow_arg(a, "a")
    bsb = _compare_flow_arg(b, "b")
    if tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise ValueError("a and b must have one shape and device, got %s on %s and %s on %s"
                         % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    n, _, H, W = a.shape
    if n < 1 or H < 1 or W < 1:
        raise ValueError("flow_compare needs a non-empty [n,2,H,W], got %s" % (tuple(a.shape),))
    taus = flow_compare_taus(taus)
    dev = a.device
    if epe_map is not None and (tuple(epe_map.shape) != (n, H, W) or epe_map.dtype != torch.float32 or epe_map.device != dev
                                or not epe_map.is_contiguous()):
        raise ValueError("epe_map must be contiguous float32 %s on %s" % ((n, H, W), dev))
    out = _out_arg(out, (n + 1, FLOW_COMPARE_FIELDS), torch.float64, dev, contiguous=True)
    need = flow_compare_workspace_bytes(n, H, W)
    if workspace is None:
        workspace, _ = _scratch(need, dev)
    wp, wb = _workspace_args(workspace, a)
    if wb < need:
        raise ValueError("workspace has %d bytes, flow_compare needs %d" % (wb, need))
    tau_arr = (ctypes.c_float * len(taus))(*taus)
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_flow_compare(a.data_ptr(), b.data_ptr(), n, H, W, bsa, bsb, tau_arr, len(taus), _ptr(epe_map), wp, wb,
                                          out.data_ptr(), _stream(a))
    check(rc, "pwc_flow_compare")
    return out


def _flow_crop_arg(flow: torch.Tensor, crop) -> Tuple[int, int, int, int, int, int]:
    """The [n,2,Hq,Wq] float32 device flow of the picture operators and its top-left crop -> (n, Hq, Wq, crop_h, crop_w, batch stride)."""
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("flow must be [n,2,Hq,Wq], got %s" % (tuple(flow.shape),))
    if flow.dtype != torch.float32:
        raise TypeError("flow must be float32, got %s" % flow.dtype)
    n, _, Hq, Wq = flow.shape
    ch, cw = (Hq, Wq) if crop is None else (int(crop[0]), int(crop[1]))
    if n < 1 or not (1 <= ch <= Hq and 1 <= cw <= Wq):
        raise ValueError("crop %dx%d does not fit the %dx%d map (or the batch is empty)" % (ch, cw, Hq, Wq))
    return n, Hq, Wq, ch, cw, _plane_dense(flow, "flow")


def _clip_arg(clip_flow: Optional[float]) -> Tuple[int, float]:
    if clip_flow is None:
        return 0, 0.0
    if not float(clip_flow) > 0.0:
        raise ValueError("clip_flow must be positive, got %r" % (clip_flow,))
    return 1, float(clip_flow)


def flow_stats_workspace_bytes(n: int, crop_h: int, crop_w: int) -> int:
    return _query_bytes(_lib.load().pwc_flow_stats_workspace_bytes(n, crop_h, crop_w), "flow-stats")


def flow_stats(flow: torch.Tensor, crop: Optional[Tuple[int, int]] = None, clip_flow: Optional[float] = None, threshold: float = 1.0,
               out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [n,4] records of pwc_flow_stats over the top-left `crop` of flow [n,2,Hq,Wq]: column 0 the maximum radius after the
    optional clip_flow rescale (what flow_to_color normalises by), column 1 the int32 bits of the number of pixels whose magnitude is >
    threshold (`.view(torch.int32)`), columns 2-3 their mean (u, v), zero when there are none (calculate_dominant_direction).
    workspace: optional device tensor of flow_stats_workspace_bytes(n, crop_h, crop_w) bytes, 8-byte aligned (allocated when absent).
    Device tensors only, no host synchronisation, bit-reproducible."""
    n, Hq, Wq, ch, cw, bs = _flow_crop_arg(flow, crop)
    use_clip, clip = _clip_arg(clip_flow)
    dev = flow.device
    out = _out_arg(out, (n, 4), torch.float32, dev, contiguous=True)
    need = flow_stats_workspace_bytes(n, ch, cw)
    if workspace is None:
        workspace, _ = _scratch(need, dev)
    wp, wb = _workspace_args(workspace, flow)
    if wb < need:
        raise ValueError("workspace has %d bytes, flow_stats needs %d" % (wb, need))
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_flow_stats(flow.data_ptr(), n, Hq, Wq, ch, cw, bs, use_clip, clip, float(threshold), wp, wb, out.data_ptr(),
                                        _stream(flow))
    check(rc, "pwc_flow_stats")
    return out


def flow_color(flow: torch.Tensor, stats: torch.Tensor, crop: Optional[Tuple[int, int]] = None, clip_flow: Optional[float] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [n,crop_h,crop_w,3] RGB colour-wheel image of pwc_flow_color (flow_to_color, pwc_extract_flow.py:58-123); `stats` is
    flow_stats' record of the same flow, crop and clip_flow, read on the device.  `out` may start at any byte address."""
    n, Hq, Wq, ch, cw, bs = _flow_crop_arg(flow, crop)
    use_clip, clip = _clip_arg(clip_flow)
    dev = flow.device
    if tuple(stats.shape) != (n, 4) or stats.dtype != torch.float32 or stats.device != dev or not stats.is_contiguous():
        raise ValueError("stats must be the contiguous float32 [%d,4] record of flow_stats on %s" % (n, dev))
    out = _out_arg(out, (n, ch, cw, 3), torch.uint8, dev, contiguous=True)
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_flow_color(flow.data_ptr(), n, Hq, Wq, ch, cw, bs, use_clip, clip, stats.data_ptr(), out.data_ptr(), _stream(flow))
    check(rc, "pwc_flow_color")
    return out


def flow_quiver(flow: torch.Tensor, frame_h: int, frame_w: int, step: int, vec_scale: Tuple[float, float], gain: float, tip_rule: int,
                min_mag: float, crop: Optional[Tuple[int, int]] = None, dominant: Optional[torch.Tensor] = None,
                angle_threshold: float = 30.0, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """(vec float32 [n,Gy,Gx,2], tip int32 [n,Gy,Gx,2], flags uint8 [n,Gy,Gx]) of pwc_flow_quiver: the arrow grid every `step` pixels
    of a frame_h x frame_w frame, from the top-left `crop` of flow [n,2,Hq,Wq] resized like cv2.resize at the grid points only.
    tip_rule 0 rounds half to even, 1 truncates; flags bit 0 = keep (magnitude not below min_mag), bit 1 = aligned with `dominant`
    (float32 [n,2] on the device, rows may be strided, e.g. flow_stats(...)[:, 2:4]; None = every arrow aligned)."""
    frame_h, frame_w, step, tip_rule = int(frame_h), int(frame_w), int(step), int(tip_rule)
    if frame_h < 1 or frame_w < 1:
        raise ValueError("frame size must be positive, got %dx%d" % (frame_h, frame_w))
    if step < 1:
        raise ValueError("step must be >= 1, got %d" % step)
    if tip_rule not in (0, 1):
        raise ValueError("tip_rule must be 0 (round half to even) or 1 (truncate), got %d" % tip_rule)
    n, Hq, Wq, ch, cw, bs = _flow_crop_arg(flow, crop)
    dev = flow.device
    dom_stride = 0
    if dominant is not None:
        if tuple(dominant.shape) != (n, 2) or dominant.dtype != torch.float32 or dominant.device != dev or dominant.stride(1) != 1 \
                or (n > 1 and dominant.stride(0) < 2):
            raise ValueError("dominant must be float32 [%d,2] on %s with unit inner stride" % (n, dev))
        dom_stride = max(int(dominant.stride(0)), 2)
    gy, gx = (frame_h + step - 1) // step, (frame_w + step - 1) // step
    o = out if out is not None else (None, None, None)
    if len(o) != 3:
        raise ValueError("out must be (vec, tip, flags)")
    vec = _out_arg(o[0], (n, gy, gx, 2), torch.float32, dev, contiguous=True)
    tip = _out_arg(o[1], (n, gy, gx, 2), torch.int32, dev, contiguous=True)
    flags = _out_arg(o[2], (n, gy, gx), torch.uint8, dev, contiguous=True)
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_flow_quiver(flow.data_ptr(), n, Hq, Wq, ch, cw, bs, frame_h, frame_w, step, float(vec_scale[0]),
                                         float(vec_scale[1]), float(gain), tip_rule, float(min_mag), _ptr(dominant), dom_stride,
                                         float(angle_threshold), vec.data_ptr(), tip.data_ptr(), flags.data_ptr(), _stream(flow))
    check(rc, "pwc_flow_quiver")
    return vec, tip, flags


def vanishing_workspace_bytes(n: int, gy: int, gx: int, grid: int = 64) -> int:
    return _query_bytes(_lib.load().pwc_vanishing_workspace_bytes(int(n), int(gy), int(gx), int(grid)), "vanishing-point")


def vanishing_point(vec: torch.Tensor, frame_h: int, frame_w: int, step: int, min_mag: float = 1.0, max_points: int = 300,
                    grid: int = 64, min_pairs: int = 50, order: Optional[torch.Tensor] = None,
                    out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, workspace: Optional[torch.Tensor] = None):
    """(vp float64 [n,5], info int32 [n,6]) of pwc_vanishing_point: per frame (vx, vy, prob, centre x, centre y) and (status, N used,
    pairs kept, best gx, best gy, inliers) from the arrow grid vec float32 [n,Gy,Gx,2] of flow_quiver for the same frame and step.
    status 0 refined, 1 bin centre kept, 2 fewer than 5 vectors, 3 fewer than min_pairs intersections, 4 empty histogram; the vp row
    of a status >= 2 is (NaN, NaN, 0, NaN, NaN).  order: int32 permutation of the Gy*Gx cells on the device, required when there are
    more cells than max_points (it decides which kept cells are used when more than max_points are kept; what a table that is no
    permutation does is spelled out in include/pwc_hip.h).  A cell with a NaN or infinite component is dropped like one below min_mag.
    vec must be contiguous: a strided view is refused, not copied.  workspace: optional device tensor of vanishing_workspace_bytes(n, Gy, Gx, grid) bytes.
    Device tensors only, no host synchronisation, bit-reproducible."""
    frame_h, frame_w, step, max_points, grid, min_pairs = int(frame_h), int(frame_w), int(step), int(max_points), int(grid), int(min_pairs)
    if frame_h < 1 or frame_w < 1:
        raise ValueError("frame size must be positive, got %dx%d" % (frame_h, frame_w))
    if step < 1:
        raise ValueError("step must be >= 1, got %d" % step)
    if not 5 <= max_points <= 1024:
        raise ValueError("max_points must be in 5..1024, got %d" % max_points)
    if not 2 <= grid <= 128:
        raise ValueError("grid must be in 2..128, got %d" % grid)
    gy, gx = (frame_h + step - 1) // step, (frame_w + step - 1) // step
    if gy * gx > 65536:
        raise ValueError("%dx%d cells, at most 65536" % (gy, gx))
    if vec.dim() != 4 or tuple(vec.shape[1:]) != (gy, gx, 2) or vec.shape[0] < 1:
        raise ValueError("vec must be [n,%d,%d,2] for a %dx%d frame at step %d, got %s" % (gy, gx, frame_h, frame_w, step, tuple(vec.shape)))
    if vec.dtype != torch.float32:
        raise TypeError("vec must be float32, got %s" % vec.dtype)
    _require_device(vec, "vec")
    if not vec.is_contiguous():
        raise ValueError("vec must be contiguous (strides %s for shape %s); it is not copied" % (vec.stride(), tuple(vec.shape)))
    n, dev = vec.shape[0], vec.device
    if order is None:
        if gy * gx > max_points:
            raise ValueError("%d cells can exceed max_points %d: pass an order table" % (gy * gx, max_points))
        op = None
    else:
        op = _table_arg(order, torch.int32, gy * gx, dev, "order")
    o = out if out is not None else (None, None)
    if len(o) != 2:
        raise ValueError("out must be (vp, info)")
    vp = _out_arg(o[0], (n, 5), torch.float64, dev, contiguous=True)
    info = _out_arg(o[1], (n, 6), torch.int32, dev, contiguous=True)
    need = vanishing_workspace_bytes(n, gy, gx, grid)
    if workspace is None:
        workspace, _ = _scratch(need, dev)
    wp, wb = _workspace_args(workspace, vec)
    if wb < need:
        raise ValueError("workspace has %d bytes, vanishing_point needs %d" % (wb, need))
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_vanishing_point(vec.data_ptr(), n, gy, gx, frame_h, frame_w, step, float(min_mag), max_points, grid, min_pairs,
                                             op, vp.data_ptr(), info.data_ptr(), wp, wb, _stream(vec))
    check(rc, "pwc_vanishing_point")
    return vp, info


AUGMENT_RECORD_BYTES = 88     # sizeof(pwc_augment_params): six fp64, four fp32, six int32
AUGMENT_FULL_RECORD_BYTES = 128     # sizeof(pwc_augment_full_params): eight fp64, one fp32, eight uint16, eleven int32
AUGMENT_FULL_MAX_SHIFT = 32767      # PWC_AUGMENT_FULL_MAX_SHIFT


def _kitti_augment_call(symbol: str, record_bytes: int, frames, gt, params, crop_hw, valid, out, status):
    """The argument checks and the call shared by pwc_kitti_augment and pwc_kitti_augment_full (one signature, one slot layout)."""
    if frames.dim() != 5 or frames.shape[1] != 2 or frames.shape[4] != 3 or frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError("frames must be contiguous uint8 [n,2,Hs,Ws,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
    _require_device(frames, "frames")
    n, _, Hs, Ws, _ = frames.shape
    dev = frames.device
    ch, cw = int(crop_hw[0]), int(crop_hw[1])
    if n < 1 or not (1 <= ch <= Hs and 1 <= cw <= Ws):
        raise ValueError("crop %dx%d does not fit the %dx%d slot (or the batch is empty)" % (ch, cw, Hs, Ws))
    kind, valid = _kitti_gt_arg(gt, valid, n, Hs, Ws, dev)
    if params.dtype != torch.uint8 or tuple(params.shape) != (n, record_bytes) or params.device != dev or not params.is_contiguous():
        raise ValueError("params must be contiguous uint8 %s on %s" % ((n, record_bytes), dev))
    o = out if out is not None else (None, None, None)
    if len(o) != 3:
        raise ValueError("out must be (x, flow, valid)")
    x = _out_arg(o[0], (n, 6, ch, cw), torch.float32, dev, contiguous=True)
    flow = _out_arg(o[1], (n, 2, ch, cw), torch.float32, dev, contiguous=True)
    vout = _out_arg(o[2], (n, 1, ch, cw), torch.float32, dev, contiguous=True)
    status = _out_arg(status, (n,), torch.int32, dev, contiguous=True)
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), symbol)(frames.data_ptr(), gt.data_ptr(), kind, _ptr(valid), n, Hs, Ws, ch, cw, params.data_ptr(),
                                          x.data_ptr(), flow.data_ptr(), vout.data_ptr(), status.data_ptr(), _stream(frames))
    check(rc, symbol)
    return x, flow, vout, status


def kitti_augment(frames: torch.Tensor, gt: torch.Tensor, params: torch.Tensor, crop_hw: Tuple[int, int],
                  valid: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                  status: Optional[torch.Tensor] = None):
    """(x float32 [n,6,ch,cw], flow float32 [n,2,ch,cw], valid float32 [n,1,ch,cw], status int32 [n]) of pwc_kitti_augment: the reduced
    augmentation, crop and flip of KittiFlowDataset in one launch.  frames: uint8 [n,2,Hs,Ws,3] slots; gt: torch.uint16 [n,Hs,Ws,3]
    (the KITTI PNG samples, `valid` must be None) or float32 [n,2,Hs,Ws] with `valid` None / bool or uint8 [n,Hs,Ws]; sample b lies
    densely at the start of each of its slots with its own row stride W_b.  params: uint8 [n,88] device records (pwc_augment_params;
    opticalflow_amd.augment builds and validates them).  status[b] != 0 marks a record the kernel refused (that sample's outputs are
    zeros).  Device tensors only, no host synchronisation, bit-reproducible."""
    return _kitti_augment_call("pwc_kitti_augment", AUGMENT_RECORD_BYTES, frames, gt, params, crop_hw, valid, out, status)


def kitti_augment_full(frames: torch.Tensor, gt: torch.Tensor, params: torch.Tensor, crop_hw: Tuple[int, int],
                       valid: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                       status: Optional[torch.Tensor] = None):
    """(x float32 [n,6,ch,cw], flow float32 [n,2,ch,cw], mask float32 [n,1,ch,cw] -- fractional after a rotation --, status int32 [n]) of
    pwc_kitti_augment_full: train2.py's KittiAugmentationPipeline (crop, flip, rotation, translation, brightness / contrast, Gaussian
    blur) in one launch.  frames / gt / valid: the slot tensors of kitti_augment.  params: uint8 [n,128] device records
    (pwc_augment_full_params; opticalflow_amd.augment_full builds and validates them).  status[b] != 0 marks a record the kernel refused
    (that sample's outputs are zeros).  Device tensors only, no host synchronisation, bit-reproducible."""
    return _kitti_augment_call("pwc_kitti_augment_full", AUGMENT_FULL_RECORD_BYTES, frames, gt, params, crop_hw, valid, out, status)


def lattice_unsplit(x: torch.Tensor, batch: int, levels: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inverse of `levels` nested split2 stores: [batch * 4**levels, C, h, w] (contiguous) -> [batch, C, h << levels, w << levels]."""
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4 or x.shape[0] != batch * 4 ** levels:
        raise ValueError("x must be a contiguous float32 device tensor [batch * 4**levels, C, h, w]")
    _, C, h, w = x.shape
    oshape = (batch, C, h << levels, w << levels)
    out = _out_arg(out, oshape, x.dtype, x.device)
    bsy = _plane_dense(out, "out")
    with torch.cuda.device(x.device):
        rc = _lib.load().pwc_lattice_unsplit_f32(x.data_ptr(), out.data_ptr(), batch, C, h, w, levels, bsy, _stream(x))
    check(rc, "pwc_lattice_unsplit_f32")
    return out


def conv3x3_workspace_bytes(B: int, cin: int, H: int, W: int, cout: int, stride: int = 1, dilation: int = 1) -> int:
    """Scratch bytes the split-K route of this layer wants (0 = it never splits)."""
    return _query_bytes(_lib.load().pwc_conv2d_workspace_bytes(B, cin, H, W, cout, stride, dilation), "conv")


def head_upfeat_supported(B: int, H: int, W: int, min_tiles: int = 64) -> bool:
    """Geometry gate of pwc_head_upfeat_fwd (mirrors stream3x3_ok in csrc/pwc_stream3x3.hip).  min_tiles < 64: the gate of
    pwc_head_upfeat_ws_fwd with a workspace (Cin slices: stream3x3_head_upfeat_sliced_ok, at least 4 tiles)."""
    return (W % 4 == 0 and W >= int(os.environ.get("PWC_STREAM_MINW", "64"))
            and B * ((W + 127) // 128) * ((H + 7) // 8) >= max(4, min(64, min_tiles)))


def head_upfeat_workspace_bytes(B: int, cin: int, H: int, W: int) -> int:
    """Scratch bytes pwc_head_upfeat_ws_fwd wants for this geometry (Cin slices of launches smaller than the chip; 0 = never)."""
    return _query_bytes(_lib.load().pwc_head_upfeat_workspace_bytes(B, cin, H, W), "head")


def head_upfeat(x: torch.Tensor, head_wpacked: torch.Tensor, head_bias: torch.Tensor, up_weight: torch.Tensor,
                up_bias: torch.Tensor, flow_out: torch.Tensor, up_out: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> None:
    """predict_flowL + upfeatL in one pass over the arena x (fused C-ABI entry pwc_head_upfeat_ws_fwd; `workspace`: scratch for the
    Cin slices of launches smaller than the chip, see head_upfeat_workspace_bytes)."""
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    B, cin, H, W = x.shape
    if tuple(flow_out.shape) != (B, 2, H, W) or tuple(up_out.shape) != (B, 2, 2 * H, 2 * W):
        raise ValueError("flow_out must be %s and up_out %s" % ((B, 2, H, W), (B, 2, 2 * H, 2 * W)))
    if tuple(up_weight.shape) != (cin, 2, 4, 4) or not up_weight.is_contiguous():
        raise ValueError("up_weight must be contiguous [Cin=%d,2,4,4]" % cin)
    need = lib.pwc_conv3x3_packed_bytes(cin, 2, PWC_F32)
    if head_wpacked.numel() * 4 != need:
        raise ValueError("packed head weights do not match Cin=%d" % cin)
    bsf = _plane_dense(flow_out, "flow_out")
    bsu = _plane_dense(up_out, "up_out")
    with torch.cuda.device(x.device):
        ws_ptr, ws_bytes = _workspace_args(workspace, x)
        rc = lib.pwc_head_upfeat_ws_fwd(x.data_ptr(), head_wpacked.data_ptr(), head_bias.data_ptr(), flow_out.data_ptr(),
                                        up_weight.data_ptr(), up_bias.data_ptr(), up_out.data_ptr(),
                                        B, cin, H, W, _dtype_code(x), bsx, bsf, bsu, ws_ptr, ws_bytes, _stream(x))
    check(rc, "pwc_head_upfeat_ws_fwd")


def deconv_as_conv3x3(wt: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(k4, s2, p1) filters [Cin, Cout, 4, 4] -> 3x3 conv filters [Cout*4, Cin, 3, 3], output channel
    co*4 + py*2 + px = phase (py, px) of output pixel (2*iy+py, 2*ix+px):
    py = 0 takes window rows a = 0, 1 with ky = 3, 1;  py = 1 takes a = 1, 2 with ky = 2, 0  (same along x)."""
    cin, cout = wt.shape[:2]
    k = wt.new_zeros((cout, 2, 2, cin, 3, 3))
    taps = {0: ((0, 3), (1, 1)), 1: ((1, 2), (2, 0))}          # phase -> ((window index, kernel index), ...)
    for py in (0, 1):
        for a, ky in taps[py]:
            for px in (0, 1):
                for e, kx in taps[px]:
                    k[:, py, px, :, a, e] = wt[:, :, ky, kx].t()
    return k.reshape(cout * 4, cin, 3, 3)


def upsample_entry(head: torch.Tensor, deconv_w: torch.Tensor, deconv_b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Exit of a decoder level whose flow head and upfeat ran as one 10-channel 3x3 convolution: head [B,10,h,w] = [flow | upfeat
    phases] -> out [B,4,2h,2w] = [deconvL(flow) | up_feat] (C-ABI pwc_upsample_entry_f32; PWCNet.py:208-209)."""
    lib = _lib.load()
    B, c, h, w = head.shape
    if c != 10 or head.dtype != torch.float32 or tuple(out.shape) != (B, 4, 2 * h, 2 * w) or out.dtype != torch.float32:
        raise ValueError("head must be float32 [B,10,h,w] and out [B,4,2h,2w], got %s / %s" % (tuple(head.shape), tuple(out.shape)))
    for t, n, shp in ((deconv_w, "deconv_w", (2, 2, 4, 4)), (deconv_b, "deconv_b", (2,))):
        if tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous() or t.device != head.device:
            raise ValueError("%s must be contiguous float32 %s on %s" % (n, shp, head.device))
    bsh, bso = _plane_dense(head, "head"), _plane_dense(out, "out")
    with torch.cuda.device(head.device):
        rc = lib.pwc_upsample_entry_f32(head.data_ptr(), deconv_w.data_ptr(), deconv_b.data_ptr(), out.data_ptr(), B, h, w, bsh, bso, _stream(head))
    check(rc, "pwc_upsample_entry_f32")
    return out


def deconv4x4s2(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.ConvTranspose2d(k=4, s=2, p=1); weight [Cin,Cout,4,4] float32 contiguous."""
    lib = _lib.load()
    bsx = _plane_dense(x, "x")
    B, cin, H, W = x.shape
    if weight.dim() != 4 or weight.shape[0] != cin or weight.shape[2:] != (4, 4) or not weight.is_contiguous():
        raise ValueError("weight must be contiguous [Cin=%d,Cout,4,4], got %s" % (cin, tuple(weight.shape)))
    cout = weight.shape[1]
    if out is None:
        out = torch.empty((B, cout, 2 * H, 2 * W), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (B, cout, 2 * H, 2 * W):
        raise ValueError("out must be %s" % ((B, cout, 2 * H, 2 * W),))
    bsy = _plane_dense(out, "out")
    with torch.cuda.device(x.device):
        rc = lib.pwc_deconv4x4s2_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                     B, cin, H, W, cout, _dtype_code(x), bsx, bsy, _stream(x))
    check(rc, "pwc_deconv4x4s2_fwd")
    return out


# ---------------------------------------------------------------- self-supervised proxy-label loss (train_pseudo / train_fundamental)
def proxy_loss_supported(flow: torch.Tensor, img1: torch.Tensor, img2: torch.Tensor, mask: Optional[torch.Tensor] = None) -> bool:
    """Python mirror of the geometry / placement rules under which pwc_proxy_loss_fwd / _bwd launch (include/pwc_hip.h):
    ROCm device tensors, f32 after the cast, 2 <= h <= H, 2 <= w <= W, C*H*W < 2^31, B <= 65535."""
    if not (flow.is_cuda and img1.is_cuda and img2.is_cuda) or (mask is not None and not mask.is_cuda):
        return False
    if flow.dim() != 4 or img1.dim() != 4 or flow.shape[1] != 2 or img1.shape != img2.shape or flow.shape[0] != img1.shape[0]:
        return False
    B, C, H, W = img1.shape
    h, w = flow.shape[-2:]
    return 2 <= h <= H and 2 <= w <= W and C * H * W < 2 ** 31 and 1 <= B <= 65535 and (H + 15) // 16 <= 65535


def proxy_loss_workspace_bytes(B: int, C: int, H: int, W: int, h: int, w: int, forward_only: bool = False) -> int:
    """Scratch bytes of pwc_proxy_loss_bwd (enough for the forward too), or of pwc_proxy_loss_fwd alone with forward_only."""
    lib = _lib.load()
    fn = lib.pwc_proxy_loss_fwd_workspace_bytes if forward_only else lib.pwc_proxy_loss_workspace_bytes
    return _query_bytes(fn(B, C, H, W, h, w), "proxy-loss")


def _proxy_args(flow, img1, img2, mask):
    B, C, H, W = img1.shape
    h, w = flow.shape[-2:]
    dev = img1.device
    flow, bsf = _f32_dense(flow, "flow", (B, 2, h, w), dev)
    img1, bs1 = _f32_dense(img1, "img1", (B, C, H, W), dev)
    img2, bs2 = _f32_dense(img2, "img2", (B, C, H, W), dev)
    m, u8, bsm = _mask_arg(mask, B, H, W, dev, "threshold", "valid_mask")
    return flow, img1, img2, m, u8, bsm, (bsf, bs1, bs2), (B, C, H, W, h, w)


def _proxy_workspace(dims, device, forward_only=False) -> Tuple[torch.Tensor, int]:
    return _scratch(proxy_loss_workspace_bytes(*dims, forward_only=forward_only), device)


def proxy_loss(flow: torch.Tensor, img1: torch.Tensor, img2: torch.Tensor, mask: Optional[torch.Tensor] = None,
               alpha_photo: float = 1.0, alpha_smooth: float = 0.1, ssim_eps: float = 0.0) -> torch.Tensor:
    """float32 [3] = (total, photo, smooth) of the proxy-label loss (pwc_proxy_loss_fwd; train_pseudo.py:65-164 with ssim_eps 0,
    train_fundamental.py:62-166 with 1e-12 and an optional [B,H,W] / [B,1,H,W] mask).  No host synchronisation."""
    lib = _lib.load()
    flow, img1, img2, m, u8, bsm, bs, dims = _proxy_args(flow, img1, img2, mask)
    out = torch.empty(3, dtype=torch.float32, device=img1.device)
    with torch.cuda.device(img1.device):
        ws, nb = _proxy_workspace(dims, img1.device, forward_only=True)
        rc = lib.pwc_proxy_loss_fwd(flow.data_ptr(), img1.data_ptr(), img2.data_ptr(), _ptr(m), u8,
                                    out.data_ptr(), *dims, float(alpha_photo), float(alpha_smooth), float(ssim_eps),
                                    bs[0], bs[1], bs[2], bsm, ws.data_ptr(), nb, _stream(img1))
    check(rc, "pwc_proxy_loss_fwd")
    return out


def proxy_loss_backward(flow: torch.Tensor, img1: torch.Tensor, img2: torch.Tensor, mask: Optional[torch.Tensor],
                        grad_out: torch.Tensor, alpha_photo: float = 1.0, alpha_smooth: float = 0.1,
                        ssim_eps: float = 0.0) -> torch.Tensor:
    """grad_flow [B,2,h,w] of the proxy-label loss for upstream gradients grad_out = (g_total, g_photo, g_smooth), a float32 [3]
    device tensor (pwc_proxy_loss_bwd: recomputes, deterministic, no host synchronisation)."""
    lib = _lib.load()
    flow, img1, img2, m, u8, bsm, bs, dims = _proxy_args(flow, img1, img2, mask)
    g = grad_out.to(device=img1.device, dtype=torch.float32).contiguous().reshape(3)
    B, _, _, _, h, w = dims
    gf = torch.empty((B, 2, h, w), dtype=torch.float32, device=img1.device)
    with torch.cuda.device(img1.device):
        ws, nb = _proxy_workspace(dims, img1.device)
        rc = lib.pwc_proxy_loss_bwd(flow.data_ptr(), img1.data_ptr(), img2.data_ptr(), _ptr(m), u8,
                                    g.data_ptr(), gf.data_ptr(), *dims, float(alpha_photo), float(alpha_smooth), float(ssim_eps),
                                    bs[0], bs[1], bs[2], bsm, ws.data_ptr(), nb, _stream(img1))
    check(rc, "pwc_proxy_loss_bwd")
    return gf


def flow_warp_image(img: torch.Tensor, flow: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """warp / warp_image of train_pseudo.py:122-157 / train_fundamental.py:80-99 (forward only, any C): img [B,C,H,W] sampled at
    x + upsample(flow) (bilinear, border, align_corners=True); flow [B,2,h,w] with 2 <= h <= H, 2 <= w <= W."""
    lib = _lib.load()
    img, flow = densify(img), densify(flow)
    B, C, H, W = img.shape
    h, w = flow.shape[-2:]
    if tuple(flow.shape) != (B, 2, h, w) or img.dtype != torch.float32 or flow.dtype != torch.float32 or flow.device != img.device:
        raise ValueError("img must be float32 [B,C,H,W] and flow float32 [B,2,h,w] on one device")
    if out is None:
        out = torch.empty_like(img, memory_format=torch.contiguous_format)
    bsi, bsf, bso = _plane_dense(img, "img"), _plane_dense(flow, "flow"), _plane_dense(out, "out")
    with torch.cuda.device(img.device):
        rc = lib.pwc_flow_warp_image_fwd(img.data_ptr(), flow.data_ptr(), out.data_ptr(), B, C, H, W, h, w, bsi, bsf, bso, _stream(img))
    check(rc, "pwc_flow_warp_image_fwd")
    return out


class ProxyLossFunction(torch.autograd.Function):
    """autograd of the proxy-label loss w.r.t. the flow: forward pwc_proxy_loss_fwd, backward pwc_proxy_loss_bwd (recomputes from
    the inputs; nothing image-sized is saved beyond the inputs themselves).  Returns a float32 [3] tensor (total, photo, smooth).
    Under torch.autocast the inputs are cast to float32.  apply(flow, img1, img2, mask, alpha_photo, alpha_smooth, ssim_eps);
    img1, img2 and mask get no gradient (callers route images that require grad to the torch composition)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, flow, img1, img2, mask=None, alpha_photo=1.0, alpha_smooth=0.1, ssim_eps=0.0):
        ctx.save_for_backward(flow, img1, img2, mask)
        ctx.cfg = (float(alpha_photo), float(alpha_smooth), float(ssim_eps))
        return proxy_loss(flow, img1, img2, mask, *ctx.cfg)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        flow, img1, img2, mask = ctx.saved_tensors
        gf = proxy_loss_backward(flow, img1, img2, mask, grad_out, *ctx.cfg)
        return gf, None, None, None, None, None, None


# ---------------------------------------------------------------- no-ground-truth validation metrics (train_pseudo / train_fundamental)
def fb_metrics_supported(flow12: torch.Tensor, flow21: Optional[torch.Tensor], H: int, W: int) -> bool:
    """Python mirror of the placement / geometry rules under which pwc_fb_metrics launches (include/pwc_hip.h): ROCm device
    tensors of one [B,2,h,w] shape, 2 <= h <= H, 2 <= w <= W, B*2*H*W < 2^31, B <= 65535.  The dtype is the caller's business
    (the kernel takes float32)."""
    if not flow12.is_cuda or flow12.dim() != 4 or flow12.shape[1] != 2:
        return False
    if flow21 is not None and (not flow21.is_cuda or flow21.shape != flow12.shape or flow21.device != flow12.device):
        return False
    B, _, h, w = flow12.shape
    return 2 <= h <= H and 2 <= w <= W and B * 2 * H * W < 2 ** 31 and 1 <= B <= 65535 and (H + 15) // 16 <= 65535


def fb_metrics_workspace_bytes(B: int, H: int, W: int) -> int:
    return _query_bytes(_lib.load().pwc_fb_metrics_workspace_bytes(B, H, W), "fb-metrics")


def fb_metrics(flow12: torch.Tensor, flow21: Optional[torch.Tensor], H: int, W: int, out: Optional[torch.Tensor] = None,
               raw: bool = False):
    """float32 [2] = (cycle, oob) of pwc_fb_metrics: mean |up(flow12) + warp(up(flow21), up(flow12))| over [B,2,H,W] (the scripts'
    forward-backward cycle) and the fraction of the B*H*W sample points x + up(flow12) that leave the image.  flow12 / flow21
    float32 [B,2,h,w] with 2 <= h <= H, 2 <= w <= W; flow21 = None: the out-of-bounds ratio alone (cycle is written as 0).
    One launch pair, no host synchronisation, bit-reproducible.  raw=True returns (out, cycle_sum, oob_count): the float64 sum
    and the int64 count the two ratios were formed from, as 0-dim device tensors."""
    lib = _lib.load()
    B, _, h, w = flow12.shape
    dev = flow12.device
    flow12, bs12 = _f32_dense(flow12, "flow12", (B, 2, h, w), dev)
    bs21 = 0
    if flow21 is not None:
        flow21, bs21 = _f32_dense(flow21, "flow21", (B, 2, h, w), dev)
    out = _out_arg(out, (2,), torch.float32, dev, contiguous=True)
    H, W = int(H), int(W)
    with torch.cuda.device(dev):
        ws, nb = _scratch(fb_metrics_workspace_bytes(B, max(H, 1), max(W, 1)), dev)
        rc = lib.pwc_fb_metrics(flow12.data_ptr(), _ptr(flow21), B, h, w, H, W, bs12, bs21,
                                ws.data_ptr(), nb, out.data_ptr(), _stream(flow12))
    check(rc, "pwc_fb_metrics")
    if raw:
        return out, ws[:1].view(torch.float64)[0], ws[1]
    return out


# ---------------------------------------------------------------- supervised flow losses (train.py / train2.py)
SUP_MAX_LEVELS = 8
MASK_RULES = {"threshold": 0, "raw": 1}   # MaskedCharbonnier's [m > 0.5] / max(sum, 1); compute_epe's raw m / (sum + 1e-8)


def _sup_geometry_ok(H: int, W: int, h: int, w: int) -> bool:
    return 2 <= h <= H and 2 <= w <= W


def sup_flow_loss_supported(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None) -> bool:
    """Python mirror of the rules under which pwc_sup_flow_loss_fwd / _bwd launch (include/pwc_hip.h): ROCm device tensors,
    pred [B,2,h,w] and gt [B,2,H,W] with 2 <= h <= H, 2 <= w <= W, 2*H*W < 2^31, B <= 65535; mask [B,H,W] or [B,1,H,W]."""
    if not (isinstance(pred, torch.Tensor) and isinstance(gt, torch.Tensor) and pred.is_cuda and gt.is_cuda):
        return False
    if pred.dim() != 4 or gt.dim() != 4 or pred.shape[1] != 2 or gt.shape[1] != 2 or pred.shape[0] != gt.shape[0]:
        return False
    B, _, H, W = gt.shape
    if mask is not None and (not mask.is_cuda or tuple(mask.shape) not in ((B, H, W), (B, 1, H, W))):
        return False
    return _sup_geometry_ok(H, W, pred.shape[2], pred.shape[3]) and 2 * H * W < 2 ** 31 and 1 <= B <= 65535


def sup_multiscale_loss_supported(preds, gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                                  images: Optional[torch.Tensor] = None) -> bool:
    """Mirror of pwc_sup_multiscale_loss_fwd / _bwd's rules: 1..8 levels [B,2,h,w] with 2 <= h <= H, 2 <= w <= W, gt [B,2,H,W],
    mask [B,H,W] / [B,1,H,W], images [B,6,H,W] (when given), all on the ROCm device, 6*H*W < 2^31, B <= 65535."""
    if not (isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dim() == 4 and gt.shape[1] == 2):
        return False
    B, _, H, W = gt.shape
    if not (1 <= len(preds) <= SUP_MAX_LEVELS):
        return False
    for p in preds:
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dim() == 4 and p.shape[0] == B and p.shape[1] == 2
                and _sup_geometry_ok(H, W, p.shape[2], p.shape[3])):
            return False
    if mask is not None and (not mask.is_cuda or tuple(mask.shape) not in ((B, H, W), (B, 1, H, W))):
        return False
    if images is not None and (not images.is_cuda or tuple(images.shape) != (B, 6, H, W)):
        return False
    return 6 * H * W < 2 ** 31 and 1 <= B <= 65535


def sup_flow_loss_workspace_bytes(B: int, H: int, W: int, h: int, w: int, backward: bool = False) -> int:
    return _query_bytes(_lib.load().pwc_sup_flow_loss_workspace_bytes(B, H, W, h, w, 1 if backward else 0), "flow-loss")


def _sup_flow_args(pred, gt, mask):
    if not (isinstance(gt, torch.Tensor) and gt.is_cuda):
        raise PwcHipError("gt must be a ROCm device tensor: the supervised loss has no CPU fallback")
    if gt.dim() != 4 or gt.shape[1] != 2:
        raise ValueError("gt must be [B,2,H,W], got %s" % (tuple(gt.shape),))
    B, _, H, W = gt.shape
    if pred.dim() != 4:
        raise ValueError("pred must be [B,2,h,w], got %s" % (tuple(pred.shape),))
    h, w = pred.shape[-2:]
    gt, bsg = _f32_dense(gt, "gt", (B, 2, H, W), gt.device)
    pred, bsp = _f32_dense(pred, "pred", (B, 2, h, w), gt.device)
    m, u8, bsm = _mask_arg(mask, B, H, W, gt.device, "raw")
    return pred, gt, m, u8, (B, H, W, h, w), (bsp, bsg, bsm)


def sup_flow_loss(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, eps: float = 1e-3,
                  rule: str = "threshold") -> torch.Tensor:
    """float32 [2] = (loss, den) of the masked Charbonnier (rule "threshold": train.py:31-48 / train2.py:114-122) or the EPE
    (rule "raw", eps 0: compute_epe train2.py:100-111) of pred [B,2,h,w] upsampled to gt [B,2,H,W] (bilinear, align_corners=False,
    vectors scaled by W/w, H/h; pred itself when h,w = H,W).  pwc_sup_flow_loss_fwd: no upsampled flow in memory, no host sync."""
    lib = _lib.load()
    pred, gt, m, u8, dims, bs = _sup_flow_args(pred, gt, mask)
    out = torch.empty(2, dtype=torch.float32, device=gt.device)
    with torch.cuda.device(gt.device):
        ws, nb = _scratch(sup_flow_loss_workspace_bytes(*dims), gt.device)
        rc = lib.pwc_sup_flow_loss_fwd(pred.data_ptr(), gt.data_ptr(), _ptr(m), u8,
                                       MASK_RULES[rule], out.data_ptr(), *dims, float(eps), *bs, ws.data_ptr(), nb, _stream(gt))
    check(rc, "pwc_sup_flow_loss_fwd")
    return out


def sup_flow_loss_backward(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor], fwd_out: torch.Tensor,
                           grad_out: torch.Tensor, eps: float = 1e-3, rule: str = "threshold") -> torch.Tensor:
    """grad_pred [B,2,h,w] = grad_out[0] d loss / d pred (pwc_sup_flow_loss_bwd; fwd_out = sup_flow_loss's result, read on the
    device for the denominator; deterministic, no host synchronisation)."""
    lib = _lib.load()
    pred, gt, m, u8, dims, bs = _sup_flow_args(pred, gt, mask)
    fo = fwd_out.to(device=gt.device, dtype=torch.float32).contiguous().reshape(2)
    g = grad_out.to(device=gt.device, dtype=torch.float32).contiguous().reshape(-1)
    B, H, W, h, w = dims
    gp = torch.empty((B, 2, h, w), dtype=torch.float32, device=gt.device)
    with torch.cuda.device(gt.device):
        ws, nb = _scratch(sup_flow_loss_workspace_bytes(*dims, backward=True), gt.device)
        rc = lib.pwc_sup_flow_loss_bwd(pred.data_ptr(), gt.data_ptr(), _ptr(m), u8,
                                       MASK_RULES[rule], fo.data_ptr(), g.data_ptr(), gp.data_ptr(), *dims, float(eps), *bs,
                                       ws.data_ptr(), nb, _stream(gt))
    check(rc, "pwc_sup_flow_loss_bwd")
    return gp


class FlowLossFunction(torch.autograd.Function):
    """autograd of the upsampled masked Charbonnier w.r.t. pred: forward pwc_sup_flow_loss_fwd, backward pwc_sup_flow_loss_bwd.
    Returns float32 [2] = (loss, den); den gets no gradient.  Under torch.autocast the inputs are cast to float32.
    apply(pred, gt, mask, eps, rule); gt and mask get no gradient (callers route a GT that requires grad to the torch chain)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pred, gt, mask=None, eps=1e-3, rule="threshold"):
        out = sup_flow_loss(pred, gt, mask, eps, rule)
        ctx.save_for_backward(pred, gt, mask, out)
        ctx.cfg = (float(eps), rule)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        pred, gt, mask, out = ctx.saved_tensors
        return sup_flow_loss_backward(pred, gt, mask, out, grad_out, *ctx.cfg), None, None, None, None


def _levels_host(preds, weights):
    L = len(preds)
    ptrs = (ctypes.c_void_p * L)(*[p.data_ptr() for p in preds])
    bss = (ctypes.c_int64 * L)(*[_plane_dense(p, "flow level %d" % i) for i, p in enumerate(preds)])
    hw = (ctypes.c_int * (2 * L))(*[int(s) for p in preds for s in p.shape[-2:]])
    wts = (ctypes.c_float * L)(*[float(x) for x in weights])
    return ptrs, bss, hw, wts


def sup_multiscale_loss_workspace_bytes(B: int, H: int, W: int, sizes, with_images: bool) -> int:
    L = len(sizes)
    hw = (ctypes.c_int * (2 * L))(*[int(s) for hw_ in sizes for s in hw_])
    return _query_bytes(_lib.load().pwc_sup_multiscale_loss_workspace_bytes(B, H, W, L, ctypes.cast(hw, ctypes.c_void_p),
                                                                          1 if with_images else 0), "multiscale-loss")


def _ms_args(preds, gt, mask, images, weights, lambda_photo, lambda_smooth):
    if not (isinstance(gt, torch.Tensor) and gt.is_cuda):
        raise PwcHipError("flows_gt must be a ROCm device tensor: the supervised loss has no CPU fallback")
    if gt.dim() != 4 or gt.shape[1] != 2:
        raise ValueError("flows_gt must be [B,2,H,W], got %s" % (tuple(gt.shape),))
    B, _, H, W = gt.shape
    gt, bsg = _f32_dense(gt, "flows_gt", (B, 2, H, W), gt.device)
    if not 1 <= len(preds) <= SUP_MAX_LEVELS or len(weights) != len(preds):
        raise ValueError("1..%d flow levels with one weight each, got %d levels / %d weights" % (SUP_MAX_LEVELS, len(preds), len(weights)))
    preds = [_f32_dense(p, "flow level %d" % i, (B, 2) + tuple(p.shape[-2:]), gt.device)[0] for i, p in enumerate(preds)]
    m, u8, bsm = _mask_arg(mask, B, H, W, gt.device, "raw", "masks")
    with_images = lambda_photo > 0.0 or lambda_smooth > 0.0
    img, bsi = None, 0
    if with_images:
        if images is None:
            raise ValueError("images [B,6,H,W] are needed when lambda_photo or lambda_smooth > 0")
        img, bsi = _f32_dense(images, "images", (B, 6, H, W), gt.device)
    return preds, gt, m, u8, img, (bsg, bsm, bsi), (B, H, W), with_images


def sup_multiscale_loss(preds, gt: torch.Tensor, mask: Optional[torch.Tensor], images: Optional[torch.Tensor], weights,
                        lambda_photo: float = 0.0, lambda_smooth: float = 0.0, eps: float = 1e-3) -> torch.Tensor:
    """float32 [1 + 3L] = (total, level losses [L], Charbonnier denominators [L], photometric denominators [L]) of
    supervised_multiscale_loss (train2.py:124-167) over the flow levels preds (pwc_sup_multiscale_loss_fwd: one launch for every
    level, plus a resize launch when a lambda is > 0).  No host synchronisation."""
    lib = _lib.load()
    preds, gt, m, u8, img, bs, dims, wi = _ms_args(preds, gt, mask, images, weights, lambda_photo, lambda_smooth)
    L = len(preds)
    ptrs, bss, hw, wts = _levels_host(preds, weights)
    out = torch.empty(1 + 3 * L, dtype=torch.float32, device=gt.device)
    with torch.cuda.device(gt.device):
        ws, nb = _scratch(sup_multiscale_loss_workspace_bytes(*dims, [p.shape[-2:] for p in preds], wi), gt.device)
        rc = lib.pwc_sup_multiscale_loss_fwd(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(bss, ctypes.c_void_p),
                                             ctypes.cast(hw, ctypes.c_void_p), ctypes.cast(wts, ctypes.c_void_p), L, gt.data_ptr(),
                                             _ptr(m), u8, _ptr(img), out.data_ptr(), *dims, float(eps),
                                             float(lambda_photo), float(lambda_smooth), *bs, ws.data_ptr(), nb, _stream(gt))
    check(rc, "pwc_sup_multiscale_loss_fwd")
    return out


def sup_multiscale_loss_backward(preds, gt: torch.Tensor, mask: Optional[torch.Tensor], images: Optional[torch.Tensor], weights,
                                 fwd_out: torch.Tensor, grad_out: torch.Tensor, lambda_photo: float = 0.0,
                                 lambda_smooth: float = 0.0, eps: float = 1e-3):
    """Gradients of the total w.r.t. every level (list of dense [B,2,h,w]) for grad_out[0] (pwc_sup_multiscale_loss_bwd; reads
    the forward's denominators from fwd_out on the device; elementwise, deterministic)."""
    lib = _lib.load()
    preds, gt, m, u8, img, bs, dims, wi = _ms_args(preds, gt, mask, images, weights, lambda_photo, lambda_smooth)
    L = len(preds)
    ptrs, bss, hw, wts = _levels_host(preds, weights)
    fo = fwd_out.to(device=gt.device, dtype=torch.float32).contiguous().reshape(1 + 3 * L)
    g = grad_out.to(device=gt.device, dtype=torch.float32).contiguous().reshape(-1)
    grads = [torch.empty(tuple(p.shape), dtype=torch.float32, device=gt.device) for p in preds]
    gptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in grads])
    with torch.cuda.device(gt.device):
        ws, nb = _scratch(sup_multiscale_loss_workspace_bytes(*dims, [p.shape[-2:] for p in preds], wi), gt.device)
        rc = lib.pwc_sup_multiscale_loss_bwd(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(bss, ctypes.c_void_p),
                                             ctypes.cast(hw, ctypes.c_void_p), ctypes.cast(wts, ctypes.c_void_p), L, gt.data_ptr(),
                                             _ptr(m), u8, _ptr(img), fo.data_ptr(), g.data_ptr(),
                                             ctypes.cast(gptrs, ctypes.c_void_p), *dims, float(eps), float(lambda_photo),
                                             float(lambda_smooth), *bs, ws.data_ptr(), nb, _stream(gt))
    check(rc, "pwc_sup_multiscale_loss_bwd")
    return grads


class MultiscaleLossFunction(torch.autograd.Function):
    """autograd of supervised_multiscale_loss w.r.t. every flow level: forward pwc_sup_multiscale_loss_fwd, backward
    pwc_sup_multiscale_loss_bwd.  apply(gt, mask, images, weights, lambda_photo, lambda_smooth, *preds) -> float32 [1 + 3L]
    (total first; only the total carries a gradient).  Under torch.autocast the inputs are cast to float32; gt, mask and images
    get no gradient."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, gt, mask, images, weights, lambda_photo, lambda_smooth, *preds):
        cfg = (tuple(float(x) for x in weights), float(lambda_photo), float(lambda_smooth))
        out = sup_multiscale_loss(list(preds), gt, mask, images, cfg[0], cfg[1], cfg[2])
        ctx.save_for_backward(gt, mask, images, out, *preds)
        ctx.cfg = cfg
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        gt, mask, images, out, *preds = ctx.saved_tensors
        w, lp, ls = ctx.cfg
        grads = sup_multiscale_loss_backward(preds, gt, mask, images, w, out, grad_out, lp, ls)
        return (None,) * 6 + tuple(grads)


# ---------------------------------------------------------------- epipolar mask + soft Sampson penalty (train_fundamental)
ROBUST_CODES = {"huber": 0, "l1": 1}   # anything else: the plain mean (code 2), as epipolar_sampson_loss


def _flow_arg(flow: torch.Tensor, name: str = "flow_full") -> Tuple[torch.Tensor, int]:
    if not isinstance(flow, torch.Tensor) or not flow.is_cuda:
        raise PwcHipError("%s must be a ROCm device tensor: the epipolar path has no CPU fallback" % name)
    if flow.dim() != 4:
        raise ValueError("%s must be float32 [B,2,H,W], got %s %s" % (name, flow.dtype, tuple(flow.shape)))
    return _f32_dense(flow, name, (flow.shape[0], 2) + tuple(flow.shape[2:]), flow.device)


def epipolar_pairs(flow: torch.Tensor, stride: int = 4, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """_flow_to_pairs of train_fundamental.py:169-194, batched: (pts float64 [B,cap,4] = (x, y, x+fu, y+fv) packed in grid order,
    N int32 [B] on the device).  Rows past N_b are unwritten."""
    lib = _lib.load()
    flow, bsf = _flow_arg(flow)
    B, _, H, W = flow.shape
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be >= 1")
    m, u8, _ = _mask_arg(mask, B, H, W, flow.device, "nonzero", "img_mask_bhw")
    cap = -(-H // stride) * -(-W // stride)
    pts = torch.empty((B, cap, 4), dtype=torch.float64, device=flow.device)
    n = torch.empty(B, dtype=torch.int32, device=flow.device)
    with torch.cuda.device(flow.device):
        rc = lib.pwc_epipolar_pairs(flow.data_ptr(), _ptr(m), u8, pts.data_ptr(), n.data_ptr(),
                                    B, H, W, stride, bsf, H * W, _stream(flow))
    check(rc, "pwc_epipolar_pairs")
    return pts, n


def epipolar_ransac(pts: torch.Tensor, n: torch.Tensor, idx: torch.Tensor, thresh: float = 0.5):
    """_ransac_F of train_fundamental.py:236-258 on epipolar_pairs output, with the caller's index table idx int32 [iters,8]
    (shared) or [B,iters,8].  Returns (F float64 [B,9], ok int32 [B], best int32 [B], counts int32 [B,iters]); no host sync."""
    lib = _lib.load()
    if pts.dim() != 3 or pts.shape[2] != 4 or pts.dtype != torch.float64 or not pts.is_cuda or not pts.is_contiguous():
        raise ValueError("pts must be a contiguous float64 [B,cap,4] device tensor")
    B, cap, _ = pts.shape
    if idx.dtype != torch.int32 or idx.device != pts.device or idx.shape[-1] != 8 or idx.dim() not in (2, 3):
        raise ValueError("idx must be int32 [iters,8] or [B,iters,8] on %s" % pts.device)
    idx = idx.contiguous()
    iters = idx.shape[-2]
    ibs = 0 if idx.dim() == 2 else 8 * iters
    if idx.dim() == 3 and idx.shape[0] != B:
        raise ValueError("idx batch %d != %d" % (idx.shape[0], B))
    if n.dtype != torch.int32 or tuple(n.shape) != (B,) or n.device != pts.device:
        raise ValueError("n must be int32 [B] on %s" % pts.device)
    dev = pts.device
    F = torch.empty((B, 9), dtype=torch.float64, device=dev)
    ok = torch.empty(B, dtype=torch.int32, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty((B, iters), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, nb = _scratch(_query_bytes(lib.pwc_epipolar_ransac_workspace_bytes(B, iters), "RANSAC"), dev)
        rc = lib.pwc_epipolar_ransac(pts.data_ptr(), n.contiguous().data_ptr(), cap, idx.data_ptr(), ibs, B, iters, float(thresh),
                                     F.data_ptr(), ok.data_ptr(), best.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb,
                                     torch.cuda.current_stream(dev).cuda_stream)
    check(rc, "pwc_epipolar_ransac")
    return F, ok, best, counts


def _F_arg(F, B: int, device) -> Tuple[torch.Tensor, int]:
    """F as float64 [9] (shared, batch stride 0) or [B,9] on the device; accepts numpy / torch [3,3] or torch [B,3,3]."""
    if not isinstance(F, torch.Tensor):
        F = torch.as_tensor(F)
    F = F.to(device=device, dtype=torch.float64)
    if F.dim() == 2 and tuple(F.shape) == (3, 3):
        return F.reshape(9).contiguous(), 0
    if F.dim() == 3 and tuple(F.shape[1:]) == (3, 3) and F.shape[0] in (1, B):
        return F.reshape(-1, 9).contiguous(), (9 if F.shape[0] == B and B > 1 else 0)
    if F.dim() == 2 and tuple(F.shape) == (B, 9):
        return F.contiguous(), 9
    raise ValueError("F must be [3,3] or [B,3,3], got %s" % (tuple(F.shape),))


def epipolar_distance(flow: torch.Tensor, F, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sampson distance of every pixel, float64 [B,H,W] (train_fundamental.py:285-296, pwc_epipolar_distance)."""
    lib = _lib.load()
    flow, bsf = _flow_arg(flow)
    B, _, H, W = flow.shape
    Fd, fbs = _F_arg(F, B, flow.device)
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.float64, device=flow.device)
    elif tuple(out.shape) != (B, H, W) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out must be contiguous float64 %s" % ((B, H, W),))
    with torch.cuda.device(flow.device):
        rc = lib.pwc_epipolar_distance(flow.data_ptr(), Fd.data_ptr(), fbs, out.data_ptr(), B, H, W, bsf, _stream(flow))
    check(rc, "pwc_epipolar_distance")
    return out


def epipolar_mask(flow: torch.Tensor, F: torch.Tensor, ok: torch.Tensor, tau: float = 1.0, keep_ratio: float = 0.2,
                  min_keep: float = 0.05, dist_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Steps 2-5 of build_epipolar_mask_from_flow (train_fundamental.py:284-327) for F float64 [B,9] and ok int32 [B] from
    epipolar_ransac: (mask bool [B,1,H,W], thr float64 [B], NaN where the mask is all true).  No host sync."""
    lib = _lib.load()
    flow, bsf = _flow_arg(flow)
    B, _, H, W = flow.shape
    dev = flow.device
    F = F.to(device=dev, dtype=torch.float64).reshape(B, 9).contiguous()
    ok = ok.to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    mask = torch.empty((B, 1, H, W), dtype=torch.bool, device=dev)
    thr = torch.empty(B, dtype=torch.float64, device=dev)
    if dist_out is not None and (tuple(dist_out.shape) != (B, H, W) or dist_out.dtype != torch.float64 or not dist_out.is_contiguous()):
        raise ValueError("dist_out must be contiguous float64 %s" % ((B, H, W),))
    with torch.cuda.device(dev):
        ws, nb = _scratch(_query_bytes(lib.pwc_epipolar_mask_workspace_bytes(B, H, W), "mask"), dev)
        rc = lib.pwc_epipolar_mask(flow.data_ptr(), F.data_ptr(), ok.data_ptr(), mask.data_ptr(), thr.data_ptr(),
                                   _ptr(dist_out), B, H, W, float(tau), float(keep_ratio),
                                   float(min_keep), bsf, ws.data_ptr(), nb, _stream(flow))
    check(rc, "pwc_epipolar_mask")
    return mask, thr


def _loss_args(flow, F, ok, valid_mask):
    flow, bsf = _flow_arg(flow)
    B, _, H, W = flow.shape
    Fd, fbs = _F_arg(F, B, flow.device)
    okt, obs = None, 0
    if ok is not None:
        okt = torch.as_tensor(ok).to(device=flow.device, dtype=torch.int32).reshape(-1).contiguous()
        if okt.numel() not in (1, B):
            raise ValueError("ok must hold 1 or B values")
        obs = 1 if okt.numel() == B and B > 1 else 0
    m, u8, bsm = _mask_arg(valid_mask, B, H, W, flow.device, "threshold", "valid_mask")
    return flow, bsf, (B, H, W), Fd, fbs, okt, obs, m, u8, bsm


def _loss_workspace(B, H, W, device):
    return _scratch(_query_bytes(_lib.load().pwc_epipolar_loss_workspace_bytes(B, H, W), "loss"), device)


def epipolar_loss(flow: torch.Tensor, F, ok=None, valid_mask: Optional[torch.Tensor] = None, robust: str = "huber",
                  delta: float = 1.0, weight: float = 0.1) -> torch.Tensor:
    """float32 [] = epipolar_sampson_loss (train_fundamental.py:331-382; pwc_epipolar_loss_fwd), 0 when nothing is selected or
    every fit failed.  No host synchronisation."""
    lib = _lib.load()
    flow, bsf, (B, H, W), Fd, fbs, okt, obs, m, u8, bsm = _loss_args(flow, F, ok, valid_mask)
    out = torch.empty(1, dtype=torch.float32, device=flow.device)
    with torch.cuda.device(flow.device):
        ws, nb = _loss_workspace(B, H, W, flow.device)
        rc = lib.pwc_epipolar_loss_fwd(flow.data_ptr(), Fd.data_ptr(), fbs, _ptr(okt), obs, _ptr(m), u8, out.data_ptr(), B, H, W,
                                       ROBUST_CODES.get(robust, 2), float(delta), float(weight), bsf, bsm, ws.data_ptr(), nb,
                                       _stream(flow))
    check(rc, "pwc_epipolar_loss_fwd")
    return out[0]


def epipolar_loss_backward(flow: torch.Tensor, F, ok, valid_mask: Optional[torch.Tensor], grad_out: torch.Tensor,
                           robust: str = "huber", delta: float = 1.0, weight: float = 0.1) -> torch.Tensor:
    """grad_flow [B,2,H,W] of epipolar_loss for the upstream gradient grad_out (a float32 device scalar; no host sync)."""
    lib = _lib.load()
    flow, bsf, (B, H, W), Fd, fbs, okt, obs, m, u8, bsm = _loss_args(flow, F, ok, valid_mask)
    g = grad_out.to(device=flow.device, dtype=torch.float32).contiguous().reshape(1)
    gf = torch.empty((B, 2, H, W), dtype=torch.float32, device=flow.device)
    with torch.cuda.device(flow.device):
        ws, nb = _loss_workspace(B, H, W, flow.device)
        rc = lib.pwc_epipolar_loss_bwd(flow.data_ptr(), Fd.data_ptr(), fbs, _ptr(okt), obs, _ptr(m), u8, g.data_ptr(), gf.data_ptr(),
                                       B, H, W, ROBUST_CODES.get(robust, 2), float(delta), float(weight), bsf, bsm, ws.data_ptr(), nb,
                                       _stream(flow))
    check(rc, "pwc_epipolar_loss_bwd")
    return gf


class EpipolarSampsonFunction(torch.autograd.Function):
    """autograd of epipolar_loss w.r.t. the flow (F, ok and the mask are constants): apply(flow, F, ok, valid_mask, robust,
    delta, weight) -> float32 scalar.  Under torch.autocast the flow is cast to float32."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, flow, F, ok=None, valid_mask=None, robust="huber", delta=1.0, weight=0.1):
        ctx.save_for_backward(flow)
        ctx.consts = (F, ok, valid_mask)
        ctx.cfg = (robust, float(delta), float(weight))
        return epipolar_loss(flow, F, ok, valid_mask, *ctx.cfg)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        (flow,) = ctx.saved_tensors
        F, ok, m = ctx.consts
        gf = epipolar_loss_backward(flow, F, ok, m, grad_out, *ctx.cfg)
        return gf, None, None, None, None, None, None


# ---------------------------------------------------------------- fused Adam / AdamW step with gradient clipping (optim.py)
def optim_chunk_elems() -> int:
    """Elements of one chunk (one workgroup) of the optimizer kernels; the host's chunk table is cut with it."""
    return int(_lib.load().pwc_optim_chunk_elems())


def optim_workspace_bytes(nchunks: int, ngroups: int) -> int:
    return _query_bytes(_lib.load().pwc_optim_workspace_bytes(int(nchunks), int(ngroups)), "optimizer workspace")


def _optim_tables(grads: torch.Tensor, tensors: torch.Tensor, chunks: torch.Tensor, nchunks: int):
    dev = grads.device
    ntensors = grads.numel()
    return (_table_arg(grads, torch.int64, 1, dev, "grads"), _table_arg(tensors, torch.int64, 4 * ntensors, dev, "tensors"),
            _table_arg(chunks, torch.int32, 2 * nchunks, dev, "chunks"))


def optim_grad_sqsum(grads: torch.Tensor, tensors: torch.Tensor, chunks: torch.Tensor, nchunks: int, ngroups: int,
                     workspace: torch.Tensor) -> None:
    """pwc_optim_grad_sqsum: one float64 partial of the sum of g^2 per chunk into the workspace.  grads int64 [ntensors] (device
    addresses, 0 = no gradient), tensors int64 [ntensors, 4] = (p, m, v, numel), chunks int32 [nchunks, 2] = (tensor, chunk)."""
    pg, pt, pc = _optim_tables(grads, tensors, chunks, nchunks)
    pw, nb = _workspace_args(workspace, grads)
    with torch.cuda.device(grads.device):
        rc = _lib.load().pwc_optim_grad_sqsum(pg, pt, pc, nchunks, ngroups, pw, nb, _stream(grads))
    check(rc, "pwc_optim_grad_sqsum")


def optim_finish(workspace: torch.Tensor, nchunks: int, ngroups: int, group: int, max_norm: Optional[float],
                 found_inf: Optional[torch.Tensor], grad_scale: Optional[torch.Tensor], lr: float, beta1: float, beta2: float,
                 step_record: torch.Tensor, norm_out: Optional[torch.Tensor]) -> None:
    """pwc_optim_finish for one parameter group: total norm and clip coefficient from the partials (max_norm None: no clipping,
    coefficient 1), GradScaler's found_inf / grad_scale, step_record float64 [ngroups, 3] = (step, beta1^step, beta2^step) advanced
    unless the step is skipped, the constants of the update written to the workspace."""
    dev = workspace.device
    pw, nb = _workspace_args(workspace, workspace)
    clip = max_norm is not None
    with torch.cuda.device(dev):
        rc = _lib.load().pwc_optim_finish(pw, nb, nchunks, ngroups, group, int(clip), float(max_norm) if clip else 0.0,
                                          _scalar_arg(found_inf, dev, "found_inf"), _scalar_arg(grad_scale, dev, "grad_scale"),
                                          float(lr), float(beta1), float(beta2),
                                          _table_arg(step_record, torch.float64, 3 * ngroups, dev, "step_record"),
                                          _scalar_arg(norm_out, dev, "norm_out"), _stream(workspace))
    check(rc, "pwc_optim_finish")


def optim_adam_update(grads: torch.Tensor, tensors: torch.Tensor, chunks: torch.Tensor, nchunks: int, chunk_begin: int,
                      chunk_count: int, ngroups: int, group: int, workspace: torch.Tensor, lr: float, beta1: float, beta2: float,
                      eps: float, weight_decay: float, decoupled: bool) -> None:
    """pwc_optim_adam_update: p, m, v of the chunks [chunk_begin, chunk_begin + chunk_count) updated in place with the constants
    pwc_optim_finish left for this group (include/pwc_hip.h has the arithmetic); the gradients are not modified."""
    pg, pt, pc = _optim_tables(grads, tensors, chunks, nchunks)
    pw, nb = _workspace_args(workspace, grads)
    with torch.cuda.device(grads.device):
        rc = _lib.load().pwc_optim_adam_update(pg, pt, pc, nchunks, chunk_begin, chunk_count, ngroups, group, pw, nb, float(lr),
                                               float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(decoupled)),
                                               _stream(grads))
    check(rc, "pwc_optim_adam_update")
