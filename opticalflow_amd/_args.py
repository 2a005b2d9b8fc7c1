"""Argument adapters shared by the wrappers of ops.py and ops_f16.py: each turns one kind of tensor argument into what the C ABI
takes (pointer, batch stride, byte count) and raises before anything is launched when the kernels' assumptions do not hold.
A new operator takes its adapters from here and does not copy them."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import PWC_F16, PWC_F32, PwcHipError

_DTYPES = {torch.float32: PWC_F32, torch.float16: PWC_F16}


def _dtype_code(t: torch.Tensor) -> int:
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise TypeError("unsupported dtype %s (float32 / float16 only)" % t.dtype) from None


def _require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise PwcHipError("%s is on %s: the HIP path needs device tensors and has no CPU fallback" % (name, t.device))


def _plane_dense(t: torch.Tensor, name: str) -> int:
    """Require [B,C,H,W] with dense C,H,W planes; return the batch stride in elements."""
    if t.dim() != 4:
        raise ValueError("%s must be 4-D [B,C,H,W], got %s" % (name, tuple(t.shape)))
    _require_device(t, name)
    B, C, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    ok = (W == 1 or sw == 1) and (H == 1 or sh == W) and (C == 1 or sc == H * W)
    if not ok:
        raise ValueError("%s must have dense C,H,W planes (strides %s for shape %s)" % (name, t.stride(), tuple(t.shape)))
    if B == 1:
        return C * H * W
    if sb < C * H * W:
        raise ValueError("%s batch stride %d smaller than C*H*W" % (name, sb))
    return sb


def _frames_dense(t: torch.Tensor, name: str) -> int:
    """uint8 device frames [n,H,W,3] with dense [H,W,3] frames -> the batch stride in bytes (free, e.g. one half of a pair buffer)."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError("%s must be a uint8 device tensor [n,H,W,3]" % name)
    n, H, W, _ = t.shape
    if min(n, H, W) <= 0:
        raise ValueError("%s: every size must be positive" % name)
    sb, sh, sw, sc = t.stride()
    if sc != 1 or (W > 1 and sw != 3) or (H > 1 and sh != 3 * W) or (n > 1 and sb < 3 * H * W):
        raise ValueError("%s must have dense [H,W,3] frames (strides %s for shape %s)" % (name, t.stride(), tuple(t.shape)))
    return sb if n > 1 else 3 * H * W


def _raw_frames_shape(t, name: str) -> Tuple[int, int, int]:
    """(n, H, W) of raw frames: a uint8 tensor [n,H,W,3] with positive sizes, wherever it lives.  Says which property fails (TypeError
    for the dtype); _frames_dense then checks placement and strides."""
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.uint8:
        raise TypeError("%s must be uint8 (raw frames), got %s" % (name, t.dtype))
    if t.dim() != 4:
        raise ValueError("%s must be 4-D [n,H,W,3], got %s" % (name, tuple(t.shape)))
    if t.shape[3] != 3:
        raise ValueError("%s must have 3 interleaved channels last [n,H,W,3], got %s" % (name, tuple(t.shape)))
    n, H, W, _ = t.shape
    if min(n, H, W) <= 0:
        raise ValueError("%s: every size must be positive, got %s" % (name, tuple(t.shape)))
    return n, H, W


def densify(t: torch.Tensor) -> torch.Tensor:
    """Return t if its C,H,W planes are dense (batch stride free), else a contiguous copy."""
    if t.dim() == 4:
        B, C, H, W = t.shape
        sb, sc, sh, sw = t.stride()
        if (W == 1 or sw == 1) and (H == 1 or sh == W) and (C == 1 or sc == H * W) and (B == 1 or sb >= C * H * W):
            return t
    return t.contiguous()


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of an optional tensor (None = NULL)."""
    return t.data_ptr() if t is not None else None


def _f32_dense(t: torch.Tensor, name: str, shape, device) -> Tuple[torch.Tensor, int]:
    """float32 tensor of this shape on this device with dense planes (copied when they are not) -> (tensor, batch stride)."""
    t = densify(t)
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != device:
        raise ValueError("%s must be float32 %s on %s, got %s %s on %s" % (name, tuple(shape), device, t.dtype, tuple(t.shape), t.device))
    return t, _plane_dense(t, name)


def _out_arg(out: Optional[torch.Tensor], shape, dtype, device, contiguous: bool = False) -> torch.Tensor:
    """The caller's `out` after a check of shape, dtype and device (and contiguity where the kernel needs it), or a new tensor."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or (contiguous and not out.is_contiguous()):
        raise ValueError("out must be %s%s %s on %s, got %s %s on %s" % ("contiguous " if contiguous else "", dtype, tuple(shape), device,
                                                                      out.dtype, tuple(out.shape), out.device))
    return out


def _bias_arg(bias: torch.Tensor, cout: int, device) -> torch.Tensor:
    if bias.dtype != torch.float32 or bias.numel() != cout or bias.device != device or not bias.is_contiguous():
        raise ValueError("bias must be float32[%d] on %s" % (cout, device))
    return bias


def _packed_arg(packed: torch.Tensor, need: int, device, what: str) -> torch.Tensor:
    """Packed float32 filters whose byte count is the library's for this layer."""
    if packed.dtype != torch.float32 or packed.numel() * 4 != need or packed.device != device:
        raise ValueError("packed %s do not match the layer (have %d B, need %d B on %s)"
                         % (what, packed.numel() * packed.element_size(), need, device))
    return packed


def _workspace_args(workspace: Optional[torch.Tensor], x: torch.Tensor) -> Tuple[int, int]:
    if workspace is None:
        return 0, 0
    if workspace.device != x.device or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous tensor on %s" % x.device)
    return workspace.data_ptr(), workspace.numel() * workspace.element_size()


def _query_bytes(n: int, what: str) -> int:
    """Result of one of the library's *_bytes queries; they answer < 0 for a geometry they do not take."""
    if n < 0:
        raise ValueError("bad %s geometry" % what)
    return int(n)


def _scratch(nbytes: int, device) -> Tuple[torch.Tensor, int]:
    """8-byte aligned device scratch of at least nbytes -> (tensor, nbytes)."""
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device), nbytes


def _mask_arg(mask: Optional[torch.Tensor], B: int, H: int, W: int, device, rule: str,
              name: str = "mask") -> Tuple[Optional[torch.Tensor], int, int]:
    """[B,H,W] / [B,1,H,W] mask as the kernels read it: (contiguous tensor, mask_u8, batch stride), (None, 0, 0) without one.
    bool -> its bytes, uint8 and float32 as they are.  Any other dtype by `rule`, which is the decision the operator's kernel takes
    on a float32 mask: "threshold" -> (mask > 0.5) as bytes, "nonzero" -> (mask != 0) as bytes, "raw" -> the values as float32."""
    if rule not in ("threshold", "raw", "nonzero"):
        raise ValueError("unknown mask rule %r" % (rule,))
    if mask is None:
        return None, 0, 0
    if mask.dim() == 4:
        mask = mask[:, 0]
    if tuple(mask.shape) != (B, H, W) or mask.device != device:
        raise ValueError("%s must be [B,H,W] or [B,1,H,W] = %s on %s, got %s on %s"
                         % (name, (B, H, W), device, tuple(mask.shape), mask.device))
    if mask.dtype == torch.bool:
        m, u8 = mask.contiguous().view(torch.uint8), 1
    elif mask.dtype == torch.uint8:
        m, u8 = mask.contiguous(), 1
    elif mask.dtype == torch.float32:
        m, u8 = mask.contiguous(), 0
    elif rule == "raw":
        m, u8 = mask.contiguous().float(), 0
    else:
        m, u8 = ((mask > 0.5) if rule == "threshold" else (mask != 0)).contiguous().view(torch.uint8), 1
    return m, u8, H * W


def _kitti_gt_arg(gt: torch.Tensor, valid: Optional[torch.Tensor], n: int, H: int, W: int, device) -> Tuple[int, Optional[torch.Tensor]]:
    """The two forms of KITTI ground truth -> (gt_kind, valid as the kernels read it).  torch.uint16 [n,H,W,3] is the flow PNG's
    samples (R G B; validity is the blue sample, so `valid` must be None): kind 1.  float32 [n,2,H,W] are flow planes with `valid`
    None / bool / uint8 [n,H,W] (bool is returned as its bytes): kind 0.  Everything is contiguous and on `device`."""
    if gt.dtype == torch.uint16:
        kind, want = 1, (n, H, W, 3)
        if valid is not None:
            raise ValueError("valid must be None with uint16 ground truth (the blue sample is the validity)")
    elif gt.dtype == torch.float32:
        kind, want = 0, (n, 2, H, W)
        if valid is not None:
            if valid.dtype == torch.bool:
                valid = valid.view(torch.uint8)
            if valid.dtype != torch.uint8 or tuple(valid.shape) != (n, H, W) or valid.device != device or not valid.is_contiguous():
                raise ValueError("valid must be a contiguous bool / uint8 %s tensor on %s" % ((n, H, W), device))
    else:
        raise ValueError("gt must be torch.uint16 [n,H,W,3] or float32 [n,2,H,W], got %s" % gt.dtype)
    if tuple(gt.shape) != want or gt.device != device or not gt.is_contiguous():
        raise ValueError("gt must be contiguous %s %s on %s, got %s on %s" % (gt.dtype, want, device, tuple(gt.shape), gt.device))
    return kind, valid


def _table_arg(t: torch.Tensor, dtype, min_numel: int, device, name: str) -> int:
    """Device pointer of a contiguous table of at least min_numel elements of this dtype on this device (the kernels trust its
    contents; its placement is checked here)."""
    _require_device(t, name)
    if t.dtype != dtype or t.device != device or not t.is_contiguous() or t.numel() < min_numel:
        raise ValueError("%s must be a contiguous %s table of at least %d elements on %s, got %s[%d] on %s"
                         % (name, dtype, min_numel, device, t.dtype, t.numel(), t.device))
    return t.data_ptr()


def _scalar_arg(t: Optional[torch.Tensor], device, name: str) -> Optional[int]:
    """Device pointer of an optional one-element float32 scalar on this device (None = NULL)."""
    if t is None:
        return None
    _require_device(t, name)
    if t.dtype != torch.float32 or t.numel() != 1 or t.device != device:
        raise ValueError("%s must be one float32 element on %s, got %s[%d] on %s" % (name, device, t.dtype, t.numel(), t.device))
    return t.data_ptr()
