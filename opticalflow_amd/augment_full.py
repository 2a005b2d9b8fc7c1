"""train2.py's training batches on the device: the host side of pwc_kitti_augment_full (include/pwc_hip.h, csrc/pwc_augment_full.hip).

KittiAugmentationPipeline (data_processing.py:136-279) runs per sample inside train2.py's collate_fn on the host: crop, flip, up to two
cv2.warpAffine calls over nine float planes, a brightness / contrast map and a cv2.GaussianBlur of both frames.  Here the host only
draws the per-sample parameters -- in the reference's order from NumPy's generator, so that the same `np.random.seed` gives the same
augmentation -- and the raw uint8 frames and the ground truth are uploaded as they are, in the slot layout of opticalflow_amd.augment
(`pack_slots`).  One launch per batch then writes (x, flow, mask).  cv2.getRotationMatrix2D, cv2.warpAffine and the 8U cv2.GaussianBlur
are defined by the restatements in the header; parity against an actual cv2 build is unpinned, and the blur weights are rounded from a
float64 Gaussian where OpenCV uses softdouble.

A frame smaller than the crop is a ValueError (the reference would return a short tensor that torch.stack rejects)."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .augment import StagedAugmenter, _augment_batch, check_params, invert_affine

# pwc_augment_full_params
FULL_PARAMS_DTYPE = np.dtype([("m", "<f8", (6,)), ("cs", "<f8", (2,)), ("gain", "<f4"), ("wk", "<u2", (7,)), ("ksize", "<u2"),
                              ("y0", "<i4"), ("x0", "<i4"), ("h", "<i4"), ("w", "<i4"), ("tx", "<i4"), ("ty", "<i4"),
                              ("flip", "<i4"), ("rot", "<i4"), ("trans", "<i4"), ("bright", "<i4"), ("blur", "<i4")])
assert FULL_PARAMS_DTYPE.itemsize == ops.AUGMENT_FULL_RECORD_BYTES
MAX_SHIFT = ops.AUGMENT_FULL_MAX_SHIFT


def rotation_matrix(center_xy, angle_deg: float) -> np.ndarray:
    """cv2.getRotationMatrix2D(center, angle, 1.0) restated in float64: [[a, b, (1-a) cx - b cy], [-b, a, b cx + (1-a) cy]] with
    a = cos(angle pi/180), b = sin(angle pi/180)."""
    rad = float(angle_deg) * (math.pi / 180.0)
    a, b = math.cos(rad), math.sin(rad)
    cx, cy = float(center_xy[0]), float(center_xy[1])
    return np.array([[a, b, (1.0 - a) * cx - b * cy], [-b, a, b * cx + (1.0 - a) * cy]], dtype=np.float64)


def gaussian_weights(sigma: float) -> Tuple[int, np.ndarray]:
    """(k, uint16 [k]): the reference's kernel size k = ceil(4 sigma) made odd, and the Q8.8 weights of OpenCV's bit-exact 8U
    GaussianBlur: the float64 kernel exp(-x^2 / (2 sigma^2)) / sum, converted from the outside in with the rounding error carried
    (v = rint(k_i 256 + err)), the centre taking what is left of 256.  OpenCV evaluates the kernel in softdouble (unpinned)."""
    sigma = float(sigma)
    k = int(math.ceil(4.0 * sigma))
    if k % 2 == 0:
        k += 1
    if not 3 <= k <= 7:
        raise ValueError("sigma %r gives a %d-tap kernel; 3, 5 and 7 taps are provided (the reference draws sigma in [0.5, 1.5))" % (sigma, k))
    r = k // 2
    e = [math.exp(-(float(i - r) ** 2) / (2.0 * sigma * sigma)) for i in range(k)]
    total = math.fsum(e)
    w = np.zeros(k, np.uint16)
    err, acc = 0.0, 0
    for i in range(r):
        adj = e[i] / total * 256.0 + err
        v = int(np.rint(adj))
        err = adj - v
        v = min(max(v, 0), 256)
        w[i] = w[k - 1 - i] = v
        acc += 2 * v
    if acc > 256:
        raise ValueError("sigma %r: the outer weights already exceed 256" % sigma)
    w[r] = 256 - acc
    return k, w


def make_full_params(n: int) -> np.ndarray:
    """n records that do nothing: identity matrix, cos 1, gain 1, the 3-tap identity blur kernel, every stage off, origin (0, 0);
    the size fields are left 0 for the caller."""
    p = np.zeros(n, dtype=FULL_PARAMS_DTYPE)
    p["m"][:, 0] = p["m"][:, 4] = 1.0
    p["cs"][:, 0] = 1.0
    p["gain"] = 1.0
    p["wk"][:, 1] = 256
    p["ksize"] = 3
    return p


def set_rotation(rec, crop_hw, angle_deg: float) -> None:
    """Switch one record's rotation on: about (crop_w // 2, crop_h // 2) as the reference, flow vectors by np.radians as the reference."""
    ch, cw = crop_hw
    rec["m"] = invert_affine(rotation_matrix((cw // 2, ch // 2), angle_deg))
    theta = np.radians(angle_deg)
    rec["cs"] = (np.cos(theta), np.sin(theta))
    rec["rot"] = 1


def set_blur(rec, sigma: float) -> None:
    k, w = gaussian_weights(sigma)
    rec["wk"] = 0
    rec["wk"][:k] = w
    rec["ksize"] = k
    rec["blur"] = 1


def sample_full_params(sizes: Sequence[Tuple[int, int]], crop_hw: Tuple[int, int] = (320, 896), augment: bool = True, rng=np.random) -> np.ndarray:
    """Per-sample records (FULL_PARAMS_DTYPE) for frames of the given (H, W), drawn from `rng` (the numpy.random module or a RandomState)
    in the order KittiAugmentationPipeline.__call__ draws: randint(0, H - ch + 1), randint(0, W - cw + 1) (both always drawn); then, if
    `augment`: rand() < 0.5 flips; rand() < 0.5 -> uniform(-17, 17) degrees; rand() < 0.5 -> randint(-10, 11) twice (tx, ty);
    rand() < 0.5 -> uniform(0.8, 1.2) twice (gain = float32 of their float64 product); rand() < 0.5 -> uniform(0.5, 1.5) sigma.
    After np.random.seed(s) the records are those of the reference's next len(sizes) samples."""
    ch, cw = int(crop_hw[0]), int(crop_hw[1])
    p = make_full_params(len(sizes))
    for rec, (H, W) in zip(p, sizes):
        H, W = int(H), int(W)
        if H < ch or W < cw:
            raise ValueError("a %dx%d frame is smaller than the %dx%d crop" % (H, W, ch, cw))
        rec["h"], rec["w"] = H, W
        rec["y0"] = rng.randint(0, H - ch + 1)
        rec["x0"] = rng.randint(0, W - cw + 1)
        if not augment:
            continue
        if rng.rand() < 0.5:
            rec["flip"] = 1
        if rng.rand() < 0.5:
            set_rotation(rec, (ch, cw), rng.uniform(-17, 17))
        if rng.rand() < 0.5:
            rec["tx"] = rng.randint(-10, 11)
            rec["ty"] = rng.randint(-10, 11)
            rec["trans"] = 1
        if rng.rand() < 0.5:
            b = rng.uniform(0.8, 1.2)
            c = rng.uniform(0.8, 1.2)
            rec["gain"] = np.float32(b * c)
            rec["bright"] = 1
        if rng.rand() < 0.5:
            set_blur(rec, rng.uniform(0.5, 1.5))
    return p


def check_full_params(params: np.ndarray, n: int, slot_hw: Tuple[int, int], crop_hw: Tuple[int, int]) -> np.ndarray:
    """The records as a contiguous FULL_PARAMS_DTYPE array after the checks the kernel repeats on the device: those of
    augment.check_params, then the shift range, the tap count and the weight sum."""
    p = check_params(params, n, slot_hw, crop_hw, dtype=FULL_PARAMS_DTYPE, too_small="")
    for b, r in enumerate(p):
        if r["trans"] and (abs(int(r["tx"])) > MAX_SHIFT or abs(int(r["ty"])) > MAX_SHIFT):
            raise ValueError("sample %d: shift (%d, %d) beyond +-%d" % (b, r["tx"], r["ty"], MAX_SHIFT))
        if r["blur"]:
            k = int(r["ksize"])
            if k not in (3, 5, 7):
                raise ValueError("sample %d: blur kernel of %d taps (3, 5 or 7)" % (b, k))
            if int(r["wk"][:k].astype(np.int64).sum()) != 256:
                raise ValueError("sample %d: the %d blur weights add up to %d, not 256" % (b, k, int(r["wk"][:k].astype(np.int64).sum())))
    return p


def augment_full_batch(pairs_u8: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor], params: np.ndarray,
                       crop_hw: Tuple[int, int] = (320, 896), out=None, return_status: bool = False):
    """(x [n,6,ch,cw], flow [n,2,ch,cw], mask [n,1,ch,cw]) float32 on the device from slot tensors already there (layout: augment.pack_slots,
    arguments: augment.augment_batch).  params: FULL_PARAMS_DTYPE records on the host (sample_full_params), validated here and uploaded.
    The mask is fractional after a rotation, as the reference's.  return_status=True adds the kernel's int32 [n] status."""
    return _augment_batch(ops.kitti_augment_full, check_full_params, pairs_u8, gt, valid, params, crop_hw, out, return_status)


class DeviceFullAugmenter(StagedAugmenter):
    """train2.py's collate_fn on the device: host samples in, the device batch (x, flow, mask) out, records drawn with
    sample_full_params; `augment=False` draws only the crop.  Constructor, steps and attributes: augment.StagedAugmenter."""

    dtype, third, op = FULL_PARAMS_DTYPE, "mask", staticmethod(ops.kitti_augment_full)

    def __init__(self, device, batch: int, max_hw: Tuple[int, int], crop_hw: Tuple[int, int] = (320, 896), gt_kind: int = 1,
                 augment: bool = True):
        super().__init__(device, batch, max_hw, crop_hw, gt_kind)
        self.augment = bool(augment)

    def sample(self, sizes):
        return sample_full_params(sizes, self.crop_hw, augment=self.augment)

    def check(self, params, n):
        return check_full_params(params, n, self.slot_hw, self.crop_hw)
