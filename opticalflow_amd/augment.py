"""KITTI training batches on the device: the host side of pwc_kitti_augment (include/pwc_hip.h, csrc/pwc_augment.hip).

KittiFlowDataset.__getitem__ (data_processing_or.py:228-294) warps, crops and flips every sample on the host and ships 9 float32
planes per sample; here the host only draws the per-sample parameters -- in the reference's order, so that the same `random.seed`
gives the same augmentation -- and the raw uint8 frames and the ground truth (uint16 PNG samples or float planes) are uploaded as they
are.  One launch per batch then writes the (x, flow_gt, valid) that train_one_epoch consumes.  cv2.warpAffine is defined by the
restatement of OpenCV's classic fixed-point path in the header; parity against an actual cv2 build is unpinned.

The reference's "upsize first when the frame is smaller than the crop" branch (:259-268) is not provided: ValueError."""
from __future__ import annotations

import random as _random
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._args import _require_device
from ._pipeline import PinnedRing

# pwc_augment_params: the inverted matrix (fp64), the forward linear part (fp32), crop origin, the sample's size, flags
PARAMS_DTYPE = np.dtype([("m", "<f8", (6,)), ("a", "<f4", (4,)), ("y0", "<i4"), ("x0", "<i4"), ("h", "<i4"), ("w", "<i4"),
                         ("warp", "<i4"), ("flip", "<i4")])
assert PARAMS_DTYPE.itemsize == ops.AUGMENT_RECORD_BYTES


def affine_matrix(center_xy, rot_deg: float, sx: float, sy: float) -> Tuple[np.ndarray, np.ndarray]:
    """(M float32 2x3, A float32 2x2) of _cv2_affine_matrix (data_processing_or.py:92-110) without a translation: A = R S in float32
    from float64 cos / sin, t = c - A c in float32 (each product and sum rounded to float32, no fused multiply-add)."""
    f32 = np.float32
    theta = np.deg2rad(rot_deg)
    cos_t, sin_t = np.cos(theta), np.sin(theta)
    A = np.array([[sx * cos_t, -sy * sin_t], [sx * sin_t, sy * cos_t]], dtype=np.float32)
    cx, cy = f32(center_xy[0]), f32(center_xy[1])
    t = np.array([cx - f32(f32(A[0, 0] * cx) + f32(A[0, 1] * cy)), cy - f32(f32(A[1, 0] * cx) + f32(A[1, 1] * cy))], dtype=np.float32)
    return np.concatenate([A, t[:, None]], axis=1), A


def invert_affine(M) -> np.ndarray:
    """The six doubles cv::warpAffine maps destination to source pixels with: M converted to double and inverted as OpenCV does."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0.0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return np.array(m, dtype=np.float64)


def make_params(n: int) -> np.ndarray:
    """n records that do nothing: identity matrix, no warp, no flip, origin (0, 0); the size fields are left 0 for the caller."""
    p = np.zeros(n, dtype=PARAMS_DTYPE)
    p["m"][:, 0] = p["m"][:, 4] = 1.0
    p["a"][:, 0] = p["a"][:, 3] = 1.0
    return p


def set_affine(rec, size_hw, rot_deg: float, sx: float, sy: float) -> None:
    """Fill one record's matrix fields for a warp about the centre of an H x W frame and switch its warp on."""
    H, W = size_hw
    M, A = affine_matrix((W * 0.5, H * 0.5), rot_deg, sx, sy)
    rec["m"] = invert_affine(M)
    rec["a"] = A.reshape(4)
    rec["warp"] = 1


def sample_params(sizes: Sequence[Tuple[int, int]], crop_hw: Tuple[int, int] = (320, 896), apply_aug: bool = True, rng=_random) -> np.ndarray:
    """Per-sample records (PARAMS_DTYPE) for frames of the given (H, W), drawn from `rng` (the `random` module or a random.Random) in
    the order KittiFlowDataset.__getitem__ draws: random() < 0.4 skips the warp, else uniform(-2, 2) degrees, uniform(.95, 1.05) zoom,
    uniform(.97, 1.03) squeeze twice; then randint(0, H - crop_h) unless they are equal, the same for x; then random() < 0.3 flips.
    apply_aug=False draws only the crop.  After random.seed(s) the records are those of the reference's next len(sizes) samples."""
    ch, cw = int(crop_hw[0]), int(crop_hw[1])
    p = make_params(len(sizes))
    for rec, (H, W) in zip(p, sizes):
        H, W = int(H), int(W)
        if H < ch or W < cw:
            raise ValueError("a %dx%d frame is smaller than the %dx%d crop (the reference's upsize branch is not provided)" % (H, W, ch, cw))
        rec["h"], rec["w"] = H, W
        if apply_aug and not rng.random() < 0.4:
            rot = rng.uniform(-2.0, 2.0)
            zoom = rng.uniform(0.95, 1.05)
            sqx = rng.uniform(0.97, 1.03)
            sqy = rng.uniform(0.97, 1.03)
            set_affine(rec, (H, W), rot, zoom * sqx, zoom * sqy)
        rec["y0"] = 0 if H == ch else rng.randint(0, H - ch)
        rec["x0"] = 0 if W == cw else rng.randint(0, W - cw)
        if apply_aug and rng.random() < 0.3:
            rec["flip"] = 1
    return p


def check_params(params: np.ndarray, n: int, slot_hw: Tuple[int, int], crop_hw: Tuple[int, int], dtype: np.dtype = PARAMS_DTYPE,
                 too_small: str = " (the reference's upsize branch is not provided)") -> np.ndarray:
    """The records as a contiguous array of `dtype` after the checks both kernels repeat on the device (there a record that fails is
    answered with zeros and a status flag; here it is a ValueError before anything is uploaded): dtype and shape, the sample fits its
    slot, the crop fits the sample, the crop origin keeps the window inside it.  `too_small` ends the message about a frame smaller
    than the crop.  augment_full.check_full_params adds the checks of its own record."""
    p = np.ascontiguousarray(params)
    if p.dtype != dtype or p.shape != (n,):
        raise ValueError("params must be %d records of the %d-byte parameter dtype, got %s %s" % (n, dtype.itemsize, p.dtype, p.shape))
    (Hs, Ws), (ch, cw) = slot_hw, crop_hw
    for b, r in enumerate(p):
        H, W = int(r["h"]), int(r["w"])
        if not (1 <= H <= Hs and 1 <= W <= Ws):
            raise ValueError("sample %d: size %dx%d does not fit the %dx%d slot" % (b, H, W, Hs, Ws))
        if ch > H or cw > W:
            raise ValueError("sample %d: a %dx%d frame is smaller than the %dx%d crop%s" % (b, H, W, ch, cw, too_small))
        if not (0 <= int(r["y0"]) <= H - ch and 0 <= int(r["x0"]) <= W - cw):
            raise ValueError("sample %d: crop origin (%d, %d) outside [0, %d] x [0, %d]" % (b, r["y0"], r["x0"], H - ch, W - cw))
    return p


def pack_slots(samples, slot_hw: Tuple[int, int], gt_kind: int, frames=None, gt=None, valid=None):
    """Host samples of differing sizes -> the slot arrays the kernel reads: (frames uint8 [n,2,Hs,Ws,3], gt, valid, sizes).  A sample
    is (img1, img2, png) with png uint16 [H,W,3] for gt_kind 1, or (img1, img2, flow [H,W,2] float32, valid [H,W] or None) for gt_kind
    0 (valid is then uint8 [n,Hs,Ws]; None for every sample -> None).  Sample b is written densely at the start of its slot with its
    own row stride W_b; the rest of a slot is left as it is.  frames / gt / valid: existing arrays to fill (pinned staging)."""
    Hs, Ws = slot_hw
    n = len(samples)
    if gt_kind not in (0, 1):
        raise ValueError("gt_kind must be 0 (float planes) or 1 (uint16 PNG samples), got %r" % (gt_kind,))
    if frames is None:
        frames = np.zeros((n, 2, Hs, Ws, 3), np.uint8)
    if gt is None:
        gt = np.zeros((n, Hs, Ws, 3), np.uint16) if gt_kind == 1 else np.zeros((n, 2, Hs, Ws), np.float32)
    with_valid = gt_kind == 0 and any(len(s) > 3 and s[3] is not None for s in samples)
    if with_valid and valid is None:
        valid = np.zeros((n, Hs, Ws), np.uint8)
    sizes = []
    for b, s in enumerate(samples):
        if len(s) != (3 if gt_kind == 1 else 4) and not (gt_kind == 0 and len(s) == 3):
            raise ValueError("sample %d: expected (img1, img2, png) or (img1, img2, flow, valid)" % b)
        im1, im2 = np.asarray(s[0]), np.asarray(s[1])
        if im1.dtype != np.uint8 or im1.ndim != 3 or im1.shape[2] < 3 or im2.dtype != np.uint8 or im2.shape != im1.shape:
            raise ValueError("sample %d: the frames must be two uint8 [H,W,>=3] images of one size" % b)
        H, W = im1.shape[:2]
        if H > Hs or W > Ws:
            raise ValueError("sample %d: %dx%d does not fit the %dx%d slot" % (b, H, W, Hs, Ws))
        sizes.append((H, W))
        fl = frames[b].reshape(2, Hs * Ws * 3)
        np.copyto(fl[0, :H * W * 3].reshape(H, W, 3), im1[..., :3])
        np.copyto(fl[1, :H * W * 3].reshape(H, W, 3), im2[..., :3])
        g = np.asarray(s[2])
        if gt_kind == 1:
            if g.dtype != np.uint16 or g.shape != (H, W, 3):
                raise ValueError("sample %d: the ground truth must be uint16 %s" % (b, (H, W, 3)))
            np.copyto(gt[b].reshape(Hs * Ws * 3)[:H * W * 3].reshape(H, W, 3), g)
        else:
            if g.dtype != np.float32 or g.shape != (H, W, 2):
                raise ValueError("sample %d: the flow must be float32 %s" % (b, (H, W, 2)))
            gl = gt[b].reshape(2, Hs * Ws)
            np.copyto(gl[0, :H * W].reshape(H, W), g[..., 0])
            np.copyto(gl[1, :H * W].reshape(H, W), g[..., 1])
            if with_valid:
                v = s[3] if len(s) > 3 and s[3] is not None else np.ones((H, W), np.uint8)
                v = np.asarray(v)
                if v.shape != (H, W):
                    raise ValueError("sample %d: valid must be %s" % (b, (H, W)))
                np.copyto(valid[b].reshape(Hs * Ws)[:H * W].reshape(H, W), v != 0, casting="unsafe")
    return frames, gt, (valid if with_valid else None), sizes


def _params_tensor(p: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(p.view(np.uint8).reshape(p.shape[0], p.dtype.itemsize))


def _augment_batch(op, check, pairs_u8, gt, valid, params, crop_hw, out, return_status):
    """augment_batch and augment_full.augment_full_batch: validate the host records with `check`, upload them, launch `op`."""
    _require_device(pairs_u8, "pairs_u8")
    if pairs_u8.dim() != 5:
        raise ValueError("pairs_u8 must be uint8 [n,2,Hs,Ws,3], got %s" % (tuple(pairs_u8.shape),))
    n, _, Hs, Ws, _ = pairs_u8.shape
    crop_hw = (int(crop_hw[0]), int(crop_hw[1]))
    p = check(params, n, (Hs, Ws), crop_hw)
    pd = _params_tensor(p).to(pairs_u8.device, non_blocking=True)
    x, flow, v, status = op(pairs_u8, gt, pd, crop_hw, valid=valid, out=out)
    return (x, flow, v, status) if return_status else (x, flow, v)


def augment_batch(pairs_u8: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor], params: np.ndarray,
                  crop_hw: Tuple[int, int] = (320, 896), out=None, return_status: bool = False):
    """(x [n,6,ch,cw], flow [n,2,ch,cw], valid [n,1,ch,cw]) float32 on the device from slot tensors already there: pairs_u8 uint8
    [n,2,Hs,Ws,3], gt torch.uint16 [n,Hs,Ws,3] (valid None) or float32 [n,2,Hs,Ws] with valid None / bool / uint8 [n,Hs,Ws] (layout:
    pack_slots).  params: PARAMS_DTYPE records on the host (sample_params), validated here and uploaded.  return_status=True adds the
    kernel's int32 [n] status (all zero after the host checks)."""
    return _augment_batch(ops.kitti_augment, check_params, pairs_u8, gt, valid, params, crop_hw, out, return_status)


class StagedAugmenter:
    """The staging driver of both augmentation operators: host samples of differing sizes in, the device batch out.

    Pinned staging, the device slots, the parameter buffer and the outputs are allocated once for `batch` samples of at most
    `max_hw`; `__call__(samples, params=None)` copies the samples into the staging slots (pack_slots), starts the uploads on the
    current stream, launches the kernel behind them and returns views of the output tensors, which the next call overwrites.  Nothing
    synchronises except the wait for the previous upload before the staging memory is rewritten.  gt_kind 1 takes (img1, img2, png
    uint16 [H,W,3]) samples, gt_kind 0 (img1, img2, flow float32 [H,W,2], valid [H,W] or None).  `stage`, `upload` and `run` are the three
    steps of a call; `run` alone may be captured in a graph and replayed after each `stage` + `upload`.

    A subclass states `dtype` (the record), `third` (the name of its third output, the attribute next to `x`, `flow` and `status`),
    `sample(sizes)` and `check(params, n)` (how records are drawn and checked) and `op` (what `run` launches)."""

    def __init__(self, device, batch: int, max_hw: Tuple[int, int], crop_hw: Tuple[int, int] = (320, 896), gt_kind: int = 1):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ops.PwcHipError("%s needs a GPU device, got %s: there is no CPU fallback" % (type(self).__name__, self.device))
        Hs, Ws = int(max_hw[0]), int(max_hw[1])
        ch, cw = int(crop_hw[0]), int(crop_hw[1])
        if batch < 1 or not (1 <= ch <= Hs and 1 <= cw <= Ws):
            raise ValueError("crop %dx%d does not fit the %dx%d slot (or the batch is empty)" % (ch, cw, Hs, Ws))
        if gt_kind not in (0, 1):
            raise ValueError("gt_kind must be 0 or 1, got %r" % (gt_kind,))
        self.batch, self.slot_hw, self.crop_hw, self.gt_kind = batch, (Hs, Ws), (ch, cw), gt_kind
        shapes = [((batch, 2, Hs, Ws, 3), torch.uint8),
                  ((batch, Hs, Ws, 3), torch.uint16) if gt_kind == 1 else ((batch, 2, Hs, Ws), torch.float32),
                  ((batch, Hs, Ws), torch.uint8), ((batch, self.dtype.itemsize), torch.uint8)]
        self._ring, self._specs = PinnedRing(1), shapes                # one staging slot of four tensors, zeroed once
        self._host = self._ring.acquire(*shapes)
        self._views = [t.zero_().numpy() for t in self._host]
        self._dev = [torch.zeros(s, dtype=d, device=self.device) for s, d in shapes]
        self.x = torch.empty((batch, 6, ch, cw), dtype=torch.float32, device=self.device)
        self.flow = torch.empty((batch, 2, ch, cw), dtype=torch.float32, device=self.device)
        self._third = torch.empty((batch, 1, ch, cw), dtype=torch.float32, device=self.device)
        setattr(self, self.third, self._third)
        self.status = torch.zeros(batch, dtype=torch.int32, device=self.device)
        self._n, self._with_valid = 0, False

    def stage(self, samples, params: Optional[np.ndarray] = None) -> np.ndarray:
        """Fill the pinned staging memory from the host samples and their records (drawn with `sample` when None)."""
        n = len(samples)
        if not 1 <= n <= self.batch:
            raise ValueError("expected 1..%d samples, got %d" % (self.batch, n))
        self._ring.acquire(*self._specs)                   # the copy that last read the staging memory is done before it is rewritten
        fr, gt, va, _ = self._views
        _, _, v, sizes = pack_slots(samples, self.slot_hw, self.gt_kind, frames=fr[:n], gt=gt[:n], valid=va[:n])
        if params is None:
            params = self.sample(sizes)
        p = self.check(params, n)
        for b, (H, W) in enumerate(sizes):
            if (int(p[b]["h"]), int(p[b]["w"])) != (H, W):
                raise ValueError("sample %d is %dx%d but its record says %dx%d" % (b, H, W, p[b]["h"], p[b]["w"]))
        np.copyto(self._views[3][:n], p.view(np.uint8).reshape(n, -1))
        self._n, self._with_valid = n, v is not None
        return p

    def upload(self) -> None:
        """Start the copies of what `stage` left to the device slots on the current stream."""
        n = self._n
        if n < 1:
            raise RuntimeError("%s.upload before stage" % type(self).__name__)
        use = (0, 1, 3) + ((2,) if self._with_valid else ())
        with torch.cuda.device(self.device):
            for i in use:
                self._dev[i][:n].copy_(self._host[i][:n], non_blocking=True)
            self._ring.mark()

    def run(self):
        """The kernel alone, on the device slots as they are, on the current stream -> views of the n staged samples in (x, flow, third
        output).  Nothing is allocated, so a graph may capture it and be replayed after each stage + upload of a batch of the same n."""
        n = self._n
        if n < 1:
            raise RuntimeError("%s.run before stage" % type(self).__name__)
        fr, gt, va, pr = self._dev
        out = (self.x[:n], self.flow[:n], self._third[:n])
        self.op(fr[:n], gt[:n], pr[:n], self.crop_hw, valid=va[:n] if self._with_valid else None, out=out, status=self.status[:n])
        return out

    def __call__(self, samples, params: Optional[np.ndarray] = None):
        self.stage(samples, params)
        self.upload()
        return self.run()


class DeviceAugmenter(StagedAugmenter):
    """The training loop's data path (train.py): host samples in, the device batch (x, flow_gt, valid) out, records drawn with
    sample_params.  Constructor, steps and attributes: StagedAugmenter."""

    dtype, third, op = PARAMS_DTYPE, "valid", staticmethod(ops.kitti_augment)

    def sample(self, sizes):
        return sample_params(sizes, self.crop_hw)

    def check(self, params, n):
        return check_params(params, n, self.slot_hw, self.crop_hw)
