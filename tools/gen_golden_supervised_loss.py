"""Generate tests/golden/g10_supervised_loss.npz from the REFERENCE's own train.py / train2.py functions, in float64 on the CPU.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.
Recipe as tools/gen_golden_proxy_loss.py: process-local module stubs, no reference file is edited.  ``cv2``, ``albumentations``,
``albumentations.pytorch`` (with ``ToTensorV2``) and ``correlation_cuda`` become empty modules (``tqdm`` too when it is not
installed); ``data_processing_or`` is imported as it is, and a stub ``data_processing`` exposes the names the scripts import
from it, with ``upsample_flow_to = data_processing_or.upsample_flow_to`` (train.py imports it from a module that lacks it).
Stored per case: the inputs (float32), the loss and the float64 autograd gradient w.r.t. every flow level.

    python tools/gen_golden_supervised_loss.py [out.npz]
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PWC_REFERENCE", os.path.join(os.path.dirname(REPO), "reference"))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _import_reference():
    _stub("cv2")
    alb = _stub("albumentations")
    alb.pytorch = _stub("albumentations.pytorch", ToTensorV2=object)
    _stub("correlation_cuda")
    try:
        import tqdm  # noqa: F401
    except ImportError:
        _stub("tqdm", tqdm=lambda x, **k: x)
    sys.path.insert(0, REF)
    import data_processing_or as dpo    # noqa: E402  (the reference's own modules)
    _stub("data_processing", KittiFlowDataset=object, KittiDataset=object, KittiAugmentationPipeline=object,
          create_kitti_loaders=None, upsample_flow_to=dpo.upsample_flow_to)
    import train                        # noqa: E402
    import train2                       # noqa: E402
    sys.path.remove(REF)
    return dpo, train, train2


def f32(t):
    return torch.from_numpy(np.asarray(t, dtype=np.float32).astype(np.float64))


def flow(rng, shape, amp):
    B, _, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    f = amp * rng.uniform(-1, 1, size=shape)
    f[:, 0] += amp * np.sin(3 * xx + 2 * yy)
    f[:, 1] += amp * np.cos(2 * xx - 3 * yy)
    return f32(f)


def image(rng, shape):
    B, C, H, W = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty(shape)
    for b in range(B):
        for c in range(C):
            fx, fy, ph = rng.uniform(0.1, 0.5, size=3)
            out[b, c] = np.sin(fx * xx + fy * yy + 6 * ph) + 0.3 * (xx * rng.normal() + yy * rng.normal() > 0) \
                + 0.1 * rng.standard_normal((H, W))
    return f32(out)


# full-resolution losses: name -> (B, H, W, h, w, mask kind, function); mask kinds: "b1" [B,1,H,W] 0/1, "b" [B,H,W] 0/1,
# "raw" [B,H,W] uniform, "zero" all zero, "none"
FLOW_CASES = {
    "train": (1, 40, 112, 10, 28, "b1", "train"),        # train.py: MaskedCharbonnier on upsample_flow_to(flow2)
    "kitti_odd": (1, 47, 155, 12, 39, "b", "train2"),    # non-integer ratios, train2's MaskedCharbonnier ([B,H,W] mask)
    "same": (2, 24, 40, 24, 40, "b", "train2"),          # pred at GT size: the plain loss
    "allzero": (1, 20, 36, 5, 9, "zero", "train"),       # max(sum valid, 1)
    "epe_raw": (2, 37, 83, 9, 21, "raw", "epe"),         # compute_epe on the upsampled flow, raw mask
    "epe_none": (1, 30, 50, 8, 13, "none", "epe"),       # compute_epe without a mask: the mean
}
# multiscale: name -> (B, H, W, level sizes, w, lambda_photo, lambda_smooth, mask kind)
MS_CASES = {
    "ms": (2, 64, 96, ((16, 24), (8, 12), (4, 6), (3, 4), (2, 3)), None, 0.0, 0.0, "b"),
    "ms_reg": (1, 48, 80, ((12, 20), (6, 10), (3, 5)), None, 0.5, 0.3, "raw"),
    "ms_odd": (1, 37, 83, ((10, 21), (5, 11), (3, 6), (2, 3)), (1.0, 0.5), 0.2, 0.1, "b1"),
}


def mask_of(rng, kind, B, H, W):
    if kind == "none":
        return None
    if kind == "zero":
        return f32(np.zeros((B, 1, H, W)))
    if kind == "raw":
        return f32(rng.uniform(0, 1, size=(B, H, W)))
    m = (rng.uniform(0, 1, size=(B, H, W)) > 0.3).astype(np.float64)
    return f32(m[:, None] if kind == "b1" else m)


def main(out_path):
    dpo, train, train2 = _import_reference()
    torch.set_default_dtype(torch.float64)
    arrays = {}
    for i, (name, (B, H, W, h, w, mk, fn)) in enumerate(FLOW_CASES.items()):
        rng = np.random.default_rng(1000 + i)
        pred = flow(rng, (B, 2, h, w), 1.5).requires_grad_(True)
        gt = f32(dpo.upsample_flow_to(flow(rng, (B, 2, h, w), 1.5), H, W).numpy() + 0.3 * rng.standard_normal((B, 2, H, W)))
        mask = mask_of(rng, mk, B, H, W)
        if fn == "train":
            loss = train.MaskedCharbonnier()(dpo.upsample_flow_to(pred, H, W), gt, mask)
        elif fn == "train2":
            loss = train2.MaskedCharbonnier()(train2.upsample_flow_to(pred, H, W), gt, mask)
        else:
            loss = train2.compute_epe(train2.upsample_flow_to(pred, H, W), gt, mask)
        (g,) = torch.autograd.grad(loss, pred)
        arrays.update({name + "/pred": pred.detach().numpy().astype(np.float32), name + "/gt": gt.numpy().astype(np.float32),
                       name + "/loss": np.array([loss.item()]), name + "/grad": g.numpy()})
        if mask is not None:
            arrays[name + "/mask"] = mask.numpy().astype(np.float32)
        print("%-10s loss %.8f max|g| %.3e" % (name, loss.item(), g.abs().max()))
    for i, (name, (B, H, W, sizes, wl, lp, ls, mk)) in enumerate(MS_CASES.items()):
        rng = np.random.default_rng(2000 + i)
        preds = [flow(rng, (B, 2, h, w), 1.2 * (H / h) ** 0.25).requires_grad_(True) for h, w in sizes]
        gt = f32(3.0 * rng.standard_normal((B, 2, H, W)))
        images = image(rng, (B, 6, H, W))
        mask = mask_of(rng, mk, B, H, W)
        m_ref = mask[:, 0] if mask.dim() == 4 else mask           # train2 takes [B,H,W]
        loss = train2.supervised_multiscale_loss(preds, images, gt, m_ref, w=list(wl) if wl else None,
                                                 lambda_photo=lp, lambda_smooth=ls)
        grads = torch.autograd.grad(loss, preds)
        if lp > 0 or ls > 0:
            arrays[name + "/images"] = images.numpy().astype(np.float32)         # read only when a lambda is > 0
        arrays.update({name + "/gt": gt.numpy().astype(np.float32),
                       name + "/mask": mask.numpy().astype(np.float32), name + "/loss": np.array([loss.item()]),
                       name + "/cfg": np.array([lp, ls]), name + "/w": np.array(wl if wl else [], dtype=np.float64),
                       name + "/nlev": np.array([len(sizes)])})
        for k, (p, g) in enumerate(zip(preds, grads)):
            arrays["%s/pred%d" % (name, k)] = p.detach().numpy().astype(np.float32)
            arrays["%s/grad%d" % (name, k)] = g.numpy()
        print("%-10s loss %.8f max|g| %s" % (name, loss.item(), ["%.2e" % g.abs().max() for g in grads]))
    np.savez_compressed(out_path, **arrays)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g10_supervised_loss.npz"))
