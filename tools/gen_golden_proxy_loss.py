"""Generate tests/golden/g8_proxy_loss.npz from the REFERENCE's own ProxyLabelLoss classes, in float64 on the CPU.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.
Recipe as oracle/gen_golden.py: process-local module stubs, no reference file is edited -- ``torchvision``,
``torchvision.transforms`` and ``correlation_cuda`` (imported at module level by train_pseudo.py / train_fundamental.py and
their models package, unused by the loss) become empty modules; so do ``tqdm`` / ``PIL`` when they are not installed.
Stored per case: the inputs, (total, photo, smooth) and the float64 autograd gradient of `total` w.r.t. the flow.

    python tools/gen_golden_proxy_loss.py [out.npz]
"""
import math
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
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms")
    _stub("correlation_cuda")
    for opt in ("tqdm", "PIL"):
        try:
            __import__(opt)
        except ImportError:
            _stub(opt, tqdm=lambda x, **k: x)
            if opt == "PIL":
                _stub("PIL.Image")
    sys.path.insert(0, REF)
    import train_pseudo as tp          # noqa: E402  (the reference's scripts)
    import train_fundamental as tf     # noqa: E402
    sys.path.remove(REF)
    return tp, tf


def image(shape, seed):
    """Structured test image in the normalised range [-2.1, 2.6]: seeded sinusoids plus a few step edges plus a little noise."""
    g = np.random.default_rng(seed)
    B, C, H, W = shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty(shape)
    for b in range(B):
        for c in range(C):
            v = np.zeros((H, W))
            for _ in range(3):
                fx, fy, ph = g.uniform(0.05, 0.6), g.uniform(0.05, 0.6), g.uniform(0, 2 * math.pi)
                v += g.uniform(0.3, 1.0) * np.sin(fx * xx + fy * yy + ph)
            for _ in range(2):
                a, bb, cc = g.normal(), g.normal(), g.uniform(-0.5, 0.5) * (H + W)
                v += g.uniform(0.5, 1.2) * (a * xx + bb * yy > cc)
            v += 0.1 * g.standard_normal((H, W))
            v = (v - v.min()) / max(v.max() - v.min(), 1e-9)
            out[b, c] = -2.1 + 4.7 * v
    return torch.from_numpy(out.astype(np.float32).astype(np.float64))      # float32-representable: the kernels' inputs


def flow(shape, seed, amp):
    g = np.random.default_rng(seed)
    B, _, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    f = amp * g.uniform(-1, 1, size=shape)
    f[:, 0] += amp * np.sin(3 * xx + 2 * yy)
    f[:, 1] += amp * np.cos(2 * xx - 3 * yy)
    return torch.from_numpy(f.astype(np.float32).astype(np.float64))


# name: (img shape, flow shape, variant, masked, amp, alpha_photo, alpha_smooth); the three "base" shapes share their images
# (stored once, as float32, under "base/"), which keeps the file under 1 MB
CASES = {
    "base_pseudo": ((2, 3, 64, 96), (2, 2, 16, 24), "pseudo", False, 2.0, 1.0, 0.1),
    "base_fund": ((2, 3, 64, 96), (2, 2, 16, 24), "fundamental", False, 2.0, 1.0, 0.1),
    "odd": ((1, 3, 37, 53), (1, 2, 10, 14), "pseudo", False, 1.5, 0.7, 0.3),
    "same": ((2, 3, 24, 40), (2, 2, 24, 40), "fundamental", False, 1.5, 1.0, 0.1),
    "clamp": ((1, 3, 32, 48), (1, 2, 8, 12), "pseudo", False, 25.0, 1.0, 0.1),
    "masked": ((2, 3, 64, 96), (2, 2, 16, 24), "fundamental", True, 2.0, 1.0, 0.1),
}


def main(out_path):
    tp, tf = _import_reference()
    torch.set_default_dtype(torch.float64)
    arrays = {}
    for i, (name, (ish, fsh, variant, masked, amp, ap, asm)) in enumerate(CASES.items()):
        shared = ish == CASES["base_pseudo"][0]
        img1, img2 = (image(ish, 100), image(ish, 101)) if shared else (image(ish, 100 + 2 * i), image(ish, 101 + 2 * i))
        fl = flow(fsh, 200 + i, amp).requires_grad_(True)
        mask = None
        if masked:
            rng = np.random.default_rng(300 + i)
            mask = torch.from_numpy(rng.uniform(0, 1, size=(ish[0], 1, ish[2], ish[3])).astype(np.float32).astype(np.float64))
        if variant == "pseudo":
            total, photo, smooth = tp.ProxyLabelLoss(ap, asm)(fl, img1, img2)
        else:
            total, photo, smooth = tf.ProxyLabelLoss(ap, asm)(fl, img1, img2, valid_mask=mask)
        (g,) = torch.autograd.grad(total, fl)
        ipfx = "base" if shared else name
        arrays.update({ipfx + "/img1": img1.numpy().astype(np.float32), ipfx + "/img2": img2.numpy().astype(np.float32),
                       name + "/flow": fl.detach().numpy().astype(np.float32),
                       name + "/loss": np.array([total.item(), photo.item(), smooth.item()]), name + "/grad_flow": g.numpy(),
                       name + "/cfg": np.array([ap, asm, 1.0 if variant == "fundamental" else 0.0])})
        if mask is not None:
            arrays[name + "/mask"] = mask.numpy().astype(np.float32)
        print("%-12s total %.6f photo %.6f smooth %.6f max|g| %.3e" % (name, total.item(), photo.item(), smooth.item(), g.abs().max()))
    # train_pseudo's forward-backward consistency warps a C = 2 flow field (train_pseudo.py:178-193)
    img = flow((2, 2, 32, 48), 400, 3.0)
    fl = flow((2, 2, 8, 12), 401, 1.5)
    arrays["warp2/img"], arrays["warp2/flow"] = img.numpy().astype(np.float32), fl.numpy().astype(np.float32)
    arrays["warp2/out"] = tp.ProxyLabelLoss().warp(img, fl.clone()).numpy()
    arrays["warp2/out_fund"] = tf.warp_image(img, fl.clone()).numpy()
    np.savez_compressed(out_path, **arrays)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g8_proxy_loss.npz"))
