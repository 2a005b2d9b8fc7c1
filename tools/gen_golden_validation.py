"""Generate tests/golden/g11_validation.npz from the REFERENCE's own validation functions, in float64 on the CPU.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.
Recipe as tools/gen_golden_proxy_loss.py: process-local module stubs, no reference file is edited -- ``torchvision``,
``torchvision.transforms`` and ``correlation_cuda`` become empty modules; so do ``tqdm`` / ``PIL`` when they are not installed.
Per case the reference's own ``_upsample_flow_to`` / ``upsample_flow_to``, ``ProxyLabelLoss.warp`` / ``warp_image``, the cycle
expression ``(flow12 + warp(flow21, flow12)).abs().mean()`` and ``_oob_ratio`` / ``oob_ratio`` run on float64 tensors.  Stored:
the two flows (float32), (H, W), the cycle, the out-of-bounds ratio and the count it stands for, from both scripts' functions
(they agree; the fixture keeps both so the tests can say so).

    python tools/gen_golden_validation.py [out.npz]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_proxy_loss import REPO, _import_reference  # noqa: E402


def field(shape, seed, amp, noise):
    """Seeded sinusoids of amplitude `amp` plus `noise` x standard normal, float32-representable."""
    g = np.random.default_rng(seed)
    B, _, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    f = noise * g.standard_normal(shape)
    f[:, 0] += amp * np.sin(3 * xx + 2 * yy + g.uniform(0, 6))
    f[:, 1] += amp * np.cos(2 * xx - 3 * yy + g.uniform(0, 6))
    return f.astype(np.float32)


# name: (B, H, W, h, w, kind, amp, noise)
CASES = {
    "smooth": (2, 64, 96, 16, 24, "pair", 2.0, 0.0),
    "rough": (2, 64, 96, 16, 24, "pair", 1.5, 1.0),
    "odd": (1, 37, 53, 10, 14, "pair", 1.5, 0.5),
    "same": (2, 24, 40, 24, 40, "pair", 3.0, 1.0),
    "zero": (2, 32, 48, 8, 12, "zero", 0.0, 0.0),
    "const_neg": (1, 32, 48, 8, 12, "const_neg", 0.0, 0.0),
    "clamp": (1, 32, 48, 8, 12, "pair", 25.0, 5.0),
    "oob_only": (2, 40, 56, 10, 14, "oob_only", 4.0, 1.0),
}


def flows(name, i):
    B, H, W, h, w, kind, amp, noise = CASES[name]
    shape = (B, 2, h, w)
    if kind == "zero":
        return np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    if kind == "const_neg":
        f = np.empty(shape, np.float32)
        f[:, 0], f[:, 1] = 1.75, -0.625
        return f, -f
    f12 = field(shape, 500 + 2 * i, amp, noise)
    if kind == "oob_only":
        return f12, None
    # a backward flow that roughly undoes the forward one, plus its own structure: the cycle is small but not zero
    return f12, (-f12 + field(shape, 501 + 2 * i, 0.3 * max(amp, 1.0), 0.3 * noise)).astype(np.float32)


def main(out_path):
    tp, tf = _import_reference()
    torch.set_default_dtype(torch.float64)
    crit = tp.ProxyLabelLoss()
    arrays = {}
    for i, name in enumerate(CASES):
        B, H, W, h, w = CASES[name][:5]
        f12, f21 = flows(name, i)
        arrays[name + "/flow12"] = f12
        arrays[name + "/size"] = np.array([H, W], np.int64)
        t12 = torch.from_numpy(f12).double()
        up12_p, up12_f = tp._upsample_flow_to(t12.clone(), H, W), tf.upsample_flow_to(t12.clone(), H, W)
        oob_p = tp._oob_ratio(up12_p.clone(), H, W, device=torch.device("cpu"), dtype=torch.float64)
        oob_f = tf.oob_ratio(t12.clone(), H, W, device=torch.device("cpu"), dtype=torch.float64)
        # the scripts return oob.float().mean(): the count is taken from the same boolean expression's mean in float64
        cnt = [int(round(float(v.double()) * B * H * W)) for v in (oob_p, oob_f)]
        cyc = [0.0, 0.0]
        if f21 is not None:
            arrays[name + "/flow21"] = f21
            t21 = torch.from_numpy(f21).double()
            up21_p, up21_f = tp._upsample_flow_to(t21.clone(), H, W), tf.upsample_flow_to(t21.clone(), H, W)
            cyc[0] = float((up12_p + crit.warp(up21_p, up12_p)).abs().mean())
            cyc[1] = float((up12_f + tf.warp_image(up21_f, up12_f)).abs().mean())
        arrays[name + "/cycle"] = np.array(cyc, np.float64)
        arrays[name + "/oob"] = np.array([float(oob_p), float(oob_f)], np.float64)
        arrays[name + "/oob_count"] = np.array(cnt, np.int64)
        print("%-10s cycle %.9f / %.9f  oob %.6f / %.6f  count %d / %d of %d" % (name, cyc[0], cyc[1], float(oob_p), float(oob_f),
                                                                               cnt[0], cnt[1], B * H * W))
    np.savez_compressed(out_path, **arrays)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g11_validation.npz"))
