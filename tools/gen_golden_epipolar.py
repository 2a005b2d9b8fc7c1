"""Generate tests/golden/g9_epipolar.npz from the REFERENCE's own epipolar functions (train_fundamental.py:169-382), on the CPU.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.  Module
stubs as tools/gen_golden_proxy_loss.py (_import_reference).  Flows are not stored: they come from the seeded recipe
tests/epipolar_oracle.rigid_flow, pinned by the sha256 of their bytes.  Stored per case: that sha256, N, the sha256 of the
index table, F of the mask fit (thresh 0.5, 2000 iterations) and of the soft-loss fit (thresh 1.0, 1000), the best index and
all counts of both (counts recomputed with the reference's own _eight_point_F / _sampson_distance in _ransac_F's loop), the
packed mask of build_epipolar_mask_from_flow, its threshold, the soft-loss value and, at the small size, its float64 gradient.

    python tools/gen_golden_epipolar.py [out.npz]
"""
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from gen_golden_proxy_loss import _import_reference   # noqa: E402
import epipolar_oracle as O                          # noqa: E402

# name: (H, W, stride, seed, tau, keep_ratio, min_keep, nan patch, image mask points)
CASES = {
    "small": (96, 128, 4, 11, 1.0, 0.2, 0.05, False, None),
    "large": (384, 512, 6, 12, 1.0, 0.2, 0.05, False, None),
    "nan": (96, 128, 4, 13, 1.0, 0.2, 0.05, True, None),
    "fewpts": (96, 128, 4, 14, 1.0, 0.2, 0.05, False, 5),
    "minkeep": (96, 128, 4, 15, 1.0, 0.02, 0.05, False, None),   # keep_ratio < min_keep: the relaxation runs
}


def case_flow(name):
    H, W, stride, seed, tau, kr, mk, nan, mpts = CASES[name]
    fl = O.rigid_flow(H, W, seed)
    if nan:
        fl[:, 20:36, 40:72] = np.nan
    return fl


def case_mask(name):
    H, W, stride, seed, tau, kr, mk, nan, mpts = CASES[name]
    if mpts is None:
        return None
    m = np.zeros((H, W), bool)
    m[0, 0:mpts * stride:stride] = True
    return m


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def counts_of(tf, x1, x2, iters, thresh, seed=0):
    rng = np.random.default_rng(seed)
    N = x1.shape[0]
    out = np.zeros(iters, np.int32)
    if N < 8:
        return out
    for i in range(iters):
        idx = rng.choice(N, size=8, replace=False)
        out[i] = int((tf._sampson_distance(tf._eight_point_F(x1[idx], x2[idx]), x1, x2) < thresh).sum())
    return out


def main(out_path):
    _, tf = _import_reference()
    arrays = {}
    for name, (H, W, stride, seed, tau, kr, mk, nan, mpts) in CASES.items():
        fl = case_flow(name)
        m = case_mask(name)
        hw2 = np.ascontiguousarray(fl.transpose(1, 2, 0))
        x1, x2 = tf._flow_to_pairs(hw2, stride=stride, mask_hw=m)
        N = x1.shape[0]
        arrays[name + "/flow_sha"] = sha(fl)
        arrays[name + "/cfg"] = np.array([H, W, stride, seed, tau, kr, mk, N], np.float64)
        for tag, iters, thresh in (("fit", 2000, 0.5), ("soft", 1000, 1.0)):
            try:
                F = tf._ransac_F(x1, x2, max_iters=iters, thresh=thresh, seed=0)
                ok = True
            except RuntimeError:
                F, ok = np.zeros((3, 3)), False
            c = counts_of(tf, x1, x2, iters, thresh)
            arrays[name + "/%s_F" % tag], arrays[name + "/%s_ok" % tag] = F, np.array(ok)
            arrays[name + "/%s_counts" % tag] = c.astype(np.int16 if c.max() < 32767 else np.int32)
            arrays[name + "/%s_best" % tag] = np.array(int(np.argmax(c)) if N >= 8 else -1)
        if N >= 8:
            arrays[name + "/idx_sha"] = sha(O.index_table(N, 0, 2000))
        ft = torch.from_numpy(fl).unsqueeze(0)
        mt = None if m is None else torch.from_numpy(m).unsqueeze(0)
        mask = tf.build_epipolar_mask_from_flow(ft, tau=tau, stride=stride, img_mask_bhw=mt, keep_ratio=kr, min_keep=mk)
        mask = mask[0, 0].numpy()
        arrays[name + "/mask"] = np.packbits(mask.ravel())
        thr = np.nan
        if arrays[name + "/fit_ok"]:
            d = tf._sampson_distance(arrays[name + "/fit_F"], *[np.stack([a.ravel(), b.ravel(), np.ones(H * W)], 1) for a, b in (
                (np.mgrid[0:H, 0:W][1].astype(np.float64), np.mgrid[0:H, 0:W][0].astype(np.float64)),
                ((np.mgrid[0:H, 0:W][1] + hw2[..., 0]).astype(np.float64), (np.mgrid[0:H, 0:W][0] + hw2[..., 1]).astype(np.float64)))])
            d = d.reshape(H, W)
            fin = np.isfinite(d)
            if fin.any():
                thr = float(tau)
                if 0 < kr < 1:
                    thr = min(thr, float(np.quantile(d[fin], kr)))
                if 0 < mk < 1 and (fin & (d <= thr)).mean() < mk:
                    thr = min(float(tau), float(np.quantile(d[fin], mk)))
                assert np.array_equal(fin & (d <= thr), mask)
        arrays[name + "/thr"] = np.array(thr)
        if arrays[name + "/soft_ok"]:
            Fs = arrays[name + "/soft_F"]
            vm = torch.from_numpy(mask).view(1, 1, H, W)
            arrays[name + "/soft_loss"] = np.array(float(tf.epipolar_sampson_loss(ft, Fs, valid_mask=vm, weight=0.1)))
            if name == "small":
                f64 = torch.from_numpy(fl.astype(np.float64)).unsqueeze(0).requires_grad_(True)
                l64 = tf.epipolar_sampson_loss(f64, Fs, valid_mask=vm, weight=0.1)
                (g,) = torch.autograd.grad(l64, f64)
                arrays[name + "/soft_loss64"] = np.array(float(l64.detach()))
                arrays[name + "/soft_grad64"] = g[0].numpy()
        print("%-8s N %5d fit ok %d best %4d count %5d  soft ok %d  keep %.4f thr %.6g" % (
            name, N, arrays[name + "/fit_ok"], arrays[name + "/fit_best"], arrays[name + "/fit_counts"].max() if N >= 8 else 0,
            arrays[name + "/soft_ok"], mask.mean(), thr))
    np.savez_compressed(out_path, **arrays)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g9_epipolar.npz"))
