"""Generate tests/golden/g12_kitti_score.npz from the REFERENCE's own KITTI scoring functions, in float64 on the CPU.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.
Recipe as tools/gen_golden_validation.py: process-local module stubs, no reference file is edited -- ``torchvision``,
``torchvision.transforms``, ``cv2`` and ``correlation_cuda`` become stub modules; so do ``tqdm`` / ``PIL`` when they are not installed.
The stub ``cv2.imread`` returns ``kitti.read_png16_rgb(path)[..., ::-1]`` (OpenCV's BGR order), so the reference's own
``load_flow_kitti_png`` decodes a PNG written by ``kitti.write_png16_rgb``.  Per case and sample the reference's ``unpad``,
``flow_resize``, ``epe_metric`` and ``fl_all_metric`` (inference_kitti.py) run on float64 inputs, and ``compute_epe`` / ``compute_fl``
(inference.py) beside them.  Stored: the quarter-resolution flow (float32), (crop_h, crop_w, out_h, out_w), the uint16 ground truth,
and per sample EPE and Fl-all from both scripts, the valid count and the outlier count.

Inputs: the quarter-resolution field is sinusoids of amplitude `amp` plus `noise` x N(0,1); the ground truth is the reference's own
float64 upsample plus an error vector of uniform length 0..6 px and uniform angle, quantised to 1/64 px by the PNG encoding, valid
on a seeded fraction of the pixels.  The generator ASSERTS the conditions the tests rely on: every sample with valid pixels has an
outlier fraction in [0.2, 0.8]; in at least two cases both threshold branches (3 px, 5 % of |gt|) are each active on >= 10 % of the
valid pixels; at most 1e-4 of a case's valid pixels lie within 1e-4 px of their threshold (the knife-edge band).  These are
properties of the inputs and of the float64 reference alone; when a seed violates one, change the seed.

    python tools/gen_golden_kitti_score.py [out.npz]
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_proxy_loss import REF, REPO, _stub  # noqa: E402

sys.path.insert(0, REPO)
from opticalflow_amd import kitti  # noqa: E402

KNIFE = 1e-4


def _import_reference():
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms")
    _stub("correlation_cuda")
    _stub("cv2", IMREAD_UNCHANGED=-1, imread=lambda path, flags=None: np.ascontiguousarray(kitti.read_png16_rgb(str(path))[..., ::-1]))
    for opt in ("tqdm", "PIL"):
        try:
            __import__(opt)
        except ImportError:
            _stub(opt, tqdm=lambda x, **k: x)
            if opt == "PIL":
                sys.modules["PIL"].Image = _stub("PIL.Image")
    for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[m]                 # the reference's scripts import their own `models` package
    sys.path.insert(0, REF)
    import inference_kitti as rk       # noqa: E402  (the reference's scripts)
    import inference as ri             # noqa: E402
    sys.path.remove(REF)
    return rk, ri


def field(shape, seed, amp, noise):
    g = np.random.default_rng(seed)
    n, _, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    f = noise * g.standard_normal(shape)
    for b in range(n):
        f[b, 0] += amp * np.sin(3 * xx + 2 * yy + g.uniform(0, 6))
        f[b, 1] += amp * np.cos(2 * xx - 3 * yy + g.uniform(0, 6))
    return f.astype(np.float32)


# name: (n, (Hq, Wq), (crop_h, crop_w), (out_h, out_w), amp, noise, validity per sample, seed)
#   a H x W image is padded to multiples of 64 and the network's output is a quarter of that; "pad-quarter" crops remove pad // 4,
#   the reference's `unpad` removes the full pad amounts from the quarter-resolution map (inference_kitti.py:66-71,220)
CASES = {
    "smooth": (1, (16, 32), (16, 24), (64, 96), 2.0, 0.0, (0.3,), 1200),
    "rough": (2, (16, 32), (16, 24), (64, 96), 18.0, 0.5, (0.3, 0.3), 1201),
    "odd": (1, (16, 48), (16, 33), (61, 131), 2.0, 0.5, (0.3,), 1202),                 # pad-quarter crop of a 61 x 131 image
    "ref_unpad": (1, (32, 48), (24, 36), (120, 180), 2.0, 0.5, (0.3,), 1203),          # the reference's crop of a 120 x 180 image
    "identity": (2, (32, 48), (24, 40), (24, 40), 22.0, 0.5, (0.3, 0.3), 1204),
    "sparse": (1, (16, 32), (16, 24), (64, 96), 2.0, 0.5, (0.2,), 1205),
    "empty": (3, (16, 32), (16, 24), (64, 96), 2.0, 0.5, (0.3, 0.0, 0.3), 1206),       # the middle sample has no valid pixel
    "all_valid": (1, (16, 32), (16, 24), (40, 56), 2.0, 0.5, (1.0,), 1207),
    "large": (1, (16, 32), (16, 24), (64, 96), 22.0, 0.5, (0.3,), 1208),               # 0.05 |gt| > 3 on about half of the pixels
}


def main(out_path):
    rk, ri = _import_reference()
    arrays, both_branches = {}, 0
    tmp = tempfile.mkdtemp()
    for name, (n, (Hq, Wq), (ch, cw), (H, W), amp, noise, validity, seed) in CASES.items():
        g = np.random.default_rng(seed)
        fq = field((n, 2, Hq, Wq), seed + 100, amp, noise)
        pred = rk.flow_resize(rk.unpad(torch.from_numpy(fq).double(), Hq - ch, Wq - cw).clone(), H, W).numpy()      # [n,2,H,W] float64
        assert pred.shape == (n, 2, H, W) and pred.dtype == np.float64
        gt16 = np.zeros((n, H, W, 3), np.uint16)
        rows = {k: [] for k in ("epe_k", "fl_k", "epe_i", "fl_i", "nv", "no", "knife", "rel")}
        for b in range(n):
            length, angle = g.uniform(0, 6, (H, W)), g.uniform(0, 2 * np.pi, (H, W))
            gt = pred[b].transpose(1, 2, 0) + np.stack([length * np.cos(angle), length * np.sin(angle)], axis=-1)
            valid = g.uniform(0, 1, (H, W)) < validity[b]
            enc = kitti.encode_flow_rgb16(np.round(gt * 64.0) / 64.0, valid)
            enc[~valid] = 0                                                         # like KITTI's own files: nothing where invalid
            gt16[b] = enc
            path = os.path.join(tmp, "%s_%d.png" % (name, b))
            kitti.write_png16_rgb(path, enc)
            flow_gt, valid_ref = rk.load_flow_kitti_png(path)                       # the reference's decoder on a real PNG
            assert flow_gt.dtype == np.float32 and np.array_equal(valid_ref, valid)
            fp, fg = pred[b].transpose(1, 2, 0), flow_gt.astype(np.float64)
            e_k, f_k = rk.epe_metric(fp, fg, valid_ref), rk.fl_all_metric(fp, fg, valid_ref)
            e_i, f_i = ri.compute_epe(fp, fg, valid_ref), ri.compute_fl(fp, fg, valid_ref)
            nv = int(np.count_nonzero(valid_ref))
            no = int(round(f_k * nv / 100.0)) if nv else 0
            d = fp - fg
            epe, mag = np.sqrt((d * d).sum(-1)), np.sqrt((fg * fg).sum(-1))
            thr = np.maximum(3.0, 0.05 * mag)
            assert no == int(np.count_nonzero((epe > thr) & valid_ref))
            for k, v in zip(rows, (e_k, f_k, e_i, f_i, nv, no, int(np.count_nonzero((np.abs(epe - thr) < KNIFE) & valid_ref)),
                                   int(np.count_nonzero((0.05 * mag > 3.0) & valid_ref)))):
                rows[k].append(v)
            if nv:
                assert 0.2 <= no / nv <= 0.8, (name, b, no / nv)
        nv_all = sum(rows["nv"])
        assert sum(rows["knife"]) <= 1e-4 * nv_all, (name, rows["knife"], nv_all)
        both_branches += 0.1 <= sum(rows["rel"]) / nv_all <= 0.9
        arrays[name + "/flow_q"] = fq
        arrays[name + "/geom"] = np.array([ch, cw, H, W], np.int64)
        arrays[name + "/gt"] = gt16
        arrays[name + "/epe"] = np.array([rows["epe_k"], rows["epe_i"]], np.float64)
        arrays[name + "/fl"] = np.array([rows["fl_k"], rows["fl_i"]], np.float64)
        arrays[name + "/n_valid"] = np.array(rows["nv"], np.int64)
        arrays[name + "/n_outlier"] = np.array(rows["no"], np.int64)
        print("%-10s epe %s fl %s valid %s outliers %s relative-branch %.2f knife-edge %d"
              % (name, np.round(rows["epe_k"], 4), np.round(rows["fl_k"], 2), rows["nv"], rows["no"], sum(rows["rel"]) / nv_all,
                 sum(rows["knife"])))
    assert both_branches >= 2, both_branches
    np.savez_compressed(out_path, **arrays)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g12_kitti_score.npz"))
