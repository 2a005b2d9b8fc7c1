"""Generate tests/golden/g14_augment.npz from the REFERENCE's own KittiFlowDataset (data_processing_or.py).

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.  Recipe as
tools/gen_golden_flowviz.py: process-local stub modules, no reference file is edited or copied.  ``cv2`` is a stub whose ``warpAffine``
is tests/augment_oracle.warp_affine (cv2 is not installed; that restatement of OpenCV's classic fixed-point path is what the product's
kernel is defined by, and parity against a cv2 build is unpinned) and whose ``resize`` is harness.cv2_resize_linear (not reached: no
frame here is smaller than the crop).  ``read_kitti_flow_png`` is replaced IN THE IMPORTED MODULE'S NAMESPACE by
kitti.load_flow_kitti_png reshaped to its return form: under cv2's BGR channel order the reference's mask auto-detection assigns KITTI's
G channel to u, and this project decodes R -> u, G -> v as inference_kitti.py and KITTI define; the swap is not reproduced.

Tiny 8-bit frame PNGs and 16-bit flow PNGs are written into a temporary directory, and ``KittiFlowDataset.__getitem__`` is run on them
under ``random.seed(s)`` for the SEEDS below.  Stored: the inputs, the seeds, the parameters augment.sample_params draws under the same
seeds, and the three tensors the reference returned.  The generator ASSERTS that the oracle fed with the drawn parameters reproduces the
reference's tensors exactly (so the draws and the matrices are the reference's), that augment.affine_matrix and the oracle's equal the
reference's _cv2_affine_matrix on the extremes of the draw at the fixture's and at KITTI's sizes, and that skip, warp, flip and
warp + flip all occur (when a seed set violates the last, change it).

    python tools/gen_golden_augment.py [out.npz]
"""
import os
import random
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_proxy_loss import REF, REPO, _stub  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from opticalflow_amd import augment, harness, kitti  # noqa: E402
import augment_oracle as AO  # noqa: E402

SIZES = [(48, 80), (45, 77), (50, 72)]
CROP = (32, 64)
SEEDS = [0, 1, 2, 5]


def _warp_affine(src, M, dsize, dst=None, flags=1, borderMode=4, borderValue=0):
    assert flags == 1 and borderMode == 4
    src = np.ascontiguousarray(src)
    if src.ndim == 3 and src.shape[2] == 1:
        src = src[..., 0]                      # cv2 hands a one-channel [H,W,1] image back as [H,W]
    return AO.warp_affine(src, np.asarray(M), (dsize[1], dsize[0]))


def _resize(src, dsize, dst=None, fx=0, fy=0, interpolation=1):
    W, H = dsize
    return harness.cv2_resize_linear(torch.from_numpy(np.ascontiguousarray(src)), H, W).numpy()


def _import_reference():
    _stub("cv2", INTER_LINEAR=1, INTER_NEAREST=0, BORDER_REFLECT_101=4, IMREAD_UNCHANGED=-1, warpAffine=_warp_affine, resize=_resize,
          imread=lambda *a, **k: None)
    sys.path.insert(0, REF)
    try:
        import data_processing_or as dp        # noqa: E402  (the reference's module)
    finally:
        sys.path.remove(REF)

    def read_flow(path):
        flow, valid = kitti.load_flow_kitti_png(path)
        return flow, valid.astype(np.uint8)[..., None]
    dp.read_kitti_flow_png = read_flow
    return dp


def main(out_path):
    dp = _import_reference()
    from PIL import Image
    samples = [AO.make_sample(size, 1414 + i) for i, size in enumerate(SIZES)]
    arrays = {"seeds": np.array(SEEDS, np.int64), "crop": np.array(CROP, np.int64)}
    kinds = set()
    with tempfile.TemporaryDirectory() as tmp:
        lines = []
        for i, (im1, im2, png) in enumerate(samples):
            paths = [os.path.join(tmp, "%d_%s.png" % (i, k)) for k in ("a", "b", "flow")]
            Image.fromarray(im1).save(paths[0])
            Image.fromarray(im2).save(paths[1])
            kitti.write_png16_rgb(paths[2], png)
            assert np.array_equal(np.asarray(Image.open(paths[0]).convert("RGB")), im1)
            lines.append(" ".join(paths))
            arrays["im1/%d" % i], arrays["im2/%d" % i], arrays["png/%d" % i] = im1, im2, png
        list_txt = os.path.join(tmp, "list.txt")
        open(list_txt, "w").write("\n".join(lines) + "\n")
        ds = dp.KittiFlowDataset(tmp, list_txt=list_txt, crop_hw=CROP, apply_aug=True)
        plain = dp.KittiFlowDataset(tmp, list_txt=list_txt, crop_hw=CROP, apply_aug=False)
        for s in SEEDS + [-1]:
            random.seed(abs(s))
            ref = [(ds if s >= 0 else plain)[i] for i in range(len(samples))]
            random.seed(abs(s))
            params = augment.sample_params(SIZES, CROP, apply_aug=s >= 0)
            for i, ((x, flow, valid), p) in enumerate(zip(ref, params)):
                im1, im2, png = samples[i]
                u, v, m = AO.decode_png(png)
                rec = {k: p[k] for k in p.dtype.names}
                ox, of, ov = AO.augment(im1, im2, u, v, m, rec, CROP)
                for name, a, b in (("x", x, ox), ("flow", flow, of), ("valid", valid, ov)):
                    a = a.numpy()
                    assert a.dtype == np.float32 and a.shape == b.shape, (s, i, name, a.dtype, a.shape)
                    assert np.array_equal(a, b), (s, i, name, int((a != b).sum()))
                    arrays["%s/%d/%d" % (name, s, i)] = a
                kinds.add((int(p["warp"]), int(p["flip"])))
                print("seed %2d sample %d %s warp %d flip %d origin (%d, %d): the oracle equals the reference" %
                      (s, i, SIZES[i], p["warp"], p["flip"], p["y0"], p["x0"]))
            for k in params.dtype.names:
                arrays["params/%d/%s" % (s, k)] = params[k]
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}, kinds
    # the product's matrix against the reference's on the extremes of the draw and a few values inside
    for rot, sx, sy in [(2.0, 1.0815, 0.9215), (-2.0, 0.9215, 1.0815), (0.37, 1.013, 0.988), (-1.21, 0.97, 1.04), (75.0, 0.3, 0.3)]:
        for H, W in SIZES + [(375, 1242), (370, 1224)]:
            M, A = augment.affine_matrix((W * 0.5, H * 0.5), rot, sx, sy)
            Mr, Ar = dp._cv2_affine_matrix(center_xy=(W * 0.5, H * 0.5), rot_deg=rot, sx=sx, sy=sy)
            assert M.dtype == Mr.dtype == np.float32 and np.array_equal(M, Mr) and np.array_equal(A, Ar), (rot, sx, sy, H, W, M, Mr)
            Mo, Ao = AO.affine_matrix((W * 0.5, H * 0.5), rot, sx, sy)
            assert np.array_equal(M, Mo) and np.array_equal(A, Ao)
            assert np.array_equal(augment.invert_affine(M), AO.invert_affine(M))
    np.savez_compressed(out_path, **arrays)
    size = os.path.getsize(out_path)
    print("wrote %s (%d bytes)" % (out_path, size))
    assert size <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g14_augment.npz"))
