"""Generate tests/golden/g15_augment_full.npz from the REFERENCE's own KittiAugmentationPipeline (data_processing.py:136-279).

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.  Recipe as
tools/gen_golden_augment.py: process-local stub modules, no reference file is edited or copied.  ``albumentations`` and
``albumentations.pytorch`` are empty stubs (imported by the reference, not used by the pipeline).  ``cv2`` is a stub whose
``getRotationMatrix2D``, ``warpAffine`` and ``GaussianBlur`` are the restatements of tests/augment_full_oracle.py (cv2 is not installed;
those restatements of OpenCV's classic fixed-point warp and bit-exact 8U blur are what the product's kernel is defined by, and parity
against a cv2 build is unpinned).

``KittiAugmentationPipeline(CROP, augment=True / False)`` is run under ``np.random.seed(s)`` for the SEEDS below on three tiny samples of
different sizes, built as ``KittiDataset.__getitem__`` builds them (float32 [H,W,6] frames, float32 [2,H,W] flow, float32 [H,W] mask).
Stored: the inputs, the seeds, the records augment_full.sample_full_params draws under the same seeds, and the three tensors the
reference returned.  The generator ASSERTS that the oracle's whole-sample function fed with the drawn records reproduces the reference's
tensors exactly -- which pins the draw order, the float64 flow rotation with the aliased u, the float32 brightness map and the /255.0 --
that augment_full.rotation_matrix / gaussian_weights equal the oracle's, that each of the five stages occurs both on and off, and that
at least one sample has all five on (when a seed set violates the last two, change it).

    python tools/gen_golden_augment_full.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_proxy_loss import REF, REPO, _stub  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from opticalflow_amd import augment_full  # noqa: E402
import augment_full_oracle as FO  # noqa: E402

SIZES = [(48, 80), (45, 77), (50, 72)]
CROP = (32, 64)
SEEDS = [5, 25, 11, 20]
STAGES = ("flip", "rot", "trans", "bright", "blur")
BORDER_REFLECT = 2


def _warp_affine(src, M, dsize, dst=None, flags=1, borderMode=0, borderValue=0):
    assert flags == 1 and borderMode == BORDER_REFLECT
    src = np.ascontiguousarray(src)
    assert src.dtype == np.float32
    return FO.warp_affine(src, np.asarray(M), (dsize[1], dsize[0]))


def _gaussian_blur(src, ksize, sigmaX, dst=None, sigmaY=0, borderType=4):
    assert src.dtype == np.uint8 and sigmaY == 0 and borderType == 4
    k, w = FO.gaussian_weights(sigmaX)
    assert tuple(ksize) == (k, k), (ksize, k)
    return FO.gaussian_blur_u8(np.ascontiguousarray(src), w)


def _get_rotation_matrix(center, angle, scale):
    assert scale == 1.0
    return FO.rotation_matrix(center, angle)


def _import_reference():
    _stub("cv2", BORDER_REFLECT=BORDER_REFLECT, IMREAD_UNCHANGED=-1, IMREAD_COLOR=1, COLOR_BGR2RGB=4, getRotationMatrix2D=_get_rotation_matrix,
          warpAffine=_warp_affine, GaussianBlur=_gaussian_blur, imread=lambda *a, **k: None, cvtColor=lambda *a, **k: None)
    alb = _stub("albumentations")
    alb.pytorch = _stub("albumentations.pytorch", ToTensorV2=object)
    sys.path.insert(0, REF)
    try:
        import data_processing as dp           # noqa: E402  (the reference's module)
    finally:
        sys.path.remove(REF)
    return dp


def main(out_path):
    dp = _import_reference()
    samples = [FO.make_sample(size, 1515 + i) for i, size in enumerate(SIZES)]
    arrays = {"seeds": np.array(SEEDS, np.int64), "crop": np.array(CROP, np.int64)}
    decoded = []
    for i, (im1, im2, png) in enumerate(samples):
        arrays["im1/%d" % i], arrays["im2/%d" % i], arrays["png/%d" % i] = im1, im2, png
        decoded.append(FO.decode_png(png))
    on = {k: set() for k in STAGES}
    all_on = 0
    for s in SEEDS + [-1]:
        pipe = dp.KittiAugmentationPipeline(CROP, augment=s >= 0)
        np.random.seed(abs(s))
        ref = []
        for (im1, im2, _), (u, v, m) in zip(samples, decoded):
            # what KittiDataset.__getitem__ hands over (:119-133): float32 frames side by side, flow [2,H,W], mask [H,W]
            ref.append(pipe({"images": np.concatenate([im1.astype(np.float32), im2.astype(np.float32)], axis=2),
                             "flow": np.stack([u, v], axis=0).copy(), "mask": m.copy()}))
        np.random.seed(abs(s))
        params = augment_full.sample_full_params(SIZES, CROP, augment=s >= 0)
        for i, (out, p) in enumerate(zip(ref, params)):
            im1, im2, _ = samples[i]
            u, v, m = decoded[i]
            rec = {k: p[k] for k in p.dtype.names}
            ox, of, om = FO.augment_full((im1, im2, u, v, m), rec, CROP)
            for name, a, b in (("x", out["images"], ox), ("flow", out["flow"], of), ("mask", out["mask"][None], om)):
                a = a.numpy()
                assert a.dtype == np.float32 and a.shape == b.shape, (s, i, name, a.dtype, a.shape, b.shape)
                assert np.array_equal(a, b), (s, i, name, int((a != b).sum()))
                arrays["%s/%d/%d" % (name, s, i)] = a
            if s >= 0:
                for k in STAGES:
                    on[k].add(int(p[k]))
                all_on += all(int(p[k]) for k in STAGES)
            print("seed %2d sample %d %s origin (%d, %d) %s: the oracle equals the reference" %
                  (s, i, SIZES[i], p["y0"], p["x0"], " ".join("%s=%d" % (k, p[k]) for k in STAGES)))
        for k in params.dtype.names:
            arrays["params/%d/%s" % (s, k)] = params[k]
    assert all(v == {0, 1} for v in on.values()), on
    assert all_on >= 1, "no sample with all five stages on"
    # the product's host arithmetic against the oracle's over the range of the draws
    for angle in (-17.0, 17.0, 0.0, 3.3, -11.25):
        for ch, cw in (CROP, (320, 896), (5, 7)):
            assert np.array_equal(augment_full.rotation_matrix((cw // 2, ch // 2), angle), FO.rotation_matrix((cw // 2, ch // 2), angle))
    for sigma in np.linspace(0.5, 1.5, 101, endpoint=False).tolist() + [0.75, FO.SIG_ABOVE, 1.25]:
        (k, w), (ko, wo) = augment_full.gaussian_weights(sigma), FO.gaussian_weights(sigma)
        assert k == ko and np.array_equal(w, wo), sigma
    np.savez_compressed(out_path, **arrays)
    size = os.path.getsize(out_path)
    print("wrote %s (%d bytes)" % (out_path, size))
    assert size <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g15_augment_full.npz"))
