"""KITTI training augmentation without a GPU: the NumPy oracle (tests/augment_oracle.py) against the tensors the reference's own
KittiFlowDataset returned (tests/golden/g14_augment.npz, written by tools/gen_golden_augment.py behind a stub cv2 whose warpAffine is
the oracle's), the host side of opticalflow_amd.augment, the C ABI addition and the argument checks.  Everything compares exactly.
In the fixture the key -1 stands for `apply_aug=False` under random.seed(1)."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import augment_oracle as AO  # noqa: E402

N_SAMPLES = 3


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "g14_augment.npz")) as z:
        return {k: z[k] for k in z.files}


def runs(gold):
    return [int(s) for s in gold["seeds"]] + [-1]


def test_fixture_fits_and_covers_every_branch(gold):
    assert os.path.getsize(os.path.join(HERE, "golden", "g14_augment.npz")) <= 1 << 20
    kinds = set()
    for s in runs(gold):
        kinds |= set(zip(gold["params/%d/warp" % s].tolist(), gold["params/%d/flip" % s].tolist()))
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}
    sizes = {gold["im1/%d" % i].shape[:2] for i in range(N_SAMPLES)}
    assert len(sizes) == N_SAMPLES                     # three different (H, W)
    assert (gold["params/-1/warp"] == 0).all() and (gold["params/-1/flip"] == 0).all()


def test_identity_matrix_returns_the_source_bit_for_bit():
    g = np.random.default_rng(3)
    M = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    for shape in ((7, 9), (1, 5), (6, 1)):
        u8 = g.integers(0, 256, shape + (3,)).astype(np.uint8)
        fl = (g.standard_normal(shape) * 50).astype(np.float32)
        assert np.array_equal(AO.warp_affine(u8, M, shape), u8)
        assert np.array_equal(AO.warp_affine(u8[..., 0].copy(), M, shape), u8[..., 0])
        assert np.array_equal(AO.warp_affine(fl, M, shape).view(np.uint32), fl.view(np.uint32))


def test_sample_params_draws_what_the_reference_draws(gold):
    from opticalflow_amd import augment
    sizes = [gold["im1/%d" % i].shape[:2] for i in range(N_SAMPLES)]
    crop = tuple(int(v) for v in gold["crop"])
    for s in runs(gold):
        random.seed(abs(s))
        p = augment.sample_params(sizes, crop, apply_aug=s >= 0)
        assert p.dtype == augment.PARAMS_DTYPE and p.dtype.itemsize == 88
        for k in p.dtype.names:
            want = gold["params/%d/%s" % (s, k)]
            assert p[k].dtype == want.dtype and np.array_equal(p[k], want), (s, k)
        # a random.Random instance draws the same as the module after the same seed
        q = augment.sample_params(sizes, crop, apply_aug=s >= 0, rng=random.Random(abs(s)))
        assert q.tobytes() == p.tobytes()
    with pytest.raises(ValueError):
        augment.sample_params([(31, 80)], crop)          # the upsize branch is not provided
    with pytest.raises(ValueError):
        augment.sample_params([(48, 63)], crop)


def test_oracle_reproduces_the_references_tensors(gold):
    crop = tuple(int(v) for v in gold["crop"])
    for s in runs(gold):
        for i in range(N_SAMPLES):
            rec = {k: gold["params/%d/%s" % (s, k)][i] for k in ("m", "a", "y0", "x0", "h", "w", "warp", "flip")}
            u, v, m = AO.decode_png(gold["png/%d" % i])
            x, flow, valid = AO.augment(gold["im1/%d" % i], gold["im2/%d" % i], u, v, m, rec, crop)
            assert np.array_equal(x, gold["x/%d/%d" % (s, i)])
            assert np.array_equal(flow, gold["flow/%d/%d" % (s, i)])
            assert np.array_equal(valid, gold["valid/%d/%d" % (s, i)])
            rows = [0, 5, crop[0] - 1]
            xr, fr, vr = AO.augment(gold["im1/%d" % i], gold["im2/%d" % i], u, v, m, rec, crop, rows=rows)
            assert np.array_equal(xr, x[:, rows]) and np.array_equal(fr, flow[:, rows]) and np.array_equal(vr, valid[:, rows])


def test_invert_affine_on_hand_computed_matrices():
    from opticalflow_amd import augment
    for inv in (AO.invert_affine, augment.invert_affine):
        assert np.array_equal(inv(np.array([[1, 0, 0], [0, 1, 0]], np.float32)), [1, 0, 0, 0, 1, 0])
        # pure translation by (3, -5): the inverse translates back
        assert np.array_equal(inv(np.array([[1, 0, 3], [0, 1, -5]], np.float32)), [1, 0, -3, 0, 1, 5])
        # scale (2, 4) and translation (6, 8): x = (x' - 6) / 2, y = (y' - 8) / 4
        assert np.array_equal(inv(np.array([[2, 0, 6], [0, 4, 8]], np.float32)), [0.5, 0, -3, 0, 0.25, -2])
        # rotation by 90 degrees [[0, -1], [1, 0]] with translation (1, 2): inverse [[0, 1], [-1, 0]], b = (-2, 1)
        assert np.array_equal(inv(np.array([[0, -1, 1], [1, 0, 2]], np.float32)), [0, 1, -2, -1, 0, 1])
        # singular: D = 0 stays 0 as in cv::warpAffine
        assert np.array_equal(inv(np.array([[1, 2, 3], [2, 4, 5]], np.float32)), [0, 0, 0, 0, 0, 0])


def test_affine_matrix_product_and_oracle_agree():
    from opticalflow_amd import augment
    for rot, sx, sy in [(2.0, 1.0815, 0.9215), (-2.0, 0.9215, 1.0815), (0.37, 1.013, 0.988), (75.0, 0.3, 0.3), (0.0, 1.0, 1.0)]:
        for H, W in [(48, 80), (375, 1242), (9, 13)]:
            M, A = augment.affine_matrix((W * 0.5, H * 0.5), rot, sx, sy)
            Mo, Ao = AO.affine_matrix((W * 0.5, H * 0.5), rot, sx, sy)
            assert M.dtype == np.float32 and M.shape == (2, 3) and A.shape == (2, 2)
            assert np.array_equal(M, Mo) and np.array_equal(A, Ao) and np.array_equal(M[:, :2], A)
            assert np.array_equal(augment.invert_affine(M), AO.invert_affine(M))
    M, _ = augment.affine_matrix((40.0, 24.0), 0.0, 1.0, 1.0)
    assert np.array_equal(M, [[1, 0, 0], [0, 1, 0]])


def test_reflect101_index_table():
    assert AO.reflect101(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert AO.reflect101(np.arange(-5, 6), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert AO.reflect101(np.arange(-12, 13), 5).tolist() == [4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4]
    assert int(AO.reflect101(5, 5)) == 3 and int(AO.reflect101(-1, 5)) == 1 and int(AO.reflect101(8, 5)) == 0


def test_valid_at_exactly_one_half_is_not_valid():
    # a half-pixel shift between a valid and an invalid column gives 0.5 exactly
    valid = np.array([[1, 0, 1, 1]], np.float32)
    M = np.array([[1, 0, 0.5], [0, 1, 0]], np.float32)
    w = AO.warp_affine(valid, M, (1, 4))
    assert w.tolist() == [[0.5, 0.5, 0.5, 1.0]] and ((w > 0.5) == [[False, False, False, True]]).all()


def test_new_symbol_declared_exported_bound_and_abi_13():
    from opticalflow_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pwc_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bpwc_kitti_augment\s*\(", text) and re.search(r"\bpwc_augment_params\b", text)
    assert "pwc_kitti_augment" in _lib.SIGNATURES and hasattr(lib, "pwc_kitti_augment")
    assert _lib.ABI_VERSION == 13 and _lib.load().pwc_abi_version() == 13
    assert re.search(r"#define PWC_ABI_VERSION 13\b", text)


def test_c_argument_checks_launch_nothing():
    from opticalflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(frames=p, gt=p, kind=0, valid=None, n=1, Hs=8, Ws=8, ch=4, cw=4, params=p, x=p, flow=p, vout=p, status=p):
        return lib.pwc_kitti_augment(frames, gt, kind, valid, n, Hs, Ws, ch, cw, params, x, flow, vout, status, None)
    # every call below fails its checks, which come before anything touches a device
    for kw in (dict(frames=None), dict(gt=None), dict(params=None), dict(x=None), dict(flow=None), dict(vout=None), dict(status=None),
               dict(n=0), dict(Hs=0), dict(Ws=-1), dict(ch=0), dict(cw=0), dict(n=65536), dict(Hs=32768), dict(Ws=32768),
               dict(ch=9), dict(cw=9), dict(kind=2), dict(kind=-1), dict(kind=1, valid=p)):
        assert call(**kw) == -1, kw
    assert b"pwc_kitti_augment" in lib.pwc_last_error()
    for kw in (dict(x=p + 2), dict(flow=p + 1), dict(vout=p + 2), dict(status=p + 2), dict(gt=p + 2), dict(kind=1, gt=p + 1),
               dict(params=p + 4)):
        assert call(**kw) == -3, kw


def test_wrapper_argument_errors_raise_without_a_device():
    from opticalflow_amd import PwcHipError, augment, ops
    frames = torch.zeros(2, 2, 8, 12, 3, dtype=torch.uint8)
    gt = torch.zeros(2, 8, 12, 3, dtype=torch.uint16)
    params = augment.make_params(2)
    params["h"], params["w"] = 8, 12
    dev_params = torch.zeros(2, 88, dtype=torch.uint8)
    with pytest.raises(PwcHipError):
        augment.augment_batch(frames, gt, None, params, (4, 8))
    with pytest.raises(PwcHipError):
        ops.kitti_augment(frames, gt, dev_params, (4, 8))
    with pytest.raises(PwcHipError):
        augment.DeviceAugmenter("cpu", 2, (8, 12), (4, 8))
    with pytest.raises(ValueError):
        ops.kitti_augment(frames[:, :, :, :, :2], gt, dev_params, (4, 8))
    with pytest.raises(ValueError):
        ops.kitti_augment(frames.float(), gt, dev_params, (4, 8))
    # the host-side record checks of augment_batch (they repeat the kernel's)
    for field, value in (("h", 9), ("w", 13), ("h", 3), ("w", 7), ("y0", 5), ("x0", 5), ("y0", -1), ("x0", -1), ("h", 0)):
        bad = params.copy()
        bad[field][1] = value
        with pytest.raises(ValueError):
            augment.check_params(bad, 2, (8, 12), (4, 8))
    assert augment.check_params(params, 2, (8, 12), (4, 8)).tobytes() == params.tobytes()
    with pytest.raises(ValueError):
        augment.check_params(params, 3, (8, 12), (4, 8))
    with pytest.raises(ValueError):
        augment.check_params(np.zeros((2, 88), np.uint8), 2, (8, 12), (4, 8))


def test_pack_slots_keeps_each_samples_own_row_stride():
    from opticalflow_amd import augment
    samples = [AO.make_sample((5, 7), 1), AO.make_sample((6, 4), 2)]
    frames, gt, valid, sizes = augment.pack_slots(samples, (6, 7), 1)
    assert valid is None and sizes == [(5, 7), (6, 4)] and frames.shape == (2, 2, 6, 7, 3) and gt.shape == (2, 6, 7, 3)
    for b, (im1, im2, png) in enumerate(samples):
        H, W = im1.shape[:2]
        assert np.array_equal(frames[b, 0].reshape(-1)[:H * W * 3].reshape(H, W, 3), im1)
        assert np.array_equal(frames[b, 1].reshape(-1)[:H * W * 3].reshape(H, W, 3), im2)
        assert np.array_equal(gt[b].reshape(-1)[:H * W * 3].reshape(H, W, 3), png)
    fl = [(a, b, np.stack(AO.decode_png(p)[:2], -1), p[..., 2]) for a, b, p in samples]
    _, g0, v0, _ = augment.pack_slots(fl, (6, 7), 0)
    assert g0.shape == (2, 2, 6, 7) and v0.shape == (2, 6, 7) and v0.dtype == np.uint8
    assert np.array_equal(g0[1, 1].reshape(-1)[:24].reshape(6, 4), fl[1][2][..., 1])
    assert np.array_equal(v0[1].reshape(-1)[:24].reshape(6, 4), samples[1][2][..., 2] != 0)
    with pytest.raises(ValueError):
        augment.pack_slots(samples, (5, 7), 1)           # the second sample is 6 rows high


def test_case_table_covers_what_the_gpu_tests_rely_on():
    crop, items = AO.CASES["mixed"]
    assert len(items) == 5 and len({size for size, _ in items}) >= 3
    kinds = {("warp" in kw, bool(kw.get("flip"))) for _, kw in items}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert AO.CASES["skip_flip"][0][1] % 4 != 0 and all("warp" not in kw for _, kw in AO.CASES["skip_flip"][1])
    # the corner origins of the extremes case
    crop, items = AO.CASES["extremes"]
    origins = {(kw.get("y0", 0), kw.get("x0", 0)) for _, kw in items}
    assert origins == {(0, 0), (items[0][0][0] - crop[0], items[0][0][1] - crop[1])}
    # the far case: the unreflected source positions of the window's corners leave the 9 x 13 source by more than one period
    _, recs, crop, _ = AO.case_inputs("far")
    m, (y0, x0) = recs[0]["m"], (recs[0]["y0"], recs[0]["x0"])
    xs = [m[0] * X + m[1] * Y + m[2] for Y in (y0, y0 + crop[0] - 1) for X in (x0, x0 + crop[1] - 1)]
    ys = [m[3] * X + m[4] * Y + m[5] for Y in (y0, y0 + crop[0] - 1) for X in (x0, x0 + crop[1] - 1)]
    assert max(xs) - 12 > 24 or min(xs) < -24 or max(ys) - 8 > 16 or min(ys) < -16
    for name in AO.CASES:
        samples, recs, crop, slot = AO.case_inputs(name)
        x, flow, valid = AO.case_expected(samples, recs, crop)
        assert x.shape == (len(recs), 6) + crop and 0 < valid.mean() < 1 and x.min() >= 0 and x.max() <= 1
