"""CPU checks of train2.py's augmentation on the device (opticalflow_amd/augment_full.py, pwc_kitti_augment_full): the NumPy oracle
against the fixture made from the reference's own KittiAugmentationPipeline, the host-side parameters, the symbol and the argument
errors that come back without a device.  The kernel itself is checked in tests/test_gpu_augment_full.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_full_oracle as FO  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(48, 80), (45, 77), (50, 72)]
STAGES = ("flip", "rot", "trans", "bright", "blur")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(REPO, "tests", "golden", "g15_augment_full.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_samples(gold):
    return [(gold["im1/%d" % i], gold["im2/%d" % i], gold["png/%d" % i]) for i in range(3)]


def test_oracle_equals_the_reference_fixture(gold):
    samples = fixture_samples(gold)
    assert [s[0].shape[:2] for s in samples] == SIZES
    crop = tuple(int(v) for v in gold["crop"])
    on = {k: set() for k in STAGES}
    all_on = 0
    for s in [int(v) for v in gold["seeds"]] + [-1]:
        for i, (im1, im2, png) in enumerate(samples):
            rec = {k: gold["params/%d/%s" % (s, k)][i] for k in ("m", "cs", "gain", "wk", "ksize", "y0", "x0", "h", "w", "tx", "ty") + STAGES}
            u, v, m = FO.decode_png(png)
            got = FO.augment_full((im1, im2, u, v, m), rec, crop)
            for name, g in zip(("x", "flow", "mask"), got):
                assert np.array_equal(g, gold["%s/%d/%d" % (name, s, i)]), (s, i, name)
            if s >= 0:
                for k in STAGES:
                    on[k].add(int(rec[k]))
                all_on += all(int(rec[k]) for k in STAGES)
            else:
                assert not any(int(rec[k]) for k in STAGES)
    assert all(v == {0, 1} for v in on.values()) and all_on >= 1
    # a rotated mask is fractional: the reference does not threshold it again
    frac = [gold[k] for k in gold if k.startswith("mask/")]
    assert any(((f > 0) & (f < 1)).any() for f in frac)


def test_sample_full_params_reproduces_the_fixtures_records(gold):
    from opticalflow_amd import augment_full
    crop = tuple(int(v) for v in gold["crop"])
    for s in [int(v) for v in gold["seeds"]] + [-1]:
        np.random.seed(abs(s))
        p = augment_full.sample_full_params(SIZES, crop, augment=s >= 0)
        rs = np.random.RandomState(abs(s))
        q = augment_full.sample_full_params(SIZES, crop, augment=s >= 0, rng=rs)
        assert p.tobytes() == q.tobytes()
        for k in p.dtype.names:
            assert np.array_equal(p[k], gold["params/%d/%s" % (s, k)]) and p[k].dtype == gold["params/%d/%s" % (s, k)].dtype, (s, k)
    # both origins are drawn even when the range is a single value
    np.random.seed(7)
    a = augment_full.sample_full_params([(32, 64)], (32, 64))
    np.random.seed(7)
    np.random.randint(0, 1), np.random.randint(0, 1)
    assert int(a["flip"][0]) == int(np.random.rand() < 0.5) and a["y0"][0] == 0 and a["x0"][0] == 0
    with pytest.raises(ValueError):
        augment_full.sample_full_params([(31, 64)], (32, 64))
    with pytest.raises(ValueError):
        augment_full.sample_full_params([(32, 63)], (32, 64))


def test_gaussian_weights_known_answers_and_tap_count_switches():
    from opticalflow_amd import augment_full
    known = {0.5: [27, 202, 27], 0.75: [58, 140, 58], 1.0: [14, 62, 104, 62, 14], 1.25: [24, 61, 86, 61, 24],
             1.5: [9, 29, 55, 70, 55, 29, 9]}
    for mod in (augment_full, FO):
        for sigma, want in known.items():
            k, w = mod.gaussian_weights(sigma)
            assert k == len(want) and w.dtype == np.uint16 and w.tolist() == want, (mod.__name__, sigma, w)
        assert mod.gaussian_weights(0.75)[0] == 3 and mod.gaussian_weights(float(np.nextafter(0.75, 1.0)))[0] == 5
        assert mod.gaussian_weights(1.25)[0] == 5 and mod.gaussian_weights(float(np.nextafter(1.25, 2.0)))[0] == 7
    for sigma in np.linspace(0.5, 1.5, 41, endpoint=False):
        (k, w), (ko, wo) = augment_full.gaussian_weights(sigma), FO.gaussian_weights(sigma)
        assert k == ko and np.array_equal(w, wo) and int(w.astype(np.int64).sum()) == 256 and np.array_equal(w, w[::-1])
    with pytest.raises(ValueError):
        augment_full.gaussian_weights(2.0)


def test_rotation_matrix_identity_and_angle_zero_is_exact():
    from opticalflow_amd import augment, augment_full
    for mod in (augment_full, FO):
        M = mod.rotation_matrix((32, 16), 0)
        assert M.dtype == np.float64 and np.array_equal(M, [[1, 0, 0], [0, 1, 0]])
    for angle in (-17.0, 17.0, 3.3):
        assert np.array_equal(augment_full.rotation_matrix((32, 16), angle), FO.rotation_matrix((32, 16), angle))
        # a rotation keeps its centre
        M = augment_full.rotation_matrix((32, 16), angle)
        assert np.allclose(M @ [32, 16, 1], [32, 16], atol=1e-12)
    rec = augment_full.make_full_params(1)[0]
    augment_full.set_rotation(rec, (32, 64), 0.0)
    assert rec["rot"] == 1 and np.array_equal(rec["m"], [1, 0, 0, 0, 1, 0]) and np.array_equal(rec["cs"], [1, 0])
    src = np.random.default_rng(1).normal(size=(9, 13, 3)).astype(np.float32)
    out = FO.warp_affine(src, FO.rotation_matrix((6, 4), 0.0), (9, 13))
    assert out.tobytes() == np.where(src == 0, np.float32(0), src).tobytes()
    # ... and through the whole-sample function: rot=0.0 equals no rotation
    samples, _, crop, _ = FO.case_inputs("extremes")
    im1, im2, png = samples[2]
    u, v, m = FO.decode_png(png)
    a = FO.augment_full((im1, im2, u, v, m), FO.record((48, 80), crop, y0=4, x0=4, rot=0.0), crop)
    b = FO.augment_full((im1, im2, u, v, m), FO.record((48, 80), crop, y0=4, x0=4), crop)
    assert all(np.array_equal(s, t) for s, t in zip(a, b))
    assert np.array_equal(augment.invert_affine(M), FO.invert_affine(M))


def test_integer_translation_through_the_generic_warp_is_the_reflected_gather():
    src = np.random.default_rng(2).normal(size=(5, 7, 2)).astype(np.float32)
    for tx, ty in ((10, -10), (-10, 10), (3, 0), (0, -4), (-7, -5), (10, 10)):
        out = FO.warp_affine(src, np.float32([[1, 0, tx], [0, 1, ty]]), (5, 7))
        ys, xs = FO.reflect(np.arange(5) - ty, 5), FO.reflect(np.arange(7) - tx, 7)
        assert np.array_equal(out, src[ys][:, xs]), (tx, ty)
    assert FO.reflect(np.arange(-7, 8), 3).tolist() == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert FO.reflect(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert FO.reflect101(np.arange(-5, 6), 3).tolist() == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]


def test_gaussian_blur_u8_properties():
    g = np.random.default_rng(3)
    flat = np.full((6, 9, 3), 201, np.uint8)
    for sigma in (0.5, 1.0, 1.5):
        k, w = FO.gaussian_weights(sigma)
        assert np.array_equal(FO.gaussian_blur_u8(flat, w), flat)                  # the weights add up to exactly 256
        src = g.integers(0, 256, (1, 9), dtype=np.uint8)                            # one row: reflect101 with len == 1
        rowwise = FO.gaussian_blur_u8(src, w)
        xs = FO.reflect101(np.arange(-(k // 2), 9 + k // 2), 9)
        h = sum(int(w[i]) * src[0, xs[i:i + 9]].astype(np.int64) for i in range(k))
        assert np.array_equal(rowwise[0], (h * 256 + 32768) >> 16)
    assert np.array_equal(FO.gaussian_blur_u8(flat, [0, 256, 0]), flat)


def test_new_symbol_declared_exported_bound_and_record_size():
    from opticalflow_amd import _lib, augment_full, ops
    raw = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bpwc_kitti_augment_full\s*\(", text) and re.search(r"\bpwc_augment_full_params\b", text)
    assert "pwc_kitti_augment_full" in _lib.SIGNATURES and hasattr(lib, "pwc_kitti_augment_full")
    assert _lib.SIGNATURES["pwc_kitti_augment_full"] == _lib.SIGNATURES["pwc_kitti_augment"]
    assert _lib.ABI_VERSION == 13 and _lib.load().pwc_abi_version() == 13
    assert augment_full.FULL_PARAMS_DTYPE.itemsize == ops.AUGMENT_FULL_RECORD_BYTES == 128
    assert re.search(r"#define PWC_AUGMENT_FULL_MAX_SHIFT %d\b" % ops.AUGMENT_FULL_MAX_SHIFT, text)
    # the record's layout as the header declares it
    offs = {k: augment_full.FULL_PARAMS_DTYPE.fields[k][1] for k in augment_full.FULL_PARAMS_DTYPE.names}
    assert offs == {"m": 0, "cs": 48, "gain": 64, "wk": 68, "ksize": 82, "y0": 84, "x0": 88, "h": 92, "w": 96, "tx": 100, "ty": 104,
                    "flip": 108, "rot": 112, "trans": 116, "bright": 120, "blur": 124}
    # every unpinned point is stated where the operator is defined
    assert raw.count("parity against an actual cv2 build is unpinned") >= 3 and "softdouble" in raw and "NUMPY 2" in raw


def test_c_argument_checks_launch_nothing():
    from opticalflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(frames=p, gt=p, kind=0, valid=None, n=1, Hs=8, Ws=8, ch=4, cw=4, params=p, x=p, flow=p, mout=p, status=p):
        return lib.pwc_kitti_augment_full(frames, gt, kind, valid, n, Hs, Ws, ch, cw, params, x, flow, mout, status, None)
    # every call below fails its checks, which come before anything touches a device
    for kw in (dict(frames=None), dict(gt=None), dict(params=None), dict(x=None), dict(flow=None), dict(mout=None), dict(status=None),
               dict(n=0), dict(Hs=0), dict(Ws=-1), dict(ch=0), dict(cw=0), dict(n=65536), dict(Hs=32768), dict(Ws=32768),
               dict(ch=9), dict(cw=9), dict(kind=2), dict(kind=-1), dict(kind=1, valid=p)):
        assert call(**kw) == -1, kw
    assert b"pwc_kitti_augment_full" in lib.pwc_last_error()
    for kw in (dict(x=p + 2), dict(flow=p + 1), dict(mout=p + 2), dict(status=p + 2), dict(gt=p + 2), dict(kind=1, gt=p + 1),
               dict(params=p + 4)):
        assert call(**kw) == -3, kw


def test_wrapper_argument_errors_raise_without_a_device():
    from opticalflow_amd import PwcHipError, augment_full, ops
    frames = torch.zeros(2, 2, 8, 12, 3, dtype=torch.uint8)
    gt = torch.zeros(2, 8, 12, 3, dtype=torch.uint16)
    params = augment_full.make_full_params(2)
    params["h"], params["w"] = 8, 12
    dev_params = torch.zeros(2, 128, dtype=torch.uint8)
    with pytest.raises(PwcHipError):
        augment_full.augment_full_batch(frames, gt, None, params, (4, 8))
    with pytest.raises(PwcHipError):
        ops.kitti_augment_full(frames, gt, dev_params, (4, 8))
    with pytest.raises(PwcHipError):
        augment_full.DeviceFullAugmenter("cpu", 2, (8, 12), (4, 8))
    with pytest.raises(ValueError):
        ops.kitti_augment_full(frames[:, :, :, :, :2], gt, dev_params, (4, 8))
    with pytest.raises(ValueError):
        ops.kitti_augment_full(frames.float(), gt, dev_params, (4, 8))


def test_check_full_params_rejects_what_the_kernel_would_flag():
    from opticalflow_amd import augment_full
    params = augment_full.make_full_params(2)
    params["h"], params["w"] = 8, 12
    augment_full.set_blur(params[1], 1.0)
    params["trans"][1], params["tx"][1], params["ty"][1] = 1, -10, 10
    assert augment_full.check_full_params(params, 2, (8, 12), (4, 8)).tobytes() == params.tobytes()
    for field, value in (("h", 9), ("w", 13), ("h", 3), ("w", 7), ("y0", 5), ("x0", 5), ("y0", -1), ("x0", -1), ("h", 0),
                         ("ksize", 4), ("ksize", 9), ("ksize", 1), ("ksize", 3), ("tx", 32768), ("ty", -32768)):
        bad = params.copy()
        bad[field][1] = value
        with pytest.raises(ValueError):
            augment_full.check_full_params(bad, 2, (8, 12), (4, 8))
    bad = params.copy()
    bad["wk"][1, 2] += 1                                           # the weights no longer add up to 256
    with pytest.raises(ValueError):
        augment_full.check_full_params(bad, 2, (8, 12), (4, 8))
    # the fields of a stage that is off are not looked at
    off = params.copy()
    off["blur"][1], off["ksize"][1], off["trans"][1], off["tx"][1] = 0, 9, 0, 1 << 20
    augment_full.check_full_params(off, 2, (8, 12), (4, 8))
    with pytest.raises(ValueError):
        augment_full.check_full_params(params, 3, (8, 12), (4, 8))
    with pytest.raises(ValueError):
        augment_full.check_full_params(np.zeros((2, 128), np.uint8), 2, (8, 12), (4, 8))


def test_case_table_covers_what_the_gpu_tests_rely_on():
    for name in FO.CASES:
        samples, recs, crop, slot = FO.case_inputs(name)
        x, flow, mask = FO.case_expected(samples, recs, crop)
        assert x.shape == (len(recs), 6) + crop and 0 < mask.mean() < 1 and x.min() >= 0 and x.max() <= 1
    crop, items = FO.CASES["stages"]
    assert crop == (32, 64) and {s for s, _ in items} == set(SIZES)
    seen = {(frozenset(k for k in ("rot", "trans", "bright", "blur") if k in kw), bool(kw.get("flip"))) for _, kw in items}
    for stage in ((), ("rot",), ("trans",), ("bright",), ("blur",), ("rot", "trans", "bright", "blur")):
        assert (frozenset(stage), False) in seen and (frozenset(stage), True) in seen, stage
    assert FO.CASES["ragged"][0][1] % 4 != 0 and FO.CASES["ragged"][0][1] % 128 != 0
    assert FO.CASES["tiny"][0] == (5, 7) and FO.CASES["line"][0] == (1, 9)
    for name in ("tiny", "line"):
        _, recs, _, _ = FO.case_inputs(name)
        assert any(r["blur"] and r["ksize"] == 7 and r["rot"] and abs(r["tx"]) == 10 and abs(r["ty"]) == 10 for r in recs)
    ch, cw = FO.CASES["tiles"][0]
    assert ch > 2 * 8 and ch % 8 and cw > 2 * 128 and cw % 128 and cw % 4 == 0 and all(kw.get("blur") for _, kw in FO.CASES["tiles"][1])
    # the clamp of the brightness stage is hit at both ends
    samples, recs, crop, _ = FO.case_inputs("extremes")
    x, _, _ = FO.case_expected(samples, recs, crop)
    assert recs[3]["gain"] == np.float32(0.64) and recs[4]["gain"] == np.float32(1.44)
    assert (x[4] == 0).any() and (x[4] == 1).any() and x[3].min() > 0 and x[3].max() < 1
    assert [r["ksize"] for r in recs[5:10]] == [3, 3, 5, 5, 7]
    assert {bool(r["blur"]) for r in FO.case_inputs("mixed")[1]} == {False, True}
