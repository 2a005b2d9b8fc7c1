"""CPU checks of the device-side KITTI scoring (csrc/pwc_kitti_score.hip, ops.kitti_score, kitti.evaluate_stream): the float64
oracle reproduces the reference's own float64 results (g12 fixture) and the fixture meets the input conditions its generator asserts;
the C ABI is declared, bound, exported and refuses bad arguments before any launch."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import REPO, load_golden
import kitti_score_oracle as KO

NAMES = ("pwc_kitti_score_workspace_bytes", "pwc_kitti_score")
CASES = ("smooth", "rough", "odd", "ref_unpad", "identity", "sparse", "empty", "all_valid", "large")
PWC_EINVAL, PWC_EALIGN = -1, -3


def _case(z, name):
    ch, cw, H, W = (int(v) for v in z[name + "/geom"])
    return z[name + "/flow_q"], ch, cw, H, W, z[name + "/gt"]


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference_fp64(name):
    z = load_golden("g12_kitti_score.npz")
    fq, ch, cw, H, W, gt = _case(z, name)
    m = KO.score(fq, ch, cw, H, W, gt)
    nv, no = z[name + "/n_valid"], z[name + "/n_outlier"]
    epe_k, epe_i = z[name + "/epe"]
    fl_k, fl_i = z[name + "/fl"]
    print("%s: epe oracle %s reference %s; outliers oracle %s reference %s of %s valid; knife-edge %s relative branch %s"
          % (name, m["epe"], epe_k, m["n_outlier"], no, nv, m["knife_edge"], m["n_relative"]))
    # both sides are float64 and the fixture has no knife-edge pixel: the counts are exact
    assert np.array_equal(m["n_valid"], nv) and np.array_equal(m["n_outlier"], no)
    np.testing.assert_allclose(m["epe"], epe_k, rtol=1e-9, atol=0, equal_nan=True)
    np.testing.assert_allclose(m["fl"], fl_k, rtol=1e-12, atol=0, equal_nan=True)
    # the two reference scripts agree (inference.py reports 0.0 where inference_kitti.py reports nan: no valid pixel)
    has = nv > 0
    np.testing.assert_allclose(epe_i[has], epe_k[has], rtol=1e-12, atol=0)
    np.testing.assert_allclose(fl_i[has], fl_k[has], rtol=1e-12, atol=0)
    assert np.all(np.isnan(epe_k[~has])) and np.all(np.isnan(fl_k[~has])) and np.all(epe_i[~has] == 0.0) and np.all(fl_i[~has] == 0.0)
    # the fixture's own input conditions
    frac = no[has] / nv[has]
    assert np.all((frac >= 0.2) & (frac <= 0.8))
    assert m["knife_edge"].sum() <= 1e-4 * nv.sum()
    if name == "empty":
        assert list(has) == [True, False, True]
    if name == "all_valid":
        assert nv[0] == H * W
    if name == "identity":
        assert (ch, cw) == (H, W) == (24, 40)
    if name == "odd":
        assert (H, W, ch, cw) == (61, 131, 16, 33)


def test_fixture_exercises_both_threshold_branches():
    z = load_golden("g12_kitti_score.npz")
    both = 0
    for name in CASES:
        fq, ch, cw, H, W, gt = _case(z, name)
        m = KO.score(fq, ch, cw, H, W, gt)
        rel = m["n_relative"].sum() / float(m["n_valid"].sum())
        both += 0.1 <= rel <= 0.9
    assert both >= 2


def test_oracle_float_and_png_forms_agree():
    z = load_golden("g12_kitti_score.npz")
    fq, ch, cw, H, W, gt = _case(z, "empty")
    g, ok = KO.decode(gt)
    a, b = KO.score(fq, ch, cw, H, W, gt), KO.score(fq, ch, cw, H, W, g, ok)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_symbols_declared_bound_exported():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define PWC_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13
    assert "pwc_kitti_score.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()
    import opticalflow_amd
    from opticalflow_amd import kitti, ops
    for n in ("kitti_score", "kitti_score_workspace_bytes"):
        assert hasattr(ops, n)
    for n in ("ScoredInfer", "evaluate_stream"):
        assert hasattr(kitti, n) and not hasattr(opticalflow_amd, n)          # opticalflow_amd.kitti is the interface


def test_workspace_bytes_formula():
    from opticalflow_amd import _lib
    lib = _lib.load()
    # 24 bytes {fp64 sum, int64 valid, int64 outliers} per sample in front, then per 16 x 64 tile
    assert lib.pwc_kitti_score_workspace_bytes(1, 16, 64) == 24 * (1 + 1)
    assert lib.pwc_kitti_score_workspace_bytes(1, 17, 65) == 24 * (1 + 4)
    assert lib.pwc_kitti_score_workspace_bytes(16, 375, 1242) == 24 * 16 * (1 + 24 * 20)
    assert lib.pwc_kitti_score_workspace_bytes(3, 61, 131) == 24 * 3 * (1 + 4 * 3)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.pwc_kitti_score_workspace_bytes(*bad) == -1


def test_abi_argument_errors_without_gpu():
    """Argument validation happens before any launch, so it can be checked without a device (the pointers are never dereferenced)."""
    from opticalflow_amd import _lib
    lib = _lib.load()
    P = 1 << 20                                                  # a 16-byte aligned stand-in address
    n, Hq, Wq, ch, cw, H, W = 2, 16, 32, 16, 24, 64, 96
    need = lib.pwc_kitti_score_workspace_bytes(n, H, W)

    def call(flow_q=P, n=n, Hq=Hq, Wq=Wq, ch=ch, cw=cw, H=H, W=W, bsq=2 * Hq * Wq, gt=P, kind=1, valid=None, flow_out=None, ws=P,
             ws_bytes=need, out=P):
        rc = lib.pwc_kitti_score(flow_q, n, Hq, Wq, ch, cw, H, W, bsq, gt, kind, valid, flow_out, ws, ws_bytes, out, None)
        return rc, lib.pwc_last_error().decode()

    for kw in (dict(flow_q=None), dict(gt=None), dict(ws=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "null pointer" in msg, (kw, rc, msg)
    for kw in (dict(n=0), dict(Hq=0), dict(Wq=-1), dict(ch=0), dict(cw=0), dict(H=0), dict(W=0)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "bad shape" in msg, (kw, rc, msg)
    for kw in (dict(ch=Hq + 1), dict(cw=Wq + 1)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "larger than the map" in msg, (kw, rc, msg)
    rc, msg = call(bsq=2 * Hq * Wq - 1)
    assert rc == PWC_EINVAL and "batch stride" in msg
    for kind in (2, -1):
        rc, msg = call(kind=kind)
        assert rc == PWC_EINVAL and "gt_kind" in msg
    rc, msg = call(kind=1, valid=P)
    assert rc == PWC_EINVAL and "valid must be NULL" in msg
    rc, msg = call(ws_bytes=need - 1)
    assert rc == PWC_EINVAL and "workspace needs %d bytes" % need in msg
    rc, msg = call(ws=P + 4)
    assert rc == PWC_EALIGN and "8-byte aligned" in msg
    for kw in (dict(flow_q=P + 2), dict(out=P + 1), dict(flow_out=P + 2), dict(gt=P + 1, kind=1), dict(gt=P + 2, kind=0)):
        rc, msg = call(**kw)
        assert rc == PWC_EALIGN and "aligned" in msg, (kw, rc, msg)
    # grid / batch limits, as in pwc_fb_metrics
    big = lib.pwc_kitti_score_workspace_bytes(65536, 16, 64)
    rc, msg = call(n=65536, H=16, W=64, ws_bytes=big)
    assert rc == PWC_EINVAL and "65535" in msg
    rc, msg = call(n=4, H=16384, W=16384, ws_bytes=1 << 40)
    assert rc == PWC_EINVAL and "2^31" in msg


def test_python_surface():
    from opticalflow_amd import kitti
    sig = inspect.signature(kitti.evaluate_stream)
    assert list(sig.parameters)[:5] == ["model", "samples", "device", "batch", "reference_unpad"]
    assert sig.parameters["batch"].default == 16 and sig.parameters["reference_unpad"].default is True
    sig = inspect.signature(kitti.evaluate_pairs_sharded)
    assert sig.parameters["route"].default == "host"
    assert inspect.signature(kitti.ShardedStream.for_model).parameters["score"].default is False
    with pytest.raises(ValueError, match="route"):
        kitti.evaluate_pairs_sharded(None, [], route="bogus")
    # host-side totals -> rows: float64 ratios, nan for a sample without a valid pixel, which the mean skips
    rows = kitti.rows_from_totals([6.0, 0.0, 1.0], [4, 0, 2], [1, 0, 2])
    assert rows[0] == (1.5, 25.0) and np.isnan(rows[1][0]) and np.isnan(rows[1][1]) and rows[2] == (0.5, 100.0)
