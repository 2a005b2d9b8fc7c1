"""CPU checks of the epipolar mask / soft Sampson penalty (train_fundamental.py:169-382): the C ABI is declared, bound and
exported and validates its arguments before any launch; the workspace formulas; the NumPy oracle reproduces the reference's own
results (g9 fixture); the host index table and the seeded flows match the fixture's sha256."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import REPO, load_golden
import epipolar_oracle as O

NAMES = ("pwc_epipolar_pairs", "pwc_epipolar_ransac_workspace_bytes", "pwc_epipolar_ransac", "pwc_epipolar_distance",
         "pwc_epipolar_mask_workspace_bytes", "pwc_epipolar_mask", "pwc_epipolar_loss_workspace_bytes", "pwc_epipolar_loss_fwd",
         "pwc_epipolar_loss_bwd")
CASES = ("small", "large", "nan", "fewpts", "minkeep")


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def case_flow(z, name):
    H, W, stride, seed = (int(v) for v in z[name + "/cfg"][:4])
    fl = O.rigid_flow(H, W, seed)
    if name == "nan":
        fl[:, 20:36, 40:72] = np.nan
    assert np.array_equal(_sha(fl), z[name + "/flow_sha"]), "seeded flow recipe drifted from the fixture"
    return fl


def case_mask(z, name):
    H, W, stride = (int(v) for v in z[name + "/cfg"][:3])
    if name != "fewpts":
        return None
    m = np.zeros((H, W), bool)
    m[0, 0:5 * stride:stride] = True
    return m


def test_symbols_declared_bound_exported():
    from opticalflow_amd import _lib, epipolar, ops
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define PWC_ABI_VERSION 13" in text and _lib.load().pwc_abi_version() == 13
    for n in ("epipolar_pairs", "epipolar_ransac", "epipolar_distance", "epipolar_mask", "epipolar_loss",
              "epipolar_loss_backward", "EpipolarSampsonFunction"):
        assert hasattr(ops, n)
    for n in ("ransac_fundamental", "sampson_distance", "build_epipolar_mask_from_flow", "epipolar_sampson_loss", "index_table"):
        assert hasattr(epipolar, n)
    assert "pwc_epipolar.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()


def test_workspace_formulas():
    from opticalflow_amd import _lib
    lib = _lib.load()
    pad8 = lambda n: (n + 7) // 8 * 8          # noqa: E731
    for B, it in ((1, 1), (4, 2000), (16, 1000), (3, 7)):
        assert lib.pwc_epipolar_ransac_workspace_bytes(B, it) == pad8(B * it * 72)
    for B, H, W in ((4, 384, 512), (16, 448, 1024), (1, 1, 1), (3, 37, 53)):
        assert lib.pwc_epipolar_mask_workspace_bytes(B, H, W) == pad8(B * H * W * 8) + pad8(4 * B)
        assert lib.pwc_epipolar_loss_workspace_bytes(B, H, W) == 16 * B * (-(-(H * W) // 2048)) + 16
    for bad in ((0, 1), (1, 0), (-1, 5)):
        assert lib.pwc_epipolar_ransac_workspace_bytes(*bad) == -1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -2)):
        assert lib.pwc_epipolar_mask_workspace_bytes(*bad) == -1
        assert lib.pwc_epipolar_loss_workspace_bytes(*bad) == -1


_BUF_BYTES = 1 << 20


@pytest.fixture(scope="module")
def host_bufs():
    # host memory handed to entries that must reject their arguments before touching (or launching on) any pointer
    bufs = [ctypes.create_string_buffer(_BUF_BYTES) for _ in range(8)]
    return [ctypes.addressof(b) for b in bufs]


def test_argument_errors_before_launch(host_bufs):
    from opticalflow_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUP = -1, -2
    p = host_bufs
    B, H, W = 2, 16, 24
    # pairs: null, shape, stride, batch stride, misalignment
    assert lib.pwc_epipolar_pairs(None, None, 0, p[1], p[2], B, H, W, 4, 2 * H * W, 0, None) == EINVAL
    assert lib.pwc_epipolar_pairs(p[0], None, 0, p[1], p[2], B, H, W, 0, 2 * H * W, 0, None) == EINVAL
    assert lib.pwc_epipolar_pairs(p[0], None, 0, p[1], p[2], B, H, W, 4, 2 * H * W - 1, 0, None) == EINVAL
    assert lib.pwc_epipolar_pairs(p[0], p[3], 1, p[1], p[2], B, H, W, 4, 2 * H * W, H * W - 1, None) == EINVAL
    assert lib.pwc_epipolar_pairs(p[0] + 2, None, 0, p[1], p[2], B, H, W, 4, 2 * H * W, 0, None) == EUNSUP
    assert lib.pwc_epipolar_pairs(p[0], None, 0, p[1] + 4, p[2], B, H, W, 4, 2 * H * W, 0, None) == EUNSUP
    # ransac: null, shape, index stride, workspace, alignment, NaN threshold
    it = 10
    nb = lib.pwc_epipolar_ransac_workspace_bytes(B, it)
    args = lambda **k: [k.get("pts", p[0]), p[1], 96, p[2], k.get("ibs", 0), B, k.get("it", it), k.get("thr", 0.5), p[3], p[4],
                        p[5], p[6], k.get("ws", p[7]), k.get("nb", nb), None]   # noqa: E731
    assert lib.pwc_epipolar_ransac(*args(pts=None)) == EINVAL
    assert lib.pwc_epipolar_ransac(*args(it=0)) == EINVAL
    assert lib.pwc_epipolar_ransac(*args(ibs=8 * it - 1)) == EINVAL
    assert lib.pwc_epipolar_ransac(*args(nb=nb - 8)) == EINVAL
    assert lib.pwc_epipolar_ransac(*args(ws=p[7] + 4)) == EINVAL
    assert lib.pwc_epipolar_ransac(*args(pts=p[0] + 4)) == EUNSUP
    assert lib.pwc_epipolar_ransac(*args(thr=float("nan"))) == EUNSUP
    # distance
    assert lib.pwc_epipolar_distance(p[0], None, 0, p[1], B, H, W, 2 * H * W, None) == EINVAL
    assert lib.pwc_epipolar_distance(p[0], p[2], 5, p[1], B, H, W, 2 * H * W, None) == EINVAL
    assert lib.pwc_epipolar_distance(p[0], p[2], 9, p[1] + 4, B, H, W, 2 * H * W, None) == EUNSUP
    # mask
    nm = lib.pwc_epipolar_mask_workspace_bytes(B, H, W)
    margs = lambda **k: [p[0], p[1], k.get("ok", p[2]), p[3], p[4], None, B, H, W, k.get("tau", 1.0), 0.2, 0.05,
                         k.get("bs", 2 * H * W), p[5], k.get("nb", nm), None]   # noqa: E731
    assert lib.pwc_epipolar_mask(*margs(ok=None)) == EINVAL
    assert lib.pwc_epipolar_mask(*margs(bs=2 * H * W - 1)) == EINVAL
    assert lib.pwc_epipolar_mask(*margs(nb=nm - 1)) == EINVAL
    assert lib.pwc_epipolar_mask(*margs(tau=float("nan"))) == EUNSUP
    assert lib.pwc_epipolar_mask(*margs(ok=p[2] + 2)) == EUNSUP
    # loss fwd / bwd
    nl = lib.pwc_epipolar_loss_workspace_bytes(B, H, W)
    largs = lambda **k: [p[0], p[1], 9, None, 0, None, 0, k.get("out", p[2]), B, H, W, k.get("robust", 0), k.get("delta", 1.0),
                         0.1, 2 * H * W, 0, p[3], k.get("nb", nl), None]   # noqa: E731
    assert lib.pwc_epipolar_loss_fwd(*largs(out=None)) == EINVAL
    assert lib.pwc_epipolar_loss_fwd(*largs(robust=3)) == EINVAL
    assert lib.pwc_epipolar_loss_fwd(*largs(nb=nl - 8)) == EINVAL
    assert lib.pwc_epipolar_loss_fwd(*largs(delta=0.0)) == EUNSUP
    a = largs()
    assert lib.pwc_epipolar_loss_bwd(*(a[:7] + [None, p[4]] + a[8:])) == EINVAL
    assert lib.pwc_epipolar_loss_bwd(*(a[:7] + [p[5], p[4] + 2] + a[8:])) == EUNSUP
    assert b"pwc_epipolar_loss_bwd" in lib.pwc_last_error()


def test_host_index_table_matches_fixture():
    from opticalflow_amd import epipolar
    z = load_golden("g9_epipolar.npz")
    for name in CASES:
        N = int(z[name + "/cfg"][7])
        if N < 8:
            assert name + "/idx_sha" not in z.files
            continue
        t = epipolar.index_table(N, 0, 2000)
        assert t.dtype == np.int32 and t.shape == (2000, 8)
        assert np.array_equal(_sha(t), z[name + "/idx_sha"]), name
        assert np.array_equal(epipolar.index_table(N, 0, 1000), t[:1000])       # the soft fit's prefix
        assert np.array_equal(O.index_table(N, 0, 2000), t)


def test_reference_svd_quirk_is_not_the_null_vector():
    # the thin SVD of an 8 x 9 matrix returns 8 right vectors: VT[-1] is the 8th singular vector, not the null vector
    A = np.random.default_rng(0).standard_normal((8, 9))
    v = np.linalg.svd(A, full_matrices=False)[2][-1]
    assert np.linalg.norm(A @ v) > 1e-3
    assert np.linalg.norm(A @ np.linalg.svd(A)[2][-1]) < 1e-12


@pytest.mark.parametrize("name", ["small", "nan", "fewpts", "minkeep"])
def test_oracle_reproduces_g9(name):
    z = load_golden("g9_epipolar.npz")
    H, W, stride = (int(v) for v in z[name + "/cfg"][:3])
    tau, kr, mk = (float(v) for v in z[name + "/cfg"][4:7])
    fl = case_flow(z, name)
    hw2 = np.ascontiguousarray(fl.transpose(1, 2, 0))
    m = case_mask(z, name)
    p1, p2 = O.flow_to_pairs(hw2, stride, m)
    assert p1.shape[0] == int(z[name + "/cfg"][7])
    for tag, iters, thr in (("fit", 2000, 0.5), ("soft", 1000, 1.0)):
        fit = O.ransac(p1, p2, iters, thr, 0)
        assert fit["ok"] == bool(z[name + "/%s_ok" % tag])
        if not fit["ok"]:
            continue
        assert np.array_equal(fit["counts"], z[name + "/%s_counts" % tag].astype(np.int64))
        assert fit["best"] == int(z[name + "/%s_best" % tag])
        Fr = z[name + "/%s_F" % tag]
        assert np.abs(fit["F"] - Fr).max() <= 1e-12 * max(1.0, np.abs(Fr).max())
    mask, thr, _ = O.epipolar_mask(hw2, tau, stride, m, kr, mk)
    assert np.array_equal(np.packbits(mask.ravel()), z[name + "/mask"])
    if thr is None:
        assert np.isnan(z[name + "/thr"])
    else:
        assert thr == float(z[name + "/thr"])
    if bool(z[name + "/soft_ok"]):
        F32 = z[name + "/soft_F"].astype(np.float32)
        loss, _ = O.soft_loss(fl[None], F32, mask[None], weight=0.1)
        # the reference evaluates x2^T F x1 in float32, where it cancels (d ~ 1e-5 of its terms): 1e-3 of the value, not 1e-6
        assert abs(loss - float(z[name + "/soft_loss"])) <= 1e-3 * abs(float(z[name + "/soft_loss"]))
    if name == "small":
        loss64, g64 = O.soft_loss(fl[None], z[name + "/soft_F"], mask[None], weight=0.1)
        assert abs(loss64 - float(z[name + "/soft_loss64"])) <= 1e-12 * abs(loss64)
        gr = z[name + "/soft_grad64"]
        assert np.abs(g64[0] - gr).max() <= 1e-6 * np.abs(gr).max()      # autograd and the closed form cancel differently


def test_oracle_reproduces_g9_counts_large():
    # the 384 x 512 stride-6 case: counts of every hypothesis and the chosen index (the refit F at 1e-12 too)
    z = load_golden("g9_epipolar.npz")
    name = "large"
    fl = case_flow(z, name)
    p1, p2 = O.flow_to_pairs(np.ascontiguousarray(fl.transpose(1, 2, 0)), 6, None)
    fit = O.ransac(p1, p2, 2000, 0.5, 0)
    assert np.array_equal(fit["counts"], z[name + "/fit_counts"].astype(np.int64)) and fit["best"] == int(z[name + "/fit_best"])
    Fr = z[name + "/fit_F"]
    assert np.abs(fit["F"] - Fr).max() <= 1e-12 * max(1.0, np.abs(Fr).max())


def test_product_refuses_cpu_tensors():
    import torch
    from opticalflow_amd import epipolar
    from opticalflow_amd._lib import PwcHipError
    f = torch.zeros(1, 2, 16, 16)
    for fn in (lambda: epipolar.ransac_fundamental(f), lambda: epipolar.build_epipolar_mask_from_flow(f),
               lambda: epipolar.sampson_distance(f, np.eye(3)), lambda: epipolar.epipolar_sampson_loss(f, np.eye(3))):
        with pytest.raises(PwcHipError):
            fn()
