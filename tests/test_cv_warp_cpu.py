"""cv2.warpPerspective-exact warp (opticalflow_amd/cv_warp.py), what can be said without a GPU: the NumPy oracle the GPU tests compare
against equals a plain scalar loop and the hand-worked vectors; the host helpers are the oracle's own bit for bit; the new entry
point is declared, bound and exported; the wrappers refuse what they cannot take; and the tie case tells round-half-even from
round-half-up.  cv2 parity is unpinned."""
import os
import re

import numpy as np
import pytest
import torch

import cv_warp_oracle as R
from opticalflow_amd import _lib, cv_warp, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOL = "pwc_cv_warp_perspective_u8"
PWC_EINVAL, PWC_EALIGN = -1, -3                 # include/pwc_hip.h


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", sorted(R.WARP_CASES))
def test_oracle_equals_the_scalar_loop(name):
    n, src, dst, seed = R.WARP_CASES[name]
    frames = R.make_frames(n, src, seed)
    for M, inverse in R.case_matrices(name):
        got = R.warp_frames(frames, M, dst, inverse)
        assert got.shape == (n,) + dst + (3,) and got.dtype == np.uint8
        for i, f in enumerate(frames):
            m = M if M.ndim == 2 else M[i]
            assert np.array_equal(got[i], R.warp_scalar(f, m if inverse else R.invert3x3(m), dst)), (name, i)


def test_oracle_reproduces_the_hand_worked_vectors():
    t = np.asarray([[10, 20], [30, 40]], np.uint8)
    assert R.warp(t, R.translation(0.5, 0.5), (2, 2), inverse=True).tolist() == [[25, 15], [18, 10]]
    img = R.make_frames(1, (11, 13), 5)[0]
    assert np.array_equal(R.warp(img, np.eye(3), (11, 13)), img)                 # weight 32 * 32 is exact on bytes
    assert np.array_equal(R.warp(img, np.eye(3), (11, 13), inverse=True), img)
    # an integer shift: destination (x, y) reads source (x - 2, y + 3); what is vacated is 0
    got = R.warp(img, R.translation(-2.0, 3.0), (11, 13), inverse=True)
    want = np.zeros_like(img)
    want[:8, 2:] = img[3:, :11]
    assert np.array_equal(got, want)
    # the forward form of the same shift
    assert np.array_equal(R.warp(img, R.translation(2.0, -3.0), (11, 13)), want)
    # a larger destination: the image sits in its corner
    big = R.warp(img, np.eye(3), (14, 20))
    assert np.array_equal(big[:11, :13], img) and not big[11:].any() and not big[:, 13:].any()


def test_cases_reach_what_they_name():
    """Each case of the table holds the situation its comment claims."""
    def c(name, k=0):
        _, (H, W), (h, w), _ = R.WARP_CASES[name]
        M, inverse = R.case_matrices(name)[k]
        return R.coords(M if inverse else R.invert3x3(M), h, w) + (H, W)
    sx, sy, ax, ay, H, W = c("topview")
    inside = (sx >= 0) & (sx < W - 1) & (sy >= 0) & (sy < H - 1)
    assert 0.9 < inside.mean() < 1.0 and ax.any() and ay.any()
    sx, sy, ax, ay, H, W = c("shift")
    assert not ax.any() and not ay.any() and (sx < 0).any() and (sy >= H).any()
    sx, sy, ax, ay, H, W = c("subpix")
    assert (ax == 13).all() and (ay == 5).all()
    sx, sy, ax, ay, H, W = c("zoomout")
    assert ((sx < -1) | (sx >= W)).any() and ((sx >= 0) & (sx < W - 1) & (sy >= 0) & (sy < H - 1)).any()
    sx, sy, ax, ay, H, W = c("horizon", 0)                                       # Wd == 0 at x = 3: the coordinate is (0, 0)
    assert (sx[:, 3] == 0).all() and (sy[:, 3] == 0).all() and (ax[:, 3] == 0).all()
    sx, sy, ax, ay, H, W = c("horizon", 1)                                       # 8 * 32 / -1e-10 and (y + 5) * 32 / -1e-10 clamp
    assert (sx[:, 3] == -32768).all() and (sy[:, 3] == -32768).all()
    assert (sx[:, 2] < 0).all() and (sx[:, 4:] > 0).all()                        # the denominator changes sign across the column
    _, (H, W), (h, w), _ = R.WARP_CASES["short"]
    assert min(16, h) == 5 and min(1024 // 5, w) == w                            # one block
    _, _, (h, w), _ = R.WARP_CASES["topview"]
    assert min(1024 // min(16, h), w) == 64 and -(-w // 64) == 3                 # three 64-pixel blocks


def test_int_clamps_are_reached():
    """Products past the int32 range clamp to INT_MIN / INT_MAX before cvRound, in both signs, and a NaN product becomes INT_MAX."""
    Mi = np.array([[1.0, 0.0, 5.0], [0.0, -1.0, -5.0], [1.0, 0.0, -3.0000000001]])
    sx, sy, ax, ay = R.coords(Mi, 4, 8)
    assert (sx[:, 3] == -32768).all() and (sy[:, 3] == 32767).all() and (ax[:, 3] == 0).all() and (ay[:, 3] == 31).all()
    Mi = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 5e-324]])      # 32 / denormal = inf; 0 * inf = NaN at x = 0
    sx, sy, ax, ay = R.coords(Mi, 2, 2)
    assert sx[0, 0] == 32767 and ax[0, 0] == 31 and sx[0, 1] == 32767 and sy[1, 0] == 32767


def test_host_helpers():
    M = R.topview_matrix(1920, 1080)
    assert np.abs(cv_warp.invert3x3(M) @ M - np.eye(3)).max() < 1e-12
    for wh in ((1920, 1080), (150, 100), (5, 37), (50, 40)):
        src, dst = R.topview_points(*wh)
        P = cv_warp.perspective_matrix(src, dst)
        assert P[2, 2] == 1.0
        q = np.concatenate([src.astype(np.float64), np.ones((4, 1))], axis=1) @ P.T
        assert np.abs(q[:, :2] / q[:, 2:] - dst.astype(np.float64)).max() < 1e-9
        # the product's helpers are the oracle's own, bit for bit
        assert np.array_equal(_bits(cv_warp.topview_matrix(*wh)), _bits(R.topview_matrix(*wh)))
        assert np.array_equal(_bits(cv_warp.invert3x3(P)), _bits(R.invert3x3(P)))
        assert np.array_equal(_bits(cv_warp.perspective_matrix(src, dst)), _bits(R.perspective_matrix(src, dst)))
    assert np.array_equal(_bits(cv_warp.inverse_maps(M)), _bits(R.invert3x3(M).reshape(9)))
    assert np.array_equal(_bits(cv_warp.inverse_maps(M, inverse_map=True)), _bits(M.reshape(9)))
    both = cv_warp.inverse_maps(np.stack([M, np.eye(3)]))
    assert both.shape == (2, 9) and np.array_equal(_bits(both[0]), _bits(R.invert3x3(M).reshape(9)))
    nan = np.eye(3)
    nan[1, 2] = np.nan
    for call in (lambda: cv_warp.invert3x3(np.zeros((3, 3))), lambda: cv_warp.invert3x3(np.ones((3, 3))),
                 lambda: cv_warp.invert3x3(nan), lambda: cv_warp.invert3x3(np.eye(4)), lambda: cv_warp.inverse_maps(nan, True),
                 lambda: cv_warp.inverse_maps(np.full((3, 3), np.inf)), lambda: cv_warp.inverse_maps(np.zeros((2, 3, 3))),
                 lambda: cv_warp.inverse_maps(np.eye(2)), lambda: cv_warp.perspective_matrix(np.zeros((3, 2)), np.zeros((3, 2)))):
        with pytest.raises(ValueError):
            call()


def test_new_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = _lib.load()
    assert lib.pwc_abi_version() == _lib.ABI_VERSION == 13
    decl = re.search(r"^int %s\(([^;]*)\);" % NEW_SYMBOL, header, re.M | re.S)
    assert decl, "%s is not declared in include/pwc_hip.h" % NEW_SYMBOL
    assert NEW_SYMBOL in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NEW_SYMBOL][1]) == decl.group(1).count(",") + 1
    assert getattr(lib, NEW_SYMBOL).argtypes == _lib.SIGNATURES[NEW_SYMBOL][1]
    assert "pwc_cv_warp.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()
    import opticalflow_amd
    assert opticalflow_amd.cv_warp is cv_warp and opticalflow_amd.TopviewInfer is cv_warp.TopviewInfer
    assert opticalflow_amd.TopviewStream is cv_warp.TopviewStream


def test_library_checks_arguments_before_touching_memory():
    """The argument checks come before any use of the pointers, so they can be exercised with made-up addresses and no device."""
    lib = _lib.load()
    a, m = 0x10000, 0x20000
    good = dict(src=a, dst=a, n=1, H=4, W=4, h=4, w=4, mat=m, ms=0, sb=48, db=48, stream=None)       # in the ABI's argument order
    call = lambda **k: lib.pwc_cv_warp_perspective_u8(*{**good, **k}.values())
    for bad in (dict(src=None), dict(dst=None), dict(mat=None), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(H=32768), dict(W=32768),
                dict(h=32768), dict(w=32768), dict(n=0), dict(n=65536), dict(ms=5), dict(ms=-9), dict(sb=47), dict(db=47)):
        assert call(**bad) == PWC_EINVAL, bad
    assert call(mat=m + 4) == PWC_EALIGN


def test_wrappers_reject_host_tensors_and_wrong_shapes():
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    M = np.eye(3)
    with pytest.raises(ValueError):
        ops.cv_warp_perspective(frames, torch.zeros(9, dtype=torch.float64), torch.zeros_like(frames))     # host tensors
    for call in (lambda: cv_warp.warp_frames(frames, M), lambda: cv_warp.warp_frames(frames.float(), M),
                 lambda: cv_warp.warp_frames(frames[0], M), lambda: cv_warp.warp_frames(torch.zeros((1, 8, 8, 4), dtype=torch.uint8), M),
                 lambda: cv_warp.TopviewInfer(None, 8, 8, "cpu", M), lambda: cv_warp.TopviewStream(None, 8, 8, "cpu", M)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("name", sorted(R.TIE_CASES))
def test_tie_case_tells_half_even_from_half_up(name):
    n, src, dst, seed = R.WARP_CASES[name]
    frames = R.make_frames(n, src, seed)
    (M, inverse), = R.case_matrices(name)
    even, up = R.warp_frames(frames, M, dst, inverse), R.warp_frames(frames, M, dst, inverse, half_up=True)
    changed = int((even != up).sum())
    print("%s: %d of %d bytes change under half-up rounding" % (name, changed, even.size))
    assert changed == R.TIE_CASES[name] and changed > 0
    # the tie itself: both fixed-point products sit exactly on .5
    x, y = np.arange(dst[1], dtype=np.float64), np.arange(dst[0], dtype=np.float64)
    fx, fy = (x + M[0, 2]) * 32.0, (y + M[1, 2]) * 32.0
    assert (fx - np.floor(fx) == 0.5).all() and (fy - np.floor(fy) == 0.5).all()
