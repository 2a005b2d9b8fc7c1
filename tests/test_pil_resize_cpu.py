"""Pillow-exact resize, host side (no GPU): the NumPy oracle against the Pillow-made fixture and against live Pillow, facts of the
coefficient tables, the C ABI's declarations and argument checks, and the supported-range predicate."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import pil_resize_oracle as R
from opticalflow_amd import _lib, pil_resize

SYMBOLS = ["pwc_pil_resize_ksize", "pwc_pil_resize_supported", "pwc_pil_resize_frames_u8", "pwc_pil_resize_planes_f32"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("g17_pil_resize.npz")


# ------------------------------------------------------------------ 1. oracle == fixture
@pytest.mark.parametrize("name", sorted(R.FRAME_CASES))
def test_oracle_frames_equal_fixture(golden, name):
    n, src, dst, seed = R.FRAME_CASES[name]
    frames = R.make_frames(n, src, seed)
    assert R.digest(frames) == str(golden["frame_%s_sha" % name]), "the case's input recipe changed"
    got = np.stack([R.resize_u8(f, dst) for f in frames])
    want = golden["frame_%s_u8" % name]
    assert got.shape == want.shape and np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    third = frames[:, :(src[0] + 2) // 3]
    assert set(np.unique(third)) <= {0, 255}                  # the saturated blocks are there
    if name == R.NORM_CASE:
        norm = R.normalise(got, R.IMAGENET_MEAN, R.IMAGENET_STD)
        assert np.array_equal(norm.view(np.int32), golden["frame_%s_norm" % name].view(np.int32))


@pytest.mark.parametrize("name", sorted(R.FLOW_CASES))
def test_oracle_flow_equals_fixture(golden, name):
    B, src, dst, seed = R.FLOW_CASES[name]
    flow = R.make_flow(B, src, seed)
    assert R.digest(flow) == str(golden["flow_%s_sha" % name]), "the case's input recipe changed"
    assert np.abs(flow).max() == 1e4
    got = R.resize_flow(flow, dst, scale_vectors=False)
    want = golden["flow_%s_f32" % name]
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_fixture_records_pillow_version_and_is_small(golden):
    assert re.match(r"\d+\.\d+", str(golden["pillow_version"]))
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g17_pil_resize.npz")) < 1000000


# ------------------------------------------------------------------ 2. oracle == live Pillow beyond the fixture
def test_oracle_equals_live_pillow_sweep():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(7)
    bad = []
    for I in range(1, 41):
        for O in (1, 7, 8, 64):
            # each length pair once as the horizontal and once as the vertical axis, the other axis changing too
            for (src, dst) in (((5, I), (9, O)), ((I, 6), (O, 4))):
                img = rng.randint(0, 256, src + (3,)).astype(np.uint8)
                img[: src[0] // 2] = (img[: src[0] // 2] > 127) * 255
                want = np.array(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
                if not np.array_equal(R.resize_u8(img, dst), want):
                    bad.append(("u8", src, dst))
                pl = (rng.randn(*src) * 30).astype(np.float32)
                wantf = np.array(Image.fromarray(pl).resize((dst[1], dst[0]), Image.BILINEAR))
                if not np.array_equal(R.resize_f32(pl, dst).view(np.int32), wantf.view(np.int32)):
                    bad.append(("f32", src, dst))
    assert not bad, bad[:10]


# ------------------------------------------------------------------ 3. table facts
@pytest.mark.parametrize("I,O", [(1080, 384), (1920, 512), (375, 384), (94, 96), (5, 64), (1, 8), (512, 64), (520, 65), (64, 512),
                                 (201, 67), (40, 7), (33, 1),
                                 # the edge cases of g20 (tests/test_pil_resize_edges_cpu.py)
                                 (263, 33), (1037, 130), (648, 130), (3, 40), (5, 200), (2, 130), (300, 70), (1, 20), (9, 2)])
def test_coeff_tables_facts(I, O):
    bounds, coeffs = pil_resize.coeff_tables(I, O)
    ks = pil_resize.ksize(I, O)
    assert bounds.shape == (O, 2) and bounds.dtype == np.int32 and coeffs.shape == (O, ks) and coeffs.dtype == np.float64
    first, cnt = bounds[:, 0].astype(int), bounds[:, 1].astype(int)
    assert (first >= 0).all() and (cnt >= 1).all() and (cnt <= ks).all() and (first + cnt <= I).all()
    assert (np.diff(first) >= 0).all() and (np.diff(first + cnt) >= 0).all()      # what the kernel's row staging relies on
    for i in range(O):
        assert (coeffs[i, cnt[i]:] == 0).all() and (coeffs[i] >= 0).all()
    k = pil_resize.fixed_point(coeffs)
    assert k.dtype == np.int32 and (np.abs(k.sum(1).astype(np.int64) - (1 << 22)) <= ks).all()
    assert np.abs(coeffs.sum(1) - 1.0).max() < 1e-12


def test_identity_rows_are_exactly_one_zero():
    for n in (1, 2, 64, 311):
        bounds, coeffs = pil_resize.coeff_tables(n, n)
        assert coeffs.shape == (n, 3)
        # the taps of an identity row are (left neighbour: 0, the pixel: 1) -- at the left edge the pixel alone
        for i in range(n):
            row = coeffs[i, :bounds[i, 1]]
            assert row.sum() == 1.0 and row.max() == 1.0 and sorted(row)[:-1] == [0.0] * (len(row) - 1)
            assert bounds[i, 0] + int(np.argmax(row)) == i
        k = pil_resize.fixed_point(coeffs)
        assert set(np.unique(k)) <= {0, 1 << 22}


def test_fixed_point_rounds_like_the_c_cast():
    c = np.array([[0.25, 0.5 / (1 << 22), 1.5 / (1 << 22), -0.25, -1.5 / (1 << 22), 0.0]])
    assert pil_resize.fixed_point(c).tolist() == [[1 << 20, 1, 2, -(1 << 20), -2, 0]]


def test_norm_lut_is_torch_elementwise():
    lut = pil_resize.norm_lut(R.IMAGENET_MEAN, R.IMAGENET_STD)
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    want = R.normalise(u8, R.IMAGENET_MEAN, R.IMAGENET_STD).reshape(3, 256)
    assert lut.dtype == torch.float32 and np.array_equal(lut.numpy().view(np.int32), want.view(np.int32))
    plain = pil_resize.norm_lut()
    assert np.array_equal(plain.numpy().view(np.int32), R.normalise(u8).reshape(3, 256).view(np.int32))
    with pytest.raises(ValueError):
        pil_resize.norm_lut(R.IMAGENET_MEAN, None)


# ------------------------------------------------------------------ 4. declared, exported, bound
def test_symbols_declared_exported_bound():
    import opticalflow_amd
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in SYMBOLS:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define PWC_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13 and _lib.load().pwc_abi_version() == 13
    mk = open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()
    assert "pwc_pil_resize.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert opticalflow_amd.pil_resize is pil_resize
    assert opticalflow_amd.resize_frames is pil_resize.resize_frames and opticalflow_amd.resize_flow is pil_resize.resize_flow
    from opticalflow_amd import ops
    for n in ("pil_resize_frames", "pil_resize_planes", "pil_resize_supported"):
        assert callable(getattr(ops, n))


# ------------------------------------------------------------------ 5. argument checks, nothing launched
def test_argument_checks_without_gpu():
    lib = _lib.load()
    P = ctypes.c_void_p(4096)
    odd4, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    E, A = -1, -3

    def frames(src=P, out=P, out8=None, n=2, H=270, W=480, h=96, w=128, xb=P, xk=P, xks=9, yb=P, yk=P, yks=7, lut=P, bs=3 * 96 * 128,
               group=2):
        return lib.pwc_pil_resize_frames_u8(src, out, out8, n, H, W, h, w, xb, xk, xks, yb, yk, yks, lut, bs, group, None)

    def err():
        return lib.pwc_last_error()

    for kw in ({"src": None}, {"out": None}, {"xb": None}, {"xk": None}, {"yb": None}, {"yk": None}, {"lut": None}):
        assert frames(**kw) == E and b"null pointer" in err()
    for kw in ({"n": 0}, {"H": 0}, {"W": -1}, {"h": 0}, {"w": 0}, {"group": 0}):
        assert frames(**kw) == E and b"bad shape" in err()
    assert frames(xks=7) == E and b"ksize" in err()
    assert frames(yks=9) == E and b"ksize" in err()
    assert frames(H=96 * 8 + 1) == E and b"supported" in err()
    assert frames(W=128 * 8 + 1) == E and b"supported" in err()
    assert frames(bs=3 * 96 * 128 - 1) == E and b"batch stride" in err()
    assert frames(group=1, bs=3 * 96 * 128) == E and b"batch stride" in err()         # two frames in one item need 6 planes
    assert frames(n=65536, group=65536) == E and b"grid" in err()
    assert frames(out=odd4) == A and frames(xb=odd4) == A and frames(yk=odd4) == A and frames(lut=odd4) == A

    def planes(src=P, dst=P, n=2, c=2, ih=24, iw=80, oh=94, ow=311, xb=P, xk=P, xks=3, yb=P, yk=P, yks=3, fac=None, bs=2 * 24 * 80):
        return lib.pwc_pil_resize_planes_f32(src, dst, n, c, ih, iw, oh, ow, xb, xk, xks, yb, yk, yks, fac, bs, None)

    for kw in ({"src": None}, {"dst": None}, {"xb": None}, {"xk": None}, {"yb": None}, {"yk": None}):
        assert planes(**kw) == E and b"null pointer" in err()
    for kw in ({"n": 0}, {"c": 0}, {"ih": 0}, {"iw": 0}, {"oh": -3}, {"ow": 0}):
        assert planes(**kw) == E and b"bad shape" in err()
    assert planes(xks=5) == E and b"ksize" in err()
    assert planes(ih=40, oh=17, yks=5) == E and b"ksize" in err()                     # 40 -> 17 needs 2 * ceil(2.35) + 1 = 7
    assert planes(ih=94 * 8 + 1) == E and b"supported" in err()
    assert planes(bs=2 * 24 * 80 - 1) == E and b"batch stride" in err()
    assert planes(n=32768, c=2) == E and b"grid" in err()
    assert planes(src=odd4) == A and planes(dst=odd4) == A and planes(fac=odd4) == A
    assert planes(xk=odd8) == A and planes(yk=odd8) == A                               # doubles: 8-byte alignment


# ------------------------------------------------------------------ 6. the supported range
def test_supported_predicates():
    from opticalflow_amd import ops
    lib = _lib.load()
    for I, O in ((1080, 384), (1920, 512), (375, 384), (64, 512), (512, 64), (1, 8), (8, 1), (520, 65), (96, 375), (5, 64), (1, 9), (64, 513)):
        assert lib.pwc_pil_resize_ksize(I, O) == pil_resize.ksize(I, O)
    # more than 8 only to an output shorter than a tile, while the tile's table slice (64 rows of 17 entries on x) and its source
    # span still fit what the kernels stage: 9 -> 1 (ksize 21), 16 -> 1 (33), 29 -> 3 (21), 512 -> 32 (33 x 32 = 1056 entries)
    for I, O in ((9, 1), (16, 1), (29, 3), (512, 32), (72, 8)):
        assert lib.pwc_pil_resize_ksize(I, O) == pil_resize.ksize(I, O) > 17
    for I, O in ((513, 64), (1041, 130), (545, 33), (2000, 3), (0, 4), (4, 0), (-1, 4), ((1 << 20) + 1, 1 << 20)):
        assert lib.pwc_pil_resize_ksize(I, O) == -1
    assert ops.pil_resize_supported((1080, 1920), (384, 512)) and ops.pil_resize_supported((375, 1242), (384, 1280))
    assert ops.pil_resize_supported((96, 320), (375, 1242)) and ops.pil_resize_supported((512, 520), (64, 65))
    assert ops.pil_resize_supported((1, 1), (8, 8)) and ops.pil_resize_supported((64, 64), (64, 64))
    assert not ops.pil_resize_supported((513, 64), (64, 64)) and not ops.pil_resize_supported((64, 513), (64, 64))
    assert ops.pil_resize_supported((64, 64), (513, 64)) and ops.pil_resize_supported((129, 5), (64, 64))          # any upscale
    assert not ops.pil_resize_supported((0, 64), (64, 64)) and not ops.pil_resize_supported((64, 64), (64, -2))
    # the short-output extension is per axis and per tile: 16 rows of 17 entries on y, 64 rows on x
    assert ops.pil_resize_supported((16, 16), (1, 1)) and ops.pil_resize_supported((9, 9), (1, 1)) and ops.pil_resize_supported((37, 29), (19, 3))
    assert ops.pil_resize_supported((128, 8), (16, 8)) and not ops.pil_resize_supported((129, 8), (16, 8)) and ops.pil_resize_supported((8, 129), (8, 16))
    assert ops.pil_resize_supported((126, 8), (14, 8)) and not ops.pil_resize_supported((127, 8), (14, 8))          # 14 x 19 <= 16 x 17 < 14 x 21
    assert not ops.pil_resize_supported((4, 513), (4, 64)) and not ops.pil_resize_supported((2000, 4), (3, 4))
    with pytest.raises(ValueError, match="supported range"):
        pil_resize.prepare((2160, 3840), (64, 64), "cpu")
    with pytest.raises(ValueError):
        pil_resize.coeff_tables(0, 4)


def test_frame_ingest_refuses_mixed_sizes_before_any_device_work():
    ing = pil_resize.FrameIngest((8, 8), device="cpu", batch=2)
    a, b = np.zeros((6, 6, 3), np.uint8), np.zeros((6, 7, 3), np.uint8)
    with pytest.raises(ValueError, match="must be uint8"):
        ing.pairs([a], [b])
    with pytest.raises(ValueError, match="frames per side"):
        ing.pairs([a, a, a], [a, a, a])
