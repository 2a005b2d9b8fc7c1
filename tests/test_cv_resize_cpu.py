"""cv2.resize-exact ingest / exit (opticalflow_amd/cv_resize.py), what can be said without a GPU: the NumPy oracle the GPU tests
compare against is the statement harness.cv2_resize_linear makes and reproduces the hand-worked vectors of tests/test_harness.py; the
host tables are the scalar loop's; the byte table is the reference's division; the new entry points are declared, bound and exported;
the wrappers refuse what they cannot take; and the tie cases tell round-half-even from round-half-up.  cv2 parity is unpinned."""
import os
import re

import numpy as np
import pytest
import torch

import cv_resize_oracle as R
from opticalflow_amd import _lib, cv_resize, harness, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pwc_cv_resize_frames_u8", "pwc_cv_resize_flow_f32")


@pytest.mark.parametrize("name", sorted(R.FRAME_CASES))
def test_oracle_frames_equal_harness(name):
    n, src, dst, seed = R.FRAME_CASES[name]
    frames = R.make_frames(n, src, seed)
    for f in frames:
        want = harness.cv2_resize_linear(torch.from_numpy(f), *dst).numpy()
        assert np.array_equal(R.resize_u8(f, dst), want)
    # and the whole ingest against the chain's own steps with the reference's division: flip, / 255 in float64 -> float32, HWC -> CHW
    got = R.ingest(frames[:1], dst, flip=True)[0]
    r = harness.cv2_resize_linear(torch.from_numpy(frames[0]), *dst).numpy()[:, :, ::-1]
    assert np.array_equal(got, (1.0 * r / 255.0).astype(np.float32).transpose(2, 0, 1))


@pytest.mark.parametrize("name", sorted(R.FLOW_CASES))
def test_oracle_flow_equals_harness(name):
    n, src, dst, seed = R.FLOW_CASES[name]
    flow = R.make_flow(n, src, seed, specials=name == R.SPECIALS_CASE)
    for plane in flow.reshape((-1,) + src):
        want = harness.cv2_resize_linear(torch.from_numpy(plane), *dst).numpy()
        assert R.same_bits_nan_by_position(R.resize_f32(plane, dst), want)
    # the exit as harness.postprocess writes it (x 20, resize, u * W / W_, v * H / H_, [H,W,2]) where its padded size is 4 x the flow's
    if harness.padded_size(*dst) == (4 * src[0], 4 * src[1]):
        want = harness.postprocess(torch.from_numpy(flow[:1]), *dst).numpy()
        fu, fv = R.script_factors(dst, src)
        assert R.same_bits_nan_by_position(R.flow_exit(flow[:1], dst, 20.0, fu, fv, hwc=True)[0], want)


def test_harness_case_is_the_script_geometry():
    _, src, dst, _ = R.FLOW_CASES["harness"]
    assert harness.padded_size(*dst) == (4 * src[0], 4 * src[1])


def test_oracle_reproduces_the_hand_worked_vectors():
    u8 = lambda v: np.asarray(v, np.uint8)
    assert R.resize_u8(u8([[10, 20]]), (1, 4)).tolist() == [[10, 13, 18, 20]]
    assert R.resize_u8(u8([[0], [255]]), (3, 1)).tolist() == [[0], [128], [255]]
    assert R.resize_u8(u8([[0, 100, 200, 50]]), (1, 2)).tolist() == [[50, 125]]
    assert R.resize_f32(np.asarray([[1.0, 3.0]], np.float32), (1, 4)).tolist() == [[1.0, 1.5, 2.5, 3.0]]
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(R.resize_u8(a, (3, 4)), a)                             # weight 2048 is exact on bytes


def test_byte_lut_is_the_reference_division():
    v = np.arange(256)
    want = (v.astype(np.float64) / 255.0).astype(np.float32)                     # script_pwc.py:58, then .float()
    lut = cv_resize.byte_lut()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256)
    for c in range(3):
        assert np.array_equal(lut[c].numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(want, v.astype(np.float32) / np.float32(255))          # topview.py:94
    recip = v.astype(np.float32) * (np.float32(1) / np.float32(255))             # what t / 255.0 is on the device
    assert int((recip != want).sum()) == 126
    assert np.array_equal(cv_resize.byte_lut(R.IMAGENET_MEAN, R.IMAGENET_STD).numpy().view(np.int32),
                          R.byte_lut(R.IMAGENET_MEAN, R.IMAGENET_STD).view(np.int32))
    with pytest.raises(ValueError):
        cv_resize.byte_lut(mean=R.IMAGENET_MEAN)
    with pytest.raises(ValueError):
        cv_resize.byte_lut((0, 0, 0), (1, 0, 1))


@pytest.mark.parametrize("src,dst", [(13, 64), (517, 576), (38, 129), (5, 64), (1, 64), (64, 64), (40, 9), (5, 11), (1, 3), (48, 150),
                                     (436, 448), (1080, 1088)])
def test_axis_table_equals_the_scalar_loop(src, dst):
    s0, fx = cv_resize.axis_table(src, dst)
    w0, wf = R.axis_scalar(src, dst)
    assert s0.dtype == np.int32 and fx.dtype == np.float32
    assert np.array_equal(s0, w0) and np.array_equal(fx.view(np.int32), wf.view(np.int32))
    assert s0.min() >= 0 and s0.max() <= src - 1
    o0, _, of = R.axis(src, dst)
    assert np.array_equal(o0, w0) and np.array_equal(of.view(np.int32), wf.view(np.int32))
    with pytest.raises(ValueError):
        cv_resize.axis_table(0, dst)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = _lib.load()
    assert lib.pwc_abi_version() == _lib.ABI_VERSION == 13
    for name in NEW_SYMBOLS:
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M | re.S)
        assert decl, "%s is not declared in include/pwc_hip.h" % name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "pwc_cv_resize.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()


def test_wrappers_reject_host_tensors_and_wrong_shapes():
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    flow = torch.zeros((1, 2, 4, 4))
    tab = (torch.zeros(8, dtype=torch.int32), torch.zeros(8))
    lut = cv_resize.byte_lut()
    out = torch.zeros((1, 3, 8, 8))
    with pytest.raises(ValueError):
        ops.cv_resize_frames(frames, (8, 8), tab, tab, lut, out)                 # host tensors
    with pytest.raises(ValueError):
        ops.cv_resize_flow(flow, (8, 8), tab, tab)
    for call in (lambda: cv_resize.resize_frames(frames), lambda: cv_resize.resize_frames(frames.float()),
                 lambda: cv_resize.resize_frames(frames[0]), lambda: cv_resize.resize_frames(torch.zeros((1, 8, 8, 4), dtype=torch.uint8)),
                 lambda: cv_resize.ingest_pairs(frames), lambda: cv_resize.ingest_pairs(torch.zeros((1, 3, 8, 8, 3), dtype=torch.uint8)),
                 lambda: cv_resize.resize_flow(flow, (8, 8)), lambda: cv_resize.resize_flow(flow[:, :1], (8, 8)),
                 lambda: cv_resize.resize_flow(flow.double(), (8, 8)), lambda: cv_resize.resize_flow(flow, (8, 8), layout="cwh"),
                 lambda: cv_resize.CvGraphedInfer(None, 8, 8, "cpu", mode="kitti")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        harness.estimate_flow(None, frames[0], frames[0], prepost="cuda")


@pytest.mark.parametrize("name", sorted(R.TIE_CASES))
def test_tie_cases_tell_half_even_from_half_up(name):
    n, src, dst, seed = R.FRAME_CASES[name]
    frames = R.make_frames(n, src, seed)
    even = np.stack([R.resize_u8(f, dst) for f in frames])
    up = np.stack([R.resize_u8(f, dst, half_up=True) for f in frames])
    changed = int((even != up).sum())
    print("%s: %d of %d bytes change under half-up rounding" % (name, changed, even.size))
    assert changed == R.TIE_CASES[name] and changed > 0
    # the tie itself: a weight whose 11-bit product sits exactly on .5, on the axis the case names
    s, d = (src[1], dst[1]) if name == "tie_x" else (src[0], dst[0])
    _, _, f = R.axis(s, d)
    prod = np.concatenate([f * np.float32(2048), (np.float32(1) - f) * np.float32(2048)])
    assert bool((prod - np.floor(prod) == 0.5).any())
