"""CPU checks of the fused resize / score / encode path (csrc/pwc_pil_resize.hip pwc_pil_flow_eval, ops.pil_flow_eval,
pil_resize.eval_flow, opticalflow_amd/inference_eval.py): the NumPy oracle reproduces what the reference's own inference.py functions
recorded in the g22 fixture, the cases meet the conditions the GPU tests rely on, the C ABI is declared, bound, exported and refuses
bad arguments before any launch, and `evaluate` keeps its books."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from conftest import REPO, load_golden
import inference_eval_cases as C
import inference_eval_oracle as O
import pil_resize_oracle as R

NAMES = ("pwc_pil_flow_eval_workspace_bytes", "pwc_pil_flow_eval")
PWC_EINVAL, PWC_EALIGN = -1, -3
case = C.case


def fixture_arrays(z, name, pred, enc):
    """Compare the oracle's flow / encoded arrays with the fixture (arrays for the small cases, sha256 for the larger)."""
    if name + "/flow" in z:
        return np.array_equal(pred.view(np.int32), z[name + "/flow"].view(np.int32)), np.array_equal(enc, z[name + "/enc"])
    return (np.array_equal(R.digest_bytes(pred), z[name + "/flow_digest"]), np.array_equal(R.digest_bytes(enc), z[name + "/enc_digest"]))


@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_reproduces_reference(name):
    z = load_golden("g22_inference_eval.npz")
    flow, pred, gt, valid, m = case(name)
    same_flow, same_enc = fixture_arrays(z, name, pred, O.encode(pred, "reference"))
    assert same_flow, "the oracle's resize_flow differs from the reference's"
    assert same_enc, "the oracle's encoded array differs from the one the reference's save_flow builds"
    assert np.array_equal(m["n_valid"], z[name + "/n_valid"]) and np.array_equal(m["n_outlier"], z[name + "/n_outlier"])
    for b in range(len(m["n_valid"])):
        N = int(m["n_valid"][b])
        ours = m["sum_epe"][b] / N
        ref = z[name + "/epe"][b]
        # The reference's figure is NumPy's float32 mean of the SAME float32 addends (all positive): an addend passes through at most
        # 15 additions in one of the 8 lanes of a 128-element block, 3 to merge the lanes and ceil(log2(N / 128)) pairwise levels
        # above the blocks, then one division: (19 + levels) roundings of 2^-24 relative each.  Ours is their float64 sum, off by
        # less than N * 2^-53.  1.01 covers the second-order terms.
        levels = max(0, math.ceil(math.log2(N / 128.0))) if N > 128 else 0
        bound = 1.01 * (19 + levels) * 2.0 ** -24 + N * 2.0 ** -53
        print("%s[%d]: EPE oracle %.9g reference %.9g relative gap %.3g (bound %.3g)" % (name, b, ours, ref, abs(ours - ref) / ref, bound))
        assert abs(ours - ref) <= bound * ref
        # FL is a ratio of the exact counts
        assert z[name + "/fl"][b] == m["n_outlier"][b] / N * 100.0


@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_meet_their_conditions(name):
    flow, pred, gt, valid, m = case(name)
    epe, mag = m["epe"], m["mag"]
    # the predicate as inference.py writes it equals the kernel's fmaxf form, on every pixel
    assert np.array_equal(O.outliers_reference(epe, mag), O.outliers_fmax(epe, mag))
    # far inside the encodable range: no clamp is active in the fixture
    assert np.abs(pred).max() < 500 and np.abs(gt).max() <= 500
    ok = m["n_valid"] > 0
    assert ok.all()
    if name != "one_px":                         # one pixel is an outlier or it is not
        assert np.all((m["n_outlier"] > 0) & (m["n_outlier"] < m["n_valid"]))
    else:
        assert pred.shape[2:] == (1, 1)
    rel = int((O.relative_ruled(mag) & valid).sum())
    if name not in C.NO_RELATIVE:
        assert rel > 0
    # ground truth survives the PNG encoding exactly, in both orders
    for order in ("kitti", "reference"):
        g2, v2 = O.decode(C.gt_u16(gt, valid, order), order)
        assert np.array_equal(g2, gt) and np.array_equal(v2, valid)


def test_encoder_orders_and_clamp():
    p = np.array([-600.0, -512.0, -511.99, -0.01, 0.0, 0.0078125, 20.3, 511.98, 511.99, 512.0, 700.0, np.nan, np.inf, -np.inf], np.float32)
    pred = np.stack([p, p[::-1]])[None, :, None, :]                  # [1,2,1,14]
    ref, kit = O.encode(pred, "reference"), O.encode(pred, "kitti")
    want = np.array([0, 0, 0, 32767, 32768, 32768, 34067, 65534, 65535, 65535, 65535, 0, 65535, 0], np.uint16)
    assert np.array_equal(kit[0, 0, :, 0], want) and np.array_equal(kit[0, 0, :, 1], want[::-1]) and np.all(kit[..., 2] == 1)
    assert np.array_equal(ref[..., 0], kit[..., 2]) and np.array_equal(ref[..., 1], kit[..., 1]) and np.array_equal(ref[..., 2], kit[..., 0])
    # the module's host encoder is the same function
    from opticalflow_amd import inference_eval as IE
    for order in ("reference", "kitti"):
        assert np.array_equal(IE.encode_flow(pred[0].transpose(1, 2, 0), order), O.encode(pred, order)[0])
    # inside the range it agrees with kitti.encode_flow_rgb16 (which also clips)
    from opticalflow_amd import kitti
    flow, pr, gt, valid, m = case("tile_edges")
    assert np.array_equal(IE.encode_flow(pr[0].transpose(1, 2, 0), "kitti"), kitti.encode_flow_rgb16(pr[0].transpose(1, 2, 0)))


def test_host_metrics_match_the_fixture():
    from opticalflow_amd import inference_eval as IE
    z = load_golden("g22_inference_eval.npz")
    for name in ("tile_edges", "tall"):
        flow, pred, gt, valid, m = case(name)
        for b in range(pred.shape[0]):
            p = pred[b].transpose(1, 2, 0)
            assert IE.compute_epe(p, gt[b], valid[b]) == z[name + "/epe"][b]
            assert IE.compute_fl(p, gt[b], valid[b]) == z[name + "/fl"][b]
    none = np.zeros((3, 4), bool)
    assert IE.compute_epe(np.ones((3, 4, 2), np.float32), np.zeros((3, 4, 2), np.float32), none) == 0.0
    assert IE.compute_fl(np.ones((3, 4, 2), np.float32), np.zeros((3, 4, 2), np.float32), none) == 0.0
    assert IE.rows_from_totals([6.0, 0.0], [4, 0], [1, 0]) == [(1.5, 25.0), (0.0, 0.0)]


def test_symbols_declared_bound_exported():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define PWC_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13
    assert "pwc_pil_resize.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()
    import opticalflow_amd
    from opticalflow_amd import inference_eval, ops, pil_resize
    for n in ("pil_flow_eval", "pil_flow_eval_workspace_bytes"):
        assert hasattr(ops, n)
    assert hasattr(pil_resize, "eval_flow") and opticalflow_amd.eval_flow is pil_resize.eval_flow
    assert opticalflow_amd.inference_eval is inference_eval and opticalflow_amd.ResizedEval is inference_eval.ResizedEval
    assert pil_resize.FlowEval._fields == ("scores", "totals", "encoded", "flow")
    sig = inspect.signature(pil_resize.eval_flow)
    assert list(sig.parameters)[:8] == ["flow", "size", "gt", "valid", "gt_order", "encode", "keep_flow", "scale_vectors"]
    assert sig.parameters["gt_order"].default == "kitti" and sig.parameters["encode"].default is None
    sig = inspect.signature(inference_eval.evaluate)
    assert sig.parameters["image_size"].default == (384, 1280) and sig.parameters["batch"].default == 16
    assert sig.parameters["order"].default == "reference" and sig.parameters["output_dir"].default is None


def test_workspace_bytes_formula():
    from opticalflow_amd import _lib
    lib = _lib.load()
    # 24 bytes {fp64 sum, int64 valid, int64 outliers} per sample in front, then per 16 x 64 tile: pwc_kitti_score's layout
    assert lib.pwc_pil_flow_eval_workspace_bytes(1, 16, 64) == 24 * (1 + 1)
    assert lib.pwc_pil_flow_eval_workspace_bytes(2, 17, 65) == 24 * 2 * (1 + 4)
    assert lib.pwc_pil_flow_eval_workspace_bytes(16, 375, 1242) == 24 * 16 * (1 + 24 * 20)
    assert lib.pwc_pil_flow_eval_workspace_bytes(3, 94, 311) == 24 * 3 * (1 + 6 * 5)
    for shape in ((1, 16, 64), (3, 94, 311), (16, 375, 1242)):
        assert lib.pwc_pil_flow_eval_workspace_bytes(*shape) == lib.pwc_kitti_score_workspace_bytes(*shape)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.pwc_pil_flow_eval_workspace_bytes(*bad) == -1


def test_abi_argument_errors_without_gpu():
    """Argument validation happens before any launch, so it can be checked without a device (the pointers are never dereferenced)."""
    from opticalflow_amd import _lib
    from opticalflow_amd.pil_resize import ksize
    lib = _lib.load()
    P = 1 << 20                                                  # a 16-byte aligned stand-in address
    n, h, w, H, W = 2, 24, 80, 94, 311
    need = lib.pwc_pil_flow_eval_workspace_bytes(n, H, W)

    def call(src=P, n=n, h=h, w=w, H=H, W=W, xb=P, xk=P, xks=None, yb=P, yk=P, yks=None, fac=P, bss=None, gt=P, kind=1, valid=None,
             flow_out=None, enc_out=None, order=0, ws=P, ws_bytes=need, out=P):
        xks = ksize(max(w, 1), max(W, 1)) if xks is None else xks
        yks = ksize(max(h, 1), max(H, 1)) if yks is None else yks
        bss = 2 * h * w if bss is None else bss
        rc = lib.pwc_pil_flow_eval(src, n, h, w, H, W, xb, xk, xks, yb, yk, yks, fac, bss, gt, kind, valid, flow_out, enc_out, order, ws,
                                   ws_bytes, out, None)
        return rc, lib.pwc_last_error().decode()

    for kw in (dict(src=None), dict(xb=None), dict(xk=None), dict(yb=None), dict(yk=None)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "null pointer" in msg, (kw, rc, msg)
    rc, msg = call(gt=None)
    assert rc == PWC_EINVAL and "nothing requested" in msg
    for kw in (dict(ws=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "needs workspace and out" in msg, (kw, rc, msg)
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=0)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "bad shape" in msg, (kw, rc, msg)
    rc, msg = call(h=9 * H + 8, bss=2 * (9 * H + 8) * w)          # a downscale beyond 8 to more than a tile of rows
    assert rc == PWC_EINVAL and "supported scale range" in msg
    for kw in (dict(xks=5), dict(yks=5)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "ksize" in msg, (kw, rc, msg)
    rc, msg = call(bss=2 * h * w - 1)
    assert rc == PWC_EINVAL and "batch stride" in msg
    for kind in (3, -1):
        rc, msg = call(kind=kind)
        assert rc == PWC_EINVAL and "gt_kind" in msg
    for order in (2, -1):
        rc, msg = call(enc_out=P, order=order)
        assert rc == PWC_EINVAL and "enc_order" in msg
    for kw in (dict(kind=1, valid=P), dict(kind=2, valid=P), dict(gt=None, enc_out=P, valid=P)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "valid must be NULL" in msg, (kw, rc, msg)
    big = lib.pwc_pil_flow_eval_workspace_bytes(65536, H, W)
    rc, msg = call(n=65536, ws_bytes=big)
    assert rc == PWC_EINVAL and "65535" in msg
    rc, msg = call(ws_bytes=need - 1)
    assert rc == PWC_EINVAL and "workspace needs %d bytes" % need in msg
    rc, msg = call(ws=P + 4)
    assert rc == PWC_EALIGN and "8-byte aligned" in msg
    for kw in (dict(src=P + 2), dict(xb=P + 2), dict(yb=P + 2), dict(fac=P + 2), dict(xk=P + 4), dict(yk=P + 4), dict(out=P + 2),
               dict(flow_out=P + 2), dict(enc_out=P + 1), dict(gt=P + 1, kind=1), dict(gt=P + 1, kind=2), dict(gt=P + 2, kind=0)):
        rc, msg = call(**kw)
        assert rc == PWC_EALIGN and "aligned" in msg, (kw, rc, msg)


class FakePipe:
    """Stands in for ResizedEval in `evaluate`: records what it is fed and reports totals derived from the frames' first byte."""
    made = []

    def __init__(self, model, in_hw, image_size, device, batch=1, gt=None, encode=None, rows=0):
        self.in_hw, self.image_size, self.batch, self.gt_form, self.encode, self.rows = tuple(in_hw), tuple(image_size), batch, gt, encode, rows
        self.fed, self.totals, self.last = [], {}, None
        FakePipe.made.append(self)

    def feed(self, f1, f2, gts, row0):
        assert len(f1) == len(f2) <= self.batch and (gts is None) == (self.gt_form is None)
        assert all(tuple(f.shape[:2]) == self.in_hw for f in f1)
        self.fed.append((row0, [int(f[0, 0, 0]) for f in f1]))
        self.last = [int(f[0, 0, 0]) for f in f1]
        for j, tag in enumerate(self.last):
            nv = 0 if tag == 7 else 4                            # sample 7 has no valid pixel
            self.totals[row0 + j] = (float(tag) * nv, nv, 1 if nv else 0)

    def download_encoded(self, n):
        assert n == len(self.last) and self.encode is not None
        H, W = self.in_hw
        return np.stack([np.full((H, W, 3), tag, np.uint16) for tag in self.last])

    def results(self, rows):
        assert rows == self.rows == len(self.totals)
        t = [self.totals[i] for i in range(rows)]
        return (np.array([r[0] for r in t]), np.array([r[1] for r in t], np.float64), np.array([r[2] for r in t], np.float64))


def test_evaluate_bookkeeping(tmp_path):
    from opticalflow_amd import inference_eval as IE
    from opticalflow_amd import kitti

    def img(tag, hw):
        return np.full(hw + (3,), tag, np.uint8)
    A, B = (5, 7), (6, 4)
    gtA, gtB = np.zeros(A + (3,), np.uint16), np.zeros(B + (3,), np.uint16)
    #          tag  size  ground truth
    spec = [(1, A, gtA), (2, B, gtB), (3, A, None), (4, A, gtA), (7, B, gtB), (5, A, gtA), (6, A, gtA)]
    samples = [(img(t, hw), img(t, hw), g, "%06d_10.png" % t) for t, hw, g in spec]
    FakePipe.made = []
    res = IE.evaluate(None, samples, image_size=(64, 128), batch=3, output_dir=str(tmp_path), order="reference", device="cpu",
                      make_pipeline=FakePipe)
    # one pipeline per (size, ground-truth form); batches of at most `batch`; rows counted per pipeline
    got = {(p.in_hw, p.gt_form): p for p in FakePipe.made}
    assert set(got) == {(A, "reference"), (B, "reference"), (A, None)}
    assert got[(A, "reference")].fed == [(0, [1, 4, 5]), (3, [6])] and got[(A, "reference")].batch == 3
    assert got[(B, "reference")].fed == [(0, [2, 7])] and got[(B, "reference")].batch == 2
    assert got[(A, None)].fed == [(0, [3])]
    assert all(p.image_size == (64, 128) and p.encode == "reference" for p in FakePipe.made)
    # rows in input order; no ground truth -> None; no valid pixel -> (0.0, 0.0), counted
    assert res["rows"] == [(1.0, 25.0), (2.0, 25.0), None, (4.0, 25.0), (0.0, 0.0), (5.0, 25.0), (6.0, 25.0)]
    assert res["num_samples"] == 6 and res["EPE"] == pytest.approx((1 + 2 + 4 + 0 + 5 + 6) / 6.0) and res["FL"] == pytest.approx(125.0 / 6.0)
    # every sample written under the reference's name rule, with its own contents
    for t, hw, _ in spec:
        back = kitti.read_png16_rgb(str(tmp_path / ("%06d_10_flow.png" % t)))
        assert back.shape == hw + (3,) and np.all(back == t)
    # without output_dir a sample without ground truth is not run, and nothing is encoded
    FakePipe.made = []
    res = IE.evaluate(None, samples[:4], image_size=(64, 128), batch=16, device="cpu", make_pipeline=FakePipe)
    assert {(p.in_hw, p.gt_form, p.encode, p.batch) for p in FakePipe.made} == {(A, "reference", None, 2), (B, "reference", None, 1)}
    assert res["rows"][2] is None and res["num_samples"] == 3
    # nothing scored: the three keys are absent, as in the reference
    FakePipe.made = []
    res = IE.evaluate(None, [samples[2]], output_dir=str(tmp_path / "only"), device="cpu", make_pipeline=FakePipe, order="kitti")
    assert res == {"rows": [None]} and FakePipe.made[0].encode == "kitti"
    # the float form is its own group
    FakePipe.made = []
    fl = (np.zeros(A + (2,), np.float32), np.ones(A, bool))
    IE.evaluate(None, [samples[0], (img(9, A), img(9, A), fl, "x.png")], device="cpu", make_pipeline=FakePipe)
    assert {p.gt_form for p in FakePipe.made} == {"reference", "float"}


def test_save_flow_writes_a_readable_file(tmp_path):
    from opticalflow_amd import inference_eval as IE
    from opticalflow_amd import kitti
    flow, pred, gt, valid, m = case("tile_edges")
    f = np.ascontiguousarray(pred[0].transpose(1, 2, 0))
    assert IE.flow_filename("000012_10.png") == "000012_10_flow.png" and IE.flow_filename("a.png") == "a.png"
    path = IE.save_flow(f, str(tmp_path / "out"), "000012_10.png")
    assert path.endswith("000012_10_flow.png")
    back = kitti.read_png16_rgb(path)
    assert np.array_equal(back, O.encode(pred[:1], "reference")[0])
    # an encoded array is written as it is; in the devkit's order the project's own decoder reads it
    path = IE.save_flow(O.encode(pred[:1], "kitti")[0], str(tmp_path / "out"), "k_10.png", order="kitti")
    dec, ok = kitti.load_flow_kitti_png(path)
    assert ok.all() and np.abs(dec - f).max() <= 1.0 / 64
    with pytest.raises(ValueError):
        IE.encode_flow(f, "rgb")
