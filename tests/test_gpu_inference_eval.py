"""GPU checks of the fused resize / score / encode kernel (pwc_pil_flow_eval) and the evaluation pipeline on top of it
(pil_resize.eval_flow, inference_eval.ResizedEval / evaluate) against the g22 fixture, which holds what the reference's own
inference.py functions computed, and against tests/inference_eval_oracle.py."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import inference_eval_cases as C
import inference_eval_oracle as O
import pil_resize_oracle as R

from opticalflow_amd import inference_eval as IE
from opticalflow_amd import kitti, pil_resize

pytestmark = pytest.mark.gpu
CANARY16, CANARY32 = 0xABCD, 7.0


@pytest.fixture(scope="module")
def golden():
    return load_golden("g22_inference_eval.npz")


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _totals(t):
    """int64 [n,3] device totals -> (sum_epe float64 [n], n_valid int64 [n], n_outlier int64 [n]) on the host (copies: the device
    tensor is a view of a cached workspace)."""
    a = t.cpu().numpy().copy()
    return a[:, 0].copy().view(np.float64), a[:, 1], a[:, 2]


def _inputs(name, device, order="kitti"):
    flow, pred, gt, valid, m = C.case(name)
    return _dev(flow, device), _dev(C.gt_u16(gt, valid, order), device)


def _check_scores(got, m):
    """Totals and scores of one call against the oracle's `score` dict: counts exact, the sum within n_valid * 2^-53 relative (the
    addends are the same float32 values, only the order of the float64 additions differs), scores the float32 of the totals."""
    s, nv, no = _totals(got.totals)
    assert np.array_equal(nv, m["n_valid"]), "valid counts %s, reference %s" % (nv, m["n_valid"])
    assert np.array_equal(no, m["n_outlier"]), "outlier counts %s, reference %s" % (no, m["n_outlier"])
    gap = np.abs(s - m["sum_epe"])
    print("sum_epe %s oracle %s gap %s" % (s, m["sum_epe"], gap))
    assert np.all(gap <= m["n_valid"] * 2.0 ** -53 * m["sum_epe"])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.stack([(s / nv).astype(np.float32), (100.0 * no / nv).astype(np.float32)], axis=1)
    want[nv == 0] = np.nan
    sc = got.scores.cpu().numpy()
    assert np.array_equal(np.isnan(sc), np.isnan(want)) and np.array_equal(_bits(np.nan_to_num(sc)), _bits(np.nan_to_num(want)))


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_matches_the_reference(gpu_device, golden, name):
    B, hw, HW, _ = C.CASES[name]
    flow, pred, gt, valid, m = C.case(name)
    assert pil_resize.vertical_first(hw, HW) == (name == "tall")
    x, g = _inputs(name, gpu_device)
    got = pil_resize.eval_flow(x, HW, gt=g, encode="reference", keep_flow=True)
    assert tuple(got.flow.shape) == (B, 2) + HW and tuple(got.encoded.shape) == (B,) + HW + (3,) and got.encoded.dtype == torch.uint16
    _check_scores(got, m)
    f, e = got.flow.cpu().numpy(), got.encoded.cpu().numpy()
    if name + "/flow" in golden:
        assert np.array_equal(_bits(f), _bits(golden[name + "/flow"])), "%d flow values differ from the reference's" % int((_bits(f) != _bits(golden[name + "/flow"])).sum())
        assert np.array_equal(e, golden[name + "/enc"])
    else:
        assert np.array_equal(R.digest_bytes(f), golden[name + "/flow_digest"]) and np.array_equal(R.digest_bytes(e), golden[name + "/enc_digest"])
    # counts against the reference's own, with no pixel left out
    assert np.array_equal(_totals(got.totals)[1], golden[name + "/n_valid"]) and np.array_equal(_totals(got.totals)[2], golden[name + "/n_outlier"])
    # the parent's resize_flow gives the same bits
    assert np.array_equal(_bits(f), _bits(pil_resize.resize_flow(x, HW)))
    # the devkit's order
    kit = pil_resize.eval_flow(x, HW, encode="kitti")
    assert kit.scores is None and kit.totals is None and kit.flow is None
    assert np.array_equal(kit.encoded.cpu().numpy(), O.encode(pred, "kitti"))


@pytest.mark.parametrize("name", ["tile_edges", "down", "identity", "kitti_like", "tall"])
def test_variants_agree_and_runs_repeat(gpu_device, name):
    _, _, HW, _ = C.CASES[name]
    x, g = _inputs(name, gpu_device)
    full = pil_resize.eval_flow(x, HW, gt=g, encode="reference", keep_flow=True)
    t_full, s_full = full.totals.cpu().numpy().copy(), _bits(full.scores).copy()
    score = pil_resize.eval_flow(x, HW, gt=g)
    assert score.encoded is None and score.flow is None
    assert np.array_equal(score.totals.cpu().numpy(), t_full) and np.array_equal(_bits(score.scores), s_full)
    enc = pil_resize.eval_flow(x, HW, encode="reference")
    assert np.array_equal(enc.encoded.cpu().numpy(), full.encoded.cpu().numpy())
    both = pil_resize.eval_flow(x, HW, gt=g, encode="reference")
    assert np.array_equal(both.totals.cpu().numpy(), t_full) and np.array_equal(both.encoded.cpu().numpy(), full.encoded.cpu().numpy())
    again = pil_resize.eval_flow(x, HW, gt=g, encode="reference", keep_flow=True)
    assert np.array_equal(again.totals.cpu().numpy(), t_full) and np.array_equal(_bits(again.scores), s_full)
    assert np.array_equal(_bits(again.flow), _bits(full.flow)) and np.array_equal(again.encoded.cpu().numpy(), full.encoded.cpu().numpy())


@pytest.mark.parametrize("name", ["tile_edges", "kitti_like"])
def test_ground_truth_forms_agree(gpu_device, name):
    _, _, HW, _ = C.CASES[name]
    flow, pred, gt, valid, m = C.case(name)
    x, gk = _inputs(name, gpu_device, "kitti")
    _, gr = _inputs(name, gpu_device, "reference")
    gf = _dev(gt.transpose(0, 3, 1, 2), gpu_device)
    a = pil_resize.eval_flow(x, HW, gt=gk).totals.cpu().numpy().copy()
    b = pil_resize.eval_flow(x, HW, gt=gr, gt_order="reference").totals.cpu().numpy().copy()
    c = pil_resize.eval_flow(x, HW, gt=gf, valid=_dev(valid, gpu_device)).totals.cpu().numpy().copy()
    d = pil_resize.eval_flow(x, HW, gt=gf, valid=_dev(valid.astype(np.uint8) * 200, gpu_device)).totals.cpu().numpy().copy()
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    # the wrong order is a different (and wrong) reading of the same samples
    assert not np.array_equal(a, pil_resize.eval_flow(x, HW, gt=gr, gt_order="kitti").totals.cpu().numpy())
    # valid=None: every pixel counts
    _check_scores(pil_resize.eval_flow(x, HW, gt=gf), O.score(pred, gt, None))
    with pytest.raises(ValueError):
        pil_resize.eval_flow(x, HW, gt=gk, valid=_dev(valid, gpu_device))
    with pytest.raises(ValueError):
        pil_resize.eval_flow(x, HW)


def test_sample_without_a_valid_pixel(gpu_device):
    name = "tile_edges"
    _, _, HW, _ = C.CASES[name]
    flow, pred, gt, valid, m = C.case(name)
    v = valid.copy()
    v[1] = False
    got = pil_resize.eval_flow(_dev(flow, gpu_device), HW, gt=_dev(C.gt_u16(gt, v, "kitti"), gpu_device))
    _check_scores(got, O.score(pred, gt, v))
    s, nv, no = _totals(got.totals)
    sc = got.scores.cpu().numpy()
    assert nv[1] == 0 and no[1] == 0 and s[1] == 0.0 and np.isnan(sc[1]).all() and nv[0] == m["n_valid"][0] and not np.isnan(sc[0]).any()
    assert IE.rows_from_totals(s, nv, no)[1] == (0.0, 0.0)


def test_prediction_beyond_the_encodable_range_clamps(gpu_device):
    name = "tile_edges"
    _, _, HW, _ = C.CASES[name]
    flow = C.make_flow(name) * np.float32(9.0)                     # +-180 px before the x3.25 / x2.8 rescale: beyond +-512
    flow[0, 0, 0, 0] = np.nan
    pred = O.predict(flow, HW)
    assert np.nanmax(pred[:, 0]) > 520 and np.nanmin(pred[:, 1]) < -500 and np.isnan(pred).any()
    for order in ("reference", "kitti"):
        got = pil_resize.eval_flow(_dev(flow, gpu_device), HW, encode=order, keep_flow=True)
        f = got.flow.cpu().numpy()
        assert np.array_equal(np.isnan(f), np.isnan(pred)) and np.array_equal(_bits(np.nan_to_num(f)), _bits(np.nan_to_num(pred)))
        e = got.encoded.cpu().numpy()
        assert np.array_equal(e, O.encode(pred, order))
        assert (e == 65535).any() and (e == 0).any()


def test_captured_replay_equals_eager(gpu_device):
    name = "kitti_like"
    B, hw, HW, _ = C.CASES[name]
    x, g = _inputs(name, gpu_device)
    eager = pil_resize.eval_flow(x, HW, gt=g, encode="reference", keep_flow=True)          # also makes the tables resident
    want = (eager.totals.cpu().numpy().copy(), _bits(eager.scores).copy(), eager.encoded.cpu().numpy(), _bits(eager.flow).copy())
    xs, gs = torch.zeros_like(x), g.clone()
    enc = _dev(np.zeros((B,) + HW + (3,), np.uint16), gpu_device)
    fl = torch.zeros((B, 2) + HW, dtype=torch.float32, device=gpu_device)
    sc = torch.zeros((B, 2), dtype=torch.float32, device=gpu_device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pil_resize.eval_flow(xs, HW, gt=gs, encode="reference", keep_flow=True, encoded_out=enc, flow_out=fl, scores_out=sc)
    assert got.encoded is enc and got.flow is fl and got.scores is sc
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(got.totals.cpu().numpy(), want[0]) and np.array_equal(_bits(sc), want[1])
    assert np.array_equal(enc.cpu().numpy(), want[2]) and np.array_equal(_bits(fl), want[3])
    # new contents of the captured inputs, same graph
    flow, pred, gt, valid, m = C.case(name)
    xs.copy_(_dev(flow[::-1], gpu_device))
    gs.copy_(_dev(C.gt_u16(gt, valid, "kitti")[::-1], gpu_device))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(got.totals.cpu().numpy(), want[0][::-1]) and np.array_equal(_bits(fl), want[3][::-1])


def test_misaligned_views_and_canaries(gpu_device):
    name = "tile_edges"                                            # W = 65: rows of the uint16 arrays are 2-byte aligned at best
    B, (h, w), HW, _ = C.CASES[name]
    flow, pred, gt, valid, m = C.case(name)
    N = B * HW[0] * HW[1]
    pool = torch.full(((B + 1) * 3 * h * w + 1,), 99.0, dtype=torch.float32, device=gpu_device)
    big = pool[1:].view(B + 1, 3, h, w)[1:]                        # a batch slice of a larger tensor that starts one float in
    big[:, :2] = _dev(flow, gpu_device)
    x = big[:, :2]                                                 # ... and of it a channel slice: batch stride 3 h w
    assert x.data_ptr() % 16 == 4
    gbuf = _dev(np.concatenate([[CANARY16], C.gt_u16(gt, valid, "reference").reshape(-1), [CANARY16]]).astype(np.uint16), gpu_device)
    g = gbuf[1:-1].view(B, HW[0], HW[1], 3)                        # starts one element in: 2-byte aligned only
    ebuf = _dev(np.full(3 * N + 2, CANARY16, np.uint16), gpu_device)
    enc = ebuf[1:-1].view(B, HW[0], HW[1], 3)
    fbuf = torch.full((2 * N + 2,), CANARY32, dtype=torch.float32, device=gpu_device)
    fl = fbuf[1:-1].view(B, 2, HW[0], HW[1])
    sbuf = torch.full((2 * B + 2,), CANARY32, dtype=torch.float32, device=gpu_device)
    sc = sbuf[1:-1].view(B, 2)
    assert g.data_ptr() % 4 == 2 and enc.data_ptr() % 4 == 2 and fl.data_ptr() % 16 == 4
    got = pil_resize.eval_flow(x, HW, gt=g, gt_order="reference", encode="kitti", keep_flow=True, encoded_out=enc, flow_out=fl, scores_out=sc)
    _check_scores(got, m)
    assert np.array_equal(_bits(fl), _bits(pred)) and np.array_equal(enc.cpu().numpy(), O.encode(pred, "kitti"))
    e, f, s = ebuf.cpu().numpy(), fbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert e[0] == CANARY16 and e[-1] == CANARY16 and f[0] == CANARY32 and f[-1] == CANARY32 and s[0] == CANARY32 and s[-1] == CANARY32
    assert bool((big[:, 2] == 99.0).all().item()) and np.array_equal(_bits(big[:, :2]), _bits(flow))
    assert bool((pool[:1 + 3 * h * w] == 99.0).all().item())
    assert gbuf.cpu().numpy()[0] == CANARY16 and gbuf.cpu().numpy()[-1] == CANARY16


@pytest.mark.parametrize("name", ["tile_edges", "kitti_like"])
def test_encode_then_score_round_trip(gpu_device, name):
    B, _, HW, _ = C.CASES[name]
    x, _ = _inputs(name, gpu_device)
    enc = pil_resize.eval_flow(x, HW, encode="reference").encoded
    got = pil_resize.eval_flow(x, HW, gt=enc, gt_order="reference")
    s, nv, no = _totals(got.totals)
    # truncation loses less than 1/64 px per component
    assert np.all(nv == HW[0] * HW[1]) and np.all(no == 0) and np.all(s / nv <= np.sqrt(2.0) / 64.0) and np.all(s > 0)


# ------------------------------------------------------------------ the pipeline
SIZE = (128, 320)                                                  # the smallest network input test_gpu_pil_resize.py runs
ORIG = ((94, 311), (90, 300))


@pytest.fixture(scope="module")
def net(gpu_device):
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet()
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    return net.to(gpu_device).eval()


def _pairs_and_gt(net, hw, seed, device, empty=None):
    """Two frame pairs of one original size, infer_resized's flow for them (the parent's path, batch 2) and a seeded ground truth
    around it: (f1, f2 uint8 [2,H,W,3] host, want float32 [2,2,H,W], gt float32 [2,H,W,2], valid bool [2,H,W])."""
    f1, f2 = R.make_frames(2, hw, seed), R.make_frames(2, hw, seed + 1)
    want = pil_resize.infer_resized(net, _dev(f1, device), _dev(f2, device), SIZE).cpu().numpy()
    assert np.isfinite(want).all()
    rng = np.random.RandomState(seed + 2)
    gt = want.transpose(0, 2, 3, 1).astype(np.float64) + rng.randn(2, hw[0], hw[1], 2) * 2.0
    gt = (np.round(np.clip(gt, -500.0, 500.0) * 64.0) / 64.0).astype(np.float32)
    valid = rng.rand(2, hw[0], hw[1]) < 0.7
    if empty is not None:
        valid[empty] = False
    return f1, f2, want, gt, valid


def _host_rows(want, gt, valid):
    return [(IE.compute_epe(want[b].transpose(1, 2, 0), gt[b], valid[b]), IE.compute_fl(want[b].transpose(1, 2, 0), gt[b], valid[b]))
            for b in range(want.shape[0])]


def _close_rows(got, want):
    assert len(got) == len(want)
    for (e, f), (we, wf) in zip(got, want):
        # FL: a ratio of the same integer counts (one count apart would be >= 100 / n_valid); EPE: the host's float32 mean against the
        # fp64 sum of the same addends -- (19 + log2(N / 128)) * 2^-24 as in test_inference_eval_cpu.py, 2e-6 for these sizes
        assert f == pytest.approx(wf, rel=1e-12, abs=0) and e == pytest.approx(we, rel=2e-6, abs=0)


def test_resized_eval_equals_infer_resized_and_host_scoring(gpu_device, net):
    hw = ORIG[0]
    f1, f2, want, gt, valid = _pairs_and_gt(net, hw, 2301, gpu_device)
    pipe = IE.ResizedEval(net, hw, SIZE, gpu_device, batch=2, gt="kitti", encode="kitti", keep_flow=True, rows=4)
    got = pipe(_dev(f1, gpu_device), _dev(f2, gpu_device), _dev(C.gt_u16(gt, valid, "kitti"), gpu_device), row0=2)
    assert np.array_equal(_bits(got.flow), _bits(want)), "the captured pipeline's flow differs from infer_resized's"
    assert np.array_equal(got.encoded.cpu().numpy(), O.encode(want, "kitti"))
    _check_scores(got, O.score(want, gt, valid))
    s, nv, no = pipe.results(4)
    assert np.all(nv[:2] == 0) and np.array_equal(nv[2:], valid.reshape(2, -1).sum(1))
    _close_rows(IE.rows_from_totals(s[2:], nv[2:], no[2:]), _host_rows(want, gt, valid))
    # host data through the pinned ring, one pair only: rows land where asked
    got = pipe.feed([f1[1]], [f2[1]], [C.gt_u16(gt, valid, "kitti")[1]], row0=0)
    assert np.array_equal(_bits(got.flow), _bits(want[1:]))
    s, nv, no = pipe.results(1)
    assert nv[0] == valid[1].sum()


def test_evaluate_two_sizes_against_the_parent_path(gpu_device, net, tmp_path):
    A = _pairs_and_gt(net, ORIG[0], 2311, gpu_device)
    B = _pairs_and_gt(net, ORIG[1], 2321, gpu_device, empty=1)     # its second sample has no valid pixel
    samples, want_rows, want_files = [], [], []
    for j in range(2):                                             # sizes interleaved: A0 B0 A1 B1
        for tag, (f1, f2, want, gt, valid) in (("a", A), ("b", B)):
            samples.append((f1[j], f2[j], C.gt_u16(gt, valid, "reference")[j], "%s%d_10.png" % (tag, j)))
            want_rows.append(_host_rows(want[j:j + 1], gt[j:j + 1], valid[j:j + 1])[0])
            want_files.append(("%s%d_10_flow.png" % (tag, j), IE.encode_flow(want[j].transpose(1, 2, 0), "reference")))
    res = IE.evaluate(net, samples, image_size=SIZE, batch=2, output_dir=str(tmp_path), order="reference", device=gpu_device)
    assert res["num_samples"] == 4 and len(res["rows"]) == 4
    _close_rows(res["rows"], want_rows)
    assert res["rows"][3] == (0.0, 0.0) and want_rows[3] == (0.0, 0.0)
    assert res["EPE"] == pytest.approx(np.mean([r[0] for r in want_rows]), rel=2e-6) and res["FL"] == pytest.approx(np.mean([r[1] for r in want_rows]), rel=1e-12)
    for fname, enc in want_files:
        assert np.array_equal(kitti.read_png16_rgb(str(tmp_path / fname)), enc), fname
