"""GPU checks of the vanishing point (csrc/pwc_vanishing.hip, opticalflow_amd/vanishing.py) against the NumPy oracle on the cases of
tests/golden/g16_vanishing.npz, whose results are the reference's own (tests/test_vanishing_cpu.py ties the oracle to them).

How a result is compared.  hipcc's fp64 hypot and math.hypot may differ in the last place and everything downstream inherits that,
so nothing here asks for the host chain's bits:
  * status, N used, pairs kept, best bin and inlier count must be EQUAL: the fixture's margin conditions (asserted for every case by
    the CPU test) keep each of them away from its decision boundary;
  * centre: relative 1e-12 (the same edge formula on both sides);
  * prob: relative 1e-6 (fixed-point weights: 2^-41 of a normalised weight >= 1e-4, see the kernel's header);
  * refined xy: 1e3 * cond(A_in)^2 * 2^-53 * max(1, |vx|, |vy|), cond from the oracle's SVD; the observed error is printed.
Observed on MI355X (relative centre / relative prob / xy error as a fraction of its tolerance): see DESIGN.md section 22."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vanishing_oracle as VO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_vanishing.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def expected(gold):
    """The oracle on every case, computed once and shared."""
    out = {}
    for name, c in VO.CASES.items():
        idx = gold["idx/" + name] if gold["idx/" + name].size else None
        out[name] = VO.estimate(gold["vec/" + name], c["frame"], c["step"], c["min_mag"], c["max_points"], c["grid_size"], c["min_pairs"],
                                idx=idx)
    return out


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _kw(case):
    c = VO.CASES[case]
    return dict(step=c["step"], min_mag=c["min_mag"], max_points=c["max_points"], grid_size=c["grid_size"], min_pairs=c["min_pairs"])


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _compare(case, r, xy, prob, center, info):
    """One frame of a device result (host values) against the oracle's record r."""
    status, n_used, pairs, bx, by, inl = (int(v) for v in info)
    want = (r["status"], r["n_used"], r["pairs_kept"] if r["status"] != 2 else 0, r["best"][0], r["best"][1], r["inliers"])
    assert (status, n_used, pairs, bx, by, inl) == want, (case, (status, n_used, pairs, bx, by, inl), want)
    if r["status"] >= 2:
        assert np.isnan(xy).all() and np.isnan(center).all() and prob == 0.0
        return
    ec = max(_rel(center[0], r["center"][0]), _rel(center[1], r["center"][1]))
    ep = _rel(prob, r["prob"])
    tol = VO.xy_tolerance(r)
    exy = max(abs(xy[0] - r["xy"][0]), abs(xy[1] - r["xy"][1]))
    print("case %s: centre rel %.2e, prob rel %.2e, xy error %.3e of tolerance %.3e (cond %.3f)" % (case, ec, ep, exy, tol, r["cond"] or 0))
    assert ec <= 1e-12 and ep <= 1e-6 and exy <= tol
    if case in VO.EXACT_EDGE_CASES:
        assert prob == r["prob"] or ep <= 2.0 ** -50            # weights are exactly 1: only the 1e-9 term's scaling rounds


def _vec(gold, case, dev):
    return torch.from_numpy(gold["vec/" + case]).unsqueeze(0).to(dev)


@pytest.mark.parametrize("case", sorted(VO.CASES))
def test_every_case_singly(gold, expected, dev, case):
    from opticalflow_amd import ops, vanishing
    c, r = VO.CASES[case], expected[case]
    vec = _vec(gold, case, dev)
    if gold["idx/" + case].size:                                 # the subsample: the order table that reproduces the recorded draw
        order = torch.from_numpy(VO.order_from_idx(r["keep"], gold["idx/" + case])).to(dev)
        vp, info = ops.vanishing_point(vec, c["frame"][0], c["frame"][1], c["step"], c["min_mag"], c["max_points"], c["grid_size"],
                                       c["min_pairs"], order=order)
        got = vanishing.VanishingPoints(vp[:, 0:2], vp[:, 2], vp[:, 3:5], info)
    else:
        got = vanishing.vanishing_point(vec, c["frame"], **_kw(case))
    assert got.xy.dtype == torch.float64 and got.info.dtype == torch.int32 and tuple(got.info.shape) == (1, 6) and got.xy.is_cuda
    assert got.ok.tolist() == [r["status"] <= 1]
    _compare(case, r, got.xy[0].cpu().numpy(), float(got.prob[0]), got.center[0].cpu().numpy(), got.info[0].cpu().numpy())
    host = vanishing.to_host(got)
    assert len(host) == 1 and ((host[0] is None) == (r["status"] >= 2))
    if host[0] is not None:
        assert host[0] == (float(got.xy[0, 0]), float(got.xy[0, 1]), float(got.prob[0]))


@pytest.mark.parametrize("grid", [65, 128])
def test_grid_above_64_votes_into_the_global_histogram(gold, dev, grid):
    """A pair workgroup keeps its votes in LDS up to a 64 x 64 grid and adds them to the frame's histogram directly above it: the
    first size past that threshold (odd, so the edges are not round numbers) and the largest.  No reference value is recorded at these
    grid sizes, so the oracle is the reference and the margin conditions are asserted here, on the oracle's values."""
    from opticalflow_amd import vanishing
    for case in ("a", "b"):
        c = VO.CASES[case]
        kw = dict(_kw(case), grid_size=grid)
        r = VO.estimate(gold["vec/" + case], c["frame"], c["step"], c["min_mag"], c["max_points"], grid, c["min_pairs"])
        m = VO.margins(r, case)
        assert r["status"] == 0 and all(m.values()), [k for k, v in m.items() if not v]
        got = vanishing.vanishing_point(_vec(gold, case, dev), c["frame"], **kw)
        _compare("%s/grid%d" % (case, grid), r, got.xy[0].cpu().numpy(), float(got.prob[0]), got.center[0].cpu().numpy(),
                 got.info[0].cpu().numpy())


def test_batch_with_failing_frames_between_good_ones(gold, expected, dev):
    from opticalflow_amd import vanishing
    names = VO.BATCH_CASES
    vec = torch.cat([_vec(gold, n, dev) for n in names], 0).contiguous()
    got = vanishing.vanishing_point(vec, VO.CASES[names[0]]["frame"], **_kw(names[0]))
    xy, prob, center, info = got.xy.cpu().numpy(), got.prob.cpu().numpy(), got.center.cpu().numpy(), got.info.cpu().numpy()
    assert got.ok.tolist() == [expected[n]["status"] <= 1 for n in names] == [True, False, True, False]
    for b, n in enumerate(names):
        _compare(n, expected[n], xy[b], float(prob[b]), center[b], info[b])
        single = vanishing.vanishing_point(vec[b:b + 1].clone(), VO.CASES[n]["frame"], **_kw(n))
        assert torch.equal(single.info[0], got.info[b]) and torch.equal(single.xy.view(torch.int64)[0], got.xy.view(torch.int64)[b])
    host = vanishing.to_host(got)
    assert [h is None for h in host] == [False, True, False, True]


def test_two_runs_give_equal_bits(gold, dev):
    from opticalflow_amd import vanishing
    for case in ("b", "c"):                                      # the most pairs; the library's own order table
        c = VO.CASES[case]
        vec = _vec(gold, case, dev)
        vp, info = torch.empty(1, 5, dtype=torch.float64, device=dev), torch.empty(1, 6, dtype=torch.int32, device=dev)
        first = vanishing.vanishing_point(vec, c["frame"], seed=3, out=(vp, info), **_kw(case))
        assert first.info.data_ptr() == info.data_ptr() and first.xy.data_ptr() == vp.data_ptr()
        a_vp, a_info = vp.clone(), info.clone()
        assert int(a_info[0, 0]) <= 1 and int(a_info[0, 1]) == {"b": 300, "c": 32}[case]
        for _ in range(2):
            vp.fill_(float("nan"))
            info.fill_(-7)
            vanishing.vanishing_point(vec, c["frame"], seed=3, out=(vp, info), **_kw(case))
            assert torch.equal(vp.view(torch.int64), a_vp.view(torch.int64)) and torch.equal(info, a_info)
    other = vanishing.vanishing_point(vec, c["frame"], seed=4, **_kw("c"))
    assert int(other.info[0, 1]) == 32 and not torch.equal(other.xy, a_vp[:, 0:2])      # another seed selects other cells


def test_estimator_replayed_from_a_graph_equals_the_eager_call(gold, dev):
    from opticalflow_amd import vanishing
    names = VO.BATCH_CASES
    c = VO.CASES[names[0]]
    vec = torch.cat([_vec(gold, n, dev) for n in names], 0).contiguous()
    eager = vanishing.vanishing_point(vec, c["frame"], **_kw(names[0]))
    est = vanishing.VanishingEstimator(len(names), c["frame"], device=dev, **_kw(names[0]))
    static = vec.clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        est.run(static)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = est.run(static)
    est.vp.fill_(float("nan"))
    est.info.fill_(-7)
    graph.replay()
    assert torch.equal(out.info, eager.info) and torch.equal(est.vp.view(torch.int64), torch.cat(
        [eager.xy, eager.prob[:, None], eager.center], 1).view(torch.int64))
    static.copy_(vec.flip(0))                                    # new contents, same graph
    graph.replay()
    assert torch.equal(out.info, eager.info.flip(0)) and torch.equal(out.xy.view(torch.int64), eager.xy.flip(0).contiguous().view(torch.int64))
    with pytest.raises(ValueError):
        est.run(vec[:2])


def test_from_flow_equals_quiver_then_vanishing_point(dev):
    from opticalflow_amd import flowviz, vanishing
    g = torch.Generator().manual_seed(22)
    hq, wq, frame = 24, 32, (96, 128)
    yy, xx = torch.meshgrid(torch.arange(hq, dtype=torch.float32), torch.arange(wq, dtype=torch.float32), indexing="ij")
    flow = torch.stack([torch.stack([0.12 * (xx - fx), 0.12 * (yy - fy)], 0) for fx, fy in ((17.3, 9.6), (9.1, 14.2))], 0)
    flow = (flow + 0.02 * torch.randn(2, 2, hq, wq, generator=g)).to(dev)
    got = vanishing.vanishing_point_from_flow(flow, frame, step=8, min_mag=0.5, max_points=64, seed=1)
    arrows = flowviz.quiver_arrows(flow, frame, step=8, min_mag=0.5, style="video")
    want = vanishing.vanishing_point(arrows.vec, frame, step=8, min_mag=0.5, max_points=64, seed=1)
    assert torch.equal(got.info, want.info) and torch.equal(got.xy.view(torch.int64), want.xy.view(torch.int64))
    assert torch.equal(got.prob, want.prob) and got.ok.all() and (got.info[:, 1] == 64).all()
    # the focus of the first frame, in frame pixels (the flow is at quarter resolution): within a bin or two of (4 * 17.3, 4 * 9.6)
    assert abs(float(got.xy[0, 0]) - 4 * 17.3) < 8 and abs(float(got.xy[0, 1]) - 4 * 9.6) < 8
    crop = vanishing.vanishing_point_from_flow(flow, frame, step=8, min_mag=0.5, crop=(20, 28), max_points=64, seed=1)
    assert crop.ok.all() and not torch.equal(crop.xy, got.xy)


def test_non_contiguous_vec_is_refused(gold, dev):
    from opticalflow_amd import vanishing
    wide = torch.zeros(1, 6, 8, 4, device=dev)
    wide[..., :2] = _vec(gold, "a", dev)
    view = wide[..., :2]
    assert not view.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        vanishing.vanishing_point(view, (96, 128))
    got = vanishing.vanishing_point(view.contiguous(), (96, 128))
    assert int(got.info[0, 0]) == 0
