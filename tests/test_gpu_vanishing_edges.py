"""GPU checks of the vanishing point (csrc/pwc_vanishing.hip) off the eight small cases of tests/test_gpu_vanishing.py: the cases of
tests/golden/g19_vanishing_edges.npz (VO.EDGE_CASES; tests/test_vanishing_cpu.py ties the oracle to the reference's own return values
on them and asserts their margins), and around them the decisions the kernels make that no fixture case reaches: a by-order selection
whose cut falls inside a later round of 256 positions, max_points = 1024, N = 5, gx = 65 536, a portrait frame, exact ties of the
arg-max, status 1, pairs == min_pairs, a magnitude exactly min_mag, an `order` that is no permutation, non-finite vectors.

A result is compared as tests/test_gpu_vanishing.py compares it, by its own _compare: status, N, pairs, best bin and inliers EQUAL,
centre relative 1e-12, prob relative 1e-6, refined xy within VO.xy_tolerance, prob bit-equal or within 2^-50 for the exact cases.
Where a test changes a field, a parameter or the selection, no reference value is recorded, so the oracle is the reference and the
margin conditions are asserted in the test, on the oracle's values.  Observed on MI355X: DESIGN.md section 22."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vanishing_oracle as VO  # noqa: E402
from test_gpu_vanishing import _compare  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INTERLEAVED = ("p768", "p1792", "full1024", "wide")      # order tables that put the cut of the selection far into the table


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold():
    return _load("g19_vanishing_edges.npz")


@pytest.fixture(scope="module")
def field_a():
    return _load("g16_vanishing.npz")["vec/a"]


@pytest.fixture(scope="module")
def expected(gold):
    """The oracle on every edge case, computed once and shared."""
    return {name: _oracle(gold["vec/" + name], c, idx=gold["idx/" + name] if gold["idx/" + name].size else None)
            for name, c in VO.EDGE_CASES.items()}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _oracle(vec, c, idx=None, **over):
    p = dict(c, **over)
    return VO.estimate(vec, p["frame"], p["step"], p["min_mag"], p["max_points"], p["grid_size"], p["min_pairs"], idx=idx)


def _assert_margins(r, case):
    m = VO.edge_margins(r, case)
    assert all(m.values()), (case, [k for k, v in m.items() if not v])


def _device(vec, c, dev, order=None, **over):
    """ops.vanishing_point on vec [Gy,Gx,2] or [B,Gy,Gx,2] (NumPy) -> (vp [B,5], info [B,6]) on the device."""
    from opticalflow_amd import ops
    p = dict(c, **over)
    v = torch.from_numpy(np.ascontiguousarray(vec))
    v = (v.unsqueeze(0) if v.dim() == 3 else v).to(dev)
    if order is not None:
        order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    return ops.vanishing_point(v, p["frame"][0], p["frame"][1], p["step"], p["min_mag"], p["max_points"], p["grid_size"],
                               p["min_pairs"], order=order)


def _check(case, r, vp, info, b=0):
    vp, info = vp.cpu().numpy(), info.cpu().numpy()
    _compare(case, r, vp[b, 0:2], float(vp[b, 2]), vp[b, 3:5], info[b])


def _bits(vp):
    return vp.contiguous().view(torch.int64)


def _case_order(case, r, gold):
    if not gold["idx/" + case].size:
        return None
    make = VO.order_from_idx_interleaved if case in INTERLEAVED else VO.order_from_idx
    return make(r["keep"], gold["idx/" + case])


@pytest.mark.parametrize("case", sorted(VO.EDGE_CASES))
def test_every_edge_case_singly(gold, expected, dev, case):
    c, r = VO.EDGE_CASES[case], expected[case]
    vp, info = _device(gold["vec/" + case], c, dev, order=_case_order(case, r, gold))
    assert vp.dtype == torch.float64 and info.dtype == torch.int32 and tuple(vp.shape) == (1, 5) and tuple(info.shape) == (1, 6)
    _check(case, r, vp, info)
    if case == "n5":                                             # min_mag raised above the weakest of the five: four are left
        mags = np.sort(r["mags"])
        raised = 0.5 * (mags[0] + mags[1])
        r2 = _oracle(gold["vec/n5"], c, min_mag=raised)
        assert r2["status"] == 2 and r2["n_kept"] == 4 and (np.abs(r2["mag_all"] - raised) > 1e-6 * raised).all()
        vp2, info2 = _device(gold["vec/n5"], c, dev, min_mag=raised)
        _check("n5/raised", r2, vp2, info2)
        assert torch.isnan(vp2[0, [0, 1, 3, 4]]).all() and info2[0].tolist() == [2, 4, 0, -1, -1, 0]
    if case == "st1":                                            # the bin centre stands, bit for bit
        assert int(info[0, 0]) == 1 and int(info[0, 5]) < 5 and torch.equal(_bits(vp[:, 0:2]), _bits(vp[:, 3:5]))


@pytest.mark.parametrize("case", ["atmin", "n5", "plus1"])
def test_min_pairs_boundary(gold, expected, dev, case):
    c, r = VO.EDGE_CASES[case], expected[case]
    P = r["pairs_kept"]
    assert r["status"] == 0 and P >= 5
    order = _case_order(case, r, gold)
    idx = gold["idx/" + case] if gold["idx/" + case].size else None
    at, above = _oracle(gold["vec/" + case], c, idx=idx, min_pairs=P), _oracle(gold["vec/" + case], c, idx=idx, min_pairs=P + 1)
    assert at["status"] == 0 and above["status"] == 3 and at["pairs_kept"] == above["pairs_kept"] == P
    vp, info = _device(gold["vec/" + case], c, dev, order=order, min_pairs=P)
    _check(case, at, vp, info)
    assert info[0, 0:3].tolist() == [0, r["n_used"], P]
    vp, info = _device(gold["vec/" + case], c, dev, order=order, min_pairs=P + 1)
    _check(case, above, vp, info)
    assert info[0].tolist() == [3, r["n_used"], P, -1, -1, 0] and torch.isnan(vp[0, [0, 1, 3, 4]]).all() and float(vp[0, 2]) == 0.0


@pytest.mark.parametrize("case", VO.TIE_CASES)
def test_ties_go_to_the_lowest_flat_index(gold, expected, dev, case):
    """Two or more bins attain the maximum with exactly equal weight (2^40 per vote on the device).  As recorded the tied pair differs
    in gx; mirrored in y it still does, at other gy (other lanes); transposed it differs in gy."""
    c = VO.EDGE_CASES[case]
    vec = gold["vec/" + case]
    mirrored = np.ascontiguousarray(vec[::-1] * np.array([1.0, -1.0], np.float32))
    transposed = np.ascontiguousarray(vec.transpose(1, 0, 2)[..., ::-1])
    for label, v in (("", vec), ("/mirrored in y", mirrored), ("/transposed", transposed)):
        r = expected[case] if v is vec else _oracle(v, c)
        _assert_margins(r, case)
        tied = VO.tie_bins(r)
        assert r["status"] == 0 and len(tied) >= 2 and r["hist"].ravel()[tied[1]] == r["best_weight"], label
        assert r["best"] == tuple(int(k) for k in np.unravel_index(np.argmax(r["hist"]), r["hist"].shape))
        if label == "/transposed":
            assert tied[0] // c["grid_size"] == tied[1] // c["grid_size"]          # same gx, the pair differs in gy
        vp, info = _device(v, c, dev)
        assert (int(info[0, 3]), int(info[0, 4])) == r["best"], (case + label, info[0].tolist(), r["best"], VO.tie_lanes(r))
        _check(case, r, vp, info)                                                   # the case's own name: prob is held to exactness
        assert float(vp[0, 2]) == r["prob"] or abs(float(vp[0, 2]) - r["prob"]) <= 2.0 ** -50 * r["prob"]


def test_mixed_batch_by_order_and_row_major(gold, expected, dev):
    """One launch, one order table: frame 1 has at most max_points kept cells and is selected row-major between two frames that are
    selected by order."""
    c, r = VO.EDGE_CASES["plus1"], expected["plus1"]
    vec = gold["vec/plus1"]
    fewer = vec.copy()
    fewer.reshape(-1, 2)[np.flatnonzero(r["keep"])[:5]] = 0.0
    rf = _oracle(fewer, c)
    _assert_margins(rf, "plus1")
    assert rf["status"] == 0 and rf["n_kept"] == r["n_kept"] - 5 <= c["max_points"] and rf["n_used"] == rf["n_kept"]
    order = VO.order_from_idx(r["keep"], gold["idx/plus1"])
    vp, info = _device(np.stack([vec, fewer, vec]), c, dev, order=order)
    for b, want in enumerate((r, rf, r)):
        _check("plus1/frame %d" % b, want, vp, info, b)
    one_vp, one_info = _device(vec, c, dev, order=order)
    for b in (0, 2):
        assert torch.equal(_bits(vp[b:b + 1]), _bits(one_vp)) and torch.equal(info[b:b + 1], one_info)
    few_vp, few_info = _device(fewer, c, dev, order=order[::-1])                   # row-major whatever the table says
    assert torch.equal(_bits(vp[1:2]), _bits(few_vp)) and torch.equal(info[1:2], few_info)


@pytest.mark.parametrize("case,seed", [("p768", 0), ("p1792", 0)])
def test_library_order_table_on_the_shipped_geometry(gold, expected, dev, case, seed):
    """vanishing.vanishing_point(vec, ..., seed=s): the shipped call on the shipped geometry.  The oracle gets the cells the
    documented rule selects from vanishing.order_table."""
    from opticalflow_amd import vanishing
    c, keep = VO.EDGE_CASES[case], expected[case]["keep"]
    table = vanishing.order_table(keep.size, seed)
    cells = VO.select_by_order(keep, table, c["max_points"])
    cut = VO.cut_position(keep, table, c["max_points"])
    assert len(cells) == 300 and cut % 64 != 0 and (256 <= cut < 512 if case == "p768" else cut >= 512), cut
    r = _oracle(gold["vec/" + case], c, idx=VO.idx_of_cells(keep, cells))
    _assert_margins(r, case)
    assert r["status"] == 0 and np.array_equal(r["cells"], cells)
    got = vanishing.vanishing_point(torch.from_numpy(gold["vec/" + case]).unsqueeze(0).to(dev), c["frame"], step=c["step"],
                                    min_mag=c["min_mag"], max_points=c["max_points"], grid_size=c["grid_size"],
                                    min_pairs=c["min_pairs"], seed=seed)
    _compare("%s/seed %d" % (case, seed), r, got.xy[0].cpu().numpy(), float(got.prob[0]), got.center[0].cpu().numpy(),
             got.info[0].cpu().numpy())


def test_order_that_is_no_permutation(gold, expected, dev):
    """include/pwc_hip.h: entries outside 0 .. cells-1 are skipped, an entry that repeats an earlier one selects its cell again, and
    when the table names fewer than max_points kept cells, those are all that is used."""
    c, r = VO.EDGE_CASES["plus1"], expected["plus1"]
    keep, cells = r["keep"], r["keep"].size
    g = np.random.default_rng(19)
    kept, unkept = np.flatnonzero(keep), np.flatnonzero(~keep)
    valid = g.choice(kept, size=100, replace=False)
    order = np.concatenate([valid, valid[[3, 3, 17, 40, 77, 99]], unkept, np.resize([-1, cells, 2 ** 30, -2 ** 31, cells + 7], 82)])
    order = order[g.permutation(len(order))]
    assert len(order) == cells == 192 and len(unkept) == 4 and r["n_kept"] > c["max_points"]
    want = VO.select_by_order(keep, order, c["max_points"])
    assert len(want) == 106 < c["max_points"] and len(set(want.tolist())) == 100 and keep[want].all()
    ro = _oracle(gold["vec/plus1"], c, idx=VO.idx_of_cells(keep, want))
    _assert_margins(ro, "plus1")
    assert ro["status"] == 0 and ro["n_used"] == 106 and np.array_equal(ro["cells"], want)
    vp, info = _device(gold["vec/plus1"], c, dev, order=order)
    assert int(info[0, 1]) == 106
    _check("plus1/no permutation", ro, vp, info)


def test_two_runs_give_equal_bits_at_the_size_limits(gold, dev):
    from opticalflow_amd import vanishing
    for case in ("full1024", "wide"):                            # the most atomics; the most select rounds
        c = VO.EDGE_CASES[case]
        kw = dict(step=c["step"], min_mag=c["min_mag"], max_points=c["max_points"], grid_size=c["grid_size"], min_pairs=c["min_pairs"])
        vec = torch.from_numpy(gold["vec/" + case]).unsqueeze(0).to(dev)
        vp, info = torch.empty(1, 5, dtype=torch.float64, device=dev), torch.empty(1, 6, dtype=torch.int32, device=dev)
        vanishing.vanishing_point(vec, c["frame"], seed=3, out=(vp, info), **kw)
        a_vp, a_info = vp.clone(), info.clone()
        assert int(a_info[0, 0]) == 0 and int(a_info[0, 1]) == 1024
        for _ in range(2):
            vp.fill_(float("nan"))
            info.fill_(-7)
            vanishing.vanishing_point(vec, c["frame"], seed=3, out=(vp, info), **kw)
            assert torch.equal(_bits(vp), _bits(a_vp)) and torch.equal(info, a_info)


def test_non_finite_vectors_are_dropped(field_a, dev):
    """A NaN cell and a (+Inf, 1) cell in the middle frame of three: the frame is answered as if both cells were 0, and its
    neighbours are untouched."""
    c = VO.CASES["a"]
    clean = _oracle(field_a, c)
    cells = np.flatnonzero(clean["keep"])
    bad, zeroed = field_a.copy(), field_a.copy()
    bad.reshape(-1, 2)[cells[3]] = np.nan
    bad.reshape(-1, 2)[cells[10]] = (np.inf, 1.0)
    zeroed.reshape(-1, 2)[cells[[3, 10]]] = 0.0
    rz = _oracle(zeroed, c)
    m = VO.margins(rz, "a")
    assert rz["status"] == 0 and rz["n_kept"] == clean["n_kept"] - 2 and all(m.values()), [k for k, v in m.items() if not v]
    vp, info = _device(np.stack([field_a, bad, field_a]), c, dev)
    z_vp, z_info = _device(zeroed, c, dev)
    assert torch.equal(_bits(vp[1:2]), _bits(z_vp)) and torch.equal(info[1:2], z_info)
    _check("a/non-finite", rz, vp, info, 1)
    one_vp, one_info = _device(field_a, c, dev)
    _check("a", clean, one_vp, one_info)
    for b in (0, 2):
        assert torch.equal(_bits(vp[b:b + 1]), _bits(one_vp)) and torch.equal(info[b:b + 1], one_info)
