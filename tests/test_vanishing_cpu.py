"""Vanishing points without a GPU: the NumPy oracle (tests/vanishing_oracle.py) against the reference's own return values
(tests/golden/g16_vanishing.npz, written by tools/gen_golden_vanishing.py), the margin conditions that make every discrete outcome of
a fixture case safe, the device's subsample rule, the C ABI additions and the wrappers' argument checks; and the same three fixture
checks for the edge cases (VO.EDGE_CASES, tests/golden/g19_vanishing_edges.npz), which tests/test_gpu_vanishing_edges.py runs."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import vanishing_oracle as VO  # noqa: E402

NEW_SYMBOLS = ("pwc_vanishing_workspace_bytes", "pwc_vanishing_point")


@pytest.fixture(scope="module")
def gold():
    path = os.path.join(HERE, "golden", "g16_vanishing.npz")
    assert os.path.getsize(path) <= 1 << 20
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def results(gold):
    """The oracle on every case, computed once."""
    out = {}
    for name, c in VO.CASES.items():
        idx = gold["idx/" + name] if gold["idx/" + name].size else None
        out[name] = VO.estimate(gold["vec/" + name], c["frame"], c["step"], c["min_mag"], c["max_points"], c["grid_size"], c["min_pairs"],
                                idx=idx)
    return out


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize("case", sorted(VO.CASES))
def test_oracle_reproduces_the_reference(gold, results, case):
    r = results[case]
    assert gold["vec/" + case].shape == VO.grid_shape(VO.CASES[case]["frame"], VO.CASES[case]["step"]) + (2,)
    if not bool(gold["ref_ok/" + case]):
        assert r["status"] >= 2 and r["xy"] is None and r["prob"] is None
        return
    vx, vy, prob = gold["ref/" + case]
    assert r["status"] == 0
    assert _rel(vx, r["xy"][0]) <= 1e-12 and _rel(vy, r["xy"][1]) <= 1e-12 and _rel(prob, r["prob"]) <= 1e-12


@pytest.mark.parametrize("case", sorted(VO.CASES))
def test_margin_conditions_hold(results, case):
    m = VO.margins(results[case], case)
    assert set(m) == {"mag", "denom", "range", "edges", "best", "inlier", "mag_ratio", "cond"}
    assert all(m.values()), [k for k, v in m.items() if not v]


def test_cases_show_what_they_are_there_for(gold, results):
    r = results
    assert r["a"]["n_kept"] % 2 == 1 and r["a"]["n_kept"] < 48 and r["g"]["n_kept"] % 2 == 0
    assert r["b"]["n_kept"] == 300 and r["b"]["xy"][0] < 0 and -0.5 * 135 < r["b"]["xy"][0]
    assert not float(r["b"]["x_edges"][1]).is_integer()                                         # ragged grid, non-integer edges
    assert r["c"]["n_kept"] > 32 and r["c"]["n_used"] == 32 and gold["idx/c"].size == 32
    assert np.isin(r["d"]["ix"], r["d"]["x_edges"]).all() and np.isin(r["d"]["iy"], r["d"]["y_edges"]).all()
    assert r["e"]["status"] == 2 and r["f"]["status"] == 3 and r["f"]["pairs_kept"] == 0
    assert r["g"]["hist"].shape == (16, 16)
    geo = {(VO.CASES[c]["frame"], VO.CASES[c]["step"], VO.CASES[c]["grid_size"], VO.CASES[c]["max_points"]) for c in VO.BATCH_CASES}
    assert len(geo) == 1 and len(VO.BATCH_CASES) >= 3
    st = [r[c]["status"] for c in VO.BATCH_CASES]
    assert any(st[i] >= 2 and st[i - 1] <= 1 and st[i + 1] <= 1 for i in range(1, len(st) - 1))


def test_pair_loop_and_array_form_agree(gold):
    c = VO.CASES["a"]
    kw = dict(step=c["step"], min_mag=c["min_mag"], max_points=c["max_points"], grid_size=c["grid_size"], min_pairs=c["min_pairs"])
    a, b = VO.estimate(gold["vec/a"], c["frame"], **kw), VO.estimate(gold["vec/a"], c["frame"], loop=True, **kw)
    assert np.array_equal(a["ix"], b["ix"]) and np.array_equal(a["iy"], b["iy"]) and np.array_equal(a["hist"], b["hist"])
    assert a["xy"] == b["xy"] and a["prob"] == b["prob"] and len(b["denom"]) == a["n_used"] * (a["n_used"] - 1) // 2


def test_bin_edges_rule():
    e = VO.edges(-67.5, 202.5, 64)
    assert e[0] == -67.5 and e[64] == 202.5 and np.array_equal(e, np.linspace(-67.5, 202.5, 65))
    h, _, _ = np.histogram2d([e[3], 202.5], [e[5], np.nextafter(e[5], -np.inf)], bins=64, range=[[-67.5, 202.5], [-67.5, 202.5]])
    assert h[3, 5] == 1 and h[63, 4] == 1                       # e[k] <= v goes up, v == hi goes to the last bin


def test_order_rule_reproduces_the_recorded_draw(gold, results):
    from opticalflow_amd import vanishing
    r = results["c"]
    keep, idx = r["keep"], gold["idx/c"]
    order = VO.order_from_idx(keep, idx)
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(keep.size))
    assert np.array_equal(VO.select_by_order(keep, order, 32), np.flatnonzero(keep)[idx])
    assert np.array_equal(VO.select_by_order(keep, order, 32), r["cells"])
    # at most max_points kept: row-major, whatever the order says
    assert np.array_equal(VO.select_by_order(keep, order[::-1], keep.sum()), np.flatnonzero(keep))
    # the library's own table: a permutation, the same on every call, another for another seed
    t = vanishing.order_table(192, 0)
    assert t.dtype == np.int32 and np.array_equal(np.sort(t), np.arange(192)) and t is vanishing.order_table(192, 0)
    assert np.array_equal(t, np.random.default_rng(0).permutation(192)) and not np.array_equal(t, vanishing.order_table(192, 1))
    sub = VO.select_by_order(keep, t, 32)
    assert len(sub) == 32 and len(set(sub.tolist())) == 32 and keep[sub].all()


def test_new_symbols_declared_exported_bound_and_abi_13():
    import opticalflow_amd
    from opticalflow_amd import _lib, ops, vanishing
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pwc_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 13 and _lib.load().pwc_abi_version() == 13
    assert re.search(r"#define PWC_ABI_VERSION 13\b", text)
    assert opticalflow_amd.vanishing is vanishing and opticalflow_amd.vanishing_point is vanishing.vanishing_point
    assert callable(ops.vanishing_point) and callable(ops.vanishing_workspace_bytes)
    assert vanishing.VanishingPoints._fields == ("xy", "prob", "center", "info")
    vp = vanishing.VanishingPoints(torch.zeros(3, 2), torch.zeros(3), torch.zeros(3, 2), torch.tensor([[0] * 6, [1] * 6, [2] * 6]))
    assert vp.ok.tolist() == [True, True, False]


def test_workspace_query_and_c_argument_checks_launch_nothing():
    from opticalflow_amd import _lib
    lib = _lib.load()
    q = lib.pwc_vanishing_workspace_bytes
    assert q(1, 6, 8, 64) == 24 + 8 * 64 * 64 + 4096 and q(3, 15, 20, 16) == 3 * (24 + 8 * 256 + 4096)
    assert q(0, 6, 8, 64) == -1 and q(1, 6, 8, 1) == -1 and q(1, 6, 8, 129) == -1 and q(1, 257, 256, 64) == -1 and q(1, 256, 256, 128) > 0
    buf = (ctypes.c_double * 8192)()
    p = ctypes.addressof(buf)
    nbytes = ctypes.sizeof(buf)
    call = lib.pwc_vanishing_point

    def args(vec=p, n=1, gy=6, gx=8, fh=96, fw=128, step=16, min_mag=1.0, max_points=300, grid=64, min_pairs=50, order=None, vp=p,
             info=p, ws=p, wsb=nbytes):
        return (vec, n, gy, gx, fh, fw, step, min_mag, max_points, grid, min_pairs, order, vp, info, ws, wsb, None)

    # every call below fails its checks, which come before anything touches a device
    for bad in (dict(vec=None), dict(vp=None), dict(info=None), dict(ws=None)):
        assert call(*args(**bad)) == -1 and b"null pointer" in lib.pwc_last_error()
    assert call(*args(grid=1)) == -1 and call(*args(grid=129)) == -1 and b"grid" in lib.pwc_last_error()
    assert call(*args(max_points=4)) == -1 and call(*args(max_points=1025)) == -1 and b"max_points" in lib.pwc_last_error()
    assert call(*args(gy=257, gx=256, fh=257, fw=256, step=1, order=p)) == -1 and b"cells" in lib.pwc_last_error()
    assert call(*args(step=0)) == -1 and b"step" in lib.pwc_last_error()
    assert call(*args(wsb=24 + 8 * 64 * 64 + 4095)) == -1 and b"workspace" in lib.pwc_last_error()
    assert call(*args(max_points=47)) == -1 and b"order" in lib.pwc_last_error()          # 48 cells, no order table
    assert call(*args(gy=7)) == -1 and call(*args(n=0)) == -1
    assert call(*args(ws=p + 4)) == -3 and call(*args(max_points=47, order=p + 2)) == -3
    assert b"pwc_vanishing_point" in lib.pwc_last_error()


def test_wrapper_argument_errors_raise_without_a_device():
    from opticalflow_amd import PwcHipError, ops, vanishing
    host = torch.zeros(1, 6, 8, 2)
    with pytest.raises(PwcHipError):
        ops.vanishing_point(host, 96, 128, 16)
    with pytest.raises(PwcHipError):
        vanishing.vanishing_point(host, (96, 128))
    with pytest.raises(PwcHipError):
        vanishing.vanishing_point(host, (96, 128), max_points=32)
    with pytest.raises(PwcHipError):
        vanishing.vanishing_point_from_flow(torch.zeros(1, 2, 24, 32), (96, 128))
    with pytest.raises(TypeError):
        ops.vanishing_point(host.double(), 96, 128, 16)
    with pytest.raises(ValueError):
        ops.vanishing_point(torch.zeros(1, 6, 9, 2), 96, 128, 16)
    with pytest.raises(ValueError):
        ops.vanishing_point(host, 96, 128, 0)
    with pytest.raises(ValueError):
        ops.vanishing_point(host, 96, 128, 16, max_points=4)
    with pytest.raises(ValueError):
        ops.vanishing_point(host, 96, 128, 16, grid=129)
    with pytest.raises(ValueError):
        vanishing.vanishing_point(host, (96, 128), step=0)
    with pytest.raises(ValueError):
        ops.vanishing_workspace_bytes(1, 6, 8, 1)
    assert ops.vanishing_workspace_bytes(2, 6, 8, 64) == 2 * (24 + 8 * 64 * 64 + 4096)


# ---- the edge cases: tests/golden/g19_vanishing_edges.npz (tools/gen_golden_vanishing.py edges), VO.EDGE_CASES ----

@pytest.fixture(scope="module")
def edge_gold():
    path = os.path.join(HERE, "golden", "g19_vanishing_edges.npz")
    assert os.path.getsize(path) <= 1 << 20
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def edge_results(edge_gold):
    """The oracle on every edge case, computed once."""
    out = {}
    for name, c in VO.EDGE_CASES.items():
        idx = edge_gold["idx/" + name] if edge_gold["idx/" + name].size else None
        out[name] = VO.estimate(edge_gold["vec/" + name], c["frame"], c["step"], c["min_mag"], c["max_points"], c["grid_size"],
                                c["min_pairs"], idx=idx)
    return out


@pytest.mark.parametrize("case", sorted(VO.EDGE_CASES))
def test_oracle_reproduces_the_reference_on_the_edge_cases(edge_gold, edge_results, case):
    r = edge_results[case]
    assert edge_gold["vec/" + case].shape == VO.grid_shape(VO.EDGE_CASES[case]["frame"], VO.EDGE_CASES[case]["step"]) + (2,)
    assert np.array_equal(edge_gold["vec/" + case], VO.make_field(case, int(edge_gold["seed/" + case])))
    assert bool(edge_gold["ref_ok/" + case]) and r["status"] <= 1        # every edge case is one the reference answers
    vx, vy, prob = edge_gold["ref/" + case]
    assert _rel(vx, r["xy"][0]) <= 1e-12 and _rel(vy, r["xy"][1]) <= 1e-12 and _rel(prob, r["prob"]) <= 1e-12


@pytest.mark.parametrize("case", sorted(VO.EDGE_CASES))
def test_margin_conditions_hold_on_the_edge_cases(edge_results, case):
    r = edge_results[case]
    m = VO.edge_margins(r, case)
    assert set(m) == {"mag", "denom", "range", "edges", "best", "inlier", "mag_ratio", "cond", "normal_eq"}
    assert all(m.values()), [k for k, v in m.items() if not v]
    frac = VO.normal_equations_fraction(r)
    print("case %s: normal equations at %.3g of the xy tolerance" % (case, frac))
    assert frac <= 0.1
    if case in VO.EXACT_EDGE_CASES:                     # what replaces "mag" and "best" there: axis-aligned vectors of magnitude 0, 1, 2
        vec = r["vec"].reshape(-1, 2).astype(np.float64)
        below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
        assert ((vec == 0).any(axis=1)).all() and np.isin(np.abs(vec).max(axis=1), [0.0, 1.0, 2.0, below]).all()
        assert np.array_equal(r["mag_all"], np.abs(vec).max(axis=1)) and len(set(r["mags"].tolist())) == 1
        assert np.array_equal(r["hist"], np.round(r["hist"]))
    else:                                               # no exemption anywhere else: the plain rules, spelled out
        c = VO.EDGE_CASES[case]
        assert (np.abs(r["mag_all"] - c["min_mag"]) > 1e-6 * c["min_mag"]).all()
        assert r["best_weight"] >= (1.0 + 1e-6) * r["runner_up"]


def test_edge_cases_show_what_they_are_there_for(edge_gold, edge_results):
    r, E = edge_results, VO.EDGE_CASES
    # the cut of the by-order compaction (256 positions per round, 64 per wave)
    for case, rounds in (("p768", (1,)), ("p1792", range(2, 7))):
        keep, idx = r[case]["keep"], edge_gold["idx/" + case]
        assert keep.size == {"p768": 768, "p1792": 1792}[case] and r[case]["n_kept"] > 700 and r[case]["n_used"] == 300 == len(idx)
        order = VO.order_from_idx_interleaved(keep, idx)
        assert np.array_equal(np.sort(order), np.arange(keep.size))
        assert np.array_equal(VO.select_by_order(keep, order, 300), r[case]["cells"])
        cut = VO.cut_position(keep, order, 300)
        assert cut // 256 in rounds and cut % 64 != 0, (case, cut)
        assert keep[order[cut]] and keep[order[:cut + 1]].sum() == 300
    assert r["plus1"]["n_kept"] == E["plus1"]["max_points"] + 1 == r["plus1"]["n_used"] + 1 and r["plus1"]["keep"].size == 192
    H, W = E["full1024"]["frame"]
    assert H > W and r["full1024"]["keep"].size == 2048 and r["full1024"]["n_kept"] > 1024 and r["full1024"]["n_used"] == 1024
    assert len(r["full1024"]["denom"]) == 523776 and edge_gold["vec/full1024"].shape == (64, 32, 2)
    assert r["n5"]["n_kept"] == r["n5"]["n_used"] == 5 and r["n5"]["status"] in (0, 1) and E["n5"]["min_pairs"] == 5
    assert r["n5"]["pairs_kept"] >= 5
    mags = np.sort(r["n5"]["mags"])
    raised = 0.5 * (mags[0] + mags[1])                  # above the weakest of the five: four are left
    assert mags[0] * (1 + 1e-6) < raised < mags[1] * (1 - 1e-6)
    c = E["n5"]
    assert VO.estimate(edge_gold["vec/n5"], c["frame"], c["step"], raised, c["max_points"], c["grid_size"], c["min_pairs"])["status"] == 2
    assert r["st1"]["status"] == 1 and 5 <= r["st1"]["n_kept"] <= 8 and r["st1"]["inliers"] < 5 and r["st1"]["xy"] == r["st1"]["center"]
    assert r["st1"]["pairs_kept"] >= E["st1"]["min_pairs"]
    assert edge_gold["vec/wide"].shape == (1, 65536, 2) and r["wide"]["status"] == 0 and r["wide"]["n_used"] == 1024 < r["wide"]["n_kept"]
    assert 0 in r["wide"]["cells"] and 65535 in r["wide"]["cells"] and 1400 < r["wide"]["n_kept"] < 1600
    assert (edge_gold["vec/wide"][0, ~r["wide"]["keep"]] == 0).all()
    for case in VO.TIE_CASES:                           # the maximum attained at least twice, exactly
        t = VO.tie_bins(r[case])
        h = r[case]["hist"].ravel()
        assert len(t) >= 2 and h[t[0]] == h[t[1]] == r[case]["best_weight"] == r[case]["runner_up"] and r[case]["status"] == 0
        assert r[case]["best"] == tuple(int(v) for v in np.unravel_index(t[0], r[case]["hist"].shape))
    # which lanes of the arg-max hold the two lowest tied bins (VO.tie_lanes says why each grid gives what it gives)
    a, b = VO.tie_lanes(r["tie"])
    assert a == b and VO.tie_bins(r["tie"])[1] - VO.tie_bins(r["tie"])[0] >= 256      # one lane walks both: its ascending scan decides
    a, b = VO.tie_lanes(r["tie16"])
    assert a < b and r["tie16"]["hist"].size == 256                                      # one bin per lane: only the tree decides
    a, b = VO.tie_lanes(r["tie32"])
    assert a > b and VO.tie_tree_sides(r["tie32"]) == (1, 0)                             # lower index, higher lane, upper side of the tree
    assert VO.tie_tree_sides(r["tie"]) is None
    m = r["atmin"]["mag_all"]
    below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    assert E["atmin"]["min_mag"] == 2.0 and r["atmin"]["n_kept"] == (m == 2.0).sum() > 0 and (m == 1.0).any() and (m == below).any()
    assert set(np.unique(m).tolist()) <= {0.0, 1.0, below, 2.0}


def test_selection_rule_for_an_order_that_is_no_permutation():
    keep = np.array([1, 0, 1, 1, 0, 1, 1, 1], bool)
    order = np.array([7, -1, 8, 2 ** 30, 1, 2, 7, 4, 3, 0], np.int64)        # outside the grid: skipped; not kept: skipped; 7 twice
    assert VO.select_by_order(keep, order, 5).tolist() == [7, 2, 7, 3, 0]
    assert VO.select_by_order(keep, order, 3).tolist() == [7, 2, 7] and VO.cut_position(keep, order, 3) == 6
    assert VO.select_by_order(keep, order, 6).tolist() == [0, 2, 3, 5, 6, 7]  # at most max_points kept: row-major, order unused


def test_non_finite_vectors_are_dropped_by_the_oracle(gold):
    c = VO.CASES["a"]
    kw = dict(step=c["step"], min_mag=c["min_mag"], max_points=c["max_points"], grid_size=c["grid_size"], min_pairs=c["min_pairs"])
    r = VO.estimate(gold["vec/a"], c["frame"], **kw)
    cells = np.flatnonzero(r["keep"])
    bad, zeroed = gold["vec/a"].copy(), gold["vec/a"].copy()
    bad.reshape(-1, 2)[cells[3]] = np.nan
    bad.reshape(-1, 2)[cells[10]] = (np.inf, 1.0)
    zeroed.reshape(-1, 2)[cells[[3, 10]]] = 0.0
    rb, rz = VO.estimate(bad, c["frame"], **kw), VO.estimate(zeroed, c["frame"], **kw)
    assert rb["n_kept"] == rz["n_kept"] == r["n_kept"] - 2 and np.array_equal(rb["keep"], rz["keep"])
    assert rb["status"] == rz["status"] == 0 and rb["xy"] == rz["xy"] and rb["prob"] == rz["prob"]
