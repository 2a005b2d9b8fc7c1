"""CPU checks of the device flow-comparison report (csrc/pwc_flow_compare.hip, ops.flow_compare, opticalflow_amd.compare): the C ABI is
declared, bound, exported and refuses bad arguments before any launch; the g18 fixture's inputs are the recipe's; the float64 oracle
agrees with the values the reference's own compare_flows / print_flow_stats returned and printed; the host formatting reproduces the
reference's lines character for character."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import flow_compare_oracle as FO

NAMES = ("pwc_flow_compare_workspace_bytes", "pwc_flow_compare")
F32_KEYS = ("L2 diff", "MAE", "Max abs diff", "Relative L2 diff", "Relative MAE", "Cosine similarity", "EPE mean", "EPE max")
REF_KEYS = ["L2 diff", "MAE", "Max abs diff", "Relative L2 diff", "Relative MAE", "Pearson corr", "Cosine similarity", "EPE mean",
            "EPE max", "agreements"]
PWC_EINVAL = -1
_ROWS = {}


def _oracle_rows(name):
    """the oracle's rows for the reference's four thresholds, computed once per case"""
    if name not in _ROWS:
        a, b = FO.make_inputs(name)
        _ROWS[name] = (FO.digest(a, b), FO.rows(a, b, FO.REF_TAUS))
    return _ROWS[name]


def _reference_row(z, name, r):
    """the reference's returned dict of row r, with the dtypes it returned them in"""
    m = {k: z[name + "/ref32"][r, i] for i, k in enumerate(F32_KEYS)}
    m["Pearson corr"] = z[name + "/pearson"][r]
    m["agreements"] = {"agree@%s" % t: z[name + "/agree"][r, i] for i, t in enumerate(FO.REF_TAUS)}
    return {k: m[k] for k in REF_KEYS}


def test_symbols_declared_bound_exported():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define PWC_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13 and _lib.load().pwc_abi_version() == 13
    assert "pwc_flow_compare.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()
    import opticalflow_amd
    from opticalflow_amd import compare, ops
    for n in ("flow_compare", "flow_compare_workspace_bytes"):
        assert hasattr(ops, n)
    for n in ("compare_flows", "compare_models", "FlowComparer", "FlowComparison", "format_report", "format_stats"):
        assert hasattr(compare, n)
    assert opticalflow_amd.compare is compare and opticalflow_amd.compare_flows is compare.compare_flows


def test_record_layout_mirrors_the_header():
    from opticalflow_amd import ops
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    defs = dict(line.split()[1:3] for line in text.splitlines() if line.startswith("#define PWC_FC_") or line.startswith("#define PWC_FLOW_COMPARE_"))
    assert int(defs["PWC_FLOW_COMPARE_FIELDS"]) == ops.FLOW_COMPARE_FIELDS == 44
    assert int(defs["PWC_FLOW_COMPARE_MAX_TAUS"]) == ops.FLOW_COMPARE_MAX_TAUS == 8
    fc = {k[len("PWC_"):]: int(v) for k, v in defs.items() if k.startswith("PWC_FC_")}
    assert len(fc) == 30 and all(getattr(ops, k) == v for k, v in fc.items())
    # every index is used once: two runs of 8 (counts, agreements) and 28 single fields
    used = sorted(v for k, v in fc.items() if k not in ("FC_COUNT0", "FC_AGREE0"))
    used += list(range(fc["FC_COUNT0"], fc["FC_COUNT0"] + 8)) + list(range(fc["FC_AGREE0"], fc["FC_AGREE0"] + 8))
    assert sorted(used) == list(range(44))


def test_workspace_bytes_formula():
    from opticalflow_amd import _lib, ops
    lib = _lib.load()
    # 128 bytes {9 fp64 sums, 8 int32 counts, 6 float extrema} per 32 x 128 tile
    assert lib.pwc_flow_compare_workspace_bytes(1, 1, 1) == 128
    assert lib.pwc_flow_compare_workspace_bytes(2, 32, 128) == 128 * 2
    assert lib.pwc_flow_compare_workspace_bytes(3, 33, 129) == 128 * 3 * 4
    assert lib.pwc_flow_compare_workspace_bytes(1, 528, 2048) == 128 * 17 * 16
    assert lib.pwc_flow_compare_workspace_bytes(1, 8673, 4) == 128 * 272
    assert lib.pwc_flow_compare_workspace_bytes(16, 375, 1242) == 128 * 16 * 12 * 10
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.pwc_flow_compare_workspace_bytes(*bad) == -1
        with pytest.raises(ValueError):
            ops.flow_compare_workspace_bytes(*bad)
    assert ops.flow_compare_workspace_bytes(2, 33, 200) == 128 * 2 * 2 * 2
    assert FO.TILE_H == 32 and FO.TILE_W == 128
    c = FO.CASES["many_tiles"]
    assert -(-c["H"] // FO.TILE_H) * -(-c["W"] // FO.TILE_W) > FO.FINISH_LANES


def test_abi_argument_errors_without_gpu():
    """Every argument check comes before any launch, so it runs without a device (the device pointers are never dereferenced)."""
    from opticalflow_amd import _lib
    lib = _lib.load()
    P = 1 << 20                                                  # a 16-byte aligned stand-in address
    n, H, W = 2, 33, 200
    need = lib.pwc_flow_compare_workspace_bytes(n, H, W)
    good = (ctypes.c_float * 4)(0.25, 0.5, 1.0, 2.0)

    def call(a=P, b=P, n=n, H=H, W=W, bsa=2 * H * W, bsb=2 * H * W, taus=good, ntau=4, epe_map=None, ws=P, ws_bytes=need, out=P):
        rc = lib.pwc_flow_compare(a, b, n, H, W, bsa, bsb, taus, ntau, epe_map, ws, ws_bytes, out, None)
        return rc, lib.pwc_last_error().decode()

    for kw in (dict(a=None), dict(b=None), dict(taus=None), dict(ws=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "null pointer" in msg, (kw, rc, msg)
    for kw in (dict(n=0), dict(H=0), dict(W=-1)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "bad shape" in msg, (kw, rc, msg)
    for ntau in (0, -1, 9):
        rc, msg = call(ntau=ntau)
        assert rc == PWC_EINVAL and "ntau %d outside 1..8" % ntau in msg, (ntau, rc, msg)
    for bad in (-0.5, math.nan, math.inf):
        rc, msg = call(taus=(ctypes.c_float * 4)(0.25, bad, 1.0, 2.0))
        assert rc == PWC_EINVAL and "threshold 1 is not a finite non-negative number" in msg, (bad, rc, msg)
    for kw in (dict(bsa=2 * H * W - 1), dict(bsb=2 * H * W - 1)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "batch stride" in msg, (kw, rc, msg)
    rc, msg = call(ws_bytes=need - 1)
    assert rc == PWC_EINVAL and "workspace needs %d bytes" % need in msg
    for kw in (dict(ws=P + 4), dict(out=P + 4)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "8-byte aligned" in msg, (kw, rc, msg)
    for kw in (dict(a=P + 2), dict(b=P + 1), dict(epe_map=P + 2)):
        rc, msg = call(**kw)
        assert rc == PWC_EINVAL and "4-byte aligned" in msg, (kw, rc, msg)
    big = lib.pwc_flow_compare_workspace_bytes(65536, 16, 64)
    rc, msg = call(n=65536, H=16, W=64, bsa=2048, bsb=2048, ws_bytes=big)
    assert rc == PWC_EINVAL and "65535" in msg
    rc, msg = call(n=4, H=16384, W=16384, bsa=1 << 40, bsb=1 << 40, ws_bytes=1 << 40)
    assert rc == PWC_EINVAL and "2^31" in msg


def test_python_wrapper_refuses_before_any_launch():
    from opticalflow_amd import PwcHipError, compare, ops
    a = torch.zeros(1, 2, 4, 8)
    with pytest.raises(PwcHipError, match="no CPU fallback"):
        ops.flow_compare(a, a)
    with pytest.raises(PwcHipError, match="no CPU fallback"):
        compare.compare_flows(a, a)
    with pytest.raises(TypeError, match="float32 only"):
        ops.flow_compare(a.half(), a.half())
    with pytest.raises(TypeError, match="float32"):
        ops.flow_compare(a.double(), a.double())
    with pytest.raises(ValueError, match=r"\[n,2,H,W\]"):
        ops.flow_compare(torch.zeros(1, 3, 4, 8), torch.zeros(1, 3, 4, 8))
    with pytest.raises(PwcHipError):
        compare.FlowComparer(1, 4, 8, "cpu")
    for bad in ((), (0.1,) * 9, (-1.0,), (math.nan,), (math.inf,)):
        with pytest.raises(ValueError, match="threshold"):
            ops.flow_compare_taus(bad)
    assert ops.flow_compare_taus([1, 0.5]) == (1.0, 0.5)


@pytest.mark.parametrize("name", sorted(FO.CASES))
def test_fixture_inputs_are_the_recipe(name):
    z = load_golden("g18_flow_compare.npz")
    c = FO.CASES[name]
    a, b = FO.make_inputs(name)
    assert a.shape == b.shape == (c["n"], 2, c["H"], c["W"]) and a.dtype == b.dtype == np.float32
    assert _oracle_rows(name)[0] == str(z[name + "/digest"]), "the recipe no longer gives the fixture's inputs"
    assert z[name + "/ref32"].shape == (c["n"] + 1, 8) and z[name + "/agree"].shape == (c["n"] + 1, 4)


def test_case_list_covers_the_kernel_paths():
    C = FO.CASES
    assert (C["one"]["H"], C["one"]["W"]) == (1, 1) and (C["tiny"]["H"], C["tiny"]["W"]) == (3, 5)
    assert (C["tile"]["n"], C["tile"]["H"], C["tile"]["W"]) == (2, 32, 128)
    assert (C["tile_p1"]["n"], C["tile_p1"]["H"], C["tile_p1"]["W"]) == (3, 33, 129)
    assert (C["ref"]["H"], C["ref"]["W"]) == (96, 128)
    pa, pb = C["strided"]["pad"]
    assert (C["strided"]["n"], C["strided"]["H"], C["strided"]["W"]) == (2, 33, 200) and pa != pb and pa % 4 == 0 and pb % 4 == 0
    assert any(p % 4 for p in C["strided_odd"]["pad"])
    assert C["w_odd"]["W"] % 4 != 0 and C["misaligned"]["W"] % 4 == 0 and C["misaligned"]["offset"] % 4 != 0
    assert len(FO.case_taus("tau1")) == 1 and len(FO.case_taus("tau8")) == 8
    assert {"equal", "a_zero", "b_const", "ties"} <= set(C)


@pytest.mark.parametrize("name", sorted(FO.CASES))
def test_oracle_agrees_with_the_reference(name):
    z = load_golden("g18_flow_compare.npz")
    dev_keys = [str(k) for k in z["deviation_keys"]]
    recorded = dict(zip(dev_keys, z["deviation"]))
    print("recorded largest deviations of the reference from the oracle:", recorded)
    for r, want in enumerate(_oracle_rows(name)[1]):
        ref = _reference_row(z, name, r)
        N = want["_"]["N"]
        # bit-equal: the maxima, every agreement percentage, min / max
        assert ref["Max abs diff"] == want["Max abs diff"] and ref["EPE max"] == want["EPE max"], (name, r)
        assert ref["Max abs diff"].dtype == np.float32 and want["Max abs diff"].dtype == np.float32
        assert {k: float(v) for k, v in ref["agreements"].items()} == want["agreements"], (name, r)
        st = z[name + "/stats"][r]                                  # [field][min, max, mean, std] as print_flow_stats formats them
        for i, f in enumerate(("a", "b")):
            assert st[i, 0] == want["stats"][f]["min"] and st[i, 1] == want["stats"][f]["max"], (name, r, f)
            scale = want["_"]["mean_abs"][f]
            for j, k in ((2, "mean"), (3, "std")):
                dev = abs(float(st[i, j]) - want["stats"][f][k]) / scale if scale else abs(float(st[i, j]))
                assert dev <= 4 * recorded[k] and dev <= N * 2.0 ** -24, (name, r, f, k, dev)
        for k in ("L2 diff", "MAE", "Relative L2 diff", "Relative MAE", "Pearson corr", "Cosine similarity", "EPE mean"):
            g, w = float(ref[k]), float(want[k])
            if np.isnan(w) or np.isnan(g):
                assert np.isnan(w) and np.isnan(g), (name, r, k, g, w)                   # NaN exactly where the reference has NaN
                continue
            dev = abs(g - w) / abs(w) if w != 0.0 else abs(g)
            assert dev <= 4 * recorded[k] and dev <= N * 2.0 ** -24, (name, r, k, g, w, dev)
    if name in ("a_zero", "b_const"):
        assert all(np.isnan(z[name + "/pearson"]))
    if name == "equal":
        assert np.all(z[name + "/agree"] == 100.0) and np.all(z[name + "/ref32"][:, 2] == 0.0)


def test_ties_are_decided_by_the_inclusive_comparison():
    a, b = FO.make_inputs("ties")
    e = FO.epe_map(a, b)
    assert set(np.unique(e)) == {0.25, 0.5, 1.0, 2.0, 3.0}
    row = _oracle_rows("ties")[1][-1]
    for t in FO.REF_TAUS:
        inclusive, strict = np.count_nonzero(e <= t), np.count_nonzero(e < t)
        assert inclusive > strict and row["agreements"]["agree@%s" % t] == inclusive / e.size * 100.0


def test_ordinary_cases_meet_the_generator_conditions():
    for name in FO.ORDINARY:
        a, b = FO.make_inputs(name)
        rows = FO.rows(a, b, FO.case_taus(name)) if "taus" in FO.CASES[name] else _oracle_rows(name)[1]
        assert all(r["_"]["nearest_tau"] > 1e-6 for r in rows), name
        mid = [v for v in rows[-1]["agreements"].values() if 5.0 < v < 95.0]
        assert len(mid) >= min(2, len(FO.case_taus(name))), (name, rows[-1]["agreements"])
        assert all(np.isnan(r["_"]["kappa"]) or r["_"]["kappa"] <= 100.0 for r in rows)


@pytest.mark.parametrize("name", ("tiny", "tile_p1", "ref", "b_const", "a_zero", "equal", "ties"))
def test_formatting_reproduces_the_reference_lines(name):
    from opticalflow_amd import compare
    z = load_golden("g18_flow_compare.npz")
    c = FO.CASES[name]
    for r in range(c["n"] + 1):
        printed, drawn, stats = (s.split("\n") for s in str(z[name + "/lines"][r]).split("\f"))
        shape = ((c["n"] if r == c["n"] else 1) * c["H"], c["W"], 2)
        ref = _reference_row(z, name, r)
        assert compare.format_report(ref, shape, shape) == printed
        assert compare.format_report(ref, shape, shape, drawn=True) == drawn
        st = z[name + "/stats"][r]
        got = []
        for i, tag in enumerate(("pth", "onnx")):
            got += compare.format_stats(tag, shape, dict(zip(FO.STAT_KEYS, st[i])))
        assert got == stats
    assert printed[0].startswith("L2 diff           : ") and printed[-1].startswith("Agreement @ EPE<=2.00 : ") and len(printed) == 13
    assert drawn[0] == "flow_pth shape : %s" % (shape,) and drawn[2] == "" and len(drawn) == 12 and len(stats) == 10


def test_to_host_keys_and_threshold_formatting():
    from opticalflow_amd import compare, ops
    taus = (0.25, 0.5, 1.0, 2.0)
    rec = torch.arange(3 * ops.FLOW_COMPARE_FIELDS, dtype=torch.float64).reshape(3, ops.FLOW_COMPARE_FIELDS)
    per_sample, batch = compare.FlowComparison(rec, taus, (2, 2, 4, 8)).to_host()
    assert len(per_sample) == 2
    for row, m in zip(rec.tolist(), per_sample + [batch]):
        assert list(m) == REF_KEYS + ["stats"]
        assert list(m["agreements"]) == ["agree@0.25", "agree@0.5", "agree@1.0", "agree@2.0"]
        assert m["agreements"]["agree@1.0"] == row[ops.FC_AGREE0 + 2] and m["L2 diff"] == row[ops.FC_L2]
        assert m["Max abs diff"] == row[ops.FC_MAX_ABS] and m["EPE max"] == row[ops.FC_EPE_MAX] and m["Pearson corr"] == row[ops.FC_PEARSON]
        assert set(m["stats"]) == {"a", "b"} and list(m["stats"]["a"]) == ["min", "max", "mean", "std"]
        assert m["stats"]["b"]["std"] == row[ops.FC_STD_B] and m["stats"]["a"]["min"] == row[ops.FC_MIN_A]
    _, one = compare.FlowComparison(rec, (0.1, 3, 1.25), (2, 2, 4, 8)).to_host()
    assert list(one["agreements"]) == ["agree@0.1", "agree@3.0", "agree@1.25"]
    assert [compare.agreement_key(t) for t in taus] == [f"agree@{t}" for t in taus]
