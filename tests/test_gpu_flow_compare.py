"""GPU checks of the device flow-comparison report (csrc/pwc_flow_compare.hip, ops.flow_compare, opticalflow_amd.compare) against the
float64 oracle (tests/flow_compare_oracle.py, which states the derived tolerances) and the reference's recorded values (g18 fixture):
every case per sample and for the batch row, the EPE map, bit-reproducibility, graph replay, compare_models, refused inputs."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import flow_compare_oracle as FO

pytestmark = pytest.mark.gpu
_ORACLE = {}


def _oracle(name):
    """(a, b, rows for the case's thresholds, EPE map), computed once and left unchanged"""
    if name not in _ORACLE:
        a, b = FO.make_inputs(name)
        _ORACLE[name] = (a, b, FO.rows(a, b, FO.case_taus(name)), FO.epe_map(a, b))
    return _ORACLE[name]


def _place(x, pad, offset, dev):
    """x [n,2,H,W] on the device with `pad` extra elements in the batch stride, starting `offset` elements past a 16-byte boundary"""
    n, _, H, W = x.shape
    bs = 2 * H * W + pad
    buf = torch.full((offset + n * bs,), float("nan"), dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:].as_strided((n, 2, H, W), (bs, H * W, W, 1))
    view.copy_(torch.from_numpy(x))
    return view


def _device_inputs(name, dev):
    c = FO.CASES[name]
    a, b = _oracle(name)[:2]
    pa, pb = c.get("pad", (0, 0))
    off = c.get("offset", 0)
    return _place(a, pa, off, dev), _place(b, pb, off, dev)


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("name", sorted(FO.CASES))
def test_cases_against_oracle_and_reference(gpu_device, name):
    from opticalflow_amd import compare, ops
    z = load_golden("g18_flow_compare.npz")
    c = FO.CASES[name]
    taus = FO.case_taus(name)
    _, _, want_rows, want_map = _oracle(name)
    da, db = _device_inputs(name, gpu_device)
    assert da.data_ptr() % 16 == 4 * c.get("offset", 0)
    cmp_map = compare.compare_flows(da, db, taus, epe_map=True)
    cmp_plain = compare.compare_flows(da, db, taus)
    again = compare.compare_flows(da, db, taus)
    # the EPE map is the oracle's float32 map bit for bit; the record does not depend on it; two runs give the same bits
    assert cmp_map.epe_map.dtype == torch.float32 and np.array_equal(cmp_map.epe_map.cpu().numpy().view(np.int32), want_map.view(np.int32))
    assert cmp_plain.epe_map is None
    assert torch.equal(_bits(cmp_map.record), _bits(cmp_plain.record)) and torch.equal(_bits(again.record), _bits(cmp_plain.record))
    per_sample, batch = cmp_plain.to_host()
    assert len(per_sample) == c["n"]
    raw = cmp_plain.record.cpu().numpy()
    worst = {}
    for r, (got, want) in enumerate(zip(per_sample + [batch], want_rows)):
        used = FO.check_row(got, want, where="%s row %d" % (name, r))
        for k, v in used.items():
            worst[k] = max(worst.get(k, 0.0), v)
        x = want["_"]
        assert raw[r, ops.FC_N] == x["N"] and raw[r, ops.FC_P] == x["P"]
        assert list(raw[r, ops.FC_COUNT0:ops.FC_COUNT0 + len(taus)]) == x["counts"]
        assert np.all(raw[r, ops.FC_COUNT0 + len(taus):ops.FC_COUNT0 + 8] == 0) and np.all(np.isnan(raw[r, ops.FC_AGREE0 + len(taus):ops.FC_AGREE0 + 8]))
        if taus == FO.REF_TAUS:
            # ... and bit-equal to what the reference itself returned
            ref32 = z[name + "/ref32"][r]
            assert got["Max abs diff"] == float(ref32[2]) and got["EPE max"] == float(ref32[7])
            assert list(got["agreements"].values()) == list(z[name + "/agree"][r])
            st = z[name + "/stats"][r]
            for i, f in enumerate(("a", "b")):
                assert got["stats"][f]["min"] == float(st[i, 0]) and got["stats"][f]["max"] == float(st[i, 1])
            assert np.isnan(got["Pearson corr"]) == np.isnan(z[name + "/pearson"][r])
    print("%s: largest deviation from the oracle in units of the derived bound: %s"
          % (name, {(k if isinstance(k, str) else "%s %s" % k[1:]): "%.3g" % v for k, v in worst.items() if v > 0}))


def test_comparer_replayed_from_a_graph_equals_the_eager_call(gpu_device):
    from opticalflow_amd import compare
    dev = gpu_device
    a, b = _oracle("tile_p1")[:2]
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    eager = compare.compare_flows(da, db, epe_map=True)
    flipped = compare.compare_flows(db.flip(0).contiguous(), da.flip(0).contiguous(), epe_map=True)
    cmp = compare.FlowComparer(*((a.shape[0],) + a.shape[2:]), dev, epe_map=True)
    sa, sb = da.clone(), db.clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        cmp.run(sa, sb)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cmp.run(sa, sb)
    cmp.record.fill_(float("nan"))
    cmp.epe_map.fill_(-1.0)
    graph.replay()
    assert torch.equal(_bits(out.record), _bits(eager.record)) and torch.equal(out.epe_map, eager.epe_map)
    sa.copy_(db.flip(0))                                         # new contents, same graph
    sb.copy_(da.flip(0))
    graph.replay()
    assert torch.equal(_bits(out.record), _bits(flipped.record)) and torch.equal(out.epe_map, flipped.epe_map)
    assert not torch.equal(_bits(flipped.record), _bits(eager.record))
    with pytest.raises(ValueError):
        cmp.run(da[:2], db[:2])


def test_compare_models_equals_compare_flows_of_the_two_forwards(gpu_device):
    from opticalflow_amd import PWCDCNet, compare
    from opticalflow_amd.weights import synthetic_state_dict
    dev = gpu_device
    nets = []
    for precision in ("fp32", "fp16-strict"):
        net = PWCDCNet(precision=precision)
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
        nets.append(net.to(dev).eval())
    x = torch.rand(1, 6, 64, 64, generator=torch.Generator().manual_seed(11)).to(dev)
    got = compare.compare_models(nets[0], nets[1], x, epe_map=True)
    fa, fb = nets[0](x), nets[1](x)
    want = compare.compare_flows(fa, fb, epe_map=True)
    assert tuple(got.shape) == tuple(fa.shape) == (1, 2, 16, 16)
    assert torch.equal(_bits(got.record), _bits(want.record)) and torch.equal(got.epe_map, want.epe_map)
    _, batch = got.to_host()
    assert np.isfinite(batch["EPE mean"]) and batch["EPE mean"] <= batch["EPE max"] and batch["agreements"]["agree@2.0"] == 100.0


def test_tool_prints_the_report_of_two_flo_files(gpu_device, tmp_path, capsys):
    import os
    import sys
    from conftest import REPO
    from opticalflow_amd import compare, write_flo
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import compare_flows as tool
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))
    a, b, want_rows, _ = _oracle("tiny")
    pa, pb = str(tmp_path / "a.flo"), str(tmp_path / "b.flo")
    write_flo(pa, a[0].transpose(1, 2, 0))
    write_flo(pb, b[0].transpose(1, 2, 0))
    tool.main([pa, pb, "--device", str(gpu_device)])
    out = capsys.readouterr().out.splitlines()
    _, batch = compare.compare_flows(torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device)).to_host()
    assert out[:13] == compare.format_report(batch, (3, 5, 2), (3, 5, 2))
    assert out[13] == "[a.flo] shape=(3, 5, 2)" and out[18] == "[b.flo] shape=(3, 5, 2)" and len(out) == 23
    assert out[2] == "Max abs diff      : %s" % float(want_rows[-1]["Max abs diff"])
    assert out[9:13] == ["Agreement @ EPE<=%4.2f : %6.2f%%" % (t, v) for t, v in zip(FO.REF_TAUS, want_rows[-1]["agreements"].values())]


def test_refused_inputs_raise_before_any_launch(gpu_device):
    from opticalflow_amd import PwcHipError, compare, ops
    dev = gpu_device
    a = torch.zeros(2, 2, 8, 12, device=dev)
    with pytest.raises(TypeError, match="float32 only"):
        compare.compare_flows(a.half(), a.half())
    with pytest.raises(TypeError, match="float32 only"):
        compare.compare_flows(a, a.half())
    with pytest.raises(PwcHipError, match="no CPU fallback"):
        compare.compare_flows(a, a.cpu())
    with pytest.raises(PwcHipError, match="no CPU fallback"):
        compare.compare_flows(a.cpu(), a)
    with pytest.raises(ValueError, match="one shape"):
        compare.compare_flows(a, a[:, :, :, :8].contiguous())
    with pytest.raises(ValueError, match="one shape"):
        compare.compare_flows(a, a[:1])
    with pytest.raises(ValueError, match="dense"):
        compare.compare_flows(a[:, :, :, ::2], a[:, :, :, ::2])
    with pytest.raises(ValueError, match="epe_map"):
        ops.flow_compare(a, a, epe_map=torch.zeros(2, 8, 12, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError, match="workspace has"):
        ops.flow_compare(a, a, workspace=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        ops.flow_compare(a, a, out=torch.zeros(3, 44, device=dev))
    with pytest.raises(ValueError, match="threshold"):
        compare.compare_flows(a, a, taus=())
