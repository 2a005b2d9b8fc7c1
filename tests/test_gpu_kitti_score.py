"""GPU checks of the device-side KITTI scoring: the fused EPE / Fl-all kernel (csrc/pwc_kitti_score.hip) against the reference's own
float64 numbers (g12 fixture) and, exactly, against the host functions' float32 arithmetic on ops.flow_upsample's output; the two
ground-truth forms, flow_out, reproducibility; kitti.evaluate_stream and evaluate_pairs_sharded(route="hip") against the host loop."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import kitti_score_oracle as KO

pytestmark = pytest.mark.gpu

CASES = ("smooth", "rough", "odd", "ref_unpad", "identity", "sparse", "empty", "all_valid", "large")


def _field(n, hq, wq, seed, amp=6.0, noise=0.5):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, hq), torch.linspace(0, 1, wq), indexing="ij")
    ph = torch.rand(n, 2, generator=g) * 6.0
    f = torch.stack([torch.stack((amp * torch.sin(3 * xx + 2 * yy + ph[b, 0]), amp * torch.cos(2 * xx - 3 * yy + ph[b, 1]))) for b in range(n)])
    return f + noise * torch.randn(n, 2, hq, wq, generator=g)


def _make_gt(full, seed, validity=0.3):
    """uint16 KITTI samples [n,H,W,3] around a full-resolution flow [n,2,H,W]: the flow plus an error vector of uniform length
    0..6 px and uniform angle (about half of the valid pixels are outliers), quantised to 1/64 px, valid on `validity` of the pixels."""
    from opticalflow_amd import kitti
    g = np.random.default_rng(seed)
    n, _, H, W = full.shape
    out = np.zeros((n, H, W, 3), np.uint16)
    for b in range(n):
        length, angle = g.uniform(0, 6, (H, W)), g.uniform(0, 2 * np.pi, (H, W))
        gt = full[b].transpose(1, 2, 0).astype(np.float64) + np.stack([length * np.cos(angle), length * np.sin(angle)], axis=-1)
        out[b] = kitti.encode_flow_rgb16(np.round(gt * 64.0) / 64.0, g.uniform(0, 1, (H, W)) < validity)
    return out


def _host_totals(full, gt16):
    """kitti.epe_metric / kitti.fl_all_metric's float32 arithmetic on a downloaded full-resolution flow, kept as the raw totals:
    per sample (float64 sum of the float32 epe values over valid pixels, #valid, #valid outliers)."""
    from opticalflow_amd import kitti
    rows = []
    for b in range(full.shape[0]):
        fg, valid = kitti.decode_flow_rgb16(gt16[b])
        fp = np.ascontiguousarray(full[b].transpose(1, 2, 0))
        d = fp - fg
        epe = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
        mag = np.sqrt(fg[..., 0] ** 2 + fg[..., 1] ** 2)
        outlier = (epe > np.maximum(3.0, 0.05 * mag)) & valid
        assert epe.dtype == np.float32 and mag.dtype == np.float32 and (0.05 * mag).dtype == np.float32
        nv, no = int(np.count_nonzero(valid)), int(np.count_nonzero(outlier))
        if nv:                                            # the same numbers through the host functions themselves
            assert kitti.fl_all_metric(fp, fg, valid) == 100.0 * no / nv
            np.testing.assert_allclose(kitti.epe_metric(fp, fg, valid), epe[valid].astype(np.float64).sum() / nv, rtol=1e-6)
        rows.append((float(epe[valid].astype(np.float64).sum()), nv, no))
    return rows


def _score(fq, ch, cw, H, W, gt, dev, **kw):
    from opticalflow_amd import ops
    gt_t = torch.as_tensor(gt).to(dev)
    out, s, nv, no = ops.kitti_score(torch.as_tensor(fq).to(dev) if not torch.is_tensor(fq) or not fq.is_cuda else fq, ch, cw, H, W, gt_t,
                                     raw=True, **kw)
    return out.cpu().numpy(), s.cpu().numpy().copy(), nv.cpu().numpy().copy(), no.cpu().numpy().copy()


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_reference_g12(gpu_device, name):
    z = load_golden("g12_kitti_score.npz")
    ch, cw, H, W = (int(v) for v in z[name + "/geom"])
    fq, gt = z[name + "/flow_q"], z[name + "/gt"]
    knife = KO.score(fq, ch, cw, H, W, gt)["knife_edge"]
    out, s, nv, no = _score(fq, ch, cw, H, W, gt, gpu_device)
    ref_epe, ref_nv, ref_no = z[name + "/epe"][0], z[name + "/n_valid"], z[name + "/n_outlier"]
    print("%s: epe hip %s reference %s; outliers hip %s reference %s of %s valid, knife-edge %s" % (name, s / np.maximum(nv, 1), ref_epe, no, ref_no, nv, knife))
    assert np.array_equal(nv, ref_nv)
    assert np.all(np.abs(no - ref_no) <= knife)
    for b in range(len(nv)):
        if nv[b] == 0:
            assert s[b] == 0.0 and no[b] == 0 and np.isnan(out[b, 0]) and np.isnan(out[b, 1]) and np.isnan(ref_epe[b])
            continue
        np.testing.assert_allclose(s[b] / nv[b], ref_epe[b], rtol=1e-5, atol=0)
        # the float32 results are the ratios of the raw totals, rounded once
        assert out[b, 0] == np.float32(s[b] / nv[b]) and out[b, 1] == np.float32(100.0 * no[b] / nv[b])
    if name == "empty":
        assert nv[0] > 0 and nv[2] > 0                    # the neighbours of the empty sample are scored as usual (checked above)


# (n, out_h, out_w, crop_h, crop_w, Hq, Wq)
EXACT = [(3, 61, 131, 16, 33, 16, 48), (2, 100, 150, 25, 38, 32, 48), (2, 375, 1242, 87, 282, 96, 320), (2, 375, 1242, 94, 311, 96, 320),
         (2, 24, 40, 24, 40, 24, 40)]


def _exact(fq_dev, ch, cw, H, W, dev, seed):
    from opticalflow_amd import ops
    full = ops.flow_upsample(fq_dev, ch, cw, H, W).cpu().numpy()
    gt16 = _make_gt(full, seed)
    host = _host_totals(full, gt16)
    out, s, nv, no = _score(fq_dev, ch, cw, H, W, gt16, dev)
    for b, (hs, hv, ho) in enumerate(host):
        print("sample %d: sum hip %.12g host %.12g; valid %d / %d; outliers %d / %d" % (b, s[b], hs, nv[b], hv, no[b], ho))
        assert hv > 0 and 0.2 < ho / hv < 0.8
        # +, -, x, sqrt and compare are correctly rounded in float32 on both sides: no allowance on the counts
        assert nv[b] == hv and no[b] == ho
        np.testing.assert_allclose(s[b], hs, rtol=1e-10, atol=0)           # summation order only
    return full, gt16, (s, nv, no)


@pytest.mark.parametrize("n,H,W,ch,cw,Hq,Wq", EXACT)
def test_counts_equal_host_float32_arithmetic(gpu_device, n, H, W, ch, cw, Hq, Wq):
    fq = _field(n, Hq, Wq, 7 * H + W + ch).to(gpu_device)
    _exact(fq, ch, cw, H, W, gpu_device, seed=H + cw)


def test_strided_flow_q_view(gpu_device):
    """flow_q as a view into a larger buffer: batch stride above 2*Hq*Wq."""
    buf = torch.zeros((3, 5, 32, 48), device=gpu_device)
    buf[:, 1:3] = _field(3, 32, 48, 99).to(gpu_device)
    view = buf[:, 1:3]
    assert view.stride(0) == 5 * 32 * 48 and not view.is_contiguous()
    _, _, strided = _exact(view, 25, 38, 100, 150, gpu_device, seed=5)
    _, _, dense = _exact(view.contiguous(), 25, 38, 100, 150, gpu_device, seed=5)
    for a, b in zip(strided, dense):
        assert a.tobytes() == b.tobytes()


def test_ground_truth_forms_and_flow_out_and_reproducibility(gpu_device):
    from opticalflow_amd import kitti, ops
    n, H, W, ch, cw, Hq, Wq = 3, 61, 131, 16, 33, 16, 48
    fq = _field(n, Hq, Wq, 321).to(gpu_device)
    full = ops.flow_upsample(fq, ch, cw, H, W)
    gt16 = _make_gt(full.cpu().numpy(), 17)
    gt16[1, ..., 2] = 0                                                      # one sample without a valid pixel
    png = _score(fq, ch, cw, H, W, gt16, gpu_device)
    again = _score(fq, ch, cw, H, W, gt16, gpu_device)
    for a, b in zip(png[1:], again[1:]):                                     # two launches: byte-identical totals
        assert a.tobytes() == b.tobytes()
    assert np.isnan(png[0][1]).all() and not np.isnan(png[0][[0, 2]]).any()
    # the float route on the decoded ground truth: byte-identical raw totals
    dec = [kitti.decode_flow_rgb16(gt16[b]) for b in range(n)]
    planes = np.ascontiguousarray(np.stack([d[0].transpose(2, 0, 1) for d in dec]))
    valid = torch.from_numpy(np.stack([d[1] for d in dec])).to(gpu_device)
    flt = _score(fq, ch, cw, H, W, planes, gpu_device, valid=valid)
    for a, b in zip(png[1:], flt[1:]):
        assert a.tobytes() == b.tobytes()
    assert png[0].tobytes() == flt[0].tobytes()
    # valid=None: every pixel counts
    allv = _score(fq, ch, cw, H, W, planes, gpu_device)
    assert list(allv[2]) == [H * W] * n
    # flow_out: the full-resolution flow as well, bit-identical to flow_upsample, same totals
    fo = torch.full((n, 2, H, W), float("nan"), device=gpu_device)
    with_fo = _score(fq, ch, cw, H, W, gt16, gpu_device, flow_out=fo)
    assert torch.equal(fo, full)
    for a, b in zip(png[1:], with_fo[1:]):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        ops.kitti_score(fq, ch, cw, H, W, torch.as_tensor(gt16).to(gpu_device), valid=valid)


@pytest.fixture(scope="module")
def nets(gpu_device):
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    out = {}
    for prec in ("fp32", "fp16-strict"):
        net = PWCDCNet(precision=prec) if prec != "fp32" else PWCDCNet()
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=2, gain=0.85, bias_std=0.02))
        out[prec] = net.to(gpu_device).eval()
    return out


def _pairs(count, seed, H=100, W=150):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))
            for _ in range(count)]


@pytest.mark.parametrize("prec,form", [("fp32", "png16"), ("fp16-strict", "png16"), ("fp32", "float")])
def test_evaluate_stream_equals_host_loop(gpu_device, nets, prec, form):
    """5 samples at batch 2 (tail batch n = 1): rows against host metrics of the full-resolution flows a GraphedInfer(batch=2)
    produces on the same inputs."""
    from opticalflow_amd import kitti
    net = nets[prec]
    pairs = _pairs(5, 31)
    pipe = kitti.GraphedInfer(net, 100, 150, gpu_device, batch=2)
    full = torch.cat([pipe(u8).cpu() for u8 in kitti.BatchStream(pairs, gpu_device, 2)], 0).numpy()
    gt16 = _make_gt(full, 41)
    gt16[3, ..., 2] = 0                                                      # a sample whose validity channel is all zero
    host = _host_totals(full, gt16)
    if form == "png16":
        samples = [(a, b, gt16[i]) for i, (a, b) in enumerate(pairs)]
    else:
        samples = [(a, b, kitti.decode_flow_rgb16(gt16[i])) for i, (a, b) in enumerate(pairs)]
    epe, fl, rows = kitti.evaluate_stream(net, samples, gpu_device, batch=2)
    assert len(rows) == 5
    for i, ((hs, hv, ho), (e, f)) in enumerate(zip(host, rows)):
        print("sample %d: epe %.9g host %.9g; fl %.9g host %s" % (i, e, hs / hv if hv else float("nan"), f, 100.0 * ho / hv if hv else None))
        if hv == 0:
            assert i == 3 and np.isnan(e) and np.isnan(f)
            continue
        assert f == 100.0 * ho / hv                                          # the counts are exact
        np.testing.assert_allclose(e, kitti.epe_metric(full[i].transpose(1, 2, 0), *kitti.decode_flow_rgb16(gt16[i])), rtol=1e-6)
    assert epe == float(np.nanmean([r[0] for r in rows])) and fl == float(np.nanmean([r[1] for r in rows]))
    assert not np.isnan(epe) and not np.isnan(fl)


def test_scored_infer_table_and_keep_flow(gpu_device, nets):
    from opticalflow_amd import kitti
    net = nets["fp32"]
    pairs = _pairs(2, 57)
    ref = kitti.GraphedInfer(net, 100, 150, gpu_device, batch=2)
    u8 = next(iter(kitti.BatchStream(pairs, gpu_device, 2)))
    full = ref(u8).clone()
    gt16 = _make_gt(full.cpu().numpy(), 3)
    pipe = kitti.ScoredInfer(net, 100, 150, gpu_device, batch=2, rows=6, keep_flow=True)
    assert kitti.ScoredInfer(net, 100, 150, gpu_device, batch=2).flow_full is None           # default: no full-resolution flow
    scores = pipe(u8, torch.from_numpy(gt16).to(gpu_device), 4).cpu().numpy()
    assert torch.equal(pipe.flow_full, full)
    s, nv, no = pipe.results()
    host = _host_totals(full.cpu().numpy(), gt16)
    assert np.all(nv[:4] == 0) and [int(v) for v in nv[4:]] == [h[1] for h in host] and [int(v) for v in no[4:]] == [h[2] for h in host]
    for b in range(2):
        assert scores[b, 0] == np.float32(s[4 + b] / nv[4 + b]) and scores[b, 1] == np.float32(100.0 * no[4 + b] / nv[4 + b])
    with pytest.raises(ValueError):
        pipe(u8, torch.from_numpy(gt16).to(gpu_device), 5)                   # rows 5..6 do not fit a table of 6


def test_sharded_hip_route_equals_host_route(gpu_device, nets):
    """World size 1, no process group."""
    from opticalflow_amd import kitti
    net = nets["fp32"]
    pairs = _pairs(3, 77)
    stream = kitti.ShardedStream.for_model(net, 100, 150, gpu_device, batch=2, score=True)
    full = torch.cat([f.cpu() for _, f, _ in stream.run(pairs)], 0).numpy()
    gt16 = _make_gt(full, 9)
    samples = [(a, b) + kitti.decode_flow_rgb16(gt16[i]) for i, (a, b) in enumerate(pairs)]
    host = kitti.evaluate_pairs_sharded(stream, samples)
    hip = kitti.evaluate_pairs_sharded(stream, samples, route="hip")
    print("host %s hip %s" % (host, hip))
    assert hip[2] == host[2] == 3
    np.testing.assert_allclose(hip[:2], host[:2], rtol=1e-6, atol=0)
    plain = kitti.ShardedStream(gpu_device, batch=2, infer=stream.infer)
    with pytest.raises(ValueError):
        kitti.evaluate_pairs_sharded(plain, samples, route="hip")
