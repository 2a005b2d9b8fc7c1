"""GPU checks of the flow pictures (csrc/pwc_flowviz.hip, opticalflow_amd/flowviz.py): the colour image, the statistics and the arrow
grid against the reference's own outputs (tests/golden/g13_flowviz.npz) under the knife-edge rule of tests/flowviz_oracle.py, the
3-bytes-per-pixel output layout at every alignment, bit-exactness of the arrow vectors against harness.cv2_resize_linear, and the
rendered FlowStream against the eager calls."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowviz_oracle as FO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_flowviz.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _nchw(field, dev):
    """[h,w,2] numpy -> [1,2,h,w] device tensor (bit-exact, signed zeros included)."""
    return torch.from_numpy(np.ascontiguousarray(field.transpose(2, 0, 1))).unsqueeze(0).to(dev)


def _batch3(gold, dev):
    f = _nchw(gold["field/odd"], dev)
    return torch.cat([f, f.flip(-1) * 0.5, f.flip(-2) * 2.0 + 0.25], 0).contiguous()


# ---- 1. colour against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(FO.COLOR_CASES))
def test_color_is_the_references_up_to_knife_edges(gold, dev, case):
    from opticalflow_amd import flowviz
    fname, crop = FO.COLOR_CASES[case]
    flow = _nchw(gold["field/" + fname], dev)
    for ci, clip in enumerate(FO.CLIPS):
        got = flowviz.flow_to_color(flow, clip_flow=clip, crop=crop)
        ref = gold["color/%s/%d" % (case, ci)]
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + ref.shape and got.is_contiguous()
        _, _, knife = FO.color(FO.cropped(gold["field/" + fname], crop), clip)
        d = got[0].cpu().numpy().astype(np.int64) - ref
        print("%s clip %s: %d of %d channels differ, %d knife-edge" % (case, clip, np.count_nonzero(d), d.size, knife.sum()))
        assert np.abs(d).max() <= 1 and not (d != 0)[~knife].any()
        if case == "zero":
            assert (got == 255).all()
        if case == "axis":
            px = got[0].cpu().numpy()
            assert (px[0] == (255, 0, 0)).all() and (px[1] == (255, 0, 43)).all()      # v = +0.0 and v = -0.0: the wheel's wrap
        if case == "one":
            assert np.array_equal(got[0].cpu().numpy(), ref)


# ---- 2. layout ------------------------------------------------------------------------------------------------------------------
def test_color_batch_of_unaligned_samples_equals_single_calls(gold, dev):
    from opticalflow_amd import flowviz
    f3 = _batch3(gold, dev)
    assert (37 * 53 * 3) % 4 == 3                                   # samples 1 and 2 start at unaligned addresses
    for clip in FO.CLIPS:
        got = flowviz.flow_to_color(f3, clip_flow=clip)
        for b in range(3):
            assert torch.equal(got[b], flowviz.flow_to_color(f3[b:b + 1].clone(), clip_flow=clip)[0])
    assert not torch.equal(got[0], got[1])


def test_color_batch_stride_and_crop_from_a_larger_map(gold, dev):
    from opticalflow_amd import flowviz
    f3 = _batch3(gold, dev)
    arena = torch.full((3, 5, 37, 53), 7.0, device=dev)
    arena[:, 1:3] = f3
    view = arena[:, 1:3]
    assert not view.is_contiguous()
    assert torch.equal(flowviz.flow_to_color(view), flowviz.flow_to_color(f3))
    big = _nchw(gold["field/smooth"], dev)
    for crop in ((77, 130), (1, 1), (96, 1), (5, 160)):
        small = big[:, :, :crop[0], :crop[1]].contiguous()
        for clip in FO.CLIPS:
            assert torch.equal(flowviz.flow_to_color(big, clip_flow=clip, crop=crop), flowviz.flow_to_color(small, clip_flow=clip))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_color_writes_only_its_slice_of_a_larger_buffer(gold, dev, offset):
    from opticalflow_amd import flowviz
    f3 = _batch3(gold, dev)
    for flow in (f3, f3[:1, :, :1, :1].contiguous(), f3[:2, :, :3, :7].contiguous()):
        n, _, h, w = flow.shape
        total = n * h * w * 3
        buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        lo = 16 + offset
        out = buf[lo:lo + total].view(n, h, w, 3)
        assert out.data_ptr() % 4 == offset
        got = flowviz.flow_to_color(flow, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert (buf[:lo] == 0xA5).all() and (buf[lo + total:] == 0xA5).all()
        assert torch.equal(out, flowviz.flow_to_color(flow))


# ---- 3. statistics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(FO.DOMINANT_CASES))
def test_stats_maximum_count_and_mean(gold, dev, case):
    from opticalflow_amd import flowviz, ops
    fname, crop, thr = FO.DOMINANT_CASES[case]
    flow = _nchw(gold["field/" + fname], dev)
    cf = FO.cropped(gold["field/" + fname], crop)
    rec = ops.flow_stats(flow, crop=crop, threshold=thr)
    u, v = _nchw(cf, dev)[0]
    assert rec[0, 0].item() == torch.sqrt(u * u + v * v).amax().item()              # exactly: max of correctly rounded fp32 radii
    _, n, mean, knife = FO.stats(cf, thr)
    assert knife == 0
    mean_d, count_d = flowviz.dominant_direction(flow, threshold=thr, crop=crop)
    assert count_d.dtype == torch.int64 and count_d.item() == n == int(gold["domn/" + case])
    got = mean_d[0].cpu().numpy().astype(np.float64)
    print(case, "mean", got, "oracle", mean, "count", n)
    assert (np.abs(got - mean) <= 2.0 ** -23 * np.abs(mean) + 1e-9).all()
    if n == 0:
        assert (got == 0).all()
    # with the clip the maximum is the clipped radius: 6 fp32 roundings in the chain, bound 1e-6 relative
    mx = FO.stats(cf, thr, clip_flow=4.0)[0]
    assert abs(ops.flow_stats(flow, crop=crop, clip_flow=4.0)[0, 0].item() - mx) <= 1e-6 * mx
    assert mx <= 4.0 * (1 + 1e-6)


def test_stats_batch_and_more_than_one_tile(gold, dev):
    from opticalflow_amd import ops
    f3 = _batch3(gold, dev)                                           # 37 x 53: three tile rows; smooth 96 x 160: 6 x 3 tiles
    rec = ops.flow_stats(f3)
    for b in range(3):
        assert torch.equal(rec[b], ops.flow_stats(f3[b:b + 1].clone())[0])
    with pytest.raises(ValueError):
        ops.flow_stats(f3, workspace=torch.empty(8, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.flow_color(f3, rec, out=torch.empty((3, 37, 53, 4), dtype=torch.uint8, device=dev))


# ---- 4. arrows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(FO.QUIVER_CASES))
def test_quiver_vectors_exact_tips_and_flags_up_to_knife_edges(gold, dev, case):
    from opticalflow_amd import flowviz, harness
    fname, crop, (H, W), step, style, scale, min_mag, dom, thr, vs = FO.QUIVER_CASES[case]
    flow = _nchw(gold["field/" + fname], dev)
    cf = FO.cropped(gold["field/" + fname], crop)
    d = torch.from_numpy(gold["dom/" + dom]).view(1, 2).to(dev) if dom else None
    a = flowviz.quiver_arrows(flow, (H, W), step=step, scale=scale, min_mag=min_mag, crop=crop, style=style, dominant=d,
                              angle_threshold=thr, vec_scale=vs)
    gy, gx = -(-H // step), -(-W // step)
    assert tuple(a.vec.shape) == (1, gy, gx, 2) and tuple(a.tip.shape) == (1, gy, gx, 2) and tuple(a.flags.shape) == (1, gy, gx)
    assert a.vec.dtype == torch.float32 and a.tip.dtype == torch.int32 and a.flags.dtype == torch.uint8
    # vectors: harness.cv2_resize_linear with torch on the device, sampled at the grid points, times vec_scale -- bit for bit
    h, w = cf.shape[:2]
    sx, sy = vs if vs is not None else (float(W) / float(w), float(H) / float(h))
    planes = _nchw(cf, dev)[0]
    ru = harness.cv2_resize_linear(planes[0].contiguous(), H, W)[::step, ::step] * sx
    rv = harness.cv2_resize_linear(planes[1].contiguous(), H, W)[::step, ::step] * sy
    assert torch.equal(a.vec[0].view(torch.int32), torch.stack((ru, rv), -1).contiguous().view(torch.int32))
    # tips and flags: the reference's own arrow list
    gain, rule = FO.gain_rule(style, scale)
    o = FO.quiver(cf, (H, W), step, gain, rule, min_mag, vec_scale=vs, dominant=gold["dom/" + dom] if dom else None, angle_threshold=thr)
    flags = a.flags[0].cpu().numpy()
    keep, aligned, tip = (flags & 1).astype(bool), (flags & 2).astype(bool), a.tip[0].cpu().numpy().astype(np.int64)
    rkeep, rtip, raligned = gold["q/%s/keep" % case], gold["q/%s/tip" % case], gold["q/%s/aligned" % case]
    assert not (keep != rkeep)[~o["knife_keep"]].any()
    both = keep & rkeep
    dt = np.abs(tip - rtip)
    print(case, "kept", keep.sum(), "of", keep.size, "tips differing", np.count_nonzero(dt[both]), "knife-edge", o["knife_tip"].sum())
    assert dt[both].max(initial=0) <= 1 and not (dt != 0)[both[..., None] & ~o["knife_tip"]].any()
    assert not (aligned != raligned)[both & ~o["knife_aligned"]].any()
    if d is None:
        assert aligned.all()                                          # no dominant direction: the reference's default red


def test_quiver_batch_zero_dominant_and_argument_errors(gold, dev):
    from opticalflow_amd import flowviz, ops
    f3 = _batch3(gold, dev)
    dom, _ = flowviz.dominant_direction(f3)
    assert dom.stride(0) == 4                                         # rows of the stats record, read in place
    a = flowviz.quiver_arrows(f3, (148, 212), step=20, scale=5.0, style="topview", dominant=dom, vec_scale=(1.0, 1.0))
    for b in range(3):
        s = flowviz.quiver_arrows(f3[b:b + 1].clone(), (148, 212), step=20, scale=5.0, style="topview", dominant=dom[b:b + 1].clone(),
                                  vec_scale=(1.0, 1.0))
        assert all(torch.equal(x[b], y[0]) for x, y in zip(a, s))
    assert 0 < ((a.flags >> 1) & 1).sum().item() < a.flags.numel()
    z = flowviz.quiver_arrows(f3, (148, 212), step=20, dominant=torch.zeros(3, 2, device=dev))
    assert ((z.flags >> 1) & 1).all()                                 # zero dominant direction: every arrow aligned
    with pytest.raises(ValueError):
        flowviz.quiver_arrows(f3, (148, 212), step=0)
    with pytest.raises(ValueError):
        flowviz.quiver_arrows(f3, (148, 212), crop=(38, 53))
    with pytest.raises(ValueError):
        flowviz.quiver_arrows(f3, (148, 212), dominant=torch.zeros(3, 2))
    with pytest.raises(ValueError):
        ops.flow_quiver(f3, 148, 212, 16, (1.0, 1.0), 1.0, 0, 0.5, out=(torch.empty(1, device=dev),) * 3)
    with pytest.raises(TypeError):
        flowviz.flow_to_color(f3.half())


# ---- 5. reproducibility ---------------------------------------------------------------------------------------------------------
def test_every_output_has_the_same_bytes_on_a_second_call(gold, dev):
    from opticalflow_amd import flowviz, ops
    flow = torch.cat([_nchw(gold["field/smooth"], dev)] * 2, 0)
    flow[1] = flow[1].flip(-1) * 1.5

    def run():
        rec = ops.flow_stats(flow, clip_flow=4.0, threshold=0.7)
        col = flowviz.flow_to_color(flow, clip_flow=4.0, crop=(77, 130))
        a = flowviz.quiver_arrows(flow, (384, 640), step=16, dominant=rec[:, 2:4], min_mag=8.0)
        return [t.clone() for t in (rec, col) + tuple(a)]
    first, second = run(), run()
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x, y.view(torch.uint8) if y.dtype != torch.uint8 else y)


# ---- 6. the rendered stream -----------------------------------------------------------------------------------------------------
def _net(dev, precision):
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet(precision=precision)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    return net.to(dev).eval()


@pytest.mark.parametrize("precision,batch,use_graph", [("fp32", 1, True), ("fp32", 1, False), ("fp32", 2, True), ("fp32", 2, False),
                                                       ("fp16", 1, True)])
def test_rendered_stream_equals_the_eager_calls(dev, precision, batch, use_graph):
    from opticalflow_amd import flowviz, video
    net = _net(dev, precision)
    qkw = dict(frame_hw=(64, 128), step=20, scale=5.0, style="topview", vec_scale=(1.0, 1.0), min_mag=0.5)
    spec = video.RenderSpec(color=True, clip_flow=4.0, quiver=qkw, dominant=True, threshold=0.05, crop=(15, 31))
    plain = video.FlowStream(net, batch, 64, 128, use_graph=use_graph)
    stream = video.FlowStream(net, batch, 64, 128, use_graph=use_graph, render=spec)
    g = torch.Generator().manual_seed(3)
    first = torch.rand(1, 3, 64, 128, generator=g).to(dev)
    plain.prime(first)
    stream.prime(first)
    assert plain.rendered is None
    for _ in range(3):
        frames = torch.rand(batch, 3, 64, 128, generator=g).to(dev)
        flow = stream.push(frames).clone()
        assert torch.equal(flow, plain.push(frames))                  # rendering changes nothing about the flow
        r = stream.rendered
        assert torch.equal(r.color, flowviz.flow_to_color(flow, clip_flow=4.0, crop=(15, 31)))
        mean, count = flowviz.dominant_direction(flow, threshold=0.05, crop=(15, 31))
        assert torch.equal(r.stats[:, 2:4], mean) and torch.equal(r.stats.view(torch.int32)[:, 1].long(), count)
        eager = flowviz.quiver_arrows(flow, crop=(15, 31), dominant=mean, **qkw)
        assert all(torch.equal(x, y) for x, y in zip(r.arrows, eager))
        assert flow.abs().max().item() > 0


def test_flow_video_rendered_yields_flow_videos_flows(dev):
    from opticalflow_amd import flowviz, video
    net = _net(dev, "fp32")
    g = np.random.default_rng(5)
    frames = [g.integers(0, 256, (64, 128, 3), dtype=np.uint8) for _ in range(4)]
    flows = list(video.flow_video(net, frames, use_graph=True))
    outs = list(video.flow_video_rendered(net, frames, color=True, quiver=dict(step=16, min_mag=0.0), use_graph=True, with_flow=True))
    assert len(outs) == len(flows) == 3
    for f, o in zip(flows, outs):
        assert np.array_equal(o["flow"], f)
        fd = torch.from_numpy(np.ascontiguousarray(f.transpose(2, 0, 1))).unsqueeze(0).to(dev)
        assert np.array_equal(o["color"], flowviz.flow_to_color(fd)[0].cpu().numpy())
        a = flowviz.quiver_arrows(fd, (64, 128), step=16, min_mag=0.0)
        assert np.array_equal(o["vec"], a.vec[0].cpu().numpy()) and np.array_equal(o["tip"], a.tip[0].cpu().numpy())
        assert o["flags"].shape == (4, 8) and (o["flags"] & 1).all()
    lean = next(iter(video.flow_video_rendered(net, frames[:2], color=True, use_graph=False)))
    assert sorted(lean) == ["color"] and np.array_equal(lean["color"], outs[0]["color"])
