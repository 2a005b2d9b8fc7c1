"""Video streams fed raw uint8 frames (opticalflow_amd.video.RawFlowStream, flow_video / flow_video_rendered with ingest="hip",
flow_video_vanishing) and the strict half-precision stream plan (engine_strict.PwcVideoPlanStrict).

The raw streams must give the bits of the existing streams fed the host-ingested float frames: only the producer of the input tensor
differs, and tests/test_gpu_video_ingest.py holds that producer to the host helpers bit for bit.  The strict stream is held to the
project's bar for the mode (mean EPE < 1e-3 against the fp32 pairwise forward) and to the strict pairwise forward, and the strict
pairwise forward to a recording made before its level-2 tail moved into a method of its own."""
import numpy as np
import pytest
import torch

from conftest import load_golden, seeded_rand

pytestmark = pytest.mark.gpu

_NETS = {}


def _net(dev, precision="fp32"):
    """synthetic_state_dict(seed=3, gain=0.85, bias_std=0.02), as tests/test_video.py; one model per precision for the module."""
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    if precision not in _NETS:
        net = PWCDCNet(precision=precision).to(dev).eval()
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=3, gain=0.85, bias_std=0.02))
        _NETS[precision] = net
    return _NETS[precision]


def _frames(n, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, H, W, 3)).astype(np.uint8)


def _host_ingest(frames):
    from opticalflow_amd.kitti import pad_to_64
    from opticalflow_amd.video import frame_to_tensor
    return torch.cat([pad_to_64(frame_to_tensor(f).unsqueeze(0))[0] for f in frames], 0)


@pytest.mark.parametrize("batch,use_graph", [(1, False), (1, True), (2, False), (2, True)])
def test_raw_stream_equals_flow_stream_on_host_ingested_frames(gpu_device, batch, use_graph):
    """120x250 frames: Hp x Wp = 128x256, pads 8 and 6, crop 24x58.  NumPy, CPU-tensor and device-tensor frames all go in."""
    from opticalflow_amd.video import FlowStream, RawFlowStream
    dev, net = gpu_device, _net(gpu_device)
    H, W, n = 120, 250, 1 + 2 * batch
    frames = _frames(n, H, W, 11)
    host = _host_ingest(frames).to(dev)
    ref = FlowStream(net, batch, 128, 256, use_graph=use_graph)
    ref.prime(host[0])
    want = [ref.push(host[1 + k * batch:1 + (k + 1) * batch]).clone() for k in range(2)]
    raw = RawFlowStream(net, batch, H, W, use_graph=use_graph)
    assert (raw.height, raw.width, raw.pads, raw.crop) == (128, 256, (8, 6), (24, 58))
    with pytest.raises(RuntimeError):
        raw.push(frames[1:1 + batch])
    with pytest.raises(ValueError):
        raw.prime(frames[0, :, :-1])
    raw.prime(torch.from_numpy(frames[0]))                                        # a CPU tensor
    got = [raw.push(frames[1:1 + batch]).clone(),                                 # a NumPy array
           raw.push(torch.from_numpy(frames[1 + batch:1 + 2 * batch]).to(dev)).clone()]      # a device tensor
    for k in range(2):
        assert got[k].shape == want[k].shape == (batch, 2, 32, 64)
        assert want[k].abs().max().item() > 1e-2
        assert torch.equal(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())
    # the staging slots alternate: four more pushes from the host, each the continuation of the sequence
    more = _frames(4 * batch, H, W, 12)
    mh = _host_ingest(more).to(dev)
    for k in range(4):
        w = ref.push(mh[k * batch:(k + 1) * batch]).clone()
        assert torch.equal(raw.push(more[k * batch:(k + 1) * batch]), w), k


def test_flow_video_hip_ingest_equals_host_ingest(gpu_device):
    from opticalflow_amd.video import flow_video
    net = _net(gpu_device)
    frames = list(_frames(4, 100, 150, 5))
    host = list(flow_video(net, frames))
    hip = list(flow_video(net, frames, ingest="hip"))
    assert len(host) == len(hip) == 3
    for a, b in zip(host, hip):
        assert a.shape == b.shape == (4, 6, 2) and b.dtype == np.float32 and np.abs(a).max() > 1e-3
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_flow_video_rendered_hip_ingest_equals_host_ingest(gpu_device):
    from opticalflow_amd.video import flow_video_rendered
    net = _net(gpu_device)
    frames = list(_frames(4, 100, 150, 6))
    kw = dict(color=True, quiver=dict(step=8, min_mag=0.1), dominant=True, with_flow=True)
    host = list(flow_video_rendered(net, frames, **kw))
    hip = list(flow_video_rendered(net, frames, ingest="hip", **kw))
    assert len(host) == len(hip) == 3
    for a, b in zip(host, hip):
        assert sorted(a) == sorted(b) == ["color", "flags", "flow", "tip", "vec"]
        assert b["color"].shape == (4, 6, 3) and b["vec"].shape == (13, 19, 2)
        for key in a:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key


def test_flow_video_vanishing_equals_the_estimate_from_the_streams_flow(gpu_device):
    """Arrow grid and vanishing point of every pair against quiver_arrows / vanishing_point_from_flow applied to the flow the same
    stream hands out; the arrows also against flow_video_rendered's."""
    from opticalflow_amd import vanishing
    from opticalflow_amd.video import flow_video_rendered, flow_video_vanishing
    dev, net = gpu_device, _net(gpu_device)
    H, W = 120, 250
    frames = list(_frames(4, H, W, 7))
    kw = dict(step=8, min_mag=0.25)
    est = dict(max_points=200, min_pairs=10, seed=2)
    outs = list(flow_video_vanishing(net, frames, with_flow=True, **kw, **est))
    rend = list(flow_video_rendered(net, frames, color=False, quiver=dict(scale=1, **kw), ingest="hip"))
    assert len(outs) == len(rend) == 3
    found = 0
    for o, r in zip(outs, rend):
        assert o["flow"].shape == (24, 58, 2) and o["vec"].shape == (15, 32, 2)
        for key in ("vec", "tip", "flags"):
            assert np.array_equal(o[key].view(np.uint8), r[key].view(np.uint8)), key
        flow = torch.from_numpy(o["flow"]).permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)
        want = vanishing.to_host(vanishing.vanishing_point_from_flow(flow, (H, W), **kw, **est))[0]
        print("flow_video_vanishing:", o["vanishing"], "from the flow:", want)
        assert o["vanishing"] == want
        found += want is not None
    assert found > 0, "no pair gave a vanishing point: the test compares nothing but None"


@pytest.mark.parametrize("batch", [1, 2])
def test_strict_stream_meets_the_bar_of_the_mode(gpu_device, batch):
    """FlowStream(PWCDCNet(precision="fp16-strict")), graphed.  Mean EPE against the fp32 net's pairwise forward < 1e-3, the bar of the
    mode, and at most 1e-4 above the strict PAIRWISE forward's EPE: what tests/test_video.py allows the fp32 stream against the fp32
    pairwise forward, since the only new source of difference is the pyramid's batch size in the fp32 upper part.
    Measured on the MI355X, pairwise / stream: 5.5688e-4 / 5.5688e-4 at batch 1, 5.5647e-4 / 5.5644e-4 at batch 2."""
    from opticalflow_amd.video import FlowStream
    from oracle import pwc_oracle as O
    dev = gpu_device
    net32, strict = _net(dev), _net(dev, "fp16-strict")
    H, W, n = 128, 192, 1 + 2 * batch
    frames = seeded_rand((n, 3, H, W), 77, 0, 1).to(dev)
    x = torch.cat([frames[:-1], frames[1:]], 1)
    ref = net32(x).cpu()
    pair = strict(x).cpu()
    stream = FlowStream(strict, batch, H, W, use_graph=True)
    with pytest.raises(RuntimeError):
        stream.push(frames[1:1 + batch])
    stream.prime(frames[0])
    got = torch.cat([stream.push(frames[1 + k * batch:1 + (k + 1) * batch]).clone() for k in range(2)], 0).cpu()
    assert got.shape == ref.shape == (n - 1, 2, H // 4, W // 4) and ref.abs().max().item() > 1e-2
    e_pair, e_stream = O.epe(pair, ref), O.epe(got, ref)
    print("fp16-strict batch %d: mean EPE against the fp32 pairwise forward: strict pairwise %.4e, strict stream %.4e (mean|flow| %.3f)"
          % (batch, e_pair, e_stream, ref.abs().mean().item()))
    assert e_pair < 1e-3
    assert e_stream < 1e-3
    assert e_stream <= e_pair + 1e-4


def test_strict_forward_keeps_its_bits(gpu_device):
    """PWCDCNet(precision="fp16-strict").forward on one 128x192 pair against a recording made on the MI355X before the level-2 tail of
    PwcPlanStrict.run became _level2 (tests/golden/g21_strict_forward.npz: seeds and flow2)."""
    g = load_golden("g21_strict_forward.npz")
    strict = _net(gpu_device, "fp16-strict")
    assert (int(g["wseed"]), float(g["gain"]), float(g["bias_std"])) == (3, 0.85, 0.02)
    x = seeded_rand(g["xshape"], int(g["xseed"])).to(gpu_device)
    flow = strict(x).cpu().numpy()
    assert flow.shape == g["flow2"].shape == (1, 2, 32, 48) and np.abs(flow).max() > 1e-2
    assert np.array_equal(flow.view(np.int32), g["flow2"].view(np.int32))
