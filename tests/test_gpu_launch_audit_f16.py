"""Launch audit of the half-precision plans: every ops_f16.* launch of one eager forward of the fp16 plan (and of the video plan,
and of the fp16-strict plan, whose fp32 part is audited by launch_audit.LaunchAudit in the same run) against a float64 CPU
reference of that single operator, computed from the launch's own inputs, with a per-element bound (tests/launch_audit_f16.py);
pad lanes and stray stores on every launch; then the union of routes reached against a fixed list."""
import time

import pytest
import torch

import launch_audit_f16 as LA16
from conftest import seeded_rand
from launch_audit import MASK_EXCLUDED_MAX

pytestmark = pytest.mark.gpu

ALL_OPTIONS = ("conv_wino4", "w4_tailsplit", "w4_smallsplit", "w4_small_min_wgs", "corr_pipe", "corr_pipe_min_tiles", "corr_roll",
               "corr_small_tiles", "head10", "f16_level_corr", "warpcorr_window", "stream_slice_wgs", "c1_in_arena", "head_sliced_min_tiles")
ENV_SWITCHES = ("PWC_F16_FUSE_PYR1", "PWC_CONV16F_W8")

# (id, plan, variant, B, H, W, options, environment, net keywords, what it reaches)
CONFIGS = [
    ("f16-b16-448x1024", "fp16", "dc", 16, 448, 1024, None, None, None,
     "the benchmark shape: w8 kernels (MT 1/2/3), tall NT=4 tiles, two-per-CU, tiled correlation"),
    ("f16-b1-448x1024", "fp16", "dc", 1, 448, 1024, None, None, None, "fill rule (narrow tiles), direct correlation at small levels"),
    ("f16-b3-384x1280", "fp16", "dc", 3, 384, 1280, None, None, None, "KITTI's padded size, odd batch"),
    ("f16-b5-64x64", "fp16", "dc", 5, 64, 64, None, None, None, "tiny maps, level 6 at 1x1"),
    ("f16-old-b2-256x512", "fp16", "old", 2, 256, 512, None, None, None,
     "image_conv_s2 + layer-by-layer pyramid, mask threshold 0.999"),
    ("f16-opts-b2-256x512", "fp16", "dc", 2, 256, 512, {"f16_level_corr": 1}, {"PWC_F16_FUSE_PYR1": "0"},
     dict(normalize_corr=True, align_corners=True), "fused entry, layer-by-layer pyramid, normalized cost volume, align_corners"),
    ("f16-w8off-b8-256x512", "fp16", "dc", 8, 256, 512, None, {"PWC_CONV16F_W8": "0"}, None,
     "the 5-wave kernel where the plan would take w8"),
    ("f16-video-b4-256x512", "video", "dc", 4, 256, 512, None, None, None, "PwcVideoPlanF16 prime + push: overlapping pair views"),
    ("strict-b16-448x1024", "strict", "dc", 16, 448, 1024, None, None, None,
     "wide split filters on w8 and 5-wave kernels, hi/lo hand-over"),
    ("strict-b1-448x1024", "strict", "dc", 1, 448, 1024, None, None, None, "batch 1"),
    ("strict-b3-384x1280", "strict", "dc", 3, 384, 1280, None, None, None, "the KITTI default mode"),
    ("strict-old-b2-256x512", "strict", "old", 2, 256, 512, None, None, None, "PWCDCNet_old through the strict plan"),
    ("strict-fast-b2-256x512", "strict-fast", "dc", 2, 256, 512, None, None, None, "the plain-filter ladder (PWC_STRICT_PLAIN=fast)"),
]

ROUTES_SEEN = {}
_SD = {}


@pytest.fixture
def all_options(monkeypatch):
    """save every library option and the environment switches the half plans read, restore them afterwards"""
    from opticalflow_amd import _lib
    saved = {n: _lib.get_option(n) for n in ALL_OPTIONS}
    for e in ENV_SWITCHES:
        monkeypatch.delenv(e, raising=False)
    yield _lib.set_option
    for n, v in saved.items():
        _lib.set_option(n, v)


def _net(variant, precision, dev, kw=None):
    from opticalflow_amd import PWCDCNet, PWCDCNet_old
    from opticalflow_amd.weights import synthetic_state_dict
    net = (PWCDCNet if variant == "dc" else PWCDCNet_old)(precision=precision, **(kw or {}))
    if variant not in _SD:
        _SD[variant] = synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02)
    net.load_state_dict(_SD[variant])
    return net.to(dev).eval(), _SD[variant]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_launch_audit_f16(gpu_device, monkeypatch, all_options, cfg):
    cid, kind, variant, B, H, W, opts, env, kw, _why = cfg
    from opticalflow_amd import engine_strict
    from opticalflow_amd.engine_f16 import PwcVideoPlanF16
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.time()
    for k, v in (opts or {}).items():
        all_options(k, v)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if kind == "strict-fast":
        monkeypatch.setattr(engine_strict, "PLAIN_FILTERS", engine_strict.parse_plain_filters("fast"))
    precision = "fp16" if kind in ("fp16", "video") else "fp16-strict"
    net, sd = _net(variant, precision, gpu_device, kw)
    audit = LA16.LaunchAuditF16(sd, seed=B * 131 + H + W)
    with torch.no_grad():
        if kind == "video":
            frames = seeded_rand((B + 1, 3, H, W), 7100 + B + H + W).to(gpu_device)
            params = {k: v.detach() for k, v in net.state_dict(keep_vars=True).items()}
            plan = PwcVideoPlanF16(params, B, H, W, gpu_device, net.md, net.normalize_corr, net.align_corners, variant)
            audit.install(monkeypatch, plan)
            plan.prime(frames[:1])
            plan.push(frames[1:])
        else:
            x = seeded_rand((B, 6, H, W), 7000 + B + H + W).to(gpu_device)
            plan = net._plan_for(x)
            if kind == "strict-fast":
                assert not plan.split["conv2_3"] and plan.split["conv2_0"] and plan.split["head2"]
            audit.install(monkeypatch, plan)
            plan.run(x)
        torch.cuda.synchronize()
    monkeypatch.undo()
    t_audit = time.time() - t0
    ROUTES_SEEN[cid] = audit.routes
    worst = audit.worst_by_family()
    recs = audit.all_records()
    print("\n[%s] %d launches (%d half-precision), %.1f s; worst error/bound per family: %s" % (
        cid, len(recs), len(audit.records), t_audit, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    print("[%s] routes: %s" % (cid, " ".join(sorted(audit.routes))))
    for r in recs:
        if r["pixels"]:
            assert r["excluded"] <= MASK_EXCLUDED_MAX * r["pixels"], r
    print("[%s] pixels near the mask threshold left out: %d; up_flow double-rounding ties: %d" % (
        cid, sum(r["excluded"] for r in recs), sum(r.get("double_rounding", 0) for r in audit.records)))
    bad = audit.failures()
    assert not bad, bad[:5]
    assert len(audit.records) > (10 if kind.startswith("strict") else 40)
    ops = {r["op"] for r in audit.records}
    assert "conv3x3_f16" in ops and ("to_c8_hilo" in ops if kind.startswith("strict") else "correlation_c8" in ops)


def test_route_coverage_f16():
    """every route named in launch_audit_f16.ROUTES_REQUIRED_F16 was reached by the configurations above (run in the same session)"""
    missing_cfg = [c[0] for c in CONFIGS if c[0] not in ROUTES_SEEN]
    if missing_cfg:
        pytest.skip("needs the launch-audit configurations of this module in the same run (missing %s)" % missing_cfg)
    union = set().union(*ROUTES_SEEN.values())
    print("\nroute union: %s" % " ".join(sorted(union)))
    assert set(LA16.ROUTES_REQUIRED_F16) <= union, sorted(set(LA16.ROUTES_REQUIRED_F16) - union)


def test_comparator_reports_a_perturbed_bias_channel_f16(gpu_device):
    """a real conv3x3_f16 launch with one bias a few half ulps off, checked against the TRUE bias: the comparator names that
    channel only, and the unperturbed launch passes"""
    from opticalflow_amd import ops_f16
    g = torch.Generator().manual_seed(12)
    B, cin, cout, H, W = 2, 48, 40, 24, 72
    x = torch.randn(B, cin, H, W, generator=g).half().float()
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    c = 21
    b[c] = 3.0                                    # half ulp 2^-9 here; the channel's outputs sit near 3
    bp = b.clone()
    bp[c] = b[c] + 3 * 2.0 ** -9
    xd = ops_f16.to_c8(x.to(gpu_device))
    wp = ops_f16.pack_conv3x3_f16(w.to(gpu_device))
    ref, s = LA16.LA.conv_ref(x, LA16.sat_half(w).double(), b, act=False)

    def run(bias):
        y = ops_f16.conv3x3_f16(xd, wp, bias.to(gpu_device), cin, cout, leaky_slope=None)
        return LA16.c8_to_nchw(y.cpu())[:, :cout]
    r, _, chans = LA16.worst(LA16.half_ratio(run(bp), ref, s))
    assert chans == [c], (r, chans)
    assert LA16.worst(LA16.half_ratio(run(b), ref, s))[0] <= 1.0
