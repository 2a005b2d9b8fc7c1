"""Launch audit of the fp32 inference plan: every ops.* launch of one eager forward against a float64 CPU reference of that single
operator, computed from the launch's own recorded inputs, with a per-element bound (tests/launch_audit.py), at the geometries and
options that send layers to different kernel routes; then flow2 (and the training-mode tuple up to 256x512) end to end against the
float64 oracle with a MAX per-pixel endpoint-error bound; then the union of routes reached against a fixed list, and the union of
kernel instantiations launched against launch_audit.KERNELS_REQUIRED.  Each configuration's plan must also hold exactly the routing
signatures the device-less census recorded for it (tests/plan_census.py, tests/golden/plan_census_configs.json):
tests/test_plan_census_cpu.py proves on the CPU that those signatures cover every small geometry of its grid.

The fp16 / fp16-strict plans have their own per-launch audit (tests/test_gpu_launch_audit_f16.py, tests/launch_audit_f16.py: half
operands, fp32 accumulation, one rounding to half at the store); multi-GPU runs are outside both."""
import time

import pytest
import torch

import launch_audit as LA
import plan_census as PC
from conftest import seeded_rand
from oracle import pwc_oracle as O

pytestmark = pytest.mark.gpu

# per-pixel endpoint error of flow2 (and flows 3-6) against the float64 oracle.  Observed on MI355X over every configuration
# below: max <= 1.95e-5 (b16 / b32 at 448x1024), mean <= 3.5e-6; bounds ~10x that.
E2E_MAX_EPE = 2e-4
E2E_MEAN_EPE = 4e-5

ALL_OPTIONS = ("conv_wino4", "w4_tailsplit", "w4_smallsplit", "w4_small_min_wgs", "corr_pipe", "corr_pipe_min_tiles", "corr_roll",
               "corr_small_tiles", "head10", "f16_level_corr", "warpcorr_window", "stream_slice_wgs", "c1_in_arena", "head_sliced_min_tiles")
NON_DEFAULT = {"head10": 0, "warpcorr_window": 0, "w4_tailsplit": 0, "w4_smallsplit": 0, "c1_in_arena": 0, "corr_pipe": 1,
               "corr_pipe_min_tiles": 1, "stream_slice_wgs": 32}

# (id, variant, B, H, W, options, what it covers)
CONFIGS = [
    ("b1-448x1024", "dc", 1, 448, 1024, None, "README batch 1: F(4x4) small-launch Cin splits, sliced heads, lattice context"),
    ("b2-448x1024", "dc", 2, 448, 1024, None, "README batch 2: sliced head at level 3, whole-launch Cin splits"),
    ("b4-448x1024", "dc", 4, 448, 1024, None, "README batch 4"),
    ("b8-448x1024", "dc", 8, 448, 1024, None, "README batch 8"),
    ("b16-448x1024", "dc", 16, 448, 1024, None, "the benchmark workload: one-pass heads, F(4x4) tail splits, 96 = 64 + 32"),
    ("b32-448x1024", "dc", 32, 448, 1024, None, "README batch 32: the largest launches"),
    ("b3-384x1280", "dc", 3, 384, 1280, None, "KITTI's padded size in fp32, odd batch"),
    ("b4-320x896", "dc", 4, 320, 896, None, "train.py's shape through the inference plan"),
    ("b2-448x960", "dc", 2, 448, 960, None, "W/4 = 240: no lattice context (dilated F(2x2) / direct context), level 5 W % 4 != 0"),
    ("b1-1024x448", "dc", 1, 1024, 448, None, "portrait, H > W"),
    ("b5-64x64", "dc", 5, 64, 64, None, "small maps: head10, small-map correlation, folded tiles, level 6 at 1x1"),
    ("b3-128x192", "dc", 3, 128, 192, None, "small maps, W not a power of two"),
    ("old-b2-256x512", "old", 2, 256, 512, None, "PWCDCNet_old: permuted filters through the same kernels"),
    ("opts-b2-256x512", "dc", 2, 256, 512, NON_DEFAULT, "non-default options: conv+deconv heads, round-2 fused kernel, unsplit F(4x4)"),
    # small geometries chosen by greedy cover over the plan census (tests/test_plan_census_cpu.py)
    ("b8-192x320", "dc", 8, 192, 320, None, "W/4 = 80: conv2_0..2 and dc_conv1 on unsplit F(2x2), conv2_3 on split-K F(2x2), conv2_4 and "
                                            "conv3_0..2 on the direct kernel; level maps 80 .. 5 columns wide"),
    ("b8-384x64", "dc", 8, 384, 64, None, "portrait strip, W/4 = 16: conv2_2 and dc_conv1 (Cin 565) on the direct kernel"),
    ("b6-192x192", "dc", 6, 192, 192, None, "W/4 = 48: conv2_3 on the direct kernel"),
    ("b8-320x192", "dc", 8, 320, 192, None, "portrait: conv2_3 on unsplit F(2x2)"),
    # kernel instantiations no configuration above launches (tools/kernel_census.py, launch_audit.KERNELS_REQUIRED)
    ("b7-128x384", "dc", 7, 128, 384, None, "F(4x4) whole-launch Cin splits in 3, 6 and 8 slices on 32-column tile groups"),
    ("b5-128x256", "dc", 5, 128, 256, None, "F(4x4) in 5 slices on 64-column groups; the stacked 8x16 form in 4 slices"),
    ("b7-128x256", "dc", 7, 128, 256, None, "the direct kernel's 96-cout tile <3, 1> at two workgroups per CU"),
]

ROUTES_SEEN = {}
KERNELS_SEEN = {}


@pytest.fixture
def all_options():
    """save every library option and restore it afterwards (the plan reads several of them when it is built)"""
    from opticalflow_amd import _lib
    saved = {n: _lib.get_option(n) for n in ALL_OPTIONS}
    yield _lib.set_option
    for n, v in saved.items():
        _lib.set_option(n, v)


_SD = {}


def _net(variant, dev):
    from opticalflow_amd import PWCDCNet, PWCDCNet_old
    from opticalflow_amd.weights import synthetic_state_dict
    net = (PWCDCNet if variant == "dc" else PWCDCNet_old)()
    if variant not in _SD:
        _SD[variant] = synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02)
    net.load_state_dict(_SD[variant])
    return net.to(dev).eval(), _SD[variant]


def _epe_max(a, b):
    return (a.double() - b.double()).pow(2).sum(1).sqrt().max().item()


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_launch_audit(gpu_device, monkeypatch, all_options, cfg):
    cid, variant, B, H, W, opts, _why = cfg
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.time()
    x = seeded_rand((B, 6, H, W), 7000 + B + H + W)
    xd = x.to(gpu_device)
    default_flow = None
    if opts:
        net, _ = _net(variant, gpu_device)
        default_flow = net(xd).cpu()
        for k, v in opts.items():
            all_options(k, v)
    net, sd = _net(variant, gpu_device)
    plan = net._plan_for(xd)
    audit = LA.LaunchAudit(seed=B * 131 + H + W)
    audit.install(monkeypatch, plan)
    with torch.no_grad():
        flow = plan.run(xd).cpu()
        flows = [f.cpu() for f in plan.flows()]
    monkeypatch.undo()
    t_audit = time.time() - t0
    ROUTES_SEEN[cid] = audit.routes
    KERNELS_SEEN[cid] = audit.kernels
    worst = audit.worst_by_family()
    print("\n[%s] %d launches, %.1f s; worst error/bound per family: %s" % (
        cid, len(audit.records), t_audit, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    print("[%s] routes: %s" % (cid, " ".join(sorted(audit.routes))))
    print("[%s] kernels: %s" % (cid, " | ".join(sorted(audit.kernels))))
    # the census (built without a device, 256 compute units assumed) must describe THIS plan, or its coverage proof is about another one
    census = PC.load_config_census()[cid]
    got_sigs, got_shape = PC.plan_signatures(plan), PC.plan_shape(plan)
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    assert got_sigs == census[0] and got_shape == census[1], (
        "the plan built on this device (%d compute units) differs from the census for %s (256 assumed): only on the device %s, only "
        "in the census %s, shape %s vs %s" % (cus, cid, sorted(got_sigs - census[0]), sorted(census[0] - got_sigs), got_shape, census[1]))
    for r in audit.records:
        if r["pixels"]:
            assert r["excluded"] <= LA.MASK_EXCLUDED_MAX * r["pixels"], r
    ex = sum(r["excluded"] for r in audit.records)
    print("[%s] pixels near the mask threshold left out: %d" % (cid, ex))
    bad = audit.failures()
    assert not bad, bad[:5]
    assert len(audit.records) > 40

    # end to end against the float64 oracle, max and mean per-pixel endpoint error
    fwd = O.pwc_forward if variant == "dc" else O.pwc_forward_old
    sd64 = {k: v.double() for k, v in sd.items()}
    items = sorted({0, B - 1})
    train_tuple = H * W <= 256 * 512
    for i in items:
        with torch.no_grad():
            ref = fwd(sd64, x[i:i + 1].double(), all_levels=train_tuple)
        refs = ref if train_tuple else (ref,)
        got = flows if train_tuple else [flow]
        for lvl, (g, r) in enumerate(zip(got, refs)):
            emax, emean = _epe_max(g[i:i + 1], r), O.epe(g[i:i + 1].double(), r)
            print("[%s] item %d flow%d: max EPE %.3e, mean %.3e vs fp64 oracle" % (cid, i, lvl + 2, emax, emean))
            assert emax < E2E_MAX_EPE and emean < E2E_MEAN_EPE, (cid, i, lvl + 2, emax, emean)
    if default_flow is not None:
        emax = _epe_max(flow, default_flow)
        print("[%s] vs the default-option flow: max EPE %.3e" % (cid, emax))
        assert emax < E2E_MAX_EPE
    print("[%s] total %.1f s" % (cid, time.time() - t0))


def test_route_coverage():
    """every route named in launch_audit.ROUTES_REQUIRED was reached by the configurations above (run in the same session)"""
    missing_cfg = [c[0] for c in CONFIGS if c[0] not in ROUTES_SEEN]
    if missing_cfg:
        pytest.skip("needs the launch-audit configurations of this module in the same run (missing %s)" % missing_cfg)
    union = set().union(*ROUTES_SEEN.values())
    print("\nroute union: %s" % " ".join(sorted(union)))
    assert set(LA.ROUTES_REQUIRED) <= union, sorted(set(LA.ROUTES_REQUIRED) - union)


def test_kernel_coverage():
    """every kernel instantiation named in launch_audit.KERNELS_REQUIRED -- what the plan launches anywhere on the census grid and at
    the benchmark sizes (tools/kernel_census.py) -- was launched, and so checked per element, by the configurations above"""
    missing_cfg = [c[0] for c in CONFIGS if c[0] not in KERNELS_SEEN]
    if missing_cfg:
        pytest.skip("needs the launch-audit configurations of this module in the same run (missing %s)" % missing_cfg)
    union = set().union(*KERNELS_SEEN.values())
    print("\nkernel union (%d): %s" % (len(union), " | ".join(sorted(union))))
    assert set(LA.KERNELS_REQUIRED) <= union, sorted(set(LA.KERNELS_REQUIRED) - union)


def test_comparator_reports_a_perturbed_bias_channel(gpu_device):
    """a real kernel run with one bias 1e-5 relative off, checked against the TRUE bias: the comparator names that channel only"""
    from opticalflow_amd import ops
    g = torch.Generator().manual_seed(11)
    B, cin, cout, H, W = 2, 16, 32, 24, 64
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    _, s = LA.conv_ref(x, w, torch.zeros(cout), act=False)
    c = 13
    b[c] = 2.0 * s[:, c].mean().item()                    # a bias of the size of its channel's sum of |terms|
    bp = b.clone()
    bp[c] = b[c] * (1 + 1e-5)
    wd = w.to(gpu_device)
    got = ops.conv3x3(x.to(gpu_device), ops.pack_conv3x3(wd), bp.to(gpu_device), cout, leaky_slope=None).cpu()
    ref, s = LA.conv_ref(x, w, b, act=False)
    r, _, chans = LA.worst(LA.bounded_ratio(got, ref, s, LA.REL_DIRECT))
    assert chans == [c], (r, chans)
    ok = ops.conv3x3(x.to(gpu_device), ops.pack_conv3x3(wd), b.to(gpu_device), cout, leaky_slope=None).cpu()
    assert LA.worst(LA.bounded_ratio(ok, ref, s, LA.REL_DIRECT))[0] <= 1.0


def test_small_stream_slice_target_keeps_a_working_head_route(gpu_device, all_options):
    """ADVICE r4 (engine.py:150): with a small "stream_slice_wgs" the library does not cut a 14..63-tile level along Cin, and
    pwc_head_upfeat_ws_fwd refuses it.  4 x 256 x 512, level 3 (32 x 64, 16 tiles of 8 x 128): the plan used to pick the streaming
    head there from the tile count alone and the forward raised PWC_EUNSUPPORTED.  The plan now asks the library's slice plan."""
    from opticalflow_amd import engine, ops
    x = seeded_rand((4, 6, 256, 512), 77).to(gpu_device)
    cin = engine.level_in_channels(3) + engine.DENSE_TOTAL
    net, _ = _net("dc", gpu_device)
    ref = net(x).cpu()
    assert net._plan_for(x).stream_head[3] and ops.head_upfeat_workspace_bytes(4, cin, 32, 64) > 0     # default: sliced head
    all_options("stream_slice_wgs", 32)
    assert ops.head_upfeat_workspace_bytes(4, cin, 32, 64) == 0
    net, _ = _net("dc", gpu_device)
    plan = net._plan_for(x)
    assert not plan.stream_head[3]
    got = net(x).cpu()
    assert _epe_max(got, ref) < E2E_MAX_EPE
