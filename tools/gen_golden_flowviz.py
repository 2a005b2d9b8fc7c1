"""Generate tests/golden/g13_flowviz.npz from the REFERENCE's own picture-making functions.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.  Recipe as
tools/gen_golden_kitti_score.py: process-local stub modules, no reference file is edited or copied.  ``cv2`` is a stub whose
``resize`` is harness.cv2_resize_linear (cv2 is not installed; that restatement is what the product's arrow kernel is defined by),
whose ``arrowedLine`` RECORDS (pt1, pt2, color) -- this is how the reference's own arrow list gets into the fixture -- and whose
``rectangle`` / ``putText`` do nothing; ``matplotlib``, ``ptflops``, ``tqdm``, ``correlation_cuda`` become stubs when they are not
installed.  Run: ``flow_to_color`` (pwc_extract_flow.py), ``create_quiver_frame`` (pwc_extract_flow_video.py),
``calculate_dominant_direction`` and ``draw_flow_arrows`` (topview.py; when the module cannot be imported even with stubs, the two
functions are compiled from its file with ``ast`` in this process -- their text goes nowhere).

The cases and the knife-edge definitions are in tests/flowviz_oracle.py.  The generator ASSERTS what the tests rely on, all of it
properties of the inputs, the float64 oracle and the reference alone (when a seed violates one, change the seed):
  colour    an all-fp32 numpy emulation of the chain is within COLOR_DELTA / 3 levels of the float64 oracle before truncation;
            knife-edge channels <= 5e-3 of a case's channels; the reference differs from the truncated oracle by <= 1 level and only on
            knife-edge channels
  dominant  no pixel within FLAG_DELTA of the threshold; the reference's count equals the oracle's
  arrows    knife-edge tip coordinates, keep flags and aligned flags each <= 1e-2 of a case's; the reference's arrows differ from the
            oracle's only there (tips by <= 1)

    python tools/gen_golden_flowviz.py [out.npz]
"""
import ast
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_proxy_loss import REF, REPO, _stub  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from opticalflow_amd import harness  # noqa: E402
import flowviz_oracle as FO  # noqa: E402

ARROWS = []


def _resize(src, dsize, dst=None, fx=0, fy=0, interpolation=1):
    W, H = dsize
    return harness.cv2_resize_linear(torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)), H, W).numpy()


def _functions_from_file(path, names):
    """The named top-level functions of a Python file, compiled in this process with numpy and the stub cv2 in scope."""
    tree = ast.parse(open(path).read())
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    scope = {"np": np, "cv2": sys.modules["cv2"]}
    exec(compile(tree, path, "exec"), scope)
    return type("topview", (), {n: staticmethod(scope[n]) for n in names})


def _import_reference():
    _stub("correlation_cuda")
    _stub("cv2", INTER_LINEAR=1, FONT_HERSHEY_SIMPLEX=0, LINE_AA=16, resize=_resize,
          arrowedLine=lambda img, p1, p2, color, *a, **k: ARROWS.append((tuple(p1), tuple(p2), tuple(color))),
          rectangle=lambda *a, **k: None, putText=lambda *a, **k: None)
    for opt in ("tqdm", "ptflops", "matplotlib", "PIL"):
        try:
            __import__(opt)
        except ImportError:
            m = _stub(opt, tqdm=lambda x, **k: x, get_model_complexity_info=None)
            if opt == "matplotlib":
                m.pyplot = _stub("matplotlib.pyplot")
            if opt == "PIL":
                m.Image = _stub("PIL.Image")
    for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[m]                 # the reference's scripts import their own `models` package
    sys.path.insert(0, REF)
    try:
        import pwc_extract_flow as pe          # noqa: E402  (the reference's scripts)
        import pwc_extract_flow_video as pv    # noqa: E402
        try:
            import topview as tv               # noqa: E402
        except Exception:
            tv = _functions_from_file(os.path.join(REF, "topview.py"), ("calculate_dominant_direction", "draw_flow_arrows"))
    finally:
        sys.path.remove(REF)
    return pe, pv, tv


def make_fields():
    out = {}
    for i, (name, (h, w)) in enumerate(FO.FIELDS.items()):
        g = np.random.default_rng(1311 + i)
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        wave = np.stack([np.sin(5 * xx + 3 * yy + g.uniform(0, 6)), np.cos(4 * xx - 6 * yy + g.uniform(0, 6))], axis=-1)
        noise = g.standard_normal((h, w, 2))
        if name == "smooth":
            f = 4.0 * wave + 0.5 * noise           # radii up to ~6: clip_flow = 4 bites
        elif name == "noise":
            f = 2.5 * noise
        elif name == "radial":
            f = 0.1 * np.stack([xx * (w - 1) - (w - 1) / 2.0, yy * (h - 1) - (h - 1) / 2.0], axis=-1)
        elif name == "tiny":
            f = 1e-3 * (wave + 0.3 * noise)
        elif name == "huge":
            f = 300.0 * (wave + 0.3 * noise)
        elif name == "odd":
            f = 3.0 * wave + 0.4 * noise
        elif name == "one":
            f = np.array([[[0.7, -1.3]]])
        elif name == "zero":
            f = np.zeros((h, w, 2))
        elif name == "axis":                     # u > 0 and v exactly +0.0 (row 0) and -0.0 (row 1): the two sides of the wheel's wrap
            f = np.zeros((h, w, 2))
            f[..., 0] = 1.0                      # at u = 3 the blue channel of the -0.0 side is 43.0007: knife-edge by the input's choice
            f[1, :, 1] = -0.0
        out[name] = np.ascontiguousarray(f, dtype=np.float32)
    assert not np.signbit(out["axis"][0, :, 1]).any() and np.signbit(out["axis"][1, :, 1]).all()
    return out


def color_fp32(flow, clip_flow):
    """The colour chain with every operation in float32 -> the values before truncation (what an fp32 kernel can be expected to do)."""
    f32 = np.float32
    u, v = flow[..., 0], flow[..., 1]
    if clip_flow is not None:
        rad = np.sqrt(u * u + v * v)
        k = f32(clip_flow) / np.maximum(np.maximum(rad, f32(1e-5)), f32(clip_flow))
        u, v = u * k, v * k
    rad = np.sqrt(u * u + v * v)
    ang = np.arctan2(-v, -u) / f32(np.pi)
    fk = (ang + f32(1)) / f32(2) * f32(54) + f32(1)
    k0 = np.floor(fk)
    f = (fk - k0)[..., None]
    k0 = (k0.astype(np.int64) - 1) % 55
    wheel = FO.colorwheel().astype(f32) / f32(255)
    col = (f32(1) - f) * wheel[k0] + f * wheel[(k0 + 1) % 55]
    rn = np.clip(rad / (rad.max() + f32(1e-5)), f32(0), f32(1))[..., None]
    col = f32(1) - rn * (f32(1) - col)
    pre = np.clip(col, f32(0), f32(1)) * f32(255)
    assert pre.dtype == f32
    return pre


def arrows_to_grid(arrows, H, W, step):
    gy, gx = (H + step - 1) // step, (W + step - 1) // step
    keep, tip, aligned = np.zeros((gy, gx), bool), np.zeros((gy, gx, 2), np.int32), np.zeros((gy, gx), bool)
    for (x, y), (x2, y2), color in arrows:
        assert x % step == 0 and y % step == 0 and not keep[y // step, x // step]
        keep[y // step, x // step] = True
        tip[y // step, x // step] = (x2, y2)
        aligned[y // step, x // step] = tuple(color) == (0, 0, 255)
    return keep, tip, aligned


def main(out_path):
    pe, pv, tv = _import_reference()
    fields = make_fields()
    arrays = {"field/" + k: v for k, v in fields.items()}
    for case, (fname, crop) in FO.COLOR_CASES.items():
        flow = FO.cropped(fields[fname], crop)
        for ci, clip in enumerate(FO.CLIPS):
            ref = pe.flow_to_color(flow, clip_flow=clip)
            assert ref.dtype == np.uint8 and ref.shape == flow.shape[:2] + (3,)
            rgb, pre, knife = FO.color(flow, clip)
            emu = float(np.abs(color_fp32(flow, clip).astype(np.float64) - pre).max())
            d = ref.astype(np.int64) - rgb.astype(np.int64)
            frac = knife.mean()
            print("color %-7s clip %-4s fp32 emulation error %.2e levels, knife-edge %d of %d (%.2e), reference != oracle on %d"
                  % (case, clip, emu, knife.sum(), knife.size, frac, np.count_nonzero(d)))
            assert emu <= FO.COLOR_DELTA / 3, (case, clip, emu)
            assert frac <= 5e-3, (case, clip, frac)
            assert np.abs(d).max() <= 1 and not (d != 0)[~knife].any(), (case, clip)
            arrays["color/%s/%d" % (case, ci)] = ref
    assert (arrays["color/zero/0"] == 255).all()
    assert tuple(arrays["color/axis/0"][0, 0]) == (255, 0, 0) and tuple(arrays["color/axis/0"][1, 0]) == (255, 0, 43)
    for case, (fname, crop, thr) in FO.DOMINANT_CASES.items():
        flow = FO.cropped(fields[fname], crop)
        ref = np.asarray(tv.calculate_dominant_direction(flow, threshold=thr), dtype=np.float32)
        _, n, mean, knife = FO.stats(flow, thr)
        mag = np.sqrt((flow.astype(np.float64) ** 2).sum(-1))
        assert knife == 0, (case, knife)
        sel = flow[mag > thr]
        bound = 1e-5 * float(np.abs(sel).mean()) if n else 0.0
        assert np.abs(ref - mean).max() <= bound, (case, ref, mean)
        print("dominant %-7s count %d mean %s (reference float32 %s)" % (case, n, mean, ref))
        arrays["dom/" + case] = ref
        arrays["domn/" + case] = np.int64(n)
    assert arrays["domn/tiny"] == 0 and (arrays["dom/tiny"] == 0).all()
    for case, (fname, crop, (H, W), step, style, scale, min_mag, dom, thr, vs) in FO.QUIVER_CASES.items():
        flow = FO.cropped(fields[fname], crop)
        frame = np.zeros((H, W, 3), np.uint8)
        d = arrays["dom/" + dom] if dom else None
        del ARROWS[:]
        if style == "video":
            assert vs is None
            pv.create_quiver_frame(frame, flow, step=step, scale=scale, min_mag=min_mag, title="t")
        else:
            assert min_mag == 0.5 and vs == (1.0, 1.0)
            full = flow if flow.shape[:2] == (H, W) else _resize(flow, (W, H))
            tv.draw_flow_arrows(frame, full, step=step, scale=scale, dominant_dir=d, angle_threshold=thr)
        keep, tip, aligned = arrows_to_grid(ARROWS, H, W, step)
        gain, rule = FO.gain_rule(style, scale)
        o = FO.quiver(flow, (H, W), step, gain, rule, min_mag, vec_scale=vs, dominant=d, angle_threshold=thr)
        n = keep.size
        print("arrows %-10s grid %s kept %d of %d, knife-edge tips %d keep %d aligned %d"
              % (case, keep.shape, keep.sum(), n, o["knife_tip"].sum(), o["knife_keep"].sum(), o["knife_aligned"].sum()))
        assert o["knife_tip"].sum() <= 1e-2 * 2 * n and o["knife_keep"].sum() <= 1e-2 * n and o["knife_aligned"].sum() <= 1e-2 * n, case
        assert not (keep != o["keep"])[~o["knife_keep"]].any(), case
        both = keep & o["keep"]
        dt = np.abs(tip.astype(np.int64) - o["tip"])
        assert dt[both].max(initial=0) <= 1 and not (dt != 0)[both[..., None] & ~o["knife_tip"]].any(), case
        assert not (aligned != o["aligned"])[both & ~o["knife_aligned"]].any(), case
        if case not in ("low",):
            assert 0 < keep.sum(), case
        arrays["q/%s/keep" % case], arrays["q/%s/tip" % case], arrays["q/%s/aligned" % case] = keep, tip, aligned
    mix = [c for c in FO.QUIVER_CASES if 0 < arrays["q/%s/keep" % c].sum() < arrays["q/%s/keep" % c].size]
    assert len(mix) >= 3, mix                                   # kept and dropped arrows both occur
    assert any(0 < (arrays["q/%s/aligned" % c] & arrays["q/%s/keep" % c]).sum() < arrays["q/%s/keep" % c].sum()
               for c in FO.QUIVER_CASES if FO.QUIVER_CASES[c][4] == "topview")
    np.savez_compressed(out_path, **arrays)
    size = os.path.getsize(out_path)
    print("wrote %s (%d bytes)" % (out_path, size))
    assert size <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g13_flowviz.npz"))
