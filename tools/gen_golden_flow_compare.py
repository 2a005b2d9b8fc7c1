"""Generate tests/golden/g18_flow_compare.npz from the REFERENCE's own compare_flows / print_flow_stats (onnx_pth_compare.py).

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.
Recipe as tools/gen_golden_kitti_score.py: process-local module stubs, no reference file is edited -- ``cv2``, ``onnxruntime``,
``matplotlib`` / ``matplotlib.pyplot`` and ``correlation_cuda`` become stub modules.  Per case (tests/flow_compare_oracle.py CASES,
inputs from seeds) the reference's own ``compare_flows`` runs on every sample as an (H, W, 2) array and on the samples stacked along
H, with its stdout captured; ``print_flow_stats`` runs on both fields of every row; the lines the script draws beside its report
image (its ``lines = [...]`` block, executed from the reference's file with the row's values) are recorded too.  Stored: the seeds'
digests, the reference's returned values (float32 where it returns float32), its lines, the min / max / mean / std that
print_flow_stats formats, and the largest relative deviation of each metric from the float64 oracle.  The fields are not stored.

The generator ASSERTS what the tests rely on -- properties of the inputs and of the float64 oracle alone; on a violation, change
the seed:
  (a) in every ordinary case no pixel's float64 EPE lies within 1e-6 px of a threshold;
  (b) every ordinary case has at least two thresholds with agreement strictly between 5 % and 95 %;
  (c) Pearson's condition number kappa <= 100 in every non-degenerate row;
  (d) the reference's float32 values lie within N * 2^-24 relative of the oracle (the worst case of a float32 sum of N terms).

    python tools/gen_golden_flow_compare.py [out.npz]
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_proxy_loss import REF, REPO, _stub  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
import flow_compare_oracle as FO  # noqa: E402

F32_KEYS = ("L2 diff", "MAE", "Max abs diff", "Relative L2 diff", "Relative MAE", "Cosine similarity", "EPE mean", "EPE max")
SUM_KEYS = ("L2 diff", "MAE", "Relative L2 diff", "Relative MAE", "Pearson corr", "Cosine similarity", "EPE mean", "mean", "std")


def _import_reference():
    _stub("cv2")
    _stub("onnxruntime")
    mpl = _stub("matplotlib")
    mpl.pyplot = _stub("matplotlib.pyplot")
    _stub("correlation_cuda")
    for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[m]                 # the reference's script imports its own `models` package
    sys.path.insert(0, REF)
    import onnx_pth_compare as ref     # noqa: E402  (the reference's script)
    sys.path.remove(REF)
    return ref


def _drawn_block():
    """The reference's `lines = [ ... ]` statement (the text it draws beside the report image), as code compiled from its own file."""
    src = open(os.path.join(REF, "onnx_pth_compare.py"), encoding="utf-8").read().splitlines()
    first = next(i for i, s in enumerate(src) if s.strip() == "lines = [")
    last = next(i for i in range(first, len(src)) if src[i].strip() == "]")
    return compile("\n".join(s.strip() for s in src[first:last + 1]), "onnx_pth_compare.py lines", "exec")


def _captured(fn, *args):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = fn(*args)
    return out, buf.getvalue().splitlines()


def _rel(got, want):
    got, want = float(got), float(want)
    if np.isnan(want) or np.isnan(got):
        assert np.isnan(want) and np.isnan(got), (got, want)
        return 0.0
    return abs(got - want) / abs(want) if want != 0.0 else abs(got)


def main(out_path):
    ref = _import_reference()
    drawn = _drawn_block()
    arrays, worst, text = {}, {k: 0.0 for k in SUM_KEYS}, {}
    for name, c in FO.CASES.items():
        a, b = FO.make_inputs(name)
        n = a.shape[0]
        taus = FO.case_taus(name)
        want_rows = FO.rows(a, b, FO.REF_TAUS)                    # the reference has its four thresholds only
        own_rows = FO.rows(a, b, taus)
        f32, pear, agree, stats, lines = [], [], [], [], []
        for r in range(n + 1):
            sl = slice(r, r + 1) if r < n else slice(0, n)
            fa = np.ascontiguousarray(np.concatenate([x.transpose(1, 2, 0) for x in a[sl]], axis=0))     # (k*H, W, 2)
            fb = np.ascontiguousarray(np.concatenate([x.transpose(1, 2, 0) for x in b[sl]], axis=0))
            m, printed = _captured(ref.compare_flows, fa, fb)
            want = want_rows[r]
            N = want["_"]["N"]
            assert all(isinstance(m[k], np.float32) for k in F32_KEYS) and isinstance(m["Pearson corr"], np.float64)
            assert list(m["agreements"]) == list(want["agreements"])
            # exact: the maxima and every agreement percentage
            assert m["Max abs diff"] == want["Max abs diff"] and m["EPE max"] == want["EPE max"], (name, r)
            assert all(m["agreements"][k] == want["agreements"][k] for k in m["agreements"]), (name, r)
            for k in F32_KEYS + ("Pearson corr",):
                dev = _rel(m[k], want[k])
                assert dev <= N * 2.0 ** -24, (name, r, k, m[k], want[k])                                   # (d)
                if k in worst:
                    worst[k] = max(worst[k], dev)
            kappa = want["_"]["kappa"]
            assert np.isnan(kappa) or kappa <= 100.0, (name, r, kappa)                                      # (c)
            st_lines, st_vals = [], []
            for tag, fld, f in (("pth", fa, "a"), ("onnx", fb, "b")):
                _, pl = _captured(ref.print_flow_stats, tag, fld)
                st_lines += pl
                vals = (fld.min(), fld.max(), fld.mean(), fld.std())                                        # what those lines format
                assert vals[0] == want["stats"][f]["min"] and vals[1] == want["stats"][f]["max"]
                scale = want["_"]["mean_abs"][f]
                for k, v in zip(("mean", "std"), vals[2:]):
                    dev = abs(float(v) - want["stats"][f][k]) / scale if scale else abs(float(v))
                    assert dev <= N * 2.0 ** -24, (name, r, f, k, v, want["stats"][f][k])
                    worst[k] = max(worst[k], dev)
                st_vals.append(np.array(vals, np.float32))
            ns = {"flow_pth": fa, "flow_onnx": fb, "metrics": m}
            exec(drawn, ns)
            f32.append(np.array([m[k] for k in F32_KEYS], np.float32))
            pear.append(m["Pearson corr"])
            agree.append([m["agreements"][k] for k in m["agreements"]])
            stats.append(np.stack(st_vals))
            lines.append("\n".join(printed) + "\f" + "\n".join(ns["lines"]) + "\f" + "\n".join(st_lines))
        if name in FO.ORDINARY:
            for row in own_rows:
                assert row["_"]["nearest_tau"] > 1e-6, (name, row["_"]["nearest_tau"])                        # (a)
            mid = [v for v in own_rows[-1]["agreements"].values() if 5.0 < v < 95.0]
            assert len(mid) >= min(2, len(taus)), (name, own_rows[-1]["agreements"])                        # (b)
        arrays[name + "/digest"] = np.array(FO.digest(a, b))
        arrays[name + "/ref32"] = np.stack(f32)
        arrays[name + "/pearson"] = np.array(pear, np.float64)
        arrays[name + "/agree"] = np.array(agree, np.float64)
        arrays[name + "/stats"] = np.stack(stats)
        arrays[name + "/lines"] = np.array(lines)
        print("%-12s n=%d %dx%d nearest threshold %.2e agreements %s kappa %.2f"
              % (name, n, c["H"], c["W"], min(r["_"]["nearest_tau"] for r in own_rows),
                 np.round(list(own_rows[-1]["agreements"].values()), 1), want_rows[-1]["_"]["kappa"]))
    arrays["deviation_keys"] = np.array(SUM_KEYS)
    arrays["deviation"] = np.array([worst[k] for k in SUM_KEYS], np.float64)
    print("largest relative deviation of the reference's float32 values from the float64 oracle:")
    for k in SUM_KEYS:
        print("  %-18s %.3e" % (k, worst[k]))
    np.savez_compressed(out_path, **arrays)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g18_flow_compare.npz"))
