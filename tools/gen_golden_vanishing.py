"""Generate tests/golden/g16_vanishing.npz from the REFERENCE's own estimate_vanishing_point_from_flow.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.  The script's
module imports cv2, which is not installed, so only that one function is taken: the file is parsed with ``ast`` and the function is
compiled in this process with ``math`` and ``np`` in scope.  Its text goes nowhere.

The cases, their generators and the margin conditions are in tests/vanishing_oracle.py.  A case's seed is re-drawn until
  * every margin condition of vanishing_oracle.margins holds (no exemption),
  * the case shows what it is there for (odd / even N, a focus outside the frame, N > max_points, ...),
  * the oracle reproduces the reference's return value: None where it returned None, else vx, vy, prob to a relative 1e-12.
For the subsample case NumPy's global state is seeded, the function is called, and the index list the same seed draws is recorded.

    python tools/gen_golden_vanishing.py [out.npz]
"""
import ast
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PWC_REFERENCE", os.path.join(os.path.dirname(REPO), "reference"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import vanishing_oracle as VO  # noqa: E402

NAME = "estimate_vanishing_point_from_flow"


def reference_function():
    path = os.path.join(REF, "pwc_extract_flow_video_vanishpoint.py")
    tree = ast.parse(open(path).read())
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == NAME]
    assert len(tree.body) == 1
    scope = {"np": np, "math": math}
    exec(compile(tree, path, "exec"), scope)
    return scope[NAME]


def rel_close(a, b, tol=1e-12):
    return abs(a - b) <= tol * max(abs(a), abs(b), 1e-300)


def shows_its_point(name, r):
    c = VO.CASES[name]
    H, W = c["frame"]
    if name in ("a", "h"):
        return r["status"] == 0 and r["n_kept"] % 2 == 1 and r["n_kept"] < r["keep"].size
    if name == "b":
        return r["status"] == 0 and r["n_kept"] == r["keep"].size == c["max_points"] and -0.5 * W < r["xy"][0] < 0 and r["center"][0] < 0
    if name == "c":
        return r["status"] == 0 and r["n_kept"] > c["max_points"]
    if name == "d":
        on_edge = np.isin(r["ix"], r["x_edges"]).all() and np.isin(r["iy"], r["y_edges"]).all() if r["hist"] is not None else False
        return r["status"] == 0 and bool(on_edge)
    if name == "e":
        return r["status"] == 2 and 0 < r["n_kept"] < 5
    if name == "f":
        return r["status"] == 3 and r["n_kept"] >= 5 and r["pairs_kept"] == 0
    if name == "g":
        return r["status"] == 0 and r["n_kept"] % 2 == 0
    raise KeyError(name)


def main(out_path):
    fn = reference_function()
    arrays = {}
    for ci, (name, c) in enumerate(VO.CASES.items()):
        kw = dict(step=c["step"], min_mag=c["min_mag"], max_points=c["max_points"], grid_size=c["grid_size"], min_pairs=c["min_pairs"])
        for seed in range(1600 + 100 * ci, 1600 + 100 * ci + 100):
            vec = VO.make_field(name, seed)
            flow = VO.frame_flow(vec, c["frame"], c["step"])
            np.random.seed(seed)
            ref = fn(flow, **kw)
            n_kept = int((~(np.hypot(vec[..., 0].astype(np.float64), vec[..., 1].astype(np.float64)) < c["min_mag"])).sum())
            idx = None
            if n_kept > c["max_points"]:
                np.random.seed(seed)
                idx = np.random.choice(n_kept, c["max_points"], replace=False)
            r = VO.estimate(vec, c["frame"], idx=idx, **kw)
            m = VO.margins(r, name)
            same = (ref is None) == (r["status"] >= 2) and (ref is None or (
                rel_close(ref[0], r["xy"][0]) and rel_close(ref[1], r["xy"][1]) and rel_close(ref[2], r["prob"])))
            if all(m.values()) and same and shows_its_point(name, r):
                break
            print("case %s seed %d rejected: margins %s, oracle == reference %s, shows its point %s"
                  % (name, seed, [k for k, v in m.items() if not v], same, shows_its_point(name, r)))
        else:
            raise SystemExit("case %s: no seed satisfied the conditions" % name)
        print("case %s seed %d: status %d N %d/%d pairs %d best %s inliers %d cond %s reference %s"
              % (name, seed, r["status"], r["n_used"], r["n_kept"], r["pairs_kept"], r["best"], r["inliers"], r["cond"], ref))
        arrays["vec/" + name] = vec
        arrays["seed/" + name] = np.int64(seed)
        arrays["idx/" + name] = np.asarray(idx if idx is not None else [], dtype=np.int64)
        arrays["ref_ok/" + name] = np.bool_(ref is not None)
        arrays["ref/" + name] = np.asarray(ref if ref is not None else [np.nan] * 3, dtype=np.float64)
    np.savez_compressed(out_path, **arrays)
    size = os.path.getsize(out_path)
    print("wrote %s (%d bytes)" % (out_path, size))
    assert size <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g16_vanishing.npz"))
