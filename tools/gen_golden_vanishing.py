"""Generate tests/golden/g16_vanishing.npz, or with `edges` tests/golden/g19_vanishing_edges.npz, from the REFERENCE's own
estimate_vanishing_point_from_flow.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE); the tests read the fixture.  The script's
module imports cv2, which is not installed, so only that one function is taken: the file is parsed with ``ast`` and the function is
compiled in this process with ``math`` and ``np`` in scope.  Its text goes nowhere.

The cases, their generators and the margin conditions are in tests/vanishing_oracle.py.  A case's seed is re-drawn until
  * every margin condition of vanishing_oracle.margins holds (no exemption),
  * the case shows what it is there for (odd / even N, a focus outside the frame, N > max_points, ...),
  * the oracle reproduces the reference's return value: None where it returned None, else vx, vy, prob to a relative 1e-12.
For the subsample case NumPy's global state is seeded, the function is called, and the index list the same seed draws is recorded.

The edge cases (vanishing_oracle.EDGE_CASES) follow the same protocol with vanishing_oracle.edge_margins, which adds that a float64
restatement of the kernel's own normal equations lands within 10 % of xy_tolerance of the oracle's lstsq answer.

    python tools/gen_golden_vanishing.py [out.npz]
    python tools/gen_golden_vanishing.py edges [out.npz]
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


def edge_shows_its_point(name, r, idx):
    c = VO.EDGE_CASES[name]
    H, W = c["frame"]
    if name in ("p768", "p1792"):                      # the cut of the by-order compaction: inside round 2 / a later round, mid-wave
        if not (r["status"] == 0 and r["n_kept"] > 700 and idx is not None):
            return False
        cut = VO.cut_position(r["keep"], VO.order_from_idx_interleaved(r["keep"], idx), c["max_points"])
        return cut % 64 != 0 and (256 <= cut < 512 if name == "p768" else cut >= 512)
    if name == "plus1":
        return r["status"] == 0 and r["n_kept"] == c["max_points"] + 1
    if name == "full1024":
        return r["status"] == 0 and H > W and r["n_kept"] > 1024 and r["n_used"] == 1024 == c["max_points"]
    if name == "n5":
        return r["status"] in (0, 1) and r["n_kept"] == 5
    if name == "st1":
        return r["status"] == 1 and 5 <= r["n_kept"] <= 8 and r["inliers"] < 5 and r["xy"] == r["center"]
    if name == "wide":
        return r["status"] == 0 and r["n_kept"] > 1024 and 0 in r["cells"] and r["keep"].size - 1 in r["cells"]
    if name in VO.TIE_CASES:
        if r["status"] != 0 or len(VO.tie_bins(r)) < 2:
            return False
        lanes = VO.tie_lanes(r)                        # tie32: the lower index in the higher lane and on the upper side of the tree
        return lanes[0] > lanes[1] and VO.tie_tree_sides(r) == (1, 0) if name == "tie32" else True
    if name == "atmin":
        m = r["mag_all"]
        return (r["status"] == 0 and r["n_kept"] == int((m == 2.0).sum()) and (m == 1.0).any()
                and (m == float(np.nextafter(np.float32(2.0), np.float32(0.0)))).any())
    raise KeyError(name)


def shows_its_point(name, r, idx=None):
    if name in VO.EDGE_CASES:
        return edge_shows_its_point(name, r, idx)
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


def main(out_path, table=VO.CASES, margins=VO.margins, first_seed=1600, tries=100):
    fn = reference_function()
    arrays = {}
    for ci, (name, c) in enumerate(table.items()):
        kw = dict(step=c["step"], min_mag=c["min_mag"], max_points=c["max_points"], grid_size=c["grid_size"], min_pairs=c["min_pairs"])
        for seed in range(first_seed + tries * ci, first_seed + tries * ci + tries):
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
            m = margins(r, name)
            same = (ref is None) == (r["status"] >= 2) and (ref is None or (
                rel_close(ref[0], r["xy"][0]) and rel_close(ref[1], r["xy"][1]) and rel_close(ref[2], r["prob"])))
            shows = shows_its_point(name, r, idx)
            if all(m.values()) and same and shows:
                break
            print("case %s seed %d rejected: margins %s, oracle == reference %s, shows its point %s"
                  % (name, seed, [k for k, v in m.items() if not v], same, shows))
        else:
            raise SystemExit("case %s: no seed satisfied the conditions" % name)
        print("case %s seed %d: status %d N %d/%d pairs %d best %s inliers %d cond %s normal equations %.3g of tolerance, reference %s"
              % (name, seed, r["status"], r["n_used"], r["n_kept"], r["pairs_kept"], r["best"], r["inliers"], r["cond"],
                 VO.normal_equations_fraction(r), ref))
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
    args = sys.argv[1:]
    if args and args[0] == "edges":
        main(args[1] if len(args) > 1 else os.path.join(REPO, "tests", "golden", "g19_vanishing_edges.npz"), VO.EDGE_CASES,
             VO.edge_margins, first_seed=19000, tries=400)
    else:
        main(args[0] if args else os.path.join(REPO, "tests", "golden", "g16_vanishing.npz"))
