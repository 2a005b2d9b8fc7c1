"""NumPy restatement of estimate_vanishing_point_from_flow (pwc_extract_flow_video_vanishpoint.py:93-255) on the arrow grid, with the
intermediate values the tests compare (tests/test_vanishing_cpu.py, tests/test_gpu_vanishing.py), the fixture's cases and the margin
conditions that make the discrete outcomes of a case safe against a last-place difference in hypot.

Differences from the reference, all on purpose:
  * the input is the grid of sampled vectors vec [Gy,Gx,2] (the reference's flow[y, x] at y = gy*step, x = gx*step), not the frame;
  * the random subsample is the explicit index list `idx` into the kept vectors (what np.random.choice returned);
  * failures are status codes (2 fewer than 5 vectors, 3 fewer than min_pairs intersections, 4 empty histogram) and a refinement
    that does not happen is status 1, as csrc/pwc_vanishing.hip reports them;
  * a cell is kept when its magnitude is >= min_mag AND finite, the kernel's rule.  The reference's `mag < min_mag: continue` keeps a
    NaN magnitude, which poisons its median; for finite vectors the two rules are the same, so every recorded result is unchanged.
"""
import math

import numpy as np

# name -> frame (H, W), step, min_mag, max_points, grid_size, min_pairs, field kind
CASES = {
    "a": dict(frame=(96, 128), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="radial_in"),
    "b": dict(frame=(100, 135), step=7, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="radial_out"),
    "c": dict(frame=(96, 128), step=8, min_mag=1.0, max_points=32, grid_size=64, min_pairs=50, kind="radial_sub"),
    "d": dict(frame=(64, 64), step=8, min_mag=0.5, max_points=300, grid_size=64, min_pairs=50, kind="axis"),
    "e": dict(frame=(96, 128), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="few"),
    "f": dict(frame=(96, 128), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="translation"),
    "g": dict(frame=(96, 128), step=16, min_mag=1.0, max_points=300, grid_size=16, min_pairs=50, kind="radial_even"),
    "h": dict(frame=(96, 128), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="radial_in2"),
}
# The cases of tests/golden/g19_vanishing_edges.npz (tools/gen_golden_vanishing.py edges): the sizes, limits and decision boundaries the
# eight cases above stay away from.  Same columns.
EDGE_CASES = {
    # the shipped geometries; 300 of > 700 kept cells, the cut of the selection inside the second round of 256 positions, mid-wave
    "p768": dict(frame=(384, 512), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="edge_weak"),
    # ... and inside a third or later round: half the cells are weak, so the 300th kept one comes late in any order
    "p1792": dict(frame=(448, 1024), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="edge_half"),
    # max_points = n_kept - 1: the by-order path drops exactly one cell
    "plus1": dict(frame=(96, 128), step=8, min_mag=1.0, max_points=187, grid_size=64, min_pairs=50, kind="edge_188"),
    # a portrait frame and the largest max_points: every LDS array full, 523 776 pairs
    "full1024": dict(frame=(512, 256), step=8, min_mag=1.0, max_points=1024, grid_size=64, min_pairs=50, kind="edge_portrait"),
    # the smallest N that is not status 2: 12 of the 16 pair workgroups have no row
    "n5": dict(frame=(96, 128), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=5, kind="five"),
    # fewer than 5 inliers: the bin centre stands
    "st1": dict(frame=(96, 128), step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=5, kind="seven"),
    # gx = 65 536, the largest index the 16-bit grid coordinates hold; cells 0 and 65 535 selected
    "wide": dict(frame=(1, 65536), step=1, min_mag=1.0, max_points=1024, grid_size=16, min_pairs=50, kind="wide"),
    # unit axis-aligned vectors, mirror-symmetric in x: the histogram maximum is attained by two bins with exactly equal weight
    "tie": dict(frame=(64, 64), step=8, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, kind="tie"),
    "tie16": dict(frame=(64, 64), step=8, min_mag=1.0, max_points=300, grid_size=16, min_pairs=50, kind="tie"),
    # the same at 32 x 32 bins, the grid at which this geometry lets the lower tied index sit in the HIGHER lane (see tie_lanes)
    "tie32": dict(frame=(64, 64), step=8, min_mag=1.0, max_points=300, grid_size=32, min_pairs=50, kind="tie"),
    # magnitudes exactly min_mag (kept), exactly half of it and one float32 below it (dropped)
    "atmin": dict(frame=(64, 64), step=8, min_mag=2.0, max_points=300, grid_size=64, min_pairs=50, kind="atmin"),
}
ALL_CASES = dict(CASES, **EDGE_CASES)
TIE_CASES = ("tie", "tie16", "tie32")
# intersections exactly on bin edges, in exact arithmetic on both sides.  For the edge cases among them every vector is axis-aligned
# with magnitude 0, 1 or 2 (hypot(m, 0) == m on every implementation) and every weight is exactly 1 (2^40 on the device), so no
# last-place difference can exist: their "mag" margin is "every vector is axis-aligned" (the tie cases have magnitude == min_mag on
# purpose, as atmin has) and their "best" margin allows an exact tie, the next distinct weight at most (1 - 1e-6) x the best.
EXACT_EDGE_CASES = ("d",) + TIE_CASES + ("atmin",)
BATCH_CASES = ("a", "e", "h", "f")  # one geometry and grid size: a failing frame between good ones, another at the end
MAX_MAG_RATIO = 100.0
MAX_COND = 1e3


def grid_shape(frame, step):
    return -(-frame[0] // step), -(-frame[1] // step)


def make_field(name, seed):
    """float32 [Gy,Gx,2] of a case; the generator re-draws `seed` until the margins hold."""
    c = ALL_CASES[name]
    (H, W), step, kind = c["frame"], c["step"], c["kind"]
    gy, gx = grid_shape(c["frame"], step)
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(gy) * float(step), np.arange(gx) * float(step), indexing="ij")
    if kind.startswith("radial"):
        focus, gain, sigma = {"radial_in": ((70.3, 41.7), 0.12, 0.15), "radial_in2": ((30.5, 60.2), 0.12, 0.15),
                              "radial_even": ((50.9, 30.1), 0.12, 0.15), "radial_sub": ((66.6, 50.5), 0.12, 0.10),
                              "radial_out": ((-30.0, 45.0), 0.05, 0.05)}[kind]
        f = gain * np.stack([xx - focus[0], yy - focus[1]], axis=-1) + sigma * g.standard_normal((gy, gx, 2))
        if kind != "radial_out":                       # some cells below min_mag, so that the selection has something to drop
            weak = g.choice(gy * gx, size=int(g.integers(2, 6)), replace=False)
            f.reshape(-1, 2)[weak] *= 0.02
    elif kind == "axis":
        dirs = np.array([(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (0.0, 0.0)])
        f = dirs[g.integers(0, 5, size=(gy, gx))]
    elif kind == "few":
        f = 0.05 * g.standard_normal((gy, gx, 2))
        strong = g.choice(gy * gx, size=3, replace=False)
        f.reshape(-1, 2)[strong] = 3.0 * g.standard_normal((3, 2)) + 4.0
    elif kind == "translation":
        f = np.broadcast_to(np.array([3.0, 1.5]), (gy, gx, 2)).copy()
    else:
        f = _edge_field(kind, g, gy, gx, step, xx, yy)
    return np.ascontiguousarray(f, dtype=np.float32)


def _edge_field(kind, g, gy, gx, step, xx, yy):
    """The fields of EDGE_CASES (float64 [Gy,Gx,2])."""
    dirs = np.array([(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (0.0, 0.0)])
    if kind in ("edge_weak", "edge_half", "edge_188", "edge_portrait"):
        focus, gain, sigma = {"edge_weak": ((250.3, 190.7), 0.10, 0.15), "edge_half": ((500.3, 230.7), 0.10, 0.15),
                              "edge_188": ((68.3, 52.4), 0.25, 0.10), "edge_portrait": ((130.3, 250.7), 0.12, 0.15)}[kind]
        f = gain * np.stack([xx - focus[0], yy - focus[1]], axis=-1) + sigma * g.standard_normal((gy, gx, 2))
        n_weak = gy * gx // 2 if kind == "edge_half" else 4 if kind == "edge_188" else int(g.integers(3, 8))
        weak = g.choice(gy * gx, size=n_weak, replace=False)
        f.reshape(-1, 2)[weak] *= 0.005
    elif kind in ("five", "seven"):
        # weak noise everywhere; five (four) strong cells pointing away from one focus, and for "seven" three strong strays
        f = 0.05 * g.standard_normal((gy, gx, 2))
        focus = np.array([60.0, 45.0]) + g.uniform(-6.0, 6.0, 2)
        n_good, n_stray = (5, 0) if kind == "five" else (4, 3)
        cells = g.choice(gy * gx, size=n_good + n_stray, replace=False)
        pos = np.stack([(cells % gx) * float(step), (cells // gx) * float(step)], axis=-1)
        sigma = 0.15 if kind == "five" else 0.01
        v = 0.12 * (pos - focus) + sigma * g.standard_normal(pos.shape)
        v[n_good:] = 3.0 * g.standard_normal((n_stray, 2)) + 4.0
        f.reshape(-1, 2)[cells] = v
    elif kind == "wide":
        # one row of 65 536 cells, exact zeros but for ~1500 cells that point at (fx, fy) just above the row: ~500 within a few hundred
        # pixels of it (steep lines, which keep the refinement well conditioned), ~1000 anywhere, and the two end cells
        fx, fy = 28672.37, 0.45
        near = int(fx) - 400 + g.choice(800, size=500, replace=False)
        far = g.choice(gx, size=1000, replace=False)
        cells = np.unique(np.concatenate([near, far, [0, gx - 1]]))
        tx, ty = fx + 0.002 * g.standard_normal(len(cells)), fy + 0.002 * g.standard_normal(len(cells))
        d = np.stack([tx - cells, ty - 0.0], axis=-1)
        d *= (g.uniform(2.0, 20.0, len(cells)) / np.hypot(d[:, 0], d[:, 1]))[:, None]
        f = np.zeros((gy, gx, 2))
        f[0, cells] = d
    elif kind == "tie":
        half = dirs[g.integers(0, 5, size=(gy, gx // 2))]
        f = np.concatenate([half, half[:, ::-1] * np.array([-1.0, 1.0])], axis=1)          # mirror image about the vertical centre line
    elif kind == "atmin":
        below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
        scale = np.array([2.0, 2.0, 2.0, 1.0, below])[g.integers(0, 5, size=(gy, gx))]
        f = dirs[g.integers(0, 5, size=(gy, gx))] * scale[..., None]
    else:
        raise ValueError(kind)
    return f


def frame_flow(vec, frame, step):
    """An (H, W, 2) float32 flow whose samples every `step` pixels are vec (what the reference's function takes)."""
    flow = np.zeros(tuple(frame) + (2,), np.float32)
    flow[::step, ::step] = vec
    return flow


def order_from_idx(keep, idx):
    """A permutation of the cells under which the device's rule selects kept[idx[0]], kept[idx[1]], ...: those cells first, then
    every other cell in ascending order."""
    kept = np.flatnonzero(np.asarray(keep).ravel())
    first = kept[np.asarray(idx, dtype=np.int64)]
    rest = np.setdiff1d(np.arange(np.asarray(keep).size), first)
    return np.concatenate([first, rest]).astype(np.int32)


def order_from_idx_interleaved(keep, idx):
    """As order_from_idx, with every cell that is NOT kept spread evenly among the selected ones, before the last of them: the
    selection skips those, so the same cells are selected, and the cut falls len(idx) - 1 + (cells not kept) positions in."""
    keep = np.asarray(keep).ravel()
    first = np.flatnonzero(keep)[np.asarray(idx, dtype=np.int64)]
    unkept = np.flatnonzero(~keep)
    at = (np.arange(len(unkept)) * (len(first) - 1)) // max(len(unkept), 1) + 1      # in front of first[at], 1 <= at <= len(first) - 1
    head = np.insert(first, at, unkept)
    rest = np.setdiff1d(np.flatnonzero(keep), first)
    return np.concatenate([head, rest]).astype(np.int32)


def select_by_order(keep, order, max_points):
    """The device's selection rule: all kept cells row-major when there are at most max_points of them, else the kept cells ranked by
    their position in `order`, the first max_points, in that order.  `order` is meant to be a permutation of the cells; when it is not,
    an entry outside 0 .. cells-1 is skipped and an entry that repeats an earlier one selects its cell again (include/pwc_hip.h)."""
    keep = np.asarray(keep).ravel()
    kept = np.flatnonzero(keep)
    if len(kept) <= max_points:
        return kept
    order = np.asarray(order, dtype=np.int64)
    order = order[(order >= 0) & (order < keep.size)]
    return order[keep[order]][:max_points]


def cut_position(keep, order, max_points):
    """Position in `order` of the last selected cell (the by-order path): where `r < n_used` cuts the compaction."""
    keep = np.asarray(keep).ravel()
    order = np.asarray(order, dtype=np.int64)
    valid = (order >= 0) & (order < keep.size)
    hit = np.zeros(len(order), bool)
    hit[valid] = keep[order[valid]]
    return int(np.flatnonzero(hit)[:max_points][-1])


def idx_of_cells(keep, cells):
    """The index list into the kept cells that names `cells` (the inverse of kept[idx])."""
    kept = np.flatnonzero(np.asarray(keep).ravel())
    idx = np.searchsorted(kept, np.asarray(cells, dtype=np.int64))
    assert np.array_equal(kept[idx], cells)
    return idx


def edges(lo, hi, grid):
    """np.linspace(lo, hi, grid + 1) spelled out: k * ((hi - lo) / grid) + lo, the last edge hi itself."""
    e = np.arange(grid + 1, dtype=np.float64) * ((hi - lo) / grid) + lo
    e[grid] = hi
    return e


def pairs_loop(xs, ys, dxn, dyn, mags, H, W):
    """The reference's double loop over the pairs (:167-194), in Python as it is there -> (ix, iy, w, denom of every pair)."""
    inter_x, inter_y, inter_w, denoms = [], [], [], []
    N = len(xs)
    for i in range(N):
        p1x, p1y, d1x, d1y = xs[i], ys[i], dxn[i], dyn[i]
        for j in range(i + 1, N):
            d2x, d2y = dxn[j], dyn[j]
            denom = d1x * d2y - d1y * d2x
            denoms.append(denom)
            if abs(denom) < 1e-6:
                continue
            dp_x, dp_y = xs[j] - p1x, ys[j] - p1y
            t1 = (dp_x * d2y - dp_y * d2x) / denom
            ix, iy = p1x + t1 * d1x, p1y + t1 * d1y
            if -0.5 * W <= ix <= 1.5 * W and -0.5 * H <= iy <= 1.5 * H:
                inter_x.append(ix)
                inter_y.append(iy)
                inter_w.append(mags[i] * mags[j])
    return np.array(inter_x), np.array(inter_y), np.array(inter_w), np.array(denoms)


def pairs_numpy(xs, ys, dxn, dyn, mags, H, W):
    """The same values, element for element and in the same pair order, as array expressions.  Also returns the intersections of
    every non-parallel pair before the range test (for the margins)."""
    ii, jj = np.triu_indices(len(xs), 1)
    denom = dxn[ii] * dyn[jj] - dyn[ii] * dxn[jj]
    ok = ~(np.abs(denom) < 1e-6)
    ii, jj, dn = ii[ok], jj[ok], denom[ok]
    t1 = ((xs[jj] - xs[ii]) * dyn[jj] - (ys[jj] - ys[ii]) * dxn[jj]) / dn
    ix, iy = xs[ii] + t1 * dxn[ii], ys[ii] + t1 * dyn[ii]
    inside = (-0.5 * W <= ix) & (ix <= 1.5 * W) & (-0.5 * H <= iy) & (iy <= 1.5 * H)
    return ix[inside], iy[inside], (mags[ii] * mags[jj])[inside], denom, ix, iy


def estimate(vec, frame, step=16, min_mag=1.0, max_points=300, grid_size=64, min_pairs=50, idx=None, loop=False):
    """dict of the result and every intermediate value.  xy / prob are None for status >= 2."""
    H, W = frame
    vec = np.asarray(vec)
    gy, gx = vec.shape[:2]
    assert (gy, gx) == grid_shape(frame, step) and vec.dtype == np.float32
    dx, dy = vec[..., 0].astype(np.float64).ravel(), vec[..., 1].astype(np.float64).ravel()
    mag = np.array([math.hypot(a, b) for a, b in zip(dx, dy)])
    keep = (mag >= min_mag) & np.isfinite(mag)         # == ~(mag < min_mag) for finite vectors; the reference keeps a NaN magnitude
    cells = np.flatnonzero(keep)
    r = dict(status=0, mag_all=mag, keep=keep, n_kept=len(cells), n_used=min(len(cells), max_points), pairs_kept=0, best=(-1, -1),
             inliers=0, xy=None, prob=None, center=None, denom=np.zeros(0), ix_all=np.zeros(0), iy_all=np.zeros(0), ix=np.zeros(0),
             iy=np.zeros(0), dists=np.zeros(0), thresh=None, cond=None, runner_up=None, best_weight=None, hist=None, cells=cells, vec=vec)
    if len(cells) < 5:
        r["status"] = 2
        return r
    if len(cells) > max_points:
        if idx is None:
            raise ValueError("more than max_points vectors are kept: the subsample needs idx")
        cells = cells[np.asarray(idx, dtype=np.int64)]
        assert len(cells) <= max_points                # fewer only from an `order` that is no permutation
        r["n_used"] = len(cells)
        if len(cells) < 5:
            r["status"] = 2
            return r
    r["cells"] = cells
    xs, ys = (cells % gx).astype(np.float64) * step, (cells // gx).astype(np.float64) * step
    mags = mag[cells]
    dxn, dyn = dx[cells] / mags, dy[cells] / mags
    r.update(mags=mags, xs=xs, ys=ys, dxn=dxn, dyn=dyn)
    if loop:
        ix, iy, w, denom = pairs_loop(xs, ys, dxn, dyn, mags, H, W)
        ix_all, iy_all = ix, iy
    else:
        ix, iy, w, denom, ix_all, iy_all = pairs_numpy(xs, ys, dxn, dyn, mags, H, W)
    r.update(denom=denom, ix_all=ix_all, iy_all=iy_all, ix=ix, iy=iy, pairs_kept=len(ix))
    if len(ix) < min_pairs:
        r["status"] = 3
        return r
    x_min, x_max, y_min, y_max = -0.5 * W, 1.5 * W, -0.5 * H, 1.5 * H
    hist, x_edges, y_edges = np.histogram2d(ix, iy, bins=grid_size, range=[[x_min, x_max], [y_min, y_max]], weights=w)
    assert np.array_equal(x_edges, edges(x_min, x_max, grid_size)) and np.array_equal(y_edges, edges(y_min, y_max, grid_size))
    r.update(hist=hist, x_edges=x_edges, y_edges=y_edges)
    max_idx = int(np.argmax(hist))
    if hist.flat[max_idx] <= 0:
        r["status"] = 4
        return r
    bx, by = np.unravel_index(max_idx, hist.shape)
    flat = np.sort(hist.ravel())
    vx = 0.5 * (x_edges[bx] + x_edges[bx + 1])
    vy = 0.5 * (y_edges[by] + y_edges[by + 1])
    prob = float(hist[bx, by] / (np.sum(hist) + 1e-9))
    r.update(best=(int(bx), int(by)), best_weight=float(flat[-1]), runner_up=float(flat[-2]), center=(float(vx), float(vy)), prob=prob)
    nx, ny = -dyn, dxn
    A = np.stack([nx, ny], axis=1)
    b = nx * xs + ny * ys
    candidate = np.array([vx, vy], dtype=np.float32)
    dists = np.abs(A @ candidate - b)
    thresh = np.median(dists) * 3.0 + 1e-6
    inl = dists < thresh
    r.update(dists=dists, thresh=float(thresh), inlier_mask=inl, inliers=int(inl.sum()), xy=(float(vx), float(vy)), status=1)
    if inl.sum() >= 5:
        sv = np.linalg.svd(A[inl], compute_uv=False)
        r["cond"] = float(sv[0] / sv[-1]) if sv[-1] > 0 else float("inf")
        sol = np.linalg.lstsq(A[inl], b[inl], rcond=None)[0]
        r.update(xy=(float(sol[0]), float(sol[1])), status=0)
    return r


def margins(r, case):
    """The conditions under which a last-place difference upstream cannot change a discrete outcome of this case -> {name: bool}."""
    c = ALL_CASES[case]
    (H, W), min_mag = c["frame"], c["min_mag"]
    exact_edge_case = case in EXACT_EDGE_CASES and case in EDGE_CASES
    out = {}
    if exact_edge_case:                                # hypot(m, 0) == m exactly: a magnitude may sit on min_mag
        out["mag"] = bool(((r["vec"][..., 0] == 0) | (r["vec"][..., 1] == 0)).all())
    else:
        out["mag"] = bool((np.abs(r["mag_all"] - min_mag) > 1e-6 * min_mag).all())
    out["denom"] = bool((np.abs(np.abs(r["denom"]) - 1e-6) > 1e-6 * 1e-6).all())
    lim = True
    for v, size in ((r["ix_all"], W), (r["iy_all"], H)):
        v = v[np.isfinite(v)]
        lim = lim and bool((np.abs(v + 0.5 * size) > 1e-9 * size).all() and (np.abs(v - 1.5 * size) > 1e-9 * size).all())
    out["range"] = lim
    edge_ok = True
    if r["hist"] is not None and case not in EXACT_EDGE_CASES:
        for v, e, size in ((r["ix"], r["x_edges"], W), (r["iy"], r["y_edges"], H)):
            k = np.clip(np.searchsorted(e, v), 1, len(e) - 1)                     # the nearest edge is e[k - 1] or e[k]
            edge_ok = edge_ok and bool((np.minimum(np.abs(v - e[k - 1]), np.abs(v - e[k])) > 1e-9 * size).all())
    out["edges"] = edge_ok
    if exact_edge_case and r["hist"] is not None:      # integer weights: an exact tie is safe, the next DISTINCT weight must be clear
        lower = r["hist"][r["hist"] < r["best_weight"]]
        out["best"] = lower.size == 0 or float(lower.max()) <= (1.0 - 1e-6) * r["best_weight"]
    else:
        out["best"] = r["runner_up"] is None or r["best_weight"] >= (1.0 + 1e-6) * r["runner_up"]
    out["inlier"] = r["thresh"] is None or bool((np.abs(r["dists"] - r["thresh"]) > 1e-9 * r["thresh"]).all())
    out["mag_ratio"] = r["n_kept"] == 0 or float(r["mag_all"][r["keep"]].max()) <= MAX_MAG_RATIO * min_mag
    out["cond"] = r["cond"] is None or r["cond"] <= MAX_COND
    return out


def xy_tolerance(r):
    """The normal-equations bound the refined point is compared with: 1e3 * cond(A_in)^2 * 2^-53 * max(1, |vx|, |vy|)."""
    cond = r["cond"] if r["cond"] is not None else 1.0
    return 1e3 * cond * cond * 2.0 ** -53 * max(1.0, abs(r["xy"][0]), abs(r["xy"][1]))


def normal_equations_xy(r):
    """The kernel's own refinement restated in float64 NumPy: the 2 x 2 normal equations of the inlier lines with the right-hand side
    taken about the bin centre, solved by Cramer's rule (np.sum's order, no contraction) -> (vx, vy), or None without a refinement."""
    if r["status"] != 0:
        return None
    inl = r["inlier_mask"]
    cx, cy = r["center"]
    nx, ny = -r["dyn"][inl], r["dxn"][inl]
    cc = (nx * r["xs"][inl] + ny * r["ys"][inl]) - (nx * cx + ny * cy)
    s0, s1, s2, s3, s4 = np.sum(nx * nx), np.sum(nx * ny), np.sum(ny * ny), np.sum(nx * cc), np.sum(ny * cc)
    det = s0 * s2 - s1 * s1
    return float(cx + (s2 * s3 - s1 * s4) / det), float(cy + (s0 * s4 - s1 * s3) / det)


def normal_equations_fraction(r):
    """|normal_equations_xy - the oracle's lstsq answer| as a fraction of xy_tolerance: how much of the bound the method alone uses,
    before any device is involved (0.0 without a refinement)."""
    ne = normal_equations_xy(r)
    if ne is None:
        return 0.0
    return max(abs(ne[0] - r["xy"][0]), abs(ne[1] - r["xy"][1])) / xy_tolerance(r)


MAX_NORMAL_EQ_FRACTION = 0.1


def edge_margins(r, case):
    """margins() and, for the cases of EDGE_CASES, that the normal equations themselves stay within 10 % of xy_tolerance."""
    out = margins(r, case)
    out["normal_eq"] = normal_equations_fraction(r) <= MAX_NORMAL_EQ_FRACTION
    return out


def tie_bins(r):
    """Flat indices gx * grid + gy of the bins that attain the histogram maximum, ascending."""
    return np.flatnonzero(r["hist"].ravel() == r["hist"].max())


def tie_lanes(r, threads=256):
    """Lanes of finish_kernel's arg-max that hold the two lowest tied bins (lane = flat index mod 256).  On a 64 x 64 frame at step 8
    the lines are x = 8 cx and y = 8 cy, every bin that gets a vote has gx = (8 cx + 32) / (128 / grid), and the count of bin
    (cx, cy) is (vertical cells in column cx) * (horizontal cells in row cy): the tied bins are a product set columns x rows.  With
    grid 64, gx = 16 + 4 cx is a multiple of 4, so lane = gy: a pair that differs in gx alone sits in ONE lane (its ascending scan
    decides), and no field of this geometry puts the lower of two tied indices into the higher lane.  With grid 16 there is one bin
    per lane.  With grid 32, gx = 8 + 2 cx and lane = (gx mod 8) * 32 + gy: columns 3 | 4 (gx 14 | 16) or 2 | 5 (gx 12 | 18) put the
    LOWER index in the HIGHER lane."""
    t = tie_bins(r)
    return int(t[0] % threads), int(t[1] % threads)


def tie_tree_sides(r, threads=256):
    """Where the two lowest tied bins meet in the arg-max's tree reduction (slot tid takes slot tid + s for s = 128, 64, ...): the
    lanes a and b first share a slot at s = 2^k, k the lowest bit in which they differ, one of them coming from the lower slot (0) and
    one from the upper (1) -> (side of the lower index, side of the higher index), or None when one lane holds both.  (1, 0) is the
    arrangement in which a tree that kept the lower SLOT on a tie would return the higher index; columns 3 | 4 at grid 32 give it
    (lanes 192 + gy | gy), columns 2 | 5 do not (lanes 128 + gy | 64 + gy meet at s = 64 with the lower index below)."""
    a, b = tie_lanes(r, threads)
    if a == b:
        return None
    k = ((a ^ b) & -(a ^ b)).bit_length() - 1
    return (a >> k) & 1, (b >> k) & 1
