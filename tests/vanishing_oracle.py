"""NumPy restatement of estimate_vanishing_point_from_flow (pwc_extract_flow_video_vanishpoint.py:93-255) on the arrow grid, with the
intermediate values the tests compare (tests/test_vanishing_cpu.py, tests/test_gpu_vanishing.py), the fixture's cases and the margin
conditions that make the discrete outcomes of a case safe against a last-place difference in hypot.

Differences from the reference, all on purpose:
  * the input is the grid of sampled vectors vec [Gy,Gx,2] (the reference's flow[y, x] at y = gy*step, x = gx*step), not the frame;
  * the random subsample is the explicit index list `idx` into the kept vectors (what np.random.choice returned);
  * failures are status codes (2 fewer than 5 vectors, 3 fewer than min_pairs intersections, 4 empty histogram) and a refinement
    that does not happen is status 1, as csrc/pwc_vanishing.hip reports them.
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
EXACT_EDGE_CASES = ("d",)          # intersections exactly on bin edges, in exact arithmetic on both sides
BATCH_CASES = ("a", "e", "h", "f")  # one geometry and grid size: a failing frame between good ones, another at the end
MAX_MAG_RATIO = 100.0
MAX_COND = 1e3


def grid_shape(frame, step):
    return -(-frame[0] // step), -(-frame[1] // step)


def make_field(name, seed):
    """float32 [Gy,Gx,2] of a case; the generator re-draws `seed` until the margins hold."""
    c = CASES[name]
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
        raise ValueError(kind)
    return np.ascontiguousarray(f, dtype=np.float32)


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


def select_by_order(keep, order, max_points):
    """The device's selection rule: all kept cells row-major when there are at most max_points of them, else the kept cells ranked by
    their position in `order`, the first max_points, in that order."""
    keep = np.asarray(keep).ravel()
    kept = np.flatnonzero(keep)
    if len(kept) <= max_points:
        return kept
    order = np.asarray(order, dtype=np.int64)
    return order[keep[order]][:max_points]


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
    keep = ~(mag < min_mag)
    cells = np.flatnonzero(keep)
    r = dict(status=0, mag_all=mag, keep=keep, n_kept=len(cells), n_used=min(len(cells), max_points), pairs_kept=0, best=(-1, -1),
             inliers=0, xy=None, prob=None, center=None, denom=np.zeros(0), ix_all=np.zeros(0), iy_all=np.zeros(0), ix=np.zeros(0),
             iy=np.zeros(0), dists=np.zeros(0), thresh=None, cond=None, runner_up=None, best_weight=None, hist=None, cells=cells)
    if len(cells) < 5:
        r["status"] = 2
        return r
    if len(cells) > max_points:
        if idx is None:
            raise ValueError("more than max_points vectors are kept: the subsample needs idx")
        cells = cells[np.asarray(idx, dtype=np.int64)]
        assert len(cells) == max_points
    r["cells"] = cells
    xs, ys = (cells % gx).astype(np.float64) * step, (cells // gx).astype(np.float64) * step
    mags = mag[cells]
    dxn, dyn = dx[cells] / mags, dy[cells] / mags
    r.update(mags=mags)
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
    c = CASES[case]
    (H, W), min_mag = c["frame"], c["min_mag"]
    out = {}
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
            edge_ok = edge_ok and bool((np.abs(v[:, None] - e[None, :]).min(axis=1) > 1e-9 * size).all())
    out["edges"] = edge_ok
    out["best"] = r["runner_up"] is None or r["best_weight"] >= (1.0 + 1e-6) * r["runner_up"]
    out["inlier"] = r["thresh"] is None or bool((np.abs(r["dists"] - r["thresh"]) > 1e-9 * r["thresh"]).all())
    out["mag_ratio"] = r["n_kept"] == 0 or float(r["mag_all"][r["keep"]].max()) <= MAX_MAG_RATIO * min_mag
    out["cond"] = r["cond"] is None or r["cond"] <= MAX_COND
    return out


def xy_tolerance(r):
    """The normal-equations bound the refined point is compared with: 1e3 * cond(A_in)^2 * 2^-53 * max(1, |vx|, |vy|)."""
    cond = r["cond"] if r["cond"] is not None else 1.0
    return 1e3 * cond * cond * 2.0 ** -53 * max(1.0, abs(r["xy"][0]), abs(r["xy"][1]))
