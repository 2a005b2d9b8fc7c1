"""float64 NumPy restatement of the reference's epipolar utilities (train_fundamental.py:169-382), the oracle of
csrc/pwc_epipolar.hip.  Written from the reference's semantics; line numbers cite the reference's train_fundamental.py.

Per sample, on host arrays: flow_hw2 is [H,W,2] (float32 values), masks are [H,W]."""
import numpy as np

SQRT2 = np.sqrt(2.0)


def flow_to_pairs(flow_hw2, stride=4, mask_hw=None):
    """:169-194 -- strided grid points, endpoints in float64, non-finite / masked-out points dropped in grid order."""
    H, W, _ = flow_hw2.shape
    ys, xs = np.mgrid[0:H:stride, 0:W:stride]
    x = xs.ravel().astype(np.float64)
    y = ys.ravel().astype(np.float64)
    x2 = x + flow_hw2[ys, xs, 0].ravel().astype(np.float64)
    y2 = y + flow_hw2[ys, xs, 1].ravel().astype(np.float64)
    keep = np.isfinite(x2) & np.isfinite(y2)
    if mask_hw is not None:
        keep &= mask_hw[ys, xs].ravel().astype(bool)
    one = np.ones(int(keep.sum()))
    return np.stack([x[keep], y[keep], one], 1), np.stack([x2[keep], y2[keep], one], 1)


def hartley(p):
    """:197-207 -- homogeneous division by (w + 1e-12), centroid to 0, mean distance to sqrt(2)."""
    p = p / (p[:, 2:3] + 1e-12)
    c = p[:, :2].mean(axis=0)
    r = np.sqrt(((p[:, :2] - c) ** 2).sum(axis=1))
    s = SQRT2 / np.mean(r + 1e-12)
    T = np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])
    return (T @ p.T).T, T


def design_matrix(p1, p2):
    """:211-216 -- the n x 9 system of the Hartley-normalised pairs and the two normalisations: (A, T1, T2)."""
    q1, T1 = hartley(p1)
    q2, T2 = hartley(p2)
    u, v, up, vp = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    return np.column_stack([u * up, v * up, up, vp * u, vp * v, vp, u, v, np.ones_like(u)]), T1, T2


def eight_point(p1, p2, full_matrices=False):
    """:210-225 -- the right singular vector of the min(n, 9)-th largest singular value (numpy's thin SVD; for n = 8 that is
    NOT the null vector), rank 2, denormalise, scale by F[2,2] or the Frobenius norm.  full_matrices=True is NOT the reference:
    it always takes the 9th vector, the mistake a test of the n = 8 refit has to be able to see."""
    A, T1, T2 = design_matrix(p1, p2)
    vt = np.linalg.svd(A, full_matrices=full_matrices)[2]
    Fn = vt[-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Fn)
    Fn = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    Fm = T2.T @ Fn @ T1
    nrm = np.linalg.norm(Fm)
    if nrm > 0:
        Fm = Fm / (Fm[2, 2] if abs(Fm[2, 2]) > 1e-12 else nrm)
    return Fm


def sampson(Fm, p1, p2):
    """:228-233 -- Sampson distance with the homogeneous division by (w + 1e-12)."""
    p1 = p1 / (p1[:, 2:3] + 1e-12)
    p2 = p2 / (p2[:, 2:3] + 1e-12)
    a = p1 @ Fm.T
    b = p2 @ Fm
    e = (p2 * a).sum(axis=1)
    return e ** 2 / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2 + 1e-12)


def index_table(N, seed, iters):
    """:240-245 -- the sampler's index sequence: one default_rng(seed), one choice(N, 8, replace=False) per iteration."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(N, size=8, replace=False) for _ in range(iters)]).astype(np.int32)


def ransac(p1, p2, max_iters=2000, thresh=0.5, seed=0, idx=None):
    """:236-258 -> dict(F, ok, best, counts, hyps, idx).  Fails (ok False) when N < 8 or the best count < 8.
    idx [iters,8] replaces the sampler's table (max_iters and seed are then unused).  A row of it that holds an index outside
    [0, N) is the one input the reference cannot have: the product documents it as a NaN hypothesis with count 0, and so it is here."""
    N = p1.shape[0]
    if idx is not None:
        max_iters = len(idx)
    if N < 8:
        return dict(F=None, ok=False, best=-1, counts=np.zeros(max_iters, np.int64))
    if idx is None:
        idx = index_table(N, seed, max_iters)
    counts = np.empty(max_iters, np.int64)
    Fs = []
    for i in range(max_iters):
        if idx[i].min() < 0 or idx[i].max() >= N:
            Fs.append(np.full((3, 3), np.nan))
            counts[i] = 0
            continue
        Fc = eight_point(p1[idx[i]], p2[idx[i]])
        Fs.append(Fc)
        counts[i] = int((sampson(Fc, p1, p2) < thresh).sum())
    best = int(np.argmax(counts))            # first of the strictly largest
    if counts[best] < 8:
        return dict(F=None, ok=False, best=best, counts=counts, hyps=np.stack(Fs), idx=idx)
    inl = sampson(Fs[best], p1, p2) < thresh
    return dict(F=eight_point(p1[inl], p2[inl]), ok=True, best=best, counts=counts, hyps=np.stack(Fs), idx=idx)


def distance_map(flow_hw2, Fm):
    """:284-296 -- d of every pixel from the refit F."""
    H, W, _ = flow_hw2.shape
    ys, xs = np.mgrid[0:H, 0:W]
    one = np.ones(H * W)
    p1 = np.stack([xs.ravel().astype(np.float64), ys.ravel().astype(np.float64), one], 1)
    p2 = np.stack([(xs + flow_hw2[..., 0]).ravel().astype(np.float64), (ys + flow_hw2[..., 1]).ravel().astype(np.float64), one], 1)
    return sampson(Fm, p1, p2).reshape(H, W)


def threshold_mask(d, tau=1.0, keep_ratio=0.2, min_keep=0.05):
    """:298-327 on a distance map -> (mask [H,W] bool, thr or None when all true)."""
    fin = np.isfinite(d)
    if not fin.any():
        return np.ones(d.shape, bool), None
    dv = d[fin]
    thr = float(tau)
    if 0.0 < keep_ratio < 1.0:
        thr = min(thr, float(np.quantile(dv, keep_ratio)))
    keep = fin & (d <= thr)
    if 0.0 < min_keep < 1.0 and keep.mean() < min_keep:
        thr = min(float(tau), float(np.quantile(dv, min_keep)))      # may tighten: restated as written
        keep = fin & (d <= thr)
    return keep, thr


def epipolar_mask(flow_hw2, tau=1.0, stride=4, mask_hw=None, keep_ratio=0.2, min_keep=0.05):
    """:261-327 for one sample -> (mask, thr, fit dict)."""
    p1, p2 = flow_to_pairs(flow_hw2, stride, mask_hw)
    fit = ransac(p1, p2, 2000, 0.5, 0)
    if not fit["ok"]:
        return np.ones(flow_hw2.shape[:2], bool), None, fit
    m, thr = threshold_mask(distance_map(flow_hw2, fit["F"]), tau, keep_ratio, min_keep)
    return m, thr, fit


def soft_loss(flow_b2hw, F32, valid=None, robust="huber", delta=1.0, weight=0.1, ok=None):
    """:331-382 in float64 from float32 flow, float32 endpoints and the float32-rounded F (per sample [B,3,3] or shared [3,3]) -> (loss, grad [B,2,H,W]).
    ok [B] (or None): samples with ok False select nothing."""
    f = np.asarray(flow_b2hw, np.float64)
    B, _, H, W = f.shape
    Fs = np.asarray(F32, np.float64)
    Fs = np.broadcast_to(Fs, (B, 3, 3)) if Fs.ndim == 2 else Fs
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    sel = np.ones((B, H, W), bool) if valid is None else (np.asarray(valid, np.float64).reshape(B, H, W) > 0.5)
    if ok is not None:
        sel &= np.asarray(ok, bool).reshape(-1, 1, 1)
    tot, dsum, parts = 0.0, [], []
    for b in range(B):
        Fm = Fs[b]
        # (xs + flow).float(): the endpoint is a float32 sum in the reference, also in a float64 run (:360-361)
        u2 = (xs.astype(np.float32) + f[b, 0].astype(np.float32)).astype(np.float64)
        v2 = (ys.astype(np.float32) + f[b, 1].astype(np.float32)).astype(np.float64)
        a = Fm[0, 0] * xs + Fm[0, 1] * ys + Fm[0, 2]
        bb = Fm[1, 0] * xs + Fm[1, 1] * ys + Fm[1, 2]
        c = Fm[2, 0] * xs + Fm[2, 1] * ys + Fm[2, 2]
        t0 = Fm[0, 0] * u2 + Fm[1, 0] * v2 + Fm[2, 0]
        t1 = Fm[0, 1] * u2 + Fm[1, 1] * v2 + Fm[2, 1]
        n = u2 * a + v2 * bb + c
        den = a * a + bb * bb + t0 * t0 + t1 * t1 + 1e-12
        d = n * n / den
        gx = 2 * n * a / den - n * n / den ** 2 * (2 * t0 * Fm[0, 0] + 2 * t1 * Fm[0, 1])
        gy = 2 * n * bb / den - n * n / den ** 2 * (2 * t0 * Fm[1, 0] + 2 * t1 * Fm[1, 1])
        parts.append((d, gx, gy))
    cnt = int(sel.sum())
    grad = np.zeros((B, 2, H, W))
    if cnt == 0:
        return 0.0, grad
    for b, (d, gx, gy) in enumerate(parts):
        r = np.sqrt(d + 1e-12)
        if robust == "huber":
            val, dl = np.where(r <= delta, 0.5 * r ** 2 / delta, r - 0.5 * delta), np.where(r <= delta, 0.5 / delta, 0.5 / r)
        elif robust == "l1":
            val, dl = r, 0.5 / r
        else:
            val, dl = d, np.ones_like(d)
        s = sel[b]
        tot += val[s].sum()
        grad[b, 0][s] = (weight / cnt * dl * gx)[s]
        grad[b, 1][s] = (weight / cnt * dl * gy)[s]
    return weight * tot / cnt, grad


# ---------------------------------------------------------------- seeded test flows (shared by the generator and the tests)
def rigid_flow(H, W, seed, outlier=True, noise=0.05):
    """Rigid-scene flow [2,H,W] float32: random smooth inverse depth, small rotation + translation of a pinhole camera, a
    moving-object block that violates the epipolar geometry, and Gaussian noise."""
    g = np.random.default_rng(seed)
    f = 0.9 * W
    cx, cy = W / 2.0, H / 2.0
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    inv = np.full((H, W), 0.2)
    for _ in range(4):
        kx, ky, ph = g.uniform(0.5, 3) * 2 * np.pi / W, g.uniform(0.5, 3) * 2 * np.pi / H, g.uniform(0, 2 * np.pi)
        inv += g.uniform(0.02, 0.08) * (1 + np.sin(kx * xs + ky * ys + ph))
    wx, wy, wz = g.uniform(-0.01, 0.01, 3)
    R = np.array([[1, -wz, wy], [wz, 1, -wx], [-wy, wx, 1]])
    t = np.array([g.uniform(-0.3, 0.3), g.uniform(-0.2, 0.2), g.uniform(0.2, 0.5)])
    X = np.stack([(xs - cx) / f, (ys - cy) / f, np.ones_like(xs)], 0) / inv
    Y = np.tensordot(R, X, 1) + t.reshape(3, 1, 1)
    u2, v2 = f * Y[0] / Y[2] + cx, f * Y[1] / Y[2] + cy
    fl = np.stack([u2 - xs, v2 - ys], 0)
    if outlier:
        h0, w0 = int(g.integers(0, H // 2)), int(g.integers(0, W // 2))
        fl[0, h0:h0 + H // 4, w0:w0 + W // 4] += g.uniform(3, 6)
        fl[1, h0:h0 + H // 4, w0:w0 + W // 4] -= g.uniform(2, 4)
    fl += noise * g.standard_normal(fl.shape)
    return fl.astype(np.float32)
