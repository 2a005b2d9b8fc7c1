"""NumPy float64 restatement of the flow-comparison report (csrc/pwc_flow_compare.hip; the reference's compare_flows and
print_flow_stats, onnx_pth_compare.py:133-201, :225-230), the tolerances the device has to meet against it, and the seeded input
recipe of the g18 fixture.

What is float32 and what is float64 follows the kernel's contract: the difference d = a - b and the per-pixel endpoint error
epe = sqrt(fl32(du*du) + fl32(dv*dv)) are formed in float32 (this reproduces the reference's float32 np.linalg.norm bit for bit, so
maxima, threshold counts and agreement percentages are exact); every sum is taken in float64 over the widened float32 values;
Pearson and the standard deviations are two-pass (mean-centred) in float64.  Pearson is NaN and a standard deviation exactly 0 when
the field's min == max; Pearson is clipped to [-1, 1] as np.corrcoef clips it.

Tolerances (derived, not tuned; N = scalars in the row, u = 2**-53):
  exact          Max abs diff, EPE max, min / max, every count, every agreement percentage, the EPE map
  relative 4Nu   L2 diff, MAE, Relative L2 diff, Relative MAE, EPE mean -- sums of non-negative terms: any order of N fp64 additions is
                 within (N-1)u relative, the factor 4 covers the square root and the divisions
  absolute 4Nu   Cosine similarity, because |S ab| <= ||a|| ||b||
  absolute 16Nu kappa            Pearson corr, kappa = sqrt(S a^2 S b^2) / (N sigma_a sigma_b) from this oracle
  absolute 16Nu kappa S|f|/N     mean and std of field f (the one-pass variance loses rms_f / sigma_f <= kappa); where Pearson is NaN
                 kappa is not defined and the field's own rms_f / sigma_f stands in (1 for a flat field, whose std must be exactly 0)

The inputs use only additions, multiplications, divisions and square roots of np.random.default_rng uniforms, so the recipe gives the
same bytes on every machine (no libm call); the fixture stores seeds, digests and results, not the fields.
"""
import hashlib

import numpy as np

U = 2.0 ** -53
REF_TAUS = (0.25, 0.5, 1.0, 2.0)
TILE_H, TILE_W, FINISH_LANES = 32, 128, 256
NONNEG = ("L2 diff", "MAE", "Relative L2 diff", "Relative MAE", "EPE mean")
EXACT = ("Max abs diff", "EPE max")
STAT_KEYS = ("min", "max", "mean", "std")

# name: n, H, W, kind, seed, taus, layout (GPU placement: extra elements in the batch stride of a and of b, element offset of the
# base pointers from a 16-byte boundary)
#   kind "smooth": smooth field + bounded error vectors; "equal": b = a; "a_zero"; "b_const"; "ties": axis-aligned differences of
#   exactly 0.25 / 0.5 / 1 / 2 / 3 px on quarter-pixel fields, so the inclusive <= decides the counts
CASES = {
    "one": dict(n=1, H=1, W=1, kind="smooth", seed=1800),
    "tiny": dict(n=1, H=3, W=5, kind="smooth", seed=1801),
    "tile": dict(n=2, H=TILE_H, W=TILE_W, kind="smooth", seed=1802),
    "tile_p1": dict(n=3, H=TILE_H + 1, W=TILE_W + 1, kind="smooth", seed=1803),
    "ref": dict(n=1, H=96, W=128, kind="smooth", seed=1804),                             # the reference's own 384 x 512 run
    "strided": dict(n=2, H=33, W=200, kind="smooth", seed=1805, pad=(40, 8)),            # 16-byte loads, unequal batch strides
    "strided_odd": dict(n=2, H=33, W=200, kind="smooth", seed=1806, pad=(7, 3)),         # strides that force the guarded loads
    "many_tiles": dict(n=1, H=32 * 271 + 1, W=4, kind="smooth", seed=1807),              # 272 tiles > the finish workgroup's 256 lanes
    "w_odd": dict(n=2, H=19, W=67, kind="smooth", seed=1808),                            # W % 4 != 0
    "misaligned": dict(n=1, H=40, W=136, kind="smooth", seed=1809, offset=1),             # 4-byte but not 16-byte aligned base
    "equal": dict(n=1, H=20, W=72, kind="equal", seed=1810),
    "a_zero": dict(n=1, H=20, W=72, kind="a_zero", seed=1811),
    "b_const": dict(n=2, H=20, W=72, kind="b_const", seed=1812),
    "ties": dict(n=1, H=20, W=72, kind="ties", seed=1813),
    "tau1": dict(n=1, H=17, W=65, kind="smooth", seed=1814, taus=(0.75,)),
    "tau8": dict(n=1, H=17, W=65, kind="smooth", seed=1815, taus=(0.1, 0.2, 0.3, 0.6, 0.9, 1.3, 1.7, 3.0)),
}
# an "ordinary" case: the smooth recipe with enough pixels for a percentage strictly between 5 and 95 to exist
ORDINARY = tuple(k for k, c in CASES.items() if c["kind"] == "smooth" and c["n"] * c["H"] * c["W"] >= 15)


def case_taus(name):
    return tuple(CASES[name].get("taus", REF_TAUS))


def make_inputs(name):
    """(a, b) float32 [n,2,H,W] of a case, from its seed."""
    c = CASES[name]
    n, H, W, kind = c["n"], c["H"], c["W"], c["kind"]
    g = np.random.default_rng(c["seed"])
    yy, xx = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    a = np.empty((n, 2, H, W), np.float64)
    for s in range(n):
        p = g.uniform(-1.0, 1.0, 4)
        a[s, 0] = 6.0 * (4.0 * xx * (1.0 - xx) - 0.5 + 0.6 * yy * p[0]) + p[1]
        a[s, 1] = 4.0 * (yy * yy - 0.7 * xx * p[2]) + p[3]
    a += g.uniform(-0.05, 0.05, a.shape)
    e = g.uniform(-1.0, 1.0, a.shape) * (1.9 * g.uniform(0.0, 1.0, (n, 1, H, W)))        # error vectors of length 0 .. 2.7 px
    if kind == "smooth":
        b = a - e
    elif kind == "equal":
        b = a
    elif kind == "a_zero":
        a = np.zeros_like(a)
        b = a - e
    elif kind == "b_const":
        b = np.full_like(a, 0.75)
    elif kind == "ties":
        a = np.round(a * 4.0) / 4.0
        mag = np.array([0.25, 0.5, 1.0, 2.0, 3.0])[g.integers(0, 5, (n, H, W))] * np.where(g.integers(0, 2, (n, H, W)) == 1, 1.0, -1.0)
        axis = g.integers(0, 2, (n, H, W))
        d = np.stack([np.where(axis == 0, mag, 0.0), np.where(axis == 1, mag, 0.0)], axis=1)
        b = a - d
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def digest(a, b):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes() + np.ascontiguousarray(b).tobytes()).hexdigest()


def epe_map(a, b):
    """float32 [n,H,W]: the per-pixel endpoint error exactly as the kernel and the reference form it."""
    d = a.astype(np.float32) - b.astype(np.float32)
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def _stats(f64, f32):
    n = f64.size
    lo, hi = f32.min(), f32.max()
    mean = f64.sum() / n
    c = f64 - mean
    ss = (c * c).sum()
    return {"min": lo, "max": hi, "mean": mean, "std": 0.0 if lo == hi else np.sqrt(ss / n)}, ss


def report(a, b, taus=REF_TAUS):
    """One row of the report for a, b float32 [k,2,H,W]: the k samples count as one field (the samples stacked along H).  Returns the
    reference's keys, "stats", and under "_" what the tolerances need."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    d = a - b
    e = epe_map(a, b)
    A, B, D, E = a.astype(np.float64).ravel(), b.astype(np.float64).ravel(), d.astype(np.float64).ravel(), e.astype(np.float64).ravel()
    N, P = A.size, E.size
    sd2, sabsd, sa2, sb2, sabsa, sabsb, sab = (D * D).sum(), np.abs(D).sum(), (A * A).sum(), (B * B).sum(), np.abs(A).sum(), np.abs(B).sum(), (A * B).sum()
    l2, mae = np.sqrt(sd2), sabsd / N
    st_a, ssa = _stats(A, a)
    st_b, ssb = _stats(B, b)
    flat = st_a["min"] == st_a["max"] or st_b["min"] == st_b["max"]
    with np.errstate(all="ignore"):
        if flat:
            pearson, kappa = np.nan, np.nan
        else:
            ca, cb = A - st_a["mean"], B - st_b["mean"]
            pearson = float(np.clip((ca * cb).sum() / np.sqrt(ssa * ssb), -1.0, 1.0))
            kappa = float(np.sqrt(sa2 * sb2) / np.sqrt(ssa * ssb))
    counts = [int(np.count_nonzero(e <= np.float32(t))) for t in taus]
    kap = {}
    for key, s2, ss in (("a", sa2, ssa), ("b", sb2, ssb)):
        kap[key] = kappa if not flat else (float(np.sqrt(s2 / ss)) if ss > 0 else 1.0)
    return {
        "L2 diff": l2,
        "MAE": mae,
        "Max abs diff": np.abs(d).max(),
        "Relative L2 diff": l2 / (np.sqrt(sa2) + 1e-8),
        "Relative MAE": mae / (sabsa / N + 1e-8),
        "Pearson corr": pearson,
        "Cosine similarity": sab / (np.sqrt(sa2) * np.sqrt(sb2) + 1e-8),
        "EPE mean": E.sum() / P,
        "EPE max": e.max(),
        "agreements": {"agree@%s" % (float(t),): float(c) / float(P) * 100.0 for t, c in zip(taus, counts)},
        "stats": {"a": st_a, "b": st_b},
        "_": {"N": N, "P": P, "kappa": kappa, "kappa_stats": kap, "counts": counts, "mean_abs": {"a": sabsa / N, "b": sabsb / N},
              "nearest_tau": float(np.min(np.abs(np.sqrt(D.reshape(d.shape)[:, 0] ** 2 + D.reshape(d.shape)[:, 1] ** 2)[..., None]
                                                 - np.asarray(taus, np.float64))))},
    }


def rows(a, b, taus=REF_TAUS):
    """The n + 1 rows of the device record: every sample, then the batch (the samples stacked along H)."""
    n = a.shape[0]
    return [report(a[s:s + 1], b[s:s + 1], taus) for s in range(n)] + [report(a, b, taus)]


def tolerances(row):
    """{key: ("exact" | "rel" | "abs", bound)} for one oracle row; stats under ("stats", field, key)."""
    N, x = row["_"]["N"], row["_"]
    tol = {k: ("exact", 0.0) for k in EXACT}
    tol.update({k: ("rel", 4.0 * N * U) for k in NONNEG})
    tol["Cosine similarity"] = ("abs", 4.0 * N * U)
    tol["Pearson corr"] = ("abs", 16.0 * N * U * x["kappa"]) if np.isfinite(x["kappa"]) else ("nan", 0.0)
    for f in ("a", "b"):
        tol[("stats", f, "min")] = tol[("stats", f, "max")] = ("exact", 0.0)
        bound = 16.0 * N * U * x["kappa_stats"][f] * x["mean_abs"][f]
        tol[("stats", f, "mean")] = ("abs", bound)
        tol[("stats", f, "std")] = ("exact", 0.0) if row["stats"][f]["min"] == row["stats"][f]["max"] else ("abs", bound)
    return tol


def check_row(got, want, where=""):
    """Assert one device (or restated) row against an oracle row; returns {key: deviation in units of its bound (0 for exact)}."""
    tol, used = tolerances(want), {}

    def one(key, g, w):
        kind, bound = tol[key]
        g, w = float(g), float(w)
        if kind == "nan" or np.isnan(w):
            assert np.isnan(g) and np.isnan(w), (where, key, g, w)
            used[key] = 0.0
        elif kind == "exact":
            assert g == w, (where, key, g, w)
            used[key] = 0.0
        else:
            err = abs(g - w) / (abs(w) if kind == "rel" and w != 0.0 else 1.0)
            assert err <= bound, (where, key, g, w, err, bound)
            used[key] = err / bound if bound > 0 else 0.0

    for key in EXACT + NONNEG + ("Cosine similarity", "Pearson corr"):
        one(key, got[key], want[key])
    assert list(got["agreements"]) == list(want["agreements"]), (where, list(got["agreements"]), list(want["agreements"]))
    for k, w in want["agreements"].items():
        assert float(got["agreements"][k]) == w, (where, k, got["agreements"][k], w)
    for f in ("a", "b"):
        for k in STAT_KEYS:
            one(("stats", f, k), got["stats"][f][k], want["stats"][f][k])
    return used
