"""Shared by the conformer-evaluation tests (not a test module): the fp64 reference of the aligned RMSD, a NumPy mirror of
the kernel's formula, the case builders and the COV / MAT reference.

Reference: SVD-Kabsch with the determinant correction; the RMSD is formed from the rotated residual itself, a sum of squares
with no cancellation near zero.  Mirror: what csrc/conformer_rmsd.hip computes (centroids, cross-covariance, Horn's 4 x 4
matrix, its largest eigenvalue, sqrt(max(0, (G_x + G_y - 2 lambda) / n))) in fp64 with LAPACK's eigvalsh.  |mirror - reference|
over the cases is the error of the FORMULA at fp64; the device tests allow 8 x its worst value (the project's usual margin over
a formula's own error; it also covers an eigen-solver and a summation order that differ from LAPACK's and NumPy's)."""
import numpy as np

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 129, 200)
KINDS = ("random", "rigid", "mirror", "noisy", "planar", "collinear", "rigid_shift100")
R_CASE, K_CASE = 3, 4
MARGIN = 8.0


# ---- reference and mirror ---------------------------------------------------------------------------------------------------
def kabsch_rmsd(x, y):
    """min over proper rotations Q and translations of sqrt(mean_a |Q (x_a - c_x) - (y_a - c_y)|^2), fp64, residual formed."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return float("nan")
    xc, yc = x - x.mean(0), y - y.mean(0)
    U, _, Vt = np.linalg.svd(xc.T @ yc)
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    Q = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    res = xc @ Q.T - yc
    return float(np.sqrt((res * res).sum() / x.shape[0]))


def horn_matrix(S):
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])


def mirror_rmsd(x, y):
    """The kernel's formula in NumPy fp64."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    xc, yc = x - x.mean(0), y - y.mean(0)
    lam = np.linalg.eigvalsh(horn_matrix(xc.T @ yc))[-1]
    return float(np.sqrt(max(0.0, ((xc * xc).sum() + (yc * yc).sum() - 2.0 * lam) / x.shape[0])))


def rmsd_block(ref, gen, fn=kabsch_rmsd, keep=None):
    """[R, K] of fn over ref [R, n, 3] x gen [K, n, 3], on the atoms `keep` (bool [n]) when given."""
    if keep is not None:
        ref, gen = ref[:, keep], gen[:, keep]
    return np.array([[fn(x, y) for y in gen] for x in ref], dtype=np.float64)


# ---- cases ------------------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _rigid(rng, x):
    t = rng.normal(size=3)
    return x @ random_rotation(rng).T + 5.0 * t / np.linalg.norm(t)


def make_case(kind, n, seed=0):
    """(ref [3, n, 3], gen [4, n, 3]) fp32, coordinate scale about 2 A.  Generated conformer k is built from reference k % 3, so
    entry [k % 3, k] is the case proper and the others are unrelated pairs of the same family."""
    rng = np.random.default_rng([seed, KINDS.index(kind), n])
    if kind == "planar":
        ref = rng.normal(size=(R_CASE, n, 3)) * 2.0
        ref[:, :, 2] = 0.0
    elif kind == "collinear":
        ref = np.stack([np.outer(1.5 * np.arange(n), random_rotation(rng)[0]) + rng.normal(size=3) for _ in range(R_CASE)])
    else:
        ref = rng.normal(size=(R_CASE, n, 3)) * 2.0
    gen = []
    for k in range(K_CASE):
        x = ref[k % R_CASE]
        if kind == "random":
            y = rng.normal(size=(n, 3)) * 2.0
        elif kind in ("rigid", "rigid_shift100", "collinear"):
            y = _rigid(rng, x)
        elif kind == "mirror":
            y = x * np.array([1.0, 1.0, -1.0])
        elif kind == "noisy":
            y = x @ random_rotation(rng).T + 0.3 * rng.normal(size=(n, 3))
        elif kind == "planar":
            y = _rigid(rng, x + 0.01 * rng.normal(size=(n, 3)))
        else:
            raise ValueError(kind)
        gen.append(y)
    gen = np.stack(gen)
    if kind == "rigid_shift100":
        ref, gen = ref + 100.0, gen + 100.0
    return ref.astype(np.float32), gen.astype(np.float32)


def all_cases(seed=0):
    return [(kind, n) + make_case(kind, n, seed) for kind in KINDS for n in SIZES]


_CACHE = {}


def case_references(seed=0):
    """{(kind, n): (ref, gen, reference [3, 4], mirror [3, 4])}, computed once per process."""
    if seed not in _CACHE:
        _CACHE[seed] = {(kind, n): (ref, gen, rmsd_block(ref, gen), rmsd_block(ref, gen, mirror_rmsd))
                        for kind, n, ref, gen in all_cases(seed)}
    return _CACHE[seed]


def formula_error(seed=0):
    """Worst |mirror - reference| over the cases, and the same per case kind."""
    per = {k: 0.0 for k in KINDS}
    for (kind, _), (_, _, want, mir) in case_references(seed).items():
        per[kind] = max(per[kind], float(np.abs(mir - want).max()))
    return max(per.values()), per


# ---- COV / MAT --------------------------------------------------------------------------------------------------------------
def cov_mat_reference(M, thresholds):
    """COV-R, MAT-R, COV-P, MAT-P and the finite generated conformers of one [R, K] matrix; NaN entries count as +inf."""
    M = np.asarray(M, dtype=np.float64)
    R, K = M.shape
    Minf = np.where(np.isnan(M), np.inf, M)
    rowmin, colmin = Minf.min(axis=1), Minf.min(axis=0)
    fin = np.isfinite(colmin)
    nfin = int(fin.sum())
    return {"cov_r": [float((rowmin <= d).sum()) / R for d in thresholds],
            "cov_p": [float((colmin <= d).sum()) / K for d in thresholds],
            "mat_r": float(rowmin.mean()) if nfin else float("nan"),
            "mat_p": float(colmin[fin].mean()) if nfin else float("nan"),
            "num_finite": nfin, "rowmin": rowmin, "colmin": colmin}


def summary_reference(mats, thresholds):
    """The dictionary evaluate_conformers returns, from per-molecule reference matrices."""
    per = [cov_mat_reference(M, thresholds) for M in mats]
    ok = [p for p in per if p["num_finite"] > 0]
    res = {"num_molecules": len(per), "num_failed": len(per) - len(ok),
           "per_molecule": {k: [p[k] for p in per] for k in ("cov_r", "mat_r", "cov_p", "mat_p", "num_finite")}}
    for name, f in (("mean", np.mean), ("median", np.median)):
        res[name] = {"cov_r": f(np.array([p["cov_r"] for p in ok]), axis=0).tolist(), "mat_r": float(f([p["mat_r"] for p in ok])),
                     "cov_p": f(np.array([p["cov_p"] for p in ok]), axis=0).tolist(), "mat_p": float(f([p["mat_p"] for p in ok]))}
    return res


def min_gap_to_thresholds(mats, thresholds):
    """Smallest |row or column minimum - threshold| over the finite minima of the matrices."""
    gap = np.inf
    for M in mats:
        p = cov_mat_reference(M, thresholds)
        v = np.concatenate([p["rowmin"], p["colmin"]])
        v = v[np.isfinite(v)]
        for d in thresholds:
            if v.size:
                gap = min(gap, float(np.abs(v - d).min()))
    return gap
