"""Shared by the distance-MMD tests (not a test module): a NumPy mirror of the definition in moleculesde_amd/conformer_mmd.py,
the case builders and the tolerance.

The mirror is the oracle: the definition written out densely ([C, C] matrices of every subset) in one dtype.  In fp64 it is
the reference; the SAME code in fp32 gives the error a single-precision evaluation of the definition makes on these inputs,
and the device tests allow 8 x the largest |fp32 mirror - fp64 mirror| of each statistic over the whole case set (the project's
usual margin over an fp32 CPU evaluation's own error; suite-wide because single cases come out as low as 1e-8)."""
import numpy as np

MARGIN = 8.0
STATS = ("single_median", "single_mean", "pair_median", "pair_mean", "all")


# ---- the mirror ---------------------------------------------------------------------------------------------------------------
def distance_table(pos, atom_pairs, dtype=np.float64):
    """z [C, E] = |pos[:, u] - pos[:, v]| for pos [C, n, 3] and molecule-local atom pairs [E, 2], everything in `dtype`."""
    p = np.asarray(pos).astype(dtype)
    d = p[:, atom_pairs[:, 0]] - p[:, atom_pairs[:, 1]]
    return np.sqrt((d * d).sum(-1, dtype=dtype)).astype(dtype)


def squared_distances(z, cols):
    """L [C, C] = sum over the columns `cols` of (z[a, e] - z[b, e])^2."""
    zs = z[:, list(cols)]
    d = zs[:, None, :] - zs[None, :, :]
    return (d * d).sum(-1, dtype=z.dtype)


def bandwidth(z, cols):
    """sigma^2 = sum_{a, b} L_ab / (C^2 - C)."""
    C = z.shape[0]
    return squared_distances(z, cols).sum(dtype=z.dtype) / z.dtype.type(C * C - C)


def mmd(z, R, cols, kernel_mul=2.0, kernel_num=5):
    """MMD(S) of the samples z [C, E] (the first R the references) over the columns S = cols, in z's dtype."""
    t = z.dtype.type
    L = squared_distances(z, cols)
    s2 = bandwidth(z, cols)
    if s2 == 0:
        return t(0)
    k = np.zeros_like(L)
    for i in range(kernel_num):
        k = k + np.exp(-L / (s2 * t(kernel_mul) ** t(i - kernel_num // 2)))
    return k[:R, :R].mean(dtype=z.dtype) + k[R:, R:].mean(dtype=z.dtype) - t(2) * k[:R, R:].mean(dtype=z.dtype)


def molecule_statistics(ref, gen, atom_pairs, keep=None, kernel_mul=2.0, kernel_num=5, dtype=np.float64):
    """The definition for one molecule: ref [R, n, 3], gen [K, n, 3] fp32, atom_pairs [E, 2] molecule-local ATOM indices, keep
    bool [n] = the evaluated atoms (None: all).  Returns {"single" [E], "pair" [E (E - 1) / 2], "stats" [7], "finite" [R + K]}."""
    ref, gen = np.asarray(ref), np.asarray(gen)
    atoms = slice(None) if keep is None else np.flatnonzero(keep)
    fr = np.isfinite(ref[:, atoms]).all(axis=(1, 2))
    fg = np.isfinite(gen[:, atoms]).all(axis=(1, 2))
    R, K, E = int(fr.sum()), int(fg.sum()), int(atom_pairs.shape[0])
    nan = float("nan")
    out = {"finite": np.concatenate([fr, fg]).astype(np.uint8), "single": np.full(E, nan), "pair": np.full(E * (E - 1) // 2, nan)}
    stats = [nan] * 5 + [float(R), float(K)]
    if R and K and E:
        z = distance_table(np.concatenate([ref[fr], gen[fg]]), atom_pairs, dtype)
        out["single"] = np.array([mmd(z, R, [e], kernel_mul, kernel_num) for e in range(E)], dtype=np.float64)
        out["pair"] = np.array([mmd(z, R, [e, f], kernel_mul, kernel_num) for e in range(E) for f in range(e + 1, E)],
                               dtype=np.float64)
        stats[0], stats[1] = float(np.median(out["single"])), float(out["single"].mean())
        if E >= 2:
            stats[2], stats[3] = float(np.median(out["pair"])), float(out["pair"].mean())
        stats[4] = float(mmd(z, R, range(E), kernel_mul, kernel_num))
    out["stats"] = np.array(stats, dtype=np.float64)
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------
def chain_pairs(n, max_hops):
    """Atom pairs u < v of an n-atom chain at most max_hops bonds apart, ordered by (u, v)."""
    return np.array([(u, v) for u in range(n) for v in range(u + 1, min(n, u + max_hops + 1))], dtype=np.int32).reshape(-1, 2)


def all_pairs(n):
    return np.array([(u, v) for u in range(n) for v in range(u + 1, n)], dtype=np.int32).reshape(-1, 2)


def make_conformers(rng, n, R, K, ref_noise=0.12, gen_noise=0.3):
    """ref [R, n, 3], gen [K, n, 3] fp32: a chain of about 1.5 A steps, the references perturbed by ref_noise, the generated
    conformers by gen_noise per coordinate (another distribution of every distance: MMD well above 0)."""
    base = np.cumsum(rng.normal(size=(n, 3)) * 0.9, axis=0)
    ref = base[None] + ref_noise * rng.normal(size=(R, n, 3))
    gen = base[None] + gen_noise * rng.normal(size=(K, n, 3))
    return ref.astype(np.float32), gen.astype(np.float32)


# name: (R, K, atoms, evaluated atoms (None: all), pairs in the evaluated-atom numbering)
def suite():
    """The parity cases: (R, K) = (1, 1), (3, 4), (5, 70): C just past one wavefront, (64, 64): a multiple of it, (2, 130);
    E = 1 (no Pair item), 2, 7 (21 Pair items), 21 and one all-pairs case; one case evaluated on a subset of its atoms; and
    R + K = 1024, the most the kernels stage (conformer_mmd.MAX_POOLED)."""
    rng = np.random.default_rng(77)
    keep8 = np.array([1, 0, 1, 1, 0, 1, 0, 1], dtype=bool)                 # 5 evaluated atoms of 8
    spec = [("r1k1_e1", 1, 1, 3, None, np.array([[0, 2]], dtype=np.int32)),
            ("r3k4_e2", 3, 4, 4, None, np.array([[0, 1], [1, 3]], dtype=np.int32)),
            ("r5k70_e7", 5, 70, 6, None, chain_pairs(6, 3)[:7]),
            ("r64k64_allpairs", 64, 64, 5, None, all_pairs(5)),
            ("r2k130_e21", 2, 130, 9, None, chain_pairs(9, 3)),
            ("r3k4_masked_e7", 3, 4, 8, keep8, chain_pairs(5, 2)),
            ("r24k1000_e2_limit", 24, 1000, 3, None, np.array([[0, 1], [0, 2]], dtype=np.int32))]
    cases = {}
    for name, R, K, n, keep, pairs in spec:
        ref, gen = make_conformers(rng, n, R, K)
        cases[name] = {"ref": ref, "gen": gen, "keep": keep, "pairs": pairs}
    return cases


def atom_pairs_of(case):
    """The case's pairs as molecule-local atom indices."""
    keep = case["keep"]
    return case["pairs"] if keep is None else np.flatnonzero(keep)[case["pairs"]].astype(np.int32)


_CACHE = {}


def suite_reference():
    """{name: (case, fp64 mirror, fp32 mirror)}, computed once per process."""
    if "suite" not in _CACHE:
        _CACHE["suite"] = {name: (c, molecule_statistics(c["ref"], c["gen"], atom_pairs_of(c), c["keep"], dtype=np.float64),
                                  molecule_statistics(c["ref"], c["gen"], atom_pairs_of(c), c["keep"], dtype=np.float32))
                           for name, c in suite().items()}
    return _CACHE["suite"]


def tolerances():
    """Per statistic (and for the Single and Pair items themselves) MARGIN x the largest |fp32 mirror - fp64 mirror| over the
    suite, and those largest differences."""
    err = {k: 0.0 for k in STATS + ("single_items", "pair_items")}
    for _, want, f32 in suite_reference().values():
        for i, k in enumerate(STATS):
            d = abs(f32["stats"][i] - want["stats"][i])
            if np.isfinite(d):
                err[k] = max(err[k], float(d))
        for k in ("single", "pair"):
            if want[k].size:
                err[k + "_items"] = max(err[k + "_items"], float(np.abs(f32[k] - want[k]).max()))
    return {k: MARGIN * v for k, v in err.items()}, err


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q
