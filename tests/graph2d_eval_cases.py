"""NumPy mirror of csrc/graph2d_eval.hip (msde_graph2d_decode, msde_graph2d_summary) and the case builders of
tests/test_graph2d_eval_host.py and tests/test_gpu_graph2d_eval.py.

The mirror uses the kernel's fp64 formulas -- v = 0.5 ((double)a_ij + (double)a_ji), q = clamp(floor(v + 0.5), 0, max_bond),
ratios and means as quotients of the same integers summed in the same order -- so every integer output and every ratio is
compared EXACTLY; only sum |v - t| is a long fp64 sum, taken here with math.fsum (correctly rounded) and compared within the
summation bound.  The connected components come from another algorithm than the kernel's label propagation (boolean closure
of the adjacency matrix by repeated squaring).

A molecule of a launch is a tuple (x [K, n, ncls] fp32, adj [K, n, n] fp32, z [n] int, tgt [n, n] uint8, flag [n] uint8)."""
import math

import numpy as np

HALF_BONDS = np.array([0, 2, 4, 6, 3, 2])           # half-bond units of codes 0..5: none, single, double, triple, aromatic, misc
SIZES = (2, 3, 31, 32, 33, 63, 64, 65, 100)
CLASSES = (1, 5, 64, 65, 119, 130)
SAMPLES = (1, 2, 10, 65)


def tri(n):
    """Row-major upper-triangle indices: the order of the signature's codes."""
    return np.triu_indices(n, 1)


def quantise(adj, max_bond):
    """(v, q) [n, n] of one sample: fp64 symmetrised value and the clamped code (NaN -> 0)."""
    a = adj.astype(np.float64)
    with np.errstate(invalid="ignore"):                  # inf - inf on a pair that makes the sample non-finite anyway
        v = 0.5 * (a + a.T)
        f = np.floor(v + 0.5)
        q = np.where(f >= 1.0, np.minimum(f, float(max_bond)), 0.0)
    return v, np.nan_to_num(q, nan=0.0).astype(np.int64)


def components(bonded, flag):
    """Connected components of the graph `bonded` [n, n] bool on the atoms with flag != 0: closure by repeated squaring."""
    n = bonded.shape[0]
    keep = flag != 0
    R = (bonded & keep[:, None] & keep[None, :]) | np.eye(n, dtype=bool)
    for _ in range(max(1, int(np.ceil(np.log2(max(n, 2)))))):
        R = (R.astype(np.float32) @ R.astype(np.float32)) > 0
    root = R.argmax(1)                                   # the lowest index an atom reaches
    return int((keep & (root == np.arange(n))).sum())


def decode_sample(x, adj, z, tgt, flag, max_bond=4, max_valence2=None):
    """One sample: (sig uint8 [n + n (n - 1) / 2], counts [9] int64, adj_l1 float, sum of the |v - t| terms' magnitudes)."""
    n = x.shape[0]
    keep = flag != 0
    pair = keep[:, None] & keep[None, :] & ~np.eye(n, dtype=bool)
    iu, ju = tri(n)
    up = pair[iu, ju]
    t = tgt.astype(np.int64)[iu, ju][up]
    true_bonds = int((t > 0).sum())
    L = n + n * (n - 1) // 2
    if not (np.isfinite(x[keep]).all() and np.isfinite(adj[pair]).all()):
        return np.zeros(L, dtype=np.uint8), np.array([0, 0, 0, 0, true_bonds, 0, 0, 0, 0]), float("nan"), float("nan")
    cls = np.where(keep, x.argmax(1), 0)                 # numpy's argmax returns the first of equal maxima
    v, q = quantise(adj, max_bond)
    q = np.where(pair, q, 0)
    qu, vu = q[iu, ju][up], v[iu, ju][up]
    tp = int(((qu > 0) & (t > 0)).sum())
    fp = int(((qu > 0) & (t == 0)).sum())
    atoms = int((cls[keep] == z[keep]).sum())
    exact = int(atoms == int(keep.sum()) and bool((qu == t).all()))
    val2 = HALF_BONDS[q].sum(1)
    viol = 0
    if max_valence2 is not None:
        cap = np.asarray(max_valence2).astype(np.int64)[cls]
        viol = int((keep & (cap > 0) & (val2 > cap)).sum())
    terms = np.abs(vu - t)
    counts = np.array([1, atoms, tp, fp, true_bonds - tp, int(((t > 0) & (qu == t)).sum()), exact, components(q > 0, flag), viol])
    sig = np.concatenate([cls, q[iu, ju]]).astype(np.uint8)
    return sig, counts, math.fsum(terms), math.fsum(terms)


def summarise(sigs, counts, l1, flag):
    """One molecule: (stats [11] fp64, first [K] uint8) from its samples' signatures [K, L], counts [K, 9] and adj_l1 [K]."""
    K = len(sigs)
    nf = int((flag != 0).sum())
    pairs = nf * (nf - 1) // 2
    first = np.zeros(K, dtype=np.uint8)
    for k in range(K):
        if counts[k][0]:
            first[k] = not any(counts[e][0] and np.array_equal(sigs[e], sigs[k]) for e in range(k))
    acc = prec = rcl = f1 = ordr = ex = valid = tot = 0.0
    fin = anyx = 0
    for k in range(K):
        c = [int(v) for v in counts[k]]
        if not c[0]:
            continue
        tp, fp, fn = c[2], c[3], c[4]
        fin += 1
        acc += c[1] / nf
        prec += tp / (tp + fp) if tp + fp > 0 else 1.0
        rcl += tp / (tp + fn) if tp + fn > 0 else 1.0
        f1 += (2 * tp) / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else 1.0
        ordr += c[5] / tp if tp > 0 else 1.0
        ex += float(c[6])
        anyx |= c[6]
        valid += 1.0 if c[7] == 1 and c[8] == 0 else 0.0
        tot += float(l1[k])
    stats = [acc / K, prec / K, rcl / K, f1 / K, ordr / K, ex / K, valid / K, float(first.sum()) / K, float(anyx),
             tot / fin / max(pairs, 1) if fin else float("nan"), float(fin)]
    return np.array(stats, dtype=np.float64), first


def mirror_launch(mols, max_bond=4, max_valence2=None):
    """Every molecule of a launch: a list of dicts sig [K, L], counts [K, 9], l1 [K], l1_abs [K], stats [11], first [K]."""
    out = []
    for x, adj, z, tgt, flag in mols:
        rows = [decode_sample(x[k], adj[k], z, tgt, flag, max_bond, max_valence2) for k in range(x.shape[0])]
        sig, counts = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        l1, l1_abs = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
        stats, first = summarise(sig, counts, l1, flag)
        out.append(dict(sig=sig, counts=counts, l1=l1, l1_abs=l1_abs, stats=stats, first=first))
    return out


# ------------------------------------------------------------------------------------------------ builders
def random_graph(rng, n, ncls, bondless=0):
    """(z, tgt, flag): a random tree with a few ring closures and codes 1..4; the last `bondless` atoms lose every bond, which
    unflags them."""
    tgt = np.zeros((n, n), dtype=np.uint8)
    for i in range(1, n):
        p = int(rng.integers(max(0, i - 3), i))
        tgt[p, i] = tgt[i, p] = rng.integers(1, 5)
    for _ in range(n // 8):
        a, b = (int(v) for v in rng.integers(0, n, size=2))
        if a != b and tgt[a, b] == 0:
            tgt[a, b] = tgt[b, a] = rng.integers(1, 5)
    assert n - bondless >= 2
    for a in range(n - bondless, n):                     # the last atoms have no children in the tree: the rest stays connected
        tgt[a, :] = 0
        tgt[:, a] = 0
    return rng.integers(0, ncls, size=n), tgt, (tgt.sum(1) > 0).astype(np.uint8)


def target_scores(z, tgt, ncls, K=1):
    """The target graph written as the sampler's tensors: one-hot scores and the codes as floats."""
    x = np.zeros((K, len(z), ncls), dtype=np.float32)
    x[:, np.arange(len(z)), z] = 1.0
    return x, np.repeat(tgt.astype(np.float32)[None], K, axis=0)


def noisy_samples(rng, z, tgt, ncls, K, symmetric):
    """K samples around the target: scores one-hot + N(0, 0.3), adjacency codes + U(-0.45, 0.45) and, on about 2 / n of the
    entries, a further U(-1, 1) (symmetric or not), so that classes and codes go wrong in some places and stay right in most:
    some samples are exact, some lose a bond and fall apart, most gain a few."""
    x, adj = target_scores(z, tgt, ncls, K)
    n = len(z)
    x = x + 0.3 * rng.normal(size=x.shape).astype(np.float32)
    noise = rng.uniform(-0.45, 0.45, size=(K, n, n)) + (rng.random(size=(K, n, n)) < min(0.5, 2.0 / n)) * rng.uniform(-1, 1, size=(K, n, n))
    noise = noise.astype(np.float32)
    if symmetric:
        noise = np.triu(noise, 1)
        noise = noise + noise.transpose(0, 2, 1)
    return x.astype(np.float32), (adj + noise).astype(np.float32)


def ragged_case(ncls, seed):
    """Nine molecules, one of every size of SIZES, with K cycling through SAMPLES (the start of the cycle moves with ncls, so
    every K meets small and large molecules over the six launches); odd molecules asymmetric; two with bond-less atoms."""
    rng = np.random.default_rng(seed)
    mols = []
    for j, n in enumerate(SIZES):
        K = SAMPLES[(j + CLASSES.index(ncls)) % len(SAMPLES)]
        z, tgt, flag = random_graph(rng, n, ncls, bondless=2 if n in (33, 64) else 0)
        x, adj = noisy_samples(rng, z, tgt, ncls, K, symmetric=j % 2 == 0)
        mols.append((x, adj, z, tgt, flag))
    return mols


def ring(n, code=1):
    tgt = np.zeros((n, n), dtype=np.uint8)
    for i in range(n):
        tgt[i, (i + 1) % n] = tgt[(i + 1) % n, i] = code
    return tgt


def path(order, code=1):
    """A path through the atoms in the given order."""
    n = len(order)
    tgt = np.zeros((n, n), dtype=np.uint8)
    for a, b in zip(order[:-1], order[1:]):
        tgt[a, b] = tgt[b, a] = code
    return tgt


def below(v):
    """The fp32 number one ulp below v."""
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def quantisation_pairs(max_bond=4):
    """(a_ij, a_ji, expected code) at max_bond = 4: the boundaries c +- 0.5 and one fp32 ulp below them, negative values, values
    above max_bond, and asymmetric pairs whose fp64 mean sits on (or one fp64 step off) a boundary while neither element does."""
    rows = []
    for c in range(0, max_bond + 1):
        rows.append((c + 0.5, c + 0.5, min(c + 1, max_bond)))            # 0.5 -> 1: halves round up
        rows.append((below(c + 0.5), below(c + 0.5), c))
        if c > 0:
            rows.append((c - 0.5, c - 0.5, c))
            rows.append((below(c - 0.5), below(c - 0.5), c - 1))
    rows += [(-0.5, -0.5, 0), (-3.0, -3.0, 0), (-0.49, -0.49, 0), (below(0.0), below(0.0), 0),
             (max_bond + 2.0, max_bond + 2.0, max_bond), (1e30, 1e30, max_bond), (-1e30, -1e30, 0),
             (1.0, 2.0, 2), (2.0, 1.0, 2), (0.25, 0.75, 1), (0.0, 1.0, 1), (3.0, 4.0, 4), (1.25, 1.5, 1),
             # 0.5 and the fp32 number below it: the fp64 mean is 0.5 - 2^-26 -> 0; an fp32 sum would round to 1.0 -> mean 0.5 -> 1
             (0.5, below(0.5), 0), (below(0.5), 0.5, 0), (2.5, below(2.5), 2),
             (1e30, -1e30, 0), (7.0, -6.0, 1)]
    return [(np.float32(a), np.float32(b), int(q)) for a, b, q in rows]


def quantisation_case(ncls=5):
    """One molecule whose upper triangle carries quantisation_pairs() in row-major order (the rest of the pairs hold 0), every
    atom flagged; the target is a path with double bonds."""
    rows = quantisation_pairs()
    n = 2
    while n * (n - 1) // 2 < len(rows):
        n += 1
    iu, ju = tri(n)
    adj = np.zeros((1, n, n), dtype=np.float32)
    for (a, b, _), i, j in zip(rows, iu, ju):
        adj[0, i, j], adj[0, j, i] = a, b
    z = np.arange(n) % ncls
    tgt = path(list(range(n)), code=2)
    x, _ = target_scores(z, tgt, ncls, 1)
    want = np.zeros(len(iu), dtype=np.uint8)
    want[:len(rows)] = [q for _, _, q in rows]
    return (x, adj, z, tgt, np.ones(n, dtype=np.uint8)), want


def argmax_case():
    """130 classes, all scores negative (-5 .. -1), the maximum -0.5 placed per atom: at one class; at the first and the last
    class; at classes 63 and 64 (two lanes, the 64-lane boundary); at 5 and 69 (one lane, two strides); at 64 and 1; at 129
    alone; everywhere.  Returns the molecule and the expected classes."""
    ncls = 130
    places = [(17,), (0, 129), (63, 64), (5, 69), (64, 1), (129,), tuple(range(130)), (128, 127, 65)]
    want = [17, 0, 63, 5, 1, 129, 0, 65]
    n = len(places)
    rng = np.random.default_rng(1)
    x = rng.uniform(-5.0, -1.0, size=(1, n, ncls)).astype(np.float32)
    for i, p in enumerate(places):
        x[0, i, list(p)] = -0.5
    tgt = path(list(range(n)))
    z = np.array(want)
    return (x, tgt.astype(np.float32)[None].copy(), z, tgt, np.ones(n, dtype=np.uint8)), want


def component_case(n=100, seed=2, ncls=5):
    """One molecule, a path through n atoms in a shuffled order, and five samples: the path itself (1 component); the path along
    0, 1, 2, ... (labelled with its order), along n - 1, ..., 0 (against it); the shuffled path with one bond removed (2); the
    shuffled path with three atoms cut loose (isolated decoded atoms among flagged atoms)."""
    rng = np.random.default_rng(seed)
    order = [int(v) for v in rng.permutation(n)]
    tgt = path(order)
    z = rng.integers(0, ncls, size=n)
    x, _ = target_scores(z, tgt, ncls, 5)
    cut = tgt.copy()
    a, b = order[n // 2], order[n // 2 + 1]
    cut[a, b] = cut[b, a] = 0
    loose = tgt.copy()
    for a in (order[0], order[n // 3], order[n - 2]):        # an end (its neighbour stays bonded) and two inner atoms
        loose[a, :] = 0
        loose[:, a] = 0
    adj = np.stack([tgt, path(list(range(n))), path(list(range(n - 1, -1, -1))), cut, loose]).astype(np.float32)
    loose_parts = components(loose > 0, np.ones(n))
    return (x, adj, z, tgt, np.ones(n, dtype=np.uint8)), [1, 1, 1, 2, loose_parts]


def valence_case():
    """119 classes (class = atomic number - 1).  Samples of a 7-atom star around atom 0: a carbon with two aromatic bonds and a
    single one (8 half-bonds: at the cap of 4 bonds); with three aromatic bonds (9: one half-bond over); with five single bonds
    (10); an iron centre (unchecked) with six single bonds; a hydrogen centre with two.  The leaves are iron: unchecked."""
    ncls, n = 119, 7
    C, H, Fe = 5, 0, 25
    centre = [C, C, C, Fe, H]
    bonds = [[4, 4, 1], [4, 4, 4], [1, 1, 1, 1, 1], [1] * 6, [1, 1]]
    want = [0, 1, 1, 0, 1]
    tgt = np.zeros((n, n), dtype=np.uint8)
    tgt[0, 1:] = tgt[1:, 0] = 1
    z = np.array([C] + [Fe] * (n - 1))
    x = np.zeros((len(bonds), n, ncls), dtype=np.float32)
    adj = np.zeros((len(bonds), n, n), dtype=np.float32)
    for k, (c, bl) in enumerate(zip(centre, bonds)):
        x[k, 0, c] = 1.0
        x[k, 1:, Fe] = 1.0
        for j, code in enumerate(bl):
            adj[k, 0, 1 + j] = adj[k, 1 + j, 0] = code
    return (x, adj, z, tgt, np.ones(n, dtype=np.uint8)), want


def uniqueness_case(ncls=5, n=9):
    """K = 10 samples of one molecule with three distinct signatures A, B (A with another code on the LAST pair), C (A with
    another class on one atom) in the order A B A C B A nan(A) C A B: first = 1 1 0 1 0 0 0 0 0 0, and sample 6, a copy of A
    with a NaN score, is not finite."""
    rng = np.random.default_rng(4)
    z, tgt, flag = random_graph(rng, n, ncls)
    assert flag.all()
    xa, aa = target_scores(z, tgt, ncls, 1)
    ab = aa.copy()
    ab[0, n - 2, n - 1] = ab[0, n - 1, n - 2] = (tgt[n - 2, n - 1] + 1) % 4 + 1
    xc = xa.copy()
    xc[0, 3] = 0.0
    xc[0, 3, (z[3] + 1) % ncls] = 1.0
    xn = xa.copy()
    xn[0, 5, 1] = np.nan
    seq = [(xa, aa), (xa, ab), (xa, aa), (xc, aa), (xa, ab), (xa, aa), (xn, aa), (xc, aa), (xa, aa), (xa, ab)]
    x, adj = np.concatenate([s[0] for s in seq]), np.concatenate([s[1] for s in seq])
    return (x, adj, z, tgt, flag), [1, 1, 0, 1, 0, 0, 0, 0, 0, 0]
