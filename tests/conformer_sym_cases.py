"""Shared by the symmetry-aware conformer-evaluation tests (not a test module): graphs whose automorphism groups are known,
the fp64 reference of the best RMSD over a permutation list, the NumPy mirror of the device formula, and the case builders.

Reference: sym_rmsd_block = min over p of conformer_eval_cases.kabsch_rmsd(x[perms[p]][keep], y[keep]) (SVD-Kabsch, residual
formed).  Mirror: the same minimum of conformer_eval_cases.mirror_rmsd (Horn's eigenvalue formula in fp64 with LAPACK), which
is what csrc/conformer_rmsd.hip computes per permutation.  The device tests allow MARGIN x the worst |mirror - reference| over
the cases of their own file (formula_error below), as tests/conformer_eval_cases.py does for the plain kernel."""
import numpy as np

import conformer_eval_cases as C

CARBON, NITROGEN, HYDROGEN = 5, 6, 0            # x[:, 0] = atomic number minus one; 0 is what heavy_atom_mask drops


class Graph:
    """n atoms, undirected bonds [(u, v)], one colour per atom and per bond; keep = the atoms that are not hydrogen."""

    def __init__(self, name, n, bonds, count, atom_colour=None, bond_colour=None):
        self.name, self.n, self.bonds, self.count = name, n, list(bonds), count
        self.atom_colour = np.full(n, CARBON, dtype=np.int64) if atom_colour is None else np.asarray(atom_colour, dtype=np.int64)
        self.bond_colour = np.zeros(len(self.bonds), dtype=np.int64) if bond_colour is None else np.asarray(bond_colour, dtype=np.int64)
        self.keep = self.atom_colour != HYDROGEN

    @property
    def edge_index(self):
        """[2, 2 E]: both directions, as the records store it."""
        e = np.asarray(self.bonds, dtype=np.int64).reshape(-1, 2).T
        return np.concatenate([e, e[::-1]], axis=1)

    @property
    def edge_colour(self):
        return np.concatenate([self.bond_colour, self.bond_colour])


def _ring(first, size=6):
    return [(first + i, first + (i + 1) % size) for i in range(size)]


def _chain34():
    """A 10-atom backbone 0 .. 9 that carries, in this order, a three-leaf group on atom 0, a 6-ring on 3, a three-leaf group on
    5, a 6-ring on 7 and a three-leaf group on 9: nothing maps the backbone onto itself but the identity, each group's leaves
    permute (3! each) and each ring flips about its attachment (2 each): 6^3 * 2^2 = 864."""
    bonds = [(i, i + 1) for i in range(9)]
    nxt = 10
    for at, kind in ((0, "leaves"), (3, "ring"), (5, "leaves"), (7, "ring"), (9, "leaves")):
        if kind == "leaves":
            bonds += [(at, nxt)] + [(nxt, nxt + 1 + j) for j in range(3)]
            nxt += 4
        else:
            bonds += [(at, nxt)] + _ring(nxt)
            nxt += 6
    assert nxt == 34
    return bonds


_CUBE = [(u, u ^ b) for u in range(8) for b in (1, 2, 4) if u < u ^ b]

GRAPHS = [
    Graph("path5", 5, [(i, i + 1) for i in range(4)], 2),
    Graph("star4", 5, [(0, i) for i in range(1, 5)], 24),
    Graph("ring6", 6, _ring(0), 12),
    Graph("ring6_alternating_bonds", 6, _ring(0), 6, bond_colour=[0, 1, 0, 1, 0, 1]),
    Graph("ring6_one_atom_recoloured", 6, _ring(0), 2, atom_colour=[NITROGEN] + [CARBON] * 5),
    Graph("cubane", 8, _CUBE, 48),
    Graph("tert_butyl_ring6", 10, _ring(0) + [(0, 6), (6, 7), (6, 8), (6, 9)], 12),
    Graph("star4_one_leaf_masked", 5, [(0, i) for i in range(1, 5)], 6, atom_colour=[CARBON] * 4 + [HYDROGEN]),
    Graph("chain34", 34, _chain34(), 864),
    Graph("two_paths3", 6, [(0, 1), (1, 2), (3, 4), (4, 5)], 8),
]


def group(g, max_count=1024):
    from moleculesde_amd.automorphism import automorphisms
    return automorphisms(g.n, g.edge_index, g.atom_colour, g.edge_colour, keep=g.keep, max_count=max_count)


def is_automorphism(g, row):
    """row maps the kept atoms one to one onto the kept atoms, fixes the others, and preserves atom colours, bonds with their
    colours and non-bonds."""
    kept = np.flatnonzero(g.keep)
    row = np.asarray(row)
    if sorted(row[kept].tolist()) != kept.tolist() or not np.array_equal(row[~g.keep], np.flatnonzero(~g.keep)):
        return False
    if not np.array_equal(g.atom_colour[row[kept]], g.atom_colour[kept]):
        return False
    bonds = {}
    for (u, v), c in zip(g.bonds, g.bond_colour.tolist()):
        if g.keep[u] and g.keep[v]:
            bonds[(u, v)] = bonds[(v, u)] = c
    return {(int(row[u]), int(row[v])): c for (u, v), c in bonds.items()} == bonds


# ---- reference and mirror ---------------------------------------------------------------------------------------------------
def sym_rmsd_block(ref, gen, perms, keep=None, fn=C.kabsch_rmsd):
    """[R, K] of min over p of fn(x[perms[p]][keep], y[keep]) for ref [R, n, 3], gen [K, n, 3], perms [P, n]; NaN where a
    conformer is not finite on a kept atom."""
    keep = np.ones(ref.shape[1], dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    out = np.empty((ref.shape[0], gen.shape[0]), dtype=np.float64)
    for r, x in enumerate(ref):
        xs = [x[p][keep] for p in perms]
        for k, y in enumerate(gen):
            yk = y[keep]
            vals = [fn(xp, yk) for xp in xs]
            out[r, k] = np.nan if np.isnan(vals).any() else min(vals)
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------
def random_permutations(rng, n, P, keep=None):
    """[P, n] int32: the identity, then P - 1 random permutations of the kept atoms (the others stay)."""
    kept = np.arange(n) if keep is None else np.flatnonzero(keep)
    out = np.tile(np.arange(n, dtype=np.int32), (P, 1))
    for p in range(1, P):
        out[p, kept] = rng.permutation(kept)
    return out


_AXIS_ROTATIONS = [Q for Q in (np.eye(3)[list(perm)] * np.array(sign)[:, None]
                               for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
                               for sign in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1),
                                            (-1, -1, -1)))
                   if np.linalg.det(Q) > 0]
assert len(_AXIS_ROTATIONS) == 24


def relabelled_copy(g, seed, exact=True):
    """(ref [1, n, 3], gen [1, n, 3], perm): an asymmetric random reference (sigma = 1.5 A) and gen[a] = Q ref[perm[a]] + t with
    perm a non-identity automorphism of g.  exact: the coordinates are multiples of 2^-10 A, Q is one of the 24 proper axis
    rotations and t a multiple of 2^-10, so the copy is rigid in fp32 to the last bit and its true best RMSD is 0; otherwise Q is
    a random rotation, |t| = 5 A, and rounding to fp32 leaves about 1e-7 A."""
    rng = np.random.default_rng([seed, GRAPHS.index(g)])
    perms, _ = group(g)
    perm = perms[1 + int(rng.integers(0, len(perms) - 1))]
    ref = rng.normal(size=(g.n, 3)) * 1.5
    if exact:
        ref = np.rint(ref * 1024.0) / 1024.0
        gen = ref[perm] @ _AXIS_ROTATIONS[int(rng.integers(0, 24))].T + np.rint(rng.normal(size=3) * 2048.0) / 1024.0
    else:
        gen = C._rigid(rng, ref[perm])
    ref32, gen32 = ref.astype(np.float32), gen.astype(np.float32)
    if exact:
        assert np.array_equal(ref32, ref) and np.array_equal(gen32, gen)
    return ref32[None], gen32[None], perm


def formula_error(cases):
    """Worst |mirror - reference| over cases given as (ref, gen, perms, keep), and the two matrices of every case."""
    worst, mats = 0.0, []
    for ref, gen, perms, keep in cases:
        want = sym_rmsd_block(ref, gen, perms, keep)
        mir = sym_rmsd_block(ref, gen, perms, keep, fn=C.mirror_rmsd)
        worst = max(worst, float(np.abs(mir - want).max()))
        mats.append((want, mir))
    return worst, mats
