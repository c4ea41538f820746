"""COV / MAT evaluation of generated conformers on the batched Kabsch-RMSD kernels (csrc/conformer_rmsd.hip).

For every molecule the RMSD after optimal rigid alignment (proper rotations only) between each of its R reference and each
of its K generated conformers is computed on the device in fp64, and from that R x K matrix, still on the device,

    COV-R(delta) = #{r : min_k rmsd[r, k] <= delta} / R        MAT-R = mean_r min_k rmsd[r, k]
    COV-P(delta) = #{k : min_r rmsd[r, k] <= delta} / K        MAT-P = mean over the finite k of min_r rmsd[r, k]

Two modes.  By default atoms are paired in stored order: plain Kabsch with NO symmetry permutation, an UPPER bound of rdkit's
`GetBestRMS` (which also tries the molecule's graph automorphisms); COV is then a lower and MAT an upper bound of the figures
an rdkit evaluation reports, with equality for molecules without a symmetric group.  With `symmetry=True` (`--symmetry`) the
RMSD of a pair is the minimum over the automorphisms of the molecular graph (element and bond order, no chirality:
automorphism.py enumerates them on the host, csrc/conformer_rmsd.hip aligns once per permutation): the figure the published
COV / MAT tables use.  It is exact up to `max_automorphisms` permutations per molecule; a larger group is cut there
(reported as `num_truncated`), which leaves an upper bound that is still never above the plain one.  A generated conformer with a non-finite coordinate on an evaluated atom counts as
unmatched: it stays in the denominator of COV-P and is left out of MAT-P; a molecule with no finite generated conformer has
COV 0 and MAT NaN, is counted in `num_failed` and left out of the summary's mean and median.

`records` is what sampler.generate_samples_from_testset returns (or the pickle it writes): per molecule a MolData with
`x`, `positions`, `pos_gen [K n, 3]`, `num_pos_gen` and `finite`.  There is no CPU path: the kernels need a HIP device.

    python -m moleculesde_amd.conformer_eval samples.pkl [--references refs.pt] [--threshold 0.5 1.25] [--all_atoms]
                                             [--symmetry] [--max_automorphisms 1024]
"""
import argparse
import ctypes
import json
import math
import pickle
import sys

import numpy as np
import torch

from . import _lib
from .automorphism import automorphisms
from ._torchabi import _f32, _p, _stream

TILE = 8            # CR_TR = CR_TK of csrc/conformer_rmsd.hip
MOL_WORDS = 8       # int64 per molecule of the table (include/msde_hip.h)
REC_DOUBLES = 5     # fp64 per conformer record of the workspace
LDS_ATOMS = 160     # CS_LDS_ATOMS: the largest molecule whose tile the symmetric kernel centres into LDS


class Plan:
    """Host-built tables of one launch: `mol` [G, 8] int64 and `tiles` [n_tiles, 3] int32 on the device (include/msde_hip.h),
    `out_off` [G + 1] and `conf_off` [G + 1] int64 on the host (molecule g owns rmsd[out_off[g] : out_off[g + 1]], viewed
    [R_g, K_g], and conf_min[conf_off[g] : conf_off[g + 1]], its R_g row minima then its K_g column minima)."""

    def __init__(self, n_atoms, num_ref, num_gen, device):
        n = np.asarray(list(n_atoms), dtype=np.int64).reshape(-1)
        R = np.asarray(list(num_ref), dtype=np.int64).reshape(-1)
        K = np.asarray(list(num_gen), dtype=np.int64).reshape(-1)
        if not (len(n) == len(R) == len(K)) or len(n) == 0:
            raise ValueError("n_atoms, num_ref and num_gen must be non-empty and of equal length")
        if (n < 1).any() or (R < 1).any() or (K < 1).any():
            raise ValueError("every molecule needs at least one atom, one reference and one generated conformer")
        G = len(n)

        def excl(v):
            return np.concatenate([[0], np.cumsum(v)]).astype(np.int64)

        self.G, self.n, self.R, self.K = G, n, R, K
        self.ref_row, self.gen_row, self.atom_off = excl(R * n), excl(K * n), excl(n)
        self.out_off, self.conf_off = excl(R * K), excl(R + K)
        mol = np.stack([n, R, K, self.ref_row[:-1], self.gen_row[:-1], self.out_off[:-1], self.atom_off[:-1],
                        self.conf_off[:-1]], axis=1)
        tiles = []
        for g in range(G):
            r0, k0 = np.meshgrid(np.arange(0, R[g], TILE), np.arange(0, K[g], TILE), indexing="ij")
            tiles.append(np.stack([np.full(r0.size, g), r0.reshape(-1), k0.reshape(-1)], axis=1))
        tiles = np.concatenate(tiles).astype(np.int32)
        self.n_tiles, self.n_conf = int(tiles.shape[0]), int(self.conf_off[-1])
        self.mol = torch.from_numpy(np.ascontiguousarray(mol)).to(device)
        self.tiles = torch.from_numpy(np.ascontiguousarray(tiles)).to(device)


def _permutation_tables(permutations, n, keep):
    """Host checks of rmsd_matrix's `permutations` (G arrays [P_g, n_g]; n [G]; keep: host bool [sum n] or None) and the two
    tables of msde_conf_rmsd_matrix_sym: sym [G, 2] int64 (P_g, first element in perms) and perms [sum P_g n_g] int32."""
    if len(permutations) != len(n):
        raise ValueError(f"{len(permutations)} permutation tables for {len(n)} molecules")
    sym, flat, off, atom0 = [], [], 0, 0
    for g, (pg, ng) in enumerate(zip(permutations, n)):
        ng = int(ng)
        pg = np.asarray(pg.cpu() if torch.is_tensor(pg) else pg)
        if pg.ndim != 2 or pg.shape[0] < 1 or pg.shape[1] != ng or pg.dtype.kind not in "iu":
            raise ValueError(f"molecule {g}: permutations {pg.shape} {pg.dtype} are not an integer [P >= 1, {ng}] table")
        if pg.min() < 0 or pg.max() >= ng:
            raise ValueError(f"molecule {g}: a permutation names an atom outside [0, {ng})")
        kept = np.arange(ng) if keep is None else np.flatnonzero(keep[atom0:atom0 + ng])
        if not np.array_equal(np.sort(pg[:, kept], axis=1), np.broadcast_to(kept, (pg.shape[0], kept.size))):
            raise ValueError(f"molecule {g}: a permutation row is not a bijection of the kept atoms onto the kept atoms")
        sym.append((pg.shape[0], off))
        flat.append(pg.astype(np.int32).reshape(-1))
        off += pg.size
        atom0 += ng
    return np.asarray(sym, dtype=np.int64), np.concatenate(flat)


def rmsd_matrix(ref_pos, gen_pos, n_atoms, num_ref, num_gen, atom_mask=None, plan=None, permutations=None, lds_atoms=None):
    """Aligned RMSD of every (reference, generated) pair of every molecule of a ragged set, in one launch.

    ref_pos [sum R_g n_g, 3] and gen_pos [sum K_g n_g, 3] (device, conformer-major within a molecule: the layout of `pos_gen`);
    n_atoms, num_ref, num_gen: G host integers each; atom_mask [sum n_g] (device, bool / uint8; None = all atoms) keeps the
    atoms that are evaluated, the same for every conformer of a molecule.  Returns (rmsd, out_off): rmsd fp64 on the device,
    molecule g's matrix is rmsd[out_off[g] : out_off[g + 1]].view(R_g, K_g); out_off [G + 1] int64 on the host.

    permutations=None: plain Kabsch in stored atom order, proper rotations only, no symmetry permutation -- an upper bound of
    rdkit's GetBestRMS.  permutations = a list of G host integer arrays [P_g, n_g] (automorphism.automorphisms): the minimum
    over the rows p of the RMSD with reference atom permutations[g][p][a] paired with generated atom a -- the best RMSD over the
    listed symmetries, GetBestRMS itself when the list is the molecule's whole group.  The tables are checked on the host
    (shape, indices in [0, n_g), every row a bijection of the kept atoms onto the kept atoms; ValueError otherwise) and
    uploaded once.  lds_atoms (0 .. LDS_ATOMS; default: the largest n_g that fits) sizes the symmetric kernel's LDS staging
    and does not change a bit of the result.
    A conformer with a non-finite coordinate on a kept atom gives NaN in its row / column and changes no other entry."""
    tables = None
    if permutations is not None:
        n_host = plan.n if plan is not None else np.asarray(list(n_atoms), dtype=np.int64).reshape(-1)
        keep = None if atom_mask is None else (torch.as_tensor(atom_mask).reshape(-1) != 0).cpu().numpy()
        if keep is not None and keep.size != int(n_host.sum()):
            raise ValueError(f"atom_mask has {keep.size} entries for {int(n_host.sum())} atoms")
        tables = _permutation_tables(list(permutations), n_host, keep)
        fits = n_host[n_host <= LDS_ATOMS]
        lds_atoms = (int(fits.max()) if fits.size else 0) if lds_atoms is None else int(lds_atoms)
        if not 0 <= lds_atoms <= LDS_ATOMS:
            raise ValueError(f"lds_atoms must lie in [0, {LDS_ATOMS}]")
    ref_pos, gen_pos = _f32(ref_pos), _f32(gen_pos)
    if plan is None:
        plan = Plan(n_atoms, num_ref, num_gen, ref_pos.device)
    if tuple(ref_pos.shape) != (int(plan.ref_row[-1]), 3) or tuple(gen_pos.shape) != (int(plan.gen_row[-1]), 3):
        raise ValueError(f"ref_pos {tuple(ref_pos.shape)} / gen_pos {tuple(gen_pos.shape)} do not hold sum R n = "
                         f"{int(plan.ref_row[-1])} / sum K n = {int(plan.gen_row[-1])} rows of 3")
    mask = None
    if atom_mask is not None:
        if not atom_mask.is_cuda:
            raise _lib.MsdeHipError("moleculesde_amd kernels need tensors on the HIP device (no CPU fallback)")
        if atom_mask.numel() != int(plan.atom_off[-1]):
            raise ValueError(f"atom_mask has {atom_mask.numel()} entries for {int(plan.atom_off[-1])} atoms")
        mask = (atom_mask.reshape(-1) != 0).to(torch.uint8).contiguous()
    dev = ref_pos.device
    prep = torch.empty(plan.n_conf * REC_DOUBLES, dtype=torch.float64, device=dev)
    out = torch.empty(int(plan.out_off[-1]), dtype=torch.float64, device=dev)
    if tables is None:
        _lib.call("msde_conf_rmsd_matrix", _p(ref_pos), _p(gen_pos), _p(plan.mol), plan.G, _p(plan.tiles),
                  ctypes.c_longlong(plan.n_tiles), _p(mask), ctypes.c_longlong(plan.n_conf), _p(prep), _p(out), _stream())
    else:
        sym, perms = torch.from_numpy(tables[0]).to(dev), torch.from_numpy(tables[1]).to(dev)
        _lib.call("msde_conf_rmsd_matrix_sym", _p(ref_pos), _p(gen_pos), _p(plan.mol), plan.G, _p(plan.tiles),
                  ctypes.c_longlong(plan.n_tiles), _p(mask), ctypes.c_longlong(plan.n_conf), _p(sym), _p(perms), lds_atoms,
                  _p(prep), _p(out), _stream())
    return out, torch.from_numpy(plan.out_off.copy())


def cov_mat(rmsd, num_ref, num_gen, thresholds, plan=None):
    """COV / MAT of every molecule from the device matrix of rmsd_matrix.  Returns (stats, conf_min, conf_off): stats [G, 2 T + 3]
    fp64 on the device = COV-R [T], COV-P [T], MAT-R, MAT-P, number of finite generated conformers; conf_min = per molecule its
    R row minima then its K column minima (NaN read as +inf), at conf_off[g] (host)."""
    if not rmsd.is_cuda:
        raise _lib.MsdeHipError("moleculesde_amd kernels need tensors on the HIP device (no CPU fallback)")
    if plan is None:
        plan = Plan(np.ones(len(list(num_ref)), dtype=np.int64), num_ref, num_gen, rmsd.device)
    thr = [float(t) for t in thresholds]
    if len(thr) == 0:
        raise ValueError("at least one threshold")
    if rmsd.dtype != torch.float64 or rmsd.numel() != int(plan.out_off[-1]):
        raise ValueError(f"rmsd must be the fp64 matrix of rmsd_matrix ({int(plan.out_off[-1])} entries)")
    rmsd = rmsd.contiguous()
    T = len(thr)
    thr_dev = torch.tensor(thr, dtype=torch.float64).to(rmsd.device)
    conf_min = torch.empty(plan.n_conf, dtype=torch.float64, device=rmsd.device)
    stats = torch.empty(plan.G, 2 * T + 3, dtype=torch.float64, device=rmsd.device)
    _lib.call("msde_conf_cov_mat", _p(rmsd), _p(plan.mol), plan.G, _p(thr_dev), T, _p(conf_min), _p(stats), _stream())
    return stats, conf_min, torch.from_numpy(plan.conf_off.copy())


def heavy_atom_mask(x):
    """Atoms that are not hydrogen.  Column 0 of `x` (or a 1-D `x`) is the atomic number minus one -- the featuriser stores
    `atom.GetAtomicNum() - 1` (Geom3D/datasets/dataset_utils.py:122-127), synthetic.make_molecule(with_h=True) marks its
    hydrogens with 0 (synthetic.py) and tools/make_golden_finetune_qm9.py reads 0 back as Z = 1 -- so hydrogen is index 0."""
    z = x if x.dim() == 1 else x[:, 0]
    return z != 0


def _collect(records, references, heavy_atoms_only):
    """Host-side checks and packing: (ref_pos, gen_pos, mask or None, n, R, K), CPU tensors."""
    if len(records) == 0:
        raise ValueError("no records")
    if references is not None and len(references) != len(records):
        raise ValueError(f"{len(references)} reference sets for {len(records)} records")
    refs, gens, masks, n_l, R_l, K_l = [], [], [], [], [], []
    for i, rec in enumerate(records):
        n = int(rec.x.size(0))
        K = int(torch.as_tensor(rec.num_pos_gen).reshape(-1)[0])
        gen = torch.as_tensor(rec.pos_gen, dtype=torch.float32).cpu()
        if K < 1 or gen.dim() != 2 or tuple(gen.shape) != (K * n, 3):
            raise ValueError(f"record {i}: pos_gen {tuple(gen.shape)} does not hold num_pos_gen = {K} conformers of {n} atoms")
        ref = rec.positions if references is None else references[i]
        ref = torch.as_tensor(ref, dtype=torch.float32).cpu()
        if ref.dim() == 2:
            ref = ref[None]
        if ref.dim() != 3 or ref.size(0) < 1 or tuple(ref.shape[1:]) != (n, 3):
            raise ValueError(f"record {i}: references {tuple(ref.shape)} are not [R, {n}, 3]")
        if not getattr(rec, "finite", True):
            gen = torch.full_like(gen, float("nan"))          # the trajectory left the finite numbers: nothing of it counts
        keep = heavy_atom_mask(rec.x.cpu()) if heavy_atoms_only else torch.ones(n, dtype=torch.bool)
        if int(keep.sum()) == 0:
            raise ValueError(f"record {i}: the atom mask keeps no atom (heavy_atoms_only on a molecule of hydrogens)")
        refs.append(ref.reshape(-1, 3)); gens.append(gen); masks.append(keep)
        n_l.append(n); R_l.append(int(ref.size(0))); K_l.append(K)
    mask = torch.cat(masks) if heavy_atoms_only else None
    return torch.cat(refs), torch.cat(gens), mask, n_l, R_l, K_l


def _groups(records, heavy_atoms_only, max_automorphisms):
    """Per record the automorphisms of its molecular graph (atoms coloured by x[:, 0], bonds by edge_attr[:, 0]) on the atoms it
    is evaluated on: (list of [P_g, n_g] int32, number of truncated groups)."""
    perms, truncated = [], 0
    for i, rec in enumerate(records):
        ei, ea = getattr(rec, "edge_index", None), getattr(rec, "edge_attr", None)
        if ei is None or ea is None:
            raise ValueError(f"record {i}: symmetry=True needs the record's edge_index and edge_attr")
        x = torch.as_tensor(rec.x).cpu()
        ei, ea = torch.as_tensor(ei).cpu().numpy(), torch.as_tensor(ea).cpu().numpy()
        if ei.ndim != 2 or ei.shape[0] != 2 or ea.shape[0] != ei.shape[1]:
            raise ValueError(f"record {i}: edge_index {ei.shape} / edge_attr {ea.shape} are not [2, E] / [E, ...]")
        keep = heavy_atom_mask(x).numpy() if heavy_atoms_only else None
        p, cut = automorphisms(int(x.size(0)), ei, (x if x.dim() == 1 else x[:, 0]).numpy(),
                               ea if ea.ndim == 1 else ea[:, 0], keep=keep, max_count=max_automorphisms)
        perms.append(p)
        truncated += int(cut)
    return perms, truncated


def summarize(stats, thresholds):
    """The result dictionary from the host copy of the kernel's stats [G, 2 T + 3] (numpy, fp64)."""
    T = len(thresholds)
    cov_r, cov_p, mat_r, mat_p, fin = stats[:, :T], stats[:, T:2 * T], stats[:, 2 * T], stats[:, 2 * T + 1], stats[:, 2 * T + 2]
    ok = fin > 0
    res = {"thresholds": [float(t) for t in thresholds], "num_molecules": int(stats.shape[0]), "num_failed": int((~ok).sum()),
           "per_molecule": {"cov_r": cov_r.tolist(), "mat_r": mat_r.tolist(), "cov_p": cov_p.tolist(), "mat_p": mat_p.tolist(),
                            "num_finite": [int(v) for v in fin]}}
    for name, f in (("mean", np.mean), ("median", np.median)):
        if ok.any():
            res[name] = {"cov_r": f(cov_r[ok], axis=0).tolist(), "mat_r": float(f(mat_r[ok])),
                         "cov_p": f(cov_p[ok], axis=0).tolist(), "mat_p": float(f(mat_p[ok]))}
        else:
            res[name] = {"cov_r": [float("nan")] * T, "mat_r": float("nan"), "cov_p": [float("nan")] * T, "mat_p": float("nan")}
    return res


def evaluate_conformers(records, references=None, thresholds=(0.5, 1.25), heavy_atoms_only=True, device=None, symmetry=False,
                        max_automorphisms=1024):
    """COV-R / MAT-R / COV-P / MAT-P of the generated conformers of `records` (a list from generate_samples_from_testset, or
    the path of its pickle).  references[i] is [R_i, n_i, 3]; default: the record's own `positions` as its single reference.
    heavy_atoms_only evaluates on the atoms with x[:, 0] != 0 (heavy_atom_mask); a molecule left without an atom raises
    ValueError.  Records with finite == False and conformers with non-finite coordinates count as unmatched (module docstring).

    Returns {"thresholds", "num_molecules", "num_failed", "per_molecule": {"cov_r" [G][T], "mat_r" [G], "cov_p" [G][T],
    "mat_p" [G], "num_finite" [G]}, "mean": {...}, "median": {...}}; mean and median over the molecules with at least one finite
    generated conformer (NaN when there is none).

    symmetry=False: no symmetry permutation (see rmsd_matrix) -- COV is a lower, MAT an upper bound of an rdkit evaluation.
    symmetry=True: each record's automorphism group is built from its `x`, `edge_index` and `edge_attr` on the atoms it is
    evaluated on (heavy_atoms_only: the group of the heavy-atom sub-graph) and every RMSD is the minimum over it, as in
    rdkit's GetBestRMS; at most max_automorphisms permutations per molecule (a larger group is cut there: still an upper bound,
    never above the plain one).  The result gains "symmetry": {"num_permutations" [G], "num_truncated"}.  A record without
    `edge_index` / `edge_attr` raises a ValueError that names it."""
    if isinstance(records, (str, bytes)) or hasattr(records, "__fspath__"):
        with open(records, "rb") as f:
            records = pickle.load(f)
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) == 0:
        raise ValueError("at least one threshold")
    records = list(records)
    ref, gen, mask, n, R, K = _collect(records, references, heavy_atoms_only)
    if not symmetry:
        return summarize(_device_stats(ref, gen, mask, n, R, K, thresholds, device), thresholds)
    perms, truncated = _groups(records, heavy_atoms_only, max_automorphisms)
    res = summarize(_device_stats(ref, gen, mask, n, R, K, thresholds, device, permutations=perms), thresholds)
    res["symmetry"] = {"num_permutations": [int(p.shape[0]) for p in perms], "num_truncated": truncated}
    return res


def _device_stats(ref, gen, mask, n, R, K, thresholds, device=None, permutations=None):
    """Both kernels on the packed host tensors of _collect; the matrix stays on the device, the [G, 2 T + 3] stats come back."""
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.MsdeHipError("conformer evaluation needs a HIP device (no CPU fallback)")
    plan = Plan(n, R, K, dev)
    rmsd, _ = rmsd_matrix(ref.to(dev), gen.to(dev), n, R, K, None if mask is None else mask.to(dev), plan=plan,
                          permutations=permutations)
    stats, _, _ = cov_mat(rmsd, R, K, thresholds, plan=plan)
    return stats.cpu().numpy()


def _parser():
    ap = argparse.ArgumentParser(prog="python -m moleculesde_amd.conformer_eval",
                                 description="COV / MAT of the conformers in a pickle of generate_samples_from_testset")
    ap.add_argument("samples", help="pickle written by generate_samples_from_testset(out_path=...)")
    ap.add_argument("--references", default=None,
                    help="torch.save'd list with one [R_i, n_i, 3] tensor per record (default: each record's positions)")
    ap.add_argument("--threshold", type=float, nargs="+", default=[0.5, 1.25], help="COV thresholds in Angstrom")
    ap.add_argument("--all_atoms", action="store_true", help="evaluate on all atoms, not on the heavy atoms only")
    ap.add_argument("--per_molecule", action="store_true", help="keep the per-molecule lists in the printed line")
    ap.add_argument("--symmetry", action="store_true",
                    help="best RMSD over the automorphisms of each molecular graph (as rdkit's GetBestRMS), not stored atom order")
    ap.add_argument("--max_automorphisms", type=int, default=1024, metavar="N",
                    help="with --symmetry: at most N permutations per molecule (a memory bound on the table)")
    return ap


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def main(argv=None):
    args = _parser().parse_args(argv)
    refs = torch.load(args.references) if args.references else None
    res = evaluate_conformers(args.samples, refs, thresholds=args.threshold, heavy_atoms_only=not args.all_atoms,
                              symmetry=args.symmetry, max_automorphisms=args.max_automorphisms)
    if not args.per_molecule:
        res.pop("per_molecule")
        if "symmetry" in res:
            res["symmetry"].pop("num_permutations")
    print(json.dumps(_jsonable(res)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
