"""COV / MAT evaluation of generated conformers on the batched Kabsch-RMSD kernels (csrc/conformer_rmsd.hip).

For every molecule the RMSD after optimal rigid alignment (proper rotations only) between each of its R reference and each
of its K generated conformers is computed on the device in fp64, and from that R x K matrix, still on the device,

    COV-R(delta) = #{r : min_k rmsd[r, k] <= delta} / R        MAT-R = mean_r min_k rmsd[r, k]
    COV-P(delta) = #{k : min_r rmsd[r, k] <= delta} / K        MAT-P = mean over the finite k of min_r rmsd[r, k]

Atoms are paired in stored order: this is plain Kabsch with NO symmetry permutation, an upper bound of rdkit's
`GetBestRMS` (which also tries the molecule's graph automorphisms); COV is therefore a lower and MAT an upper bound of the
figures an rdkit evaluation reports.  A generated conformer with a non-finite coordinate on an evaluated atom counts as
unmatched: it stays in the denominator of COV-P and is left out of MAT-P; a molecule with no finite generated conformer has
COV 0 and MAT NaN, is counted in `num_failed` and left out of the summary's mean and median.

`records` is what sampler.generate_samples_from_testset returns (or the pickle it writes): per molecule a MolData with
`x`, `positions`, `pos_gen [K n, 3]`, `num_pos_gen` and `finite`.  There is no CPU path: the kernels need a HIP device.

    python -m moleculesde_amd.conformer_eval samples.pkl [--references refs.pt] [--threshold 0.5 1.25] [--all_atoms]
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
from ._torchabi import _f32, _p, _stream

TILE = 8            # CR_TR = CR_TK of csrc/conformer_rmsd.hip
MOL_WORDS = 8       # int64 per molecule of the table (include/msde_hip.h)
REC_DOUBLES = 5     # fp64 per conformer record of the workspace


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


def rmsd_matrix(ref_pos, gen_pos, n_atoms, num_ref, num_gen, atom_mask=None, plan=None):
    """Aligned RMSD of every (reference, generated) pair of every molecule of a ragged set, in one launch.

    ref_pos [sum R_g n_g, 3] and gen_pos [sum K_g n_g, 3] (device, conformer-major within a molecule: the layout of `pos_gen`);
    n_atoms, num_ref, num_gen: G host integers each; atom_mask [sum n_g] (device, bool / uint8; None = all atoms) keeps the
    atoms that are evaluated, the same for every conformer of a molecule.  Returns (rmsd, out_off): rmsd fp64 on the device,
    molecule g's matrix is rmsd[out_off[g] : out_off[g + 1]].view(R_g, K_g); out_off [G + 1] int64 on the host.

    Plain Kabsch in stored atom order, proper rotations only, no symmetry permutation: an upper bound of rdkit's GetBestRMS.
    A conformer with a non-finite coordinate on a kept atom gives NaN in its row / column and changes no other entry."""
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
    _lib.call("msde_conf_rmsd_matrix", _p(ref_pos), _p(gen_pos), _p(plan.mol), plan.G, _p(plan.tiles),
              ctypes.c_longlong(plan.n_tiles), _p(mask), ctypes.c_longlong(plan.n_conf), _p(prep), _p(out), _stream())
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


def evaluate_conformers(records, references=None, thresholds=(0.5, 1.25), heavy_atoms_only=True, device=None):
    """COV-R / MAT-R / COV-P / MAT-P of the generated conformers of `records` (a list from generate_samples_from_testset, or
    the path of its pickle).  references[i] is [R_i, n_i, 3]; default: the record's own `positions` as its single reference.
    heavy_atoms_only evaluates on the atoms with x[:, 0] != 0 (heavy_atom_mask); a molecule left without an atom raises
    ValueError.  Records with finite == False and conformers with non-finite coordinates count as unmatched (module docstring).

    Returns {"thresholds", "num_molecules", "num_failed", "per_molecule": {"cov_r" [G][T], "mat_r" [G], "cov_p" [G][T],
    "mat_p" [G], "num_finite" [G]}, "mean": {...}, "median": {...}}; mean and median over the molecules with at least one finite
    generated conformer (NaN when there is none).  No symmetry permutation: see rmsd_matrix."""
    if isinstance(records, (str, bytes)) or hasattr(records, "__fspath__"):
        with open(records, "rb") as f:
            records = pickle.load(f)
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) == 0:
        raise ValueError("at least one threshold")
    ref, gen, mask, n, R, K = _collect(list(records), references, heavy_atoms_only)
    return summarize(_device_stats(ref, gen, mask, n, R, K, thresholds, device), thresholds)


def _device_stats(ref, gen, mask, n, R, K, thresholds, device=None):
    """Both kernels on the packed host tensors of _collect; the matrix stays on the device, the [G, 2 T + 3] stats come back."""
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.MsdeHipError("conformer evaluation needs a HIP device (no CPU fallback)")
    plan = Plan(n, R, K, dev)
    rmsd, _ = rmsd_matrix(ref.to(dev), gen.to(dev), n, R, K, None if mask is None else mask.to(dev), plan=plan)
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
    res = evaluate_conformers(args.samples, refs, thresholds=args.threshold, heavy_atoms_only=not args.all_atoms)
    if not args.per_molecule:
        res.pop("per_molecule")
    print(json.dumps(_jsonable(res)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
