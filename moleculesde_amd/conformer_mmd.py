"""Distance-distribution MMD of generated conformers on the kernels of csrc/conformer_mmd.hip: does the generated ENSEMBLE of a
molecule have the distribution of interatomic distances of its reference ensemble?  (COV / MAT of conformer_eval.py asks
whether each reference conformer is found; a sampler that collapses onto one good conformer passes that and fails this.)

The definition is this project's; the conformer-generation literature reports tables of this kind without one
shared implementation.  For one molecule with R reference and K generated conformers and E evaluated atom pairs (u_e, v_e):

    z[a, e] = |pos_a[u_e] - pos_a[v_e]|            the conformers pooled, references first, C = R + K
    L_ab    = sum_{e in S} (z[a, e] - z[b, e])^2    for a subset S of the columns
    sigma^2 = sum_{a, b} L_ab / (C^2 - C)           the bandwidth; additive over the columns of S
    k(a, b) = sum_{i < kernel_num} exp(-L_ab / (sigma^2 kernel_mul^(i - kernel_num // 2)))      (defaults 2.0, 5: 1/4 .. 4)
    MMD(S)  = mean_{a, b in ref} k + mean_{a, b in gen} k - 2 mean_{a in ref, b in gen} k       (V-statistic with diagonals)

and MMD(S) = 0 exactly when sigma^2 = 0.  Per molecule: Single = median and mean of MMD({e}) over e; Pair = median and mean of
MMD({e, f}) over e < f (NaN when E < 2); All = MMD of all E columns.  Medians as NumPy's (mean of the two middle values).
A conformer with a non-finite coordinate on an evaluated atom is excluded from every sum and count; R and K are then the
counts that remain.  No reference or no generated conformer left: NaN, counted in `num_failed`; no evaluated pair (E = 0)
with conformers left: NaN, counted in `num_without_pairs` only.

Evaluated pairs: the pairs u < v of evaluated atoms (heavy atoms by default, as in conformer_eval) at most `max_hops` bonds
apart in the FULL molecular graph of the record's `edge_index` (through hydrogens too); default 3 = bonds, angles, torsions;
None = all pairs.  There is no CPU path: the kernels need a HIP device.

    python -m moleculesde_amd.conformer_mmd samples.pkl [--references refs.pt] [--max_hops N | --all_pairs] [--all_atoms]
"""
import argparse
import ctypes
import json
import pickle
import sys

import numpy as np
import torch

from . import _lib
from .conformer_eval import _collect, _jsonable, heavy_atom_mask
from ._torchabi import _f32, _p, _stream

MAX_POOLED = 1024   # CM_MAX_POOLED of csrc/conformer_mmd.hip: the largest R + K of one molecule (two fp64 columns in LDS)
MAX_KERNELS = 16    # CM_MAX_KERNELS
MOL_WORDS = 8       # int64 per molecule of the table (include/msde_hip.h)
STATS = ("single_median", "single_mean", "pair_median", "pair_mean", "all")


def _graph_pairs(n, edge_index, keep, max_hops):
    """[E, 2] int32 pairs u < v, ordered by (u, v), in the numbering of the kept atoms (keep: bool [n]), of kept atoms at most
    max_hops bonds apart in the graph on ALL n atoms (edge_index [2, M], either direction); max_hops None: all pairs."""
    kept = np.flatnonzero(keep)
    if max_hops is None:
        u, v = np.triu_indices(kept.size, 1)
        return np.stack([u, v], axis=1).astype(np.int32)
    if int(max_hops) < 1:
        raise ValueError("max_hops must be at least 1 (or None for all pairs)")
    ei = np.asarray(edge_index)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index {ei.shape} is not [2, M]")
    if ei.size and (ei.min() < 0 or ei.max() >= n):
        raise ValueError(f"edge_index names an atom outside [0, {n})")
    nbr = [[] for _ in range(n)]
    for a, b in zip(ei[0].tolist(), ei[1].tolist()):
        nbr[a].append(b)
        nbr[b].append(a)
    local = np.full(n, -1, dtype=np.int64)
    local[kept] = np.arange(kept.size)
    out = []
    for s in kept.tolist():                                    # breadth-first from every kept atom, max_hops levels
        seen, level, near = {s}, [s], []
        for _ in range(int(max_hops)):
            nxt = []
            for a in level:
                for b in nbr[a]:
                    if b not in seen:
                        seen.add(b)
                        nxt.append(b)
            near += nxt
            level = nxt
        out += [(int(local[s]), int(local[b])) for b in sorted(near) if b > s and local[b] >= 0]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def distance_pairs(record, heavy_atoms_only=True, max_hops=3):
    """The evaluated atom pairs of one record: [E, 2] int32, u < v, ordered by (u, v), indexed in the evaluated-atom numbering
    (position among the atoms heavy_atom_mask keeps, or among all atoms).  Hops are counted in the record's whole graph."""
    x = torch.as_tensor(record.x).cpu()
    n = int(x.size(0))
    keep = heavy_atom_mask(x).numpy() if heavy_atoms_only else np.ones(n, dtype=bool)
    ei = getattr(record, "edge_index", None)
    if max_hops is not None and ei is None:
        raise ValueError("distance_pairs with max_hops needs the record's edge_index")
    return _graph_pairs(n, None if ei is None else torch.as_tensor(ei).cpu().numpy(), keep, max_hops)


def _excl(v):
    return np.concatenate([[0], np.cumsum(v)]).astype(np.int64)


class Plan:
    """Host-built tables of one launch, NumPy only (`upload` puts them on the device).  mol [G, 8] int64, pair_ptr [G + 1]
    int64, atom_pairs [sum E, 2] int32 (molecule-local ATOM indices), items [n_items, 3] int32 (the Single items of every
    molecule, then the Pair items), pairitem_ptr [G + 1] int64: include/msde_hip.h.  ValueError on anything that does not fit."""

    def __init__(self, n_atoms, num_ref, num_gen, pairs, pair_ptr, keep=None):
        n = np.asarray(list(n_atoms), dtype=np.int64).reshape(-1)
        R = np.asarray(list(num_ref), dtype=np.int64).reshape(-1)
        K = np.asarray(list(num_gen), dtype=np.int64).reshape(-1)
        if not (len(n) == len(R) == len(K)) or len(n) == 0:
            raise ValueError("n_atoms, num_ref and num_gen must be non-empty and of equal length")
        if (n < 1).any() or (R < 1).any() or (K < 1).any():
            raise ValueError("every molecule needs at least one atom, one reference and one generated conformer")
        G, C = len(n), R + K
        if int(C.max()) > MAX_POOLED:
            g = int(C.argmax())
            raise ValueError(f"molecule {g}: {int(R[g])} + {int(K[g])} pooled conformers exceed the {MAX_POOLED} the kernels stage")
        ptr = np.asarray(pair_ptr, dtype=np.int64).reshape(-1)
        pairs = np.asarray(pairs).reshape(-1, 2)
        if len(ptr) != G + 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or int(ptr[-1]) != pairs.shape[0]:
            raise ValueError(f"pair_ptr is not the [G + 1] offsets of the {pairs.shape[0]} pairs of {G} molecules")
        if pairs.size and pairs.dtype.kind not in "iu":
            raise ValueError("pairs must be integers")
        atom_off = _excl(n)
        if keep is not None:
            keep = np.asarray(keep).reshape(-1) != 0
            if keep.size != int(atom_off[-1]):
                raise ValueError(f"atom_mask has {keep.size} entries for {int(atom_off[-1])} atoms")
        atom_pairs = np.zeros((pairs.shape[0], 2), dtype=np.int32)
        for g in range(G):
            kept = np.arange(n[g]) if keep is None else np.flatnonzero(keep[atom_off[g]:atom_off[g + 1]])
            pg = pairs[ptr[g]:ptr[g + 1]]
            if pg.size and (pg.min() < 0 or pg.max() >= kept.size):
                raise ValueError(f"molecule {g}: a pair names an atom outside its {kept.size} evaluated atoms")
            atom_pairs[ptr[g]:ptr[g + 1]] = kept[pg]
        E = np.diff(ptr)
        self.G, self.n, self.R, self.K, self.E = G, n, R, K, E
        self.ref_row, self.gen_row, self.atom_off, self.conf_off = _excl(R * n), _excl(K * n), atom_off, _excl(C)
        self.z_off, self.pair_ptr, self.pairitem_ptr = _excl(C * E), ptr, _excl(E * (E - 1) // 2)
        self.n_conf, self.n_cols, self.c_max = int(self.conf_off[-1]), int(ptr[-1]), int(C.max())
        self.mol = np.ascontiguousarray(np.stack([n, R, K, self.ref_row[:-1], self.gen_row[:-1], self.z_off[:-1],
                                                  atom_off[:-1], self.conf_off[:-1]], axis=1))
        single = np.stack([np.repeat(np.arange(G), E), np.concatenate([np.arange(e) for e in E] + [np.zeros(0, np.int64)]),
                           np.full(self.n_cols, -1)], axis=1)
        both = [np.zeros((0, 3), dtype=np.int64)]
        for g in range(G):
            e, f = np.triu_indices(int(E[g]), 1)               # ordered by (e, f)
            both.append(np.stack([np.full(e.size, g), e, f], axis=1))
        self.items = np.ascontiguousarray(np.concatenate([single] + both).astype(np.int32))
        self.n_items = int(self.items.shape[0])
        self.atom_pairs = atom_pairs
        self.keep = keep
        self.dev = None

    def upload(self, device):
        """The device copies of the tables (once per device)."""
        if self.dev is None or self.dev["device"] != device:
            def put(a):
                return torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self.dev = {"device": device, "mol": put(self.mol), "pair_ptr": put(self.pair_ptr),
                        "pairitem_ptr": put(self.pairitem_ptr),
                        "pairs": put(self.atom_pairs if self.n_cols else np.zeros((1, 2), dtype=np.int32)),
                        "items": put(self.items if self.n_items else np.zeros((1, 3), dtype=np.int32))}
        return self.dev


def _kernel_parameters(kernel_mul, kernel_num):
    mul, num = float(kernel_mul), int(kernel_num)
    if not (mul > 0.0 and np.isfinite(mul)) or num != kernel_num or not 1 <= num <= MAX_KERNELS:
        raise ValueError(f"kernel_mul must be positive and finite and kernel_num an integer in [1, {MAX_KERNELS}]")
    return mul, num


def _segment_median(values, ptr):
    """Median of values[ptr[g] : ptr[g + 1]] per segment on the device (NumPy's convention; NaN for an empty segment and for a
    segment that holds a NaN): one sort by value, one stable sort by segment."""
    G, n = ptr.numel() - 1, values.numel()
    cnt = ptr[1:] - ptr[:-1]
    nan = torch.full((G,), float("nan"), dtype=torch.float64, device=values.device)
    if n == 0:
        return nan
    seg = torch.repeat_interleave(torch.arange(G, device=values.device), cnt, output_size=n)
    v, order = torch.sort(values)
    _, by_seg = torch.sort(seg[order], stable=True)
    v = v[by_seg]
    lo = (ptr[:-1] + (cnt - 1).clamp_min(0) // 2).clamp_max(n - 1)
    hi = (ptr[:-1] + cnt // 2).clamp_max(n - 1)
    return torch.where(cnt > 0, 0.5 * (v[lo] + v[hi]), nan)


def mmd_statistics(ref_pos, gen_pos, n_atoms, num_ref, num_gen, pairs, pair_ptr, atom_mask=None, kernel_mul=2.0, kernel_num=5,
                   exp_path=0, plan=None):
    """Single / Pair / All distance MMD of every molecule of a ragged set, on the device.

    ref_pos [sum R_g n_g, 3], gen_pos [sum K_g n_g, 3] (device, the layout of conformer_eval.rmsd_matrix); n_atoms, num_ref,
    num_gen: G host integers each; pairs [sum E_g, 2] integers in the evaluated-atom numbering (distance_pairs; host or device,
    read on the host) with pair_ptr [G + 1] host offsets; atom_mask [sum n_g] (device, None = all atoms) keeps the evaluated
    atoms.  exp_path 0: one exponential and squarings when kernel_mul == 2, 1: kernel_num exponentials always.

    Returns a dictionary of device tensors (offsets on the host): "single" fp64 [sum E] = MMD({e}) with "single_off" [G + 1];
    "pair" fp64 = MMD({e, f}), e < f ordered by (e, f), with "pair_off" [G + 1]; "all" fp64 [G]; "stats" fp64 [G, 7] = single
    median, single mean, pair median, pair mean, all, R used, K used; "finite" uint8 [sum (R + K)], 0 for an excluded
    conformer (per molecule its references, then its generated conformers).  ValueError when the sizes do not fit or a molecule
    pools more than MAX_POOLED conformers; nothing is ever truncated."""
    mul, num = _kernel_parameters(kernel_mul, kernel_num)
    if exp_path not in (0, 1):
        raise ValueError("exp_path is 0 or 1")
    if plan is None:
        keep = None if atom_mask is None else (torch.as_tensor(atom_mask).reshape(-1) != 0).cpu().numpy()
        pairs = pairs.cpu().numpy() if torch.is_tensor(pairs) else np.asarray(pairs)
        ptr = pair_ptr.cpu().numpy() if torch.is_tensor(pair_ptr) else np.asarray(list(pair_ptr))
        plan = Plan(n_atoms, num_ref, num_gen, pairs, ptr, keep)
    if tuple(ref_pos.shape) != (int(plan.ref_row[-1]), 3) or tuple(gen_pos.shape) != (int(plan.gen_row[-1]), 3):
        raise ValueError(f"ref_pos {tuple(ref_pos.shape)} / gen_pos {tuple(gen_pos.shape)} do not hold sum R n = "
                         f"{int(plan.ref_row[-1])} / sum K n = {int(plan.gen_row[-1])} rows of 3")
    ref_pos, gen_pos = _f32(ref_pos), _f32(gen_pos)
    dev = ref_pos.device
    mask = None
    if atom_mask is not None:
        if not atom_mask.is_cuda:
            raise _lib.MsdeHipError("moleculesde_amd kernels need tensors on the HIP device (no CPU fallback)")
        mask = (atom_mask.reshape(-1) != 0).to(torch.uint8).contiguous()
    t = plan.upload(dev)
    G, nan = plan.G, float("nan")
    finite = torch.zeros(plan.n_conf, dtype=torch.uint8, device=dev)
    rank = torch.full((plan.n_conf,), -1, dtype=torch.int32, device=dev)
    used = torch.zeros(G, 2, dtype=torch.int32, device=dev)
    # every fp64 output starts as NaN: an entry a kernel failed to write cannot pass for a value
    z = torch.full((max(1, int(plan.z_off[-1])),), nan, dtype=torch.float64, device=dev)
    colsum = torch.full((max(1, plan.n_cols),), nan, dtype=torch.float64, device=dev)
    mmd = torch.full((max(1, plan.n_items),), nan, dtype=torch.float64, device=dev)
    means = torch.full((G, 2), nan, dtype=torch.float64, device=dev)
    all_mmd = torch.full((G,), nan, dtype=torch.float64, device=dev)
    LL, D = ctypes.c_longlong, ctypes.c_double
    _lib.call("msde_conf_dist_table", _p(ref_pos), _p(gen_pos), _p(t["mol"]), G, _p(mask), LL(plan.n_conf), _p(t["pair_ptr"]),
              _p(t["pairs"]), _p(finite), _p(rank), _p(used), _p(z), _stream())
    _lib.call("msde_conf_mmd_subsets", _p(z), _p(t["mol"]), G, _p(t["pair_ptr"]), LL(plan.n_cols), _p(used), _p(t["items"]),
              LL(plan.n_items), _p(t["pairitem_ptr"]), plan.c_max, D(mul), num, int(exp_path), _p(colsum), _p(mmd), _p(means),
              _stream())
    _lib.call("msde_conf_mmd_all", _p(z), _p(t["mol"]), G, _p(t["pair_ptr"]), _p(used), _p(colsum), D(mul), num, int(exp_path),
              _p(all_mmd), _stream())
    single, pair = mmd[:plan.n_cols], mmd[plan.n_cols:plan.n_items]
    stats = torch.stack([_segment_median(single, t["pair_ptr"]), means[:, 0], _segment_median(pair, t["pairitem_ptr"]),
                         means[:, 1], all_mmd, used[:, 0].double(), used[:, 1].double()], dim=1)
    return {"single": single, "single_off": torch.from_numpy(plan.pair_ptr.copy()), "pair": pair,
            "pair_off": torch.from_numpy(plan.pairitem_ptr.copy()), "all": all_mmd, "stats": stats, "finite": finite}


def summarize(stats, num_pairs):
    """The result dictionary from the host copy of stats [G, 7] (numpy, fp64) and the evaluated pairs per molecule."""
    E = np.asarray(num_pairs, dtype=np.int64)
    failed = (stats[:, 5] == 0) | (stats[:, 6] == 0)
    res = {"num_molecules": int(stats.shape[0]), "num_failed": int(failed.sum()),
           "num_without_pairs": int(((E == 0) & ~failed).sum()),
           "per_molecule": {name: stats[:, i].tolist() for i, name in enumerate(STATS)}}
    res["per_molecule"].update(num_ref_used=[int(v) for v in stats[:, 5]], num_gen_used=[int(v) for v in stats[:, 6]],
                               num_pairs=[int(v) for v in E])
    for key, f in (("mean", np.mean), ("median", np.median)):
        res[key] = {}
        for i, name in enumerate(STATS):
            v = stats[:, i][np.isfinite(stats[:, i])]
            res[key][name] = float(f(v)) if v.size else float("nan")
    return res


def evaluate_distance_mmd(records, references=None, heavy_atoms_only=True, max_hops=3, kernel_mul=2.0, kernel_num=5, device=None):
    """Single / Pair / All distance MMD (module docstring) between the reference and the generated conformers of `records` (a
    list from generate_samples_from_testset, or the path of its pickle; references and heavy_atoms_only as in
    conformer_eval.evaluate_conformers).  max_hops bounds the bond-graph distance of an evaluated atom pair (None: all pairs).

    Returns {"num_molecules", "num_failed", "num_without_pairs", "max_hops", "kernel_mul", "kernel_num", "per_molecule":
    {"single_median", "single_mean", "pair_median", "pair_mean", "all", "num_ref_used", "num_gen_used", "num_pairs"} ([G] each),
    "mean": {...}, "median": {...}}: mean and median of each of the five statistics over the molecules where it is finite."""
    if isinstance(records, (str, bytes)) or hasattr(records, "__fspath__"):
        with open(records, "rb") as f:
            records = pickle.load(f)
    records = list(records)
    mul, num = _kernel_parameters(kernel_mul, kernel_num)
    ref, gen, mask, n, R, K = _collect(records, references, heavy_atoms_only)
    pairs = [distance_pairs(rec, heavy_atoms_only, max_hops) for rec in records]
    ptr = _excl([p.shape[0] for p in pairs])
    plan = Plan(n, R, K, np.concatenate(pairs), ptr, None if mask is None else mask.numpy())
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.MsdeHipError("the distance MMD needs a HIP device (no CPU fallback)")
    out = mmd_statistics(ref.to(dev), gen.to(dev), n, R, K, None, None, None if mask is None else mask.to(dev), mul, num,
                         plan=plan)
    res = summarize(out["stats"].cpu().numpy(), plan.E)
    res.update(max_hops=None if max_hops is None else int(max_hops), kernel_mul=mul, kernel_num=num)
    return res


def _parser():
    ap = argparse.ArgumentParser(prog="python -m moleculesde_amd.conformer_mmd",
                                 description="distance-distribution MMD of the conformers in a pickle of "
                                             "generate_samples_from_testset")
    ap.add_argument("samples", help="pickle written by generate_samples_from_testset(out_path=...)")
    ap.add_argument("--references", default=None,
                    help="torch.save'd list with one [R_i, n_i, 3] tensor per record (default: each record's positions)")
    hops = ap.add_mutually_exclusive_group()
    hops.add_argument("--max_hops", type=int, default=3, metavar="N",
                      help="evaluate atom pairs at most N bonds apart (default 3: bonds, angles, torsions)")
    hops.add_argument("--all_pairs", action="store_true", help="evaluate every pair of evaluated atoms")
    ap.add_argument("--all_atoms", action="store_true", help="evaluate on all atoms, not on the heavy atoms only")
    ap.add_argument("--kernel_mul", type=float, default=2.0)
    ap.add_argument("--kernel_num", type=int, default=5)
    ap.add_argument("--per_molecule", action="store_true", help="keep the per-molecule lists in the printed line")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    refs = torch.load(args.references) if args.references else None
    res = evaluate_distance_mmd(args.samples, refs, heavy_atoms_only=not args.all_atoms,
                                max_hops=None if args.all_pairs else args.max_hops, kernel_mul=args.kernel_mul,
                                kernel_num=args.kernel_num)
    if not args.per_molecule:
        res.pop("per_molecule")
    print(json.dumps(_jsonable(res)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
