"""Graph evaluation of the 3D->2D sampler's output on the decode kernels (csrc/graph2d_eval.hip).

sampler_3d2d.node_adj_PC_generation / generate_2d_from_3d return two float tensors per sample: `x [n, num_class_X]`, class
scores around a one-hot element, and `adj [n, n]`, values around `bond type + 1` (the encoding the model trains on:
edge_attr[:, 0] + 1 -- 1 single, 2 double, 3 triple, 4 aromatic, 5 misc; 0 no bond).  This module turns them back into molecular
graphs and compares them with the graph the 3D input came from, for every sample of every molecule of a ragged set in two
launches:

    class of atom i   = argmax_c x[i, c], the lowest index among equal scores
    code of pair i<j  = q = clamp(floor(v + 0.5), 0, max_bond),  v = 0.5 (adj[i, j] + adj[j, i]) in fp64

on the atoms the sampler flags (an atom without a bond is masked like padding and takes part in nothing).  Per sample: atoms
correct, bond existence TP / FP / FN, bond orders correct on the true positives, exact match, connected components and valence
violations of the decoded graph, sum |v - t|; per molecule the means over its K samples of atom accuracy, bond precision, recall,
F1, bond-order accuracy (each of these ratios is 1 where its denominator is 0), exact-match rate, valid rate (finite, one
component, no valence violation), the fraction of unique decoded graphs, best-of-K exact match and the mean |v - t| per pair.
A sample with a NaN or an infinity on a flagged atom or pair is NON-FINITE: it stays in every denominator and adds nothing; a
molecule with no finite sample is counted in `num_failed` and left out of the summary's mean and median -- the conventions of
conformer_eval.evaluate_conformers.  There is no CPU path: the kernels need a HIP device.

    python -m moleculesde_amd.graph2d_eval samples.pkl [--max_bond N] [--no_valence] [--per_molecule]
"""
import argparse
import ctypes
import json
import os
import pickle
import sys
import types

import numpy as np
import torch

from . import _lib
from ._torchabi import _f32, _p, _stream
from .conformer_eval import _jsonable

MOL_WORDS = 8       # int64 per molecule of the table (include/msde_hip.h)
REC_INTS = 9        # int32 per sample record
N_STATS = 11        # fp64 per molecule
N_MAX = 1024        # GE_NMAX of csrc/graph2d_eval.hip
COUNT_NAMES = ("finite", "atoms_correct", "tp", "fp", "fn", "order_correct", "exact", "components", "valence_violations")
STAT_NAMES = ("atom_accuracy", "bond_precision", "bond_recall", "bond_f1", "bond_order_accuracy", "exact_match", "valid",
              "unique", "any_exact", "adj_l1")

# The largest number of bonds (sum of bond orders) an atom of the element may carry in a decoded graph, by atomic number; every
# other element is unchecked.  This table is THIS PROJECT'S CHOICE, not the reference's (which has no evaluation of the 3D->2D
# samples at all): the generated graph carries no formal charges, so the caps are those of the charged forms too -- N 4
# (ammonium), O 3 (oxonium) -- and of the hypervalent ones (P 5, S 6).
DEFAULT_MAX_VALENCE = {1: 1, 5: 4, 6: 4, 7: 4, 8: 3, 9: 1, 14: 4, 15: 5, 16: 6, 17: 1, 35: 1, 53: 1}


def valence_table(max_valence, ncls):
    """max_valence2 [ncls] uint8 of the kernel: the cap in half-bond units by class (class c is atomic number c + 1, the
    featuriser's `GetAtomicNum() - 1`), 0 = unchecked.  max_valence: "default" (DEFAULT_MAX_VALENCE), None (no check: returns
    None) or a dict {atomic number: bonds}."""
    if max_valence is None:
        return None
    table = DEFAULT_MAX_VALENCE if isinstance(max_valence, str) and max_valence == "default" else max_valence
    if not isinstance(table, dict):
        raise ValueError('max_valence must be "default", None or a dict {atomic number: bonds}')
    out = np.zeros(int(ncls), dtype=np.uint8)
    for zn, bonds in table.items():
        zn, bonds = int(zn), int(bonds)
        if zn < 1 or not 1 <= bonds <= 127:
            raise ValueError(f"max_valence: atomic number {zn} with {bonds} bonds is outside Z >= 1, 1 <= bonds <= 127")
        if zn - 1 < ncls:
            out[zn - 1] = 2 * bonds
    return out


class Plan:
    """Host-built table of one launch: `mol` [G, 8] int64 on the device (include/msde_hip.h) and its columns on the host:
    sample k of molecule g owns record samp_off[g] + k and the sig_len[g] signature bytes at sig_off[g] + k sig_len[g]."""

    def __init__(self, n_atoms, num_gen, ncls, device):
        n = np.asarray(list(n_atoms), dtype=np.int64).reshape(-1)
        K = np.asarray(list(num_gen), dtype=np.int64).reshape(-1)
        if len(n) != len(K) or len(n) == 0:
            raise ValueError("n_atoms and num_gen must be non-empty and of equal length")
        if (n < 1).any() or (K < 1).any():
            raise ValueError("every molecule needs at least one atom and one generated sample")
        ncls = int(ncls)
        if not 1 <= ncls <= 256:
            raise ValueError(f"ncls = {ncls} is outside [1, 256] (a decoded class is one byte)")

        def excl(v):
            return np.concatenate([[0], np.cumsum(v)]).astype(np.int64)

        self.G, self.n, self.K, self.ncls = len(n), n, K, ncls
        self.sig_len = n + n * (n - 1) // 2
        self.x_off, self.adj_off = excl(K * n * ncls), excl(K * n * n)
        self.atom_off, self.tgt_off = excl(n), excl(n * n)
        self.samp_off, self.sig_off = excl(K), excl(K * self.sig_len)
        self.n_samples, self.n_max = int(self.samp_off[-1]), int(n.max())
        mol = np.stack([n, K, self.x_off[:-1], self.adj_off[:-1], self.atom_off[:-1], self.tgt_off[:-1], self.samp_off[:-1],
                        self.sig_off[:-1]], axis=1)
        self.mol = torch.from_numpy(np.ascontiguousarray(mol)).to(device)


def _dev(t, dtype, what, numel):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.MsdeHipError("moleculesde_amd kernels need tensors on the HIP device (no CPU fallback)")
    if t.numel() != numel:
        raise ValueError(f"{what} has {t.numel()} entries, the launch needs {numel}")
    return t.reshape(-1).to(dtype).contiguous()


def decode(x_gen, adj_gen, z, adj_tgt, atom_flag, n_atoms, num_gen, max_bond=4, max_valence2=None, ncls=None, plan=None):
    """msde_graph2d_decode on a ragged set (device tensors, flat or of any shape with the right number of elements):
    x_gen [sum K n ncls] and adj_gen [sum K n n] fp32, sample-major within a molecule; z [sum n] target classes; adj_tgt
    [sum n n] target codes 0..5; atom_flag [sum n] (non-zero = evaluated); n_atoms, num_gen: G host integers each;
    max_valence2: [ncls] uint8 (host or device; valence_table) or None.  ncls defaults to x_gen.numel() / sum K n.
    Returns a namespace: sig (uint8, plan.sig_off / plan.sig_len), counts [S, 9] int32 (COUNT_NAMES), adj_l1 [S] fp64,
    atom_flag (the uint8 tensor the kernels read), plan."""
    max_bond = int(max_bond)
    if not 1 <= max_bond <= 5:
        raise ValueError(f"max_bond = {max_bond} is outside [1, 5]")
    if plan is None:
        n = np.asarray(list(n_atoms), dtype=np.int64).reshape(-1)
        K = np.asarray(list(num_gen), dtype=np.int64).reshape(-1)
        rows = int((n * K).sum()) if len(n) == len(K) and len(n) else 0
        if ncls is None:
            if not torch.is_tensor(x_gen) or rows == 0 or x_gen.numel() % rows:
                raise ValueError("x_gen does not hold a whole number of classes for sum K n rows")
            ncls = x_gen.numel() // rows
        plan = Plan(n, K, ncls, x_gen.device if torch.is_tensor(x_gen) else "cuda")
    if plan.n_max > N_MAX:
        raise _lib.MsdeHipError(f"a molecule of {plan.n_max} atoms: the decode kernel holds at most {N_MAX} (labels in LDS)")
    if not torch.is_tensor(x_gen) or not x_gen.is_cuda:
        raise _lib.MsdeHipError("moleculesde_amd kernels need tensors on the HIP device (no CPU fallback)")
    dev = x_gen.device
    n_atoms_all, S = int(plan.atom_off[-1]), plan.n_samples
    if x_gen.numel() != int(plan.x_off[-1]) or adj_gen.numel() != int(plan.adj_off[-1]):
        raise ValueError(f"x_gen ({x_gen.numel()}) / adj_gen ({adj_gen.numel()}) do not hold sum K n ncls = {int(plan.x_off[-1])} / "
                         f"sum K n n = {int(plan.adj_off[-1])} elements")
    x_gen, adj_gen = _f32(x_gen).reshape(-1), _f32(adj_gen).reshape(-1)
    z = _dev(z, torch.int32, "z", n_atoms_all)
    adj_tgt = _dev(adj_tgt, torch.uint8, "adj_tgt", int(plan.tgt_off[-1]))
    flag = _dev(atom_flag != 0 if torch.is_tensor(atom_flag) else atom_flag, torch.uint8, "atom_flag", n_atoms_all)
    mv = None
    if max_valence2 is not None:
        mv = torch.as_tensor(max_valence2).reshape(-1).to(torch.uint8).to(dev).contiguous()
        if mv.numel() != plan.ncls:
            raise ValueError(f"max_valence2 has {mv.numel()} entries for {plan.ncls} classes")
    sig = torch.empty(int(plan.sig_off[-1]), dtype=torch.uint8, device=dev)
    counts = torch.empty(S, REC_INTS, dtype=torch.int32, device=dev)
    adj_l1 = torch.empty(S, dtype=torch.float64, device=dev)
    _lib.call("msde_graph2d_decode", _p(x_gen), _p(adj_gen), _p(z), _p(adj_tgt), _p(flag), _p(mv), _p(plan.mol), plan.G,
              ctypes.c_longlong(S), plan.n_max, plan.ncls, max_bond, _p(sig), _p(counts), _p(adj_l1), _stream())
    return types.SimpleNamespace(sig=sig, counts=counts, adj_l1=adj_l1, atom_flag=flag, plan=plan)


def summary(dec):
    """msde_graph2d_summary on the namespace decode returned: (stats [G, 11] fp64 -- STAT_NAMES, then the number of finite
    samples -- and first [S] uint8: 1 where a finite sample's signature equals that of no earlier finite sample of its
    molecule), both on the device."""
    plan, dev = dec.plan, dec.sig.device
    first = torch.empty(plan.n_samples, dtype=torch.uint8, device=dev)
    stats = torch.empty(plan.G, N_STATS, dtype=torch.float64, device=dev)
    _lib.call("msde_graph2d_summary", _p(dec.sig), _p(dec.counts), _p(dec.adj_l1), _p(dec.atom_flag), _p(plan.mol), plan.G,
              _p(first), _p(stats), _stream())
    return stats, first


def graphs_from_signatures(sig, plan):
    """Host: the signatures (uint8 numpy, plan.sig_off layout) as per-molecule lists of per-sample MolData: x [n, 9] int64 with
    x[:, 0] the class and zeros elsewhere, edge_index [2, 2 E] in both directions sorted by (source, target), edge_attr
    [2 E, 3] with edge_attr[:, 0] = q - 1 and zeros elsewhere."""
    from .batch import MolData
    out = []
    for g in range(plan.G):
        n, L = int(plan.n[g]), int(plan.sig_len[g])
        iu, ju = np.triu_indices(n, 1)                       # row-major: the kernel's order
        mol = []
        for k in range(int(plan.K[g])):
            s = sig[int(plan.sig_off[g]) + k * L:int(plan.sig_off[g]) + (k + 1) * L]
            code = np.zeros((n, n), dtype=np.int64)
            code[iu, ju] = s[n:]
            code = code + code.T
            src, dst = np.nonzero(code)                      # sorted by (source, target)
            x = np.zeros((n, 9), dtype=np.int64)
            x[:, 0] = s[:n]
            ea = np.zeros((src.size, 3), dtype=np.int64)
            ea[:, 0] = code[src, dst] - 1
            mol.append(MolData(x=torch.from_numpy(x), edge_index=torch.from_numpy(np.stack([src, dst]).astype(np.int64)),
                               edge_attr=torch.from_numpy(ea)))
        out.append(mol)
    return out


def decode_graphs(x_gen, adj_gen, n_atoms, num_gen, atom_flag=None, max_bond=4):
    """The decoded graphs of a ragged set of samples (device tensors in decode's layout; atom_flag [sum n] or None = every
    atom): a list with one entry per molecule, each a list of K MolData (graphs_from_signatures) that can go wherever a
    MolData goes.  A non-finite sample decodes to all-zero classes and no bonds."""
    n = np.asarray(list(n_atoms), dtype=np.int64).reshape(-1)
    if not torch.is_tensor(x_gen) or not x_gen.is_cuda:
        raise _lib.MsdeHipError("moleculesde_amd kernels need tensors on the HIP device (no CPU fallback)")
    dev = x_gen.device
    atoms = int(n.sum())
    flag = torch.ones(atoms, dtype=torch.uint8, device=dev) if atom_flag is None else atom_flag
    dec = decode(x_gen, adj_gen, torch.zeros(atoms, dtype=torch.int32, device=dev),
                 torch.zeros(int((n * n).sum()), dtype=torch.uint8, device=dev), flag, n, num_gen, max_bond=max_bond)
    return graphs_from_signatures(dec.sig.cpu().numpy(), dec.plan)


def target_of(rec, i=0):
    """Host: (z [n] int64, adj_tgt [n, n] uint8, atom_flag [n] uint8) of a record's true graph: z = x[:, 0], the code of a
    bond = edge_attr[:, 0] + 1 (read as undirected), the flag = the atom has a bond (the sampler's node flags)."""
    x = torch.as_tensor(rec.x).cpu()
    z = (x if x.dim() == 1 else x[:, 0]).long().numpy()
    n = z.shape[0]
    ei, ea = torch.as_tensor(rec.edge_index).cpu().numpy(), torch.as_tensor(rec.edge_attr).cpu().numpy()
    if ei.ndim != 2 or ei.shape[0] != 2 or ea.shape[0] != ei.shape[1]:
        raise ValueError(f"record {i}: edge_index {ei.shape} / edge_attr {ea.shape} are not [2, E] / [E, ...]")
    bond = (ea if ea.ndim == 1 else ea[:, 0]).astype(np.int64)
    if ei.size and (ei.min() < 0 or ei.max() >= n):
        raise ValueError(f"record {i}: edge_index names an atom outside [0, {n})")
    if bond.size and (bond.min() < 0 or bond.max() > 4):
        raise ValueError(f"record {i}: bond types must lie in [0, 4] (codes 1..5)")
    adj = np.zeros((n, n), dtype=np.uint8)
    keep = ei[0] != ei[1]
    adj[ei[0][keep], ei[1][keep]] = bond[keep] + 1
    adj = np.maximum(adj, adj.T)
    return z, adj, (adj.sum(1) > 0).astype(np.uint8)


def _collect(records):
    """Host-side checks and packing of evaluate_graphs: flat CPU tensors (x_gen, adj_gen, z, adj_tgt, flag), n, K, ncls."""
    if len(records) == 0:
        raise ValueError("no records")
    xs, adjs, zs, tgts, flags, n_l, K_l, ncls = [], [], [], [], [], [], [], None
    for i, rec in enumerate(records):
        z, tgt, flag = target_of(rec, i)
        n = z.shape[0]
        xg = torch.as_tensor(rec.x_gen, dtype=torch.float32).cpu()
        ag = torch.as_tensor(rec.adj_gen, dtype=torch.float32).cpu()
        if xg.dim() != 3 or xg.size(0) < 1 or xg.size(1) != n or tuple(ag.shape) != (xg.size(0), n, n):
            raise ValueError(f"record {i}: x_gen {tuple(xg.shape)} / adj_gen {tuple(ag.shape)} are not [K, {n}, ncls] / [K, {n}, {n}]")
        if ncls is None:
            ncls = int(xg.size(2))
        if int(xg.size(2)) != ncls:
            raise ValueError(f"record {i}: {int(xg.size(2))} classes, the records before it have {ncls}")
        if z.min() < 0 or z.max() >= ncls:
            raise ValueError(f"record {i}: an atom class outside [0, {ncls})")
        if int(flag.sum()) == 0:
            raise ValueError(f"record {i}: no flagged atom (the molecule has no bond: the sampler masks all of it)")
        xs.append(xg.reshape(-1)); adjs.append(ag.reshape(-1))
        zs.append(torch.from_numpy(z.astype(np.int32))); tgts.append(torch.from_numpy(tgt.reshape(-1)))
        flags.append(torch.from_numpy(flag)); n_l.append(n); K_l.append(int(xg.size(0)))
    return (torch.cat(xs), torch.cat(adjs), torch.cat(zs), torch.cat(tgts), torch.cat(flags)), n_l, K_l, ncls


def summarize(stats):
    """The result dictionary from the host copy of the kernel's stats [G, 11] (numpy, fp64)."""
    fin = stats[:, N_STATS - 1]
    ok = fin > 0
    res = {"num_molecules": int(stats.shape[0]), "num_failed": int((~ok).sum()),
           "per_molecule": {name: stats[:, j].tolist() for j, name in enumerate(STAT_NAMES)}}
    res["per_molecule"]["num_finite"] = [int(v) for v in fin]
    for key, f in (("mean", np.mean), ("median", np.median)):
        res[key] = {name: float(f(stats[ok, j])) if ok.any() else float("nan") for j, name in enumerate(STAT_NAMES)}
    return res


def evaluate_graphs(records, max_bond=4, max_valence="default", device=None):
    """The figures of the module docstring for `records` (a list, or the path of the pickle generate_graphs_from_testset
    writes): one entry per molecule carrying the true graph `x`, `edge_index`, `edge_attr` and the samples `x_gen [K, n, ncls]`,
    `adj_gen [K, n, n]` (record_from_sample).  max_valence: "default" = DEFAULT_MAX_VALENCE -- this project's table, not the
    reference's: H 1, B 4, C 4, N 4, O 3, F 1, Si 4, P 5, S 6, Cl 1, Br 1, I 1 bonds, the caps of the charged forms since a
    decoded graph carries no formal charge, every other element unchecked --, a dict {atomic number: bonds}, or None (no check).

    Returns {"num_molecules", "num_failed", "max_bond", "per_molecule": {name: [G] for name in STAT_NAMES, "num_finite": [G]},
    "mean": {...}, "median": {...}}; mean and median over the molecules with at least one finite sample (NaN when there is
    none).  A molecule with no flagged atom (no bond) raises ValueError."""
    if isinstance(records, (str, bytes)) or hasattr(records, "__fspath__"):
        with open(records, "rb") as f:
            records = pickle.load(f)
    max_bond = int(max_bond)
    if not 1 <= max_bond <= 5:
        raise ValueError(f"max_bond = {max_bond} is outside [1, 5]")
    packed, n, K, ncls = _collect(list(records))
    mv = valence_table(max_valence, ncls)
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.MsdeHipError("graph evaluation needs a HIP device (no CPU fallback)")
    x_gen, adj_gen, z, tgt, flag = (t.to(dev) for t in packed)
    dec = decode(x_gen, adj_gen, z, tgt, flag, n, K, max_bond=max_bond, max_valence2=mv, ncls=ncls)
    stats, _ = summary(dec)
    res = summarize(stats.cpu().numpy())
    res["max_bond"] = max_bond
    return res


def record_from_sample(data, x, adj):
    """A record of evaluate_graphs from one molecule (a MolData) and the padded output of generate_2d_from_3d for it,
    x [K, Nm, ncls] and adj [K, Nm, Nm] with Nm >= n: the molecule's own tensors plus x_gen [K, n, ncls], adj_gen [K, n, n] (CPU)."""
    from .batch import MolData
    n = int(data.num_nodes)
    if x.dim() != 3 or adj.dim() != 3 or x.size(0) != adj.size(0) or x.size(1) < n or adj.size(1) < n or adj.size(2) < n:
        raise ValueError(f"x {tuple(x.shape)} / adj {tuple(adj.shape)} are not [K, Nm, ncls] / [K, Nm, Nm] with Nm >= {n}")
    rec = MolData(**{key: getattr(data, key).clone().detach() for key in data.keys()})
    rec.x_gen = x[:, :n].detach().float().cpu().clone()
    rec.adj_gen = adj[:, :n, :n].detach().float().cpu().clone()
    return rec


def launch_chunks(start, end, num_molecules, molecules_per_launch):
    """The launches of generate_graphs_from_testset: the molecule indices of molecules[start:end] (clamped to the set) cut
    into consecutive chunks of molecules_per_launch, the last one possibly shorter."""
    per = int(molecules_per_launch)
    if per < 1:
        raise ValueError("molecules_per_launch must be at least 1")
    start, end = max(0, int(start)), min(int(end), int(num_molecules))
    return [list(range(lo, min(lo + per, end))) for lo in range(start, end, per)]


def generate_graphs_from_testset(molecules, model_3d, sde_model, num_repeat=10, start=0, end=100, noise_seed=None, out_path=None,
                                 molecules_per_launch=1, **kw):
    """The 3D->2D inference script's test-set loop: num_repeat samples for every molecule of molecules[start:end].
    molecules_per_launch=1 (the default): one sampler_3d2d.generate_2d_from_3d call per molecule.  molecules_per_launch > 1:
    that many molecules share each reverse-SDE trajectory (sampler_3d2d.generate_2d_from_3d_grouped on
    csrc/dense_pc_grouped.hip: per-molecule corrector statistics and noise seeds, so a molecule's samples do not depend on the
    chunking up to the score networks' rounding), and every record carries `diverged`: True where the
    trajectory left the finite numbers for that molecule (the others of its launch are not affected).  Either way a
    molecule's noise seed is sampler.group_seed(noise_seed, its index in `molecules`): its samples do not depend on start /
    end; noise_seed=None draws one from torch's CPU generator.  kw goes to node_adj_PC_generation[_grouped] (num_steps,
    max_iters, snr, ...).  Returns the list of records (record_from_sample); out_path: a directory (the pickle is written into
    it under the name "3D_to_2D_{start}_{end}_repeat_{num_repeat}") or a file path."""
    from .sampler import group_seed
    from .sampler_3d2d import generate_2d_from_3d, generate_2d_from_3d_grouped
    if num_repeat < 1:
        raise ValueError("num_repeat must be at least 1")
    chunks = launch_chunks(start, end, len(molecules), molecules_per_launch)
    name = "3D_to_2D_{}_{}_repeat_{}".format(start, end, num_repeat)
    start, end = max(0, int(start)), min(int(end), len(molecules))
    if noise_seed is None:
        noise_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    records = []
    if int(molecules_per_launch) == 1:
        for i in range(start, end):
            x, adj, _, _ = generate_2d_from_3d(model_3d, sde_model, molecules[i], num_repeat=num_repeat,
                                               noise_seed=group_seed(noise_seed, i), **kw)
            records.append(record_from_sample(molecules[i], x, adj))
    else:
        for idx in chunks:
            samples, bad = generate_2d_from_3d_grouped(model_3d, sde_model, [molecules[i] for i in idx], num_repeat,
                                                       [group_seed(noise_seed, i) for i in idx], **kw)
            bad = bad.cpu().tolist()
            for k, i in enumerate(idx):
                rec = record_from_sample(molecules[i], samples[k][0], samples[k][1])
                rec.diverged = bool(bad[k])
                records.append(rec)
    if out_path is not None:
        path = os.path.join(out_path, name) if os.path.isdir(out_path) else out_path
        with open(path, "wb") as fout:
            pickle.dump(records, fout)
    return records


def _parser():
    ap = argparse.ArgumentParser(prog="python -m moleculesde_amd.graph2d_eval",
                                 description="graph reconstruction figures of the samples in a pickle of "
                                             "generate_graphs_from_testset")
    ap.add_argument("samples", help="pickle written by generate_graphs_from_testset(out_path=...)")
    ap.add_argument("--max_bond", type=int, default=4, metavar="N", help="the largest bond code decoded (1..5; 5 admits 'misc')")
    ap.add_argument("--no_valence", action="store_true", help="skip the valence check of the valid rate")
    ap.add_argument("--per_molecule", action="store_true", help="keep the per-molecule lists in the printed line")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    res = evaluate_graphs(args.samples, max_bond=args.max_bond, max_valence=None if args.no_valence else "default")
    if not args.per_molecule:
        res.pop("per_molecule")
    print(json.dumps(_jsonable(res)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
