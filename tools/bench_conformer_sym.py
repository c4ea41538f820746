"""Time the symmetry-aware conformer RMSD (msde_conf_rmsd_matrix_sym) on the workload of tools/bench_conformer_eval.py:
`--molecules` molecules of 20 to 60 atoms, `--refs` reference and `--gens` generated conformers each (default 200 x 50 x 100),
all atoms, with SYNTHETIC permutation tables of P rows per molecule (the identity and P - 1 random permutations), P in
`--perms` (default 1 2 12 72).  In ONE process, on the same inputs, per P:
  (a) sym_ms      the new launch (preparation + symmetric kernel), tables and buffers already on the device;
  (b) looped_ms   what the tree could do before: P calls of rmsd_matrix on permuted copies of the references (a device gather
                  by a prebuilt row index) with a running torch.minimum;
  (c) plain_ms    msde_conf_rmsd_matrix alone (once: it has no P).
Device events around `--launches` back-to-back launches ((b): `--looped_launches`), `--rounds` rounds after a warm-up round,
the three alternating within a round; median and min / max over rounds.  (a) and (b) are compared value by value.
Then evaluate_conformers from host tensors, symmetry=False and symmetry=True, on records that carry synthetic molecular graphs
(synthetic.make_molecule: random labels, so most groups are trivial) -- host clock around calls that end in a synchronise;
the host enumeration of the groups (conformer_eval._groups) is timed on its own and is part of the symmetry=True figure."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_conformer_eval import THRESHOLDS, event_ms, host_ms, put, workload  # noqa: E402
from moleculesde_amd import _lib, conformer_eval as ce  # noqa: E402
from moleculesde_amd._torchabi import _p, _stream  # noqa: E402
from moleculesde_amd.batch import MolData  # noqa: E402
from moleculesde_amd.synthetic import make_molecule  # noqa: E402


def tables(n, P, rng):
    out = []
    for ng in n:
        t = np.tile(np.arange(ng, dtype=np.int32), (P, 1))
        for p in range(1, P):
            t[p] = rng.permutation(ng)
        out.append(t)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--molecules", type=int, default=200)
    ap.add_argument("--refs", type=int, default=50)
    ap.add_argument("--gens", type=int, default=100)
    ap.add_argument("--perms", type=int, nargs="+", default=[1, 2, 12, 72])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--looped_launches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    G, R, K = a.molecules, a.refs, a.gens
    n, refs, gens = workload(G, R, K)
    pairs = G * R * K
    ref_h = torch.from_numpy(np.concatenate([r.reshape(-1, 3) for r in refs]))
    gen_h = torch.from_numpy(np.concatenate([g.reshape(-1, 3) for g in gens]))
    ref_d, gen_d = ref_h.to(dev), gen_h.to(dev)
    plan = ce.Plan(n, [R] * G, [K] * G, dev)
    prep = torch.empty(plan.n_conf * ce.REC_DOUBLES, dtype=torch.float64, device=dev)
    out_plain = torch.empty(pairs, dtype=torch.float64, device=dev)
    out_sym = torch.empty(pairs, dtype=torch.float64, device=dev)
    lds_atoms = min(max(n), ce.LDS_ATOMS)
    base = {"what": "conformer_sym", "molecules": G, "refs": R, "gens": K, "atoms_min_max": [min(n), max(n)], "pairs": pairs,
            "tiles": plan.n_tiles, "lds_atoms": lds_atoms, "launches": a.launches, "looped_launches": a.looped_launches,
            "rounds": a.rounds}

    def k_plain():
        _lib.call("msde_conf_rmsd_matrix", _p(ref_d), _p(gen_d), _p(plan.mol), G, _p(plan.tiles), ctypes.c_longlong(plan.n_tiles),
                  _p(None), ctypes.c_longlong(plan.n_conf), _p(prep), _p(out_plain), _stream())

    lines = []
    rng = np.random.default_rng(1)
    for P in a.perms:
        tabs = tables(n, P, rng)
        sym_h, perms_h = ce._permutation_tables(tabs, np.asarray(n), None)
        sym_d, perms_d = torch.from_numpy(sym_h).to(dev), torch.from_numpy(perms_h).to(dev)
        # (b): row index of the permuted copy p of the references, ref_p[r, a] = ref[r, tabs[p][a]]
        idx = []
        for p in range(P):
            rows = [plan.ref_row[g] + (np.arange(R)[:, None] * n[g] + tabs[g][p][None, :]).reshape(-1) for g in range(G)]
            idx.append(torch.from_numpy(np.concatenate(rows).astype(np.int64)).to(dev))

        def k_sym():
            _lib.call("msde_conf_rmsd_matrix_sym", _p(ref_d), _p(gen_d), _p(plan.mol), G, _p(plan.tiles),
                      ctypes.c_longlong(plan.n_tiles), _p(None), ctypes.c_longlong(plan.n_conf), _p(sym_d), _p(perms_d), lds_atoms,
                      _p(prep), _p(out_sym), _stream())

        def k_looped():
            best = None
            for p in range(P):
                m, _ = ce.rmsd_matrix(ref_d[idx[p]], gen_d, n, [R] * G, [K] * G, plan=plan)
                best = m if best is None else torch.minimum(best, m)
            return best

        runs = (("sym_ms", k_sym, a.launches), ("looped_ms", k_looped, a.looped_launches), ("plain_ms", k_plain, a.launches))
        ts = {name: [] for name, _, _ in runs}
        for rnd in range(a.rounds + 1):                       # round 0 warms up
            for name, fn, launches in runs:
                t = event_ms(fn, launches)
                if rnd:
                    ts[name].append(t)
        rec = dict(base, permutations=P)
        for name, _, _ in runs:
            put(rec, name, ts[name])
        rec["looped_over_sym"] = round(rec["looped_ms"] / rec["sym_ms"], 2)
        rec["sym_over_plain"] = round(rec["sym_ms"] / rec["plain_ms"], 2)
        rec["alignments_per_us"] = round(pairs * P / (rec["sym_ms"] * 1e3), 1)
        k_sym()
        rec["max_abs_diff_sym_vs_looped"] = float("%.3g" % (out_sym - k_looped()).abs().max().item())
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    # evaluate_conformers from host tensors, on records with graphs
    rng = np.random.default_rng(2)
    recs = []
    for g in range(G):
        m = make_molecule(rng, n[g])
        recs.append(MolData(x=m.x, edge_index=m.edge_index, edge_attr=m.edge_attr, positions=torch.from_numpy(refs[g][0]),
                            pos_gen=torch.from_numpy(gens[g].reshape(-1, 3)), num_pos_gen=torch.tensor([K]), finite=True))
    refs_t = [torch.from_numpy(r) for r in refs]
    rec = dict(base, what="conformer_sym_evaluate", repeats=a.repeats)
    ts = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        groups, cut = ce._groups(recs, False, 1024)
        ts.append((time.perf_counter() - t) * 1e3)
    put(rec, "enumeration_ms", ts, 3)
    counts = [int(p.shape[0]) for p in groups]
    rec["groups"] = {"trivial": sum(c == 1 for c in counts), "max": max(counts), "total_permutations": sum(counts), "truncated": cut}
    for name, symmetry in (("evaluate_plain_ms", False), ("evaluate_symmetry_ms", True)):
        put(rec, name, host_ms(lambda: ce.evaluate_conformers(recs, refs_t, THRESHOLDS, heavy_atoms_only=False, device=dev,
                                                              symmetry=symmetry), a.repeats), 3)
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
