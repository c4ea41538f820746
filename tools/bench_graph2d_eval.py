"""Time the graph evaluation of the 3D->2D samples (moleculesde_amd/graph2d_eval.py) on a synthetic workload: `--molecules`
molecules of 10 to 32 atoms with `--samples` samples each (default 200 x 10), 119 classes, the default valence table.  In ONE
process, on the same inputs:
  (a) decode_kernel   msde_graph2d_decode alone, table and buffers already on the device;
  (b) summary_kernel  msde_graph2d_summary alone on its outputs;
  (c) device_path     both launches from packed HOST tensors: table, uploads, kernels, the stats back on the host;
  (d) evaluate        evaluate_graphs(records): (c) plus the host packing of the records (targets from edge lists);
  (e) torch_ops       the same evaluation written with torch ops on the device, on tensors padded to the largest molecule and
                      already resident: argmax, fp64 symmetrisation and rounding, masked counts, label propagation until a
                      host-side check sees no change, a K x K signature comparison per molecule, the means; stats back on the host.
(a) and (b): device events around `--launches` back-to-back launches, `--rounds` rounds after a warm-up round, median and
min / max over rounds.  (c) to (e): a host clock around calls that end in a synchronise, median and min / max over `--repeats`
calls after one warm-up call.  Also reported: how many of the torch version's integer counts differ from the kernels' and the
largest difference of the per-molecule figures.  The arrays are some tens of MB: no bandwidth figure is derived."""
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
from moleculesde_amd import _lib, graph2d_eval as ge  # noqa: E402
from moleculesde_amd._torchabi import _p, _stream  # noqa: E402
from moleculesde_amd.batch import MolData  # noqa: E402

NCLS, MAX_BOND = 119, 4
HALF = [0, 2, 4, 6, 3, 2]


def workload(G, K, seed=0):
    """Records of evaluate_graphs: random trees with a ring closure or two, organic elements, bond types 0..3; samples = one-hot
    scores + N(0, 0.15) and codes + U(-0.45, 0.45) with a larger error on about one sample in four, symmetric (the fused
    sampler's state is): exact, wrong, disconnected and over-bonded samples all occur."""
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(G):
        n = int(rng.integers(10, 33))
        pairs = [(int(rng.integers(max(0, i - 3), i)), i) for i in range(1, n)]
        for _ in range(2):
            a, b = sorted(int(v) for v in rng.integers(0, n, size=2))
            if a != b and (a, b) not in pairs:
                pairs.append((a, b))
        tgt = np.zeros((n, n), dtype=np.float32)
        src, dst, attr = [], [], []
        for a, b in pairs:
            t = int(rng.choice([0, 0, 0, 1, 3]))
            tgt[a, b] = tgt[b, a] = t + 1
            src += [a, b]; dst += [b, a]; attr += [[t, 0, 0]] * 2
        x = np.zeros((n, 9), dtype=np.int64)
        x[:, 0] = rng.choice([5, 5, 5, 6, 7, 15], size=n)
        xg = np.zeros((K, n, NCLS), dtype=np.float32)
        xg[:, np.arange(n), x[:, 0]] = 1.0
        xg += 0.15 * rng.normal(size=xg.shape).astype(np.float32)
        noise = rng.uniform(-0.45, 0.45, size=(K, n, n)) + (rng.random((K, n, n)) < 0.5 / n ** 2) * rng.uniform(-1, 1, size=(K, n, n))
        noise = np.triu(noise, 1)
        ag = (tgt[None] + noise + noise.transpose(0, 2, 1)).astype(np.float32)
        recs.append(MolData(x=torch.from_numpy(x), edge_index=torch.tensor([src, dst], dtype=torch.long),
                            edge_attr=torch.tensor(attr, dtype=torch.long), x_gen=torch.from_numpy(xg), adj_gen=torch.from_numpy(ag)))
    return recs


def padded(recs, K, dev):
    """The torch version's inputs, resident: x [S, Nm, ncls], adj [S, Nm, Nm], z [S, Nm], tgt [S, Nm, Nm], flag [S, Nm]."""
    Nm, G = max(r.num_nodes for r in recs), len(recs)
    xp, ap = torch.zeros(G, K, Nm, NCLS), torch.zeros(G, K, Nm, Nm)
    zp, tp, fl = torch.zeros(G, Nm, dtype=torch.long), torch.zeros(G, Nm, Nm, dtype=torch.long), torch.zeros(G, Nm, dtype=torch.bool)
    for g, r in enumerate(recs):
        n = r.num_nodes
        z, tgt, flag = ge.target_of(r)
        xp[g, :, :n], ap[g, :, :n, :n] = r.x_gen, r.adj_gen
        zp[g, :n], tp[g, :n, :n], fl[g, :n] = torch.from_numpy(z), torch.from_numpy(tgt.astype(np.int64)), torch.from_numpy(flag != 0)
    rep = lambda t: t[:, None].expand(G, K, *t.shape[1:]).reshape(G * K, *t.shape[1:])
    return [t.to(dev).contiguous() for t in (xp.reshape(G * K, Nm, NCLS), ap.reshape(G * K, Nm, Nm), rep(zp), rep(tp), rep(fl))]


def torch_eval(xp, ap, zp, tp, fl, mv2, G, K):
    """(counts [S, 9] int64, stats [G, 11] fp64 on the host) from torch ops on the device."""
    S, Nm = fl.shape
    dev = fl.device
    idx = torch.arange(Nm, device=dev)
    pair = fl[:, :, None] & fl[:, None, :] & (idx[:, None] != idx[None, :])
    up = pair & (idx[:, None] < idx[None, :])
    fin = (torch.isfinite(xp) | ~fl[:, :, None]).all(2).all(1) & (torch.isfinite(ap) | ~pair).all(2).all(1)
    cls = xp.argmax(-1)
    v = 0.5 * (ap.double() + ap.double().transpose(1, 2))
    q = torch.floor(v + 0.5).clamp(0, MAX_BOND).long() * pair
    cnt = lambda m: (m & up).sum((1, 2))
    tpc, fpc, tb = cnt((q > 0) & (tp > 0)), cnt((q > 0) & (tp == 0)), cnt(tp > 0)
    ordc, ne = cnt((tp > 0) & (q == tp)), cnt(q != tp)
    atoms, nf = ((cls == zp) & fl).sum(1), fl.sum(1)
    exact = (atoms == nf) & (ne == 0)
    half = torch.tensor(HALF, device=dev)
    cap = mv2[cls]
    viol = (fl & (cap > 0) & (half[q].sum(2) > cap)).sum(1)
    lab = idx[None].expand(S, Nm).contiguous()
    bonded = q > 0
    while True:
        new = torch.minimum(lab, torch.where(bonded, lab[:, None, :], Nm).min(2).values)
        if torch.equal(new, lab):
            break
        lab = new
    comps = (fl & (lab == idx[None])).sum(1)
    l1 = ((v - tp).abs() * up).sum((1, 2))
    sig = torch.cat([cls * fl, q.reshape(S, -1)], 1).view(G, K, -1)
    same = (sig[:, :, None, :] == sig[:, None, :, :]).all(-1)
    finm = fin.view(G, K)
    earlier = torch.tril(torch.ones(K, K, dtype=torch.bool, device=dev), -1)[None] & finm[:, None, :]
    first = finm & ~(same & earlier).any(2)
    one = torch.ones((), dtype=torch.float64, device=dev)
    ratio = lambda a, b: torch.where(b > 0, a.double() / b.clamp_min(1).double(), one)
    per = torch.stack([atoms.double() / nf.double(), ratio(tpc, tpc + fpc), ratio(tpc, tb), ratio(2 * tpc, tpc + fpc + tb),
                       ratio(ordc, tpc), exact.double(), ((comps == 1) & (viol == 0)).double()], 1) * fin[:, None]
    pairs = (nf * (nf - 1) // 2).view(G, K)[:, 0].clamp_min(1).double()
    nfin = finm.sum(1).double()
    stats = torch.cat([per.view(G, K, -1).mean(1), first.double().mean(1, keepdim=True),
                       (exact & fin).view(G, K).any(1, keepdim=True).double(),
                       ((l1 * fin).view(G, K).sum(1) / nfin / pairs)[:, None], nfin[:, None]], 1)
    z0 = torch.zeros_like(tpc)
    counts = torch.stack([fin.long(), atoms, tpc, fpc, tb - tpc, ordc, exact.long(), comps, viol], 1) * fin[:, None] + \
        torch.stack([z0, z0, z0, z0, tb, z0, z0, z0, z0], 1) * ~fin[:, None]
    return counts.cpu(), stats.cpu()


def host_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def event_ms(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def put(rec, key, ts, digits=4):
    rec[key] = round(statistics.median(ts), digits)
    rec[key + "_min_max"] = [round(min(ts), digits), round(max(ts), digits)]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default="")
    p.add_argument("--molecules", type=int, default=200)
    p.add_argument("--samples", type=int, default=10)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    a = p.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    G, K = a.molecules, a.samples
    recs = workload(G, K)
    packed, n, Ks, ncls = ge._collect(recs)
    mv = ge.valence_table("default", ncls)
    rec = {"what": "graph2d_eval", "molecules": G, "samples": K, "atoms_min_max": [min(n), max(n)], "classes": ncls,
           "input_MB": round(sum(t.numel() * t.element_size() for t in packed) / 1e6, 2), "launches": a.launches,
           "rounds": a.rounds, "repeats": a.repeats}

    # (a), (b): the kernels alone
    x_d, adj_d, z_d, tgt_d, flag_d = (t.to(dev) for t in packed)
    dec = ge.decode(x_d, adj_d, z_d, tgt_d, flag_d, n, Ks, max_bond=MAX_BOND, max_valence2=mv, ncls=ncls)
    plan, mv_d = dec.plan, torch.from_numpy(mv).to(dev)
    first = torch.empty(plan.n_samples, dtype=torch.uint8, device=dev)
    stats = torch.empty(G, ge.N_STATS, dtype=torch.float64, device=dev)

    def k_decode():
        _lib.call("msde_graph2d_decode", _p(x_d), _p(adj_d), _p(z_d), _p(tgt_d), _p(dec.atom_flag), _p(mv_d), _p(plan.mol), G,
                  ctypes.c_longlong(plan.n_samples), plan.n_max, ncls, MAX_BOND, _p(dec.sig), _p(dec.counts), _p(dec.adj_l1), _stream())

    def k_summary():
        _lib.call("msde_graph2d_summary", _p(dec.sig), _p(dec.counts), _p(dec.adj_l1), _p(dec.atom_flag), _p(plan.mol), G,
                  _p(first), _p(stats), _stream())
    for name, fn in (("decode_kernel_ms", k_decode), ("summary_kernel_ms", k_summary)):
        event_ms(fn, a.launches)
        put(rec, name, [event_ms(fn, a.launches) for _ in range(a.rounds)])
    dev_counts, dev_stats = dec.counts.cpu().long(), stats.cpu()

    # (c), (d): from the host
    def device_path():
        d = ge.decode(*(t.to(dev) for t in packed), n, Ks, max_bond=MAX_BOND, max_valence2=mv, ncls=ncls)
        return ge.summary(d)[0].cpu()
    put(rec, "device_path_ms", host_ms(device_path, a.repeats), 3)
    put(rec, "evaluate_ms", host_ms(lambda: ge.evaluate_graphs(recs), a.repeats), 3)

    # (e) torch ops on resident padded tensors
    pad = padded(recs, K, dev)
    mv_l = mv_d.long()
    put(rec, "torch_ops_ms", host_ms(lambda: torch_eval(*pad, mv_l, G, K), a.repeats), 3)
    t_counts, t_stats = torch_eval(*pad, mv_l, G, K)
    rec["torch_ops_counts_differing"] = int((t_counts != dev_counts).sum())
    rec["torch_ops_stats_max_abs_diff"] = float("%.3g" % (t_stats - dev_stats).abs().nan_to_num().max())
    rec["torch_ops_over_device_path"] = round(rec["torch_ops_ms"] / rec["device_path_ms"], 2)
    rec["mean_exact_match"] = round(float(dev_stats[:, 5].mean()), 4)
    rec["mean_valid"] = round(float(dev_stats[:, 6].mean()), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
