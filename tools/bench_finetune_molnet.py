"""Steps per second of the MoleculeNet fine-tune step (moleculesde_amd.finetune_molnet.MoleculeNetTrainer) against the same
step built from torch ops on top of the same GIN (F.dropout, index_add pooling, nn.Linear, BCEWithLogitsLoss in fp64,
torch.optim.Adam), in one process.  Settings: Tox21-shaped (bs 32, 12 tasks) and ToxCast-shaped (bs 32, 617 tasks), GIN 5 x
300, dropout 0.5, synthetic MoleculeNet-shaped batches (synthetic.make_molnet_batch, sizes unverified).  One JSON line per
setting.

    python tools/bench_finetune_molnet.py [--steps 50] [--warmup 10] [--batches 8] [--only hip|torch]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("tox21", 32, 12), ("toxcast", 32, 617)]


def _model(dev, emb, layers, drop, seed):
    import moleculesde_amd.geom3d as G
    torch.manual_seed(seed)
    m = G.GNN(layers, emb, JK="last", drop_ratio=drop, gnn_type="GIN").to(dev)
    head = torch.nn.Linear(emb, 1).to(dev)
    return m, head


def _time(fn, batches, steps, warmup):
    for i in range(warmup):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def bench_setting(name, bs, T, args, dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.finetune_molnet import MoleculeNetTrainer
    from moleculesde_amd.synthetic import make_molnet_batch
    batches = [G.prepare_batch(make_molnet_batch(bs, T, seed=100 + i), dev) for i in range(args.batches)]
    atoms = sum(int(b.x.size(0)) for b in batches) / len(batches)
    out = {"setting": name, "bs": bs, "tasks": T, "emb": args.emb, "layers": args.layers, "dropout": args.dropout,
           "mean_atoms_per_batch": round(atoms, 1), "steps": args.steps, "warmup": args.warmup}
    if args.only in (None, "hip"):
        m, _ = _model(dev, args.emb, args.layers, args.dropout, 0)
        head = torch.nn.Linear(args.emb, T).to(dev)
        tr = MoleculeNetTrainer(m, head, lr=1e-4, epochs=100, seed=1)
        s = _time(lambda b: tr.step(b), batches, args.steps, args.warmup)
        out["hip_ms_per_step"] = round(s * 1e3, 3)
        out["hip_steps_per_s"] = round(1.0 / s, 2)
    if args.only in (None, "torch"):
        m, _ = _model(dev, args.emb, args.layers, args.dropout, 0)
        head = torch.nn.Linear(args.emb, T).to(dev)
        opt = torch.optim.Adam([{"params": m.parameters(), "lr": 1e-4}, {"params": head.parameters(), "lr": 1e-4}], lr=1e-4)
        crit = torch.nn.BCEWithLogitsLoss(reduction="none")

        def torch_step(b):
            m.train()
            h = m(b.x, b.edge_index, b.edge_attr)
            cnt = torch.bincount(b.batch, minlength=b.num_graphs).clamp(min=1).to(h.dtype)
            pool = torch.zeros(b.num_graphs, h.size(1), device=dev).index_add_(0, b.batch, h) / cnt[:, None]
            pred = head(pool)
            if torch.sum(torch.isnan(pred)) > 0:
                return None
            y = b.y.view(pred.shape).to(torch.float64)
            valid = y ** 2 > 0
            lm = crit(pred.double(), (y + 1) / 2)
            lm = torch.where(valid, lm, torch.zeros_like(lm))
            opt.zero_grad()
            loss = torch.sum(lm) / torch.sum(valid)
            loss.backward()
            opt.step()
            return loss.item()
        s = _time(torch_step, batches, args.steps, args.warmup)
        out["torch_ops_ms_per_step"] = round(s * 1e3, 3)
        out["torch_ops_steps_per_s"] = round(1.0 / s, 2)
    if "hip_ms_per_step" in out and "torch_ops_ms_per_step" in out:
        out["speedup_vs_torch_ops"] = round(out["torch_ops_ms_per_step"] / out["hip_ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--emb", type=int, default=300)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--setting", choices=[s[0] for s in SETTINGS], default=None)
    args = ap.parse_args()
    from moleculesde_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    for name, bs, T in SETTINGS:
        if args.setting in (None, name):
            print(json.dumps(bench_setting(name, bs, T, args, dev)), flush=True)


if __name__ == "__main__":
    main()
