"""Milliseconds per step of the QM9 fine-tune step (moleculesde_amd.finetune_qm9.QM9Trainer) in three modes, in one process:
  captured  -- one bucket's hipGraph replayed per batch, fresh raw blobs fed one step ahead by bucket.BlobFeeder;
  eager     -- the exact-size step on host-prepared batches (geom3d.prepare_batch), launched from the host;
  torch_ops -- the same SchNet with nn.Linear + L1Loss + torch.optim.Adam (the script's step built from torch ops).
Settings: bs 128 (the script's default), emb 300, SchNet 6 x 128 filters, 51 gaussians, cutoff 10, synthetic QM9-shaped
batches (synthetic.make_qm9_batch; targets from make_qm9_targets).  Each mode also reports evaluation molecules / s.  One
JSON line per mode.

    python tools/bench_finetune_qm9.py [--steps 50] [--warmup 10] [--batches 8] [--only captured|eager|torch_ops]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model(dev, args):
    import moleculesde_amd.geom3d as G
    torch.manual_seed(0)
    m = G.SchNet(hidden_channels=args.emb, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                 readout="mean", node_class=119).to(dev)
    head = torch.nn.Linear(args.emb, 1).to(dev)
    return m, head


def _host_batches(args):
    from moleculesde_amd.synthetic import make_qm9_batch, make_qm9_targets
    hb, ys = [], []
    for i in range(args.batches):
        b = make_qm9_batch(args.bs, seed=100 + i)
        b.x[b.x == 0] = 1
        del b.edge_index, b.edge_attr, b.extended_edge_index
        hb.append(b)
        ys.append(make_qm9_targets(b, seed=i)[:, 7].contiguous())
    return hb, ys


def _timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bench(mode, args, dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import bucket as BK, hip
    from moleculesde_amd.finetune_qm9 import QM9Trainer
    hb, ys = _host_batches(args)
    atoms = sum(int(b.x.numel()) for b in hb) / len(hb)
    out = {"mode": mode, "bs": args.bs, "emb": args.emb, "interactions": 6, "filters": 128, "gaussians": 51,
           "mean_atoms_per_batch": round(atoms, 1), "steps": args.steps, "warmup": args.warmup, "batches": args.batches}
    m, head = _model(dev, args)
    mean, std = -10.0, 5.0
    if mode == "captured":
        tr = QM9Trainer(m, head, lr=1e-4, epochs=100, train_mean=mean, train_std=std)
        caps = BK.Caps.covering([BK.raw_sizes_z(b) for b in hb])
        bk = tr.make_bucket(caps)
        blobs = [BK.pack_raw_z(b, caps, y, pin=True) for b, y in zip(hb, ys)]
        tr.capture_bucket(bk, blobs[0])
        feeder = BK.BlobFeeder(bk)
        feeder.submit(blobs[0])

        def step(i):
            feeder.submit(blobs[(i + 1) % len(blobs)])
            feeder.load_next()
            tr.replay(bk)
        for i in range(args.warmup):
            step(i)
        s = _timed(step, args.steps)
        feeder.load_next()                   # drain the blob submitted one step ahead
        evaluate = lambda: tr.evaluate(list(zip(hb, ys)), bucket=bk)
    elif mode == "eager":
        tr = QM9Trainer(m, head, lr=1e-4, epochs=100, train_mean=mean, train_std=std)
        db = [(G.prepare_batch(b.clone(), dev), y.to(dev)) for b, y in zip(hb, ys)]
        for i in range(args.warmup):
            tr.step(*db[i % len(db)])
        s = _timed(lambda i: tr.step(*db[i % len(db)]), args.steps)
        evaluate = lambda: tr.evaluate(db)
    else:
        db = [(G.prepare_batch(b.clone(), dev), y.to(dev)) for b, y in zip(hb, ys)]
        opt = torch.optim.Adam([{"params": m.parameters(), "lr": 1e-4}, {"params": head.parameters(), "lr": 1e-4}], lr=1e-4)
        crit = torch.nn.L1Loss()

        def step(i):
            b, y = db[i % len(db)]
            pred = head(m(b.x, b.positions, b.batch)).squeeze()
            loss = crit(pred, (y - mean) / std)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.item()           # the script's loss_acc += loss.cpu().detach().item()
        for i in range(args.warmup):
            step(i)
        s = _timed(step, args.steps)

        @torch.no_grad()
        def evaluate():
            ps = [(head(m(b.x, b.positions, b.batch)).squeeze() * std + mean) for b, _ in db]
            return torch.cat(ps).cpu()
    out["ms_per_step"] = round(s * 1e3, 3)
    out["molecules_per_s"] = round(args.bs / s, 1)
    evaluate()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.eval_reps):
        evaluate()
    torch.cuda.synchronize()
    te = (time.perf_counter() - t0) / args.eval_reps
    out["eval_molecules_per_s"] = round(args.bs * len(hb) / te, 1)
    hip.clear_row_bounds()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--emb", type=int, default=300)
    ap.add_argument("--eval_reps", type=int, default=5)
    ap.add_argument("--only", choices=["captured", "eager", "torch_ops"], default=None)
    args = ap.parse_args()
    from moleculesde_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    for mode in ("captured", "eager", "torch_ops"):
        if args.only in (None, mode):
            print(json.dumps(bench(mode, args, dev)), flush=True)


if __name__ == "__main__":
    main()
