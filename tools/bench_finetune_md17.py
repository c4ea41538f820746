"""MD17 fine-tuning epochs (moleculesde_amd.finetune_md17.MD17Trainer) on the aspirin shape: 21 atoms, SchNet(300, 128
filters, 6 interactions, 51 gaussians, cutoff 10) + Linear(300, 1), synthetic conformations (synthetic.make_md17_batch's
molecule plus noise).  One JSON line per mode:
  train_captured     -- ms per step of MD17Trainer.train_epoch at batch 1 over --train conformations: gather kernel + one
                        replayed step per batch, the loss summed on the device, one host read per epoch;
  train_forcetrainer -- ms per step of ForceTrainer.step_graph on the same conformations (host copies into the graph's inputs);
  eval_captured      -- evaluation molecules / s of MD17Trainer.evaluate at --eval_bs over --eval conformations, captured;
  eval_eager         -- the same evaluation launched from the host;
  eval_reference     -- the reference's eval() loop (finetune_MD17.py:93-142) with torch ops on the same device: the oracle's
                        SchNet, a host-to-device copy per batch, autograd.grad(create_graph=True), torch.cat of the forces;
  fit_epoch          -- wall time of one MD17Trainer.fit epoch (train, validation, test), captured graphs already made.

    python tools/bench_finetune_md17.py [--train 1000] [--eval 10277] [--eval_bs 128] [--only MODE[,MODE]]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(hidden_channels=300, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, readout="mean",
          node_class=119)
MODES = ["train_captured", "train_forcetrainer", "eval_captured", "eval_eager", "eval_reference", "fit_epoch"]


def _data(M, seed):
    from moleculesde_amd.synthetic import make_md17_batch
    b = make_md17_batch(1, seed=3, n_atoms=21)
    g = torch.Generator().manual_seed(seed)
    pos = b.positions[None] + 0.05 * torch.randn(M, 21, 3, generator=g)
    y = -4.06e5 + torch.randn(M, generator=g)
    f = 30 * torch.randn(M, 21, 3, generator=g)
    return b.x.clone(), pos, y, f


def _trainer(dev, bs=1):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.finetune_md17 import MD17Trainer, energy_force_normalization
    torch.manual_seed(0)
    m, head = G.SchNet(**KW).to(dev), torch.nn.Linear(300, 1).to(dev)
    x, pos, y, f = _data(64, 1)
    return MD17Trainer(m, head, lr=5e-4, epochs=100, normalization=energy_force_normalization(y, f), train_batch_size=bs)


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def bench(mode, args, dev):
    from moleculesde_amd.finetune_md17 import ResidentSplit
    out = {"mode": mode, "atoms": 21, "emb": 300, "filters": 128, "interactions": 6, "gaussians": 51}
    x, pos, y, f = _data(args.train, 11)
    train = ResidentSplit(x, pos, y, f, dev)
    x, pos_e, y_e, f_e = _data(args.eval, 12)
    ev = ResidentSplit(x, pos_e, y_e, f_e, dev)
    if mode == "train_captured":
        tr = _trainer(dev)
        gen = torch.Generator().manual_seed(0)
        tr.train_epoch(train, generator=gen)                  # capture + one epoch
        dt, loss = _sync_time(lambda: tr.train_epoch(train, generator=gen))
        out.update(train=args.train, bs=1, ms_per_step=round(dt / args.train * 1e3, 3), epoch_s=round(dt, 3),
                   loss_acc=loss)
    elif mode == "train_forcetrainer":
        import moleculesde_amd.geom3d as G
        from moleculesde_amd.finetune_md17 import ForceTrainer
        from moleculesde_amd.synthetic import make_md17_batch
        torch.manual_seed(0)
        m, head = G.SchNet(**KW).to(dev), torch.nn.Linear(300, 1).to(dev)
        ft = ForceTrainer(m, head, lr=5e-4)
        b = G.prepare_batch(make_md17_batch(1, seed=3, n_atoms=21), dev)
        ft.capture(b, train.y[:1], train.force[0])
        perm = torch.randperm(args.train)

        def epoch():
            for i in perm.tolist():
                ft.step_graph(train.pos[i], train.y[i:i + 1], train.force[i])
        epoch()
        dt, _ = _sync_time(epoch)
        out.update(train=args.train, bs=1, ms_per_step=round(dt / args.train * 1e3, 3), epoch_s=round(dt, 3))
    elif mode in ("eval_captured", "eval_eager"):
        tr = _trainer(dev)
        captured = mode == "eval_captured"
        tr.evaluate(ev, args.eval_bs, captured=captured)      # capture / warm-up
        dt, mae = _sync_time(lambda: tr.evaluate(ev, args.eval_bs, captured=captured))
        out.update(eval=args.eval, eval_bs=args.eval_bs, eval_s=round(dt, 4), molecules_per_s=round(args.eval / dt, 1),
                   energy_mae=mae[0], force_mae=mae[1])
    elif mode == "eval_reference":
        from oracle import restate as R
        torch.manual_seed(0)
        m, head = R.SchNet(**KW).to(dev), torch.nn.Linear(300, 1).to(dev)
        hx, hpos, hy, hf = x, pos_e, y_e, f_e                  # host tensors: the loader hands out host batches

        def run():
            model_eval = []
            pf, af = torch.Tensor([]).to(dev), torch.Tensor([]).to(dev)
            pe, ae = [], []
            for k in range(0, args.eval, args.eval_bs):
                b = min(args.eval_bs, args.eval - k)
                xb = hx.repeat(b).to(dev)
                p = hpos[k:k + b].reshape(-1, 3).to(dev).requires_grad_()
                bt = torch.arange(b).repeat_interleave(21).to(dev)
                yb, fb = hy[k:k + b].to(dev), hf[k:k + b].reshape(-1, 3).to(dev)
                e = head(m(xb, p, bt)).squeeze(1)
                force = -torch.autograd.grad(outputs=e, inputs=p, grad_outputs=torch.ones_like(e), create_graph=True,
                                             retain_graph=True)[0].detach_()
                pe.append(e.cpu().detach())
                ae.append(yb.cpu())
                pf = torch.cat([pf, force], dim=0)
                af = torch.cat([af, fb], dim=0)
            model_eval.append((torch.mean(torch.abs(torch.cat(pe) - torch.cat(ae))).item(),
                               torch.mean(torch.abs(pf - af)).item()))
            return model_eval[0]
        n0 = args.eval
        args.eval = min(n0, 4 * args.eval_bs)                  # warm-up on a few batches
        run()
        args.eval = n0
        dt, mae = _sync_time(run)
        out.update(eval=args.eval, eval_bs=args.eval_bs, eval_s=round(dt, 4), molecules_per_s=round(args.eval / dt, 1))
    elif mode == "fit_epoch":
        x, pv, yv, fv = _data(1000, 13)
        valid = ResidentSplit(x, pv, yv, fv, dev)
        tr = _trainer(dev)
        tr.epochs = 1
        gen = torch.Generator().manual_seed(0)
        tr.fit(train, valid, ev, eval_batch_size=args.eval_bs, generator=gen, log=None)      # captures
        dt, h = _sync_time(lambda: tr.fit(train, valid, ev, eval_batch_size=args.eval_bs, generator=gen, log=None))
        out.update(train=args.train, valid=1000, test=args.eval, eval_bs=args.eval_bs, epoch_s=round(dt, 3),
                   val_force_mae=h["val_force"][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=1000)
    ap.add_argument("--eval", type=int, default=10277)         # 80 full batches of 128 and a short one of 37
    ap.add_argument("--eval_bs", type=int, default=128)
    ap.add_argument("--only", default=",".join(MODES))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from moleculesde_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    for mode in args.only.split(","):
        r = bench(mode, args, dev)
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
