"""Time the InfoNCE_dot_prod and EBM_dot_prod contrastive kernels (csrc/contrastive_infonce.hip), forward + backward, against
the same loss built from torch ops (pretrain.do_CL on the device: vendor BLAS for the products), and one exact-size eager
pretrain step (configs[1] flags) with InfoNCE_dot_prod against one with EBM_node_dot_prod.  A and B alternate in one
process; each number is the median over rounds of HIP-event time per call.  Prints one JSON line per measurement and
appends them to --out.

    python tools/bench_contrastive.py [--out profiles/pr_contrastive_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moleculesde_amd import hip, pretrain  # noqa: E402

PEAK_FP32_TF = 157.3          # MI355X fp32 matrix peak


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3           # us per call


def ab(fa, fb, iters, rounds=7):
    for f in (fa, fb):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, iters))
        tb.append(timed(fb, iters))
    return statistics.median(ta), statistics.median(tb)


def fwd_bwd(loss_fn, X, Y):
    def run():
        X.grad = Y.grad = None
        loss, _ = loss_fn(X, Y)
        loss.backward()
    return run


def kernels(emit):
    dev = torch.device("cuda", 0)
    for N, D in ((3588, 300), (560, 300)):
        g = torch.Generator().manual_seed(N)
        X = (torch.randn(N, D, generator=g) / D ** 0.5).to(dev).requires_grad_(True)
        Y = (0.7 * X.detach().cpu() + 3.3 * torch.randn(N, D, generator=g) / D ** 0.5).to(dev).requires_grad_(True)
        for metric, mine in (("InfoNCE_dot_prod", lambda x, y: hip.contrastive_infonce(x, y, 0.1)),
                             ("EBM_dot_prod", lambda x, y: hip.contrastive_ebm_shift(x, y, 1, 0.1))):
            a = types.SimpleNamespace(CL_similarity_metric=metric, CL_neg_samples=1, T=0.1)

            def ops(x, y, a=a):
                l1, a1 = pretrain.do_CL(x, y, a, None)
                l2, a2 = pretrain.do_CL(y, x, a, None)
                return (l1 + l2) / 2, (a1 + a2) / 2
            t_hip, t_ops = ab(fwd_bwd(mine, X, Y), fwd_bwd(ops, X, Y), iters=20 if N > 1000 else 100)
            rec = {"what": "contrastive_fwd_bwd", "metric": metric, "N": N, "D": D, "hip_us": round(t_hip, 1),
                   "torch_ops_us": round(t_ops, 1), "speedup": round(t_ops / t_hip, 3)}
            if metric == "InfoNCE_dot_prod":
                flop = 3 * 2 * N * N * D
                rec["fp32_peak_fraction"] = round(flop / (t_hip * 1e-6) / (PEAK_FP32_TF * 1e12), 3)
                # forward alone (S, partials, merge)
                t_f, _ = ab(lambda: mine(X.detach(), Y.detach()), lambda: None, iters=20)
                rec["hip_fwd_us"] = round(t_f, 1)
            emit(rec)


def steps(emit, bs):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_batch
    dev = torch.device("cuda", 0)
    trs = {}
    for metric in ("InfoNCE_dot_prod", "EBM_node_dot_prod"):
        torch.manual_seed(0)
        trs[metric] = pretrain.Trainer(pretrain.readme_args(CL_similarity_metric=metric, SDE_coeff_generative_3Dto2D=0,
                                                            batch_size=bs), dev)
    b = G.prepare_batch(make_batch(bs, seed=1), dev)
    t_i, t_e = ab(lambda: trs["InfoNCE_dot_prod"].step(b), lambda: trs["EBM_node_dot_prod"].step(b), iters=10, rounds=5)
    emit({"what": "eager_pretrain_step", "batch_size": bs, "atoms": int(b.x.size(0)), "InfoNCE_dot_prod_us": round(t_i, 1),
          "EBM_node_dot_prod_us": round(t_e, 1), "difference_us": round(t_i - t_e, 1)})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="")
    p.add_argument("--batch_size", type=int, default=256)
    a = p.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    kernels(emit)
    steps(emit, a.batch_size)


if __name__ == "__main__":
    main()
