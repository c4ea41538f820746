"""Time the captured configs[2]-shaped pretrain step (README flags: batch 256, emb 300, contrastive + 2D->3D + 3D->2D losses)
with each of the three 3D->2D models the pretraining script can select: SDEModel3Dto2D_node_adj_dense (base), _02 and _03.
One process, one trainer per model, the three graphs replayed in alternation; each number is the median over rounds of
HIP-event time per replay.  Launches per step: GPU kernels of one eager step under the torch profiler (the captured graph
replays the same launches).  Prints one JSON line per model and appends them to --out.

    python tools/bench_sde3d2d_03.py [--out profiles/pr_sde3d2d_03_bench.jsonl] [--only _03]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moleculesde_amd import pretrain  # noqa: E402

MODELS = {"base": "SDEModel3Dto2D_node_adj_dense", "_02": "SDEModel3Dto2D_node_adj_dense_02",
          "_03": "SDEModel3Dto2D_node_adj_dense_03"}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters            # ms per call


def launches(tr, b):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        tr.step(b)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "Memcpy" not in e.name and "Memset" not in e.name)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="")
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--only", default="", help="comma-separated subset of base,_02,_03 (default: all three)")
    a = p.parse_args()
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_batch
    dev = torch.device("cuda", 0)
    names = [k for k in MODELS if not a.only or k in a.only.split(",")]
    b = G.prepare_batch(make_batch(a.batch_size, seed=1), dev)
    trs, n_launch = {}, {}
    for k in names:
        torch.manual_seed(0)
        tr = pretrain.Trainer(pretrain.readme_args(batch_size=a.batch_size, SDE_3Dto2D_model=MODELS[k]), dev)
        for _ in range(2):
            tr.step(b)
        n_launch[k] = launches(tr, b)
        tr.capture(b)
        trs[k] = tr
    for k in names:
        for _ in range(3):
            trs[k].step_graph(b)
    torch.cuda.synchronize()
    t = {k: [] for k in names}
    for _ in range(a.rounds):
        for k in names:
            t[k].append(timed(lambda: trs[k].step_graph(b), a.iters))
    for k in names:
        rec = {"what": "captured_pretrain_step", "model": MODELS[k], "batch_size": a.batch_size, "emb_dim": 300,
               "atoms": int(b.x.size(0)), "ms_per_step": round(statistics.median(t[k]), 4),
               "ms_min": round(min(t[k]), 4), "ms_max": round(max(t[k]), 4), "launches_per_step": n_launch[k]}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
