"""Time the captured capacity-bucket pretrain step (configs[1] flags: README command without the 3D->2D head, 256 molecules)
for the three --CL_similarity_metric values -- InfoNCE_dot_prod and EBM_dot_prod behind --captured_cl, EBM_node_dot_prod as
bench.py's headline runs it -- against the exact-size eager step of the same trainer on the same batches, which is the only
way InfoNCE_dot_prod and EBM_dot_prod train without --captured_cl.

Per metric: one Trainer, `--pool` distinct synthetic batches, one bucket covering them and ONE captured graph
(Trainer.capture_bucket); the captured mode replays it per batch (one device copy of the raw blob + one replay, as
bench.py's stream mode), the eager mode launches Trainer.step on the resident exact-size batches.  The two modes alternate
in one process (--eager_only: the eager mode alone) for `--rounds` rounds of `--steps` steps; a round is a host clock around
the steps ending in a device synchronise.  Reported: the median over rounds of ms per step, and the min / max over rounds (the run-to-run spread).
Prints one JSON line per metric and appends it to --out.

    python tools/bench_contrastive_bucket.py [--out profiles/pr_contrastive_bucket_bench.jsonl]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moleculesde_amd import bucket as BK, pretrain  # noqa: E402
from moleculesde_amd.geom3d import prepare_batch  # noqa: E402
from moleculesde_amd.synthetic import make_batch  # noqa: E402

METRICS = ("InfoNCE_dot_prod", "EBM_dot_prod", "EBM_node_dot_prod")


def timed_ms(fn, items, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        fn(items[s % len(items)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(metric, a, dev):
    torch.manual_seed(0)
    args = pretrain.readme_args(CL_similarity_metric=metric, SDE_coeff_generative_3Dto2D=0, batch_size=a.batch_size,
                                captured_cl=True)
    tr = pretrain.Trainer(args, dev)
    cpu = [make_batch(a.batch_size, seed=s) for s in range(a.pool)]
    pool = [prepare_batch(b.clone(), dev) for b in cpu]
    needs = [BK.raw_sizes(b) for b in cpu]
    caps = BK.Caps.covering(needs)
    for b in pool:                                        # every exact shape once (workspaces, code objects)
        tr.step(b)
    modes = {"eager": (tr.step, pool)}
    bk = None
    if not a.eager_only:
        bk = tr.make_bucket(caps)
        blobs = [BK.pack_raw(b, caps).to(dev) for b in cpu]
        tr.capture_bucket(bk, blobs[0])
        modes = {"captured": (lambda blob: tr.step_bucket(bk, blob), blobs), "eager": (tr.step, pool)}
    for fn, items in modes.values():
        timed_ms(fn, items, a.warmup)
    assert bk is None or bk.check()[0]
    ms = {k: [] for k in modes}
    gc.collect()
    gc.disable()
    try:
        for _ in range(a.rounds):
            for k, (fn, items) in modes.items():
                ms[k].append(timed_ms(fn, items, a.steps))
    finally:
        gc.enable()
    assert bk is None or bk.check()[0]
    loss = {k: float(v) for k, v in tr.log.items()}
    assert all(v == v and abs(v) != float("inf") for v in loss.values()), loss
    rec = {"what": "pretrain_step_configs1", "metric": metric, "batch_size": a.batch_size, "pool": a.pool,
           "atoms_min_max": [min(n["N"] for n in needs), max(n["N"] for n in needs)], "capacity_atoms": caps.N,
           "steps_per_round": a.steps, "rounds": a.rounds}
    for k in modes:
        rec[k + "_ms"] = round(statistics.median(ms[k]), 4)
        rec[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    if "captured" in modes:
        rec["eager_over_captured"] = round(rec["eager_ms"] / rec["captured_ms"], 3)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="")
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--pool", type=int, default=8)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--metrics", default=",".join(METRICS))
    p.add_argument("--eager_only", action="store_true",
                   help="time the exact-size eager step alone (what a tree without --captured_cl can run for every metric)")
    p.add_argument("--tag", default="", help="copied into every record (e.g. which checkout ran)")
    a = p.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    for metric in a.metrics.split(","):
        rec = measure(metric, a, dev)
        if a.tag:
            rec["tag"] = a.tag
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
