"""Time the captured pretrain step (configs[1] flags: the README command without the 3D->2D head, 256 molecules per batch) on
a synthetic molecule store of 16 384 molecules with and without sub-graph masking (--SSL_masking_ratio), in ONE process:
  (a) ratio0     dataset.DatasetRunner on whole molecules (every step one graph replay that gathers its own batch);
  (b) ratio015   the same runner on an epoch plan with mask_ratio 0.15: the graph holds msde_dataset_gather_batch_masked and
                 msde_plan_build_ext; the per-epoch mask kernel and permutation upload are inside the timed window;
both on capacities covering the UNMASKED timed epochs (masked batches are smaller and always fit), each on a trainer of its
own.  A round is device events around `--epochs` passes over the store; the rows alternate for `--rounds` rounds; reported:
the median over rounds of ms per step and the min / max over rounds (the run's own repeat-to-repeat spread).
Then, alone on an idle device, device events around back-to-back launches of
  (c) the unmasked gather, (d) the masked gather (each with its one-thread advance launch behind it),
  (e) the per-epoch mask kernel over the whole store (reported per launch and per million molecules).
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_synthetic_store import synthetic_molecules  # noqa: E402
from moleculesde_amd import bucket as BK, dataset as DS, pretrain  # noqa: E402


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    steps = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default="")
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--batches", type=int, default=64, help="batches per epoch: the store holds batches * batch_size molecules")
    p.add_argument("--ratio", type=float, default=0.15)
    p.add_argument("--distinct_epochs", type=int, default=2)
    p.add_argument("--epochs", type=int, default=4, help="passes over the store per round (epochs * batches steps)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--launches", type=int, default=500, help="back-to-back launches per timing of rows (c) to (e)")
    a = p.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    Bsz, M = a.batch_size, a.batch_size * a.batches
    store = DS.MoleculeStore.from_molecules(synthetic_molecules(M, seed=0))
    whole = [store.epoch_plan(e + 1, Bsz, seed=0) for e in range(a.distinct_epochs)]
    masked = [store.epoch_plan(e + 1, Bsz, seed=0, mask_ratio=a.ratio, mask_seed=0) for e in range(a.distinct_epochs)]
    caps = BK.Caps.covering([pl.need(k) for pl in whole for k in range(pl.n_full)])
    steps = a.epochs * a.batches
    args = pretrain.readme_args(SDE_coeff_generative_3Dto2D=0, batch_size=Bsz)
    runs = {}
    for name, plans in (("ratio0", whole), ("ratio015", masked)):
        torch.manual_seed(0)
        tr = pretrain.Trainer(args, dev)
        rd = DS.ResidentDataset(store, dev)
        runs[name] = (tr, rd, DS.DatasetRunner(tr, rd, plans[0], caps=caps), plans)

    def row(name):
        _, _, runner, plans = runs[name]
        return lambda: sum(runner.run(plans[e % len(plans)]) for e in range(a.epochs))
    rows = {k: row(k) for k in runs}
    for fn in rows.values():                      # warm-up: one round of every row
        event_ms(fn)
    ms = {k: [] for k in rows}
    gc.collect()
    gc.disable()
    try:
        for _ in range(a.rounds):
            for k, fn in rows.items():
                ms[k].append(event_ms(fn))
    finally:
        gc.enable()
    for tr, rd, runner, _ in runs.values():
        assert runner.fallbacks == 0 and int(rd.err.cpu()) == 0 and runner.bk.check()[0]
        assert all(bool(torch.isfinite(v)) for v in tr.log.values())
    rec = {"what": "pretrain_mask_configs1", "batch_size": Bsz, "molecules": M, "atoms": int(store.x.size(0)),
           "mask_ratio": a.ratio, "atoms_kept_share": round(float(masked[0].needs["N"].sum() / whole[0].needs["N"].sum()), 4),
           "steps_per_round": steps, "rounds": a.rounds, "capacities": caps.as_dict()}
    for k in rows:
        rec[k + "_ms"] = round(statistics.median(ms[k]), 4)
        rec[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    rec["ratio015_over_ratio0"] = round(rec["ratio015_ms"] / rec["ratio0_ms"], 4)
    # the launches alone, on the masked runner's resident store and bucket
    _, rd, runner, _ = runs["ratio015"]
    bk = runner.bk
    rd.begin_epoch(masked[0])
    n = a.launches

    def gathers(ext_in):
        def fn():
            for i in range(n):
                if i % a.batches == 0:
                    rd.counter.zero_()
                rd.launch_gather(bk.raw, bk.layout, caps, ext_in=ext_in)
            return n
        return fn

    def masks():
        for i in range(n):
            rd.launch_mask(a.ratio, 0, 1 + i)
        return n
    alone = {"gather_launch_us": gathers(None), "masked_gather_launch_us": gathers(bk.ext_in), "mask_epoch_launch_us": masks}
    for fn in alone.values():
        event_ms(fn)
    us = {k: [] for k in alone}
    for _ in range(a.rounds):
        for k, fn in alone.items():
            us[k].append(event_ms(fn) * 1e3)
    assert int(rd.err.cpu()) == 0
    for k in alone:
        rec[k] = round(statistics.median(us[k]), 2)
        rec[k + "_min_max"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
    rec["mask_epoch_us_per_million_molecules"] = round(rec["mask_epoch_launch_us"] / M * 1e6, 1)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
