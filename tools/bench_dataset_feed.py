"""Time three ways of feeding the captured pretrain step (configs[1] flags: the README command without the 3D->2D head, 256
molecules per batch) with the SAME batches of a synthetic molecule store:
  (a) dataset   dataset.DatasetRunner: the store on the device, every step one graph replay that gathers its own batch
                (csrc/dataset.hip); the per-epoch permutation upload is inside the timed window;
  (b) blobs     pretrain.StreamRunner on pre-packed pinned raw blobs of the same batches: bench.py's headline feed, no
                collate work at all;
  (c) collate   the same batches collated and packed on the host per step (Batch.from_data_list + bucket.pack_raw +
                Trainer.step_bucket) from MolData objects made BEFORE the clock starts -- the reference's per-sample
                Dataset.get work (slicing, extend_graph, centring) is not in this row: what a user with a real dataset had
                before the resident store, at its cheapest.
One process; (a) on a trainer of its own, (b) and (c) share one (same bucket, same graph).  A round is device events around
`--epochs` passes over the store's epochs (256 steps); the rows alternate for `--rounds` rounds; reported: the median
over rounds of ms per step and the min / max over rounds (the run-to-run spread).  All three run on capacities covering the
timed epochs, so no batch falls back; `epoch1_rule_fallbacks` counts the batches of the later timed epochs that the default
rule (dataset.caps_for on epoch 1) would have sent to the exact-size step.

The gather kernel's own time comes from a separate profiler run of `--gather_only` (N eager gathers, nothing else):
    rocprofv3 --output-format csv --kernel-trace --stats -d DIR -o run -- python tools/bench_dataset_feed.py --gather_only
    python tools/bench_dataset_feed.py --kernel_stats DIR --out profiles/pr_dataset_feed_bench.jsonl
"""
import argparse
import csv
import gc
import glob
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_synthetic_store import synthetic_molecules  # noqa: E402
from moleculesde_amd import bucket as BK, dataset as DS, pretrain  # noqa: E402
from moleculesde_amd.batch import Batch  # noqa: E402


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    steps = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def gather_stats(path):
    """Average / min / max microseconds of dataset_gather_kernel from rocprofv3's kernel statistics under `path`."""
    for f in sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(f)):
            if "dataset_gather_kernel" in row.get("Name", ""):
                us = lambda k: round(float(row[k]) / 1e3, 3)
                return {"gather_kernel_calls": int(row["Calls"]), "gather_kernel_us": us("AverageNs"),
                        "gather_kernel_us_min_max": [us("MinNs"), us("MaxNs")]}
    return None


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default="")
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--batches", type=int, default=64, help="batches per epoch: the store holds batches * batch_size molecules")
    p.add_argument("--distinct_epochs", type=int, default=2, help="distinct epoch permutations the timed passes cycle over")
    p.add_argument("--epochs", type=int, default=4, help="passes over the store per round (epochs * batches steps)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--gather_only", action="store_true", help="launch the gather alone (for a profiler's kernel trace)")
    p.add_argument("--kernel_stats", default="", help="directory of a rocprofv3 --kernel-trace --stats run of --gather_only")
    a = p.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    Bsz, M = a.batch_size, a.batch_size * a.batches
    store = DS.MoleculeStore.from_molecules(synthetic_molecules(M, seed=0))
    plans = [store.epoch_plan(e + 1, Bsz, seed=0) for e in range(a.distinct_epochs)]
    caps = BK.Caps.covering([pl.need(k) for pl in plans for k in range(pl.n_full)])
    rule = DS.caps_for(plans[0])
    steps = a.epochs * a.batches
    rd = DS.ResidentDataset(store, dev)
    if a.gather_only:
        bk = BK.Bucket(caps, dev)
        for e in range(a.epochs):
            rd.begin_epoch(plans[e % len(plans)])
            for _ in range(a.batches):
                rd.launch_gather(bk.raw, bk.layout, caps)
        torch.cuda.synchronize()
        assert int(rd.err.cpu()) == 0
        print(f"{steps} gathers of {Bsz} molecules, blob {bk.layout['_total'] * 4} bytes")
        return
    args = pretrain.readme_args(SDE_coeff_generative_3Dto2D=0, batch_size=Bsz)
    # the host side of rows (b) and (c): every timed batch as MolData lists (centred, with the extended graph, as the
    # reference's Dataset.get hands them to the loader), collated once for (b)'s blobs
    mols = [[[store.molecule(int(i), remove_center=True, extended=True) for i in pl.molecules(k)] for k in range(a.batches)]
            for pl in plans]
    host = [[Batch.from_data_list(m) for m in ep] for ep in mols]
    torch.manual_seed(0)
    tr_a = pretrain.Trainer(args, dev)
    run_a = DS.DatasetRunner(tr_a, rd, plans[0], caps=caps)
    torch.manual_seed(0)
    tr_b = pretrain.Trainer(args, dev)
    run_b = pretrain.StreamRunner(tr_b, [b for ep in host for b in ep])
    assert run_b.caps.as_dict() == caps.as_dict(), (run_b.caps.as_dict(), caps.as_dict())
    blobs = [[run_b.pack(b) for b in ep] for ep in host]
    assert all(b is not None for ep in blobs for b in ep)

    def row_a():
        return sum(run_a.run(plans[e % len(plans)]) for e in range(a.epochs))

    def row_b():
        return sum(run_b.run(blobs[e % len(plans)], a.batches) for e in range(a.epochs))

    def row_c():
        for e in range(a.epochs):
            for m in mols[e % len(plans)]:
                tr_b.step_bucket(run_b.bk, BK.pack_raw(Batch.from_data_list(m), caps))
        return steps
    rows = {"dataset": row_a, "blobs": row_b, "collate": row_c}
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
    assert run_a.fallbacks == 0 and run_b.fallbacks == 0 and int(rd.err.cpu()) == 0 and run_b.bk.check()[0]
    for tr in (tr_a, tr_b):
        assert all(bool(torch.isfinite(v)) for v in tr.log.values())
    rec = {"what": "pretrain_feed_configs1", "batch_size": Bsz, "molecules": M, "atoms": int(store.x.size(0)),
           "directed_bonds": int(store.edge_index.size(1)), "steps_per_round": steps, "rounds": a.rounds,
           "capacities": caps.as_dict(), "blob_bytes": run_a.bk.layout["_total"] * 4,
           "epoch1_rule_fallbacks": int(sum(int((~pl.fits(rule)).sum()) for pl in plans[1:]))}
    for k in rows:
        rec[k + "_ms"] = round(statistics.median(ms[k]), 4)
        rec[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    rec["dataset_over_blobs"] = round(rec["dataset_ms"] / rec["blobs_ms"], 4)
    rec["collate_over_dataset"] = round(rec["collate_ms"] / rec["dataset_ms"], 3)
    rec["dataset_molecules_per_s"] = round(Bsz / rec["dataset_ms"] * 1e3)
    if a.kernel_stats:
        st = gather_stats(a.kernel_stats)
        assert st is not None, f"no dataset_gather_kernel row under {a.kernel_stats}"
        rec.update(st)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
