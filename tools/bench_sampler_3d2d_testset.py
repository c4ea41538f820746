"""2D graph generation for a synthetic test set: graph2d_eval.generate_graphs_from_testset at several molecules_per_launch, with
molecules_per_launch=1 -- the per-molecule loop over sampler_3d2d.generate_2d_from_3d that existed before the grouped sampler --
measured in the same run as the baseline.  Molecules: synthetic.make_molecule of 10-32 atoms; SchNet emb 300 (6 interactions);
the production 3D->2D head, VE; num_repeat 10; 1000 steps.  Every side includes what a user pays per molecule (collation,
plan, SchNet forward, step table, capture, the copy back); wall clock around a device synchronise, best and median of --reps
passes over the whole test set, the configurations alternating within a pass.  With untrained weights long trajectories leave
the finite range (README): `diverged` counts the molecules flagged, which costs the kernels nothing more or less.  Also per
configuration: peak device memory of a pass, kernel launches per iteration and the mean device time of the three sampler kernels
(eager runs under the torch profiler, separate from the timed passes).  Appends one JSON line per configuration to --out
(default profiles/pr_sampler_3d2d_testset_bench.jsonl)."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import moleculesde_amd.geom3d as G
from moleculesde_amd import graph2d_eval as ge, sampler_3d2d as S
from moleculesde_amd.geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense
from moleculesde_amd.synthetic import make_molecule

ap = argparse.ArgumentParser()
ap.add_argument("--molecules", type=int, default=100)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--num_repeat", type=int, default=10)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--per_launch", type=int, nargs="+", default=[1, 10, 25, 50])
ap.add_argument("--launches_only", action="store_true", help="skip the timings: launch counts and kernel times only")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_sampler_3d2d_testset_bench.jsonl"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(0)
rng = np.random.default_rng(0)
mols = [make_molecule(rng, int(rng.integers(10, 33))) for _ in range(args.molecules)]
sch = G.SchNet(hidden_channels=300, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10, readout="mean",
               node_class=119).to(dev).eval()
m = SDEModel3Dto2D_node_adj_dense(dim3D=300, nhid=16, num_layers=4, num_linears=3, c_hid=8, c_final=4, adim=16, emb_dim=300,
                                  beta_min=0.1, beta_max=1.0, num_diffusion_timesteps=1000, c_init=2).to(dev).eval()


def run(per, molecules=None, steps=None):
    molecules = mols if molecules is None else molecules
    return ge.generate_graphs_from_testset(molecules, sch, m, num_repeat=args.num_repeat, start=0, end=len(molecules), noise_seed=0,
                                           molecules_per_launch=per, num_steps=args.steps,
                                           max_iters=args.steps if steps is None else steps)


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated(), out


def launches_per_iteration(per):
    """Kernel launches of one iteration of a `per`-molecule trajectory: eager runs of 3 and 5 iterations under the profiler,
    difference / 2 (the fixed part -- SchNet, step table, initial state -- cancels); and count per iteration and mean device
    time of the sampler's own kernels in the 5-iteration run."""
    from torch.profiler import profile, ProfilerActivity
    counts = []
    for steps in (3, 3, 5):          # (the first run warms every shape up)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            if per == 1:
                S.generate_2d_from_3d(sch, m, mols[0], num_repeat=args.num_repeat, noise_seed=1, num_steps=args.steps, max_iters=steps,
                                      use_graph=False)
            else:
                S.generate_2d_from_3d_grouped(sch, m, mols[:per], args.num_repeat, list(range(1, per + 1)), num_steps=args.steps,
                                              max_iters=steps, use_graph=False)
            torch.cuda.synchronize()
        rows = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
        counts.append(sum(e.count for e in rows))
    kernels = {e.key.split("(")[0][:60]: [e.count / 5.0, round(e.device_time_total / e.count, 2)] for e in rows
               if "dense_pc_" in e.key and e.count >= 5}
    return (counts[2] - counts[1]) / 2.0, kernels


def emit(row):
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


n_mol = len(mols)
common = {"molecules": n_mol, "atoms": int(sum(mol.num_nodes for mol in mols)), "num_repeat": args.num_repeat, "steps": args.steps,
          "device": torch.cuda.get_device_name(0)}
# warm-up: every code object and one short pass of either side
run(1, mols[:2], 20)
run(2, mols[:4], 20)

times = {per: [] for per in args.per_launch}
peak, diverged = {}, {}
for _ in range(0 if args.launches_only else args.reps):
    for per in args.per_launch:
        dt, mem, recs = timed(lambda: run(per))
        times[per].append(dt)
        peak[per] = max(peak.get(per, 0), mem)
        if per > 1:
            diverged[per] = sum(bool(r.diverged) for r in recs)

base = None
for per in ([] if args.launches_only else args.per_launch):
    ts = times[per]
    best, med = min(ts), statistics.median(ts)
    trajectories = -(-n_mol // per)
    r = dict(common, config="per-molecule loop (generate_2d_from_3d)" if per == 1 else "generate_2d_from_3d_grouped",
             molecules_per_launch=per, seconds_best=round(best, 4), seconds_median=round(med, 4), seconds_all=[round(t, 4) for t in ts],
             molecules_per_s=round(n_mol / best, 3), molecules_per_s_median=round(n_mol / med, 3), trajectories=trajectories,
             us_per_iteration=round(best / (trajectories * args.steps) * 1e6, 2), peak_device_memory_MiB=round(peak[per] / 2 ** 20, 1))
    if per > 1:
        r["molecules_diverged"] = diverged[per]
    if per == 1:
        base = r
    elif base is not None:
        r["speedup_vs_loop"] = round(r["molecules_per_s"] / base["molecules_per_s"], 3)
    emit(r)
for per in args.per_launch:
    n_launch, kernels = launches_per_iteration(per)
    emit(dict(common, config="launches", molecules_per_launch=per, launches_per_iteration=n_launch,
              sampler_kernel_calls_per_iteration_and_mean_us=kernels))
