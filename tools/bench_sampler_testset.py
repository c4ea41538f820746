"""Conformer generation for a synthetic test set: generate_samples_from_testset at several molecules_per_launch against the
host loop it replaces (one position_PC_generation trajectory per molecule, as the reference script runs its test set).
Molecules: synthetic.make_molecule, sizes drawn as in make_batch; GIN emb 300; num_repeat 10; 1000 steps.  Both sides include
everything a user pays per molecule (collation, plan, GIN forward, tabulation, capture, the copy back); wall clock around a
device synchronise, best and median of --reps passes over the whole test set, the two sides alternating.  Appends one JSON line
per configuration to --out (default profiles/pr_sampler_testset_bench.jsonl)."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import moleculesde_amd.geom3d as G
from moleculesde_amd import sampler
from moleculesde_amd.synthetic import make_molecule

ap = argparse.ArgumentParser()
ap.add_argument("--molecules", type=int, default=32)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--num_repeat", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--per_launch", type=int, nargs="+", default=[1, 4, 8, 16, 25, 32])
ap.add_argument("--launches_only", action="store_true", help="skip the timings: launch counts and kernel times only")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_sampler_testset_bench.jsonl"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(0)
rng = np.random.default_rng(0)
mols = [make_molecule(rng) for _ in range(args.molecules)]
gnn = G.GNN(5, 300, JK="last", drop_ratio=0, gnn_type="GIN").to(dev).eval()
s23 = G.SDEModel2Dto3D_02(emb_dim=300, hidden_dim=32, beta_min=0.2, beta_max=1.0, num_diffusion_timesteps=1000,
                          beta_schedule=None, SDE_type="VE", use_extend_graph=True).to(dev).eval()


def baseline():
    """The only way before the grouped driver: a host loop, one trajectory per molecule."""
    out = []
    for i, m in enumerate(mols):
        b = G.prepare_batch(sampler.repeat_data(m, args.num_repeat), dev)
        with torch.no_grad():
            rep = gnn(b.x, b.edge_index, b.edge_attr)
        out.append(sampler.position_PC_generation(s23, rep, b, num_steps=args.steps, noise_seed=sampler.group_seed(0, i)).cpu())
    return out


def grouped(per):
    return sampler.generate_samples_from_testset(mols, gnn, s23, num_repeat=args.num_repeat, start=0, end=len(mols),
                                                 molecules_per_launch=per, num_steps=args.steps, noise_seed=0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def launches_per_iteration(per):
    """Kernel launches of one iteration of a `per`-molecule trajectory: eager runs of 3 and 5 iterations under the profiler,
    difference / 2 (the fixed part -- tabulation, starting coordinates -- cancels); and the mean device time of the kernels
    that run at least once per iteration, from the 5-iteration run."""
    from torch.profiler import profile, ProfilerActivity
    b = G.prepare_batch(sampler.repeat_data(mols[:per], args.num_repeat), dev)
    with torch.no_grad():
        rep = gnn(b.x, b.edge_index, b.edge_attr)
    ptr = [0] + list(np.cumsum([args.num_repeat * m.num_nodes for m in mols[:per]]))
    counts = []
    for steps in (3, 3, 5):          # (the first run warms every shape up)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            sampler.position_PC_generation_grouped(s23, rep, b, ptr, num_steps=steps, use_graph=False, group_seeds=[1] * per)
            torch.cuda.synchronize()
        rows = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
        counts.append(sum(e.count for e in rows))
    kernels = {e.key[:60]: [e.count / 5.0, round(e.device_time_total / e.count, 2)] for e in rows if e.count >= 5}
    return (counts[2] - counts[1]) / 2.0, kernels


def emit(row):
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


n_mol = len(mols)
common = {"molecules": n_mol, "atoms": int(sum(m.num_nodes for m in mols)), "num_repeat": args.num_repeat, "steps": args.steps,
          "device": torch.cuda.get_device_name(0)}
# warm-up: every code object, and the shapes of one short pass of either side
sampler.generate_samples_from_testset(mols[:2], gnn, s23, num_repeat=args.num_repeat, end=2, molecules_per_launch=2, num_steps=20,
                                      noise_seed=0)
b0 = G.prepare_batch(sampler.repeat_data(mols[0], args.num_repeat), dev)
with torch.no_grad():
    sampler.position_PC_generation(s23, gnn(b0.x, b0.edge_index, b0.edge_attr), b0, num_steps=20, noise_seed=1)

times = {"baseline": []}
times.update({per: [] for per in args.per_launch})
for _ in range(0 if args.launches_only else args.reps):
    times["baseline"].append(timed(baseline))
    for per in args.per_launch:
        times[per].append(timed(lambda: grouped(per)))


def row(name, ts, trajectories, extra):
    best, med = min(ts), statistics.median(ts)
    r = dict(common, config=name, seconds_best=round(best, 4), seconds_median=round(med, 4), seconds_all=[round(t, 4) for t in ts],
             molecules_per_s=round(n_mol / best, 3), molecules_per_s_median=round(n_mol / med, 3), trajectories=trajectories,
             us_per_iteration=round(best / (trajectories * args.steps) * 1e6, 2))
    r.update(extra)
    return r


if not args.launches_only:
    base = row("baseline: position_PC_generation per molecule", times["baseline"], n_mol, {"molecules_per_launch": 1})
    emit(base)
for per in ([] if args.launches_only else args.per_launch):
    r = row("generate_samples_from_testset", times[per], -(-n_mol // per), {"molecules_per_launch": per})
    r["speedup_vs_baseline"] = round(r["molecules_per_s"] / base["molecules_per_s"], 3)
    emit(r)
for per in args.per_launch:
    n_launch, kernels = launches_per_iteration(per)
    emit(dict(common, config="launches", molecules_per_launch=per, launches_per_iteration=n_launch,
              kernel_calls_per_iteration_and_mean_us=kernels))
