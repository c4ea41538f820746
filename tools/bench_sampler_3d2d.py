"""Time the 3D->2D predictor-corrector sampler (moleculesde_amd/sampler_3d2d.py): 1000 iterations on one 14-atom molecule x 10
replicas (configs[3]'s shape), emb 300, production head, VE; graph replay and eager; kernels per iteration and per score
evaluation (torch profiler, one eager iteration).  Prints one JSON line.

    python tools/bench_sampler_3d2d.py [--iters 1000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import sampler_3d2d as S
    from moleculesde_amd.geom3d import dense_head as DH
    from moleculesde_amd.geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense
    from moleculesde_amd.synthetic import make_batch
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = SDEModel3Dto2D_node_adj_dense(dim3D=300, nhid=16, num_layers=4, num_linears=3, c_hid=8, c_final=4, adim=16, emb_dim=300,
                                      beta_min=0.1, beta_max=1.0, num_diffusion_timesteps=1000, c_init=2).to(dev).eval()
    b = G.prepare_batch(make_batch(10, seed=1, sizes=[14] * 10), dev)
    rep = torch.randn(b.batch.numel(), 300, device=dev)
    res = {"shape": "10 x 14 atoms, emb 300", "iters": a.iters}
    for mode, graph in (("graph", True), ("eager", False)):
        S.node_adj_PC_generation(rep, b, m, max_iters=5, noise_seed=1, use_graph=graph)     # warm-up (weight layouts, capture)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = S.node_adj_PC_generation(rep, b, m, max_iters=a.iters, noise_seed=1, use_graph=graph)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[f"{mode}_s"] = round(dt, 4)
        res[f"{mode}_us_per_iter"] = round(1e6 * dt / a.iters, 1)
        res[f"{mode}_finite"] = bool(all(torch.isfinite(t).all() for t in out))
    # kernels of one eager iteration and of one score evaluation
    from torch.profiler import profile, ProfilerActivity
    pl = S._layout(b, rep, None, None, None)
    _, _, B, Nm, mol_ptr, sizes, batch, local, flags, h3 = pl
    pair_ptr = DH.ragged_layout(mol_ptr)
    cfg = DH.types.SimpleNamespace(N=h3.size(0), P=int(pair_ptr[-1]), B=B, n_max=max(sizes), mol_ptr=mol_ptr, pair_ptr=pair_ptr)
    _, par = S.step_table(m.sde_adj, 1000)
    pc = S.FusedPC(m, h3, cfg, flags[batch, local].contiguous(), Nm, par, 1, 0.2, 0.9, 3)
    pc.iteration()
    torch.cuda.synchronize()
    for key, fn in (("kernels_per_score_eval", lambda: pc.ev(pc.x)), ("kernels_per_iter", pc.iteration)):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        res[key] = len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
