"""Generate tests/golden/sampler_3d2d.npz: the 3D->2D predictor-corrector sampler on the GENUINE reference classes
(oracle/ref_loader.genuine(): SDE_dense.VESDE / VPSDE with their reverse(score_fn).discretize, EdgeScoreNetwork_dense /
NodeScoreNetwork_dense) at the production head, with the three intended changes of DESIGN §7.1 (no early stop, VP alpha =
alphas[k], symmetric initial adjacency).  The inference script itself cannot be imported (its config module parses argv, it
needs rdkit), so its corrector update is restated below; every raw N(0,1) draw is stored so a test can inject it.

Ragged batch of 3 molecules (9, 5, 7 atoms; atom 3 of the last one bond-less), padded to Nm = 9, dim3D = 8, 119 classes,
5 iterations of the 1000-step schedule with n_steps = 2, VE and VP.  Parameters, representation and noise are
fp16-representable fp32 values stored as fp16 (exact); x outputs are stored for the 21 atom rows only.

    python tools/make_golden_sampler_3d2d.py        (needs the reference checkout: build container only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

B, NM, FD, NCLS, ITERS, NSTEPS, EPS, SNR, SEPS = 3, 9, 8, 119, 5, 2, 1e-4, 0.2, 0.9
SIZES = [9, 5, 7]
RANGES = {"ve": ("VESDE", 0.1, 1.0), "vp": ("VPSDE", 0.2, 1.0)}     # build_from_args "VE" / "VP"


def masked_sym(z, flags):
    z = z.triu(1)
    z = z + z.transpose(-1, -2)
    return z * flags[:, :, None] * flags[:, None, :]


def masked(z, flags):
    return z * flags[:, :, None]


class Heads(torch.nn.Module):
    """What RSDE.discretize reads of the SDE model: embedding_3D, embedding_X."""

    def __init__(self):
        super().__init__()
        self.embedding_X = torch.nn.Linear(NCLS, FD)
        self.embedding_3D = torch.nn.Linear(FD, FD)


def main():
    g = ref_loader.genuine()
    SD = g.SDE_dense
    torch.manual_seed(77)
    heads = Heads()
    edge = g.EdgeScoreNetwork_dense(dim3D=FD, nhid=16, num_layers=4, num_linears=3, c_init=2, c_hid=8, c_final=4, adim=16,
                                    num_heads=4, conv="MLP")
    node = g.NodeScoreNetwork_dense(nfeat=FD, depth=4, nhid=16, nout=NCLS)
    with torch.no_grad():             # non-zero biases, O(1) activations
        for i, (_, p) in enumerate(list(heads.named_parameters()) + list(edge.named_parameters()) + list(node.named_parameters())):
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape) * 0.6 - 0.3)
            else:
                p.copy_(torch.randn(p.shape) / p.shape[1] ** 0.5)
            p.copy_(p.half().float())     # fp16-representable inputs: the fixture stores them in half the bytes, exactly
    flags = torch.zeros(B, NM)
    for b, n in enumerate(SIZES):
        flags[b, :n] = 1
    flags[2, 3] = 0
    rep = torch.randn(B, NM, FD).half().float() * flags[:, :, None]
    raw = dict(x_init=torch.randn(B, NM, NCLS), adj_init=torch.randn(B, NM, NM),
               corr_adj=torch.randn(ITERS, NSTEPS, B, NM, NM), corr_x=torch.randn(ITERS, NSTEPS, B, NM, NCLS),
               pred_adj=torch.randn(ITERS, B, NM, NM), pred_x=torch.randn(ITERS, B, NM, NCLS))
    raw = {k: v.half().float() for k, v in raw.items()}
    out = {f"noise.{k}": v.half().numpy() for k, v in raw.items()}
    out.update(rep=rep.numpy(), flags=flags.numpy(), sizes=np.array(SIZES), n_steps=np.array(NSTEPS), eps=np.array(EPS),
               snr=np.array(SNR), scale_eps=np.array(SEPS))
    sd = {f"embedding_X.{k}": v for k, v in heads.embedding_X.state_dict().items()}
    sd.update({f"embedding_3D.{k}": v for k, v in heads.embedding_3D.state_dict().items()})
    sd.update({f"edge_score_network.{k}": v for k, v in edge.state_dict().items()})
    sd.update({f"node_score_network.{k}": v for k, v in node.state_dict().items()})
    out.update({f"sd.{k}": v.half().numpy() for k, v in sd.items()})
    ragged_rows = torch.cat([torch.arange(n) + b * NM for b, n in enumerate(SIZES)])

    for tag, (cls, lo, hi) in RANGES.items():
        sde_x, sde_adj = getattr(SD, cls)(lo, hi, 1000), getattr(SD, cls)(lo, hi, 1000)
        out[f"{tag}.range"] = np.array([lo, hi])

        def score_fn_of(sde, net):
            def score_fn(px, adj, flg, t):
                std = sde.marGINal_prob(torch.zeros_like(adj), t)[1]
                return -net(px, adj, flg) / std[:, None, None]
            return score_fn
        sf_x, sf_adj = score_fn_of(sde_x, node), score_fn_of(sde_adj, edge)
        rsde_x, rsde_adj = sde_x.reverse(sf_x, False), sde_adj.reverse(sf_adj, False)
        timesteps = torch.linspace(sde_adj.T, EPS, sde_adj.N)
        # the per-step table, from the genuine classes
        k = (timesteps * (sde_adj.N - 1) / sde_adj.T).long()
        ones = torch.ones(sde_adj.N, 1, 1)
        std_all = sde_adj.marGINal_prob(ones, timesteps)[1]
        G_all = sde_adj.discretize(ones, timesteps)[1]
        vp = isinstance(sde_adj, SD.VPSDE)
        alpha_all = sde_adj.alphas[k] if vp else torch.ones_like(timesteps)
        fa_all = torch.sqrt(sde_adj.alphas[k]) if vp else torch.ones_like(timesteps)
        out[f"{tag}.table.k"] = k.int().numpy()
        out[f"{tag}.table.par"] = torch.stack([std_all, G_all, alpha_all, fa_all], 1).float().numpy()

        with torch.no_grad():
            x = masked(raw["x_init"], flags)
            adj = masked_sym(raw["adj_init"], flags)          # prior_sampling_sym (intended), masked
            for i in range(ITERS):
                t = torch.ones(B) * timesteps[i]
                # corrector: one score of the common old state, n_steps Langevin steps on it (x fed back)
                px = heads.embedding_3D(rep) + heads.embedding_X(x)
                new = {}
                for obj, sde, sf, v in (("adj", sde_adj, sf_adj, adj), ("x", sde_x, sf_x, x)):
                    grad = sf(px, adj, flags, t)
                    if i == 0:
                        out[f"{tag}.score0_{obj}"] = grad.numpy()
                    alpha = sde.alphas[(t * (sde.N - 1) / sde.T).long()] if vp else torch.ones_like(t)
                    for s in range(NSTEPS):
                        zr = raw[f"corr_{obj}"][i, s]
                        z = masked_sym(zr, flags) if obj == "adj" else masked(zr, flags)
                        gn = grad.reshape(B, -1).norm(dim=-1).mean()
                        nn_ = z.reshape(B, -1).norm(dim=-1).mean()
                        step = (SNR * nn_ / gn) ** 2 * 2 * alpha
                        vm = v + step[:, None, None] * grad
                        v = vm + torch.sqrt(step * 2)[:, None, None] * z * SEPS
                    new[obj] = (v, vm)
                x, adj = new["x"][0], new["adj"][0]
                # predictor: the genuine RSDE.discretize on the common corrected state
                fa_, Ga = rsde_adj.discretize(x, adj, flags, t, rep, heads, is_adj=True)
                fx_, Gx = rsde_x.discretize(x, adj, flags, t, rep, heads, is_adj=False)
                adj_mean = adj - fa_
                adj_n = adj_mean + Ga[:, None, None] * masked_sym(raw["pred_adj"][i], flags)
                x_mean = x - fx_
                x_n = x_mean + Gx[:, None, None] * masked(raw["pred_x"][i], flags)
                x, adj = x_n, adj_n
                out[f"{tag}.it{i}.x"] = x.reshape(B * NM, NCLS)[ragged_rows].numpy()
                out[f"{tag}.it{i}.x_mean"] = x_mean.reshape(B * NM, NCLS)[ragged_rows].numpy()
                out[f"{tag}.it{i}.adj"] = adj.numpy()
                out[f"{tag}.it{i}.adj_mean"] = adj_mean.numpy()
    path = os.path.join(ROOT, "tests", "golden", "sampler_3d2d.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
