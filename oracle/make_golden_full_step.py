"""Generate tests/golden/full_step_dropout.npz from the reference's own files (verbatim on the stand-in third-party layer;
needs the reference checkout at oracle/ref_loader.REF_ROOT): one pretrain forward + backward of GNN (GIN) + SchNet +
SDEModel2Dto3D_02 + SDEModel3Dto2D_node_adj_dense with dropout ON, every random draw (dropout masks, noise, time steps) in
program order under torch.manual_seed.  Run in float64 (default dtype, parameters and batch): a float32 fixture would
carry the host's BLAS rounding (thread count, vector width) into a comparison meant to be bit-tight.
Parameters are a deterministic function of their position (set_parameters(), repeated by the test), so the fixture stores
only the state-dict key order and the buffers.  Stored besides: the batch, the five outputs of step() (float64) and every
parameter gradient as fixed-point integers in the narrowest integer type that holds them, q = round(grad / scale /
GRAD_STEP) with scale the model's largest gradient magnitude (plus the names of parameters the step leaves without one).  tests/test_oracle_vs_reference.py replays it
through oracle/restate.py with build() / set_parameters() / step() below, so that both sides run the same procedure.
    python oracle/make_golden_full_step.py"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

E, FILTERS, INTERACTIONS = 48, 32, 3
INIT_SEED, STEP_SEED = 0, 5
BATCH = dict(num_graphs=8, seed=1)
MODELS = ("gnn", "sch", "s23", "s32")
OUTPUTS = ("h2", "h3", "loss_2Dto3D", "loss_x", "loss_adj")
PARAM_SEED = 7000
GRAD_STEP = 2.0 ** -17     # fixed-point step of the stored gradients, in units of the model's largest gradient magnitude


def build(ns):
    """The four models from namespace `ns` (the reference's classes, or oracle.restate) at the test configuration."""
    kw23 = dict(emb_dim=E, hidden_dim=32, beta_min=0.2, beta_max=1.0, num_diffusion_timesteps=1000, beta_schedule=None,
                SDE_type="VE", use_extend_graph=True)
    kw32 = dict(dim3D=E, c_init=2, c_hid=8, c_final=4, num_heads=4, adim=16, nhid=16, num_layers=4, emb_dim=E,
                num_linears=3, beta_min=0.1, beta_max=1.0, num_diffusion_timesteps=1000, SDE_type="VE", num_class_X=119,
                noise_on_one_hot=True)
    kws = dict(hidden_channels=E, num_filters=FILTERS, num_interactions=INTERACTIONS, num_gaussians=51, cutoff=10,
               readout="mean", node_class=119)
    return dict(gnn=ns.GNN(5, E, JK="last", drop_ratio=0, gnn_type="GIN"), sch=ns.SchNet(**kws),
                s23=ns.SDEModel2Dto3D_02(**kw23), s32=ns.SDEModel3Dto2D_node_adj_dense(**kw32))


def set_parameters(models):
    """Every parameter of every model from a generator seeded by its position (float32 draws, widened to the parameter's
    dtype: identical under any default dtype).  Biases are non-zero on purpose."""
    i = 0
    with torch.no_grad():
        for k in MODELS:
            for _, p in models[k].named_parameters():
                gen = torch.Generator().manual_seed(PARAM_SEED + i)
                i += 1
                if p.dim() == 1:
                    v = torch.rand(p.shape, generator=gen, dtype=torch.float32) * 0.6 - 0.3
                else:
                    v = torch.randn(p.shape, generator=gen, dtype=torch.float32) / float(p.shape[1]) ** 0.5
                p.copy_(v.to(p.dtype))


def buffers(model):
    """The state-dict entries that are not parameters (BatchNorm statistics, fixed offsets, ...)."""
    names = {n for n, _ in model.named_parameters()}
    return {n: v for n, v in model.state_dict().items() if n not in names}


def to_double(b):
    """The batch with its floating-point tensors in float64 (index tensors untouched)."""
    for k in b.tensor_keys():
        v = getattr(b, k)
        if v.is_floating_point():
            setattr(b, k, v.double())
    return b


def step(m, b, seed):
    """Forward of all four models and the backward of the summed losses; returns OUTPUTS in order."""
    torch.manual_seed(seed)
    h2 = m["gnn"](b.x, b.edge_index, b.edge_attr)
    _, h3 = m["sch"](b.x[:, 0], b.positions, b.batch, return_latent=True)
    l23 = m["s23"](h2, b, anneal_power=0)["position"]
    lx, la = m["s32"](h3, b, reduce_mean=True, continuous=True, train=True, anneal_power=0)
    (l23 + lx + la).backward()
    return h2, h3, l23, lx, la


def main():
    from oracle import ref_loader
    from oracle.make_golden import batch_np
    from moleculesde_amd.synthetic import make_batch
    warnings.filterwarnings("ignore")
    ns = ref_loader.verbatim()
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(INIT_SEED)
    ref = build(ns)
    set_parameters(ref)
    b = to_double(make_batch(BATCH["num_graphs"], BATCH["seed"]))
    out = {"seed": np.int64(STEP_SEED)}
    for k in MODELS:         # the state BEFORE the step (the forward updates BatchNorm statistics)
        out[f"{k}.sd_keys"] = np.array(list(ref[k].state_dict().keys()))
        out.update({f"{k}.buf.{n}": v.detach().numpy().copy() for n, v in buffers(ref[k]).items()})
    out.update(batch_np(b))
    res = step(ref, b.clone(), STEP_SEED)
    out.update({n: v.detach().numpy() for n, v in zip(OUTPUTS, res)})
    for k in MODELS:
        named = list(ref[k].named_parameters())
        scale = max(p.grad.abs().max().item() for _, p in named if p.grad is not None)
        out[f"{k}.grad_scale"] = np.float64(scale)
        for n, p in named:
            if p.grad is not None:
                q = torch.round(p.grad / (scale * GRAD_STEP)).to(torch.int64)
                m = int(q.abs().max())
                assert m < 2 ** 31
                dt = torch.int8 if m < 2 ** 7 else torch.int16 if m < 2 ** 15 else torch.int32   # the narrowest that holds it
                out[f"{k}.qgrad.{n}"] = q.to(dt).numpy()
        out[f"{k}.no_grad"] = np.array([n for n, p in named if p.grad is None], dtype=str)
    path = os.path.join(ROOT, "tests", "golden", "full_step_dropout.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
