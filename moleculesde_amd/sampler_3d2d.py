"""3D->2D reverse-SDE predictor-corrector sampler: atom types and adjacency from a molecule's 3D representation with a
trained SDEModel3Dto2D_node_adj_dense, as INTENDED by node_adj_PC_generation
(examples/pretrain_MoleculeSDE_inference_3D_to_2D_VE_VP.py:96-262; DESIGN §7.1 lists what differs from the script as
shipped: no early stop, VP alpha, symmetric initial adjacency).

Per time step t_k of linspace(T, eps, N):  Langevin corrector on (x, adj) -> reverse-diffusion predictor on the corrected
(x, adj).  Both correctors score the same old state and both predictors the same corrected one, so one evaluation of the two
score networks serves each half, and the corrector's n_steps inner steps reuse the score of its input state (:226-233).

Fused path (default): csrc/dense_pc.hip on the ragged layout of geom3d/dense_head.py, scores from dense_head.ScoreEval; two eager
warm-up iterations, then one captured iteration replayed with no host work.  Operator path (`corrector_update` /
`predictor_update`): plain torch on padded tensors through the model's modules -- the cross-check of the tests, and the
fallback for shapes the kernels do not cover when `model.allow_operator_path` is set.

Several test-set molecules per trajectory (`node_adj_PC_generation_grouped`, `generate_2d_from_3d_grouped`, at the end of this
file): csrc/dense_pc_grouped.hip keeps the corrector's statistics and the noise seed per group of replicas; the
single-trajectory path above is what it is compared with and is not routed through it."""
import ctypes

import torch

from . import _lib, hip as _hip, plan as _plan, slabs
from .geom3d import dense_head as _dh
from .geom3d.sde import VPSDE
from .geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense_02, SDEModel3Dto2D_node_adj_dense_03, mask_adjs, mask_x

_p = _hip._p


# ------------------------------------------------------------------------------------------------ host helpers
def step_table(sde, num_steps, eps=1e-4):
    """(k [S] int64, par [S, 4] fp32) on the CPU for timesteps = linspace(T, eps, num_steps) in fp32, with the SDE's own torch
    ops: k = long(t (N-1) / T), par = {std(t) (marGINal_prob), G(t) (discretize), alpha_k (VP; VE: 1), fa_k} where the
    discretised drift is f(x) = fa x - x (VP: fa = sqrt(alpha_k), VE: 1)."""
    t = torch.linspace(sde.T, eps, num_steps)
    k = (t * (sde.N - 1) / sde.T).long()
    ones = torch.ones(num_steps, 1, 1)
    std = sde.marGINal_prob(ones, t)[1]
    G = sde.discretize(ones, t)[1]
    if isinstance(sde, VPSDE):
        alpha = sde.alphas[k]
        fa = torch.sqrt(alpha)
    else:
        alpha = fa = torch.ones(num_steps)
    return k, torch.stack([std.float(), G.float(), alpha.float(), fa.float()], 1).contiguous()


def sym_noise(raw, flags):
    """gen_noise(sym=True) (SDE_model_3D_to_2D_node_adj_dense.py:532-540) on a given raw draw [B, Nm, Nm]."""
    z = raw.triu(1)
    return mask_adjs(z + z.transpose(-1, -2), flags)


def ragged_pairs(adj, sizes):
    """Padded [B, Nm, Nm] -> the ragged pair vector [P] (molecule b at pair_ptr[b] + i n_b + j)."""
    return torch.cat([adj[b, :n, :n].reshape(-1) for b, n in enumerate(sizes)])


def ragged_pair_noise(raw, flags, sizes):
    """The ragged symmetric pair vector the fused kernels draw from a raw padded [B, Nm, Nm] sample: entry (i, j) reads the
    raw (min(i,j), max(i,j)) value, 0 on the diagonal, masked by the flags -- gen_noise's semantics."""
    out = []
    for b, n in enumerate(sizes):
        idx = torch.arange(n)
        lo, hi = torch.minimum(idx[:, None], idx[None, :]), torch.maximum(idx[:, None], idx[None, :])
        z = raw[b][lo, hi] * (lo != hi).to(raw.dtype) * flags[b, :n, None] * flags[b, None, :n]
        out.append(z.reshape(-1))
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------ operator path
def _score(model, representation, x, adj, flags, std, net):
    px = model.embedding_3D(representation) + model.embedding_X(x)
    return -net(px, adj, flags) / std[:, None, None]


def _draw(raw, like, flags, sym):
    z = torch.randn_like(like) if raw is None else raw
    return sym_noise(z, flags) if sym else mask_x(z, flags)


def corrector_update(model, representation, x, adj, flags, t, snr=0.2, scale_eps=0.9, n_steps=1, noise_adj=None,
                     noise_x=None):
    """LangevinCorrector.update_fn (:213-262) for adj and x on one common input state: scores computed once, n_steps steps
    (noise_* [n_steps] raw draws, None: torch.randn).  VP: alpha = alphas[k].  Returns (x, adj, x_mean, adj_mean)."""
    out = []
    for obj in ("adj", "x"):
        sde = model.sde_adj if obj == "adj" else model.sde_x
        net = model.edge_score_network if obj == "adj" else model.node_score_network
        std = sde.marGINal_prob(torch.zeros_like(adj), t)[1]
        alpha = sde.corrector_alpha(t) if isinstance(sde, VPSDE) else torch.ones_like(t)
        grad = _score(model, representation, x, adj, flags, std, net)
        v = adj if obj == "adj" else x
        raws = noise_adj if obj == "adj" else noise_x
        vm = v
        for s in range(n_steps):
            z = _draw(None if raws is None else raws[s], v, flags, obj == "adj")
            grad_norm = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
            noise_norm = torch.norm(z.reshape(z.shape[0], -1), dim=-1).mean()
            step_size = (snr * noise_norm / grad_norm) ** 2 * 2 * alpha
            vm = v + step_size[:, None, None] * grad
            v = vm + torch.sqrt(step_size * 2)[:, None, None] * z * scale_eps
        out.append((v, vm))
    (adj_n, adj_m), (x_n, x_m) = out
    return x_n, adj_n, x_m, adj_m


def predictor_update(model, representation, x, adj, flags, t, noise_adj=None, noise_x=None):
    """ReverseDiffusionPredictor.update_fn (:172-190) with RSDE.discretize (SDE_dense.py:97-105) for adj and x on one common
    state.  Returns (x, adj, x_mean, adj_mean)."""
    out = []
    for obj in ("adj", "x"):
        sde = model.sde_adj if obj == "adj" else model.sde_x
        net = model.edge_score_network if obj == "adj" else model.node_score_network
        v = adj if obj == "adj" else x
        std = sde.marGINal_prob(torch.zeros_like(adj), t)[1]
        f, G = sde.discretize(v, t)
        score = _score(model, representation, x, adj, flags, std, net)
        rev_f = f - G[:, None, None] ** 2 * score
        z = _draw(noise_adj if obj == "adj" else noise_x, v, flags, obj == "adj")
        vm = v - rev_f
        out.append((vm + G[:, None, None] * z, vm))
    (adj_n, adj_m), (x_n, x_m) = out
    return x_n, adj_n, x_m, adj_m


# ------------------------------------------------------------------------------------------------ fused path
class FusedPC:
    """One trajectory's device state and buffers for csrc/dense_pc.hip (allocated once: a captured iteration allocates
    nothing).  `noises`: the injected raw draws (dict of padded tensors, see node_adj_PC_generation) or None (counter noise
    keyed by `seed`)."""

    def __init__(self, model, h3, cfg, flags, Nm, par, n_steps, snr, scale_eps, seed, noises=None, x_init=None,
                 adj_init=None):
        dev = h3.device
        self.model, self.cfg, self.Nm, self.n_steps = model, cfg, Nm, n_steps
        self.ev = _dh.ScoreEval(model, cfg, h3, flags)
        N, P, B = cfg.N, cfg.P, cfg.B
        e = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.x, self.x_mean, self.score_x = e(N, _dh.XP_LD), e(N, _dh.XP_LD), e(N, _dh.XP_LD)
        self.adj, self.adj_mean, self.score_adj = e(P), e(P), e(P)
        self.part = e(B * (2 + 2 * n_steps))
        self.step = torch.zeros(2, dtype=torch.int64, device=dev)
        self.par = par.to(dev)
        self.flags = flags
        self.keep = []
        s = _lib.DensePcParams()
        s.mol_ptr, s.pair_ptr, s.flags, s.par, s.step = (t.data_ptr() for t in (cfg.mol_ptr, cfg.pair_ptr, flags, self.par,
                                                                                self.step))
        s.E3, s.XC, s.AC = self.ev.E3.data_ptr(), self.ev.XC.data_ptr(), self.ev.AC.data_ptr()
        s.x, s.adj, s.x_mean, s.adj_mean = (t.data_ptr() for t in (self.x, self.adj, self.x_mean, self.adj_mean))
        s.score_adj, s.score_x, s.part = self.score_adj.data_ptr(), self.score_x.data_ptr(), self.part.data_ptr()
        noises = dict(noises or {})
        if x_init is not None:
            noises["x_init"] = x_init
        for field, key in (("nz_init_adj", "adj_init"), ("nz_init_x", "x_init"), ("nzc_adj", "corr_adj"), ("nzc_x", "corr_x"),
                           ("nzp_adj", "pred_adj"), ("nzp_x", "pred_x")):
            if noises.get(key) is not None:
                t = noises[key].to(dev, torch.float32).contiguous()
                self.keep.append(t)
                setattr(s, field, t.data_ptr())
        self.iters = int(noises["pred_adj"].shape[0]) if noises.get("pred_adj") is not None else 0
        s.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        s.B, s.Nm, s.ncls, s.n_steps, s.S, s.iters = B, Nm, model.num_class_X, n_steps, par.size(0), self.iters
        s.F, s.ldxc = h3.size(1), self.ev.XC.stride(0)
        s.snr, s.scale_eps = float(snr), float(scale_eps)
        self.params = s
        given = None
        if adj_init is not None:
            given = adj_init.to(dev, torch.float32).contiguous()
            self.keep.append(given)
        _lib.call("msde_dense_pc_init", ctypes.byref(s), _p(given), _hip._stream())

    def iteration(self):
        ev, s = self.ev, ctypes.byref(self.params)
        G2, OUT = ev(self.x)
        _lib.call("msde_dense_pc_corrector", s, _p(G2), G2.size(1), _p(ev.w2), _p(ev.b2), _p(OUT), _hip._stream())
        G2, OUT = ev(self.x)
        _lib.call("msde_dense_pc_predictor", s, _p(G2), G2.size(1), _p(ev.w2), _p(ev.b2), _p(OUT), _hip._stream())


def _check_model(model, probability_flow):
    if probability_flow:
        raise NotImplementedError("probability_flow=True: the 3D->2D inference script never sets it (its ODE predictor is not "
                                  "built)")
    if isinstance(model, SDEModel3Dto2D_node_adj_dense_03) or getattr(model, "COND_3D", False):
        # its score networks read embedding_3D(h) beside every layer's input, score_fn(x, adj, node_3D_repr, flags, t): the
        # script's sampler passes no conditioning, and the evaluation below is the base model's arithmetic
        raise NotImplementedError(f"{type(model).__name__}: SDEModel3Dto2D_node_adj_dense_03 conditions every score-network "
                                  "layer on embedding_3D(h); the reference has no sampler for it (the script's sampler passes "
                                  "no conditioning)")
    if isinstance(model, SDEModel3Dto2D_node_adj_dense_02):
        raise NotImplementedError("SDEModel3Dto2D_node_adj_dense_02: the script's sampler SUMS embedding_3D and embedding_X "
                                  "(:228,240; SDE_dense.py:88,99), which contradicts _02's concatenated 2*dim3D input")
    if not model.noise_on_one_hot:
        raise NotImplementedError("noise_on_one_hot=False: the sampler generates one-hot class scores only")


def _layout(data, representation, B, max_num_nodes, flags):
    """Ragged layout (mol_ptr, pair_ptr, sizes), flags [B, Nm] (from the bonds unless given) and the ragged representation."""
    pl = _plan.get_plan(data)
    dn = _plan.dense_plan(pl, data)
    B = pl.B if B is None else int(B)
    Nm = dn.N_max if max_num_nodes is None else int(max_num_nodes)
    if B != pl.B or Nm < dn.N_max:
        raise ValueError(f"B = {B}, max_num_nodes = {Nm} do not fit the batch ({pl.B} molecules, up to {dn.N_max} atoms)")
    mol_ptr = pl.mol_ptr.to(torch.int32)
    sizes = (pl.mol_ptr[1:] - pl.mol_ptr[:-1]).tolist()
    batch = data.batch.long()
    local = torch.arange(batch.numel(), device=batch.device) - pl.mol_ptr.long()[batch]
    if flags is None:
        flags = torch.zeros(B, Nm, device=batch.device)
        flags[:, :dn.N_max] = dn.flags
    flags = flags.float()
    if representation.dim() == 3:        # the reference's padded [B, Nm, F]
        representation = representation[batch, local]
    return pl, dn, B, Nm, mol_ptr, sizes, batch, local, flags, representation.float().contiguous()


@torch.no_grad()
def node_adj_PC_generation(representation, data, SDE_model, B=None, max_num_nodes=None, num_class_X=None,
                           probability_flow=False, eps=1e-4, snr=0.2, scale_eps=0.9, n_steps=1, *, num_steps=None,
                           max_iters=None, x_init=None, adj_init=None, flags=None, noises=None, noise_seed=None,
                           use_graph=True, iters_per_graph=1):
    """node_adj_PC_generation (:96-147) as intended.  representation: padded [B, Nm, F] or ragged [N, F] (data.batch order).
    Returns padded (x [B, Nm, ncls], adj [B, Nm, Nm], x_mean, adj_mean), zero outside the flags.

    num_steps: time steps of the schedule (default sde_adj.N); max_iters: stop after that many (the script's 11).  x_init /
    adj_init: padded initial state (masked here; the fused path needs a symmetric adj_init).  noises: injected raw N(0,1)
    draws in the reference's padded shapes -- "adj_init" [B, Nm, Nm] (triu(1) + transpose taken), "x_init" [B, Nm, ncls],
    "corr_adj" [I, n_steps, B, Nm, Nm], "corr_x" [I, n_steps, B, Nm, ncls], "pred_adj" [I, B, Nm, Nm], "pred_x"
    [I, B, Nm, ncls] for I >= the iterations run; None: the counter generator keyed by noise_seed (default: one draw from
    torch's generator).  use_graph / iters_per_graph: replay captured iterations (fused path)."""
    model = SDE_model
    _check_model(model, probability_flow)
    ncls = model.num_class_X
    if num_class_X is not None and int(num_class_X) != ncls:
        raise ValueError(f"num_class_X = {num_class_X} but the model has {ncls} classes")
    pl, dn, B, Nm, mol_ptr, sizes, batch, local, flags, h3 = _layout(data, representation, B, max_num_nodes, flags)
    dev = h3.device
    sde = model.sde_adj
    S = sde.N if num_steps is None else int(num_steps)
    iters = S if max_iters is None else min(S, int(max_iters))
    noises = dict(noises or {})
    if noises.get("pred_adj") is not None and noises["pred_adj"].shape[0] < iters:
        raise ValueError(f"injected noise covers {noises['pred_adj'].shape[0]} iterations, {iters} requested")
    fused = _dh.fused_supported(model.edge_score_network, model.node_score_network, Nm) and dev.type == "cuda" and \
        n_steps <= 127
    if fused and adj_init is not None:
        a = adj_init.float()
        if not torch.equal(a, a.transpose(-1, -2)):
            fused = False
            why = "adj_init is not symmetric (the fused kernels keep the adjacency exactly symmetric)"
    else:
        why = "this configuration is outside the fused HIP kernels (production head, <= 32 atoms, n_steps <= 127)"
    if not fused:
        if not getattr(model, "allow_operator_path", False):
            raise _lib.MsdeHipError(f"node_adj_PC_generation: {why} -- set `model.allow_operator_path = True` to run it operator "
                                    "by operator")
        return _generate_ops(model, h3, batch, local, flags, B, Nm, ncls, S, iters, eps, snr, scale_eps, n_steps, x_init,
                             adj_init, noises)

    # ---- fused path
    pair_ptr = _dh.ragged_layout(mol_ptr)
    cfg = _dh.types.SimpleNamespace(N=h3.size(0), P=int(pair_ptr[-1]), B=B, n_max=max(sizes), mol_ptr=mol_ptr.contiguous(),
                                    pair_ptr=pair_ptr.contiguous())
    flags_r = flags[batch, local].contiguous()
    _, par = step_table(sde, S, eps)
    if noise_seed is not None:
        seed = int(noise_seed)
    else:
        seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())
    pc = FusedPC(model, h3, cfg, flags_r, Nm, par, n_steps, snr, scale_eps, seed, noises, x_init, adj_init)
    graph, graph_k, k_iters = None, None, 1
    i = 0
    while i < iters:
        if use_graph and graph is None and i == 2:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with slabs.no_gc(collect=False), torch.cuda.graph(graph):
                pc.iteration()                   # capture only records; the replay below executes iteration i
            k_iters = max(1, min(int(iters_per_graph), iters - i))
            if k_iters > 1:
                graph_k = torch.cuda.CUDAGraph()
                with slabs.no_gc(collect=False), torch.cuda.graph(graph_k):
                    for _ in range(k_iters):
                        pc.iteration()
        if graph_k is not None and iters - i >= k_iters:
            graph_k.replay()
            i += k_iters
        elif graph is not None:
            graph.replay()
            i += 1
        else:
            pc.iteration()
            i += 1
    return to_padded(pc, batch, local, sizes, B, Nm, ncls)


def to_padded(pc, batch, local, sizes, B, Nm, ncls):
    """(x, adj, x_mean, adj_mean) of a FusedPC state in the reference's padded shapes."""
    dev = pc.x.device
    outs = []
    for xr, ar in ((pc.x, pc.adj), (pc.x_mean, pc.adj_mean)):
        xp = torch.zeros(B, Nm, ncls, device=dev)
        xp[batch, local] = xr[:, :ncls]
        ap = torch.zeros(B, Nm, Nm, device=dev)
        o = 0
        for b, n in enumerate(sizes):
            ap[b, :n, :n] = ar[o:o + n * n].view(n, n)
            o += n * n
        outs.append((xp, ap))
    (x, adj), (x_mean, adj_mean) = outs
    return x, adj, x_mean, adj_mean


def _generate_ops(model, h3, batch, local, flags, B, Nm, ncls, S, iters, eps, snr, scale_eps, n_steps, x_init, adj_init,
                  noises):
    dev = h3.device
    rep = torch.zeros(B, Nm, h3.size(1), device=dev)
    rep[batch, local] = h3
    if x_init is None:
        x_init = noises.get("x_init")
    x = mask_x(torch.randn(B, Nm, ncls, device=dev) if x_init is None else x_init.to(dev).float(), flags)
    if adj_init is not None:
        adj = mask_adjs(adj_init.to(dev).float(), flags)
    else:
        raw = noises.get("adj_init")
        adj = sym_noise(torch.randn(B, Nm, Nm, device=dev) if raw is None else raw.to(dev).float(), flags)
    x_mean, adj_mean = x, adj
    timesteps = torch.linspace(model.sde_adj.T, eps, S).to(dev)
    g = lambda key, i: None if noises.get(key) is None else noises[key][i].to(dev).float()
    for i in range(iters):
        t = torch.ones(B, device=dev) * timesteps[i]
        x, adj, x_mean, adj_mean = corrector_update(model, rep, x, adj, flags, t, snr, scale_eps, n_steps, g("corr_adj", i),
                                                    g("corr_x", i))
        x, adj, x_mean, adj_mean = predictor_update(model, rep, x, adj, flags, t, g("pred_adj", i), g("pred_x", i))
    return x, adj, x_mean, adj_mean


def generate_2d_from_3d(molecule_model_3D, SDE_model, data, num_repeat=10, **kw):
    """generate_samples_from_testset (:41-93) for one molecule (a MolData): repeat it num_repeat times, take SchNet's / PaiNN's
    return_latent node representation, sample.  Returns (x, adj, x_mean, adj_mean) padded, [num_repeat, Nm, *]."""
    from .batch import Batch
    from .geom3d.nn import prepare_batch
    _check_model(SDE_model, kw.get("probability_flow", False))      # before the 3D encoder runs
    dev = next(SDE_model.parameters()).device
    rep_data = prepare_batch(Batch.from_data_list([data] * num_repeat), dev)
    molecule_model_3D.eval()
    SDE_model.eval()
    z = rep_data.x[:, 0] if rep_data.x.dim() == 2 else rep_data.x
    with torch.no_grad():
        if type(molecule_model_3D).__name__ == "PaiNN":
            _, h = molecule_model_3D(z, rep_data.positions, rep_data.radius_edge_index, rep_data.batch, return_latent=True)
        else:
            _, h = molecule_model_3D(z, rep_data.positions, rep_data.batch, return_latent=True)
    return node_adj_PC_generation(h, rep_data, SDE_model, **kw)


# ------------------------------------------------------------------------------------------------ several molecules per trajectory
# A GROUP is a contiguous range of the batch's molecules, [group_ptr[g], group_ptr[g + 1]): the replicas of one test-set
# molecule.  Groups share the launch and the time schedule and nothing else: the corrector's mean norms and the noise seed
# are per group (csrc/dense_pc_grouped.hip), so a molecule's samples do not depend on what shares its trajectory.
_M64 = (1 << 64) - 1


def _check_mol_groups(group_ptr, B, group_seeds):
    """Host-side refusal of a bad group table over MOLECULES (the kernels index with it): returns it as a list of ints."""
    gp = [int(v) for v in (group_ptr.tolist() if isinstance(group_ptr, torch.Tensor) else group_ptr)]
    if len(gp) < 2 or gp[0] != 0 or gp[-1] != int(B):
        raise ValueError("group_ptr must run from 0 to the number of molecules (%d), got %r" % (B, gp[:1] + gp[-1:]))
    for a, b in zip(gp[:-1], gp[1:]):
        if b < a:
            raise ValueError("group_ptr is not monotone (%d after %d)" % (b, a))
        if b == a:
            raise ValueError("group_ptr holds an empty group (at molecule %d)" % a)
    if group_seeds is not None and len(group_seeds) != len(gp) - 1:
        raise ValueError("group_seeds has %d entries for %d groups" % (len(group_seeds), len(gp) - 1))
    return gp


def _group_mean(v, group_index, num_groups):
    s = torch.zeros(num_groups, dtype=v.dtype, device=v.device).index_add_(0, group_index, v)
    c = torch.zeros(num_groups, dtype=v.dtype, device=v.device).index_add_(0, group_index, torch.ones_like(v))
    return s / c


def corrector_steps_grouped(x, adj, score_x, score_adj, z_x, z_adj, flags, alpha, group_index, num_groups, snr=0.2,
                            scale_eps=0.9):
    """The Langevin corrector's arithmetic GIVEN THE SCORES, on padded tensors in plain torch (any device and dtype): the
    host / fp64 reference of msde_dense_pc_corrector_grouped and the arithmetic of corrector_update_grouped.  x [B, Nm, ncls],
    adj [B, Nm, Nm] and their scores (of this input state, used for every inner step); z_x [n_steps, B, Nm, ncls], z_adj
    [n_steps, B, Nm, Nm] RAW draws (masked / symmetrised here); alpha: a scalar, [B], or a pair (alpha_x, alpha_adj) of them;
    group_index [B] int64: the group of every molecule.  step_s = (snr mean_g||z_s|| / mean_g||score||)^2 2 alpha with both
    means over the molecule's own group.  Returns (x, adj, x_mean, adj_mean)."""
    alpha_x, alpha_adj = alpha if isinstance(alpha, (tuple, list)) else (alpha, alpha)
    out = []
    for v, grad, zs, al, sym in ((adj, score_adj, z_adj, alpha_adj, True), (x, score_x, z_x, alpha_x, False)):
        B = v.shape[0]
        al = torch.as_tensor(al, dtype=v.dtype, device=v.device).expand(B)
        grad_norm = _group_mean(torch.norm(grad.reshape(B, -1), dim=-1), group_index, num_groups)
        vm = v
        for s in range(len(zs)):
            z = sym_noise(zs[s], flags) if sym else mask_x(zs[s], flags)
            noise_norm = _group_mean(torch.norm(z.reshape(B, -1), dim=-1), group_index, num_groups)
            step_size = ((snr * noise_norm / grad_norm) ** 2 * 2)[group_index] * al
            vm = v + step_size[:, None, None] * grad
            v = vm + torch.sqrt(step_size * 2)[:, None, None] * z * scale_eps
        out.append((v, vm))
    (adj_n, adj_m), (x_n, x_m) = out
    return x_n, adj_n, x_m, adj_m


def corrector_update_grouped(model, representation, x, adj, flags, t, group_index, num_groups, snr=0.2, scale_eps=0.9,
                             n_steps=1, noise_adj=None, noise_x=None):
    """corrector_update with the two mean norms taken per group (group_index [B]): the operator path of the grouped sampler."""
    scores, alphas = {}, {}
    for obj in ("adj", "x"):
        sde = model.sde_adj if obj == "adj" else model.sde_x
        net = model.edge_score_network if obj == "adj" else model.node_score_network
        std = sde.marGINal_prob(torch.zeros_like(adj), t)[1]
        alphas[obj] = sde.corrector_alpha(t) if isinstance(sde, VPSDE) else torch.ones_like(t)
        scores[obj] = _score(model, representation, x, adj, flags, std, net)
    z_adj = [torch.randn_like(adj) for _ in range(n_steps)] if noise_adj is None else noise_adj
    z_x = [torch.randn_like(x) for _ in range(n_steps)] if noise_x is None else noise_x
    return corrector_steps_grouped(x, adj, scores["x"], scores["adj"], z_x[:n_steps], z_adj[:n_steps], flags,
                                   (alphas["x"], alphas["adj"]), group_index, num_groups, snr, scale_eps)


def _seed_tensor(seeds, dev):
    """64-bit patterns in an int64 tensor."""
    return torch.tensor([(int(s) & _M64) - (1 << 64) * ((int(s) & _M64) >> 63) for s in seeds], dtype=torch.int64, device=dev)


class GroupedPC:
    """FusedPC's state for csrc/dense_pc_grouped.hip: the same buffers and msde_dense_pc_params (its `seed` is not read) plus the
    group table -- group_ptr [G + 1] int32 over molecules, group_seed [G], group_bad [G] int32 -- allocated once."""

    def __init__(self, model, h3, cfg, flags, Nm, par, n_steps, snr, scale_eps, group_ptr, group_seeds, noises=None,
                 x_init=None, adj_init=None):
        dev = h3.device
        gp = _check_mol_groups(group_ptr, cfg.B, group_seeds)
        self.model, self.cfg, self.Nm, self.n_steps, self.G = model, cfg, Nm, n_steps, len(gp) - 1
        self.ev = _dh.ScoreEval(model, cfg, h3, flags)
        N, P, B = cfg.N, cfg.P, cfg.B
        e = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.x, self.x_mean, self.score_x = e(N, _dh.XP_LD), e(N, _dh.XP_LD), e(N, _dh.XP_LD)
        self.adj, self.adj_mean, self.score_adj = e(P), e(P), e(P)
        self.part = e(B * (2 + 2 * n_steps))
        self.step = torch.zeros(2, dtype=torch.int64, device=dev)
        self.par = par.to(dev)
        self.flags = flags
        self.group_ptr = torch.tensor(gp, dtype=torch.int32, device=dev)
        self.group_seed = _seed_tensor(group_seeds, dev)
        self.group_bad = torch.zeros(self.G, dtype=torch.int32, device=dev)
        self.keep = []
        s = _lib.DensePcParams()
        s.mol_ptr, s.pair_ptr, s.flags, s.par, s.step = (t.data_ptr() for t in (cfg.mol_ptr, cfg.pair_ptr, flags, self.par,
                                                                                self.step))
        s.E3, s.XC, s.AC = self.ev.E3.data_ptr(), self.ev.XC.data_ptr(), self.ev.AC.data_ptr()
        s.x, s.adj, s.x_mean, s.adj_mean = (t.data_ptr() for t in (self.x, self.adj, self.x_mean, self.adj_mean))
        s.score_adj, s.score_x, s.part = self.score_adj.data_ptr(), self.score_x.data_ptr(), self.part.data_ptr()
        noises = dict(noises or {})
        if x_init is not None:
            noises["x_init"] = x_init
        for field, key in (("nz_init_adj", "adj_init"), ("nz_init_x", "x_init"), ("nzc_adj", "corr_adj"), ("nzc_x", "corr_x"),
                           ("nzp_adj", "pred_adj"), ("nzp_x", "pred_x")):
            if noises.get(key) is not None:
                t = noises[key].to(dev, torch.float32).contiguous()
                self.keep.append(t)
                setattr(s, field, t.data_ptr())
        self.iters = int(noises["pred_adj"].shape[0]) if noises.get("pred_adj") is not None else 0
        s.seed = 0
        s.B, s.Nm, s.ncls, s.n_steps, s.S, s.iters = B, Nm, model.num_class_X, n_steps, par.size(0), self.iters
        s.F, s.ldxc = h3.size(1), self.ev.XC.stride(0)
        s.snr, s.scale_eps = float(snr), float(scale_eps)
        self.params = s
        g = _lib.DensePcGroups()
        g.group_ptr, g.group_seed, g.group_bad, g.G = (self.group_ptr.data_ptr(), self.group_seed.data_ptr(),
                                                       self.group_bad.data_ptr(), self.G)
        self.groups = g
        given = None
        if adj_init is not None:
            given = adj_init.to(dev, torch.float32).contiguous()
            self.keep.append(given)
        _lib.call("msde_dense_pc_init_grouped", ctypes.byref(s), ctypes.byref(g), _p(given), _hip._stream())

    def iteration(self):
        ev, s, g = self.ev, ctypes.byref(self.params), ctypes.byref(self.groups)
        G2, OUT = ev(self.x)
        _lib.call("msde_dense_pc_corrector_grouped", s, g, _p(G2), G2.size(1), _p(ev.w2), _p(ev.b2), _p(OUT), _hip._stream())
        G2, OUT = ev(self.x)
        _lib.call("msde_dense_pc_predictor_grouped", s, g, _p(G2), G2.size(1), _p(ev.w2), _p(ev.b2), _p(OUT), _hip._stream())


@torch.no_grad()
def node_adj_PC_generation_grouped(representation, data, SDE_model, group_ptr, B=None, max_num_nodes=None, num_class_X=None,
                                   probability_flow=False, eps=1e-4, snr=0.2, scale_eps=0.9, n_steps=1, *, group_seeds=None,
                                   num_steps=None, max_iters=None, x_init=None, adj_init=None, flags=None, noises=None,
                                   noise_seed=None, use_graph=True, iters_per_graph=1):
    """node_adj_PC_generation for G groups of molecules that share the trajectory but no statistic: group g = molecules
    [group_ptr[g], group_ptr[g + 1]) of `data` (the replicas of one test-set molecule).  Returns (x, adj, x_mean, adj_mean,
    group_bad): the padded outputs of node_adj_PC_generation for the whole batch and group_bad [G] int32, 1 where an x_mean /
    adj_mean value of the group was not finite at some iteration (the other groups are not affected).

    Same keywords and structure as node_adj_PC_generation (step table once, two eager warm-up iterations, one captured
    iteration replayed) on csrc/dense_pc_grouped.hip.  group_seeds: one noise seed per group -- with the counter noise group g
    walks the trajectory of node_adj_PC_generation(noise_seed=group_seeds[g]) on that group alone, up to the score networks'
    rounding; None: sampler.group_seed(noise_seed, g) where noise_seed is given, else G seeds drawn once from the device's torch
    generator.  A bad group table raises ValueError before any launch.  Shapes outside the fused kernels raise MsdeHipError
    unless `model.allow_operator_path` is set; then the grouped operator path (corrector_update_grouped / predictor_update,
    torch's generator for noise that is not injected) runs."""
    model = SDE_model
    _check_model(model, probability_flow)
    ncls = model.num_class_X
    if num_class_X is not None and int(num_class_X) != ncls:
        raise ValueError(f"num_class_X = {num_class_X} but the model has {ncls} classes")
    pl, dn, B, Nm, mol_ptr, sizes, batch, local, flags, h3 = _layout(data, representation, B, max_num_nodes, flags)
    gp = _check_mol_groups(group_ptr, B, group_seeds)
    G = len(gp) - 1
    dev = h3.device
    sde = model.sde_adj
    S = sde.N if num_steps is None else int(num_steps)
    iters = S if max_iters is None else min(S, int(max_iters))
    noises = dict(noises or {})
    if noises.get("pred_adj") is not None and noises["pred_adj"].shape[0] < iters:
        raise ValueError(f"injected noise covers {noises['pred_adj'].shape[0]} iterations, {iters} requested")
    fused = _dh.fused_supported(model.edge_score_network, model.node_score_network, Nm) and dev.type == "cuda" and \
        n_steps <= 127
    why = "this configuration is outside the fused HIP kernels (production head, <= 32 atoms, n_steps <= 127)"
    if fused and adj_init is not None:
        a = adj_init.float()
        if not torch.equal(a, a.transpose(-1, -2)):
            fused = False
            why = "adj_init is not symmetric (the fused kernels keep the adjacency exactly symmetric)"
    if not fused:
        if not getattr(model, "allow_operator_path", False):
            raise _lib.MsdeHipError(f"node_adj_PC_generation_grouped: {why} -- set `model.allow_operator_path = True` to run it "
                                    "operator by operator")
        return _generate_ops_grouped(model, h3, batch, local, flags, B, Nm, ncls, S, iters, eps, snr, scale_eps, n_steps,
                                     x_init, adj_init, noises, gp)

    # ---- fused path
    if group_seeds is None:
        if noise_seed is not None:
            from .sampler import group_seed
            group_seeds = [group_seed(noise_seed, g) for g in range(G)]
        else:      # ONE draw of G seeds per call from the device's torch generator
            group_seeds = torch.randint(0, 2 ** 62, (G,), dtype=torch.int64, device=dev).tolist()
    pair_ptr = _dh.ragged_layout(mol_ptr)
    cfg = _dh.types.SimpleNamespace(N=h3.size(0), P=int(pair_ptr[-1]), B=B, n_max=max(sizes), mol_ptr=mol_ptr.contiguous(),
                                    pair_ptr=pair_ptr.contiguous())
    flags_r = flags[batch, local].contiguous()
    _, par = step_table(sde, S, eps)
    pc = GroupedPC(model, h3, cfg, flags_r, Nm, par, n_steps, snr, scale_eps, gp, group_seeds, noises, x_init, adj_init)
    graph, graph_k, k_iters = None, None, 1
    i = 0
    while i < iters:
        if use_graph and graph is None and i == 2:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with slabs.no_gc(collect=False), torch.cuda.graph(graph):
                pc.iteration()                   # capture only records; the replay below executes iteration i
            k_iters = max(1, min(int(iters_per_graph), iters - i))
            if k_iters > 1:
                graph_k = torch.cuda.CUDAGraph()
                with slabs.no_gc(collect=False), torch.cuda.graph(graph_k):
                    for _ in range(k_iters):
                        pc.iteration()
        if graph_k is not None and iters - i >= k_iters:
            graph_k.replay()
            i += k_iters
        elif graph is not None:
            graph.replay()
            i += 1
        else:
            pc.iteration()
            i += 1
    return to_padded(pc, batch, local, sizes, B, Nm, ncls) + (pc.group_bad.clone(),)


def _generate_ops_grouped(model, h3, batch, local, flags, B, Nm, ncls, S, iters, eps, snr, scale_eps, n_steps, x_init,
                          adj_init, noises, gp):
    """_generate_ops with the corrector's means per group and group_bad kept as the predictor kernel keeps it."""
    dev = h3.device
    G = len(gp) - 1
    group_index = torch.repeat_interleave(torch.arange(G, device=dev),
                                          torch.tensor([b - a for a, b in zip(gp[:-1], gp[1:])], device=dev))
    rep = torch.zeros(B, Nm, h3.size(1), device=dev)
    rep[batch, local] = h3
    if x_init is None:
        x_init = noises.get("x_init")
    x = mask_x(torch.randn(B, Nm, ncls, device=dev) if x_init is None else x_init.to(dev).float(), flags)
    if adj_init is not None:
        adj = mask_adjs(adj_init.to(dev).float(), flags)
    else:
        raw = noises.get("adj_init")
        adj = sym_noise(torch.randn(B, Nm, Nm, device=dev) if raw is None else raw.to(dev).float(), flags)
    x_mean, adj_mean = x, adj
    group_bad = torch.zeros(G, dtype=torch.int32, device=dev)
    timesteps = torch.linspace(model.sde_adj.T, eps, S).to(dev)
    g = lambda key, i: None if noises.get(key) is None else noises[key][i].to(dev).float()
    for i in range(iters):
        t = torch.ones(B, device=dev) * timesteps[i]
        x, adj, x_mean, adj_mean = corrector_update_grouped(model, rep, x, adj, flags, t, group_index, G, snr, scale_eps, n_steps,
                                                            g("corr_adj", i), g("corr_x", i))
        x, adj, x_mean, adj_mean = predictor_update(model, rep, x, adj, flags, t, g("pred_adj", i), g("pred_x", i))
        nonfinite = ((~torch.isfinite(x_mean)).reshape(B, -1).any(1) | (~torch.isfinite(adj_mean)).reshape(B, -1).any(1))
        hit = torch.zeros(G, dtype=torch.int32, device=dev).index_add_(0, group_index, nonfinite.to(torch.int32)).clamp_(max=1)
        group_bad = torch.maximum(group_bad, hit)
    return x, adj, x_mean, adj_mean, group_bad


def generate_2d_from_3d_grouped(molecule_model_3D, SDE_model, molecules, num_repeat=10, group_seeds=None, **kw):
    """generate_2d_from_3d for a list of molecules (MolData) in ONE trajectory: one batch of num_repeat replicas of every
    molecule, group-major, one pass of SchNet's / PaiNN's return_latent over it, node_adj_PC_generation_grouped with one
    group (and one of group_seeds) per molecule.  Returns (samples, group_bad): samples[k] = (x, adj, x_mean, adj_mean) of
    molecule k, padded [num_repeat, Nm, *] with Nm the chunk's largest molecule; group_bad [len(molecules)] int32."""
    from .batch import Batch
    from .geom3d.nn import prepare_batch
    _check_model(SDE_model, kw.get("probability_flow", False))      # before the 3D encoder runs
    molecules, R = list(molecules), int(num_repeat)
    if not molecules or R < 1:
        raise ValueError("generate_2d_from_3d_grouped needs at least one molecule and num_repeat >= 1")
    gp = [R * k for k in range(len(molecules) + 1)]
    _check_mol_groups(gp, gp[-1], group_seeds)
    dev = next(SDE_model.parameters()).device
    rep_data = prepare_batch(Batch.from_data_list([m for m in molecules for _ in range(R)]), dev)
    molecule_model_3D.eval()
    SDE_model.eval()
    z = rep_data.x[:, 0] if rep_data.x.dim() == 2 else rep_data.x
    with torch.no_grad():
        if type(molecule_model_3D).__name__ == "PaiNN":
            _, h = molecule_model_3D(z, rep_data.positions, rep_data.radius_edge_index, rep_data.batch, return_latent=True)
        else:
            _, h = molecule_model_3D(z, rep_data.positions, rep_data.batch, return_latent=True)
    *outs, bad = node_adj_PC_generation_grouped(h, rep_data, SDE_model, gp, group_seeds=group_seeds, **kw)
    return [tuple(t[gp[k]:gp[k + 1]] for t in outs) for k in range(len(molecules))], bad
