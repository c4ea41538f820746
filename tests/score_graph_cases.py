"""Graph, inputs, references and tolerances of the score-graph kernel tests (tests/test_score_graph_host.py on the host,
tests/test_gpu_score_graph.py on the device).

The graph is the extended graph of helpers.SCORE_GRAPH_SPECS: in-degrees 0, 1, 2, 7..16, 63, 64, 65 and 99, the first and the
last node without in-edges, N = 347 (odd, 3 mod 4).  Every operation is written once in plain torch ops and evaluated twice
on the CPU from the same fp32 inputs: in fp64 (the reference) and in fp32 (the yardstick: what an honest fp32 evaluation
loses).  A kernel output passes when its worst error, relative to the largest reference magnitude, is at most TOL_FACTOR
times the yardstick of that output; the factor covers the kernels' other order of additions (8-lane strided partial sums,
batches of 4 edges) and an expf that is 1 to 2 ulp off.  Gradients that are copies of the incoming gradient (skip, base)
have a yardstick of zero and are compared exactly.  Nothing here is taken from a kernel's result."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

import helpers as H_

TOL_FACTOR = 8.0
DEG_CLASSES = (("deg 0", 0, 0), ("deg 1-7", 1, 7), ("deg 8-63", 8, 63), ("deg 64+", 64, 10 ** 9))
FNV = 0x100000001B3
_M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def graph():
    """Host view of the fixture: batch, host plan (canonical by-target edge order), src / dst / in-degree as int64."""
    from moleculesde_amd import hip
    b = H_.build_batch(H_.SCORE_GRAPH_SPECS, seed=H_.SCORE_GRAPH_SEED)
    N = int(b.x.size(0))
    pl = hip.build_csr(b.extended_edge_index, N)
    g = types.SimpleNamespace(batch=b, plan=pl, N=N, E=pl.E, src=pl.src.long(), dst=pl.dst.long())
    g.deg = (pl.rowptr[1:] - pl.rowptr[:-1]).long()
    return g


def device_plan(dev, spare=0):
    """A fresh plan of the fixture on the device (CsrPlan.to moves in place); spare > 0: capacity for `spare` more edges than
    the graph has, padded the way the radius-graph plans are (src = dst = -1 past rowptr[N])."""
    from moleculesde_amd import hip
    g = graph()
    pl = hip.build_csr(g.batch.extended_edge_index, g.N)
    if spare:
        pad = torch.full((spare,), -1, dtype=torch.int32)
        pl.src, pl.dst = torch.cat([pl.src, pad]), torch.cat([pl.dst, pad])
        pl.E += spare
    return pl.to(dev)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ operations, any dtype ---
def attention(q, k, v, ee, src, dst, N, heads, mask=None):
    """TransformerConv message + softmax over the in-edges of the target (maximum subtracted, + 1e-16 as in PyG's softmax)
    + aggregate; mask [E, heads]: the dropout factor on alpha (0 or 1 / (1 - p))."""
    E, D = ee.shape
    Ch = D // heads
    eh = ee.view(E, heads, Ch)
    logit = (q[dst].view(E, heads, Ch) * (k[src].view(E, heads, Ch) + eh)).sum(-1) / math.sqrt(Ch)
    m = torch.full((N, heads), -math.inf, dtype=logit.dtype).scatter_reduce(
        0, dst[:, None].expand(E, heads), logit.detach(), "amax", include_self=True)
    p = torch.exp(logit - m[dst])
    s = torch.zeros(N, heads, dtype=p.dtype).index_add(0, dst, p)
    alpha = p / (s[dst] + 1e-16)
    if mask is not None:
        alpha = alpha * mask.to(alpha.dtype)
    msg = (v[src].view(E, heads, Ch) + eh) * alpha[..., None]
    return torch.zeros(N, heads, Ch, dtype=msg.dtype).index_add(0, dst, msg).view(N, D)


def frame_mix(coff, basis, dst, N):
    """mean over in-edges of (c0 b_diff + c1 b_cross + c2 b_vert); 0 for a node without in-edges."""
    mixed = (coff[:, :, None] * basis.view(-1, 3, 3)).sum(1)
    deg = torch.zeros(N, dtype=mixed.dtype).index_add(0, dst, torch.ones(dst.numel(), dtype=mixed.dtype)).clamp(min=1)
    return torch.zeros(N, 3, dtype=mixed.dtype).index_add(0, dst, mixed) / deg[:, None]


def dropout_factor(E, heads, p, seed, seed_dev=None):
    """The kernels' mask on alpha[e, h] (e: position in by-target order): msde_uniform(seed', e * heads + h) >= float32(p) with
    seed' = seed + seed_dev * FNV (mod 2^64), times 1 / (1 - p)."""
    from moleculesde_amd.finetune_molnet import msde_uniform
    s = (int(seed) + (0 if seed_dev is None else int(seed_dev)) * FNV) & _M64
    keep = msde_uniform(s, np.arange(E * heads, dtype=np.uint64)).reshape(E, heads) >= np.float32(p)
    return torch.from_numpy(keep).double() / (1.0 - float(np.float32(p)))


# ------------------------------------------------------------------------------------------ reference + yardstick of a case ---
def _evaluate(fn, inputs, w, dtype):
    """out = fn(**inputs cast to dtype); gradients of (out * w).sum() for every input.  Returns {"out", "g_<name>"} in fp64."""
    leaves = {n: t.detach().to(dtype).clone().requires_grad_(True) for n, t in inputs.items()}
    out = fn(**leaves)
    (out * w.to(dtype)).sum().backward()
    res = {"out": out.detach().double()}
    res.update({"g_" + n: t.grad.double() for n, t in leaves.items()})
    return res


def _yardsticks(ref, low):
    return {n: float((low[n] - ref[n]).abs().max()) / float(ref[n].abs().max()) for n in ref}


def _case(fn, inputs, w, exact=()):
    """exact: outputs that are copies of an input (the gradient of an added term is w itself): no yardstick, compared exactly."""
    ref, low = _evaluate(fn, inputs, w, torch.float64), _evaluate(fn, inputs, w, torch.float32)
    yard = _yardsticks(ref, low)
    for n in exact:
        assert yard.pop(n) == 0.0
    return types.SimpleNamespace(inputs=inputs, w=w, ref=ref, low=low, yard=yard)


def _plus(c, name, add):
    """out + add (skip / base, fp32) under `name`: reference, and the yardstick of the fp32 sum (g_add = w exactly)."""
    c.ref[name] = c.ref["out"] + add.double()
    low = (c.low["out"].float() + add).double()
    c.yard[name] = float((low - c.ref[name]).abs().max()) / float(c.ref[name].abs().max())


@functools.lru_cache(maxsize=None)
def attention_case(heads, Ch, qscale=1.0, p=0.0, seed=0, seed_dev=None):
    """q, k, v, skip [N, D], ee [E, D], w [N, D] (fp32) and the fp64 reference / fp32 yardstick of attention(...) and of
    attention(...) + skip ("out_skip"; the other gradients are the same, and g_skip = w exactly)."""
    g = graph()
    D = heads * Ch
    base = 1000 * heads + 10 * Ch
    inputs = {"q": _randn(base + 1, g.N, D) * qscale, "k": _randn(base + 2, g.N, D), "v": _randn(base + 3, g.N, D),
              "ee": _randn(base + 4, g.E, D)}
    skip, w = _randn(base + 5, g.N, D), _randn(base + 6, g.N, D)
    mask = dropout_factor(g.E, heads, p, seed, seed_dev) if p > 0 else None
    c = _case(lambda q, k, v, ee: attention(q, k, v, ee, g.src, g.dst, g.N, heads, mask), inputs, w)
    c.skip, c.mask = skip, mask
    _plus(c, "out_skip", skip)
    return c


SHARED_LAYERS = 3


@functools.lru_cache(maxsize=None)
def shared_projection_case(heads, Ch):
    """SHARED_LAYERS attention layers reading their edge features from column blocks of one ee_all [E, L D]: q, k, v, skip per
    layer, loss = sum of the layers' (out * w).sum().  Reference / yardstick of every layer's output and of g_ee_all."""
    g = graph()
    D, L = heads * Ch, SHARED_LAYERS
    base = 5000 + 1000 * heads + 10 * Ch
    inputs = {"ee_all": _randn(base, g.E, L * D)}
    for l in range(L):
        for j, n in enumerate("qkvs"):
            inputs[f"{n}{l}"] = _randn(base + 10 * l + j + 1, g.N, D)
    w = _randn(base + 99, g.N, L * D)

    def fn(ee_all, **t):
        return torch.cat([attention(t[f"q{l}"], t[f"k{l}"], t[f"v{l}"], ee_all[:, l * D:(l + 1) * D].contiguous(), g.src, g.dst,
                                    g.N, heads) + t[f"s{l}"] for l in range(L)], dim=1)
    return _case(fn, inputs, w, exact=[f"g_s{l}" for l in range(L)])


MLP_IN = 64


@functools.lru_cache(maxsize=None)
def frame_mix_case():
    g = graph()
    inputs = {"coff": _randn(31, g.E, 3)}
    basis, base, w = _randn(32, g.E, 9), _randn(33, g.N, 3), _randn(34, g.N, 3)
    c = _case(lambda coff: frame_mix(coff, basis.to(coff.dtype), g.dst, g.N), inputs, w)
    c.basis, c.base = basis, base
    _plus(c, "out_base", base)
    return c


@functools.lru_cache(maxsize=None)
def head_mix_case(hidden):
    """Linear(MLP_IN, hidden) -> SiLU -> Linear(hidden, 3) on every edge, frame mix, mean over in-edges."""
    g = graph()
    s = 100 * hidden
    inputs = {"x": _randn(s + 1, g.E, MLP_IN), "W1": _randn(s + 2, hidden, MLP_IN) / MLP_IN ** 0.5, "b1": _randn(s + 3, hidden) * 0.3,
              "W2": _randn(s + 4, 3, hidden) / hidden ** 0.5, "b2": _randn(s + 5, 3) * 0.3}
    basis, base, w = _randn(s + 6, g.E, 9), _randn(s + 7, g.N, 3), _randn(s + 8, g.N, 3)
    c = _case(lambda x, W1, b1, W2, b2: frame_mix(F.linear(F.silu(F.linear(x, W1, b1)), W2, b2), basis.to(x.dtype), g.dst, g.N),
              inputs, w)
    c.basis, c.base = basis, base
    _plus(c, "out_base", base)
    return c


# ---------------------------------------------------------------------------------------------------------------- geometry ---
GEOM_C = 32
GEOM_SHIFT = (0.7, -1.1, 0.4)      # the molecules are centred: a 2-atom molecule at (p, -p) would have no frame (p x -p = 0)
U = 2.0 ** -24                     # unit roundoff of fp32


@functools.lru_cache(maxsize=None)
def geometry_case():
    """Positions (fp32), Fourier weights and the fp64 coord2basis / Fourier features of every edge (SDE_model_2D_to_3D.py:35-66,
    342-369), with a tolerance per edge derived from the conditioning of its frame:

      kappa = |r| |c| / |r x c|   (r, c: the two end points; the cross product loses that factor)
      basis       16 u kappa                       each cross component is a difference of two rounded products (2 u |r||c|
                                                   before the normalisation = 2 u kappa after it); vert = diff x cross inherits
                                                   it; 8 x for the normalisations and the three-term sums
      coordinates 2 max(|r|, |c|) * basis          (basis rows . position)
      arguments   2 pi |W| * coordinates + |arg| 2^-23 * 4      (the product x * W * 2 * pi and sinf / cosf at |arg|)
      pseudo-cos  delta = 4 * coordinates / min(|r|, |c|) + 8 u (a quotient of the coordinates by their norms)
      pseudo-sin  sqrt(2 delta):  |sqrt(1 - a^2) - sqrt(1 - b^2)| <= sqrt(|a^2 - b^2|) <= sqrt(2 |a - b|) for |a|, |b| <= 1"""
    g = graph()
    pos = (g.batch.positions + torch.tensor(GEOM_SHIFT)).float()
    Wd, Wc = _randn(41, GEOM_C), _randn(42, GEOM_C)
    P, wd, wc = pos.double(), Wd.double(), Wc.double()
    r, c = P[g.src], P[g.dst]
    diff, cross = r - c, torch.cross(r, c, dim=-1)
    dist = diff.norm(dim=-1, keepdim=True)
    cn = cross.norm(dim=-1, keepdim=True)
    diff, cross = diff / (dist + 1e-6), cross / (cn + 1e-6)
    vert = torch.cross(diff, cross, dim=-1)
    frame = torch.stack([diff, cross, vert], dim=1)                        # [E, 3, 3]
    ci, cj = (frame @ r[:, :, None]).squeeze(-1), (frame @ c[:, :, None]).squeeze(-1)
    ci[:, 1], cj[:, 1] = ci[:, 1].abs(), cj[:, 1].abs()
    two_pi = 2 * math.pi

    def fourier(x, W):                                                     # x [E, 1] -> (args [E, C], [sin | cos])
        a = x * W[None, :] * two_pi
        return a, torch.cat([a.sin(), a.cos()], dim=-1)
    a_d, feat_d = fourier(dist, wd)
    args, feats = {}, {}
    for n, co in (("i", ci), ("j", cj)):
        a0, f0 = fourier(co[:, 0:1], wc)
        a2, f2 = fourier(co[:, 2:3], wc)
        args[n], feats[n] = torch.cat([a0, a0, a2, a2], dim=-1), torch.cat([f0, f2], dim=-1)
    pcos = (ci * cj).sum(-1) / (ci.norm(dim=-1) + 1e-6) / (cj.norm(dim=-1) + 1e-6)
    psin = torch.sqrt(1 - pcos ** 2)
    rn, cnorm = r.norm(dim=-1), c.norm(dim=-1)
    kappa = rn * cnorm / cn.squeeze(-1)
    t_basis = 16 * U * kappa
    t_coord = 2 * torch.maximum(rn, cnorm) * t_basis
    t_arg = two_pi * wc.abs()[None, :].repeat(1, 4) * t_coord[:, None]     # [E, 4C], column order of feat_i / feat_j
    delta = 4 * t_coord / torch.minimum(rn, cnorm) + 8 * U
    return types.SimpleNamespace(
        pos=pos, Wd=Wd, Wc=Wc, kappa=kappa,
        ref={"feat_d": feat_d, "basis": frame.reshape(-1, 9), "feat_i": feats["i"], "feat_j": feats["j"], "pcos": pcos, "psin": psin},
        tol={"feat_d": torch.cat([a_d, a_d], dim=-1).abs() * 2.0 ** -23 * 4 + 2 * U, "basis": t_basis[:, None].expand(-1, 9),
             "feat_i": t_arg + args["i"].abs() * 2.0 ** -23 * 4, "feat_j": t_arg + args["j"].abs() * 2.0 ** -23 * 4,
             "pcos": delta, "psin": torch.sqrt(2 * delta)})


def geometry_fp32():
    """The same features evaluated in fp32 on the CPU (oracle/restate.py's coord2basis and Fourier projection): the host test
    holds them to the per-edge tolerances above, so that the derived bounds are ones an honest fp32 evaluation meets."""
    from oracle import restate as R
    g, gc = graph(), geometry_case()
    pos = gc.pos
    cd, cc, cv = R.coord2basis(pos, g.src, g.dst)
    eb = torch.stack([cd, cc, cv], dim=1)
    ci = torch.matmul(eb, pos[g.src].unsqueeze(-1)).squeeze(-1)
    cj = torch.matmul(eb, pos[g.dst].unsqueeze(-1)).squeeze(-1)
    ci[:, 1], cj[:, 1] = ci[:, 1].abs(), cj[:, 1].abs()
    fd, fc = R.GaussianFourierProjection(GEOM_C), R.GaussianFourierProjection(GEOM_C)
    fd.W.data, fc.W.data = gc.Wd, gc.Wc
    emb = lambda co: torch.cat([fc(co[:, 0:1]), fc(co[:, 2:3])], dim=-1)    # noqa: E731
    pcos = (ci * cj).sum(-1) / (ci.norm(dim=-1) + 1e-6) / (cj.norm(dim=-1) + 1e-6)
    with torch.no_grad():
        return {"feat_d": fd((pos[g.src] - pos[g.dst]).norm(dim=-1, keepdim=True)), "basis": torch.cat([cd, cc, cv], dim=1),
                "feat_i": emb(ci), "feat_j": emb(cj), "pcos": pcos, "psin": torch.sqrt(1 - pcos ** 2)}


# ------------------------------------------------------------------------------------------------------------ comparison ---
def class_errors(got, ref, row_deg):
    """Worst |got - ref| / max |ref| over the rows of each in-degree class (None: no such rows); row_deg: in-degree of the node a
    row belongs to (node rows: the node; edge rows: the target), or None for tensors without such rows (weights)."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf)) / (scale if scale > 0 else 1.0)
    if row_deg is None:
        return [("all", float(err.max()))]
    out = []
    for name, lo, hi in DEG_CLASSES:
        rows = (row_deg >= lo) & (row_deg <= hi)
        out.append((name, float(err[rows].max()) if bool(rows.any()) and err[rows].numel() else None))
    return out


def compare(case, name, got, ref, yard, row_deg, failures):
    """Record yardstick, tolerance and achieved error per in-degree class of one output; add what misses to `failures`."""
    tol = TOL_FACTOR * yard
    errs = class_errors(got, ref, row_deg)
    H_.record_parity(f"score_graph {case} {name}: yardstick {yard:.2e} tol {tol:.2e} achieved "
                     + ", ".join(f"{n} {'-' if e is None else f'{e:.2e}'}" for n, e in errs))
    failures += [f"{case} {name} {n}: {e:.3e} > {tol:.3e}" for n, e in errs if e is not None and not e <= tol]
