"""The 2D->3D score network's graph kernels (edge attention in both kernel forms, frame mix + mean, its fusion with the basis
MLP, per-edge geometry) on a graph with in-degrees 0, 1, 2, 7..16, 63, 64, 65 and 99, a first and a last node without
in-edges and N = 347 (helpers.SCORE_GRAPH_SPECS; pinned by tests/test_score_graph_host.py), through the entry points the model
calls (hip.edge_attention_fused, hip.edge_geometry_stacked, hip.mlp_head_mix) as well as the plain ones.

Every reference is fp64 autograd on the CPU from the fp32 inputs (tests/score_graph_cases.py); every element is compared.
Tolerance of an output: 8 x the error of an fp32 CPU evaluation of the same operation against fp64, relative to the largest
reference magnitude (the geometry has per-edge tolerances derived from the conditioning of the frame instead).  Each
comparison records yardstick, tolerance and achieved error per in-degree class (0, 1-7, 8-63, 64 and above)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import score_graph_cases as S  # noqa: E402
from helpers import record_parity  # noqa: E402
from moleculesde_amd import slabs  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()  # fails loudly if libmsde_hip.so is missing
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def plan(dev):
    return S.device_plan(dev)


# ------------------------------------------------------------------------------------------------------------ attention ---
def _run_attention(dev, plan, label, c, heads, p=0.0, seed=0, seed_dev=None):
    """hip.edge_attention and hip.edge_attention_fused ([N, 4D] buffer, random skip block) on the inputs of case c: output and
    the gradients of q, k, v, ee (and skip) against c.ref."""
    from moleculesde_amd import hip
    g = S.graph()
    node_deg, edge_deg = g.deg, g.deg[g.dst]
    D = c.w.size(1)
    sd = torch.tensor([seed_dev], dtype=torch.int64, device=dev) if seed_dev is not None else None
    wd = c.w.to(dev)
    failures = []

    ds = {n: c.inputs[n].to(dev).requires_grad_(True) for n in ("q", "k", "v", "ee")}
    out = hip.edge_attention(ds["q"], ds["k"], ds["v"], ds["ee"], plan, heads, p, seed, sd)
    (out * wd).sum().backward()
    S.compare(label + " plain", "out", out, c.ref["out"], c.yard["out"], node_deg, failures)
    for n in ("q", "k", "v", "ee"):
        S.compare(label + " plain", "g_" + n, ds[n].grad, c.ref["g_" + n], c.yard["g_" + n], edge_deg if n == "ee" else node_deg,
                  failures)

    qkvs = torch.cat([c.inputs["q"], c.inputs["k"], c.inputs["v"], c.skip], dim=1).to(dev).requires_grad_(True)
    ee = c.inputs["ee"].to(dev).requires_grad_(True)
    out = hip.edge_attention_fused(qkvs, ee, plan, heads, p, seed, sd)
    (out * wd).sum().backward()
    S.compare(label + " fused", "out", out, c.ref["out_skip"], c.yard["out_skip"], node_deg, failures)
    for j, n in enumerate(("q", "k", "v")):
        S.compare(label + " fused", "g_" + n, qkvs.grad[:, j * D:(j + 1) * D], c.ref["g_" + n], c.yard["g_" + n], node_deg, failures)
    S.compare(label + " fused", "g_ee", ee.grad, c.ref["g_ee"], c.yard["g_ee"], edge_deg, failures)
    assert torch.equal(qkvs.grad[:, 3 * D:].cpu(), c.w), f"{label} fused: g_skip is the incoming gradient itself"
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("heads,Ch", [(8, 4), (4, 8), (2, 2)])
def test_attention_every_in_degree(dev, plan, heads, Ch):
    """Wave-per-target kernels (8 x 4) and thread-per-(target, head) kernels (4 x 8, 2 x 2) at unit scale."""
    _run_attention(dev, plan, f"attention {heads}x{Ch}", S.attention_case(heads, Ch), heads)


@pytest.mark.parametrize("heads,Ch", [(8, 4), (2, 2)])
def test_attention_large_logits(dev, plan, heads, Ch):
    """q scaled by 40, logits of a few hundred: finite and within tolerance only with the maximum subtracted."""
    _run_attention(dev, plan, f"large logits {heads}x{Ch}", S.attention_case(heads, Ch, qscale=40.0), heads)


@pytest.mark.parametrize("heads,Ch", [(8, 4), (2, 2)])
@pytest.mark.parametrize("p,seed_dev", [(0.1, None), (0.5, None), (0.1, 5)])
def test_attention_dropout_exact_mask(dev, plan, heads, Ch, p, seed_dev):
    """Dropout on alpha with the mask rebuilt on the host (msde_uniform(seed', e * H + h) >= p, seed' = seed + seed_dev * FNV)
    and applied in the fp64 reference: output and all gradients, the softmax-backward term under the mask included."""
    c = S.attention_case(heads, Ch, p=p, seed=1234, seed_dev=seed_dev)
    _run_attention(dev, plan, f"dropout {heads}x{Ch} p {p} seed_dev {seed_dev}", c, heads, p, 1234, seed_dev)


@pytest.mark.parametrize("heads,Ch", [(8, 4), (2, 2)])
def test_shared_edge_projection(dev, plan, heads, Ch):
    """Three fused layers reading column blocks of one ee_all [E, 3D] through one `shared` dict: every block of the gradient of
    ee_all matches fp64, exactly one layer's backward returns the buffer, the dict is empty afterwards, and a second pass
    through the same dict gives the same result."""
    from moleculesde_amd import hip
    g = S.graph()
    c = S.shared_projection_case(heads, Ch)
    L, D = S.SHARED_LAYERS, heads * Ch
    node_deg, edge_deg = g.deg, g.deg[g.dst]
    ee_all = c.inputs["ee_all"].to(dev).requires_grad_(True)
    qkvs = [torch.cat([c.inputs[f"{n}{l}"] for n in "qkvs"], dim=1).to(dev).requires_grad_(True) for l in range(L)]
    wd = c.w.to(dev)
    shared = {}

    def run():
        returned, outs = [], []
        for l in range(L):
            ee_l = ee_all.view(g.E, L * D)       # an autograd edge of this layer alone: the hook sees what its backward returned
            ee_l.register_hook(lambda gr, l=l: returned.append((l, tuple(gr.shape))) if gr is not None else None)
            outs.append(hip.edge_attention_fused(qkvs[l], ee_l, plan, heads, 0.0, 0, None, l * D, shared))
        out = torch.cat(outs, dim=1)
        (out * wd).sum().backward()
        assert shared == {}
        res = (out.detach().clone(), ee_all.grad.clone(), [t.grad.clone() for t in qkvs], returned)
        ee_all.grad = None
        for t in qkvs:
            t.grad = None
        return res

    out, g_ee, g_qkvs, returned = run()
    assert len(returned) == 1 and returned[0][1] == (g.E, L * D), returned
    failures = []
    label = f"shared projection {heads}x{Ch}"

    def block(name, l):      # column block l of an output: reference, and the yardstick of that block alone
        ref, low = c.ref[name][:, l * D:(l + 1) * D], c.low[name][:, l * D:(l + 1) * D]
        return ref, float((low - ref).abs().max()) / float(ref.abs().max())
    for l in range(L):
        S.compare(label, f"out[{l}]", out[:, l * D:(l + 1) * D], *block("out", l), node_deg, failures)
        S.compare(label, f"g_ee_all[{l}]", g_ee[:, l * D:(l + 1) * D], *block("g_ee_all", l), edge_deg, failures)
        for j, n in enumerate("qkv"):
            S.compare(label, f"g_{n}{l}", g_qkvs[l][:, j * D:(j + 1) * D], c.ref[f"g_{n}{l}"], c.yard[f"g_{n}{l}"], node_deg, failures)
        assert torch.equal(g_qkvs[l][:, 3 * D:].cpu(), c.w[:, l * D:(l + 1) * D])
    assert not failures, "\n".join(failures)
    out2, g_ee2, g_qkvs2, returned2 = run()
    assert len(returned2) == 1
    assert torch.equal(out2, out) and torch.equal(g_ee2, g_ee) and all(torch.equal(a, b) for a, b in zip(g_qkvs2, g_qkvs))


def test_attention_backward_rejects_short_row_strides(dev, plan):
    """msde_edge_attention_bwd checks ld and ldg like the forward checks ld: MSDE_EINVAL before any launch.  (Every buffer has
    its full size, so the shorter stride would stay inside it.)"""
    from moleculesde_amd import _lib
    from moleculesde_amd._torchabi import _p, _stream
    g = S.graph()
    heads, Ch, D = 8, 4, 32
    node = lambda: torch.zeros(g.N, D, device=dev)      # noqa: E731
    edge = lambda: torch.zeros(g.E, D, device=dev)      # noqa: E731
    go, q, k, v, g_skip, g_q = (node() for _ in range(6))
    ee, g_ee, g_kpe, g_vpe = (edge() for _ in range(4))
    alpha = torch.zeros(g.E, heads, device=dev)
    fn = _lib.load().msde_edge_attention_bwd

    def call(ld, gs, ldg):
        return fn(_p(go), _p(q), _p(k), _p(v), ld, _p(gs), ldg, _p(ee), 0, _p(alpha), _p(plan.rowptr), _p(plan.src), g.N, heads, Ch,
                  0.0, 0, _p(None), _p(g_q), _p(g_ee), _p(g_kpe), _p(g_vpe), 0, _stream())
    EINVAL = -1
    assert call(D - 4, None, D) == EINVAL
    assert call(D, g_skip, D - 4) == EINVAL
    assert call(D, None, D - 4) == EINVAL               # g_q has the row stride ldg too
    assert call(D, g_skip, D) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- frame mix, fused head ---
@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("spare", [0, 37])
def test_frame_mix_mean_every_in_degree(dev, with_base, spare):
    """spare: a plan with capacity for 37 more edges than the graph has (rows past rowptr[N] never read -- they hold NaN -- and
    their gradient rows zero)."""
    from moleculesde_amd import hip
    g = S.graph()
    c = S.frame_mix_case()
    pl = S.device_plan(dev, spare)
    pad = lambda t: torch.cat([t, torch.full((spare, t.size(1)), float("nan"))]) if spare else t      # noqa: E731
    cd = pad(c.inputs["coff"]).to(dev).requires_grad_(True)
    based = c.base.to(dev).requires_grad_(True) if with_base else None
    out = hip.frame_mix_mean(cd, pad(c.basis).to(dev).contiguous(), pl, based)
    (out * c.w.to(dev)).sum().backward()
    failures = []
    label = f"frame mix base {with_base} spare {spare}"
    name = "out_base" if with_base else "out"
    S.compare(label, "out", out, c.ref[name], c.yard[name], g.deg, failures)
    assert cd.grad.shape == (g.E + spare, 3)
    S.compare(label, "g_coff", cd.grad[:g.E], c.ref["g_coff"], c.yard["g_coff"], g.deg[g.dst], failures)
    if spare:
        assert bool((cd.grad[g.E:] == 0).all()), "gradient rows past rowptr[N]"
    if with_base:
        assert torch.equal(based.grad.cpu(), c.w)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("hidden", [128, 32])
@pytest.mark.parametrize("with_base", [False, True])
def test_mlp_head_mix_every_in_degree(dev, plan, hidden, with_base):
    """hip.mlp_head_mix (basis MLP + frame mix + mean + running sum) inside a parameter-gradient batch (queued slabs) and
    outside one: output, g_x, both Linear layers' gradients, g_base."""
    from moleculesde_amd import hip
    from moleculesde_amd.geom3d import nn as mnn
    g = S.graph()
    c = S.head_mix_case(hidden)
    bd, wd = c.basis.to(dev).contiguous(), c.w.to(dev)
    failures = []
    for batched in (False, True):
        d1, d2 = mnn.Linear(S.MLP_IN, hidden).to(dev), mnn.Linear(hidden, 3).to(dev)
        with torch.no_grad():
            d1.weight.copy_(c.inputs["W1"]); d1.bias.copy_(c.inputs["b1"])
            d2.weight.copy_(c.inputs["W2"]); d2.bias.copy_(c.inputs["b2"])
        xd = c.inputs["x"].to(dev).requires_grad_(True)
        based = c.base.to(dev).requires_grad_(True) if with_base else None
        assert hip.mlp_head_mix_ok(xd, d1, d2)
        if batched:
            slabs.begin_param_grad_batch([d1.weight, d1.bias, d2.weight, d2.bias])
        try:
            out = hip.mlp_head_mix(xd, d1, d2, bd, plan, based)
            (out * wd).sum().backward()
        finally:
            if batched:
                slabs.flush_wgrad_gemms()
                slabs.finish_param_grad_batch()
        label = f"head mix H {hidden} base {with_base} batched {batched}"
        name = "out_base" if with_base else "out"
        S.compare(label, "out", out, c.ref[name], c.yard[name], g.deg, failures)
        S.compare(label, "g_x", xd.grad, c.ref["g_x"], c.yard["g_x"], g.deg[g.dst], failures)
        for n, t in (("W1", d1.weight), ("b1", d1.bias), ("W2", d2.weight), ("b2", d2.bias)):
            S.compare(label, "g_" + n, t.grad, c.ref["g_" + n], c.yard["g_" + n], None, failures)
        if with_base:
            assert torch.equal(based.grad.cpu(), c.w)
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------- geometry ---
def test_edge_geometry_stacked_layout(dev, plan):
    """hip.edge_geometry_stacked (interleaved feat rows, float4 angle slot in X) against fp64 with the per-edge tolerances of
    score_graph_cases.geometry_case (no edge masked out), and bit for bit against hip.edge_geometry."""
    from moleculesde_amd import hip
    g = S.graph()
    gc = S.geometry_case()
    C = Hd = S.GEOM_C
    pos, Wd, Wc = gc.pos.to(dev), gc.Wd.to(dev), gc.Wc.to(dev)
    feat_d, feat, X, basis = hip.edge_geometry_stacked(pos, plan, Wd, Wc, Hd)
    assert feat_d.shape == (g.E, 2 * C) and feat.shape == (2 * g.E, 4 * C) and X.shape == (2 * g.E, Hd + 4)
    got = {"feat_d": feat_d, "basis": basis, "feat_i": feat[0::2], "feat_j": feat[1::2], "psin": X[0::2, Hd], "pcos": X[0::2, Hd + 1]}
    failures = []
    for name, ref in gc.ref.items():
        t = got[name].double().cpu()
        assert t.shape == ref.shape, name
        err = (t - ref).abs()
        bad = ~(err <= gc.tol[name])                      # NaN counts as a miss
        record_parity(f"score_graph geometry {name}: worst err {float(err.max()):.2e}, worst err / tolerance "
                      f"{float((err / gc.tol[name]).max()):.3f} (tolerance {float(gc.tol[name].min()):.1e} .. "
                      f"{float(gc.tol[name].max()):.1e} per edge)")
        if bool(bad.any()):
            failures.append(f"{name}: {int(bad.sum())}/{bad.numel()} outside the tolerance")
    assert not failures, "\n".join(failures)
    assert bool((X[0::2, Hd + 2:] == 0).all()) and bool((X[1::2, Hd:] == 0).all())
    fd2, fi2, fj2, ang2, basis2 = hip.edge_geometry(pos, plan, Wd, Wc)
    assert torch.equal(fd2, feat_d) and torch.equal(basis2, basis)
    assert torch.equal(fi2, feat[0::2]) and torch.equal(fj2, feat[1::2])
    assert torch.equal(ang2, X[0::2, Hd:Hd + 2])
