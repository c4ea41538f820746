"""The one-workgroup-per-molecule kernels on molecules of 16 to 32 atoms (and the refusals above 32) against fp64.

Every other GPU test builds its molecules with synthetic.make_molecule (2..20 atoms), so the rows 20..31 of the per-molecule
kernels -- the last partial 16-row tiles, the third and fourth trips of the pair loops, the whole-molecule LDS map of the dense
edge layer and the streamed (Em > 384) edge features of the equivariant score kernels -- are run here.  The molecules come from
helpers.build_molecule (exact atom count and bond pattern; tests/test_mol_size_host.py pins the batches on the host).  Every
comparison is elementwise against an fp64 CPU run of the oracle (oracle/restate.py), or against the operator path where the
dropout masks must be identical; the worst error over atom rows [0,16), [16,20) and [20,n) is recorded per case."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restate as R  # noqa: E402
import helpers as H  # noqa: E402
from helpers import assert_close, record_parity  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _sizes(b):
    return torch.bincount(b.batch, minlength=b.num_graphs).tolist()


def _per_mol_close(got, ref, sizes, padded, rtol, atol_scale, what):
    """assert_close molecule by molecule, atol = atol_scale x the largest |ref| of that molecule (a defect confined to a few
    rows of one molecule is not diluted by the rest of the batch)."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    start = 0
    for b, n in enumerate(sizes):
        g, r = (got[b], ref[b]) if padded else (got[start:start + n], ref[start:start + n])
        start += n
        scale = float(r.abs().max()) if r.numel() else 0.0
        assert_close(g, r, rtol, atol_scale * scale, f"{what} (molecule {b}, {n} atoms)")


def _report(tag, what, got, ref, sizes, padded):
    record_parity(f"mol-size {tag}: {what}: worst |err| / scale by atom rows {H.fmt_blocks(H.block_errors(got, ref, sizes, padded))}")


def _param_grads_close(named_got, named_ref, rtol, atol_scale, what):
    """Every parameter gradient; atol scaled by the model's largest fp64 gradient (analytically-zero gradients are rounding)."""
    ref = {k: v.grad for k, v in named_ref if v.grad is not None}
    scale = max(float(v.abs().max()) for v in ref.values())
    worst = 0.0
    n = 0
    for k, p in named_got:
        if k not in ref:
            continue
        assert p.grad is not None, f"{what}: no gradient for {k}"
        assert_close(p.grad, ref[k], rtol, atol_scale * scale, f"{what}:{k}")
        worst = max(worst, float((p.grad.double().cpu() - ref[k]).abs().max()) / scale)
        n += 1
    assert n == len(ref), (n, len(ref))
    return worst


# ------------------------------------------------------------------ dense 3D->2D score networks at the variant boundaries ---
F_HEAD, NOUT = 32, 119


def _head_nets(dev):
    from moleculesde_amd.geom3d import sde_3d_to_2d as S
    kw = dict(dim3D=F_HEAD, nhid=16, num_layers=3, num_linears=3, c_init=2, c_hid=8, c_final=4, adim=16, num_heads=4, conv="MLP")
    edge = S.EdgeScoreNetwork_dense(**kw)
    node = S.NodeScoreNetwork_dense(nfeat=F_HEAD, depth=4, nhid=16, nout=NOUT)
    H.fill_like_generator(edge, 7000)
    H.fill_like_generator(node, 9000)
    oe = R.EdgeScoreNetwork_dense(**kw)
    on = R.NodeScoreNetwork_dense(nfeat=F_HEAD, depth=4, nhid=16, nout=NOUT)
    oe.load_state_dict(edge.state_dict())
    on.load_state_dict(node.state_dict())
    return edge.to(dev), node.to(dev), oe.double(), on.double()


_FWD = re.compile(r"dense_edge_layer_fwd_kernel(?:<(\d+), ?(\d+), ?(\d+)>|ILi(\d+)ELi(\d+)ELi(\d+)E)")


def _edge_fwd_forms(names):
    """(C, CO, split) of every dense_edge_layer_fwd_kernel launch, from demangled or mangled kernel names."""
    forms = set()
    for nm in names:
        if "dense_edge_layer_fwd_kernel" not in nm:
            continue
        m = _FWD.search(nm)
        assert m, f"kernel name without its template arguments: {nm}"
        forms.add(tuple(int(g) for g in (m.groups()[:3] if m.group(1) else m.groups()[3:])))
    return forms


def expected_edge_fwd_forms(n_max):
    """msde_dense_edge_layer_fwd: the split form (two workgroups per molecule) while 2 x its LDS map + 2 KiB fits in 160 KiB --
    (8, 8) up to 22 atoms, (8, 4) up to 23, (2, 8) always -- the whole form (one workgroup) above."""
    return {(2, 8, 1), (8, 8, 1 if n_max <= 22 else 0), (8, 4, 1 if n_max <= 23 else 0)}


@pytest.mark.parametrize("N", [16, 17, 20, 21, 22, 23, 24, 31, 32])
def test_dense_score_networks_vs_fp64(dev, N):
    """geom3d.dense_head.score_networks (csrc/dense_head.hip edge-layer forward / backward, node GCN, on padded N-row
    molecules) against R.EdgeScoreNetwork_dense / R.NodeScoreNetwork_dense in fp64: both scores, the gradient of x and every
    parameter gradient.  Three molecules: N atoms; a dense N-atom molecule with a bondless atom at row N - 2; a smaller one
    padded to N (flags switch the padded rows off).  The profiler shows which forward form of the edge layer ran."""
    from moleculesde_amd import plan as P
    from moleculesde_amd.geom3d import dense_head as DH
    from torch.profiler import profile, ProfilerActivity
    torch.manual_seed(N)
    edge, node, oe, on = _head_nets(dev)
    b = H.build_batch([(N, "random"), (N, "dense", (N - 2,)), (max(N - 5, 2), "random")], seed=N)
    dn = P.dense_plan(P.build_plan(b), b)
    assert dn.N_max == N and _sizes(b)[:2] == [N, N]
    flags = dn.flags
    assert float(flags[1, N - 2]) == 0.0 and float(flags[1].sum()) == N - 1        # the bondless atom is switched off
    z = torch.randn(3, N, N).triu(1)
    adj = (dn.adj + 0.3 * (z + z.transpose(1, 2))) * flags[:, :, None] * flags[:, None, :]
    x = torch.randn(3, N, F_HEAD)
    w_e, w_n = torch.randn(3, N, N), torch.randn(3, N, NOUT)
    assert DH.fused_supported(edge, node, N)

    xd = x.to(dev).requires_grad_(True)
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        se, sn = DH.score_networks(edge, node, xd, adj.to(dev), flags.to(dev))
        torch.cuda.synchronize()
    forms = _edge_fwd_forms([e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])
    assert forms == expected_edge_fwd_forms(N), (N, sorted(forms))
    ((se * w_e.to(dev)).sum() + (sn * w_n.to(dev)).sum()).backward()

    x64 = x.double().requires_grad_(True)
    a64, f64 = adj.double(), flags.double()
    ref_e, ref_n = oe(x64, a64, f64), on(x64, a64, f64)
    ((ref_e * w_e.double()).sum() + (ref_n * w_n.double()).sum()).backward()

    sizes = [N] * 3
    tag = f"score_networks N={N} fwd forms {sorted(forms)}"
    _report(tag, "edge score", se, ref_e, sizes, True)
    _report(tag, "node score", sn, ref_n, sizes, True)
    _report(tag, "grad x", xd.grad, x64.grad, sizes, True)
    _per_mol_close(se, ref_e, sizes, True, 1e-4, 1e-5, "edge score")
    _per_mol_close(sn, ref_n, sizes, True, 1e-4, 1e-5, "node score")
    _per_mol_close(xd.grad, x64.grad, sizes, True, 1e-3, 1e-4, "grad x")
    we = _param_grads_close(edge.named_parameters(), oe.named_parameters(), 1e-3, 1e-4, "edge net")
    wn = _param_grads_close(node.named_parameters(), on.named_parameters(), 1e-3, 1e-4, "node net")
    record_parity(f"mol-size {tag}: parameter gradients worst |err| / model scale: edge {we:.1e} node {wn:.1e}")


# ------------------------------------------------------------------ full 3D->2D losses on ragged large molecules ---
E_3D = 300


def _model_3d2d(dev, seed):
    import moleculesde_amd.geom3d as G
    kw = dict(dim3D=E_3D, c_init=2, c_hid=8, c_final=4, num_heads=4, adim=16, nhid=16, num_layers=4, emb_dim=E_3D,
              num_linears=3, beta_min=0.1, beta_max=1.0, num_diffusion_timesteps=1000, SDE_type="VE", num_class_X=119,
              noise_on_one_hot=True)
    m = G.SDEModel3Dto2D_node_adj_dense(**kw)
    H.fill_like_generator(m, seed)
    om = R.SDEModel3Dto2D_node_adj_dense(**kw)
    om.load_state_dict(m.state_dict())
    return m.to(dev).train(), om.double().train()


def _oracle_losses64(om, cpu_b, h3, seed):
    """The oracle's forward in fp64 under torch.manual_seed(seed); the noise is drawn in fp32 as the replayed product draws it
    (program order of SDE_model_3D_to_2D_node_adj_dense.py:112-146), then widened."""
    orig = torch.randn_like
    dtype = torch.get_default_dtype()
    torch.randn_like = lambda x, **k: orig(x.float()).to(x.dtype)
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(seed)
        return om(h3, cpu_b, continuous=True, train=True, reduce_mean=True, anneal_power=0)
    finally:
        torch.set_default_dtype(dtype)
        torch.randn_like = orig


def _losses_vs_fp64(dev, m, om, cpu_b, tag, seed=31):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.geom3d import dense_head as DH
    b = G.prepare_batch(cpu_b.clone(), dev)
    sizes = _sizes(cpu_b)
    h3 = torch.randn(sum(sizes), E_3D)
    m.noise = G.CpuReplayNoise(seed)
    hd = h3.to(dev).requires_grad_(True)
    calls = DH.FUSED_CALLS
    lx, la = m(hd, b, reduce_mean=True, continuous=True, train=True, anneal_power=0)
    fused = DH.FUSED_CALLS == calls + 1
    (0.7 * lx + 1.3 * la).backward()
    h64 = h3.double().requires_grad_(True)
    rx, ra = _oracle_losses64(om, cpu_b, h64, seed)
    (0.7 * rx + 1.3 * ra).backward()
    record_parity(f"mol-size {tag}: loss_x rel err {abs(float(lx) / float(rx) - 1):.1e}, loss_adj rel err "
                  f"{abs(float(la) / float(ra) - 1):.1e}")
    _report(tag, "grad h3", hd.grad, h64.grad, sizes, False)
    assert_close(lx, rx, 1e-4, 0, "loss_x")
    assert_close(la, ra, 1e-4, 0, "loss_adj")
    _per_mol_close(hd.grad, h64.grad, sizes, False, 1e-3, 1e-4, "grad h3")
    w = _param_grads_close(m.named_parameters(), om.named_parameters(), 1e-3, 1e-4, "3D->2D")
    record_parity(f"mol-size {tag}: parameter gradients worst |err| / model scale {w:.1e}")
    return fused


@pytest.mark.parametrize("n_max", [23, 32])
def test_sde3d2d_losses_ragged_large_vs_fp64(dev, n_max):
    """SDEModel3Dto2D_node_adj_dense on the fused head (dense_prepare, both edge-layer forms, node GCN, loss kernels, the
    N_max loss normaliser) against the fp64 oracle under replayed noise: both losses, the gradient of the 3D representation
    per molecule and every parameter gradient."""
    m, om = _model_3d2d(dev, 5000 + n_max)
    cpu_b = H.build_batch(H.loss_specs(n_max), seed=n_max)
    assert max(_sizes(cpu_b)) == n_max and _sizes(cpu_b) == [s[0] for s in H.loss_specs(n_max)]
    assert _losses_vs_fp64(dev, m, om, cpu_b, f"3D->2D losses n_max={n_max}"), "the fused head kernels must have run"


# ------------------------------------------------------------------ equivariant score kernels past 384 edges ---
def _escore_case(dev, seed, train=False):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import escore, plan as P
    from moleculesde_amd.geom3d import sde_2d_to_3d as M
    torch.manual_seed(seed)
    cpu_b = H.build_batch(H.ESCORE_SPECS, seed=1)
    em = H.mol_edge_counts(cpu_b)
    assert any(H.ES_EAL - 8 <= e <= H.ES_EAL for e in em) and any(e > H.ES_EAL for e in em) and H.ES_EMAX in em, em
    dev_b = G.prepare_batch(cpu_b.clone(), dev)
    pl = P.get_plan(dev_b)
    ep = pl.ext
    assert pl.N_max == 32
    net = M.EquivariantScoreNetwork(32, hidden_coff_dim=128)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.normal_(1, 0.3)
                mod.bias.normal_(0, 0.3)
    net = net.to(dev).train(train)
    assert escore.supported(net, pl)
    x = torch.randn(ep.N, 32)
    ea = torch.randn(ep.E, 32) * 0.7
    basis = torch.randn(ep.E, 9)
    return cpu_b, pl, ep, net, x, ea, basis, em


def _oracle64(net, cpu_b, ep, ea_canon, basis):
    o = R.EquivariantScoreNetwork(32, hidden_coff_dim=128)
    o.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    o = o.double().eval()
    perm = ep.perm_t.cpu()
    ea = torch.empty_like(ea_canon, dtype=torch.float64)
    bs = torch.empty_like(basis, dtype=torch.float64)
    ea[perm] = ea_canon.double()
    bs[perm] = basis.double()
    return o, cpu_b.extended_edge_index, ea, [bs[:, 0:3], bs[:, 3:6], bs[:, 6:9]]


def _escore_grads(net, ep, pl, xd, ed, bd, w, mol):
    from moleculesde_amd.geom3d import sde_2d_to_3d as M
    net.zero_grad(set_to_none=True)
    x = xd.clone().requires_grad_(True)
    e = ed.clone().requires_grad_(True)
    keep = M.MOL_KERNEL_TRAIN
    M.MOL_KERNEL_TRAIN = mol
    try:
        out = net(ep, x, e, bd, pl)["gradient"]
        (out * w).sum().backward()
    finally:
        M.MOL_KERNEL_TRAIN = keep
    return out.detach(), x.grad, e.grad, {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def test_escore_mol_training_path_vs_fp64_past_384_edges(dev):
    """msde_escore_mol_fwd (autograd variant) + msde_escore_mol_bwd without dropout against the fp64 oracle's autograd: score,
    node-feature gradient, edge-feature gradient (per molecule, streamed when Em > 384) and every parameter gradient."""
    cpu_b, pl, ep, net, x, ea, basis, em = _escore_case(dev, 3)
    sizes = _sizes(cpu_b)
    xd, ed, bd = x.to(dev), ea.to(dev), basis.to(dev)
    w = torch.randn(ep.N, 3)
    out, gx, ge, gp = _escore_grads(net, ep, pl, xd, ed, bd, w.to(dev), True)
    o, ei, ea_o, basis_o = _oracle64(net, cpu_b, ep, ea, basis)
    xo = x.double().requires_grad_(True)
    eo = ea_o.clone().requires_grad_(True)
    ref = o(ei, xo, eo, basis_o)["gradient"]
    (ref * w.double()).sum().backward()
    perm = ep.perm_t.cpu()
    tag = f"escore training path Em={em}"
    _report(tag, "score", out, ref, sizes, False)
    _report(tag, "grad x", gx, xo.grad, sizes, False)
    _per_mol_close(out, ref, sizes, False, 1e-4, 2e-5, "score")
    _per_mol_close(gx, xo.grad, sizes, False, 2e-4, 5e-5, "g node features")
    _per_mol_close(ge, eo.grad[perm], em, False, 2e-4, 5e-5, "g edge features")
    og = {k: p.grad for k, p in o.named_parameters() if p.grad is not None}
    oscale = max(float(v.abs().max()) for v in og.values())
    assert set(og) <= set(gp)
    for k, v in og.items():
        assert_close(gp[k], v, 2e-4, 5e-5 * oscale, f"grad {k}")


def test_escore_mol_training_path_dropout_vs_operator_path_past_384_edges(dev):
    """Dropout on: the one-launch forward / backward against the operator path with the identical masks."""
    cpu_b, pl, ep, net, x, ea, basis, em = _escore_case(dev, 4, train=True)
    sizes = _sizes(cpu_b)
    xd, ed, bd = x.to(dev), ea.to(dev), basis.to(dev)
    wd = torch.randn(ep.N, 3).to(dev)
    net._calls = 7
    o1, gx1, ge1, gp1 = _escore_grads(net, ep, pl, xd, ed, bd, wd, True)
    net._calls = 7
    o2, gx2, ge2, gp2 = _escore_grads(net, ep, pl, xd, ed, bd, wd, False)
    _report(f"escore dropout Em={em}", "score vs operator path", o1, o2, sizes, False)
    _per_mol_close(o1, o2, sizes, False, 1e-5, 2e-6, "forward (training variant)")
    _per_mol_close(gx1, gx2, sizes, False, 1e-4, 2e-5, "g node features")
    _per_mol_close(ge1, ge2, em, False, 1e-4, 2e-5, "g edge features")
    assert set(gp1) == set(gp2)
    scale = max(float(v.abs().max()) for v in gp2.values())
    for k in gp2:
        assert_close(gp1[k], gp2[k], 1e-4, 2e-5 * scale, f"grad {k}")
    net.eval()
    with torch.no_grad():
        clean = net(ep, xd, ed, bd, pl)["gradient"]
    assert not torch.allclose(o1, clean)                  # dropout was really on


def test_escore_mol_forward_nograd_vs_fp64_past_384_edges(dev):
    """escore.forward_nograd (msde_escore_mol_fwd, inference variant) against fp64."""
    from moleculesde_amd import escore
    cpu_b, pl, ep, net, x, ea, basis, em = _escore_case(dev, 5)
    sizes = _sizes(cpu_b)
    with torch.no_grad():
        got = escore.forward_nograd(net, ep, pl, x.to(dev), ea.to(dev), basis.to(dev), 0, None)
    o, ei, ea_o, basis_o = _oracle64(net, cpu_b, ep, ea, basis)
    with torch.no_grad():
        ref = o(ei, x.double(), ea_o, basis_o)["gradient"]
    _report(f"escore forward_nograd Em={em}", "score", got, ref, sizes, False)
    _per_mol_close(got, ref, sizes, False, 1e-4, 2e-5, "forward_nograd")


def _score_models(dev, cls):
    import moleculesde_amd.geom3d as G
    kw = dict(emb_dim=32, hidden_dim=32, beta_min=0.1, beta_max=1.0, num_diffusion_timesteps=1000, beta_schedule=None,
              SDE_type="VE", use_extend_graph=True)
    model = getattr(G, cls)(**kw).to(dev).eval()
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.normal_(1, 0.3)
                mod.bias.normal_(0, 0.3)
    o = getattr(R, cls)(**kw)
    o.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return model, o.double().eval()


def score_raw_fp64(o, rep, cpu_b, pos):
    """The oracle's get_score network output (before -1 / std) in fp64."""
    ei = cpu_b.extended_edge_index
    with torch.no_grad():
        node_attr, edge_attr, basis = o._edge_and_node_features(rep.detach().cpu().double(), pos.detach().cpu().double(), ei)
        return o.score_network(ei, node_attr, edge_attr, basis)["gradient"]


@pytest.mark.parametrize("cls", ["SDEModel2Dto3D_02", "SDEModel2Dto3D_01"])
def test_escore_get_score_vs_fp64_past_384_edges(dev, cls):
    """get_score_raw on msde_escore_mol_score (per-edge launch + one workgroup per molecule) and get_score against fp64, at
    a small and a large diffusion time.  Bar as test_get_score_fused_matches_operator_path (hardware sin in the Fourier
    features)."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import escore, plan as P
    from moleculesde_amd.geom3d import sde_2d_to_3d as M
    torch.manual_seed(11)
    cpu_b = H.build_batch(H.ESCORE_SPECS, seed=1)
    em = H.mol_edge_counts(cpu_b)
    assert H.ES_EMAX in em and any(e > H.ES_EAL for e in em)
    sizes = _sizes(cpu_b)
    b = G.prepare_batch(cpu_b.clone(), dev)
    model, o = _score_models(dev, cls)
    gnn = G.GNN(3, 32, gnn_type="GIN").to(dev).eval()
    with torch.no_grad():
        rep = gnn(b.x, b.edge_index, b.edge_attr)
    pl = P.get_plan(b)
    assert escore.score_supported(model, pl) and M.MOL_KERNEL and M.MOL_KERNEL_SCORE
    for scale in (0.3, 6.0):
        pos = (b.positions + scale * torch.randn_like(b.positions)).contiguous()
        got = model.get_score_raw(rep, b, pos)
        ref = score_raw_fp64(o, rep, cpu_b, pos)
        _report(f"escore get_score_raw {cls} pos noise {scale} Em={em}", "score", got, ref, sizes, False)
        _per_mol_close(got, ref, sizes, False, 2e-4, 2e-4, f"get_score_raw (noise {scale})")
        t = torch.full((pos.size(0),), 0.37, device=dev)
        sc = model.get_score(rep, b, pos, None, t)
        _, std = o.sde_pos.marGINal_prob(pos.cpu().double(), t.cpu().double())
        _per_mol_close(sc, -ref / std[:, None], sizes, False, 2e-4, 2e-4, f"get_score (noise {scale})")


# ------------------------------------------------------------------ 33 and 40 atoms: refused, operator path on request ---
def test_above_32_atoms_refused_and_operator_path_vs_fp64(dev):
    """Molecules of 33 and 40 atoms: no fused kernel claims them (fused_supported, escore.supported, score_supported); the
    3D->2D model raises MsdeHipError unless allow_operator_path is set, and with it matches the fp64 oracle."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import escore, plan as P
    from moleculesde_amd._lib import MsdeHipError
    from moleculesde_amd.geom3d import dense_head as DH
    from moleculesde_amd.geom3d import sde_2d_to_3d as M
    m, om = _model_3d2d(dev, 6100)
    assert DH.fused_supported(m.edge_score_network, m.node_score_network, 32)
    for n in (33, 40):
        assert not DH.fused_supported(m.edge_score_network, m.node_score_network, n)
    net = M.EquivariantScoreNetwork(32, hidden_coff_dim=128).to(dev)
    s23, _ = _score_models(dev, "SDEModel2Dto3D_02")
    for n in (33, 40):
        cb = H.build_batch([(n, "random"), (5, "chain")], seed=n)
        pl = P.get_plan(G.prepare_batch(cb.clone(), dev))
        assert pl.N_max == n and not escore.supported(net, pl) and not escore.score_supported(s23, pl)
    cpu_b = H.build_batch([(40, "random"), (33, "dense"), (17, "random"), (2, "chain")], seed=40)
    b = G.prepare_batch(cpu_b.clone(), dev)
    m.noise = G.CpuReplayNoise(3)
    with pytest.raises(MsdeHipError, match="allow_operator_path"):
        m(torch.randn(b.x.size(0), E_3D, device=dev), b, reduce_mean=True, continuous=True, train=True, anneal_power=0)
    m.allow_operator_path = True
    assert not _losses_vs_fp64(dev, m, om, cpu_b, "3D->2D operator path n_max=40"), "the fused head must not have run"
