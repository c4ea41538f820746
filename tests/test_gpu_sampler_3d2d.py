"""The 3D->2D predictor-corrector sampler (moleculesde_amd/sampler_3d2d.py, csrc/dense_pc.hip) on the GPU: against the
fixture the genuine reference classes produced (tests/golden/sampler_3d2d.npz), fused vs operator path at production size,
graph replay, determinism, invariants, launches and refusals."""
import numpy as np
import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _model(sde_type, F, lo, hi, dev):
    from moleculesde_amd.geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense
    m = SDEModel3Dto2D_node_adj_dense(dim3D=F, nhid=16, num_layers=4, num_linears=3, c_hid=8, c_final=4, adim=16, emb_dim=F,
                                      beta_min=lo, beta_max=hi, num_diffusion_timesteps=1000, c_init=2, num_heads=4,
                                      SDE_type=sde_type)
    return m.to(dev).eval()


def _batch(sizes, dev, seed=5, bondless=None):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_batch
    b = make_batch(len(sizes), seed=seed, sizes=sizes)
    if bondless is not None:       # drop every bond of one atom: node_flags = 0 for it (App. B.5)
        keep = (b.edge_index[0] != bondless) & (b.edge_index[1] != bondless)
        b.edge_index, b.edge_attr = b.edge_index[:, keep], b.edge_attr[keep]
    return G.prepare_batch(b, dev)


def _golden_setup(tag, dev):
    g = load_golden("sampler_3d2d.npz")
    lo, hi = (float(v) for v in g[f"{tag}.range"])
    m = _model(tag.upper(), g["rep"].shape[-1], lo, hi, dev)
    sd = {k[3:]: torch.from_numpy(v.astype(np.float32)) for k, v in g.items() if k.startswith("sd.")}
    m.load_state_dict(sd)
    sizes = [int(s) for s in g["sizes"]]
    b = _batch(sizes, dev)
    noises = {k[6:]: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in g.items() if k.startswith("noise.")}
    flags = torch.from_numpy(g["flags"]).to(dev)
    rep = torch.from_numpy(g["rep"]).to(dev)
    return g, m, b, noises, flags, rep, sizes


def _rows(sizes, Nm):
    return torch.cat([torch.arange(n) + b * Nm for b, n in enumerate(sizes)])


def _check(got, ref, flags_pad, what, rtol=1e-3, atol=1e-4):
    got = got.detach().cpu()
    ref = torch.as_tensor(ref).float()
    err = (got - ref).abs() - rtol * ref.abs()
    assert float(err.max()) <= atol, (what, float(err.max()))


@pytest.mark.parametrize("tag", ["ve", "vp"])
@pytest.mark.parametrize("path", ["fused", "ops"])
def test_fixture_trajectory(dev, tag, path):
    """5 iterations of VE / VP with n_steps = 2 and the injected draws: every iteration's (x, adj, x_mean, adj_mean) within
    rtol 1e-3 / atol 1e-4, exactly 0 outside the flags; the first evaluation's scores too (fused: the corrector's score buffers;
    operator path: get_score_fn)."""
    from moleculesde_amd import sampler_3d2d as S
    g, m, b, noises, flags, rep, sizes = _golden_setup(tag, dev)
    B, Nm = flags.shape
    ncls = m.num_class_X
    rows = _rows(sizes, Nm)
    fm = (flags[:, :, None] * flags[:, None, :]).cpu()
    m.allow_operator_path = path == "ops"
    _, _, _, _, _, _, batch, local, _, h3 = S._layout(b, rep, None, None, flags)
    for it in range(5):
        if path == "fused":
            out = S.node_adj_PC_generation(rep, b, m, n_steps=2, max_iters=it + 1, flags=flags, noises=noises, use_graph=False)
        else:
            out = S._generate_ops(m, h3, batch, local, flags, B, Nm, ncls, 1000, it + 1, float(g["eps"]), 0.2, 0.9, 2, None,
                                  None, noises)
        x, adj, x_mean, adj_mean = (t.detach().cpu() for t in out)
        for name, t in (("x", x), ("x_mean", x_mean)):
            _check(t.reshape(B * Nm, ncls)[rows], g[f"{tag}.it{it}.{name}"], flags, f"{tag} {path} it{it} {name}")
            assert not (t * (1 - flags.cpu()[:, :, None])).any()
        for name, t in (("adj", adj), ("adj_mean", adj_mean)):
            _check(t, g[f"{tag}.it{it}.{name}"], flags, f"{tag} {path} it{it} {name}")
            assert not (t * (1 - fm)).any()
    if path == "fused":
        from moleculesde_amd.geom3d import dense_head as DH
        pl = S._layout(b, rep, None, None, flags)
        _, dn, B_, Nm_, mol_ptr, sizes_, batch, local, flags_, h3 = pl
        pair_ptr = DH.ragged_layout(mol_ptr)
        cfg = DH.types.SimpleNamespace(N=h3.size(0), P=int(pair_ptr[-1]), B=B, n_max=max(sizes), mol_ptr=mol_ptr, pair_ptr=pair_ptr)
        _, par = S.step_table(m.sde_adj, 1000, float(g["eps"]))
        pc = S.FusedPC(m, h3, cfg, flags_[batch, local].contiguous(), Nm, par, 2, 0.2, 0.9, 0, noises)
        G2, OUT = pc.ev(pc.x)
        import ctypes
        S._lib.call("msde_dense_pc_corrector", ctypes.byref(pc.params), S._p(G2), G2.size(1), S._p(pc.ev.w2), S._p(pc.ev.b2),
                    S._p(OUT), S._hip._stream())
        sx = torch.zeros(B * Nm, ncls, device=dev)
        sx[rows.to(dev)] = pc.score_x[:, :ncls]
        _check(sx.view(B, Nm, ncls), g[f"{tag}.score0_x"], flags, "score0 x", 1e-3, 1e-3)
        _check(S.ragged_pairs(torch.from_numpy(g[f"{tag}.score0_adj"]), sizes), pc.score_adj.cpu(), flags, "score0 adj", 1e-3, 1e-3)
    else:
        sfx = m.get_score_fn(m.sde_x, m.node_score_network, train=False)
        sfa = m.get_score_fn(m.sde_adj, m.edge_score_network, train=False)
        x0 = noises["x_init"] * flags[:, :, None]
        a0 = S.sym_noise(noises["adj_init"], flags)
        px = m.embedding_3D(rep) + m.embedding_X(x0)
        t = torch.ones(B, device=dev) * torch.linspace(1, float(g["eps"]), 1000)[0].to(dev)
        _check(sfx(px, a0, flags, t), g[f"{tag}.score0_x"], flags, "get_score_fn x", 1e-3, 1e-3)
        _check(sfa(px, a0, flags, t), g[f"{tag}.score0_adj"], flags, "get_score_fn adj", 1e-3, 1e-3)


def _prod_case(case, dev):
    if case == "replicas":
        sizes, bondless = [14] * 10, None
    elif case == "large":          # the corrector / predictor rows 20..31 and the whole-molecule edge-layer forward
        sizes, bondless = [32, 23, 17, 21, 2], None
    else:
        sizes, bondless = [2, 20, 7, 13, 5, 17, 9, 11], 2 + 20 + 3      # atom 3 of the third molecule
    b = _batch(sizes, dev, seed=11, bondless=bondless)
    return b, sizes


@pytest.mark.parametrize("case", ["replicas", "ragged", "large"])
@pytest.mark.parametrize("sde_type", ["VE", "VP"])
@pytest.mark.parametrize("n_steps", [1, 3])
def test_fused_matches_operator_path_production(dev, case, sde_type, n_steps):
    """emb 300, production head: 10 iterations with injected noise, fused vs operator path within 1e-4 relative."""
    from moleculesde_amd import sampler_3d2d as S
    torch.manual_seed(3)
    m = _model(sde_type, 300, 0.1 if sde_type == "VE" else 0.2, 1.0, dev)
    b, sizes = _prod_case(case, dev)
    B, Nm, I = len(sizes), max(sizes), 10
    rep = torch.randn(b.batch.numel(), 300, device=dev)
    ncls = m.num_class_X
    noises = dict(x_init=torch.randn(B, Nm, ncls, device=dev), adj_init=torch.randn(B, Nm, Nm, device=dev),
                  corr_adj=torch.randn(I, n_steps, B, Nm, Nm, device=dev), corr_x=torch.randn(I, n_steps, B, Nm, ncls, device=dev),
                  pred_adj=torch.randn(I, B, Nm, Nm, device=dev), pred_x=torch.randn(I, B, Nm, ncls, device=dev))
    fused = S.node_adj_PC_generation(rep, b, m, n_steps=n_steps, max_iters=I, noises=noises)
    pl = S._layout(b, rep, None, None, None)
    flags, batch, local = pl[8], pl[6], pl[7]
    if case == "ragged":
        assert float(flags.sum()) == sum(sizes) - 1
    if case == "large":
        assert Nm == 32 and float(flags.sum()) == sum(sizes)
    ops = S._generate_ops(m, rep, batch, local, flags, B, Nm, ncls, 1000, I, 1e-4, 0.2, 0.9, n_steps, None, None, noises)
    for name, f, o in zip(("x", "adj", "x_mean", "adj_mean"), fused, ops):
        scale = float(o.abs().max())
        err = float((f - o).abs().max())
        assert err <= 1e-4 * scale, (name, err, scale)


def _counter_run(dev, seed, use_graph=True, ipg=1, iters=8, sde_type="VE"):
    from moleculesde_amd import sampler_3d2d as S
    torch.manual_seed(7)
    m = _model(sde_type, 64, 0.1, 1.0, dev)
    b, sizes = _prod_case("ragged", dev)
    rep = torch.randn(b.batch.numel(), 64, device=dev)
    return S.node_adj_PC_generation(rep, b, m, max_iters=iters, noise_seed=seed, use_graph=use_graph, iters_per_graph=ipg), sizes


def test_replay_and_determinism(dev):
    """Counter noise: graph replay (also 4 iterations per graph) == eager bitwise; two runs equal; another seed differs."""
    eager, _ = _counter_run(dev, 123, use_graph=False)
    for ipg in (1, 4):
        rep, _ = _counter_run(dev, 123, use_graph=True, ipg=ipg)
        for a, c in zip(eager, rep):
            assert torch.equal(a, c), ipg
    again, _ = _counter_run(dev, 123, use_graph=False)
    assert all(torch.equal(a, c) for a, c in zip(eager, again))
    other, _ = _counter_run(dev, 124, use_graph=False)
    assert not torch.equal(eager[1], other[1]) and not torch.equal(eager[0], other[0])


@pytest.mark.parametrize("sde_type", ["VE", "VP"])
def test_invariants_after_50_iterations(dev, sde_type):
    (x, adj, x_mean, adj_mean), sizes = _counter_run(dev, 9, iters=50, sde_type=sde_type)
    from moleculesde_amd import sampler_3d2d as S
    for t in (x, adj, x_mean, adj_mean):
        assert torch.isfinite(t).all()
    for a in (adj, adj_mean):
        assert torch.equal(a, a.transpose(1, 2))
        assert not a.diagonal(dim1=1, dim2=2).any()
    Nm = max(sizes)
    for bi, n in enumerate(sizes):
        assert not x[bi, n:].any() and not adj[bi, n:].any() and not adj[bi, :, n:].any()
    # the bond-less atom (molecule 2, atom 3)
    assert not x[2, 3].any() and not adj[2, 3].any() and not adj[2, :, 3].any()


def test_launches_one_eager_iteration(dev):
    """Every kernel of an eager iteration comes from libmsde_hip.so; count <= 2 x (one score evaluation) + 4."""
    from torch.profiler import profile, ProfilerActivity
    from moleculesde_amd import sampler_3d2d as S
    from moleculesde_amd.geom3d import dense_head as DH
    torch.manual_seed(1)
    m = _model("VP", 300, 0.2, 1.0, dev)
    b, sizes = _prod_case("replicas", dev)
    rep = torch.randn(b.batch.numel(), 300, device=dev)
    pl = S._layout(b, rep, None, None, None)
    _, _, B, Nm, mol_ptr, sizes, batch, local, flags, h3 = pl
    pair_ptr = DH.ragged_layout(mol_ptr)
    cfg = DH.types.SimpleNamespace(N=h3.size(0), P=int(pair_ptr[-1]), B=B, n_max=max(sizes), mol_ptr=mol_ptr, pair_ptr=pair_ptr)
    _, par = S.step_table(m.sde_adj, 1000)
    pc = S.FusedPC(m, h3, cfg, flags[batch, local].contiguous(), Nm, par, 1, 0.2, 0.9, 5)
    pc.iteration()
    pc.iteration()
    torch.cuda.synchronize()

    def kernels(fn):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    ev = kernels(lambda: pc.ev(pc.x))
    names = kernels(pc.iteration)
    ours = ("dense_", "gemm_ex", "gemm_small", "gemm_rsa", "gemm_t2", "transpose_", "gemm_grouped_wgrad", "reduce_slabs", "colsum",
            "bn_")
    foreign = [n for n in names if not any(k in n for k in ours)]
    assert not foreign, sorted(set(foreign))
    assert len(ev) > 10, ev
    assert len(names) <= 2 * len(ev) + 4, (len(names), len(ev))
    print(f"kernels per score evaluation {len(ev)}, per iteration {len(names)}")


def test_refusals(dev):
    from moleculesde_amd import _lib
    from moleculesde_amd import sampler_3d2d as S
    from moleculesde_amd.geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense_02
    torch.manual_seed(2)
    m = _model("VE", 16, 0.1, 1.0, dev)
    b, sizes = _prod_case("ragged", dev)
    rep = torch.randn(b.batch.numel(), 16, device=dev)
    B, Nm = len(sizes), max(sizes)
    a = torch.randn(B, Nm, Nm, device=dev)
    with pytest.raises(_lib.MsdeHipError):
        S.node_adj_PC_generation(rep, b, m, max_iters=1, adj_init=a)
    m.allow_operator_path = True
    S.node_adj_PC_generation(rep, b, m, max_iters=1, adj_init=a)            # the operator path runs it
    m.allow_operator_path = False
    big = _batch([33, 5], dev)
    with pytest.raises(_lib.MsdeHipError):
        S.node_adj_PC_generation(torch.randn(38, 16, device=dev), big, m, max_iters=1)
    with pytest.raises(NotImplementedError):
        S.node_adj_PC_generation(rep, b, m, probability_flow=True)
    m2 = SDEModel3Dto2D_node_adj_dense_02(dim3D=16, nhid=16, num_layers=4, num_linears=3, c_hid=8, c_final=4, adim=16, emb_dim=16,
                                          beta_min=0.1, beta_max=1.0, num_diffusion_timesteps=1000, c_init=2).to(dev)
    with pytest.raises(NotImplementedError):
        S.node_adj_PC_generation(rep, b, m2)
