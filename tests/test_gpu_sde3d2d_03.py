"""SDEModel3Dto2D_node_adj_dense_03 on the GPU (SDE_model_3D_to_2D_node_adj_dense.py:352-521): the fused dense head and the
operator path against the fixture produced by the reference's own class (tools/make_golden_f3_03.py), the fused head against
the operator path at production dimensions, the three Trainer step paths, the conditioned node-GCN kernel entry points, the
sampler's refusals and the checkpoint layout."""
import ctypes

import numpy as np
import pytest
import torch

from moleculesde_amd import slabs

pytestmark = pytest.mark.gpu

from helpers import assert_close, batch_from, disable_dropout, fill_like_generator, load_golden, sub  # noqa: E402

M03 = "SDEModel3Dto2D_node_adj_dense_03"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _model(G, E, **kw):
    return G.SDEModel3Dto2D_node_adj_dense_03(dim3D=E, c_init=2, c_hid=8, c_final=4, num_heads=4, adim=16, nhid=16,
                                              num_layers=4, emb_dim=E, num_linears=3, beta_min=0.1, beta_max=1.0,
                                              num_diffusion_timesteps=1000, SDE_type="VE", num_class_X=119,
                                              noise_on_one_hot=True, **kw)


def _grads_close(model, ggrads, rtol, atol_scale, what):
    scale = max(float(v.abs().max()) for v in ggrads.values())
    for n, p in model.named_parameters():
        if n not in ggrads:         # the last edge layer's func_v feeds nothing (the reference leaves it without gradient)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, f"{what}: no grad for {n}"
        assert_close(p.grad, ggrads[n], rtol, atol_scale * scale, f"{what}:{n}")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "operator"])
def test_golden_f3_sde3d2d_03(dev, fused):
    """Both losses under replayed noise, the gradient of the 3D representation and every parameter gradient against the
    reference's _03 (dim3D = 12: layer-0 inputs 36 wide, later layers 28)."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.geom3d import dense_head, sde_3d_to_2d as S
    g = load_golden("f3_sde3d2d_03.npz")
    b = G.prepare_batch(batch_from(g), dev)
    E = g["h3"].shape[1]
    m = _model(G, E)
    assert [k for k, _ in m.named_parameters()] == list(g["param_names"])
    assert [list(p.shape) + [0] * (2 - p.dim()) for _, p in m.named_parameters()] == g["param_shapes"].tolist()
    fill_like_generator(m, 4200)
    m.to(dev).train()
    m.noise = G.CpuReplayNoise(int(g["seed"]))
    h3 = torch.from_numpy(g["h3"]).to(dev).requires_grad_(True)
    calls = dense_head.FUSED_CALLS
    S.USE_FUSED_HEAD = fused
    try:
        lx, la = m(h3, b, reduce_mean=True, continuous=True, train=True, anneal_power=0)
    finally:
        S.USE_FUSED_HEAD = True
    assert dense_head.FUSED_CALLS == calls + (1 if fused else 0), "wrong path ran"
    assert_close(lx, g["loss_x"], 1e-4, 1e-6, "loss_x")
    assert_close(la, g["loss_adj"], 1e-4, 1e-6, "loss_adj")
    (lx + la).backward()
    assert_close(h3.grad, g["grad_h3"], 1e-3, 1e-4 * float(np.abs(g["grad_h3"]).max()), "grad h3")
    _grads_close(m, sub(g, "grad."), 1e-3, 2e-4, "sde3d2d_03")


def _ragged_batch(G, dev, bs, seed):
    from moleculesde_amd.synthetic import make_batch
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 33, bs)
    sizes[0], sizes[-1] = 32, 1
    return G.prepare_batch(make_batch(bs, seed=seed, sizes=sizes.tolist()), dev)


@pytest.mark.parametrize("reduce_mean,anneal", [(True, 0.0), (False, 1.5), (True, 1.5), (False, 0.0)])
def test_fused_vs_operator_production_dims(dev, reduce_mean, anneal):
    """Emb 300, 64 molecules of 1 to 32 atoms: the fused head against the operator path of the same module (pinned to the
    reference by test_golden_f3_sde3d2d_03): both losses, the gradient of the 3D representation, every parameter gradient."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.geom3d import dense_head as DH, sde_3d_to_2d as S
    torch.manual_seed(12)
    emb = 300
    m = _model(G, emb).to(dev).train()
    b = _ragged_batch(G, dev, 64, 41)
    h3 = torch.randn(b.x.size(0), emb, device=dev)
    res = {}
    for fused in (False, True):
        S.USE_FUSED_HEAD = fused
        calls0 = DH.FUSED_CALLS
        try:
            m.noise = G.CpuReplayNoise(99)
            h = h3.clone().requires_grad_(True)
            for p in m.parameters():
                p.grad = None
            lx, la = m(h, b, reduce_mean=reduce_mean, continuous=True, train=True, anneal_power=anneal)
            assert DH.FUSED_CALLS == calls0 + (1 if fused else 0), "wrong path ran"
            (lx * 0.7 + la * 1.3).backward()
            res[fused] = (lx.detach(), la.detach(), h.grad.clone(), {n: (p.grad.clone() if p.grad is not None else None)
                                                                    for n, p in m.named_parameters()})
        finally:
            S.USE_FUSED_HEAD = True
    (lx0, la0, gh0, gp0), (lx1, la1, gh1, gp1) = res[False], res[True]
    assert_close(lx1, lx0, 2e-5, 0, "loss_x")
    assert_close(la1, la0, 2e-5, 0, "loss_adj")
    assert_close(gh1, gh0, 1e-3, 1e-5 * float(gh0.abs().max()), "grad h3")
    scale = max(float(v.abs().max()) for v in gp0.values() if v is not None)
    for n, v0 in gp0.items():
        v1 = gp1[n]
        if v0 is None or float(v0.abs().max()) == 0.0:
            assert v1 is None or float(v1.abs().max()) <= 1e-6 * scale, n      # unused output branch of the last layer
            continue
        assert v1 is not None, n
        assert_close(v1, v0, 2e-3, 2e-5 * scale, f"grad {n}")


def test_fused_03_launches_no_torch_operator(dev):
    """Every kernel of a fused _03 forward + backward under a Trainer (FlatAdam layout, device noise) is one of the library's."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import pretrain
    from moleculesde_amd.synthetic import make_batch
    from torch.profiler import profile, ProfilerActivity
    torch.manual_seed(3)
    tr = pretrain.Trainer(pretrain.readme_args(emb_dim=64, SDE_3Dto2D_model=M03), dev)
    m = tr.models["SDE_3Dto2D_model"]
    assert type(m).__name__ == M03
    m.noise = G.DeviceNoise(seed=11)
    b = G.prepare_batch(make_batch(64, seed=43), dev)
    h3 = torch.randn(b.x.size(0), 64, device=dev, requires_grad=True)

    def run():
        tr.opt.zero_grad()
        h3.grad = None
        lx, la = m(h3, b, reduce_mean=True, continuous=True, train=True, anneal_power=0)
        out = torch.stack([lx, la])
        slabs.begin_param_grad_batch(tr.opt.params)
        try:
            torch.autograd.backward(out, torch.ones_like(out))
        finally:
            slabs.finish_param_grad_batch()
    run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        run()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 30, names
    assert any("dense_node_gcn_fwd_kernel" in n for n in names), sorted(set(names))
    ours = ("dense_", "gemm_ex", "gemm_small", "gemm_rsa", "gemm_t2", "transpose_", "gemm_grouped_wgrad", "reduce_slabs", "colsum", "bn_")
    foreign = [n for n in names if not any(k in n for k in ours)]
    foreign = [n for n in foreign if "CatArrayBatchedCopy" not in n and "FillFunctor" not in n and "Memcpy" not in n
               and "Memset" not in n]
    assert not foreign, sorted(set(foreign))
    assert h3.grad is not None and float(h3.grad.abs().max()) > 0


def test_trainer_paths_agree(dev):
    """readme_args with _03: the eager step, the captured exact-size step and the capacity-bucket graph (device-built plan,
    row bounds) give the same loss terms and parameters from the same state."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import bucket as BK, hip, pretrain
    from moleculesde_amd.synthetic import make_batch
    args = pretrain.readme_args(emb_dim=64, SDE_3Dto2D_model=M03)
    torch.manual_seed(31)
    tr = pretrain.Trainer(args, dev)
    tr.overlap_streams = False
    for m in tr.models.values():
        disable_dropout(m)
    assert type(tr.models["SDE_3Dto2D_model"]).__name__ == M03

    class Noise(G.DeviceNoise):
        def __init__(self):
            super().__init__(seed=77)
            g = torch.Generator().manual_seed(5)
            self.big = torch.randn(8192, 3, generator=g).to(dev)
            self.ints = torch.randint(0, 1000, (4096,), generator=g).to(dev)

        def randn_like(self, x):
            assert x.dim() == 2 and x.size(1) == 3
            return self.big[:x.size(0)].clone()

        def randint(self, high, size, device):
            return self.ints[:size[0]].clone()
    noise, head_noise = Noise(), G.DeviceNoise(seed=99)
    tr.noise = noise
    tr.models["SDE_2Dto3D_model"].noise = noise
    tr.models["SDE_3Dto2D_model"].noise = head_noise
    snap = lambda: (tr.opt.flat_p.clone(), tr.opt.m.clone(), tr.opt.v.clone(), tr.opt.step_dev.clone(),
                    tr.step_counter.clone(), {k: {n: v.clone() for n, v in m.state_dict().items()} for k, m in tr.models.items()})

    def restore(s):
        tr.opt.flat_p.copy_(s[0]); tr.opt.m.copy_(s[1]); tr.opt.v.copy_(s[2]); tr.opt.step_dev.copy_(s[3])
        tr.step_counter.copy_(s[4])
        for k, m in tr.models.items():
            m.load_state_dict(s[5][k])

    def eager(batch, calls):
        noise.calls, head_noise.calls = calls[0] - 1, calls[1] - 1
        for k in tr.log:
            tr.log[k].zero_()
        tr.step(batch)
        torch.cuda.synchronize()
        return {k: float(v) for k, v in tr.log.items()}, tr.opt.flat_p.clone()

    def compare(got, ref, s0, what):
        for k in got[0]:
            assert abs(got[0][k] - ref[0][k]) <= 5e-5 * abs(ref[0][k]) + 1e-7, (what, k, got[0][k], ref[0][k])
        ua, ub = (got[1] - s0[0]).double(), (ref[1] - s0[0]).double()
        cos = float((ua * ub).sum() / (ua.norm() * ub.norm()))
        assert cos > 0.995, (what, cos)

    cpu = [make_batch(40, seed=s) for s in (51, 52)]
    # captured exact-size step
    exact = [G.prepare_batch(c.clone(), dev) for c in cpu]
    tr.step(exact[0])
    tr.capture(exact[0])
    calls = (noise.calls, head_noise.calls)
    for _ in range(2):
        s0 = snap()
        for k in tr.log:
            tr.log[k].zero_()
        tr.step_graph(exact[0])
        torch.cuda.synchronize()
        got = ({k: float(v) for k, v in tr.log.items()}, tr.opt.flat_p.clone())
        restore(s0)
        ref = eager(exact[0], calls)
        compare(got, ref, s0, "graph")
    # capacity-bucket graph on two different batches
    needs = [BK.raw_sizes(c) for c in cpu]
    caps = BK.Caps.covering(needs, n_max=24)
    bk = tr.make_bucket(caps)
    blobs = [BK.pack_raw(c, caps).to(dev) for c in cpu]
    tr.capture_bucket(bk, blobs[0])
    calls = (noise.calls, head_noise.calls)
    for i in (1, 0):
        s0 = snap()
        for k in tr.log:
            tr.log[k].zero_()
        tr.step_bucket(bk, blobs[i])
        torch.cuda.synchronize()
        got = ({k: float(v) for k, v in tr.log.items()}, tr.opt.flat_p.clone())
        restore(s0)
        hip.clear_row_bounds()
        ref = eager(G.prepare_batch(cpu[i].clone(), dev), calls)
        compare(got, ref, s0, f"bucket {i}")
    hip.clear_row_bounds()
    assert all(np.isfinite(v) for v in ref[0].values())


def _gcn_inputs(dev, sizes, F3, pad=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = torch.tensor(sizes)
    N, P = int(n.sum()), int((n * n).sum())
    mol_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)]).int().to(dev)
    pair_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), (n * n).cumsum(0)]).int().to(dev)
    AC = torch.zeros(P + pad, 32)
    q = 0
    for k in sizes:                 # symmetric bond-type adjacency, zero diagonal
        a = torch.randint(0, 4, (k, k), generator=g).float().triu(1)
        AC[q:q + k * k, 0] = (a + a.t()).reshape(-1)
        q += k * k
    FW = 16 + F3
    W = torch.randn(3 * FW * 16, generator=g) * 0.3
    d = dict(N=N, P=P, mol_ptr=mol_ptr, pair_ptr=pair_ptr, AC=AC.to(dev), FW=FW,
             XW0=(torch.randn(N + pad, 16, generator=g)).to(dev), W=W.to(dev), bl=(torch.randn(64, generator=g) * 0.2).to(dev),
             PE=torch.randn(N + pad, 48, generator=g).to(dev), gXS=torch.randn(N + pad, 64, generator=g).to(dev))
    d["PE"][N:] = float("nan")      # padding rows: never read
    d["XW0"][N:] = float("nan")
    return d


def _gcn_fwd(d, ex, dev, PE=None, wstride=256):
    from moleculesde_amd import _lib, hip
    XS = torch.full((d["N"] + 5, 70), -7.0, device=dev)
    B = d["mol_ptr"].numel() - 1
    p = hip._p
    if ex:
        _lib.call("msde_dense_node_gcn_fwd_ex", p(d["XW0"]), p(d["AC"]), p(d["mol_ptr"]), p(d["pair_ptr"]), p(d["W"]), wstride,
                  p(d["bl"]), p(PE), 48, B, 32, ctypes.c_void_p(XS.data_ptr() + 4 * 3), 70, hip._stream())
    else:
        _lib.call("msde_dense_node_gcn_fwd", p(d["XW0"]), p(d["AC"]), p(d["mol_ptr"]), p(d["pair_ptr"]), p(d["W"]), p(d["bl"]),
                  B, 32, ctypes.c_void_p(XS.data_ptr() + 4 * 3), 70, hip._stream())
    return XS


def _gcn_bwd(d, XS, ex, dev, wstride=256):
    from moleculesde_amd import _lib, hip
    p = hip._p
    B = d["mol_ptr"].numel() - 1
    GP = torch.full((d["N"] + 5, 64), -7.0, device=dev)
    MM = torch.full((d["N"] + 5, 64), -7.0, device=dev)
    xs = ctypes.c_void_p(XS.data_ptr() + 4 * 3)
    if ex:
        _lib.call("msde_dense_node_gcn_bwd_ex", p(d["gXS"]), 64, xs, 70, p(d["AC"]), p(d["mol_ptr"]), p(d["pair_ptr"]), p(d["W"]),
                  wstride, B, 32, p(GP), p(MM), hip._stream())
    else:
        _lib.call("msde_dense_node_gcn_bwd", p(d["gXS"]), 64, xs, 70, p(d["AC"]), p(d["mol_ptr"]), p(d["pair_ptr"]), p(d["W"]),
                  B, 32, p(GP), p(MM), hip._stream())
    return GP, MM


def test_node_gcn_ex_without_conditioning_is_bitwise_the_old_entry(dev):
    """msde_dense_node_gcn_{fwd,bwd}_ex with no conditioning term and the dense stride 256 launch exactly what the old entry
    points launch: bitwise equal outputs, padding rows untouched."""
    d = _gcn_inputs(dev, [32, 1, 7, 20, 2, 13], 0, seed=1)
    d["W"] = d["W"][:768].contiguous()
    a, b = _gcn_fwd(d, False, dev), _gcn_fwd(d, True, dev)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert bool((a[d["N"]:] == -7.0).all()) and bool((a[:, :3] == -7.0).all()) and bool((a[:, 67:] == -7.0).all())
    ga, ma = _gcn_bwd(d, a, False, dev)
    gb, mb = _gcn_bwd(d, a, True, dev)
    torch.cuda.synchronize()
    assert torch.equal(ga, gb) and torch.equal(ma, mb)
    assert bool((ga[d["N"]:] == -7.0).all()) and bool((ma[d["N"]:] == -7.0).all())


def test_node_gcn_ex_conditioned_vs_fp64(dev):
    """The conditioned chain x_{l+1} = tanh(An (x_l W_l,x + PE_l) + b_l) with W_l,x the first 16 rows of [16 + F3][16]
    weights, against fp64 on the host; the backward's MM = An^T GP and GP against fp64 too.  Padding rows (NaN inputs) are
    neither read nor written."""
    F3 = 12
    sizes = [32, 1, 7, 20, 2, 13]
    d = _gcn_inputs(dev, sizes, F3, seed=2)
    XS = _gcn_fwd(d, True, dev, PE=d["PE"], wstride=d["FW"] * 16)
    GP, MM = _gcn_bwd(d, XS, True, dev, wstride=d["FW"] * 16)
    torch.cuda.synchronize()
    N = d["N"]
    assert bool((XS[N:] == -7.0).all()) and bool((GP[N:] == -7.0).all()) and bool((MM[N:] == -7.0).all())
    W = d["W"].double().cpu().view(3, d["FW"], 16)[:, :16]
    bl, PE, AC = d["bl"].double().cpu().view(4, 16), d["PE"].double().cpu(), d["AC"].double().cpu()
    XW0, gXS = d["XW0"].double().cpu(), d["gXS"].double().cpu()
    ref_xs, ref_gp, ref_mm = torch.zeros(N, 64, dtype=torch.float64), torch.zeros(N, 64, dtype=torch.float64), \
        torch.zeros(N, 64, dtype=torch.float64)
    a0 = q0 = 0
    for n in sizes:
        A = AC[q0:q0 + n * n, 0].view(n, n).clone()
        A.fill_diagonal_(1.0)
        r = A.sum(-1).clamp(min=1).pow(-0.5)
        An = r[:, None] * A * r[None, :]
        xw, ys = XW0[a0:a0 + n], []
        for l in range(4):
            y = torch.tanh(An @ xw + bl[l])
            ys.append(y)
            if l < 3:
                xw = y @ W[l] + PE[a0:a0 + n, 16 * l:16 * l + 16]
        ref_xs[a0:a0 + n] = torch.cat(ys, -1)
        gx = torch.zeros(n, 16, dtype=torch.float64)
        for l in range(3, -1, -1):
            gp = (gx + gXS[a0:a0 + n, 16 * l:16 * l + 16]) * (1 - ys[l] ** 2)
            mm = An.t() @ gp
            ref_gp[a0:a0 + n, 16 * l:16 * l + 16], ref_mm[a0:a0 + n, 16 * l:16 * l + 16] = gp, mm
            if l > 0:
                gx = mm @ W[l - 1].t()
        a0 += n
        q0 += n * n
    assert_close(XS[:N, 3:67], ref_xs, 1e-5, 1e-5, "XS")
    assert_close(GP[:N], ref_gp, 1e-4, 1e-5, "GP")
    assert_close(MM[:N], ref_mm, 1e-4, 1e-5, "MM")


def test_sampler_refuses_03(dev):
    """The script's sampler has no conditioning argument: node_adj_PC_generation, generate_2d_from_3d and the forward-only
    ScoreEval refuse _03 by name instead of running the base model's arithmetic on it."""
    import types
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import sampler_3d2d as SM
    from moleculesde_amd.geom3d import dense_head as DH
    from moleculesde_amd.synthetic import make_batch
    m = _model(G, 16).to(dev).eval()
    b = G.prepare_batch(make_batch(3, seed=4), dev)
    rep = torch.randn(b.x.size(0), 16, device=dev)
    with pytest.raises(NotImplementedError, match="_03"):
        SM.node_adj_PC_generation(rep, b, m, max_iters=1)
    sch = G.SchNet(hidden_channels=16, num_filters=16, num_interactions=1, num_gaussians=51, cutoff=10, readout="mean",
                   node_class=119).to(dev)
    mol = make_batch(1, seed=5)
    with pytest.raises(NotImplementedError, match="_03"):
        SM.generate_2d_from_3d(sch, m, mol, num_repeat=2)
    cfg = types.SimpleNamespace(N=b.x.size(0), P=1, B=3)
    with pytest.raises(NotImplementedError, match="_03"):
        DH.ScoreEval(m, cfg, rep, torch.ones(b.x.size(0), device=dev))


def test_checkpoint_round_trip(dev, tmp_path):
    """Trainer.save and a strict reload of SDE_3Dto2D_model: the fixture's key layout, the same tensors."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import pretrain
    from moleculesde_amd.geom3d import sde_3d_to_2d as S
    g = load_golden("f3_sde3d2d_03.npz")
    args = pretrain.readme_args(emb_dim=12, SDE_3Dto2D_model=M03)
    torch.manual_seed(5)
    tr = pretrain.Trainer(args, dev)
    path = tmp_path / "ck.pth"
    tr.save(str(path))
    ck = torch.load(str(path), map_location="cpu")
    sd = ck["SDE_3Dto2D_model"]
    assert list(sd.keys()) == list(g["param_names"])
    assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == g["param_shapes"].tolist()
    m = S.build_from_args(args)
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert type(m).__name__ == M03
