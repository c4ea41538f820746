"""Many molecules per reverse-SDE trajectory (moleculesde_amd/sampler.py: position_PC_generation_grouped,
generate_samples_from_testset; csrc/pointwise.hip: msde_pc_corrector_grouped / msde_pc_predictor_grouped) on the GPU: the
kernels against fp64 and against the single-molecule kernels, group isolation, trajectories against single-molecule
trajectories, graph replay, and the test-set driver under different chunkings."""
import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 300, 600]      # one atom, the wave boundary, more atoms than the 256-thread block, the block-size switch (512)
SNR, SCALE_EPS = 0.16, 0.7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _call(name, *args):
    from moleculesde_amd import _lib, hip
    _lib.call(name, *[hip._p(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args], hip._stream())


@pytest.fixture(scope="module")
def kin(dev):
    """Inputs of the kernel tests, drawn once: raw network outputs, coordinates, 5 x 2 noise tensors, a 6-row table whose rows
    differ, the group table."""
    g = torch.Generator().manual_seed(5)
    n = sum(SIZES)
    r = lambda *s: torch.randn(*s, generator=g)
    par = torch.stack([0.5 + torch.rand(6, generator=g), 0.1 + torch.rand(6, generator=g), 0.9 + 0.1 * torch.rand(6, generator=g),
                       1.0 + 0.05 * torch.rand(6, generator=g)], 1)
    d = dict(n=n, G=len(SIZES), ptr=[0] + list(np.cumsum(SIZES)), out_c=r(n, 3), out_p=r(n, 3), pos=r(n, 3), nz_c=r(5, n, 3),
             nz_p=r(5, n, 3), par=par.float())
    d["dev"] = {k: v.to(dev).contiguous() for k, v in d.items() if isinstance(v, torch.Tensor)}
    d["dev"]["ptr"] = torch.tensor(d["ptr"], dtype=torch.int32, device=dev)
    return d


def _pair(kin, dev, k, step, out_c=None, out_p=None, seeds=None, bad=None):
    """One corrector + predictor pair on the grouped kernels (explicit noise k, or in-kernel noise when `seeds` is given):
    (xc, xm_c, x, x_mean), every output buffer NaN beforehand."""
    t = kin["dev"]
    n, G = kin["n"], kin["G"]
    xc, xm_c, x, xm = (torch.full((n, 3), float("nan"), device=dev) for _ in range(4))
    out_c = t["out_c"] if out_c is None else out_c
    out_p = t["out_p"] if out_p is None else out_p
    bad = torch.zeros(G, dtype=torch.int32, device=dev) if bad is None else bad
    _call("msde_pc_corrector_grouped", out_c, t["pos"], None if seeds is not None else t["nz_c"][k], t["par"], step, seeds, t["ptr"],
          G, n, max(SIZES), SNR, SCALE_EPS, xc, xm_c)
    _call("msde_pc_predictor_grouped", out_p, xc, None if seeds is not None else t["nz_p"][k], t["par"], step, seeds, t["ptr"], G, n,
          x, xm, bad)
    return xc, xm_c, x, xm, bad


def test_grouped_kernels_match_fp64_and_count_iterations(dev, kin):
    """5 consecutive corrector / predictor pairs with explicit noise against the fp64 formulas per group (rtol 1e-4, atol 1e-5);
    every group's counter advances by exactly 1 per corrector call and the predictor uses its corrector's table row."""
    step = torch.zeros(kin["G"], dtype=torch.int64, device=dev)
    par = kin["par"].double()
    ptr = kin["ptr"]
    for k in range(5):
        xc, xm_c, x, xm, bad = _pair(kin, dev, k, step)
        assert step.tolist() == [k + 1] * kin["G"]
        assert bad.tolist() == [0] * kin["G"]
        std, Gt, alpha, fa = (float(v) for v in par[k])
        for g in range(kin["G"]):
            s = slice(ptr[g], ptr[g + 1])
            score = -kin["out_c"][s].double() / std
            z = kin["nz_c"][k][s].double()
            pos = kin["pos"][s].double()
            stp = (SNR * z.norm(dim=1).mean() / score.norm(dim=1).mean()) ** 2 * 2 * alpha
            ref_m = pos + stp * score
            ref_x = ref_m + torch.sqrt(2 * stp) * SCALE_EPS * z
            assert_close(xm_c[s], ref_m, 1e-4, 1e-5, "corrector x_mean, group %d pair %d" % (g, k))
            assert_close(xc[s], ref_x, 1e-4, 1e-5, "corrector x, group %d pair %d" % (g, k))
            p = xc[s].double().cpu()                    # the predictor's input is the corrector's fp32 output
            score2 = -kin["out_p"][s].double() / std
            ref_m2 = p - ((fa - 1.0) * p - Gt * Gt * score2)
            assert_close(xm[s], ref_m2, 1e-4, 1e-5, "predictor x_mean, group %d pair %d" % (g, k))
            assert_close(x[s], ref_m2 + Gt * kin["nz_p"][k][s].double(), 1e-4, 1e-5, "predictor x, group %d pair %d" % (g, k))
    from moleculesde_amd import _lib
    with pytest.raises(_lib.MsdeHipError):
        _call("msde_pc_corrector_grouped", kin["dev"]["out_c"], kin["dev"]["pos"], kin["dev"]["nz_c"][0], kin["dev"]["par"], step, None,
              kin["dev"]["ptr"], 0, kin["n"], 600, SNR, SCALE_EPS, xc, xm_c)
    with pytest.raises(_lib.MsdeHipError):
        _call("msde_pc_predictor_grouped", kin["dev"]["out_p"], xc, kin["dev"]["nz_p"][0], kin["dev"]["par"], step, None, None,
              kin["G"], kin["n"], x, xm, bad)


def test_grouped_kernels_equal_the_single_molecule_kernels_bit_for_bit(dev, kin):
    """In-kernel noise, row 3 of the table: group g of the grouped pair == msde_pc_corrector / msde_pc_predictor on the group's
    slice with seed = group_seed[g] and the same row (same reduction order, same draws), torch.equal."""
    t = kin["dev"]
    seeds = [7, 2 ** 63 + 12345, 3, 2 ** 64 - 1, 99, 1 << 40, 123456789]
    seeds_dev = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64, device=dev)
    step = torch.full((kin["G"],), 3, dtype=torch.int64, device=dev)
    xc, xm_c, x, xm, _ = _pair(kin, dev, 0, step, seeds=seeds_dev)
    assert torch.isfinite(x).all() and torch.isfinite(xc).all()
    ptr = kin["ptr"]
    for g, ng in enumerate(SIZES):
        s = slice(ptr[g], ptr[g + 1])
        one = torch.full((1,), 3, dtype=torch.int64, device=dev)
        a, am, b, bm = (torch.full((ng, 3), float("nan"), device=dev) for _ in range(4))
        _call("msde_pc_corrector", t["out_c"][s].contiguous(), t["pos"][s].contiguous(), None, t["par"], one, seeds[g], ng, SNR,
              SCALE_EPS, a, am)
        _call("msde_pc_predictor", t["out_p"][s].contiguous(), a, None, t["par"], one, seeds[g], ng, b, bm)
        assert int(one) == 4
        for got, ref, what in ((xc[s], a, "corrector x"), (xm_c[s], am, "corrector x_mean"), (x[s], b, "predictor x"),
                               (xm[s], bm, "predictor x_mean")):
            assert torch.equal(got, ref), (what, ng, float((got - ref).abs().max()))


def test_a_diverged_group_is_flagged_and_disturbs_no_other(dev, kin):
    t = kin["dev"]
    ptr, bad_g = kin["ptr"], 3
    clean = _pair(kin, dev, 1, torch.full((kin["G"],), 2, dtype=torch.int64, device=dev))
    oc, op = t["out_c"].clone(), t["out_p"].clone()
    oc[ptr[bad_g]:ptr[bad_g + 1]] = float("inf")
    op[ptr[bad_g]:ptr[bad_g + 1]] = float("inf")
    hurt = _pair(kin, dev, 1, torch.full((kin["G"],), 2, dtype=torch.int64, device=dev), out_c=oc, out_p=op)
    assert clean[4].tolist() == [0] * kin["G"]
    assert hurt[4].tolist() == [int(g == bad_g) for g in range(kin["G"])]
    # sticky: a clean pair on the same flag buffer leaves it set
    again = _pair(kin, dev, 1, torch.full((kin["G"],), 2, dtype=torch.int64, device=dev), bad=hurt[4])
    assert again[4].tolist() == [int(g == bad_g) for g in range(kin["G"])]
    keep = torch.ones(kin["n"], dtype=torch.bool, device=dev)
    keep[ptr[bad_g]:ptr[bad_g + 1]] = False
    for a, b in zip(clean[:4], hurt[:4]):
        assert torch.equal(a[keep], b[keep])
        assert not torch.isfinite(b[~keep]).any()


# ---- trajectories ------------------------------------------------------------------------------------------------------------------
def _models(sde_type, dev):
    import moleculesde_amd.geom3d as G
    torch.manual_seed(0)
    gnn = G.GNN(3, 32, gnn_type="GIN").to(dev).eval()
    bmin, bmax = (0.2, 1.0) if sde_type == "VE" else (0.2, 30.0)
    s23 = G.SDEModel2Dto3D_02(emb_dim=32, hidden_dim=32, beta_min=bmin, beta_max=bmax, num_diffusion_timesteps=1000,
                              beta_schedule=None, SDE_type=sde_type, use_extend_graph=True).to(dev).eval()
    return gnn, s23


def _prepared(mols, repeat, gnn, dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import sampler
    b = G.prepare_batch(sampler.repeat_data(mols, repeat), dev)
    with torch.no_grad():
        rep = gnn(b.x, b.edge_index, b.edge_attr)
    return b, rep


@pytest.fixture(scope="module")
def three(dev):
    """Molecules of 2, 13 and 20 atoms, 3 replicas each: the grouped batch and the three single-molecule batches (VE models)."""
    from moleculesde_amd.synthetic import make_molecule
    rng = np.random.default_rng(2)
    mols = [make_molecule(rng, n) for n in (2, 13, 20)]
    ptr = [0] + list(np.cumsum([3 * m.num_nodes for m in mols]))
    pos0 = torch.randn(ptr[-1], 3, generator=torch.Generator().manual_seed(9)).to(dev)
    return mols, ptr, pos0


@pytest.mark.parametrize("sde_type", ["VE", "VP"])
def test_grouped_trajectory_matches_single_molecule_trajectories(dev, three, monkeypatch, sde_type):
    """10 steps, torch_noise=True with the noise tensors injected through torch.randn_like (the grouped call gets the whole
    tensors, each single-molecule call the molecule's slices), use_graph=False: every molecule of the grouped run ==
    position_PC_generation on that molecule alone, rtol 1e-4 / atol 1e-5."""
    from moleculesde_amd import sampler
    mols, ptr, pos0 = three
    gnn, s23 = _models(sde_type, dev)
    noise = torch.randn(20, ptr[-1], 3, generator=torch.Generator().manual_seed(4)).to(dev)

    def inject(rows):
        it = iter(noise)
        monkeypatch.setattr(torch, "randn_like", lambda like: next(it)[rows].contiguous())

    b, rep = _prepared(mols, 3, gnn, dev)
    inject(slice(0, ptr[-1]))
    got, bad = sampler.position_PC_generation_grouped(s23, rep, b, ptr, num_steps=10, pos_init=pos0, use_graph=False, denoise=False,
                                                      torch_noise=True)
    assert bad.tolist() == [0, 0, 0] and torch.isfinite(got).all()
    for g, m in enumerate(mols):
        s = slice(ptr[g], ptr[g + 1])
        b1, rep1 = _prepared([m], 3, gnn, dev)
        inject(s)
        ref = sampler.position_PC_generation(s23, rep1, b1, num_steps=10, pos_init=pos0[s], use_graph=False, denoise=False,
                                             torch_noise=True)
        assert_close(got[s], ref, 1e-4, 1e-5, "grouped vs alone, %s, molecule of %d atoms" % (sde_type, m.num_nodes))


def test_grouped_production_mode(dev, three):
    """In-kernel noise, 12 steps, group_seeds given: against per-molecule position_PC_generation(noise_seed=group_seeds[g]);
    replayed against host-launched (1e-5 / 1e-6); iters_per_graph 4 against 1 and two identical calls bit for bit."""
    from moleculesde_amd import sampler
    mols, ptr, pos0 = three
    gnn, s23 = _models("VE", dev)
    seeds = [11, 2 ** 63 + 5, 77]
    b, rep = _prepared(mols, 3, gnn, dev)
    kw = dict(num_steps=12, pos_init=pos0, denoise=False, group_seeds=seeds)
    e1, bad = sampler.position_PC_generation_grouped(s23, rep, b, ptr, use_graph=False, **kw)
    e2, _ = sampler.position_PC_generation_grouped(s23, rep, b, ptr, use_graph=False, **kw)
    g1, bad_g = sampler.position_PC_generation_grouped(s23, rep, b, ptr, use_graph=True, **kw)
    g4, _ = sampler.position_PC_generation_grouped(s23, rep, b, ptr, use_graph=True, iters_per_graph=4, **kw)
    assert bad.tolist() == [0, 0, 0] and bad_g.tolist() == [0, 0, 0] and bad.dtype == torch.int32
    assert torch.isfinite(e1).all() and torch.equal(e1, e2)
    assert torch.equal(g4, g1)
    assert_close(g1, e1, 1e-5, 1e-6, "replayed vs host-launched grouped trajectory")
    o1, _ = sampler.position_PC_generation_grouped(s23, rep, b, ptr, use_graph=False, **dict(kw, group_seeds=[11, 2 ** 63 + 5, 78]))
    assert torch.equal(o1[:ptr[2]], e1[:ptr[2]]) and not torch.allclose(o1[ptr[2]:], e1[ptr[2]:])
    for g, m in enumerate(mols):
        s = slice(ptr[g], ptr[g + 1])
        b1, rep1 = _prepared([m], 3, gnn, dev)
        ref = sampler.position_PC_generation(s23, rep1, b1, num_steps=12, pos_init=pos0[s], denoise=False, use_graph=False,
                                             noise_seed=seeds[g])
        assert_close(e1[s], ref, 1e-4, 1e-5, "grouped vs position_PC_generation(noise_seed), molecule of %d atoms" % m.num_nodes)


def test_driver_does_not_depend_on_the_chunking(dev):
    """5 molecules, 3 conformers each, 12 steps: 2 molecules per launch (a short last chunk) against 5 and against 1; a chunk
    holding a 12- and a 33-atom molecule (the score network's operator path for that chunk) against the two sampled alone."""
    from moleculesde_amd import sampler
    from moleculesde_amd.synthetic import make_molecule
    gnn, s23 = _models("VE", dev)
    rng = np.random.default_rng(8)
    mols = [make_molecule(rng, n) for n in (5, 13, 2, 20, 9)]
    kw = dict(num_repeat=3, start=0, end=5, num_steps=12, noise_seed=3)
    r2 = sampler.generate_samples_from_testset(mols, gnn, s23, molecules_per_launch=2, **kw)
    r5 = sampler.generate_samples_from_testset(mols, gnn, s23, molecules_per_launch=5, **kw)
    r1 = sampler.generate_samples_from_testset(mols, gnn, s23, molecules_per_launch=1, **kw)
    assert len(r2) == len(r5) == len(r1) == 5
    for m, a, b, c in zip(mols, r2, r5, r1):
        assert a.finite and b.finite and c.finite
        assert a.pos_gen.shape == (3 * m.num_nodes, 3) and a.pos_gen.device.type == "cpu" and a.num_pos_gen.tolist() == [3]
        assert torch.equal(a.x, m.x)
        assert_close(a.pos_gen, b.pos_gen, 1e-4, 1e-5, "2 per launch vs 5 per launch, %d atoms" % m.num_nodes)
        assert_close(a.pos_gen, c.pos_gen, 1e-4, 1e-5, "2 per launch vs 1 per launch, %d atoms" % m.num_nodes)
    assert not torch.allclose(r2[0].pos_gen[:5], r2[0].pos_gen[5:10])          # the replicas are different conformers
    big = [make_molecule(rng, 12), make_molecule(rng, 33)]
    together = sampler.generate_samples_from_testset(big, gnn, s23, molecules_per_launch=2, **dict(kw, end=2))
    alone = sampler.generate_samples_from_testset(big, gnn, s23, molecules_per_launch=1, **dict(kw, end=2))
    for m, a, b in zip(big, together, alone):
        assert a.finite and b.finite
        assert_close(a.pos_gen, b.pos_gen, 1e-4, 1e-5, "12 + 33 atoms in one launch vs alone, %d atoms" % m.num_nodes)
