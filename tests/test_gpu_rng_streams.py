"""Every kernel that draws its own randomness against the host mirror of the counter generator (tests/rng_mirror.py): WHICH
draw lands on WHICH element.  Normal draws are compared with the float64 mirror within `randn_tol` (8 x the float32-vs-float64
difference of the mirror itself, about 1.2e-5; a wrong index or seed is an O(1) difference), integer time steps, permutations
and dropout masks exactly.  A handful of launches on tens of rows each; nothing here is statistical."""
import ctypes
import math

import numpy as np
import pytest
import torch

import rng_mirror as RM
from helpers import assert_close, record_parity

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SNR, SCALE_EPS = 0.16, 0.7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def draws():
    """check(got, mirror float64, what): a device tensor of normal draws against the mirror within randn_tol; the largest
    error seen goes into the parity record next to the tolerance."""
    tol, spread = RM.measure_randn_tol()
    worst = {"err": 0.0, "n": 0}

    def check(got, ref, what):
        got = torch.as_tensor(got).detach().double().cpu().numpy()
        ref = np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        err = float(np.abs(got - ref).max()) if got.size else 0.0
        worst["err"], worst["n"] = max(worst["err"], err), worst["n"] + got.size
        print(f"{what}: {got.size} draws, max |device - mirror| {err:.3e} (randn_tol {tol:.3e})")
        assert err <= tol, f"{what}: max |device - mirror| {err:.3e} > randn_tol {tol:.3e}"

    check.tol = tol
    yield check
    record_parity(f"rng streams: device normal draws vs float64 mirror, {worst['n']} draws: max err {worst['err']:.3e}; "
                  f"randn_tol {tol:.3e} (= 8 x float32-vs-float64 mirror {spread:.3e})")


def _ctr(value, dev):
    return None if value is None else torch.tensor([value], dtype=torch.int64, device=dev)


def _i64(u):
    """A 64-bit pattern as the int64 torch holds."""
    u = int(u) & M64
    return u - (1 << 64) if u >> 63 else u


def _call(name, *args):
    from moleculesde_amd import _lib, hip
    _lib.call(name, *[hip._p(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args], hip._stream())


# ------------------------------------------------------------------------------------------------ msde_ve_perturb_rng
@pytest.mark.parametrize("seed", [1234, M64])
@pytest.mark.parametrize("ctr", [None, 0, 3])
def test_ve_perturb_rng_draws(dev, draws, seed, ctr):
    """Molecules of 1, 2, 9, 3, 4 atoms (B = 5, H = 3): noise_out is draw 3 i + c of seed', the integer time step recovered
    from std_out is the mirror's (and antithetic), pos_out = pos + std * noise.  Seed 2^64 - 1: the wrap-around."""
    from moleculesde_amd import hip
    sizes, T, eps, smin, smax = [1, 2, 9, 3, 4], 1000, 1e-5, 0.1, 1.0
    B, N, H = len(sizes), sum(sizes), len(sizes) // 2 + 1
    g = torch.Generator().manual_seed(1)
    pos = torch.randn(N, 3, generator=g).to(dev)
    mol = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    noise, out, std = hip.ve_perturb_rng(pos, mol.to(dev, torch.int32), B, T, eps, smin, smax, seed, _ctr(ctr, dev))
    st = RM.ve_perturb_streams(seed, ctr, sizes)
    draws(noise, st["noise"].randn(), f"ve_perturb_rng noise seed {seed} ctr {ctr}")
    ts = torch.round(((torch.log(std.double().cpu() / smin) / math.log(smax / smin)) - eps) / (1 - eps) * T).long()
    want = torch.from_numpy(RM.time_steps(seed, ctr, B, T))
    assert torch.equal(ts, want[mol]), (ts.tolist(), want.tolist())
    assert all(int(want[b]) + int(want[b + H]) == T - 1 for b in range(B - H))
    t = want[mol].double() / T * (1 - eps) + eps
    assert_close(std, smin * (smax / smin) ** t, 2e-6, 0, "std at the mirror's time step")
    assert_close(out, pos.double() + std.double()[:, None] * noise.double(), 1e-6, 1e-6, "pos + std * noise")


# ------------------------------------------------------------------------------------------------ msde_dense_prepare
def _chain_bonds(sizes, bondless):
    """CSR by target atom of chain molecules (bond i - (i + 1), both directions) without the bonds of the atoms in `bondless`
    (global indices): rowptr [N + 1], src [E], bond type [E]."""
    rows, a0 = [], 0
    for n in sizes:
        for i in range(n):
            nb = [j for j in (i - 1, i + 1) if 0 <= j < n and a0 + i not in bondless and a0 + j not in bondless]
            rows.append([a0 + j for j in nb])
        a0 += n
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    src = np.array([s for r in rows for s in r], dtype=np.int32)
    return rowptr, src, (np.arange(len(src)) % 3).astype(np.float32)


@pytest.mark.parametrize("sde_vp", [0, 1])
@pytest.mark.parametrize("ctr", [None, 2])
def test_dense_prepare_device_draws(dev, draws, sde_vp, ctr):
    """draws, noise_adj and noise_x all NULL; molecules of 2, 5, 32, 7 atoms, atom 3 of the last without bonds, 119 classes.
    z_adj: lower triangle bitwise equal to the upper, the upper the masked mirror draw of (lo, hi); z_x: the masked mirror
    draws; mean_std: the SDE's marginal at the mirror's time step.  Tolerance of mean_std: t, the exponent and powf / expf carry
    a few float32 roundings -> 2e-6 relative; the VP std = sqrt(1 - exp(2 lmc)) subtracts from 1: its square is off by up to
    8 x 2^-24 (expf within 2 ulp below 1, the rounded exponent, the subtraction), i.e. the std by 8 x 2^-24 / (2 std)."""
    sizes, ncls, T, eps, seed = [2, 5, 32, 7], 119, 1000, 1e-5, 0xC0FFEE123456789
    B, N = len(sizes), sum(sizes)
    lone = 2 + 5 + 32 + 3
    p0, p1 = (0.1, 1.0)
    rowptr, src, val = _chain_bonds(sizes, {lone})
    a0 = np.concatenate([[0], np.cumsum(sizes)])
    q0 = np.concatenate([[0], np.cumsum(np.square(sizes))])
    P = int(q0[-1])
    z_atom = (np.arange(N) * 7 % ncls).astype(np.int32)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    AC, z_adj, flags, mean_std, px, z_x = nan(P, 32), nan(P), nan(N), nan(B, 2), nan(N, 120), nan(N, 120)
    _call("msde_dense_prepare", t_(rowptr), t_(src), t_(val), t_(z_atom), t_(a0.astype(np.int32)), t_(q0.astype(np.int32)), None,
          None, B, T, eps, sde_vp, p0, p1, None, None, 32, seed, _ctr(ctr, dev), ncls, max(sizes), AC, z_adj, flags, mean_std, px,
          z_x)
    fl = np.ones(N)
    fl[lone] = 0.0
    assert flags.cpu().tolist() == fl.tolist()
    st = RM.dense_prepare_streams(seed, ctr, sizes, ncls)
    za = z_adj.cpu()
    for b, n in enumerate(sizes):
        m = za[q0[b]:q0[b + 1]].view(n, n)
        assert torch.equal(m, m.t()) and not m.diagonal().any(), f"molecule {b}: z_adj symmetric, zero diagonal"
    draws(z_adj, RM.sym_from_pairs(st["pair"].randn(), sizes, fl), f"dense_prepare z_adj vp {sde_vp} ctr {ctr}")
    draws(z_x[:, :ncls], st["cls"].randn() * fl[:, None], f"dense_prepare z_x vp {sde_vp} ctr {ctr}")
    assert not z_x[:, ncls:].any() and not z_adj.view(-1)[[int(q0[3] + 3 * 7 + 4)]].any() and not z_x[lone].any()
    ts = RM.time_steps(seed, ctr, B, T)
    H = B // 2 + 1
    assert all(int(ts[b]) + int(ts[b + H]) == T - 1 for b in range(B - H))
    t = ts.astype(np.float64) / T * (1 - eps) + eps
    if sde_vp:
        lmc = -0.25 * t * t * (p1 - p0) - 0.5 * t * p0
        mean, sd = np.exp(lmc), np.sqrt(1.0 - np.exp(2.0 * lmc))
        atol = 8 * 2.0 ** -24 / (2 * sd)
    else:
        mean, sd = np.ones(B), p0 * (p1 / p0) ** t
        atol = np.zeros(B)
    ms = mean_std.double().cpu().numpy()
    print("mean_std errors", np.abs(ms[:, 0] - mean).max(), np.abs(ms[:, 1] - sd).max(), "time steps", ts.tolist())
    assert (np.abs(ms[:, 0] - mean) <= 2e-6 * mean).all(), (ms[:, 0], mean)
    assert (np.abs(ms[:, 1] - sd) <= 2e-6 * sd + atol).all(), (ms[:, 1], sd)


# ------------------------------------------------------------------------------------------------ msde_pc_* (2D->3D sampler)
def _pc_inputs(n, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    par = torch.stack([0.5 + torch.rand(6, generator=g), 0.1 + torch.rand(6, generator=g), 0.9 + 0.1 * torch.rand(6, generator=g),
                       1.0 + 0.05 * torch.rand(6, generator=g)], 1).float()
    d = dict(out_c=torch.randn(n, 3, generator=g), out_p=torch.randn(n, 3, generator=g), pos=torch.randn(n, 3, generator=g), par=par)
    return d, {k: v.to(dev).contiguous() for k, v in d.items()}


def _pc_check(d, sl, par_row, z_c, z_p, xc, xm_c, x, xm, what):
    """The fp64 formulas of test_grouped_kernels_match_fp64_and_count_iterations on the atoms `sl`, fed with mirror draws."""
    std, Gt, alpha, fa = (float(v) for v in par_row.double())
    score = -d["out_c"][sl].double() / std
    z = torch.from_numpy(z_c).view(-1, 3)
    pos = d["pos"][sl].double()
    stp = (SNR * z.norm(dim=1).mean() / score.norm(dim=1).mean()) ** 2 * 2 * alpha
    ref_m = pos + stp * score
    assert_close(xm_c[sl], ref_m, 1e-4, 1e-5, what + " corrector x_mean")
    assert_close(xc[sl], ref_m + torch.sqrt(2 * stp) * SCALE_EPS * z, 1e-4, 1e-5, what + " corrector x")
    p = xc[sl].double().cpu()
    score2 = -d["out_p"][sl].double() / std
    ref_m2 = p - ((fa - 1.0) * p - Gt * Gt * score2)
    assert_close(xm[sl], ref_m2, 1e-4, 1e-5, what + " predictor x_mean")
    assert_close(x[sl], ref_m2 + Gt * torch.from_numpy(z_p).view(-1, 3), 1e-4, 1e-5, what + " predictor x")


@pytest.mark.parametrize("n", [7, 40])
@pytest.mark.parametrize("seed", [1234, 2 ** 63 + 12345])
def test_pc_single_kernels_draw_the_mirror_noise(dev, n, seed):
    """msde_pc_corrector / msde_pc_predictor with noise = NULL, rows 0..4 through the device counter: x and x_mean against the
    fp64 formulas with z = mirror draw (seed, row, stream, element) -- these break when pc_draw and the mirror are changed apart."""
    d, t = _pc_inputs(n, dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    for row in range(5):
        xc, xm_c, x, xm = (torch.full((n, 3), float("nan"), device=dev) for _ in range(4))
        _call("msde_pc_corrector", t["out_c"], t["pos"], None, t["par"], step, seed, n, SNR, SCALE_EPS, xc, xm_c)
        _call("msde_pc_predictor", t["out_p"], xc, None, t["par"], step, seed, n, x, xm)
        assert int(step) == row + 1
        _pc_check(d, slice(0, n), d["par"][row], RM.pc_draw_stream(seed, row, 0, 3 * n).randn(),
                  RM.pc_draw_stream(seed, row, 1, 3 * n).randn(), xc, xm_c, x, xm, f"n {n} row {row}")


def test_pc_grouped_kernels_draw_the_mirror_noise(dev):
    """The grouped pair on groups of 7, 1 and 40 atoms with seeds from sampler.group_seed: group g draws (group_seed[g], row,
    stream, element counted from the group's first coordinate)."""
    from moleculesde_amd.sampler import group_seed
    sizes = [7, 1, 40]
    n, G = sum(sizes), len(sizes)
    ptr = [0] + list(np.cumsum(sizes))
    seeds = [group_seed(1234, g) for g in range(G)]
    d, t = _pc_inputs(n, dev, seed=6)
    seeds_dev = torch.tensor([_i64(s) for s in seeds], dtype=torch.int64, device=dev)
    ptr_dev = torch.tensor(ptr, dtype=torch.int32, device=dev)
    step = torch.zeros(G, dtype=torch.int64, device=dev)
    bad = torch.zeros(G, dtype=torch.int32, device=dev)
    for row in range(5):
        xc, xm_c, x, xm = (torch.full((n, 3), float("nan"), device=dev) for _ in range(4))
        _call("msde_pc_corrector_grouped", t["out_c"], t["pos"], None, t["par"], step, seeds_dev, ptr_dev, G, n, max(sizes), SNR,
              SCALE_EPS, xc, xm_c)
        _call("msde_pc_predictor_grouped", t["out_p"], xc, None, t["par"], step, seeds_dev, ptr_dev, G, n, x, xm, bad)
        assert step.tolist() == [row + 1] * G and bad.tolist() == [0] * G
        for g, ng in enumerate(sizes):
            _pc_check(d, slice(ptr[g], ptr[g + 1]), d["par"][row], RM.pc_draw_stream(seeds[g], row, 0, 3 * ng).randn(),
                      RM.pc_draw_stream(seeds[g], row, 1, 3 * ng).randn(), xc, xm_c, x, xm, f"group {g} row {row}")


# ------------------------------------------------------------------------------------------------ msde_dense_pc_* (3D->2D sampler)
def test_dense_pc_counter_noise(dev, draws):
    """csrc/dense_pc.hip with the counter generator, set up through sampler_3d2d.FusedPC; molecules of 2, 5, 32 atoms, atom 2 of
    the second flagged off, n_steps = 1.  Init: x and adj are the masked mirror draws of row -1.  Corrector (row 0, draw 0):
    (x - x_mean) / z_mirror is ONE constant over all classes and one over all pairs within 1e-4 relative (|z| < 0.1 left out:
    under 10 % of N(0,1) draws, at most 15 % asserted).  Predictor (row 0, draw n_steps): x - x_mean = G z_mirror within
    G randn_tol + 4 ulp of |x|."""
    from moleculesde_amd import sampler_3d2d as S
    from moleculesde_amd.geom3d import dense_head as DH
    from moleculesde_amd.geom3d import prepare_batch
    from moleculesde_amd.geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense
    from moleculesde_amd.synthetic import make_batch
    torch.manual_seed(3)
    sizes, F, seed, n_steps = [2, 5, 32], 8, 0xFEEDFACE12345, 1
    m = SDEModel3Dto2D_node_adj_dense(dim3D=F, nhid=16, num_layers=4, num_linears=3, c_hid=8, c_final=4, adim=16, emb_dim=F,
                                      beta_min=0.1, beta_max=1.0, num_diffusion_timesteps=1000, c_init=2, num_heads=4,
                                      SDE_type="VE").to(dev).eval()
    b = prepare_batch(make_batch(len(sizes), seed=5, sizes=sizes), dev)
    B, Nm, ncls = len(sizes), max(sizes), m.num_class_X
    flags = torch.zeros(B, Nm, device=dev)
    for k, n in enumerate(sizes):
        flags[k, :n] = 1.0
    flags[1, 2] = 0.0
    rep = torch.randn(sum(sizes), F, device=dev)
    _, _, _, _, mol_ptr, _, batch, local, flags_, h3 = S._layout(b, rep, None, None, flags)
    pair_ptr = DH.ragged_layout(mol_ptr)
    cfg = DH.types.SimpleNamespace(N=h3.size(0), P=int(pair_ptr[-1]), B=B, n_max=Nm, mol_ptr=mol_ptr.contiguous(),
                                   pair_ptr=pair_ptr.contiguous())
    _, par = S.step_table(m.sde_adj, 1000, 1e-4)
    fl = flags_[batch, local].contiguous()
    pc = S.FusedPC(m, h3, cfg, fl, Nm, par, n_steps, 0.2, 0.9, seed, None)
    fl = fl.double().cpu().numpy()
    pb, lo, hi = RM.pair_index(sizes)
    a0 = np.concatenate([[0], np.cumsum(sizes)])
    q0 = np.concatenate([[0], np.cumsum(np.square(sizes))])
    up = torch.from_numpy(q0[pb] + lo * np.asarray(sizes)[pb] + hi)              # ragged position of every pair lo < hi
    pmask = fl[a0[pb] + lo] * fl[a0[pb] + hi]
    eps32 = 2.0 ** -23

    def state():
        torch.cuda.synchronize()
        return tuple(v.detach().double().cpu() for v in (pc.x[:, :ncls], pc.x_mean[:, :ncls], pc.adj, pc.adj_mean))

    def symmetric(adj):
        for k, n in enumerate(sizes):
            a = adj[q0[k]:q0[k + 1]].view(n, n)
            assert torch.equal(a, a.t())

    # ---- initial sample
    st = RM.dense_pc_streams(seed, -1, 0, sizes, ncls)
    x, xm, adj, am = state()
    draws(x, st["cls"].randn() * fl[:, None], "dense_pc_init x")
    draws(adj, RM.sym_from_pairs(st["pair"].randn(), sizes, fl), "dense_pc_init adj")
    symmetric(adj)
    assert torch.equal(x, xm) and torch.equal(adj, am) and not pc.x[:, ncls:].any()

    # ---- corrector, row 0, inner step 0
    s = ctypes.byref(pc.params)
    G2, OUT = pc.ev(pc.x)
    S._lib.call("msde_dense_pc_corrector", s, S._p(G2), G2.size(1), S._p(pc.ev.w2), S._p(pc.ev.b2), S._p(OUT), S._hip._stream())
    st = RM.dense_pc_streams(seed, 0, 0, sizes, ncls)
    x, xm, adj, am = state()
    symmetric(adj)
    for what, diff, z, live in (("classes", (x - xm).numpy(), st["cls"].randn(), np.broadcast_to(fl[:, None], (len(fl), ncls)) > 0),
                                ("pairs", (adj - am)[up].numpy(), st["pair"].randn(), pmask > 0)):
        assert not diff[~live].any(), f"corrector {what}: no noise outside the flags"
        use = live & (np.abs(z) >= 0.1)
        left_out = 1.0 - use.sum() / live.sum()
        ratio = diff[use] / z[use]
        c = float(np.median(ratio))
        spread = float(np.abs(ratio / c - 1.0).max())
        print(f"dense_pc corrector {what}: (x - x_mean) / z_mirror = {c:.6e}, relative spread {spread:.3e}, left out {left_out:.3f}")
        assert left_out <= 0.15
        assert c > 0 and spread <= 1e-4, f"corrector {what}: (x - x_mean) / z_mirror is not one constant ({spread:.3e})"

    # ---- predictor, row 0, draw n_steps
    G2, OUT = pc.ev(pc.x)
    S._lib.call("msde_dense_pc_predictor", s, S._p(G2), G2.size(1), S._p(pc.ev.w2), S._p(pc.ev.b2), S._p(OUT), S._hip._stream())
    st = RM.dense_pc_streams(seed, 0, n_steps, sizes, ncls)
    x, xm, adj, am = state()
    symmetric(adj)
    assert pc.step.tolist() == [1, 1]
    Gt = float(par[0, 1])
    for what, diff, ref, mag in (("classes", x - xm, Gt * st["cls"].randn() * fl[:, None], x.abs()),
                                 ("pairs", (adj - am)[up], Gt * st["pair"].randn() * pmask, adj[up].abs())):
        err = (diff - torch.from_numpy(ref)).abs()
        tol = Gt * draws.tol + 4 * eps32 * mag
        print(f"dense_pc predictor {what}: G = {Gt:.4e}, max |(x - x_mean) - G z_mirror| {float(err.max()):.3e}, "
              f"max err / tol {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), f"predictor {what}: {float((err / tol).max()):.3f} x the tolerance"


# ------------------------------------------------------------------------------------------------ msde_randperm
@pytest.mark.parametrize("n", [1, 2, 37, 300])
@pytest.mark.parametrize("ctr", [None, 2])
def test_randperm_equals_the_mirror_ranks(dev, n, ctr):
    from moleculesde_amd import hip
    seed = 77
    out = hip.randperm(n, dev, seed, _ctr(ctr, dev), count=2).cpu().long()
    for w in range(2):
        assert out[w].tolist() == RM.randperm(seed, ctr, w, n).tolist(), (n, ctr, w)


def test_randperm_below_a_device_row_bound(dev):
    """Capacity 37, 29 valid rows on the device: a permutation of the first 29 (the mirror's for n = 29), the rest map to
    themselves."""
    cap, n, seed = 37, 29, 2 ** 64 - 3
    out = torch.full((2, cap), -1, dtype=torch.int32, device=dev)
    _call("msde_randperm", cap, 2, seed, _ctr(1, dev), out, torch.tensor([n], dtype=torch.int32, device=dev))
    for w in range(2):
        assert out[w].cpu().tolist() == RM.randperm(seed, 1, w, n, ncap=cap).tolist()


# ------------------------------------------------------------------------------------------------ dropout masks
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("ctr", [None, 5])
def test_silu_dropout_keeps_the_mirror_set(dev, p, ctr):
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(9)
    x = torch.randn(37, 32, generator=g) * 2
    w = torch.randn(37, 32, generator=g)
    keep = torch.from_numpy(RM.silu_dropout_stream(1234, ctr, x.numel()).keep(p)).view(37, 32)
    xd = x.to(dev).requires_grad_(True)
    y = hip.silu_dropout(xd, p, 1234, _ctr(ctr, dev))
    (y * w.to(dev)).sum().backward()
    assert torch.equal((y != 0).cpu(), keep), "forward: kept set"
    assert torch.equal((xd.grad != 0).cpu(), keep), "backward: kept set"
    xr = x.double().requires_grad_(True)
    ref = torch.nn.functional.silu(xr) * keep / (1 - p)
    (ref * w.double()).sum().backward()
    assert_close(y, ref.detach(), 1e-5, 1e-6, "kept values")
    assert_close(xd.grad, xr.grad, 1e-5, 1e-6, "kept gradients")


@pytest.mark.parametrize("silu_out", [False, True])
def test_gat_tail_dropout_is_the_mirror_mask(dev, silu_out):
    """hip.gat_tail on 33 rows, p = 0.1: the fp64 operator chain with the mirror mask (uniform of row * 32 + column) on the
    feed-forward's SiLU matches the output and all ten gradients at test_gat_tail_kernel's tolerances."""
    from moleculesde_amd import hip
    from moleculesde_amd.geom3d import nn as _nn
    torch.manual_seed(31)
    N, D, p, seed, ctr = 33, 32, 0.1, 1234, 5
    n1, n2 = torch.nn.LayerNorm(D), torch.nn.LayerNorm(D)
    f0, f3 = torch.nn.Linear(D, D), torch.nn.Linear(D, D)
    with torch.no_grad():
        for m in (n1, n2):
            m.weight.normal_(1, 0.3); m.bias.normal_(0, 0.3)
    n1, n2, f0, f3 = (m.double() for m in (n1, n2, f0, f3))          # float32 values, double arithmetic
    x = torch.randn(N, D).double().requires_grad_(True)
    res = torch.randn(N, D).double().requires_grad_(True)
    w = torch.randn(N, D).double()
    keep = torch.from_numpy(RM.gat_tail_stream(seed, ctr, N).keep(p))
    y1 = res + n1(x)
    out = y1 + n2(f3(torch.nn.functional.silu(f0(y1)) * keep / (1 - p)))
    out = torch.nn.functional.silu(out) if silu_out else out
    (out * w).sum().backward()
    ref_grads = [x.grad, res.grad] + [q.grad for q in (n1.weight, n1.bias, f0.weight, f0.bias, f3.weight, f3.bias, n2.weight, n2.bias)]
    m1, m2 = torch.nn.LayerNorm(D).to(dev), torch.nn.LayerNorm(D).to(dev)
    g0, g3 = _nn.Linear(D, D).to(dev), _nn.Linear(D, D).to(dev)
    with torch.no_grad():
        for a, b in ((m1, n1), (m2, n2), (g0, f0), (g3, f3)):
            a.weight.copy_(b.weight); a.bias.copy_(b.bias)
    xd, rd = x.detach().float().to(dev).requires_grad_(True), res.detach().float().to(dev).requires_grad_(True)
    od = hip.gat_tail(xd, rd, m1, g0, g3, m2, p, seed, _ctr(ctr, dev), silu_out)
    assert_close(od, out.detach(), 1e-4, 1e-5, "gat tail fwd with the mirror mask")
    (od * w.float().to(dev)).sum().backward()
    got = [xd.grad, rd.grad, m1.weight.grad, m1.bias.grad, g0.weight.grad, g0.bias.grad, g3.weight.grad, g3.bias.grad,
           m2.weight.grad, m2.bias.grad]
    for a, b, nme in zip(got, ref_grads, ["g_x", "g_res", "ln1_g", "ln1_b", "W0", "b0", "W3", "b3", "ln2_g", "ln2_b"]):
        assert_close(a, b, 2e-4, 2e-5 * float(b.abs().max()) + 1e-6, f"gat tail grad {nme}")
