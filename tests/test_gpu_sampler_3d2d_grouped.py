"""Several molecules per 3D->2D reverse-SDE trajectory (sampler_3d2d.node_adj_PC_generation_grouped, csrc/dense_pc_grouped.hip)
against the single-trajectory path it stands beside: the kernels bit for bit against csrc/dense_pc.hip on each group alone, the
float64 formulas, the pinned draws, a non-finite group, whole trajectories, the production head, the test-set driver and the
refusals.  Every comparison asserts first that its reference side is finite."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import rng_mirror as RM
from helpers import record_parity

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
RTOL, ATOL = 1e-4, 1e-5             # fused kernels vs float64, the figure of tests/test_gpu_sampler_testset.py
RANDN_TOL = 1.2e-5                  # device normal draw vs float64 mirror, the figure of tests/test_gpu_rng_streams.py
SNR, SCALE_EPS = 0.2, 0.9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _model(sde_type, F, dev):
    from moleculesde_amd.geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense
    lo = 0.1 if sde_type == "VE" else 0.2
    m = SDEModel3Dto2D_node_adj_dense(dim3D=F, nhid=16, num_layers=4, num_linears=3, c_hid=8, c_final=4, adim=16, emb_dim=F,
                                      beta_min=lo, beta_max=1.0, num_diffusion_timesteps=1000, c_init=2, num_heads=4,
                                      SDE_type=sde_type)
    return m.to(dev).eval()


def _molecules(sizes, seed=6):
    from moleculesde_amd.synthetic import make_molecule
    rng = np.random.default_rng(seed)
    return [make_molecule(rng, int(n)) for n in sizes]


def _replicas(mols, reps, dev):
    """The group-major batch: reps[k] replicas of molecule k; returns (batch, group_ptr over molecules, sizes per molecule)."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.batch import Batch
    lst = [m for m, r in zip(mols, reps) for _ in range(r)]
    gp = [0] + list(np.cumsum(reps))
    return G.prepare_batch(Batch.from_data_list(lst), dev), [int(v) for v in gp], [m.num_nodes for m in lst]


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t).all()), "the reference side is not finite"


def _same(got, ref, what):
    """Bit-for-bit equality with a finite reference."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    _finite(ref)
    assert torch.equal(got, ref), (what, float((got.double() - ref.double()).abs().max()))


def _close(got, ref, what):
    """|got - ref| <= ATOL + RTOL |ref| with a finite reference; returns the largest absolute difference."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    _finite(ref)
    err = (got - ref).abs()
    assert bool((err <= ATOL + RTOL * ref.abs()).all()), (what, float(err.max()), float(ref.abs().max()))
    return float(err.max())


# ------------------------------------------------------------------------------------------------ kernel-level set-up
SIZES, REPS = (2, 5, 13, 32), (1, 3, 2, 2)          # a single-replica group, a 2-atom molecule (one pair), the 32-atom limit
SEEDS = [0xFEEDFACE12345, 7, M64, 0x123456789ABCDEF]


class _Kernels:
    """The batch of SIZES x REPS (the last atom of every replica of the 13-atom molecule bond-less: flag 0) with a grouped state and,
    on separate buffers, a single-trajectory state whose entry points are driven group by group on pointer slices."""

    def __init__(self, dev, sde_type, n_steps, noises=None):
        from moleculesde_amd import _lib, sampler_3d2d as S
        from moleculesde_amd.geom3d import dense_head as DH
        self.S, self.lib, self.dev = S, _lib, dev
        torch.manual_seed(3)
        mols = _molecules(SIZES)
        m13 = mols[2]
        keep = (m13.edge_index[0] != 12) & (m13.edge_index[1] != 12)
        m13.edge_index, m13.edge_attr = m13.edge_index[:, keep], m13.edge_attr[keep]
        self.m = _model(sde_type, 16, dev)
        b, self.gp, self.sizes = _replicas(mols, REPS, dev)
        self.G, self.n_steps, self.ncls = len(REPS), n_steps, self.m.num_class_X
        rep = torch.randn(sum(self.sizes), 16, device=dev)
        _, _, self.B, self.Nm, mol_ptr, _, self.batch, self.local, self.flags, h3 = S._layout(b, rep, None, None, None)
        assert float(self.flags.sum()) == sum(self.sizes) - REPS[2]
        pair_ptr = DH.ragged_layout(mol_ptr)
        self.cfg = DH.types.SimpleNamespace(N=h3.size(0), P=int(pair_ptr[-1]), B=self.B, n_max=self.Nm, mol_ptr=mol_ptr.contiguous(),
                                            pair_ptr=pair_ptr.contiguous())
        _, self.par = S.step_table(self.m.sde_adj, 1000, 1e-4)
        fl = self.flags[self.batch, self.local].contiguous()
        self.h3, self.fl = h3, fl
        self.grouped = S.GroupedPC(self.m, h3, self.cfg, fl, self.Nm, self.par, n_steps, SNR, SCALE_EPS, self.gp, SEEDS, noises)
        self.F2 = self.grouped.ev.G2.size(1)

    def single(self):
        S = self.S
        pc = S.FusedPC(self.m, self.h3, self.cfg, self.fl, self.Nm, self.par, self.n_steps, SNR, SCALE_EPS, 1)
        pc.slices = []
        for g in range(self.G):
            s = self.lib.DensePcParams.from_buffer_copy(pc.params)
            s.mol_ptr, s.pair_ptr = pc.params.mol_ptr + 4 * self.gp[g], pc.params.pair_ptr + 4 * self.gp[g]
            s.B, s.seed = self.gp[g + 1] - self.gp[g], SEEDS[g]
            pc.slices.append(s)
        return pc

    def heads(self, k):
        g = torch.Generator(device=self.dev).manual_seed(100 + k)
        return (torch.randn(self.cfg.P, self.F2, device=self.dev, generator=g),
                torch.randn(self.cfg.N, self.grouped.ev.OUT.size(1), device=self.dev, generator=g))

    def call_grouped(self, name, G2, OUT):
        S, pc = self.S, self.grouped
        self.lib.call(name, ctypes.byref(pc.params), ctypes.byref(pc.groups), S._p(G2), G2.size(1), S._p(pc.ev.w2), S._p(pc.ev.b2),
                      S._p(OUT), S._hip._stream())

    def call_single(self, pc, name, G2, OUT):
        S = self.S
        for s in pc.slices:
            self.lib.call(name, ctypes.byref(s), S._p(G2), G2.size(1), S._p(pc.ev.w2), S._p(pc.ev.b2), S._p(OUT), S._hip._stream())

    def padded(self, pc):
        return self.S.to_padded(pc, self.batch, self.local, self.sizes, self.B, self.Nm, self.ncls)


@pytest.mark.parametrize("sde_type", ["VE", "VP"])
@pytest.mark.parametrize("n_steps", [1, 2])
def test_kernels_equal_single_kernels_bitwise(dev, sde_type, n_steps):
    """Init and three corrector / predictor pairs on given random G2 / OUT, counter noise: the grouped entry points on the whole
    batch equal msde_dense_pc_* on each group's slice alone with seed = group_seed[g], bit for bit (the same draws, the same
    sums in the same order), in x, adj, x_mean, adj_mean and the rewritten XC[:, :F] and AC[:, 0:2]."""
    k = _Kernels(dev, sde_type, n_steps)
    S, gpc = k.S, k.grouped
    spc = k.single()
    for s in spc.slices:
        k.lib.call("msde_dense_pc_init", ctypes.byref(s), None, S._hip._stream())

    def same(when):
        torch.cuda.synchronize()
        F = k.h3.size(1)
        for name, a, c in (("x", spc.x, gpc.x), ("adj", spc.adj, gpc.adj), ("x_mean", spc.x_mean, gpc.x_mean),
                           ("adj_mean", spc.adj_mean, gpc.adj_mean), ("XC", spc.ev.XC[:, :F], gpc.ev.XC[:, :F]),
                           ("AC", spc.ev.AC[:, 0:2], gpc.ev.AC[:, 0:2])):
            _finite(a)
            assert torch.equal(a, c), (when, name, float((a - c).abs().max()))
        assert a.abs().sum() > 0

    same("init")
    for it in range(3):
        G2, OUT = k.heads(2 * it)
        k.call_grouped("msde_dense_pc_corrector_grouped", G2, OUT)
        k.call_single(spc, "msde_dense_pc_corrector", G2, OUT)
        same(f"corrector {it}")
        G2, OUT = k.heads(2 * it + 1)
        k.call_grouped("msde_dense_pc_predictor_grouped", G2, OUT)
        k.call_single(spc, "msde_dense_pc_predictor", G2, OUT)
        same(f"predictor {it}")
    assert gpc.step.tolist() == [3, 3] and spc.step.tolist() == [3, 3]
    assert gpc.group_bad.tolist() == [0] * k.G


def _scores64(k, G2, OUT, std):
    """The padded float64 scores the kernels form from the heads: -(G2 . w2 + b2) on the pairs i < j, mirrored, and -OUT, both
    masked and divided by std."""
    ev = k.grouped.ev
    net = G2.double() @ ev.w2.double().reshape(-1) + ev.b2.double().reshape(-1)[0]
    pad = torch.zeros(k.B, k.Nm, k.Nm, dtype=torch.float64, device=k.dev)
    o = 0
    for b, n in enumerate(k.sizes):
        pad[b, :n, :n] = net[o:o + n * n].view(n, n)
        o += n * n
    fl = k.flags.double()
    up = pad.triu(1)
    s_adj = -(up + up.transpose(1, 2)) * fl[:, :, None] * fl[:, None, :] / std
    s_x = torch.zeros(k.B, k.Nm, k.ncls, dtype=torch.float64, device=k.dev)
    s_x[k.batch, k.local] = OUT.double()[:, :k.ncls]
    return -s_x * fl[:, :, None] / std, s_adj


@pytest.mark.parametrize("sde_type", ["VE", "VP"])
@pytest.mark.parametrize("n_steps", [1, 2])
def test_kernels_against_float64_formulas(dev, sde_type, n_steps):
    """The same batch with injected noise: every corrector call against corrector_steps_grouped and every predictor call
    against its formula, both in float64 on the state the kernel read, within rtol 1e-4 / atol 1e-5; and the corrector's
    result is NOT the batch-mean corrector's on the whole batch (a kernel that ignored group_ptr would be)."""
    from moleculesde_amd.geom3d.sde_3d_to_2d import mask_x
    torch.manual_seed(11)
    I, B, Nm = 3, sum(REPS), max(SIZES)
    ncls = 119
    r = lambda *s: torch.randn(*s, device=dev)
    noises = dict(x_init=r(B, Nm, ncls), adj_init=r(B, Nm, Nm), corr_adj=r(I, n_steps, B, Nm, Nm), corr_x=r(I, n_steps, B, Nm, ncls),
                  pred_adj=r(I, B, Nm, Nm), pred_x=r(I, B, Nm, ncls))
    k = _Kernels(dev, sde_type, n_steps, noises)
    assert k.ncls == ncls and k.Nm == Nm
    S = k.S
    gi = torch.repeat_interleave(torch.arange(k.G, device=dev), torch.tensor(REPS, device=dev))
    one = torch.zeros_like(gi)
    fl = k.flags.double()
    d = lambda t: t.double()
    state = [d(t) for t in k.padded(k.grouped)]
    _finite(*state)
    assert torch.equal(state[0], d(mask_x(noises["x_init"], k.flags))) and torch.equal(state[1], d(S.sym_noise(noises["adj_init"], k.flags)))
    worst = 0.0
    for it in range(I):
        std, Gt, alpha, fa = (float(v) for v in k.par[it].double())
        G2, OUT = k.heads(2 * it)
        k.call_grouped("msde_dense_pc_corrector_grouped", G2, OUT)
        s_x, s_adj = _scores64(k, G2, OUT, std)
        args = (state[0], state[1], s_x, s_adj, d(noises["corr_x"][it]), d(noises["corr_adj"][it]), fl, alpha)
        want = S.corrector_steps_grouped(*args, gi, k.G, SNR, SCALE_EPS)
        batch_mean = S.corrector_steps_grouped(*args, one, 1, SNR, SCALE_EPS)
        got = k.padded(k.grouped)
        for name, g_, w_, bm in zip(("x", "adj", "x_mean", "adj_mean"), got, want, batch_mean):
            worst = max(worst, _close(g_, w_, f"corrector {it} {name}"))
            _finite(bm)
            assert not torch.allclose(d(g_), bm, rtol=1e-2, atol=1e-3), f"corrector {it} {name}: the batch-mean result"
        state = [d(t) for t in got]
        G2, OUT = k.heads(2 * it + 1)
        k.call_grouped("msde_dense_pc_predictor_grouped", G2, OUT)
        s_x, s_adj = _scores64(k, G2, OUT, std)
        z_x = d(mask_x(noises["pred_x"][it], k.flags))
        z_adj = d(S.sym_noise(noises["pred_adj"][it], k.flags))
        xm = state[0] - ((fa * state[0] - state[0]) - Gt * Gt * s_x)
        am = state[1] - ((fa * state[1] - state[1]) - Gt * Gt * s_adj)
        got = k.padded(k.grouped)
        for name, g_, w_ in zip(("x", "adj", "x_mean", "adj_mean"), got, (xm + Gt * z_x, am + Gt * z_adj, xm, am)):
            worst = max(worst, _close(g_, w_, f"predictor {it} {name}"))
        state = [d(t) for t in got]
    assert k.grouped.group_bad.tolist() == [0] * k.G
    record_parity(f"sampler_3d2d grouped kernels vs float64 formulas ({sde_type}, n_steps {n_steps}): max abs err {worst:.3e} "
                  f"(rtol {RTOL:g} / atol {ATOL:g})")


def test_initial_draws_pinned(dev):
    """Counter noise: the initial x / adj of group g are the masked mirror draws of tests/rng_mirror.dense_pc_streams for
    (group_seed[g], row -1) and that group's sizes alone, within 1.2e-5."""
    k = _Kernels(dev, "VE", 1)
    torch.cuda.synchronize()
    x, adj = k.grouped.x[:, :k.ncls].double().cpu().numpy(), k.grouped.adj.double().cpu().numpy()
    fl = k.fl.double().cpu().numpy()
    a0 = np.concatenate([[0], np.cumsum(k.sizes)])
    q0 = np.concatenate([[0], np.cumsum(np.square(k.sizes))])
    worst = 0.0
    for g in range(k.G):
        lo, hi = k.gp[g], k.gp[g + 1]
        sizes = k.sizes[lo:hi]
        st = RM.dense_pc_streams(SEEDS[g], -1, 0, sizes, k.ncls)
        f = fl[a0[lo]:a0[hi]]
        want_x = st["cls"].randn() * f[:, None]
        want_adj = np.asarray(RM.sym_from_pairs(st["pair"].randn(), sizes, f), dtype=np.float64)
        assert np.isfinite(want_x).all() and np.isfinite(want_adj).all()
        ex = float(np.abs(x[a0[lo]:a0[hi]] - want_x).max())
        ea = float(np.abs(adj[q0[lo]:q0[hi]] - want_adj).max())
        print(f"group {g}: max |device - mirror| x {ex:.3e}, adj {ea:.3e}")
        worst = max(worst, ex, ea)
        assert ex <= RANDN_TOL and ea <= RANDN_TOL, (g, ex, ea)
    record_parity(f"sampler_3d2d grouped initial draws vs float64 mirror: max err {worst:.3e} (tol {RANDN_TOL:g})")


# ------------------------------------------------------------------------------------------------ trajectories
def _traj_setup(dev, sde_type, sizes=(5, 9, 14), R=3):
    torch.manual_seed(5)
    mols = _molecules(sizes, seed=8)
    m = _model(sde_type, 16, dev)
    b, gp, msizes = _replicas(mols, [R] * len(sizes), dev)
    rep = torch.randn(sum(msizes), 16, device=dev)
    return mols, m, b, gp, msizes, rep


def test_nonfinite_group_disturbs_no_other(dev):
    """A NaN in one group's x_init: after three iterations that group's group_bad is 1, the others' 0, and every other group's
    state equals the run without the NaN bit for bit."""
    from moleculesde_amd import sampler_3d2d as S
    mols, m, b, gp, msizes, rep = _traj_setup(dev, "VE")
    B, Nm, ncls = len(msizes), max(msizes), m.num_class_X
    x_init = torch.randn(B, Nm, ncls, device=dev)
    kw = dict(group_seeds=[11, 12, 13], max_iters=3, use_graph=False)
    clean = S.node_adj_PC_generation_grouped(rep, b, m, gp, x_init=x_init, **kw)
    poisoned = x_init.clone()
    poisoned[gp[1] + 1, 0, 3] = float("nan")
    bad = S.node_adj_PC_generation_grouped(rep, b, m, gp, x_init=poisoned, **kw)
    assert clean[4].tolist() == [0, 0, 0] and bad[4].tolist() == [0, 1, 0]
    for g in (0, 2):
        for name, c, p in zip(("x", "adj", "x_mean", "adj_mean"), clean, bad):
            _finite(c[gp[g]:gp[g + 1]])
            assert torch.equal(c[gp[g]:gp[g + 1]], p[gp[g]:gp[g + 1]]), (g, name)
    assert not bool(torch.isfinite(bad[2][gp[1]:gp[2]]).all())


@pytest.mark.parametrize("sde_type", ["VE", "VP"])
def test_trajectory_against_single_driver(dev, sde_type):
    """Three molecules (5, 9, 14 atoms) x 3 replicas, five iterations (two eager, three replayed), counter noise: the grouped
    driver against node_adj_PC_generation on each molecule alone with noise_seed = group_seeds[g].  The issue's bound was rtol
    1e-4 / atol 1e-5, to be tightened if the device showed no difference at all, since the score networks' launches hold other
    molecules in the two runs; the measured difference is exactly 0 for VE and VP
    (profiles/pr_sampler_3d2d_grouped_parity_numbers.txt), so this asserts bit-for-bit equality.  Replay equals use_graph=False
    bit for bit."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import sampler_3d2d as S
    from moleculesde_amd.batch import Batch
    mols, m, b, gp, msizes, rep = _traj_setup(dev, sde_type)
    seeds = [0xABCDEF0123, 99, M64 - 5]
    got = S.node_adj_PC_generation_grouped(rep, b, m, gp, group_seeds=seeds, max_iters=5)
    eager = S.node_adj_PC_generation_grouped(rep, b, m, gp, group_seeds=seeds, max_iters=5, use_graph=False)
    _finite(*eager[:4])
    for a, c in zip(got, eager):
        assert torch.equal(a, c)
    assert got[4].tolist() == [0, 0, 0]
    a0 = np.concatenate([[0], np.cumsum(msizes)])
    for g, mol in enumerate(mols):
        lo, hi = gp[g], gp[g + 1]
        bg = G.prepare_batch(Batch.from_data_list([mol] * (hi - lo)), dev)
        ref = S.node_adj_PC_generation(rep[a0[lo]:a0[hi]], bg, m, max_iters=5, noise_seed=seeds[g])
        n = mol.num_nodes
        for name, r_, g_ in zip(("x", "adj", "x_mean", "adj_mean"), ref, got):
            assert not g_[lo:hi, n:].any(), "padding rows are zero"
            g_ = g_[lo:hi, :n] if name.startswith("x") else g_[lo:hi, :n, :n]
            print(f"{sde_type} group {g} {name}: max |grouped - single| {float((g_ - r_).abs().max()):.3e}")
            _same(g_, r_, f"{sde_type} group {g} {name}")
    record_parity(f"sampler_3d2d grouped trajectory vs single driver per molecule ({sde_type}, 5 iterations): bitwise equal")


@pytest.mark.parametrize("sde_type", ["VE", "VP"])
def test_production_head_fused_vs_operator_path(dev, sde_type):
    """emb 300, production score networks, two groups (3 x 14 atoms, 2 x 20 atoms), n_steps 2, 10 iterations with injected
    noise: the grouped fused path against the grouped operator path within 1e-4 relative."""
    from moleculesde_amd import sampler_3d2d as S
    torch.manual_seed(3)
    m = _model(sde_type, 300, dev)
    mols = _molecules((14, 20), seed=11)
    b, gp, msizes = _replicas(mols, [3, 2], dev)
    B, Nm, I, n_steps, ncls = len(msizes), max(msizes), 10, 2, m.num_class_X
    rep = torch.randn(sum(msizes), 300, device=dev)
    r = lambda *s: torch.randn(*s, device=dev)
    noises = dict(x_init=r(B, Nm, ncls), adj_init=r(B, Nm, Nm), corr_adj=r(I, n_steps, B, Nm, Nm), corr_x=r(I, n_steps, B, Nm, ncls),
                  pred_adj=r(I, B, Nm, Nm), pred_x=r(I, B, Nm, ncls))
    fused = S.node_adj_PC_generation_grouped(rep, b, m, gp, n_steps=n_steps, max_iters=I, noises=noises, group_seeds=[1, 2])
    pl = S._layout(b, rep, None, None, None)
    flags, batch, local = pl[8], pl[6], pl[7]
    ops = S._generate_ops_grouped(m, rep, batch, local, flags, B, Nm, ncls, 1000, I, 1e-4, SNR, SCALE_EPS, n_steps, None, None,
                                  noises, gp)
    assert fused[4].tolist() == [0, 0] and ops[4].tolist() == [0, 0]
    for name, f, o in zip(("x", "adj", "x_mean", "adj_mean"), fused, ops):
        _finite(o)
        scale = float(o.abs().max())
        err = float((f - o).abs().max())
        print(f"{sde_type} {name}: max |fused - ops| {err:.3e}, scale {scale:.3e}")
        assert err <= 1e-4 * scale, (name, err, scale)


# ------------------------------------------------------------------------------------------------ the test-set driver
def test_driver_chunkings_agree(dev, tmp_path):
    """Five synthetic molecules of 6-20 atoms, 3 samples each, 4 iterations: the records of molecules_per_launch 2 and 5 against
    each other and against molecules_per_launch=1 (the per-molecule loop), bit for bit -- the tolerance of the trajectory test
    above, whose measured difference is 0; a start / end sub-range gives the same records for the same molecules; evaluate_graphs runs on the result; the pickle name is unchanged."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import graph2d_eval as ge
    torch.manual_seed(0)
    sch = G.SchNet(hidden_channels=64, num_filters=128, num_interactions=1, num_gaussians=51, cutoff=10, readout="mean",
                   node_class=119).to(dev)
    m = _model("VE", 64, dev)
    mols = _molecules((6, 20, 11, 9, 15), seed=4)
    kw = dict(num_repeat=3, noise_seed=7, num_steps=1000, max_iters=4)
    runs = {per: ge.generate_graphs_from_testset(mols, sch, m, start=0, end=5, molecules_per_launch=per, **kw) for per in (1, 2, 5)}
    for per in (2, 5):
        assert len(runs[per]) == 5
        for k, (ref, rec, mol) in enumerate(zip(runs[1], runs[per], mols)):
            assert rec.diverged is False and torch.equal(rec.edge_index, mol.edge_index)
            assert tuple(rec.x_gen.shape) == (3, mol.num_nodes, m.num_class_X)
            print(f"per {per} molecule {k}: max |grouped - loop| x {float((rec.x_gen - ref.x_gen).abs().max()):.3e}, "
                  f"adj {float((rec.adj_gen - ref.adj_gen).abs().max()):.3e}")
            _same(rec.x_gen, ref.x_gen, f"per {per} molecule {k} x")
            _same(rec.adj_gen, ref.adj_gen, f"per {per} molecule {k} adj")
    for k in range(5):
        _same(runs[2][k].x_gen, runs[5][k].x_gen, f"2 vs 5 molecule {k} x")
        _same(runs[2][k].adj_gen, runs[5][k].adj_gen, f"2 vs 5 molecule {k} adj")
    sub = ge.generate_graphs_from_testset(mols, sch, m, start=1, end=4, molecules_per_launch=2, out_path=str(tmp_path), **kw)
    assert len(sub) == 3
    for k, rec in zip((1, 2, 3), sub):
        _same(rec.x_gen, runs[5][k].x_gen, f"sub-range molecule {k} x")
        _same(rec.adj_gen, runs[5][k].adj_gen, f"sub-range molecule {k} adj")
    files = list(tmp_path.iterdir())
    assert [f.name for f in files] == ["3D_to_2D_1_4_repeat_3"]
    with open(files[0], "rb") as f:
        back = pickle.load(f)
    assert all(torch.equal(a.x_gen, c.x_gen) and a.diverged == c.diverged for a, c in zip(sub, back))
    res = ge.evaluate_graphs(runs[5])
    assert res["num_molecules"] == 5 and res["num_failed"] == 0
    record_parity("sampler_3d2d test-set driver, molecules_per_launch 2 / 5 vs 1 and a sub-range: bitwise equal")


def test_refusals(dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import _lib, graph2d_eval as ge, sampler_3d2d as S
    from moleculesde_amd.geom3d.sde_3d_to_2d import SDEModel3Dto2D_node_adj_dense_02, SDEModel3Dto2D_node_adj_dense_03
    torch.manual_seed(2)
    sch = G.SchNet(hidden_channels=64, num_filters=128, num_interactions=1, num_gaussians=51, cutoff=10, readout="mean",
                   node_class=119).to(dev)
    m = _model("VE", 64, dev)
    mols = _molecules((33, 5), seed=9)
    kw = dict(num_repeat=2, noise_seed=1, num_steps=1000, max_iters=1, start=0, end=2, molecules_per_launch=2)
    with pytest.raises(_lib.MsdeHipError):
        ge.generate_graphs_from_testset(mols, sch, m, **kw)
    m.allow_operator_path = True
    recs = ge.generate_graphs_from_testset(mols, sch, m, **kw)            # the grouped operator path runs it
    m.allow_operator_path = False
    assert len(recs) == 2 and tuple(recs[0].adj_gen.shape) == (2, 33, 33) and recs[0].diverged is False
    assert bool(torch.isfinite(recs[0].x_gen).all())

    m16 = _model("VE", 16, dev)
    b, gp, msizes = _replicas(_molecules((5, 7), seed=3), [2, 2], dev)
    rep = torch.randn(sum(msizes), 16, device=dev)
    for table in ([0, 2, 3], [1, 2, 4], [0, 2, 2, 4], [0, 3, 2, 4], [0]):
        with pytest.raises(ValueError):
            S.node_adj_PC_generation_grouped(rep, b, m16, table, max_iters=1)
    with pytest.raises(ValueError):
        S.node_adj_PC_generation_grouped(rep, b, m16, gp, group_seeds=[1, 2, 3], max_iters=1)
    with pytest.raises(NotImplementedError):
        S.node_adj_PC_generation_grouped(rep, b, m16, gp, probability_flow=True)
    common = dict(dim3D=16, nhid=16, num_layers=4, num_linears=3, c_hid=8, c_final=4, adim=16, emb_dim=16, beta_min=0.1, beta_max=1.0,
                  num_diffusion_timesteps=1000, c_init=2)
    for cls in (SDEModel3Dto2D_node_adj_dense_02, SDEModel3Dto2D_node_adj_dense_03):
        with pytest.raises(NotImplementedError):
            S.node_adj_PC_generation_grouped(rep, b, cls(**common).to(dev), gp)
