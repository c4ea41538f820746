"""The CFConv kernels (csrc/cfconv_pair.hip, csrc/cfconv_fused.hip, csrc/cfconv_fused_bwd.hip, the aggregate kernels of
csrc/schnet.hip) on molecules of 21 to 65 atoms against fp64.

Every other CFConv test builds its molecules with synthetic.make_batch (2..20 atoms): in-degrees of at most 19, so a 32-edge
chunk of the per-edge forward always holds several targets, the pair kernels never see more than 20 atoms, and the
32-neighbour cap never binds.  Here the batches are helpers.CFCONV_PAIR_SPECS (up to 33 atoms: in-degrees up to 32, chunks that
are ONE target -- whole, and continued from the chunk before --, targets that straddle two chunks, the pair form at its limit) and helpers.CFCONV_CAP_SPECS (up to 65 atoms: the
cap binds, the graph is asymmetric, by-source rows of up to 64 edges); tests/test_cfconv_sizes_host.py pins both on the host.
The graph is the oracle's edge list as a host-built CSR, so a CFConv defect cannot be taken for a graph defect (the radius
kernels have one test of their own here).  References, yardsticks and tolerances: tests/cfconv_cases.py -- 8 x the error of an
fp32 CPU evaluation against fp64, per molecule (atom rows) or per row (filter rows), never a constant fitted to a result.
Every achieved figure is recorded (helpers.record_parity) as error / tolerance per in-degree class."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restate as R  # noqa: E402
import cfconv_cases as CC  # noqa: E402
import helpers as H  # noqa: E402
from helpers import record_parity  # noqa: E402

U = 2.0 ** -24          # unit roundoff of fp32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _dev_params(c, dev, grad=True):
    return [p.clone().to(dev).requires_grad_(grad) for p in c.params]


def _weight_grads(tag, c, pd, failures):
    for name, p in zip(("gW1", "gb1", "gW2", "gb2"), pd):
        assert p.grad is not None, f"{tag}: no gradient for {name}"
        CC.compare_whole(tag, name, p.grad, c.ref[name], c.yard[name], failures)


# ------------------------------------------------------------------------------------------------ 1. pair form ---
def _pair_plan(c, dev, pad):
    """Batch plan + pair plan of the pair fixture; pad: capacity padding (extra atoms owned by molecule B, larger pair
    capacity) with the distances beyond `count` NaN-filled."""
    from moleculesde_amd import hip, plan as P
    g = c.g
    pl = P.plan_to(P.build_plan(g.batch, with_ext=False), dev)
    assert pl.N_max == 33 and pl.P2_cap == g.pairs
    pos_d = g.pos.to(dev)
    if pad:
        pl.batch_i32 = torch.cat([pl.batch_i32, torch.full((pad,), pl.B, dtype=torch.int32, device=dev)])
        pos_d = torch.cat([pos_d, torch.randn(pad, 3, generator=torch.Generator().manual_seed(pad)).to(dev)])
        pl.P2_cap = pl.P2_cap + 100
    pp = hip.pair_plan(pos_d, pl, c.cutoff)
    return pl, pp


@pytest.mark.parametrize("cutoff,G,pad", [(10.0, 51, 0), (10.0, 51, 37), (4.0, 51, 0), (4.0, 51, 37), (10.0, 50, 0), (10.0, 20, 0)])
def test_pair_form_vs_fp64(dev, cutoff, G, pad):
    """hip.pair_plan (pair index and distances against a host enumeration), hip.cfconv_pair_forward (filter rows per pair,
    exact zero rows beyond the cutoff; the aggregation per molecule) and hip.cfconv_pair's backward (g_x1, the four
    filter-network gradients) on molecules of up to 33 atoms.  pad: a capacity bucket's padding -- the padded atoms get
    exact zeros and nothing beyond `count` (NaN-filled distances and filter rows) reaches a result."""
    from moleculesde_amd import hip
    c = CC.case("pair", cutoff, G)
    g = c.g
    tag = f"pair form cutoff {cutoff:g} G {G} pad {pad}"
    failures = []
    pl, pp = _pair_plan(c, dev, pad)
    N, P2 = g.N, g.pairs

    # ---- the pair list
    pi, pj, edge = CC.pair_index(g)
    assert int(pp.count[0]) == P2 and pp.P == P2 + (100 if pad else 0)
    ptr = [0]
    for n in g.sizes:
        ptr.append(ptr[-1] + n * (n - 1) // 2)
    assert pp.pair_ptr.cpu().tolist() == ptr
    assert torch.equal(pp.pi[:P2].cpu().long(), pi) and torch.equal(pp.pj[:P2].cpu().long(), pj), "row-major a < b"
    assert bool((pi < pj).all())
    pdist = pp.pd[:P2].cpu().double()
    inside = edge >= 0
    assert bool((pdist[~inside] == -1.0).all()), "pairs beyond the cutoff carry distance -1 exactly"
    assert int((~inside).sum()) == (0 if cutoff == 10.0 else (2 * P2 - g.E) // 2)
    d64 = (g.pos.double()[pi] - g.pos.double()[pj]).norm(dim=-1)
    # sqrtf(dx dx + dy dy + dz dz): differences 1 u, squares 3 u, sum 5 u, root 2.5 u + 1 u
    derr = ((pdist - d64).abs() / d64)[inside]
    record_parity(f"cfconv_sizes {tag} pair distance: worst relative error {float(derr.max()) / U:.2f} u (bound 4 u)")
    assert float(derr.max()) <= 4 * U
    if pad:
        pp.pd[P2:] = float("nan")

    # ---- filter rows + aggregation
    x1_full, w_full = c.x1, c.w
    if pad:
        gen = torch.Generator().manual_seed(1000 + pad)
        x1_full = torch.cat([c.x1, torch.randn(pad, CC.F, generator=gen)])
        w_full = torch.cat([c.w, torch.randn(pad, CC.F, generator=gen)])
    x1d = x1_full.to(dev).requires_grad_(True)
    pd = _dev_params(c, dev)
    off = c.offset.to(dev)
    out2, Wf = hip.cfconv_pair_forward(x1d.detach(), pp, *[p.detach() for p in pd], off, c.coeff, cutoff)
    assert Wf.size(0) == pp.P
    ref_rows, low_rows, _ = CC.pair_rows(c)
    assert bool((Wf[:P2][~inside.to(dev)] == 0).all()), "exact zero filter rows beyond the cutoff"
    hw = torch.zeros(P2, dtype=torch.float64)
    hw[inside] = CC.cutoff_hardware_term(c)[edge[inside]]
    CC.compare_rows(tag, "filter rows", Wf[:P2], ref_rows, low_rows, g.deg[pi], failures, extra_tol=hw)
    Wf_own = None
    if pad:                     # the aggregation and the backward on a buffer the test owns: NaN beyond count
        Wf_own = Wf.clone()
        Wf_own[P2:] = float("nan")
    out = hip.cfconv_pair(x1d, *pd, pp, off, c.coeff, cutoff, Wf=Wf_own)
    assert torch.equal(out, out2), "bitwise reproducible (fixed order, no atomics)"
    groups = CC.mol_groups(g)
    CC.compare_rows(tag, "out", out[:N], c.ref["out"], c.low["out"], g.deg, failures, groups)

    # ---- backward
    (out * w_full.to(dev)).sum().backward()
    CC.compare_rows(tag, "g_x1", x1d.grad[:N], c.ref["g_x1"], c.low["g_x1"], g.deg, failures, groups)
    _weight_grads(tag, c, pd, failures)
    if pad:
        assert float(out[N:].abs().max()) == 0.0 and float(x1d.grad[N:].abs().max()) == 0.0, "padded atoms: exact zeros"
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cutoff", [10.0, 4.0])
def test_pair_filters_of_all_blocks_bitwise(dev, cutoff):
    """hip.cfconv_pair_filters for 3 blocks (msde_cfconv_pair_filter_multi) == the per-block launches, bit for bit, on a pair
    list of 2421 pairs (75 full 32-pair blocks + 21)."""
    from moleculesde_amd import hip
    c = CC.case("pair", cutoff, 51)
    pl, pp = _pair_plan(c, dev, 0)
    nets = [[p.to(dev) for p in c.params]]
    for k in (1, 2):
        blk = R.InteractionBlock(hidden_channels=64, num_gaussians=51, num_filters=CC.F, cutoff=cutoff)
        H.fill_like_generator(blk, 4000 + 10 * k)
        nets.append([p.detach().to(dev) for p in (blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[2].weight, blk.mlp[2].bias)])
    off = c.offset.to(dev)
    Wfs = hip.cfconv_pair_filters(pp, nets, off, c.coeff, cutoff)
    x = c.x1.to(dev)
    P2 = int(pp.count[0])
    for l in range(3):
        _, Wf1 = hip.cfconv_pair_forward(x, pp, *nets[l], off, c.coeff, cutoff)
        assert torch.equal(Wfs[l][:P2], Wf1[:P2]), f"filter rows of block {l}"
    assert not torch.equal(Wfs[0][:P2], Wfs[1][:P2])


# ------------------------------------------------------------------------------------- 2 / 3. per-edge (fused) form ---
def _edge_form(c, dev, cpw):
    """hip.cfconv_fused (+ backward) and hip.cfconv_fused_forward(want_filter=True) on the oracle's graph as a host-built CSR."""
    from moleculesde_amd import hip
    g = c.g
    pl = CC.device_plan(g, dev)
    pd = _dev_params(c, dev)
    x1d = c.x1.to(dev).requires_grad_(True)
    dist, off = g.dist.to(dev), c.offset.to(dev)
    old = hip.FUSED_CHUNKS_PER_WG
    hip.FUSED_CHUNKS_PER_WG = cpw
    try:
        out = hip.cfconv_fused(x1d, *pd, dist, pl, off, c.coeff, c.cutoff)
        out2, Wf = hip.cfconv_fused_forward(x1d.detach(), dist, pl, *[p.detach() for p in pd], off, c.coeff, c.cutoff,
                                            want_filter=True)
    finally:
        hip.FUSED_CHUNKS_PER_WG = old
    (out * c.w.to(dev)).sum().backward()
    return out, out2, Wf, x1d.grad, pd


@pytest.mark.parametrize("name,G,cpw", [("pair", 51, 1), ("pair", 51, 3), ("pair", 50, 3), ("pair", 20, 1),
                                        ("cap", 51, 1), ("cap", 51, 3), ("cap", 50, 1), ("cap", 20, 3)])
def test_edge_form_vs_fp64(dev, name, G, cpw):
    """The per-edge fused kernels at in-degree 32.  "pair": the symmetric graph with 32-edge chunks that are ONE degree-32
    target (first == last target of the chunk, nothing partial: a plain store), degree-32 targets that straddle two chunks,
    and a last, 10-edge chunk that is one degree-19 target begun in the chunk before (first == last target AND partial: the
    atomic combination) -- two launches are bitwise equal (the forward's two-addend claim).  "cap": the asymmetric graph of molecules of up to 65 atoms -- the input gradient gathers
    over by-source rows of up to 64 edges, 1280 edges have no reverse.  Output, filter rows, g_x1 and the weight gradients
    against fp64, the error per in-degree class (g_x1 also per out-degree class)."""
    c = CC.case(name, 10.0, G)
    g = c.g
    tag = f"edge form {name} G {G} chunks/wg {cpw}"
    failures = []
    out, out2, Wf, g_x1, pd = _edge_form(c, dev, cpw)
    assert torch.equal(out, out2), "two launches bitwise equal (at most two addends per target on top of zero)"
    assert Wf.size(0) == g.E
    groups = CC.mol_groups(g)
    CC.compare_rows(tag, "filter rows", Wf, c.ref["Wf"], c.low["Wf"], g.deg[g.dst], failures, extra_tol=CC.cutoff_hardware_term(c))
    CC.compare_rows(tag, "out", out, c.ref["out"], c.low["out"], g.deg, failures, groups)
    CC.compare_rows(tag, "g_x1", g_x1, c.ref["g_x1"], c.low["g_x1"], g.deg, failures, groups)
    CC.compare_rows(tag, "g_x1 (by out-degree)", g_x1, c.ref["g_x1"], c.low["g_x1"], g.out_deg, failures, groups,
                    classes=CC.OUT_DEG_CLASSES)
    _weight_grads(tag, c, pd, failures)
    assert not failures, "\n".join(failures)


def test_pair_and_edge_forms_agree(dev):
    """The two forms on the same symmetric graph (up to 33 atoms, cutoff 10): each within its own tolerance of fp64 (the
    tests above), their difference within the sum of the two tolerances."""
    from moleculesde_amd import hip
    c = CC.case("pair", 10.0, 51)
    g = c.g
    out_e, _, Wf_e, gx_e, pd_e = _edge_form(c, dev, 1)
    pl, pp = _pair_plan(c, dev, 0)
    pd_p = _dev_params(c, dev)
    x1d = c.x1.to(dev).requires_grad_(True)
    out_p = hip.cfconv_pair(x1d, *pd_p, pp, c.offset.to(dev), c.coeff, c.cutoff)
    (out_p * c.w.to(dev)).sum().backward()
    groups = CC.mol_groups(g)
    failures = []
    for name, a, b in (("out", out_p, out_e), ("g_x1", x1d.grad, gx_e)):
        tol = 2 * CC.rows_tolerance(c.ref[name], c.low[name], groups)
        ratio, err = CC.row_ratios(a, b.detach().double().cpu(), tol)
        per = CC.class_worst(ratio, g.deg)
        record_parity(f"cfconv_sizes pair vs edge form {name}: worst difference {float(err.max()):.2e}; difference / (sum of the two "
                      f"tolerances) by class: {CC._fmt(per)}")
        failures += [f"{name} {n}: {v:.3f}" for n, v in per if v is not None and not v <= 1.0]
    for name, a, b in zip(("gW1", "gb1", "gW2", "gb2"), pd_p, pd_e):
        d = float((a.grad - b.grad).abs().max())
        record_parity(f"cfconv_sizes pair vs edge form {name}: worst difference {d:.2e}, sum of the two tolerances "
                      f"{2 * CC.TOL_FACTOR * c.yard[name]:.2e}")
        if not d <= 2 * CC.TOL_FACTOR * c.yard[name]:
            failures.append(f"{name}: {d:.3e}")
    assert not failures, "\n".join(failures)


# --------------------------------------------------------------------------------------------- 4. decomposed form ---
@pytest.mark.parametrize("name", ["pair", "cap"])
def test_decomposed_form_vs_fp64(dev, name):
    """hip.rbf_cutoff + hip.cfconv_aggregate (forward, g_x1, g_Wf) with 37 spare edge slots: src = -1 and NaN filter rows in
    the tail.  Smearing rows and cutoff factors per edge, the aggregation per molecule, g_Wf per edge; tail rows of rbf, C
    and g_Wf are zero."""
    from moleculesde_amd import hip
    spare = 37
    a = CC.aggregate_case(name)
    g = a.g
    tag = f"decomposed form {name}"
    failures = []
    pl = CC.device_plan(g, dev, spare)
    E, N = g.E, g.N
    assert pl.E == E + spare and int(pl.rowptr[-1]) == E
    dist = torch.cat([g.dist, torch.zeros(spare)]).to(dev)
    rbf, C = hip.rbf_cutoff(dist, pl.rowptr[N:], a.offset.to(dev), a.coeff, a.cutoff)
    edge_deg = g.deg[g.dst]
    CC.compare_rows(tag, "rbf", rbf[:E], a.ref["rbf"], a.low["rbf"], edge_deg, failures)
    CC.compare_rows(tag, "C", C[:E].view(-1, 1), a.ref["C"], a.low["C"], edge_deg, failures)
    assert bool((rbf[E:] == 0).all()) and bool((C[E:] == 0).all()), "padded edge slots: zero smearing rows and cutoff"
    Wf = torch.cat([a.Wf, torch.full((spare, CC.F), float("nan"))]).to(dev).requires_grad_(True)
    x1d = a.x1.to(dev).requires_grad_(True)
    out = hip.cfconv_aggregate(x1d, Wf, C, pl)
    (out * a.w.to(dev)).sum().backward()
    groups = CC.mol_groups(g)
    CC.compare_rows(tag, "out", out, a.ref["out"], a.low["out"], g.deg, failures, groups)
    CC.compare_rows(tag, "g_x1", x1d.grad, a.ref["g_x1"], a.low["g_x1"], g.deg, failures, groups)
    CC.compare_rows(tag, "g_x1 (by out-degree)", x1d.grad, a.ref["g_x1"], a.low["g_x1"], g.out_deg, failures, groups,
                    classes=CC.OUT_DEG_CLASSES)
    CC.compare_rows(tag, "g_Wf", Wf.grad[:E], a.ref["g_Wf"], a.low["g_Wf"], edge_deg, failures)
    assert bool((Wf.grad[E:] == 0).all()), "g_Wf (padded rows zero)"
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------- 5. graph tables, cap binding ---
def _radius_tables(dev, b, cutoff, n_max):
    """hip.radius_plan against the oracle's edge list: src / dst / rowptr exactly, distances, perm_s / rowptr_s the stable
    by-source grouping (the assertions of test_gpu_kernels._radius_check)."""
    from moleculesde_amd import hip, plan as P
    pl = P.plan_to(P.build_plan(b, with_ext=False), dev)
    pos = b.positions.float()
    N = pos.size(0)
    rp, dist = hip.radius_plan(pos.to(dev), pl.batch_i32, pl.mol_ptr, cutoff, pl.E_r_cap, 32, n_max=n_max)
    ei = R.radius_graph(pos, cutoff, b.batch, 32)
    E = ei.size(1)
    assert int(rp.rowptr[-1]) == E <= pl.E_r_cap
    assert torch.equal(rp.src[:E].cpu().long(), ei[0]) and torch.equal(rp.dst[:E].cpu().long(), ei[1])
    assert torch.equal(rp.rowptr.cpu().long(), torch.searchsorted(ei[1], torch.arange(N + 1)))
    assert bool((rp.src[E:] == -1).all()) and bool((rp.dst[E:] == -1).all()) and bool((dist[E:] == 0).all())
    d64 = (pos.double()[ei[0]] - pos.double()[ei[1]]).norm(dim=-1)
    assert float(((dist[:E].cpu().double() - d64).abs() / d64).max()) <= 4 * U
    perm = rp.perm_s[:E].cpu().long()
    assert torch.equal(torch.sort(perm)[0], torch.arange(E)), "a permutation of the real edges"
    s_sorted = ei[0][perm]
    assert torch.equal(s_sorted, torch.sort(ei[0], stable=True)[0]), "grouped by source"
    assert torch.equal(perm, torch.argsort(ei[0], stable=True)), "stable: canonical order inside a source's row"
    assert torch.equal(rp.rowptr_s.cpu().long(), torch.searchsorted(s_sorted, torch.arange(N + 1)))
    return rp, ei, pl


def test_radius_tables_where_the_cap_binds(dev):
    """hip.radius_plan on several molecules with the 32-neighbour cap binding at once (34, 40, 65, 33 atoms beside 1 and 7):
    the general transposition on the whole cap batch (65 atoms > RADIUS_TRANSPOSE_MOL_NMAX, with and without n_max), and the
    one-workgroup-per-molecule transposition on the batch's molecules of at most 64 atoms."""
    from moleculesde_amd import hip
    b = CC.batch("cap")
    rp, ei, pl = _radius_tables(dev, b, 10.0, None)
    assert pl.N_max == 65 > hip.RADIUS_TRANSPOSE_MOL_NMAX
    deg_s = rp.rowptr_s[1:] - rp.rowptr_s[:-1]
    assert int((rp.rowptr[1:] - rp.rowptr[:-1]).max()) == 32 and int(deg_s.max()) == 64
    rp2, _, _ = _radius_tables(dev, b, 10.0, pl.N_max)
    assert torch.equal(rp2.perm_s, rp.perm_s) and torch.equal(rp2.rowptr_s, rp.rowptr_s)
    small = H.build_batch([s for s in H.CFCONV_CAP_SPECS if s[0] <= hip.RADIUS_TRANSPOSE_MOL_NMAX], seed=H.CFCONV_CAP_SEED)
    rp3, _, pl3 = _radius_tables(dev, small, 10.0, None)
    assert pl3.N_max == 40 and int((rp3.rowptr_s[1:] - rp3.rowptr_s[:-1]).max()) == 39
    rp4, _, _ = _radius_tables(dev, small, 10.0, pl3.N_max)
    assert torch.equal(rp4.perm_s, rp3.perm_s) and torch.equal(rp4.rowptr_s, rp3.rowptr_s), "identical tables, padding included"


# ------------------------------------------------------------------------------------------------ 6. path switch ---
SIZE_CLASSES = (("1-3 atoms", 1, 3), ("20-21 atoms", 20, 21), ("31-32 atoms", 31, 32), ("33 atoms", 33, 33), ("34 atoms", 34, 34))


def _schnet_run(dev, c, use_pairs=True):
    import moleculesde_amd.geom3d as G
    from torch.profiler import profile, ProfilerActivity
    m = G.SchNet(**CC.SCHNET_KW)
    m.load_state_dict(c.state)
    m.to(dev)
    m.use_pairs = use_pairs
    b = G.prepare_batch(c.batch.clone(), dev)
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out, h = m(b.x[:, 0], b.positions, b.batch, return_latent=True)
        ((out * c.w_out.to(dev)).sum() + (h * c.w_h.to(dev)).sum()).backward()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    # the recomputing weight-gradient kernel (cfconv_fused_bwd_w_pipe_kernel) serves both forms (SYM instantiation for pairs):
    # it tells nothing about the path and is left out
    return m, out, h, {"pair": sorted(n for n in names if re.search(r"cfconv_pair_|pair_build", n)),
                       "edge": sorted(n for n in names if re.search(r"cfconv_fused_fwd|cfconv_aggregate_bwd_x|radius_", n))}


@pytest.mark.parametrize("switch,use_pairs", [(False, True), (True, True), (False, False)])
def test_schnet_path_switch_vs_fp64(dev, switch, use_pairs):
    """geom3d.SchNet (2 interactions) around the 33 / 34-atom switch between the pair kernels and the per-edge kernels:
    readout, latent (per molecule) and every parameter gradient against R.SchNet in fp64, bar 8 x R.SchNet's fp32 CPU error;
    the profiler's kernel names show which CFConv form ran.  N_max 33: pair_build / cfconv_pair_* and none of radius_* /
    cfconv_fused_fwd / cfconv_aggregate_bwd_x; N_max 34 (the radius graph is no longer symmetric): the reverse; use_pairs =
    False at N_max 33: the per-edge path on the device's own radius graph."""
    c = CC.schnet_case(switch)
    tag = f"schnet N_max {max(c.sizes)} use_pairs {use_pairs}"
    m, out, h, kernels = _schnet_run(dev, c, use_pairs)
    pairs_expected = use_pairs and not switch
    assert max(c.sizes) == (34 if switch else 33)
    assert bool(kernels["pair"]) == pairs_expected and bool(kernels["edge"]) == (not pairs_expected), kernels
    if pairs_expected:
        assert {k for k in ("pair_build", "cfconv_pair_filter", "cfconv_pair_aggregate") if any(k in n for n in kernels["pair"])} \
            == {"pair_build", "cfconv_pair_filter", "cfconv_pair_aggregate"}, kernels
    else:
        assert {k for k in ("radius_fill", "cfconv_fused_fwd", "cfconv_aggregate_bwd_x") if any(k in n for n in kernels["edge"])} \
            == {"radius_fill", "cfconv_fused_fwd", "cfconv_aggregate_bwd_x"}, kernels
    failures = []
    groups = [(c.mol_ptr[k], c.mol_ptr[k + 1]) for k in range(len(c.sizes))]
    sizes = torch.tensor(c.sizes)
    CC.compare_rows(tag, "readout", out, c.ref["out"], c.low["out"], sizes, failures, classes=SIZE_CLASSES)
    CC.compare_rows(tag, "latent", h, c.ref["h"], c.low["h"], torch.repeat_interleave(sizes, sizes), failures, groups,
                    classes=SIZE_CLASSES)
    tols = CC.param_tolerances(c)
    got = dict(m.named_parameters())
    assert {"grad " + k for k in got} == set(tols)
    worst = ("", 0.0)
    for k, p in got.items():
        assert p.grad is not None, f"{tag}: no gradient for {k}"
        gr = p.grad.detach().double().cpu()
        err = float((gr - c.ref["grad " + k]).abs().max()) if bool(torch.isfinite(gr).all()) else float("inf")
        ratio = err / tols["grad " + k]
        worst = max(worst, (k, ratio), key=lambda t: t[1])
        if not ratio <= 1.0:
            failures.append(f"{tag} grad {k}: err {err:.3e} / tol {ratio:.3f}")
    record_parity(f"cfconv_sizes {tag} parameter gradients: worst err / tol {worst[1]:.2f} ({worst[0]}); kernels "
                  f"{'pair' if pairs_expected else 'per-edge'}")
    assert not failures, "\n".join(failures)
