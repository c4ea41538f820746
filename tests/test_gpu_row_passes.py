"""Row kernels whose column loop is a compile-time pass count (csrc/msde_common.h, LAUNCH_ROWS_PASSES): the GIN gathers, the
embedding sum and the contrastive row kernels -- and the row loop of msde_bn_bwd_fin_cols at chunk edges -- against fp64
evaluations of the same formulas on the host.  Widths: 256 (one pass of 64 float4 lanes), 260 (a second pass with one live
lane), 300 (the workload: two passes), 600 (three passes), 772 (four passes: the run-time column loop).  The tolerances are those of the
tests of the same kernels in tests/test_gpu_kernels.py; every case is run twice and the two results must be bit-equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restate as R  # noqa: E402
from helpers import assert_close  # noqa: E402

WIDTHS = [256, 260, 300, 600, 772]
# 3 + 4 + 2 rows of three bond tables, one below the other (the table-gradient kernel that hip.gin_aggregate's backward also
# launches keeps two copies of the table in LDS: 9 rows fit at D = 772, the 13 of the ogb bond encoder do not)
BOND_DIMS = (3, 4, 2)
BOND_ROWS = sum(BOND_DIMS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()  # fails loudly if libmsde_hip.so is missing
    return torch.device("cuda", 0)


def _graph(N):
    """N = 11: four molecules -- atom 0 alone; the pair 1-2; the path 3-4-5; the star with centre 6 and leaves 7..10.  Every
    bond is stored in both directions.  The path carries two more one-way edges (3->4 and 4->5, parallel to its bonds), so that
    in-degree 3 (atom 4) and out-degree 3 (atom 4) occur beside 0, 1, 2 and 4.  N = 1: one atom, no edge."""
    if N == 1:
        return torch.zeros(2, 0, dtype=torch.long)
    assert N == 11
    bonds = [(1, 2), (3, 4), (4, 5), (6, 7), (6, 8), (6, 9), (6, 10)]
    e = [(a, b) for a, b in bonds] + [(b, a) for a, b in bonds] + [(3, 4), (4, 5)]
    ei = torch.tensor(e, dtype=torch.long).t().contiguous()
    for row in (ei[1], ei[0]):                       # in-degrees (the forward gathers), out-degrees (the backward gather)
        assert set(torch.bincount(row, minlength=N).tolist()) == {0, 1, 2, 3, 4}
    return ei


def _gin_case(N, D, seed):
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(seed)
    plan = hip.build_csr(_graph(N), N)
    E = plan.E
    off = torch.tensor([0, BOND_DIMS[0], BOND_DIMS[0] + BOND_DIMS[1]])
    codes = torch.stack([torch.randint(0, d, (E,), generator=g) for d in BOND_DIMS], 1) + off    # canonical (by-target) edge order
    tab = torch.randn(BOND_ROWS, D, generator=g)
    x = torch.randn(N, D, generator=g)
    w = torch.randn(N, D, generator=g)
    return plan, codes.to(torch.int32), tab, x, w


def _gin_ref(plan, codes, tab, h, w, eps):
    """fp64: out_i = (1 + eps) h_i + sum over edges e into i, in edge order, of relu(h_src(e) + (t0 + t1) + t2), and the
    gradient of sum(out * w) with respect to h."""
    h = h.double().requires_grad_(True)
    t = tab.double()
    src, dst = plan.src.long().cpu(), plan.dst.long().cpu()
    c = codes.long()
    out = (1.0 + eps) * h
    if src.numel():
        msg = torch.relu(h[src] + ((t[c[:, 0]] + t[c[:, 1]]) + t[c[:, 2]]))
        out = out.index_add(0, dst, msg)
    (out * w.double()).sum().backward()
    return out.detach(), h.grad


@pytest.mark.parametrize("N", [11, 1])
@pytest.mark.parametrize("D", WIDTHS)
def test_gin_aggregate_row_passes(dev, N, D):
    """msde_gin_aggregate_fwd / _bwd_x (hip.gin_aggregate without a link): forward and input gradient, 1e-5 / 1e-5 as in
    test_gin_aggregate -- a sum has at most 5 terms whatever D is."""
    from moleculesde_amd import hip
    plan, codes, tab, x, w = _gin_case(N, D, 100 + N + D)
    ref, gref = _gin_ref(plan, codes, tab, x, w, 0.3)
    plan = plan.to(dev)
    codes_d, tab_d, w_d = codes.to(dev), tab.to(dev), w.to(dev)
    eps = torch.full((1,), 0.3, device=dev)
    runs = []
    for _ in range(2):
        xd = x.to(dev).requires_grad_(True)
        out = hip.gin_aggregate(xd, tab_d, eps, plan, codes_d)
        (out * w_d).sum().backward()
        runs.append((out.detach(), xd.grad))
    assert_close(runs[0][0], ref, 1e-5, 1e-5, "gin fwd")
    assert_close(runs[0][1], gref, 1e-5, 1e-5, "gin g_x")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("N", [11, 1])
@pytest.mark.parametrize("D", WIDTHS)
def test_gin_aggregate_bn_link_row_passes(dev, N, D, relu):
    """msde_gin_aggregate_bn_fwd (hip.gin_aggregate with a BnLink): the layer input h = [relu](z scale + shift) is formed on the
    fly and written out (h_out); forward, h_out and the gradient with respect to h, 1e-5 / 1e-5."""
    from moleculesde_amd import hip
    plan, codes, tab, z, w = _gin_case(N, D, 200 + N + D)
    g = torch.Generator().manual_seed(300 + N + D)
    scale, shift = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.5
    h = z.double() * scale.double() + shift.double()
    h = torch.relu(h) if relu else h
    ref, gref = _gin_ref(plan, codes, tab, h, w, 0.3)
    plan = plan.to(dev)
    codes_d, tab_d, w_d = codes.to(dev), tab.to(dev), w.to(dev)
    eps = torch.full((1,), 0.3, device=dev)
    vec = torch.stack([scale, shift]).to(dev)
    z_d = z.to(dev)
    runs = []
    for _ in range(2):
        xd = torch.full((N, D), float("nan"), device=dev).requires_grad_(True)      # written by the kernel
        out = hip.gin_aggregate(xd, tab_d, eps, plan, codes_d, hip.BnLink(z_d, vec, relu))
        (out * w_d).sum().backward()
        runs.append((out.detach(), xd.detach().clone(), xd.grad))
    assert_close(runs[0][0], ref, 1e-5, 1e-5, "gin bn fwd")
    assert_close(runs[0][1], h, 1e-5, 1e-5, "gin bn h_out")
    assert_close(runs[0][2], gref, 1e-5, 1e-5, "gin bn g_x")
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "two runs differ"


@pytest.mark.parametrize("K", [9, 1])
@pytest.mark.parametrize("N", [11, 1])
@pytest.mark.parametrize("D", WIDTHS)
def test_embedding_sum_row_passes(dev, N, D, K):
    """msde_embedding_sum_fwd: out_i = sum over k, left to right, of tab[codes[i, k]]; 1e-6 / 1e-6 as in test_embedding_sum."""
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(400 + N + D + K)
    rows = 7 * K
    tab = torch.randn(rows, D, generator=g)
    codes = torch.randint(0, 7, (N, K), generator=g) + 7 * torch.arange(K)
    ref = tab.double()[codes].sum(1)
    tab_d, codes_d = tab.to(dev), codes.to(torch.int32).to(dev)
    none = torch.zeros(1, dtype=torch.int32, device=dev)       # the node lists serve the backward alone
    with torch.no_grad():
        a = hip.embedding_sum(tab_d, codes_d, none, none)
        b = hip.embedding_sum(tab_d, codes_d, none, none)
    assert_close(a, ref, 1e-6, 1e-6, "embedding sum")
    assert torch.equal(a, b), "two runs differ"


@pytest.mark.parametrize("N", [11, 1])
@pytest.mark.parametrize("D", WIDTHS)
def test_contrastive_rows_row_passes(dev, N, D):
    """msde_cl_ebm_fwd / _bwd (hip.contrastive_ebm) against the oracle's dual_CL in fp64 with the same permutations; the
    tolerances of test_contrastive_ebm_kernels."""
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(500 + N + D)
    X = (torch.randn(N, D, generator=g) * 0.3)
    Y = (torch.randn(N, D, generator=g) * 0.3)
    p1, p2 = torch.randperm(N, generator=g), torch.randperm(N, generator=g)
    Xr, Yr = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    ref, acc_ref = R.dual_CL(Xr, Yr, 0.1, p1, p2)
    (ref * 1.7).backward()
    runs = []
    for _ in range(2):
        Xd, Yd = X.to(dev).requires_grad_(True), Y.to(dev).requires_grad_(True)
        loss, acc = hip.contrastive_ebm(Xd, Yd, p1.to(dev), p2.to(dev), 0.1)
        (loss * 1.7).backward()
        runs.append((loss.detach().clone(), acc.detach().clone(), Xd.grad, Yd.grad))
    loss, acc, gX, gY = runs[0]
    assert_close(loss, ref.detach(), 1e-5, 1e-6, "CL loss")
    assert abs(float(acc) - acc_ref) < 1e-6
    assert_close(gX, Xr.grad, 1e-4, 1e-5 * float(Xr.grad.abs().max()), "CL gX")
    assert_close(gY, Yr.grad, 1e-4, 1e-5 * float(Yr.grad.abs().max()), "CL gY")
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "two runs differ"


# 64-row chunks at every shape: one partial chunk, 2 + a 2-row tail, 4 + a 1-row tail; 70 strips = a second trip of the strip loop
# (the 128-row chunk needs >= 256 workgroups: (3588, 600) in test_bn_bwd_fin_cols_matches_finish_plus_pass)
@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("M,C,strips", [(1, 300, 1), (17, 300, 2), (130, 600, 57), (257, 260, 70)])
def test_bn_bwd_fin_cols_rows(dev, M, C, strips, gate):
    """msde_bn_bwd_fin_cols against fp64: the strip partials summed to dbeta | dgamma, p | w | u formed from them, and
    out = p g' + w z + u over the valid rows with g' = g gated by z xf3 + xf4 > 0; the row bound sits below M and the rows behind
    it are exactly zero; G is a column block of a wider buffer.  2e-5 / 2e-5 as in
    test_bn_bwd_fin_cols_matches_finish_plus_pass."""
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(600 + M + C + strips)
    stats = torch.randn(strips, 2, C, generator=g)
    gamma, mean = torch.randn(C, generator=g), torch.randn(C, generator=g)
    rstd = torch.rand(C, generator=g) + 0.5
    Gw = torch.randn(M, C + 8, generator=g)
    Z = torch.randn(M, C, generator=g)
    xf3 = torch.randn(C, generator=g) if gate else None
    xf4 = torch.randn(C, generator=g) if gate else None
    mv = M - max(1, M // 4)
    # fp64
    s = stats.double().sum(0)
    sum_g, sum_gx = s[0], s[1] * rstd.double()
    inv = 1.0 / mv if mv > 0 else 0.0
    c1, c2 = sum_g * inv, sum_gx * inv
    p = gamma.double() * rstd.double()
    wv = -p * c2 * rstd.double()
    u = p * (c2 * rstd.double() * mean.double() - c1)
    Gd, Zd = Gw[:, 4:4 + C].double(), Z.double()
    if gate:
        Gd = torch.where(Zd * xf3.double() + xf4.double() <= 0, torch.zeros_like(Gd), Gd)
    ref = p * Gd + wv * Zd + u
    ref[mv:] = 0.0
    gb_ref = torch.stack([sum_gx, sum_g])
    # device
    stats_d, gamma_d, mean_d, rstd_d = stats.to(dev), gamma.to(dev), mean.to(dev), rstd.to(dev)
    G_d = Gw.to(dev)[:, 4:4 + C]
    Z_d = Z.to(dev)
    xf3_d = xf3.to(dev) if gate else None
    xf4_d = xf4.to(dev) if gate else None
    with hip.row_bounds({M: torch.tensor([mv], dtype=torch.int32, device=dev)}):
        rows = hip.bound_tensor(M)
        out = torch.full((M, C), float("nan"), device=dev)
        gb = hip._bn_bwd_fin_cols(stats_d, strips, M, C, gamma_d, mean_d, rstd_d, G_d, Z_d, xf3_d, xf4_d, out, rows)
        out_b = torch.full((M, C), float("nan"), device=dev)
        gb_b = hip._bn_bwd_fin_cols(stats_d, strips, M, C, gamma_d, mean_d, rstd_d, G_d, Z_d, xf3_d, xf4_d, out_b, rows)
    assert torch.isfinite(out).all() and bool((out[mv:] == 0).all()), "rows behind the bound are not zero"
    assert_close(out, ref, 2e-5, 2e-5, "input gradient")
    assert_close(gb, gb_ref, 2e-5, 2e-5, "dgamma | dbeta")
    assert torch.equal(out, out_b) and torch.equal(gb, gb_b), "two runs differ"
