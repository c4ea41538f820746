"""Per-operator checks of the twice-differentiable force-path set (moleculesde_amd.dd) against fp64.

Every operator is run on seeded fp32 inputs on the device and compared with a plain fp64 torch restatement of the same
math, run on the CPU, at three levels: the forward; the first derivative autograd.grad(y, inputs, v, create_graph=True);
and the second derivative, the gradient of <w, first derivative> with respect to the inputs AND to v.  Inputs are drawn
in fp32 so that both sides see the same numbers.

Tolerances: `tol` returns (rtol, atol as a fraction of the reference's largest magnitude).  fp32 unit roundoff is
EPS = 2^-24.  A pointwise chain of a few roundings and one transcendental stays within a few ulp, so 16 EPS (~1e-6) per
level; a sum of K terms in fp32 adds rounding growing like sqrt(K) (random-sign errors), so 16 EPS (1 + sqrt(K)) per
reduction on the path, relative to the largest reference entry (entries that cancel to ~0 carry the absolute error of
their terms).  Third derivatives are not part of the set and must raise."""
import math
import types

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()  # fails loudly if libmsde_hip.so is missing
    return torch.device("cuda", 0)


def tol(K=1, depth=1):
    """(rtol, atol fraction) for `depth` chained stages, each a reduction of K terms (K = 1: pointwise)."""
    t = depth * 16 * EPS * (1.0 + (math.sqrt(K) if K > 1 else 0.0))
    return t, t


def _close(got, ref, tl, what):
    if ref is None and got is None:
        return
    if ref is None:
        ref = torch.zeros(got.shape, dtype=torch.float64)
    ref = ref.detach().double().cpu()
    got = torch.zeros_like(ref) if got is None else got.detach().double().cpu()
    rtol, afrac = tl
    assert_close(got, ref, rtol, afrac * float(ref.abs().max()) if ref.numel() else 0.0, what)


def _tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def levels(f_dev, f_ref, xs, dev, tols, second=True, seed=0, what=""):
    """Forward, first and second derivative of f_dev (device, fp32) against f_ref (CPU, fp64).  xs: CPU fp32 inputs.
    tols: three (rtol, atol fraction) pairs.  Returns the device results (y, first grads, second grads)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    xd = [x.to(dev).requires_grad_(True) for x in xs]
    xr = [x.double().requires_grad_(True) for x in xs]
    yd, yr = _tuple(f_dev(*xd)), _tuple(f_ref(*xr))
    assert len(yd) == len(yr)
    for i, (a, b) in enumerate(zip(yd, yr)):
        _close(a, b, tols[0], f"{what} forward[{i}]")
    vs = [torch.randn(y.shape, generator=gen) for y in yr]
    vd = [v.to(dev).requires_grad_(True) for v in vs]
    vr = [v.double().requires_grad_(True) for v in vs]
    gd = torch.autograd.grad(yd, xd, vd, create_graph=second, allow_unused=True)
    gr = torch.autograd.grad(yr, xr, vr, create_graph=second, allow_unused=True)
    for i, (a, b) in enumerate(zip(gd, gr)):
        _close(a, b, tols[1], f"{what} d/dx[{i}]")
    if not second:
        return yd, gd, None
    ws = [None if g is None else torch.randn(g.shape, generator=gen) for g in gr]

    def dd2(gs, xs_, vs_, to):
        pairs = [(g, w.to(to) if to is not None else w.double()) for g, w in zip(gs, ws)
                 if g is not None and g.requires_grad]
        if not pairs:
            return [None] * (len(xs_) + len(vs_))
        return torch.autograd.grad([p[0] for p in pairs], list(xs_) + list(vs_), [p[1] for p in pairs], allow_unused=True)
    hd, hr = dd2(gd, xd, vd, dev), dd2(gr, xr, vr, None)
    for i, (a, b) in enumerate(zip(hd, hr)):
        _close(a, b, tols[2], f"{what} d2[{i}]")
    return yd, gd, hd


def elementwise_derivative(f, x, order):
    """f^(order)(x) for an elementwise fp64 function, by autograd (independent of the kernels' closed forms)."""
    x = x.double().detach().requires_grad_(True)
    y = f(x)
    for _ in range(order):
        y = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
    return y.detach()


# ------------------------------------------------------------------------------------------------ fp64 references
LOG2 = math.log(2.0)


def ref_ssp(x):
    return torch.log1p(torch.exp(x)) - LOG2       # |x| <= 30: exact in fp64, no threshold switch


def ref_silu(x):
    return x * torch.sigmoid(x)


def ref_sqrt_eps(eps):
    e = float(torch.tensor(eps, dtype=torch.float32))     # the kernel adds eps as an fp32 scalar
    return lambda x: torch.sqrt(x + e)


def ref_cutoff(rc, keep):
    def f(d):
        return torch.where(keep & (d < rc), 0.5 * (torch.cos(math.pi * d / rc) + 1.0), torch.zeros_like(d))
    return f


def ref_rbf(offset, coeff, keep):
    off = offset.double()

    def f(d):
        y = torch.exp(coeff * (d.unsqueeze(1) - off) ** 2)
        return torch.where(keep.unsqueeze(1), y, torch.zeros_like(y))
    return f


def _kind_args(kind):
    """(kind id, p0, dd function, fp64 reference) of the pointwise kinds with no mask"""
    from moleculesde_amd import dd
    return {"ssp": (0, 0.0, dd.ssp, ref_ssp),
            "silu": (3, 0.0, dd.silu, ref_silu),
            "sqrt_eps": (4, 1e-8, lambda x: dd.sqrt_eps(x, 1e-8), ref_sqrt_eps(1e-8))}[kind]


def _ssp_inputs():
    return torch.cat([torch.linspace(-30, 30, 4001), torch.tensor([19.999, 20.0, 20.001, -20.0, 0.0])])


def _sqrt_inputs():
    gen = torch.Generator().manual_seed(3)
    return torch.cat([torch.zeros(8), torch.tensor([1e-12, 1e-10, 3e-9, 1e-8, 1e-6]), torch.rand(500, generator=gen) * 4])


# ------------------------------------------------------------------------------------------------ pointwise
@pytest.mark.parametrize("kind", ["ssp", "silu", "sqrt_eps"])
def test_unary_three_levels(dev, kind):
    _, _, f, r = _kind_args(kind)
    gen = torch.Generator().manual_seed(1)
    if kind == "ssp":
        x = _ssp_inputs()
        tl = tol()
    elif kind == "silu":
        x = torch.cat([torch.linspace(-30, 30, 2001), torch.randn(3000, generator=gen) * 4])
        tl = tol()
    else:
        x = _sqrt_inputs()
        # every term of sqrt(s + eps) and its derivatives is positive (no cancellation): elementwise relative, no atol, so
        # the order-2 value at s = 0 (-2.5e11) does not hide errors at ordinary s
        tl = (16 * EPS, 0.0)
    levels(f, r, [x], dev, (tl, (2 * tl[0], tl[1]), (3 * tl[0], tl[1])), what=kind)


@pytest.mark.parametrize("kind", ["ssp", "silu", "sqrt_eps"])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_unary_orders(dev, kind, order):
    from moleculesde_amd import dd
    k, p0, _, r = _kind_args(kind)
    x = _ssp_inputs() if kind != "sqrt_eps" else _sqrt_inputs()
    y = dd._Unary.apply(x.to(dev), k, order, p0, None)
    # one transcendental and <= 6 roundings: 16 EPS elementwise, plus 16 EPS of the largest value for results that are
    # differences of O(1) terms (ssp near 0, s (1 - s) for s -> 1); sqrt_eps has no cancellation: elementwise only
    tl = (16 * EPS, 0.0) if kind == "sqrt_eps" else tol()
    _close(y, elementwise_derivative(r, x, order), tl, f"{kind} order {order}")
    if kind == "sqrt_eps" and order == 2:
        assert abs(float(y[0]) / -2.5e11 - 1.0) < 1e-5          # s = 0 exactly (PaiNN's zero vector features)


def test_cutoff_three_levels_and_mask(dev):
    from moleculesde_amd import dd
    rc = 5.0
    gen = torch.Generator().manual_seed(2)
    below = float(torch.nextafter(torch.tensor(rc), torch.tensor(0.0)))
    d = torch.cat([torch.linspace(0, 1.2 * rc, 3001), torch.tensor([rc, below, rc, below, 1.2 * rc])])
    src = torch.randint(0, 7, d.shape, generator=gen, dtype=torch.int32)
    src[::5] = -1                                                   # padded slots
    src[-5:-3] = 0                                                  # d == rc and one ulp below, unmasked
    keep = src >= 0
    sd = src.to(dev)
    yd, gd, hd = levels(lambda x: dd.cosine_cutoff(x, rc, sd), ref_cutoff(rc, keep), [d], dev,
                        (tol(), tol(depth=2), tol(depth=3)), what="cutoff")
    dead = (~keep) | (d >= rc)
    assert bool((yd[0][dead.to(dev)] == 0).all()) and bool((gd[0][dead.to(dev)] == 0).all())
    assert all(bool((h[dead.to(dev)] == 0).all()) for h in hd if h is not None)
    assert 0.0 <= float(yd[0][-4]) < 1e-6                           # one ulp below rc: (cos(pi - tiny) + 1) / 2
    for order in (0, 1, 2):
        y = dd._Unary.apply(d.to(dev), 1, order, rc, sd)
        ref = elementwise_derivative(ref_cutoff(rc, keep), d, order)
        _close(y, ref, tol(), f"cutoff order {order}")
        assert bool((y[dead.to(dev)] == 0).all()), f"cutoff order {order}: masked / d >= rc not zero"


def test_recip_three_levels(dev):
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(4)
    m = torch.rand(5000, generator=gen) * 3.5 + 0.5
    x = m * torch.where(torch.rand(5000, generator=gen) < 0.5, -1.0, 1.0)
    # the second level chains three products and a reciprocal per element
    levels(dd.recip, lambda t: 1.0 / t, [x], dev, (tol(), tol(depth=3), tol(depth=6)), what="recip")
    src = torch.randint(-1, 3, x.shape, generator=gen, dtype=torch.int32)
    keep, sd = src >= 0, src.to(dev)
    yd, gd, hd = levels(lambda t: dd.recip(t, sd), lambda t: torch.where(keep, 1.0 / t, torch.zeros_like(t)), [x], dev,
                        (tol(), tol(depth=3), tol(depth=6)), what="masked recip")
    pad = (~keep).to(dev)
    assert bool((yd[0][pad] == 0).all()) and bool((gd[0][pad] == 0).all()) and all(bool((h[pad] == 0).all()) for h in hd)


@pytest.mark.parametrize("n", [1, 7, 1023, 4097, 4096 * 256 * 2 + 5])
def test_mul_add_scale(dev, n):
    """ragged n; the last n needs the grid-stride loop (the grid is capped at 4096 blocks of 256)"""
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    # products and sums of fp32 numbers: one rounding each per level, two for the second level's chained products
    levels(dd.mul, lambda x, y: x * y, [a, b], dev, (tol(), tol(), tol(depth=2)), what=f"mul n={n}")
    levels(dd.add, lambda x, y: x + y, [a, b], dev, (tol(), tol(), tol()), what=f"add n={n}")
    levels(lambda x: dd.scale(x, -1.75), lambda x: -1.75 * x, [a], dev, (tol(), tol(), tol()), what=f"scale n={n}")


def test_third_derivative_raises(dev):
    from moleculesde_amd import dd
    x = torch.linspace(0.1, 3.0, 64, device=dev)
    v = torch.ones_like(x)
    for kind, p0 in ((0, 0.0), (1, 5.0), (3, 0.0), (4, 1e-8)):
        xr = x.clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(dd._Unary.apply(xr, kind, 2, p0, None), xr, v)
        g = x.clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(dd._UnaryMul.apply(g, None, xr, kind, 2, p0, None), (g, xr), v)
        y = dd._Unary.apply(xr, kind, 0, p0, None)                  # differentiate f three times
        g1 = torch.autograd.grad(y, xr, v, create_graph=True)[0]
        g2 = torch.autograd.grad(g1, xr, v, create_graph=True)[0]
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(g2, xr, v)
    off = torch.linspace(0, 3, 8, device=dev)
    xr = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(dd._Rbf.apply(xr, None, off, -2.0, 2), xr, torch.ones(64, 8, device=dev))
    y = dd.rbf(xr, None, off, -2.0)
    g1 = torch.autograd.grad(y, xr, torch.ones_like(y), create_graph=True)[0]
    g2 = torch.autograd.grad(g1, xr, v, create_graph=True)[0]
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(g2, xr, v)


# ------------------------------------------------------------------------------------------------ rbf
def _schnet_rbf(G, stop=10.0):
    off = torch.linspace(0.0, stop, G)
    coeff = -0.5 / float(off[1] - off[0]) ** 2 if G > 1 else -0.5     # GaussianSmearing (schnet.py:205-207)
    return off, coeff


@pytest.mark.parametrize("G,stop", [(51, 10.0), (1, 0.0), (50, 5.0)])
def test_rbf_three_levels(dev, G, stop):
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(G)
    E = 777
    off, coeff = _schnet_rbf(G, stop)
    d = torch.rand(E, generator=gen) * 12.0                         # far beyond the last Gaussian too
    src = torch.randint(0, 9, (E,), generator=gen, dtype=torch.int32)
    src[::7] = -1
    keep = src >= 0
    sd, od = src.to(dev), off.to(dev)
    # forward pointwise; the first derivative in d sums G terms (row_dot), the second two such sums in a chain
    yd, gd, hd = levels(lambda x: dd.rbf(x, sd, od, coeff), ref_rbf(off, coeff, keep), [d], dev,
                        (tol(), tol(G), tol(G, depth=2)), what=f"rbf G={G}")
    pad = (~keep).to(dev)
    assert bool((yd[0][pad] == 0).all()) and bool((gd[0][pad] == 0).all()) and bool((hd[0][pad] == 0).all())
    for order in (0, 1, 2):
        y = dd._Rbf.apply(d.to(dev), sd, od, coeff, order)
        dx = d.double().unsqueeze(1).repeat(1, G)
        ref = elementwise_derivative(lambda t: torch.exp(coeff * (t - off.double()) ** 2), dx, order)
        ref[~keep] = 0.0
        _close(y, ref, tol(), f"rbf G={G} order {order}")
        assert bool((y[pad] == 0).all())


# ------------------------------------------------------------------------------------------------ sums and fan-out
@pytest.mark.parametrize("n", [1, 2, 8, 9, 17])
def test_sum_n(dev, n):
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(n)
    xs = [torch.randn(3001, generator=gen) for _ in range(n)]
    # n addends (chained launches beyond 8): n - 1 roundings, bounded by the reduction tolerance of n terms
    levels(lambda *t: dd.sum_n(t), lambda *t: sum(t), xs, dev, (tol(n), tol(n), tol(n)), what=f"sum_n {n}")


def test_fanout_unused_consumer(dev):
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(5)
    x, c0, c1 = (torch.randn(300, 8, generator=gen) for _ in range(3))

    def f_dev(x, c0, c1):
        o = dd.fanout(x, 3)                                        # o[2] unused: its gradient is None
        return dd.add(dd.mul(o[0], c0), dd.mul(o[1], c1))

    levels(f_dev, lambda x, c0, c1: x * c0 + x * c1, [x, c0, c1], dev, (tol(2), tol(2), tol(2, depth=2)), what="fanout")


@pytest.mark.parametrize("layout", ["aligned", "ld_odd", "misaligned", "cols_odd"])
def test_fanout_column_blocks(dev, layout):
    """The gradients of a fan-out whose consumers are column blocks of one wider buffer (torch.cat's backward hands out
    strided views): summed in place by _sum_rows_n when the operands qualify, by sum_n on copies when they do not."""
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(6)
    M, C, n = 1000, (6 if layout == "cols_odd" else 16), 3
    x = torch.randn(M, C, generator=gen, device="cpu").to(dev).requires_grad_(True)
    lead = 1 if layout == "misaligned" else 0
    tail = 1 if layout == "ld_odd" else 0
    V = torch.randn(M, lead + n * C + tail, generator=gen)
    outs = dd.fanout(x, n)
    parts = ([torch.zeros(M, lead, device=dev)] if lead else []) + list(outs) + ([torch.zeros(M, tail, device=dev)] if tail else [])
    y = torch.cat(parts, 1)
    before = dd.CALLS.get("msde_dd_sum_rows_n", 0)
    y.backward(V.to(dev))                                          # no create_graph: grad mode off in the backward
    used = dd.CALLS.get("msde_dd_sum_rows_n", 0) - before
    assert used == (1 if layout == "aligned" else 0), (layout, used)
    ref = sum(V[:, lead + i * C: lead + (i + 1) * C].double() for i in range(n))
    _close(x.grad, ref, tol(n), f"fanout blocks {layout}")
    # the strided path against sum_n on contiguous copies of the same blocks
    blocks = [V.to(dev)[:, lead + i * C: lead + (i + 1) * C] for i in range(n)]
    if layout == "aligned":
        with torch.no_grad():
            assert torch.equal(dd._sum_rows_n(blocks), dd.sum_n([b.contiguous() for b in blocks]))
    else:
        assert dd._sum_rows_n(blocks) is None


# ------------------------------------------------------------------------------------------------ per-edge rows
@pytest.mark.parametrize("E,K", [(37, 1), (37, 3), (101, 63), (101, 64), (101, 65), (50, 200), (20000, 64)])
def test_mul_rows_row_dot(dev, E, K):
    """the last case: E > 16384 rows (row_dot's grid-stride step) and E K > 1.05 M elements (mul_rows's)"""
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(E * K)
    M, s, a, b = (torch.randn(E, K, generator=gen), torch.randn(E, generator=gen), torch.randn(E, K, generator=gen),
                  torch.randn(E, K, generator=gen))
    # mul_rows is a product per element; its first derivative in s and its second are row dots of K terms
    levels(dd.mul_rows, lambda m, t: m * t.unsqueeze(1), [M, s], dev, (tol(), tol(K), tol(K)), what=f"mul_rows {E}x{K}")
    levels(dd.row_dot, lambda x, y: (x * y).sum(1), [a, b], dev, (tol(K), tol(), tol(K)), what=f"row_dot {E}x{K}")


@pytest.mark.parametrize("used", [(True, False, False), (False, True, True), (True, True, True)])
def test_components_merge3(dev, used):
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(501, 3, generator=gen)

    def f_dev(t):
        c = dd.components(t)
        return tuple(ci for ci, u in zip(c, used) if u)

    def f_ref(t):
        return tuple(t[:, i] for i, u in enumerate(used) if u)
    levels(f_dev, f_ref, [x], dev, ((0.0, 0.0),) * 3, what=f"components {used}")     # copies: exact
    parts = [torch.randn(501, generator=gen) if u else None for u in used]
    live = [p for p in parts if p is not None]

    def m_dev(*ts):
        it = iter(ts)
        return dd._Merge3.apply(*[next(it) if u else None for u in used])

    def m_ref(*ts):
        it = iter(ts)
        return torch.stack([next(it) if u else torch.zeros(501, dtype=torch.float64) for u in used], 1)
    levels(m_dev, m_ref, live, dev, ((0.0, 0.0),) * 3, what=f"merge3 {used}")


def _radius_case(dev, cutoff=3.0):
    """A real radius plan with padded slots: molecule 0 spread wider than the cutoff, molecule 1 a single atom, molecule 2
    four atoms close together and one isolated atom."""
    from moleculesde_amd import hip, plan as P
    gen = torch.Generator().manual_seed(8)
    m0 = torch.rand(12, 3, generator=gen) * 6.0
    m1 = torch.zeros(1, 3)
    m2 = torch.cat([torch.rand(4, 3, generator=gen) * 2.0, torch.tensor([[20.0, 20.0, 20.0]])])
    pos = torch.cat([m0, m1, m2])
    batch = torch.tensor([0] * 12 + [1] + [2] * 5)
    d = types.SimpleNamespace(x=torch.zeros(pos.size(0), dtype=torch.long), batch=batch, num_graphs=3, edge_index=None,
                              edge_attr=None)
    pl = P.plan_to(P.build_plan(d, max_nbr=32, with_ext=False), dev)
    rp, _ = hip.radius_plan(pos.to(dev), pl.batch_i32, pl.mol_ptr, cutoff, pl.E_r_cap, 32)
    E = int(rp.rowptr[-1])
    assert 0 < E < rp.E, (E, rp.E)                                 # padded slots exist
    src, dst = rp.src[:E].long().cpu(), rp.dst[:E].long().cpu()
    assert int((src == 17).sum()) == 0 and int((dst == 12).sum()) == 0     # isolated / single atoms: no edges
    return pos, rp, E, src, dst


def _ref_edge_diff(E_cap, src, dst):
    def f(p):
        d = p[src] - p[dst]
        return torch.cat([d, torch.zeros(E_cap - d.size(0), 3, dtype=d.dtype)])
    return f


def _ref_row_norm(E):
    def f(v):
        pad = torch.arange(v.size(0)) >= E
        sq = torch.where(pad, torch.ones_like(v[:, 0]), (v * v).sum(1))
        return torch.where(pad, torch.ones_like(sq), torch.sqrt(sq))
    return f


def test_edge_diff_scatter_row_norm(dev):
    from moleculesde_amd import dd
    pos, rp, E, src, dst = _radius_case(dev)
    Ec, N = rp.E, pos.size(0)
    # differences: one rounding; the scatter (first derivative) sums a node's <= 11 in- and out-edges
    yd, gd, _ = levels(lambda p: dd.edge_diff(p, rp), _ref_edge_diff(Ec, src, dst), [pos], dev,
                       (tol(), tol(32), tol(32)), what="edge_diff")
    assert bool((yd[0][E:] == 0).all())
    assert bool((gd[0][12] == 0).all()) and bool((gd[0][17] == 0).all())
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(Ec, 3, generator=gen)

    def scatter_ref(t):
        return torch.zeros(N, 3, dtype=t.dtype).index_add(0, src, t[:E]).index_add(0, dst, -t[:E])
    yd, gd, _ = levels(lambda t: dd._EdgeScatter.apply(t, rp), scatter_ref, [g], dev, (tol(32), tol(), tol(32)),
                       what="edge_scatter")
    assert bool((gd[0][E:] == 0).all())
    # row norm of vectors that are zero on the padded slots (as edge_diff leaves them): norm 1 there, zero gradient
    v = torch.cat([torch.randn(E, 3, generator=gen), torch.zeros(Ec - E, 3)])
    yd, gd, hd = levels(lambda t: dd.row_norm(t, rp), _ref_row_norm(E), [v], dev, (tol(3), tol(3, 2), tol(3, 4)),
                        what="row_norm")
    assert bool((yd[0][E:] == 1).all()) and bool((gd[0][E:] == 0).all()) and bool((hd[0][E:] == 0).all())
    # the chain the force path differentiates twice: positions -> distances
    levels(lambda p: dd.row_norm(dd.edge_diff(p, rp), rp), lambda p: _ref_row_norm(E)(_ref_edge_diff(Ec, src, dst)(p)),
           [pos], dev, (tol(3), tol(32, 2), tol(32, 4)), what="distance")


# ------------------------------------------------------------------------------------------------ per molecule
@pytest.mark.parametrize("sizes", [[3, 1, 5, 1], [1], [40]])
@pytest.mark.parametrize("mean", [False, True])
def test_seg_reduce_expand(dev, sizes, mean):
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(len(sizes) * 10 + int(mean))
    B, N, K = len(sizes), sum(sizes), 16
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    mol_ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(sizes).cumsum(0)]).to(torch.int32).to(dev)
    bi = batch.to(torch.int32).to(dev)
    cnt = torch.tensor(sizes, dtype=torch.float64).unsqueeze(1)

    def ref(h):
        s = torch.zeros(B, K, dtype=h.dtype).index_add(0, batch, h)
        return s / cnt if mean else s
    h = torch.randn(N, K, generator=gen)
    L = max(sizes)
    levels(lambda t: dd.seg_reduce(t, mol_ptr, bi, mean), ref, [h], dev, (tol(L), tol(), tol(L)), what=f"seg {sizes} {mean}")
    g = torch.randn(B, K, generator=gen)
    levels(lambda t: dd._SegExpand.apply(t, mol_ptr, bi, mean), lambda t: (t / cnt if mean else t)[batch], [g], dev,
           (tol(), tol(L), tol()), what=f"seg_expand {sizes} {mean}")


# ------------------------------------------------------------------------------------------------ message passing
@pytest.mark.parametrize("Fd", [32, 64, 128])
def test_edge_aggregate(dev, Fd):
    from moleculesde_amd import dd
    pos, rp, E, src, dst = _radius_case(dev)
    N = pos.size(0)
    gen = torch.Generator().manual_seed(Fd)
    x, W = torch.randn(N, Fd, generator=gen), torch.randn(rp.E, Fd, generator=gen)

    def ref(x, W):
        return torch.zeros(N, Fd, dtype=x.dtype).index_add(0, dst, x[src] * W[:E])
    # sums over a node's <= 11 edges at every level (aggregation, its transpose; the edge product is pointwise)
    yd, gd, hd = levels(lambda a, b: dd.edge_aggregate(a, b, rp), ref, [x, W], dev, (tol(16), tol(16), tol(16, 2)),
                        what=f"edge_aggregate Fd={Fd}")
    assert bool((gd[1][E:] == 0).all()) and bool((hd[1][E:] == 0).all())     # padded slots: no weight gradient
    assert bool((yd[0][[12, 17]] == 0).all())


# ------------------------------------------------------------------------------------------------ dense
DENSE = [(1, 1, 32), (37, 32, 32), (37, 128, 1), (1029, 37, 128), (1029, 64, 51), (37, 1, 64)]


def _dense_tol(M, N, K, depth):
    return tol(max(M, N, K), depth)


@pytest.mark.parametrize("M,N,K", DENSE)
def test_dense_three_levels(dev, M, N, K):
    """create_graph: the weight gradients go through mm_tn + colsum, the second level through their backward"""
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    x, W, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / math.sqrt(K), torch.randn(N, generator=gen)
    g = torch.randn(M, N, generator=gen)
    t1, t2 = _dense_tol(M, N, K, 1), _dense_tol(M, N, K, 2)
    levels(dd.linear, lambda a, w, c: a @ w.T + c, [x, W, b], dev, (t1, t1, t2), what=f"linear {M}x{N}x{K}")
    levels(dd.mm_nt, lambda a, w: a @ w.T, [x, W], dev, (t1, t1, t2), what=f"mm_nt {M}x{N}x{K}")
    levels(dd.mm_nn, lambda a, w: a @ w, [g, W], dev, (t1, t1, t2), what=f"mm_nn {M}x{N}x{K}")
    levels(dd.mm_tn, lambda a, c: a.T @ c, [g, x], dev, (t1, t1, t2), what=f"mm_tn {M}x{N}x{K}")
    levels(dd.colsum, lambda a: a.sum(0), [g], dev, (t1, t1, t1), what=f"colsum {M}x{N}")
    levels(lambda c: dd._BroadcastRows.apply(c, M), lambda c: c.expand(M, -1), [b], dev, (tol(), t1, t1),
           what=f"broadcast_rows {M}x{N}")


@pytest.mark.parametrize("route", ["create_graph", "immediate", "batch"])
@pytest.mark.parametrize("op", ["linear", "mm_nt"])
@pytest.mark.parametrize("M,N,K", [(1, 32, 32), (37, 1, 64), (1029, 64, 51)])
def test_dense_weight_gradient_routes(dev, route, op, M, N, K):
    """The force path: d = d(out)/d(x) with create_graph under positions_only, then the parameter gradients of
    <v2, out> + <w, d>.  Each weight receives two contributions: the product's own and that of mm_nn inside d, by
    mm_tn + colsum (create_graph), by the immediate split-M launch, or queued into a parameter-gradient batch."""
    from moleculesde_amd import dd, slabs
    gen = torch.Generator().manual_seed(M + N + K)
    x0, W0, b0 = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / math.sqrt(K), torch.randn(N, generator=gen)
    v, v2, w = torch.randn(M, N, generator=gen), torch.randn(M, N, generator=gen), torch.randn(M, K, generator=gen)
    bias = op == "linear"

    def run(x, W, b, v, v2, w, f, positions_only):
        y = f(x, W, b) if bias else f(x, W)
        with positions_only():
            d = torch.autograd.grad(y, x, v, create_graph=True)[0]
        return y, d

    # fp64 reference
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x0, W0, b0))
    yr, dr = run(xr, Wr, br, v.double(), v2.double(), w.double(), lambda a, W_, c=None: a @ W_.T + (c if c is not None else 0),
                 _nullctx)
    ref = torch.autograd.grad([yr, dr], [xr, Wr, br] if bias else [xr, Wr], [v2.double(), w.double()], allow_unused=True)
    xd, Wd, bd = (t.to(dev).requires_grad_(True) for t in (x0, W0, b0))
    f = dd.linear if bias else dd.mm_nt
    y, d = run(xd, Wd, bd, v.to(dev), v2.to(dev), w.to(dev), f, dd.positions_only)
    _close(d, dr, _dense_tol(M, N, K, 1), f"{op} {route}: input gradient")
    ins = [xd, Wd, bd] if bias else [xd, Wd]
    if route == "create_graph":
        got = torch.autograd.grad([y, d], ins, [v2.to(dev), w.to(dev)], create_graph=True)
    else:
        if route == "batch":
            slabs.begin_param_grad_batch(ins[1:])
        try:
            torch.autograd.backward([y, d], [v2.to(dev), w.to(dev)])
        finally:
            if route == "batch":
                slabs.finish_param_grad_batch()
        got = [t.grad for t in ins]
    torch.cuda.synchronize()
    for name, a, r in zip(("x", "W", "b"), got, ref):
        assert a is not None, f"{op} {route}: no gradient for {name}"
        _close(a, r, _dense_tol(M, N, K, 2), f"{op} {route}: d/d{name}")


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize("route", ["immediate", "batch"])
@pytest.mark.parametrize("bias_kind", ["frozen", "non_leaf"])
def test_linear_bias_kinds(dev, route, bias_kind):
    from moleculesde_amd import dd, slabs
    M, N, K = 37, 32, 48
    gen = torch.Generator().manual_seed(11)
    x0, W0, b0, v = (torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(N, generator=gen),
                     torch.randn(M, N, generator=gen))
    xd, Wd = x0.to(dev).requires_grad_(True), W0.to(dev).requires_grad_(True)
    bd = b0.to(dev).requires_grad_(bias_kind == "non_leaf")
    b_in = dd.scale(bd, 2.0) if bias_kind == "non_leaf" else bd
    y = dd.linear(xd, Wd, b_in)
    if route == "batch":
        slabs.begin_param_grad_batch([Wd] + ([bd] if bias_kind == "non_leaf" else []))
    try:
        y.backward(v.to(dev))
    finally:
        if route == "batch":
            slabs.finish_param_grad_batch()
    torch.cuda.synchronize()
    t = _dense_tol(M, N, K, 1)
    _close(xd.grad, v.double() @ W0.double(), t, "x")
    _close(Wd.grad, v.double().T @ x0.double(), t, "W")
    if bias_kind == "frozen":
        assert bd.grad is None
    else:
        _close(bd.grad, 2.0 * v.double().sum(0), t, "non-leaf bias")


@pytest.mark.parametrize("op", ["linear", "mm_nt", "mm_nn"])
def test_positions_only(dev, op):
    """dd.positions_only(): no parameter gradients, input gradients unchanged"""
    from moleculesde_amd import dd
    M, N, K = 37, 32, 48
    gen = torch.Generator().manual_seed(12)
    x0, W0, b0 = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(N, generator=gen)
    xd, Wd, bd = (t.to(dev).requires_grad_(True) for t in (x0, W0, b0))
    if op == "mm_nn":                       # g [M, N] W [N, K]
        g0 = torch.randn(M, N, generator=gen)
        xd = g0.to(dev).requires_grad_(True)
        y, ref_y = dd.mm_nn(xd, Wd), g0.double() @ W0.double()
        v = torch.randn(M, K, generator=gen)
        ref = v.double() @ W0.double().T
    else:
        y = dd.linear(xd, Wd, bd) if op == "linear" else dd.mm_nt(xd, Wd)
        v = torch.randn(M, N, generator=gen)
        ref = v.double() @ W0.double()
    before = dd.CALLS.get("msde_linear_bwd_w", 0)
    with dd.positions_only():
        y.backward(v.to(dev))
    assert dd.CALLS.get("msde_linear_bwd_w", 0) == before           # no weight-gradient launch either
    assert Wd.grad is None and bd.grad is None
    _close(xd.grad, ref, _dense_tol(M, N, K, 1), f"{op} input gradient")


# ------------------------------------------------------------------------------------------------ closure
OURS = ("dd_", "gemm_ex", "gemm_small", "gemm_f32_mfma", "wgrad", "reduce_slabs", "colsum", "cfconv_aggregate", "radius_",
        "scan", "embedding_sum", "segment_sum", "transpose")
# what autograd itself or the test launches: copies of inputs, zero-filled unused gradients, the engine's accumulation
ALLOWED = ("FillFunctor", "Memcpy", "Memset", "CUDAFunctor_add", "direct_copy", "elementwise_kernel_manual_unroll")
U, UM, BIN, RD, MR = "msde_dd_unary", "msde_dd_unary_mul", "msde_dd_binary", "msde_dd_row_dot", "msde_dd_mul_rows"
GEMM = {"msde_gemm_ex", "msde_linear_bwd_w", "msde_colsum", "msde_dd_broadcast_rows"}


def _closure_cases(dev):
    from moleculesde_amd import dd
    gen = torch.Generator().manual_seed(13)
    r = lambda *s: torch.randn(*s, generator=gen)                   # noqa: E731
    pos, rp, E, _, _ = _radius_case(dev)
    off, coeff = _schnet_rbf(51)
    od = off.to(dev)
    d = torch.rand(200, generator=gen) * 6
    s = torch.randint(-1, 3, (200,), generator=gen, dtype=torch.int32).to(dev)
    mol_ptr = torch.tensor([0, 3, 4, 9], dtype=torch.int32, device=dev)
    bi = torch.tensor([0, 0, 0, 1, 2, 2, 2, 2, 2], dtype=torch.int32, device=dev)
    # name: (function, inputs, {launch names allowed at forward, first, second differentiation})
    return {
        "ssp": (dd.ssp, [r(100)], ({U}, {UM}, {UM})),
        "silu": (dd.silu, [r(100)], ({U}, {UM}, {UM})),
        "sqrt_eps": (lambda x: dd.sqrt_eps(x, 1e-8), [r(100).abs()], ({U}, {UM}, {UM})),
        "cutoff": (lambda x: dd.cosine_cutoff(x, 5.0, s), [d], ({U}, {UM}, {UM})),
        "recip": (dd.recip, [r(100).abs() + 0.5], ({U}, {U, BIN}, {U, BIN})),
        "mul": (dd.mul, [r(100), r(100)], ({BIN}, {BIN}, {BIN})),
        "add": (dd.add, [r(100), r(100)], ({BIN}, set(), set())),
        "scale": (lambda x: dd.scale(x, 3.0), [r(100)], ({BIN}, {BIN}, {BIN})),
        "sum_n": (lambda *t: dd.sum_n(t), [r(100) for _ in range(9)], ({"msde_dd_sum_n"}, set(), set())),
        "fanout": (lambda x, c: dd.mul(dd.fanout(x, 3)[0], c), [r(100), r(100)],
                   ({BIN}, {BIN, "msde_dd_sum_n"}, {BIN, "msde_dd_sum_n"})),
        "rbf": (lambda x: dd.rbf(x, s, od, coeff), [d], ({"msde_dd_rbf"}, {"msde_dd_rbf", RD}, {"msde_dd_rbf", RD, MR})),
        "mul_rows": (dd.mul_rows, [r(50, 7), r(50)], ({MR}, {MR, RD}, {MR, RD})),
        "row_dot": (dd.row_dot, [r(50, 7), r(50, 7)], ({RD}, {MR}, {MR, RD})),
        "components": (dd.components, [r(50, 3)], ({"msde_dd_transpose3"}, {"msde_dd_merge3"}, {"msde_dd_transpose3"})),
        "edge_diff": (lambda p: dd.edge_diff(p, rp), [pos], ({"msde_dd_edge_diff"}, {"msde_dd_edge_scatter"},
                                                           {"msde_dd_edge_diff"})),
        "row_norm": (lambda p: dd.row_norm(dd.edge_diff(p, rp), rp), [pos],
                     ({"msde_dd_edge_diff", "msde_dd_row_norm"}, {"msde_dd_edge_scatter", "msde_dd_row_norm", U, BIN, MR},
                      {"msde_dd_edge_diff", "msde_dd_edge_scatter", "msde_dd_row_norm", U, BIN, MR, RD})),
        "seg_reduce": (lambda h: dd.seg_reduce(h, mol_ptr, bi, True), [r(9, 8)],
                       ({"msde_segment_sum_rows"}, {"msde_dd_seg_expand"}, {"msde_segment_sum_rows"})),
        "linear": (dd.linear, [r(37, 16), r(8, 16), r(8)], ({"msde_gemm_ex"}, GEMM, GEMM)),
        "mm_nn": (dd.mm_nn, [r(37, 8), r(8, 16)], ({"msde_gemm_ex"}, GEMM, GEMM)),
        "mm_tn": (dd.mm_tn, [r(37, 8), r(37, 16)], ({"msde_linear_bwd_w"}, GEMM, GEMM)),
        "colsum": (dd.colsum, [r(37, 8)], ({"msde_colsum"}, {"msde_dd_broadcast_rows"}, {"msde_colsum"})),
        "edge_aggregate": (lambda x, W: dd.edge_aggregate(x, W, rp), [r(pos.size(0), 32), r(rp.E, 32)],
                           ({"msde_cfconv_aggregate"}, set(), set())),
    }


CLOSURE = ["ssp", "silu", "sqrt_eps", "cutoff", "recip", "mul", "add", "scale", "sum_n", "fanout", "rbf", "mul_rows",
           "row_dot", "components", "edge_diff", "row_norm", "seg_reduce", "linear", "mm_nn", "mm_tn", "colsum",
           "edge_aggregate"]


@pytest.mark.parametrize("name", CLOSURE)
def test_closure(dev, name):
    """Forward, first and second differentiation of each operator launch only the library kernels its backward is
    written with (dd.CALLS), and no torch compute kernel or vendor GEMM (profiler)."""
    from torch.profiler import profile, ProfilerActivity
    from moleculesde_amd import dd
    f, xs, allowed = _closure_cases(dev)[name]
    gen = torch.Generator().manual_seed(14)
    xd = [x.to(dev).requires_grad_(True) for x in xs]
    with torch.no_grad():
        shapes = [y.shape for y in _tuple(f(*xd))]
    vd = [torch.randn(sh, generator=gen).to(dev).requires_grad_(True) for sh in shapes]
    torch.cuda.synchronize()

    def stage(fn):
        before = dict(dd.CALLS)
        out = fn()
        return out, {k for k, n in dd.CALLS.items() if n != before.get(k, 0)}

    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        y, k0 = stage(lambda: _tuple(f(*xd)))
        g, k1 = stage(lambda: torch.autograd.grad(y, xd, vd, create_graph=True, allow_unused=True))
        live = [t for t in g if t is not None and t.requires_grad]
        ws = [torch.ones_like(t) for t in live]
        _, k2 = stage(lambda: torch.autograd.grad(live, xd + vd, ws, allow_unused=True))
        torch.cuda.synchronize()
    assert k0 and k0 <= allowed[0], (name, "forward", k0)
    assert k1 <= allowed[1], (name, "first", k1)
    assert k2 <= allowed[2], (name, "second", k2)
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    foreign = sorted({n for n in names if not any(k in n for k in OURS)})
    bad = [n for n in foreign if not any(k in n for k in ALLOWED)]
    assert not bad, (name, bad)
    assert not any("Cijk" in n for n in names)
