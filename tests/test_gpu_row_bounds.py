"""Row-bound contract (include/msde_hip.h, "Row bounds"): every entry point that reduces over rows, at a row CAPACITY C with
the valid count c on the device, against a plain fp64 CPU version of the same operation over the first c rows.

What each test does (see BOUNDED for which test covers which entry point):
  - rows >= c of every operand, values and gradients alike, are POISON: finite, far from the data (97 + a row-dependent offset,
    alternating signs), so one padded row in a reduction moves the result far outside tolerance;
  - every output, workspace, slab and partial buffer is filled with NaN before each call (the library never memsets): a split,
    strip or workgroup with no valid rows that skips its write shows up;
  - counts: the weight-gradient family sweeps {0, 1, 3, 31, 32, 33, 255, 256, 257, k_per_split s and +-1 for a middle split s,
    C - 37, C}; the rest {1, 33, C - 37, C} (and 0 for sum-type reductions: exactly zero);
  - identities, bit-exact: a bound equal to C gives the NULL-bound result, two runs agree, the grouped weight-gradient launch
    gives the per-layer slabs where the header promises it;
  - captured once with torch.cuda.graph (one stream, serial launches), replayed after writing C, a small and a middle count into
    the device count: nothing may be decided on the host from the capture-time count, no stale partial may survive.
Padded rows of a row-wise output must be finite; where the header promises zeros (explicitly zeroed gradients), exactly zero.
(A row-wise kernel that merely passes a gradient through gives poison out for poison in: the zero gradients of padded rows in
the product come from the data, not from the kernel.)"""
import ctypes
import math

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

NAN = float("nan")

# entry point -> (test(s) of this file covering it, capacity the product passes).  msde_plan_row_lists alone is checked elsewhere:
# its output is an index table, compared bit-exactly with the host lists by tests/test_gpu_plan.py.
BOUNDED = {
    "msde_linear_bwd_w": ("test_linear_bwd_w_bounded", "N / E_b / E_e / P / 2*E_e: every eager Linear weight gradient"),
    "msde_linear_bwd_w_partial": ("test_wgrad_partial_and_grouped", "same rows as msde_linear_bwd_w (batched path)"),
    "msde_linear_bwd_w_describe": ("test_wgrad_partial_and_grouped", "contiguous operands of the grouped launch"),
    "msde_linear_bwd_w_describe_ld": ("test_wgrad_partial_and_grouped", "column blocks (slabs.py); N, E_e, P, 2*E_e"),
    "msde_linear_bwd_w_grouped_ex": ("test_wgrad_partial_and_grouped", "bound taken from each describe row"),
    "msde_colsum": ("test_colsum_bounded", "N / E_e: bias gradients next to a vendor product"),
    "msde_bn_fwd": ("test_bn_fwd_bwd_bounded", "N (unfused BatchNorm) / E_e (edge BatchNorm)"),
    "msde_bn_bwd": ("test_bn_fwd_bwd_bounded", "N / E_e"),
    "msde_gemm_rs": ("test_gemm_stats_and_bn_finish[strips]", "N (GIN MLP statistics epilogue) via msde_rs_desc.m_valid"),
    "msde_gemm_t2": ("test_gemm_stats_and_bn_finish[tiles]", "N via msde_rs_desc.m_valid"),
    "msde_bn_fin_fwd": ("test_gemm_stats_and_bn_finish, test_pair_stats_bounded", "N / E_e"),
    "msde_bn_fin_bwd": ("test_gemm_stats_and_bn_finish, test_pair_stats_bounded", "N / E_e"),
    "msde_bn_bwd_cols": ("test_bn_cols_family_bounded", "N"),
    "msde_bn_bwd_fin_cols": ("test_bn_cols_family_bounded", "N"),
    "msde_bn_bwd_colstats": ("test_bn_cols_family_bounded", "N"),
    "msde_pair_gather_add_stats": ("test_pair_stats_bounded", "E_e (edge_2D_emb of the 2D->3D model)"),
    "msde_pair_bn_dgrad_stats": ("test_pair_stats_bounded", "E_e"),
    "msde_gin_aggregate_bwd_x_stats": ("test_gin_bounded", "none: not called by the product (the bound is ABI)"),
    "msde_gin_aggregate_bwd_tab": ("test_gin_bounded", "N and E_b"),
    "msde_gin_aggregate_bwd_tab_multi": ("test_gin_bounded", "N and E_b"),
    "msde_plan_row_lists": ("test_gpu_plan.py::test_device_plan_bit_identical_to_host_plan (row lists bit-exact)", "N"),
    "msde_rbf_cutoff_fwd": ("test_rbf_cutoff_bounded", "none in the product (pair path); bound is ABI"),
    "msde_mlp_head_bwd": ("test_mlp_head_bwd_bounded", "E_e (basis MLP, 2*E_e when stacked)"),
    "msde_mlp_head_mix_bwd": ("test_mlp_head_mix_bwd_bounded", "E_e"),
    "msde_cl_ebm_fwd": ("test_contrastive_bounded", "N"),
    "msde_cl_ebm_bwd": ("test_contrastive_bounded", "N"),
    "msde_randperm": ("test_randperm_bounded", "N"),
    "msde_gat_tail_bwd": ("test_gat_tail_bwd_bounded", "N"),
    "msde_dense_loss_fwd": ("test_dense_loss_nmax_bounded", "none (no row bound): nmax_dev = the batch's largest molecule"),
    "msde_dense_loss_bwd": ("test_dense_loss_nmax_bounded", "nmax_dev as above"),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _p(t):
    from moleculesde_amd import hip
    return hip._p(t)


def _st():
    from moleculesde_amd import hip
    return hip._stream()


def _call(name, *args):
    from moleculesde_amd import _lib
    _lib.call(name, *args)


def poison_(t, c):
    """Rows >= c of t (dim 0) := +-(97 + r % 13): finite, far from N(0,1) data, alternating sign."""
    C = t.size(0)
    if c < C:
        r = torch.arange(c, C, device=t.device, dtype=torch.float32)
        v = (97.0 + torch.remainder(r, 13.0)) * (1.0 - 2.0 * torch.remainder(r, 2.0))
        t[c:] = v.view(-1, *([1] * (t.dim() - 1))).to(t.dtype)
    return t


def seeded(shape, c, seed, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return poison_(torch.randn(*shape, generator=g) * scale, c).to(dev)


def clip_counts(C, counts):
    return sorted({min(max(int(x), 0), C) for x in counts})


def counts_std(C, zero=False):
    return clip_counts(C, ([0] if zero else []) + [1, 33, C - 37, C])


def counts_wgrad(C, kps, splits):
    s = max(1, splits // 2)
    return clip_counts(C, [0, 1, 3, 31, 32, 33, 255, 256, 257, kps * s - 1, kps * s, kps * s + 1, C - 37, C])


class Ops:
    """Float operands seeded at full capacity; prep(c) restores the seeded values and poisons rows >= c."""

    def __init__(self, dev, seed):
        self.dev, self.g, self.items = dev, torch.Generator().manual_seed(seed), []

    def add(self, shape, scale=1.0, shift=0.0):
        base = torch.randn(*shape, generator=self.g) * scale + shift
        t = base.to(self.dev)
        self.items.append((t, base))
        return t, base

    def prep(self, c):
        for t, base in self.items:
            t.copy_(base)
            poison_(t, c)


def drive(dev, C, counts, bufs, launch, check, ops, outs=None, replay=True, vals=None):
    """bufs: every buffer the call writes (NaN-filled, int buffers -7, before each call); launch(bound or None) enqueues the
    bounded call(s); check(c) asserts on bufs.  outs: names compared bit-exactly between runs (default: all).  vals(c): the
    device counts for count c when a call takes several (e.g. atoms and edges; default [c])."""
    vals = vals or (lambda c: [c])
    bt = torch.empty(len(vals(C)), dtype=torch.int32, device=dev)
    outs = list(bufs) if outs is None else outs

    def setb(c):
        bt.copy_(torch.tensor(vals(c), dtype=torch.int32))

    def prefill_and_launch(b):
        for t in bufs.values():
            t.fill_(NAN if t.is_floating_point() else -7)
        launch(b)

    def run(b):
        prefill_and_launch(b)
        torch.cuda.synchronize()
        return {k: bufs[k].clone() for k in outs}

    last = None
    for c in counts:
        ops.prep(c)
        setb(c)
        last = run(bt)
        check(c)
        if c == C:
            null = run(None)
            for k in outs:
                assert same(null[k], last[k]), f"{k}: a bound equal to the capacity differs from a NULL bound"
    again = run(bt)
    for k in outs:
        assert same(again[k], last[k]), f"{k}: two runs differ"
    if not replay:
        return
    pos = [x for x in counts if x > 0]
    small, mid = pos[0], pos[len(pos) // 2]
    ops.prep(C)
    setb(C)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):           # warm-up on a side stream, as torch.cuda.graph expects
        prefill_and_launch(bt)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):            # one stream, serial launches, no parallel branches
        prefill_and_launch(bt)
    for c in (C, small, mid):
        ops.prep(c)
        setb(c)
        g.replay()
        torch.cuda.synchronize()
        check(c)
    del g


def same(a, b):
    """Bit-equal, NaN where the other is NaN (slack at the end of a workspace is never written)."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def close(got, ref, rtol, atol, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    assert_close(got, ref, rtol, atol, what)


def zero_rows(t, c, what):
    assert torch.isfinite(t).all(), f"{what}: non-finite values"
    if c < t.size(0):
        assert float(t[c:].abs().max()) == 0.0, f"{what}: rows behind the bound are not zero"


def wgrad_atol(g, x, c):
    """fp32 accumulation over c rows: sqrt(c)-scaled absolute term on the magnitudes of the VALID rows."""
    if c == 0:
        return 0.0
    return 4e-6 * math.sqrt(c) * float(g.abs().max()) * float(x.abs().max())


def _lib_handle():
    from moleculesde_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("C,N,K", [(3588, 300, 300), (35186, 64, 300), (777, 20, 36)])
def test_linear_bwd_w_bounded(dev, C, N, K):
    """msde_linear_bwd_w (one layer, its slab reduction included): gW = gY^T X and gb = column sums of gY over the valid rows;
    gW, gb and the workspace NaN-filled; c = 0 gives exact zeros."""
    lib = _lib_handle()
    ops = Ops(dev, C + N + K)
    gY, gYc = ops.add((C, N))
    X, Xc = ops.add((C, K))
    ws_bytes = int(lib.msde_linear_bwd_w_workspace_bytes(C, N, K))
    splits = ws_bytes // (4 * (N * K + N))
    # the per-layer split plan is not exported: derive k_per_split (a multiple of the 32-row K tile) from the split count the
    # library sized the workspace for, and insist that it reproduces that count -- a changed policy fails here, not silently
    kps = (-(-C // splits) + 31) // 32 * 32
    assert ws_bytes == splits * (N * K + N) * 4 and kps % 32 == 0 and -(-C // kps) == splits and (splits - 1) * kps < C, \
        (C, N, K, splits, kps)
    bufs = {"gW": torch.empty(N, K, device=dev), "gb": torch.empty(N, device=dev), "ws": torch.empty(ws_bytes // 4, device=dev)}

    def launch(b):
        _call("msde_linear_bwd_w", _p(gY), _p(X), C, N, K, _p(bufs["gW"]), _p(bufs["gb"]), _p(bufs["ws"]), _p(b), _st())

    def check(c):
        g, x = gYc[:c].double(), Xc[:c].double()
        if c == 0:
            zero_rows(bufs["gW"], 0, "gW c=0"), zero_rows(bufs["gb"], 0, "gb c=0")
            return
        close(bufs["gW"], g.t() @ x, 1e-5, wgrad_atol(g, x, c), f"gW c={c}")
        close(bufs["gb"], g.sum(0), 1e-5, wgrad_atol(g, torch.ones(1), c), f"gb c={c}")

    drive(dev, C, counts_wgrad(C, kps, splits), bufs, launch, check, ops, outs=["gW", "gb"])


@pytest.mark.parametrize("C,N,K,ld", [(3588, 300, 300, False), (35186, 32, 300, True), (35186, 128, 32, False),
                                      (52680, 16, 32, True), (333, 20, 36, False), (777, 8, 200, True)])
def test_wgrad_partial_and_grouped(dev, C, N, K, ld):
    """msde_linear_bwd_w_partial (slabs [splits][N*K] + bias partials [splits][N]) and the grouped launch of the same problem
    (msde_linear_bwd_w_describe / _describe_ld + msde_linear_bwd_w_grouped_ex, one tile per workgroup and a 7-workgroup limit).
    Every split's slab is written (splits wholly behind the bound: exact zeros), the slabs sum to the fp64 product, and the
    grouped weight slabs equal the per-layer ones bit for bit for the 64 x 64, 32 x 128 and 128 x 32 tile shapes; bias partials
    bit for bit for 64 x 64 only (the narrow shapes group a K tile's rows differently for the column sums, see the header)."""
    lib = _lib_handle()
    ops = Ops(dev, C + 7 * N + K)
    pad = 8 if ld else 0
    gYw, gYc = ops.add((C, N + pad))
    Xw, Xc = ops.add((C, K + pad))
    gYc, Xc = gYc[:, pad // 2:pad // 2 + N], Xc[:, pad // 2:pad // 2 + K]
    gY, X = gYw[:, pad // 2:pad // 2 + N], Xw[:, pad // 2:pad // 2 + K]          # column blocks of wider buffers when ld
    gYk, Xk = torch.empty(C, N, device=dev), torch.empty(C, K, device=dev)     # contiguous copies for the per-layer kernel
    splits = int(lib.msde_linear_bwd_w_splits(C, N, K))
    n_slab = splits * (N * K + N)
    bufs = {"per_layer": torch.empty(n_slab, device=dev), "grouped": torch.empty(n_slab, device=dev),
            "grouped7": torch.empty(n_slab, device=dev)}
    bt_holder = {}

    def describe(slab, bound):
        row = torch.zeros(16, dtype=torch.int64)
        if ld:
            nb = lib.msde_linear_bwd_w_describe_ld(_p(gY), N + pad, _p(X), K + pad, C, N, K, 1, _p(slab), _p(bound),
                                                   ctypes.c_void_p(row.data_ptr()))
        else:
            nb = lib.msde_linear_bwd_w_describe(_p(gY), _p(X), C, N, K, 1, _p(slab), _p(bound), ctypes.c_void_p(row.data_ptr()))
        assert nb > 0, nb
        return row.to(dev), torch.tensor([0, nb], dtype=torch.int32, device=dev), nb, row

    tables = {}

    def launch(b):
        key = b is None
        if key not in tables:
            tables[key] = (describe(bufs["grouped"], b), describe(bufs["grouped7"], b))
        gYk.copy_(gY), Xk.copy_(X)
        _call("msde_linear_bwd_w_partial", _p(gYk), _p(Xk), C, N, K, 1, _p(bufs["per_layer"]), _p(b), _st())
        for (probs, prefix, nb, _), mw in zip(tables[key], (0, 7)):
            _call("msde_linear_bwd_w_grouped_ex", _p(probs), _p(prefix), 1, nb, mw, _st())

    row0 = describe(bufs["grouped"], None)[3]
    kps, shape = int(row0[8]), int(row0[15]) >> 1
    assert int(row0[7]) == splits

    def check(c):
        g, x = gYc[:c].double(), Xc[:c].double()
        for name in ("per_layer", "grouped", "grouped7"):
            s = bufs[name]
            assert torch.isfinite(s).all(), f"{name} c={c}: a slab or bias partial was not written"
            w = s[:splits * N * K].view(splits, N, K)
            bb = s[splits * N * K:].view(splits, N)
            behind = torch.arange(splits, device=s.device) * kps >= c           # splits wholly behind the bound: no tiles
            if bool(behind.any()):
                assert float(w[behind].abs().max()) == 0.0 and float(bb[behind].abs().max()) == 0.0, f"{name}: split behind c={c}"
            close(w.double().sum(0), g.t() @ x, 1e-5, wgrad_atol(g, x, c) + 1e-30, f"{name} weight slabs c={c}")
            close(bb.double().sum(0), g.sum(0), 1e-5, wgrad_atol(g, torch.ones(1), c) + 1e-30, f"{name} bias partials c={c}")
        pl, gr, gr7 = bufs["per_layer"], bufs["grouped"], bufs["grouped7"]
        assert torch.equal(gr, gr7), "grouped launch: the workgroup limit changed the slabs"
        nw = splits * N * K
        if shape in (0, 1, 2):
            assert torch.equal(gr[:nw], pl[:nw]), f"tile shape {shape}: grouped weight slabs differ from the per-layer kernel"
        if shape == 0:
            assert torch.equal(gr[nw:], pl[nw:]), "64 x 64 tiles: grouped bias partials differ from the per-layer kernel"

    drive(dev, C, counts_wgrad(C, kps, splits), bufs, launch, check, ops)


# ------------------------------------------------------------------------------------------------ column sums, BatchNorm
@pytest.mark.parametrize("C,W", [(3588, 300), (35186, 64), (777, 13)])
def test_colsum_bounded(dev, C, W):
    """msde_colsum: out[c] = sum of the valid rows (its workspace NaN-filled); c = 0 gives exact zeros."""
    lib = _lib_handle()
    ops = Ops(dev, C + W)
    X, Xc = ops.add((C, W))
    bufs = {"out": torch.empty(W, device=dev), "ws": torch.empty(int(lib.msde_bn_workspace_floats(C, W)), device=dev)}

    def launch(b):
        _call("msde_colsum", _p(X), C, W, _p(bufs["out"]), _p(bufs["ws"]), _p(b), _st())

    def check(c):
        if c == 0:
            return zero_rows(bufs["out"], 0, "colsum c=0")
        close(bufs["out"], Xc[:c].double().sum(0), 1e-5, wgrad_atol(Xc[:c], torch.ones(1), c), f"colsum c={c}")

    drive(dev, C, counts_std(C, zero=True), bufs, launch, check, ops, outs=["out"])


@pytest.mark.parametrize("C,W", [(3588, 600), (35186, 32), (777, 20)])
def test_bn_fwd_bwd_bounded(dev, C, W):
    """msde_bn_fwd / msde_bn_bwd (training-mode BatchNorm1d, no ReLU) with the statistics over the valid rows: output, saved
    mean / rstd, running buffers, input gradient (zero behind the bound, as norm.hip promises), dgamma, dbeta."""
    lib = _lib_handle()
    ops = Ops(dev, C + W)
    X, Xc = ops.add((C, W), 2.0, 0.5)
    dY, dYc = ops.add((C, W))
    g = torch.Generator().manual_seed(W)
    gamma_c, beta_c = torch.randn(W, generator=g) * 0.3 + 1, torch.randn(W, generator=g) * 0.3
    gamma, beta = gamma_c.to(dev), beta_c.to(dev)
    nws = int(lib.msde_bn_workspace_floats(C, W))
    bufs = {k: torch.empty(C, W, device=dev) for k in ("Y", "dX")}
    bufs.update({k: torch.empty(W, device=dev) for k in ("mean", "rstd", "dgamma", "dbeta", "rm", "rv")})
    bufs.update({"ws": torch.empty(nws, device=dev), "ws2": torch.empty(nws, device=dev)})

    def launch(b):
        bufs["rm"].zero_(), bufs["rv"].fill_(1.0)
        _call("msde_bn_fwd", _p(X), C, W, _p(gamma), _p(beta), 1e-5, 0.1, _p(bufs["rm"]), _p(bufs["rv"]), 0, _p(bufs["Y"]),
              _p(bufs["mean"]), _p(bufs["rstd"]), _p(bufs["ws"]), _p(b), _st())
        _call("msde_bn_bwd", _p(dY), _p(X), _p(bufs["mean"]), _p(bufs["rstd"]), _p(gamma), _p(beta), 0, C, W, _p(bufs["dX"]),
              _p(bufs["dgamma"]), _p(bufs["dbeta"]), _p(bufs["ws2"]), _p(b), _st())

    def check(c):
        x = Xc[:c].double()
        mu, var = x.mean(0), x.var(0, unbiased=False)
        rs = 1 / torch.sqrt(var + 1e-5)
        xh = (x - mu) * rs
        close(bufs["mean"], mu, 1e-5, 1e-5, f"bn mean c={c}")
        close(bufs["rstd"], rs, 1e-4, 1e-5, f"bn rstd c={c}")
        cond = 4e-7 * float(rs.max()) * float(x.abs().max())    # rounding of x - mean, amplified by rstd (316 at c = 1)
        close(bufs["Y"][:c], xh * gamma_c.double() + beta_c.double(), 1e-4, 1e-4 + cond, f"bn y c={c}")
        assert torch.isfinite(bufs["Y"]).all()
        close(bufs["rm"], 0.1 * mu, 1e-5, 1e-6, f"running mean c={c}")
        if c > 1:
            close(bufs["rv"], 0.9 + 0.1 * var * c / (c - 1), 1e-4, 1e-6, f"running var c={c}")
        d = dYc[:c].double()
        db, dg = d.sum(0), (d * xh).sum(0)
        dx = gamma_c.double() * rs * (d - db / c - xh * dg / c)
        at = wgrad_atol(d, xh, c)
        close(bufs["dbeta"], db, 1e-4, at, f"dbeta c={c}")
        close(bufs["dgamma"], dg, 1e-4, at + 1e-6, f"dgamma c={c}")
        close(bufs["dX"][:c], dx, 1e-3, 1e-5 * float(dx.abs().max()) + 1e-6, f"dX c={c}")
        zero_rows(bufs["dX"], c, f"dX c={c}")

    drive(dev, C, counts_std(C), bufs, launch, check, ops, outs=["Y", "dX", "mean", "rstd", "dgamma", "dbeta", "rm", "rv"])


@pytest.mark.parametrize("kind,C,W", [("strips", 3588, 300), ("strips", 200, 64), ("tiles", 3588, 600)])
def test_gemm_stats_and_bn_finish(dev, kind, C, W):
    """msde_gemm_rs / msde_gemm_t2 statistics epilogues (msde_rs_desc.m_valid) finished by msde_bn_fin_fwd / msde_bn_fin_bwd:
    z = x W1^T + b with MSDE_RS_STATS_BNFWD -> mean / rstd / scale / shift / running buffers; g' = gy W2 with
    MSDE_RS_STATS_BNBWD around (z, mean) -> dbeta = sum g', dgamma = rstd sum g' (z - mean), and p g' + w z + u = the
    BatchNorm input gradient.  Strip partials NaN-filled: strips wholly behind the bound must be written too."""
    from moleculesde_amd import hip
    lib = _lib_handle()
    t2 = kind == "tiles"
    K0, K2 = 300, 128
    if t2:
        assert lib.msde_gemm_t2_supported(C, W, K0, 0) == 1 and lib.msde_gemm_t2_supported(C, W, K2, 0) == 1
    ops = Ops(dev, C + W)
    x, xc = ops.add((C, K0))
    gy, gyc = ops.add((C, K2))
    g = torch.Generator().manual_seed(C * W)
    W1c, b1c = torch.randn(W, K0, generator=g) / K0 ** 0.5, torch.randn(W, generator=g) * 0.1 + 2.0
    W2c = torch.randn(K2, W, generator=g) / K2 ** 0.5              # g' = gy W2: [C, K2] x [K2, W]
    gam_c, bet_c = torch.randn(W, generator=g) * 0.3 + 1, torch.randn(W, generator=g) * 0.3
    W1, b1, gam, bet = W1c.to(dev), b1c.to(dev), gam_c.to(dev), bet_c.to(dev)
    B1 = W1 if t2 else W1.t().contiguous()                         # [N][K] for tiles, [K][N] for strips
    B2 = W2c.t().contiguous().to(dev) if t2 else W2c.to(dev)

    def geometry(K):
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _call("msde_gemm_t2_geometry" if t2 else "msde_gemm_rs_geometry", C, W, K, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value
    s1, r1 = geometry(K0)
    s2, _ = geometry(K2)
    bufs = {"z": torch.empty(C, W, device=dev), "gp": torch.empty(C, W, device=dev), "st1": torch.empty(s1, 2, W, device=dev),
            "st2": torch.empty(s2, 2, W, device=dev), "vec": torch.empty(4, W, device=dev), "pwu": torch.empty(5, W, device=dev),
            "rm": torch.empty(W, device=dev), "rv": torch.empty(W, device=dev)}

    def launch(b):
        bufs["rm"].zero_(), bufs["rv"].fill_(1.0)
        v, q = bufs["vec"], bufs["pwu"]
        hip.gemm_rs(x, B1, bufs["z"], bias=b1, stats=bufs["st1"], stats_mode="bnfwd", m_valid=b, N=W, K=K0, b_kmajor=not t2,
                    t2=t2, fallback=False)
        _call("msde_bn_fin_fwd", _p(bufs["st1"]), s1, r1, C, _p(b), W, _p(gam), _p(bet), 1e-5, 0.1, _p(bufs["rm"]),
              _p(bufs["rv"]), _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), _st())
        hip.gemm_rs(gy, B2, bufs["gp"], stats=bufs["st2"], stats_mode="bnbwd", stats_z=bufs["z"], stats_mean=v[2], m_valid=b,
                    N=W, K=K2, b_kmajor=not t2, t2=t2, fallback=False)
        _call("msde_bn_fin_bwd", _p(bufs["st2"]), s2, C, _p(b), W, _p(gam), _p(v[2]), _p(v[3]), _p(q[0]), _p(q[1]), _p(q[2]),
              _p(q[3]), _p(q[4]), _st())

    def check(c):
        assert torch.isfinite(bufs["z"]).all() and torch.isfinite(bufs["gp"]).all()
        z = xc[:c].double() @ W1c.double().t() + b1c.double()
        mu, var = z.mean(0), z.var(0, unbiased=False)
        rs = 1 / torch.sqrt(var + 1e-5)
        v, q = bufs["vec"], bufs["pwu"]
        close(v[2], mu, 1e-5, 1e-5, f"mean c={c}")
        close(v[3], rs, 1e-4, 1e-5, f"rstd c={c}")
        close(v[0], gam_c.double() * rs, 1e-4, 1e-5, f"scale c={c}")
        close(v[1], bet_c.double() - mu * gam_c.double() * rs, 1e-4, 1e-4, f"shift c={c}")
        close(bufs["rm"], 0.1 * mu, 1e-5, 1e-6, f"running mean c={c}")
        if c > 1:
            close(bufs["rv"], 0.9 + 0.1 * var * c / (c - 1), 1e-4, 1e-5, f"running var c={c}")
        gp = gyc[:c].double() @ W2c.double()
        zg, mg = bufs["z"][:c].double().cpu(), v[2].double().cpu()      # the statistics are taken around the stored z, mean
        S1, S2 = gp.sum(0), (gp * (zg - mg)).sum(0)
        at = wgrad_atol(gp, zg - mg, c) + 1e-6
        close(q[4], S1, 1e-4, wgrad_atol(gp, torch.ones(1), c), f"dbeta c={c}")
        close(q[3], S2 * v[3].double().cpu(), 1e-4, at, f"dgamma c={c}")
        rsg = v[3].double().cpu()
        dx = gam_c.double() * rsg * (gp - S1 / c - (zg - mg) * rsg * rsg * S2 / c)
        got = q[0].double().cpu() * bufs["gp"][:c].double().cpu() + q[1].double().cpu() * zg + q[2].double().cpu()
        cond = 1e-6 * float(rsg.max()) * float(gam_c.abs().max()) * float(gp.abs().max())   # rstd-amplified rounding (c = 1)
        assert_close(got, dx, 1e-3, 2e-5 * float(dx.abs().max()) + 1e-6 + cond, f"p g' + w z + u c={c}")

    drive(dev, C, counts_std(C), bufs, launch, check, ops, outs=["z", "gp", "st1", "st2", "vec", "pwu", "rm", "rv"])


# ------------------------------------------------------------------------------------------------ losses, permutations, RBF, head
@pytest.mark.parametrize("C,D", [(3588, 300), (777, 20)])
def test_contrastive_bounded(dev, C, D):
    """msde_cl_ebm_fwd / _bwd (dual EBM-NCE, examples/util.py:52-68,76-79) over the valid rows with permutations of them (padded
    entries map to themselves, as msde_randperm leaves them): loss / accuracy against the oracle's dual_CL in fp64, gX / gY on
    the valid rows, zero behind the bound; `rows` (the logits) finite everywhere."""
    from oracle import restate as R
    ops = Ops(dev, C + D)
    X, Xc = ops.add((C, D), 0.3)
    Y, Yc = ops.add((C, D), 0.3)
    perms = {}
    p1, p2 = torch.empty(C, dtype=torch.int32, device=dev), torch.empty(C, dtype=torch.int32, device=dev)
    gl = torch.tensor([1.7], device=dev)
    bufs = {"rows": torch.empty(C, 3, device=dev), "inv1": torch.empty(C, dtype=torch.int32, device=dev),
            "inv2": torch.empty(C, dtype=torch.int32, device=dev), "out": torch.empty(2, device=dev),
            "gX": torch.empty(C, D, device=dev), "gY": torch.empty(C, D, device=dev)}
    prep0 = ops.prep

    def prep(c):
        prep0(c)
        g = torch.Generator().manual_seed(c)
        a, b = torch.arange(C), torch.arange(C)
        a[:c], b[:c] = torch.randperm(c, generator=g), torch.randperm(c, generator=g)
        perms[c] = (a, b)
        p1.copy_(a), p2.copy_(b)
    ops.prep = prep

    def launch(b):
        _call("msde_cl_ebm_fwd", _p(X), _p(Y), _p(p1), _p(p2), C, D, 10.0, _p(bufs["rows"]), _p(bufs["inv1"]), _p(bufs["inv2"]),
              _p(bufs["out"]), _p(b), _st())
        _call("msde_cl_ebm_bwd", _p(X), _p(Y), _p(p1), _p(p2), _p(bufs["inv1"]), _p(bufs["inv2"]), _p(bufs["rows"]), _p(gl), C, D,
              10.0, _p(bufs["gX"]), _p(bufs["gY"]), _p(b), _st())

    def check(c):
        a, b = perms[c]
        xr = Xc[:c].double().requires_grad_(True)
        yr = Yc[:c].double().requires_grad_(True)
        loss, acc = R.dual_CL(xr, yr, 0.1, a[:c], b[:c])
        (loss * 1.7).backward()
        close(bufs["out"][0], loss.detach(), 1e-5, 1e-6, f"CL loss c={c}")
        assert abs(float(bufs["out"][1]) - float(acc)) < 1e-6, f"CL accuracy c={c}"
        close(bufs["gX"][:c], xr.grad, 1e-4, 1e-5 * float(xr.grad.abs().max()), f"gX c={c}")
        close(bufs["gY"][:c], yr.grad, 1e-4, 1e-5 * float(yr.grad.abs().max()), f"gY c={c}")
        zero_rows(bufs["gX"], c, "gX"), zero_rows(bufs["gY"], c, "gY")
        assert torch.isfinite(bufs["rows"]).all(), f"rows c={c}: padded logits not written"

    drive(dev, C, counts_std(C), bufs, launch, check, ops, outs=["rows", "out", "gX", "gY"])


@pytest.mark.parametrize("C", [3588, 777])
def test_randperm_bounded(dev, C):
    """msde_randperm with a row bound: each of the two draws is a permutation of range(c) followed by the identity."""
    ops = Ops(dev, C)
    bufs = {"out": torch.empty(2, C, dtype=torch.int32, device=dev)}

    def launch(b):
        _call("msde_randperm", C, 2, 1234, _p(None), _p(bufs["out"]), _p(b), _st())

    def check(c):
        o = bufs["out"].cpu().long()
        for r in range(2):
            assert torch.equal(torch.sort(o[r, :c])[0], torch.arange(c)), f"draw {r}: not a permutation of range({c})"
            assert torch.equal(o[r, c:], torch.arange(c, C)), f"draw {r}: padded entries do not map to themselves"

    drive(dev, C, counts_std(C), bufs, launch, check, ops)


@pytest.mark.parametrize("C,G", [(49152, 51), (777, 50)])
def test_rbf_cutoff_bounded(dev, C, G):
    """msde_rbf_cutoff_fwd: Gaussian smearing + cosine cutoff (no zeroing past the cutoff: schnet.py:186) on the valid edges,
    exact zeros behind E_dev (header)."""
    ops = Ops(dev, C)
    d, dc = ops.add((C,), 0.0, 0.0)
    dc.copy_(torch.rand(C, generator=torch.Generator().manual_seed(C)) * 12.0)
    off = torch.linspace(0, 10, G)
    coeff, cutoff = -0.5 / float(off[1] - off[0]) ** 2, 10.0
    offd = off.to(dev)
    bufs = {"rbf": torch.empty(C, G, device=dev), "C": torch.empty(C, device=dev)}

    def launch(b):
        _call("msde_rbf_cutoff_fwd", _p(d), _p(b), C, G, _p(offd), coeff, cutoff, _p(bufs["rbf"]), _p(bufs["C"]), _st())

    def check(c):
        x = dc[:c].double()
        close(bufs["rbf"][:c], torch.exp(coeff * (x[:, None] - off.double()) ** 2), 1e-5, 1e-6, f"rbf c={c}")
        cref = 0.5 * (torch.cos(x * math.pi / cutoff) + 1)
        close(bufs["C"][:c], cref, 1e-5, 1e-6, f"cutoff c={c}")
        zero_rows(bufs["rbf"], c, "rbf"), zero_rows(bufs["C"], c, "C")

    drive(dev, C, counts_std(C), bufs, launch, check, ops)


@pytest.mark.parametrize("C,H,J", [(35186, 128, 3), (777, 36, 4)])
def test_mlp_head_bwd_bounded(dev, C, H, J):
    """msde_mlp_head_bwd (basis MLP output layer, equivariant_scorenetwork.py:142-146): gZ = (g W) silu'(Z) on the valid rows
    and zero behind the bound (header), [gW | gb] = [g^T silu(Z) | sum g] over the valid rows; slabs NaN-filled."""
    lib = _lib_handle()
    ops = Ops(dev, C + H)
    Z, Zc = ops.add((C, H))
    g, gc = ops.add((C, J))
    Wc = torch.randn(J, H, generator=torch.Generator().manual_seed(H)) / H ** 0.5
    W = Wc.to(dev)
    nsl = int(lib.msde_mlp_head_bwd_slabs(C, H))
    wl = (J * H + J + 3) // 4 * 4
    bufs = {"gZ": torch.empty(C, H, device=dev), "gWb": torch.empty(wl, device=dev), "ws": torch.empty(nsl * wl, device=dev)}

    def launch(b):
        _call("msde_mlp_head_bwd", _p(Z), H, _p(W), _p(g), C, H, J, _p(bufs["gZ"]), _p(bufs["gWb"]), _p(bufs["ws"]), _p(b), _st())

    def check(c):
        z, gg = Zc[:c].double(), gc[:c].double()
        sg = torch.sigmoid(z)
        silu, dsilu = z * sg, sg * (1 + z * (1 - sg))
        close(bufs["gZ"][:c], (gg @ Wc.double()) * dsilu, 1e-4, 1e-6, f"gZ c={c}")
        zero_rows(bufs["gZ"], c, "gZ")
        at = wgrad_atol(gg, silu, c) + 1e-30
        close(bufs["gWb"][:J * H].view(J, H), gg.t() @ silu, 1e-5, at, f"gW c={c}")
        close(bufs["gWb"][J * H:J * H + J], gg.sum(0), 1e-5, wgrad_atol(gg, torch.ones(1), c) + 1e-30, f"gb c={c}")

    drive(dev, C, counts_std(C), bufs, launch, check, ops, outs=["gZ", "gWb"])


# ------------------------------------------------------------------------------------------------ BatchNorm column kernels
@pytest.mark.parametrize("C,W,gate", [(3588, 300, True), (1000, 20, False)])
def test_bn_cols_family_bounded(dev, C, W, gate):
    """msde_bn_bwd_colstats (per 64-row strip: sum g', sum g' (Z - mean), g' = G gated by Y > 0), msde_bn_bwd_cols
    (p g' + w Z + u, g' gated where Z xf3 + xf4 <= 0; zero behind the bound) and msde_bn_bwd_fin_cols (the finish of strip
    partials inside the same pass: dgamma = rstd sum_s S2, dbeta = sum_s S1, counts from the bound)."""
    ops = Ops(dev, C + W)
    G, Gc = ops.add((C, W))
    Z, Zc = ops.add((C, W), 1.0, 0.3)
    Y, Yc = ops.add((C, W))
    g = torch.Generator().manual_seed(W)
    vec_c = [torch.randn(W, generator=g) for _ in range(5)]
    mean_c, p_c, w_c, u_c, xf4_c = vec_c
    rstd_c, gam_c, xf3_c = torch.rand(W, generator=g) + 0.5, torch.randn(W, generator=g), torch.randn(W, generator=g)
    strips = -(-C // 64)
    st_c = torch.randn(strips, 2, W, generator=g)
    mean, p, w, u, xf4, rstd, gam, xf3, st = (t.to(dev) for t in (mean_c, p_c, w_c, u_c, xf4_c, rstd_c, gam_c, xf3_c, st_c))
    xf3p, xf4p = (xf3, xf4) if gate else (None, None)
    bufs = {"stats": torch.empty(strips, 2, W, device=dev), "cols": torch.empty(C, W, device=dev),
            "fin": torch.empty(C, W, device=dev), "gb": torch.empty(2, W, device=dev)}

    def launch(b):
        _call("msde_bn_bwd_colstats", _p(G), _p(Z), _p(Y), _p(mean), C, _p(b), W, _p(bufs["stats"]), _st())
        _call("msde_bn_bwd_cols", _p(G), W, _p(Z), W, _p(p), _p(w), _p(u), _p(xf3p), _p(xf4p), C, _p(b), W, _p(bufs["cols"]), W,
              _st())
        _call("msde_bn_bwd_fin_cols", _p(st), strips, _p(gam), _p(mean), _p(rstd), _p(G), W, _p(Z), W, _p(xf3p), _p(xf4p), C,
              _p(b), W, _p(bufs["fin"]), W, _p(bufs["gb"][0]), _p(bufs["gb"][1]), _st())

    def gated(c):
        gg, z = Gc[:c].double(), Zc[:c].double()
        return torch.where(z * xf3_c.double() + xf4_c.double() <= 0, torch.zeros_like(gg), gg) if gate else gg

    def check(c):
        gg, z = Gc[:c].double(), Zc[:c].double()
        g1 = torch.where(Yc[:c].double() > 0, gg, torch.zeros_like(gg))
        at = wgrad_atol(g1, z - mean_c.double(), c) + 1e-6
        close(bufs["stats"][:, 0].double().sum(0), g1.sum(0), 1e-5, at, f"colstats sum g' c={c}")
        close(bufs["stats"][:, 1].double().sum(0), (g1 * (z - mean_c.double())).sum(0), 1e-5, at, f"colstats sum g'(z-m) c={c}")
        behind = torch.arange(strips) * 64 >= c
        if bool(behind.any()):
            assert float(bufs["stats"][behind.to(dev)].abs().max()) == 0.0, f"colstats: strips behind c={c} not zero"
        ref = p_c.double() * gated(c) + w_c.double() * z + u_c.double()
        close(bufs["cols"][:c], ref, 1e-5, 1e-5, f"bn_bwd_cols c={c}")
        zero_rows(bufs["cols"], c, f"bn_bwd_cols c={c}")
        S1, S2 = st_c[:, 0].double().sum(0), st_c[:, 1].double().sum(0)
        rs, gm, mu = rstd_c.double(), gam_c.double(), mean_c.double()
        pp = gm * rs
        fin = pp * gated(c) + (-pp * (S2 * rs / c) * rs) * z + pp * ((S2 * rs / c) * rs * mu - S1 / c)
        close(bufs["gb"][1], S1, 1e-5, 1e-5, f"fin_cols dbeta c={c}")
        close(bufs["gb"][0], S2 * rs, 1e-5, 1e-5, f"fin_cols dgamma c={c}")
        close(bufs["fin"][:c], fin, 1e-4, 1e-4 * float(fin.abs().max()) + 1e-5, f"fin_cols c={c}")
        zero_rows(bufs["fin"], c, f"fin_cols c={c}")

    drive(dev, C, counts_std(C), bufs, launch, check, ops)


# ------------------------------------------------------------------------------------------------ edge BatchNorm (2D->3D)
@pytest.mark.parametrize("C,Nat", [(35186, 3588), (777, 100)])
def test_pair_stats_bounded(dev, C, Nat):
    """msde_pair_gather_add_stats -> msde_bn_fin_fwd (strips of msde_pair_strip() edges) and msde_pair_bn_dgrad_stats ->
    msde_bn_fin_bwd over the valid edges e < *e_valid; padded slots carry src = dst = -1 as the plan leaves them.  Gathered
    rows have mean ~3, so zero rows counted into the statistics would show."""
    lib = _lib_handle()
    D, H = 32, 32
    SR = int(lib.msde_pair_strip())
    strips = -(-C // SR)
    ops = Ops(dev, C + Nat)
    AB, ABc = ops.add((Nat, 2 * D), 1.0, 1.5)
    AB.copy_(ABc)
    ops.items.pop()                                       # node rows: all valid (the bound is on edges)
    gE, gEc = ops.add((C, H))
    g = torch.Generator().manual_seed(C)
    Wc = torch.randn(H, D, generator=g) / H ** 0.5
    gam_c, bet_c = torch.randn(D, generator=g) * 0.3 + 1, torch.randn(D, generator=g) * 0.3
    W, gam, bet = Wc.to(dev), gam_c.to(dev), bet_c.to(dev)
    src, dst = torch.full((C,), -1, dtype=torch.int32, device=dev), torch.full((C,), -1, dtype=torch.int32, device=dev)
    edges = {}
    prep0 = ops.prep

    def prep(c):
        prep0(c)
        gg = torch.Generator().manual_seed(c)
        s_, d_ = torch.full((C,), -1, dtype=torch.int32), torch.full((C,), -1, dtype=torch.int32)
        s_[:c], d_[:c] = torch.randint(0, Nat, (c,), generator=gg), torch.randint(0, Nat, (c,), generator=gg)
        edges[c] = (s_[:c].long(), d_[:c].long())
        src.copy_(s_), dst.copy_(d_)
    ops.prep = prep
    bufs = {"pre": torch.empty(C, D, device=dev), "st": torch.empty(strips, 2, D, device=dev), "v": torch.empty(4, D, device=dev),
            "GA": torch.empty(C, D, device=dev), "sta": torch.empty(strips, 2, D, device=dev), "q": torch.empty(5, D, device=dev),
            "rm": torch.empty(D, device=dev), "rv": torch.empty(D, device=dev)}

    def launch(b):
        v, q = bufs["v"], bufs["q"]
        bufs["rm"].zero_(), bufs["rv"].fill_(1.0)
        _call("msde_pair_gather_add_stats", _p(AB), AB.data_ptr() + 4 * D, 2 * D, _p(src), _p(dst), C, D, _p(b), _p(bufs["pre"]),
              _p(bufs["st"]), _st())
        _call("msde_bn_fin_fwd", _p(bufs["st"]), strips, SR, C, _p(b), D, _p(gam), _p(bet), 1e-5, 0.1, _p(bufs["rm"]),
              _p(bufs["rv"]), _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), _st())
        _call("msde_pair_bn_dgrad_stats", _p(gE), H, _p(W), _p(bufs["pre"]), _p(v[0]), _p(v[1]), _p(v[2]), C, H, D, _p(b),
              _p(bufs["GA"]), _p(bufs["sta"]), _st())
        _call("msde_bn_fin_bwd", _p(bufs["sta"]), strips, C, _p(b), D, _p(gam), _p(v[2]), _p(v[3]), _p(q[0]), _p(q[1]), _p(q[2]),
              _p(q[3]), _p(q[4]), _st())

    def check(c):
        s_, d_ = edges[c]
        pre = ABc[s_, :D].double() + ABc[d_, D:].double()
        close(bufs["pre"][:c], pre, 1e-6, 1e-6, f"gathered rows c={c}")
        zero_rows(bufs["pre"], c, "gathered rows")
        mu, var = pre.mean(0), pre.var(0, unbiased=False)
        rs = 1 / torch.sqrt(var + 1e-5)
        v, q = bufs["v"], bufs["q"]
        close(v[2], mu, 1e-5, 1e-5, f"edge bn mean c={c}")
        close(v[3], rs, 1e-4, 1e-5 + 1e-6 * float(rs.max()), f"edge bn rstd c={c}")
        sc, sh, mg = v[0].double().cpu(), v[1].double().cpu(), v[2].double().cpu()
        pg = bufs["pre"][:c].double().cpu()
        ga = gEc[:c].double() @ Wc.double()
        ga = torch.where(pg * sc + sh <= 0, torch.zeros_like(ga), ga)
        close(bufs["GA"][:c], ga, 1e-4, 1e-5, f"GA c={c}")
        assert torch.isfinite(bufs["GA"]).all()
        S1, S2 = ga.sum(0), (ga * (pg - mg)).sum(0)
        at = wgrad_atol(ga, pg - mg, c) + 1e-6
        close(q[4], S1, 1e-4, at, f"edge dbeta c={c}")
        close(q[3], S2 * v[3].double().cpu(), 1e-4, at * float(v[3].max()), f"edge dgamma c={c}")

    drive(dev, C, counts_std(C), bufs, launch, check, ops)


# ------------------------------------------------------------------------------------------------ GIN
def _gin_graph(Nat, E, cN, cE, seed):
    """cE bond slots among the first cN atoms, by-target canonical order; padded slots src = dst = -1, codes 0."""
    g = torch.Generator().manual_seed(seed)
    src = torch.full((E,), -1, dtype=torch.int64)
    dst = torch.full((E,), -1, dtype=torch.int64)
    if cN > 0 and cE > 0:
        d_ = torch.sort(torch.randint(0, cN, (cE,), generator=g))[0]
        src[:cE], dst[:cE] = torch.randint(0, cN, (cE,), generator=g), d_
    codes = torch.zeros(E, 3, dtype=torch.int64)
    codes[:cE] = torch.stack([torch.randint(0, 5, (cE,), generator=g), torch.randint(5, 11, (cE,), generator=g),
                              torch.randint(11, 13, (cE,), generator=g)], 1)
    s_valid = src[:cE]
    perm_s = torch.arange(E)
    perm_s[:cE] = torch.argsort(s_valid, stable=True)
    rowptr_s = torch.searchsorted(s_valid[perm_s[:cE]], torch.arange(Nat + 1))
    return src, dst, codes, rowptr_s, perm_s


@pytest.mark.parametrize("C,E,D", [(3588, 7300, 300), (333, 700, 64)])
def test_gin_bounded(dev, C, E, D):
    """msde_gin_aggregate_bwd_tab (bond-table and eps gradients, bounds n_dev on atoms and e_dev on bonds), its slab form and
    msde_gin_aggregate_bwd_tab_multi (two layers, slabs summed here), and msde_gin_aggregate_bwd_x_stats (input gradient with
    the previous BatchNorm's strip partials over rows < *m_valid): fp64 over the valid atoms and bonds."""
    lib = _lib_handle()
    R = 13
    ops = Ops(dev, C + D)
    x, xc = ops.add((C, D))
    gA, gAc = ops.add((C, D))
    x2, x2c = ops.add((C, D))
    g2, g2c = ops.add((C, D))
    zp, zpc = ops.add((C, D))
    gg = torch.Generator().manual_seed(D)
    tab_c, mean_c = torch.randn(R, D, generator=gg) * 0.5, torch.randn(D, generator=gg)
    tab, mean = tab_c.to(dev), mean_c.to(dev)
    eps = torch.tensor([0.3], device=dev)
    frac = E / C

    def cE_of(c):
        return min(E, int(round(c * frac)))
    graphs = {}
    srcd, dstd = torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
    codesd, permd = torch.empty(E, 3, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
    rpd = torch.empty(C + 1, dtype=torch.int32, device=dev)
    prep0 = ops.prep

    def prep(c):
        prep0(c)
        gr = graphs[c] = _gin_graph(C, E, c, cE_of(c), c)
        for t, v in zip((srcd, dstd, codesd, rpd, permd), gr):
            t.copy_(v.to(torch.int32))
    ops.prep = prep
    nws = int(lib.msde_gin_aggregate_bwd_tab_workspace_floats(C, E, D, R))
    nsl = int(lib.msde_gin_aggregate_bwd_tab_slabs(C, E))
    bufs = {"g_tab": torch.empty(R, D, device=dev), "g_eps": torch.empty(1, device=dev), "ws": torch.empty(nws, device=dev),
            "ws_a": torch.empty(nws, device=dev), "ws_b": torch.empty(nws, device=dev), "ws_1": torch.empty(nws, device=dev),
            "g_x": torch.empty(C, D, device=dev), "stats": torch.empty(-(-C // 16), 2, D, device=dev)}
    harr = lambda *ts: ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), ctypes.c_void_p)  # noqa: E731

    def launch(b):
        nb, eb = (b[0:1], b[1:2]) if b is not None else (None, None)
        _call("msde_gin_aggregate_bwd_tab", _p(gA), _p(x), _p(tab), _p(codesd), _p(srcd), _p(dstd), C, E, D, R, _p(bufs["g_tab"]),
              _p(bufs["g_eps"]), _p(bufs["ws"]), _p(nb), _p(eb), _st())
        _call("msde_gin_aggregate_bwd_tab", _p(gA), _p(x), _p(tab), _p(codesd), _p(srcd), _p(dstd), C, E, D, R, _p(None),
              _p(None), _p(bufs["ws_1"]), _p(nb), _p(eb), _st())
        _call("msde_gin_aggregate_bwd_tab_multi", harr(gA, g2), harr(x, x2), harr(tab, tab), harr(bufs["ws_a"], bufs["ws_b"]), 2,
              _p(codesd), _p(srcd), _p(dstd), C, E, D, R, _p(nb), _p(eb), _st())
        _call("msde_gin_aggregate_bwd_x_stats", _p(gA), _p(x), _p(tab), _p(codesd), _p(eps), _p(rpd), _p(permd), _p(dstd), C,
              _p(nb), D, _p(zp), _p(mean), 1, _p(bufs["g_x"]), _p(bufs["stats"]), _st())

    def tab_ref(g, xx, c):
        src, dst, codes, _, _ = graphs[c]
        ce = cE_of(c)
        s_, d_, cd = src[:ce], dst[:ce], codes[:ce]
        emb = tab_c.double()[cd].sum(1)
        m = g.double()[d_] * ((xx.double()[s_] + emb) > 0)
        gt = torch.zeros(R, D, dtype=torch.float64)
        for k in range(3):
            gt.index_add_(0, cd[:, k], m)
        return gt, (g.double()[:c] * xx.double()[:c]).sum().reshape(1), m, s_

    def slab_sum(ws):
        return ws[:nsl * R * D].view(nsl, R * D).double().sum(0).view(R, D), ws[nsl * R * D:nsl * R * D + nsl].double().sum()

    def check(c):
        gt, ge, m, s_ = tab_ref(gAc, xc, c)
        at = 4e-6 * math.sqrt(max(cE_of(c), 1)) * 3 * float(gAc[:c].abs().max() if c else 0) + 1e-6
        close(bufs["g_tab"], gt, 1e-5, at, f"g_tab c={c}")
        close(bufs["g_eps"], ge, 1e-5, wgrad_atol(gAc[:c], xc[:c], c) * math.sqrt(D) + 1e-6, f"g_eps c={c}")
        for name, (gref, eref) in (("ws_1", (gt, ge)), ("ws_a", (gt, ge)), ("ws_b", tab_ref(g2c, x2c, c)[:2])):
            assert torch.isfinite(bufs[name][:nsl * (R * D + 1)]).all(), f"{name} c={c}: a slab was not written"
            st_, se_ = slab_sum(bufs[name])
            close(st_, gref, 1e-5, at * 2, f"{name} table slabs c={c}")
            close(se_.reshape(1), eref, 1e-5, wgrad_atol(gAc[:c], xc[:c], c) * math.sqrt(D) + 1e-6, f"{name} eps slabs c={c}")
        # input gradient by source + strip statistics of the gated result over rows < c
        gx = 1.3 * gAc.double().clone()
        gx[:c].index_add_(0, s_, m)
        close(bufs["g_x"][:c], gx[:c], 1e-5, 1e-5, f"g_x c={c}")
        assert torch.isfinite(bufs["g_x"]).all()
        g1 = torch.where(xc[:c].double() > 0, gx[:c], torch.zeros_like(gx[:c]))
        z = zpc[:c].double() - mean_c.double()
        at2 = wgrad_atol(g1, z, c) + 1e-5
        close(bufs["stats"][:, 0].double().sum(0), g1.sum(0), 1e-5, at2, f"x_stats sum g' c={c}")
        close(bufs["stats"][:, 1].double().sum(0), (g1 * z).sum(0), 1e-5, at2, f"x_stats sum g'(z-m) c={c}")

    drive(dev, C, counts_std(C, zero=True), bufs, launch, check, ops, vals=lambda c: [c, cE_of(c)],
          outs=["g_tab", "g_eps", "ws_1", "ws_a", "ws_b", "g_x", "stats"])


# ------------------------------------------------------------------------------------------------ GAT tail, basis-MLP head
@pytest.mark.parametrize("C", [3588, 333])
def test_gat_tail_bwd_bounded(dev, C):
    """msde_gat_tail_bwd (GATLayer tail, equivariant_scorenetwork.py:27-38, p = 0): the LayerNorm-parameter partials ln_part
    [blocks][4D] summed over blocks against fp64 autograd over the valid rows -- blocks whose rows are all padding must be
    written (as zeros) -- and the row-wise gradients on the valid rows (finite behind the bound)."""
    lib = _lib_handle()
    D = 32
    ops = Ops(dev, C)
    x, xc = ops.add((C, D))
    res, resc = ops.add((C, D))
    go, goc = ops.add((C, D))
    g = torch.Generator().manual_seed(C)
    P = {k: (torch.randn(*sh, generator=g) * sc + sh0) for k, sh, sc, sh0 in
         (("g1", (D,), 0.3, 1.0), ("b1", (D,), 0.3, 0.0), ("W0", (D, D), D ** -0.5, 0.0), ("b0", (D,), 0.1, 0.0),
          ("W3", (D, D), D ** -0.5, 0.0), ("b3", (D,), 0.1, 0.0), ("g2", (D,), 0.3, 1.0), ("b2", (D,), 0.3, 0.0))}
    Pd = {k: v.to(dev) for k, v in P.items()}
    nblk = int(lib.msde_gat_tail_blocks(C))
    bufs = {k: torch.empty(C, D, device=dev) for k in ("out", "y1", "h0", "x2", "g_x", "g_res", "g_x2", "a", "g_h0")}
    bufs["ln_part"] = torch.empty(nblk, 4 * D, device=dev)

    def launch(b):
        _call("msde_gat_tail_fwd", _p(x), _p(res), _p(Pd["g1"]), _p(Pd["b1"]), _p(Pd["W0"]), _p(Pd["b0"]), _p(Pd["W3"]),
              _p(Pd["b3"]), _p(Pd["g2"]), _p(Pd["b2"]), C, D, 1e-5, 1e-5, 0.0, 0, _p(None), 0, _p(bufs["out"]), _p(bufs["y1"]),
              _p(bufs["h0"]), _p(bufs["x2"]), _st())
        _call("msde_gat_tail_bwd", _p(go), _p(x), _p(bufs["y1"]), _p(bufs["h0"]), _p(bufs["x2"]), _p(Pd["g1"]), _p(Pd["W0"]),
              _p(Pd["W3"]), _p(Pd["g2"]), _p(Pd["b2"]), C, D, 1e-5, 1e-5, 0.0, 0, _p(None), 0, _p(bufs["g_x"]), _p(bufs["g_res"]),
              _p(bufs["g_x2"]), _p(bufs["a"]), _p(bufs["g_h0"]), _p(bufs["ln_part"]), _p(b), _st())

    def check(c):
        F = torch.nn.functional
        pr = {k: v.double().requires_grad_(True) for k, v in P.items()}
        xr, rr = xc[:c].double().requires_grad_(True), resc[:c].double().requires_grad_(True)
        y1 = rr + F.layer_norm(xr, (D,), pr["g1"], pr["b1"], 1e-5)
        out = y1 + F.layer_norm(F.silu(y1 @ pr["W0"].t() + pr["b0"]) @ pr["W3"].t() + pr["b3"], (D,), pr["g2"], pr["b2"], 1e-5)
        out.backward(goc[:c].double())
        ln = bufs["ln_part"].double().sum(0).cpu()
        for k, (lo, nm) in enumerate(((0, "g2"), (D, "b2"), (2 * D, "g1"), (3 * D, "b1"))):
            ref = pr[nm].grad
            close(ln[lo:lo + D], ref, 1e-4, 4e-6 * math.sqrt(c) * 4 * float(goc[:c].abs().max()) + 1e-6, f"ln_part {nm} c={c}")
        close(bufs["g_x"][:c], xr.grad, 2e-4, 2e-5 * float(xr.grad.abs().max()) + 1e-6, f"g_x c={c}")
        close(bufs["g_res"][:c], rr.grad, 2e-4, 2e-5 * float(rr.grad.abs().max()) + 1e-6, f"g_res c={c}")
        for k in bufs:
            assert torch.isfinite(bufs[k]).all(), f"{k} c={c}: non-finite (padded rows must be finite)"

    drive(dev, C, counts_std(C), bufs, launch, check, ops)


@pytest.mark.parametrize("C,Nn", [(35186, 3588), (777, 100)])
def test_mlp_head_mix_bwd_bounded(dev, C, Nn):
    """msde_mlp_head_mix_bwd (basis-MLP head fused with the frame mix + mean, equivariant_scorenetwork.py:142-166): gZ on the
    valid edges (zero behind the bound) and the head's [gW | gb] summed from its workgroup slabs, against fp64; padded edge
    slots have dst = -1 and lie outside the by-target CSR."""
    lib = _lib_handle()
    H = 128
    ops = Ops(dev, C + Nn)
    Z, Zc = ops.add((C, H))
    basis, basisc = ops.add((C, 9))
    g = torch.Generator().manual_seed(C)
    W2c, gnode_c = torch.randn(3, H, generator=g) / H ** 0.5, torch.randn(Nn, 3, generator=g)
    W2, gnode = W2c.to(dev), gnode_c.to(dev)
    dst = torch.empty(C, dtype=torch.int32, device=dev)
    rowptr = torch.empty(Nn + 1, dtype=torch.int32, device=dev)
    dsts = {}
    prep0 = ops.prep

    def prep(c):
        prep0(c)
        d_ = torch.full((C,), -1, dtype=torch.int64)
        d_[:c] = torch.sort(torch.randint(0, Nn, (c,), generator=torch.Generator().manual_seed(c)))[0]
        dsts[c] = d_[:c]
        dst.copy_(d_.to(torch.int32)), rowptr.copy_(torch.searchsorted(d_[:c], torch.arange(Nn + 1)).to(torch.int32))
    ops.prep = prep
    nsl = int(lib.msde_mlp_head_bwd_slabs(C, H))
    wl = (3 * H + 3 + 3) & ~3
    bufs = {"gZ": torch.empty(C, H, device=dev), "ws": torch.empty(nsl * wl, device=dev)}

    def launch(b):
        _call("msde_mlp_head_mix_bwd", _p(Z), H, _p(W2), _p(gnode), _p(basis), _p(dst), _p(rowptr), C, H, _p(bufs["gZ"]),
              _p(bufs["ws"]), _p(b), _st())

    def check(c):
        d_ = dsts[c]
        deg = torch.zeros(Nn, dtype=torch.float64).index_add_(0, d_, torch.ones(c, dtype=torch.float64)).clamp(min=1)
        gcoff = (basisc[:c].double().view(c, 3, 3) * (gnode_c.double()[d_] / deg[d_, None])[:, None, :]).sum(2)
        z = Zc[:c].double()
        sg = torch.sigmoid(z)
        silu, dsilu = z * sg, sg * (1 + z * (1 - sg))
        close(bufs["gZ"][:c], (gcoff @ W2c.double()) * dsilu, 1e-4, 1e-6, f"gZ c={c}")
        zero_rows(bufs["gZ"], c, "gZ")
        assert torch.isfinite(bufs["ws"]).all(), f"c={c}: a head slab was not written"
        tot = bufs["ws"].view(nsl, wl).double().sum(0).cpu()
        at = wgrad_atol(gcoff, silu, c) + 1e-6
        close(tot[:3 * H].view(3, H), gcoff.t() @ silu, 1e-5, at, f"gW2 c={c}")
        close(tot[3 * H:3 * H + 3], gcoff.sum(0), 1e-5, wgrad_atol(gcoff, torch.ones(1), c) + 1e-6, f"gb2 c={c}")

    drive(dev, C, counts_std(C), bufs, launch, check, ops)


@pytest.mark.parametrize("B", [256, 7])
def test_dense_loss_nmax_bounded(dev, B):
    """msde_dense_loss_fwd / _bwd with the device-side N_max (reduce_mean scales 1 / (B N_max ncls), 1 / (B N_max^2)) swept
    over N_max, captured once and replayed at several values: equal to the host-scale call with those scales (to fp32 rounding
    of the scale) -- nothing is taken from the capture-time value; part / residual / gradient buffers NaN-filled."""
    ncls, F2, XL = 119, 60, 120
    g = torch.Generator().manual_seed(B)
    n = torch.randint(2, 21, (B,), generator=g)
    n[0] = 20
    N, P = int(n.sum()), int((n * n).sum())
    mol_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)]).to(torch.int32).to(dev)
    pair_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), (n * n).cumsum(0)]).to(torch.int32).to(dev)
    ops = Ops(dev, B)
    G2, Z2 = torch.randn(P, F2, generator=g).to(dev), torch.randn(P, F2, generator=g).to(dev)
    w2, b2 = (torch.randn(F2, generator=g) / 8).to(dev), torch.randn(1, generator=g).to(dev)
    OUT, z_x = torch.randn(N, XL, generator=g).to(dev), torch.randn(N, XL, generator=g).to(dev)
    z_adj, flags = torch.randn(P, generator=g).to(dev), torch.ones(N, device=dev)
    ms = torch.stack([torch.rand(B, generator=g), torch.rand(B, generator=g) + 0.5], 1).to(dev)
    gl = torch.tensor([1.3, 0.7], device=dev)
    part_n = B * 4 * 2

    def mk():
        return {"res_adj": torch.empty(P, device=dev), "res_x": torch.empty(N, XL, device=dev), "part": torch.empty(part_n, device=dev),
                "out": torch.empty(2, device=dev), "gS": torch.empty(P, device=dev), "gZ2": torch.empty(P, F2, device=dev),
                "gOUT": torch.empty(N, XL, device=dev)}
    bufs, host = mk(), mk()

    def call(o, nm, sx, sa):
        _call("msde_dense_loss_fwd", _p(G2), F2, _p(w2), _p(b2), _p(OUT), _p(z_adj), _p(z_x), _p(flags), _p(ms), _p(mol_ptr),
              _p(pair_ptr), B, ncls, 0.0, sx, sa, _p(nm), _p(o["res_adj"]), _p(o["res_x"]), _p(o["part"]), _p(o["out"]), _st())
        _call("msde_dense_loss_bwd", _p(gl[0:1]), _p(gl[1:2]), _p(o["res_adj"]), _p(o["res_x"]), _p(Z2), F2, _p(w2), _p(flags),
              _p(ms), _p(mol_ptr), _p(pair_ptr), B, ncls, 0.0, sx, sa, _p(nm), _p(o["gS"]), _p(o["gZ2"]), _p(o["gOUT"]), _st())

    def launch(b):
        if b is None:                      # the host-scale call at N_max = 32 (the capacity of this sweep)
            call(bufs, None, 1.0 / (B * 32 * ncls), 1.0 / (B * 32 * 32))
        else:
            call(bufs, b, 123.0, 456.0)    # scales from the device N_max override these

    def check(nm):
        for t in host.values():
            t.fill_(NAN)
        call(host, None, 1.0 / (B * nm * ncls), 1.0 / (B * nm * nm))
        torch.cuda.synchronize()
        for k in bufs:
            got, ref = bufs[k], host[k]
            if k in ("res_x", "gOUT"):          # [N, 120] rows: the pad column behind the 119 classes is not part of the result
                got, ref = got[:, :ncls], ref[:, :ncls]
            assert torch.isfinite(got).all(), f"{k} N_max={nm}: not written"
            close(got, ref.double().cpu(), 2e-6, 1e-12, f"{k} N_max={nm}")

    drive(dev, 32, [1, 20, 25, 32], bufs, launch, check, ops, outs=list(bufs))
