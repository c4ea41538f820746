"""Graphs, inputs, references and tolerances of the CFConv size tests (tests/test_cfconv_sizes_host.py on the host,
tests/test_gpu_cfconv_sizes.py on the device).

Two batches of helpers.build_batch: "pair" (helpers.CFCONV_PAIR_SPECS, molecules of 1 to 33 atoms: the radius graph is symmetric,
in-degrees 0, 1, 2, 19, 20, 30, 31 and 32, degree-32 targets that fill a 32-edge chunk exactly and ones that straddle two) and
"cap" (helpers.CFCONV_CAP_SPECS, molecules of up to 65 atoms: the 32-neighbour cap binds, the graph is asymmetric, by-source rows
reach 64 edges).  The graph is always the oracle's (oracle.restate.radius_graph); the device radius kernels are not in the loop.

The CFConv interior (schnet.py:141-145,185-195: distance, smearing, Linear(G, 128), shifted softplus, Linear(128, 128), times
the cosine cutoff, gather, scatter-sum by target) is written once with the oracle's modules and evaluated twice on the CPU from
the same fp32 inputs (positions, x1, filter-network parameters, output weights w): in fp64 (the reference) and in fp32 (the
yardstick: what an honest fp32 evaluation loses).  A kernel result passes when its error is at most TOL_FACTOR times the
yardstick of that quantity -- per molecule for per-atom quantities, per edge / pair row for the filter rows, whole tensor for
the weight gradients (see row_tolerance); the filter rows alone get one derived additive term for the hardware cosine of the
cutoff factor (see cutoff_hardware_term).  Nothing here is taken from a kernel's result."""
import functools
import math
import types

import torch

import helpers as H_

TOL_FACTOR = 8.0
F = 128
# in-degree classes of the report (targets of a chunk that is one target, of a straddling target, ...); "other" takes the
# degrees in between (cutoff 4.0: 7..30; cap batch: 6)
DEG_CLASSES = (("deg 0", 0, 0), ("deg 1-2", 1, 2), ("deg 19-21", 19, 21), ("deg 30-31", 30, 31), ("deg 32", 32, 32))
OUT_DEG_CLASSES = (("out-deg 0", 0, 0), ("out-deg 1-32", 1, 32), ("out-deg 33-64", 33, 64))
FIXTURES = {"pair": (H_.CFCONV_PAIR_SPECS, H_.CFCONV_PAIR_SEED), "cap": (H_.CFCONV_CAP_SPECS, H_.CFCONV_CAP_SEED)}


@functools.lru_cache(maxsize=None)
def batch(name, last=None):
    """The host batch; last: a spec that replaces the batch's last molecule (the path-switch test)."""
    specs, seed = FIXTURES[name]
    return H_.build_batch(specs if last is None else specs[:-1] + [last], seed=seed)


@functools.lru_cache(maxsize=None)
def graph(name, cutoff):
    """Host view of a fixture at a cutoff: the oracle's radius graph (by target, sources in index order, at most 32), the fp32
    distances of its edges, in- / out-degrees, molecule sizes."""
    from oracle import restate as R
    b = batch(name)
    pos = b.positions.float()
    N = int(pos.size(0))
    ei = R.radius_graph(pos, cutoff, b.batch, 32)
    g = types.SimpleNamespace(name=name, cutoff=cutoff, batch=b, pos=pos, N=N, E=int(ei.size(1)), src=ei[0], dst=ei[1])
    g.sizes = torch.bincount(b.batch, minlength=b.num_graphs).tolist()
    g.mol_ptr = [0]
    for n in g.sizes:
        g.mol_ptr.append(g.mol_ptr[-1] + n)
    g.pairs = sum(n * (n - 1) // 2 for n in g.sizes)                   # unordered atom pairs (the pair form's list)
    g.deg = torch.bincount(g.dst, minlength=N)
    g.out_deg = torch.bincount(g.src, minlength=N)
    g.rowptr = torch.cat([torch.zeros(1, dtype=torch.long), g.deg.cumsum(0)])
    g.dist = (pos[g.src] - pos[g.dst]).norm(dim=-1)                    # fp32: the per-edge kernels' distance input
    key = set(zip(g.src.tolist(), g.dst.tolist()))
    g.unreversed = sum((t, s) not in key for s, t in key)
    return g


def device_plan(g, dev, spare=0):
    """A fresh CSR plan of the oracle's edge list on the device (hip.build_csr: by target, stable, + the by-source view);
    spare > 0: capacity for `spare` more edges, padded the way the radius plans are (src = dst = -1 past rowptr[N])."""
    from moleculesde_amd import hip
    pl = hip.build_csr(torch.stack([g.src, g.dst]), g.N)
    assert torch.equal(pl.src.long(), g.src) and torch.equal(pl.dst.long(), g.dst)      # already in canonical order
    if spare:
        pad = torch.full((spare,), -1, dtype=torch.int32)
        pl.src, pl.dst = torch.cat([pl.src, pad]), torch.cat([pl.dst, pad])
        pl.E += spare
    return pl.to(dev)


def pair_index(g):
    """Host enumeration of the unordered pairs: (pi, pj, edge) with pair p of molecule m, local atoms a < b, at
    pair_ptr[m] + a n - a (a + 1) / 2 + (b - a - 1); edge = the oracle's edge j -> i (source j, target i) or -1 beyond the
    cutoff.  Only meaningful on a symmetric graph."""
    key = {(s, t): e for e, (s, t) in enumerate(zip(g.src.tolist(), g.dst.tolist()))}
    pi, pj, edge, base = [], [], [], 0
    for m, n in enumerate(g.sizes):
        a0 = g.mol_ptr[m]
        for a in range(n):
            for b in range(a + 1, n):
                assert len(pi) == base + a * n - a * (a + 1) // 2 + (b - a - 1)
                pi.append(a0 + a)
                pj.append(a0 + b)
                e = key.get((a0 + b, a0 + a), -1)
                assert (e < 0) == ((a0 + a, a0 + b) not in key)
                edge.append(e)
        base += n * (n - 1) // 2
    return torch.tensor(pi), torch.tensor(pj), torch.tensor(edge)


# ------------------------------------------------------------------------------------------------ reference + yardstick ---
NAMES = ("Wf", "out", "g_x1", "gW1", "gb1", "gW2", "gb2")


def _interior(g, blk, gs, x1, w, dtype, src=None, dst=None):
    """The CFConv interior in `dtype` from the fp32 inputs; loss = (out * w).sum().  fp64: the distance is the exact one of the
    fp32 positions; fp32: the rounded one the kernels are given (g.dist) or compute."""
    from oracle import restate as R
    src, dst = (g.src, g.dst) if src is None else (src, dst)
    pos = g.pos.to(dtype)
    d = (pos[src] - pos[dst]).norm(dim=-1)
    C = 0.5 * (torch.cos(d * math.pi / g.cutoff) + 1.0)
    Wf = blk.mlp(gs(d)) * C.view(-1, 1)
    x = x1.detach().to(dtype).clone().requires_grad_(True)
    out = R.scatter_sum(x[src] * Wf, dst, g.N)
    blk.zero_grad(set_to_none=True)
    (out * w.to(dtype)).sum().backward()
    res = {"Wf": Wf, "out": out, "g_x1": x.grad, "gW1": blk.mlp[0].weight.grad, "gb1": blk.mlp[0].bias.grad,
           "gW2": blk.mlp[2].weight.grad, "gb2": blk.mlp[2].bias.grad}
    return {k: v.detach().double().clone() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def case(name, cutoff, G=51):
    """Inputs (fp32), the fp64 reference `ref`, the fp32 CPU run `low` and the worst fp32 error per quantity `yard` (absolute) of
    the CFConv interior on fixture `name`.  Parameters from helpers.fill_like_generator (nonzero biases)."""
    from oracle import restate as R
    g = graph(name, cutoff)
    seed = 100 * G + (7 if name == "pair" else 9) + int(cutoff)
    gen = torch.Generator().manual_seed(seed)
    x1, w = torch.randn(g.N, F, generator=gen), torch.randn(g.N, F, generator=gen)
    blk = R.InteractionBlock(hidden_channels=64, num_gaussians=G, num_filters=F, cutoff=cutoff)
    H_.fill_like_generator(blk, 3000 + seed)
    gs = R.GaussianSmearing(0.0, cutoff, G)
    params = [p.detach().clone() for p in (blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[2].weight, blk.mlp[2].bias)]
    low = _interior(g, blk, gs, x1, w, torch.float32)
    blk64, gs64 = blk.double(), gs.double()
    ref = _interior(g, blk64, gs64, x1, w, torch.float64)
    c = types.SimpleNamespace(g=g, G=G, cutoff=cutoff, x1=x1, w=w, params=params, offset=gs.offset.float().clone(), coeff=gs.coeff,
                              ref=ref, low=low, blk64=blk64, gs64=gs64)
    c.yard = {k: float((low[k] - ref[k]).abs().max()) for k in NAMES}
    c.scale = {k: float(ref[k].abs().max()) for k in NAMES}
    return c


def symmetrised_g_x1(c):
    """fp64 g_x1 of the same interior on the symmetrised graph (every edge together with its reverse): what a kernel that
    assumed a symmetric radius graph would return on the cap fixture."""
    g = c.g
    key = sorted(set(zip(g.src.tolist(), g.dst.tolist())) | set(zip(g.dst.tolist(), g.src.tolist())), key=lambda p: (p[1], p[0]))
    src, dst = torch.tensor([p[0] for p in key]), torch.tensor([p[1] for p in key])
    return _interior(g, c.blk64, c.gs64, c.x1, c.w, torch.float64, src, dst)["g_x1"]


# The forward kernels take the cosine of the cutoff factor C = (cos(pi d / cutoff) + 1) / 2 from the hardware (__cosf) and their
# softplus from the hardware exp2 / log; the figure stated for these is an absolute error of about 1e-7 (comment of ssp_fast in
# csrc/cfconv_fused.hip).  The fp32 CPU run has no such term: where C is small (d close to the cutoff, cos flat at -1) it gets C
# to within 3e-8 and a filter row (W2 h + b2) C to within a few 1e-8 of the row's own small scale.  The kernel's row is instead
# off by up to |W2 h + b2| * delta_C with delta_C = EPS_HW / 2 -- an absolute, not a relative, error of C.  So the per-row bar
# of the filter rows gets that one term, evaluated in fp64 on the fixture, on top of TOL_FACTOR x the yardstick:
#     hw[e] = max_c |(W2 h_e + b2)_c| * EPS_HW / 2
# (at most 2e-7 on these fixtures, against 2.7e-6 for a row of full scale; it matters for the pairs within 0.1 of a cutoff of
# 4).  exp2 / log needed no room (every other quantity passes at 8 x the yardstick alone), so no term is added for them, and
# none to the per-molecule outputs, where a single small row no longer shows.
EPS_HW = 1e-7


def cutoff_hardware_term(c):
    """hw [E] per edge of the oracle's list (see above)."""
    g = c.g
    pos = g.pos.double()
    d = (pos[g.src] - pos[g.dst]).norm(dim=-1)
    with torch.no_grad():
        pre = c.blk64.mlp(c.gs64(d))
    return pre.abs().max(dim=1)[0] * (0.5 * EPS_HW)


def pair_rows(c, name="Wf"):
    """ref / low filter rows in pair order (zero rows beyond the cutoff) and the pair -> edge map."""
    pi, pj, edge = pair_index(c.g)
    out = []
    for t in (c.ref[name], c.low[name]):
        rows = torch.zeros(edge.numel(), F, dtype=torch.float64)
        rows[edge >= 0] = t[edge[edge >= 0]]
        out.append(rows)
    return out[0], out[1], edge


# ---------------------------------------------------------------------------------------------- decomposed form's inputs ---
@functools.lru_cache(maxsize=None)
def aggregate_case(name, cutoff=10.0, G=51):
    """hip.rbf_cutoff + hip.cfconv_aggregate: smearing rows, cutoff factors, and out_i = sum_j x1_j (Wf_ij C_ij) with its
    gradients of x1 and Wf, for a given fp32 Wf [E, 128] (pre-cutoff filter rows: any fp32 tensor).  ref / low / yard as
    in case()."""
    from oracle import restate as R
    g = graph(name, cutoff)
    gen = torch.Generator().manual_seed(77 + len(name))
    x1, w = torch.randn(g.N, F, generator=gen), torch.randn(g.N, F, generator=gen)
    Wf = torch.randn(g.E, F, generator=gen) * 0.5
    gs = R.GaussianSmearing(0.0, cutoff, G)
    offset, coeff = gs.offset.clone(), gs.coeff

    def run(dtype):
        gs_ = R.GaussianSmearing(0.0, cutoff, G).to(dtype)
        pos = g.pos.to(dtype)
        d = (pos[g.src] - pos[g.dst]).norm(dim=-1)
        C = 0.5 * (torch.cos(d * math.pi / cutoff) + 1.0)
        x, W = x1.detach().to(dtype).clone().requires_grad_(True), Wf.detach().to(dtype).clone().requires_grad_(True)
        out = R.scatter_sum(x[g.src] * (W * C.view(-1, 1)), g.dst, g.N)
        (out * w.to(dtype)).sum().backward()
        res = {"rbf": gs_(d), "C": C.view(-1, 1), "out": out, "g_x1": x.grad, "g_Wf": W.grad}
        return {k: v.detach().double().clone() for k, v in res.items()}
    low = run(torch.float32)
    ref = run(torch.float64)
    c = types.SimpleNamespace(g=g, G=G, cutoff=cutoff, x1=x1, w=w, Wf=Wf, offset=offset, coeff=coeff, ref=ref, low=low)
    c.yard = {k: float((low[k] - ref[k]).abs().max()) for k in ref}
    c.scale = {k: float(ref[k].abs().max()) for k in ref}
    return c


# ------------------------------------------------------------------------------------------- whole SchNet (path switch) ---
SCHNET_KW = dict(hidden_channels=64, num_filters=F, num_interactions=2, num_gaussians=51, cutoff=10.0, readout="mean",
                 node_class=119)
SWITCH_SPEC = (34, "hub")          # replaces the pair batch's last (1-atom) molecule: N_max 33 -> 34


@functools.lru_cache(maxsize=None)
def schnet_case(switch):
    """R.SchNet (2 interactions, hidden 64, 128 filters, 51 Gaussians, cutoff 10, parameters from fill_like_generator) on the
    pair batch (switch False: N_max 33) or on the pair batch with its last molecule replaced by 34 atoms (switch True), in
    fp64 and fp32: readout, latent and every parameter gradient of loss = (out * w_out).sum() + (h * w_h).sum()."""
    import copy
    from oracle import restate as R
    b = batch("pair", SWITCH_SPEC if switch else None)
    o = R.SchNet(**SCHNET_KW)
    H_.fill_like_generator(o, 8100)
    z, N, B = b.x[:, 0].long(), int(b.x.size(0)), int(b.num_graphs)
    gen = torch.Generator().manual_seed(8200 + int(switch))
    w_out, w_h = torch.randn(B, 64, generator=gen), torch.randn(N, 64, generator=gen)

    def run(dtype):
        m = copy.deepcopy(o).to(dtype)
        out, h = m(z, b.positions.to(dtype), b.batch, return_latent=True)
        ((out * w_out.to(dtype)).sum() + (h * w_h.to(dtype)).sum()).backward()
        res = {"out": out, "h": h}
        res.update({"grad " + k: p.grad for k, p in m.named_parameters()})
        return {k: v.detach().double().clone() for k, v in res.items()}
    low, ref = run(torch.float32), run(torch.float64)
    sizes = torch.bincount(b.batch, minlength=B).tolist()
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    c = types.SimpleNamespace(batch=b, state={k: v.clone() for k, v in o.state_dict().items()}, w_out=w_out, w_h=w_h, ref=ref,
                              low=low, sizes=sizes, mol_ptr=ptr)
    c.yard = {k: float((low[k] - ref[k]).abs().max()) for k in ref}
    c.scale = {k: float(ref[k].abs().max()) for k in ref}
    return c


def param_tolerances(c):
    """Tolerance of every parameter gradient of schnet_case: TOL_FACTOR x its own worst fp32 error, floored by the worst
    relative fp32 error over all parameters applied to its own scale (the rule of row_tolerance, a parameter as the group)."""
    names = [k for k in c.ref if k.startswith("grad ")]
    rel = max(c.yard[k] / c.scale[k] for k in names if c.scale[k] > 0)
    return {k: TOL_FACTOR * max(c.yard[k], rel * c.scale[k]) for k in names}


# ------------------------------------------------------------------------------------------------------------ comparison ---
def row_tolerance(ref, low, groups):
    """Tolerance per group of rows (a molecule's atoms; a single edge / pair row): TOL_FACTOR x the group's own worst fp32
    error, floored by the batch's worst fp32 error taken relative to the batch's scale and applied to the group's scale -- a
    group whose fp32 run happened to round well is still allowed the batch's relative error, but never another group's
    absolute scale.  A group whose reference is all zero (an atom without neighbours, a pair beyond the cutoff) gets 0: exact.
    groups: [(lo, hi)] row ranges.  Returns a tensor [len(groups)]."""
    err = (low - ref).abs()
    scale = float(ref.abs().max())
    rel = float(err.max()) / scale if scale > 0 else 0.0
    tol = torch.zeros(len(groups), dtype=torch.float64)
    for k, (lo, hi) in enumerate(groups):
        if hi > lo:
            tol[k] = TOL_FACTOR * max(float(err[lo:hi].max()), rel * float(ref[lo:hi].abs().max()))
    return tol


def mol_groups(g):
    return [(g.mol_ptr[m], g.mol_ptr[m + 1]) for m in range(len(g.sizes))]


def rows_tolerance(ref, low, groups=None):
    """Per-ROW tolerance [rows] of a 2-D quantity: row_tolerance of the row's group (groups None: every row its own group)."""
    R_ = ref.size(0)
    if groups is None:
        err = (low - ref).abs()
        scale = float(ref.abs().max())
        rel = float(err.max()) / scale if scale > 0 else 0.0
        return TOL_FACTOR * torch.maximum(err.max(dim=1)[0], rel * ref.abs().max(dim=1)[0]) if R_ else torch.zeros(0, dtype=torch.float64)
    tg = row_tolerance(ref, low, groups)
    tol = torch.zeros(R_, dtype=torch.float64)
    for k, (lo, hi) in enumerate(groups):
        tol[lo:hi] = tg[k]
    return tol


def row_ratios(got, ref, tol_rows):
    """error / tolerance per row [rows]; 0 where both are 0, inf where the error exceeds a zero tolerance or is not finite."""
    got = torch.as_tensor(got).detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf)).max(dim=1)[0]
    ratio = err / tol_rows
    ratio[(err == 0) & (tol_rows == 0)] = 0.0
    return ratio, err


def class_worst(values, row_deg, classes=DEG_CLASSES):
    """[(class, worst value over the rows whose degree is in the class or None)] + ("other", ...) for rows in no class."""
    out, seen = [], torch.zeros_like(row_deg, dtype=torch.bool)
    for cname, lo, hi in classes:
        rows = (row_deg >= lo) & (row_deg <= hi)
        seen |= rows
        out.append((cname, float(values[rows].max()) if bool(rows.any()) else None))
    if bool((~seen).any()):
        out.append(("other", float(values[~seen].max())))
    return out


def _fmt(pairs, f="{:.2f}"):
    return ", ".join(f"{n} {'-' if v is None else f.format(v)}" for n, v in pairs)


def compare_rows(tag, name, got, ref, low, row_deg, failures, groups=None, classes=DEG_CLASSES, extra_tol=None):
    """One per-row quantity (per-atom: groups = molecules; filter rows: groups None): record the worst error / tolerance
    per degree class, add what exceeds 1 to `failures`.  extra_tol [rows]: a derived additive term (see hardware_term)."""
    tol = rows_tolerance(ref, low, groups)
    if extra_tol is not None:
        tol = tol + extra_tol
    ratio, err = row_ratios(got, ref, tol)
    per = class_worst(ratio, row_deg, classes)
    if extra_tol is not None:       # for the record: the same without the derived term, and the error of C that would explain
        rb = row_ratios(got, ref, tol - extra_tol)[0]                                      # the rows that need the term on their own
        need = (rb > 1.0) & (extra_tol > 0)
        implied = float((err[need] / (extra_tol[need] / (0.5 * EPS_HW))).max()) if bool(need.any()) else 0.0
        H_.record_parity(f"cfconv_sizes {tag} {name}: without the cutoff-factor term err / tol by class: {_fmt(class_worst(rb, row_deg, classes))}; "
                         f"{int(need.sum())} rows need it, their worst error / max |W2 h + b2| = {implied:.2e} (the term allows {0.5 * EPS_HW:.1e})")
    H_.record_parity(f"cfconv_sizes {tag} {name}: scale {float(ref.abs().max()):.2e} fp32-cpu err {float((low - ref).abs().max()):.2e} "
                     f"achieved err {float(err.max()) if err.numel() else 0.0:.2e}; err / tol by class: {_fmt(per)}")
    failures += [f"{tag} {name} {n}: err / tol {v:.3f}" for n, v in per if v is not None and not v <= 1.0]
    return max([v for _, v in per if v is not None], default=0.0)


def compare_whole(tag, name, got, ref, yard, failures):
    """A weight gradient: whole tensor against TOL_FACTOR x the fp32 run's worst error."""
    got = torch.as_tensor(got).detach().double().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
    ratio = err / (TOL_FACTOR * yard)
    H_.record_parity(f"cfconv_sizes {tag} {name}: scale {float(ref.abs().max()):.2e} fp32-cpu err {yard:.2e} achieved err {err:.2e}; "
                     f"err / tol all {ratio:.2f}")
    if not ratio <= 1.0:
        failures.append(f"{tag} {name}: err / tol {ratio:.3f}")
    return ratio
