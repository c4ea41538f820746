"""Host-side pins of the CFConv size tests (tests/cfconv_cases.py, tests/test_gpu_cfconv_sizes.py): the two batches have the
node / edge counts, in- and out-degrees and chunk offsets the device tests rely on, the fp32-vs-fp64 error budget of every
quantity is nonzero and small, the asymmetric reference differs from a symmetrised one by far more than its tolerance, and
hip.pair_plan refuses molecules the pair form cannot hold.  No GPU."""
import ctypes
import types

import pytest
import torch

import cfconv_cases as CC
import helpers as H


def _chunk_offsets(g, degree):
    return sorted(set((g.rowptr[:-1][g.deg == degree] % 32).tolist()))


def test_pair_fixture_properties():
    g = CC.graph("pair", 10.0)
    assert g.sizes == [s[0] for s in H.CFCONV_PAIR_SPECS] and max(g.sizes) == 33 and g.N == 177
    ordered_pairs = sum(n * (n - 1) for n in g.sizes)
    assert g.E == 4842 == ordered_pairs, "cutoff 10: every ordered pair is an edge"
    assert g.unreversed == 0, "symmetric"
    assert sorted(set(g.deg.tolist())) == [0, 1, 2, 19, 20, 30, 31, 32]
    assert torch.equal(g.deg, g.out_deg)
    # a degree-32 target at offset 0 fills one 32-edge chunk alone (first == last target of the chunk); one at offset 2
    # straddles two chunks
    assert _chunk_offsets(g, 32) == [0, 2]
    assert g.E % 64 == 42 and (ordered_pairs // 2) % 32 == 21
    # the last, partial chunk (E % 32 = 10 edges) is ONE target whose first edges lie in the chunk before: the place where a
    # single-target chunk needs the forward's atomic combination (a full chunk of one degree-32 target has no partial target)
    tail, last = g.E - g.E % 32, int(g.dst[-1])
    assert int(g.dst[tail]) == last and int(g.rowptr[last]) < tail and int(g.deg[last]) == 19
    assert int(g.deg[0]) == 0 and int(g.deg[-1]) == 0, "first and last atom without edges"
    assert float(g.dist.max()) < 10.0

    g4 = CC.graph("pair", 4.0)
    assert g4.E == 2754 < ordered_pairs and g4.unreversed == 0
    deg = [d for m, n in enumerate(g4.sizes) if n > 3 for d in g4.deg[g4.mol_ptr[m]:g4.mol_ptr[m + 1]].tolist()]
    assert min(deg) == 7 and max(deg) == 30, "in-degrees of the larger molecules at cutoff 4"
    pi, pj, edge = CC.pair_index(g4)
    assert int((edge < 0).sum()) == (ordered_pairs - g4.E) // 2 > 0


def test_cap_fixture_properties():
    g = CC.graph("cap", 10.0)
    assert g.sizes == [s[0] for s in H.CFCONV_CAP_SPECS] and max(g.sizes) == 65 and g.N == 180
    assert g.E == 5546
    assert sorted(set(g.deg.tolist())) == [0, 6, 32]
    assert int(g.out_deg.min()) == 0 and int(g.out_deg.max()) == 64
    assert any(33 <= d <= 64 for d in g.out_deg.tolist()) and any(1 <= d <= 32 for d in g.out_deg.tolist())
    assert g.unreversed == 1280, "edges whose reverse the 32-neighbour cap dropped"
    assert g.E % 32 == 10 and g.E % 64 == 42
    assert _chunk_offsets(g, 32) == [0]
    from moleculesde_amd import hip
    assert max(g.sizes) > hip.RADIUS_TRANSPOSE_MOL_NMAX, "the one-launch transposition does not apply to this batch"


def test_path_switch_batch():
    """The path-switch test's second batch: the pair batch with its last molecule replaced by 34 atoms (N_max 33 -> 34)."""
    b = CC.batch("pair", (34, "hub"))
    sizes = torch.bincount(b.batch).tolist()
    assert sizes == [s[0] for s in H.CFCONV_PAIR_SPECS[:-1]] + [34]
    from oracle import restate as R
    ei = R.radius_graph(b.positions, 10.0, b.batch, 32)
    key = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert ei.size(1) == sum(n * min(n - 1, 32) for n in sizes), "every pair within the cutoff; the cap drops 34 edges"
    assert sum((t, s) not in key for s, t in key) > 0, "34 atoms: the radius graph is no longer symmetric"


@pytest.mark.parametrize("name,cutoff,G", [("pair", 10.0, 51), ("pair", 4.0, 51), ("pair", 10.0, 50), ("pair", 10.0, 20),
                                           ("cap", 10.0, 51), ("cap", 10.0, 50), ("cap", 10.0, 20)])
def test_error_budget(name, cutoff, G):
    """The fp32 CPU run is a usable yardstick: its worst error against fp64 is nonzero and below 1e-4 of the quantity's
    scale, for every quantity the device tests compare."""
    c = CC.case(name, cutoff, G)
    for k in CC.NAMES:
        assert c.scale[k] > 0 and 0 < c.yard[k] < 1e-4 * c.scale[k], (k, c.yard[k], c.scale[k])
    g = c.g
    # atoms without neighbours / pairs beyond the cutoff: reference exactly zero, tolerance exactly zero
    tol = CC.rows_tolerance(c.ref["out"], c.low["out"], CC.mol_groups(g))
    lone = [g.mol_ptr[m] for m, n in enumerate(g.sizes) if n == 1]
    assert lone and all(float(tol[i]) == 0 and float(c.ref["out"][i].abs().max()) == 0 for i in lone)
    assert float(tol.max()) <= CC.TOL_FACTOR * c.yard["out"] * (1 + 1e-12)       # no molecule is allowed more than the batch
    assert all(float(tol[g.mol_ptr[m]]) > 0 for m, n in enumerate(g.sizes) if n > 1)
    rt = CC.rows_tolerance(c.ref["Wf"], c.low["Wf"])
    assert rt.numel() == g.E and float(rt.min()) > 0 and float(rt.max()) <= CC.TOL_FACTOR * c.yard["Wf"] * (1 + 1e-12)


def test_asymmetric_reference_differs_from_symmetrised():
    """On the cap batch the gradient of x1 gathers over by-source rows that are NOT the by-target rows: a kernel that took
    the graph for symmetric (the pair form's assumption) is off by orders of magnitude more than the tolerance."""
    c = CC.case("cap", 10.0, 51)
    diff = (CC.symmetrised_g_x1(c) - c.ref["g_x1"]).abs().max(dim=1)[0]
    tol = CC.rows_tolerance(c.ref["g_x1"], c.low["g_x1"], CC.mol_groups(c.g))
    assert float(diff.max()) > 1e4 * float(tol.max())
    # the atoms that differ are the late ones of a large molecule: sources the cap dropped from their neighbours' lists
    g = c.g
    key = set(zip(g.src.tolist(), g.dst.tolist()))
    gains = torch.zeros(g.N, dtype=torch.bool)
    gains[[t for s, t in key if (t, s) not in key]] = True
    assert 0 < int(gains.sum()) < g.N and float(diff[gains].min()) > 1e3 * float(tol.max())
    assert float(diff[~gains].max()) < 1e-12 and bool((g.out_deg[~gains] > 32).any())     # (same edges, another order of the sum)
    # the symmetric batch: the two agree exactly (same edge set)
    cs = CC.case("pair", 10.0, 51)
    assert float((CC.symmetrised_g_x1(cs) - cs.ref["g_x1"]).abs().max()) < 1e-12


def test_pair_plan_refuses_more_than_33_atoms():
    """hip.pair_plan: the pair kernels index a molecule's pairs assuming the 32-neighbour cap cannot bind; a plan that knows
    N_max > 33 is refused on the host, before any launch (no device needed to see it)."""
    from moleculesde_amd import hip
    pl = types.SimpleNamespace(N_max=34, B=1, P2_cap=34 * 33 // 2, mol_ptr=torch.tensor([0, 34], dtype=torch.int32),
                               batch_i32=torch.zeros(34, dtype=torch.int32))
    assert hip.PAIR_NMAX == 33
    with pytest.raises(ValueError, match="33"):
        hip.pair_plan(torch.zeros(34, 3), pl, 10.0)


def test_entry_points_refuse_null_arguments():
    """The C entry points under the CFConv size tests return MSDE_EINVAL for a missing operand before anything is launched
    (msde_radius_fill checked only rowptr; the others are pinned as they are)."""
    from moleculesde_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fill = lambda pos, src, dist: lib.msde_radius_fill(pos, p, p, 1, 100.0, 32, p, src, p, dist, 1, None)      # noqa: E731
    assert fill(None, p, p) == EINVAL and fill(p, None, p) == EINVAL and fill(p, p, None) == EINVAL
    assert lib.msde_radius_fill(p, p, p, 1, 100.0, 32, None, p, p, p, 1, None) == EINVAL
    fwd = lambda dst, agg: lib.msde_cfconv_fused_fwd(p, p, p, p, dst, p, p, p, p, p, 1, 128, 51, 1, -12.5, 10.0, 1, agg, None, None)  # noqa: E731
    assert fwd(None, p) == EINVAL and fwd(p, None) == EINVAL
    assert lib.msde_pair_build(p, p, 1, 100.0, p, p, p, None, 1, None, None) == EINVAL
    assert lib.msde_cfconv_pair_aggregate(p, p, p, p, None, 1, 1, 128, p, None) == EINVAL
    assert lib.msde_cfconv_pair_filter(None, p, p, p, p, p, p, 128, 51, 1, -12.5, 10.0, 0, p, None) == EINVAL
    assert lib.msde_cfconv_aggregate_bwd_x(p, p, None, None, p, p, 1, 128, p, None) == EINVAL
