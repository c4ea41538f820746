"""Symmetry-aware conformer evaluation on the GPU (csrc/conformer_rmsd.hip: msde_conf_rmsd_matrix_sym; conformer_eval.py:
rmsd_matrix(permutations=...), evaluate_conformers(symmetry=True)) against the fp64 reference of tests/conformer_sym_cases.py.

Tolerance of every RMSD comparison: 8 x the worst |NumPy fp64 mirror of the device formula - sym_rmsd_block| over THIS file's
cases (the arbitrary permutation lists, the relabelled rigid copies, exact and rounded to fp32, and the masked molecules),
computed here on the host.  It is set by the rigid copies, whose eigenvalue round-off goes through a square root at zero.
Every case is a handful of molecules of at most 200 atoms: the whole file takes seconds."""
import numpy as np
import pytest
import torch

import conformer_eval_cases as C
import conformer_sym_cases as S
from helpers import record_parity

pytestmark = pytest.mark.gpu

# (n, R, K, P): P = 1; n = 1 and 2; 63 / 64 / 65 permutations and atoms (the 64-entry blocks the kernel hands a permutation
# row out in); a 10 x 17 block of 2 x 3 tiles with 129 permutations; 130 atoms in LDS, 200 on the global-memory path; and
# P = 4 / 5 around the four permutations a workgroup's four waves take per pass
SHAPES = [(1, 2, 3, 1), (2, 1, 1, 2), (5, 3, 4, 24), (20, 3, 4, 63), (20, 3, 4, 64), (20, 9, 1, 65), (20, 10, 17, 129),
          (63, 2, 3, 3), (64, 2, 3, 3), (65, 2, 3, 3), (130, 2, 9, 2), (200, 1, 2, 3), (20, 3, 4, 4), (20, 3, 4, 5)]
SEEDS = (0, 1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def _collect_the_samplers_graphs_here():
    """The sampler test below captures hipGraphs; whatever of them is left as cyclic garbage is collected when this module is
    done, with the device idle, instead of whenever the collector next runs inside some later test (moleculesde_amd/slabs.py,
    no_gc: destroying a graph or releasing pool memory at an arbitrary moment is a hazard of its own)."""
    yield
    import gc
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.synchronize()


def _launch(dev, refs, gens, perms=None, mask=None, lds_atoms=None):
    """One launch over molecules given as (ref [R, n, 3], gen [K, n, 3]) fp32 arrays: the per-molecule [R, K] blocks (host)."""
    from moleculesde_amd import conformer_eval as ce
    n = [r.shape[1] for r in refs]
    R = [r.shape[0] for r in refs]
    K = [g.shape[0] for g in gens]
    ref = torch.from_numpy(np.concatenate([r.reshape(-1, 3) for r in refs])).to(dev)
    gen = torch.from_numpy(np.concatenate([g.reshape(-1, 3) for g in gens])).to(dev)
    m = None if mask is None else torch.from_numpy(np.concatenate(mask).astype(np.uint8)).to(dev)
    out, off = ce.rmsd_matrix(ref, gen, n, R, K, atom_mask=m, permutations=perms, lds_atoms=lds_atoms)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    return [h[int(off[g]):int(off[g + 1])].reshape(R[g], K[g]) for g in range(len(refs))]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def arbitrary():
    """The ragged set of SHAPES: random conformers (scale 2 A), the identity and P - 1 random permutations each."""
    rng = np.random.default_rng(31)
    refs = [(2.0 * rng.normal(size=(R, n, 3))).astype(np.float32) for n, R, K, P in SHAPES]
    gens = [(2.0 * rng.normal(size=(K, n, 3))).astype(np.float32) for n, R, K, P in SHAPES]
    perms = [S.random_permutations(rng, n, P) for n, R, K, P in SHAPES]
    return dict(refs=refs, gens=gens, perms=perms)


@pytest.fixture(scope="module")
def masked():
    """The star with a dropped leaf (its 6 automorphisms), and 70 atoms of which a random half is kept (5 random permutations of
    the kept atoms), 3 references and 4 generated conformers each."""
    rng = np.random.default_rng(32)
    star = S.GRAPHS[7]
    keep = [star.keep, rng.random(70) < 0.5]
    perms = [S.group(star)[0], S.random_permutations(rng, 70, 5, keep[1])]
    refs = [(2.0 * rng.normal(size=(3, n, 3))).astype(np.float32) for n in (5, 70)]
    gens = [(2.0 * rng.normal(size=(4, n, 3))).astype(np.float32) for n in (5, 70)]
    return dict(refs=refs, gens=gens, perms=perms, keep=keep)


@pytest.fixture(scope="module")
def copies():
    """Per graph of the table and seed a relabelled rigid copy, exact in fp32 and rounded to fp32, with the graph's own group."""
    out = []
    for g in S.GRAPHS:
        perms = S.group(g)[0]
        for seed in SEEDS:
            for exact in (True, False):
                ref, gen, _ = S.relabelled_copy(g, seed, exact)
                out.append(dict(graph=g, exact=exact, ref=ref, gen=gen, perms=perms))
    return out


@pytest.fixture(scope="module")
def reference(arbitrary, masked, copies):
    """The fp64 reference and the mirror of every case of this file, once, and the tolerance they give."""
    cases = [(r, g, p, None) for r, g, p in zip(arbitrary["refs"], arbitrary["gens"], arbitrary["perms"])]
    cases += [(r, g, p, k) for r, g, p, k in zip(masked["refs"], masked["gens"], masked["perms"], masked["keep"])]
    cases += [(c["ref"], c["gen"], c["perms"], c["graph"].keep) for c in copies]
    worst, mats = S.formula_error(cases)
    na, nm = len(SHAPES), len(masked["refs"])
    return dict(tol=C.MARGIN * worst, formula=worst, arbitrary=[m[0] for m in mats[:na]], masked=[m[0] for m in mats[na:na + nm]],
                copies=[m[0] for m in mats[na + nm:]])


@pytest.fixture(scope="module")
def ragged(dev, arbitrary):
    return _launch(dev, arbitrary["refs"], arbitrary["gens"], arbitrary["perms"])


def test_arbitrary_permutation_lists_match_the_reference(ragged, reference):
    tol = reference["tol"]
    worst = 0.0
    for got, want, shape in zip(ragged, reference["arbitrary"], SHAPES):
        assert got.shape == want.shape and np.isfinite(got).all(), shape
        worst = max(worst, float(np.abs(got - want).max()))
    record_parity("conformer_sym: device best RMSD vs fp64 min over permutations of SVD-Kabsch; tolerance 8 x %.2e = %.2e A"
                  % (reference["formula"], tol))
    record_parity("conformer_sym:   %-28s device max |err| %.2e A   (%d molecules, (n, R, K, P) = %s)"
                  % ("arbitrary permutation lists", worst, len(SHAPES), SHAPES))
    assert worst <= tol, (worst, tol)


def test_relabelled_rigid_copy_is_found_only_with_the_symmetry(dev, copies, reference):
    """gen = Q ref[perm] + t with perm a non-identity automorphism: plain Kabsch is above 0.05 A, the symmetric RMSD is 0."""
    tol = reference["tol"]
    refs, gens = [c["ref"] for c in copies], [c["gen"] for c in copies]
    keep = [c["graph"].keep for c in copies]
    plain = _launch(dev, refs, gens, mask=keep)
    sym = _launch(dev, refs, gens, [c["perms"] for c in copies], mask=keep)
    worst = {True: 0.0, False: 0.0}
    for c, p, s, want in zip(copies, plain, sym, reference["copies"]):
        name = (c["graph"].name, c["exact"])
        want_plain = C.rmsd_block(c["ref"], c["gen"], keep=c["graph"].keep)
        assert want_plain.min() >= 0.05 + 1e-3 and want.max() <= 0.05 - 1e-3, name     # the reference's own gap to 0.05 A
        assert p.min() > 0.05, (name, p)
        worst[c["exact"]] = max(worst[c["exact"]], float(np.abs(s - want).max()))
        if c["exact"]:
            assert want.max() <= 2e-14, (name, want)                                     # the copy is rigid to the last bit
            assert s.max() <= tol, (name, s, tol)
        assert np.abs(s - want).max() <= tol, (name, s, want, tol)
    record_parity("conformer_sym:   %-28s device max |err| %.2e A   (%d graphs x %d seeds)"
                  % ("relabelled copy, exact in fp32", worst[True], len(S.GRAPHS), len(SEEDS)))
    record_parity("conformer_sym:   %-28s device max |err| %.2e A" % ("relabelled copy, fp32-rounded", worst[False]))


def test_symmetric_is_at_most_plain_and_equal_for_the_identity_alone(dev, arbitrary, ragged, reference):
    tol = reference["tol"]
    refs, gens = arbitrary["refs"], arbitrary["gens"]
    plain = _launch(dev, refs, gens)
    ident = _launch(dev, refs, gens, [p[:1] for p in arbitrary["perms"]])
    lower = 0
    for shape, s, p, i in zip(SHAPES, ragged, plain, ident):
        assert (s <= p + tol).all(), shape                              # every list holds the identity
        assert np.abs(i - p).max() <= tol, shape                        # P = 1: the plain kernel's value, another summation order
        lower += int((s < p - 1e-3).sum())
    assert np.abs(ragged[0] - plain[0]).max() <= tol                    # SHAPES[0] has P = 1 as it stands
    assert lower > 0                                                    # and the permutations do lower some entries


def test_ragged_equals_single_launches_itself_shuffled_rows_and_the_global_path_bitwise(dev, arbitrary, ragged):
    refs, gens, perms = arbitrary["refs"], arbitrary["gens"], arbitrary["perms"]
    for g in range(len(SHAPES)):
        assert _same_bits(_launch(dev, [refs[g]], [gens[g]], [perms[g]]), [ragged[g]]), SHAPES[g]
    assert _same_bits(_launch(dev, refs, gens, perms), ragged)
    rng = np.random.default_rng(33)
    shuffled = [p[rng.permutation(len(p))] for p in perms]
    assert any(len(p) > 1 and p[0].tolist() != list(range(p.shape[1])) for p in shuffled)        # the identity left row 0
    assert _same_bits(_launch(dev, refs, gens, shuffled), ragged)
    assert _same_bits(_launch(dev, refs, gens, perms, lds_atoms=0), ragged)                      # nothing staged in LDS
    assert _same_bits(_launch(dev, refs, gens, perms, lds_atoms=64), ragged)                     # n <= 64 staged, the rest not


def test_atom_mask(dev, masked, reference):
    tol = reference["tol"]
    got = _launch(dev, masked["refs"], masked["gens"], masked["perms"], mask=masked["keep"])
    full = _launch(dev, masked["refs"], masked["gens"], [np.arange(n, dtype=np.int32)[None] for n in (5, 70)])
    worst = 0.0
    for g, want in enumerate(reference["masked"]):
        worst = max(worst, float(np.abs(got[g] - want).max()))
        assert np.abs(got[g] - want).max() <= tol, g
        assert np.abs(full[g] - want).max() > 1e-3                      # neither the mask nor the permutations are a no-op
    record_parity("conformer_sym:   %-28s device max |err| %.2e A" % ("masked star, masked 70 atoms", worst))
    ones = _launch(dev, masked["refs"], masked["gens"], masked["perms"], mask=masked["keep"], lds_atoms=0)
    assert _same_bits(ones, got)


def test_non_finite_coordinates_poison_one_row_or_column_only(dev, arbitrary, ragged):
    refs, gens, perms = arbitrary["refs"], [g.copy() for g in arbitrary["gens"]], arbitrary["perms"]
    gens[6][5, 7, 1] = np.nan                       # the 10 x 17 molecule: generated conformer 5
    gens[10][8, 129, 2] = np.inf                    # the 130-atom molecule: the last atom of the last conformer
    gens[11][1, 0, 0] = np.nan                      # the 200-atom molecule (global-memory path)
    got = _launch(dev, refs, gens, perms)
    for g in range(len(SHAPES)):
        bad = {6: 5, 10: 8, 11: 1}.get(g)
        cols = [k for k in range(SHAPES[g][2]) if k != bad]
        assert np.array_equal(got[g][:, cols].view(np.int64), ragged[g][:, cols].view(np.int64)), SHAPES[g]
        if bad is not None:
            assert np.isnan(got[g][:, bad]).all()
    r2 = [r.copy() for r in refs]
    r2[6][4, 0, 0] = np.inf                         # a reference: its row
    got = _launch(dev, r2, arbitrary["gens"], perms)
    assert np.isnan(got[6][4]).all()
    rows = [r for r in range(10) if r != 4]
    assert np.array_equal(got[6][rows].view(np.int64), ragged[6][rows].view(np.int64))
    assert _same_bits(got[:6] + got[7:], ragged[:6] + ragged[7:])


def _records(copies_of, K=3):
    """One record per graph: the reference of seed 0 as `positions`, K relabelled rigid copies of it as `pos_gen`."""
    from moleculesde_amd.batch import MolData
    recs = []
    for g in S.GRAPHS:
        ref = S.relabelled_copy(g, 0)[0][0]
        rng = np.random.default_rng([7, S.GRAPHS.index(g)])
        perms = S.group(g)[0]
        gens = []
        for _ in range(K):
            perm = perms[1 + int(rng.integers(0, len(perms) - 1))]
            gens.append(ref[perm] @ S._AXIS_ROTATIONS[int(rng.integers(0, 24))].T + np.rint(rng.normal(size=3) * 2048.0) / 1024.0)
        x = torch.zeros(g.n, 9, dtype=torch.long)
        x[:, 0] = torch.from_numpy(g.atom_colour)
        attr = torch.zeros(2 * len(g.bonds), 3, dtype=torch.long)
        attr[:, 0] = torch.from_numpy(g.edge_colour)
        recs.append(MolData(x=x, edge_index=torch.from_numpy(g.edge_index), edge_attr=attr, positions=torch.from_numpy(ref.copy()),
                            pos_gen=torch.from_numpy(np.concatenate(gens).astype(np.float32)), num_pos_gen=torch.tensor([K]),
                            finite=True))
    return recs


def test_evaluate_conformers_with_and_without_symmetry(dev, reference):
    """Hand-built records on the symmetric graphs whose generated conformers are relabelled copies of the reference: all covered
    at 0.05 A with the symmetry, none without; the group sizes are those of the table."""
    from moleculesde_amd import conformer_eval as ce
    recs = _records(S.GRAPHS)
    for rec, g in zip(recs, S.GRAPHS):                                   # the inputs keep clear of the threshold, in fp64
        ref, gen = rec.positions.numpy()[None], rec.pos_gen.numpy().reshape(-1, g.n, 3)
        assert C.rmsd_block(ref, gen, keep=g.keep).min() >= 0.05 + 1e-3, g.name
        assert S.sym_rmsd_block(ref, gen, S.group(g)[0], g.keep).max() <= 0.05 - 1e-3, g.name
    sym = ce.evaluate_conformers(recs, thresholds=(0.05,), symmetry=True)
    plain = ce.evaluate_conformers(recs, thresholds=(0.05,))
    assert "symmetry" not in plain
    assert sym["symmetry"] == {"num_permutations": [g.count for g in S.GRAPHS], "num_truncated": 0}
    G = len(S.GRAPHS)
    assert sym["per_molecule"]["cov_r"] == [[1.0]] * G and sym["per_molecule"]["cov_p"] == [[1.0]] * G
    assert plain["per_molecule"]["cov_r"] == [[0.0]] * G and plain["per_molecule"]["cov_p"] == [[0.0]] * G
    assert sym["mean"]["cov_r"] == [1.0] and sym["mean"]["cov_p"] == [1.0] and plain["mean"]["cov_r"] == [0.0]
    assert max(sym["per_molecule"]["mat_r"] + sym["per_molecule"]["mat_p"]) <= reference["tol"]
    assert min(plain["per_molecule"]["mat_r"] + plain["per_molecule"]["mat_p"]) > 0.05
    cut = ce.evaluate_conformers(recs, thresholds=(0.05,), symmetry=True, max_automorphisms=100)
    assert cut["symmetry"]["num_truncated"] == 1 and cut["symmetry"]["num_permutations"][8] == 100
    for key in ("mat_r", "mat_p"):                                       # a cut group: between the full group and plain
        assert all(s - reference["tol"] <= c <= p + reference["tol"]
                   for s, c, p in zip(sym["per_molecule"][key], cut["per_molecule"][key], plain["per_molecule"][key]))


def test_sampler_output_agrees_in_both_modes(dev, reference):
    """The sampler's own synthetic molecules (random element and bond labels: almost every group is trivial) through both modes:
    equal within the tolerance where the group is trivial, never larger with the symmetry."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import conformer_eval as ce, sampler
    from moleculesde_amd.synthetic import make_molecule
    torch.manual_seed(0)
    gnn = G.GNN(3, 32, gnn_type="GIN").to(dev).eval()
    s23 = G.SDEModel2Dto3D_02(emb_dim=32, hidden_dim=32, beta_min=0.2, beta_max=1.0, num_diffusion_timesteps=1000,
                              beta_schedule=None, SDE_type="VE", use_extend_graph=True).to(dev).eval()
    rng = np.random.default_rng(3)
    mols = [make_molecule(rng, n) for n in (9, 14, 11)]
    recs = sampler.generate_samples_from_testset(mols, gnn, s23, num_repeat=2, start=0, end=3, num_steps=3, noise_seed=5)
    plain, sym = ce.evaluate_conformers(recs), ce.evaluate_conformers(recs, symmetry=True)
    counts = sym["symmetry"]["num_permutations"]
    assert len(counts) == 3 and min(counts) >= 1 and sym["symmetry"]["num_truncated"] == 0
    assert sym["num_failed"] == plain["num_failed"] and sym["per_molecule"]["num_finite"] == plain["per_molecule"]["num_finite"]
    for key in ("mat_r", "mat_p"):
        for g in range(3):
            a, b = sym["per_molecule"][key][g], plain["per_molecule"][key][g]
            if np.isnan(b):
                assert np.isnan(a)
            elif counts[g] == 1:
                assert abs(a - b) <= reference["tol"]
            else:
                assert a <= b + reference["tol"]
