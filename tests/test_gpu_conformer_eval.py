"""Conformer evaluation on the GPU (moleculesde_amd/conformer_eval.py; csrc/conformer_rmsd.hip: msde_conf_rmsd_matrix,
msde_conf_cov_mat) against the fp64 references of tests/conformer_eval_cases.py.

Tolerance of every RMSD comparison: 8 x the worst |mirror - reference| over the case set, computed here on the host (the
error of the kernel's formula in fp64 with LAPACK; about 8 x 8e-7 A, set by the collinear chains).  Every case is a molecule of
at most 200 atoms with a handful of conformers: the whole file takes seconds."""
import numpy as np
import pytest
import torch

import conformer_eval_cases as C
from helpers import record_parity

pytestmark = pytest.mark.gpu

RAGGED = [(1, 2, 3), (65, 1, 5), (7, 9, 1), (20, 10, 17), (64, 3, 4), (130, 2, 9)]       # (n, R, K): n = 1, n = 65, R = 1, K = 1,
THRESHOLDS = (1.0, 2.7, 3.3)                                                           # and a 10 x 17 block of 2 x 3 tiles


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def tol():
    return C.MARGIN * C.formula_error()[0]


def _launch(dev, refs, gens, mask=None):
    """One launch over molecules given as (ref [R, n, 3], gen [K, n, 3]) fp32 arrays: (device matrix, host offsets)."""
    from moleculesde_amd import conformer_eval as ce
    n = [r.shape[1] for r in refs]
    R = [r.shape[0] for r in refs]
    K = [g.shape[0] for g in gens]
    ref = torch.from_numpy(np.concatenate([r.reshape(-1, 3) for r in refs])).to(dev)
    gen = torch.from_numpy(np.concatenate([g.reshape(-1, 3) for g in gens])).to(dev)
    m = None if mask is None else torch.from_numpy(np.concatenate(mask)).to(dev)
    out, off = ce.rmsd_matrix(ref, gen, n, R, K, atom_mask=m)
    torch.cuda.synchronize()
    return out, off


def _blocks(out, off, refs, gens):
    h = out.cpu().numpy()
    return [h[int(off[g]):int(off[g + 1])].reshape(refs[g].shape[0], gens[g].shape[0]) for g in range(len(refs))]


@pytest.fixture(scope="module")
def ragged(dev):
    """The six ragged molecules (random conformers, scale 2 A), their device matrix and the reference matrices."""
    rng = np.random.default_rng(21)
    refs = [(2.0 * rng.normal(size=(R, n, 3))).astype(np.float32) for n, R, K in RAGGED]
    gens = [(2.0 * rng.normal(size=(K, n, 3))).astype(np.float32) for n, R, K in RAGGED]
    out, off = _launch(dev, refs, gens)
    return dict(refs=refs, gens=gens, out=out, off=off, want=[C.rmsd_block(r, g) for r, g in zip(refs, gens)])


def test_every_case_kind_at_every_size_matches_the_reference(dev, tol):
    """7 kinds x 10 sizes, each a molecule with R = 3 and K = 4 (a transposed index cannot pass), in one launch."""
    cases = C.case_references()
    keys = list(cases)
    refs, gens = [cases[k][0] for k in keys], [cases[k][1] for k in keys]
    got = _blocks(*_launch(dev, refs, gens), refs, gens)
    worst = {k: 0.0 for k in C.KINDS}
    for key, g in zip(keys, got):
        assert g.shape == (C.R_CASE, C.K_CASE) and np.isfinite(g).all(), key
        worst[key[0]] = max(worst[key[0]], float(np.abs(g - cases[key][2]).max()))
    ferr, fper = C.formula_error()
    record_parity("conformer_eval: device RMSD vs fp64 SVD-Kabsch, 7 kinds x n in %s, R = 3, K = 4; tolerance 8 x %.2e = %.2e A"
                  % (list(C.SIZES), ferr, tol))
    for kind in C.KINDS:
        record_parity("conformer_eval:   %-15s device max |err| %.2e A   (fp64 NumPy mirror of the formula: %.2e A)"
                      % (kind, worst[kind], fper[kind]))
    for kind in C.KINDS:
        assert worst[kind] <= tol, (kind, worst[kind], tol)
    for n in C.SIZES:                                                    # and the values mean what the kinds say
        j = keys.index(("rigid_shift100", n))
        assert max(got[j][k % 3, k] for k in range(4)) < 1e-5 + tol
        j = keys.index(("mirror", n))
        vals = [got[j][k % 3, k] for k in range(4)]
        assert max(vals) < 1e-5 + tol if n <= 3 else min(vals) > 0.1, (n, vals)


def test_ragged_launch_equals_single_launches_and_itself_bitwise(dev, ragged, tol):
    refs, gens = ragged["refs"], ragged["gens"]
    got = _blocks(ragged["out"], ragged["off"], refs, gens)
    assert ragged["off"].tolist() == [0] + list(np.cumsum([R * K for _, R, K in RAGGED]))
    for g, (r, y) in enumerate(zip(refs, gens)):
        assert np.abs(got[g] - ragged["want"][g]).max() <= tol, RAGGED[g]
        alone, off = _launch(dev, [r], [y])
        assert off.tolist() == [0, r.shape[0] * y.shape[0]]
        assert np.array_equal(alone.cpu().numpy().view(np.int64), got[g].reshape(-1).view(np.int64)), RAGGED[g]
    again, _ = _launch(dev, refs, gens)
    assert torch.equal(again.view(torch.int64), ragged["out"].view(torch.int64))


def _h_molecules():
    """Three molecules with hydrogens, 3 references (the molecule, rigidly moved and perturbed by 0.2 A) and 4 generated
    conformers (perturbed by 0.4 A) each."""
    from moleculesde_amd.synthetic import make_molecule
    rng = np.random.default_rng(12)
    mols, refs, gens = [], [], []
    for n in (12, 20, 33):
        m = make_molecule(rng, n, with_h=True)
        p = m.positions.numpy().astype(np.float64)
        mols.append(m)
        refs.append(np.stack([C._rigid(rng, p + 0.2 * rng.normal(size=p.shape)) for _ in range(3)]).astype(np.float32))
        gens.append(np.stack([C._rigid(rng, p + 0.4 * rng.normal(size=p.shape)) for _ in range(4)]).astype(np.float32))
    return mols, refs, gens


def test_atom_mask(dev, ragged, tol):
    from moleculesde_amd import conformer_eval as ce
    refs, gens = ragged["refs"], ragged["gens"]
    ones, _ = _launch(dev, refs, gens, mask=[np.ones(n, dtype=np.uint8) for n, _, _ in RAGGED])
    assert torch.equal(ones.view(torch.int64), ragged["out"].view(torch.int64))          # all atoms kept = no mask, bitwise
    mols, hr, hg = _h_molecules()
    keep = [ce.heavy_atom_mask(m.x).numpy() for m in mols]
    assert all(0 < k.sum() < k.size for k in keep)
    got = _blocks(*_launch(dev, hr, hg, mask=keep), hr, hg)
    full = _blocks(*_launch(dev, hr, hg), hr, hg)
    for g in range(len(mols)):
        want = C.rmsd_block(hr[g], hg[g], keep=keep[g])                                  # the reference on the compacted atoms
        assert np.abs(got[g] - want).max() <= tol
        assert np.abs(full[g] - want).max() > 1e-3                                       # the mask is not a no-op


def test_nan_coordinates_poison_one_column_only(dev, ragged):
    refs, gens = ragged["refs"], [g.copy() for g in ragged["gens"]]
    gens[3][5, 7, 1] = np.nan                       # molecule 3 (10 x 17): generated conformer 5, atom 7, y
    gens[5][8, 129, 2] = np.inf                     # molecule 5 (2 x 9): the last atom of the last conformer
    got = _blocks(*_launch(dev, refs, gens), refs, gens)
    clean = _blocks(ragged["out"], ragged["off"], refs, gens)
    for g in range(len(RAGGED)):
        bad = {3: 5, 5: 8}.get(g)
        cols = [k for k in range(RAGGED[g][2]) if k != bad]
        assert np.array_equal(got[g][:, cols].view(np.int64), clean[g][:, cols].view(np.int64))
        if bad is not None:
            assert np.isnan(got[g][:, bad]).all()
    r2 = [r.copy() for r in refs]
    r2[3][4, 0, 0] = np.nan                         # a reference: its row
    got = _blocks(*_launch(dev, r2, ragged["gens"]), refs, gens)
    assert np.isnan(got[3][4]).all()
    rows = [r for r in range(10) if r != 4]
    assert np.array_equal(got[3][rows].view(np.int64), clean[3][rows].view(np.int64))
    # a non-finite coordinate on an atom the mask leaves out does not count
    mask = [np.ones(n, dtype=np.uint8) for n, _, _ in RAGGED]
    mask[3][7] = 0
    a = _blocks(*_launch(dev, refs, gens[:3] + [gens[3]] + ragged["gens"][4:], mask=mask), refs, gens)
    b = _blocks(*_launch(dev, refs, ragged["gens"], mask=mask), refs, gens)
    assert np.isfinite(a[3]).all() and np.array_equal(a[3].view(np.int64), b[3].view(np.int64))


def test_cov_mat_kernel(dev, ragged):
    """msde_conf_cov_mat on the ragged matrix with NaN columns added: molecule 0 loses all of its columns, molecule 3 two."""
    from moleculesde_amd import conformer_eval as ce

    def poison(mats):
        mats = [m.copy() for m in mats]
        mats[0][:, :] = np.nan
        mats[3][:, [2, 16]] = np.nan
        return mats

    want = poison(ragged["want"])
    assert C.min_gap_to_thresholds(want, THRESHOLDS) > 1e-3        # a condition on the inputs: no count hinges on a tolerance
    R, K = [r for _, r, _ in RAGGED], [k for _, _, k in RAGGED]
    dev_mats = poison(_blocks(ragged["out"], ragged["off"], ragged["refs"], ragged["gens"]))
    rmsd = torch.from_numpy(np.concatenate([m.reshape(-1) for m in dev_mats])).to(dev)
    stats, conf_min, conf_off = ce.cov_mat(rmsd, R, K, THRESHOLDS)
    torch.cuda.synchronize()
    stats, conf_min, T = stats.cpu().numpy(), conf_min.cpu().numpy(), len(THRESHOLDS)
    assert stats.shape == (len(RAGGED), 2 * T + 3) and conf_off.tolist() == [0] + list(np.cumsum([r + k for r, k in zip(R, K)]))
    seen = set()
    for g in range(len(RAGGED)):
        ref_m, ref_w = C.cov_mat_reference(dev_mats[g], THRESHOLDS), C.cov_mat_reference(want[g], THRESHOLDS)
        assert stats[g, :T].tolist() == ref_m["cov_r"] == ref_w["cov_r"], g
        assert stats[g, T:2 * T].tolist() == ref_m["cov_p"] == ref_w["cov_p"], g
        assert stats[g, 2 * T + 2] == ref_m["num_finite"]
        mins = conf_min[int(conf_off[g]):int(conf_off[g + 1])]
        assert np.array_equal(mins[:R[g]], ref_m["rowmin"]) and np.array_equal(mins[R[g]:], ref_m["colmin"])
        seen.update(stats[g, :2 * T].tolist())
        if g == 0:
            assert ref_m["num_finite"] == 0 and not stats[g, :2 * T].any() and np.isnan(stats[g, 2 * T:2 * T + 2]).all()
        else:
            rel = max(R[g], K[g]) * 2.0 ** -52
            assert abs(stats[g, 2 * T] - ref_m["mat_r"]) <= rel * ref_m["mat_r"]
            assert abs(stats[g, 2 * T + 1] - ref_m["mat_p"]) <= rel * ref_m["mat_p"]
    assert stats[3, 2 * T + 2] == 15
    assert len(seen - {0.0, 1.0}) >= 2                              # the thresholds cut through the minima, not around them


def _records(mols, gens):
    from moleculesde_amd.batch import MolData
    out = []
    for m, g in zip(mols, gens):
        out.append(MolData(x=m.x.clone(), positions=m.positions.clone(), pos_gen=torch.from_numpy(g.reshape(-1, 3).copy()),
                           num_pos_gen=torch.tensor([g.shape[0]]), finite=True))
    return out


def test_evaluate_conformers_on_hand_built_records(dev, tol, tmp_path):
    """Records as the sampler writes them, through evaluate_conformers with the record's own positions and with three explicit
    references per molecule, heavy atoms and all atoms, a NaN conformer and a failed record; from the list and from a pickle."""
    import pickle
    from moleculesde_amd import conformer_eval as ce
    mols, refs, gens = _h_molecules()
    gens = [g.copy() for g in gens]
    gens[1][2, 3, 0] = np.nan                                        # one conformer of molecule 1 is not finite
    mols[1].x[3, 0] = 6                                              # ... on a heavy atom, so that it counts in both modes
    recs = _records(mols, gens)
    recs[2].finite = False                                           # the sampler flagged molecule 2
    thr = (0.45, 0.8)
    for explicit in (False, True):
        for heavy in (True, False):
            keeps = [ce.heavy_atom_mask(m.x).numpy() if heavy else None for m in mols]
            rr = refs if explicit else [m.positions.numpy()[None] for m in mols]
            want = [C.rmsd_block(r, g, keep=k) for r, g, k in zip(rr, gens, keeps)]
            want[2][:] = np.nan
            assert C.min_gap_to_thresholds(want, thr) > 1e-3
            ref = C.summary_reference(want, thr)
            got = ce.evaluate_conformers(recs, [torch.from_numpy(r) for r in refs] if explicit else None, thresholds=thr,
                                         heavy_atoms_only=heavy)
            assert got["thresholds"] == list(thr) and got["num_molecules"] == 3 and got["num_failed"] == 1 == ref["num_failed"]
            pm, pr = got["per_molecule"], ref["per_molecule"]
            assert pm["num_finite"] == pr["num_finite"] == [4, 3, 0]
            assert pm["cov_r"] == pr["cov_r"] and pm["cov_p"] == pr["cov_p"]
            assert pm["cov_r"][2] == [0.0, 0.0] and np.isnan(pm["mat_r"][2]) and np.isnan(pm["mat_p"][2])
            for key in ("mat_r", "mat_p"):
                assert np.abs(np.array(pm[key][:2]) - np.array(pr[key][:2])).max() <= tol
            for name in ("mean", "median"):
                assert got[name]["cov_r"] == pytest.approx(ref[name]["cov_r"], abs=1e-15)
                assert got[name]["cov_p"] == pytest.approx(ref[name]["cov_p"], abs=1e-15)
                assert abs(got[name]["mat_r"] - ref[name]["mat_r"]) <= tol and abs(got[name]["mat_p"] - ref[name]["mat_p"]) <= tol
    path = tmp_path / "samples.pkl"
    with open(path, "wb") as f:
        pickle.dump(recs, f)
    a, b = ce.evaluate_conformers(str(path), thresholds=thr), ce.evaluate_conformers(recs, thresholds=thr)
    assert a["per_molecule"]["mat_p"][:2] == b["per_molecule"]["mat_p"][:2] and a["mean"] == b["mean"]


def test_sampler_output_goes_through(dev):
    """Two synthetic molecules through generate_samples_from_testset (2 conformers, 3 steps) and evaluate_conformers: shapes and
    keys fit, every value is finite or the molecule is flagged."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import conformer_eval as ce, sampler
    from moleculesde_amd.synthetic import make_molecule
    torch.manual_seed(0)
    gnn = G.GNN(3, 32, gnn_type="GIN").to(dev).eval()
    s23 = G.SDEModel2Dto3D_02(emb_dim=32, hidden_dim=32, beta_min=0.2, beta_max=1.0, num_diffusion_timesteps=1000,
                              beta_schedule=None, SDE_type="VE", use_extend_graph=True).to(dev).eval()
    rng = np.random.default_rng(3)
    mols = [make_molecule(rng, n) for n in (9, 14)]
    recs = sampler.generate_samples_from_testset(mols, gnn, s23, num_repeat=2, start=0, end=2, num_steps=3, noise_seed=5)
    res = ce.evaluate_conformers(recs)
    assert res["num_molecules"] == 2 and res["thresholds"] == [0.5, 1.25]
    pm = res["per_molecule"]
    assert len(pm["cov_r"]) == 2 and all(len(v) == 2 for v in pm["cov_r"] + pm["cov_p"])
    failed = 0
    for g, rec in enumerate(recs):
        if pm["num_finite"][g] == 0:
            failed += 1
            assert np.isnan(pm["mat_r"][g]) and np.isnan(pm["mat_p"][g])
        else:
            assert rec.finite and np.isfinite([pm["mat_r"][g], pm["mat_p"][g]]).all() and pm["mat_p"][g] >= pm["mat_r"][g] >= 0
            assert all(0 <= v <= 1 for v in pm["cov_r"][g] + pm["cov_p"][g])
    assert res["num_failed"] == failed
