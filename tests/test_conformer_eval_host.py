"""Conformer evaluation without a GPU (moleculesde_amd/conformer_eval.py): the fp64 reference the device tests compare with,
the COV / MAT reference on a hand-computed matrix, the host-side argument checks and the command line's parser."""
import numpy as np
import pytest
import torch

import conformer_eval_cases as C
from moleculesde_amd import _lib, conformer_eval as ce
from moleculesde_amd.batch import MolData


def test_reference_rigid_copies_are_zero_and_chiral_mirrors_are_not():
    """Entry [k % 3, k] of a case is the case proper.  A rigid copy (rotation + 5 A translation, also shifted by +100) is below
    1e-5 A (fp32 rounding of the stored coordinates is all that is left); z -> -z is 0 for n <= 3 (a planar set is its own
    mirror image) and above 0.1 A for the chiral n >= 4."""
    refs = C.case_references()
    for n in C.SIZES:
        for kind in ("rigid", "rigid_shift100", "collinear"):
            want = refs[(kind, n)][2]
            assert max(want[k % 3, k] for k in range(C.K_CASE)) < 1e-5, (kind, n, want)
        mirror = [refs[("mirror", n)][2][k % 3, k] for k in range(C.K_CASE)]
        if n <= 3:
            assert max(mirror) < 1e-5, (n, mirror)
        else:
            assert min(mirror) > 0.1, (n, mirror)


def test_reference_is_invariant_under_reordering_and_common_rotation():
    ref, gen = C.make_case("noisy", 65)
    want = C.rmsd_block(ref, gen)
    pr, pk = [2, 0, 1], [3, 1, 0, 2]
    assert np.array_equal(C.rmsd_block(ref[pr], gen[pk]), want[pr][:, pk])          # conformers reordered: entries move, bitwise
    Q = C.random_rotation(np.random.default_rng(4))
    rot = C.rmsd_block(ref.astype(np.float64) @ Q.T, gen.astype(np.float64) @ Q.T)
    assert np.abs(rot - want).max() < 1e-9


def test_mirror_follows_the_reference():
    """The kernel's formula in fp64 against the reference: the collinear chains are the worst (the eigenvalue problem's
    round-off goes through a square root near zero), everything else is far below 1e-6."""
    worst, per = C.formula_error()
    assert worst < 5e-6, per
    assert max(v for k, v in per.items() if k != "collinear") < 1e-6, per


def test_cov_mat_reference_on_a_hand_computed_matrix():
    nan = float("nan")
    M = [[0.4, 1.0, nan, 2.0],
         [0.9, 0.3, nan, 1.5],
         [1.6, 1.2, nan, 1.3]]
    got = C.cov_mat_reference(M, (0.35, 0.5, 1.25))
    assert got["rowmin"].tolist() == [0.4, 0.3, 1.2] and got["colmin"].tolist() == [0.4, 0.3, np.inf, 1.3]
    assert got["cov_r"] == [1 / 3, 2 / 3, 1.0]
    assert got["cov_p"] == [0.25, 0.5, 0.5]                       # the NaN column stays in the denominator
    assert got["mat_r"] == pytest.approx(1.9 / 3, rel=1e-15) and got["mat_p"] == pytest.approx(2.0 / 3, rel=1e-15)
    assert got["num_finite"] == 3
    dead = C.cov_mat_reference([[nan, nan], [nan, nan]], (0.5,))
    assert dead["cov_r"] == [0.0] and dead["cov_p"] == [0.0] and dead["num_finite"] == 0
    assert np.isnan(dead["mat_r"]) and np.isnan(dead["mat_p"])


def _record(n=5, K=2, z=None):
    x = torch.zeros(n, 9, dtype=torch.long)
    x[:, 0] = torch.tensor([5] * n if z is None else z)
    return MolData(x=x, positions=torch.randn(n, 3), pos_gen=torch.randn(K * n, 3), num_pos_gen=torch.tensor([K]), finite=True)


def test_evaluate_conformers_rejects_mismatched_atom_counts():
    rec = _record()
    rec.pos_gen = rec.pos_gen[:-1]
    with pytest.raises(ValueError, match="pos_gen"):
        ce.evaluate_conformers([rec])
    with pytest.raises(ValueError, match="references"):
        ce.evaluate_conformers([_record()], references=[torch.randn(2, 4, 3)])
    with pytest.raises(ValueError, match="reference sets"):
        ce.evaluate_conformers([_record(), _record()], references=[torch.randn(2, 5, 3)])
    with pytest.raises(ValueError):
        ce.evaluate_conformers([])


def test_evaluate_conformers_rejects_an_empty_mask():
    with pytest.raises(ValueError, match="keeps no atom"):
        ce.evaluate_conformers([_record(z=[0] * 5)])
    assert ce.heavy_atom_mask(torch.tensor([0, 5, 0, 7])).tolist() == [False, True, False, True]     # 1-D x: QM9-style batches
    assert ce.heavy_atom_mask(_record(z=[0, 6, 0, 0, 7]).x).tolist() == [False, True, False, False, True]


def test_heavy_atom_convention_matches_the_synthetic_molecules():
    """make_molecule(with_h=True) marks hydrogens with x[:, 0] = 0 and draws heavy atoms from indices >= 5."""
    from moleculesde_amd.synthetic import make_molecule
    m = make_molecule(np.random.default_rng(0), 20, with_h=True)
    keep = ce.heavy_atom_mask(m.x)
    assert 0 < int(keep.sum()) < 20 and bool((m.x[keep, 0] >= 5).all()) and bool((m.x[~keep, 0] == 0).all())


def test_cpu_tensors_raise():
    ref, gen = torch.randn(5, 3), torch.randn(10, 3)
    with pytest.raises(_lib.MsdeHipError):
        ce.rmsd_matrix(ref, gen, [5], [1], [2])
    with pytest.raises(_lib.MsdeHipError):
        ce.cov_mat(torch.zeros(2, dtype=torch.float64), [1], [2], (0.5,))
    with pytest.raises(_lib.MsdeHipError):
        ce.evaluate_conformers([_record()], device="cpu")


def test_plan_tables():
    """Offsets of a ragged set and the 8 x 8 tiles that cover every pair once."""
    p = ce.Plan([3, 1, 7], [9, 1, 2], [17, 1, 8], "cpu")
    assert p.out_off.tolist() == [0, 153, 154, 170] and p.conf_off.tolist() == [0, 26, 28, 38]
    assert p.mol.tolist() == [[3, 9, 17, 0, 0, 0, 0, 0], [1, 1, 1, 27, 51, 153, 3, 26], [7, 2, 8, 28, 52, 154, 4, 28]]
    assert p.n_tiles == 2 * 3 + 1 + 1 and p.n_conf == 38
    seen = set()
    for g, r0, k0 in p.tiles.tolist():
        for r in range(r0, min(r0 + ce.TILE, int(p.R[g]))):
            for k in range(k0, min(k0 + ce.TILE, int(p.K[g]))):
                assert (g, r, k) not in seen
                seen.add((g, r, k))
    assert len(seen) == 170
    with pytest.raises(ValueError):
        ce.Plan([3, 0], [1, 1], [1, 1], "cpu")
    with pytest.raises(ValueError):
        ce.Plan([3], [1, 1], [1], "cpu")


def test_summary_and_json():
    stats = np.array([[1.0, 0.5, 0.3, 0.4, 4.0], [0.0, 0.0, np.nan, np.nan, 0.0], [0.5, 0.25, 0.5, 0.8, 3.0]])
    res = ce.summarize(stats, [0.5])
    assert res["num_molecules"] == 3 and res["num_failed"] == 1
    assert res["mean"]["cov_r"] == [0.75] and res["mean"]["mat_p"] == pytest.approx(0.6) and res["median"]["mat_r"] == pytest.approx(0.4)
    assert res["per_molecule"]["num_finite"] == [4, 0, 3]
    assert ce._jsonable(res)["per_molecule"]["mat_r"][1] is None
    none = ce.summarize(stats[1:2], [0.5])
    assert none["num_failed"] == 1 and np.isnan(none["mean"]["mat_r"]) and np.isnan(none["median"]["cov_p"][0])


def test_cli_parser():
    a = ce._parser().parse_args(["samples.pkl"])
    assert a.samples == "samples.pkl" and a.references is None and a.threshold == [0.5, 1.25] and not a.all_atoms
    a = ce._parser().parse_args(["s.pkl", "--references", "refs.pt", "--threshold", "0.75", "2", "--all_atoms", "--per_molecule"])
    assert a.references == "refs.pt" and a.threshold == [0.75, 2.0] and a.all_atoms and a.per_molecule
    with pytest.raises(SystemExit):
        ce._parser().parse_args([])
