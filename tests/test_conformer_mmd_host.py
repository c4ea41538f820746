"""Host-side tests of the distance-MMD evaluation (no GPU): the NumPy mirror of the definition against closed forms, the
evaluated-pair lists of known graphs, the packing checks, and the C ABI declarations."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import conformer_mmd_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the mirror ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0.3, 1.0, 17.5])
def test_closed_form_one_reference_one_generated_one_distance(d):
    """R = K = 1, E = 1, distances 0 and d: L = d^2 = sigma^2, so MMD = 10 - 2 (e^-4 + e^-2 + e^-1 + e^-1/2 + e^-1/4) for any d."""
    want = 10.0 - 2.0 * sum(math.exp(-s) for s in (4.0, 2.0, 1.0, 0.5, 0.25))
    assert abs(want - 6.18627638) < 1e-8
    z = np.array([[0.0], [d]])
    assert abs(C.mmd(z, 1, [0]) - want) < 1e-14
    ref = np.zeros((1, 2, 3), dtype=np.float32)
    gen = np.array([[[0, 0, 0], [d, 0, 0]]], dtype=np.float32)
    # the same through the coordinates: the reference's two atoms coincide (distance 0), the generated ones are d apart
    got = C.molecule_statistics(ref, gen, np.array([[0, 1]], dtype=np.int32))
    assert abs(got["stats"][0] - want) < 1e-14 and abs(got["stats"][1] - want) < 1e-14 and abs(got["stats"][4] - want) < 1e-14
    assert np.isnan(got["stats"][2]) and np.isnan(got["stats"][3]) and got["pair"].size == 0       # E < 2: no Pair
    assert got["stats"][5:].tolist() == [1.0, 1.0]


def test_zero_bandwidth_gives_exactly_zero():
    z = np.full((7, 3), 1.25)
    for cols in ([0], [0, 2], [0, 1, 2]):
        assert C.bandwidth(z, cols) == 0.0 and C.mmd(z, 3, cols) == 0.0
    z32 = z.astype(np.float32)
    assert C.mmd(z32, 3, [1]) == 0.0 and C.mmd(z32, 3, [1]).dtype == np.float32      # the dtype switch keeps the dtype


def test_bandwidth_is_additive_over_the_columns():
    rng = np.random.default_rng(5)
    z = rng.normal(size=(11, 4)) + 2.0
    for e in range(4):
        for f in range(e + 1, 4):
            assert C.bandwidth(z, [e, f]) == pytest.approx(C.bandwidth(z, [e]) + C.bandwidth(z, [f]), rel=1e-14)
    assert C.bandwidth(z, range(4)) == pytest.approx(sum(C.bandwidth(z, [e]) for e in range(4)), rel=1e-14)


def test_pair_statistics_of_the_mirror():
    """Two distances: Single from each column, Pair from both, All = the one pair; a generated ensemble drawn from the
    reference distribution scores far below a shifted one."""
    rng = np.random.default_rng(6)
    ref, gen = C.make_conformers(rng, 4, 20, 30, ref_noise=0.2, gen_noise=0.2)
    pairs = np.array([[0, 1], [1, 3]], dtype=np.int32)
    same = C.molecule_statistics(ref, gen, pairs)
    assert same["single"].shape == (2,) and same["pair"].shape == (1,)
    assert same["stats"][2] == same["stats"][3] == same["pair"][0] == same["stats"][4]
    far = C.molecule_statistics(ref, gen * np.float32(1.5), pairs)
    assert 0 <= same["stats"][4] < 0.5 < far["stats"][4]
    f32 = C.molecule_statistics(ref, gen, pairs, dtype=np.float32)
    assert 0 < np.abs(f32["stats"][:5] - same["stats"][:5]).max() < 1e-4        # the fp32 switch computes in fp32


# ---- evaluated pairs ----------------------------------------------------------------------------------------------------------
def _record(z, bonds):
    src = [a for a, b in bonds] + [b for a, b in bonds]
    dst = [b for a, b in bonds] + [a for a, b in bonds]
    return SimpleNamespace(x=torch.tensor(z, dtype=torch.long)[:, None], edge_index=torch.tensor([src, dst], dtype=torch.long))


def test_distance_pairs_on_known_graphs():
    from moleculesde_amd.conformer_mmd import distance_pairs
    chain = _record([5] * 5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    p = distance_pairs(chain, max_hops=3)
    assert p.dtype == np.int32 and p.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [1, 4], [2, 3], [2, 4], [3, 4]]
    assert p.tolist() == C.chain_pairs(5, 3).tolist()
    assert distance_pairs(chain, max_hops=1).tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    assert len(distance_pairs(chain, max_hops=None)) == 10 and len(distance_pairs(chain, max_hops=4)) == 10
    ring = _record([5] * 6, [(i, (i + 1) % 6) for i in range(6)])
    p = distance_pairs(ring, max_hops=3)
    assert len(p) == 15 and p.tolist() == sorted(p.tolist()) and p.tolist() == C.all_pairs(6).tolist()
    assert sorted(distance_pairs(ring, max_hops=1).tolist()) == sorted([sorted(b) for b in [(i, (i + 1) % 6) for i in range(6)]])
    assert len(distance_pairs(ring, max_hops=2)) == 12


def test_distance_pairs_drop_hydrogens_but_walk_through_them():
    from moleculesde_amd.conformer_mmd import distance_pairs
    # atoms 0 C, 1 H, 2 C, 3 C, 4 H: bonds C0-H1, H1-C2 (two heavy atoms on one hydrogen), C2-C3, C3-H4
    rec = _record([5, 0, 5, 5, 0], [(0, 1), (1, 2), (2, 3), (3, 4)])
    # evaluated numbering: atom 0 -> 0, atom 2 -> 1, atom 3 -> 2
    assert distance_pairs(rec, max_hops=1).tolist() == [[1, 2]]
    assert distance_pairs(rec, max_hops=2).tolist() == [[0, 1], [1, 2]]          # C0 .. C2 are 2 hops apart, through H1
    assert distance_pairs(rec, max_hops=3).tolist() == [[0, 1], [0, 2], [1, 2]]
    assert distance_pairs(rec, heavy_atoms_only=False, max_hops=1).tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    assert distance_pairs(rec, max_hops=None).tolist() == [[0, 1], [0, 2], [1, 2]]
    lone = SimpleNamespace(x=torch.tensor([[5], [5]]))
    assert distance_pairs(lone, max_hops=None).tolist() == [[0, 1]]
    with pytest.raises(ValueError):
        distance_pairs(lone, max_hops=3)                                         # no edge_index to count hops in


# ---- packing ------------------------------------------------------------------------------------------------------------------
def test_plan_tables():
    from moleculesde_amd.conformer_mmd import Plan
    keep = np.array([1, 0, 1, 1] + [1, 1, 1], dtype=bool)
    pairs = np.array([[0, 1], [0, 2], [1, 2]] + [[0, 2]], dtype=np.int32)
    plan = Plan([4, 3], [2, 1], [3, 5], pairs, [0, 3, 4], keep)
    assert plan.atom_pairs.tolist() == [[0, 2], [0, 3], [2, 3], [0, 2]]          # evaluated numbering -> atom indices
    assert plan.mol.tolist() == [[4, 2, 3, 0, 0, 0, 0, 0], [3, 1, 5, 8, 12, 15, 4, 5]]
    assert plan.items.tolist() == [[0, 0, -1], [0, 1, -1], [0, 2, -1], [1, 0, -1], [0, 0, 1], [0, 0, 2], [0, 1, 2]]
    assert plan.pairitem_ptr.tolist() == [0, 3, 3] and plan.n_cols == 4 and plan.n_items == 7 and plan.c_max == 6
    empty = Plan([2], [1], [1], np.zeros((0, 2), dtype=np.int32), [0, 0])
    assert empty.n_items == 0 and empty.items.shape == (0, 3)


def test_packing_errors():
    from moleculesde_amd import conformer_mmd as cm
    from moleculesde_amd.batch import MolData
    one = np.array([[0, 1]], dtype=np.int32)
    with pytest.raises(ValueError, match="pooled conformers"):                   # never truncated silently
        cm.Plan([3], [cm.MAX_POOLED - 3], [4], one, [0, 1])
    cm.Plan([3], [cm.MAX_POOLED - 4], [4], one, [0, 1])
    assert cm.MAX_POOLED >= 1024
    with pytest.raises(ValueError):
        cm.Plan([3], [1], [1], np.array([[0, 3]], dtype=np.int32), [0, 1])       # atom 3 of 3
    with pytest.raises(ValueError):
        cm.Plan([3], [1], [1], np.array([[0, 2]], dtype=np.int32), [0, 1], keep=np.array([1, 1, 0]))   # 2 evaluated atoms
    with pytest.raises(ValueError):
        cm.Plan([3], [1], [1], one, [0, 2])
    with pytest.raises(ValueError):
        cm.Plan([3, 3], [1], [1], one, [0, 1, 1])
    # atom-count mismatches, with host tensors: the size checks come before anything touches a device
    ref, gen = torch.zeros(2 * 3, 3), torch.zeros(4 * 3, 3)
    with pytest.raises(ValueError):
        cm.mmd_statistics(ref, gen[:-1], [3], [2], [4], one, [0, 1])
    with pytest.raises(ValueError):
        cm.mmd_statistics(ref, gen, [4], [2], [4], one, [0, 1])
    with pytest.raises(ValueError):
        cm.mmd_statistics(ref, gen, [3], [2], [4], one, [0, 1], kernel_num=0)
    with pytest.raises(ValueError):
        cm.mmd_statistics(ref, gen, [3], [2], [4], one, [0, 1], atom_mask=torch.ones(4, dtype=torch.bool))
    rec = MolData(x=torch.full((3, 9), 5), positions=torch.zeros(3, 3), pos_gen=torch.zeros(7, 3), num_pos_gen=torch.tensor([2]),
                  edge_index=torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), finite=True)
    with pytest.raises(ValueError, match="pos_gen"):
        cm.evaluate_distance_mmd([rec])
    rec.pos_gen = torch.zeros(6, 3)
    with pytest.raises(ValueError, match="references"):
        cm.evaluate_distance_mmd([rec], references=[torch.zeros(2, 4, 3)])
    rec.pos_gen, rec.num_pos_gen = torch.zeros(3 * cm.MAX_POOLED, 3), torch.tensor([cm.MAX_POOLED])
    with pytest.raises(ValueError, match="pooled conformers"):
        cm.evaluate_distance_mmd([rec])


def test_summary_counts_failures_and_molecules_without_pairs():
    from moleculesde_amd.conformer_mmd import summarize
    nan = float("nan")
    stats = np.array([[0.5, 0.6, 0.7, 0.8, 0.9, 2, 3],          # a full molecule
                      [0.1, 0.2, nan, nan, 0.3, 1, 1],          # E = 1: no Pair
                      [nan, nan, nan, nan, nan, 1, 0],          # no generated conformer left
                      [nan, nan, nan, nan, nan, 2, 2]])         # no evaluated pair
    res = summarize(stats, [3, 1, 3, 0])
    assert res["num_molecules"] == 4 and res["num_failed"] == 1 and res["num_without_pairs"] == 1
    assert res["mean"]["single_median"] == pytest.approx(0.3) and res["median"]["pair_mean"] == 0.8
    assert res["mean"]["all"] == pytest.approx(0.6) and res["per_molecule"]["num_pairs"] == [3, 1, 3, 0]
    assert res["per_molecule"]["num_gen_used"] == [3, 1, 0, 2]
    none = summarize(stats[2:], [3, 0])
    assert all(np.isnan(v) for v in none["mean"].values())


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_source_is_built():
    from moleculesde_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "msde_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in ("msde_conf_dist_table", "msde_conf_mmd_subsets", "msde_conf_mmd_all"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert "conformer_mmd.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "moleculesde_amd", "csrc", "conformer_mmd.hip")).read()
    from moleculesde_amd import conformer_mmd as cm
    assert int(re.search(r"#define CM_MAX_POOLED (\d+)", src).group(1)) == cm.MAX_POOLED
    assert int(re.search(r"#define CM_MAX_KERNELS (\d+)", src).group(1)) == cm.MAX_KERNELS
