"""Host side of pretraining on a molecule store (moleculesde_amd/dataset.py; no GPU): the store's round trip and validation,
the extended-edge counts, the epoch plan against bucket.raw_sizes on the collated batches, and the centring arithmetic
against the reference's fp32 `positions - positions.mean(dim=0)` (Geom3D/datasets/dataset_3D.py:120-122)."""
import numpy as np
import pytest
import torch

from dataset_cases import off_centre_molecules, path_molecule, same_molecule


def _store(sizes, seed=0):
    from moleculesde_amd.dataset import MoleculeStore
    mols = off_centre_molecules(sizes, seed)
    return mols, MoleculeStore.from_molecules(mols)


def test_store_round_trip_and_from_collated(tmp_path):
    from moleculesde_amd.dataset import MoleculeStore
    mols, store = _store([1, 2, 17, 5, 9, 14, 20, 3, 11, 8, 32, 6], seed=1)
    path = str(tmp_path / "store.pt")
    store.save(path)
    back = MoleculeStore.load(path)
    assert len(back) == 12
    for i, m in enumerate(mols):
        got = back.molecule(i, extended=True)
        assert same_molecule(got, m), i
        assert torch.equal(got.extended_edge_index, m.extended_edge_index) and got.x.dtype == torch.int64
    for k in ("x", "positions", "edge_index", "edge_attr", "atom_ptr", "bond_ptr", "ext_count"):
        assert torch.equal(getattr(back, k), getattr(store, k)) and getattr(back, k).dtype == getattr(store, k).dtype, k
    assert store.x.dtype == torch.int32 and store.atom_ptr.dtype == torch.int64 and store.positions.dtype == torch.float32
    # the collated pair of an InMemoryDataset (molecule-local edge_index), hand-built for 3 molecules
    three = mols[1:4]
    na = [m.x.size(0) for m in three]
    nb = [m.edge_index.size(1) for m in three]
    data = {"x": torch.cat([m.x for m in three]), "positions": torch.cat([m.positions for m in three]),
            "edge_index": torch.cat([m.edge_index for m in three], dim=1), "edge_attr": torch.cat([m.edge_attr for m in three])}
    sa, sb = torch.tensor([0, na[0], na[0] + na[1], sum(na)]), torch.tensor([0, nb[0], nb[0] + nb[1], sum(nb)])
    slices = {"x": sa, "positions": sa, "edge_index": sb, "edge_attr": sb}
    a, b = MoleculeStore.from_collated(data, slices), MoleculeStore.from_molecules(three)
    for k in ("x", "positions", "edge_index", "edge_attr", "atom_ptr", "bond_ptr", "ext_count"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_ext_count_is_the_extended_graph_size():
    from moleculesde_amd.batch import extend_graph_index
    from moleculesde_amd.dataset import MoleculeStore
    mols = off_centre_molecules([1, 2, 3, 17, 31, 32, 12, 12, 20], seed=2) + [path_molecule(7)]
    store = MoleculeStore.from_molecules(mols)
    for i, m in enumerate(mols):
        assert int(store.ext_count[i]) == extend_graph_index(m.edge_index, m.x.size(0)).size(1), i
    assert int(store.ext_count[-1]) == sum(1 for i in range(7) for j in range(7) if i != j and abs(i - j) <= 4)
    assert int(store.ext_count[0]) == 0


@pytest.mark.parametrize("what", ["atom_code", "bond_endpoint", "coordinate", "empty"])
def test_validation_names_the_first_offending_molecule(what):
    from moleculesde_amd.batch import MolData
    from moleculesde_amd.dataset import MoleculeStore
    mols = off_centre_molecules([4, 6, 5, 3], seed=3)
    if what == "atom_code":
        mols[2].x[1, 1] = 4                      # column 1 holds codes 0..3
    elif what == "bond_endpoint":
        mols[2].edge_index[1, 0] = 5             # a 5-atom molecule: indices 0..4
    elif what == "coordinate":
        mols[2].positions[0, 2] = float("inf")
    else:
        mols[2] = MolData(x=torch.zeros(0, 9, dtype=torch.long), edge_index=torch.zeros(2, 0, dtype=torch.long),
                          edge_attr=torch.zeros(0, 3, dtype=torch.long), positions=torch.zeros(0, 3))
    with pytest.raises(ValueError, match="molecule 2"):
        MoleculeStore.from_molecules(mols)
    if what == "empty":                          # the same through the collated pair: a repeated pointer
        good = off_centre_molecules([4, 6], seed=3)
        data = {"x": torch.cat([m.x for m in good]), "positions": torch.cat([m.positions for m in good]),
                "edge_index": torch.cat([m.edge_index for m in good], dim=1), "edge_attr": torch.cat([m.edge_attr for m in good])}
        sa = torch.tensor([0, 4, 4, 10])
        sb = torch.tensor([0, good[0].edge_index.size(1), good[0].edge_index.size(1), data["edge_index"].size(1)])
        with pytest.raises(ValueError, match="molecule 1 is empty"):
            MoleculeStore.from_collated(data, {"x": sa, "positions": sa, "edge_index": sb, "edge_attr": sb})


def test_epoch_plan_matches_raw_sizes_and_shards():
    from moleculesde_amd import bucket as BK
    from moleculesde_amd.dataset import caps_for
    sizes = np.random.default_rng(4).integers(1, 25, size=37)
    _, store = _store(sizes, seed=4)
    plan = store.epoch_plan(1, 8, seed=5)
    assert len(plan) == 5 and plan.n_full == 4 and sorted(plan.perm.tolist()) == list(range(37))
    for k in range(4):
        assert plan.need(k) == BK.raw_sizes(store.collate(plan.molecules(k))), k
    assert plan.need(4)["B"] == 5 and plan.need(4) == BK.raw_sizes(store.collate(plan.molecules(4)))
    caps = caps_for(plan)
    fits = plan.fits(caps)
    assert fits[:4].all() and not fits[4], "full batches fit their covering capacities, the short last batch never does"
    assert all(caps.fits(plan.need(k)) == bool(fits[k]) for k in range(5))
    # reproducible per (seed, epoch); epochs differ; no shuffle is the store's order
    assert np.array_equal(store.epoch_plan(1, 8, seed=5).perm, plan.perm)
    assert not np.array_equal(store.epoch_plan(2, 8, seed=5).perm, plan.perm)
    assert not np.array_equal(store.epoch_plan(1, 8, seed=6).perm, plan.perm)
    assert np.array_equal(store.epoch_plan(1, 8, shuffle=False).perm, np.arange(37))
    # two ranks: disjoint shards of equal length whose union is a prefix of the permutation
    r0, r1 = (store.epoch_plan(1, 8, seed=5, rank=r, world=2) for r in (0, 1))
    assert len(r0.perm) == len(r1.perm) == 18 and not set(r0.perm.tolist()) & set(r1.perm.tolist())
    assert set(r0.perm.tolist()) | set(r1.perm.tolist()) == set(plan.perm[:36].tolist())
    assert np.array_equal(r0.full_perm, plan.perm) and np.array_equal(r1.full_perm, plan.perm)
    assert r0.need(0) == BK.raw_sizes(store.collate(r0.molecules(0)))
    # a permutation of the caller's own is checked on the host
    with pytest.raises(ValueError, match="outside"):
        store.epoch_plan(1, 8, perm=[0, 1, 37])


def test_centring_stays_within_the_fp32_bound_and_flags_parse():
    """|centred_positions - (p - p.mean(0))| <= (n + 2) 2^-24 max|p|: sequential fp32 summation of n terms, one division, one
    subtraction on the reference's side; the store's own centre is exact to one rounding."""
    from moleculesde_amd import pretrain
    mols, store = _store([1, 2, 17, 32], seed=6)
    for i, m in enumerate(mols):
        n = m.x.size(0)
        ref = m.positions - m.positions.mean(dim=0)
        got = store.centred_positions(i)
        assert got.dtype == torch.float32 and got.shape == ref.shape
        bound = (n + 2) * 2.0 ** -24 * float(m.positions.abs().max())
        assert float(m.positions.abs().max()) > 3.0, "the molecule sits off the origin"
        assert float((got - ref).abs().max()) <= bound, (n, float((got - ref).abs().max()), bound)
        assert torch.equal(store.molecule(i, remove_center=True).positions, got)
        assert torch.equal(store.molecule(i).positions, m.positions)
    a = pretrain.main_parser().parse_args([])
    assert a.dataset_file is None and a.shuffle_seed == 0 and not a.no_shuffle and not a.keep_center
    assert a.steps_per_epoch is None
    assert not hasattr(pretrain.readme_args(), "dataset_file")
    b = pretrain.main_parser().parse_args(["--dataset_file", "s.pt", "--no_shuffle", "--keep_center", "--shuffle_seed", "3"])
    assert b.dataset_file == "s.pt" and b.no_shuffle and b.keep_center and b.shuffle_seed == 3
