"""Sub-graph masking (--SSL_masking_ratio), host side: the kept-atom count of Geom3D/datasets/dataset_3D.py:56-62, the BFS
draw of bfs_keep (the mirror of csrc/dataset.hip), the masked molecule with its INDUCED extended edges, the masked epoch
plan's needs and the parser.  No GPU."""
import numpy as np
import pytest
import torch

from dataset_cases import path_molecule
from dataset_mask_cases import B, BONDLESS5, PATH6, STAR7, TRIANGLES, bits, mask_store
from moleculesde_amd import bucket as BK
from moleculesde_amd.batch import extend_graph_index
from moleculesde_amd.dataset import MoleculeStore, bfs_keep, keep_counts


@pytest.fixture(scope="module")
def store():
    return mask_store()


def test_keep_counts_are_the_scripts_sub_num_plus_one():
    for r in (0.15, 0.5, 0.97):
        got = keep_counts(r, 64)
        assert got.dtype == np.int32 and len(got) == 65
        for n in range(1, 65):
            assert got[n] == min(n, int(n * (1 - r)) + 1), (r, n)
    assert keep_counts(0.15)[20] == 18 and keep_counts(0.5)[8] == 5 and keep_counts(0.97)[32] == 1     # sub_num + 1
    assert len(keep_counts(0.15)) == 33
    assert all(keep_counts(0.01)[n] == n for n in range(1, 33))


def test_bfs_on_a_path_keeps_one_contiguous_run_and_reaches_every_run():
    st = MoleculeStore.from_molecules([path_molecule(8)])
    k = int(keep_counts(0.5)[8])
    assert k == 5
    runs = {((1 << k) - 1) << lo for lo in range(8 - k + 1)}
    seen = {bfs_keep(st, 0.5, 7, e)[0] for e in range(4000)}
    assert seen <= runs, sorted(bits(w) for w in seen - runs)[:3]     # BFS keeps a connected molecule connected
    assert seen == runs


def test_empty_frontier_branch_on_bondless_and_disconnected_molecules(store):
    kc = keep_counts(0.15)
    for e in range(64):
        w5, wt = bfs_keep(store, 0.15, 3, e, [BONDLESS5, TRIANGLES])
        assert bin(w5).count("1") == kc[5] == 5 and w5 >> 5 == 0      # no bond at all: every draw is over the unkept atoms
        assert bin(wt).count("1") == kc[6] == 6 and wt == 0b111111    # the second triangle is reached only through that branch
    for e in range(64):
        wt = bfs_keep(store, 0.5, 3, e, [TRIANGLES])[0]
        assert bin(wt).count("1") == keep_counts(0.5)[6] == 4
        a, b = wt & 0b111, wt >> 3
        assert 0b111 in (a, b), bin(wt)                               # one triangle is exhausted before the other is entered
        w = bfs_keep(store, 0.5, 3, e, [STAR7])[0]
        assert bin(w).count("1") == 4 and w & 1                       # a connected star: four kept atoms include the hub


def test_masks_repeat_for_the_same_seed_and_epoch_and_change_with_the_epoch(store):
    a, b = bfs_keep(store, 0.15, 5, 1), bfs_keep(store, 0.15, 5, 1)
    assert a == b and len(a) == len(store) and all(isinstance(w, int) for w in a)
    assert bfs_keep(store, 0.15, 5, 2) != a and bfs_keep(store, 0.15, 6, 1) != a
    some = [3, PATH6, 35]
    assert bfs_keep(store, 0.15, 5, 1, some) == [a[i] for i in some]          # no dependence on the batch a molecule lands in
    n = np.diff(store.atom_ptr.numpy())
    for w, ni in zip(a, n):
        assert bin(w).count("1") == keep_counts(0.15)[ni] and w >> int(ni) == 0


def test_extended_edges_of_a_masked_molecule_are_induced_not_recomputed(store):
    keep = 0b111101                                                   # path of 6, atom 1 dropped
    d = store.molecule(PATH6, keep=keep, extended=True)
    assert d.x.size(0) == 5
    ext = {tuple(c) for c in d.extended_edge_index.t().tolist()}
    for pair in ((0, 1), (0, 2), (0, 3)):                             # original 0-2, 0-3, 0-4: joined through the dropped atom 1
        assert pair in ext and pair[::-1] in ext
    assert (0, 4) not in ext                                          # original 0-5: five bonds apart
    assert 0 not in d.edge_index.flatten().tolist()                   # atom 0 lost its only bond
    assert d.edge_index.t().tolist() == [[1, 2], [2, 3], [3, 4], [2, 1], [3, 2], [4, 3]]          # stored order, relabelled
    alone = {tuple(c) for c in extend_graph_index(d.edge_index, 5).t().tolist()}
    assert not alone & {(0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)} and alone < ext
    # rows filtered alike, a boolean row means the same as the word, the centre is over the kept atoms
    whole = store.molecule(PATH6)
    idx = [0, 2, 3, 4, 5]
    assert torch.equal(d.x, whole.x[idx]) and torch.equal(d.positions, whole.positions[idx])
    d2 = store.molecule(PATH6, keep=[True, False, True, True, True, True], extended=True, remove_center=True)
    assert torch.equal(d2.extended_edge_index, d.extended_edge_index) and torch.equal(d2.edge_attr, d.edge_attr)
    mean = whole.positions[idx].double().mean(0)
    assert torch.allclose(d2.positions.double(), whole.positions[idx].double() - mean, atol=1e-5)
    assert float(d2.positions.double().mean(0).abs().max()) < 1e-5
    for bad in (0, 1 << 6):
        with pytest.raises(ValueError):
            store.molecule(PATH6, keep=bad)


@pytest.mark.parametrize("remove_center", [True, False], ids=["centred", "raw"])
def test_full_keep_words_collate_the_whole_molecules(store, remove_center):
    """The CPU twin of tests/test_gpu_dataset_mask.py::test_full_keep_words_make_the_masked_gather_the_unmasked_one."""
    from moleculesde_amd.dataset import ext_rows_of
    n = np.diff(store.atom_ptr.numpy())
    plan = store.epoch_plan(1, B, seed=3)
    for k in range(plan.n_batches):
        mols = plan.molecules(k)
        whole = store.collate(mols, remove_center=remove_center)
        full = store.collate(mols, remove_center=remove_center, keeps=[(1 << int(n[int(m)])) - 1 for m in mols])
        assert sorted(full.tensor_keys()) == sorted(whole.tensor_keys()) and full.num_graphs == whole.num_graphs
        for key in whole.tensor_keys():
            a, b = getattr(full, key), getattr(whole, key)
            assert a.dtype == b.dtype and torch.equal(a, b), (k, key)
        rows = []                                                     # extend_graph_index of each whole molecule, as words
        for m in mols:
            d = store.molecule(int(m))
            r = [0] * d.x.size(0)
            for s, t in extend_graph_index(d.edge_index, d.x.size(0)).t().tolist():
                r[s] |= 1 << t
            rows += r
        assert [int(w) & 0xFFFFFFFF for w in ext_rows_of(full).tolist()] == rows


def test_masked_epoch_plan_needs_are_exact_for_atoms_and_bounds_for_edges(store):
    for r in (0.15, 0.5):
        plan = store.epoch_plan(2, B, seed=4, mask_ratio=r, mask_seed=9)
        whole = store.epoch_plan(2, B, seed=4)
        assert plan.n_batches == 5 and np.array_equal(plan.perm, whole.perm)
        smaller = False
        for k in range(plan.n_batches):
            keeps = plan.keeps(k)
            assert keeps == bfs_keep(store, r, 9, 2, plan.molecules(k))
            got = BK.raw_sizes(store.collate(plan.molecules(k), keeps=keeps))
            need = plan.need(k)
            for key in ("N", "P", "E_r", "B"):
                assert need[key] == got[key], (r, k, key)
            for key in ("E_b", "E_e"):
                assert need[key] >= got[key] and need[key] == whole.need(k)[key], (r, k, key)
                smaller |= need[key] > got[key]
            assert need["n_max"] == whole.need(k)["n_max"]
        assert smaller
    assert store.epoch_plan(2, B, seed=4).keeps(0) is None
    with pytest.raises(ValueError):
        store.epoch_plan(1, B, mask_ratio=1.0)


def test_parser_defaults_and_errors(capsys):
    from moleculesde_amd import pretrain
    a = pretrain.parse_main_args([])
    assert a.SSL_masking_ratio == 0 and a.mask_seed == 0
    a = pretrain.parse_main_args(["--dataset_file", "s.pt", "--SSL_masking_ratio", "0.15", "--mask_seed", "3"])
    assert a.SSL_masking_ratio == 0.15 and a.mask_seed == 3
    for argv in (["--SSL_masking_ratio", "0.15"], ["--dataset_file", "s.pt", "--SSL_masking_ratio", "1.0"],
                 ["--dataset_file", "s.pt", "--SSL_masking_ratio", "-0.1"]):
        with pytest.raises(SystemExit):
            pretrain.parse_main_args(argv)
    assert "SSL_masking_ratio" in capsys.readouterr().err
