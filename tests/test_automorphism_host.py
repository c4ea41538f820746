"""The host half of the symmetry-aware conformer evaluation, without a GPU: moleculesde_amd/automorphism.py on graphs whose
groups are known (tests/conformer_sym_cases.py), against a brute force over all permutations and, where it is installed,
networkx; the host-side checks of rmsd_matrix(permutations=...) and evaluate_conformers(symmetry=True); the parser's flags."""
import itertools

import numpy as np
import pytest
import torch

import conformer_sym_cases as S
from moleculesde_amd import _lib, conformer_eval as ce
from moleculesde_amd.automorphism import automorphisms
from moleculesde_amd.batch import MolData


@pytest.mark.parametrize("g", S.GRAPHS, ids=lambda g: g.name)
def test_group_has_the_known_size_and_every_row_is_an_automorphism(g):
    perms, truncated = S.group(g)
    assert perms.dtype == np.int32 and perms.shape == (g.count, g.n) and not truncated
    assert perms[0].tolist() == list(range(g.n))
    assert len({tuple(r) for r in perms.tolist()}) == g.count                       # rows are distinct
    assert all(S.is_automorphism(g, r) for r in perms)
    again, _ = S.group(g)
    assert np.array_equal(perms, again)                                              # a deterministic order


@pytest.mark.parametrize("g", [g for g in S.GRAPHS if g.n <= 7], ids=lambda g: g.name)
def test_group_equals_brute_force(g):
    kept = np.flatnonzero(g.keep)
    want = set()
    for image in itertools.permutations(kept.tolist()):
        row = np.arange(g.n)
        row[kept] = image
        if S.is_automorphism(g, row):
            want.add(tuple(row.tolist()))
    assert len(want) == g.count
    assert {tuple(r) for r in S.group(g)[0].tolist()} == want


def test_group_equals_networkx():
    nx = pytest.importorskip("networkx")
    from networkx.algorithms.isomorphism import GraphMatcher, categorical_edge_match, categorical_node_match
    for g in S.GRAPHS:
        G = nx.Graph()
        for a in np.flatnonzero(g.keep).tolist():
            G.add_node(a, c=int(g.atom_colour[a]))
        for (u, v), c in zip(g.bonds, g.bond_colour.tolist()):
            if g.keep[u] and g.keep[v]:
                G.add_edge(u, v, b=c)
        gm = GraphMatcher(G, G, node_match=categorical_node_match("c", None), edge_match=categorical_edge_match("b", None))
        want = set()
        for iso in gm.isomorphisms_iter():
            row = list(range(g.n))
            for u, v in iso.items():
                row[u] = v
            want.add(tuple(row))
        assert {tuple(r) for r in S.group(g)[0].tolist()} == want, g.name


def test_max_count_truncates_and_keeps_the_identity_first():
    g = next(g for g in S.GRAPHS if g.count == 864)
    perms, truncated = S.group(g, max_count=100)
    assert perms.shape == (100, 34) and truncated and perms[0].tolist() == list(range(34))
    assert np.array_equal(perms, S.group(g)[0][:100])                                # a prefix of the full enumeration
    exact, truncated = S.group(g, max_count=864)
    assert exact.shape == (864, 34) and not truncated                                # a group of exactly max_count is whole
    with pytest.raises(ValueError):
        S.group(g, max_count=0)


def test_tolerated_edge_lists():
    """One direction only, duplicates, self-loops and bonds to dropped atoms do not change the group."""
    ring = S.GRAPHS[2]
    one_way = np.asarray(ring.bonds).T
    assert automorphisms(6, one_way, ring.atom_colour, ring.bond_colour)[0].shape == (12, 6)
    messy = np.concatenate([ring.edge_index, ring.edge_index[:, :3], [[2, 4], [2, 4]]], axis=1)
    assert automorphisms(6, messy, ring.atom_colour, np.zeros(messy.shape[1]))[0].shape == (12, 6)
    star = S.GRAPHS[7]                                                               # leaf 4 is dropped: its bond is ignored
    perms, _ = S.group(star)
    assert (perms[:, 4] == 4).all() and (perms[:, 0] == 0).all() and perms.shape[0] == 6
    none, truncated = automorphisms(3, np.zeros((2, 0), dtype=np.int64), [5, 5, 5], [], keep=[0, 0, 0])
    assert none.tolist() == [[0, 1, 2]] and not truncated                            # nothing kept: the identity
    free, _ = automorphisms(3, np.zeros((2, 0), dtype=np.int64), [5, 5, 6], [])
    assert sorted(free.tolist()) == [[0, 1, 2], [1, 0, 2]]                           # no bonds: equal atoms swap
    with pytest.raises(ValueError):
        automorphisms(3, [[0], [3]], [5, 5, 5], [0])


def test_a_200_atom_molecule_stops_at_max_count_quickly():
    """Twenty three-leaf groups on a 120-atom chain: 6^20 automorphisms; the enumeration returns its first 1024."""
    import time
    bonds, nxt = [(i, i + 1) for i in range(119)], 120
    for at in range(0, 120, 6):
        bonds += [(at, nxt)] + [(nxt, nxt + 1 + j) for j in range(3)]
        nxt += 4
    g = S.Graph("chain200", 200, bonds, None)
    t = time.perf_counter()
    perms, truncated = S.group(g)
    assert perms.shape == (1024, 200) and truncated and time.perf_counter() - t < 5.0
    assert len({tuple(r) for r in perms.tolist()}) == 1024 and all(S.is_automorphism(g, r) for r in perms[::37])


# ---- rmsd_matrix(permutations=...) and evaluate_conformers(symmetry=True): what is checked before a device is needed ---------
def test_rmsd_matrix_rejects_bad_permutation_tables():
    ref, gen = torch.randn(2 * 4 + 3, 3), torch.randn(3 * 4 + 3, 3)                  # molecules of 4 and 3 atoms
    args = (ref, gen, [4, 3], [2, 1], [3, 1])
    ident = [np.arange(4)[None], np.arange(3)[None]]
    with pytest.raises(ValueError, match="permutation tables for"):
        ce.rmsd_matrix(*args, permutations=ident[:1])
    with pytest.raises(ValueError, match="molecule 1"):
        ce.rmsd_matrix(*args, permutations=[ident[0], np.arange(4)[None]])          # a row of the wrong length
    with pytest.raises(ValueError, match="molecule 0"):
        ce.rmsd_matrix(*args, permutations=[np.arange(4), ident[1]])                # not two-dimensional
    with pytest.raises(ValueError, match="molecule 0"):
        ce.rmsd_matrix(*args, permutations=[np.zeros((0, 4), dtype=np.int64), ident[1]])      # no row
    with pytest.raises(ValueError, match="molecule 0"):
        ce.rmsd_matrix(*args, permutations=[np.arange(4)[None].astype(np.float64), ident[1]])
    with pytest.raises(ValueError, match="outside"):
        ce.rmsd_matrix(*args, permutations=[np.array([[0, 1, 2, 4]]), ident[1]])
    with pytest.raises(ValueError, match="outside"):
        ce.rmsd_matrix(*args, permutations=[ident[0], np.array([[0, -1, 2]])])
    with pytest.raises(ValueError, match="bijection"):
        ce.rmsd_matrix(*args, permutations=[np.array([[0, 1, 2, 3], [0, 1, 1, 3]]), ident[1]])
    mask = torch.tensor([1, 1, 0, 1, 1, 1, 1], dtype=torch.uint8)
    with pytest.raises(ValueError, match="bijection"):                               # a kept atom sent to the dropped atom 2
        ce.rmsd_matrix(*args, atom_mask=mask, permutations=[np.array([[0, 2, 1, 3]]), ident[1]])
    with pytest.raises(ValueError, match="lds_atoms"):
        ce.rmsd_matrix(*args, permutations=ident, lds_atoms=ce.LDS_ATOMS + 1)
    with pytest.raises(_lib.MsdeHipError):                                           # valid tables: only the device is missing
        ce.rmsd_matrix(*args, atom_mask=mask, permutations=[np.array([[1, 0, 0, 3]]), ident[1]])


def test_permutation_tables_layout():
    sym, perms = ce._permutation_tables([np.array([[0, 1, 2], [2, 1, 0]]), np.array([[1, 0]])], [3, 2], None)
    assert sym.dtype == np.int64 and sym.tolist() == [[2, 0], [1, 6]]
    assert perms.dtype == np.int32 and perms.tolist() == [0, 1, 2, 2, 1, 0, 1, 0]


def _record(g, K=2):
    x = torch.zeros(g.n, 9, dtype=torch.long)
    x[:, 0] = torch.from_numpy(g.atom_colour)
    attr = torch.zeros(2 * len(g.bonds), 3, dtype=torch.long)
    attr[:, 0] = torch.from_numpy(g.edge_colour)
    return MolData(x=x, edge_index=torch.from_numpy(g.edge_index), edge_attr=attr, positions=torch.randn(g.n, 3),
                   pos_gen=torch.randn(K * g.n, 3), num_pos_gen=torch.tensor([K]), finite=True)


def test_groups_of_records_follow_the_evaluated_atoms():
    recs = [_record(g) for g in S.GRAPHS]
    perms, truncated = ce._groups(recs, True, 1024)
    assert [p.shape[0] for p in perms] == [g.count for g in S.GRAPHS] and truncated == 0
    perms, truncated = ce._groups(recs, False, 1024)                                 # all atoms: the masked leaf is an atom of
    assert perms[7].shape[0] == 6 and truncated == 0                                 # another colour, the group is the same
    perms, truncated = ce._groups(recs, True, 100)
    assert [p.shape[0] for p in perms] == [min(g.count, 100) for g in S.GRAPHS] and truncated == 1


def test_symmetry_needs_the_graph_of_every_record():
    recs = [_record(S.GRAPHS[0]), _record(S.GRAPHS[1])]
    del recs[1].edge_index
    with pytest.raises(ValueError, match="record 1"):
        ce.evaluate_conformers(recs, symmetry=True)
    with pytest.raises(_lib.MsdeHipError):                                           # the plain mode never looks at the graph
        ce.evaluate_conformers(recs, device="cpu")


def test_cli_parser_symmetry_flags():
    a = ce._parser().parse_args(["s.pkl"])
    assert a.symmetry is False and a.max_automorphisms == 1024
    a = ce._parser().parse_args(["s.pkl", "--symmetry", "--max_automorphisms", "64"])
    assert a.symmetry is True and a.max_automorphisms == 64
