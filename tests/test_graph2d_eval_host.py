"""Graph evaluation of the 3D->2D samples without a GPU (moleculesde_amd/graph2d_eval.py): the NumPy mirror the device tests
compare with on hand-computed graphs, the host tables, the argument checks, the signature -> graph conversion and the parser."""
import numpy as np
import pytest
import torch

import graph2d_eval_cases as C
from moleculesde_amd import _lib, graph2d_eval as ge
from moleculesde_amd.batch import MolData

NAMES = ge.COUNT_NAMES


def _counts(c):
    return dict(zip(NAMES, (int(v) for v in c)))


def test_mirror_four_atom_path():
    """Target 0-1-2-3 (single, double, single).  Sample: 0-1 single, 1-2 single (a wrong order), 2-3 missing, 0-3 extra; atom 2
    decoded to another class.  TP / FP / FN = 2 / 1 / 1, one order correct, 3 atoms correct, one component, not exact."""
    tgt = np.zeros((4, 4), dtype=np.uint8)
    tgt[0, 1] = tgt[1, 0] = 1
    tgt[1, 2] = tgt[2, 1] = 2
    tgt[2, 3] = tgt[3, 2] = 1
    z = np.array([5, 6, 7, 5])
    x, _ = C.target_scores(z, tgt, 10)
    x[0, 2] = 0.0
    x[0, 2, 1] = 0.3
    adj = np.zeros((1, 4, 4), dtype=np.float32)
    adj[0, 0, 1] = adj[0, 1, 0] = 1.2
    adj[0, 1, 2] = adj[0, 2, 1] = 1.4
    adj[0, 0, 3] = adj[0, 3, 0] = 0.6
    adj[0, 2, 3] = adj[0, 3, 2] = 0.4
    sig, counts, l1, _ = C.decode_sample(x[0], adj[0], z, tgt, np.ones(4, dtype=np.uint8))
    c = _counts(counts)
    assert (c["tp"], c["fp"], c["fn"]) == (2, 1, 1)
    assert c["finite"] == 1 and c["atoms_correct"] == 3 and c["order_correct"] == 1 and c["exact"] == 0
    assert c["components"] == 1 and c["valence_violations"] == 0
    assert sig.tolist() == [5, 6, 1, 5] + [1, 0, 1, 1, 0, 0]               # pairs 01 02 03 12 13 23
    assert l1 == pytest.approx(0.2 + 0.6 + 0.6 + 0.6, rel=1e-6)            # |1.2 - 1| + |0.6 - 0| + |1.4 - 2| + |0.4 - 1|
    stats, first = C.summarise(sig[None], counts[None], [l1], np.ones(4))
    assert first.tolist() == [1]
    assert stats[:9].tolist() == [0.75, 2 / 3, 2 / 3, 4 / 6, 0.5, 0.0, 1.0, 1.0, 0.0] and stats[10] == 1.0
    assert stats[9] == pytest.approx(2.0 / 6, rel=1e-6)


def test_mirror_cut_ring_and_five_bonded_carbon():
    tgt = C.ring(6, code=4)
    z = np.full(6, 5)
    x, adj = C.target_scores(z, tgt, 119)
    adj[0, 0, 1] = adj[0, 1, 0] = 0.0
    adj[0, 3, 4] = adj[0, 4, 3] = 0.2
    mv = ge.valence_table("default", 119)
    _, counts, _, _ = C.decode_sample(x[0], adj[0], z, tgt, np.ones(6, dtype=np.uint8), max_valence2=mv)
    c = _counts(counts)
    assert c["components"] == 2 and (c["tp"], c["fp"], c["fn"]) == (4, 0, 2) and c["order_correct"] == 4 and c["exact"] == 0
    assert c["atoms_correct"] == 6 and c["valence_violations"] == 0
    _, whole, _, _ = C.decode_sample(x[0], tgt.astype(np.float32), z, tgt, np.ones(6, dtype=np.uint8), max_valence2=mv)
    assert _counts(whole)["exact"] == 1 and _counts(whole)["components"] == 1
    (vx, vadj, vz, vtgt, vflag), want = C.valence_case()
    got = [_counts(C.decode_sample(vx[k], vadj[k], vz, vtgt, vflag, max_valence2=mv)[1])["valence_violations"]
           for k in range(len(want))]
    assert got == want == [0, 1, 1, 0, 1]                                  # at the cap, half a bond over, five bonds, Fe, H
    none = [_counts(C.decode_sample(vx[k], vadj[k], vz, vtgt, vflag)[1])["valence_violations"] for k in range(len(want))]
    assert none == [0] * 5


def test_mirror_flags_non_finite_quantisation_components_uniqueness():
    """Unflagged atoms are not read; a NaN on a flagged pair gives the non-finite record; the case builders' expectations hold
    for the mirror itself."""
    rng = np.random.default_rng(0)
    z, tgt, flag = C.random_graph(rng, 12, 5, bondless=2)
    assert flag.tolist() == [1] * 10 + [0] * 2
    x, adj = C.noisy_samples(rng, z, tgt, 5, 2, symmetric=False)
    ref = C.decode_sample(x[0], adj[0], z, tgt, flag)
    off = int(np.flatnonzero(flag == 0)[0])
    x2, a2 = x.copy(), adj.copy()
    x2[0, off], a2[0, off, :], a2[0, :, off] = np.nan, np.inf, -np.inf
    a2[0][np.diag_indices(12)] = np.nan                                    # the diagonal is not a pair
    got = C.decode_sample(x2[0], a2[0], z, tgt, flag)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    on = np.flatnonzero(flag)[:2]
    a3 = adj.copy()
    a3[0, on[1], on[0]] = np.nan                                           # the lower element of a flagged pair
    sig, counts, l1, _ = C.decode_sample(x[0], a3[0], z, tgt, flag)
    assert not sig.any() and np.isnan(l1)
    assert counts.tolist() == [0, 0, 0, 0, int((np.triu(tgt, 1) > 0).sum()), 0, 0, 0, 0]
    (qx, qadj, qz, qtgt, qflag), want = C.quantisation_case()
    sig = C.decode_sample(qx[0], qadj[0], qz, qtgt, qflag)[0]
    assert sig[len(qz):].tolist() == want.tolist()
    (cx, cadj, cz, ctgt, cflag), comps = C.component_case()
    assert comps == [1, 1, 1, 2, 6]
    assert [int(C.decode_sample(cx[k], cadj[k], cz, ctgt, cflag)[1][7]) for k in range(5)] == comps
    (ax, aadj, az, atgt, aflag), classes = C.argmax_case()
    assert C.decode_sample(ax[0], aadj[0], az, atgt, aflag)[0][:len(classes)].tolist() == classes
    mol, first = C.uniqueness_case()
    res = C.mirror_launch([mol])[0]
    assert res["first"].tolist() == first and res["counts"][:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]
    assert res["stats"][7] == 0.3 and res["stats"][10] == 9.0 and res["stats"][8] == 1.0
    assert res["stats"][5] == 4 / 10                                       # the four finite copies of A are exact


def test_plan_tables():
    plan = ge.Plan([3, 5, 2], [2, 1, 4], 7, "cpu")
    assert plan.G == 3 and plan.n_samples == 7 and plan.n_max == 5
    assert plan.sig_len.tolist() == [6, 15, 3]
    assert plan.mol.dtype == torch.int64 and tuple(plan.mol.shape) == (3, ge.MOL_WORDS)
    assert plan.mol.tolist() == [[3, 2, 0, 0, 0, 0, 0, 0],
                                 [5, 1, 2 * 3 * 7, 2 * 9, 3, 9, 2, 12],
                                 [2, 4, 2 * 3 * 7 + 5 * 7, 2 * 9 + 25, 8, 34, 3, 27]]
    assert plan.x_off[-1] == 42 + 35 + 56 and plan.adj_off[-1] == 18 + 25 + 16 and plan.sig_off[-1] == 12 + 15 + 12
    big = ge.Plan([70000], [3], 119, "cpu")                                # offsets are 64-bit
    assert int(big.adj_off[-1]) == 3 * 70000 * 70000 > 2 ** 31
    for bad in (([], [], 5), ([3], [1, 2], 5), ([0], [1], 5), ([3], [0], 5), ([3], [1], 0), ([3], [1], 257)):
        with pytest.raises(ValueError):
            ge.Plan(*bad, "cpu")


def test_valence_table_and_default():
    assert ge.DEFAULT_MAX_VALENCE == {1: 1, 5: 4, 6: 4, 7: 4, 8: 3, 9: 1, 14: 4, 15: 5, 16: 6, 17: 1, 35: 1, 53: 1}
    t = ge.valence_table("default", 119)
    assert t.dtype == np.uint8 and t.shape == (119,)
    assert t[0] == 2 and t[5] == 8 and t[6] == 8 and t[7] == 6 and t[15] == 12 and t[52] == 2 and t[25] == 0
    assert int((t > 0).sum()) == 12
    assert ge.valence_table(None, 119) is None
    assert ge.valence_table("default", 6).tolist() == [2, 0, 0, 0, 8, 8]   # classes past ncls are dropped
    assert ge.valence_table({6: 3}, 10).tolist() == [0, 0, 0, 0, 0, 6, 0, 0, 0, 0]
    for bad in ("rdkit", {0: 1}, {6: 0}, {6: 200}, 4):
        with pytest.raises(ValueError):
            ge.valence_table(bad, 10)


def _record(n=6, K=2, ncls=10, seed=0):
    rng = np.random.default_rng(seed)
    z, tgt, _ = C.random_graph(rng, n, ncls)
    src, dst = np.nonzero(tgt)
    ea = np.zeros((src.size, 3), dtype=np.int64)
    ea[:, 0] = tgt[src, dst].astype(np.int64) - 1
    x = np.zeros((n, 9), dtype=np.int64)
    x[:, 0] = z
    xg, ag = C.target_scores(z, tgt, ncls, K)
    return MolData(x=torch.from_numpy(x), edge_index=torch.from_numpy(np.stack([src, dst])), edge_attr=torch.from_numpy(ea),
                   x_gen=torch.from_numpy(xg), adj_gen=torch.from_numpy(ag)), z, tgt


def test_target_of_and_record_from_sample():
    rec, z, tgt = _record()
    gz, gt, gf = ge.target_of(rec)
    assert gz.tolist() == z.tolist() and np.array_equal(gt, tgt) and gf.tolist() == [1] * 6
    one_way = MolData(x=rec.x, edge_index=rec.edge_index[:, rec.edge_index[0] < rec.edge_index[1]],
                      edge_attr=rec.edge_attr[rec.edge_index[0] < rec.edge_index[1]])
    assert np.array_equal(ge.target_of(one_way)[1], tgt)                   # bonds are read as undirected
    lone = MolData(x=torch.zeros(3, 9, dtype=torch.long), edge_index=torch.tensor([[0], [1]]), edge_attr=torch.zeros(1, 3, dtype=torch.long))
    assert ge.target_of(lone)[2].tolist() == [1, 1, 0]                     # an atom without a bond is not flagged
    xp, ap = torch.randn(3, 8, 10), torch.randn(3, 8, 8)
    out = ge.record_from_sample(rec, xp, ap)
    assert tuple(out.x_gen.shape) == (3, 6, 10) and tuple(out.adj_gen.shape) == (3, 6, 6)
    assert torch.equal(out.x_gen, xp[:, :6]) and torch.equal(out.adj_gen, ap[:, :6, :6]) and torch.equal(out.edge_index, rec.edge_index)
    with pytest.raises(ValueError):
        ge.record_from_sample(rec, xp[:, :5], ap)


def test_argument_checks_and_no_cpu_path():
    rec, z, tgt = _record()
    for mb in (0, 6):
        with pytest.raises(ValueError, match="max_bond"):
            ge.evaluate_graphs([rec], max_bond=mb)
    with pytest.raises(ValueError, match="no records"):
        ge.evaluate_graphs([])
    nobond = MolData(x=rec.x, edge_index=torch.zeros(2, 0, dtype=torch.long), edge_attr=torch.zeros(0, 3, dtype=torch.long),
                     x_gen=rec.x_gen, adj_gen=rec.adj_gen)
    with pytest.raises(ValueError, match="no flagged atom"):
        ge.evaluate_graphs([rec, nobond])
    wrong = MolData(x=rec.x, edge_index=rec.edge_index, edge_attr=rec.edge_attr, x_gen=rec.x_gen, adj_gen=rec.adj_gen[:, :5, :5])
    with pytest.raises(ValueError, match="record 0"):
        ge.evaluate_graphs([wrong])
    other, _, _ = _record(ncls=11)
    with pytest.raises(ValueError, match="classes"):
        ge.evaluate_graphs([rec, other])
    hot = MolData(x=rec.x, edge_index=rec.edge_index, edge_attr=rec.edge_attr + 5, x_gen=rec.x_gen, adj_gen=rec.adj_gen)
    with pytest.raises(ValueError, match="bond types"):
        ge.evaluate_graphs([hot])
    with pytest.raises(_lib.MsdeHipError):                                 # no CPU path
        ge.evaluate_graphs([rec], device="cpu")
    n, K = [6], [2]
    args = (rec.x_gen, rec.adj_gen, torch.from_numpy(z), torch.from_numpy(tgt), torch.ones(6, dtype=torch.uint8), n, K)
    with pytest.raises(_lib.MsdeHipError):
        ge.decode(*args)
    with pytest.raises(_lib.MsdeHipError):
        ge.decode_graphs(rec.x_gen, rec.adj_gen, n, K)
    with pytest.raises(ValueError, match="max_bond"):
        ge.decode(*args, max_bond=9)
    with pytest.raises(_lib.MsdeHipError, match="1024"):
        ge.decode(torch.zeros(1025 * 3), torch.zeros(1025 * 1025), torch.zeros(1025), torch.zeros(1025 * 1025), torch.ones(1025),
                  [1025], [1])


def test_signatures_become_the_input_graph():
    """The target written as scores, decoded by the mirror and turned into graphs: the input's sorted edge list, bond types and
    classes come back, in both directions."""
    rec, z, tgt = _record(n=9, K=2, seed=3)
    res = C.mirror_launch([(rec.x_gen.numpy(), rec.adj_gen.numpy(), z, tgt, np.ones(9, dtype=np.uint8))])[0]
    plan = ge.Plan([9], [2], 10, "cpu")
    graphs = ge.graphs_from_signatures(res["sig"].reshape(-1), plan)
    assert len(graphs) == 1 and len(graphs[0]) == 2
    order = np.lexsort((rec.edge_index[1].numpy(), rec.edge_index[0].numpy()))
    for g in graphs[0]:
        assert torch.equal(g.edge_index, rec.edge_index[:, order])
        assert torch.equal(g.edge_attr[:, 0], rec.edge_attr[order, 0]) and not g.edge_attr[:, 1:].any()
        assert g.x[:, 0].tolist() == z.tolist() and tuple(g.x.shape) == (9, 9) and g.num_nodes == 9
    assert res["counts"][:, 6].tolist() == [1, 1] and res["first"].tolist() == [1, 0]


def test_summarize_and_parser():
    stats = np.array([[0.5, 1, 1, 1, 1, 0.5, 1, 0.5, 1, 0.25, 2], [0.0] * 9 + [np.nan, 0], [1.0, 0.5, 0.5, 0.5, 1, 0, 0, 1, 0, 0.75, 4]])
    res = ge.summarize(stats)
    assert res["num_molecules"] == 3 and res["num_failed"] == 1 and res["per_molecule"]["num_finite"] == [2, 0, 4]
    assert res["mean"]["atom_accuracy"] == 0.75 and res["median"]["adj_l1"] == 0.5 and res["mean"]["any_exact"] == 0.5
    assert set(res["mean"]) == set(ge.STAT_NAMES)
    dead = ge.summarize(stats[1:2])
    assert dead["num_failed"] == 1 and all(np.isnan(v) for v in dead["mean"].values())
    a = ge._parser().parse_args(["samples.pkl"])
    assert a.samples == "samples.pkl" and a.max_bond == 4 and not a.no_valence and not a.per_molecule
    a = ge._parser().parse_args(["s.pkl", "--max_bond", "5", "--no_valence", "--per_molecule"])
    assert a.max_bond == 5 and a.no_valence and a.per_molecule
