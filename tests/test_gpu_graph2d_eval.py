"""Graph evaluation of the 3D->2D samples on the GPU (moleculesde_amd/graph2d_eval.py; csrc/graph2d_eval.hip:
msde_graph2d_decode, msde_graph2d_summary) against the NumPy mirror of tests/graph2d_eval_cases.py.

Every integer output (signatures, the nine counts, `first`) and every ratio of the summary is compared EXACTLY: the mirror
forms them from the same fp64 operations in the same order.  Only sum |v - t| is a long fp64 sum; the kernel's value is
compared with the mirror's math.fsum within n_pairs * 2^-53 * sum |v - t| -- (n_pairs - 1) roundings of the running sum plus the
one of fsum, first order in 2^-53: derived, not measured (achieved: the sums are equal; sums of a few thousand differences of
24-bit numbers are exact in fp64).  All molecules but one have at most 100 atoms: the file takes seconds."""
import pickle

import numpy as np
import pytest
import torch

import graph2d_eval_cases as C
from helpers import record_parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _launch(dev, mols, max_bond=4, mv=None):
    """Both kernels on one launch of molecules (tuples of graph2d_eval_cases): per molecule what mirror_launch returns."""
    from moleculesde_amd import graph2d_eval as ge
    n, K = [m[2].shape[0] for m in mols], [m[0].shape[0] for m in mols]
    cat = lambda j, dt: torch.from_numpy(np.concatenate([np.asarray(m[j]).reshape(-1) for m in mols]).astype(dt)).to(dev)
    dec = ge.decode(cat(0, np.float32), cat(1, np.float32), cat(2, np.int32), cat(3, np.uint8), cat(4, np.uint8), n, K,
                    max_bond=max_bond, max_valence2=mv, ncls=mols[0][0].shape[2])
    stats, first = ge.summary(dec)
    torch.cuda.synchronize()
    p = dec.plan
    sig, counts, l1 = dec.sig.cpu().numpy(), dec.counts.cpu().numpy(), dec.adj_l1.cpu().numpy()
    stats, first = stats.cpu().numpy(), first.cpu().numpy()
    out = []
    for g in range(p.G):
        s0, s1 = int(p.samp_off[g]), int(p.samp_off[g + 1])
        out.append(dict(sig=sig[int(p.sig_off[g]):int(p.sig_off[g + 1])].reshape(K[g], -1), counts=counts[s0:s1], l1=l1[s0:s1],
                        stats=stats[g], first=first[s0:s1]))
    return out


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("sig", "counts", "first")) and \
        all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in ("l1", "stats"))


def _check(got, want, flags, what):
    """Exact on everything but the fp64 sums; returns the worst |adj_l1 - fsum| / bound met."""
    worst = 0.0
    for g, (a, w) in enumerate(zip(got, want)):
        assert np.array_equal(a["sig"], w["sig"]), (what, g)
        assert np.array_equal(a["counts"], w["counts"]), (what, g, a["counts"], w["counts"])
        assert np.array_equal(a["first"], w["first"]), (what, g)
        assert np.array_equal(a["stats"][:9], w["stats"][:9]) and a["stats"][10] == w["stats"][10], (what, g, a["stats"], w["stats"])
        nf = int((flags[g] != 0).sum())
        pairs = nf * (nf - 1) // 2
        fin = w["counts"][:, 0] != 0
        assert np.isnan(a["l1"][~fin]).all(), (what, g)
        bound = pairs * U * w["l1_abs"][fin]
        err = np.abs(a["l1"][fin] - w["l1"][fin])
        assert (err <= bound).all(), (what, g, err, bound)
        if fin.any():
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            # the mean: the samples' bounds, K roundings of their sum, two divisions
            mean_bound = (bound.sum() + fin.sum() * U * w["l1_abs"][fin].sum()) / fin.sum() / max(pairs, 1) + 4 * U * abs(w["stats"][9])
            assert abs(a["stats"][9] - w["stats"][9]) <= mean_bound, (what, g)
        else:
            assert np.isnan(a["stats"][9]), (what, g)
    return worst


@pytest.fixture(scope="module")
def ragged(dev):
    """The six ragged launches (one per class count; nine molecules of 2 .. 100 atoms, K in {1, 2, 10, 65} each), their device
    results and the mirror's, computed once."""
    from moleculesde_amd import graph2d_eval as ge
    out = {}
    for ncls in C.CLASSES:
        mols = C.ragged_case(ncls, seed=100 + ncls)
        mv = ge.valence_table("default", ncls)
        out[ncls] = dict(mols=mols, mv=mv, got=_launch(dev, mols, mv=mv), want=C.mirror_launch(mols, max_valence2=mv))
    return out


def test_every_size_class_count_and_sample_count_matches_the_mirror(ragged):
    seen_n, seen_K, worst, wrong, broken = set(), set(), 0.0, 0, 0
    for ncls, r in ragged.items():
        worst = max(worst, _check(r["got"], r["want"], [m[4] for m in r["mols"]], ncls))
        for m, w in zip(r["mols"], r["want"]):
            seen_n.add(m[2].shape[0]); seen_K.add(m[0].shape[0])
            wrong += int((w["counts"][:, 6] == 0).sum()); broken += int((w["counts"][:, 7] > 1).sum())
    assert seen_n == set(C.SIZES) and seen_K == set(C.SAMPLES)
    assert wrong > 0 and broken > 0                                  # the noise does make wrong and disconnected graphs
    record_parity("graph2d_eval: 6 ragged launches (ncls in %s; n in %s; K in %s): every integer output and ratio equal to the "
                  "NumPy mirror; adj_l1 vs math.fsum: worst |err| / (n_pairs 2^-53 sum|v - t|) = %.3g (bound: 1)"
                  % (list(C.CLASSES), list(C.SIZES), list(C.SAMPLES), worst))


def test_ragged_launch_equals_single_launches_and_itself_bitwise(dev, ragged):
    r = ragged[119]
    for g, m in enumerate(r["mols"]):
        alone = _launch(dev, [m], mv=r["mv"])
        assert _same_bits(alone[0], r["got"][g]), g
    again = _launch(dev, r["mols"], mv=r["mv"])
    assert all(_same_bits(a, b) for a, b in zip(again, r["got"]))
    back = _launch(dev, r["mols"][::-1], mv=r["mv"])[::-1]           # other offsets, other workgroups: the same bits
    assert all(_same_bits(a, b) for a, b in zip(back, r["got"]))


def test_argmax_ties_and_all_negative_rows(dev):
    mol, want = C.argmax_case()
    got = _launch(dev, [mol])[0]
    assert got["sig"][0, :len(want)].tolist() == want == [17, 0, 63, 5, 1, 129, 0, 65]
    assert got["counts"][0, 1] == len(want) and got["counts"][0, 6] == 1
    _check([got], C.mirror_launch([mol]), [mol[4]], "argmax")
    x, adj, z, tgt, flag = mol
    one = (np.full((2, len(z), 1), -3.0, dtype=np.float32), np.repeat(adj, 2, axis=0), np.zeros_like(z), tgt, flag)     # ncls = 1
    got = _launch(dev, [one])[0]
    assert not got["sig"][:, :len(z)].any() and got["counts"][:, 6].tolist() == [1, 1] and got["first"].tolist() == [1, 0]


@pytest.mark.parametrize("max_bond", [4, 2, 5, 1])
def test_quantisation_boundaries(dev, max_bond):
    mol, want = C.quantisation_case()
    got = _launch(dev, [mol], max_bond=max_bond)[0]
    n = len(mol[2])
    if max_bond == 4:
        assert got["sig"][0, n:].tolist() == want.tolist()
    else:
        assert got["sig"][0, n:].max() == max_bond
    _check([got], C.mirror_launch([mol], max_bond=max_bond), [mol[4]], max_bond)


def test_components_of_long_paths(dev):
    mol, want = C.component_case()
    got = _launch(dev, [mol])[0]
    assert got["counts"][:, 7].tolist() == want == [1, 1, 1, 2, 6]
    assert got["counts"][:, 0].tolist() == [1] * 5 and got["counts"][0, 6] == 1
    _check([got], C.mirror_launch([mol]), [mol[4]], "components")


def test_largest_supported_molecule(dev):
    """n = 1024, the bound of the labels in LDS: a path along 0, 1, ..., 1021 (the lowest label has 1021 bonds to travel) whose
    middle bond the second sample loses, the last two atoms bond-less; next to a 2-atom molecule in the same launch."""
    n = 1024
    tgt = np.zeros((n, n), dtype=np.uint8)
    a = np.arange(n - 3)
    tgt[a, a + 1] = tgt[a + 1, a] = 1
    z = np.arange(n) % 2
    flag = (tgt.sum(1) > 0).astype(np.uint8)
    assert flag.sum() == n - 2
    x, adj = C.target_scores(z, tgt, 2, 2)
    adj[1, 500, 501] = adj[1, 501, 500] = 0.3
    small = C.target_scores(np.array([0, 1]), C.path([0, 1]), 2, 1) + (np.array([0, 1]), C.path([0, 1]), np.ones(2, dtype=np.uint8))
    mols = [small, (x, adj, z, tgt, flag)]
    got = _launch(dev, mols)
    assert got[1]["counts"][:, 7].tolist() == [1, 2] and got[1]["counts"][:, 6].tolist() == [1, 0]
    assert got[1]["counts"][:, 2].tolist() == [n - 3, n - 4] and got[1]["first"].tolist() == [1, 1]
    _check(got, C.mirror_launch(mols), [m[4] for m in mols], "n = 1024")


def test_valence_at_the_cap_and_over(dev):
    from moleculesde_amd import graph2d_eval as ge
    mol, want = C.valence_case()
    mv = ge.valence_table("default", 119)
    got = _launch(dev, [mol], mv=mv)[0]
    assert got["counts"][:, 8].tolist() == want == [0, 1, 1, 0, 1]
    _check([got], C.mirror_launch([mol], max_valence2=mv), [mol[4]], "valence")
    assert not _launch(dev, [mol])[0]["counts"][:, 8].any()          # no table: nothing is checked


def test_uniqueness(dev):
    mol, want = C.uniqueness_case()
    got = _launch(dev, [mol])[0]
    assert got["first"].tolist() == want and got["stats"][7] == 0.3 and got["stats"][10] == 9.0
    assert got["counts"][:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]
    _check([got], C.mirror_launch([mol]), [mol[4]], "unique")


def test_non_finite_values(dev, ragged):
    """A NaN / inf in a sample changes that sample's record (and its molecule's summary) only; on unflagged atoms, on their rows
    and columns of the adjacency and on the diagonal it changes nothing."""
    r = ragged[65]
    mols = [tuple(np.array(a, copy=True) for a in m) for m in r["mols"]]
    flagged = lambda g: np.flatnonzero(mols[g][4])
    g1, g2 = 3, 8                                                    # n = 32 and n = 100
    k1, k2 = mols[g1][0].shape[0] - 1, 1
    mols[g1][0][k1, flagged(g1)[-1], 64] = np.nan                    # the last class of the last flagged atom of the last sample
    i, j = flagged(g2)[[1, -1]]
    mols[g2][1][k2, j, i] = -np.inf                                  # the lower element of a flagged pair
    got = _launch(dev, mols, mv=r["mv"])
    want = C.mirror_launch(mols, max_valence2=r["mv"])
    _check(got, want, [m[4] for m in mols], "nan")
    for g in range(len(mols)):
        if g not in (g1, g2):
            assert _same_bits(got[g], r["got"][g]), g
            continue
        bad = k1 if g == g1 else k2
        keep = [k for k in range(mols[g][0].shape[0]) if k != bad]
        assert got[g]["counts"][bad, 0] == 0 and np.isnan(got[g]["l1"][bad]) and not got[g]["sig"][bad].any()
        assert got[g]["counts"][bad, 4] == r["got"][g]["counts"][bad, 2] + r["got"][g]["counts"][bad, 4]      # fn = the true bonds
        for key in ("sig", "counts"):
            assert np.array_equal(got[g][key][keep], r["got"][g][key][keep]), (g, key)
        assert np.array_equal(got[g]["l1"][keep].view(np.int64), r["got"][g]["l1"][keep].view(np.int64))
        assert got[g]["stats"][10] == r["got"][g]["stats"][10] - 1
    clean = [tuple(np.array(a, copy=True) for a in m) for m in r["mols"]]
    hit = 0
    for x, adj, z, tgt, flag in clean:
        off = np.flatnonzero(flag == 0)
        x[:, off] = np.nan
        adj[:, off, :] = np.inf
        adj[:, :, off] = -np.inf
        adj[:, np.arange(len(z)), np.arange(len(z))] = np.nan
        hit += len(off)
    assert hit >= 2
    got = _launch(dev, clean, mv=r["mv"])
    assert all(_same_bits(a, b) for a, b in zip(got, r["got"]))


def test_unsupported_and_invalid_arguments(dev):
    """The C entry points' own refusals (the Python wrapper raises before it calls): n_max above 1024 and ncls above 256 are
    MSDE_EUNSUP, max_bond outside 1..5 and null pointers MSDE_EINVAL; nothing is launched."""
    import ctypes
    from moleculesde_amd import _lib
    from moleculesde_amd._torchabi import _p, _stream
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int64, device=dev)
    call = lambda n_max, ncls, max_bond, first=t: lib.msde_graph2d_decode(
        _p(first), _p(t), _p(t), _p(t), _p(t), _p(None), _p(t), 1, ctypes.c_longlong(1), n_max, ncls, max_bond, _p(t), _p(t), _p(t),
        _stream())
    assert call(1025, 5, 4) == -2 and call(8, 257, 4) == -2
    assert call(8, 5, 0) == -1 and call(8, 5, 6) == -1 and call(8, 5, 4, None) == -1 and call(0, 5, 4) == -1
    assert lib.msde_graph2d_summary(_p(t), _p(t), _p(t), _p(t), _p(t), 0, _p(t), _p(t), _stream()) == -1
    torch.cuda.synchronize()


def _records(mols, ncls):
    """Records of evaluate_graphs from case molecules (bond-less atoms keep their class and lose their edges)."""
    from moleculesde_amd.batch import MolData
    out = []
    for x, adj, z, tgt, flag in mols:
        src, dst = np.nonzero(tgt)
        ea = np.zeros((src.size, 3), dtype=np.int64)
        ea[:, 0] = tgt[src, dst].astype(np.int64) - 1
        xx = np.zeros((len(z), 9), dtype=np.int64)
        xx[:, 0] = z
        out.append(MolData(x=torch.from_numpy(xx), edge_index=torch.from_numpy(np.stack([src, dst]).astype(np.int64)),
                           edge_attr=torch.from_numpy(ea), x_gen=torch.from_numpy(x), adj_gen=torch.from_numpy(adj)))
    return out


def _compare_summary(res, want, names):
    """evaluate_graphs' dictionary against the mirror's per-molecule stats: exact but for adj_l1 (checked by _check elsewhere)."""
    stats = np.stack([w["stats"] for w in want])
    for j, name in enumerate(names):
        if name != "adj_l1":
            assert res["per_molecule"][name] == stats[:, j].tolist(), name
    assert res["per_molecule"]["num_finite"] == [int(v) for v in stats[:, 10]]
    ok = stats[:, 10] > 0
    assert res["num_failed"] == int((~ok).sum()) and res["num_molecules"] == len(want)
    for key, f in (("mean", np.mean), ("median", np.median)):
        for j, name in enumerate(names):
            assert res[key][name] == pytest.approx(float(f(stats[ok, j])), rel=1e-12), (key, name)


def test_oracle_sample_and_evaluate_graphs(dev, ragged, tmp_path):
    """The target graph written as scores: exact, one component, accuracy 1, unique 1 / K; decode_graphs returns the input's
    sorted edge list.  evaluate_graphs on the noisy ragged molecules (from a list and from a pickle) equals the mirror, with the
    default valence table, without it, and with a molecule that has no finite sample."""
    from moleculesde_amd import _lib, graph2d_eval as ge
    rng = np.random.default_rng(8)
    mols = []
    for n, K in ((2, 1), (17, 3), (33, 2)):
        z, tgt, flag = C.random_graph(rng, n, 119, bondless=1 if n == 33 else 0)
        mols.append(C.target_scores(z, tgt, 119, K) + (z, tgt, flag))
    recs = _records(mols, 119)
    res = ge.evaluate_graphs(recs, max_valence=None)
    pm = res["per_molecule"]
    for name in ("atom_accuracy", "bond_precision", "bond_recall", "bond_f1", "bond_order_accuracy", "exact_match", "valid", "any_exact"):
        assert pm[name] == [1.0, 1.0, 1.0], name
    assert pm["unique"] == [1.0, 1 / 3, 0.5] and pm["adj_l1"] == [0.0, 0.0, 0.0] and pm["num_finite"] == [1, 3, 2]
    assert res["num_failed"] == 0 and res["max_bond"] == 4 and res["mean"]["exact_match"] == 1.0
    n, K = [m[2].shape[0] for m in mols], [m[0].shape[0] for m in mols]
    graphs = ge.decode_graphs(torch.cat([r.x_gen.reshape(-1) for r in recs]).to(dev),
                              torch.cat([r.adj_gen.reshape(-1) for r in recs]).to(dev), n, K,
                              atom_flag=torch.from_numpy(np.concatenate([m[4] for m in mols])).to(dev))
    for rec, m, gs in zip(recs, mols, graphs):
        assert len(gs) == m[0].shape[0]
        for g in gs:
            assert torch.equal(g.edge_index, rec.edge_index) and torch.equal(g.edge_attr[:, 0], rec.edge_attr[:, 0])
            assert g.x[:, 0].tolist() == np.where(m[4] != 0, m[2], 0).tolist()
    with pytest.raises(_lib.MsdeHipError):
        ge.decode_graphs(recs[0].x_gen.reshape(-1), recs[0].adj_gen.reshape(-1).to(dev), n[:1], K[:1])
    # the noisy molecules of the 119-class launch; the third molecule loses every sample
    r = ragged[119]
    noisy = [tuple(np.array(a, copy=True) for a in m) for m in r["mols"][:5]]
    noisy[2][0][:, 0, 0] = np.inf
    recs = _records(noisy, 119)
    path = tmp_path / "samples.pkl"
    with open(path, "wb") as f:
        pickle.dump(recs, f)
    for mv in ("default", None):
        want = C.mirror_launch(noisy, max_valence2=ge.valence_table(mv, 119))
        for src in (recs, str(path)):
            res = ge.evaluate_graphs(src, max_valence=mv)
            _compare_summary(res, want, ge.STAT_NAMES)
            assert res["num_failed"] == 1 and res["per_molecule"]["num_finite"][2] == 0 and np.isnan(res["per_molecule"]["adj_l1"][2])
    assert ge.main([str(path), "--no_valence"]) == 0


def test_sampler_output_end_to_end(dev, tmp_path):
    """Three molecules (one with a bond-less atom) through generate_graphs_from_testset on a small untrained base model -- built
    as tests/test_gpu_sampler_3d2d.py builds it -- with a five-step schedule, the pickle read back, evaluate_graphs against the
    mirror on the same tensors; a molecule's samples do not depend on where the loop starts."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import graph2d_eval as ge
    from moleculesde_amd.synthetic import make_molecule
    from test_gpu_sampler_3d2d import _model
    torch.manual_seed(0)
    sch = G.SchNet(hidden_channels=64, num_filters=128, num_interactions=1, num_gaussians=51, cutoff=10, readout="mean",
                   node_class=119).to(dev)
    m = _model("VE", 64, 0.1, 1.0, dev)
    rng = np.random.default_rng(6)
    mols = [make_molecule(rng, n) for n in (7, 12, 9)]
    last = mols[1].num_nodes - 1
    keep = (mols[1].edge_index[0] != last) & (mols[1].edge_index[1] != last)
    mols[1].edge_index, mols[1].edge_attr = mols[1].edge_index[:, keep], mols[1].edge_attr[keep]
    kw = dict(num_repeat=3, noise_seed=7, num_steps=5, use_graph=False)
    recs = ge.generate_graphs_from_testset(mols, sch, m, start=0, end=3, out_path=str(tmp_path), **kw)
    files = list(tmp_path.iterdir())
    assert len(recs) == 3 and len(files) == 1
    with open(files[0], "rb") as f:
        back = pickle.load(f)
    for a, b, mol in zip(recs, back, mols):
        assert torch.equal(a.x_gen, b.x_gen) and torch.equal(a.adj_gen, b.adj_gen) and torch.equal(b.edge_index, mol.edge_index)
        assert tuple(b.x_gen.shape) == (3, mol.num_nodes, m.num_class_X) and tuple(b.adj_gen.shape) == (3, mol.num_nodes, mol.num_nodes)
    assert not back[1].x_gen[:, last].any() and not back[1].adj_gen[:, last].any()       # the sampler masks the bond-less atom
    case = []
    for rec in back:
        z, tgt, flag = ge.target_of(rec)
        case.append((rec.x_gen.numpy(), rec.adj_gen.numpy(), z, tgt, flag))
    assert case[1][4].tolist() == [1] * last + [0]
    ncls = m.num_class_X
    want = C.mirror_launch(case, max_valence2=ge.valence_table("default", ncls))
    res = ge.evaluate_graphs(str(files[0]))
    _compare_summary(res, want, ge.STAT_NAMES)
    got = _launch(dev, case, mv=ge.valence_table("default", ncls))
    _check(got, want, [c[4] for c in case], "sampler")
    alone = ge.generate_graphs_from_testset(mols, sch, m, start=1, end=2, **kw)
    assert len(alone) == 1 and torch.equal(alone[0].x_gen, recs[1].x_gen) and torch.equal(alone[0].adj_gen, recs[1].adj_gen)
