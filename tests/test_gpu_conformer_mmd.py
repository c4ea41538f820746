"""Distance-distribution MMD on the GPU (moleculesde_amd/conformer_mmd.py; csrc/conformer_mmd.hip: msde_conf_dist_table,
msde_conf_mmd_subsets, msde_conf_mmd_all) against the fp64 NumPy mirror of tests/conformer_mmd_cases.py.

Tolerance of every comparison with the mirror: per statistic 8 x the largest |fp32 mirror - fp64 mirror| over the case set,
computed on the host (conformer_mmd_cases.tolerances; about 2e-6 to 6e-6 on statistics of size 0.4 to 6).  mmd_statistics
NaN-fills every fp64 output buffer before its launches.  Molecules of 3 to 9 atoms and at most 132 pooled conformers, but for
one 3-atom molecule at the limit of 1024: the whole file takes seconds."""
import json

import numpy as np
import pytest
import torch

import conformer_mmd_cases as C
from helpers import record_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def tol():
    return C.tolerances()[0]


def _launch(dev, cases, **kw):
    """One launch over molecules given as case dictionaries (ref [R, n, 3], gen [K, n, 3], keep bool [n] or None, pairs in the
    evaluated-atom numbering): per molecule {"single", "pair", "stats" [7], "finite"} as host arrays."""
    from moleculesde_amd import conformer_mmd as cm
    n = [c["ref"].shape[1] for c in cases]
    R = [c["ref"].shape[0] for c in cases]
    K = [c["gen"].shape[0] for c in cases]
    ref = torch.from_numpy(np.concatenate([c["ref"].reshape(-1, 3) for c in cases])).to(dev)
    gen = torch.from_numpy(np.concatenate([c["gen"].reshape(-1, 3) for c in cases])).to(dev)
    mask = None
    if any(c["keep"] is not None for c in cases):
        mask = torch.from_numpy(np.concatenate([np.ones(m, dtype=bool) if c["keep"] is None else c["keep"]
                                                for c, m in zip(cases, n)])).to(dev)
    pairs = np.concatenate([c["pairs"].reshape(-1, 2) for c in cases])
    ptr = np.concatenate([[0], np.cumsum([c["pairs"].shape[0] for c in cases])])
    out = cm.mmd_statistics(ref, gen, n, R, K, pairs, ptr, atom_mask=mask, **kw)
    torch.cuda.synchronize()
    single, pair, stats, fin = (out[k].cpu().numpy() for k in ("single", "pair", "stats", "finite"))
    so, po, co = out["single_off"].tolist(), out["pair_off"].tolist(), np.concatenate([[0], np.cumsum(np.add(R, K))])
    assert so == ptr.tolist() and stats.shape == (len(cases), 7)
    return [{"single": single[so[g]:so[g + 1]], "pair": pair[po[g]:po[g + 1]], "stats": stats[g], "finite": fin[co[g]:co[g + 1]]}
            for g in range(len(cases))]


def _bits(r):
    return np.concatenate([r["single"], r["pair"], r["stats"]]).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _close(got, want, tol):
    """Worst |got - want| per statistic and per item array, with NaN required exactly where the mirror has NaN."""
    worst = {}
    for i, k in enumerate(C.STATS):
        assert np.isnan(got["stats"][i]) == np.isnan(want["stats"][i]), k
        worst[k] = 0.0 if np.isnan(want["stats"][i]) else float(abs(got["stats"][i] - want["stats"][i]))
    assert got["stats"][5:].tolist() == want["stats"][5:].tolist()
    for k in ("single", "pair"):
        assert got[k].shape == want[k].shape and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        worst[k + "_items"] = float(np.abs(got[k] - want[k]).max()) if want[k].size and not np.isnan(want[k]).any() else 0.0
    for k, v in worst.items():
        assert v <= tol[k], (k, v, tol[k])
    return worst


@pytest.fixture(scope="module")
def suite(dev):
    """The case set in ONE ragged launch (it mixes every shape), and the mirrors."""
    ref = C.suite_reference()
    names = list(ref)
    return names, [ref[k][0] for k in names], _launch(dev, [ref[k][0] for k in names]), [ref[k][1] for k in names]


def test_every_shape_matches_the_fp64_mirror(suite, tol):
    names, _, got, want = suite
    bound, f32 = C.tolerances()
    worst = {k: 0.0 for k in bound}
    for name, g, w in zip(names, got, want):
        for k, v in _close(g, w, tol).items():
            worst[k] = max(worst[k], v)
    record_parity("conformer_mmd: device vs fp64 NumPy mirror over %s" % ", ".join(names))
    for k in bound:
        record_parity("conformer_mmd:   %-14s device max |err| %.2e   fp32 mirror %.2e   bound 8 x that = %.2e"
                      % (k, worst[k], f32[k], bound[k]))
    e1 = got[names.index("r1k1_e1")]
    assert e1["pair"].size == 0 and np.isnan(e1["stats"][2:4]).all()           # E = 1: Pair is NaN
    assert abs(e1["stats"][4] - 6.18627638) < 1e-5                              # and the closed form of R = K = E = 1
    assert got[names.index("r5k70_e7")]["pair"].size == 21


def test_each_case_alone_and_the_other_exponential_path(dev, suite, tol):
    """Single-molecule launches equal the ragged launch bitwise; kernel_num exponentials instead of one and squarings stay
    inside the tolerance; another kernel_mul / kernel_num follows the mirror."""
    names, cases, got, want = suite
    for c, g, w in zip(cases, got, want):
        assert _same_bits(_launch(dev, [c])[0], g)
        _close(_launch(dev, [c], exp_path=1)[0], w, tol)
    c = cases[names.index("r3k4_masked_e7")]
    w3 = C.molecule_statistics(c["ref"], c["gen"], C.atom_pairs_of(c), c["keep"], kernel_mul=3.0, kernel_num=4)
    g3 = _launch(dev, [c], kernel_mul=3.0, kernel_num=4)[0]
    _close(g3, w3, tol)
    assert abs(g3["stats"][4] - want[names.index("r3k4_masked_e7")]["stats"][4]) > 1e-3     # the parameters are not ignored


def test_determinism(dev, suite):
    names, cases, got, _ = suite
    again = _launch(dev, cases)
    assert all(_same_bits(a, b) for a, b in zip(again, got))                    # two runs
    order = [4, 0, 6, 5, 2, 1, 3]
    moved = _launch(dev, [cases[i] for i in order])
    assert all(_same_bits(moved[j], got[i]) for j, i in enumerate(order))       # reordering permutes the results


def test_degenerate_ensembles(dev, tol):
    rng = np.random.default_rng(3)
    ref, gen = C.make_conformers(rng, 5, 6, 9)
    pairs = C.chain_pairs(5, 3)
    same = {"ref": np.repeat(ref[:1], 6, 0), "gen": np.repeat(ref[:1], 9, 0), "keep": None, "pairs": pairs}
    equal = {"ref": ref, "gen": ref.copy(), "keep": None, "pairs": pairs}
    a, b = _launch(dev, [same, equal])
    assert (a["single"] == 0).all() and (a["pair"] == 0).all() and (a["stats"][:5] == 0).all()      # exactly 0
    for i, k in enumerate(C.STATS):
        assert abs(b["stats"][i]) <= tol[k], k
    assert np.abs(b["single"]).max() <= tol["single_items"] and np.abs(b["pair"]).max() <= tol["pair_items"]


def test_excluded_conformers(dev):
    rng = np.random.default_rng(4)
    keep = np.array([1, 1, 0, 1, 1, 1], dtype=bool)                             # atom 2 is a masked hydrogen
    ref, gen = C.make_conformers(rng, 6, 4, 7)
    pairs = C.chain_pairs(5, 3)
    other_ref, other_gen = C.make_conformers(rng, 4, 3, 5)
    other = {"ref": other_ref, "gen": other_gen, "keep": None, "pairs": C.chain_pairs(4, 2)}
    clean = {"ref": ref, "gen": gen[[0, 1, 3, 4, 6]], "keep": keep, "pairs": pairs}
    bad = gen.copy()
    bad[2, 3, 1] = np.nan                                                       # generated conformer 2: a NaN on atom 3
    bad[5, 0, 2] = np.inf                                                       # generated conformer 5: an infinity on atom 0
    bad[4, 2, 0] = np.nan                                                       # a NaN on the masked hydrogen changes nothing
    dirty = {"ref": ref, "gen": bad, "keep": keep, "pairs": pairs}
    want, want_other = _launch(dev, [clean, other])
    got, got_other = _launch(dev, [dirty, other])
    assert np.isfinite(want["stats"]).all() and want["stats"][5:].tolist() == [4.0, 5.0]
    assert _same_bits(got, want) and _same_bits(got_other, want_other)          # bitwise the evaluation without them
    assert got["finite"].tolist() == [1] * 4 + [1, 1, 0, 1, 1, 0, 1] and want["finite"].all()
    mirror = C.molecule_statistics(ref, bad, C.atom_pairs_of(dirty), keep)
    assert mirror["stats"][5:].tolist() == [4.0, 5.0] and mirror["finite"].tolist() == got["finite"].tolist()
    # a reference is excluded the same way
    bad_ref = ref.copy()
    bad_ref[1, 5, 0] = -np.inf
    a = _launch(dev, [{"ref": bad_ref, "gen": gen, "keep": keep, "pairs": pairs}])[0]
    b = _launch(dev, [{"ref": ref[[0, 2, 3]], "gen": gen, "keep": keep, "pairs": pairs}])[0]
    assert _same_bits(a, b) and a["stats"][5:].tolist() == [3.0, 7.0]
    # no generated conformer left: NaN, the launch's other molecule unchanged
    none = {"ref": ref, "gen": np.full_like(gen, np.nan), "keep": keep, "pairs": pairs}
    got, got_other = _launch(dev, [none, other])
    assert np.isnan(got["stats"][:5]).all() and got["stats"][5:].tolist() == [4.0, 0.0]
    assert np.isnan(got["single"]).all() and np.isnan(got["pair"]).all() and _same_bits(got_other, want_other)


def test_rigid_motion_changes_nothing_beyond_the_tolerance(dev, suite, tol):
    names, cases, got, _ = suite
    rng = np.random.default_rng(8)
    moved = []
    for c in cases:
        m = dict(c)
        for key in ("ref", "gen"):
            x = c[key].astype(np.float64)
            m[key] = np.stack([xa @ C.random_rotation(rng).T + 3.0 * rng.normal(size=3) for xa in x]).astype(np.float32)
        moved.append(m)
    for name, a, b in zip(names, _launch(dev, moved), got):
        for i, k in enumerate(C.STATS):
            if not np.isnan(b["stats"][i]):
                assert abs(a["stats"][i] - b["stats"][i]) < tol[k], (name, k)


def _records(rng, sizes, K):
    from moleculesde_amd.batch import MolData
    from moleculesde_amd.synthetic import make_molecule
    recs, refs = [], []
    for n in sizes:
        m = make_molecule(rng, n, with_h=True)
        m.x[:2, 0] = 6                                                          # at least two heavy atoms
        p = m.positions.numpy().astype(np.float64)
        refs.append(torch.from_numpy((p[None] + 0.1 * rng.normal(size=(3,) + p.shape)).astype(np.float32)))
        gen = (p[None] + 0.3 * rng.normal(size=(K,) + p.shape)).astype(np.float32)
        recs.append(MolData(x=m.x.clone(), positions=m.positions.clone(), edge_index=m.edge_index.clone(),
                            pos_gen=torch.from_numpy(gen.reshape(-1, 3)), num_pos_gen=torch.tensor([K]), finite=True))
    return recs, refs


def test_evaluate_distance_mmd_end_to_end(dev, tol, tmp_path, capsys):
    """Synthetic records with hydrogens through evaluate_distance_mmd: equal to the low-level call on the same packing and
    inside the tolerance of the mirror; a failed record and the command line."""
    import pickle
    from moleculesde_amd import conformer_mmd as cm
    rng = np.random.default_rng(15)
    recs, refs = _records(rng, (7, 9, 8), K=6)
    recs[2].finite = False                                                      # the sampler flagged molecule 2
    res = cm.evaluate_distance_mmd(recs, refs)
    assert res["num_molecules"] == 3 and res["num_failed"] == 1 and res["num_without_pairs"] == 0
    assert res["max_hops"] == 3 and res["kernel_mul"] == 2.0 and res["kernel_num"] == 5
    pm = res["per_molecule"]
    cases = []
    for rec, r in zip(recs, refs):
        keep = cm.heavy_atom_mask(rec.x).numpy()
        gen = rec.pos_gen.numpy().reshape(6, -1, 3)
        cases.append({"ref": r.numpy(), "gen": gen if rec.finite else np.full_like(gen, np.nan), "keep": keep,
                      "pairs": cm.distance_pairs(rec)})
    low = _launch(dev, cases)
    for g, c in enumerate(cases):
        assert pm["num_pairs"][g] == c["pairs"].shape[0] > 0
        assert [pm["num_ref_used"][g], pm["num_gen_used"][g]] == low[g]["stats"][5:].tolist() == [3.0, 0.0 if g == 2 else 6.0]
        got = np.array([pm[k][g] for k in C.STATS])
        assert np.array_equal(got.view(np.int64), low[g]["stats"][:5].view(np.int64))
        _close(low[g], C.molecule_statistics(c["ref"], c["gen"], C.atom_pairs_of(c), keep), tol)
    assert np.isnan([pm[k][2] for k in C.STATS]).all()
    for k in C.STATS:
        v = np.array(pm[k][:2])
        assert res["mean"][k] == pytest.approx(v.mean(), rel=1e-15) and res["median"][k] == pytest.approx(np.median(v), rel=1e-15)
    every = cm.evaluate_distance_mmd(recs[:2], refs[:2], heavy_atoms_only=False, max_hops=None)
    assert every["per_molecule"]["num_pairs"] == [21, 36] and every["num_failed"] == 0
    path = tmp_path / "samples.pkl"
    with open(path, "wb") as f:
        pickle.dump(recs, f)
    torch.save(refs, tmp_path / "refs.pt")
    assert cm.main([str(path), "--references", str(tmp_path / "refs.pt")]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["num_failed"] == 1 and "per_molecule" not in line
    assert line["mean"] == pytest.approx(res["mean"]) and line["median"]["all"] == pytest.approx(res["median"]["all"])
    assert cm.main([str(path), "--all_pairs", "--all_atoms", "--per_molecule"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["max_hops"] is None and line["per_molecule"]["num_pairs"] == [21, 36, 28]
    assert line["per_molecule"]["all"][2] is None                               # NaN is printed as null
