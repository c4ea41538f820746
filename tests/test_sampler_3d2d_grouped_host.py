"""Host side of the grouped 3D->2D sampler: the corrector's arithmetic given the scores (sampler_3d2d.corrector_steps_grouped,
the reference of csrc/dense_pc_grouped.hip) on the CPU, the group-table checks, the test-set driver's chunking and seeds with
the sampler stubbed out, and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNR, SCALE_EPS = 0.2, 0.9


def _case(n_steps=2, seed=0):
    """Molecules of 2, 5, 5, 5, 13, 13 atoms in three groups of 1, 3, 2 replicas; one atom of the second group flagged off."""
    g = torch.Generator().manual_seed(seed)
    sizes, reps = [2, 5, 5, 5, 13, 13], [1, 3, 2]
    B, Nm, ncls = len(sizes), max(sizes), 7
    flags = torch.zeros(B, Nm, dtype=torch.float64)
    for b, n in enumerate(sizes):
        flags[b, :n] = 1.0
    flags[1:4, 2] = 0.0
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    fm = flags[:, :, None] * flags[:, None, :]
    sym = lambda a: (a.triu(1) + a.triu(1).transpose(-1, -2)) * fm
    t = dict(x=r(B, Nm, ncls) * flags[:, :, None], adj=sym(r(B, Nm, Nm)), score_x=r(B, Nm, ncls) * flags[:, :, None],
             score_adj=sym(r(B, Nm, Nm)), z_x=r(n_steps, B, Nm, ncls), z_adj=r(n_steps, B, Nm, Nm), flags=flags)
    gi = torch.repeat_interleave(torch.arange(len(reps)), torch.tensor(reps))
    gp = [0] + list(np.cumsum(reps))
    return t, gi, gp, len(reps)


def _run(S, t, gi, G, alpha, sel=slice(None)):
    return S.corrector_steps_grouped(t["x"][sel], t["adj"][sel], t["score_x"][sel], t["score_adj"][sel], t["z_x"][:, sel],
                                     t["z_adj"][:, sel], t["flags"][sel], alpha, gi, G, SNR, SCALE_EPS)


@pytest.mark.parametrize("n_steps", [1, 3])
def test_whole_batch_equals_each_group_alone(n_steps):
    from moleculesde_amd import sampler_3d2d as S
    t, gi, gp, G = _case(n_steps)
    alpha = torch.full((len(gi),), 0.97, dtype=torch.float64)
    whole = _run(S, t, gi, G, alpha)
    for g in range(G):
        sel = slice(int(gp[g]), int(gp[g + 1]))
        alone = _run(S, t, torch.zeros(sel.stop - sel.start, dtype=torch.long), 1, alpha[sel], sel)
        for name, w, a in zip(("x", "adj", "x_mean", "adj_mean"), whole, alone):
            assert bool(torch.isfinite(a).all()) and a.abs().sum() > 0
            assert torch.equal(w[sel], a), (g, name)
    # and the groups do differ from the batch-mean corrector
    mean = _run(S, t, torch.zeros_like(gi), 1, alpha)
    assert not torch.allclose(whole[0], mean[0], rtol=1e-3, atol=1e-6)


def test_one_group_is_the_batch_mean_formula():
    """One group over the whole batch: LangevinCorrector's arithmetic as corrector_update writes it (means over the batch)."""
    from moleculesde_amd import sampler_3d2d as S
    t, gi, gp, G = _case(2, seed=1)
    alpha = 0.9
    got = _run(S, t, torch.zeros_like(gi), 1, alpha)
    flags = t["flags"]
    want = []
    for v, grad, zs, sym in ((t["adj"], t["score_adj"], t["z_adj"], True), (t["x"], t["score_x"], t["z_x"], False)):
        vm = v
        for s in range(2):
            z = S.sym_noise(zs[s], flags) if sym else zs[s] * flags[:, :, None]
            grad_norm = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
            noise_norm = torch.norm(z.reshape(z.shape[0], -1), dim=-1).mean()
            step_size = (SNR * noise_norm / grad_norm) ** 2 * 2 * alpha
            vm = v + step_size * grad
            v = vm + torch.sqrt(step_size * 2) * z * SCALE_EPS
        want.append((v, vm))
    (adj_n, adj_m), (x_n, x_m) = want
    for name, g_, w_ in zip(("x", "adj", "x_mean", "adj_mean"), got, (x_n, adj_n, x_m, adj_m)):
        assert bool(torch.isfinite(w_).all())
        # the mean of B norms: one summation order against another in float64
        assert torch.allclose(g_, w_, rtol=1e-13, atol=1e-13), name


def test_group_table_checks():
    from moleculesde_amd import sampler_3d2d as S
    assert S._check_mol_groups([0, 1, 4, 6], 6, [1, 2, 3]) == [0, 1, 4, 6]
    assert S._check_mol_groups(torch.tensor([0, 6]), 6, None) == [0, 6]
    for table, seeds in (([1, 4, 6], None), ([0, 4, 5], None), ([0, 4, 4, 6], None), ([0, 4, 3, 6], None), ([0], None), ([], None),
                         ([0, 1, 4, 6], [1, 2]), ([0, 6], [])):
        with pytest.raises(ValueError):
            S._check_mol_groups(table, 6, seeds)


def test_chunks():
    from moleculesde_amd.graph2d_eval import launch_chunks
    assert launch_chunks(0, 100, 7, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert launch_chunks(2, 6, 7, 2) == [[2, 3], [4, 5]]
    assert launch_chunks(2, 7, 7, 2) == [[2, 3], [4, 5], [6]]
    assert launch_chunks(-3, 2, 7, 5) == [[0, 1]]
    assert launch_chunks(5, 5, 7, 2) == []
    assert launch_chunks(0, 3, 7, 1) == [[0], [1], [2]]
    for per in (0, -1):
        with pytest.raises(ValueError):
            launch_chunks(0, 3, 7, per)


@pytest.mark.parametrize("start,end,per", [(0, 7, 3), (2, 6, 2), (1, 100, 4), (0, 7, 50)])
def test_driver_chunks_and_seeds_with_the_sampler_stubbed(monkeypatch, tmp_path, start, end, per):
    """Which molecules and which seeds every generate_2d_from_3d_grouped call receives, the records' order, `diverged`, and the
    pickle's name."""
    from moleculesde_amd import graph2d_eval as ge, sampler_3d2d as S
    from moleculesde_amd.sampler import group_seed
    from moleculesde_amd.synthetic import make_molecule
    rng = np.random.default_rng(2)
    mols = [make_molecule(rng, n) for n in (4, 9, 6, 12, 5, 7, 3)]
    calls = []

    def stub(model_3d, sde_model, molecules, num_repeat, group_seeds, **kw):
        calls.append(([next(i for i, m in enumerate(mols) if m is mol) for mol in molecules], list(group_seeds), dict(kw)))
        Nm = max(m.num_nodes for m in molecules)
        out = []
        for mol, s in zip(molecules, group_seeds):
            x = torch.full((num_repeat, Nm, 5), float(s % 1000))
            out.append((x, torch.full((num_repeat, Nm, Nm), float(mol.num_nodes)), x, x))
        return out, torch.tensor([int(m.num_nodes == 12) for m in molecules], dtype=torch.int32)

    monkeypatch.setattr(S, "generate_2d_from_3d_grouped", stub)
    monkeypatch.setattr(S, "generate_2d_from_3d", lambda *a, **k: pytest.fail("the per-molecule loop ran"))
    recs = ge.generate_graphs_from_testset(mols, None, None, num_repeat=2, start=start, end=end, noise_seed=77, out_path=str(tmp_path),
                                           molecules_per_launch=per, max_iters=3)
    want = list(range(max(0, start), min(end, len(mols))))
    assert [i for c in calls for i in c[0]] == want
    assert all(len(c[0]) == per for c in calls[:-1]) and 1 <= len(calls[-1][0]) <= per
    for idx, seeds, kw in calls:
        assert seeds == [group_seed(77, i) for i in idx] and kw == {"max_iters": 3}
    assert len(recs) == len(want)
    for i, rec in zip(want, recs):
        n = mols[i].num_nodes
        assert tuple(rec.x_gen.shape) == (2, n, 5) and tuple(rec.adj_gen.shape) == (2, n, n)
        assert float(rec.x_gen[0, 0, 0]) == float(group_seed(77, i) % 1000) and float(rec.adj_gen[0, 0, 0]) == n
        assert rec.diverged is (n == 12) and torch.equal(rec.edge_index, mols[i].edge_index)
    assert [f.name for f in tmp_path.iterdir()] == ["3D_to_2D_{}_{}_repeat_2".format(start, end)]


def test_molecules_per_launch_must_be_positive():
    from moleculesde_amd import graph2d_eval as ge
    with pytest.raises(ValueError):
        ge.generate_graphs_from_testset([], None, None, molecules_per_launch=0)


def test_entry_points_declared():
    """include/msde_hip.h declares the three grouped entry points and the group table with the documented parameter lists;
    msde_dense_pc_params is not touched (its ctypes mirror has the same fields)."""
    from moleculesde_amd import _lib
    text = open(os.path.join(ROOT, "include", "msde_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    head = "const msde_dense_pc_params* p, const msde_dense_pc_groups* gr, "
    score = "const float* G2, int F2, const float* w2, const float* b2, const float* OUT, void* stream);"
    assert "int msde_dense_pc_init_grouped(" + head + "const float* adj_given, void* stream);" in flat
    assert "int msde_dense_pc_corrector_grouped(" + head + score in flat
    assert "int msde_dense_pc_predictor_grouped(" + head + score in flat
    assert ("typedef struct msde_dense_pc_groups { const int* group_ptr; const unsigned long long* group_seed; int* group_bad; "
            "int G; } msde_dense_pc_groups;") in flat
    assert [f[0] for f in _lib.DensePcGroups._fields_] == ["group_ptr", "group_seed", "group_bad", "G"]
    for name in ("msde_dense_pc_init_grouped", "msde_dense_pc_corrector_grouped", "msde_dense_pc_predictor_grouped"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["msde_dense_pc_corrector_grouped"]) == len(_lib.SIGNATURES["msde_dense_pc_corrector"]) + 1
    assert "dense_pc_grouped.hip" in __import__("moleculesde_amd.build", fromlist=["SOURCES"]).SOURCES
