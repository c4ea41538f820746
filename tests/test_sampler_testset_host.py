"""Host side of the many-molecules-per-trajectory 2D->3D sampler (moleculesde_amd/sampler.py: corrector_update_grouped,
group_seed, generate_samples_from_testset's chunk plan, the refusals of position_PC_generation_grouped).  No GPU."""
import os
import pickle

import numpy as np
import pytest
import torch

from moleculesde_amd import sampler
from moleculesde_amd.geom3d.sde import VESDE, VPSDE
from moleculesde_amd.synthetic import make_molecule


class _StubScore:
    """get_score = a fixed smooth function of the coordinates (no parameters, no graph)."""

    def get_score(self, representation, data, pos, sigma, t):
        return torch.sin(pos) - 0.3 * pos + 0.1 * torch.cos(2.0 * pos.flip(-1))


@pytest.mark.parametrize("sde", [VESDE(0.2, 1.0, 1000), VPSDE(0.2, 30.0, 1000)], ids=["VE", "VP"])
def test_grouped_corrector_equals_separate_calls(sde):
    """Three groups (5, 1 and 9 atoms): corrector_update_grouped == corrector_update on each slice with the same noise, fp64
    rtol 1e-12; the groups permuted give the permuted result."""
    torch.manual_seed(0)
    sizes = [5, 1, 9]
    n = sum(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    pos = torch.randn(n, 3, dtype=torch.float64)
    noise = torch.randn(n, 3, dtype=torch.float64)
    t = torch.full((n,), 0.37, dtype=torch.float64)
    gi = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    m = _StubScore()
    x, xm = sampler.corrector_update_grouped(sde, m, None, None, pos, t, 0.16, 0.7, gi, 3, noises=[noise])
    for g in range(3):
        s = slice(int(ptr[g]), int(ptr[g + 1]))
        rx, rxm = sampler.corrector_update(sde, m, None, None, pos[s], t[s], 0.16, 0.7, 1, noises=[noise[s]])
        torch.testing.assert_close(x[s], rx, rtol=1e-12, atol=0)
        torch.testing.assert_close(xm[s], rxm, rtol=1e-12, atol=0)
    order = [2, 0, 1]
    perm = torch.cat([torch.arange(int(ptr[g]), int(ptr[g + 1])) for g in order])
    gi_p = torch.repeat_interleave(torch.arange(3), torch.tensor([sizes[g] for g in order]))
    xp, xmp = sampler.corrector_update_grouped(sde, m, None, None, pos[perm], t[perm], 0.16, 0.7, gi_p, 3, noises=[noise[perm]])
    torch.testing.assert_close(xp, x[perm], rtol=1e-12, atol=0)
    torch.testing.assert_close(xmp, xm[perm], rtol=1e-12, atol=0)


def test_group_seed_is_a_pure_distinct_64_bit_mix():
    seeds = [sampler.group_seed(1234, i) for i in range(1000)]
    assert len(set(seeds)) == 1000 and all(0 <= s < 2 ** 64 for s in seeds)
    assert seeds == [sampler.group_seed(1234, i) for i in range(1000)]
    assert sampler.group_seed(0, 0) == 0xE220A8397B1DCDAF          # splitmix64's first output for state 0
    assert sampler.group_seed(1235, 0) != seeds[0]


class _Gnn(torch.nn.Module):
    def forward(self, x, edge_index, edge_attr):
        return torch.zeros(x.size(0), 4)


class _Sde23(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.sde_pos = VESDE(0.2, 1.0, 50)


def _drive(monkeypatch, **kw):
    """generate_samples_from_testset on 7 molecules with the trajectory replaced by a stub that records its launches and
    returns pos_init + the group's seed folded to a small number."""
    rng = np.random.default_rng(3)
    mols = [make_molecule(rng, n) for n in (4, 2, 7, 5, 3, 6, 2)]
    calls = []

    def stub(score_model, representation, data, group_ptr, num_steps=1000, pos_init=None, group_seeds=None, **rest):
        calls.append(dict(group_ptr=list(group_ptr), num_steps=num_steps, seeds=list(group_seeds), n=representation.size(0),
                          graphs=data.num_graphs, rest=rest))
        out = pos_init.clone()
        for g in range(len(group_ptr) - 1):
            out[group_ptr[g]:group_ptr[g + 1]] += float(group_seeds[g] % 97)
        return out, torch.zeros(len(group_ptr) - 1, dtype=torch.int32)

    monkeypatch.setattr(sampler, "position_PC_generation_grouped", stub)
    gnn, s23 = _Gnn().train(), _Sde23().train()
    recs = sampler.generate_samples_from_testset(mols, gnn, s23, **kw)
    assert not gnn.training and not s23.training
    return mols, calls, recs


def test_driver_chunk_plan_records_and_file_name(monkeypatch, tmp_path):
    mols, calls, recs = _drive(monkeypatch, num_repeat=3, start=1, end=100, molecules_per_launch=4, noise_seed=5,
                               out_path=str(tmp_path), eval_epoch=7, min_sigma=0.01, snr=0.2)
    # end is clipped to the 7 molecules; 6 of them in chunks of 4: a short last chunk
    sizes = [m.num_nodes for m in mols]
    assert [len(c["seeds"]) for c in calls] == [4, 2]
    assert calls[0]["group_ptr"] == [0] + list(np.cumsum([3 * s for s in sizes[1:5]]))
    assert calls[1]["group_ptr"] == [0] + list(np.cumsum([3 * s for s in sizes[5:7]]))
    assert calls[0]["graphs"] == 12 and calls[0]["n"] == 3 * sum(sizes[1:5])
    assert calls[0]["num_steps"] == 50 and calls[0]["rest"] == {"snr": 0.2}          # num_steps=None: the SDE's N
    assert [s for c in calls for s in c["seeds"]] == [sampler.group_seed(5, i) for i in range(1, 7)]
    assert len(recs) == 6
    for r, m in zip(recs, mols[1:]):
        assert torch.equal(r.x, m.x) and torch.equal(r.edge_index, m.edge_index) and torch.equal(r.positions, m.positions)
        assert r.pos_gen.shape == (3 * m.num_nodes, 3) and r.pos_gen.device.type == "cpu"
        assert r.num_pos_gen.tolist() == [3] and r.finite is True
    path = os.path.join(str(tmp_path), "2D_to_3D_PC_1_100_epoch_7_min_sig_0.010_repeat_3")
    with open(path, "rb") as f:
        back = pickle.load(f)
    assert len(back) == 6 and torch.equal(back[2].pos_gen, recs[2].pos_gen)


def test_driver_results_do_not_depend_on_the_chunking(monkeypatch):
    """molecules_per_launch 1, 3 and 7 and another `start`: the same seeds, the same starting coordinates, the same records."""
    _, c1, r1 = _drive(monkeypatch, num_repeat=2, start=0, end=7, molecules_per_launch=1, noise_seed=11, num_steps=4)
    _, c3, r3 = _drive(monkeypatch, num_repeat=2, start=0, end=7, molecules_per_launch=3, noise_seed=11, num_steps=4)
    _, c7, r7 = _drive(monkeypatch, num_repeat=2, start=2, end=5, molecules_per_launch=7, noise_seed=11, num_steps=4)
    assert [len(c["seeds"]) for c in c1] == [1] * 7 and [len(c["seeds"]) for c in c3] == [3, 3, 1]
    assert [len(c["seeds"]) for c in c7] == [3] and len(r7) == 3
    for a, b in zip(r1, r3):
        assert torch.equal(a.pos_gen, b.pos_gen)
    for a, b in zip(r1[2:5], r7):
        assert torch.equal(a.pos_gen, b.pos_gen)
    _, _, other = _drive(monkeypatch, num_repeat=2, start=0, end=2, molecules_per_launch=2, noise_seed=12, num_steps=4)
    assert not torch.equal(other[0].pos_gen, r1[0].pos_gen)
    _, empty_calls, empty = _drive(monkeypatch, num_repeat=2, start=9, end=20, molecules_per_launch=2, noise_seed=1)
    assert empty == [] and empty_calls == []


def test_grouped_sampler_refuses_bad_group_tables():
    rep = torch.zeros(10, 4)
    m = _Sde23()
    for ptr, seeds, word in (([0, 6, 4, 10], None, "monotone"), ([0, 4, 4, 10], None, "empty"), ([0, 4, 10], [1, 2, 3], "group_seeds"),
                             ([0, 4, 9], None, "group_ptr"), ([1, 4, 10], None, "group_ptr")):
        with pytest.raises(ValueError, match=word):
            sampler.position_PC_generation_grouped(m, rep, None, ptr, num_steps=3, group_seeds=seeds)
    with pytest.raises(ValueError, match="monotone"):
        sampler.position_PC_generation_grouped(m, rep, None, torch.tensor([0, 6, 4, 10]), num_steps=3)


def test_grouped_sampler_operator_path_on_cpu_flags_a_diverged_group_only():
    """CPU tensors and a stub with get_score take the operator path: a clean run is finite with both flags 0; with the same
    torch noise, a group whose coordinates start at inf is flagged and the other group's result does not move by a bit."""
    class M(_StubScore):
        sde_pos = VESDE(0.2, 1.0, 1000)

    sizes = [3, 5]
    pos0 = torch.randn(8, 3, generator=torch.Generator().manual_seed(1))
    rep = torch.zeros(8, 4)
    torch.manual_seed(3)
    both, bad = sampler.position_PC_generation_grouped(M(), rep, None, [0, 3, 8], num_steps=4, pos_init=pos0, use_graph=False)
    assert bad.tolist() == [0, 0] and torch.isfinite(both).all() and both.shape == (8, 3)
    pos1 = pos0.clone()
    pos1[:3] = float("inf")
    torch.manual_seed(3)
    hurt, bad = sampler.position_PC_generation_grouped(M(), rep, None, [0, 3, 8], num_steps=4, pos_init=pos1, use_graph=False)
    assert bad.tolist() == [1, 0]
    assert torch.equal(hurt[3:], both[3:])
