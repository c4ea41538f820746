"""The counter generator's host mirror (tests/rng_mirror.py) against the package's two other restatements, and the
disjointness of the random streams one sampler trajectory / one training step consumes: every stream is described by the
(seed', index) pairs of its kernel, `counters()` turns them into the 64-bit values the finaliser sees, and two draws are the
same draw exactly when those are equal -- so overlap is a set intersection, not a statistic.  No GPU."""
import itertools

import numpy as np

import rng_mirror as RM
from moleculesde_amd import dataset as DS
from moleculesde_amd import finetune_molnet as FM
from moleculesde_amd import sampler as SP

M64 = (1 << 64) - 1


def _ref_mix(seed, idx):
    """msde_mix64 on Python integers, written out independently of the mirror."""
    z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ------------------------------------------------------------------------------------------------ mirror agreement
def test_mirror_agrees_with_the_package_restatements():
    idx = [0, 1, 2, 299, 300, 123456789, (1 << 40) + 3, M64, M64 - 1]
    for seed in (0, 1, 42, 1234, M64, FM.dropout_seed(42, 3, 7), -5, 1 << 64):
        s = seed & M64
        got = RM.mix64(seed, np.array(idx, dtype=np.uint64))
        assert [int(v) for v in got] == [_ref_mix(s, i) for i in idx]
        assert [int(v) for v in got] == [DS._mix64(s, i) for i in idx]
        assert [int(RM.counters(seed, i)) for i in idx] == [(s + 0x9E3779B97F4A7C15 * (i + 1)) & M64 for i in idx]
        u = RM.uniform(seed, np.array(idx, dtype=np.uint64))
        assert u.dtype == np.float32
        assert np.array_equal(u, FM.msde_uniform(s, np.array(idx, dtype=np.uint64)))
        # the known answers of test_finetune_molnet_host.py: (mix >> 40) / 2^24
        assert [float(v) for v in u] == [(_ref_mix(s, i) >> 40) / 16777216.0 for i in idx]
        assert [int(v) for v in RM.uniform24(seed, np.array(idx, dtype=np.uint64))] == [_ref_mix(s, i) >> 40 for i in idx]
    assert int(RM.pc_mix(0)) == 0 and int(RM.pc_mix(1)) == _ref_mix(1 - 0x9E3779B97F4A7C15, 0)
    assert RM.dev_seed(42, None) == 42 and RM.dev_seed(M64, 3) == (M64 + 3 * 0x100000001B3) & M64
    assert RM.dev_seed(FM.dropout_seed(42, 2), 5) == FM.dropout_seed(42, 2, 5)
    for ns, i in ((0, 0), (1234, 7), (M64, 99)):
        assert RM.sampler_group_seed(ns, i) == SP.group_seed(ns, i)


def test_randn_is_box_muller_on_uniforms_2i_and_2i_plus_1():
    import math
    for seed in (1234, M64):
        for i in (0, 1, 5, 1 << 33):
            u1 = max((_ref_mix(seed, 2 * i) >> 40) / 16777216.0, 2.0 ** -24)
            u2 = (_ref_mix(seed, 2 * i + 1) >> 40) / 16777216.0
            want = math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)
            got = RM.randn(seed, np.array([i], dtype=np.uint64))
            assert got.dtype == np.float64 and abs(float(got[0]) - want) < 1e-14
    # the clamp: a zero first uniform gives sqrt(-2 ln 2^-24) * cos(.), not inf
    z = np.zeros(1, dtype=np.float32)
    assert np.maximum(z, np.float32(2.0 ** -24))[0] == np.float32(5.9604645e-8)
    assert RM.randn(7, np.arange(4)).shape == (4,) and RM.randn(7, np.arange(4), np.float32).dtype == np.float32


def test_randn_tolerance_is_measured_on_the_mirror():
    """randn_tol = 8 x the largest |float32 mirror - float64 mirror| over the first 2^20 draws of seed 1234 (about 1.5e-6: a few
    float32 ulp of a value near 4, from the rounded angle 2 pi u2).  Bounds: not below 1 ulp of 1.0, not above 16 ulp of the
    largest draw (sqrt(-2 ln 2^-24) = 5.77, ulp 4.8e-7) -- a wrong index or seed is an O(1) difference, 5 orders above."""
    tol, d = RM.measure_randn_tol()
    print(f"float32 vs float64 mirror over 2^20 draws: {d:.3e}; randn_tol = {tol:.3e}")
    assert tol == 8.0 * d
    assert 1.2e-7 < d < 16 * 4.8e-7
    z = RM.randn(1234, np.arange(1 << 20))
    assert abs(float(z.mean())) < 0.005 and abs(float(z.var()) - 1.0) < 0.01       # (sanity of the reference itself)


# ------------------------------------------------------------------------------------------------ disjointness
def _overlaps(streams):
    """[(a, b, shared counters)] for every pair of named streams that share a counter; a stream whose own counters repeat
    (unless its elements share draws by design: the antithetic time steps) is reported against itself."""
    sets = {k: s.counters() for k, s in streams.items()}
    bad = []
    for k, c in sets.items():
        if len(np.unique(c)) != len(c) and not streams[k].repeats:
            bad.append((k, k, len(c) - len(np.unique(c))))
    allc = np.concatenate(list(sets.values()))
    if len(np.unique(allc)) == sum(len(np.unique(c)) for c in sets.values()):
        return bad
    for a, b in itertools.combinations(sets, 2):
        n = len(np.intersect1d(sets[a], sets[b]))
        if n:
            bad.append((a, b, n))
    return bad


def _additive_pc_draw_stream(seed, row, stream, n3):
    """NEGATIVE CONTROL: pc_draw as it was before the (row, stream) seed was finalised -- seed + GOLDEN * (2 row + stream), a
    multiple of the generator's own increment, so the counters depend on 2 row + stream + 2 i alone."""
    return RM.Stream((int(seed) + RM.GOLDEN * (2 * int(row) + int(stream))) & M64, np.arange(n3), True)


def _sampler_trajectory(draw, n_atoms=7, rows=8, noise_seed=1234):
    """Corrector and predictor noise of rows 0..7 on n = 7 atoms: one single-molecule trajectory (seed = noise_seed) and two
    molecules of a grouped one (seeds from sampler.group_seed)."""
    seeds = {"single": noise_seed, "group0": SP.group_seed(noise_seed, 0), "group1": SP.group_seed(noise_seed, 1)}
    return {f"{who} row {r} {'corrector' if s == 0 else 'predictor'}": draw(seed, r, s, 3 * n_atoms)
            for who, seed in seeds.items() for r in range(rows) for s in (0, 1)}


def test_sampler_trajectory_streams_are_disjoint():
    assert _overlaps(_sampler_trajectory(RM.pc_draw_stream)) == []


def test_additive_row_seed_overlaps_negative_control():
    """The additive derivation reuses noise, and the check above sees it: corrector of row r + 1 at element i == corrector of
    row r at element i + 1, the predictor likewise, and predictor and corrector of one row share uniforms."""
    bad = _overlaps(_sampler_trajectory(_additive_pc_draw_stream))
    pairs = {(a, b) for a, b, _ in bad}
    assert ("single row 0 corrector", "single row 1 corrector") in pairs
    assert ("single row 0 predictor", "single row 1 predictor") in pairs
    assert ("single row 0 corrector", "single row 0 predictor") in pairs
    assert any(a.startswith("group0") and b.startswith("group0") for a, b in pairs)
    a = _additive_pc_draw_stream(1234, 0, 0, 30).randn()
    b = _additive_pc_draw_stream(1234, 1, 0, 30).randn()
    assert np.array_equal(a[1:], b[:-1])
    z = np.concatenate([_additive_pc_draw_stream(1234, r, 0, 30).randn() for r in range(6)])
    assert len(np.unique(z)) == 35                      # 6 iterations x 30 coordinates: 35 distinct values out of 180
    z = np.concatenate([RM.pc_draw_stream(1234, r, 0, 30).randn() for r in range(6)])
    assert len(np.unique(z)) == 180


SCORE_SEED_BASE = 0x5DE2D3D            # geom3d/sde_2d_to_3d.py EquivariantScoreNetwork._seed_base


def _training_step(calls, ctr, rank=0, tag="", net_calls=None):
    """Every stream one pretraining step draws in its kernels.  calls / net_calls: the host draw counters before the step
    (DeviceNoise.calls: three draws per step; the score network's _calls: one per eager step, default calls // 3); ctr: the
    device step counter (None: eager); rank: pretrain.Trainer folds it into the noise seed (+ 7919 r) and the score network's
    seed base (+ 0x10001 r)."""
    net_calls = calls // 3 if net_calls is None else net_calls
    noise_seed = 0x5EED + 7919 * rank
    base = SCORE_SEED_BASE + 0x10001 * rank
    atoms, ext_edges, heads, ncls = [2, 5, 32, 1], 300, 8, 119            # 40 atoms
    dense = [2, 5, 32]
    s = {}
    for w in (0, 1):                                                      # dual_CL's pair of permutations (nn.py:275)
        s[f"randperm {w}"] = RM.randperm_stream(RM.next_seed(noise_seed, calls + 1), ctr, w, 300)
    ve = RM.ve_perturb_streams(RM.next_seed(noise_seed, calls + 2), ctr, atoms)      # sde_2d_to_3d.py:278
    s["ve noise"], s["ve time"] = ve["noise"], ve["time"]
    for k, seed in (("next_seed", RM.next_seed(noise_seed, calls + 3)), ("dense_head_seed", RM.dense_head_seed(noise_seed, calls + 3))):
        dp = RM.dense_prepare_streams(seed, ctr, dense, ncls)             # consecutive next_seed(), and the head's own (:325)
        for name, st in dp.items():
            s[f"dense {name} ({k})"] = st
    for k in range(16):
        ls = RM.layer_seed(base, net_calls + 1, k)
        s[f"layer {k} attention"] = RM.attention_dropout_stream(ls, ctr, ext_edges, heads)
        s[f"layer {k} ffn"] = RM.gat_tail_stream(ls ^ RM.FFN_XOR, ctr, sum(atoms))
    return {f"{tag}{k}": v for k, v in s.items()}


def test_training_step_streams_are_disjoint():
    assert sum(len(t) for t in (RM.pair_index([2, 5, 32])[0],)) == 1 + 10 + 496
    for ctr in (None, 0, 1):
        assert _overlaps(_training_step(0, ctr)) == [], ctr
    # two consecutive values of the device counter (captured step: the host counters stand still)
    both = dict(_training_step(6, 0, tag="ctr 0: "), **_training_step(6, 1, tag="ctr 1: "))
    assert _overlaps(both) == []
    # two consecutive eager steps (three DeviceNoise draws and one score-network call each)
    both = dict(_training_step(0, None, tag="step 0: "), **_training_step(3, None, tag="step 1: "))
    assert _overlaps(both) == []
    # ranks 0 and 1 of a data-parallel run
    for ctr in (None, 2):
        both = dict(_training_step(0, ctr, 0, "rank 0: "), **_training_step(0, ctr, 1, "rank 1: "))
        assert _overlaps(both) == [], ctr


def test_sampler_3d2d_trajectory_streams_are_disjoint():
    """Initial draws (row -1), the n_steps = 2 corrector draws and the predictor draw (draw = n_steps) of rows 0..3, pair and
    class noise, two molecules."""
    sizes, ncls, n_steps = [5, 32], 119, 2
    s = {}
    for row, draws in [(-1, [0])] + [(r, [0, 1, 2]) for r in range(4)]:
        for d in draws:
            for name, st in RM.dense_pc_streams(987654321, row, d, sizes, ncls).items():
                s[f"row {row} draw {d} {name}"] = st
    assert len(s) == 2 * (1 + 4 * 3)
    assert _overlaps(s) == []
    # the check can fail: the same key for two draws is seen
    s["again"] = RM.dense_pc_streams(987654321, 2, 1, sizes, ncls)["cls"]
    assert _overlaps(s) == [("row 2 draw 1 cls", "again", 2 * (5 + 32) * ncls)]
