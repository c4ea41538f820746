"""Host-side preconditions of tests/test_gpu_score_graph.py: the batch of helpers.SCORE_GRAPH_SPECS has the node / edge counts
and the in-degrees the GPU tests claim (0, below 8, 8..63, 64 and above; first and last node without in-edges; N odd and
3 mod 4), and every yardstick the GPU tolerances are multiples of -- the error of an fp32 evaluation of the same operation
on the CPU against fp64 -- is nonzero and small, so that a broken reference cannot loosen a bound."""
import pytest
import torch

import score_graph_cases as S

YARD_MAX = 1e-4


def test_graph_has_the_in_degrees_the_gpu_tests_claim():
    g = S.graph()
    assert g.N == 347 and g.N % 2 == 1 and g.N % 4 == 3
    assert g.E == 22842 and int(g.plan.rowptr[-1]) == g.E
    assert sorted(set(g.deg.tolist())) == [0, 1, 2] + list(range(7, 17)) + [63, 64, 65, 99]
    assert int(g.deg[0]) == 0 and int(g.deg[-1]) == 0
    for _, lo, hi in S.DEG_CLASSES:                                  # every class the parity lines report has nodes
        assert bool(((g.deg >= lo) & (g.deg <= hi)).any())
    # by-target order: edge rows of a node are rowptr[i] .. rowptr[i + 1]
    assert torch.equal(g.dst, torch.repeat_interleave(torch.arange(g.N), g.deg))
    # nodes without in-edges share a workgroup (2 or 4 consecutive nodes each) with nodes that have some
    assert int(g.deg[-2]) == 0 and int(g.deg[-4]) > 0 and int(g.deg[1]) == 1 and int(g.deg[3]) == 7


def _assert_yardsticks(c, what):
    assert c.yard, what
    for name, y in c.yard.items():
        assert 0.0 < y < YARD_MAX, f"{what} {name}: yardstick {y:.3e}"
        assert bool(torch.isfinite(c.ref[name]).all()) and float(c.ref[name].abs().max()) > 0, f"{what} {name}"


@pytest.mark.parametrize("heads,Ch", [(8, 4), (4, 8), (2, 2)])
def test_attention_yardsticks(heads, Ch):
    c = S.attention_case(heads, Ch)
    _assert_yardsticks(c, f"attention {heads}x{Ch}")
    assert set(c.yard) == {"out", "out_skip", "g_q", "g_k", "g_v", "g_ee"}
    zero = S.graph().deg == 0
    assert float(c.ref["out"][zero].abs().max()) == 0.0 and float(c.ref["g_q"][zero].abs().max()) == 0.0


@pytest.mark.parametrize("heads,Ch", [(8, 4), (2, 2)])
def test_large_logit_yardsticks(heads, Ch):
    """q scaled by 40: logits of a few hundred.  The fp32 evaluation subtracts the maximum and stays finite; one that did not
    would overflow expf (the logits exceed 88.7)."""
    g = S.graph()
    c = S.attention_case(heads, Ch, qscale=40.0)
    _assert_yardsticks(c, f"large logits {heads}x{Ch}")
    q, k, ee = (c.inputs[n].double() for n in ("q", "k", "ee"))
    logit = (q[g.dst].view(g.E, heads, Ch) * (k[g.src] + ee).view(g.E, heads, Ch)).sum(-1) / Ch ** 0.5
    assert 150.0 < float(logit.max()) < 1000.0


@pytest.mark.parametrize("heads,Ch", [(8, 4), (2, 2)])
@pytest.mark.parametrize("p,seed_dev", [(0.1, None), (0.5, None), (0.1, 5)])
def test_dropout_yardsticks_and_mask(heads, Ch, p, seed_dev):
    g = S.graph()
    c = S.attention_case(heads, Ch, p=p, seed=1234, seed_dev=seed_dev)
    _assert_yardsticks(c, f"dropout {heads}x{Ch} p {p}")
    kept = float((c.mask > 0).double().mean())
    assert abs(kept - (1 - p)) < 0.01                                 # E * heads >= 45 k draws
    assert sorted(set(c.mask.flatten().tolist())) == [0.0, 1.0 / (1.0 - float(torch.tensor(p, dtype=torch.float32)))]
    other = S.dropout_factor(g.E, heads, p, 1234, None if seed_dev is not None else 5)
    assert not torch.equal(other, c.mask)                             # seed_dev changes the mask


@pytest.mark.parametrize("heads,Ch", [(8, 4), (2, 2)])
def test_shared_projection_yardsticks(heads, Ch):
    c = S.shared_projection_case(heads, Ch)
    _assert_yardsticks(c, f"shared projection {heads}x{Ch}")
    D = heads * Ch
    for l in range(S.SHARED_LAYERS):                                  # every column block carries gradient
        assert float(c.ref["g_ee_all"][:, l * D:(l + 1) * D].abs().max()) > 0
        assert torch.equal(c.ref[f"g_s{l}"], c.w[:, l * D:(l + 1) * D].double())


def test_frame_mix_yardsticks():
    c = S.frame_mix_case()
    _assert_yardsticks(c, "frame mix")
    assert set(c.yard) == {"out", "out_base", "g_coff"}
    assert float(c.ref["out"][S.graph().deg == 0].abs().max()) == 0.0   # mean over no edges: 0, not 0 / 0


@pytest.mark.parametrize("hidden", [128, 32])
def test_head_mix_yardsticks(hidden):
    c = S.head_mix_case(hidden)
    _assert_yardsticks(c, f"head mix {hidden}")
    assert set(c.yard) == {"out", "out_base", "g_x", "g_W1", "g_b1", "g_W2", "g_b2"}


def test_geometry_frames_are_well_conditioned_and_fp32_meets_the_derived_tolerances():
    """No edge of the fixture is near a degenerate frame (kappa = |r||c| / |r x c| bounded), and a plain fp32 evaluation on the
    CPU meets the per-edge tolerances derived from kappa: they are achievable, and not taken from the kernel."""
    gc = S.geometry_case()
    assert float(gc.kappa.max()) < 100.0 and float(gc.kappa.min()) >= 1.0
    assert float(gc.ref["pcos"].abs().max()) < 1.0
    low = S.geometry_fp32()
    for name, ref in gc.ref.items():
        err = (low[name].double() - ref).abs()
        assert bool((err <= gc.tol[name]).all()), f"{name}: worst err / tol {float((err / gc.tol[name]).max()):.3f}"
    assert float(gc.tol["basis"].max()) < 1e-4 and float(gc.tol["psin"].max()) < 0.1
