"""oracle/restate.py vs the reference's files executed verbatim: the full step with dropout on, replayed from the fixture
the reference produced (oracle/make_golden_full_step.py -> tests/golden/full_step_dropout.npz), and the stand-in
third-party layer the reference runs on (oracle/standins) vs the oracle's own op restatements."""
import types
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_loader, restate as R
from oracle import make_golden_full_step as FS
from moleculesde_amd.synthetic import make_batch
from helpers import batch_from, load_golden, sub


def test_full_step_matches_reference_with_dropout_on():
    """Same seed => same dropout masks and noise (program-order draws): forward is bit-identical (float64 on both sides).
    The reference's gradients are stored in fixed point (step FS.GRAD_STEP * scale, rounding error at most half of it); the
    bound below is narrowed by that error, so it still means |reference - oracle| <= 1e-5 * scale for every element."""
    warnings.filterwarnings("ignore")
    g = load_golden("full_step_dropout.npz")
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        mine = FS.build(R)
        FS.set_parameters(mine)
        for k in FS.MODELS:
            assert list(mine[k].state_dict().keys()) == [str(n) for n in g[f"{k}.sd_keys"]], k
            bufs = sub(g, f"{k}.buf.")
            assert set(bufs) == set(FS.buffers(mine[k])), k
            mine[k].load_state_dict(bufs, strict=False)
        b = batch_from(g)
        o = FS.step(mine, b.clone(), int(g["seed"]))
    finally:
        torch.set_default_dtype(old)
    for name, c in zip(FS.OUTPUTS, o):
        assert c.dtype == torch.float64, name
        assert torch.allclose(torch.from_numpy(np.asarray(g[name])), c, rtol=1e-6, atol=1e-6), name
    for k in FS.MODELS:
        scale = float(g[f"{k}.grad_scale"])
        ref_grads = {n: q.double() * (scale * FS.GRAD_STEP) for n, q in sub(g, f"{k}.qgrad.").items()}
        no_grad = {str(n) for n in g[f"{k}.no_grad"]}
        assert set(ref_grads) | no_grad == {n for n, _ in mine[k].named_parameters()}, k
        assert max(v.abs().max().item() for v in ref_grads.values()) == pytest.approx(scale, rel=FS.GRAD_STEP)
        tol = (1e-5 - FS.GRAD_STEP / 2) * scale
        for n, q in mine[k].named_parameters():
            if n in no_grad:
                assert q.grad is None, (k, n)
                continue
            assert (ref_grads[n] - q.grad).abs().max().item() <= tol, (k, n)


def test_standin_semantics_equal_oracle_ops():
    """The stand-in layer used to run the reference and the oracle's own op restatements agree."""
    ns = types.SimpleNamespace(standins=ref_loader.standins())
    torch.manual_seed(1)
    b = make_batch(6, 2)
    ei_s = ns.standins.nn.radius_graph(b.positions, r=3.0, batch=b.batch)
    ei_o = R.radius_graph(b.positions, 3.0, b.batch)
    assert torch.equal(ei_s, ei_o)
    src = torch.randn(ei_o.size(1), 4)
    assert torch.allclose(ns.standins.utils.softmax(src, ei_o[1], None, b.x.size(0)),
                          R.segment_softmax(src, ei_o[1], b.x.size(0)))
    assert torch.allclose(ns.standins.scatter.scatter(src, ei_o[1], dim=0, dim_size=b.x.size(0), reduce="mean"),
                          R.scatter_mean(src, ei_o[1], b.x.size(0)))
