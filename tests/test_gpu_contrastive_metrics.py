"""The InfoNCE_dot_prod and EBM_dot_prod contrastive kernels (csrc/contrastive_infonce.hip) against fp64 torch, their
determinism and graph capture, and the trainer paths that use them (exact-size step, captured step, pretrain.main)."""
import math
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import ROOT, assert_close, disable_dropout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _pair(N, D, seed, scale=1.0, sigma=3.3):
    """Y = 0.7 X + noise: the diagonal competes with the largest off-diagonal logits, accuracy strictly inside (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g) / math.sqrt(D) * scale
    Y = 0.7 * X + sigma * torch.randn(N, D, generator=g) / math.sqrt(D) * scale
    return X, Y


def _infonce64(X, Y, T):
    X64 = X.double().requires_grad_(True)
    Y64 = Y.double().requires_grad_(True)
    S = X64 @ Y64.T / T
    lab = torch.arange(X.shape[0])
    loss = 0.5 * (F.cross_entropy(S, lab) + F.cross_entropy(S.T, lab))
    (loss * 1.7).backward()
    return loss.detach(), S.detach(), X64.grad, Y64.grad


def _ambiguous(S):
    """Rows and columns of S whose top-two gap is below 1e-4 (1 + |max|): fp32 may pick either."""
    n = 0
    for M in (S, S.T):
        if M.shape[1] < 2:
            continue
        top = torch.topk(M, 2, dim=1).values
        n += int(((top[:, 0] - top[:, 1]) < 1e-4 * (1 + top[:, 0].abs())).sum())
    return n


def _infonce_acc64(S):
    lab = torch.arange(S.shape[0])
    return 0.5 * (float((S.argmax(1) == lab).double().mean()) + float((S.argmax(0) == lab).double().mean()))


@pytest.mark.parametrize("N,D", [(3588, 300), (560, 300), (50, 16), (7, 5), (1, 8)])
def test_infonce_kernels_vs_fp64(dev, N, D):
    from moleculesde_amd import hip
    T = 0.1
    X, Y = _pair(N, D, seed=N + D)
    ref, S, gX, gY = _infonce64(X, Y, T)
    acc_ref = _infonce_acc64(S)
    if N >= 50:
        assert 0 < acc_ref < 1, acc_ref
    Xd = X.to(dev).requires_grad_(True)
    Yd = Y.to(dev).requires_grad_(True)
    loss, acc = hip.contrastive_infonce(Xd, Yd, T)
    assert not acc.requires_grad
    assert_close(loss, ref, 1e-5, 1e-6, "InfoNCE loss")
    assert abs(float(acc) - acc_ref) * 2 * N <= _ambiguous(S) + 1e-3, (float(acc), acc_ref)
    (loss * 1.7).backward()
    assert_close(Xd.grad, gX, 1e-4, 1e-5 * float(gX.abs().max()), "InfoNCE gX")
    assert_close(Yd.grad, gY, 1e-4, 1e-5 * float(gY.abs().max()), "InfoNCE gY")


def test_infonce_large_logits(dev):
    from moleculesde_amd import hip
    T = 0.1
    X, Y = _pair(560, 300, seed=7, scale=10.0)
    ref, S, gX, gY = _infonce64(X, Y, T)
    assert float(S.abs().max()) > 500
    Xd = X.to(dev).requires_grad_(True)
    Yd = Y.to(dev).requires_grad_(True)
    loss, acc = hip.contrastive_infonce(Xd, Yd, T)
    (loss * 1.7).backward()
    assert math.isfinite(float(loss)) and bool(torch.isfinite(Xd.grad).all()) and bool(torch.isfinite(Yd.grad).all())
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    # an fp32 logit of size ~1e3 carries ~6e-5 of rounding, and exp(S - lse) that much relative error: the gradient bound
    # scales with the logits (here 10x the one of the unit-scale tests)
    assert_close(Xd.grad, gX, 1e-3, 1e-4 * float(gX.abs().max()), "InfoNCE gX (large logits)")
    assert_close(Yd.grad, gY, 1e-3, 1e-4 * float(gY.abs().max()), "InfoNCE gY (large logits)")


def test_infonce_ties_take_the_first_index(dev):
    """Small integers, T = 1: every logit is exact in fp32; duplicated rows make exact ties across tiles of 64."""
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(3)
    N, D = 150, 4
    X = torch.randint(-2, 3, (N, D), generator=g).float()
    Y = torch.randint(-2, 3, (N, D), generator=g).float()
    for a, b in ((3, 5), (10, 100), (70, 140), (0, 149)):
        X[b] = X[a]
        Y[b] = Y[a]
    S = X.double() @ Y.double().T
    lab = torch.arange(N)
    want = (int((S.argmax(1) == lab).sum()) + int((S.argmax(0) == lab).sum())) / (2 * N)
    _, acc = hip.contrastive_infonce(X.to(dev), Y.to(dev), 1.0)
    assert abs(float(acc) - want) < 1e-7, (float(acc), want)


def _ebm_shift64(X, Y, K, T):
    from moleculesde_amd import pretrain
    X64 = X.double().requires_grad_(True)
    Y64 = Y.double().requires_grad_(True)
    a = types.SimpleNamespace(CL_similarity_metric="EBM_dot_prod", CL_neg_samples=K, T=T)
    loss, acc = pretrain.dual_CL(X64, Y64, a, noise=None)
    (loss * 1.7).backward()
    with torch.no_grad():
        N = X.shape[0]
        logits = [(X64 * Y64).sum(1) / T]
        for s in range(1, K + 1):
            j = (torch.arange(N) + s) % N
            logits += [(X64 * Y64[j]).sum(1) / T, (Y64 * X64[j]).sum(1) / T]
        near0 = int((torch.cat(logits).abs() < 1e-4).sum())
    return loss.detach(), float(acc), X64.grad, Y64.grad, near0


@pytest.mark.parametrize("N,D,K", [(3588, 300, 1), (3588, 300, 3), (7, 5, 1), (7, 5, 3)])
def test_ebm_shift_kernels_vs_fp64(dev, N, D, K):
    from moleculesde_amd import hip
    T = 0.1
    X, Y = _pair(N, D, seed=N + K, sigma=1.0)
    ref, acc_ref, gX, gY, near0 = _ebm_shift64(X, Y, K, T)
    Xd = X.to(dev).requires_grad_(True)
    Yd = Y.to(dev).requires_grad_(True)
    loss, acc = hip.contrastive_ebm_shift(Xd, Yd, K, T)
    assert_close(loss, ref, 1e-5, 1e-6, "EBM_dot_prod loss")
    assert abs(float(acc) - acc_ref) * 2 * N * (1 + K) <= 2 * near0 + 1e-3, (float(acc), acc_ref)
    (loss * 1.7).backward()
    assert_close(Xd.grad, gX, 1e-4, 1e-5 * float(gX.abs().max()), "EBM_dot_prod gX")
    assert_close(Yd.grad, gY, 1e-4, 1e-5 * float(gY.abs().max()), "EBM_dot_prod gY")


@pytest.mark.parametrize("N,D", [(3588, 300), (7, 5)])
def test_ebm_shift_one_equals_the_permutation_kernel(dev, N, D):
    """K = 1 is EBM_node_dot_prod with both permutations i -> (i + 1) mod N."""
    from moleculesde_amd import hip
    X, Y = _pair(N, D, seed=5, sigma=1.0)
    perm = ((torch.arange(N) + 1) % N).to(dev)
    outs = []
    for f in (lambda x, y: hip.contrastive_ebm_shift(x, y, 1, 0.1), lambda x, y: hip.contrastive_ebm(x, y, perm, perm, 0.1)):
        Xd = X.to(dev).requires_grad_(True)
        Yd = Y.to(dev).requires_grad_(True)
        loss, acc = f(Xd, Yd)
        loss.backward()
        outs.append((loss.detach(), acc, Xd.grad, Yd.grad))
    (l1, a1, x1, y1), (l2, a2, x2, y2) = outs
    assert_close(l1, l2, 1e-6, 1e-7, "loss")
    assert float(a1) == float(a2)
    assert_close(x1, x2, 1e-6, 1e-7 * float(x2.abs().max()), "gX")
    assert_close(y1, y2, 1e-6, 1e-7 * float(y2.abs().max()), "gY")


def test_ebm_shift_rejects_k_not_below_n(dev):
    from moleculesde_amd import hip
    X = torch.randn(5, 8, device=dev)
    for K in (5, 6, 0):
        with pytest.raises(ValueError):
            hip.contrastive_ebm_shift(X, X, K, 0.1)


def _raw_calls(X, Y, N, D, kind, bufs):
    """One forward + backward through the C ABI into the given (NaN-filled) buffers."""
    from moleculesde_amd import _lib, hip
    ws, out, g, gX, gY = bufs
    if kind == "infonce":
        _lib.call("msde_cl_infonce_fwd", hip._p(X), hip._p(Y), N, D, 10.0, hip._p(ws), hip._p(out), hip._stream())
        _lib.call("msde_cl_infonce_bwd", hip._p(X), hip._p(Y), hip._p(ws), hip._p(g), N, D, 10.0, hip._p(gX), hip._p(gY),
                  hip._stream())
    else:
        _lib.call("msde_cl_ebm_shift_fwd", hip._p(X), hip._p(Y), N, D, 3, 10.0, hip._p(ws), hip._p(out), hip._stream())
        _lib.call("msde_cl_ebm_shift_bwd", hip._p(X), hip._p(Y), hip._p(ws), hip._p(g), N, D, 3, 10.0, hip._p(gX),
                  hip._p(gY), hip._stream())


@pytest.mark.parametrize("kind", ["infonce", "ebm_shift"])
def test_deterministic_and_capturable(dev, kind):
    from moleculesde_amd import _lib
    N, D = 1000, 300
    X, Y = (t.to(dev) for t in _pair(N, D, seed=11))
    nws = int(_lib.load().msde_cl_infonce_workspace_floats(N)) if kind == "infonce" else N * 7

    def fresh():
        nan = float("nan")
        return (torch.full((nws,), nan, device=dev), torch.full((2,), nan, device=dev), torch.full((1,), 1.3, device=dev),
                torch.full((N, D), nan, device=dev), torch.full((N, D), nan, device=dev))
    runs = []
    for _ in range(2):
        b = fresh()
        _raw_calls(X, Y, N, D, kind, b)
        torch.cuda.synchronize()
        runs.append(b)
    for t in (runs[0][1], runs[0][3], runs[0][4]):
        assert bool(torch.isfinite(t).all())
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    b = fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # warm-up outside the capture on the capture stream
        _raw_calls(X, Y, N, D, kind, fresh())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _raw_calls(X, Y, N, D, kind, b)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(runs[0], b):
        assert torch.equal(x, y)


# ---- the trainer -------------------------------------------------------------------------------------------------
def _cl_only_trainer(dev, metric, seed=0):
    from moleculesde_amd import pretrain
    args = pretrain.readme_args(CL_similarity_metric=metric, CL_neg_samples=2, SDE_coeff_generative_2Dto3D=0,
                                SDE_coeff_generative_3Dto2D=0, batch_size=32)
    torch.manual_seed(seed)
    return pretrain.Trainer(args, dev)


def _losses_and_grads(tr, b):
    tr.opt.zero_grad()
    loss, parts = tr.losses(b)
    tr._backward(loss)
    torch.cuda.synchronize()
    names = {id(p): f"{k}.{n}" for k, m in tr.models.items() for n, p in m.named_parameters()}
    grads = {names[id(p)]: p.grad.detach().clone() for p in tr.opt.params if p.grad is not None}
    return parts, grads


@pytest.mark.parametrize("metric", ["InfoNCE_dot_prod", "EBM_dot_prod"])
def test_trainer_contrastive_term_matches_torch_ops(dev, metric, monkeypatch):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import pretrain
    from moleculesde_amd.synthetic import make_batch
    tr = _cl_only_trainer(dev, metric)
    b = G.prepare_batch(make_batch(32, seed=4), dev)
    parts_k, g_k = _losses_and_grads(tr, b)
    monkeypatch.setattr(pretrain, "USE_FUSED_CL", False)
    parts_t, g_t = _losses_and_grads(tr, b)
    assert_close(parts_k["CL"], parts_t["CL"], 1e-5, 1e-6, "CL")
    assert abs(float(parts_k["CL_acc"]) - float(parts_t["CL_acc"])) <= 2e-3
    assert set(g_k) == set(g_t) and len(g_k) > 10
    # absolute bound from the largest gradient of the parameter's model: a bias in front of a BatchNorm has an analytically
    # zero gradient, i.e. pure rounding noise on both sides
    scale = {}
    for n, g in g_t.items():
        m = n.split(".")[0]
        scale[m] = max(scale.get(m, 0.0), float(g.abs().max()))
    for n in g_t:
        assert_close(g_k[n], g_t[n], 1e-4, 1e-5 * scale[n.split(".")[0]], n)


def test_full_step_infonce_captured_matches_eager(dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import pretrain
    from moleculesde_amd.synthetic import make_batch
    args = pretrain.readme_args(CL_similarity_metric="InfoNCE_dot_prod", SDE_coeff_generative_3Dto2D=0, batch_size=256)
    torch.manual_seed(3)
    tr_e = pretrain.Trainer(args, dev)
    tr_g = pretrain.Trainer(args, dev)
    for k in tr_e.models:
        tr_g.models[k].load_state_dict(tr_e.models[k].state_dict())
        disable_dropout(tr_e.models[k]); disable_dropout(tr_g.models[k])
    b = G.prepare_batch(make_batch(256, seed=8), dev)

    class FixedNoise(G.DeviceNoise):
        def __init__(self, n, B):
            g = torch.Generator().manual_seed(5)
            self.z = torch.randn(n, 3, generator=g).to(dev)
            self.t = torch.randint(0, 1000, (B // 2 + 1,), generator=g).to(dev)
        def randn_like(self, x): return self.z.clone()
        def randint(self, high, size, device): return self.t.clone()
        def randperm(self, n, device): raise AssertionError("InfoNCE draws no permutation")
    for tr in (tr_e, tr_g):
        tr.noise = FixedNoise(b.x.size(0), 256)
        tr.models["SDE_2Dto3D_model"].noise = tr.noise
    le, parts = tr_e.step(b)
    tr_g.step(b)
    assert all(math.isfinite(float(v)) for v in parts.values()) and math.isfinite(float(le))
    tr_g.capture(b)
    for _ in range(3):
        le, _ = tr_e.step(b)
        lg = tr_g.step_graph(b)
        assert_close(lg, le, 1e-6, 0, "graph vs eager loss")


@pytest.mark.parametrize("metric", ["InfoNCE_dot_prod", "EBM_dot_prod"])
@pytest.mark.parametrize("overlap", [True, False])
def test_new_metrics_draw_no_permutation(dev, metric, overlap):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_batch
    tr = _cl_only_trainer(dev, metric)
    tr.overlap_streams = overlap
    calls = []

    class Counting(G.DeviceNoise):
        def randperm(self, n, device):
            calls.append("randperm")
            return super().randperm(n, device)

        def randperm_pair(self, n, device):
            calls.append("randperm_pair")
            return super().randperm_pair(n, device)
    tr.noise = Counting(seed=1)
    tr.models["SDE_2Dto3D_model"].noise = tr.noise
    tr.step(G.prepare_batch(make_batch(32, seed=2), dev))
    torch.cuda.synchronize()
    assert calls == []


def test_bucket_paths_refuse_the_new_metrics(dev):
    from moleculesde_amd import pretrain
    tr = _cl_only_trainer(dev, "InfoNCE_dot_prod")
    with pytest.raises(NotImplementedError, match="InfoNCE_dot_prod"):
        tr.capture_bucket(None, None)
    tr.coeff_cl = 0                              # no contrastive term: nothing to refuse
    tr.check_bucket_metric()
    assert "EBM_node_dot_prod" in pretrain.BUCKET_CL_METRICS


def test_pretrain_main_default_flags_trains(dev):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "moleculesde_amd.pretrain", "--epochs=1", "--steps_per_epoch=2", "--batch_size=32",
           "--synthetic_pool=2"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "--eager" in r.stdout
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("CL Loss:"))
    vals = [float(v) for v in line.replace("\t", " ").split() if v.replace(".", "").replace("-", "").isdigit()]
    assert len(vals) == 4 and all(math.isfinite(v) for v in vals), line
    assert vals[0] > 0
