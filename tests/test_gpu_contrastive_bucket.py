"""InfoNCE_dot_prod and EBM_dot_prod on capacity buckets: the row-bounded entry points msde_cl_infonce_{fwd,bwd}_rows and
msde_cl_ebm_shift_{fwd,bwd}_rows (csrc/contrastive_infonce.hip) at a row CAPACITY C with the valid count c on the device,
against fp64 torch over the first c rows, and the trainer paths that use them behind --captured_cl.

The four entry points take their bound as `const int* n_rows`, a name the header scan of
tests/test_host_logic.py::test_every_row_bounded_entry_point_has_a_row_bound_test does not pick up, so they are not keys of
BOUNDED in tests/test_gpu_row_bounds.py; the tests here are written to that file's standard with its own driver (`drive`):
rows >= c of X and Y are NaN, every output and workspace is NaN-filled before each call, a bound equal to C is bit-equal to a
NULL bound and to the unbounded entry point, two runs are bit-equal, and one graph captured at C is replayed after writing C,
the smallest and a middle count into the device count."""
import math
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import ROOT, assert_close, disable_dropout
from test_gpu_row_bounds import Ops, close, drive, same, zero_rows

pytestmark = pytest.mark.gpu

NAN = float("nan")
C = 200                                     # four 64-row tiles, the last one holding 8 rows
INFONCE_COUNTS = [1, 2, 63, 64, 65, 128, 129, 163, 200]
INFONCE_SEED = {20: 1, 70: 2}               # per depth; _infonce_data() documents how a seed qualifies (70: seed 1 does not)
EBM_COUNTS = [4, 33, 163, 200]
EBM_SEED = {1: 1, 3: 1}                     # per K
T = 0.1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _p(t):
    from moleculesde_amd import hip
    return hip._p(t)


def _st():
    from moleculesde_amd import hip
    return hip._stream()


def _call(name, *args):
    from moleculesde_amd import _lib
    _lib.call(name, *args)


def _nan_ops(dev, bases):
    """Ops over the given host tensors whose prep(c) restores them and then turns rows >= c into NaN."""
    ops = Ops(dev, 0)
    tens = []
    for base in bases:
        t = base.to(dev)
        ops.items.append((t, base))
        tens.append(t)
    prep0 = ops.prep

    def prep(c):
        prep0(c)
        for t in tens:
            t[c:] = NAN
    ops.prep = prep
    return ops, tens


def _infonce64(X, Y, T):
    """tests/test_gpu_contrastive_metrics.py::_infonce64: dual InfoNCE in fp64, gradients of 1.7 * loss."""
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


def _infonce_data(D, seed):
    """Y = 0.7 X + noise (the diagonal competes with the largest off-diagonal logits: accuracy strictly inside (0, 1) for the
    larger counts).  A seed qualifies when, for every count c, no row or column of S[:c, :c] has a top-two gap under
    1e-4 (1 + |max|) in fp64 -- the test asserts it before it compares accuracies to 1e-6."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(C, D, generator=g) / math.sqrt(D)
    Y = 0.7 * X + 3.3 * torch.randn(C, D, generator=g) / math.sqrt(D)
    return X, Y


@pytest.mark.parametrize("D", [20, 70])
def test_infonce_bounded(dev, D):
    """msde_cl_infonce_fwd_rows / _bwd_rows: loss, accuracy and gX / gY over the first c rows against fp64; gradient rows
    behind the bound exactly zero; identities and graph replay as in the module docstring.  D = 20: one backward column tile,
    K no multiple of 16; D = 70: a second, partial column tile."""
    from moleculesde_amd import _lib
    Xc, Yc = _infonce_data(D, INFONCE_SEED[D])
    ops, (X, Y) = _nan_ops(dev, [Xc, Yc])
    gl = torch.tensor([1.7], device=dev)
    nws = int(_lib.load().msde_cl_infonce_workspace_floats(C))
    bufs = {"ws": torch.empty(nws, device=dev), "out": torch.empty(2, device=dev), "gX": torch.empty(C, D, device=dev),
            "gY": torch.empty(C, D, device=dev)}
    refs = {}
    for c in INFONCE_COUNTS:                       # fp64 references, once
        loss, S, gX, gY = _infonce64(Xc[:c], Yc[:c], T)
        refs[c] = (loss, _infonce_acc64(S), gX, gY, _ambiguous(S))

    def launch(b):
        _call("msde_cl_infonce_fwd_rows", _p(X), _p(Y), C, D, 1.0 / T, _p(bufs["ws"]), _p(bufs["out"]), _p(b), _st())
        _call("msde_cl_infonce_bwd_rows", _p(X), _p(Y), _p(bufs["ws"]), _p(gl), C, D, 1.0 / T, _p(bufs["gX"]), _p(bufs["gY"]),
              _p(b), _st())

    def check(c):
        loss, acc, gX, gY, amb = refs[c]
        print(f"InfoNCE D={D} c={c}: loss {float(bufs['out'][0]):.7f} vs {float(loss):.7f}, acc {float(bufs['out'][1]):.6f} vs "
              f"{acc:.6f}, max|gX err| {float((bufs['gX'][:c].double().cpu() - gX).abs().max()):.2e} of {float(gX.abs().max()):.2e}")
        close(bufs["out"][0], loss, 1e-5, 1e-6, f"InfoNCE loss c={c}")
        close(bufs["gX"][:c], gX, 1e-4, 1e-5 * float(gX.abs().max()), f"InfoNCE gX c={c}")
        close(bufs["gY"][:c], gY, 1e-4, 1e-5 * float(gY.abs().max()), f"InfoNCE gY c={c}")
        zero_rows(bufs["gX"], c, f"InfoNCE gX c={c}"), zero_rows(bufs["gY"], c, f"InfoNCE gY c={c}")
        assert torch.isfinite(bufs["out"]).all(), f"InfoNCE out c={c}"
        assert amb == 0, f"seed {INFONCE_SEED[D]}: {amb} ambiguous rows / columns at c={c}"
        assert abs(float(bufs["out"][1]) - acc) < 1e-6, (c, float(bufs["out"][1]), acc)

    drive(dev, C, INFONCE_COUNTS, bufs, launch, check, ops)
    # a NULL bound is the unbounded entry point, bit for bit
    ops.prep(C)
    got = {}
    for name in ("new", "old"):
        for t in bufs.values():
            t.fill_(NAN)
        if name == "new":
            launch(None)
        else:
            _call("msde_cl_infonce_fwd", _p(X), _p(Y), C, D, 1.0 / T, _p(bufs["ws"]), _p(bufs["out"]), _st())
            _call("msde_cl_infonce_bwd", _p(X), _p(Y), _p(bufs["ws"]), _p(gl), C, D, 1.0 / T, _p(bufs["gX"]), _p(bufs["gY"]),
                  _st())
        torch.cuda.synchronize()
        got[name] = {k: v.clone() for k, v in bufs.items()}
    for k in bufs:
        assert same(got["new"][k], got["old"][k]), f"{k}: msde_cl_infonce_*_rows(NULL) differs from msde_cl_infonce_*"
    check(C)


def _ebm_data(K, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(C, 20, generator=g) / math.sqrt(20)
    Y = 0.7 * X + torch.randn(C, 20, generator=g) / math.sqrt(20)
    return X, Y


def _ebm_shift64(X, Y, K, wrap=False):
    """fp64 dual EBM_dot_prod over all rows of X, Y: pretrain.dual_CL (the torch-op restatement of examples/util.py), or with
    wrap=True a restatement whose shifts are taken modulo the row count (K >= rows: the kernels' memory-safety contract).
    Returns loss, accuracy, gradients of 1.7 * loss, and the number of logits within 1e-4 of zero (fp32 may take either sign)."""
    from moleculesde_amd import pretrain
    n = X.shape[0]
    X64 = X.double().requires_grad_(True)
    Y64 = Y.double().requires_grad_(True)
    idx = [(torch.arange(n) + s) % n for s in range(1, K + 1)]
    if wrap:
        bce = F.binary_cross_entropy_with_logits
        loss, hits = 0.0, 0.0
        for A, B in ((X64, Y64), (Y64, X64)):
            pos = (A * B).sum(1) / T
            neg = torch.cat([(A * B[j]).sum(1) / T for j in idx])
            loss = loss + bce(pos, torch.ones_like(pos)) + K * bce(neg, torch.zeros_like(neg))
            hits += (float((pos > 0).sum()) + float((neg < 0).sum())) / (pos.numel() + neg.numel())
        loss, acc = loss / 2, hits / 2
    else:
        a = types.SimpleNamespace(CL_similarity_metric="EBM_dot_prod", CL_neg_samples=K, T=T)
        loss, acc = pretrain.dual_CL(X64, Y64, a, noise=None)
    (loss * 1.7).backward()
    with torch.no_grad():
        logits = [(X64 * Y64).sum(1) / T]
        for j in idx:
            logits += [(X64 * Y64[j]).sum(1) / T, (Y64 * X64[j]).sum(1) / T]
        near0 = int((torch.cat(logits).abs() < 1e-4).sum())
    return loss.detach(), float(acc), X64.grad, Y64.grad, near0


def _ebm_case(dev, K, counts, seed, wrap=False, replay=True):
    D = 20
    Xc, Yc = _ebm_data(K, seed)
    ops, (X, Y) = _nan_ops(dev, [Xc, Yc])
    gl = torch.tensor([1.7], device=dev)
    bufs = {"rows": torch.empty(C, 1 + 2 * K, device=dev), "out": torch.empty(2, device=dev),
            "gX": torch.empty(C, D, device=dev), "gY": torch.empty(C, D, device=dev)}
    refs = {c: _ebm_shift64(Xc[:c], Yc[:c], K, wrap) for c in counts}

    def launch(b):
        _call("msde_cl_ebm_shift_fwd_rows", _p(X), _p(Y), C, D, K, 1.0 / T, _p(bufs["rows"]), _p(bufs["out"]), _p(b), _st())
        _call("msde_cl_ebm_shift_bwd_rows", _p(X), _p(Y), _p(bufs["rows"]), _p(gl), C, D, K, 1.0 / T, _p(bufs["gX"]),
              _p(bufs["gY"]), _p(b), _st())

    def check(c):
        loss, acc, gX, gY, near0 = refs[c]
        print(f"EBM_dot_prod K={K} c={c}: loss {float(bufs['out'][0]):.7f} vs {float(loss):.7f}, acc {float(bufs['out'][1]):.6f} "
              f"vs {acc:.6f}, max|gX err| {float((bufs['gX'][:c].double().cpu() - gX).abs().max()):.2e} of {float(gX.abs().max()):.2e}")
        close(bufs["out"][0], loss, 1e-5, 1e-6, f"EBM_dot_prod loss c={c}")
        close(bufs["gX"][:c], gX, 1e-4, 1e-5 * float(gX.abs().max()), f"EBM_dot_prod gX c={c}")
        close(bufs["gY"][:c], gY, 1e-4, 1e-5 * float(gY.abs().max()), f"EBM_dot_prod gY c={c}")
        zero_rows(bufs["gX"], c, f"EBM_dot_prod gX c={c}"), zero_rows(bufs["gY"], c, f"EBM_dot_prod gY c={c}")
        assert torch.isfinite(bufs["out"]).all(), f"EBM_dot_prod out c={c}"
        assert torch.isfinite(bufs["rows"]).all(), f"rows c={c}: padded logits not written"
        assert near0 == 0, f"seed {seed}: {near0} logits within 1e-4 of zero at c={c}"
        assert abs(float(bufs["out"][1]) - acc) < 1e-6, (c, float(bufs["out"][1]), acc)

    drive(dev, C, counts, bufs, launch, check, ops, replay=replay)
    return ops, X, Y, gl, bufs, launch, check


@pytest.mark.parametrize("K", [1, 3])
def test_ebm_shift_bounded(dev, K):
    """msde_cl_ebm_shift_fwd_rows / _bwd_rows against the fp64 dual_CL over the first c rows: shifts wrap modulo c, divisors use
    c, gradient rows behind the bound exactly zero, `rows` finite everywhere; identities and graph replay as in the module
    docstring."""
    ops, X, Y, gl, bufs, launch, check = _ebm_case(dev, K, EBM_COUNTS, EBM_SEED[K])
    D = 20
    ops.prep(C)
    got = {}
    for name in ("new", "old"):
        for t in bufs.values():
            t.fill_(NAN)
        if name == "new":
            launch(None)
        else:
            _call("msde_cl_ebm_shift_fwd", _p(X), _p(Y), C, D, K, 1.0 / T, _p(bufs["rows"]), _p(bufs["out"]), _st())
            _call("msde_cl_ebm_shift_bwd", _p(X), _p(Y), _p(bufs["rows"]), _p(gl), C, D, K, 1.0 / T, _p(bufs["gX"]),
                  _p(bufs["gY"]), _st())
        torch.cuda.synchronize()
        got[name] = {k: v.clone() for k, v in bufs.items()}
    for k in bufs:
        assert same(got["new"][k], got["old"][k]), f"{k}: msde_cl_ebm_shift_*_rows(NULL) differs from msde_cl_ebm_shift_*"
    check(C)


def test_ebm_shift_more_shifts_than_rows_is_memory_safe(dev):
    """c = 2 valid rows, K = 3 shifts: the host cannot reject it (the count is on the device), the kernels take (i +- s) mod c.
    Compared with the torch restatement whose indices are taken mod c; every buffer NaN-filled, padded rows NaN."""
    _ebm_case(dev, 3, [2], EBM_SEED[3], wrap=True, replay=False)


# ---- the trainer -------------------------------------------------------------------------------------------------
def _trainer(dev, metric, full, seed=31, **over):
    from moleculesde_amd import pretrain
    kw = dict(emb_dim=64, CL_similarity_metric=metric, CL_neg_samples=2, captured_cl=True)
    if not full:
        kw.update(SDE_coeff_generative_2Dto3D=0, SDE_coeff_generative_3Dto2D=0)
    kw.update(over)
    args = pretrain.readme_args(**kw)
    torch.manual_seed(seed)
    tr = pretrain.Trainer(args, dev)
    tr.overlap_streams = False
    for m in tr.models.values():
        disable_dropout(m)
    return tr


@pytest.mark.parametrize("full", [False, True], ids=["cl_only", "full"])
@pytest.mark.parametrize("metric", ["InfoNCE_dot_prod", "EBM_dot_prod"])
def test_one_graph_serves_different_batches_captured_cl(dev, metric, full):
    """tests/test_gpu_plan.py::test_one_graph_serves_different_batches with --captured_cl and the two metrics: ONE captured
    bucket step replayed on different batches, each compared with the eager step on the exact-size batch from the same state
    (logged losses within 5e-5 |ref| + 1e-7, cosine of the two parameter updates > 0.995: that test's bounds)."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import bucket as BK, hip
    from moleculesde_amd.synthetic import make_batch
    tr = _trainer(dev, metric, full)
    tr.check_bucket_metric()                       # the flag is set: nothing to refuse

    class Noise(G.DeviceNoise):
        """Position noise / time steps from fixed device tensors (padding independent, capturable)."""

        def __init__(self):
            super().__init__(seed=77)
            g = torch.Generator().manual_seed(5)
            self.big = torch.randn(8192, 3, generator=g).to(dev)
            self.ints = torch.randint(0, 1000, (4096,), generator=g).to(dev)

        def randn_like(self, x):
            assert x.dim() == 2 and x.size(1) == 3
            return self.big[:x.size(0)].clone()

        def randint(self, high, size, device):
            return self.ints[:size[0]].clone()

        def randperm(self, n, device):
            raise AssertionError(f"{metric} draws no permutation")

        def randperm_pair(self, n, device):
            raise AssertionError(f"{metric} draws no permutation")
    noise = Noise()
    head_noise = G.DeviceNoise(seed=99)
    tr.noise = noise
    if "SDE_2Dto3D_model" in tr.models:
        tr.models["SDE_2Dto3D_model"].noise = noise
    if "SDE_3Dto2D_model" in tr.models:            # the dense head must see a DeviceNoise (in-kernel draws)
        tr.models["SDE_3Dto2D_model"].noise = head_noise

    cpu = [make_batch(40, seed=s) for s in (51, 52, 53)]
    needs = [BK.raw_sizes(b) for b in cpu]
    caps = BK.Caps.covering(needs, n_max=24)
    bk = tr.make_bucket(caps)
    blobs = [BK.pack_raw(b, caps).to(dev) for b in cpu]
    tr.capture_bucket(bk, blobs[0])
    snap = lambda: (tr.opt.flat_p.clone(), tr.opt.m.clone(), tr.opt.v.clone(), tr.opt.step_dev.clone(),
                    tr.step_counter.clone(), {k: {n: v.clone() for n, v in m.state_dict().items()} for k, m in tr.models.items()})

    def restore(s):
        tr.opt.flat_p.copy_(s[0]); tr.opt.m.copy_(s[1]); tr.opt.v.copy_(s[2]); tr.opt.step_dev.copy_(s[3])
        tr.step_counter.copy_(s[4])
        for k, m in tr.models.items():
            m.load_state_dict(s[5][k])
    calls = (noise.calls, head_noise.calls)
    try:
        for i in (1, 2, 0):
            s0 = snap()
            for k in tr.log:
                tr.log[k].zero_()
            tr.step_bucket(bk, blobs[i])
            torch.cuda.synchronize()
            ok, sizes = bk.check()
            assert ok and sizes["N"] == needs[i]["N"] and sizes["E_e"] == needs[i]["E_e"], sizes
            got_log = {k: float(v) for k, v in tr.log.items()}
            got_p = tr.opt.flat_p.clone()
            restore(s0)
            # eager step on the exact-size batch with the host plan; host-side draw counters as they were at capture time
            noise.calls, head_noise.calls = calls[0] - 1, calls[1] - 1
            for k in tr.log:
                tr.log[k].zero_()
            exact = G.prepare_batch(cpu[i].clone(), dev)
            tr.step(exact)
            torch.cuda.synchronize()
            assert math.isfinite(got_log["CL"]) and got_log["CL"] > 0, got_log
            for k in got_log:
                ref = float(tr.log[k])
                print(f"{metric} full={full} batch {i} {k}: bucket {got_log[k]:.8g} exact {ref:.8g}")
                assert abs(got_log[k] - ref) <= 5e-5 * abs(ref) + 1e-7, (i, k, got_log[k], ref)
            ua, ub = (got_p - s0[0]).double(), (tr.opt.flat_p - s0[0]).double()
            cos = float((ua * ub).sum() / (ua.norm() * ub.norm()))
            print(f"{metric} full={full} batch {i}: cosine of the two updates {cos:.6f}")
            assert cos > 0.995, (i, cos)
    finally:
        hip.clear_row_bounds()


def test_step_stream_rejects_more_shifts_than_atoms(dev):
    """EBM_dot_prod on a bucket: the kernels see the capacity, so CL_neg_samples >= the batch's atom count is refused where the
    host batch is known."""
    from moleculesde_amd import bucket as BK, hip
    from moleculesde_amd.synthetic import make_batch
    cpu_b = make_batch(4, seed=3)
    need = BK.raw_sizes(cpu_b)
    tr = _trainer(dev, "EBM_dot_prod", False, CL_neg_samples=need["N"])
    tr.check_bucket_metric()
    bk = tr.make_bucket(BK.Caps.covering([need], n_max=24))
    try:
        with pytest.raises(ValueError, match="CL_neg_samples"):
            tr.step_stream(bk, cpu_b)
    finally:
        hip.clear_row_bounds()


def test_pretrain_main_captured_cl_trains(dev):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "moleculesde_amd.pretrain", "--captured_cl", "--epochs=1", "--steps_per_epoch=2",
           "--batch_size=32", "--synthetic_pool=2"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "--eager" not in r.stdout and "exact-size batches" not in r.stdout, r.stdout[-2000:]
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("CL Loss:"))
    vals = [float(v) for v in line.replace("\t", " ").split() if v.replace(".", "").replace("-", "").isdigit()]
    assert len(vals) == 4 and all(math.isfinite(v) for v in vals), line
    assert vals[0] > 0
    assert "0 fell back" in r.stdout, r.stdout[-2000:]
