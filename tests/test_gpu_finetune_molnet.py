"""MoleculeNet fine-tune on the device (moleculesde_amd/finetune_molnet.py, csrc/molnet_head.hip, msde_dropout_rows_*):
the head kernels and the row dropout against fp64 restatements (poisoned padding past the row bound included), the trainer
against tests/golden/finetune_molnet.npz (produced by the reference's own GNN, tools/make_golden_finetune_molnet.py), the
trainer with dropout 0.5 against fp64 with the host-mirrored masks, GIN on 33- to 150-atom molecules, the NaN skip,
repeatability and evaluation."""
import numpy as np
import pytest
import torch

from helpers import assert_close, batch_from, load_golden, sub

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------- fp64 restatements ---
def _bn(z, sd, pre, train):
    if train:
        mu, var = z.mean(0), z.var(0, unbiased=False)
    else:
        mu, var = sd[pre + "running_mean"], sd[pre + "running_var"]
    return (z - mu) / torch.sqrt(var + 1e-5) * sd[pre + "weight"] + sd[pre + "bias"]


def gin64(sd, b, L, train=True, masks=None, p=0.0):
    """molecule_gnn_model.py:13-32,168-197 (GIN, JK last) in fp64 on the host; sd: fp64 leaf tensors (grads flow);
    masks[l]: boolean keep mask of layer l (dropout scale 1 / (1 - p))."""
    x, ei, ea = b.x.cpu(), b.edge_index.cpu(), b.edge_attr.cpu()
    h = sum(sd[f"atom_encoder.atom_embedding_list.{k}.weight"][x[:, k]] for k in range(x.size(1)))
    for l in range(L):
        g = f"gnns.{l}."
        ee = sum(sd[f"{g}bond_encoder.bond_embedding_list.{k}.weight"][ea[:, k]] for k in range(ea.size(1)))
        agg = torch.zeros_like(h).index_add(0, ei[1], torch.relu(h[ei[0]] + ee))
        z = (1 + sd[g + "eps"]) * h + agg
        z = z @ sd[g + "mlp.0.weight"].T + sd[g + "mlp.0.bias"]
        z = torch.relu(_bn(z, sd, g + "mlp.1.", train))
        z = z @ sd[g + "mlp.3.weight"].T + sd[g + "mlp.3.bias"]
        z = _bn(z, sd, f"batch_norms.{l}.", train)
        if l < L - 1:
            z = torch.relu(z)
        if masks is not None and train and p > 0:
            z = z * torch.from_numpy(masks[l]).double() / (1.0 - p)
        h = z
    return h


def head64(h, mol_ptr, W, bias, y):
    """global_mean_pool + Linear + the script's masked fp64 BCE (finetune_MoleculeNet.py:121-141)."""
    mp = mol_ptr.tolist()
    pool = torch.stack([h[mp[i]:mp[i + 1]].mean(0) if mp[i + 1] > mp[i] else h.new_zeros(h.size(1)) for i in range(len(mp) - 1)])
    logits = pool @ W.T + bias
    yy = y.double()
    valid = yy ** 2 > 0
    lm = torch.nn.functional.binary_cross_entropy_with_logits(logits, (yy + 1) / 2, reduction="none")
    lm = torch.where(valid, lm, torch.zeros_like(lm))
    return logits, lm, lm.sum() / valid.sum()


def _sd64(model, head=None):
    sd = {k: v.detach().double().cpu().clone().requires_grad_(v.is_floating_point() and "running" not in k
                                                            and "num_batches" not in k)
          for k, v in model.state_dict().items()}
    if head is not None:
        sd["head.weight"] = head.weight.detach().double().cpu().clone().requires_grad_(True)
        sd["head.bias"] = head.bias.detach().double().cpu().clone().requires_grad_(True)
    return sd


def _grads_close_l2(named, ref, rel_l2, what):
    """Relative L2 error of every gradient <= rel_l2 of the larger of its own norm and 1e-3 of the largest norm (biases
    in front of a BatchNorm have an analytically zero gradient: rounding noise on both sides)."""
    nmax = max(float(v.norm()) for v in ref.values() if v is not None)
    for n, g in named:
        r = ref[n]
        assert g is not None and r is not None, f"{what}: {n} has no gradient"
        err = float((g.double().cpu() - r).norm())
        den = max(float(r.norm()), 1e-3 * nmax)
        assert err <= rel_l2 * den, f"{what}:{n}: rel L2 {err / den:.3e}"


# ------------------------------------------------------------------------------------------------ head kernels ---
def _ragged(sizes, D, pad, seed, device):
    g = torch.Generator().manual_seed(seed)
    N = int(sum(sizes))
    h = torch.randn(N + pad, D, generator=g)
    h[N:] = float("nan")                                  # poisoned padding past the row bound
    mol_ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32)
    return h, mol_ptr, N


@pytest.mark.parametrize("T,B,D", [(1, 128, 300), (12, 32, 37), (617, 64, 384)])
def test_head_kernels_vs_fp64(dev, T, B, D):
    from moleculesde_amd import hip
    rng = np.random.default_rng(T + B)
    sizes = rng.integers(1, 40, size=B)
    sizes[0], sizes[1], sizes[-1] = 1, 150, 97
    h, mol_ptr, N = _ragged(sizes, D, pad=45, seed=T, device=dev)
    g = torch.Generator().manual_seed(7 + T)
    W = torch.randn(T, D, generator=g) / D ** 0.5
    bias = torch.randn(T, generator=g) * 0.3
    y = torch.from_numpy(np.where(rng.random((B, T)) < 0.3, 1.0, -1.0) * (rng.random((B, T)) > 0.25)).float()
    y[3, :] = 0.0                                         # a molecule with every label missing
    if T > 1:
        y[:, T // 2] = 0.0                                # a task column with every label missing
    bound = torch.tensor([N], dtype=torch.int32, device=dev)

    hd = h.to(dev).requires_grad_(True)
    Wd, bd = W.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    logits = hip.molnet_head(hd, Wd, bd, mol_ptr.to(dev), bound)
    stats, dlog, lm = hip.molnet_bce(logits.detach(), y.to(dev), want_loss_mat=True)
    logits.backward(dlog)

    h64 = h[:N].double().requires_grad_(True)
    W64, b64 = W.double().requires_grad_(True), bias.double().requires_grad_(True)
    l64, lm64, loss64 = head64(h64, mol_ptr, W64, b64, y)
    loss64.backward()
    assert_close(logits, l64.detach(), 1e-4, 1e-5, "logits")
    assert_close(lm, lm64.detach(), 1e-4, 1e-6, "loss_mat")
    st = stats.cpu()
    assert abs(float(st[0]) - float(loss64)) <= 1e-5 * abs(float(loss64)), (float(st[0]), float(loss64))
    assert int(st[1]) == int((y ** 2 > 0).sum()) and int(st[2]) == 0
    gs = float(h64.grad.abs().max())
    assert_close(hd.grad[:N], h64.grad, 1e-4, 1e-5 * gs, "grad h")
    assert torch.equal(hd.grad[N:].cpu(), torch.zeros(45, D)), "rows past the bound get no gradient"
    assert_close(Wd.grad, W64.grad, 1e-4, 1e-5 * float(W64.grad.abs().max()), "grad W")
    assert_close(bd.grad, b64.grad, 1e-4, 1e-6, "grad b")
    # bitwise repeatable
    logits2 = hip.molnet_head(hd.detach(), Wd.detach(), bd.detach(), mol_ptr.to(dev), bound)
    stats2, dlog2, _ = hip.molnet_bce(logits2, y.to(dev))
    assert torch.equal(logits2, logits.detach()) and torch.equal(stats2, stats) and torch.equal(dlog2, dlog)


def test_bce_without_valid_label_is_nan_with_zero_gradient(dev):
    """0 / 0 as the reference: the loss is NaN, d loss / d logits is 0 everywhere (torch.where backward)."""
    from moleculesde_amd import hip
    logits = torch.randn(4, 3, device=dev)
    stats, dlog, _ = hip.molnet_bce(logits, torch.zeros(4, 3, device=dev))
    st = stats.cpu()
    assert np.isnan(float(st[0])) and int(st[1]) == 0 and int(st[2]) == 0
    assert torch.equal(dlog.cpu(), torch.zeros(4, 3))
    logits[1, 2] = float("nan")
    stats, _, _ = hip.molnet_bce(logits, torch.ones(4, 3, device=dev))
    assert int(stats[2].item()) == 1


# --------------------------------------------------------------------------------------------------- dropout ---
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_dropout_rows_mask_equals_host_mirror(dev, p):
    from moleculesde_amd import hip
    from moleculesde_amd.finetune_molnet import dropout_keep_mask
    M, D, seed, layer, step = 777, 300, 1234, 2, 5
    x = (torch.rand(M, D) + 0.5).to(dev).requires_grad_(True)
    sdev = torch.tensor([step], dtype=torch.int64, device=dev)
    y = hip.dropout_rows(x, p, seed, layer, sdev)
    keep = dropout_keep_mask(seed, layer, step, M, D, p)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    ref = x.detach().cpu().numpy() * scale * keep
    assert np.array_equal(y.detach().cpu().numpy(), ref.astype(np.float32))
    n = M * D
    assert abs(keep.mean() - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5        # binomial bound
    g = torch.randn(M, D, device=dev)
    y.backward(g)
    assert np.array_equal(x.grad.cpu().numpy(), (g.cpu().numpy() * scale * keep).astype(np.float32)), "backward mask"
    # another step / layer: another mask; p = 0: the identity
    y2 = hip.dropout_rows(x.detach(), p, seed, layer, torch.tensor([step + 1], dtype=torch.int64, device=dev))
    assert not torch.equal((y2 != 0).cpu(), (y != 0).cpu())
    y3 = hip.dropout_rows(x.detach(), p, seed, layer + 1, sdev)
    assert not torch.equal((y3 != 0).cpu(), (y != 0).cpu())
    assert torch.equal(hip.dropout_rows(x.detach(), 0.0, seed, layer, sdev), x.detach())


def test_dropout_rows_leaves_rows_past_the_bound(dev):
    from moleculesde_amd import _lib, hip
    from moleculesde_amd._torchabi import _p, _stream
    from moleculesde_amd.finetune_molnet import dropout_keep_mask
    M, D, N = 64, 37, 50
    x = torch.randn(M, D, device=dev)
    bound = torch.tensor([N], dtype=torch.int32, device=dev)
    y = hip.dropout_rows(x, 0.5, 9, 0, None, bound)
    keep = dropout_keep_mask(9, 0, None, N, D, 0.5)
    assert np.array_equal(y[:N].cpu().numpy(), (x[:N].cpu().numpy() * np.float32(2) * keep).astype(np.float32))
    assert torch.equal(y[N:], x[N:])
    z = x.clone()                                          # in place
    _lib.call("msde_dropout_rows_fwd", _p(z), M, D, _p(bound), 0.5, 9, 0, _p(None), _p(z), _stream())
    assert torch.equal(z, y)


def _small_gnn(dev, L=3, D=32, drop=0.5, seed=0):
    import moleculesde_amd.geom3d as G
    torch.manual_seed(seed)
    return G.GNN(L, D, JK="last", drop_ratio=drop, gnn_type="GIN").to(dev)


def test_gnn_without_opt_in_calls_f_dropout(dev, monkeypatch):
    import moleculesde_amd.geom3d as G
    import moleculesde_amd.geom3d.gnn as gnn_mod
    from moleculesde_amd.synthetic import make_molnet_batch
    calls = []
    real = gnn_mod.F.dropout

    def spy(h, p, training=True, inplace=False):
        calls.append((p, training))
        return real(h, p, training=training)
    monkeypatch.setattr(gnn_mod.F, "dropout", spy)
    m = _small_gnn(dev).train()
    assert m.device_dropout is None
    b = G.prepare_batch(make_molnet_batch(6, 3, seed=2), dev)
    m(b.x, b.edge_index, b.edge_attr)
    assert calls == [(0.5, True)] * 3


def _trainer(dev, drop, seed=0, T=12, L=3, D=32, lr=1e-3):
    from moleculesde_amd.finetune_molnet import MoleculeNetTrainer
    m = _small_gnn(dev, L, D, drop, seed)
    torch.manual_seed(seed + 1)
    head = torch.nn.Linear(D, T).to(dev)
    return MoleculeNetTrainer(m, head, lr=lr, epochs=10, seed=77)


def test_trainer_never_reaches_f_dropout(dev, monkeypatch):
    import moleculesde_amd.geom3d as G
    import moleculesde_amd.geom3d.gnn as gnn_mod
    from moleculesde_amd.synthetic import make_molnet_batch

    def boom(*a, **k):
        raise AssertionError("F.dropout reached")
    tr = _trainer(dev, 0.5)
    monkeypatch.setattr(gnn_mod.F, "dropout", boom)
    b = G.prepare_batch(make_molnet_batch(8, 12, seed=4), dev)
    for _ in range(2):
        assert np.isfinite(tr.step(b))
    tr.evaluate([b])


# ------------------------------------------------------------------------------------------ trainer vs fixture ---
def test_trainer_matches_reference_fixture(dev, tmp_path):
    """Three steps at dropout 0 against the reference's own GNN + torch Adam (tools/make_golden_finetune_molnet.py); then
    evaluate() against the fixture's eval-mode logits and an fp64 restatement."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import finetune_molnet as FM
    g = load_golden("finetune_molnet.npz")
    L, D, lr = int(g["num_layer"]), int(g["emb"]), float(g["lr"])
    T = g["batch.y"].shape[1]
    m = G.GNN(L, D, JK="last", drop_ratio=0, gnn_type="GIN")
    m.load_state_dict(sub(g, "sd."))
    head = torch.nn.Linear(D, T)
    head.load_state_dict(sub(g, "head."))
    tr = FM.MoleculeNetTrainer(m.to(dev), head.to(dev), lr=lr, epochs=100)
    before = {n: p.detach().clone() for n, p in list(m.named_parameters()) + [("head." + n, p) for n, p in head.named_parameters()]}
    b = G.prepare_batch(batch_from(g), dev)
    for s in range(3):
        loss = tr.step(b)
        assert not tr.last_skipped
        assert abs(loss - g["losses"][s]) <= 1e-4 * abs(g["losses"][s]), (s, loss, g["losses"][s])
        assert_close(tr.last_logits, g["logits"][s], 1e-3, 1e-4, f"logits step {s}")
    ref_after = dict(sub(g, "sd_after."))
    ref_after.update({"head." + k: v for k, v in sub(g, "head_after.").items()})
    sd = dict(m.state_dict())
    sd.update({"head." + k: v for k, v in head.state_dict().items()})
    for k, v in ref_after.items():
        if "running" in k:
            # every BatchNorm here follows a Linear (mlp.0 -> mlp.1, mlp.3 -> batch_norms) whose bias has an analytically zero
            # gradient: Adam turns rounding noise into +-lr moves on both sides, which reach the running mean through the
            # momentum (0.1) -- at most 0.1 * 2 * steps * lr apart; the running variance does not see them
            atol = 0.1 * 2 * 3 * lr if k.endswith("running_mean") else 1e-5
            assert_close(sd[k], v, 1e-4, atol, k)
        elif "num_batches_tracked" in k:
            assert int(sd[k]) == int(v) == 3, k
    # parameters: the update (after - before) as a whole vector; per entry within the Adam step bound
    du = torch.cat([(sd[n].cpu() - before[n].cpu()).flatten() for n in before])
    dr = torch.cat([(ref_after[n] - before[n].cpu()).flatten() for n in before])
    assert float((du - dr).norm() / dr.norm()) < 2e-2
    assert float((du - dr).abs().max()) <= 2 * 3 * lr * 1.001
    # evaluation, at the reference's parameters after the steps (the pre-BatchNorm biases above differ by rounding noise x lr,
    # which eval mode -- running statistics -- does not cancel); they load through load_model's `model` layout
    torch.save({"model": {k: v for k, v in sub(g, "sd_after.").items()}}, str(tmp_path / "after.pth"))
    tr.load_model(str(tmp_path / "after.pth"))
    head.load_state_dict(sub(g, "head_after."))
    mean, y_true, y_scores = tr.evaluate([b])
    assert_close(y_scores, g["eval.logits"], 1e-4, 1e-5, "eval logits vs fixture")
    sd64 = _sd64(m, head)
    with torch.no_grad():
        l64, _, _ = head64(gin64(sd64, b, L, train=False), b._msde_plan.mol_ptr.cpu(), sd64["head.weight"],
                           sd64["head.bias"], torch.from_numpy(g["batch.y"]))
    assert_close(y_scores, l64, 1e-4, 1e-5, "eval logits vs fp64")
    m64, _ = FM.roc_auc_tasks(g["batch.y"], l64.numpy(), g["batch.y"] ** 2 > 0)
    assert mean == pytest.approx(m64, abs=1e-12)
    assert np.array_equal(y_true, g["batch.y"])


# ----------------------------------------------------------------------------------------------- dropout 0.5 ---
def test_trainer_step_with_dropout_vs_fp64(dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.finetune_molnet import dropout_keep_mask
    from moleculesde_amd.synthetic import make_molnet_batch
    L, D, T, p = 3, 32, 12, 0.5
    tr = _trainer(dev, p, seed=3, T=T, L=L, D=D)
    b = G.prepare_batch(make_molnet_batch(16, T, seed=8, sizes=[40, 7, 150, 12, 33, 3, 18, 25, 61, 9, 14, 2, 22, 35, 11, 5]), dev)
    sd64 = _sd64(tr.model, tr.head)
    N = b.x.size(0)
    masks = [dropout_keep_mask(tr.seed, l, 1, N, D, p) for l in range(L)]      # the first step runs with counter 1
    loss = tr.step(b)
    h = gin64(sd64, b, L, masks=masks, p=p)
    _, _, loss64 = head64(h, b._msde_plan.mol_ptr.cpu(), sd64["head.weight"], sd64["head.bias"], b.y.cpu())
    loss64.backward()
    assert abs(loss - float(loss64)) <= 1e-4 * abs(float(loss64)), (loss, float(loss64))
    named = [(n, p_.grad) for n, p_ in tr.model.named_parameters()] + [("head.weight", tr.head.weight.grad),
                                                                       ("head.bias", tr.head.bias.grad)]
    _grads_close_l2(named, {n: sd64[n].grad for n, _ in named}, 1e-3, "dropout step")
    assert int(tr.seed_dev.item()) == 1


# ---------------------------------------------------------------------------------------- GIN on large molecules ---
def test_gin_on_33_to_150_atom_molecules_vs_fp64(dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_molnet_batch
    L, D = 5, 64
    m = _small_gnn(dev, L, D, 0.0, seed=5).train()
    sizes = [33, 150, 47, 96, 64, 128, 35, 80]
    b = G.prepare_batch(make_molnet_batch(len(sizes), 1, seed=12, sizes=sizes), dev)
    sd64 = _sd64(m)
    out = m(b.x, b.edge_index, b.edge_attr)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    (out * r.to(dev)).sum().backward()
    h64 = gin64(sd64, b, L)
    (h64 * r.double()).sum().backward()
    assert_close(out, h64.detach(), 1e-3, 1e-4, "GIN out")
    _grads_close_l2([(n, p.grad) for n, p in m.named_parameters()], {n: sd64[n].grad for n, _ in m.named_parameters()},
                    1e-3, "GIN large molecules")


# ----------------------------------------------------------------------------------------- NaN skip, repeatability ---
def test_nan_step_is_skipped(dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_molnet_batch
    tr = _trainer(dev, 0.5, seed=6)
    b = G.prepare_batch(make_molnet_batch(8, 12, seed=9), dev)
    tr.step(b)
    with torch.no_grad():
        tr.head.bias[3] = float("nan")
    snap = [t.clone() for t in (tr.opt.flat_p, tr.opt.m, tr.opt.v, tr.opt.step_dev)]
    grads = [p.grad.clone() for p in tr.opt.params]
    tr.step(b)
    assert tr.last_skipped
    for a, s in zip((tr.opt.flat_p, tr.opt.m, tr.opt.v, tr.opt.step_dev), snap):
        assert torch.equal(a.nan_to_num(), s.nan_to_num())
    assert int(tr.opt.step_dev.item()) == 1
    assert all(torch.equal(p.grad, g_) for p, g_ in zip(tr.opt.params, grads)), "no zero_grad / backward on a skipped step"


def test_two_identical_runs_are_bitwise_equal(dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_molnet_batch
    batches = [G.prepare_batch(make_molnet_batch(32, 617, seed=s), dev) for s in (1, 2)]
    runs = []
    for _ in range(2):
        tr = _trainer(dev, 0.5, seed=11, T=617, D=64)
        losses = [tr.step(bb) for bb in batches + batches]
        tr.scheduler_step()
        runs.append((losses, tr.opt.flat_p.clone(), tr.opt.m.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_scheduler_writes_device_rates(dev):
    tr = _trainer(dev, 0.0, lr=2e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=2e-4), 10)
    for _ in range(4):
        sch.optimizer.step()
        sch.step()
        tr.scheduler_step()
    want = torch.tensor([sch.get_last_lr()[0]] * 2, dtype=torch.float32)
    assert torch.equal(tr.opt.seg_lr.cpu(), want)


def test_checkpoint_round_trip(dev, tmp_path):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import make_molnet_batch
    tr = _trainer(dev, 0.0, seed=2)
    b = G.prepare_batch(make_molnet_batch(8, 12, seed=3), dev)
    tr.step(b)
    path = str(tmp_path / "model.pth")
    tr.save_model(path)
    w = torch.load(path)
    assert set(w) == {"model", "graph_pred_linear"}
    tr2 = _trainer(dev, 0.0, seed=9)
    tr2.load_model(path)
    for k, v in tr.model.state_dict().items():
        assert torch.equal(tr2.model.state_dict()[k], v), k
    torch.save({"model_2D": tr.model.state_dict()}, str(tmp_path / "pre.pth"))
    tr3 = _trainer(dev, 0.0, seed=10)
    tr3.load_model(str(tmp_path / "pre.pth"))
    tr3.head.load_state_dict(tr.head.state_dict())
    tr.model.eval(); tr3.model.eval()
    with torch.no_grad():
        assert torch.equal(tr3.forward(b), tr.forward(b))
