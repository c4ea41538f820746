"""MD17 fine-tuning epochs on the device (moleculesde_amd/finetune_md17.py MD17Trainer, csrc/md17.hip): the evaluation,
loss-with-sum and gather kernels against restatements, two eager epochs of fit() against tests/golden/finetune_md17.npz
(produced by the reference's own SchNet, tools/make_golden_finetune_md17.py), the captured train epoch and evaluation
against their eager forms, evaluation leaving the training state alone, PaiNN against the same loop from torch ops, and
checkpoints."""
import numpy as np
import pytest
import torch

from helpers import assert_close, load_golden, sub

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------- kernels ---
def eval64(E, y, dE, f):
    """eval()'s sums in fp64: |E - y| with the difference formed in fp32, forces -dE with NaN entries dropped."""
    se = (E.float() - y.float()).double().abs().sum()
    F = -dE.float()
    keep = ~torch.isnan(F)
    sf = (F[keep] - f.float()[keep]).double().abs().sum()
    return float(se), float(E.numel()), float(sf), float(keep.sum())


@pytest.mark.parametrize("B", [1, 7, 128])
@pytest.mark.parametrize("case", ["plain", "nan_force", "nan_energy", "md17_scale", "md17_scale_norm"])
def test_eval_accumulate_vs_fp64(dev, B, case):
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(B * 31 + len(case))
    NA = 21
    E, y = torch.randn(B, generator=g), torch.randn(B, generator=g)
    dE, f = torch.randn(B * NA * 3, generator=g), torch.randn(B * NA * 3, generator=g)
    if case == "nan_force":
        dE[torch.randperm(dE.numel(), generator=g)[:max(1, dE.numel() // 10)]] = float("nan")
    if case == "nan_energy":
        E[B // 2] = float("nan")
    if case.startswith("md17_scale"):
        # aspirin energies are about -4e5 kcal/mol; forces of order 30
        y = -4.06e5 + 5 * torch.randn(B, generator=g)
        E = y + 3 * torch.randn(B, generator=g)
        dE, f = 30 * dE, 30 * f
        if case == "md17_scale_norm":
            e_mean, f_mean = torch.tensor([-1.93e4]), torch.tensor(28.5)
            E = torch.randn(B, generator=g) * f_mean + e_mean * NA
    acc = torch.zeros(4, dtype=torch.float64, device=dev)
    hip.md17_eval_accumulate(E.to(dev), y.to(dev), dE.to(dev), f.to(dev), acc)
    hip.md17_eval_accumulate(E.to(dev), y.to(dev), dE.to(dev), f.to(dev), acc)    # accumulates
    got = acc.cpu().tolist()
    ref = eval64(E, y, dE, f)
    for a, r, name in zip(got, [2 * v for v in ref], ("sum |dE|", "molecules", "sum |dF|", "kept forces")):
        if case == "nan_energy" and name == "sum |dE|":
            assert np.isnan(a)
        else:
            assert abs(a - r) <= 1e-12 * abs(r) + 1e-12, (name, a, r)
    # bitwise repeatable
    acc2 = torch.zeros(4, dtype=torch.float64, device=dev)
    for _ in range(2):
        hip.md17_eval_accumulate(E.to(dev), y.to(dev), dE.to(dev), f.to(dev), acc2)
    assert torch.equal(acc.nan_to_num(), acc2.nan_to_num())


@pytest.mark.parametrize("B,NA", [(1, 21), (7, 21), (128, 21), (64, 32)])
def test_loss_acc_bitwise_equals_loss_kernel(dev, B, NA):
    from moleculesde_amd import _lib, hip
    g = torch.Generator().manual_seed(B + NA)
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    total = 0.0
    for s in range(3):
        E, y = torch.randn(B, generator=g).to(dev), torch.randn(B, generator=g).to(dev)
        dE, f = torch.randn(B * NA * 3, generator=g).to(dev), torch.randn(B * NA * 3, generator=g).to(dev)
        loss = torch.empty(1, device=dev)
        gE, gd = torch.empty_like(E), torch.empty_like(dE)
        _lib.call("msde_l1_energy_force_loss", hip._p(E), hip._p(y), B, hip._p(dE), hip._p(f), dE.numel(), -1.0, 0.05, 0.95,
                  hip._p(loss), hip._p(gE), hip._p(gd), hip._stream())
        l2, gE2, gd2 = hip.l1_energy_force_loss_acc(E, y, dE, f, -1.0, 0.05, 0.95, acc)
        assert torch.equal(loss, l2) and torch.equal(gE, gE2) and torch.equal(gd, gd2)
        total += float(np.float64(loss.item()))
    assert float(acc.item()) == total


@pytest.mark.parametrize("with_perm", [False, True])
def test_gather_batch_matches_indexing(dev, with_perm):
    from moleculesde_amd import hip
    M, NA, B = 23, 21, 5                       # 4 full batches and a remainder of 3
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(M, NA, 3, generator=g).to(dev)
    y = torch.randn(M, generator=g).to(dev)
    force = torch.randn(M, NA, 3, generator=g).to(dev)
    perm = torch.randperm(M, generator=g).to(dev, torch.int32) if with_perm else None
    order = perm.long() if with_perm else torch.arange(M, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    dp, dy, df = torch.full((B * NA, 3), -7.0, device=dev), torch.full((B,), -7.0, device=dev), torch.full((B * NA, 3), -7.0, device=dev)
    for k in range(M // B):
        hip.md17_gather_batch(pos, y, force, perm, ctr, B, dp, dy, df)
        idx = order[k * B:(k + 1) * B]
        assert torch.equal(dp, pos[idx].view(-1, 3)) and torch.equal(dy, y[idx]) and torch.equal(df, force[idx].view(-1, 3))
    assert int(ctr.item()) == M // B
    # the short last batch through a B = 3 buffer with the full batches' stride
    r = M % B
    rp, ry, rf = torch.full((r * NA, 3), -7.0, device=dev), torch.full((r,), -7.0, device=dev), torch.full((r * NA, 3), -7.0, device=dev)
    hip.md17_gather_batch(pos, y, force, perm, ctr, B, rp, ry, rf)
    idx = order[(M // B) * B:]
    assert torch.equal(rp, pos[idx].view(-1, 3)) and torch.equal(ry, y[idx]) and torch.equal(rf, force[idx].view(-1, 3))
    # a full-size buffer past the end: only the valid rows are written, the rest keep what they held
    ctr.fill_(M // B)
    dp.fill_(-7.0); dy.fill_(-7.0)
    hip.md17_gather_batch(pos, y, force, perm, ctr, B, dp, dy, df)
    assert torch.equal(dp[:r * NA], pos[idx].view(-1, 3)) and bool((dp[r * NA:] == -7.0).all())
    assert torch.equal(dy[:r], y[idx]) and bool((dy[r:] == -7.0).all())
    assert int(ctr.item()) == M // B + 1


# ------------------------------------------------------------------------------------------ trainer vs fixture ---
def _model(g, dev, seed_offset=0):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.synthetic import seeded_parameters
    m = G.SchNet(hidden_channels=int(g["emb"]), num_filters=int(g["filters"]), num_interactions=int(g["interactions"]),
                 num_gaussians=int(g["gaussians"]), cutoff=float(g["cutoff"]), readout="mean", node_class=119)
    head = torch.nn.Linear(int(g["emb"]), 1)
    seeded_parameters(m, int(g["seed"]) + seed_offset)
    seeded_parameters(head, int(g["seed"]) + 1 + seed_offset)
    return m.to(dev), head.to(dev)


def _splits(g, dev, kind):
    from moleculesde_amd.finetune_md17 import ResidentSplit
    return [ResidentSplit(torch.as_tensor(g["x"]), torch.as_tensor(g[n + ".pos"]), torch.as_tensor(g[n + ".y_" + kind]),
                          torch.as_tensor(g[n + ".f_" + kind]), dev) for n in ("train", "valid", "test")]


def _trainer(g, dev, kind, seed_offset=0, captured=True, **kw):
    from moleculesde_amd import finetune_md17 as FM
    m, head = _model(g, dev, seed_offset)
    norm = None
    if kind == "norm":
        norm = FM.energy_force_normalization(torch.as_tensor(g["train.y_norm"]), torch.as_tensor(g["train.f_norm"]))
        assert np.array_equal(norm[0].numpy(), g["norm.e_mean"]) and np.array_equal(norm[1].numpy(), g["norm.f_mean"])
        assert norm[2] == int(g["norm.n_atom"])
    tr = FM.MD17Trainer(m, head, lr=float(g["lr"]), epochs=int(g["epochs"]), normalization=norm,
                        train_batch_size=int(g["train_bs"]), **kw)
    tr.captured = captured
    return tr


def _full_sd(flat):
    sd = dict(flat)
    sd.update({k.replace(".mlp.", ".conv.nn."): v for k, v in flat.items() if ".mlp." in k})
    return sd


@pytest.mark.parametrize("kind", ["raw", "norm"])
def test_fit_matches_reference_fixture(dev, kind, tmp_path):
    """Two eager epochs of fit() (train batch 2 with a short last batch, evaluation batch 3 with short last batches)
    against the reference's SchNet + torch Adam + CosineAnnealingLR(2): step losses, loss_acc, parameters, and the
    validation / test MAEs of both epochs; then the best-epoch selection and the checkpoints it wrote."""
    g = load_golden("finetune_md17.npz")
    tr = _trainer(g, dev, kind, captured=False)
    train, valid, test = _splits(g, dev, kind)
    before = {n: p.detach().clone() for n, p in list(tr.model.named_parameters()) +
              [("head." + n, p) for n, p in tr.head.named_parameters()]}
    rec = []
    step = tr.step

    def recording_step(split, idx):
        loss = step(split, idx)
        rec.append(float(loss))
        return loss
    tr.step = recording_step
    h = tr.fit(train, valid, test, eval_batch_size=int(g["eval_bs"]), output_model_dir=str(tmp_path),
               generator=torch.Generator().manual_seed(int(g["perm_seed"])), log=None)
    ref_losses = g[kind + ".losses"]
    assert len(rec) == len(ref_losses)
    for s, (a, b) in enumerate(zip(rec, ref_losses)):
        assert abs(a - b) <= 1e-4 * abs(b), (s, a, b)
    for a, b in zip(h["loss"], g[kind + ".loss_acc"]):
        assert abs(a - b) <= 1e-4 * abs(b), (h["loss"], g[kind + ".loss_acc"])
    eabs = 0.07 if kind == "norm" else 0.0      # energies near 4e5: fp32 spacing 0.03
    for name, ref in (("val", g[kind + ".val"]), ("test", g[kind + ".test"])):
        for e in range(2):
            ge, gf = h[name + "_energy"][e], h[name + "_force"][e]
            assert abs(ge - ref[e][0]) <= 1e-4 * abs(ref[e][0]) + eabs, (name, e, ge, ref[e][0])
            assert abs(gf - ref[e][1]) <= 1e-4 * abs(ref[e][1]), (name, e, gf, ref[e][1])
    ref_after = dict(sub(g, kind + ".sd_after."))
    ref_after.update({"head." + k: v for k, v in sub(g, kind + ".head_after.").items()})
    sd = dict(tr.model.state_dict())
    sd.update({"head." + k: v for k, v in tr.head.state_dict().items()})
    lr, steps = float(g["lr"]), len(rec)
    du = torch.cat([(sd[n].cpu() - before[n].cpu()).flatten() for n in before])
    dr = torch.cat([(ref_after[n] - before[n].cpu()).flatten() for n in before])
    assert float((du - dr).norm() / dr.norm()) < 2e-2
    assert float((du - dr).abs().max()) <= 2 * steps * lr * 1.001
    best = int(np.argmin([v[1] for v in g[kind + ".val"]]))
    assert h["best_val_idx"] == best
    assert h["best_test_force"] == h["test_force"][best]
    import os
    assert os.path.exists(tmp_path / "model.pth") and os.path.exists(tmp_path / "model_final.pth")
    w = torch.load(str(tmp_path / "model_final.pth"), map_location="cpu")
    assert set(w) == {"model", "graph_pred_linear"}
    # evaluation at the reference's final parameters, loaded through load_model's `model` layout
    torch.save({"model": _full_sd(sub(g, kind + ".sd_after.")), "graph_pred_linear": sub(g, kind + ".head_after.")},
               str(tmp_path / "ref.pth"))
    tr.load_model(str(tmp_path / "ref.pth"))
    te = tr.evaluate(test, int(g["eval_bs"]), captured=False)
    ref = g[kind + ".test"][-1]
    assert abs(te[0] - ref[0]) <= 1e-5 * abs(ref[0]) + eabs and abs(te[1] - ref[1]) <= 1e-5 * abs(ref[1]), (te, ref)


def _state(tr):
    o = tr.opt
    grads = [None if p.grad is None else p.grad.clone() for p in o.params]
    return [t.clone() for t in (o.flat_p, o.m, o.v, o.step_dev)], grads


def _same_state(a, b):
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for x, y in zip(a[1], b[1]):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("kind", ["raw", "norm"])
def test_captured_epoch_and_evaluation_match_eager(dev, kind):
    """The captured train epoch (gather kernel + one replayed step per batch, short last batch eager) and the captured
    evaluation (one graph per batch size) against the eager forms: losses and MAEs within 1e-6 relative; two captured
    evaluations are bitwise equal; evaluation leaves parameters, Adam state and .grad untouched."""
    g = load_golden("finetune_md17.npz")
    train, valid, test = _splits(g, dev, kind)
    res = {}
    for captured in (False, True):
        tr = _trainer(g, dev, kind, captured=captured)
        if captured:                      # capturing the train graph (warm-up steps included) trains nothing
            o, bs = tr.opt, tr.train_batch_size
            before = [t.clone() for t in (o.flat_p, o.m, o.v, o.step_dev, tr.loss_acc)]
            first = tr._capture(train, "train", bs, bs)
            assert first.keys is not None
            for t, t0 in zip((o.flat_p, o.m, o.v, o.step_dev, tr.loss_acc), before):
                assert torch.equal(t, t0)
        out = []
        gen = torch.Generator().manual_seed(5)
        for _ in range(2):
            out.append(tr.train_epoch(train, generator=gen, captured=captured))
            st = _state(tr)
            out.extend(tr.evaluate(valid, 3, captured=captured))
            out.extend(tr.evaluate(test, 128, captured=captured))       # one short batch only
            out.extend(tr.evaluate(train, 1, captured=captured))        # --eval_train at batch size 1
            _same_state(st, _state(tr))
        if captured:
            again = tr.evaluate(valid, 3)
            assert again == tuple(out[-6:-4]), (again, out[-6:-4])
        res[captured] = (out, torch.cat([p.detach().flatten() for p in tr.opt.params]).cpu())
    for a, b in zip(res[True][0], res[False][0]):
        assert abs(a - b) <= 1e-6 * abs(b) + 1e-9, (res[True][0], res[False][0])
    assert_close(res[True][1], res[False][1], 1e-5, 1e-6, "parameters after two epochs")


def test_painn_epoch_and_evaluation_match_torch_ops(dev):
    """PaiNN (eager): one train epoch (batch 2, a short last batch) and an evaluation against the same loop built from
    torch ops on the same device: energies, forces by autograd.grad, L1 losses, torch.optim.Adam over two groups."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import finetune_md17 as FM
    from moleculesde_amd.synthetic import seeded_parameters
    g = load_golden("finetune_md17.npz")
    train, valid, _ = _splits(g, dev, "raw")
    lr = 1e-3

    def build():
        m = G.PaiNN(n_atom_basis=32, n_interactions=2, n_rbf=20, cutoff=5.0, max_z=119, n_out=1, readout="mean")
        h = m.create_output_layers()
        seeded_parameters(m, 4)
        seeded_parameters(h, 5)
        return m.to(dev), h.to(dev)
    m1, h1 = build()
    tr = FM.MD17Trainer(m1, h1, lr=lr, epochs=3, train_batch_size=2)
    gen = torch.Generator().manual_seed(9)
    loss_acc = tr.train_epoch(train, generator=gen)
    mae = tr.evaluate(valid, 3)

    m2, h2 = build()
    opt = torch.optim.Adam([{"params": m2.parameters(), "lr": lr}, {"params": h2.parameters(), "lr": lr}], lr=lr)
    order = torch.randperm(len(train), generator=torch.Generator().manual_seed(9)).to(dev)

    def batch_of(split, idx):
        pos, y, f = split.rows(idx)
        b = tr._template(split, int(idx.numel()))
        tr._painn_edges(b, pos)
        return b, pos.clone().requires_grad_(True), y, f
    losses = []
    for k in range(0, len(train), 2):
        b, pos, y, f = batch_of(train, order[k:k + 2])
        e = h2(m2(b.x, pos, b.radius_edge_index, b.batch)).squeeze(1)
        force = -torch.autograd.grad(e, pos, grad_outputs=torch.ones_like(e), create_graph=True, retain_graph=True)[0]
        loss = 0.05 * torch.nn.functional.l1_loss(e, y) + 0.95 * torch.nn.functional.l1_loss(force, f)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert abs(loss_acc - np.mean(losses)) <= 1e-4 * abs(np.mean(losses)), (loss_acc, losses)
    pe, ae, pf, af = [], [], [], []
    ar = torch.arange(len(valid), device=dev)
    for k in range(0, len(valid), 3):
        b, pos, y, f = batch_of(valid, ar[k:k + 3])
        e = h2(m2(b.x, pos, b.radius_edge_index, b.batch)).squeeze(1)
        force = -torch.autograd.grad(e, pos, grad_outputs=torch.ones_like(e))[0]
        pe.append(e.detach()); ae.append(y); pf.append(force); af.append(f)
    ref = (float((torch.cat(pe) - torch.cat(ae)).abs().mean()), float((torch.cat(pf) - torch.cat(af)).abs().mean()))
    # the parameters differ by at most the Adam updates' rounding after three steps
    assert abs(mae[0] - ref[0]) <= 2e-2 * abs(ref[0]) and abs(mae[1] - ref[1]) <= 2e-2 * abs(ref[1]), (mae, ref)


def test_checkpoints_roundtrip(dev, tmp_path):
    from oracle import restate as R
    g = load_golden("finetune_md17.npz")
    tr = _trainer(g, dev, "raw")
    path = str(tmp_path / "model.pth")
    tr.save_model(path)
    w = torch.load(path, map_location="cpu")
    assert set(w) == {"model", "graph_pred_linear"}
    om = R.SchNet(hidden_channels=int(g["emb"]), num_filters=int(g["filters"]), num_interactions=int(g["interactions"]),
                  num_gaussians=int(g["gaussians"]), cutoff=float(g["cutoff"]), readout="mean", node_class=119)
    om.load_state_dict(w["model"], strict=True)
    tr2 = _trainer(g, dev, "raw", seed_offset=50)
    tr2.load_model(path)
    for (n, a), (_, b) in zip(tr.model.state_dict().items(), tr2.model.state_dict().items()):
        assert torch.equal(a, b), n
    assert torch.equal(tr.head.weight, tr2.head.weight)
    # the loaded parameters are what the captured evaluation reads
    _, valid, _ = _splits(g, dev, "raw")
    assert tr2.evaluate(valid, 3) == tr.evaluate(valid, 3)
    tr3 = _trainer(g, dev, "raw", seed_offset=60)
    hw = tr3.head.weight.detach().clone()
    torch.save({"model_3D": tr.model.state_dict(), "model": tr3.model.state_dict()}, str(tmp_path / "pre.pth"))
    tr3.load_model(str(tmp_path / "pre.pth"))
    for (n, a), (_, b) in zip(tr.model.state_dict().items(), tr3.model.state_dict().items()):
        assert torch.equal(a, b), n
    assert torch.equal(tr3.head.weight, hw)
