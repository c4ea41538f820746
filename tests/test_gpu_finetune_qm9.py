"""QM9 property fine-tune on the device (moleculesde_amd/finetune_qm9.py, csrc/qm9_head.hip, 1-D z capacity buckets): the
head kernels against fp64 restatements, the eager trainer against tests/golden/finetune_qm9.npz (produced by the
reference's own SchNet, tools/make_golden_finetune_qm9.py), the captured bucket step against the eager step, the eager
fallback, the overflow flag, PaiNN against the same step built from torch ops, and checkpoints."""
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


# ------------------------------------------------------------------------------------------- fp64 restatements ---
def head64(out, W, b, y, mean, std, mode, pred_given=None):
    """pred, yhat, loss, dpred, dout, dW, db of finetune_QM9.py:158-171 in fp64 (yhat formed in fp32, as torch forms it)."""
    yhat = ((y.float() - mean) / std).double()
    if pred_given is None:
        pred = out.double() @ W.double().view(-1) + b.double()
    else:
        pred = pred_given.double()
    B = pred.numel()
    d = pred - yhat
    if mode == "mae":
        loss, dpred = d.abs().mean(), torch.sign(d) / B
    else:
        loss, dpred = (d * d).mean(), 2 * d / B
    res = {"pred": pred, "loss": loss, "dpred": dpred}
    if pred_given is None:
        res.update(dout=dpred[:, None] * W.double().view(1, -1), dW=dpred @ out.double(), db=dpred.sum())
    return res


@pytest.mark.parametrize("mode", ["mae", "mse"])
@pytest.mark.parametrize("B", [1, 7, 128, 1000])
@pytest.mark.parametrize("D", [64, 300])
def test_head_train_kernel_vs_fp64(dev, mode, B, D):
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(B * 1000 + D)
    out = torch.randn(B, D, generator=g)
    W, b = torch.randn(1, D, generator=g) / D ** 0.5, torch.randn(1, generator=g)
    y = torch.randn(B, 13, generator=g) * 3 + 2
    mean, std = 1.5, 2.5
    yc = y[:, 4]
    r = head64(out, W, b, yc, mean, std, mode)
    yd = y.to(dev)[:, 4]                                      # strided column view: ldy = 13
    dW, db = torch.zeros(1, D, device=dev), torch.zeros(1, device=dev)
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    args = (out.to(dev), W.to(dev), b.to(dev), yd, mean, std, mode)
    pred, loss, dout = hip.qm9_head_train(*args, dW=dW, db=db, loss_acc=acc)
    assert_close(pred, r["pred"], 1e-5, 1e-5, "pred")
    assert_close(loss, r["loss"].view(1), 1e-5, 1e-7, "loss")
    assert_close(dout, r["dout"], 1e-5, 1e-9, "d out")
    assert_close(dW.view(-1), r["dW"], 1e-5, 1e-7, "dW")
    assert_close(db, r["db"].view(1), 1e-5, 1e-7, "db")
    # a second launch: bitwise equal, and the device loss sum has both losses
    dW2, db2 = torch.zeros_like(dW), torch.zeros_like(db)
    pred2, loss2, dout2 = hip.qm9_head_train(*args, dW=dW2, db=db2, loss_acc=acc)
    for a_, b_ in ((pred, pred2), (loss, loss2), (dout, dout2), (dW, dW2), (db, db2)):
        assert torch.equal(a_, b_)
    assert float(acc) == 2 * float(loss.double())


@pytest.mark.parametrize("mode", ["mae", "mse"])
def test_head_loss_only_form_and_ties(dev, mode):
    """Loss-only form (W null; the PaiNN head): dpred as torch's autograd gives it; an L1 tie (pred == yhat) gives 0."""
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(5)
    B = 129
    p = torch.randn(B, generator=g)
    y = torch.randn(B, generator=g)
    y[::3] = p[::3]                                           # exact ties: mean 0, std 1 keep yhat == y
    pd, yd = p.to(dev).requires_grad_(), y.to(dev)
    pred, loss, dpred = hip.qm9_head_train(pd.detach(), None, None, yd, 0.0, 1.0, mode)
    crit = torch.nn.L1Loss() if mode == "mae" else torch.nn.MSELoss()
    lt = crit(pd, yd)
    lt.backward()
    assert torch.equal(pred, pd.detach())
    assert_close(loss, lt.detach().view(1), 1e-6, 1e-8, "loss")
    assert_close(dpred, pd.grad, 1e-6, 1e-9, "dpred vs autograd")
    assert bool((dpred[::3] == 0).all())
    if mode == "mae":
        assert torch.equal(dpred, pd.grad)
    _, _, dpred2 = hip.qm9_head_train(pd.detach(), None, None, yd, 0.0, 1.0, mode)
    assert torch.equal(dpred, dpred2)


def test_head_eval_kernel(dev):
    from moleculesde_amd import hip
    g = torch.Generator().manual_seed(9)
    D, mean, std = 96, -3.25, 4.5
    W, b = torch.randn(1, D, generator=g) / D ** 0.5, torch.randn(1, generator=g)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    preds, ys, ref = [], [], []
    for B in (128, 77, 5):
        out = torch.randn(B, D, generator=g)
        y = torch.randn(B, generator=g) * 4 - 3
        preds.append(hip.qm9_head_eval(out.to(dev), W.to(dev), b.to(dev), y.to(dev), mean, std, acc))
        ys.append(y)
        ref.append((out @ W.view(-1) + b) * std + mean)      # fp32, as the script de-standardises
    p = torch.cat(preds).cpu()
    assert_close(p, torch.cat(ref), 1e-5, 1e-5, "de-standardised predictions")
    a = acc.cpu().tolist()
    assert a[1] == 210
    mae_np = float(np.mean(np.abs(p.numpy().astype(np.float64) - torch.cat(ys).numpy().astype(np.float64))))
    assert abs(a[0] / a[1] - mae_np) <= 1e-6 * mae_np


# ------------------------------------------------------------------------------------------ trainer vs fixture ---
def _golden_model(g, dev, loss="mae", epochs=None):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import finetune_qm9 as FQ
    from moleculesde_amd.synthetic import seeded_parameters
    m = G.SchNet(hidden_channels=int(g["emb"]), num_filters=int(g["filters"]), num_interactions=int(g["interactions"]),
                 num_gaussians=int(g["gaussians"]), cutoff=float(g["cutoff"]), readout="mean", node_class=119)
    head = torch.nn.Linear(int(g["emb"]), 1)
    seeded_parameters(m, int(g["seed"]))
    seeded_parameters(head, int(g["seed"]) + 1)
    tr = FQ.QM9Trainer(m.to(dev), head.to(dev), lr=float(g["lr"]), epochs=int(epochs or g["epochs"]), loss=loss,
                       train_mean=float(g["mean"]), train_std=float(g["std"]), task_id=int(g["task"]))
    return m, head, tr


def _golden_batches(g, dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd.batch import Batch
    out = []
    for i in range(2):
        d = sub(g, f"batch{i}.")
        y = d.pop("y")
        b = Batch(x=d["x"], positions=d["positions"], batch=d["batch"])
        b.num_graphs = y.size(0)
        out.append((G.prepare_batch(b, dev), y.to(dev)))
    return out


def _full_sd(flat):
    sd = dict(flat)
    sd.update({k.replace(".mlp.", ".conv.nn."): v for k, v in flat.items() if ".mlp." in k})
    return sd


def test_trainer_matches_reference_fixture(dev, tmp_path):
    """Two epochs over two batches (L1, Adam, CosineAnnealingLR(2)) against the reference's own SchNet + torch Adam; then
    evaluate() at the reference's parameters against the fixture's MAE, y_true and y_scores; then two MSE steps."""
    g = load_golden("finetune_qm9.npz")
    m, head, tr = _golden_model(g, dev)
    lr = float(g["lr"])
    pairs = _golden_batches(g, dev)
    before = {n: p.detach().clone() for n, p in list(m.named_parameters()) + [("head." + n, p) for n, p in head.named_parameters()]}
    rec = []

    def items():
        for it in pairs:
            yield it
            rec.append((float(tr.last_loss), tr.last_pred.clone()))
    accs = [tr.train_epoch(items()) for _ in range(int(g["epochs"]))]
    losses = [r[0] for r in rec]
    preds = torch.cat([r[1] for r in rec]).cpu()
    for s, (a, b) in enumerate(zip(losses, g["losses"])):
        assert abs(a - b) <= 1e-4 * abs(b), (s, a, b)
    assert_close(preds, g["preds"], 1e-3, 1e-4, "predictions")
    for a, b in zip(accs, g["loss_acc"]):
        assert abs(a - b) <= 1e-4 * abs(b), (accs, g["loss_acc"])
    ref_after = dict(sub(g, "sd_after."))
    ref_after.update({"head." + k: v for k, v in sub(g, "head_after.").items()})
    sd = dict(m.state_dict())
    sd.update({"head." + k: v for k, v in head.state_dict().items()})
    steps = len(losses)
    du = torch.cat([(sd[n].cpu() - before[n].cpu()).flatten() for n in before])
    dr = torch.cat([(ref_after[n] - before[n].cpu()).flatten() for n in before])
    assert float((du - dr).norm() / dr.norm()) < 2e-2
    assert float((du - dr).abs().max()) <= 2 * steps * lr * 1.001
    # evaluation at the reference's parameters, loaded through load_model's `model` layout
    torch.save({"model": _full_sd(sub(g, "sd_after.")), "graph_pred_linear": sub(g, "head_after.")}, str(tmp_path / "a.pth"))
    tr.load_model(str(tmp_path / "a.pth"))
    mae, y_true, y_scores = tr.evaluate(pairs)
    assert np.array_equal(y_true, g["eval.y_true"])
    assert_close(y_scores, g["eval.y_scores"], 1e-4, 1e-4, "eval y_scores")
    assert abs(mae - float(g["eval.mae"])) <= 1e-4 * float(g["eval.mae"]), (mae, float(g["eval.mae"]))
    # MSE: two steps from the initial parameters
    m2, head2, tr2 = _golden_model(g, dev, loss="mse")
    for s, (b, y) in enumerate(pairs):
        loss = float(tr2.step(b, y))
        assert abs(loss - g["mse.losses"][s]) <= 1e-4 * abs(g["mse.losses"][s]), (s, loss, g["mse.losses"][s])
        n0 = sum(int(p[1].size(0)) for p in pairs[:s])
        assert_close(tr2.last_pred, g["mse.preds"][n0:n0 + y.size(0)], 1e-3, 1e-4, f"mse predictions step {s}")


# ------------------------------------------------------------------------------------------ captured trainer ---------
def _stream_setup(dev, seed=11, B=16, n_full=9):
    from moleculesde_amd import bucket as BK
    from moleculesde_amd.synthetic import make_qm9_batch, make_qm9_targets
    hb = [make_qm9_batch(B, seed=100 + i) for i in range(n_full)] + [make_qm9_batch(5, seed=200)]
    for b in hb:
        b.x[b.x == 0] = 1
        del b.edge_index, b.edge_attr, b.extended_edge_index
    ys = [make_qm9_targets(b, seed=3)[:, 7].contiguous() for b in hb]
    caps = BK.Caps.covering([BK.raw_sizes_z(b) for b in hb[:n_full]])
    return hb, ys, caps


def _small_trainer(dev, seed=11):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import finetune_qm9 as FQ
    from moleculesde_amd.synthetic import seeded_parameters
    m = G.SchNet(hidden_channels=64, num_filters=128, num_interactions=3, num_gaussians=51, cutoff=10.0, readout="mean",
                 node_class=119)
    head = torch.nn.Linear(64, 1)
    seeded_parameters(m, seed)
    seeded_parameters(head, seed + 1)
    return FQ.QM9Trainer(m.to(dev), head.to(dev), lr=1e-3, epochs=10, train_mean=-10.0, train_std=5.0)


def test_captured_stream_matches_eager(dev):
    """8 fresh batches through one bucket's graph against eager steps on the same batches; two identical streamed runs are
    bitwise equal; the epoch's smaller last batch takes the eager fallback; an over-capacity blob raises BucketOverflow."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import bucket as BK, hip
    hb, ys, caps = _stream_setup(dev)
    runs = []
    for _ in range(2):
        tr = _small_trainer(dev)
        bk = tr.make_bucket(caps)
        assert bk.batch.x.dim() == 1 and bk.batch.x.dtype == torch.int64
        o = tr.opt
        before = [t.clone() for t in (o.flat_p, o.m, o.v, o.step_dev, tr.loss_acc)]
        tr.capture_bucket(bk, BK.pack_raw_z(hb[0], caps, ys[0]))
        for t, t0 in zip((o.flat_p, o.m, o.v, o.step_dev, tr.loss_acc), before):       # capturing trains nothing
            assert torch.equal(t, t0)
        losses = []
        for b, y in zip(hb[1:9], ys[1:9]):
            losses.append(tr.step_stream(bk, b, y).clone())
        p_full = tr.opt.flat_p.clone()
        losses.append(tr.step_stream(bk, hb[9], ys[9]).clone())     # 5 molecules: the eager fallback
        runs.append((tr, bk, torch.cat(losses), p_full, tr.opt.flat_p.clone()))
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][4], runs[1][4])
    ref = _small_trainer(dev)
    le = []
    for b, y in zip(hb[1:9], ys[1:9]):
        le.append(ref.step(G.prepare_batch(b.clone(), dev), y.to(dev)).clone())
    pe_full = ref.opt.flat_p.clone()
    le.append(ref.step(G.prepare_batch(hb[9].clone(), dev), ys[9].to(dev)).clone())
    le = torch.cat(le)
    tr, bk, lc, pc_full, pc = runs[0]
    assert_close(lc, le, 1e-5, 0.0, "streamed losses vs eager")
    assert float((pc_full - pe_full).norm() / pe_full.norm()) < 1e-5
    assert float((pc - ref.opt.flat_p).norm() / ref.opt.flat_p.norm()) < 1e-5
    # a blob forced past the host check: a 40-atom molecule in a bucket whose plan builder takes <= 32
    bad = BK.pack_raw_z(hb[1], caps, ys[1]).clone()
    o, _ = bk.layout["mol_atoms"]
    bad[o] = 40
    good = BK.pack_raw_z(hb[2], caps, ys[2])
    tr.step_bucket(bk, bad)
    with pytest.raises(BK.BucketOverflow):
        for _ in range(2):                                    # the poll is one call late
            tr.step_bucket(bk, good)
    hip.clear_row_bounds()


def test_bucket_train_epoch_and_eval(dev):
    """train_epoch through a bucket reads the host once and equals the mean of the streamed losses; evaluate through the
    bucket equals the exact-size evaluation."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import bucket as BK, hip
    hb, ys, caps = _stream_setup(dev, n_full=4)
    tr = _small_trainer(dev)
    bk = tr.make_bucket(caps)
    tr.capture_bucket(bk, BK.pack_raw_z(hb[0], caps, ys[0]))
    rec = []

    def items():
        for it in zip(hb, ys):
            yield it
            rec.append(float(tr.last_loss))
    acc = tr.train_epoch(items(), bucket=bk)
    assert abs(acc - float(np.mean(rec))) <= 1e-6 * abs(acc)
    mae_b, yt_b, ys_b = tr.evaluate(list(zip(hb, ys)), bucket=bk)
    mae_e, yt_e, ys_e = tr.evaluate([(G.prepare_batch(b.clone(), dev), y.to(dev)) for b, y in zip(hb, ys)])
    assert np.array_equal(yt_b, yt_e)
    assert_close(ys_b, ys_e, 1e-5, 1e-5, "bucket eval vs exact-size eval")
    assert abs(mae_b - mae_e) <= 1e-5 * mae_e
    hip.clear_row_bounds()


# ------------------------------------------------------------------------------------------ PaiNN -------------------
def test_painn_step_matches_torch_ops(dev):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import finetune_qm9 as FQ
    from moleculesde_amd.synthetic import make_qm9_batch, make_qm9_targets, seeded_parameters
    b = make_qm9_batch(6, seed=21)
    b.x[b.x == 0] = 1
    y = make_qm9_targets(b, seed=2)[:, 3].contiguous()
    mean, std, lr = 0.5, 2.0, 1e-3

    def build():
        m = G.PaiNN(n_atom_basis=32, n_interactions=2, n_rbf=20, cutoff=5.0, max_z=119, n_out=1, readout="mean")
        h = m.create_output_layers()
        seeded_parameters(m, 4)
        seeded_parameters(h, 5)
        return m.to(dev), h.to(dev)
    m1, h1 = build()
    tr = FQ.QM9Trainer(m1, h1, lr=lr, train_mean=mean, train_std=std)
    bd = G.prepare_batch(b.clone(), dev)
    yd = y.to(dev)
    loss = float(tr.step(bd, yd))
    m2, h2 = build()
    opt = torch.optim.Adam([{"params": m2.parameters(), "lr": lr}, {"params": h2.parameters(), "lr": lr}], lr=lr)
    pred = h2(m2(bd.x, bd.positions, bd.radius_edge_index, bd.batch)).squeeze()
    lt = torch.nn.L1Loss()(pred, (yd - mean) / std)
    opt.zero_grad()
    lt.backward()
    opt.step()
    assert abs(loss - float(lt)) <= 1e-5 * abs(float(lt))
    # the gradients the two steps fed Adam
    for (n, a), (_, r) in zip(list(m1.named_parameters()) + list(h1.named_parameters()),
                              list(m2.named_parameters()) + list(h2.named_parameters())):
        ga = a.grad if a.grad is not None else torch.zeros_like(a)
        assert_close(ga, r.grad, 1e-4, 1e-5 * float(r.grad.abs().max()) + 1e-12, f"grad {n}")
    # the first Adam step is lr * g / (|g| + eps): entries whose gradient is rounding noise (analytically zero) move by up to
    # +-lr in either step, as in test_gpu_finetune_molnet; the update as a whole vector agrees
    p1 = torch.cat([p.detach().flatten() for p in list(m1.parameters()) + list(h1.parameters())])
    p2 = torch.cat([p.detach().flatten() for p in list(m2.parameters()) + list(h2.parameters())])
    p0 = torch.cat([p.detach().flatten() for p in list(build()[0].parameters()) + list(build()[1].parameters())])
    assert float((p1 - p2).norm() / (p2 - p0).norm()) < 2e-2
    assert float((p1 - p2).abs().max()) <= 2 * lr * 1.001


# ------------------------------------------------------------------------------------------ checkpoints -------------
def test_checkpoints_roundtrip(dev, tmp_path):
    from oracle import restate as R
    tr = _small_trainer(dev)
    path = str(tmp_path / "model.pth")
    tr.save_model(path)
    w = torch.load(path, map_location="cpu")
    assert set(w) == {"model", "graph_pred_linear"}
    om = R.SchNet(hidden_channels=64, num_filters=128, num_interactions=3, num_gaussians=51, cutoff=10.0, readout="mean",
                  node_class=119)
    om.load_state_dict(w["model"], strict=True)
    oh = torch.nn.Linear(64, 1)
    oh.load_state_dict(w["graph_pred_linear"], strict=True)
    tr2 = _small_trainer(dev, seed=99)
    tr2.load_model(path)
    for (n, a), (_, b) in zip(tr.model.state_dict().items(), tr2.model.state_dict().items()):
        assert torch.equal(a, b), n
    assert torch.equal(tr.head.weight, tr2.head.weight) and torch.equal(tr.head.bias, tr2.head.bias)
    # a pretraining checkpoint (pretrain.Trainer.save layout): the encoder comes from model_3D, the head stays
    tr3 = _small_trainer(dev, seed=7)
    hw = tr3.head.weight.detach().clone()
    torch.save({"model_2D": {}, "model_3D": tr.model.state_dict(), "SDE_2Dto3D_model": {}}, str(tmp_path / "pre.pth"))
    tr3.load_model(str(tmp_path / "pre.pth"))
    for (n, a), (_, b) in zip(tr.model.state_dict().items(), tr3.model.state_dict().items()):
        assert torch.equal(a, b), n
    assert torch.equal(tr3.head.weight, hw)
