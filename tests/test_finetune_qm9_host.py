"""Host logic of the QM9 fine-tune (moleculesde_amd/finetune_qm9.py, bucket.pack_raw_z): splits, train statistics,
schedulers, task table, checkpoint and evaluation-file layouts, 1-D z raw blobs.  CPU only."""
import os

import numpy as np
import pytest
import torch

from moleculesde_amd import bucket as BK
from moleculesde_amd import finetune_qm9 as FQ
from moleculesde_amd.synthetic import make_qm9_batch, make_qm9_targets


# splitters.py:246-351, restated directly
def _ref_split(kind, num_mols, seed):
    np.random.seed(seed)
    all_idx = np.random.permutation(num_mols)
    Nmols = 133885 - 3054
    if kind == 1:
        Ntrain, Nvalid = 110000, 10000
    else:
        Ntrain = 100000
        Ntest = int(0.1 * Nmols)
        Nvalid = Nmols - (Ntrain + Ntest)
    return all_idx[:Ntrain], all_idx[Ntrain:Ntrain + Nvalid], all_idx[Ntrain + Nvalid:]


@pytest.mark.parametrize("seed", [0, 42])
@pytest.mark.parametrize("kind,sizes", [(1, (110000, 10000, 10831)), (2, (100000, 17748, 13083))])
def test_splits_match_splitters(seed, kind, sizes):
    fn = FQ.split_customized_01 if kind == 1 else FQ.split_customized_02
    got = fn(FQ.NUM_MOLS, seed)
    ref = _ref_split(kind, FQ.NUM_MOLS, seed)
    assert tuple(len(a) for a in got) == sizes
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    tr, va, te = (set(a.tolist()) for a in got)
    assert not (tr & va) and not (va & te) and not (tr & te)
    assert len(tr | va | te) == FQ.NUM_MOLS
    assert [np.array_equal(a, b) for a, b in zip(FQ.split(f"customized_0{kind}", FQ.NUM_MOLS, seed), got)] == [True] * 3
    with pytest.raises(ValueError):
        FQ.split("random", FQ.NUM_MOLS, seed)


def test_train_mean_std_bitwise():
    g = torch.Generator().manual_seed(3)
    rows = [torch.randn(13, generator=g) * 30 + 100 for _ in range(1037)]     # the dataset's per-molecule y [13]
    y = torch.stack(rows, dim=0)
    for t in (0, 7, 12):
        m, s = FQ.train_mean_std(y, t)
        assert m == y.mean(dim=0)[t].item() and s == y.std(dim=0)[t].item()
        assert isinstance(m, float) and isinstance(s, float)
    m, s = FQ.train_mean_std(y.numpy(), 4)
    assert m == y.mean(dim=0)[4].item() and s == y.std(dim=0)[4].item()


def _torch_lrs(make, epochs=12, lr=1e-3):
    p = torch.nn.Parameter(torch.zeros(1))
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([{"params": [p], "lr": lr}, {"params": [q], "lr": lr}], lr=lr)
    sch = make(opt)
    out = []
    for _ in range(epochs):
        opt.step()
        sch.step()
        out.append([g["lr"] for g in opt.param_groups])
    return out


def test_schedulers_match_torch():
    ref = _torch_lrs(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, 5))
    c = FQ.CosineAnnealing([1e-3, 1e-3], 5)
    assert [c.step() for _ in range(12)] == ref
    ref = _torch_lrs(lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=3, gamma=0.5))
    s = FQ.StepDecay([1e-3, 1e-3], 3, 0.5)
    assert [s.step() for _ in range(12)] == ref


def test_task_table():
    names = ["mu", "alpha", "homo", "lumo", "gap", "r2", "zpve", "u0", "u298", "h298", "g298", "cv", "gap_02"]
    assert FQ.TARGET_FIELDS == names
    for i, n in enumerate(names):
        assert FQ.task_id(n) == i
    with pytest.raises(ValueError, match="qm9"):
        FQ.task_id("qm9")
    with pytest.raises(ValueError):
        FQ.task_id("energy")


def test_checkpoint_layout_and_eval_file(tmp_path):
    model = torch.nn.Sequential(torch.nn.Linear(4, 3))
    head = torch.nn.Linear(3, 1)
    d = FQ.checkpoint_dict(model, head)
    assert set(d) == {"model", "graph_pred_linear"}
    assert set(d["model"]) == {"0.weight", "0.bias"} and set(d["graph_pred_linear"]) == {"weight", "bias"}
    assert set(FQ.checkpoint_dict(model, None)) == {"model"}
    # load: `model_3D` (a pretraining checkpoint) wins over `model`; graph_pred_linear when present
    m2, h2 = torch.nn.Sequential(torch.nn.Linear(4, 3)), torch.nn.Linear(3, 1)
    torch.save({"model_3D": model.state_dict(), "graph_pred_linear": head.state_dict()}, str(tmp_path / "a.pth"))
    FQ.load_state(m2, h2, str(tmp_path / "a.pth"))
    assert torch.equal(m2[0].weight, model[0].weight) and torch.equal(h2.weight, head.weight)
    # the shared load_state with QM9's key order: model_3D, then model; never a raw state dict
    from moleculesde_amd import finetune_common as FC
    assert FQ.QM9Trainer.LOAD_KEYS == ("model_3D", "model") and FQ.QM9Trainer.LOADS_HEAD and not FQ.QM9Trainer.RAW_OK
    assert FQ.checkpoint_dict is FC.checkpoint_dict
    other = torch.nn.Sequential(torch.nn.Linear(4, 3))
    torch.save({"model_3D": model.state_dict(), "model": other.state_dict()}, str(tmp_path / "b.pth"))
    torch.save({"model": other.state_dict()}, str(tmp_path / "c.pth"))
    for load in (lambda m, h, p: FQ.load_state(m, h, p), lambda m, h, p: FC.load_state(m, h, p, ("model_3D", "model"))):
        m3, h3 = torch.nn.Sequential(torch.nn.Linear(4, 3)), torch.nn.Linear(3, 1)
        h_before = h3.weight.clone()
        load(m3, h3, str(tmp_path / "b.pth"))
        assert torch.equal(m3[0].weight, model[0].weight) and torch.equal(h3.weight, h_before)
        load(m3, h3, str(tmp_path / "c.pth"))
        assert torch.equal(m3[0].weight, other[0].weight)
        torch.save(model.state_dict(), str(tmp_path / "raw.pth"))
        with pytest.raises(KeyError):
            load(m3, h3, str(tmp_path / "raw.pth"))
    path = FQ.save_evaluation_best(str(tmp_path), np.zeros(3), np.ones(3), np.zeros(2), np.ones(2))
    assert path == os.path.join(str(tmp_path), "evaluation_best.pth.npz") and os.path.exists(path)
    assert not os.path.exists(os.path.join(str(tmp_path), "evaluation_best.pth"))
    with np.load(path) as z:
        assert sorted(z.files) == ["test_pred", "test_target", "val_pred", "val_target"]


def test_mean_absolute_error_and_rotation_refused():
    p, t = np.array([1.0, 2.0, 4.0], np.float32), np.array([1.5, 2.0, 3.0], np.float32)
    assert FQ.mean_absolute_error(p, t) == np.mean(np.abs(p - t))
    with pytest.raises(NotImplementedError, match="rotation"):
        FQ.check_rotation_transform(True)
    FQ.check_rotation_transform(False)


def test_pack_raw_z_layout():
    b = make_qm9_batch(12, seed=5)
    y = make_qm9_targets(b, seed=1)[:, 7]
    need = BK.raw_sizes_z(b)
    assert need["E_b"] == 0 and need["E_e"] == 0 and need["B"] == 12
    caps = BK.Caps.covering([need])
    blob = BK.pack_raw_z(b, caps, y)
    lay = BK.raw_layout(caps, 1, True)
    assert blob.numel() == lay["_total"] and blob.dtype == torch.int32
    N = b.x.numel()
    o, n = lay["x"]
    assert n == caps.N and torch.equal(blob[o:o + N], b.x.to(torch.int32)) and not blob[o + N:o + n].any()
    o, _ = lay["pos"]
    assert torch.equal(blob[o:o + 3 * N].view(torch.float32), b.positions.reshape(-1))
    o, _ = lay["mol_atoms"]
    assert torch.equal(blob[o:o + 12], torch.bincount(b.batch, minlength=12).to(torch.int32))
    o, _ = lay["y"]
    assert torch.equal(blob[o:o + 12].view(torch.float32), y)
    for f in ("bond_src", "bond_dst", "bond_attr", "mol_bonds"):
        o, n = lay[f]
        assert not blob[o:o + n].any()
    # the default (pretrain) layout is unchanged by the new arguments
    assert BK.raw_layout(caps) == BK.raw_layout(caps, BK.K_ATOM, False)
    assert "y" not in BK.raw_layout(caps)


def test_pack_raw_z_refuses_oversize():
    b = make_qm9_batch(8, seed=2)
    y = torch.zeros(8)
    need = BK.raw_sizes_z(b)
    caps = BK.Caps.covering([need])
    tight = BK.Caps(8, need["N"] // 2, 0, 0, need["E_r"], need["P"], need["n_max"])      # too few atom rows
    assert tight.N < need["N"]
    with pytest.raises(BK.BucketOverflow):
        BK.pack_raw_z(b, tight, y)
    with pytest.raises(BK.BucketOverflow):                 # another batch size than the bucket's
        BK.pack_raw_z(make_qm9_batch(7, seed=2), caps, torch.zeros(7))
