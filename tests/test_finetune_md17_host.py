"""Host logic of the MD17 fine-tune (moleculesde_amd/finetune_md17.py): get_idx_split, the normalisation statistics, the
schedulers, the checkpoint layouts and load_model rules, fit()'s best-epoch and final-test selection.  CPU only."""
import os

import numpy as np
import pytest
import torch

from moleculesde_amd import finetune_md17 as FM


@pytest.mark.parametrize("seed", [0, 7, 42])
@pytest.mark.parametrize("n", [2100, 5000])
def test_split_matches_sklearn_shuffle(seed, n):
    sk = pytest.importorskip("sklearn.utils")
    ids = sk.shuffle(range(n), random_state=seed)
    s = FM.md17_split(n, 1000, 1000, seed)
    assert s["train"].tolist() == list(ids[:1000])
    assert s["valid"].tolist() == list(ids[1000:2000])
    assert s["test"].tolist() == list(ids[2000:])


def test_split_pinned_prefixes():
    s = FM.md17_split(5000, seed=42)
    assert [len(s[k]) for k in ("train", "valid", "test")] == [1000, 1000, 3000]
    assert s["train"].dtype == torch.int64
    r = np.arange(5000)
    np.random.RandomState(42).shuffle(r)
    assert s["train"][:5].tolist() == r[:5].tolist()
    assert sorted(torch.cat([s["train"], s["valid"], s["test"]]).tolist()) == list(range(5000))
    assert FM.md17_split(10, 3, 3, 42)["train"].tolist() == [8, 1, 5]
    assert FM.md17_split(10, 3, 3, 0)["train"].tolist() == [2, 8, 4]


def test_normalization_bitwise_equals_script_loop():
    g = torch.Generator().manual_seed(1)
    M, NA = 37, 21
    ys = -4.06e5 + 3 * torch.randn(M, 1, generator=g)
    forces = 30 * torch.randn(M, NA, 3, generator=g)
    # finetune_MD17.py:218-232 over Data objects with y [1] and force [NA, 3]
    E_total, F_total, n_atom = 0, 0, None
    for i in range(M):
        energy, force = ys[i], forces[i]
        n_atom = force.size()[0]
        energy_mean = energy / n_atom
        E_total += energy_mean
        force_rms = torch.sqrt(torch.mean(force.square()))
        F_total += force_rms
    E_total /= M
    F_total /= M
    e, f, n = FM.energy_force_normalization(ys.view(-1), forces)
    assert n == NA
    assert torch.equal(e, E_total) and e.shape == E_total.shape
    assert torch.equal(f, F_total) and f.shape == F_total.shape


@pytest.mark.parametrize("name", ["CosineAnnealingLR", "StepLR"])
def test_scheduler_sequences_equal_torch(name):
    p = [torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))]
    opt = torch.optim.Adam([{"params": [p[0]], "lr": 5e-4}, {"params": [p[1]], "lr": 5e-4}], lr=5e-4)
    if name == "CosineAnnealingLR":
        ref = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 30)
    else:
        ref = torch.optim.lr_scheduler.StepLR(opt, step_size=7, gamma=0.5)
    ours = FM.make_scheduler(name, [5e-4, 5e-4], 30, 7, 0.5)
    for _ in range(65):
        opt.step()
        ref.step()
        assert ours.step() == [g["lr"] for g in opt.param_groups]


@pytest.mark.parametrize("name", ["CosineAnnealingWarmRestarts", "ReduceLROnPlateau"])
def test_unsupported_schedulers_refused(name):
    with pytest.raises(NotImplementedError):
        FM.make_scheduler(name, [1e-3], 10, 5, 0.5)
    assert FM.make_scheduler("None", [1e-3], 10, 5, 0.5) is None


def _nets(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2)), torch.nn.Linear(2, 1)


def _eq(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


def test_load_model_rules(tmp_path):
    m1, h1 = _nets(1)
    m2, h2 = _nets(2)
    m3, h3 = _nets(3)
    path = str(tmp_path / "ck.pth")
    # model_3D wins over model unless load_latest
    torch.save({"model_3D": m1.state_dict(), "model": m2.state_dict(), "graph_pred_linear": h1.state_dict()}, path)
    mt, ht = _nets(9)
    FM.load_state(mt, ht, path)
    assert _eq(mt, m1) and _eq(ht, h1)
    FM.load_state(mt, ht, path, load_latest=True)
    assert _eq(mt, m2)
    # no head in the file: the head stays
    torch.save({"model": m3.state_dict()}, path)
    mt, ht = _nets(9)
    h_before = {k: v.clone() for k, v in ht.state_dict().items()}
    FM.load_state(mt, ht, path)
    assert _eq(mt, m3) and all(torch.equal(h_before[k], v) for k, v in ht.state_dict().items())
    # head None (a model without graph_pred_linear)
    FM.load_state(mt, None, path)
    # the shared load_state with MD17's key order gives the same three rules
    from moleculesde_amd import finetune_common as FC
    assert FM.MD17Trainer.LOAD_KEYS == ("model_3D", "model") and FM.make_scheduler is FC.make_scheduler
    torch.save({"model_3D": m1.state_dict(), "model": m2.state_dict(), "graph_pred_linear": h1.state_dict()}, path)
    mt, ht = _nets(9)
    FC.load_state(mt, ht, path, ("model_3D", "model"))
    assert _eq(mt, m1) and _eq(ht, h1)
    FC.load_state(mt, ht, path, ("model_3D", "model"), load_latest=True)
    assert _eq(mt, m2)
    torch.save({"model": m3.state_dict()}, path)
    FC.load_state(mt, None, path, ("model_3D", "model"))
    assert _eq(mt, m3) and _eq(ht, h1)
    # the saved layout
    from moleculesde_amd.finetune_qm9 import checkpoint_dict
    assert set(checkpoint_dict(m1, h1)) == {"model", "graph_pred_linear"} and set(checkpoint_dict(m1, None)) == {"model"}


class _Stub(FM.MD17Trainer):
    """fit()'s selection with scripted MAEs: no device, no model."""

    def __init__(self, epochs, val_force, test_vals):
        self.epochs, self.train_batch_size = epochs, 1
        self.val_force, self.test_vals = list(val_force), list(test_vals)
        self.calls, self.saved, self.loaded = [], [], []
        self.weights = 0

    def train_epoch(self, split, generator=None, captured=None):
        self.weights += 1
        self.calls.append(("train", split))
        return 0.5

    def evaluate(self, split, batch_size=128, captured=None):
        self.calls.append(("eval", split, batch_size))
        if split == "valid":
            return 1.0, self.val_force[self.weights - 1]
        if split == "test":
            return self.test_vals[self.weights - 1]
        return 9.0, 9.0

    def save_model(self, path):
        self.saved.append((os.path.basename(path), self.weights))

    def load_model(self, path, load_latest=False):
        self.loaded.append((os.path.basename(path), load_latest))
        self.weights = dict(self.saved)["model.pth"]


def test_fit_selects_best_validation_epoch(tmp_path):
    st = _Stub(4, [3.0, 1.0, 2.0, 1.5], [(10, 11), (20, 21), (30, 31), (40, 41)])
    h = st.fit("train", "valid", "test", output_model_dir=str(tmp_path), eval_batch_size=64, log=None)
    assert h["best_val_idx"] == 1 and (h["best_test_energy"], h["best_test_force"]) == (20, 21)
    assert h["val_force"] == [3.0, 1.0, 2.0, 1.5] and h["train_energy"] == [0, 0, 0, 0]
    assert st.saved == [("model.pth", 1), ("model.pth", 2), ("model_final.pth", 4)]
    assert ("eval", "test", 64) in st.calls and not any(c[:2] == ("eval", "train") for c in st.calls)


def test_fit_without_test_evaluation_reloads_best(tmp_path):
    st = _Stub(3, [2.0, 3.0, 1.0], [(10, 11), (20, 21), (30, 31)])
    h = st.fit("train", "valid", "test", eval_train=True, eval_test=False, output_model_dir=str(tmp_path), log=None)
    assert st.loaded == [("model.pth", True)]
    assert h["best_val_idx"] == 2 and (h["best_test_energy"], h["best_test_force"]) == (30, 31)
    assert h["test_force"] == [0, 0, 0] and h["train_force"] == [9.0, 9.0, 9.0]
    assert ("eval", "train", 1) in st.calls


def test_fit_every_other_epoch_and_no_output_dir():
    st = _Stub(4, [3.0, 1.0, 2.0, 0.5], [(10, 11), (20, 21), (30, 31), (40, 41)])
    h = st.fit("train", "valid", "test", print_every_epoch=2, log=None)
    assert len(h["val_force"]) == 2 and h["best_val_idx"] == 1 and h["best_test_force"] == 41
    assert st.saved == []


def test_resident_split_refuses_mixed_molecules():
    x = torch.tensor([[5, 0, 0], [5, 0, 1]])
    with pytest.raises(ValueError):
        FM.ResidentSplit(x, torch.zeros(2, 3, 3), torch.zeros(2), torch.zeros(2, 3, 3), "cpu")
    s = FM.ResidentSplit(torch.tensor([[5, 0, 0], [5, 0, 0]]), torch.zeros(2, 3, 3), torch.zeros(2), torch.zeros(2, 3, 3), "cpu")
    assert len(s) == 2 and s.x.tolist() == [5, 0, 0]


def test_trainer_refuses_cpu_and_unsupported_schedulers():
    m, h = _nets(0)
    with pytest.raises(RuntimeError):
        FM.MD17Trainer(m, h)
