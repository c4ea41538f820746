"""Host-side pieces of the MoleculeNet fine-tune (moleculesde_amd/finetune_molnet.py), no GPU: ROC-AUC and the script's skip
rules (examples/finetune_MoleculeNet.py:159-210), the cosine learning rates, the checkpoint layouts (:71-102), the host mirror
of the dropout mask, num_tasks, and the synthetic MoleculeNet-shaped batch."""
import numpy as np
import pytest
import torch

from moleculesde_amd import finetune_common as FC
from moleculesde_amd import finetune_molnet as FM
from moleculesde_amd.synthetic import make_molnet_batch


def _sklearn_auc():
    try:
        from sklearn.metrics import roc_auc_score
    except ImportError:
        return None
    return roc_auc_score


# ---------------------------------------------------------------------------------------------------------- ROC-AUC ---
def test_roc_auc_hand_computed_with_ties():
    assert FM.roc_auc_score([0, 0, 1, 1], [0.1, 0.4, 0.35, 0.8]) == pytest.approx(0.75)
    # every score tied: 0.5
    assert FM.roc_auc_score([0, 1, 0, 1, 1], [2.0] * 5) == pytest.approx(0.5)
    # one positive tied with one of two negatives, above the other: (1 + 0.5) / 2
    assert FM.roc_auc_score([1, 0, 0], [0.3, 0.3, 0.1]) == pytest.approx(0.75)
    # perfect and inverted orderings
    assert FM.roc_auc_score([0, 0, 1], [-3.0, -1.0, 5.0]) == 1.0
    assert FM.roc_auc_score([1, 1, 0], [-3.0, -1.0, 5.0]) == 0.0
    # the script feeds (y + 1) / 2 as floats
    assert FM.roc_auc_score(np.array([0.0, 1.0, 1.0, 0.0]), np.array([0.2, 0.2, 0.9, 0.1])) == pytest.approx(0.875)


def test_roc_auc_one_class_raises():
    with pytest.raises(ValueError):
        FM.roc_auc_score([1, 1, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        FM.roc_auc_score([], [])


def test_roc_auc_matches_sklearn():
    sk = _sklearn_auc()
    if sk is None:
        pytest.skip("sklearn is not installed")
    rng = np.random.default_rng(0)
    for n in (2, 5, 37, 400):
        for quant in (None, 4, 1):
            y = rng.integers(0, 2, size=n)
            y[0], y[-1] = 0, 1
            s = rng.normal(size=n).astype(np.float32)
            if quant is not None:
                s = np.round(s * quant) / quant         # many ties
            assert FM.roc_auc_score(y, s) == pytest.approx(sk(y, s), abs=1e-12)


def test_task_skip_and_nan_rules_match_the_script():
    """Validity = y^2 > 0 and pred not NaN; a task with one class among its valid labels (or none) is skipped; the mean is
    over the remaining tasks; NaN when none remains."""
    y = np.array([[1, -1, 0, 1], [-1, -1, 0, 1], [1, 1, 0, -1], [-1, 0, 0, 1]], dtype=np.float32)
    s = np.array([[0.9, 0.1, 0.3, np.nan], [0.2, 0.4, 0.1, 0.5], [0.7, 0.2, 0.2, 0.6], [0.1, 0.9, 0.0, 0.7]], dtype=np.float32)
    valid = np.logical_and(y ** 2 > 0, ~np.isnan(s))
    mean, per = FM.roc_auc_tasks(y, s, valid)
    # task 0: perfect; task 1: one positive (0.2) vs negatives 0.1, 0.4 -> 0.5; task 2: no valid label; task 3: the NaN row
    # drops out, positives {0.5, 0.7} vs negative {0.6} -> 0.5
    assert per[0] == 1.0 and per[1] == pytest.approx(0.5) and per[2] is None and per[3] == pytest.approx(0.5)
    assert mean == pytest.approx((1.0 + 0.5 + 0.5) / 3)
    # one class everywhere: every task skipped -> NaN
    y1 = np.ones((3, 2), dtype=np.float32)
    mean1, per1 = FM.roc_auc_tasks(y1, np.zeros((3, 2), np.float32), np.ones((3, 2), bool))
    assert per1 == [None, None] and np.isnan(mean1)


def test_golden_eval_roc_auc_from_the_fixture_logits():
    """The fixture's eval-mode logits through roc_auc_tasks give sklearn's per-task values (stored at generation time)."""
    from helpers import load_golden
    g = load_golden("finetune_molnet.npz")
    if "eval.roc_auc" not in g:
        pytest.skip("fixture generated without sklearn")
    y, s = g["batch.y"], g["eval.logits"]
    valid = np.logical_and(y ** 2 > 0, ~np.isnan(s))
    mean, per = FM.roc_auc_tasks(y, s, valid)
    ref = g["eval.roc_auc"]
    for a, r in zip(per, ref):
        assert (a is None) == bool(np.isnan(r))
        if a is not None:
            assert a == pytest.approx(r, abs=1e-12)
    assert mean == pytest.approx(float(np.nanmean(ref)))


# ---------------------------------------------------------------------------------------------------- learning rates ---
@pytest.mark.parametrize("epochs", [1, 2, 7, 100])
def test_cosine_rates_equal_torch_scheduler(epochs):
    p = torch.nn.Parameter(torch.zeros(1))
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-4}, {"params": [q], "lr": 3e-4}], lr=1e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs)
    mine = FM.CosineAnnealing([1e-4, 3e-4], epochs)
    for _ in range(epochs + 3):                # past T_max the schedule climbs again
        opt.step()
        sch.step()
        got = mine.step()
        assert got == [g["lr"] for g in opt.param_groups]


# ------------------------------------------------------------------------------------------------------- checkpoints ---
class _Gnn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 2)
        self.bn = torch.nn.BatchNorm1d(2)


def test_checkpoint_layouts(tmp_path):
    src = _Gnn()
    head = torch.nn.Linear(2, 5)
    d = FM.checkpoint_dict(src, head)
    assert set(d) == {"model", "graph_pred_linear"}
    assert set(d["model"]) == set(src.state_dict()) and set(d["graph_pred_linear"]) == {"weight", "bias"}
    for layout in ("model_2D", "model", "raw"):
        path = tmp_path / f"{layout}.pth"
        sd = src.state_dict()
        torch.save(sd if layout == "raw" else {layout: sd, "other": {"x": torch.zeros(1)}}, path)
        # the module's load_state and the shared one with MoleculeNet's key order: never a head, a raw state dict allowed
        h0 = torch.nn.Linear(2, 5)
        for load in (lambda m: FM.load_state(m, path),
                     lambda m: FC.load_state(m, None, path, ("model_2D", "model"), raw_ok=True),
                     lambda m: FC.load_state(m, h0, path, FM.MoleculeNetTrainer.LOAD_KEYS, raw_ok=True)):
            dst = _Gnn()
            load(dst)
            for k, v in src.state_dict().items():
                assert torch.equal(dst.state_dict()[k], v), (layout, k)
    # model_2D wins over model; without raw_ok a file with neither key is an error
    other = _Gnn()
    torch.save({"model": other.state_dict(), "model_2D": src.state_dict()}, tmp_path / "both.pth")
    dst = _Gnn()
    FM.load_state(dst, tmp_path / "both.pth")
    assert torch.equal(dst.lin.weight, src.lin.weight)
    with pytest.raises(KeyError):
        FC.load_state(_Gnn(), None, tmp_path / "raw.pth", ("model_2D", "model"))
    assert FM.MoleculeNetTrainer.LOADS_HEAD is False and FM.MoleculeNetTrainer.RAW_OK is True
    import inspect
    assert list(inspect.signature(FM.MoleculeNetTrainer.load_model).parameters) == ["self", "path"]      # load_latest is MD17's


def test_num_tasks():
    assert [FM.num_tasks(d) for d in ("tox21", "hiv", "bace", "bbbp", "pcba", "muv", "toxcast", "sider", "clintox")] == \
        [12, 1, 1, 1, 92, 17, 617, 27, 2]
    with pytest.raises(ValueError):
        FM.num_tasks("qm9")


# ---------------------------------------------------------------------------------------------------- dropout mirror ---
def test_host_uniform_reproduces_msde_uniform_known_answers():
    """msde_uniform (csrc/msde_common.h) at fixed points, computed independently with Python integers."""
    def ref(seed, idx):
        m = (1 << 64) - 1
        z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z = z ^ (z >> 31)
        return (z >> 40) / 16777216.0
    for seed in (0, 1, 42, 0xFFFFFFFFFFFFFFFF, FM.dropout_seed(42, 3, 7)):
        idx = np.array([0, 1, 2, 299, 300, 123456789, (1 << 40) + 3], dtype=np.uint64)
        got = FM.msde_uniform(seed, idx)
        assert got.dtype == np.float32
        assert [float(v) for v in got] == [ref(seed, int(i)) for i in idx]
    # pinned values: a change of the hash shows here
    assert float(FM.msde_uniform(0, np.array([0], np.uint64))[0]) == ref(0, 0)
    assert FM.dropout_seed(42, 0) == (42 + 0xD1B54A32D192ED69) & ((1 << 64) - 1)
    assert FM.dropout_seed(42, 2, 5) == (42 + 3 * 0xD1B54A32D192ED69 + 5 * 0x100000001B3) & ((1 << 64) - 1)


def test_host_keep_mask_shape_and_rate():
    m = FM.dropout_keep_mask(7, 1, 3, 400, 300, 0.5)
    assert m.shape == (400, 300) and m.dtype == bool
    n = m.size
    assert abs(m.mean() - 0.5) < 5 * (0.25 / n) ** 0.5
    assert FM.dropout_keep_mask(7, 1, 3, 4, 5, 0.0).all()
    assert not np.array_equal(m, FM.dropout_keep_mask(7, 1, 4, 400, 300, 0.5))
    assert not np.array_equal(m, FM.dropout_keep_mask(7, 2, 3, 400, 300, 0.5))


# --------------------------------------------------------------------------------------------------- synthetic data ---
def test_make_molnet_batch_shapes_and_labels():
    b = make_molnet_batch(256, 12, seed=3, missing=0.3)
    counts = torch.bincount(b.batch, minlength=b.num_graphs)
    assert b.y.shape == (256, 12) and b.y.dtype == torch.float32
    assert set(torch.unique(b.y).tolist()) <= {-1.0, 0.0, 1.0}
    assert abs(float((b.y == 0).float().mean()) - 0.3) < 0.05
    assert int(counts.min()) >= 2 and int(counts.max()) <= 150 and int((counts > 32).sum()) > 0
    assert b.x.shape[1] == 9 and b.edge_attr.shape[1] == 3
    big = make_molnet_batch(4, 1, seed=0, sizes=[150, 2, 100, 33])
    assert torch.bincount(big.batch).tolist() == [150, 2, 100, 33]
