"""MoleculeNet fine-tuning of the pretrained GIN -- the counterpart of examples/finetune_MoleculeNet.py (manuscript Table 2).

    node_repr = model(x, edge_index, edge_attr)                    (:120; GNN(num_layer, emb_dim, JK, drop_ratio=0.5))
    pred      = graph_pred_linear(global_mean_pool(node_repr, batch))  (:121-124; Linear(intermediate_dim, num_tasks))
    skip the batch if any pred is NaN                              (:131-134)
    loss_mat  = BCEWithLogitsLoss(reduction='none')(pred.double(), (y + 1) / 2), 0 where y == 0   (:136-139)
    loss      = sum(loss_mat) / sum(y^2 > 0);  zero_grad, backward, Adam over two param groups      (:141-144, :273-278)
    CosineAnnealingLR(optimizer, epochs) stepped once per epoch     (:152-153, :281-284)
    eval: ROC-AUC per task over the valid labels, tasks with one class skipped, mean over the rest  (:159-210)

On the device: the GIN runs its fused training path (hip.gin_mlp_bn), the dropout after every layer runs on
hip.dropout_rows (GNN.device_dropout: masks from a host seed, the layer and a device step counter -- never stored, never
F.dropout), the head is hip.molnet_head (pool + logits, one launch; backward one launch + the queued weight gradient) and
the loss is hip.molnet_bce (fp64, one launch).  The step reads 3 numbers back to the host (loss, valid count, NaN logits),
as the reference's loss.item() does.  Batches have exact sizes (host-built plans, geom3d.prepare_batch): MoleculeNet
molecules exceed the 32-atom bound of the device plan builder, so the step is launched eagerly, one batch at a time.
"""
import numpy as np
import torch

from . import _lib, hip, plan as _plan, slabs, wcache
from ._torchabi import _p, _stream
from .finetune_common import CosineAnnealing, FineTuner, checkpoint_dict, hip_device, load_state as _load_state  # noqa: F401
from .optim import FlatAdam

# examples/util.py:183-199
NUM_TASKS = {"tox21": 12, "hiv": 1, "bace": 1, "bbbp": 1, "donor": 1, "pcba": 92, "muv": 17, "toxcast": 617, "sider": 27,
             "clintox": 2}


def num_tasks(dataset):
    """get_num_task of examples/util.py:183-199."""
    if dataset not in NUM_TASKS:
        raise ValueError("Invalid dataset name.")
    return NUM_TASKS[dataset]


# ---- host mirror of the dropout mask (csrc/pointwise.hip dropout_rows_kernel, msde_common.h msde_uniform) ------------------
_M64 = (1 << 64) - 1
DR_LAYER_MIX = 0xD1B54A32D192ED69
FNV = 0x100000001B3


def dropout_seed(seed, layer, step=None):
    """seed' of the dropout kernel: seed + DR_LAYER_MIX * (layer + 1) [+ step * FNV] (mod 2^64)."""
    s = (int(seed) + DR_LAYER_MIX * (int(layer) + 1)) & _M64
    if step is not None:
        s = (s + int(step) * FNV) & _M64
    return s


def msde_uniform(seed, idx):
    """msde_uniform(seed, idx) for a numpy array of indices: the splitmix64 finaliser, 24 bits -> float32 in [0, 1)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def dropout_keep_mask(seed, layer, step, M, D, p):
    """Boolean [M, D] keep mask that hip.dropout_rows(x, p, seed, layer, seed_dev) draws when seed_dev[0] == step (None: no
    device counter)."""
    u = msde_uniform(dropout_seed(seed, layer, step), np.arange(M * D, dtype=np.uint64)).reshape(M, D)
    return u >= np.float32(p)


# ---- evaluation (finetune_MoleculeNet.py:159-210) -------------------------------------------------------------------------
def roc_auc_score(y_true, y_score):
    """sklearn.metrics.roc_auc_score for binary labels: the area under the ROC curve with tied scores sharing one threshold
    (= the Mann-Whitney statistic with ties counted one half).  Raises ValueError when only one class is present, as sklearn
    does."""
    y_true = np.asarray(y_true).ravel()
    y_score = np.asarray(y_score, dtype=np.float64).ravel()
    pos = y_true == 1
    n_pos = int(pos.sum())
    n_neg = int(y_true.size - n_pos)
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(y_score, kind="mergesort")
    s = y_score[order]
    ranks = np.empty(s.size, dtype=np.float64)
    i = 0
    while i < s.size:                  # average ranks over groups of equal scores
        j = i
        while j + 1 < s.size and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = 0.5 * (i + j) + 1.0
        i = j + 1
    r = np.empty_like(ranks)
    r[order] = ranks
    return float((r[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def roc_auc_tasks(y_true, y_scores, y_valid):
    """The script's per-task loop (:195-210): ROC-AUC of every task over its valid rows; a task whose valid labels hold one
    class only is skipped (sklearn raises and the script catches it).  Returns (mean over the remaining tasks -- NaN when
    none remain --, list of per-task values with None for a skipped task)."""
    per = []
    for i in range(y_true.shape[1]):
        v = y_valid[:, i]
        try:
            per.append(roc_auc_score((y_true[v, i] + 1) / 2, y_scores[v, i]))
        except ValueError:
            per.append(None)
    kept = [a for a in per if a is not None]
    return (sum(kept) / len(kept) if kept else float("nan")), per


# ---- checkpoints (finetune_MoleculeNet.py:71-102) -------------------------------------------------------------------------
def load_state(model, path):
    """load_model of the script: a checkpoint with `model_2D` (pretrain.Trainer.save), `model`, or a raw state dict."""
    return _load_state(model, None, path, MoleculeNetTrainer.LOAD_KEYS, raw_ok=True)


class MoleculeNetTrainer(FineTuner):
    # of finetune_common.FineTuner: scheduler_step (:152-153), save_model (:83-102: model.pth for the best epoch,
    # model_final.pth for the last) and load_model (:71-80: model_2D, model or a raw state dict, into the GIN only)
    LOAD_KEYS, RAW_OK, LOADS_HEAD = ("model_2D", "model"), True, False

    def __init__(self, model, graph_pred_linear, lr=1e-4, weight_decay=0.0, epochs=100, lr_scheduler="CosineAnnealingLR",
                 seed=42):
        """model: geom3d.GNN on the HIP device; graph_pred_linear: torch.nn.Linear(intermediate_dim, num_tasks).  Adam over the
        script's two param groups (:273-278), CosineAnnealingLR(epochs) per epoch when lr_scheduler says so (config.py:52)."""
        self.model, self.head = model, graph_pred_linear
        self.device = hip_device(next(model.parameters()), "finetune_molnet")
        if lr_scheduler not in ("CosineAnnealingLR", None, "None"):
            raise NotImplementedError(f"lr_scheduler={lr_scheduler!r}: CosineAnnealingLR (the default) or None")
        self.opt = FlatAdam([{"params": model.parameters(), "lr": lr}, {"params": graph_pred_linear.parameters(), "lr": lr}],
                            weight_decay=weight_decay)
        self.scheduler = CosineAnnealing([lr, lr], epochs) if lr_scheduler == "CosineAnnealingLR" else None
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        # dropout step counter: advanced on the device at the head of every step (skipped steps included)
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        model.device_dropout = (self.seed, self.seed_dev)
        self.last_skipped = False
        self.last_logits = None

    # ---- one training step ---------------------------------------------------------------------------------------------
    def forward(self, batch):
        """logits [B, T] of a prepared batch (the head's pooled rows are kept for the backward when grad is enabled)."""
        h = self.model(batch.x, batch.edge_index, batch.edge_attr)
        pl = _plan.get_plan(batch)
        return hip.molnet_head(h, self.head.weight, self.head.bias, pl.mol_ptr)

    def step(self, batch, y=None):
        """One step of train() (:117-145) on a prepared (geom3d.prepare_batch) batch with labels y [B, T] in {-1, 0, 1}
        (default batch.y).  Returns the loss (a float; NaN when the batch has no valid label).  A batch with a NaN logit is
        skipped as the script does: no zero_grad, backward or Adam (last_skipped is set)."""
        y = batch.y if y is None else y
        self.model.train()
        self.head.train()
        _lib.call("msde_step_counters", _p(self.seed_dev), _p(None), _stream())
        logits = self.forward(batch)
        stats, dlogits, _ = hip.molnet_bce(logits.detach(), y.view(logits.shape))
        self.last_logits = logits.detach()
        loss, _, n_nan = stats.tolist()          # the step's one host read (the script's loss.item())
        self.last_skipped = n_nan > 0
        if self.last_skipped:
            return loss
        self.opt.zero_grad()
        with slabs.param_grad_batch(self.opt.params):
            torch.autograd.backward(logits, dlogits)
        self.opt.step_from_grads()
        wcache.refresh_weight_t()
        return loss

    def train_epoch(self, batches):
        """train(): every batch, then one scheduler step.  Returns loss_acc / len(batches) (skipped batches add nothing)."""
        acc, n = 0.0, 0
        for item in batches:
            batch, y = item if isinstance(item, tuple) else (item, None)
            loss = self.step(batch, y)
            if not self.last_skipped:
                acc += loss
            n += 1
        self.scheduler_step()
        return acc / max(n, 1)

    # ---- evaluation ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, batches):
        """(y_true, y_scores, y_valid) numpy arrays over `batches` (prepared Batch with .y, or (batch, y) pairs), eval mode."""
        self.model.eval()
        self.head.eval()
        y_true, y_scores = [], []
        for item in batches:
            batch, y = item if isinstance(item, tuple) else (item, None)
            y = batch.y if y is None else y
            pred = self.forward(batch)
            y_true.append(y.view(pred.shape))
            y_scores.append(pred)
        y_true = torch.cat(y_true).cpu().numpy()
        y_scores = torch.cat(y_scores).cpu().numpy()
        y_valid = np.logical_and(y_true ** 2 > 0, ~np.isnan(y_scores))
        return y_true, y_scores, y_valid

    def evaluate(self, batches):
        """eval() (:159-210): (mean ROC-AUC over the tasks that have both classes among their valid labels -- NaN when
        none has --, y_true, y_scores)."""
        y_true, y_scores, y_valid = self.predict(batches)
        mean, _ = roc_auc_tasks(y_true, y_scores, y_valid)
        return mean, y_true, y_scores
