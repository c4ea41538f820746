"""Generate tests/golden/finetune_molnet.npz: three training steps and one evaluation of examples/finetune_MoleculeNet.py on the
GENUINE reference GNN (oracle/ref_loader.verbatim(): Geom3D.models.GNN on the stand-in third-party layer), the stand-in
global_mean_pool, torch.nn.Linear, torch.nn.BCEWithLogitsLoss and torch.optim.Adam.  The script cannot be imported (its
config module parses argv, it loads datasets), so the body of train() (:117-145) and of eval() (:159-210) is restated below.

Settings: GNN(3, 32, JK="last", drop_ratio=0), 12 tasks, 8 molecules (three of more than 32 atoms), labels in {-1, 0, 1}
with missing entries (task 11 missing for every molecule, molecule 6 missing every task), Adam lr 1e-3 over the two param
groups of :273-278, 3 steps on the same batch.  Stored: the batch, the initial GNN / head parameters, every step's loss and
logits, the parameters after the steps, BatchNorm buffers included, and an evaluation (eval-mode logits and, when sklearn
can be imported here, its ROC-AUC per task; NaN for a skipped task).

    python tools/make_golden_finetune_molnet.py        (needs the reference checkout: build container only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from moleculesde_amd.synthetic import make_molnet_batch  # noqa: E402

NUM_LAYER, EMB, T, LR, STEPS = 3, 32, 12, 1e-3, 3
SIZES = [12, 40, 7, 33, 18, 57, 3, 21]


def main():
    ref = ref_loader.verbatim()
    global_mean_pool = ref.standins.nn.global_mean_pool
    b = make_molnet_batch(len(SIZES), T, seed=5, missing=0.25, pos_rate=0.35, sizes=SIZES)
    b.y[:, T - 1] = 0.0
    b.y[6, :] = 0.0
    torch.manual_seed(123)
    model = ref.GNN(NUM_LAYER, EMB, JK="last", drop_ratio=0.0, gnn_type="GIN")
    graph_pred_linear = torch.nn.Linear(EMB, T)
    with torch.no_grad():                  # non-trivial BatchNorm affine parameters and eps
        for n, p in model.named_parameters():
            if n.endswith(".eps"):
                p.fill_(0.1)
            elif "batch_norm" in n or ".mlp.1." in n:
                p.copy_((1.0 + 0.2 * torch.randn(p.shape)) if n.endswith("weight") else 0.1 * torch.randn(p.shape))
    out = {"batch." + k: getattr(b, k).numpy() for k in b.tensor_keys()}
    out["batch.num_graphs"] = np.int64(b.num_graphs)
    out.update({"sd." + k: v.numpy().copy() for k, v in model.state_dict().items()})
    out.update({"head." + k: v.detach().numpy().copy() for k, v in graph_pred_linear.state_dict().items()})
    out.update(lr=np.float64(LR), num_layer=np.int64(NUM_LAYER), emb=np.int64(EMB))

    criterion = torch.nn.BCEWithLogitsLoss(reduction="none")
    optimizer = torch.optim.Adam([{"params": model.parameters(), "lr": LR}, {"params": graph_pred_linear.parameters(), "lr": LR}],
                                 lr=LR, weight_decay=0)
    losses, logits = [], []
    model.train()
    graph_pred_linear.train()
    for _ in range(STEPS):                 # train(), :117-145
        node_repr = model(b.x, b.edge_index, b.edge_attr)
        molecule_2D_repr = global_mean_pool(node_repr, b.batch)
        pred = graph_pred_linear(molecule_2D_repr)
        y = b.y.view(pred.shape).to(torch.float64)
        assert not bool(torch.isnan(pred).any())
        is_valid = y ** 2 > 0
        loss_mat = criterion(pred.double(), (y + 1) / 2)
        loss_mat = torch.where(is_valid, loss_mat, torch.zeros(loss_mat.shape).to(torch.float64))
        optimizer.zero_grad()
        loss = torch.sum(loss_mat) / torch.sum(is_valid)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.item()))
        logits.append(pred.detach().numpy().copy())
    out["losses"] = np.array(losses, dtype=np.float64)
    out["logits"] = np.stack(logits)
    out.update({"sd_after." + k: v.numpy().copy() for k, v in model.state_dict().items()})
    out.update({"head_after." + k: v.detach().numpy().copy() for k, v in graph_pred_linear.state_dict().items()})

    with torch.no_grad():                  # eval(), :159-210
        model.eval()
        graph_pred_linear.eval()
        pred = graph_pred_linear(global_mean_pool(model(b.x, b.edge_index, b.edge_attr), b.batch))
    out["eval.logits"] = pred.numpy()
    try:
        from sklearn.metrics import roc_auc_score
    except ImportError:
        roc_auc_score = None
    if roc_auc_score is not None:
        y_true, y_scores = b.y.numpy(), pred.numpy()
        y_valid = np.logical_and(y_true ** 2 > 0, ~np.isnan(y_scores))
        roc = []
        for i in range(T):
            v = y_valid[:, i]
            try:
                roc.append(roc_auc_score((y_true[v, i] + 1) / 2, y_scores[v, i]))
            except ValueError:
                roc.append(np.nan)
        out["eval.roc_auc"] = np.array(roc, dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "finetune_molnet.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB, losses {losses}")


if __name__ == "__main__":
    main()
