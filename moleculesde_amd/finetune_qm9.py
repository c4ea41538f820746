"""QM9 property fine-tuning of the pretrained SchNet (or PaiNN) -- the counterpart of examples/finetune_QM9.py.

    pred = graph_pred_linear(model(x, positions, batch)).squeeze()      (:145-160; Linear(emb_dim, 1); PaiNN: its output MLP)
    y    = (batch.y.view(B, -1)[:, task_id] - TRAIN_mean) / TRAIN_std   (:162-166)
    loss = L1Loss()(pred, y) (--loss mae, the default) or MSELoss(); zero_grad, backward, Adam over two groups (:168-171)
    loss_acc = mean of the step losses; CosineAnnealingLR(epochs) or StepLR stepped once per epoch (:173-180, :324-346)
    eval: pred * TRAIN_std + TRAIN_mean, MAE = mean |pred - y| over the split (:185-223)

On the device (SchNet): the encoder's pair path, then ONE launch (hip.qm9_head_train) for the head, the standardised loss,
dpred, d out, dW and db; the head's gradients are written straight into the buffers FlatAdam reads, and the loss is added
to a device-side epoch sum, so an epoch reads the host once.  QM9 molecules have at most 29 atoms, inside the 32-atom
bound of the device plan builder: a capacity bucket (bucket.Bucket(z_only=True)) holds {device-built plan, forward, head,
backward, Adam, weight-copy refresh} as one hipGraph that every full batch replays (capture_bucket / step_bucket /
step_stream); a batch that does not fit takes the exact-size eager step.  PaiNN runs eagerly with the loss-only form of
the head kernel.  Dataset processing (rdkit, units, thermochemistry) stays with the caller: targets are taken as given.
"""
import os

import numpy as np
import torch

from . import bucket as BK, hip, slabs, wcache
from .capture import CaptureSession, CapturedStep, optimizer_restore, optimizer_snapshot
from .finetune_common import (CosineAnnealing, FineTuner, StepDecay, checkpoint_dict, hip_device,  # noqa: F401
                              load_state as _load_state, make_scheduler, painn_radius_edges)
from .optim import FlatAdam

# Geom3D/datasets/dataset_QM9.py:43-57
TARGET_FIELDS = ["mu", "alpha", "homo", "lumo", "gap", "r2", "zpve", "u0", "u298", "h298", "g298", "cv", "gap_02"]
NUM_MOLS = 133885 - 3054          # splitters.py: Nmols


def task_id(task):
    """dataset.task_id of MoleculeDatasetQM9: the index of `task` among the 13 target fields.  task="qm9" (all targets
    at once) gives the reference task_id None, which its step cannot index with: refused here."""
    if task == "qm9":
        raise ValueError("task='qm9' (all 13 targets at once) cannot be fine-tuned: the step regresses one target; "
                         f"pick one of {TARGET_FIELDS}")
    if task not in TARGET_FIELDS:
        raise ValueError(f"unknown QM9 task {task!r}: one of {TARGET_FIELDS}")
    return TARGET_FIELDS.index(task)


# ---- splits (splitters.py:246-351; the null-value filter is off in the script: task_idx is not passed) -----------------
def split_customized_01(num_mols, seed=0):
    """QM9_random_customized_01: (train, valid, test) index arrays -- 110000 / 10000 / the rest of a permutation."""
    np.random.seed(seed)
    all_idx = np.random.permutation(num_mols)
    n_train, n_valid = 110000, 10000
    return all_idx[:n_train], all_idx[n_train:n_train + n_valid], all_idx[n_train + n_valid:]


def split_customized_02(num_mols, seed=0):
    """QM9_random_customized_02: 100000 train, int(0.1 * Nmols) test, the rest of Nmols valid (index order: train, valid,
    test)."""
    np.random.seed(seed)
    all_idx = np.random.permutation(num_mols)
    n_train, n_test = 100000, int(0.1 * NUM_MOLS)
    n_valid = NUM_MOLS - (n_train + n_test)
    return all_idx[:n_train], all_idx[n_train:n_train + n_valid], all_idx[n_train + n_valid:]


def split(name, num_mols, seed=0):
    if name == "customized_01":
        return split_customized_01(num_mols, seed)
    if name == "customized_02":
        return split_customized_02(num_mols, seed)
    raise ValueError("Invalid split option on QM9.")


def train_mean_std(y, task_id):
    """TRAIN_mean, TRAIN_std of the script (:263-266): train_dataset.mean()/std()[task_id].item(), i.e. the fp32
    torch.stack(y).mean(0) and the unbiased .std(0) over the train split's [N, 13] targets."""
    y = torch.as_tensor(y, dtype=torch.float32)
    return y.mean(dim=0)[task_id].item(), y.std(dim=0)[task_id].item()


def mean_absolute_error(pred, target):
    return np.mean(np.abs(pred - target))


# ---- checkpoints (finetune_QM9.py:95-130) -------------------------------------------------------------------------------
def load_state(model, graph_pred_linear, path):
    """load_model of the script: `model_3D` (a pretraining checkpoint, pretrain.Trainer.save) or `model`, plus
    `graph_pred_linear` when the file has it."""
    return _load_state(model, graph_pred_linear, path, QM9Trainer.LOAD_KEYS)


def save_evaluation_best(output_model_dir, val_target, val_pred, test_target, test_pred):
    """The script's np.savez(os.path.join(dir, "evaluation_best.pth"), ...): numpy appends ".npz", so the file that lands
    is evaluation_best.pth.npz.  Returns that path."""
    path = os.path.join(output_model_dir, "evaluation_best.pth")
    np.savez(path, val_target=val_target, val_pred=val_pred, test_target=test_target, test_pred=test_pred)
    return path + ".npz"


def check_rotation_transform(use_rotation_transform):
    """--use_rotation_transform: both encoders read interatomic distances only, so a random rotation of the coordinates
    changes nothing but rounding.  Not restated on the device: refused."""
    if use_rotation_transform:
        raise NotImplementedError("--use_rotation_transform is not supported: SchNet and PaiNN outputs depend on interatomic "
                                  "distances only, the transform changes nothing but rounding")


class QM9Trainer(FineTuner):
    # of finetune_common.FineTuner: scheduler_step, load_model (:95-108: model_3D or model, plus graph_pred_linear if present)
    # and save_model (:111-130: model.pth for the best validation MAE, model_final.pth for the last epoch)
    def __init__(self, model, graph_pred_linear, lr=1e-4, weight_decay=0.0, epochs=100, loss="mae",
                 lr_scheduler="CosineAnnealingLR", train_mean=0.0, train_std=1.0, task_id=None, lr_decay_step_size=100,
                 lr_decay_factor=0.5, use_rotation_transform=False):
        """model: geom3d.SchNet or geom3d.PaiNN on the HIP device; graph_pred_linear: torch.nn.Linear(emb_dim, 1) for SchNet,
        model.create_output_layers() for PaiNN.  Adam over the script's two param groups with one lr (:317-322).  task_id:
        the column of two-dimensional targets (None: targets are one column)."""
        check_rotation_transform(use_rotation_transform)
        if loss not in hip.QM9_LOSS_MODES:
            raise ValueError("Loss {} not included.".format(loss))
        self.model, self.head = model, graph_pred_linear
        self.device = hip_device(next(model.parameters()), "finetune_qm9")
        self.is_painn = type(model).__name__ == "PaiNN"
        if not self.is_painn and not (isinstance(graph_pred_linear, torch.nn.Linear) and graph_pred_linear.out_features == 1):
            raise ValueError("SchNet fine-tuning takes graph_pred_linear = torch.nn.Linear(emb_dim, 1)")
        self.scheduler = make_scheduler(lr_scheduler, [lr, lr], epochs, lr_decay_step_size, lr_decay_factor, strict=True)
        self.loss, self.mean, self.std, self.task_id = loss, float(train_mean), float(train_std), task_id
        self.opt = FlatAdam([{"params": model.parameters(), "lr": lr}, {"params": graph_pred_linear.parameters(), "lr": lr}],
                            weight_decay=weight_decay)
        dev = self.device
        self.loss_acc = torch.zeros(1, dtype=torch.float64, device=dev)     # device-side sum of the epoch's step losses
        if not self.is_painn:
            # the head's gradient buffers: written by the head kernel, read by FlatAdam through its chunk table
            self._gW = torch.zeros_like(graph_pred_linear.weight)
            self._gb = torch.zeros_like(graph_pred_linear.bias)
        self._graphs = {}
        self._graph_pool = None

    # ---- targets ---------------------------------------------------------------------------------------------------
    def targets(self, y, B):
        """The step's raw targets as a [B] fp32 device view: batch.y.view(B, -1)[:, task_id] (one column: that column)."""
        y = y.view(B, -1)
        y = y[:, 0] if y.size(1) == 1 else y[:, self.task_id]
        if y.dtype != torch.float32 or y.device != self.device:
            y = y.to(self.device, torch.float32)
        return y

    def _encode(self, batch):
        """The script's model call: SchNet(x, positions, batch); PaiNN also the radius graph (built as
        pretrain.Trainer._encode_3d builds it when the batch has none)."""
        if not self.is_painn:
            return self.model(batch.x, batch.positions, batch.batch)
        ei = getattr(batch, "radius_edge_index", None)
        if ei is None:
            ei = painn_radius_edges(self.model, batch, batch.positions)
        return self.model(batch.x, batch.positions, ei, batch.batch)

    # ---- one training step ---------------------------------------------------------------------------------------------
    def _step_body(self, batch, y):
        """Forward, head + loss + the head's backward (one launch), encoder backward, Adam, weight-copy refresh.  No host
        read.  Returns the device (pred [B], loss [1])."""
        self.model.train()
        self.head.train()
        rep = self._encode(batch)
        if self.is_painn:
            out = self.head(rep).squeeze(-1)
            pred, loss, dpred = hip.qm9_head_train(out.detach(), None, None, y, self.mean, self.std, self.loss,
                                                   loss_acc=self.loss_acc)
            roots, grads = out, dpred
        else:
            pred, loss, dout = hip.qm9_head_train(rep.detach(), self.head.weight, self.head.bias, y, self.mean, self.std,
                                                  self.loss, dW=self._gW, db=self._gb, loss_acc=self.loss_acc)
            roots, grads = rep, dout
        self.opt.zero_grad()
        if self.is_painn:
            # PaiNN's embedding masks its padding row with a gradient hook, which needs the gradient when autograd hands it
            # over, not after a deferred slab reduction: plain backward, weight gradients launched one by one
            torch.autograd.backward(roots, grads)
        else:
            with slabs.param_grad_batch(self.opt.params):
                torch.autograd.backward(roots, grads)
        if not self.is_painn:
            self.head.weight.grad, self.head.bias.grad = self._gW, self._gb
        self.opt.step_from_grads()
        self._last_refreshed = wcache.refresh_weight_t()
        return pred, loss

    def step(self, batch, y=None):
        """One step of train() (:145-171) on a prepared exact-size batch (geom3d.prepare_batch) with raw targets y (default
        batch.y).  Returns the loss as a device tensor [1] (no host read)."""
        y = self.targets(batch.y if y is None else y, int(batch.num_graphs))
        pred, loss = self._step_body(batch, y)
        self.last_pred, self.last_loss = pred, loss
        return loss

    # ---- capacity buckets: one captured graph for every full batch ---------------------------------------------------
    def make_bucket(self, caps):
        return BK.Bucket(caps, self.device, node_class=self.model.node_class, z_only=True)

    def capture_bucket(self, bk, warm_blob, eager_steps=1):
        """Warm up on one raw batch (sizes the workspaces), then capture {device-side plan construction + step} for the
        bucket's capacities.  The warm-up steps are undone (parameters, Adam moments, step count and the epoch's loss sum
        are restored), so the capture itself trains nothing.  Afterwards every batch that fits is `step_bucket(bk, blob)`."""
        if self.is_painn:
            raise NotImplementedError("PaiNN fine-tuning runs the exact-size eager step only")
        bk.load(warm_blob)
        bk.build_plan_on_device()
        ok, sizes = bk.check()
        if not ok:
            raise BK.BucketOverflow(f"batch does not fit the bucket: {sizes} vs {bk.caps.as_dict()}")
        snap = optimizer_snapshot(self.opt, self.loss_acc)
        with bk.bounds():
            for _ in range(eager_steps):
                self._step_body(bk.batch, bk.y)
        if self._graph_pool is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        with CaptureSession(self.opt, self.device, self._graph_pool) as session, session.graph(bk.bounds()) as g:
            bk.build_plan_on_device()
            pred, loss = self._step_body(bk.batch, bk.y)
        self._graphs[id(bk)] = CapturedStep(g, self._last_refreshed, bucket=bk, pred=pred, loss=loss)
        torch.cuda.synchronize()
        optimizer_restore(self.opt, snap, self.loss_acc)
        return g

    def step_bucket(self, bk, blob):
        """One copy of the raw blob (pack_raw_z) + one graph replay.  The device overflow flag of an earlier call is
        looked at here (one call late, no synchronisation of the running step).  Returns the graph's loss tensor [1]
        (overwritten by the next replay, as last_pred is)."""
        if bk.poll_overflow():
            raise BK.BucketOverflow("the batch of the previous step_bucket() call did not fit the bucket "
                                    f"{bk.caps.as_dict()}: its rows were left inert, that step is not a valid update")
        bk.load(blob)
        return self.replay(bk)

    def replay(self, bk):
        """The captured step on whatever the bucket's raw buffer holds (a blob loaded by bk.load or a BlobFeeder)."""
        rec = self._graphs[id(bk)]
        assert rec.bucket is bk
        rec.replay()
        self.last_pred, self.last_loss = rec.pred, rec.loss
        return rec.loss

    def fits(self, bk, batch):
        need = BK.raw_sizes_z(batch)
        return bk.caps.fits(need) and need["n_max"] <= BK.PLAN_NMAX

    def step_stream(self, bk, batch, y=None):
        """One step on a collated HOST batch (1-D z, targets y or batch.y): through the bucket's graph when the batch fits
        its capacities, otherwise the exact-size eager step (the epoch's smaller last batch, a molecule over 32 atoms)."""
        B = int(batch.num_graphs)
        y = (batch.y if y is None else y).view(B, -1)
        y = y[:, 0] if y.size(1) == 1 else y[:, self.task_id]
        if self.fits(bk, batch):
            return self.step_bucket(bk, BK.pack_raw_z(batch, bk.caps, y))
        from .geom3d import prepare_batch
        return self.step(prepare_batch(batch.clone(), self.device), y)

    # ---- epochs ----------------------------------------------------------------------------------------------------
    def train_epoch(self, batches, bucket=None):
        """train(): every batch, then one scheduler step.  Items are prepared device batches (or (batch, y) pairs); with
        `bucket`, collated host batches streamed through it (step_stream).  Reads the host once: returns the mean of the
        step losses (loss_acc / len(loader))."""
        self.loss_acc.zero_()
        n = 0
        for item in batches:
            batch, y = item if isinstance(item, tuple) else (item, None)
            if bucket is None:
                self.step(batch, y)
            else:
                self.step_stream(bucket, batch, y)
            n += 1
        if bucket is not None and bucket.poll_overflow():
            raise BK.BucketOverflow(f"a batch of this epoch did not fit the bucket {bucket.caps.as_dict()}")
        acc = float(self.loss_acc.item())
        self.scheduler_step()
        return acc / max(n, 1)

    # ---- evaluation ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _eval_batch(self, batch, y, acc):
        rep = self._encode(batch)
        if self.is_painn:
            return hip.qm9_head_eval(self.head(rep).squeeze(-1), None, None, y, self.mean, self.std, acc)
        return hip.qm9_head_eval(rep, self.head.weight, self.head.bias, y, self.mean, self.std, acc)

    @torch.no_grad()
    def evaluate(self, batches, bucket=None):
        """eval() (:185-223): (MAE, y_true, y_scores) over `batches` (prepared device batches or (batch, y) pairs; with
        `bucket`, collated host batches, the full ones built on the device through the bucket).  The predictions are
        de-standardised and |pred - y| summed on the device (fp64); the host reads once, at the end."""
        self.model.eval()
        self.head.eval()
        acc = torch.zeros(2, dtype=torch.float64, device=self.device)
        ys, preds = [], []
        for item in batches:
            batch, y = item if isinstance(item, tuple) else (item, None)
            B = int(batch.num_graphs)
            y = (batch.y if y is None else y)
            if bucket is not None and self.fits(bucket, batch):
                yv = y.view(B, -1)
                yv = yv[:, 0] if yv.size(1) == 1 else yv[:, self.task_id]
                bucket.load(BK.pack_raw_z(batch, bucket.caps, yv, pin=True))
                bucket.build_plan_on_device()
                with bucket.bounds():
                    yd = bucket.y.clone()
                    preds.append(self._eval_batch(bucket.batch, yd, acc))
            else:
                if bucket is not None:
                    from .geom3d import prepare_batch
                    batch = prepare_batch(batch.clone(), self.device)
                yd = self.targets(y, B)
                preds.append(self._eval_batch(batch, yd, acc))
            ys.append(yd)
        self.model.train()
        self.head.train()
        y_true = torch.cat(ys).cpu().numpy()
        y_scores = torch.cat(preds).cpu().numpy()
        a = acc.cpu().tolist()
        return a[0] / max(a[1], 1.0), y_true, y_scores
