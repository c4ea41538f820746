"""MD17 force fine-tuning step -- the counterpart of the training loop of examples/finetune_MD17.py:34-88.

    energy  = graph_pred_linear(model(x, positions, batch)).squeeze(1)            (:52-60; PaiNN: + radius_edge_index)
    energy  = energy * FORCE_MEAN_TOTAL + ENERGY_MEAN_TOTAL * NUM_ATOM           (:63-66, --energy_force_with_normalization)
    force   = -grad(energy, positions, ones, create_graph=True, retain_graph=True) (:68)
    loss    = MD17_energy_coeff * L1(energy, y) + MD17_force_coeff * L1(force, f) (:74; config.py:35-36: 0.05 / 0.95)
    optimizer.zero_grad(); loss.backward(); optimizer.step()                      (:76-78, Adam)

Every batch of an MD17 task is the same molecule in another conformation (MD17_train_batch_size molecules of NUM_ATOM
atoms), so the shapes never change: `ForceTrainer.capture` records the WHOLE step -- radius graph, energy, the
create_graph differentiation, both losses, the backward pass through the forces and Adam -- into ONE hipGraph whose
inputs (positions, energies, forces) are static device buffers; `step_graph` copies a batch into them and replays.  The
step is ~1500 tiny launches on a 21-atom molecule: launched from the host it is bound by launch latency, replayed it is
bound by the dependent chain on the device.  The encoder runs on the closed twice-differentiable operator set of
moleculesde_amd/dd.py (SchNet._forward_force_path, PaiNN.forward); there is no host synchronisation in the step.

Around that step, the rest of the script (MD17Trainer): get_idx_split (md17_split), the
--energy_force_with_normalization statistics (energy_force_normalization), epochs with a shuffled train loader, eval()'s
energy and force MAE, CosineAnnealingLR / StepLR per epoch, best-validation selection and the checkpoint layouts.  A split
lives on the device (ResidentSplit); for SchNet a train epoch is one captured {gather batch k, step, loss into a device sum}
replayed per batch, an evaluation one captured {gather batch k, energy, first-order forces, MAE sums} per batch size, and
each reads the host once, at its end (csrc/md17.hip).
"""
import os

import numpy as np
import torch

from . import _lib, dd, hip, slabs, wcache
from .capture import CaptureSession, CapturedStep, optimizer_restore, optimizer_snapshot
from .finetune_common import FineTuner, hip_device, load_state as _load_state, make_scheduler, painn_radius_edges  # noqa: F401
from .optim import FlatAdam


class ForceTrainer:
    def __init__(self, model, graph_pred_linear=None, lr=5e-4, energy_coeff=0.05, force_coeff=0.95, normalization=None,
                 weight_decay=0.0):
        """model: geom3d.SchNet or geom3d.PaiNN on a HIP device; graph_pred_linear: the nn.Linear(emb_dim, 1) head of
        finetune_MD17.py:276-279 (None: the encoder's readout is the energy).  normalization: None or
        (ENERGY_MEAN_TOTAL, FORCE_MEAN_TOTAL, NUM_ATOM) of finetune_MD17.py:217-230."""
        self.model, self.head = model, graph_pred_linear
        self.energy_coeff, self.force_coeff = float(energy_coeff), float(force_coeff)
        self.normalization = normalization
        params = list(model.parameters()) + (list(graph_pred_linear.parameters()) if graph_pred_linear is not None else [])
        self.device = hip_device(params[0], "finetune_md17")
        self.opt = FlatAdam([{"params": params, "lr": lr}], weight_decay=weight_decay)
        self.is_painn = type(model).__name__ == "PaiNN"
        self._captured = None

    # ---- one step, launched from the host ------------------------------------------------------------------------
    def energy_and_force(self, batch, positions, create_graph=True, negate=True):
        """finetune_MD17.py:49-68 (train) / :107-127 (eval, create_graph=False).  negate=False: returns d energy / d positions
        (= -force) without the sign flip (the training step's loss kernel applies it)."""
        if self.is_painn:
            rep = self.model(batch.x, positions, batch.radius_edge_index, batch.batch)
        else:
            rep = self.model(batch.x, positions, batch.batch)
        if isinstance(self.head, torch.nn.Linear):
            # nn.Linear(emb_dim, 1) (finetune_MD17.py:276-279) on the library's twice-differentiable Linear: its product, both
            # input gradients and the weight gradients (queued into the step's grouped launch) instead of five vendor GEMM
            # launches + a bias-gradient reduction
            energy = dd.linear(rep, self.head.weight, self.head.bias).squeeze(1)
        else:
            energy = (self.head(rep) if self.head is not None else rep).squeeze(1)
        if self.normalization is not None:
            e_mean, f_mean, n_atom = self.normalization
            energy = energy * f_mean + e_mean * n_atom
        with dd.positions_only():        # (no parameter gradients in this differentiation: skips ~30 unused weight-gradient GEMMs)
            dE = torch.autograd.grad(energy, positions, grad_outputs=self._ones_like(energy), create_graph=create_graph,
                                     retain_graph=create_graph)[0]
        return energy, (-dE if negate else dE)

    def _ones_like(self, energy):
        """d energy / d energy, kept (no fill launch per step)."""
        o = getattr(self, "_ones", None)
        if o is None or o.shape != energy.shape or o.device != energy.device:
            o = self._ones = torch.ones_like(energy)
        return o

    def _body(self, batch, positions, y, force_t):
        pos = positions.detach().requires_grad_(True)
        energy, dE = self.energy_and_force(batch, pos, negate=False)      # dE = d energy / d positions = -force
        # both L1 losses AND their derivatives w.r.t. energy and dE from one launch (msde_l1_energy_force_loss): the backward
        # pass starts from those instead of walking sub / abs / mean / mul / add / neg and their backward operators (~20 launches)
        y, force_t = hip._f32(y), hip._f32(force_t)
        e32, d32 = hip._f32(energy.detach()), hip._f32(dE.detach())
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        g_e, g_d = torch.empty_like(e32), torch.empty_like(d32)
        _lib.call("msde_l1_energy_force_loss", hip._p(e32), hip._p(y), e32.numel(), hip._p(d32), hip._p(force_t), d32.numel(), -1.0,
                  self.energy_coeff, self.force_coeff, hip._p(loss), hip._p(g_e), hip._p(g_d), hip._stream())
        loss = loss[0]
        self.opt.zero_grad()
        # the weight gradients of the whole step (two contributions per Linear: energy path and force path) as ONE grouped
        # launch + ONE slab reduction behind the backward pass (slabs.weight_grad_leaf) instead of ~170 per-layer launches
        with slabs.param_grad_batch(self.opt.params):
            torch.autograd.backward([energy, dE], [g_e, g_d])
        self.opt.step_from_grads()
        self._refreshed = wcache.refresh_weight_t()    # re-laid-out weight copies (if a layer reads one) follow the update
        return loss.detach()

    def step(self, batch, y=None, force=None):
        """batch: prepared (geom3d.prepare_batch) Batch with .positions; y [B], force [N, 3] default to batch.y / batch.force."""
        y = batch.y if y is None else y
        force = batch.force if force is None else force
        return self._body(batch, batch.positions, y.view(-1).float(), force.float())

    # ---- the same step as one hipGraph ---------------------------------------------------------------------------
    def capture(self, batch, y=None, force=None, eager_steps=2):
        """Warm up on `batch`, then capture.  The batch object (its plan: atom types, molecule pointers) is baked in: every
        later batch must hold the same molecules in the same order -- the MD17 loaders do; only positions, energies and
        forces change."""
        y = batch.y if y is None else y
        force = batch.force if force is None else force
        self._batch = batch
        self._pos = batch.positions.detach().clone()
        self._y = y.view(-1).float().clone()
        self._f = force.float().clone()
        for _ in range(eager_steps):
            self._body(batch, self._pos, self._y, self._f)
        with CaptureSession(self.opt, self.device) as session, session.graph() as g:
            loss = self._body(batch, self._pos, self._y, self._f)
        self._captured = CapturedStep(g, self._refreshed, loss=loss)
        return g

    def step_graph(self, positions, y, force):
        """Copy one batch's positions / energies / forces into the captured step's buffers and replay it.  Returns the loss
        (a device scalar, overwritten by the next replay)."""
        self._pos.copy_(positions, non_blocking=True)
        self._y.copy_(y.view(-1), non_blocking=True)
        self._f.copy_(force, non_blocking=True)
        self._captured.replay()
        return self._captured.loss


# ---- split and statistics ------------------------------------------------------------------------------------------
def md17_split(data_size, train_size=1000, valid_size=1000, seed=42):
    """DatasetMD17.get_idx_split (dataset_MD17.py:74-78): sklearn.utils.shuffle(range(n), random_state=seed), which is
    np.random.RandomState(seed).shuffle of arange(n); the first train_size, the next valid_size, the rest.  Returns
    {"train", "valid", "test"} int64 tensors, as the reference does."""
    ids = np.arange(int(data_size))
    np.random.RandomState(seed).shuffle(ids)
    n_tv = train_size + valid_size
    return {"train": torch.tensor(ids[:train_size]), "valid": torch.tensor(ids[train_size:n_tv]),
            "test": torch.tensor(ids[n_tv:])}


def energy_force_normalization(ys, forces):
    """(ENERGY_MEAN_TOTAL, FORCE_MEAN_TOTAL, NUM_ATOM) as finetune_MD17.py:218-232 forms them over the train split: per
    conformation energy / NUM_ATOM and sqrt(mean(force^2)) added in split order, in fp32 torch ops (bitwise the script's
    loop), then divided by the count.  ys: [M] (or [M, 1]) energies, forces: [M, NUM_ATOM, 3]; host tensors.  Returns a [1]
    tensor, a 0-dim tensor and an int (move the tensors to the device as the script does)."""
    ys = torch.as_tensor(ys, dtype=torch.float32).reshape(-1, 1)
    forces = torch.as_tensor(forces, dtype=torch.float32)
    e_total, f_total, n_atom = 0, 0, None
    for i in range(ys.size(0)):
        energy, force = ys[i], forces[i]
        n_atom = force.size()[0]
        e_total += energy / n_atom
        f_total += torch.sqrt(torch.mean(force.square()))
    e_total /= ys.size(0)
    f_total /= ys.size(0)
    return e_total, f_total, n_atom


class ResidentSplit:
    """One MD17 split on the device: x [NA] (the per-atom model input, shared: every MD17 conformation is the same molecule),
    positions [M, NA, 3], energies y [M] and forces [M, NA, 3], fp32 and contiguous, in the split's order."""

    def __init__(self, x, positions, y, force, device):
        x = torch.as_tensor(x)
        if x.dim() == 2:                         # one row per conformation: all rows must be the same molecule
            if not bool((x == x[:1]).all()):
                raise ValueError("ResidentSplit holds conformations of ONE molecule: the atom rows differ")
            x = x[0]
        positions = torch.as_tensor(positions, dtype=torch.float32)
        M, NA = positions.size(0), x.numel()
        if positions.shape != (M, NA, 3):
            raise ValueError(f"positions {tuple(positions.shape)} do not match [M, {NA}, 3]")
        self.x = x.to(device, torch.int64).contiguous()
        self.pos = positions.to(device).contiguous()
        self.y = torch.as_tensor(y, dtype=torch.float32).reshape(M).to(device).contiguous()
        self.force = torch.as_tensor(force, dtype=torch.float32).reshape(M, NA, 3).to(device).contiguous()
        self.num_atoms = NA

    def __len__(self):
        return self.pos.size(0)

    def rows(self, idx):
        """Positions [b * NA, 3], energies [b], forces [b * NA, 3] of the split rows idx (a device index tensor)."""
        return self.pos[idx].view(-1, 3), self.y[idx], self.force[idx].view(-1, 3)


# ---- checkpoints (finetune_MD17.py:145-186) -------------------------------------------------------------------------
def load_state(model, graph_pred_linear, path, load_latest=False):
    """load_model of the script: load_latest takes `model`; otherwise `model_3D` (a pretraining checkpoint) when present,
    else `model`; `graph_pred_linear` whenever the file has it."""
    return _load_state(model, graph_pred_linear, path, MD17Trainer.LOAD_KEYS, load_latest=load_latest)


class MD17Trainer(FineTuner):
    """examples/finetune_MD17.py's training loop, evaluation and checkpoints on the device.  model: geom3d.SchNet (with
    graph_pred_linear = nn.Linear(emb_dim, 1)) or geom3d.PaiNN (with model.create_output_layers()).  normalization: None or
    (ENERGY_MEAN_TOTAL, FORCE_MEAN_TOTAL, NUM_ATOM) of energy_force_normalization.  SchNet runs its full batches as
    captured graphs; PaiNN (its radius graph is rebuilt per conformation batch on the host side of the step) and the short
    last batch of a train epoch run eagerly with the same kernels."""

    energy_and_force = ForceTrainer.energy_and_force

    def _ones_like(self, energy):
        """d energy / d energy, one kept tensor per batch size: a captured graph reads the one it was captured with, so
        none is ever replaced (ForceTrainer keeps one, for its one shape)."""
        key = (tuple(energy.shape), energy.device)
        o = self._ones.get(key)
        if o is None:
            o = self._ones[key] = torch.ones_like(energy)
        return o

    def __init__(self, model, graph_pred_linear, lr=5e-4, epochs=100, weight_decay=0.0, lr_scheduler="CosineAnnealingLR",
                 lr_decay_step_size=100, lr_decay_factor=0.5, energy_coeff=0.05, force_coeff=0.95, normalization=None,
                 train_batch_size=1):
        self.model, self.head = model, graph_pred_linear
        self.device = hip_device(next(model.parameters()), "finetune_md17")
        self.is_painn = type(model).__name__ == "PaiNN"
        self.energy_coeff, self.force_coeff = float(energy_coeff), float(force_coeff)
        self.epochs, self.train_batch_size = int(epochs), int(train_batch_size)
        if normalization is not None:
            e_mean, f_mean, n_atom = normalization
            normalization = (torch.as_tensor(e_mean, dtype=torch.float32).to(self.device),
                             torch.as_tensor(f_mean, dtype=torch.float32).to(self.device), int(n_atom))
        self.normalization = normalization
        groups = [{"params": model.parameters(), "lr": lr}]
        if graph_pred_linear is not None:
            groups.append({"params": graph_pred_linear.parameters(), "lr": lr})
        self.scheduler = make_scheduler(lr_scheduler, [lr] * len(groups), epochs, lr_decay_step_size, lr_decay_factor)
        self.opt = FlatAdam(groups, weight_decay=weight_decay)
        dev = self.device
        self.loss_acc = torch.zeros(1, dtype=torch.float64, device=dev)     # device sum of the epoch's step losses
        self.eval_acc = torch.zeros(4, dtype=torch.float64, device=dev)     # sum |dE|, molecules, sum |dF|, force entries
        self._eval_ctr = torch.zeros(1, dtype=torch.int32, device=dev)      # batch counter of the captured evaluation
        self._train_ctr = torch.zeros(1, dtype=torch.int32, device=dev)     # batch counter of the captured train epoch
        self._templates = {}
        self._graphs = {}
        self._ones = {}
        self.captured = True        # False: every batch launched from the host (the eager form the tests compare against)

    # ---- batches ---------------------------------------------------------------------------------------------------
    def _template(self, split, B):
        """The prepared batch of B copies of the split's molecule (atom types, molecule pointers); positions come per step."""
        key = (B, tuple(split.x.tolist()))
        b = self._templates.get(key)
        if b is None:
            from .batch import Batch
            from .geom3d import prepare_batch
            NA = split.num_atoms
            b = Batch(x=split.x.cpu().repeat(B), positions=torch.zeros(B * NA, 3),
                      batch=torch.arange(B).repeat_interleave(NA))
            b.num_graphs = B
            b = self._templates[key] = prepare_batch(b, self.device)
        return b

    def _painn_edges(self, batch, positions):
        painn_radius_edges(self.model, batch, positions.detach())

    # ---- the step (train(), :34-88) and the evaluated batch (eval(), :93-142) ------------------------------------
    def _train_body(self, batch, positions, y, force):
        self.model.train()
        if self.head is not None:
            self.head.train()
        pos = positions.detach().requires_grad_(True)
        energy, dE = self.energy_and_force(batch, pos, negate=False)
        loss, g_e, g_d = hip.l1_energy_force_loss_acc(energy.detach(), y, dE.detach(), force, -1.0, self.energy_coeff,
                                                      self.force_coeff, self.loss_acc)
        self.opt.zero_grad()
        if self.is_painn:
            # PaiNN's embedding masks its padding row with a gradient hook that needs the gradient at once (finetune_qm9)
            torch.autograd.backward([energy, dE], [g_e, g_d])
        else:
            with slabs.param_grad_batch(self.opt.params):
                torch.autograd.backward([energy, dE], [g_e, g_d])
        self.opt.step_from_grads()
        self._refreshed = wcache.refresh_weight_t()
        return loss

    def _eval_body(self, batch, positions, y, force, acc):
        """Energy and first-order forces (autograd.grad without create_graph: the values of the script's create_graph=True
        + detach_), no weight gradients (dd.positions_only inside energy_and_force), the MAE sums into acc."""
        pos = positions.detach().requires_grad_(True)
        energy, dE = self.energy_and_force(batch, pos, create_graph=False, negate=False)
        hip.md17_eval_accumulate(energy.detach(), y, dE, force, acc)

    def step(self, split, idx):
        """One eager step on the split rows idx (a device index tensor).  Returns the loss, a device tensor [1]."""
        pos, y, f = split.rows(idx)
        b = self._template(split, int(idx.numel()))
        if self.is_painn:
            self._painn_edges(b, pos)
        loss = self._train_body(b, pos, y, f)
        self.last_loss = loss
        return loss

    # ---- captured graphs ---------------------------------------------------------------------------------------------
    def _capture(self, split, kind, B, stride):
        """{gather the next batch, train step or evaluated batch} as one hipGraph on static buffers.  Warm-up runs first
        (sizes workspaces); the train warm-up's update is undone, so capturing trains nothing."""
        if self.is_painn:
            raise NotImplementedError("PaiNN runs the eager step and evaluation only (its radius graph is built per batch)")
        NA = split.num_atoms
        dev = self.device
        pos, y, f = torch.zeros(B * NA, 3, device=dev), torch.zeros(B, device=dev), torch.zeros(B * NA, 3, device=dev)
        b = self._template(split, B)
        train = kind == "train"
        perm = torch.arange(len(split), dtype=torch.int32, device=dev) if train else None
        ctr = self._train_ctr if train else self._eval_ctr

        def body():
            hip.md17_gather_batch(split.pos, split.y, split.force, perm, ctr, stride, pos, y, f)
            if train:
                return self._train_body(b, pos, y, f)
            self._eval_body(b, pos, y, f, self.eval_acc)
            return None

        snap = optimizer_snapshot(self.opt, self.loss_acc) if train else None
        ctr.zero_()
        for _ in range(2 if train else 1):
            body()
        with CaptureSession(self.opt if train else None, dev) as session, session.graph() as g:
            loss = body()
        if train:
            torch.cuda.synchronize()
            optimizer_restore(self.opt, snap, self.loss_acc)
        ctr.zero_()
        self.eval_acc.zero_()
        # (the static buffers the graph reads and writes live as long as its record)
        return CapturedStep(g, self._refreshed if train else None, split=split, perm=perm, loss=loss, buffers=(pos, y, f))

    def _graph(self, split, kind, B, stride):
        key = (kind, id(split), B, stride)
        st = self._graphs.get(key)
        if st is None or st.split is not split:
            st = self._graphs[key] = self._capture(split, kind, B, stride)
        return st

    # ---- epochs ------------------------------------------------------------------------------------------------------
    def train_epoch(self, split, generator=None, captured=None):
        """train() (:34-88): a fresh shuffle (torch.randperm(len(split), generator=generator), RandomSampler's draw),
        batches of train_batch_size; SchNet's full batches replay one captured step each, fed by the gather kernel from the
        device permutation; the short last batch and PaiNN take the eager step.  Every step loss goes into a device sum;
        returns loss_acc / len(loader) after one host read, then steps the scheduler."""
        captured = self.captured if captured is None else captured
        M, bs = len(split), self.train_batch_size
        perm = torch.randperm(M, generator=generator)
        n_full, rem = M // bs, M % bs
        use_graph = captured and not self.is_painn and n_full > 0
        if use_graph:
            st = self._graph(split, "train", bs, bs)
        self.loss_acc.zero_()
        if use_graph:
            st.perm.copy_(perm.to(torch.int32))
            self._train_ctr.zero_()
            for _ in range(n_full):
                st.replay()
            self.last_loss = st.loss
        else:
            perm_d = perm.to(self.device)
            for k in range(n_full):
                self.step(split, perm_d[k * bs:(k + 1) * bs])
        if rem:
            self.step(split, perm.to(self.device)[n_full * bs:])
        acc = float(self.loss_acc.item())
        self.scheduler_step()
        return acc / (n_full + (1 if rem else 0))

    def evaluate(self, split, batch_size=128, captured=None):
        """eval() (:93-142): (energy MAE, force MAE) over the split in loader order.  SchNet: one captured graph per batch
        size that occurs (the full batches and the short last one), replayed with nothing read by the host until the end.
        Parameters, Adam state and every .grad are left as they were.  Where predicted forces are NaN, the force MAE is
        the mean over the kept entries (the script reshapes them to [-1, 3] and fails unless their count is a multiple
        of 3)."""
        captured = self.captured if captured is None else captured
        M = len(split)
        n_full, rem = M // batch_size, M % batch_size
        acc = self.eval_acc
        if captured and not self.is_painn:
            sts = [(self._graph(split, "eval", batch_size, batch_size), n_full) if n_full else None,
                   (self._graph(split, "eval", rem, batch_size), 1) if rem else None]
            acc.zero_()
            self._eval_ctr.zero_()
            wcache.sync_weight_copies()
            for item in sts:
                if item is not None:
                    for _ in range(item[1]):
                        item[0].graph.replay()
        else:
            acc.zero_()
            ar = torch.arange(M, device=self.device)
            for k in range(n_full + (1 if rem else 0)):
                idx = ar[k * batch_size:(k + 1) * batch_size]
                pos, y, f = split.rows(idx)
                b = self._template(split, int(idx.numel()))
                if self.is_painn:
                    self._painn_edges(b, pos)
                self._eval_body(b, pos, y, f, acc)
        a = acc.cpu().tolist()
        return a[0] / a[1], a[2] / a[3]

    # ---- the main loop (:324-366) ------------------------------------------------------------------------------------
    def fit(self, train, valid, test, eval_train=False, eval_test=True, print_every_epoch=1, output_model_dir="",
            eval_batch_size=128, generator=None, log=print):
        """Epochs 1..epochs: train_epoch, then every print_every_epoch epochs the train (its own batch size), validation and
        test MAEs; model.pth when the validation force MAE improves (with output_model_dir), model_final.pth at the end.
        The final test numbers are those of the best validation epoch (eval_test) or an evaluation after reloading model.pth
        with load_latest (otherwise).  Returns the per-epoch lists, the step losses' means and the selection."""
        h = {k: [] for k in ("loss", "train_energy", "train_force", "val_energy", "val_force", "test_energy", "test_force")}
        best_val_force, best_val_idx = 1e10, None
        for epoch in range(1, self.epochs + 1):
            h["loss"].append(self.train_epoch(train, generator=generator))
            if log:
                log("Epoch: {}\nLoss: {}".format(epoch, h["loss"][-1]))
            if epoch % print_every_epoch == 0:
                tr = self.evaluate(train, self.train_batch_size) if eval_train else (0, 0)
                va = self.evaluate(valid, eval_batch_size)
                te = self.evaluate(test, eval_batch_size) if eval_test else (0, 0)
                for name, v in (("train", tr), ("val", va), ("test", te)):
                    h[name + "_energy"].append(v[0])
                    h[name + "_force"].append(v[1])
                if log:
                    log("Energy\ttrain: {:.6f}\tval: {:.6f}\ttest: {:.6f}".format(tr[0], va[0], te[0]))
                    log("Force\ttrain: {:.6f}\tval: {:.6f}\ttest: {:.6f}".format(tr[1], va[1], te[1]))
                if va[1] < best_val_force:
                    best_val_force, best_val_idx = va[1], len(h["train_energy"]) - 1
                    if output_model_dir != "":
                        self.save_model(os.path.join(output_model_dir, "model.pth"))
        if output_model_dir != "":
            self.save_model(os.path.join(output_model_dir, "model_final.pth"))
        if best_val_idx is None:
            raise RuntimeError("no evaluation ran (epochs < print_every_epoch): there is no best validation epoch")
        if eval_test:
            best_test = (h["test_energy"][best_val_idx], h["test_force"][best_val_idx])
        else:
            self.load_model(os.path.join(output_model_dir, "model.pth"), load_latest=True)
            best_test = self.evaluate(test, eval_batch_size)
        h.update(best_val_idx=best_val_idx, best_test_energy=best_test[0], best_test_force=best_test[1])
        return h

    # ---- checkpoints: scheduler_step and save_model (:163-186) are finetune_common.FineTuner's --------------------------
    def load_model(self, path, load_latest=False):
        """load_model (:145-160): see load_state."""
        self._load_model(path, load_latest)
