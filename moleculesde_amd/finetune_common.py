"""What the three fine-tuning loops (finetune_molnet, finetune_qm9, finetune_md17) share: the per-epoch schedulers, the
checkpoint layouts of the scripts' save_model / load_model, PaiNN's radius graph and the device check."""
import math

import torch

from . import wcache


def hip_device(param, module):
    """The device of `param`; the fine-tuning loops run on the HIP device only."""
    if param.device.type != "cuda":
        raise RuntimeError(f"moleculesde_amd.{module} runs on the HIP device only (no CPU fallback)")
    return param.device


# ---- CosineAnnealingLR(optimizer, T_max), eta_min = 0, stepped once per epoch ----------------------------------------------
class CosineAnnealing:
    """The learning rates torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max) gives after each step(): the same recursive
    update as torch's get_lr, so the values agree to the last bit, not only to the closed form."""

    def __init__(self, base_lrs, T_max, eta_min=0.0):
        self.base_lrs = [float(v) for v in base_lrs]
        self.lrs = list(self.base_lrs)
        self.T_max, self.eta_min, self.last_epoch = int(T_max), float(eta_min), 0

    def step(self):
        self.last_epoch += 1
        e, T, lo = self.last_epoch, self.T_max, self.eta_min
        if (e - 1 - T) % (2 * T) == 0:
            self.lrs = [lr + (b - lo) * (1 - math.cos(math.pi / T)) / 2 for lr, b in zip(self.lrs, self.base_lrs)]
        else:
            self.lrs = [(1 + math.cos(math.pi * e / T)) / (1 + math.cos(math.pi * (e - 1) / T)) * (lr - lo) + lo
                        for lr in self.lrs]
        return list(self.lrs)


# ---- StepLR(optimizer, step_size, gamma), stepped once per epoch ------------------------------------------------------------
class StepDecay:
    """The learning rates torch.optim.lr_scheduler.StepLR(opt, step_size, gamma) gives after each step(): torch's recursive
    form (lr * gamma at every multiple of step_size), bit for bit."""

    def __init__(self, base_lrs, step_size, gamma=0.1):
        self.lrs = [float(v) for v in base_lrs]
        self.step_size, self.gamma, self.last_epoch = int(step_size), float(gamma), 0

    def step(self):
        self.last_epoch += 1
        if self.last_epoch % self.step_size == 0:
            self.lrs = [lr * self.gamma for lr in self.lrs]
        return list(self.lrs)


def make_scheduler(lr_scheduler, base_lrs, epochs, lr_decay_step_size, lr_decay_factor, strict=False):
    """The per-epoch schedulers of the scripts (finetune_MD17.py:297-321): CosineAnnealingLR(epochs) or StepLR.  The two
    per-iteration / metric schedulers are refused; any other name gives None (finetune_MD17.py), or with `strict`
    (finetune_QM9.py) only None / "None" do and the rest is an error."""
    if lr_scheduler in ("CosineAnnealingWarmRestarts", "ReduceLROnPlateau"):
        raise NotImplementedError(f"lr_scheduler={lr_scheduler!r} is not supported: CosineAnnealingLR, StepLR or None")
    if lr_scheduler == "CosineAnnealingLR":
        return CosineAnnealing(base_lrs, epochs)
    if lr_scheduler == "StepLR":
        return StepDecay(base_lrs, lr_decay_step_size, lr_decay_factor)
    if strict and lr_scheduler not in (None, "None"):
        raise ValueError(f"lr scheduler {lr_scheduler!r} is not included")
    return None


# ---- checkpoints ------------------------------------------------------------------------------------------------------------
def checkpoint_dict(model, graph_pred_linear):
    """save_model of the scripts: {"model": ..., "graph_pred_linear": ...}."""
    d = {"model": model.state_dict()}
    if graph_pred_linear is not None:
        d["graph_pred_linear"] = graph_pred_linear.state_dict()
    return d


def load_state(model, graph_pred_linear, path, keys, raw_ok=False, load_latest=False):
    """load_model of the scripts: the encoder from the first of `keys` the file has (a pretraining checkpoint of
    pretrain.Trainer.save names it model_2D / model_3D, a fine-tuning one `model`); raw_ok: a file with none of them is a
    raw state dict; load_latest takes `model` whatever else is there.  `graph_pred_linear` (when given) whenever the file
    has it."""
    w = torch.load(path, map_location="cpu")
    key = "model" if load_latest else next((k for k in keys if k in w), None if raw_ok else keys[-1])
    model.load_state_dict(w if key is None else w[key])
    if graph_pred_linear is not None and "graph_pred_linear" in w:
        graph_pred_linear.load_state_dict(w["graph_pred_linear"])
    return w


def painn_radius_edges(model, batch, positions):
    """PaiNN's radius_edge_index of `positions` (dataset_3D_Radius.py:155; MoleculeDataset3DRadius builds it per
    conformation), built with the radius kernels, attached to the batch and returned.  The old index stays alive while the
    new one is made, so the model's edge-plan cache (keyed by address) cannot see a reused one."""
    from . import hip, plan as _pl
    pl = _pl.get_plan(batch)
    rp, _ = hip.radius_plan(positions, pl.batch_i32, pl.mol_ptr, model.cutoff, pl.E_r_cap, 32,
                            n_max=getattr(pl, "N_max", None))
    keep = rp.src >= 0                                    # host sync: PaiNN batches are not graph-captured
    # PyG radius_graph orientation: row 0 = source, row 1 = target (the 32-neighbour cap applies per TARGET);
    # PaiNN aggregates at row 0 (painn.py:235), i.e. at the source, exactly as the reference does
    batch.radius_edge_index = torch.stack([rp.src[keep], rp.dst[keep]]).long()
    return batch.radius_edge_index


class FineTuner:
    """The epoch scheduler and the checkpoints of a fine-tuning trainer (self.model, self.head, self.opt, self.scheduler)."""
    LOAD_KEYS, RAW_OK, LOADS_HEAD = ("model_3D", "model"), False, True

    def scheduler_step(self):
        """lr_scheduler.step() once per epoch: the new rates go into FlatAdam's per-group table on the device."""
        if self.scheduler is not None:
            self.opt.set_lr(self.scheduler.step())

    def load_model(self, path):
        """load_model of the script (see load_state)."""
        self._load_model(path)

    def _load_model(self, path, load_latest=False):
        with torch.no_grad():
            load_state(self.model, self.head if self.LOADS_HEAD else None, path, self.LOAD_KEYS, self.RAW_OK, load_latest)
        wcache.bump_weight_epoch()

    def save_model(self, path):
        """save_model of the script: {"model", "graph_pred_linear"} at `path` (model.pth for the best validation epoch,
        model_final.pth for the last)."""
        torch.save(checkpoint_dict(self.model, self.head), path)
