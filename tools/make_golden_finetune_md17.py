"""Generate tests/golden/finetune_md17.npz: two epochs of examples/finetune_MD17.py on the GENUINE reference SchNet
(oracle/ref_loader.verbatim(): Geom3D.models.SchNet on the stand-in third-party layer), torch.nn.Linear(emb, 1),
torch.nn.L1Loss with the 0.05 / 0.95 energy / force coefficients, torch.optim.Adam over the script's two param groups and
CosineAnnealingLR(T_max=2) stepped once per epoch.  The script cannot be imported (its config module parses argv, it loads
datasets), so the bodies of train() (:34-88), eval() (:93-142) and the normalisation loop (:218-232) are restated below.

Settings: SchNet(hidden 32, 32 filters, 2 interactions, 51 gaussians, cutoff 10, mean readout) on one 12-atom molecule;
train / valid / test splits of 5 / 5 / 7 conformations (the molecule's positions plus noise); train batch size 2 (a short
last batch of 1), evaluation batch size 3 (short last batches of 2 and 1).  The train loader's order per epoch is
torch.randperm(5, generator) with generator = torch.Generator().manual_seed(PERM_SEED) made once (RandomSampler's draw).
Two runs: "raw." (no normalisation, targets of order 1) and "norm." (--energy_force_with_normalization, energies at MD17
scale, about -4e5, forces of order 30).  The initial parameters are synthetic.seeded_parameters(model, SEED) and
(head, SEED + 1).  Stored per run: every step's loss, loss_acc per epoch, the parameters after training (the conv.nn.*
aliases of mlp.* once), and the validation and test (energy MAE, force MAE) of both epochs.  Every stored step has
min |E - y| and min |F - f| above 1e-4, so no L1 sign can flip inside fp32 tolerance.

    python tools/make_golden_finetune_md17.py        (needs the reference checkout: build container only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from moleculesde_amd.synthetic import make_molecule, seeded_parameters  # noqa: E402

EMB, FILTERS, INTER, GAUSS, CUTOFF, LR, EPOCHS, SEED, PERM_SEED = 32, 32, 2, 51, 10.0, 5e-4, 2, 5, 77
NA, SIZES, TRAIN_BS, EVAL_BS, CE, CF = 12, (5, 5, 7), 2, 3, 0.05, 0.95


def make_data():
    rng = np.random.default_rng(17)
    m = make_molecule(rng, NA, with_h=True)
    x = m.x[:, 0].clone()
    g = torch.Generator().manual_seed(23)
    out = {"x": x}
    for name, M in zip(("train", "valid", "test"), SIZES):
        out[name + ".pos"] = m.positions[None] + 0.1 * torch.randn(M, NA, 3, generator=g)
        out[name + ".y_raw"] = torch.randn(M, generator=g)
        out[name + ".f_raw"] = torch.randn(M, NA, 3, generator=g)
        out[name + ".y_norm"] = -4.0e5 + 5.0 * torch.randn(M, generator=g)
        out[name + ".f_norm"] = 30.0 * torch.randn(M, NA, 3, generator=g)
    return out


def unique_state(model):
    return {k: v for k, v in model.state_dict().items() if ".conv.nn." not in k}


def run(ref, data, kind):
    torch.manual_seed(321)
    model = ref.SchNet(hidden_channels=EMB, num_filters=FILTERS, num_interactions=INTER, num_gaussians=GAUSS, cutoff=CUTOFF,
                       readout="mean", node_class=119)
    head = torch.nn.Linear(EMB, 1)
    seeded_parameters(model, SEED)
    seeded_parameters(head, SEED + 1)
    x = data["x"]
    split = {n: (data[n + ".pos"], data[n + f".y_{kind}"], data[n + f".f_{kind}"]) for n in ("train", "valid", "test")}
    norm = None
    if kind == "norm":                      # :218-232
        e_total, f_total, n_atom = 0, 0, None
        for i in range(SIZES[0]):
            energy, force = split["train"][1][i:i + 1], split["train"][2][i]
            n_atom = force.size()[0]
            e_total += energy / n_atom
            f_total += torch.sqrt(torch.mean(force.square()))
        e_total /= SIZES[0]
        f_total /= SIZES[0]
        norm = (e_total, f_total, n_atom)

    def loader(name, bs, order):
        pos, y, f = split[name]
        for k in range(0, len(order), bs):
            idx = order[k:k + bs]
            b = len(idx)
            yield (x.repeat(b), pos[idx].reshape(-1, 3).clone(), torch.arange(b).repeat_interleave(NA), y[idx].clone(),
                   f[idx].reshape(-1, 3).clone())

    def energy_of(xb, positions, batch):
        e = head(model(xb, positions, batch)).squeeze(1)
        if norm is not None:
            e = e * norm[1] + norm[0] * norm[2]
        return e

    criterion = torch.nn.L1Loss()
    optimizer = torch.optim.Adam([{"params": model.parameters(), "lr": LR}, {"params": head.parameters(), "lr": LR}],
                                 lr=LR, weight_decay=0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, EPOCHS)
    gen = torch.Generator().manual_seed(PERM_SEED)
    out = {"losses": [], "loss_acc": [], "val": [], "test": []}
    for _ in range(EPOCHS):
        model.train()
        head.train()
        order = torch.randperm(SIZES[0], generator=gen)
        acc, n = 0.0, 0
        for xb, positions, batch, y, f in loader("train", TRAIN_BS, order):       # train(), :46-78
            positions.requires_grad_()
            e = energy_of(xb, positions, batch)
            force = -torch.autograd.grad(outputs=e, inputs=positions, grad_outputs=torch.ones_like(e), create_graph=True,
                                         retain_graph=True)[0]
            gap = min(float((e.detach() - y).abs().min()), float((force.detach() - f).abs().min()))
            assert gap > 1e-4, gap
            loss = CE * criterion(e, y) + CF * criterion(force, f)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            acc += loss.cpu().detach().item()
            out["losses"].append(float(loss.item()))
            n += 1
        out["loss_acc"].append(acc / n)
        sched.step()
        for name in ("valid", "test"):                                               # eval(), :93-142
            model.eval()
            head.eval()
            pe, ae = [], []
            pf, af = torch.Tensor([]), torch.Tensor([])
            for xb, positions, batch, y, f in loader(name, EVAL_BS, torch.arange(len(split[name][1]))):
                positions.requires_grad_()
                e = energy_of(xb, positions, batch)
                force = -torch.autograd.grad(outputs=e, inputs=positions, grad_outputs=torch.ones_like(e),
                                             create_graph=True, retain_graph=True)[0].detach_()
                if torch.sum(torch.isnan(force)) != 0:
                    mask = torch.isnan(force)
                    force = force[~mask].reshape((-1, 3))
                    f = f[~mask].reshape((-1, 3))
                pe.append(e.cpu().detach())
                ae.append(y.cpu())
                pf = torch.cat([pf, force], dim=0)
                af = torch.cat([af, f], dim=0)
            pe, ae = torch.cat(pe), torch.cat(ae)
            out["val" if name == "valid" else "test"].append(
                [torch.mean(torch.abs(pe - ae)).item(), torch.mean(torch.abs(pf - af)).item()])
    res = {f"{kind}.losses": np.array(out["losses"]), f"{kind}.loss_acc": np.array(out["loss_acc"]),
           f"{kind}.val": np.array(out["val"]), f"{kind}.test": np.array(out["test"])}
    res.update({f"{kind}.sd_after." + k: v.numpy().copy() for k, v in unique_state(model).items()})
    res.update({f"{kind}.head_after." + k: v.detach().numpy().copy() for k, v in head.state_dict().items()})
    if norm is not None:
        res["norm.e_mean"], res["norm.f_mean"], res["norm.n_atom"] = norm[0].numpy(), norm[1].numpy(), np.int64(norm[2])
    return res


def main():
    ref = ref_loader.verbatim()
    data = make_data()
    out = {k: v.numpy() for k, v in data.items()}
    out.update(lr=np.float64(LR), emb=np.int64(EMB), filters=np.int64(FILTERS), interactions=np.int64(INTER),
               gaussians=np.int64(GAUSS), cutoff=np.float64(CUTOFF), epochs=np.int64(EPOCHS), seed=np.int64(SEED),
               perm_seed=np.int64(PERM_SEED), train_bs=np.int64(TRAIN_BS), eval_bs=np.int64(EVAL_BS))
    for kind in ("raw", "norm"):
        out.update(run(ref, data, kind))
    path = os.path.join(ROOT, "tests", "golden", "finetune_md17.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")
    for kind in ("raw", "norm"):
        print(kind, out[f"{kind}.losses"], out[f"{kind}.loss_acc"], out[f"{kind}.val"], out[f"{kind}.test"])


if __name__ == "__main__":
    main()
