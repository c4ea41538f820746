"""Canonical synthetic PCQM4Mv2-shaped / QM9-shaped / MD17-shaped batches.

No dataset exists in the build or GPU containers, so bench.py and the parity tests use this
generator.  Recipe (seeded, numpy Generator):
  n = clip(round(N(14.1, 2.9)), 2, 20) heavy atoms; bonds = random tree (parent in [i-3, i)) +
  Poisson(1.5) ring closures, both directions stored consecutively (dataset_utils.py:144-151);
  x[:,0] in {5,6,7,8,15,16}, other OGB columns uniform; positions = 1.5 A random walk along the
  tree, centred (dataset_3D.py:120-122); extended edges = pairs within <= 4 bonds
  (dataset_3D.py:12-35).
"""
import numpy as np
import torch

from .batch import Batch, MolData, extend_graph_index

ATOM_DIMS = [119, 4, 12, 12, 10, 6, 6, 2, 2]
BOND_DIMS_USED = [4, 3, 2]


def _tree_walk_positions(rng, n, parent, step=1.5):
    pos = np.zeros((n, 3), dtype=np.float64)
    for i in range(1, n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d) + 1e-12
        pos[i] = pos[parent[i]] + step * d
    pos -= pos.mean(axis=0, keepdims=True)
    return pos.astype(np.float32)


def make_molecule(rng, n=None, with_h=False):
    if n is None:
        n = int(np.clip(np.rint(rng.normal(14.1, 2.9)), 2, 20))
    parent = np.zeros(n, dtype=np.int64)
    pairs = []
    for i in range(1, n):
        parent[i] = rng.integers(max(0, i - 3), i)
        pairs.append((int(parent[i]), i))
    have = set(pairs)
    for _ in range(int(rng.poisson(1.5))):
        if n < 3:
            break
        a, b = rng.integers(0, n, size=2)
        a, b = int(min(a, b)), int(max(a, b))
        if a != b and (a, b) not in have:
            have.add((a, b))
            pairs.append((a, b))
    src, dst, attr = [], [], []
    for a, b in pairs:
        ea = [int(rng.integers(0, d)) for d in BOND_DIMS_USED]
        src += [a, b]
        dst += [b, a]
        attr += [ea, ea]
    x = np.zeros((n, 9), dtype=np.int64)
    x[:, 0] = rng.choice([5, 6, 7, 8, 15, 16], size=n)
    if with_h:
        x[rng.random(n) < 0.5, 0] = 0
    for k in range(1, 9):
        x[:, k] = rng.integers(0, ATOM_DIMS[k], size=n)
    edge_index = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    d = MolData(
        x=torch.from_numpy(x),
        edge_index=edge_index,
        edge_attr=torch.tensor(attr, dtype=torch.long).reshape(-1, 3),
        positions=torch.from_numpy(_tree_walk_positions(rng, n, parent)),
    )
    d.extended_edge_index = extend_graph_index(edge_index, n)
    return d


def make_batch(num_graphs=256, seed=0, sizes=None):
    """PCQM4Mv2-shaped batch (config 2/3 of BASELINE.json)."""
    rng = np.random.default_rng(seed)
    mols = [make_molecule(rng, None if sizes is None else int(sizes[i])) for i in range(num_graphs)]
    return Batch.from_data_list(mols)


def make_qm9_batch(num_graphs=32, seed=0):
    """QM9-shaped batch (config 1): n ~ 18 atoms incl. H, <= 29; 1-D z in `x`."""
    rng = np.random.default_rng(seed)
    mols = []
    for _ in range(num_graphs):
        n = int(np.clip(np.rint(rng.normal(18.0, 3.0)), 3, 29))
        m = make_molecule(rng, n, with_h=True)
        m.x = m.x[:, 0].contiguous()
        mols.append(m)
    return Batch.from_data_list(mols)


def make_qm9_targets(b, seed=0, noise=0.05):
    """Targets [B, 13] (float32) of a 1-D z batch as a deterministic function of the molecule: per target, a sum of per-
    element contributions, a term in the mean interatomic distance, and seeded noise -- something a property regression can
    actually fit.  The coefficients are fixed (seed 1234); `seed` draws the noise only."""
    coef = np.random.default_rng(1234)
    per_z = coef.normal(0.0, 1.0, size=(119, 13))
    per_r = coef.normal(0.0, 1.0, size=13)
    rng = np.random.default_rng(seed)
    z = b.x.numpy() if b.x.dim() == 1 else b.x[:, 0].numpy()
    pos = b.positions.detach().double().numpy()
    cnt = torch.bincount(b.batch, minlength=b.num_graphs).numpy()
    out = np.zeros((b.num_graphs, 13))
    a = 0
    for i, n in enumerate(cnt):
        zz, p = z[a:a + n], pos[a:a + n]
        d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        r = d.sum() / max(n * (n - 1), 1)
        out[i] = per_z[zz].sum(0) / np.sqrt(max(n, 1)) + per_r * r
        a += n
    out += noise * rng.normal(size=out.shape)
    return torch.from_numpy(out.astype(np.float32))


def seeded_parameters(module, seed=0):
    """Overwrite every parameter of `module` with a seeded draw that depends on its NAME and shape only (crc32 of the name
    folded into the seed; normal / sqrt(fan_in) for matrices, 0.1 * normal for vectors): two modules with the same parameter
    names get the same values whatever their construction order, so a stored fixture need not carry initial weights."""
    import zlib
    with torch.no_grad():
        for name, p in module.named_parameters():
            g = torch.Generator().manual_seed((int(seed) * 1000003 + zlib.crc32(name.encode())) & 0x7FFFFFFFFFFFFFFF)
            v = torch.randn(p.shape, generator=g, dtype=torch.float32)
            v = v / float(np.sqrt(p.shape[-1])) if p.dim() >= 2 else 0.1 * v
            p.copy_(v.to(p.device, p.dtype))
    return module


def make_md17_batch(num_graphs=1, seed=0, n_atoms=21):
    """MD17-aspirin-shaped batch (config 5): 21 atoms, 1-D z."""
    rng = np.random.default_rng(seed)
    mols = []
    for _ in range(num_graphs):
        m = make_molecule(rng, n_atoms, with_h=True)
        m.x = m.x[:, 0].contiguous()
        mols.append(m)
    return Batch.from_data_list(mols)


def molnet_sizes(rng, num_graphs, max_atoms=150, tail=0.03):
    """Heavy-atom counts of a MoleculeNet-shaped batch: round(lognormal(log 22, 0.4)) clipped to [2, 60] for most molecules,
    a `tail` fraction uniform in [60, max_atoms].  UNVERIFIED: no MoleculeNet dataset exists here; the shape follows figures
    quoted from memory (Tox21 averages about 18 heavy atoms, HIV has molecules past 200) and is meant to put molecules of
    more than 32 atoms into every batch, not to match any dataset's histogram."""
    n = np.clip(np.rint(rng.lognormal(np.log(22.0), 0.4, size=num_graphs)), 2, 60).astype(np.int64)
    big = rng.random(num_graphs) < tail
    n[big] = rng.integers(60, max_atoms + 1, size=int(big.sum()))
    return n


def make_molnet_batch(num_graphs=32, num_tasks=12, seed=0, missing=0.2, pos_rate=0.2, max_atoms=150, tail=0.03, sizes=None):
    """MoleculeNet-shaped 2D batch (finetune_MoleculeNet.py): x [N, 9], edge_index, edge_attr [E, 3] and labels y [B, T] in
    {-1, 0, +1} (float32, 0 = missing with probability `missing`, +1 with probability `pos_rate` among the rest).  Sizes from
    molnet_sizes (or `sizes`).  No positions: the fine-tune reads the 2D graph only."""
    rng = np.random.default_rng(seed)
    sizes = molnet_sizes(rng, num_graphs, max_atoms, tail) if sizes is None else np.asarray(sizes, dtype=np.int64)
    mols = []
    for i in range(num_graphs):
        m = make_molecule(rng, int(sizes[i]))
        del m.positions, m.extended_edge_index
        lab = np.where(rng.random(num_tasks) < pos_rate, 1.0, -1.0)
        lab[rng.random(num_tasks) < missing] = 0.0
        m.y = torch.from_numpy(lab.astype(np.float32)).view(1, num_tasks)
        mols.append(m)
    return Batch.from_data_list(mols)


def batch_stats(b, cutoff=10.0):
    """N, E_b, E_e, E_r (radius edges, strict < cutoff, no self loops), sum n^2, N_max."""
    N = b.x.size(0)
    pos = b.positions.detach().cpu().double()
    bid = b.batch.cpu()
    counts = torch.bincount(bid, minlength=b.num_graphs)
    E_r = 0
    start = 0
    for c in counts.tolist():
        p = pos[start:start + c]
        d2 = ((p[:, None] - p[None]) ** 2).sum(-1)
        E_r += int((d2 < cutoff * cutoff).sum()) - c
        start += c
    return {
        "N": int(N), "B": int(b.num_graphs), "E_b": int(b.edge_index.size(1)),
        "E_e": int(b.extended_edge_index.size(1)) if hasattr(b, "extended_edge_index") else 0,
        "E_r": int(E_r), "sum_n2": int((counts.double() ** 2).sum()), "N_max": int(counts.max()),
    }
