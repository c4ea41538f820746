"""Shared helpers for the parity tests: golden loading, state-dict / batch reconstruction."""
import os

import numpy as np
import torch

from moleculesde_amd.batch import Batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def record_parity(line):
    """Achieved parity numbers of a GPU test run, kept: appended to gpurun_out/parity_numbers.txt (scratch that gpurun merges
    back; the round's copy is committed as profiles/rNN_parity_numbers.txt) and printed."""
    print(line)
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_numbers.txt"), "a") as f:
            f.write(line.rstrip("\n") + "\n")
    except OSError:
        pass


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def sub(g, prefix):
    """Tensors of all entries with the given prefix, prefix stripped."""
    return {k[len(prefix):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(prefix)}


def batch_from(g, prefix="batch."):
    d = sub(g, prefix)
    ng = int(d.pop("num_graphs"))
    b = Batch(**d)
    b.num_graphs = ng
    return b


def disable_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    return model


def assert_close(a, b, rtol, atol, what=""):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())}/{a.numel()} mismatches, max abs err {err.max().item():.3e}, "
        f"ref scale {b.abs().max().item():.3e}")


def grads_close(model, ggrads, rtol, atol_scale, what=""):
    """Compare parameter grads to golden grads; atol is scaled by the largest grad magnitude of the
    whole model (gradients that are analytically zero -- bias before BatchNorm, key bias under
    softmax -- are pure rounding noise on both sides)."""
    scale = max(float(np.abs(v).max()) for v in ggrads.values()) if ggrads else 1.0
    for n, p in model.named_parameters():
        if n not in ggrads:
            continue
        assert p.grad is not None, f"{what}: no grad for {n}"
        assert_close(p.grad, ggrads[n], rtol, atol_scale * scale, f"{what}:{n}")


def fill_like_generator(net, base):
    """Deterministic parameter fill of oracle/make_golden_dense_prod.py::set_parameters (per-parameter seeded generator)."""
    with torch.no_grad():
        for i, (_, p) in enumerate(net.named_parameters()):
            gen = torch.Generator().manual_seed(base + i)
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=gen) * 0.6 - 0.3)
            else:
                fan = p.shape[1] if p.shape[0] != p.shape[1] else p.shape[0]
                p.copy_(torch.randn(p.shape, generator=gen) / fan ** 0.5)


# ------------------------------------------------------------------ molecules of an exact size and bond pattern ---
def spread_positions(rng, n, min_sep=1.0):
    """n random points in 3D, pairwise at least `min_sep` apart (so no edge frame of coord2basis is degenerate), centred."""
    side = 1.4 * max(n, 1) ** (1.0 / 3.0) + 1.0
    pos = np.zeros((0, 3))
    while pos.shape[0] < n:
        p = rng.uniform(-side / 2, side / 2, size=3)
        if pos.shape[0] == 0 or np.sqrt(((pos - p) ** 2).sum(-1)).min() >= min_sep:
            pos = np.vstack([pos, p])
    pos -= pos.mean(axis=0, keepdims=True)
    return torch.from_numpy(pos.astype(np.float32))


def bond_pairs(rng, n, pattern, p_dense=0.3):
    """Undirected bonds (a < b) of an n-atom molecule:
    chain   0-1-2-...: the fewest extended edges (8 n - 20 for n >= 5);
    hub     atom 0 bonded to every other atom: every pair within 2 bonds, extended edges n (n - 1);
    dense   every pair bonded with probability p_dense on top of a chain (connected, many bonds per atom);
    random  the spanning tree + ring closures of synthetic.make_molecule."""
    if pattern == "chain":
        return [(i - 1, i) for i in range(1, n)]
    if pattern == "hub":
        return [(0, i) for i in range(1, n)]
    if pattern == "dense":
        pairs = {(i - 1, i) for i in range(1, n)}
        pairs |= {(a, b) for a in range(n) for b in range(a + 2, n) if rng.random() < p_dense}
        return sorted(pairs)
    if pattern == "random":
        from moleculesde_amd.synthetic import make_molecule
        ei = make_molecule(rng, n).edge_index
        return [(int(a), int(b)) for a, b in ei.t().tolist() if a < b]
    raise ValueError(pattern)


def build_molecule(rng, n, pattern="random", bondless=(), p_dense=0.3):
    """A molecule of exactly n atoms with the given bond pattern (see bond_pairs), both bond directions stored consecutively,
    OGB-shaped atom / bond features, spread positions and the extended (<= 4 bonds) edge index.  Atoms in `bondless` lose
    every bond (node_flags = 0 for them in the 3D->2D head)."""
    from moleculesde_amd.batch import MolData, extend_graph_index
    from moleculesde_amd.synthetic import ATOM_DIMS, BOND_DIMS_USED
    pairs = [(a, b) for a, b in bond_pairs(rng, n, pattern, p_dense) if a not in bondless and b not in bondless]
    src, dst, attr = [], [], []
    for a, b in pairs:
        ea = [int(rng.integers(0, d)) for d in BOND_DIMS_USED]
        src += [a, b]
        dst += [b, a]
        attr += [ea, ea]
    x = np.zeros((n, 9), dtype=np.int64)
    x[:, 0] = rng.choice([5, 6, 7, 8, 15, 16], size=n)
    for k in range(1, 9):
        x[:, k] = rng.integers(0, ATOM_DIMS[k], size=n)
    edge_index = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    d = MolData(x=torch.from_numpy(x), edge_index=edge_index, edge_attr=torch.tensor(attr, dtype=torch.long).reshape(-1, 3),
                positions=spread_positions(rng, n))
    d.extended_edge_index = extend_graph_index(edge_index, n)
    return d


def build_batch(specs, seed=0):
    """Batch of build_molecule(n, pattern, bondless) for specs = [(n, pattern) or (n, pattern, bondless), ...]."""
    from moleculesde_amd.batch import Batch
    rng = np.random.default_rng(seed)
    return Batch.from_data_list([build_molecule(rng, s[0], s[1], s[2] if len(s) > 2 else ()) for s in specs])


def mol_edge_counts(b, attr="extended_edge_index"):
    """Per-molecule edge counts of a host batch."""
    ei = getattr(b, attr)
    return torch.bincount(b.batch[ei[1]], minlength=b.num_graphs).tolist()


ROW_BLOCKS = ((0, 16), (16, 20), (20, 10 ** 9))


def block_errors(got, ref, sizes, padded, scale=None):
    """Worst |got - ref| / scale over atom rows [0,16), [16,20), [20,n) of every molecule.  padded: [B, Nmax, ...] (row = atom
    index within its molecule); else ragged [sum n, ...] (atom rows in batch order).  None: the batch has no such rows."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    scale = float(ref.abs().max()) if scale is None else scale
    scale = scale if scale > 0 else 1.0
    out = []
    for lo, hi in ROW_BLOCKS:
        worst, start = None, 0
        for b, n in enumerate(sizes):
            if padded:
                g, r = got[b, lo:min(hi, n)], ref[b, lo:min(hi, n)]
            else:
                g, r = got[start + lo:start + min(hi, n)], ref[start + lo:start + min(hi, n)]
            start += n
            if g.numel():
                e = float((g - r).abs().max()) / scale
                worst = e if worst is None else max(worst, e)
        out.append(worst)
    return out


def fmt_blocks(errs):
    return " ".join(f"{name} {'-' if e is None else f'{e:.1e}'}" for name, e in zip(("[0,16)", "[16,20)", "[20,n)"), errs))


# batches of the molecule-size tests (tests/test_gpu_mol_size.py); their sizes and edge counts are pinned on the host by
# tests/test_mol_size_host.py
ES_EAL, ES_EMAX = 384, 992          # csrc/escore_mol.h: edge features in LDS up to ES_EAL extended edges per molecule
ESCORE_SPECS = [(20, "hub"), (21, "hub"), (32, "hub"), (32, "chain"), (17, "random"), (16, "random"), (31, "random"),
                (24, "dense"), (19, "chain")]
ESCORE_EM = [380, 420, 992, 236, None, None, None, 552, 132]     # None: whatever the random tree gives (checked < 384)


# batch of the score-graph kernel tests (tests/test_gpu_score_graph.py), built with seed SCORE_GRAPH_SEED; its node / edge
# counts and in-degrees ({0, 1, 2, 7..16, 63, 64, 65, 99}, first and last node without in-edges, N odd and 3 mod 4) are
# pinned on the host by tests/test_score_graph_host.py
SCORE_GRAPH_SPECS = [(1, "chain"), (2, "chain"), (8, "hub"), (9, "hub"), (10, "hub"), (64, "hub"), (65, "hub"), (66, "hub"),
                     (100, "hub"), (17, "random"), (3, "chain"), (1, "chain"), (1, "chain")]
SCORE_GRAPH_SEED = 3


# batches of the CFConv size tests (tests/test_gpu_cfconv_sizes.py; graphs, references and tolerances in tests/cfconv_cases.py);
# tests/test_cfconv_sizes_host.py pins their node / edge counts, in- and out-degrees and chunk offsets on the host
CFCONV_PAIR_SPECS = [(1, "chain"), (33, "hub"), (2, "chain"), (33, "random"), (21, "random"), (3, "chain"), (31, "dense"),
                     (32, "random"), (20, "hub"), (1, "chain")]
CFCONV_PAIR_SEED = 5               # N_max = 33: the pair form applies; radius graph symmetric, in-degrees up to 32
CFCONV_CAP_SPECS = [(34, "hub"), (40, "random"), (65, "chain"), (1, "chain"), (33, "hub"), (7, "random")]
CFCONV_CAP_SEED = 6                # N_max = 65: the 32-neighbour cap binds; asymmetric graph, by-source rows up to 64


def loss_specs(n_max):
    """Ragged 3D->2D batch: n_max- (or 32-), 21-, 17-, 2- and 1-atom molecules, a dense n_max-atom molecule and a hub whose atom
    n_max - 3 (row >= 20) is bondless."""
    return [(n_max, "random"), (21, "random"), (17, "random"), (2, "chain"), (1, "chain"), (n_max, "dense"),
            (n_max - 1, "hub", (n_max - 3,))]
