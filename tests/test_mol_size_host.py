"""Host-side preconditions of tests/test_gpu_mol_size.py: the molecule builder of tests/helpers.py makes molecules of the
exact atom count and extended-edge count the GPU tests claim (per-molecule Em through ES_EAL = 384 up to ES_EMAX = 992), the
host plan sees them, and the extended graph of these dense molecules is the reference's extend_graph (dataset_3D.py:12-35)
replayed on the stand-in sparse ops."""
import numpy as np
import pytest
import torch

import helpers as H


def _reference_extend_graph(ei, N):
    from oracle import ref_loader
    ref_loader.standins()
    import torch_sparse
    from torch_geometric.utils import remove_self_loops
    for _ in range(2):                     # (A + A^2 without self loops), twice: pairs within <= 4 bonds
        val = ei.new_ones((ei.size(1),), dtype=torch.float)
        idx, _ = torch_sparse.spspmm(ei, val, ei, val, N, N, N)
        idx, _ = remove_self_loops(idx, None)
        ei, _ = torch_sparse.coalesce(torch.cat([ei, idx], 1), None, N, N)
    return ei


@pytest.mark.parametrize("n", [1, 2, 17, 21, 32, 33, 40])
@pytest.mark.parametrize("pattern", ["chain", "hub", "dense", "random"])
def test_builder_sizes_positions_and_extended_graph(n, pattern):
    rng = np.random.default_rng(n * 7 + len(pattern))
    m = H.build_molecule(rng, n, pattern)
    assert m.x.shape == (n, 9) and m.positions.shape == (n, 3)
    ei = m.edge_index
    assert ei.size(1) == m.edge_attr.size(0) and (ei.size(1) == 0 or int(ei.max()) < n)
    assert torch.equal(ei[:, 0::2], ei[:, 1::2].flip(0))            # both directions, consecutive
    if n > 1:
        d = torch.cdist(m.positions.double(), m.positions.double()) + 1e9 * torch.eye(n, dtype=torch.float64)
        assert float(d.min()) >= 1.0 - 1e-6
    ext = m.extended_edge_index
    if n > 1:
        assert torch.equal(ext, _reference_extend_graph(ei, n))
    Em = ext.size(1)
    if pattern == "hub" or (pattern == "dense" and n > 1):
        assert Em == n * (n - 1)                                    # every pair within <= 2 (hub) or <= 4 (dense) bonds
    if pattern == "chain":
        assert Em == 2 * sum(max(n - k, 0) for k in range(1, 5))


def test_bondless_atom_has_no_bonds_and_zero_flag():
    from moleculesde_amd import plan as P
    b = H.build_batch(H.loss_specs(32), seed=2)
    pl = P.build_plan(b)
    dn = P.dense_plan(pl, b)
    sizes = [s[0] for s in H.loss_specs(32)]
    want = torch.zeros(len(sizes), 32)
    for i, s in enumerate(H.loss_specs(32)):
        want[i, :s[0]] = 1.0 if s[0] > 1 else 0.0                    # a lone atom has no bond either
        for a in (s[2] if len(s) > 2 else ()):
            want[i, a] = 0.0
    assert torch.equal(dn.flags, want)
    assert pl.N_max == 32 and (pl.mol_ptr[1:] - pl.mol_ptr[:-1]).tolist() == sizes


@pytest.mark.parametrize("n_max", [23, 32])
def test_loss_batches_hold_what_the_gpu_tests_claim(n_max):
    from moleculesde_amd import plan as P
    specs = H.loss_specs(n_max)
    b = H.build_batch(specs, seed=n_max)
    pl = P.build_plan(b)
    assert pl.N_max == n_max
    assert (pl.mol_ptr[1:] - pl.mol_ptr[:-1]).tolist() == [s[0] for s in specs]
    assert P.dense_plan(pl, b).N_max == n_max


def test_escore_batch_reaches_every_edge_storage_branch():
    """Per-molecule extended-edge counts straddle ES_EAL = 384 (edge features in LDS / streamed from global memory) and reach
    ES_EMAX = 992; the host plan's CSR (canonical order, by target) gives the same counts per molecule."""
    from moleculesde_amd import plan as P
    b = H.build_batch(H.ESCORE_SPECS, seed=1)
    em = H.mol_edge_counts(b)
    pl = P.build_plan(b)
    rp, mp = pl.ext.rowptr.long(), pl.mol_ptr.long()
    assert (rp[mp[1:]] - rp[mp[:-1]]).tolist() == em
    assert pl.N_max == 32 and (mp[1:] - mp[:-1]).tolist() == [s[0] for s in H.ESCORE_SPECS]
    for got, want in zip(em, H.ESCORE_EM):
        assert got == want if want is not None else got < H.ES_EAL
    assert any(H.ES_EAL - 8 <= e <= H.ES_EAL for e in em)
    assert any(e > H.ES_EAL for e in em) and H.ES_EMAX in em
