"""The molecule store of the sub-graph masking tests (tests/test_dataset_mask_host.py, tests/test_gpu_dataset_mask.py):
synthetic.make_molecule draws of sizes 1, 2, 3, 5, 8, 13, 21, 31 and 32 (four of each), the path of 6 atoms, a molecule of 5
atoms without bonds, two disconnected triangles and a star of 7 atoms -- 40 molecules, each shifted off its centre as
tests/dataset_cases.py does."""
import numpy as np
import torch

from dataset_cases import off_centre_molecules, path_molecule
from moleculesde_amd.batch import MolData

DRAW_SIZES = [1, 2, 3, 5, 8, 13, 21, 31, 32] * 4
PATH6, BONDLESS5, TRIANGLES, STAR7 = 36, 37, 38, 39       # molecule ids in the store
B = 8


def graph_molecule(n, pairs, seed):
    """n atoms, the undirected `pairs` stored in both directions, feature codes and coordinates from a seeded generator."""
    rng = np.random.default_rng(seed)
    src = [a for a, b in pairs] + [b for a, b in pairs]
    dst = [b for a, b in pairs] + [a for a, b in pairs]
    ei = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    return MolData(x=torch.from_numpy(rng.integers(0, 2, size=(n, 9))), edge_index=ei,
                   edge_attr=torch.from_numpy(rng.integers(0, 2, size=(ei.size(1), 3))),
                   positions=torch.from_numpy(rng.normal(0.0, 1.5, size=(n, 3)).astype(np.float32)))


def mask_molecules():
    mols = off_centre_molecules(DRAW_SIZES, seed=31)
    special = [path_molecule(6), graph_molecule(5, [], 1), graph_molecule(6, [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)], 2),
               graph_molecule(7, [(0, k) for k in range(1, 7)], 3)]
    rng = np.random.default_rng(32)
    for m in special:
        m.positions = m.positions + torch.from_numpy(rng.normal(0.0, 10.0, size=3).astype(np.float32))[None]
    assert len(mols) + len(special) == 40
    return mols + special


def mask_store():
    from moleculesde_amd.dataset import MoleculeStore
    return MoleculeStore.from_molecules(mask_molecules())


def bits(keep):
    return {i for i in range(keep.bit_length()) if (keep >> i) & 1}
