"""Write a dataset.MoleculeStore of synthetic.make_molecule molecules (PCQM4Mv2-shaped), for `pretrain --dataset_file`.
Every molecule is shifted off its centre (a few Angstrom, seeded), so that the centring of dataset_3D.py:120-122 has work.

    python tools/make_synthetic_store.py --molecules 16384 --seed 0 --out store.pt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_molecules(n_molecules, seed=0, shift=10.0, sizes=None):
    """make_molecule draws, each translated by a seeded vector of about `shift` Angstrom per axis."""
    from moleculesde_amd.synthetic import make_molecule
    rng = np.random.default_rng(seed)
    mols = []
    for i in range(n_molecules):
        m = make_molecule(rng, None if sizes is None else int(sizes[i]))
        m.positions = m.positions + torch.from_numpy(rng.normal(0.0, shift, size=3).astype(np.float32))[None]
        mols.append(m)
    return mols


def main(argv=None):
    from moleculesde_amd.dataset import MoleculeStore
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--molecules", type=int, required=True)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, required=True)
    a = p.parse_args(argv)
    store = MoleculeStore.from_molecules(synthetic_molecules(a.molecules, a.seed))
    store.save(a.out)
    print(f"{a.out}: {len(store)} molecules, {store.x.size(0)} atoms, {store.edge_index.size(1)} directed bonds, "
          f"{int(store.ext_count.sum())} extended edges")


if __name__ == "__main__":
    main()
