"""Molecules of the molecule-store tests (tests/test_dataset_host.py, tests/test_gpu_dataset.py): synthetic.make_molecule
draws of chosen sizes, each shifted off its centre by about 10 Angstrom so that the centring has work."""
import numpy as np
import torch

from moleculesde_amd.batch import MolData, extend_graph_index
from moleculesde_amd.synthetic import make_molecule


def off_centre_molecules(sizes, seed=0, shift=10.0):
    rng = np.random.default_rng(seed)
    mols = []
    for n in sizes:
        m = make_molecule(rng, int(n))
        m.positions = m.positions + torch.from_numpy(rng.normal(0.0, shift, size=3).astype(np.float32))[None]
        mols.append(m)
    return mols


def path_molecule(n):
    """The path graph 0-1-...-(n-1), both directions (test_extend_graph_path_graph_known_answer)."""
    src = list(range(n - 1)) + list(range(1, n))
    dst = list(range(1, n)) + list(range(n - 1))
    ei = torch.tensor([src, dst], dtype=torch.long)
    d = MolData(x=torch.zeros(n, 9, dtype=torch.long), edge_index=ei, edge_attr=torch.zeros(ei.size(1), 3, dtype=torch.long),
                positions=torch.arange(n * 3, dtype=torch.float32).view(n, 3))
    d.extended_edge_index = extend_graph_index(ei, n)
    return d


def same_molecule(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype
               for k in ("x", "edge_index", "edge_attr", "positions"))


def capturable_noise(G, dev, seed=77):
    """The noise of tests/test_gpu_plan.py::_capturable_noise(fixed_calls=True): position noise / time steps from fixed device
    tensors (padding independent, capturable), contrastive permutations from the device kernel with the host-side draw
    counter kept out of the seed, so that graphs captured at different times draw alike."""
    class Noise(G.DeviceNoise):
        def __init__(self):
            super().__init__(seed=seed)
            g = torch.Generator().manual_seed(5)
            self.big = torch.randn(8192, 3, generator=g).to(dev)
            self.ints = torch.randint(0, 1000, (4096,), generator=g).to(dev)

        def randn_like(self, x):
            assert x.dim() == 2 and x.size(1) == 3
            return self.big[:x.size(0)].clone()

        def randint(self, high, size, device):
            return self.ints[:size[0]].clone()

        def randperm_pair(self, n, device):
            self.calls = 0
            return super().randperm_pair(n, device)
    return Noise()
