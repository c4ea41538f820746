"""Host-side pieces of the 3D->2D sampler (moleculesde_amd/sampler_3d2d.py) against tests/golden/sampler_3d2d.npz, which the
genuine reference SDE_dense classes produced: the per-step table and the raw-noise -> ragged symmetric pair vector rule."""
import numpy as np
import torch

from helpers import load_golden


def test_step_table_matches_genuine_sde_dense():
    from moleculesde_amd.geom3d.sde import VESDE, VPSDE
    from moleculesde_amd.sampler_3d2d import step_table
    g = load_golden("sampler_3d2d.npz")
    for tag, cls in (("ve", VESDE), ("vp", VPSDE)):
        lo, hi = (float(v) for v in g[f"{tag}.range"])
        k, par = step_table(cls(lo, hi, 1000), 1000, float(g["eps"]))
        assert np.array_equal(k.numpy(), g[f"{tag}.table.k"].astype(np.int64)), tag
        ref = g[f"{tag}.table.par"].astype(np.float64)
        err = np.abs(par.numpy() - ref) / np.maximum(np.abs(ref), 1e-30)
        # std, alpha, fa: a few ulps -- torch.exp / pow take different vector paths on different host CPUs (up to 8e-7 seen)
        assert err[:, [0, 2, 3]].max() <= 2e-6, (tag, float(err[:, [0, 2, 3]].max()))
        # G = sqrt(sigma_k^2 - sigma_{k-1}^2) (VE) cancels: an ulp of sigma becomes (sigma / G)^2 ulps of G
        amp = np.maximum(1.0, (ref[:, 0] / ref[:, 1]) ** 2) if tag == "ve" else 1.0
        assert (err[:, 1] / amp).max() <= 2e-6, (tag, float((err[:, 1] / amp).max()))


def test_ragged_pair_noise_has_gen_noise_semantics():
    from moleculesde_amd.sampler_3d2d import ragged_pair_noise, ragged_pairs, sym_noise
    g = load_golden("sampler_3d2d.npz")
    flags = torch.from_numpy(g["flags"])
    sizes = [int(s) for s in g["sizes"]]
    raw = torch.from_numpy(g["noise.adj_init"]).float()
    # gen_noise(sym=True): triu(1), plus its transpose, masked -- written out element by element
    B, Nm = flags.shape
    ref = torch.zeros(B, Nm, Nm)
    for b in range(B):
        for i in range(Nm):
            for j in range(Nm):
                if i != j:
                    ref[b, i, j] = raw[b, min(i, j), max(i, j)] * flags[b, i] * flags[b, j]
    got = ragged_pair_noise(raw, flags, sizes)
    assert torch.equal(got, ragged_pairs(ref, sizes))
    assert torch.equal(sym_noise(raw, flags), ref)
    assert got.numel() == sum(n * n for n in sizes)
    # symmetric bitwise, zero diagonal, the bond-less atom's row and column zero
    a = ref[2, :7, :7]
    assert torch.equal(a, a.T) and not a.diagonal().any() and not a[3].any() and not a[:, 3].any()
