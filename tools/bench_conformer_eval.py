"""Time the COV / MAT conformer evaluation (moleculesde_amd/conformer_eval.py) on a synthetic GEOM-shaped workload:
`--molecules` molecules of 20 to 60 atoms, `--refs` reference and `--gens` generated conformers each (default 200 x 50 x 100:
one million aligned RMSDs), all atoms, thresholds 0.5 and 1.25 A.  In ONE process, on the same inputs:
  (a) rmsd_kernels   msde_conf_rmsd_matrix (preparation + pair kernel) alone, tables and buffers already on the device;
  (b) covmat_kernel  msde_conf_cov_mat alone on that matrix;
  (c) evaluate       the whole device path from host tensors: tables, uploads, both kernels, the stats back on the host;
  (d) torch_ops      the same evaluation from torch ops on the device in fp64: per molecule centring and an einsum for the 3 x 3
                     covariances, ONE batched torch.linalg.svd over all pairs, RMSD from the singular values with the
                     determinant correction, min / mean reductions per molecule;
  (e) numpy16        the same in NumPy fp64 (batched np.linalg.svd per molecule) on a pool of 16 host threads.
(a) and (b): device events around `--launches` back-to-back launches, `--rounds` rounds after a warm-up round, median and
min / max over rounds.  (c) to (e): a host clock around calls that end in a synchronise, median and min / max over `--repeats`
calls after one warm-up call.  (d) and (e) are first run on `--probe` molecules; if that predicts more than `--budget_s` seconds
for one full call, the full call is skipped and the probe's time is reported scaled to the full pair count, marked `extrapolated`.
Also reported: the largest difference between the three RMSD matrices (on the probe molecules)."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moleculesde_amd import _lib, conformer_eval as ce  # noqa: E402
from moleculesde_amd._torchabi import _p, _stream  # noqa: E402

THRESHOLDS = (0.5, 1.25)


def workload(G, R, K, seed=0):
    """Per molecule a random walk of about 1.5 A steps; references = the molecule perturbed by 0.2 A per coordinate, generated =
    by 0.1 to 0.6 A and rigidly moved: RMSDs on both sides of the thresholds."""
    rng = np.random.default_rng(seed)
    n = rng.integers(20, 61, size=G)
    refs, gens = [], []
    for g in range(G):
        base = np.cumsum(rng.normal(size=(n[g], 3)) * 0.9, axis=0)
        refs.append((base[None] + 0.2 * rng.normal(size=(R, n[g], 3))).astype(np.float32))
        q = np.linalg.qr(rng.normal(size=(K, 3, 3)))[0]
        q[:, :, 0] *= np.linalg.det(q)[:, None]                       # proper rotations
        noise = rng.uniform(0.1, 0.6, size=(K, 1, 1)) * rng.normal(size=(K, n[g], 3))
        gens.append((np.einsum("kni,kji->knj", base[None] + noise, q) + 3.0).astype(np.float32))
    return n.tolist(), refs, gens


def svd_rmsd(xc, yc, xp):
    """[R, K] RMSD of centred fp64 conformers xc [R, n, 3], yc [K, n, 3] from the singular values of the covariances; xp = torch
    or numpy (same names)."""
    H = xp.einsum("rni,knj->rkij", xc, yc)
    U, S, Vt = xp.linalg.svd(H)
    d = xp.sign(xp.linalg.det(U) * xp.linalg.det(Vt))
    lam = S[..., 0] + S[..., 1] + d * S[..., 2]
    e = (xc * xc).sum((1, 2))[:, None] + (yc * yc).sum((1, 2))[None, :] - 2.0 * lam
    return xp.sqrt(xp.clip(e, 0.0, None) / xc.shape[1])


def numpy_eval(refs, gens, threads=16):
    def one(g):
        x, y = refs[g].astype(np.float64), gens[g].astype(np.float64)
        M = svd_rmsd(x - x.mean(1, keepdims=True), y - y.mean(1, keepdims=True), np)
        rmin, cmin = M.min(1), M.min(0)
        return M, [(rmin <= t).mean() for t in THRESHOLDS] + [(cmin <= t).mean() for t in THRESHOLDS] + [rmin.mean(), cmin.mean()]
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(one, range(len(refs))))
    return [o[0] for o in out], np.array([o[1] for o in out])


def torch_eval(refs_d, gens_d):
    """refs_d / gens_d: per molecule fp32 device tensors.  One batched SVD over every pair of every molecule."""
    xs = [r.double() - r.double().mean(1, keepdim=True) for r in refs_d]
    ys = [g.double() - g.double().mean(1, keepdim=True) for g in gens_d]
    H = torch.cat([torch.einsum("rni,knj->rkij", x, y).reshape(-1, 3, 3) for x, y in zip(xs, ys)])
    U, S, Vt = torch.linalg.svd(H)
    lam = S[:, 0] + S[:, 1] + torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt)) * S[:, 2]
    mats, stats, o = [], [], 0
    thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device=H.device)
    for x, y in zip(xs, ys):
        R, K = x.shape[0], y.shape[0]
        e = (x * x).sum((1, 2))[:, None] + (y * y).sum((1, 2))[None, :] - 2.0 * lam[o:o + R * K].view(R, K)
        M = torch.sqrt(e.clamp_min(0.0) / x.shape[1])
        o += R * K
        rmin, cmin = M.min(1).values, M.min(0).values
        stats.append(torch.cat([(rmin[None] <= thr[:, None]).double().mean(1), (cmin[None] <= thr[:, None]).double().mean(1),
                                rmin.mean()[None], cmin.mean()[None]]))
        mats.append(M)
    stats = torch.stack(stats).cpu()
    return mats, stats.numpy()


def host_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def event_ms(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def put(rec, key, ts, digits=4):
    rec[key] = round(statistics.median(ts), digits)
    rec[key + "_min_max"] = [round(min(ts), digits), round(max(ts), digits)]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default="")
    p.add_argument("--molecules", type=int, default=200)
    p.add_argument("--refs", type=int, default=50)
    p.add_argument("--gens", type=int, default=100)
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--probe", type=int, default=10)
    p.add_argument("--budget_s", type=float, default=30.0)
    a = p.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    G, R, K = a.molecules, a.refs, a.gens
    n, refs, gens = workload(G, R, K)
    pairs = G * R * K
    rec = {"what": "conformer_eval", "molecules": G, "refs": R, "gens": K, "atoms_min_max": [min(n), max(n)], "pairs": pairs,
           "thresholds": list(THRESHOLDS), "launches": a.launches, "rounds": a.rounds, "repeats": a.repeats}

    # (a), (b): the kernels alone
    ref_h = torch.from_numpy(np.concatenate([r.reshape(-1, 3) for r in refs]))
    gen_h = torch.from_numpy(np.concatenate([g.reshape(-1, 3) for g in gens]))
    ref_d, gen_d = ref_h.to(dev), gen_h.to(dev)
    plan = ce.Plan(n, [R] * G, [K] * G, dev)
    prep = torch.empty(plan.n_conf * ce.REC_DOUBLES, dtype=torch.float64, device=dev)
    rmsd = torch.empty(pairs, dtype=torch.float64, device=dev)
    thr = torch.tensor(THRESHOLDS, dtype=torch.float64).to(dev)
    cmin = torch.empty(plan.n_conf, dtype=torch.float64, device=dev)
    stats = torch.empty(G, 2 * len(THRESHOLDS) + 3, dtype=torch.float64, device=dev)
    import ctypes

    def k_rmsd():
        _lib.call("msde_conf_rmsd_matrix", _p(ref_d), _p(gen_d), _p(plan.mol), G, _p(plan.tiles), ctypes.c_longlong(plan.n_tiles),
                  _p(None), ctypes.c_longlong(plan.n_conf), _p(prep), _p(rmsd), _stream())

    def k_cov():
        _lib.call("msde_conf_cov_mat", _p(rmsd), _p(plan.mol), G, _p(thr), len(THRESHOLDS), _p(cmin), _p(stats), _stream())
    for name, fn in (("rmsd_kernels_ms", k_rmsd), ("covmat_kernel_ms", k_cov)):
        event_ms(fn, a.launches)
        put(rec, name, [event_ms(fn, a.launches) for _ in range(a.rounds)])
    rec["rmsd_kernels_pairs_per_us"] = round(pairs / (rec["rmsd_kernels_ms"] * 1e3), 1)
    rec["tiles"] = plan.n_tiles
    dev_stats = stats.cpu().numpy()
    dev_mats = [rmsd[int(plan.out_off[g]):int(plan.out_off[g + 1])].view(R, K) for g in range(G)]

    # (c) the whole device path from host tensors
    put(rec, "evaluate_ms", host_ms(lambda: ce._device_stats(ref_h, gen_h, None, n, [R] * G, [K] * G, THRESHOLDS, dev), a.repeats), 3)

    # (d), (e): probe first, then the full size if it fits the budget
    P = max(1, min(a.probe, G))
    refs_d, gens_d = [torch.from_numpy(r).to(dev) for r in refs], [torch.from_numpy(g).to(dev) for g in gens]
    rows = (("torch_ops", lambda m: torch_eval(refs_d[:m], gens_d[:m])), ("numpy16", lambda m: numpy_eval(refs[:m], gens[:m])))
    for name, fn in rows:
        probe = host_ms(lambda: fn(P), 2)
        mats, st = fn(P)
        diff = max(float(np.abs(np.asarray(torch.as_tensor(mats[g]).cpu()) - dev_mats[g].cpu().numpy()).max()) for g in range(P))
        rec[name + "_max_abs_diff_to_kernels"] = float("%.3g" % diff)
        rec[name + "_cov_entries_differing"] = int((np.abs(st[:, :4] - dev_stats[:P, :4]) > 1e-12).sum())   # a count apart: >= 0.01
        rec[name + "_mat_max_abs_diff"] = float("%.3g" % np.abs(st[:, 4:] - dev_stats[:P, 4:6]).max())
        predicted = statistics.median(probe) * G / P / 1e3
        if predicted > a.budget_s:
            rec[name + "_ms"] = round(statistics.median(probe) * G / P, 1)
            rec[name + "_extrapolated_from_molecules"] = P
        else:
            put(rec, name + "_ms", host_ms(lambda: fn(G), a.repeats), 3)
        rec[name + "_over_evaluate"] = round(rec[name + "_ms"] / rec["evaluate_ms"], 1)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
