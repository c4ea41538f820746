"""2D->3D reverse-SDE predictor-corrector sampler (BASELINE.json config 4), as INTENDED by
examples/pretrain_MoleculeSDE_inference_2D_to_3D_VE_VP.py:92-212.  The script itself is broken as
shipped (missing import, undefined args, hard-coded `break` after 11 steps); this
restates the algorithm:  for t in linspace(T, eps, N):  Langevin corrector -> reverse-diffusion
predictor, each calling SDEModel2Dto3D_02.get_score on the replicated molecule batch."""
import os
import torch
from . import _lib
from . import hip as _hip_mod
from . import slabs

FUSED_PC = True     # sampler arithmetic on msde_pc_corrector / msde_pc_predictor (False: operator by operator, the reference path of the tests)


def predictor_update(sde, score_model, representation, data, pos, t, noise=None):
    """ReverseDiffusionPredictor.update_fn (:163-168)."""
    f, G = sde.reverse_discretize(score_model, pos, representation, data, t)
    noise = torch.randn_like(pos) if noise is None else noise
    x_mean = pos - f
    return x_mean + G[:, None] * noise, x_mean


def corrector_update(sde, score_model, representation, data, pos, t, snr, scale_eps, n_steps, noises=None):
    """LangevinCorrector.update_fn (:191-212): alpha = 1 for the VE SDE, alphas[timestep] for VP.  As in the script, the inner
    iterations do not feed `pos` back (App. B.2), so the score is evaluated once per call when
    n_steps == 1 and only the last pass matters otherwise."""
    alpha = sde.corrector_alpha(t) if hasattr(sde, "corrector_alpha") else torch.ones_like(t)     # VP: :198-200
    x = x_mean = pos
    for i in range(n_steps):
        grad = score_model.get_score(representation, data, pos, None, t)
        noise = torch.randn_like(pos) if noises is None else noises[i]
        grad_norm = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
        noise_norm = torch.norm(noise.reshape(noise.shape[0], -1), dim=-1).mean()
        step_size = (snr * noise_norm / grad_norm) ** 2 * 2 * alpha
        x_mean = pos + step_size[:, None] * grad
        x = x_mean + torch.sqrt(step_size * 2)[:, None] * noise * scale_eps
    return x, x_mean


@torch.no_grad()
def position_PC_generation(score_model, representation, data, num_steps=1000, snr=0.16, scale_eps=0.7,
                           n_corrector_steps=1, eps=1e-4, denoise=True, pos_init=None, use_graph=True, noise_seed=None,
                           torch_noise=False, iters_per_graph=1):
    """position_PC_generation (:92-138): returns the final coordinates [N, 3].

    The loop is latency bound (every iteration = 1 + n_corrector_steps score-network calls on a graph of
    ~10 x 14 atoms, ~150 small launches), so by default one iteration (corrector + predictor, noise drawn
    inside) is captured into a hipGraph after two eager warm-up iterations and replayed.  On the fused path (one shared
    diffusion time, one corrector step) the replay needs nothing from the host: the iteration counter and the noise live in
    the two update kernels (noise_seed: their seed; None = drawn from torch's generator), and iters_per_graph iterations
    share one graph launch.  The draw of iteration `row`, corrector (stream 0) or predictor (stream 1), flat coordinate i is
    msde_randn(msde_mix64(noise_seed, 2 * row + stream), i) (csrc/pointwise.hip pc_draw; host mirror: tests/rng_mirror.py): every
    (row, stream) has a finalised seed of its own, so no two iterations share a uniform.  torch_noise=True: the noise comes
    from torch.randn_like as in the operator path (parity tests: same generator state => same trajectory)."""
    sde = score_model.sde_pos
    n = representation.size(0)
    dev = representation.device
    pos = (torch.randn(n, 3, device=dev) if pos_init is None else pos_init.clone()).contiguous()
    timesteps = torch.linspace(sde.T, eps, num_steps, device=dev)
    vec_t = torch.ones(n, device=dev)
    x_mean = pos.clone()

    # Fused arithmetic (csrc/pointwise.hip: msde_pc_corrector / msde_pc_predictor): every atom shares the diffusion time, so
    # std(t), G(t), alpha(t) and the drift factor are tabulated ONCE for all time steps with the SDE's own methods, and each
    # half iteration is: score network -> one noise draw -> one kernel.  The operator-by-operator functions above stay the
    # reference path (tests, n_corrector_steps > 1, CPU).
    fused = (FUSED_PC and dev.type == "cuda" and n_corrector_steps == 1 and hasattr(score_model, "get_score_raw")
             and pos.dtype == torch.float32)
    if fused:
        S = num_steps
        ones = torch.ones(S, 1, device=dev)
        std_all = sde.marGINal_prob(ones, timesteps)[1]
        f_all, G_all = sde.discretize(ones, timesteps)
        alpha_all = sde.corrector_alpha(timesteps) if hasattr(sde, "corrector_alpha") else torch.ones_like(timesteps)
        par_all = torch.stack([std_all.float(), G_all.float(), alpha_all.float(), f_all[:, 0].float() + 1.0], 1).contiguous()
        # the iteration counter lives on the device (the corrector advances it) and both kernels draw their own noise from the
        # counter generator: a replayed iteration needs no host work and no random-number operator (noise_seed: one per call)
        it_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        # default seed: ONE draw from the device's torch generator per call (so torch.manual_seed / torch.cuda.manual_seed
        # govern the trajectory as they did when the noise came from torch.randn_like on the device; one host read per
        # trajectory, outside the iteration loop); an explicit noise_seed is taken modulo 2^64
        if noise_seed is not None:
            seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        else:       # (torch_noise: the kernels get their noise from torch.randn_like -- no draw, the generator is left alone)
            seed = 0 if torch_noise else int(torch.randint(0, 2 ** 62, (1,), device=dev).item())
        xc = torch.empty_like(pos)
        xm_c = torch.empty_like(pos)
        stream = _hip_mod._stream
        p_ = _hip_mod._p

    def one_step():
        if fused:
            raw = score_model.get_score_raw(representation, data, pos).contiguous()
            nz = torch.randn_like(pos) if torch_noise else None
            _lib.call("msde_pc_corrector", p_(raw), p_(pos), p_(nz), p_(par_all), p_(it_dev), seed, n, float(snr), float(scale_eps),
                      p_(xc), p_(xm_c), stream())
            raw2 = score_model.get_score_raw(representation, data, xc).contiguous()
            nz2 = torch.randn_like(pos) if torch_noise else None
            _lib.call("msde_pc_predictor", p_(raw2), p_(xc), p_(nz2), p_(par_all), p_(it_dev), seed, n, p_(pos), p_(x_mean), stream())
            return
        p, _ = corrector_update(sde, score_model, representation, data, pos, vec_t, snr, scale_eps, n_corrector_steps)
        p, m = predictor_update(sde, score_model, representation, data, p, vec_t)
        pos.copy_(p)
        x_mean.copy_(m)

    # Replay: on the fused path an iteration reads nothing from the host (counter and noise live on the device), so
    # `iters_per_graph` consecutive iterations can share ONE hipGraph; the tail that does not fill a graph replays a
    # one-iteration graph.  Measured (tools/sampler_slope.py): the loop is bound by the two score-network launches of an
    # iteration, 165-169 us per iteration for 1, 5 and 25 iterations per graph -- so the default stays 1 (cheapest capture).
    graph, graph_k, k_iters = None, None, 1
    i = 0
    while i < num_steps:
        if not fused:
            vec_t.fill_(1.0).mul_(timesteps[i])
        if use_graph and dev.type == "cuda" and graph is None and i == 2:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with slabs.no_gc(collect=False), torch.cuda.graph(graph):
                one_step()                 # capture only records; the replay below executes iteration i
            k_iters = max(1, min(int(iters_per_graph), num_steps - i)) if fused else 1
            if k_iters > 1:
                graph_k = torch.cuda.CUDAGraph()
                with slabs.no_gc(collect=False), torch.cuda.graph(graph_k):
                    for _ in range(k_iters):
                        one_step()
        if graph_k is not None and num_steps - i >= k_iters:
            graph_k.replay()
            i += k_iters
        elif graph is not None:
            graph.replay()
            i += 1
        else:
            one_step()
            i += 1
    return (x_mean if denoise else pos).clone()


# ---- many molecules per trajectory (generate_samples_from_testset, :42-89) -------------------------------------------------------
# The script runs one trajectory per test molecule (its num_repeat replicas are the whole batch), so the corrector's mean norms
# are statistics of ONE molecule.  Below, several molecules share a trajectory and every such statistic stays per GROUP (= the
# replicas of one molecule, contiguous atoms): a molecule gets the result it would get alone.
# Default chunk of generate_samples_from_testset.  Measured on one MI355X (tools/bench_sampler_testset.py,
# profiles/pr_sampler_testset_bench.jsonl; 100 synthetic molecules x 10 replicas, 1000 steps, emb 300): 16 / 25 / 32 / 50 molecules
# per launch -> 58.5 / 84.4 / 82.2 / 110.5 molecules/s (one trajectory per molecule: 6.8).  The per-molecule score kernel runs one
# workgroup per replica on 256 CUs, so with 10 replicas every 25 molecules start another round of it (65 us up to 25 molecules,
# 123 us for 32 and for 50): multiples of 25 are the efficient sizes.  Larger chunks were not measured.
MOLECULES_PER_LAUNCH = 50

_M64 = 0xFFFFFFFFFFFFFFFF


def group_seed(noise_seed, molecule_index):
    """The noise seed of one molecule: splitmix64 (Steele, Lea, Flood 2014) of noise_seed + (molecule_index + 1) * golden gamma,
    i.e. output number molecule_index of the splitmix64 stream that starts at noise_seed.  A pure function of its two arguments:
    a molecule's trajectory does not depend on how the test set is cut into launches."""
    z = (int(noise_seed) + (int(molecule_index) + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _segment_mean(v, group_index, num_groups):
    s = torch.zeros(num_groups, dtype=v.dtype, device=v.device).index_add_(0, group_index, v)
    c = torch.zeros(num_groups, dtype=v.dtype, device=v.device).index_add_(0, group_index, torch.ones_like(v))
    return s / c


def corrector_update_grouped(sde, score_model, representation, data, pos, t, snr, scale_eps, group_index, num_groups,
                             noises=None, n_steps=1):
    """corrector_update with the two mean norms taken per group (group_index [N]: the group of every atom): operator by
    operator, on any device, with anything that has get_score -- the reference of the grouped kernels and the path for
    n_corrector_steps != 1 and CPU tensors."""
    alpha = sde.corrector_alpha(t) if hasattr(sde, "corrector_alpha") else torch.ones_like(t)
    x = x_mean = pos
    for i in range(n_steps):
        grad = score_model.get_score(representation, data, pos, None, t)
        noise = torch.randn_like(pos) if noises is None else noises[i]
        grad_norm = _segment_mean(torch.norm(grad.reshape(grad.shape[0], -1), dim=-1), group_index, num_groups)
        noise_norm = _segment_mean(torch.norm(noise.reshape(noise.shape[0], -1), dim=-1), group_index, num_groups)
        # (corrector_update multiplies a 0-dim tensor into alpha, so its step size has alpha's dtype: the same here)
        step_size = ((snr * noise_norm / grad_norm) ** 2 * 2)[group_index].to(alpha.dtype) * alpha
        x_mean = pos + step_size[:, None] * grad
        x = x_mean + torch.sqrt(step_size * 2)[:, None] * noise * scale_eps
    return x, x_mean


def _check_groups(group_ptr, n, group_seeds):
    """Host-side refusal of a bad group table (the kernels index with it): returns it as a list of ints."""
    gp = [int(v) for v in (group_ptr.tolist() if isinstance(group_ptr, torch.Tensor) else group_ptr)]
    if len(gp) < 2 or gp[0] != 0 or gp[-1] != int(n):
        raise ValueError("group_ptr must run from 0 to the number of atoms (%d), got %r" % (n, gp[:1] + gp[-1:]))
    for a, b in zip(gp[:-1], gp[1:]):
        if b < a:
            raise ValueError("group_ptr is not monotone (%d after %d)" % (b, a))
        if b == a:
            raise ValueError("group_ptr holds an empty group (at atom %d)" % a)
    if group_seeds is not None and len(group_seeds) != len(gp) - 1:
        raise ValueError("group_seeds has %d entries for %d groups" % (len(group_seeds), len(gp) - 1))
    return gp


@torch.no_grad()
def position_PC_generation_grouped(score_model, representation, data, group_ptr, num_steps=1000, snr=0.16, scale_eps=0.7,
                                   n_corrector_steps=1, eps=1e-4, denoise=True, pos_init=None, use_graph=True, group_seeds=None,
                                   torch_noise=False, iters_per_graph=1):
    """position_PC_generation for G groups of atoms that share the trajectory but no statistic: group g = atoms
    [group_ptr[g], group_ptr[g + 1]) (the replicas of one molecule).  Returns (pos [N, 3], group_bad [G] int32: 1 where an
    x_mean of the group was not finite at some iteration).

    Same structure as position_PC_generation (table once, two eager warm-up iterations, capture, replay) on
    msde_pc_corrector_grouped / msde_pc_predictor_grouped; group_seeds: one noise seed per group (None: drawn from the device's
    torch generator) -- group g walks the trajectory of position_PC_generation(noise_seed=group_seeds[g]) on that group alone
    (its draws: msde_randn(msde_mix64(group_seeds[g], 2 * row + stream), coordinate counted from the group's first)).
    The operator path (CPU, n_corrector_steps != 1) draws its noise from torch's generator, as position_PC_generation's does."""
    sde = score_model.sde_pos
    n = representation.size(0)
    dev = representation.device
    gp = _check_groups(group_ptr, n, group_seeds)
    G = len(gp) - 1
    pos = (torch.randn(n, 3, device=dev) if pos_init is None else pos_init.clone()).contiguous()
    timesteps = torch.linspace(sde.T, eps, num_steps, device=dev)
    vec_t = torch.ones(n, device=dev)
    x_mean = pos.clone()
    group_bad = torch.zeros(G, dtype=torch.int32, device=dev)         # (a torch fill: the library records no memset node)

    fused = (FUSED_PC and dev.type == "cuda" and n_corrector_steps == 1 and hasattr(score_model, "get_score_raw")
             and pos.dtype == torch.float32)
    if fused:
        S = num_steps
        ones = torch.ones(S, 1, device=dev)
        std_all = sde.marGINal_prob(ones, timesteps)[1]
        f_all, G_all = sde.discretize(ones, timesteps)
        alpha_all = sde.corrector_alpha(timesteps) if hasattr(sde, "corrector_alpha") else torch.ones_like(timesteps)
        par_all = torch.stack([std_all.float(), G_all.float(), alpha_all.float(), f_all[:, 0].float() + 1.0], 1).contiguous()
        it_dev = torch.zeros(G, dtype=torch.int64, device=dev)         # one iteration counter per group (csrc/pointwise.hip)
        gp_dev = torch.tensor(gp, dtype=torch.int32, device=dev)
        max_atoms = max(b - a for a, b in zip(gp[:-1], gp[1:]))
        if group_seeds is not None:        # 64-bit patterns in an int64 tensor
            seeds_dev = torch.tensor([(int(s) & _M64) - (1 << 64) * ((int(s) & _M64) >> 63) for s in group_seeds],
                                     dtype=torch.int64, device=dev)
        else:      # ONE draw of G seeds per call from the device's torch generator (torch_noise: no draw, as position_PC_generation)
            seeds_dev = None if torch_noise else torch.randint(0, 2 ** 62, (G,), dtype=torch.int64, device=dev)
        xc = torch.empty_like(pos)
        xm_c = torch.empty_like(pos)
        stream = _hip_mod._stream
        p_ = _hip_mod._p
    else:
        group_index = torch.repeat_interleave(torch.arange(G, device=dev),
                                              torch.tensor([b - a for a, b in zip(gp[:-1], gp[1:])], device=dev))

    def one_step():
        if fused:
            raw = score_model.get_score_raw(representation, data, pos).contiguous()
            nz = torch.randn_like(pos) if torch_noise else None
            _lib.call("msde_pc_corrector_grouped", p_(raw), p_(pos), p_(nz), p_(par_all), p_(it_dev), p_(seeds_dev), p_(gp_dev), G,
                      n, max_atoms, float(snr), float(scale_eps), p_(xc), p_(xm_c), stream())
            raw2 = score_model.get_score_raw(representation, data, xc).contiguous()
            nz2 = torch.randn_like(pos) if torch_noise else None
            _lib.call("msde_pc_predictor_grouped", p_(raw2), p_(xc), p_(nz2), p_(par_all), p_(it_dev), p_(seeds_dev), p_(gp_dev), G,
                      n, p_(pos), p_(x_mean), p_(group_bad), stream())
            return
        p, _ = corrector_update_grouped(sde, score_model, representation, data, pos, vec_t, snr, scale_eps, group_index, G,
                                        n_steps=n_corrector_steps)
        p, m = predictor_update(sde, score_model, representation, data, p, vec_t)
        pos.copy_(p)
        x_mean.copy_(m)
        nonfinite = (~torch.isfinite(m)).any(dim=1).to(torch.int32)
        group_bad.copy_(torch.maximum(group_bad, torch.zeros_like(group_bad).index_add_(0, group_index, nonfinite).clamp_(max=1)))

    graph, graph_k, k_iters = None, None, 1
    i = 0
    while i < num_steps:
        if not fused:
            vec_t.fill_(1.0).mul_(timesteps[i])
        if use_graph and dev.type == "cuda" and graph is None and i == 2:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with slabs.no_gc(collect=False), torch.cuda.graph(graph):
                one_step()                 # capture only records; the replay below executes iteration i
            k_iters = max(1, min(int(iters_per_graph), num_steps - i)) if fused else 1
            if k_iters > 1:
                graph_k = torch.cuda.CUDAGraph()
                with slabs.no_gc(collect=False), torch.cuda.graph(graph_k):
                    for _ in range(k_iters):
                        one_step()
        if graph_k is not None and num_steps - i >= k_iters:
            graph_k.replay()
            i += k_iters
        elif graph is not None:
            graph.replay()
            i += 1
        else:
            one_step()
            i += 1
    return (x_mean if denoise else pos).clone(), group_bad


def repeat_data(mol, num_repeat):
    """repeat_data (:29-39) for one molecule or a list of them: the batch of num_repeat replicas of every molecule, group-major
    (all replicas of the first molecule, then the second's, ...), so a molecule's atoms are contiguous."""
    from .batch import Batch
    mols = mol if isinstance(mol, (list, tuple)) else [mol]
    return Batch.from_data_list([m for m in mols for _ in range(int(num_repeat))])


def generate_samples_from_testset(molecules, molecule_model_2D, SDE_2Dto3D_model, num_repeat=10, start=0, end=100,
                                  molecules_per_launch=None, num_steps=None, noise_seed=None, out_path=None, generator="PC",
                                  eval_epoch=None, min_sigma=0.0, **sampler_kw):
    """generate_samples_from_testset (:42-89): num_repeat conformers for every molecule of molecules[start:end] (MolData), with
    `molecules_per_launch` molecules sharing each reverse-SDE trajectory (default MOLECULES_PER_LAUNCH).  Returns the script's list
    of `return_data`: per molecule a MolData with the molecule's fields, pos_gen [num_repeat * n, 3] (CPU), num_pos_gen and
    finite (False: the trajectory left the finite numbers for this molecule; the others of its launch are not affected).

    A molecule's result is a function of (noise_seed, its index in `molecules`) only: the starting coordinates come from one
    randn call per molecule on a generator seeded by group_seed, the trajectory noise from group_seed(noise_seed, index);
    noise_seed=None draws one from torch's CPU generator.  The script's `if i >= 9: break` and its 11-iteration `break` in the
    inner loop are not reproduced.  sampler_kw goes to position_PC_generation_grouped."""
    import pickle
    from .batch import MolData
    from .geom3d.nn import prepare_batch
    molecule_model_2D.eval()
    SDE_2Dto3D_model.eval()
    dev = next(SDE_2Dto3D_model.parameters()).device
    per = int(MOLECULES_PER_LAUNCH if molecules_per_launch is None else molecules_per_launch)
    if per < 1 or num_repeat < 1:
        raise ValueError("molecules_per_launch and num_repeat must be at least 1")
    name = "2D_to_3D_{}_{}_{}_epoch_{}_min_sig_{:.3f}_repeat_{}".format(generator, start, end, eval_epoch, min_sigma, num_repeat)   # :85
    start, end = max(0, int(start)), min(int(end), len(molecules))
    steps = int(SDE_2Dto3D_model.sde_pos.N if num_steps is None else num_steps)
    if noise_seed is None:
        noise_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    records = []
    for lo in range(start, end, per):
        idx = list(range(lo, min(lo + per, end)))
        mols = [molecules[i] for i in idx]
        batch = prepare_batch(repeat_data(mols, num_repeat), dev)
        with torch.no_grad():
            rep = molecule_model_2D(batch.x, batch.edge_index, batch.edge_attr)
        gp, inits = [0], []
        for i, m in zip(idx, mols):
            g = torch.Generator().manual_seed(group_seed(group_seed(noise_seed, i), 0) >> 1)
            inits.append(torch.randn(num_repeat * m.num_nodes, 3, generator=g))          # prior_sampling (:63), one call per molecule
            gp.append(gp[-1] + num_repeat * m.num_nodes)
        pos, bad = position_PC_generation_grouped(SDE_2Dto3D_model, rep, batch, gp, num_steps=steps,
                                                  pos_init=torch.cat(inits).to(dev),
                                                  group_seeds=[group_seed(noise_seed, i) for i in idx], **sampler_kw)
        pos, bad = pos.detach().cpu(), bad.cpu().tolist()
        for k, m in enumerate(mols):
            rec = MolData(**{key: getattr(m, key).clone().detach() for key in m.keys()})
            rec.pos_gen = pos[gp[k]:gp[k + 1]].clone()                    # (num_repeat * num_node, 3), :76
            rec.num_pos_gen = torch.tensor([num_repeat], dtype=torch.long)
            rec.finite = bad[k] == 0 and bool(torch.isfinite(rec.pos_gen).all())
            records.append(rec)
    if out_path is not None:
        with open(os.path.join(out_path, name), "wb") as fout:
            pickle.dump(records, fout)
    return records
