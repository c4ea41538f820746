"""Host mirror of the in-kernel counter generator (csrc/msde_common.h: msde_mix64 / msde_uniform / msde_randn) and of the
way every kernel that draws its own randomness maps its arguments to (seed', index) pairs.  NumPy only.

The generator is splitmix64 used as a counter generator: draw `idx` of seed `s` finalises the 64-bit COUNTER
s + GOLDEN * (idx + 1).  Two draws are the same draw exactly when their counters are equal, so "do two streams overlap" is
a set intersection of `counters()` values (tests/test_rng_streams_host.py), not a statistical question; and "which draw
lands on which element" is a comparison with `Stream.randn()` / `.uniform()` (tests/test_gpu_rng_streams.py).

All integer arithmetic is modulo 2^64 and vectorised.  The normal draw is Box-Muller as msde_randn writes it, evaluated in
float64 (the reference) and in float32 (only to size the tolerance, `randn_tol`)."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15            # msde_common.h:107, the increment of the counter
FNV = 0x100000001B3                    # seed' = seed + seed_dev[0] * FNV wherever a kernel takes a device counter
TIME_XOR = 0x7157EEDC0FFEE             # pointwise.hip ve_perturb_rng_kernel / dense_head.hip dense_prepare_kernel: time-step stream
CLASS_XOR = 0xA5A5A5A5DEADBEEF         # dense_head.hip dense_prepare_kernel: atom-class noise
FFN_XOR = 0x46464E                     # geom3d/sde_2d_to_3d.py GATLayer.forward: feed-forward dropout of a layer seed
RANDPERM_MIX = 0xD1B54A32D192ED03      # pointwise.hip randperm_kernel: permutation number `which`
NEXT_SEED_MIX = 0x9E3779B1             # geom3d/nn.py DeviceNoise.next_seed / randperm / randperm_pair
PC_NMAX = 32                           # dense_pc.hip: pair (i, j) of a molecule is element i * 32 + j
_M64 = (1 << 64) - 1


def u64(x):
    """Python ints (any sign or size), lists or arrays -> uint64 modulo 2^64."""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return x
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & _M64)
    a = np.asarray(x)
    if a.dtype == object or a.dtype.kind not in "iu":
        return np.array([int(v) & _M64 for v in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)
    return a.astype(np.int64).astype(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)


def _wrap(f):
    def g(*a, **k):
        with np.errstate(over="ignore"):
            return f(*a, **k)
    g.__name__, g.__doc__ = f.__name__, f.__doc__
    return g


@_wrap
def counters(seed, idx):
    """seed + GOLDEN * (idx + 1): the value msde_mix64 finalises (msde_common.h:107)."""
    return u64(seed) + np.uint64(GOLDEN) * (u64(idx) + np.uint64(1))


@_wrap
def pc_mix(z):
    """The splitmix64 finaliser (dense_pc.hip:27-31 pc_mix; msde_common.h:108-110)."""
    z = u64(z)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mix64(seed, idx):
    """msde_mix64 (msde_common.h:106-111)."""
    return pc_mix(counters(seed, idx))


def uniform24(seed, idx):
    """The 24 random bits of msde_uniform as an integer in [0, 2^24)."""
    return (mix64(seed, idx) >> np.uint64(40)).astype(np.int64)


def uniform(seed, idx):
    """msde_uniform (msde_common.h:112-114): float32 in [0, 1), exact."""
    return uniform24(seed, idx).astype(np.float32) * np.float32(1.0 / 16777216.0)


def randn(seed, idx, dtype=np.float64):
    """msde_randn (msde_common.h:117-121): Box-Muller on uniforms 2 idx and 2 idx + 1, u1 clamped to 2^-24.  float64: the
    formula as written, in double; float32: every operation rounded to float32 as the kernel's are."""
    idx = u64(idx)
    with np.errstate(over="ignore"):
        i0 = idx * np.uint64(2)
    u1, u2 = uniform(seed, i0), uniform(seed, i0 + np.uint64(1))
    u1 = np.maximum(u1, np.float32(2.0 ** -24))
    if np.dtype(dtype) == np.float32:
        r = np.sqrt(np.float32(-2.0) * np.log(u1, dtype=np.float32), dtype=np.float32)
        return r * np.cos(np.float32(6.283185307179586) * u2, dtype=np.float32)
    u1, u2 = u1.astype(np.float64), u2.astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def measure_randn_tol(seed=1234, count=1 << 20):
    """(tolerance, largest |float32 mirror - float64 mirror|) over the first `count` normal draws of `seed`: the tolerance of a
    device draw against the float64 mirror is 8 x that difference (the device's logf / cosf may sit a few ulp from NumPy's);
    a wrong index or seed shows as an O(1) difference."""
    i = np.arange(count, dtype=np.uint64)
    d = float(np.abs(randn(seed, i, np.float32).astype(np.float64) - randn(seed, i, np.float64)).max())
    return 8.0 * d, d


class Stream:
    """The draws one kernel makes from one seed: `seed` (scalar or broadcastable array) and `idx` (array, the kernel's element
    shape), normal (two uniforms per element) or uniform (one)."""

    def __init__(self, seed, idx, normal, repeats=False):
        self.seed, self.idx, self.normal = u64(seed), u64(idx), bool(normal)
        self.repeats = repeats          # True: elements share draws by design (the antithetic time steps)

    def counters(self):
        """Every 64-bit counter the stream consumes, flat."""
        if not self.normal:
            return np.asarray(counters(self.seed, self.idx)).reshape(-1)
        with np.errstate(over="ignore"):
            i0 = self.idx * np.uint64(2)
        return np.concatenate([np.asarray(counters(self.seed, i0)).reshape(-1),
                               np.asarray(counters(self.seed, i0 + np.uint64(1))).reshape(-1)])

    def randn(self, dtype=np.float64):
        assert self.normal
        return randn(self.seed, self.idx, dtype)

    def uniform(self):
        assert not self.normal
        return uniform(self.seed, self.idx)

    def keep(self, p):
        """Dropout keep mask: msde_uniform >= p compared in float32, as the kernels compare."""
        return self.uniform() >= np.float32(p)


def dev_seed(seed, ctr=None):
    """seed' = seed + ctr * FNV (`if (seed_dev) seed += seed_dev[0] * 0x100000001B3ull`, e.g. pointwise.hip:48); ctr None: the
    kernel got no device counter."""
    s = int(seed) & _M64
    return s if ctr is None else (s + int(ctr) * FNV) & _M64


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])


# ---------------------------------------------------------------------------------------------- time steps
def time_stream(seed, ctr, B):
    """pointwise.hip:203 / dense_head.hip:74: one uniform per antithetic pair, index b (b < H) or b - H, H = B / 2 + 1, on
    seed' ^ TIME_XOR."""
    H = B // 2 + 1
    b = np.arange(B)
    return Stream(dev_seed(seed, ctr) ^ TIME_XOR, np.where(b < H, b, b - H), False, repeats=True)


def time_steps(seed, ctr, B, T):
    """Integer time step of every molecule (pointwise.hip:203-206, dense_head.hip:74-77): d0 = int(float32(u) * float32(T))
    clamped to T - 1; ts = d0 for b < H, T - d0 - 1 after that."""
    u = time_stream(seed, ctr, B).uniform()
    d0 = np.minimum((u * np.float32(T)).astype(np.int64), T - 1)
    return np.where(np.arange(B) < B // 2 + 1, d0, T - d0 - 1)


# ---------------------------------------------------------------------------------------------- training-step kernels
def ve_perturb_streams(seed, ctr, sizes):
    """msde_ve_perturb_rng (pointwise.hip:193-217): noise of coordinate c of atom i = normal draw 3 i + c of seed' (:213);
    the time-step uniforms (:203)."""
    N = int(np.sum(sizes))
    return {"noise": Stream(dev_seed(seed, ctr), np.arange(3 * N).reshape(N, 3), True),
            "time": time_stream(seed, ctr, len(sizes))}


def dense_prepare_streams(seed, ctr, sizes, ncls):
    """msde_dense_prepare with device draws (dense_head.hip:113-153).  "pair": one normal draw per unordered pair lo < hi of
    molecule b at index q0 + lo * n + hi (:120), flat over molecules in (lo, hi) order -- `pair_index` gives (b, lo, hi);
    "cls": class c of atom a0 + i at index (a0 + i) * ncls + c on seed' ^ CLASS_XOR (:139,146), shape [N, ncls]; "time"."""
    s = dev_seed(seed, ctr)
    N = int(np.sum(sizes))
    b, lo, hi = pair_index(sizes)
    n = np.asarray(sizes, dtype=np.int64)[b]
    q0 = _ptr(np.asarray(sizes, dtype=np.int64) ** 2)[b]
    return {"pair": Stream(s, q0 + lo * n + hi, True),
            "cls": Stream(s ^ CLASS_XOR, np.arange(N * ncls).reshape(N, ncls), True),
            "time": time_stream(seed, ctr, len(sizes))}


def pair_index(sizes):
    """(b, lo, hi) of every unordered atom pair lo < hi, molecules in order."""
    out = [(b, i, j) for b, n in enumerate(sizes) for i in range(n) for j in range(i + 1, n)]
    a = np.asarray(out, dtype=np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def sym_from_pairs(values, sizes, flags=None):
    """Ragged symmetric pair vector [sum n^2] (molecule b at q0 + i * n + j) from one value per unordered pair: both triangles
    get the pair's value, the diagonal 0, masked by flags[i] * flags[j] (flags: per atom, batch order)."""
    b, lo, hi = pair_index(sizes)
    sizes = np.asarray(sizes, dtype=np.int64)
    a0, q0 = _ptr(sizes), _ptr(sizes ** 2)
    out = np.zeros(int(q0[-1]), dtype=np.asarray(values).dtype)
    m = np.ones(len(b)) if flags is None else np.asarray(flags)[a0[b] + lo] * np.asarray(flags)[a0[b] + hi]
    v = np.asarray(values) * m
    out[q0[b] + lo * sizes[b] + hi] = v
    out[q0[b] + hi * sizes[b] + lo] = v
    return out


def silu_dropout_stream(seed, ctr, n):
    """msde_silu_dropout_fwd / _bwd (pointwise.hip:48-53, :62-68): uniform of the flat element index."""
    return Stream(dev_seed(seed, ctr), np.arange(n), False)


def gat_tail_stream(seed, ctr, rows, D=32):
    """msde_gat_tail (gat_tail.hip:129,135,149 and :180,229): uniform of off + j = row * D + column, D = 32."""
    return Stream(dev_seed(seed, ctr), np.arange(rows * D).reshape(rows, D), False)


def attention_dropout_stream(seed, ctr, E, H):
    """Attention dropout of a GAT layer (sde2d3d.hip:108,177: uniform of edge * H + head)."""
    return Stream(dev_seed(seed, ctr), np.arange(E * H).reshape(E, H), False)


def layer_seed(seed_base, calls, k):
    """geom3d/sde_2d_to_3d.py:170: (seed_base + calls) * 16 + 4 * module + conv = ... + k."""
    return ((int(seed_base) + int(calls)) * 16 + int(k)) & _M64


def next_seed(seed, calls):
    """geom3d/nn.py:262-264 DeviceNoise.next_seed after `calls` calls (also the seed of its randperm launches, :254,275)."""
    return (int(seed) + NEXT_SEED_MIX * int(calls)) & _M64


def dense_head_seed(seed, calls):
    """geom3d/sde_3d_to_2d.py:325: the prepare kernel's seed of the `calls`-th draw of a DeviceNoise."""
    return (int(seed) * NEXT_SEED_MIX + 0x3D2D * int(calls)) & _M64


def randperm_stream(seed, ctr, which, n):
    """msde_randperm (pointwise.hip:244-252): key i of permutation `which` finalises counter i of seed' + RANDPERM_MIX * which."""
    return Stream((dev_seed(seed, ctr) + RANDPERM_MIX * int(which)) & _M64, np.arange(n), False)


def randperm(seed, ctr, which, n, ncap=None):
    """out[i] of msde_randperm: the rank of key (mix & ~0xFFF) | i among the n keys (pointwise.hip:252-269); entries from n to
    ncap (a row bound below the capacity) map to themselves (:270)."""
    st = randperm_stream(seed, ctr, which, n)
    key = (mix64(st.seed, st.idx) & np.uint64(~0xFFF & _M64)) | st.idx
    rank = np.empty(n, dtype=np.int64)
    rank[np.argsort(key, kind="stable")] = np.arange(n)
    return np.concatenate([rank, np.arange(n, n if ncap is None else ncap)])


# ---------------------------------------------------------------------------------------------- 2D->3D sampler
def pc_draw_stream(seed, row, stream, n3):
    """pc_draw (pointwise.hip:730-732): element i of the corrector (stream 0) or predictor (stream 1) noise of iteration `row`
    is msde_randn(msde_mix64(seed, 2 * row + stream), i).  The grouped kernels call it with seed = group_seed[g] and i counted
    from the group's first coordinate (:837,852,879)."""
    return Stream(mix64(seed, 2 * int(row) + int(stream)), np.arange(n3), True)


def sampler_group_seed(noise_seed, molecule_index):
    """moleculesde_amd.sampler.group_seed: output `molecule_index` of the splitmix64 stream starting at noise_seed."""
    return int(mix64(noise_seed, molecule_index))


# ---------------------------------------------------------------------------------------------- 3D->2D sampler
def pc_noise_seed(seed, row, draw, is_x):
    """pc_noise (dense_pc.hip:36-41): key = ((row + 1) << 20) | (draw << 1) | is_x, seed' = pc_mix(seed ^ pc_mix(key)); row -1:
    the initial sample; draw: the corrector's inner step, n_steps for the predictor."""
    key = ((int(row) + 1) << 20) | (int(draw) << 1) | int(is_x)
    return int(pc_mix(u64(seed) ^ pc_mix(key)))


def dense_pc_streams(seed, row, draw, sizes, ncls):
    """The draws of one (row, draw) of csrc/dense_pc.hip for a batch: "pair": unordered pair lo < hi of molecule b at index
    (b << 32) | (lo * 32 + hi) (:110,176,227,275), flat as `pair_index`; "cls": class c of atom i of molecule b at
    (b << 32) | (i * ncls + c) (:124,182,242,289), shape [N, ncls]."""
    b, lo, hi = pair_index(sizes)
    mol = np.repeat(np.arange(len(sizes)), sizes)
    local = np.arange(len(mol)) - _ptr(sizes)[mol]
    cls = (mol[:, None] << 32) | (local[:, None] * ncls + np.arange(ncls)[None, :])
    return {"pair": Stream(pc_noise_seed(seed, row, draw, 0), (b << 32) | (lo * PC_NMAX + hi), True),
            "cls": Stream(pc_noise_seed(seed, row, draw, 1), cls, True)}
