// dense_pc.hip — the 3D->2D reverse-SDE predictor-corrector sampler (node_adj_PC_generation,
// pretrain_MoleculeSDE_inference_3D_to_2D_VE_VP.py:96-262, as intended: DESIGN §7.1) on the RAGGED layout of
// csrc/dense_head.hip: atoms in batch order, the pairs of molecule b at rows pair_ptr[b] + i*n_b + j.
//
// State: x [N, MSDE_DENSE_XP_LD] (atom-class scores, the rows embedding_X reads), adj [P] (exactly symmetric: every pair
// update computes ONE value from (min(i,j), max(i,j)) and writes both entries, because dense_edge_layer_fwd assumes
// symmetric input channels), x_mean / adj_mean, and the inputs of the next score evaluation: AC[:, 0:2] = (adj, adj^2)
// (pow_tensor, c_init = 2) and XC[:, 0:F] = embedding_3D(h) + both biases (the cached block embedding_X(x) is accumulated
// onto).
//
// Kernels (one workgroup of 256 threads per molecule, n_b <= 32):
//   dense_pc_init       initial state (prior_sampling_sym / prior_sampling, masked)
//   dense_pc_stats      corrector scores from the score networks' last layers (Linear(F2, 1) of the pair MLP folded in,
//                       -1/std, off-diagonal and flag masks) and per-molecule norms of the scores and of all n_steps noises
//   dense_pc_corrector  batch means of those norms (every workgroup reads the B partials in the same fixed order: no
//                       atomics, no grid barrier), then the n_steps Langevin steps on the stale score (:213-262)
//   dense_pc_predictor  reverse-diffusion step RSDE.discretize (SDE_dense.py:97-105) with its score computed inline
// Per-step scalars par[S][4] = {std(t_k), G(t_k), alpha_k, drift factor} are tabulated by the caller; the device counters
// step[0] (read by stats / corrector, written by the predictor) and step[1] (written by the corrector, read by the
// predictor) give the row, so that no kernel reads a counter another workgroup of the same launch writes.
#include "msde_common.h"

#define PC_NMAX 32
#define PC_AC MSDE_DENSE_AC_LD
#define PC_XP MSDE_DENSE_XP_LD

__device__ __forceinline__ unsigned long long pc_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Noise of draw `draw` of iteration `row` (row -1: the initial sample), molecule b, element `idx` (a pair: lo * 32 + hi;
// an atom class: i * ncls + c).  Injected: the reference's raw padded draw `inj[off]`; else the counter generator keyed by
// (seed, iteration, draw, adj / x, molecule, element).
__device__ __forceinline__ float pc_noise(const float* __restrict__ inj, size_t off, unsigned long long seed, long long row,
                                          int draw, int is_x, int b, int idx) {
  if (inj) return inj[off];
  const unsigned long long key = ((unsigned long long)(row + 1) << 20) | ((unsigned long long)draw << 1) | (unsigned long long)is_x;
  return msde_randn(pc_mix(seed ^ pc_mix(key)), ((unsigned long long)b << 32) | (unsigned long long)idx);
}

__device__ __forceinline__ float pc_block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);       // the same order in every thread and every launch
}

__device__ __forceinline__ long long pc_row(long long r, int S) { return r < 0 ? 0 : (r >= S ? S - 1 : r); }

// s_p = G2[p] . w + bias: the last Linear(F2, 1) of the edge network's final pair MLP (F2 % 4 == 0: G2 rows read as float4)
__device__ __forceinline__ float pc_pair_net(const float* __restrict__ G2, int F2, const float* __restrict__ w2, float b2,
                                             size_t q) {
  const float4* g = reinterpret_cast<const float4*>(G2 + q * F2);
  float v = 0.f;
  for (int k = 0; k < F2 / 4; ++k) {       // (w may sit at any offset of a flat parameter buffer: scalar reads)
    const float4 a = g[k];
    v = fmaf(a.x, w2[4 * k], v); v = fmaf(a.y, w2[4 * k + 1], v); v = fmaf(a.z, w2[4 * k + 2], v); v = fmaf(a.w, w2[4 * k + 3], v);
  }
  return v + b2;
}

// offsets of the injected draws: corrector [iters][n_steps][B][Nm][*], predictor / initial [iters][B][Nm][*]
__device__ __forceinline__ size_t pc_off_c(const msde_dense_pc_params& p, long long it, int s, int b, int i, int j, int w) {
  return ((((size_t)it * p.n_steps + s) * p.B + b) * p.Nm + i) * (size_t)w + j;
}
__device__ __forceinline__ size_t pc_off_p(const msde_dense_pc_params& p, long long it, int b, int i, int j, int w) {
  return (((size_t)it * p.B + b) * p.Nm + i) * (size_t)w + j;
}

// adj^2 of the molecule's new adjacency (in `pa`) and the two channels of the next score evaluation; the diagonal and
// the upper triangle are computed, the lower one mirrored (bitwise symmetric)
__device__ __forceinline__ void pc_write_ac(const msde_dense_pc_params& p, float (*pa)[PC_NMAX + 1], int n, int q0) {
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    float s2 = 0.f;
    for (int k = 0; k < n; ++k) s2 = fmaf(pa[i][k], pa[k][j], s2);
    float* r0 = p.AC + (size_t)(q0 + i * n + j) * PC_AC;
    float* r1 = p.AC + (size_t)(q0 + j * n + i) * PC_AC;
    r0[0] = pa[i][j]; r0[1] = s2;
    r1[0] = pa[i][j]; r1[1] = s2;
  }
}

__device__ __forceinline__ void pc_reset_embedding(const msde_dense_pc_params& p, int a0, int n) {
  for (int e = threadIdx.x; e < n * p.F; e += blockDim.x) {
    const int i = e / p.F, c = e - i * p.F;
    p.XC[(size_t)(a0 + i) * p.ldxc + c] = p.E3[(size_t)(a0 + i) * p.F + c];
  }
}

// ================================================================================================ initial sample
// adj = mask(triu(z, 1) + triu(z, 1)^T) (prior_sampling_sym, SDE_dense.py:148-150) or a caller's symmetric matrix
// (adj_given, masked); x = mask(z) (prior_sampling, :120,125)
__global__ void __launch_bounds__(256) dense_pc_init_kernel(msde_dense_pc_params p, const float* __restrict__ adj_given) {
  __shared__ float pa[PC_NMAX][PC_NMAX + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  if (n > PC_NMAX || n > p.Nm) return;
  if (b == 0 && tid == 0 && p.step) { p.step[0] = 0; p.step[1] = 0; }
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    const float m = p.flags[a0 + i] * p.flags[a0 + j];
    float a;
    if (adj_given) a = adj_given[((size_t)b * p.Nm + i) * p.Nm + j];
    else a = i < j ? pc_noise(p.nz_init_adj, pc_off_p(p, 0, b, i, j, p.Nm), p.seed, -1, 0, 0, b, i * PC_NMAX + j) : 0.f;
    a *= m;
    pa[i][j] = a; pa[j][i] = a;
    p.adj[q0 + i * n + j] = a; p.adj[q0 + j * n + i] = a;
    p.adj_mean[q0 + i * n + j] = a; p.adj_mean[q0 + j * n + i] = a;
  }
  for (int e = tid; e < n * n; e += 256) {
    float* r = p.AC + (size_t)(q0 + e) * PC_AC;
    r[PC_AC - 2] = 0.f; r[PC_AC - 1] = 0.f;
  }
  for (int e = tid; e < n * PC_XP; e += 256) {
    const int i = e / PC_XP, c = e - i * PC_XP;
    float v = 0.f;
    if (c < p.ncls)
      v = pc_noise(p.nz_init_x, pc_off_p(p, 0, b, i, c, p.ncls), p.seed, -1, 0, 1, b, i * p.ncls + c) * p.flags[a0 + i];
    p.x[(size_t)(a0 + i) * PC_XP + c] = v;
    p.x_mean[(size_t)(a0 + i) * PC_XP + c] = v;
  }
  pc_reset_embedding(p, a0, n);
  __syncthreads();
  pc_write_ac(p, pa, n, q0);
}

// ================================================================================================ corrector
// part[b][0..1] = ||score_adj_b||, ||score_x_b||; part[b][2 + 2 s], [3 + 2 s] = ||z_adj||, ||z_x|| of inner step s (norms
// over every entry of the molecule's padded block: the masked entries are 0).  score_adj [P] (symmetric), score_x [N, XP].
__global__ void __launch_bounds__(256)
dense_pc_stats_kernel(msde_dense_pc_params p, const float* __restrict__ G2, int F2, const float* __restrict__ w2,
                      const float* __restrict__ b2, const float* __restrict__ OUT) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  const int K = 2 + 2 * p.n_steps;
  float* part = p.part + (size_t)b * K;
  if (n > PC_NMAX || n > p.Nm) return;
  const long long row = pc_row(p.step ? p.step[0] : 0, p.S);
  const long long it = min(row, (long long)p.iters - 1);
  const float inv = 1.f / p.par[4 * row], bias = b2[0];
  float sa = 0.f, sx = 0.f;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    float s = 0.f;
    if (i < j) {
      const float m = p.flags[a0 + i] * p.flags[a0 + j];
      s = -pc_pair_net(G2, F2, w2, bias, (size_t)(q0 + e)) * m * inv;
    }
    p.score_adj[q0 + i * n + j] = s;
    p.score_adj[q0 + j * n + i] = s;
    sa += (i < j ? 2.f : 1.f) * s * s;
  }
  for (int e = tid; e < n * p.ncls; e += 256) {
    const int i = e / p.ncls, c = e - i * p.ncls;
    const size_t o = (size_t)(a0 + i) * PC_XP + c;
    const float s = -OUT[o] * p.flags[a0 + i] * inv;
    p.score_x[o] = s;
    sx += s * s;
  }
  sa = pc_block_sum(sa, red);
  sx = pc_block_sum(sx, red);
  if (tid == 0) { part[0] = sqrtf(sa); part[1] = sqrtf(sx); }
  for (int s = 0; s < p.n_steps; ++s) {
    float za = 0.f, zx = 0.f;
    for (int e = tid; e < n * n; e += 256) {
      const int i = e / n, j = e - i * n;
      if (j <= i) continue;
      const float z = pc_noise(p.nzc_adj, pc_off_c(p, it, s, b, i, j, p.Nm), p.seed, row, s, 0, b, i * PC_NMAX + j) *
                      p.flags[a0 + i] * p.flags[a0 + j];
      za += 2.f * z * z;
    }
    for (int e = tid; e < n * p.ncls; e += 256) {
      const int i = e / p.ncls, c = e - i * p.ncls;
      const float z = pc_noise(p.nzc_x, pc_off_c(p, it, s, b, i, c, p.ncls), p.seed, row, s, 1, b, e) * p.flags[a0 + i];
      zx += z * z;
    }
    za = pc_block_sum(za, red);
    zx = pc_block_sum(zx, red);
    if (tid == 0) { part[2 + 2 * s] = sqrtf(za); part[3 + 2 * s] = sqrtf(zx); }
  }
}

#define PC_MAX_STEPS 127
// step_s = (snr mean_b||z_s|| / mean_b||score||)^2 2 alpha; x_mean = x + step_s score; x = x_mean + sqrt(2 step_s) z_s scale_eps
// for s = 0 .. n_steps-1 with the score of the input state (computed once, :226-233)
__global__ void __launch_bounds__(256) dense_pc_corrector_kernel(msde_dense_pc_params p) {
  __shared__ float pa[PC_NMAX][PC_NMAX + 1];
  __shared__ float mean[2 + 2 * PC_MAX_STEPS];
  __shared__ float stp[2 * PC_MAX_STEPS], sq[2 * PC_MAX_STEPS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  const int K = 2 + 2 * p.n_steps, ns = p.n_steps;
  const long long row = pc_row(p.step ? p.step[0] : 0, p.S);
  const long long it = min(row, (long long)p.iters - 1);
  for (int k = tid; k < K; k += 256) {          // batch means in molecule order: the same value in every workgroup
    float s = 0.f;
    for (int bb = 0; bb < p.B; ++bb) s += p.part[(size_t)bb * K + k];
    mean[k] = s / (float)p.B;
  }
  __syncthreads();
  const float alpha = p.par[4 * row + 2];
  for (int k = tid; k < 2 * ns; k += 256) {     // k = 2 s (adj) or 2 s + 1 (x)
    const float r = p.snr * mean[2 + k] / mean[k & 1];
    const float st = r * r * 2.f * alpha;
    stp[k] = st;
    sq[k] = sqrtf(st * 2.f);
  }
  __syncthreads();
  if (b == 0 && tid == 0 && p.step) p.step[1] = row + 1;
  if (n > PC_NMAX || n > p.Nm) return;
  const float seps = p.scale_eps;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    const float m = p.flags[a0 + i] * p.flags[a0 + j];
    const float g = p.score_adj[q0 + e];
    float a = p.adj[q0 + e], am = a;
    for (int s = 0; s < ns; ++s) {
      const float z = i < j ? pc_noise(p.nzc_adj, pc_off_c(p, it, s, b, i, j, p.Nm), p.seed, row, s, 0, b, i * PC_NMAX + j) * m
                            : 0.f;
      am = a + stp[2 * s] * g;
      a = am + sq[2 * s] * z * seps;
    }
    pa[i][j] = a; pa[j][i] = a;
    p.adj[q0 + i * n + j] = a; p.adj[q0 + j * n + i] = a;
    p.adj_mean[q0 + i * n + j] = am; p.adj_mean[q0 + j * n + i] = am;
  }
  for (int e = tid; e < n * p.ncls; e += 256) {
    const int i = e / p.ncls, c = e - i * p.ncls;
    const size_t o = (size_t)(a0 + i) * PC_XP + c;
    const float f = p.flags[a0 + i], g = p.score_x[o];
    float v = p.x[o], vm = v;
    for (int s = 0; s < ns; ++s) {
      const float z = pc_noise(p.nzc_x, pc_off_c(p, it, s, b, i, c, p.ncls), p.seed, row, s, 1, b, e) * f;
      vm = v + stp[2 * s + 1] * g;
      v = vm + sq[2 * s + 1] * z * seps;
    }
    p.x[o] = v;
    p.x_mean[o] = vm;
  }
  pc_reset_embedding(p, a0, n);
  __syncthreads();
  pc_write_ac(p, pa, n, q0);
}

// ================================================================================================ predictor
// x_mean = x - (f(x) - G^2 score), x = x_mean + G z; f(x) = fa x - x (VP: fa = sqrt(alpha_k); VE: fa = 1, f = 0)
__global__ void __launch_bounds__(256)
dense_pc_predictor_kernel(msde_dense_pc_params p, const float* __restrict__ G2, int F2, const float* __restrict__ w2,
                          const float* __restrict__ b2, const float* __restrict__ OUT) {
  __shared__ float pa[PC_NMAX][PC_NMAX + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  const long long row = pc_row(p.step ? p.step[1] - 1 : 0, p.S);
  const long long it = min(row, (long long)p.iters - 1);
  if (b == 0 && tid == 0 && p.step) p.step[0] = row + 1;
  if (n > PC_NMAX || n > p.Nm) return;
  const float inv = 1.f / p.par[4 * row], G = p.par[4 * row + 1], fa = p.par[4 * row + 3], bias = b2[0];
  const float g2 = G * G;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    float s = 0.f, z = 0.f;
    if (i < j) {
      const float m = p.flags[a0 + i] * p.flags[a0 + j];
      s = -pc_pair_net(G2, F2, w2, bias, (size_t)(q0 + e)) * m * inv;
      z = pc_noise(p.nzp_adj, pc_off_p(p, it, b, i, j, p.Nm), p.seed, row, p.n_steps, 0, b, i * PC_NMAX + j) * m;
    }
    const float a = p.adj[q0 + e];
    const float am = a - ((fa * a - a) - g2 * s);
    const float an = am + G * z;
    pa[i][j] = an; pa[j][i] = an;
    p.adj[q0 + i * n + j] = an; p.adj[q0 + j * n + i] = an;
    p.adj_mean[q0 + i * n + j] = am; p.adj_mean[q0 + j * n + i] = am;
  }
  for (int e = tid; e < n * p.ncls; e += 256) {
    const int i = e / p.ncls, c = e - i * p.ncls;
    const size_t o = (size_t)(a0 + i) * PC_XP + c;
    const float f = p.flags[a0 + i];
    const float s = -OUT[o] * f * inv;
    const float z = pc_noise(p.nzp_x, pc_off_p(p, it, b, i, c, p.ncls), p.seed, row, p.n_steps, 1, b, e) * f;
    const float v = p.x[o];
    const float vm = v - ((fa * v - v) - g2 * s);
    p.x[o] = vm + G * z;
    p.x_mean[o] = vm;
  }
  pc_reset_embedding(p, a0, n);
  __syncthreads();
  pc_write_ac(p, pa, n, q0);
}

// ================================================================================================ host entry points
static int pc_check(const msde_dense_pc_params* p) {
  if (!p || p->B <= 0 || !p->mol_ptr || !p->pair_ptr || !p->flags || !p->par || !p->E3 || !p->XC || !p->x || !p->adj ||
      !p->x_mean || !p->adj_mean || !p->AC || p->F <= 0 || p->ldxc < p->F || p->ncls <= 0 || p->ncls > PC_XP || p->S <= 0 ||
      p->Nm <= 0 || p->n_steps < 1)
    return MSDE_EINVAL;
  if (p->Nm > PC_NMAX || p->n_steps > PC_MAX_STEPS) return MSDE_EUNSUP;
  const bool inj = p->nzc_adj || p->nzc_x || p->nzp_adj || p->nzp_x;
  if (inj && (!p->nzc_adj || !p->nzc_x || !p->nzp_adj || !p->nzp_x || p->iters <= 0)) return MSDE_EINVAL;
  return 0;
}

static int pc_check_head(const float* G2, int F2, const float* w2, const float* b2, const float* OUT) {
  if (!G2 || !w2 || !b2 || !OUT || F2 <= 0) return MSDE_EINVAL;
  if (F2 % 4) return MSDE_EUNSUP;
  return 0;
}

extern "C" int msde_dense_pc_init(const msde_dense_pc_params* p, const float* adj_given, void* stream) {
  if (int e = pc_check(p)) return e;
  MSDE_LAUNCH(dense_pc_init_kernel, dim3(p->B), dim3(256), 0, as_stream(stream), *p, adj_given);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_dense_pc_corrector(const msde_dense_pc_params* p, const float* G2, int F2, const float* w2, const float* b2,
                                       const float* OUT, void* stream) {
  if (int e = pc_check(p)) return e;
  if (int e = pc_check_head(G2, F2, w2, b2, OUT)) return e;
  if (!p->score_adj || !p->score_x || !p->part) return MSDE_EINVAL;
  hipStream_t st = as_stream(stream);
  MSDE_LAUNCH(dense_pc_stats_kernel, dim3(p->B), dim3(256), 0, st, *p, G2, F2, w2, b2, OUT);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(dense_pc_corrector_kernel, dim3(p->B), dim3(256), 0, st, *p);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_dense_pc_predictor(const msde_dense_pc_params* p, const float* G2, int F2, const float* w2, const float* b2,
                                       const float* OUT, void* stream) {
  if (int e = pc_check(p)) return e;
  if (int e = pc_check_head(G2, F2, w2, b2, OUT)) return e;
  MSDE_LAUNCH(dense_pc_predictor_kernel, dim3(p->B), dim3(256), 0, as_stream(stream), *p, G2, F2, w2, b2, OUT);
  MSDE_CHECK_LAUNCH();
  return 0;
}
