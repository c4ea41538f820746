// dense_pc_grouped.hip — the 3D->2D predictor-corrector sampler of csrc/dense_pc.hip for SEVERAL test-set molecules per
// trajectory.  A GROUP is a contiguous range of the batch's molecules, [group_ptr[g], group_ptr[g + 1]): the replicas of one
// test-set molecule.  Groups share the launch, the time schedule and the step counters, and nothing else:
//   * the corrector's two mean norms run over the group's own molecules (ascending, then / (float)K_g: the arithmetic
//     dense_pc_corrector_kernel does for a batch of K_g molecules, in the same order);
//   * the counter noise of molecule b is keyed by (group_seed[g], row, draw, adj / x, b - group_ptr[g], element): group g draws
//     what the single kernels draw for that group alone with seed = group_seed[g];
//   * the predictor sets group_bad[g] = 1 when a written x_mean / adj_mean value of the group is not finite (every writer
//     stores the same 1: no atomics; never cleared after init).
// Everything else -- layout, state, the step-counter protocol (no kernel reads a counter another workgroup of the same launch
// writes), one workgroup of 256 threads per molecule, fixed-order sums, n <= 32, n_steps <= 127, F2 % 4 == 0 -- is
// dense_pc.hip's, whose kernels and entry points stay as they are; the small device helpers are repeated here so that file is
// built exactly as before.  Injected draws (nz*) keep the padded offsets with the GLOBAL molecule index.
#include "msde_common.h"

#define PCG_NMAX 32
#define PCG_AC MSDE_DENSE_AC_LD
#define PCG_XP MSDE_DENSE_XP_LD
#define PCG_MAX_STEPS 127

namespace {

__device__ __forceinline__ unsigned long long pc_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// dense_pc.hip's pc_noise: `b` is the molecule's index WITHIN ITS GROUP here, `off` the padded offset (global index)
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

__device__ __forceinline__ float pc_pair_net(const float* __restrict__ G2, int F2, const float* __restrict__ w2, float b2,
                                             size_t q) {
  const float4* g = reinterpret_cast<const float4*>(G2 + q * F2);
  float v = 0.f;
  for (int k = 0; k < F2 / 4; ++k) {
    const float4 a = g[k];
    v = fmaf(a.x, w2[4 * k], v); v = fmaf(a.y, w2[4 * k + 1], v); v = fmaf(a.z, w2[4 * k + 2], v); v = fmaf(a.w, w2[4 * k + 3], v);
  }
  return v + b2;
}

__device__ __forceinline__ size_t pc_off_c(const msde_dense_pc_params& p, long long it, int s, int b, int i, int j, int w) {
  return ((((size_t)it * p.n_steps + s) * p.B + b) * p.Nm + i) * (size_t)w + j;
}
__device__ __forceinline__ size_t pc_off_p(const msde_dense_pc_params& p, long long it, int b, int i, int j, int w) {
  return (((size_t)it * p.B + b) * p.Nm + i) * (size_t)w + j;
}

__device__ __forceinline__ void pc_write_ac(const msde_dense_pc_params& p, float (*pa)[PCG_NMAX + 1], int n, int q0) {
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    float s2 = 0.f;
    for (int k = 0; k < n; ++k) s2 = fmaf(pa[i][k], pa[k][j], s2);
    float* r0 = p.AC + (size_t)(q0 + i * n + j) * PCG_AC;
    float* r1 = p.AC + (size_t)(q0 + j * n + i) * PCG_AC;
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

// The group of molecule b: the largest g with group_ptr[g] <= b (G + 1 entries, all reads inside the table).  false when the
// table does not place b in a range inside [0, B) -- the host refuses such a table; a workgroup that sees one does nothing.
struct pcg_range { int g, g0, g1; };
__device__ __forceinline__ bool pcg_find(const msde_dense_pc_groups& gr, int B, int b, pcg_range& r) {
  int lo = 0, hi = gr.G;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gr.group_ptr[mid] <= b) lo = mid; else hi = mid;
  }
  r.g = lo; r.g0 = gr.group_ptr[lo]; r.g1 = gr.group_ptr[lo + 1];
  return r.g0 >= 0 && r.g0 <= b && b < r.g1 && r.g1 <= B;
}

}  // namespace

// ================================================================================================ initial sample
__global__ void __launch_bounds__(256)
dense_pc_init_grouped_kernel(msde_dense_pc_params p, msde_dense_pc_groups gr, const float* __restrict__ adj_given) {
  __shared__ float pa[PCG_NMAX][PCG_NMAX + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  if (b == 0 && tid == 0 && p.step) { p.step[0] = 0; p.step[1] = 0; }
  if (b == 0) for (int g = tid; g < gr.G; g += 256) gr.group_bad[g] = 0;
  pcg_range r;
  if (!pcg_find(gr, p.B, b, r) || n > PCG_NMAX || n > p.Nm) return;
  const unsigned long long seed = gr.group_seed[r.g];
  const int bl = b - r.g0;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    const float m = p.flags[a0 + i] * p.flags[a0 + j];
    float a;
    if (adj_given) a = adj_given[((size_t)b * p.Nm + i) * p.Nm + j];
    else a = i < j ? pc_noise(p.nz_init_adj, pc_off_p(p, 0, b, i, j, p.Nm), seed, -1, 0, 0, bl, i * PCG_NMAX + j) : 0.f;
    a *= m;
    pa[i][j] = a; pa[j][i] = a;
    p.adj[q0 + i * n + j] = a; p.adj[q0 + j * n + i] = a;
    p.adj_mean[q0 + i * n + j] = a; p.adj_mean[q0 + j * n + i] = a;
  }
  for (int e = tid; e < n * n; e += 256) {
    float* rr = p.AC + (size_t)(q0 + e) * PCG_AC;
    rr[PCG_AC - 2] = 0.f; rr[PCG_AC - 1] = 0.f;
  }
  for (int e = tid; e < n * PCG_XP; e += 256) {
    const int i = e / PCG_XP, c = e - i * PCG_XP;
    float v = 0.f;
    if (c < p.ncls)
      v = pc_noise(p.nz_init_x, pc_off_p(p, 0, b, i, c, p.ncls), seed, -1, 0, 1, bl, i * p.ncls + c) * p.flags[a0 + i];
    p.x[(size_t)(a0 + i) * PCG_XP + c] = v;
    p.x_mean[(size_t)(a0 + i) * PCG_XP + c] = v;
  }
  pc_reset_embedding(p, a0, n);
  __syncthreads();
  pc_write_ac(p, pa, n, q0);
}

// ================================================================================================ corrector
// part[b][...]: dense_pc_stats_kernel's per-molecule norms, with the group's seed and the molecule's index in its group
__global__ void __launch_bounds__(256)
dense_pc_stats_grouped_kernel(msde_dense_pc_params p, msde_dense_pc_groups gr, const float* __restrict__ G2, int F2,
                              const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ OUT) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  const int K = 2 + 2 * p.n_steps;
  float* part = p.part + (size_t)b * K;
  pcg_range r;
  if (!pcg_find(gr, p.B, b, r) || n > PCG_NMAX || n > p.Nm) return;
  const unsigned long long seed = gr.group_seed[r.g];
  const int bl = b - r.g0;
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
    const size_t o = (size_t)(a0 + i) * PCG_XP + c;
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
      const float z = pc_noise(p.nzc_adj, pc_off_c(p, it, s, b, i, j, p.Nm), seed, row, s, 0, bl, i * PCG_NMAX + j) *
                      p.flags[a0 + i] * p.flags[a0 + j];
      za += 2.f * z * z;
    }
    for (int e = tid; e < n * p.ncls; e += 256) {
      const int i = e / p.ncls, c = e - i * p.ncls;
      const float z = pc_noise(p.nzc_x, pc_off_c(p, it, s, b, i, c, p.ncls), seed, row, s, 1, bl, e) * p.flags[a0 + i];
      zx += z * z;
    }
    za = pc_block_sum(za, red);
    zx = pc_block_sum(zx, red);
    if (tid == 0) { part[2 + 2 * s] = sqrtf(za); part[3 + 2 * s] = sqrtf(zx); }
  }
}

// step_s = (snr mean_g||z_s|| / mean_g||score||)^2 2 alpha with the means over the workgroup's own group
__global__ void __launch_bounds__(256) dense_pc_corrector_grouped_kernel(msde_dense_pc_params p, msde_dense_pc_groups gr) {
  __shared__ float pa[PCG_NMAX][PCG_NMAX + 1];
  __shared__ float mean[2 + 2 * PCG_MAX_STEPS];
  __shared__ float stp[2 * PCG_MAX_STEPS], sq[2 * PCG_MAX_STEPS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  const int K = 2 + 2 * p.n_steps, ns = p.n_steps;
  const long long row = pc_row(p.step ? p.step[0] : 0, p.S);
  const long long it = min(row, (long long)p.iters - 1);
  if (b == 0 && tid == 0 && p.step) p.step[1] = row + 1;
  pcg_range r;
  if (!pcg_find(gr, p.B, b, r)) return;
  for (int k = tid; k < K; k += 256) {          // group means in molecule order: the same value in every workgroup of the group
    float s = 0.f;
    for (int bb = r.g0; bb < r.g1; ++bb) s += p.part[(size_t)bb * K + k];
    mean[k] = s / (float)(r.g1 - r.g0);
  }
  __syncthreads();
  const float alpha = p.par[4 * row + 2];
  for (int k = tid; k < 2 * ns; k += 256) {     // k = 2 s (adj) or 2 s + 1 (x)
    const float rr = p.snr * mean[2 + k] / mean[k & 1];
    const float st = rr * rr * 2.f * alpha;
    stp[k] = st;
    sq[k] = sqrtf(st * 2.f);
  }
  __syncthreads();
  if (n > PCG_NMAX || n > p.Nm) return;
  const unsigned long long seed = gr.group_seed[r.g];
  const int bl = b - r.g0;
  const float seps = p.scale_eps;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    const float m = p.flags[a0 + i] * p.flags[a0 + j];
    const float g = p.score_adj[q0 + e];
    float a = p.adj[q0 + e], am = a;
    for (int s = 0; s < ns; ++s) {
      const float z = i < j ? pc_noise(p.nzc_adj, pc_off_c(p, it, s, b, i, j, p.Nm), seed, row, s, 0, bl, i * PCG_NMAX + j) * m
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
    const size_t o = (size_t)(a0 + i) * PCG_XP + c;
    const float f = p.flags[a0 + i], g = p.score_x[o];
    float v = p.x[o], vm = v;
    for (int s = 0; s < ns; ++s) {
      const float z = pc_noise(p.nzc_x, pc_off_c(p, it, s, b, i, c, p.ncls), seed, row, s, 1, bl, e) * f;
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
__global__ void __launch_bounds__(256)
dense_pc_predictor_grouped_kernel(msde_dense_pc_params p, msde_dense_pc_groups gr, const float* __restrict__ G2, int F2,
                                  const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ OUT) {
  // The two updates below spell out which products are fused into their sums, the way dense_pc_predictor_kernel is compiled
  // (pair loop: fma(fa, a, -a), fma(-G^2, s, .), fma(G, z, .); class loop: separate products, then fma(G, z, .)): the
  // compiler's own choice differs between two copies of the same source line, and group g must equal the single kernel
  // bit for bit (tests/test_gpu_sampler_3d2d_grouped.py).
#pragma clang fp contract(off)
  __shared__ float pa[PCG_NMAX][PCG_NMAX + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = p.mol_ptr[b], n = p.mol_ptr[b + 1] - a0, q0 = p.pair_ptr[b];
  const long long row = pc_row(p.step ? p.step[1] - 1 : 0, p.S);
  const long long it = min(row, (long long)p.iters - 1);
  if (b == 0 && tid == 0 && p.step) p.step[0] = row + 1;
  pcg_range r;
  if (!pcg_find(gr, p.B, b, r) || n > PCG_NMAX || n > p.Nm) return;
  const unsigned long long seed = gr.group_seed[r.g];
  const int bl = b - r.g0;
  const float inv = 1.f / p.par[4 * row], G = p.par[4 * row + 1], fa = p.par[4 * row + 3], bias = b2[0];
  const float g2 = G * G;
  bool bad = false;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e - i * n;
    if (j < i) continue;
    float s = 0.f, z = 0.f;
    if (i < j) {
      const float m = p.flags[a0 + i] * p.flags[a0 + j];
      s = -pc_pair_net(G2, F2, w2, bias, (size_t)(q0 + e)) * m * inv;
      z = pc_noise(p.nzp_adj, pc_off_p(p, it, b, i, j, p.Nm), seed, row, p.n_steps, 0, bl, i * PCG_NMAX + j) * m;
    }
    const float a = p.adj[q0 + e];
    const float am = a - fmaf(-g2, s, fmaf(fa, a, -a));
    const float an = fmaf(G, z, am);
    bad |= !isfinite(am);
    pa[i][j] = an; pa[j][i] = an;
    p.adj[q0 + i * n + j] = an; p.adj[q0 + j * n + i] = an;
    p.adj_mean[q0 + i * n + j] = am; p.adj_mean[q0 + j * n + i] = am;
  }
  for (int e = tid; e < n * p.ncls; e += 256) {
    const int i = e / p.ncls, c = e - i * p.ncls;
    const size_t o = (size_t)(a0 + i) * PCG_XP + c;
    const float f = p.flags[a0 + i];
    const float s = -OUT[o] * f * inv;
    const float z = pc_noise(p.nzp_x, pc_off_p(p, it, b, i, c, p.ncls), seed, row, p.n_steps, 1, bl, e) * f;
    const float v = p.x[o];
    const float vm = v - ((fa * v - v) - g2 * s);
    bad |= !isfinite(vm);
    p.x[o] = fmaf(G, z, vm);
    p.x_mean[o] = vm;
  }
  if (bad) gr.group_bad[r.g] = 1;      // every writer stores the same value
  pc_reset_embedding(p, a0, n);
  __syncthreads();
  pc_write_ac(p, pa, n, q0);
}

// ================================================================================================ host entry points
static int pcg_check(const msde_dense_pc_params* p, const msde_dense_pc_groups* gr) {
  if (!p || p->B <= 0 || !p->mol_ptr || !p->pair_ptr || !p->flags || !p->par || !p->E3 || !p->XC || !p->x || !p->adj ||
      !p->x_mean || !p->adj_mean || !p->AC || p->F <= 0 || p->ldxc < p->F || p->ncls <= 0 || p->ncls > PCG_XP || p->S <= 0 ||
      p->Nm <= 0 || p->n_steps < 1)
    return MSDE_EINVAL;
  if (!gr || !gr->group_ptr || !gr->group_seed || !gr->group_bad || gr->G <= 0 || gr->G > p->B) return MSDE_EINVAL;
  if (p->Nm > PCG_NMAX || p->n_steps > PCG_MAX_STEPS) return MSDE_EUNSUP;
  const bool inj = p->nzc_adj || p->nzc_x || p->nzp_adj || p->nzp_x;
  if (inj && (!p->nzc_adj || !p->nzc_x || !p->nzp_adj || !p->nzp_x || p->iters <= 0)) return MSDE_EINVAL;
  return 0;
}

static int pcg_check_head(const float* G2, int F2, const float* w2, const float* b2, const float* OUT) {
  if (!G2 || !w2 || !b2 || !OUT || F2 <= 0) return MSDE_EINVAL;
  if (F2 % 4) return MSDE_EUNSUP;
  return 0;
}

extern "C" int msde_dense_pc_init_grouped(const msde_dense_pc_params* p, const msde_dense_pc_groups* gr, const float* adj_given,
                                          void* stream) {
  if (int e = pcg_check(p, gr)) return e;
  MSDE_LAUNCH(dense_pc_init_grouped_kernel, dim3(p->B), dim3(256), 0, as_stream(stream), *p, *gr, adj_given);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_dense_pc_corrector_grouped(const msde_dense_pc_params* p, const msde_dense_pc_groups* gr, const float* G2,
                                               int F2, const float* w2, const float* b2, const float* OUT, void* stream) {
  if (int e = pcg_check(p, gr)) return e;
  if (int e = pcg_check_head(G2, F2, w2, b2, OUT)) return e;
  if (!p->score_adj || !p->score_x || !p->part) return MSDE_EINVAL;
  hipStream_t st = as_stream(stream);
  MSDE_LAUNCH(dense_pc_stats_grouped_kernel, dim3(p->B), dim3(256), 0, st, *p, *gr, G2, F2, w2, b2, OUT);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(dense_pc_corrector_grouped_kernel, dim3(p->B), dim3(256), 0, st, *p, *gr);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_dense_pc_predictor_grouped(const msde_dense_pc_params* p, const msde_dense_pc_groups* gr, const float* G2,
                                               int F2, const float* w2, const float* b2, const float* OUT, void* stream) {
  if (int e = pcg_check(p, gr)) return e;
  if (int e = pcg_check_head(G2, F2, w2, b2, OUT)) return e;
  MSDE_LAUNCH(dense_pc_predictor_grouped_kernel, dim3(p->B), dim3(256), 0, as_stream(stream), *p, *gr, G2, F2, w2, b2, OUT);
  MSDE_CHECK_LAUNCH();
  return 0;
}
