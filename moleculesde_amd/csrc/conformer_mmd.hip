// conformer_mmd.hip — the distance-distribution metric of generated conformers: the MMD between the reference and the
// generated ensemble of a molecule over its interatomic distances, per distance ("Single"), per pair of distances ("Pair")
// and over the whole distance vector ("All").  The definition is this project's (include/msde_hip.h):
//
//   z[a, e] = |pos_a[u_e] - pos_a[v_e]|                       the conformers pooled, references first
//   L_ab    = sum over the columns e of a subset S of (z[a, e] - z[b, e])^2
//   sigma^2 = sum_{a, b} L_ab / (C^2 - C)                       additive over the columns of S
//   k(a, b) = sum_{i < num} exp(-L_ab / (sigma^2 mul^(i - num / 2)))
//   MMD(S)  = mean_{ref, ref} k + mean_{gen, gen} k - 2 mean_{ref, gen} k      (V-statistic, diagonals included)
//
// Conformers with a non-finite coordinate on an evaluated atom are left out BEFORE anything is summed: the table holds the
// remaining C' = R' + K' samples of a column contiguously (references first), so every sum below runs over exactly the
// samples it would run over had the excluded conformers never been passed, in the same order -- bitwise the same result.
//
//   (1) cm_finite_kernel   one wavefront per conformer: 1 if every coordinate of its evaluated atoms is finite.
//   (2) cm_rank_kernel     one wavefront per molecule: the position of every kept conformer among the kept ones (ballot +
//                          popcount over 64 conformers at a time), R' and K'.
//   (3) cm_table_kernel    one wavefront per kept conformer, lanes over the atom pairs: differences, squares and the root in
//                          fp64 from the fp32 coordinates; the table is fp64, column-major per molecule (leading dimension
//                          C = R + K, rows C' .. C - 1 of a column are not written and never read).
//   (4) cm_colsum_kernel   one wavefront per column: sum_{a, b} (z_a - z_b)^2 formed from the differences themselves (no
//                          sum-of-squares cancellation; identical samples give exactly 0).
//   (5) cm_items_kernel    one wavefront per work item {e} or {e, f}: see the comment above the kernel.
//   (6) cm_means_kernel    per molecule the mean of its Single and of its Pair items.
//   (7) cm_all_kernel      one workgroup per molecule: L summed over all of its columns.
// k is symmetric and k(a, a) = num exactly (exp(-0) = 1), so (5) and (7) evaluate only the pairs a < b:
//   sum_{ref, ref} k = 2 sum_{a < b in ref} k + R' num,  likewise for gen;  sum_{ref, gen} k over its R' K' pairs.
// L, sigma^2 and the exponent are fp64; the exponential is the fp32 v_exp_f32; its value enters fp64 sums.  For mul = 2 the
// scales are powers of two of each other, exp(-L / s_{i-1}) = exp(-L / s_i)^2: ONE v_exp_f32 at the widest scale and num - 1
// squarings serve all of them; any other mul (or exp_path = 1) takes num exponentials.
// No atomics anywhere; per-lane partial sums meet in an xor butterfly and per-wave sums in index order, so an item's value
// depends on its own columns, R', K' and the kernel parameters alone.
#include "msde_common.h"

#include <math.h>

#define CM_MOL 8                   // int64 per molecule: n, R, K, ref_row0, gen_row0, z_off, atom_off, conf_off
#define CM_MAX_POOLED 1024         // largest R + K of a molecule: two fp64 columns per wave are staged in LDS
#define CM_WAVES 2                 // items (wavefronts) per workgroup of cm_items_kernel: 2 x 2 x 1024 x 8 B = 32 KiB at most
#define CM_MAX_KERNELS 16          // largest kernel_num

static_assert(CM_MAX_POOLED >= 1024, "the documented minimum of the size limit");
static_assert((size_t)CM_WAVES * 2 * CM_MAX_POOLED * sizeof(double) <= 65536, "the staging fits the LDS a launch may ask for");

// scale[i] = -log2(e) / mul^(i - num / 2), i < num (host-filled; scale[num - 1] is the widest kernel)
struct CmScales {
  double scale[CM_MAX_KERNELS];
};

__device__ __forceinline__ double cm_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double cm_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the molecule of conformer record c: the last one whose conf_off is <= c
__device__ __forceinline__ int cm_molecule_of(const long long* __restrict__ mol, int G, long long c) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mol[(size_t)mid * CM_MOL + 7] <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- (1) finite flag per conformer ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cm_finite_kernel(const float* __restrict__ ref_pos, const float* __restrict__ gen_pos,
                                                        const long long* __restrict__ mol, int G,
                                                        const unsigned char* __restrict__ mask, long long n_conf,
                                                        unsigned char* __restrict__ finite) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_conf) return;                                   // the whole wavefront leaves
  const long long* m = mol + (size_t)cm_molecule_of(mol, G, c) * CM_MOL;
  const long long n = m[0], R = m[1], j = c - m[7];
  const float* p = j < R ? ref_pos + 3 * (m[3] + j * n) : gen_pos + 3 * (m[4] + (j - R) * n);
  const unsigned char* mk = mask ? mask + m[6] : nullptr;
  bool bad = false;
  for (long long a = lane; a < n; a += 64)
    if (!mk || mk[a]) bad = bad || !(isfinite(p[3 * a]) && isfinite(p[3 * a + 1]) && isfinite(p[3 * a + 2]));
  const unsigned long long any_bad = __ballot(bad);
  if (lane == 0) finite[c] = any_bad == 0ull ? 1 : 0;
}

// ---- (2) position of every kept conformer among the kept ones; one wavefront per molecule -----------------------------------
__global__ void __launch_bounds__(64) cm_rank_kernel(const long long* __restrict__ mol,
                                                     const unsigned char* __restrict__ finite, int* __restrict__ rank,
                                                     int* __restrict__ used) {
  const int lane = threadIdx.x;
  const long long* m = mol + (size_t)blockIdx.x * CM_MOL;
  const long long R = m[1], K = m[2], c0 = m[7];
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = 0, r_used = 0;
  for (int half = 0; half < 2; ++half) {                     // references, then generated: the pooled order
    const long long first = half == 0 ? c0 : c0 + R, cnt = half == 0 ? R : K;
    for (long long j0 = 0; j0 < cnt; j0 += 64) {
      const long long j = j0 + lane;
      const bool f = j < cnt && finite[first + j] != 0;
      const unsigned long long b = __ballot(f);
      if (j < cnt) rank[first + j] = f ? base + __popcll(b & below) : -1;
      base += __popcll(b);
    }
    if (half == 0) r_used = base;
  }
  if (lane == 0) {
    used[2 * blockIdx.x] = r_used;
    used[2 * blockIdx.x + 1] = base - r_used;
  }
}

// ---- (3) the distance table -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cm_table_kernel(const float* __restrict__ ref_pos, const float* __restrict__ gen_pos,
                                                       const long long* __restrict__ mol, int G,
                                                       const long long* __restrict__ pair_ptr, const int* __restrict__ pairs,
                                                       const int* __restrict__ rank, long long n_conf,
                                                       double* __restrict__ z) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_conf) return;
  const int row = rank[c];
  if (row < 0) return;                                       // an excluded conformer has no row (wave-uniform)
  const int g = cm_molecule_of(mol, G, c);
  const long long* m = mol + (size_t)g * CM_MOL;
  const long long n = m[0], R = m[1], C = m[1] + m[2], j = c - m[7];
  const float* p = j < R ? ref_pos + 3 * (m[3] + j * n) : gen_pos + 3 * (m[4] + (j - R) * n);
  const long long E = pair_ptr[g + 1] - pair_ptr[g];
  const int* pr = pairs + 2 * pair_ptr[g];
  double* col = z + m[5] + row;
  for (long long e = lane; e < E; e += 64) {
    const long long u = pr[2 * e], v = pr[2 * e + 1];
    const double dx = (double)p[3 * u] - (double)p[3 * v], dy = (double)p[3 * u + 1] - (double)p[3 * v + 1],
                 dz = (double)p[3 * u + 2] - (double)p[3 * v + 2];
    col[e * C] = sqrt(dx * dx + dy * dy + dz * dz);
  }
}

// ---- (4) sum_{a, b} (z_a - z_b)^2 of every column; one wavefront per column ---------------------------------------------------
__global__ void __launch_bounds__(256) cm_colsum_kernel(const double* __restrict__ z, const long long* __restrict__ mol, int G,
                                                        const long long* __restrict__ pair_ptr, long long n_cols,
                                                        const int* __restrict__ used, double* __restrict__ colsum) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_cols) return;
  int lo = 0, hi = G - 1;                                    // the last molecule whose first column is <= q
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pair_ptr[mid] <= q) lo = mid; else hi = mid - 1;
  }
  const long long* m = mol + (size_t)lo * CM_MOL;
  const long long C = m[1] + m[2];
  const int cu = used[2 * lo] + used[2 * lo + 1];
  const double* col = z + m[5] + (q - pair_ptr[lo]) * C;
  double s = 0.0;
  for (int a = 0; a + 1 < cu; ++a) {
    const double za = col[a];
    for (int b = a + 1 + lane; b < cu; b += 64) {
      const double d = col[b] - za;
      s = fma(d, d, s);
    }
  }
  s = cm_wave_sum(s);
  if (lane == 0) colsum[q] = 2.0 * s;
}

// sum over the num scales of exp(-L / (sigma^2 mul^(i - num / 2))), as base-2 exponentials: scale[i] * inv_s2 is the factor of
// scale i (scale: the launch's table, wave-uniform loads), c_wide that of the widest one, scale[num - 1] * inv_s2
template <bool SQ>
__device__ __forceinline__ float cm_kernel_sum(double L, double c_wide, const double* __restrict__ scale, double inv_s2, int num) {
  if (SQ) {
    float t = __builtin_amdgcn_exp2f((float)(L * c_wide));   // the widest scale; each squaring halves the bandwidth
    float k = t;
    for (int i = 1; i < num; ++i) {
      t *= t;
      k += t;
    }
    return k;
  }
  float k = 0.f;
  for (int i = num - 1; i >= 0; --i) k += __builtin_amdgcn_exp2f((float)(L * (scale[i] * inv_s2)));   // the same order of terms
  return k;
}

// the three sums over the pairs a < b of the cu staged samples of one item (this lane's share): rr both references, gg both
// generated, rg one of each.  Row a is the same for the whole wave, the lanes run along b.
template <bool TWO, bool SQ>
__device__ __forceinline__ void cm_item_sums(const double* s0, const double* s1, int ru, int cu, int lane, double c_wide,
                                             const double* __restrict__ scale, double inv_s2, int num, double& rr, double& gg, double& rg) {
  for (int a = 0; a + 1 < cu; ++a) {
    const double a0 = s0[a], a1 = TWO ? s1[a] : 0.0;
    const bool a_ref = a < ru;
    for (int b = a + 1 + lane; b < cu; b += 64) {
      const double d0 = s0[b] - a0;
      double L = d0 * d0;
      if (TWO) {
        const double d1 = s1[b] - a1;
        L = fma(d1, d1, L);
      }
      const double k = (double)cm_kernel_sum<SQ>(L, c_wide, scale, inv_s2, num);
      if (!a_ref) gg += k;
      else if (b < ru) rr += k;
      else rg += k;
    }
  }
}

// MMD from the three sums over a < b (module comment); exact 0 when every kernel value is num
__device__ __forceinline__ double cm_mmd(double rr, double gg, double rg, int ru, int ku, int num) {
  const double r = (double)ru, k = (double)ku, d = (double)num;
  return (2.0 * rr + r * d) / (r * r) + (2.0 * gg + k * d) / (k * k) - 2.0 * rg / (r * k);
}

// ---- (5) one wavefront per work item ------------------------------------------------------------------------------------------
// items [n_items][3] int32 = molecule, column e, column f (-1: the item is {e}).  The item's one or two columns (the C' kept
// samples) are staged once into this wave's own part of the LDS; the bandwidth is the sum of the columns' entries of colsum.
// R' = 0 or K' = 0: NaN.  sigma^2 = 0: exactly 0.
__global__ void __launch_bounds__(64 * CM_WAVES) cm_items_kernel(const double* __restrict__ z, const long long* __restrict__ mol,
                                                                 const long long* __restrict__ pair_ptr,
                                                                 const int* __restrict__ used,
                                                                 const double* __restrict__ colsum,
                                                                 const int* __restrict__ items, long long n_items, int c_max,
                                                                 CmScales sc, int num, int squaring,
                                                                 double* __restrict__ out) {
  extern __shared__ __align__(16) double cm_cols[];          // [CM_WAVES][2][c_max]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long it = (long long)blockIdx.x * CM_WAVES + wave;
  const bool valid = it < n_items;                           // the same for the whole wave
  double* s0 = cm_cols + (size_t)wave * 2 * c_max;
  double* s1 = s0 + c_max;
  int g = 0, e = 0, f = -1, ru = 0, ku = 0, cu = 0;
  if (valid) {
    g = items[3 * it]; e = items[3 * it + 1]; f = items[3 * it + 2];
    ru = used[2 * g]; ku = used[2 * g + 1];
    cu = min(ru + ku, c_max);                                // ru + ku <= R + K <= c_max by the host's table
    const long long* m = mol + (size_t)g * CM_MOL;
    const long long C = m[1] + m[2];
    const double* c0 = z + m[5] + (long long)e * C;
    const double* c1 = z + m[5] + (long long)(f < 0 ? e : f) * C;
    for (int a = lane; a < cu; a += 64) {
      s0[a] = c0[a];
      s1[a] = c1[a];
    }
  }
  __syncthreads();
  if (!valid) return;
  const long long q0 = pair_ptr[g];
  const double sum_l = f < 0 ? colsum[q0 + e] : colsum[q0 + e] + colsum[q0 + f];
  const double sigma2 = sum_l / ((double)cu * (double)cu - (double)cu);
  if (ru == 0 || ku == 0 || sigma2 == 0.0) {
    if (lane == 0) out[it] = (ru == 0 || ku == 0) ? cm_nan() : 0.0;
    return;
  }
  const double inv_s2 = 1.0 / sigma2, c_wide = sc.scale[num - 1] * inv_s2;
  double rr = 0.0, gg = 0.0, rg = 0.0;
  if (squaring) {
    if (f < 0) cm_item_sums<false, true>(s0, s1, ru, cu, lane, c_wide, sc.scale, inv_s2, num, rr, gg, rg);
    else cm_item_sums<true, true>(s0, s1, ru, cu, lane, c_wide, sc.scale, inv_s2, num, rr, gg, rg);
  } else {
    if (f < 0) cm_item_sums<false, false>(s0, s1, ru, cu, lane, c_wide, sc.scale, inv_s2, num, rr, gg, rg);
    else cm_item_sums<true, false>(s0, s1, ru, cu, lane, c_wide, sc.scale, inv_s2, num, rr, gg, rg);
  }
  rr = cm_wave_sum(rr); gg = cm_wave_sum(gg); rg = cm_wave_sum(rg);
  if (lane == 0) out[it] = cm_mmd(rr, gg, rg, ru, ku, num);
}

// ---- (6) per molecule the mean of its Single items and of its Pair items ------------------------------------------------------
// The items of a launch: the Single items of every molecule (molecule g: pair_ptr[g] .. pair_ptr[g + 1]), then the Pair
// items (molecule g: n_cols + pairitem_ptr[g] ..).  grid (G, 2), one wavefront each; no item: NaN.
__global__ void __launch_bounds__(64) cm_means_kernel(const double* __restrict__ mmd, const long long* __restrict__ pair_ptr,
                                                      const long long* __restrict__ pairitem_ptr, long long n_cols,
                                                      double* __restrict__ means) {
  const int lane = threadIdx.x, g = blockIdx.x, kind = blockIdx.y;
  const long long lo = kind == 0 ? pair_ptr[g] : n_cols + pairitem_ptr[g];
  const long long hi = kind == 0 ? pair_ptr[g + 1] : n_cols + pairitem_ptr[g + 1];
  double s = 0.0;
  for (long long i = lo + lane; i < hi; i += 64) s += mmd[i];
  s = cm_wave_sum(s);
  if (lane == 0) means[2 * g + kind] = hi > lo ? s / (double)(hi - lo) : cm_nan();
}

// ---- (7) All: one workgroup per molecule ----------------------------------------------------------------------------------------
// Wave w takes the rows a = w, w + 4, ...; L of a pair is summed over the columns e = 0, 1, ... in fp64 from the table in
// global memory (a column's samples are contiguous: the lanes' loads coalesce, row a's value is the same for the wave).
template <bool SQ>
__device__ __forceinline__ void cm_all_sums(const double* __restrict__ zc, long long C, long long E, int ru, int cu, int wave,
                                            int lane, double c_wide, const double* __restrict__ scale, double inv_s2, int num,
                                            double& rr, double& gg, double& rg) {
  for (int a = wave; a + 1 < cu; a += 4) {
    const bool a_ref = a < ru;
    for (int b = a + 1 + lane; b < cu; b += 64) {
      double L = 0.0;
      for (long long e = 0; e < E; ++e) {
        const double d = zc[e * C + b] - zc[e * C + a];
        L = fma(d, d, L);
      }
      const double k = (double)cm_kernel_sum<SQ>(L, c_wide, scale, inv_s2, num);
      if (!a_ref) gg += k;
      else if (b < ru) rr += k;
      else rg += k;
    }
  }
}

__global__ void __launch_bounds__(256) cm_all_kernel(const double* __restrict__ z, const long long* __restrict__ mol,
                                                     const long long* __restrict__ pair_ptr, const int* __restrict__ used,
                                                     const double* __restrict__ colsum, CmScales sc, int num, int squaring,
                                                     double* __restrict__ out) {
  __shared__ double part[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.x;
  const long long* m = mol + (size_t)g * CM_MOL;
  const long long C = m[1] + m[2], q0 = pair_ptr[g], E = pair_ptr[g + 1] - q0;
  const int ru = used[2 * g], ku = used[2 * g + 1], cu = ru + ku;
  double sum_l = 0.0;                                        // every thread the same sum, in column order
  for (long long e = 0; e < E; ++e) sum_l += colsum[q0 + e];
  const double sigma2 = sum_l / ((double)cu * (double)cu - (double)cu);
  if (E == 0 || ru == 0 || ku == 0 || sigma2 == 0.0) {       // the same for the whole workgroup
    if (threadIdx.x == 0) out[g] = (E == 0 || ru == 0 || ku == 0) ? cm_nan() : 0.0;
    return;
  }
  const double inv_s2 = 1.0 / sigma2, c_wide = sc.scale[num - 1] * inv_s2;
  double rr = 0.0, gg = 0.0, rg = 0.0;
  if (squaring) cm_all_sums<true>(z + m[5], C, E, ru, cu, wave, lane, c_wide, sc.scale, inv_s2, num, rr, gg, rg);
  else cm_all_sums<false>(z + m[5], C, E, ru, cu, wave, lane, c_wide, sc.scale, inv_s2, num, rr, gg, rg);
  rr = cm_wave_sum(rr); gg = cm_wave_sum(gg); rg = cm_wave_sum(rg);
  if (lane == 0) {
    part[wave][0] = rr; part[wave][1] = gg; part[wave][2] = rg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rr = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
    gg = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
    rg = (part[0][2] + part[1][2]) + (part[2][2] + part[3][2]);
    out[g] = cm_mmd(rr, gg, rg, ru, ku, num);
  }
}

// the kernel parameters shared by the two MMD entry points: 0 or an error code
static int cm_scales(double mul, int num, int exp_path, CmScales* sc, int* squaring) {
  if (!(mul > 0.0) || !isfinite(mul) || num < 1 || num > CM_MAX_KERNELS || exp_path < 0 || exp_path > 1) return MSDE_EINVAL;
  for (int i = 0; i < CM_MAX_KERNELS; ++i)
    sc->scale[i] = i < num ? -1.4426950408889634074 / pow(mul, (double)(i - num / 2)) : 0.0;
  *squaring = (exp_path == 0 && mul == 2.0) ? 1 : 0;
  return 0;
}

extern "C" int msde_conf_dist_table(const float* ref_pos, const float* gen_pos, const long long* mol, int G,
                                    const unsigned char* atom_mask, long long n_conf, const long long* pair_ptr,
                                    const int* pairs, unsigned char* finite, int* rank, int* used, double* z, void* stream) {
  if (!ref_pos || !gen_pos || !mol || !pair_ptr || !pairs || !finite || !rank || !used || !z || G <= 0 ||
      n_conf < 2 * (long long)G)
    return MSDE_EINVAL;
  if ((n_conf + 3) / 4 > 0x7fffffffll) return MSDE_EUNSUP;
  const unsigned blocks = (unsigned)((n_conf + 3) / 4);
  MSDE_LAUNCH(cm_finite_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), ref_pos, gen_pos, mol, G, atom_mask, n_conf,
              finite);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(cm_rank_kernel, dim3((unsigned)G), dim3(64), 0, as_stream(stream), mol, (const unsigned char*)finite, rank, used);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(cm_table_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), ref_pos, gen_pos, mol, G, pair_ptr, pairs,
              (const int*)rank, n_conf, z);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_conf_mmd_subsets(const double* z, const long long* mol, int G, const long long* pair_ptr, long long n_cols,
                                     const int* used, const int* items, long long n_items, const long long* pairitem_ptr,
                                     int c_max, double kernel_mul, int kernel_num, int exp_path, double* colsum, double* mmd,
                                     double* means, void* stream) {
  if (!z || !mol || !pair_ptr || !used || !pairitem_ptr || !means || G <= 0 || n_cols < 0 || n_items < n_cols) return MSDE_EINVAL;
  if (n_items > 0 && (!items || !colsum || !mmd || n_cols == 0)) return MSDE_EINVAL;
  if (c_max < 2 || c_max > CM_MAX_POOLED) return MSDE_EUNSUP;
  if ((n_items + CM_WAVES - 1) / CM_WAVES > 0x7fffffffll) return MSDE_EUNSUP;
  CmScales sc;
  int squaring = 0;
  const int err = cm_scales(kernel_mul, kernel_num, exp_path, &sc, &squaring);
  if (err) return err;
  if (n_items > 0) {
    MSDE_LAUNCH(cm_colsum_kernel, dim3((unsigned)((n_cols + 3) / 4)), dim3(256), 0, as_stream(stream), z, mol, G, pair_ptr,
                n_cols, used, colsum);
    MSDE_CHECK_LAUNCH();
    const size_t lds = (size_t)CM_WAVES * 2 * c_max * sizeof(double);
    MSDE_LAUNCH(cm_items_kernel, dim3((unsigned)((n_items + CM_WAVES - 1) / CM_WAVES)), dim3(64 * CM_WAVES), lds,
                as_stream(stream), z, mol, pair_ptr, used, (const double*)colsum, items, n_items, c_max, sc, kernel_num,
                squaring, mmd);
    MSDE_CHECK_LAUNCH();
  }
  MSDE_LAUNCH(cm_means_kernel, dim3((unsigned)G, 2), dim3(64), 0, as_stream(stream), (const double*)mmd, pair_ptr, pairitem_ptr,
              n_cols, means);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_conf_mmd_all(const double* z, const long long* mol, int G, const long long* pair_ptr, const int* used,
                                 const double* colsum, double kernel_mul, int kernel_num, int exp_path, double* all_mmd,
                                 void* stream) {
  if (!z || !mol || !pair_ptr || !used || !colsum || !all_mmd || G <= 0) return MSDE_EINVAL;
  CmScales sc;
  int squaring = 0;
  const int err = cm_scales(kernel_mul, kernel_num, exp_path, &sc, &squaring);
  if (err) return err;
  MSDE_LAUNCH(cm_all_kernel, dim3((unsigned)G), dim3(256), 0, as_stream(stream), z, mol, pair_ptr, used, colsum, sc, kernel_num,
              squaring, all_mmd);
  MSDE_CHECK_LAUNCH();
  return 0;
}
