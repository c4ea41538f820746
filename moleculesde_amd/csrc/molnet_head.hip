// molnet_head.hip — the MoleculeNet fine-tuning head (examples/finetune_MoleculeNet.py:120-137) on the ragged layout:
// global_mean_pool over each molecule's rows mol_ptr[b] .. mol_ptr[b+1], graph_pred_linear = Linear(D, T), and the masked
// multi-task BCEWithLogitsLoss evaluated in fp64 like the reference (pred.double(), labels in {-1, 0, +1}, 0 = missing,
// loss = sum(loss_mat) / sum(is_valid)).  Molecule sizes are unbounded, T and D are any size (D up to MH_MAX_D: the pooled
// row sits in LDS).  Every reduction runs in a fixed order without atomics: results are bitwise repeatable.
#include "msde_common.h"

#define MH_TASKS_PER_BLOCK 64
#define MH_MAX_D 16384
#define MH_BCE_THREADS 1024

// rows [r0, r1) of molecule b that are inside the tensor (M rows) and below the row bound
__device__ __forceinline__ void mh_rows(const int* __restrict__ mol_ptr, int b, int M, const int* __restrict__ row_bound,
                                        int& r0, int& r1) {
  int hi = M;
  if (row_bound) hi = min(hi, max(row_bound[0], 0));
  r0 = min(max(mol_ptr[b], 0), hi);
  r1 = min(max(mol_ptr[b + 1], 0), hi);
  if (r1 < r0) r1 = r0;
}

// grid (B, ceil(T / 64)), 256 threads, D floats of LDS.  Every block pools its molecule (a fixed-order row sum, then one
// division by the row count as scatter-mean does; an empty molecule pools to 0) and takes the dot products of 64 tasks:
// one wave per task, lanes strided over D, butterfly sum.  Blocks with blockIdx.y == 0 store the pooled row.
__global__ void __launch_bounds__(256)
molnet_pool_logits_kernel(const float* __restrict__ h, int ldh, int M, int D, const int* __restrict__ mol_ptr,
                          const int* __restrict__ row_bound, const float* __restrict__ W, const float* __restrict__ bias,
                          int T, float* __restrict__ pool, float* __restrict__ logits) {
  extern __shared__ float sp[];
  const int b = blockIdx.x, tid = threadIdx.x;
  int r0, r1;
  mh_rows(mol_ptr, b, M, row_bound, r0, r1);
  const float cnt = (float)max(r1 - r0, 1);
  for (int d = tid; d < D; d += 256) {
    // four interleaved partial sums (row r goes to s[r % 4], fixed): four independent loads in flight per thread
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int r = r0;
    for (; r + 3 < r1; r += 4) {
      s0 += h[(long long)r * ldh + d];
      s1 += h[(long long)(r + 1) * ldh + d];
      s2 += h[(long long)(r + 2) * ldh + d];
      s3 += h[(long long)(r + 3) * ldh + d];
    }
    for (; r < r1; ++r) s0 += h[(long long)r * ldh + d];
    float s = ((s0 + s1) + (s2 + s3)) / cnt;
    sp[d] = s;
    if (blockIdx.y == 0) pool[(long long)b * D + d] = s;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int t_end = min(T, (int)(blockIdx.y + 1) * MH_TASKS_PER_BLOCK);
  for (int t = blockIdx.y * MH_TASKS_PER_BLOCK + wave; t < t_end; t += 4) {
    const float* w = W + (long long)t * D;
    float acc = 0.f;
    for (int d = lane; d < D; d += 64) acc = fmaf(sp[d], w[d], acc);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) logits[(long long)b * T + t] = acc + (bias ? bias[t] : 0.f);
  }
}

__device__ __forceinline__ double mh_sigmoid(double z) {
  if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
  double e = exp(z);
  return e / (1.0 + e);
}

// one workgroup of MH_BCE_THREADS: per-thread fp64 partial sums over a fixed stride, then a fixed tree in LDS.
//   loss_mat[i] = valid ? max(z,0) - z t + log1p(exp(-|z|)) : 0,  t = (y + 1) / 2, valid = y^2 > 0
//   stats = {sum loss_mat / count (0/0 = NaN as in the reference), count, number of NaN logits}
//   dlogits[i] = valid ? (sigmoid(z) - t) * (1 / count) : 0   (the reference's fp64 backward, cast to fp32)
__global__ void __launch_bounds__(MH_BCE_THREADS)
molnet_bce_kernel(const float* __restrict__ logits, const float* __restrict__ y, long long n, double* __restrict__ loss_mat,
                  double* __restrict__ stats, float* __restrict__ dlogits) {
  __shared__ double s_sum[MH_BCE_THREADS];
  __shared__ long long s_cnt[MH_BCE_THREADS], s_nan[MH_BCE_THREADS];
  const int tid = threadIdx.x;
  double sum = 0.0;
  long long cnt = 0, nan = 0;
  for (long long i = tid; i < n; i += MH_BCE_THREADS) {
    const double z = (double)logits[i], yy = (double)y[i];
    const bool valid = yy * yy > 0.0;
    double l = 0.0;
    if (valid) {
      const double t = (yy + 1.0) / 2.0;
      l = fmax(z, 0.0) - z * t + log1p(exp(-fabs(z)));
      ++cnt;
    }
    if (isnan(z)) ++nan;
    if (loss_mat) loss_mat[i] = l;
    sum += l;
  }
  s_sum[tid] = sum;
  s_cnt[tid] = cnt;
  s_nan[tid] = nan;
  __syncthreads();
  for (int o = MH_BCE_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_cnt[tid] += s_cnt[tid + o];
      s_nan[tid] += s_nan[tid + o];
    }
    __syncthreads();
  }
  const double total = (double)s_cnt[0];
  if (tid == 0) {
    stats[0] = s_sum[0] / total;
    stats[1] = total;
    stats[2] = (double)s_nan[0];
  }
  if (!dlogits) return;
  const double inv = 1.0 / total;
  for (long long i = tid; i < n; i += MH_BCE_THREADS) {
    const double z = (double)logits[i], yy = (double)y[i];
    float g = 0.f;
    if (yy * yy > 0.0) g = (float)((mh_sigmoid(z) - (yy + 1.0) / 2.0) * inv);
    dlogits[i] = g;
  }
}

// grid (B + 1, ceil(D / 64)), 256 threads: 64 columns per block, wave w takes the tasks t = w (mod 4) in order and the
// four partial sums are added in a fixed order: d pool[b][d] = sum_t dlogits[b][t] W[t][d], written divided by the row
// count to every row of molecule b below the bound; rows of b at or past the bound, and (block B) the rows mol_ptr[B] .. M
// of the capacity, get 0.
__global__ void __launch_bounds__(256)
molnet_head_bwd_kernel(const float* __restrict__ dlogits, int B, int T, const float* __restrict__ W, int D,
                       const int* __restrict__ mol_ptr, const int* __restrict__ row_bound, int M, float* __restrict__ dh,
                       int ldh) {
  __shared__ float red[4][64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = blockIdx.y * 64 + lane;
  const bool col = d < D;
  if (b == B) {                       // (uniform over the block: no barrier is skipped by part of it)
    if (col)
      for (int r = min(max(mol_ptr[B], 0), M) + wave; r < M; r += 4) dh[(long long)r * ldh + d] = 0.f;
    return;
  }
  int r0, r1;
  mh_rows(mol_ptr, b, M, row_bound, r0, r1);
  float acc = 0.f;
  if (col && r1 > r0) {
    const float* g = dlogits + (long long)b * T;
    for (int t = wave; t < T; t += 4) acc = fmaf(g[t], W[(long long)t * D + d], acc);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (!col) return;
  const float dp = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) / (float)max(r1 - r0, 1);
  for (int r = r0 + wave; r < r1; r += 4) dh[(long long)r * ldh + d] = dp;
  const int m1 = min(max(mol_ptr[b + 1], 0), M);
  for (int r = max(r1, min(max(mol_ptr[b], 0), M)) + wave; r < m1; r += 4) dh[(long long)r * ldh + d] = 0.f;
}

extern "C" int msde_molnet_head_fwd(const float* h, int ldh, int M, int D, const int* mol_ptr, int B, const int* row_bound,
                                    const float* W, const float* bias, int T, float* pool, float* logits, void* stream) {
  if (M < 0 || D < 1 || B < 0 || T < 1 || ldh < D || !mol_ptr || !W || !pool || !logits || (M > 0 && !h)) return MSDE_EINVAL;
  if (D > MH_MAX_D) return MSDE_EUNSUP;
  if (B == 0) return 0;
  dim3 grid(B, (T + MH_TASKS_PER_BLOCK - 1) / MH_TASKS_PER_BLOCK);
  MSDE_LAUNCH(molnet_pool_logits_kernel, grid, dim3(256), (size_t)D * sizeof(float), as_stream(stream), h, ldh, M, D,
              mol_ptr, row_bound, W, bias, T, pool, logits);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_molnet_bce(const float* logits, const float* y, int B, int T, double* loss_mat, double* stats,
                               float* dlogits, void* stream) {
  if (B < 0 || T < 1 || !logits || !y || !stats) return MSDE_EINVAL;
  MSDE_LAUNCH(molnet_bce_kernel, dim3(1), dim3(MH_BCE_THREADS), 0, as_stream(stream), logits, y, (long long)B * T, loss_mat, stats,
              dlogits);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_molnet_head_bwd(const float* dlogits, int B, int T, const float* W, int D, const int* mol_ptr,
                                    const int* row_bound, int M, float* dh, int ldh, void* stream) {
  if (M < 0 || D < 1 || B < 0 || T < 1 || ldh < D || !dlogits || !W || !mol_ptr || (M > 0 && !dh)) return MSDE_EINVAL;
  if (M == 0) return 0;
  dim3 grid(B + 1, (D + 63) / 64);
  MSDE_LAUNCH(molnet_head_bwd_kernel, grid, dim3(256), 0, as_stream(stream), dlogits, B, T, W, D, mol_ptr, row_bound, M, dh,
              ldh);
  MSDE_CHECK_LAUNCH();
  return 0;
}
