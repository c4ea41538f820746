// contrastive_infonce.hip — the 'InfoNCE_dot_prod' and 'EBM_dot_prod' branches of do_CL in both directions
// (examples/util.py:22-50,76-79: do_CL + dual_CL, node level from examples/pretrain_MoleculeSDE.py:137).
//
// InfoNCE.  S = X Y^T / T over all N atoms of the batch; the second direction's logits Y X^T / T are S^T, so one matrix
// serves both:
//   loss = [ mean_i (lse_j S_ij - S_ii) + mean_j (lse_i S_ij - S_jj) ] / 2
//   acc  = [ mean_i 1{argmax_j S_ij = i} + mean_j 1{argmax_i S_ij = j} ] / 2          (ties: the lowest index, torch.argmax)
//   dL/dS_ij = g / 2N * [ exp(S_ij - lse_r[i]) + exp(S_ij - lse_c[j]) - 2 delta_ij ]
//   gX = (dL/dS) Y / T,  gY = (dL/dS)^T X / T
// Forward: (1) a 64 x 64 tile of S per workgroup on v_mfma_f32_16x16x4_f32 (exact f32), its epilogue writes the tile to
// the workspace and per-tile row and column partials (max, sum of exp relative to it, first argmax); (2) one thread per
// row / column merges the partials in tile order into lse and a loss term; (3) one workgroup sums the terms in a fixed
// order.  Backward: one launch, both products: the A operand of gX is dL/dS read along rows of S, that of gY along its
// columns; the transform is applied while the S tile is staged, so dL/dS is never written.  No atomics anywhere.
//
// EBM_dot_prod with K deterministic cyclic shifts (util.py:16-19 cycle_index): row i has the positive <X_i, Y_i> / T, the
// negatives n1_is = <X_i, Y_(i+s) mod N> / T and n2_is = <Y_i, X_(i+s) mod N> / T for s = 1..K;
//   loss = [ 2 sum BCE(p,1) + sum BCE(n1,0) + sum BCE(n2,0) ] / 2N
//        (= mean over both directions of BCE_mean(pos, 1) + K * BCE_mean(neg, 0), the mean over all K N negatives)
//   acc  = [ 2 #{p>0} + #{n1<0} + #{n2<0} ] / (2 N (1 + K))
//
// Row bound (capacity buckets).  Every kernel takes `n_rows`, a device count: N stays the host-known CAPACITY -- grids,
// workspace size and every workspace stride are functions of N alone, so one captured graph serves every count -- and
// n = msde_true_rows(N, n_rows) <= N rows are valid (NULL: all of them).  Rows >= n are never read into a reduction (they
// may hold anything, NaN included), their gradients are written as exact zeros and their EBM logits as zeros; "N" in the
// formulas above is n.  n >= 1 is the contract; at n = 0 every kernel terminates inside its buffers, outputs unspecified.
#include "msde_common.h"

typedef float ci_f32x4 __attribute__((ext_vector_type(4)));

#define CI_BM 64                  // output tile: 64 x 64, four waves of 2 x 2 accumulators of 16 x 16
#define CI_KC 16                  // k per LDS stage of the forward (K = D, a few hundred)
#define CI_KB 64                  // k per LDS stage of the backward (K = N): four times the MFMA work behind each prefetch
#define CI_LDA 80                 // LDS stride of a [k][m] stage: the four k rows of a fragment read land on distinct banks
#define CI_LDT 65                 // LDS stride of the forward epilogue's [64][64] tile (row and column scans conflict-free)
#define CI_SMEM (CI_BM * CI_LDT)  // floats: >= the two forward stages (2 * CI_KC * CI_LDA)

__host__ __device__ static inline long long ci_tiles(int N) { return (N + CI_BM - 1) / CI_BM; }

// workspace (floats): S [N][N] | row partials max, sum, argmax [T][N] each | column partials [T][N] each |
// lse [2N] (rows, then columns) | loss terms [2N] | correct flags [2N]
struct CiWs {
  float *S, *rmax, *rsum, *cmax, *csum, *lse, *term, *corr;
  int *ridx, *cidx;
};
__host__ __device__ static inline CiWs ci_ws(float* ws, int N) {
  const long long T = ci_tiles(N), n = N;
  CiWs w;
  w.S = ws;
  float* p = ws + n * n;
  w.rmax = p; w.rsum = p + T * n; w.ridx = reinterpret_cast<int*>(p + 2 * T * n); p += 3 * T * n;
  w.cmax = p; w.csum = p + T * n; w.cidx = reinterpret_cast<int*>(p + 2 * T * n); p += 3 * T * n;
  w.lse = p; w.term = p + 2 * n; w.corr = p + 4 * n;
  return w;
}

__device__ __forceinline__ float bce_logits(float x, float z) {
  // torch.nn.BCEWithLogitsLoss element: max(x,0) - x*z + log(1 + exp(-|x|))
  return fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// KC k of the 64 x 64 tile: wave (wr, wc) owns rows 32 wr .. + 31 and columns 32 wc .. + 31 (2 x 2 MFMA tiles).
// 16x16x4 operand map: lane l holds A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15].
template <int KC>
__device__ __forceinline__ void ci_mfma_stage(const float* sA, const float* sB, int wr, int wc, int lane,
                                              ci_f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < KC / 4; ++ks) {
    const int k = 4 * ks + (lane >> 4);
    float af[2], bf[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) af[a] = sA[k * CI_LDA + 32 * wr + 16 * a + (lane & 15)];
#pragma unroll
    for (int b = 0; b < 2; ++b) bf[b] = sB[k * CI_LDA + 32 * wc + 16 * b + (lane & 15)];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a], bf[b], acc[a][b], 0, 0, 0);
  }
}

// ---- InfoNCE forward (1): S tile + partials ---------------------------------------------------------------------
// grid (T, T): blockIdx.x = column tile, blockIdx.y = row tile.  Both operands k-contiguous ([N][D] as stored); rows past
// n and k past D are staged as zeros (a padded row may hold NaN, and NaN * 0 inside an MFMA would poison the whole tile).
__global__ void __launch_bounds__(256) ci_fwd_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, int N,
                                                          const int* __restrict__ n_rows, int D, float invT,
                                                          float* __restrict__ ws) {
  const int n = msde_true_rows(N, n_rows);
  __shared__ float smem[CI_SMEM];
  float* sA = smem;
  float* sB = smem + CI_KC * CI_LDA;
  const CiWs w = ci_ws(ws, N);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave & 1, wc = wave >> 1;
  const int i0 = blockIdx.y * CI_BM, j0 = blockIdx.x * CI_BM;
  if (i0 >= n || j0 >= n) return;                // a tile wholly behind the bound: nothing reads it (whole workgroup leaves)
  const int kk = t & 15, mm = t >> 4;
  float ra[4], rb[4];
  auto load = [&](int k0) {
    const int k = k0 + kk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = mm + 16 * r;
      ra[r] = (i0 + m < n && k < D) ? X[(size_t)(i0 + m) * D + k] : 0.f;
      rb[r] = (j0 + m < n && k < D) ? Y[(size_t)(j0 + m) * D + k] : 0.f;
    }
  };
  ci_f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = ci_f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int k0 = 0; k0 < D; k0 += CI_KC) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sA[kk * CI_LDA + mm + 16 * r] = ra[r];
      sB[kk * CI_LDA + mm + 16 * r] = rb[r];
    }
    __syncthreads();
    if (k0 + CI_KC < D) load(k0 + CI_KC);       // next stage in flight behind this stage's MFMAs
    ci_mfma_stage<CI_KC>(sA, sB, wr, wc, lane, acc);
  }
  __syncthreads();
  float* sT = smem;                              // C/D map: row 4 (l >> 4) + reg, column l & 15
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sT[(32 * wr + 16 * a + 4 * (lane >> 4) + r) * CI_LDT + 32 * wc + 16 * b + (lane & 15)] = acc[a][b][r] * invT;
  __syncthreads();
  const int nr = min(CI_BM, n - i0), nc = min(CI_BM, n - j0);
  for (int e = t; e < CI_BM * CI_BM; e += 256) {
    const int r = e >> 6, c = e & 63;
    if (r < nr && c < nc) w.S[(size_t)(i0 + r) * N + j0 + c] = sT[r * CI_LDT + c];
  }
  if (wave == 0 && lane < nr) {                  // row partials over this tile's columns
    const float* row = sT + lane * CI_LDT;
    float m = row[0];
    int arg = 0;
    for (int c = 1; c < nc; ++c)
      if (row[c] > m) { m = row[c]; arg = c; }
    float s = 0.f;
    for (int c = 0; c < nc; ++c) s += expf(row[c] - m);
    const size_t o = (size_t)blockIdx.x * N + i0 + lane;
    w.rmax[o] = m; w.rsum[o] = s; w.ridx[o] = j0 + arg;
  } else if (wave == 1 && lane < nc) {           // column partials over this tile's rows
    const float* col = sT + lane;
    float m = col[0];
    int arg = 0;
    for (int r = 1; r < nr; ++r)
      if (col[r * CI_LDT] > m) { m = col[r * CI_LDT]; arg = r; }
    float s = 0.f;
    for (int r = 0; r < nr; ++r) s += expf(col[r * CI_LDT] - m);
    const size_t o = (size_t)blockIdx.y * N + j0 + lane;
    w.cmax[o] = m; w.csum[o] = s; w.cidx[o] = i0 + arg;
  }
}

// ---- InfoNCE forward (2): merge the partials of each row (u < N) and column (u - N), tile by tile in order -------------
// rows and columns < n over the ci_tiles(n) tiles that hold them; every stride stays N
__global__ void __launch_bounds__(256) ci_merge_kernel(int N, const int* __restrict__ n_rows, float* __restrict__ ws) {
  const CiWs w = ci_ws(ws, N);
  const int n = msde_true_rows(N, n_rows);
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= 2 * N) return;
  const bool col = u >= N;
  const int r = col ? u - N : u;
  if (r >= n) return;
  const float* pm = col ? w.cmax : w.rmax;
  const float* ps = col ? w.csum : w.rsum;
  const int* pi = col ? w.cidx : w.ridx;
  const int T = (int)ci_tiles(n);
  float M = pm[r];
  int arg = pi[r];
  for (int t = 1; t < T; ++t) {
    const float m = pm[(size_t)t * N + r];
    if (m > M) { M = m; arg = pi[(size_t)t * N + r]; }    // strictly greater: an equal later tile keeps the lower index
  }
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += ps[(size_t)t * N + r] * expf(pm[(size_t)t * N + r] - M);
  const float lse = M + logf(s);
  w.lse[u] = lse;
  w.term[u] = lse - w.S[(size_t)r * N + r];
  w.corr[u] = arg == r ? 1.f : 0.f;
}

// ---- InfoNCE forward (3): out = {loss, acc}, fixed-order sums over the 2n terms (n row terms, then n column terms; the
// column terms start N, not n, behind the row terms) ----------------------------------------------------------------
__global__ void __launch_bounds__(1024) ci_final_kernel(int N, const int* __restrict__ n_rows, const float* __restrict__ ws,
                                                        float* __restrict__ out) {
  __shared__ float s_l[16], s_a[16];
  const CiWs w = ci_ws(const_cast<float*>(ws), N);
  const int n = msde_true_rows(N, n_rows);
  float l = 0.f, a = 0.f;
  for (int v = threadIdx.x; v < 2 * n; v += 1024) {
    const int u = v < n ? v : N + (v - n);
    l += w.term[u]; a += w.corr[u];
  }
  l = group_sum(l, 64); a = group_sum(a, 64);
  if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = l; s_a[threadIdx.x >> 6] = a; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f, A = 0.f;
    for (int v = 0; v < 16; ++v) { L += s_l[v]; A += s_a[v]; }
    out[0] = L / (2.f * (float)n);
    out[1] = A / (2.f * (float)n);
  }
}

// ---- InfoNCE backward: blockIdx.z = 0: gX[i][d] = c sum_j P_ij Y[j][d];  = 1: gY[j][d] = c sum_i P_ij X[i][d] ------
// grid (ceil(D / 64), T, 2); P = exp(S - lse_r) + exp(S - lse_c) - 2 delta, c = g invT / 2n.  The reduction runs over the n
// valid rows; rows n <= m < N of gX and gY are written as exact zeros (a workgroup whose 64 rows lie wholly behind n writes
// only those).
__device__ __forceinline__ float ci_dlds(float s, float lr, float lc, int i, int j) {
  return expf(s - lr) + expf(s - lc) - (i == j ? 2.f : 0.f);
}

__global__ void __launch_bounds__(256) ci_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                     const float* __restrict__ ws, const float* __restrict__ g_loss, int N,
                                                     const int* __restrict__ n_rows, int D, float invT,
                                                     float* __restrict__ gX, float* __restrict__ gY) {
  constexpr int R = CI_KB / 4;                     // staged values per thread and operand
  __shared__ float sA[CI_KB * CI_LDA], sB[CI_KB * CI_LDA];
  const CiWs w = ci_ws(const_cast<float*>(ws), N);
  const int n = msde_true_rows(N, n_rows);
  const float* __restrict__ S = w.S;
  const float* __restrict__ lse_r = w.lse;
  const float* __restrict__ lse_c = w.lse + N;
  const bool tr = blockIdx.z != 0;                 // gY: the A operand runs down the columns of S
  const float* __restrict__ Bsrc = tr ? X : Y;
  float* __restrict__ G = tr ? gY : gX;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave & 1, wc = wave >> 1;
  const int m0 = blockIdx.y * CI_BM, d0 = blockIdx.x * CI_BM;
  if (m0 >= n) {                                   // wholly behind the bound (the whole workgroup): zero gradient rows
    for (int e = t; e < CI_BM * CI_BM; e += 256) {
      const int m = m0 + (e >> 6), d = d0 + (e & 63);
      if (m < N && d < D) G[(size_t)m * D + d] = 0.f;
    }
    return;
  }
  // staging roles: gX's A is k-contiguous (a row of S): k = (t & 15) + 16 q, m = (t >> 4) + 16 r; every other operand
  // here is m- / n-contiguous: m = t & 63, k = (t >> 6) + 4 r
  const int kk16 = t & 15, mm16 = t >> 4, mm64 = t & 63, kk64 = t >> 6;
  float lfix[4];                                   // the lse of the operand rows this thread always stages
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = tr ? m0 + mm64 : m0 + mm16 + 16 * r;
    lfix[r] = m < n ? (tr ? lse_c[m] : lse_r[m]) : 0.f;
  }
  float ra[R], rb[R];
  auto load = [&](int k0) {
    if (!tr) {
#pragma unroll
      for (int q = 0; q < CI_KB / 16; ++q) {
        const int j = k0 + kk16 + 16 * q;
        const float lc = j < n ? lse_c[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = m0 + mm16 + 16 * r;
          ra[4 * q + r] = (i < n && j < n) ? ci_dlds(S[(size_t)i * N + j], lfix[r], lc, i, j) : 0.f;
        }
      }
    } else {
      const int j = m0 + mm64;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = k0 + kk64 + 4 * r;
        ra[r] = (i < n && j < n) ? ci_dlds(S[(size_t)i * N + j], lse_r[i], lfix[0], i, j) : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = k0 + kk64 + 4 * r, d = d0 + mm64;
      rb[r] = (k < n && d < D) ? Bsrc[(size_t)k * D + d] : 0.f;
    }
  };
  ci_f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = ci_f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int k0 = 0; k0 < n; k0 += CI_KB) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!tr) sA[(kk16 + 16 * (r >> 2)) * CI_LDA + mm16 + 16 * (r & 3)] = ra[r];
      else sA[(kk64 + 4 * r) * CI_LDA + mm64] = ra[r];
      sB[(kk64 + 4 * r) * CI_LDA + mm64] = rb[r];
    }
    __syncthreads();
    if (k0 + CI_KB < n) load(k0 + CI_KB);
    ci_mfma_stage<CI_KB>(sA, sB, wr, wc, lane, acc);
  }
  const float c = g_loss[0] * invT / (2.f * (float)n);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 32 * wr + 16 * a + 4 * (lane >> 4) + r, d = d0 + 32 * wc + 16 * b + (lane & 15);
        if (m < N && d < D) G[(size_t)m * D + d] = m < n ? acc[a][b][r] * c : 0.f;
      }
}

extern "C" long long msde_cl_infonce_workspace_floats(int N) {
  if (N <= 0) return 0;
  const long long n = N;
  return n * n + 6 * ci_tiles(N) * n + 6 * n;
}

// grids from the capacity N alone: the same launches for every count behind n_rows
extern "C" int msde_cl_infonce_fwd_rows(const float* X, const float* Y, int N, int D, float invT, float* ws, float* out,
                                        const int* n_rows, void* stream) {
  if (N <= 0 || D <= 0 || !X || !Y || !ws || !out) return MSDE_EINVAL;
  const int T = (int)ci_tiles(N);
  MSDE_LAUNCH(ci_fwd_tile_kernel, dim3(T, T), dim3(256), 0, as_stream(stream), X, Y, N, n_rows, D, invT, ws);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(ci_merge_kernel, dim3((2 * N + 255) / 256), dim3(256), 0, as_stream(stream), N, n_rows, ws);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(ci_final_kernel, dim3(1), dim3(1024), 0, as_stream(stream), N, n_rows, (const float*)ws, out);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_cl_infonce_fwd(const float* X, const float* Y, int N, int D, float invT, float* ws, float* out,
                                   void* stream) {
  return msde_cl_infonce_fwd_rows(X, Y, N, D, invT, ws, out, nullptr, stream);
}

extern "C" int msde_cl_infonce_bwd_rows(const float* X, const float* Y, const float* ws, const float* g_loss, int N, int D,
                                        float invT, float* gX, float* gY, const int* n_rows, void* stream) {
  if (N <= 0 || D <= 0 || !X || !Y || !ws || !g_loss || !gX || !gY) return MSDE_EINVAL;
  MSDE_LAUNCH(ci_bwd_kernel, dim3((D + CI_BM - 1) / CI_BM, (unsigned)ci_tiles(N), 2), dim3(256), 0, as_stream(stream), X,
              Y, ws, g_loss, N, n_rows, D, invT, gX, gY);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_cl_infonce_bwd(const float* X, const float* Y, const float* ws, const float* g_loss, int N, int D,
                                   float invT, float* gX, float* gY, void* stream) {
  return msde_cl_infonce_bwd_rows(X, Y, ws, g_loss, N, D, invT, gX, gY, nullptr, stream);
}

// ---- EBM_dot_prod ---------------------------------------------------------------------------------------------------
// (i + s) mod n and (i - s) mod n for ANY s >= 1 (one wrap when s < n, the product's case; memory-safe when K >= n)
__device__ __forceinline__ int cls_fwd_index(int i, int s, int n) {
  int j = i + s;
  if (j >= n) { j -= n; if (j >= n) j %= n; }
  return j;
}
__device__ __forceinline__ int cls_bwd_index(int i, int s, int n) {
  int k = i - s;
  if (k < 0) { k += n; if (k < 0) k = (n - (-k) % n) % n; }
  return k;
}

// rows [N][1 + 2K]: p, n1 (s = 1..K), n2 (s = 1..K) of each row, already divided by T; zeros for rows n <= i < N
template <int V>
__global__ void cls_rows_kernel(const float* __restrict__ X, const float* __restrict__ Y, int N,
                                const int* __restrict__ n_rows, int K, int cols, int tpr, float invT,
                                float* __restrict__ rows) {
  using T = typename VecT<V>::type;
  const int rpb = blockDim.x / tpr;
  const int i = blockIdx.x * rpb + threadIdx.x / tpr;
  const int lane = threadIdx.x % tpr;
  if (i >= N) return;
  const int n = msde_true_rows(N, n_rows);
  if (i >= n) {                                          // logits of padded rows: zero (finite), never stale memory
    if (lane == 0)
      for (int s = 0; s <= 2 * K; ++s) rows[(size_t)i * (1 + 2 * K) + s] = 0.f;
    return;
  }
  const T* Xv = reinterpret_cast<const T*>(X);
  const T* Yv = reinterpret_cast<const T*>(Y);
  const T* x = Xv + (size_t)i * cols;
  const T* y = Yv + (size_t)i * cols;
  float* out = rows + (size_t)i * (1 + 2 * K);
  float p = 0.f;
  for (int c = lane; c < cols; c += tpr) p += vhsum(vmul(x[c], y[c]));
  p = group_sum(p, tpr);
  if (lane == 0) out[0] = p * invT;
  for (int s = 1; s <= K; ++s) {
    const int j = cls_fwd_index(i, s, n);
    const T* yj = Yv + (size_t)j * cols;
    const T* xj = Xv + (size_t)j * cols;
    float n1 = 0.f, n2 = 0.f;
    for (int c = lane; c < cols; c += tpr) {
      n1 += vhsum(vmul(x[c], yj[c]));
      n2 += vhsum(vmul(y[c], xj[c]));
    }
    n1 = group_sum(n1, tpr); n2 = group_sum(n2, tpr);
    if (lane == 0) { out[s] = n1 * invT; out[K + s] = n2 * invT; }
  }
}

__global__ void __launch_bounds__(1024) cls_reduce_kernel(const float* __restrict__ rows, int N,
                                                          const int* __restrict__ n_rows, int K, float* __restrict__ out) {
  __shared__ float s_l[16], s_a[16];
  const int n = msde_true_rows(N, n_rows);
  float l = 0.f, a = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float* r = rows + (size_t)i * (1 + 2 * K);
    l += 2.f * bce_logits(r[0], 1.f);
    a += r[0] > 0.f ? 2.f : 0.f;
    for (int s = 1; s <= 2 * K; ++s) {
      l += bce_logits(r[s], 0.f);
      a += r[s] < 0.f ? 1.f : 0.f;
    }
  }
  l = group_sum(l, 64); a = group_sum(a, 64);
  if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = l; s_a[threadIdx.x >> 6] = a; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f, A = 0.f;
    for (int v = 0; v < 16; ++v) { L += s_l[v]; A += s_a[v]; }
    out[0] = L / (2.f * (float)n);
    out[1] = A / (2.f * (float)n * (float)(1 + K));
  }
}

// (N = the valid rows n; rows n <= i < N get a zero gradient)
// gX_i = g/(2N T) [ -2 sig(-p_i) Y_i + sum_s sig(n1_is) Y_(i+s) + sum_s sig(n2_(i-s)s) Y_(i-s) ], gY_i the same with X and
// the roles of n1 / n2 swapped: row i-s used X_i (resp. Y_i) as its negative at shift s.  Gathers only, no atomics.
template <int V>
__global__ void cls_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ rows,
                               const float* __restrict__ g_loss, int N, const int* __restrict__ n_rows, int K, int cols,
                               int tpr, float invT, float* __restrict__ gX, float* __restrict__ gY) {
  using T = typename VecT<V>::type;
  const int rpb = blockDim.x / tpr;
  const int i = blockIdx.x * rpb + threadIdx.x / tpr;
  const int lane = threadIdx.x % tpr;
  if (i >= N) return;
  const int n = msde_true_rows(N, n_rows);
  if (i >= n) {                                          // rows past the valid ones carry a ZERO gradient
    T* zx = reinterpret_cast<T*>(gX) + (size_t)i * cols;
    T* zy = reinterpret_cast<T*>(gY) + (size_t)i * cols;
    for (int c = lane; c < cols; c += tpr) { zx[c] = vzero<V>(); zy[c] = vzero<V>(); }
    return;
  }
  const int R = 1 + 2 * K;
  const float g = g_loss[0] * invT / (float)n;
  const float dp = -g * sigmoidf_(-rows[(size_t)i * R]);
  const T* Xv = reinterpret_cast<const T*>(X);
  const T* Yv = reinterpret_cast<const T*>(Y);
  T* gXv = reinterpret_cast<T*>(gX) + (size_t)i * cols;
  T* gYv = reinterpret_cast<T*>(gY) + (size_t)i * cols;
  for (int c = lane; c < cols; c += tpr) {
    T gx = vscale(Yv[(size_t)i * cols + c], dp);
    T gy = vscale(Xv[(size_t)i * cols + c], dp);
    for (int s = 1; s <= K; ++s) {
      const int j = cls_fwd_index(i, s, n);
      const int k = cls_bwd_index(i, s, n);
      const float dn1 = 0.5f * g * sigmoidf_(rows[(size_t)i * R + s]);
      const float dn2 = 0.5f * g * sigmoidf_(rows[(size_t)i * R + K + s]);
      const float dn1k = 0.5f * g * sigmoidf_(rows[(size_t)k * R + s]);
      const float dn2k = 0.5f * g * sigmoidf_(rows[(size_t)k * R + K + s]);
      gx = vadd(gx, vscale(Yv[(size_t)j * cols + c], dn1));
      gx = vadd(gx, vscale(Yv[(size_t)k * cols + c], dn2k));
      gy = vadd(gy, vscale(Xv[(size_t)j * cols + c], dn2));
      gy = vadd(gy, vscale(Xv[(size_t)k * cols + c], dn1k));
    }
    gXv[c] = gx;
    gYv[c] = gy;
  }
}

// K < N (the capacity) is all the host can check here; K >= *n_rows is rejected by the callers that know the count and is
// memory-safe in the kernels (indices mod n)
extern "C" int msde_cl_ebm_shift_fwd_rows(const float* X, const float* Y, int N, int D, int K, float invT, float* rows,
                                          float* out, const int* n_rows, void* stream) {
  if (N <= 0 || D <= 0 || K < 1 || K >= N || !X || !Y || !rows || !out) return MSDE_EINVAL;
  LAUNCH_ROWS(cls_rows_kernel, N, D, X, Y, N, n_rows, K, cols, tpr, invT, rows);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(cls_reduce_kernel, dim3(1), dim3(1024), 0, as_stream(stream), (const float*)rows, N, n_rows, K, out);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_cl_ebm_shift_fwd(const float* X, const float* Y, int N, int D, int K, float invT, float* rows,
                                     float* out, void* stream) {
  return msde_cl_ebm_shift_fwd_rows(X, Y, N, D, K, invT, rows, out, nullptr, stream);
}

extern "C" int msde_cl_ebm_shift_bwd_rows(const float* X, const float* Y, const float* rows, const float* g_loss, int N,
                                          int D, int K, float invT, float* gX, float* gY, const int* n_rows, void* stream) {
  if (N <= 0 || D <= 0 || K < 1 || K >= N || !X || !Y || !rows || !g_loss || !gX || !gY) return MSDE_EINVAL;
  LAUNCH_ROWS(cls_bwd_kernel, N, D, X, Y, rows, g_loss, N, n_rows, K, cols, tpr, invT, gX, gY);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_cl_ebm_shift_bwd(const float* X, const float* Y, const float* rows, const float* g_loss, int N, int D,
                                     int K, float invT, float* gX, float* gY, void* stream) {
  return msde_cl_ebm_shift_bwd_rows(X, Y, rows, g_loss, N, D, K, invT, gX, gY, nullptr, stream);
}
