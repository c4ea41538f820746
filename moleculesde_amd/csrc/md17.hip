// md17.hip — the device side of an MD17 fine-tuning epoch (examples/finetune_MD17.py:34-142) beyond the step itself:
//   msde_md17_eval_accumulate   eval() (:93-142): sum |E - y|, the molecule count, sum |-dE - f| over the predicted force
//                               entries that are not NaN (the force[~mask] rule of :127-130) and their count, added to a
//                               device fp64 accumulator, so an evaluation reads the host once, at its end;
//   msde_l1_energy_force_loss_acc  the step loss of msde_l1_energy_force_loss (pointwise.hip), same arithmetic in the same
//                               order (bitwise the same loss and seeds), plus the loss added to a device fp64 epoch sum;
//   msde_md17_gather_batch      batch k of a split held on the device (k read from a device counter, rows through an
//                               optional permutation) copied into a captured graph's static inputs; the counter is
//                               incremented, so an epoch is a loop of replays with no host copy and no host read.
// All three are one workgroup of 1024 threads.  A batch is B * NA * 3 ~ 8 k floats (128 conformations of 21 atoms) up to a
// few times that: 32-96 KB read, a few microseconds on one CU, against ~1.5 us for every dependent kernel boundary a second
// (combine) launch of a two-level reduction would add; one workgroup also gives the fixed summation order for free.
#include "msde_common.h"

#define MD17_THREADS 1024
#define MD17_WAVES (MD17_THREADS / 64)

// grid 1, MD17_THREADS threads.  acc[0] += sum_b |E_b - y_b| (difference in fp32, as torch forms it; a NaN propagates),
// acc[1] += B, acc[2] += sum_i |(-dE_i) - f_i| over i with -dE_i not NaN, acc[3] += the number of those i.  Per-thread fp64
// partials, a shuffle tree per wave, the 16 wave partials summed in order by thread 0: bitwise reproducible.
__global__ void __launch_bounds__(MD17_THREADS)
md17_eval_accumulate_kernel(const float* __restrict__ E, const float* __restrict__ y, int B, const float* __restrict__ dE,
                            const float* __restrict__ f, int n3, double* __restrict__ acc) {
  __shared__ double part[3][MD17_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double se = 0.0, sf = 0.0, nf = 0.0;
  for (int i = tid; i < B; i += MD17_THREADS) {
    const float r = E[i] - y[i];
    se += fabs((double)r);
  }
  for (int i = tid; i < n3; i += MD17_THREADS) {
    const float F = -dE[i];
    if (!isnan(F)) {
      const float r = F - f[i];
      sf += fabs((double)r);
      nf += 1.0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    se += __shfl_xor(se, o, 64);
    sf += __shfl_xor(sf, o, 64);
    nf += __shfl_xor(nf, o, 64);
  }
  if (lane == 0) {
    part[0][wave] = se;
    part[1][wave] = sf;
    part[2][wave] = nf;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0, c = 0.0;
    for (int w = 0; w < MD17_WAVES; ++w) {
      a += part[0][w];
      b += part[1][w];
      c += part[2][w];
    }
    acc[0] += a;
    acc[1] += (double)B;
    acc[2] += b;
    acc[3] += c;
  }
}

// The kernel of msde_l1_energy_force_loss (pointwise.hip), statement for statement, plus loss_acc[0] += loss.
__global__ void __launch_bounds__(1024)
md17_l1_energy_force_loss_acc_kernel(const float* __restrict__ E, const float* __restrict__ y, int B,
                                     const float* __restrict__ dE, const float* __restrict__ f, int n3, float fsign, float ce,
                                     float cf, float* __restrict__ loss, float* __restrict__ gE, float* __restrict__ gdE,
                                     double* __restrict__ loss_acc) {
  __shared__ float part[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float se = 0.f, sf = 0.f;
  const float we = ce / (float)max(B, 1), wf = cf / (float)max(n3, 1);
  for (int i = tid; i < B; i += 1024) {
    const float r = E[i] - y[i];
    se += fabsf(r);
    gE[i] = we * (r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f));
  }
  for (int i = tid; i < n3; i += 1024) {
    const float r = fsign * dE[i] - f[i];
    sf += fabsf(r);
    gdE[i] = wf * fsign * (r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { se += __shfl_down(se, o, 64); sf += __shfl_down(sf, o, 64); }
  if (lane == 0) { part[0][wave] = se; part[1][wave] = sf; }
  __syncthreads();
  if (tid == 0) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < 16; ++w) { a += part[0][w]; b += part[1][w]; }
    loss[0] = we * a + wf * b;
    loss_acc[0] += (double)loss[0];
  }
}

// grid 1, MD17_THREADS threads.  k = counter[0]; row r < B of the batch is split row j = k * stride + r, read through
// perm[j] when perm is given; rows with j >= M (past the end of the split) and permuted rows outside [0, M) are not read and
// leave their destination as it was.  pos_dst [B, row] / f_dst [B, row] (row = NA * 3 floats), y_dst [B].  After a barrier
// thread 0 writes counter[0] = k + 1 (every thread has read k by then; one workgroup, so no other reader).
__global__ void __launch_bounds__(MD17_THREADS)
md17_gather_batch_kernel(const float* __restrict__ pos, const float* __restrict__ y, const float* __restrict__ force, int M,
                         int row, const int* __restrict__ perm, int* __restrict__ counter, int stride, int B,
                         float* __restrict__ pos_dst, float* __restrict__ y_dst, float* __restrict__ f_dst) {
  const int tid = threadIdx.x;
  const int k = counter[0];
  const long long row0 = (long long)k * stride;
  const long long n = (long long)B * row;
  for (long long i = tid; i < n; i += MD17_THREADS) {
    const int r = (int)(i / row), c = (int)(i - (long long)r * row);
    const long long j = row0 + r;
    if (j < 0 || j >= M) continue;
    const long long s = perm ? (long long)perm[j] : j;
    if (s < 0 || s >= M) continue;
    pos_dst[i] = pos[s * row + c];
    if (f_dst) f_dst[i] = force[s * row + c];
  }
  for (int r = tid; r < B; r += MD17_THREADS) {
    const long long j = row0 + r;
    if (j < 0 || j >= M) continue;
    const long long s = perm ? (long long)perm[j] : j;
    if (s < 0 || s >= M) continue;
    y_dst[r] = y[s];
  }
  __syncthreads();
  if (tid == 0) counter[0] = k + 1;
}

extern "C" int msde_md17_eval_accumulate(const float* E, const float* y, int B, const float* dE, const float* f, int n3,
                                         double* acc, void* stream) {
  if (B <= 0 || n3 <= 0 || !E || !y || !dE || !f || !acc) return MSDE_EINVAL;
  MSDE_LAUNCH(md17_eval_accumulate_kernel, dim3(1), dim3(MD17_THREADS), 0, as_stream(stream), E, y, B, dE, f, n3, acc);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_l1_energy_force_loss_acc(const float* E, const float* y, int B, const float* dE, const float* f, int n3,
                                             float fsign, float ce, float cf, float* loss, float* gE, float* gdE,
                                             double* loss_acc, void* stream) {
  if (B <= 0 || n3 <= 0 || !E || !y || !dE || !f || !loss || !gE || !gdE || !loss_acc) return MSDE_EINVAL;
  MSDE_LAUNCH(md17_l1_energy_force_loss_acc_kernel, dim3(1), dim3(1024), 0, as_stream(stream), E, y, B, dE, f, n3, fsign, ce,
              cf, loss, gE, gdE, loss_acc);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_md17_gather_batch(const float* pos, const float* y, const float* force, int M, int row, const int* perm,
                                      int* counter, int stride, int B, float* pos_dst, float* y_dst, float* f_dst,
                                      void* stream) {
  if (M <= 0 || row <= 0 || B <= 0 || stride < B || !pos || !y || !counter || !pos_dst || !y_dst) return MSDE_EINVAL;
  if ((force == nullptr) != (f_dst == nullptr)) return MSDE_EINVAL;
  MSDE_LAUNCH(md17_gather_batch_kernel, dim3(1), dim3(MD17_THREADS), 0, as_stream(stream), pos, y, force, M, row, perm,
              counter, stride, B, pos_dst, y_dst, f_dst);
  MSDE_CHECK_LAUNCH();
  return 0;
}
