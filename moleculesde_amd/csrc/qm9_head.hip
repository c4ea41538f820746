// qm9_head.hip — the QM9 property-regression head (examples/finetune_QM9.py:145-171, :185-223): graph_pred_linear =
// Linear(D, 1) on the readout out [B, D], the target standardisation (y - TRAIN_mean) / TRAIN_std, the L1 (default) or MSE
// loss as a mean over B, and in the same launch the whole backward of the head: d out = dpred W, dW = sum_m dpred_m out_m,
// db = sum_m dpred_m.  The loss is the last node of the step, so nothing downstream waits for a second launch.
// One workgroup: B is a mini-batch (up to QH_MAX_B) and D <= QH_MAX_D.  Every sum runs in a fixed order, in fp64, without
// atomics: two launches on the same inputs are bitwise equal, and so are two replays of a captured step.
#include "msde_common.h"

#define QH_THREADS 1024
#define QH_MAX_B 8192
#define QH_MAX_D 1024
#define QH_L1 0
#define QH_MSE 1

// phase 1 (wave per row, lanes over D): pred_m = out_m . W + b in fp64, rounded to fp32 once; with W == NULL the prediction
// is out[m * ldo] itself (the loss-only form).
__device__ __forceinline__ void qh_predict(const float* __restrict__ out, int ldo, int B, int D, const float* __restrict__ W,
                                           const float* __restrict__ b, float* __restrict__ s_pred) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (!W) {
    for (int m = tid; m < B; m += QH_THREADS) s_pred[m] = out[(long long)m * ldo];
    return;
  }
  const double bias = b ? (double)b[0] : 0.0;
  for (int m = wave; m < B; m += QH_THREADS / 64) {
    const float* o = out + (long long)m * ldo;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) acc += (double)o[d] * (double)W[d];
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
    if (lane == 0) s_pred[m] = (float)(acc + bias);
  }
}

// grid 1, QH_THREADS threads, dynamic LDS B floats.
__global__ void __launch_bounds__(QH_THREADS)
qm9_head_train_kernel(const float* __restrict__ out, int ldo, int B, int D, const float* __restrict__ W,
                      const float* __restrict__ b, const float* __restrict__ y, int ldy, float mean, float stdv, int mode,
                      float* __restrict__ pred, float* __restrict__ loss, float* __restrict__ dout,
                      float* __restrict__ dW, float* __restrict__ db, double* __restrict__ loss_acc) {
  extern __shared__ float qh_lds[];
  float* s_pred = qh_lds;            // [B]: pred, then dpred
  __shared__ double r_loss[QH_THREADS], r_g[QH_THREADS];
  const int tid = threadIdx.x;
  qh_predict(out, ldo, B, D, W, b, s_pred);
  __syncthreads();
  // dpred exactly as torch's autograd forms it: mean backward 1 / B (fp32), times sign(diff) (sign(0) = 0) for L1,
  // times 2 diff for MSE
  const float invB = 1.0f / (float)B;
  double sl = 0.0, sg = 0.0;
  for (int m = tid; m < B; m += QH_THREADS) {
    const float p = s_pred[m];
    const float yh = (y[(long long)m * ldy] - mean) / stdv;
    const float df = p - yh;
    if (pred) pred[m] = p;
    float g;
    if (mode == QH_L1) {
      sl += fabs((double)df);
      g = df > 0.f ? invB : (df < 0.f ? -invB : 0.f);
    } else {
      sl += (double)df * (double)df;
      g = (2.0f * invB) * df;
    }
    sg += (double)g;
    s_pred[m] = g;                    // the row's own slot: no other thread reads it before the barrier
    if (!W) dout[m] = g;
  }
  r_loss[tid] = sl;
  r_g[tid] = sg;
  __syncthreads();
  for (int o = QH_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      r_loss[tid] += r_loss[tid + o];
      r_g[tid] += r_g[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float l = (float)(r_loss[0] / (double)B);
    if (loss) loss[0] = l;
    if (loss_acc) loss_acc[0] += (double)l;
    if (W && db) db[0] = (float)r_g[0];
  }
  if (!W) return;
  // dW[d] = sum_m dpred_m out[m][d]: one column per thread, rows in order (coalesced over d)
  for (int d = tid; d < D; d += QH_THREADS) {
    double acc = 0.0;
    for (int m = 0; m < B; ++m) acc += (double)s_pred[m] * (double)out[(long long)m * ldo + d];
    dW[d] = (float)acc;
  }
  // d out [B, D] = dpred (x) W
  const long long n = (long long)B * D;
  for (long long i = tid; i < n; i += QH_THREADS) {
    const int m = (int)(i / D), d = (int)(i - (long long)m * D);
    dout[i] = s_pred[m] * W[d];
  }
}

// grid 1, QH_THREADS threads, dynamic LDS B floats: pred_d = pred * std + mean (fp32, as the script de-standardises),
// acc[0] += sum_m |pred_d - y_m| and acc[1] += B, both fp64.
__global__ void __launch_bounds__(QH_THREADS)
qm9_head_eval_kernel(const float* __restrict__ out, int ldo, int B, int D, const float* __restrict__ W,
                     const float* __restrict__ b, const float* __restrict__ y, int ldy, float mean, float stdv,
                     float* __restrict__ pred, double* __restrict__ acc) {
  extern __shared__ float qh_lds[];
  __shared__ double r_abs[QH_THREADS];
  const int tid = threadIdx.x;
  qh_predict(out, ldo, B, D, W, b, qh_lds);
  __syncthreads();
  double s = 0.0;
  for (int m = tid; m < B; m += QH_THREADS) {
    const float p = qh_lds[m] * stdv + mean;
    if (pred) pred[m] = p;
    if (y) s += fabs((double)p - (double)y[(long long)m * ldy]);
  }
  r_abs[tid] = s;
  __syncthreads();
  for (int o = QH_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) r_abs[tid] += r_abs[tid + o];
    __syncthreads();
  }
  if (tid == 0 && acc) {
    acc[0] += r_abs[0];
    acc[1] += (double)B;
  }
}

extern "C" int msde_qm9_head_train(const float* out, int ldo, int B, int D, const float* W, const float* b, const float* y,
                                   int ldy, float mean, float std, int mode, float* pred, float* loss, float* dout, float* dW,
                                   float* db, double* loss_acc, void* stream) {
  if (B < 1 || !out || !y || ldy < 1 || !dout || (mode != QH_L1 && mode != QH_MSE)) return MSDE_EINVAL;
  if (W && (D < 1 || ldo < D || !dW || !db)) return MSDE_EINVAL;
  if (!W && (ldo < 1 || dW || db)) return MSDE_EINVAL;
  if (B > QH_MAX_B || (W && D > QH_MAX_D)) return MSDE_EUNSUP;
  MSDE_LAUNCH(qm9_head_train_kernel, dim3(1), dim3(QH_THREADS), (size_t)B * sizeof(float), as_stream(stream), out, ldo, B,
              W ? D : 1, W, b, y, ldy, mean, std, mode, pred, loss, dout, dW, db, loss_acc);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_qm9_head_eval(const float* out, int ldo, int B, int D, const float* W, const float* b, const float* y,
                                  int ldy, float mean, float std, float* pred, double* acc, void* stream) {
  if (B < 1 || !out || (y && ldy < 1) || (acc && !y)) return MSDE_EINVAL;
  if (W && (D < 1 || ldo < D)) return MSDE_EINVAL;
  if (!W && ldo < 1) return MSDE_EINVAL;
  if (B > QH_MAX_B || (W && D > QH_MAX_D)) return MSDE_EUNSUP;
  MSDE_LAUNCH(qm9_head_eval_kernel, dim3(1), dim3(QH_THREADS), (size_t)B * sizeof(float), as_stream(stream), out, ldo, B,
              W ? D : 1, W, b, y, ldy, mean, std, pred, acc);
  MSDE_CHECK_LAUNCH();
  return 0;
}
