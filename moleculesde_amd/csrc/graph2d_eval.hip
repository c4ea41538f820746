// graph2d_eval.hip — evaluation of the 3D->2D sampler's output: decode the generated float tensors (class scores x, adjacency
// values adj around `bond type + 1`) back into molecular graphs and compare them with the graph the 3D input came from
// (neither the reference scripts nor this tree had it; the conventions are those of conformer_rmsd.hip's COV / MAT).
//
// A launch holds G molecules; molecule g has n atoms and K generated samples (ragged, host-built int64 table, include/msde_hip.h).
//   (1) ge_decode_kernel: one workgroup of four waves per SAMPLE.  A wave takes atom i at a time: argmax over its ncls class
//       scores (lanes stride the classes, xor butterfly on (value, index), a tie goes to the lowest index), then the pairs (i, j)
//       of its row, lanes striding j: v = 0.5 ((double)a_ij + (double)a_ji) -- the fp64 sum of two fp32 numbers is exact and
//       commutative, so (i, j) and (j, i) see the same v -- and q = clamp(floor(v + 0.5), 0, max_bond).  Every pair is formed from
//       both of its rows (the bond-order sum of atom i needs the whole row), counted for j > i only.  Only flagged atoms and
//       pairs of flagged atoms are loaded at all.  The decoded classes and the upper triangle of codes are the sample's
//       SIGNATURE (uint8); the counts go to a 9-int record, sum |v - t| to a double.
//       Connected components of the decoded graph: min-label propagation, labels in LDS, the decoded codes read back from the
//       signature, swept until a sweep changes no label (each sweep also hops label -> label of that label, so a long path
//       does not take n sweeps; the fixed point -- every atom carries the lowest index of its component -- is unique, so the
//       result does not depend on the order in which the waves meet the labels).
//   (2) ge_summary_kernel: one workgroup per MOLECULE: which finite samples are the first with their signature (a wave per
//       sample, byte for byte against every earlier finite sample: no hashing), then the molecule's figures, summed over its
//       samples in index order by one thread.
// Integer counts are exact in any order; the two fp64 sums (a row's |v - t| over the lanes, the rows over a wave) run in a fixed
// order; no atomics.  A sample's outputs are a function of that sample and its molecule's targets alone.
#include "msde_common.h"

#define GE_MOL 8                   // int64 per molecule: n, K, x_off, adj_off, atom_off, tgt_off, samp_off, sig_off
#define GE_REC 9                   // int32 per sample: finite, atoms_correct, tp, fp, fn, order_correct, exact, components,
                                   //                   valence_violations
#define GE_STATS 11                // fp64 per molecule (include/msde_hip.h)
#define GE_NMAX 1024               // atoms per molecule: labels [n] int and row sums [n] double live in LDS (12 KiB)
#define GE_ACC 9                   // per-wave partial counts of the decode kernel

__device__ __forceinline__ int ge_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int ge_wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double ge_wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// element of pair (i, j), i < j, in the row-major upper triangle of an n x n matrix (n <= 1024: inside int)
__host__ __device__ inline int ge_tri(int n, int i, int j) { return i * n - i * (i + 1) / 2 + (j - i - 1); }

// bond-order contribution of code q in half-bond units: single 2, double 4, triple 6, aromatic 3, misc 2
__host__ __device__ inline int ge_half_bonds(int q) { return q == 0 ? 0 : q <= 3 ? 2 * q : q == 4 ? 3 : 2; }

// the molecule that owns record `s`: the last one whose offset word `w` is <= s (ascending; at most 31 steps)
__device__ __forceinline__ const long long* ge_find(const long long* __restrict__ mol, int G, int w, long long s) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mol[(size_t)mid * GE_MOL + w] <= s) lo = mid; else hi = mid - 1;
  }
  return mol + (size_t)lo * GE_MOL;
}

// ---- (1) one sample per workgroup ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ge_decode_kernel(const float* __restrict__ x_gen, const float* __restrict__ adj_gen,
                                                        const int* __restrict__ z, const unsigned char* __restrict__ adj_tgt,
                                                        const unsigned char* __restrict__ atom_flag,
                                                        const unsigned char* __restrict__ max_valence2,
                                                        const long long* __restrict__ mol, int G, int ncls, int max_bond,
                                                        unsigned char* sig, int* __restrict__ counts,
                                                        double* __restrict__ adj_l1) {
  __shared__ int sLab[GE_NMAX];
  __shared__ double sRow[GE_NMAX];
  __shared__ int sAcc[4][GE_ACC];
  __shared__ int sChanged;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long s = blockIdx.x;
  const long long* m = ge_find(mol, G, 6, s);
  const int n = (int)m[0];
  if (n > GE_NMAX) return;                                   // the host's n_max was wrong: write nothing rather than past LDS
  const long long k = s - m[6];
  const float* xs = x_gen + m[2] + k * n * ncls;
  const float* as = adj_gen + m[3] + k * n * n;
  const int* zt = z + m[4];
  const unsigned char* flag = atom_flag + m[4];
  const unsigned char* tgt = adj_tgt + m[5];
  const int L = n + n * (n - 1) / 2;
  unsigned char* sg = sig + m[7] + k * L;                    // classes [n], then codes [n (n - 1) / 2]
  unsigned char* sp = sg + n;

  // per-lane partial counts: flagged atoms, correct atoms, tp, fp, true bonds, correct orders, unequal pairs, valence
  // violations, non-finite values met
  int c_flag = 0, c_atom = 0, c_tp = 0, c_fp = 0, c_tb = 0, c_ord = 0, c_ne = 0, c_val = 0, c_bad = 0;
  for (int i = wave; i < n; i += 4) {
    if (flag[i] == 0) {                                      // the same for the whole wave: the atom takes part in nothing
      if (lane == 0) { sg[i] = 0; sLab[i] = -1; sRow[i] = 0.0; }
      for (int j = i + 1 + lane; j < n; j += 64) sp[ge_tri(n, i, j)] = 0;
      continue;
    }
    // atom class: argmax, the lowest index among equal values
    const float* xr = xs + (size_t)i * ncls;
    float bv = -__int_as_float(0x7f800000);
    int bi = 0x7fffffff;
    for (int c = lane; c < ncls; c += 64) {
      const float v = xr[c];
      if (!isfinite(v)) c_bad = 1;
      if (v > bv) { bv = v; bi = c; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((unsigned)bi >= (unsigned)ncls) bi = 0;              // a row without one finite score: the sample is dropped below
    // bond codes of row i
    int val2 = 0;
    double l1 = 0.0;
    for (int j = lane; j < n; j += 64) {
      if (j == i) continue;
      int q = 0;
      if (flag[j] != 0) {
        const float a = as[(size_t)i * n + j], b = as[(size_t)j * n + i];
        if (!(isfinite(a) && isfinite(b))) c_bad = 1;
        const double v = 0.5 * ((double)a + (double)b);
        const double f = floor(v + 0.5);
        q = f >= 1.0 ? (f >= (double)max_bond ? max_bond : (int)f) : 0;      // NaN: 0
        val2 += ge_half_bonds(q);
        if (j > i) {
          const int t = tgt[(size_t)i * n + j];
          c_tb += t > 0;
          c_tp += q > 0 && t > 0;
          c_fp += q > 0 && t == 0;
          c_ord += t > 0 && q == t;
          c_ne += q != t;
          l1 += fabs(v - (double)t);
        }
      }
      if (j > i) sp[ge_tri(n, i, j)] = (unsigned char)q;
    }
    val2 = ge_wave_sum(val2);
    l1 = ge_wave_sum_d(l1);
    if (lane == 0) {
      sg[i] = (unsigned char)bi;
      sLab[i] = i;
      sRow[i] = l1;
      c_flag += 1;
      c_atom += bi == zt[i];
      const int cap = max_valence2 ? max_valence2[bi] : 0;
      c_val += cap != 0 && val2 > cap;
    }
  }
  {
    const int r[GE_ACC] = {ge_wave_sum(c_flag), ge_wave_sum(c_atom), ge_wave_sum(c_tp),  ge_wave_sum(c_fp), ge_wave_sum(c_tb),
                           ge_wave_sum(c_ord),  ge_wave_sum(c_ne),   ge_wave_sum(c_val), ge_wave_sum(c_bad)};
    if (lane == 0)
      for (int e = 0; e < GE_ACC; ++e) sAcc[wave][e] = r[e];
  }
  __syncthreads();                                           // counts, labels, row sums and the signature are complete
  int t[GE_ACC];
  for (int e = 0; e < GE_ACC; ++e) t[e] = sAcc[0][e] + sAcc[1][e] + sAcc[2][e] + sAcc[3][e];
  int* rec = counts + s * GE_REC;
  if (t[8] != 0) {                                           // non-finite sample: an all-zero signature, nothing counted
    for (int e = tid; e < L; e += 256) sg[e] = 0;
    if (tid == 0) {
      rec[0] = 0; rec[1] = 0; rec[2] = 0; rec[3] = 0; rec[4] = t[4]; rec[5] = 0; rec[6] = 0; rec[7] = 0; rec[8] = 0;
      adj_l1[s] = __longlong_as_double(0x7ff8000000000000ll);
    }
    return;
  }
  // connected components of the decoded graph on the flagged atoms
  volatile int* lab = sLab;
  for (;;) {
    if (tid == 0) sChanged = 0;
    __syncthreads();
    for (int i = wave; i < n; i += 4) {
      if (flag[i] == 0) continue;
      const int li = lab[i];
      int mn = li;
      for (int j = lane; j < n; j += 64) {
        if (j == i || flag[j] == 0) continue;
        if (sp[j > i ? ge_tri(n, i, j) : ge_tri(n, j, i)] != 0) mn = min(mn, lab[j]);
      }
      mn = ge_wave_min(mn);
      if (lane == 0) {
        mn = min(mn, lab[mn]);                               // a label is the index of a flagged atom of the same component
        if (mn < li) { lab[i] = mn; sChanged = 1; }
      }
    }
    __syncthreads();
    const int again = sChanged;
    __syncthreads();                                         // everyone has read the flag before it is cleared again
    if (again == 0) break;
  }
  if (wave == 0) {
    int comps = 0;
    double tot = 0.0;
    for (int i = lane; i < n; i += 64) {
      comps += sLab[i] == i;                                 // unflagged atoms carry -1
      tot += sRow[i];
    }
    comps = ge_wave_sum(comps);
    tot = ge_wave_sum_d(tot);
    if (lane == 0) {
      rec[0] = 1; rec[1] = t[1]; rec[2] = t[2]; rec[3] = t[3]; rec[4] = t[4] - t[2]; rec[5] = t[5];
      rec[6] = t[1] == t[0] && t[6] == 0;
      rec[7] = comps; rec[8] = t[7];
      adj_l1[s] = tot;
    }
  }
}

// ---- (2) one molecule per workgroup -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ge_summary_kernel(const unsigned char* __restrict__ sig, const int* __restrict__ counts,
                                                         const double* __restrict__ adj_l1,
                                                         const unsigned char* __restrict__ atom_flag,
                                                         const long long* __restrict__ mol, unsigned char* __restrict__ first,
                                                         double* __restrict__ stats) {
  __shared__ int sFirst[4];
  __shared__ int sFlag;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long* m = mol + (size_t)blockIdx.x * GE_MOL;
  const int n = (int)m[0];
  const long long K = m[1], s0 = m[6];
  const long long L = n + n * (n - 1) / 2;
  const unsigned char* sg = sig + m[7];
  int firsts = 0;                                            // the same in every lane of the wave
  for (long long k = wave; k < K; k += 4) {
    int is_first = 0;
    if (counts[(s0 + k) * GE_REC] != 0) {
      is_first = 1;
      const unsigned char* a = sg + k * L;
      for (long long e = 0; e < k && is_first; ++e) {
        if (counts[(s0 + e) * GE_REC] == 0) continue;        // a non-finite sample is nobody's earlier copy
        const unsigned char* b = sg + e * L;
        int differs = 0;
        for (long long o = 0; o < L && !differs; o += 64)
          differs = __any(o + lane < L && a[o + lane] != b[o + lane]);
        if (!differs) is_first = 0;
      }
    }
    if (lane == 0) first[s0 + k] = (unsigned char)is_first;
    firsts += is_first;
  }
  if (lane == 0) sFirst[wave] = firsts;
  if (wave == 0) {
    int nf = 0;
    for (int i = lane; i < n; i += 64) nf += atom_flag[m[4] + i] != 0;
    nf = ge_wave_sum(nf);
    if (lane == 0) sFlag = nf;
  }
  __syncthreads();
  if (tid == 0) {                                            // the means: fp64, index order
    const int nf = sFlag;
    const long long pairs = (long long)nf * (nf - 1) / 2;
    double acc = 0.0, prec = 0.0, rcl = 0.0, f1 = 0.0, ord = 0.0, ex = 0.0, valid = 0.0, l1 = 0.0;
    long long fin = 0;
    int any = 0;
    for (long long k = 0; k < K; ++k) {
      const int* c = counts + (s0 + k) * GE_REC;
      if (c[0] == 0) continue;                               // stays in the denominator K, adds nothing
      const int tp = c[2], fp = c[3], fn = c[4];
      ++fin;
      acc += (double)c[1] / (double)nf;
      prec += tp + fp > 0 ? (double)tp / (double)(tp + fp) : 1.0;
      rcl += tp + fn > 0 ? (double)tp / (double)(tp + fn) : 1.0;
      f1 += 2 * tp + fp + fn > 0 ? (double)(2 * tp) / (double)(2 * tp + fp + fn) : 1.0;
      ord += tp > 0 ? (double)c[5] / (double)tp : 1.0;
      ex += (double)c[6];
      any |= c[6];
      valid += c[7] == 1 && c[8] == 0 ? 1.0 : 0.0;
      l1 += adj_l1[s0 + k];
    }
    const double dK = (double)K;
    double* o = stats + (size_t)blockIdx.x * GE_STATS;
    o[0] = acc / dK; o[1] = prec / dK; o[2] = rcl / dK; o[3] = f1 / dK; o[4] = ord / dK; o[5] = ex / dK; o[6] = valid / dK;
    o[7] = (double)(sFirst[0] + sFirst[1] + sFirst[2] + sFirst[3]) / dK;
    o[8] = (double)any;
    o[9] = fin > 0 ? l1 / (double)fin / (double)(pairs > 0 ? pairs : 1) : __longlong_as_double(0x7ff8000000000000ll);
    o[10] = (double)fin;
  }
}

extern "C" int msde_graph2d_decode(const float* x_gen, const float* adj_gen, const int* z, const unsigned char* adj_tgt,
                                   const unsigned char* atom_flag, const unsigned char* max_valence2, const long long* mol, int G,
                                   long long n_samples, int n_max, int ncls, int max_bond, unsigned char* sig, int* counts,
                                   double* adj_l1, void* stream) {
  if (!x_gen || !adj_gen || !z || !adj_tgt || !atom_flag || !mol || !sig || !counts || !adj_l1 || G <= 0 ||
      n_samples < (long long)G || n_max < 1 || ncls < 1 || max_bond < 1 || max_bond > 5)
    return MSDE_EINVAL;
  if (n_max > GE_NMAX || ncls > 256 || n_samples > 0x7fffffffll) return MSDE_EUNSUP;
  MSDE_LAUNCH(ge_decode_kernel, dim3((unsigned)n_samples), dim3(256), 0, as_stream(stream), x_gen, adj_gen, z, adj_tgt,
              atom_flag, max_valence2, mol, G, ncls, max_bond, sig, counts, adj_l1);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_graph2d_summary(const unsigned char* sig, const int* counts, const double* adj_l1,
                                    const unsigned char* atom_flag, const long long* mol, int G, unsigned char* first,
                                    double* stats, void* stream) {
  if (!sig || !counts || !adj_l1 || !atom_flag || !mol || !first || !stats || G <= 0) return MSDE_EINVAL;
  MSDE_LAUNCH(ge_summary_kernel, dim3((unsigned)G), dim3(256), 0, as_stream(stream), sig, counts, adj_l1, atom_flag, mol, first,
              stats);
  MSDE_CHECK_LAUNCH();
  return 0;
}
