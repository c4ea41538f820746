// dataset.hip — the feed of a pretraining epoch from a molecule store held on the device (Geom3D/datasets/dataset_3D.py:106-124
// per sample, then the loader's collate): batch k of a shuffled epoch is written straight into a capacity bucket's raw blob
// (moleculesde_amd/bucket.py: raw_layout / pack_raw), k read from a device counter, so that an epoch is a loop of graph
// replays with no per-batch host work.
//   dataset_gather_kernel    every workgroup reads the same B molecule sizes (perm[k * B + r]) in the same order, forms their
//                            exclusive prefix sums (integers: order-free, no atomics) and the validity of the whole batch; an
//                            invalid batch writes NOTHING to the blob and raises the gather's own error word.  A valid batch is
//                            written 16 bytes per thread over the WHOLE blob: each word is either a gathered value or zero, so
//                            no word keeps the previous batch's contents (pack_raw zero-fills; bit-identical blobs).
//   dataset_advance_kernel   counter[0] += 1 in a one-thread launch behind the gather: no workgroup of the gather reads a word
//                            another workgroup of the same launch writes (the counter protocol of dense_pc.hip / md17.hip).
// ~330 KB per batch of 256 molecules, no LDS staging of the payload.  Measured: 14 us per launch (0.6 % of the 2.5 ms step),
// more than the bytes suggest: every workgroup walks a chain of dependent loads (counter, permutation, pointer tables, payload)
// and the centring is a loop of n load-then-add steps per coordinate word; issuing those loads ahead of the adds is the
// obvious next step and has not been measured.
#include "msde_common.h"

#define DS_THREADS 256
#define DS_MAXB 1024
#define DS_K_ATOM 9

// error word bits (moleculesde_amd/dataset.py: GATHER_ERRORS)
#define DS_ERR_PERM 1       // a perm entry outside [0, M) (or a pointer table pointing outside the store)
#define DS_ERR_NMAX 2       // a molecule of more than n_max atoms (or an empty one)
#define DS_ERR_CAP 4        // atoms or bonds of the batch exceed their capacity
#define DS_ERR_SHORT 8      // fewer than B molecules remain in the epoch

struct DsArgs {
  const int* x;                 // [n_atoms, 9]
  const float* pos;             // [n_atoms, 3]
  const int* edge_index;        // [2, n_bonds], molecule-local
  const int* edge_attr;         // [n_bonds, 3]
  const long long* atom_ptr;    // [M + 1]
  const long long* bond_ptr;    // [M + 1]
  const int* perm;              // [n_avail]
  const int* counter;
  long long M, n_atoms, n_bonds, n_avail;
  int B, cap_N, cap_Eb, n_max, remove_center;
  int off_x, off_pos, off_src, off_dst, off_attr, off_atoms, off_bonds, total;
  int* blob;
  int* err;
};

// largest r in [0, B) with pre[r] <= i, for 0 <= i < pre[B] (molecules may hold zero bonds: pre[r] == pre[r + 1])
__device__ __forceinline__ int ds_find(const int* pre, int B, int i) {
  int lo = 0, hi = B;           // invariant: pre[lo] <= i < pre[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(DS_THREADS) dataset_gather_kernel(DsArgs a) {
  __shared__ int pre_a[DS_MAXB + 1], pre_b[DS_MAXB + 1];       // sizes, then exclusive prefix sums (atoms / bonds)
  __shared__ long long st_a[DS_MAXB], st_b[DS_MAXB];           // first atom / bond of molecule r in the store
  const int tid = threadIdx.x, B = a.B;
  const long long j0 = (long long)a.counter[0] * B;
  int bad = 0;
  for (int r = tid; r < B; r += DS_THREADS) {
    const long long j = j0 + r;
    int na = 0, nb = 0;
    long long sa = 0, sb = 0;
    if (j < 0 || j >= a.n_avail) {
      bad |= DS_ERR_SHORT;
    } else {
      const long long m = (long long)a.perm[j];
      if (m < 0 || m >= a.M) {
        bad |= DS_ERR_PERM;
      } else {
        sa = a.atom_ptr[m];
        sb = a.bond_ptr[m];
        const long long ea = a.atom_ptr[m + 1], eb = a.bond_ptr[m + 1];
        if (sa < 0 || ea > a.n_atoms || sb < 0 || eb > a.n_bonds || eb < sb) {
          bad |= DS_ERR_PERM;
        } else if (ea - sa < 1 || ea - sa > a.n_max) {
          bad |= DS_ERR_NMAX;
        } else if (eb - sb > a.cap_Eb) {
          bad |= DS_ERR_CAP;
        } else {
          na = (int)(ea - sa);
          nb = (int)(eb - sb);
        }
      }
    }
    pre_a[r] = na;
    pre_b[r] = nb;
    st_a[r] = sa;
    st_b[r] = sb;
  }
  __syncthreads();
  if (tid < 64) {
    // exclusive scan over B <= 1024 sizes by one wave: a contiguous chunk per lane, a shuffle scan over the 64 chunk sums.
    // (sums stay below 2^31: at most 1024 * n_max atoms, and every bond count was bounded by cap_Eb above)
    const int chunk = (B + 63) >> 6, lo = min(tid * chunk, B), hi = min(lo + chunk, B);
    long long sa = 0, sb = 0;
    for (int r = lo; r < hi; ++r) { sa += pre_a[r]; sb += pre_b[r]; }
    long long ia = sa, ib = sb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
      if (tid >= o) { ia += ua; ib += ub; }
    }
    long long ra = ia - sa, rb = ib - sb;
    if (tid == 63 && (ia > a.cap_N || ib > a.cap_Eb)) bad |= DS_ERR_CAP;
    for (int r = lo; r < hi; ++r) {
      const int ca = pre_a[r], cb = pre_b[r];
      pre_a[r] = (int)min(ra, (long long)0x7fffffff);
      pre_b[r] = (int)min(rb, (long long)0x7fffffff);
      ra += ca;
      rb += cb;
    }
    if (tid == 63) {
      pre_a[B] = (int)min(ia, (long long)0x7fffffff);
      pre_b[B] = (int)min(ib, (long long)0x7fffffff);
    }
  }
  if (__syncthreads_or(bad)) {
    // all or nothing: every workgroup derived the same verdict from the same sizes; the blob keeps the previous batch.  The
    // error word is sticky until the host clears it; one writer (thread 0 of workgroup 0), one barrier vote per bit
    int bits = 0;
#pragma unroll
    for (int b = 1; b <= DS_ERR_SHORT; b <<= 1)
      if (__syncthreads_or(bad & b)) bits |= b;
    if (blockIdx.x == 0 && tid == 0) a.err[0] = a.err[0] | bits;
    return;
  }
  const int N = pre_a[B], E = pre_b[B];
  const int n4 = a.total >> 2;
  for (int q = blockIdx.x * DS_THREADS + tid; q < n4; q += gridDim.x * DS_THREADS) {
    const int w0 = q << 2;
    int v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int w = w0 + c;
      int out = 0;
      if (w >= a.off_bonds) {                       // mol_bonds [B]
        const int r = w - a.off_bonds;
        if (r < B) out = pre_b[r + 1] - pre_b[r];
      } else if (w >= a.off_atoms) {                // mol_atoms [B]
        const int r = w - a.off_atoms;
        if (r < B) out = pre_a[r + 1] - pre_a[r];
      } else if (w >= a.off_attr) {                 // bond_attr [E, 3]: a molecule's rows are contiguous in the store
        const int i = w - a.off_attr, e = i / 3;
        if (e < E) {
          const int r = ds_find(pre_b, B, e);
          out = a.edge_attr[st_b[r] * 3 + (i - pre_b[r] * 3)];
        }
      } else if (w >= a.off_src) {                  // bond_src [cap_Eb] | bond_dst [cap_Eb]: local index + atom offset
        const int row = w >= a.off_dst ? 1 : 0, e = w - (row ? a.off_dst : a.off_src);
        if (e < E) {
          const int r = ds_find(pre_b, B, e);
          out = a.edge_index[(long long)row * a.n_bonds + st_b[r] + (e - pre_b[r])] + pre_a[r];
        }
      } else if (w >= a.off_pos) {                  // pos [N, 3] as fp32 bit patterns
        const int i = w - a.off_pos, at = i / 3;
        if (at < N) {
          const int r = ds_find(pre_a, B, at), ax = i - at * 3;
          const float* p = a.pos + st_a[r] * 3;
          float val = p[i - pre_a[r] * 3];
          if (a.remove_center) {
            // dataset_3D.py:120-122: the mean over the molecule's atoms, summed in atom order in fp64, divided in fp64,
            // rounded to fp32, subtracted in fp32 (MoleculeStore.centred_positions does the same arithmetic)
            const int n = pre_a[r + 1] - pre_a[r];
            double s = 0.0;
            for (int t = 0; t < n; ++t) s += (double)p[t * 3 + ax];
            val = val - (float)(s / (double)n);
          }
          out = __float_as_int(val);
        }
      } else {                                      // x [N, 9]
        const int i = w - a.off_x, at = i / DS_K_ATOM;
        if (w >= a.off_x && at < N) {
          const int r = ds_find(pre_a, B, at);
          out = a.x[st_a[r] * DS_K_ATOM + (i - pre_a[r] * DS_K_ATOM)];
        }
      }
      v[c] = out;
    }
    reinterpret_cast<int4*>(a.blob)[q] = make_int4(v[0], v[1], v[2], v[3]);
  }
}

__global__ void dataset_advance_kernel(int* counter) { counter[0] = counter[0] + 1; }

extern "C" int msde_dataset_gather_batch(const int* x, const float* pos, const int* edge_index, const int* edge_attr,
                                         const long long* atom_ptr, const long long* bond_ptr, long long M, long long n_atoms,
                                         long long n_bonds, const int* perm, int* counter, long long n_avail, int B, int cap_N,
                                         int cap_Eb, int n_max, int remove_center, int off_x, int off_pos, int off_src,
                                         int off_dst, int off_attr, int off_atoms, int off_bonds, int total_words, int* blob,
                                         int* err, void* stream) {
  if (!x || !pos || !atom_ptr || !bond_ptr || !perm || !counter || !blob || !err) return MSDE_EINVAL;
  if (n_bonds > 0 && (!edge_index || !edge_attr)) return MSDE_EINVAL;
  if (M <= 0 || n_atoms <= 0 || n_bonds < 0 || n_avail < 0 || B <= 0 || B > DS_MAXB || n_max <= 0) return MSDE_EINVAL;
  if (cap_N <= 0 || cap_Eb < 0 || (long long)B * n_max > 0x7fffffffLL) return MSDE_EINVAL;
  // the layout of bucket.raw_layout: fields in this order, each starting on a 16-byte boundary and holding its capacity
  const long long sz[7] = {(long long)cap_N * DS_K_ATOM, (long long)cap_N * 3, cap_Eb, cap_Eb, (long long)cap_Eb * 3, B, B};
  const int off[8] = {off_x, off_pos, off_src, off_dst, off_attr, off_atoms, off_bonds, total_words};
  if (off_x < 0 || (total_words & 3)) return MSDE_EINVAL;
  for (int i = 0; i < 7; ++i)
    if ((off[i] & 3) || (long long)off[i] + sz[i] > (long long)off[i + 1]) return MSDE_EINVAL;
  if (off_x != 0) return MSDE_EINVAL;       // (every word of [0, total_words) belongs to a field or its padding)
  if (reinterpret_cast<uintptr_t>(blob) & 15) return MSDE_EINVAL;
  DsArgs a;
  a.x = x; a.pos = pos; a.edge_index = edge_index; a.edge_attr = edge_attr; a.atom_ptr = atom_ptr; a.bond_ptr = bond_ptr;
  a.perm = perm; a.counter = counter; a.M = M; a.n_atoms = n_atoms; a.n_bonds = n_bonds; a.n_avail = n_avail;
  a.B = B; a.cap_N = cap_N; a.cap_Eb = cap_Eb; a.n_max = n_max; a.remove_center = remove_center;
  a.off_x = off_x; a.off_pos = off_pos; a.off_src = off_src; a.off_dst = off_dst; a.off_attr = off_attr;
  a.off_atoms = off_atoms; a.off_bonds = off_bonds; a.total = total_words; a.blob = blob; a.err = err;
  const int n4 = total_words >> 2;
  int grid = (n4 + DS_THREADS - 1) / DS_THREADS;
  grid = grid < 1 ? 1 : (grid > 2 * msde_num_cus() ? 2 * msde_num_cus() : grid);
  MSDE_LAUNCH(dataset_gather_kernel, dim3(grid), dim3(DS_THREADS), 0, as_stream(stream), a);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(dataset_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), counter);
  MSDE_CHECK_LAUNCH();
  return 0;
}
