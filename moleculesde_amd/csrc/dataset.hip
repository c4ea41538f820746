// dataset.hip — the feed of a pretraining epoch from a molecule store held on the device (Geom3D/datasets/dataset_3D.py:106-124
// per sample, then the loader's collate): batch k of a shuffled epoch is written straight into a capacity bucket's raw blob
// (moleculesde_amd/bucket.py: raw_layout / pack_raw), k read from a device counter, so that an epoch is a loop of graph
// replays with no per-batch host work.
//   dataset_gather_kernel<MASKED>  ONE kernel in two forms: whole molecules (<false>) or, under sub-graph masking
//                            (--SSL_masking_ratio), the atoms a per-epoch keep word names and the bonds between them (<true>).
//                            Every workgroup reads the same B molecule sizes (perm[k * B + r]) in the same order, forms their
//                            exclusive prefix sums (integers: order-free, no atomics) and the validity of the whole batch; an
//                            invalid batch writes NOTHING and raises the gather's own error word.  A valid batch is written 16
//                            bytes per thread over the WHOLE blob: each word is either a gathered value or zero, so no word
//                            keeps the previous batch's contents (pack_raw zero-fills; bit-identical blobs).  The guards, the
//                            scan, the verdict and the walk over the blob's fields are the same code in both forms; the masked
//                            form differs where `if constexpr (MASKED)` says so: sizes are kept counts, the k-th atom is the
//                            k-th set bit of the keep word, the q-th bond is found by walking the molecule's stored bonds (a
//                            few dozen, cached) eight at a time, going on from the bond the thread's previous word found, the
//                            centre is taken over the kept atoms, and ext_in is written behind the blob.
//   dataset_advance_kernel   counter[0] += 1 in a one-thread launch behind the gather: no workgroup of the gather reads a word
//                            another workgroup of the same launch writes (the counter protocol of dense_pc.hip / md17.hip).
//   dataset_ext_rows_kernel, dataset_mask_epoch_kernel   what the masked form reads: whole-molecule extended rows (once per
//                            store) and the keep words (once per epoch); second half of this file.
// ~330 KB per batch of 256 molecules, no LDS staging of the payload.  Measured (16 384 molecules, batch 256, back-to-back
// launches, gather + advance): 14.9 us unmasked (14 us per launch inside the 2.5 ms step, 0.6 % of it), 26.9 us masked; more
// than the bytes suggest: every workgroup walks a chain of dependent loads (counter, permutation, pointer tables, payload) and
// the centring is a loop of n load-then-add steps per coordinate word; issuing those loads ahead of the adds is the obvious
// next step and has not been measured.
#include "msde_common.h"

#define DS_THREADS 256
#define DS_MAXB 1024
#define DS_K_ATOM 9

// error word bits (moleculesde_amd/dataset.py: GATHER_ERRORS)
#define DS_ERR_PERM 1       // a perm entry outside [0, M) (or a pointer table pointing outside the store)
#define DS_ERR_NMAX 2       // a molecule of more than n_max atoms (or an empty one; masked: of more than 32 atoms)
#define DS_ERR_CAP 4        // atoms or bonds of the batch exceed their capacity
#define DS_ERR_SHORT 8      // fewer than B molecules remain in the epoch
#define DS_ERR_KEEP 16      // masked only: a keep word that is zero or has bits at or above the molecule's atom count

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

// what the masked form takes on top.  A molecule of <= 32 atoms is one 32-bit word wherever a set of its atoms is meant
struct DsMaskArgs {
  const unsigned* keep;         // [M]
  const unsigned* mol_rows;     // [n_atoms]
  unsigned* ext_in;             // [cap_N]
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

// ---- bit-word helpers of the masked form (ds_full and ds_nth_bit also serve dataset_mask_epoch_kernel)
__device__ __forceinline__ unsigned ds_full(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }

// position of the j-th (0-based) set bit of w; 0 <= j < popc(w)
__device__ __forceinline__ int ds_nth_bit(unsigned w, int j) {
  for (int k = 0; k < j; ++k) w &= w - 1u;
  return __ffs(w) - 1;
}

__device__ __forceinline__ bool ds_bond_kept(int s, int d, unsigned kw) {
  return (unsigned)s < 32u && (unsigned)d < 32u && (((kw >> s) & (kw >> d)) & 1u);
}

// bits of row compressed to the positions its bits hold among the set bits of kw (row is a subset of kw)
__device__ __forceinline__ unsigned ds_compress(unsigned row, unsigned kw) {
  unsigned out = 0u;
  int c = 0;
  for (unsigned k = kw; k; k &= k - 1u, ++c)
    if (row & k & (0u - k)) out |= 1u << c;
  return out;
}

// kept flags (bit u) of the stored bonds f0 + u, u < 8, below f1 (f0 < f1): sixteen independent loads, then the tests -- a
// load-test-branch loop over the bonds costs a memory round trip per bond
#define DS_CHUNK 8
__device__ __forceinline__ unsigned ds_kept_chunk(const int* __restrict__ edge_index, long long n_bonds, long long f0,
                                                  long long f1, unsigned kw) {
  int s[DS_CHUNK], d[DS_CHUNK];
#pragma unroll
  for (int u = 0; u < DS_CHUNK; ++u) {
    const long long f = min(f0 + u, f1 - 1);
    s[u] = edge_index[f];
    d[u] = edge_index[n_bonds + f];
  }
  unsigned mask = 0u;
#pragma unroll
  for (int u = 0; u < DS_CHUNK; ++u)
    if (f0 + u < f1 && ds_bond_kept(s[u], d[u], kw)) mask |= 1u << u;
  return mask;
}

// store index of the q-th (0-based) kept bond among the stored bonds [f0, f1); f1 if there are not that many
__device__ __forceinline__ long long ds_kept_bond(const int* __restrict__ edge_index, long long n_bonds, long long f0,
                                                  long long f1, unsigned kw, int q) {
  for (long long f = f0; f < f1; f += DS_CHUNK) {
    const unsigned mask = ds_kept_chunk(edge_index, n_bonds, f, f1, kw);
    const int c = __popc(mask);
    if (q < c) return f + ds_nth_bit(mask, q);
    q -= c;
  }
  return f1;
}

// the kept bond (r, q) for the consecutive words of one thread: the words of a thread name the same or the next few kept
// bonds of one molecule, so the walk goes on from the bond found last instead of starting over
struct DsBondCursor {
  int r, q;
  long long f;
};
__device__ __forceinline__ long long ds_cursor_find(DsBondCursor& c, const int* __restrict__ edge_index, long long n_bonds,
                                                    long long sb, int m, unsigned kw, int r, int q) {
  if (c.r == r && q == c.q) return c.f;
  if (c.r == r && q > c.q && c.f < sb + m) c.f = ds_kept_bond(edge_index, n_bonds, c.f + 1, sb + m, kw, q - c.q - 1);
  else c.f = ds_kept_bond(edge_index, n_bonds, sb, sb + m, kw, q);
  c.r = r;
  c.q = q;
  return c.f;
}

// MASKED false: k is not read, and what only the masked form needs (all_b, kw_s, the bond cursor, the DS_ERR_KEEP vote) is
// compiled out: the same registers and LDS as a kernel written without it
template <bool MASKED>
__global__ void __launch_bounds__(DS_THREADS) dataset_gather_kernel(DsArgs a, DsMaskArgs k) {
  __shared__ int pre_a[DS_MAXB + 1], pre_b[DS_MAXB + 1];       // sizes as written, then exclusive prefix sums (atoms / bonds)
  __shared__ long long st_a[DS_MAXB], st_b[DS_MAXB];           // first atom / bond of molecule r in the store
  __shared__ int all_b[MASKED ? DS_MAXB : 1];                  // masked: stored bonds of molecule r
  __shared__ unsigned kw_s[MASKED ? DS_MAXB : 1];              // masked: keep word of molecule r
  const int tid = threadIdx.x, B = a.B;
  const long long j0 = (long long)a.counter[0] * B;
  int bad = 0;
  for (int r = tid; r < B; r += DS_THREADS) {
    const long long j = j0 + r;
    int na = 0, nb = 0, mb = 0;
    long long sa = 0, sb = 0;
    unsigned kw = 0u;
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
        if (sa < 0 || ea > a.n_atoms || sb < 0 || eb > a.n_bonds || eb < sb || (MASKED && eb - sb > 0x7fffffffLL)) {
          bad |= DS_ERR_PERM;
        } else if (ea - sa < 1 || ea - sa > a.n_max || (MASKED && ea - sa > 32)) {
          bad |= DS_ERR_NMAX;
        } else {
          if constexpr (MASKED) kw = k.keep[m];
          if (MASKED && (kw == 0u || (kw & ~ds_full((int)(ea - sa))))) {
            bad |= DS_ERR_KEEP;
            kw = 0u;
          } else {
            long long cnt = eb - sb;                // bonds written: all of them, or those with both ends kept
            if constexpr (MASKED) {
              cnt = 0;
              for (long long f = sb; f < eb; f += DS_CHUNK) cnt += __popc(ds_kept_chunk(a.edge_index, a.n_bonds, f, eb, kw));
            }
            if (cnt > a.cap_Eb) {
              bad |= DS_ERR_CAP;
            } else {
              na = MASKED ? __popc(kw) : (int)(ea - sa);
              nb = (int)cnt;
              mb = (int)(eb - sb);
            }
          }
        }
      }
    }
    pre_a[r] = na;
    pre_b[r] = nb;
    st_a[r] = sa;
    st_b[r] = sb;
    if constexpr (MASKED) {
      all_b[r] = mb;
      kw_s[r] = kw;
    }
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
    // all or nothing: every workgroup derived the same verdict from the same sizes; the blob (and ext_in) keeps the previous
    // batch.  The error word is sticky until the host clears it; one writer (thread 0 of workgroup 0), one barrier vote per bit
    int bits = 0;
#pragma unroll
    for (int b = 1; b <= (MASKED ? DS_ERR_KEEP : DS_ERR_SHORT); b <<= 1)
      if (__syncthreads_or(bad & b)) bits |= b;
    if (blockIdx.x == 0 && tid == 0) a.err[0] = a.err[0] | bits;
    return;
  }
  const int N = pre_a[B], E = pre_b[B];
  const int n4 = a.total >> 2;
  for (int q = blockIdx.x * DS_THREADS + tid; q < n4; q += gridDim.x * DS_THREADS) {
    const int w0 = q << 2;
    int v[4];
    DsBondCursor cur;                               // (masked only)
    cur.r = -1; cur.q = 0; cur.f = 0;
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
      } else if (w >= a.off_attr) {                 // bond_attr [E, 3]
        const int i = w - a.off_attr, e = i / 3;
        if (e < E) {
          const int r = ds_find(pre_b, B, e);
          long long f = st_b[r] + (e - pre_b[r]);   // a molecule's bonds are contiguous in the store; masked: its KEPT bonds,
          bool have = true;                         // in stored order
          if constexpr (MASKED) {
            f = ds_cursor_find(cur, a.edge_index, a.n_bonds, st_b[r], all_b[r], kw_s[r], r, e - pre_b[r]);
            have = f < st_b[r] + all_b[r];
          }
          if (have) out = a.edge_attr[f * 3 + (i - e * 3)];
        }
      } else if (w >= a.off_src) {                  // bond_src [cap_Eb] | bond_dst [cap_Eb]: local index + atom offset
        const int row = w >= a.off_dst ? 1 : 0, e = w - (row ? a.off_dst : a.off_src);
        if (e < E) {
          const int r = ds_find(pre_b, B, e);
          long long f = st_b[r] + (e - pre_b[r]);
          bool have = true;
          unsigned kw = 0u;
          if constexpr (MASKED) {
            kw = kw_s[r];
            f = ds_cursor_find(cur, a.edge_index, a.n_bonds, st_b[r], all_b[r], kw, r, e - pre_b[r]);
            have = f < st_b[r] + all_b[r];
          }
          if (have) {
            int local = a.edge_index[(long long)row * a.n_bonds + f];
            if constexpr (MASKED) local = __popc(kw & ((1u << local) - 1u));      // rank among the kept atoms (0 <= local < 32)
            out = local + pre_a[r];
          }
        }
      } else if (w >= a.off_pos) {                  // pos [N, 3] as fp32 bit patterns
        const int i = w - a.off_pos, at = i / 3;
        if (at < N) {
          const int r = ds_find(pre_a, B, at), ax = i - at * 3;
          const float* p = a.pos + st_a[r] * 3;
          unsigned kw = 0u;
          int t = at - pre_a[r];                    // the molecule's t-th atom; masked: its t-th KEPT atom
          if constexpr (MASKED) {
            kw = kw_s[r];
            t = ds_nth_bit(kw, t);
          }
          float val = p[t * 3 + ax];
          if (a.remove_center) {
            // dataset_3D.py:120-122, after the masking: the mean over the molecule's (kept) atoms, summed in atom order in
            // fp64, divided in fp64, rounded to fp32, subtracted in fp32 (MoleculeStore.centred_positions: same arithmetic)
            double s = 0.0;
            int n;
            if constexpr (MASKED) {
              n = __popc(kw);
              for (unsigned kk = kw; kk; kk &= kk - 1u) s += (double)p[(__ffs(kk) - 1) * 3 + ax];
            } else {
              n = pre_a[r + 1] - pre_a[r];
              for (int u = 0; u < n; ++u) s += (double)p[u * 3 + ax];
            }
            val = val - (float)(s / (double)n);
          }
          out = __float_as_int(val);
        }
      } else {                                      // x [N, 9]
        const int i = w - a.off_x, at = i / DS_K_ATOM;
        if (w >= a.off_x && at < N) {
          const int r = ds_find(pre_a, B, at);
          int t = at - pre_a[r];
          if constexpr (MASKED) t = ds_nth_bit(kw_s[r], t);
          out = a.x[(st_a[r] + t) * DS_K_ATOM + (i - at * DS_K_ATOM)];
        }
      }
      v[c] = out;
    }
    reinterpret_cast<int4*>(a.blob)[q] = make_int4(v[0], v[1], v[2], v[3]);
  }
  if constexpr (MASKED) {
    // ext_in [cap_N]: the whole-molecule row of each kept atom, restricted to the kept atoms, in the new numbering
    for (int at = blockIdx.x * DS_THREADS + tid; at < a.cap_N; at += gridDim.x * DS_THREADS) {
      unsigned out = 0u;
      if (at < N) {
        const int r = ds_find(pre_a, B, at);
        const unsigned kw = kw_s[r];
        out = ds_compress(k.mol_rows[st_a[r] + ds_nth_bit(kw, at - pre_a[r])] & kw, kw);
      }
      k.ext_in[at] = out;
    }
  }
}

__global__ void dataset_advance_kernel(int* counter) { counter[0] = counter[0] + 1; }

// argument checks and the argument block of the gather (returns 0 or MSDE_EINVAL)
static int ds_make_args(const int* x, const float* pos, const int* edge_index, const int* edge_attr, const long long* atom_ptr,
                        const long long* bond_ptr, long long M, long long n_atoms, long long n_bonds, const int* perm,
                        int* counter, long long n_avail, int B, int cap_N, int cap_Eb, int n_max, int remove_center, int off_x,
                        int off_pos, int off_src, int off_dst, int off_attr, int off_atoms, int off_bonds, int total_words,
                        int* blob, int* err, DsArgs* out) {
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
  *out = a;
  return 0;
}

static int ds_grid(int total_words) {
  const int n4 = total_words >> 2;
  const int grid = (n4 + DS_THREADS - 1) / DS_THREADS;
  return grid < 1 ? 1 : (grid > 2 * msde_num_cus() ? 2 * msde_num_cus() : grid);
}

// the gather in its unmasked (k == nullptr) or masked form, then the counter's own launch behind it
static int ds_launch(const DsArgs& a, const DsMaskArgs* k, int* counter, hipStream_t stream) {
  const dim3 grid(ds_grid(a.total)), block(DS_THREADS);
  if (k) MSDE_LAUNCH(dataset_gather_kernel<true>, grid, block, 0, stream, a, *k);
  else MSDE_LAUNCH(dataset_gather_kernel<false>, grid, block, 0, stream, a, DsMaskArgs());
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(dataset_advance_kernel, dim3(1), dim3(1), 0, stream, counter);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_dataset_gather_batch(const int* x, const float* pos, const int* edge_index, const int* edge_attr,
                                         const long long* atom_ptr, const long long* bond_ptr, long long M, long long n_atoms,
                                         long long n_bonds, const int* perm, int* counter, long long n_avail, int B, int cap_N,
                                         int cap_Eb, int n_max, int remove_center, int off_x, int off_pos, int off_src,
                                         int off_dst, int off_attr, int off_atoms, int off_bonds, int total_words, int* blob,
                                         int* err, void* stream) {
  DsArgs a;
  const int rc = ds_make_args(x, pos, edge_index, edge_attr, atom_ptr, bond_ptr, M, n_atoms, n_bonds, perm, counter, n_avail, B,
                              cap_N, cap_Eb, n_max, remove_center, off_x, off_pos, off_src, off_dst, off_attr, off_atoms,
                              off_bonds, total_words, blob, err, &a);
  return rc ? rc : ds_launch(a, nullptr, counter, as_stream(stream));
}

extern "C" int msde_dataset_gather_batch_masked(const int* x, const float* pos, const int* edge_index, const int* edge_attr,
                                                const long long* atom_ptr, const long long* bond_ptr, long long M,
                                                long long n_atoms, long long n_bonds, const int* perm, int* counter,
                                                long long n_avail, int B, int cap_N, int cap_Eb, int n_max, int remove_center,
                                                int off_x, int off_pos, int off_src, int off_dst, int off_attr, int off_atoms,
                                                int off_bonds, int total_words, const unsigned* keep, const unsigned* mol_rows,
                                                int* blob, unsigned* ext_in, int* err, void* stream) {
  if (!keep || !mol_rows || !ext_in) return MSDE_EINVAL;
  DsArgs a;
  const int rc = ds_make_args(x, pos, edge_index, edge_attr, atom_ptr, bond_ptr, M, n_atoms, n_bonds, perm, counter, n_avail, B,
                              cap_N, cap_Eb, n_max, remove_center, off_x, off_pos, off_src, off_dst, off_attr, off_atoms,
                              off_bonds, total_words, blob, err, &a);
  if (rc) return rc;
  DsMaskArgs k;
  k.keep = keep; k.mol_rows = mol_rows; k.ext_in = ext_in;
  return ds_launch(a, &k, counter, as_stream(stream));
}

// ------------------------------------------------------------------------------------------------ sub-graph masking
// Geom3D/datasets/dataset_3D.py:53-104 (`subgraph`, --SSL_masking_ratio), between extend_graph (:114-115) and the centring
// (:120-122): what dataset_gather_kernel<true> reads.
//   dataset_ext_rows_kernel     once per store: the whole molecule's <= 4-bond neighbourhood rows (plan_molecule_kernel's two
//                               rounds on the stored bonds).  The masked molecule's extended edges are THESE restricted to the
//                               kept atoms (:95-102), not what the kept bonds span.
//   dataset_mask_epoch_kernel   once per epoch: the random BFS of :58-70 as bit-mask arithmetic, one wave per molecule (lane i
//                               holds the out-neighbours of atom i; every lane walks the same draws, no atomics).  The draws are
//                               counter based and integer only (the loop below): moleculesde_amd/dataset.py bfs_keep mirrors them.
// Measured (16 384 molecules): the mask kernel 35 us per epoch (2.1 ms per million molecules).
#define DS_EPOCH_MIX 0xD1B54A32D192ED69ull

// lane i < n of a wave: the out-neighbours of atom i over the molecule's m stored bonds (every lane reads every bond: the
// loads are wave uniform); other lanes 0
__device__ __forceinline__ unsigned ds_bond_row(const int* __restrict__ edge_index, long long n_bonds, long long sb, long long m,
                                                int n, int lane) {
  unsigned row = 0u;
  for (long long e = 0; e < m; ++e) {
    const int s = edge_index[sb + e], d = edge_index[n_bonds + sb + e];
    if (s == lane && d >= 0 && d < n) row |= 1u << d;
  }
  return lane < n ? row : 0u;
}

// the molecule of this wave (4 per workgroup) and its checked span; false: nothing to do for it
__device__ __forceinline__ bool ds_wave_molecule(const long long* __restrict__ atom_ptr, const long long* __restrict__ bond_ptr,
                                                 long long M, long long n_atoms, long long n_bonds, long long* m, long long* sa,
                                                 long long* n, long long* sb, long long* nb) {
  *m = (long long)blockIdx.x * (DS_THREADS / 64) + (threadIdx.x >> 6);
  if (*m >= M) return false;
  *sa = atom_ptr[*m];
  *sb = bond_ptr[*m];
  const long long ea = atom_ptr[*m + 1], eb = bond_ptr[*m + 1];
  *n = ea - *sa;
  *nb = eb - *sb;
  return !(*sa < 0 || ea > n_atoms || *n < 1 || *sb < 0 || eb > n_bonds || *nb < 0);
}

__global__ void __launch_bounds__(DS_THREADS)
dataset_ext_rows_kernel(const int* __restrict__ edge_index, const long long* __restrict__ atom_ptr,
                        const long long* __restrict__ bond_ptr, long long M, long long n_atoms, long long n_bonds,
                        unsigned* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  long long m, sa, n, sb, nb;
  if (!ds_wave_molecule(atom_ptr, bond_ptr, M, n_atoms, n_bonds, &m, &sa, &n, &sb, &nb)) return;
  if (n > 32) {                                   // never gathered on the device: zero rows
    for (long long i = lane; i < n; i += 64) rows[sa + i] = 0u;
    return;
  }
  unsigned row = ds_bond_row(edge_index, n_bonds, sb, nb, (int)n, lane);
  const unsigned self = 1u << (lane & 31);
  // extend_graph: two rounds of  A <- A | (A.A minus the diagonal); the loop is wave uniform (every lane takes part in the
  // shuffles), lanes >= n hold empty rows
  for (int round = 0; round < 2; ++round) {
    unsigned acc = 0u;
    for (int k = 0; k < (int)n; ++k) {
      const unsigned rk = __shfl(row, k, 64);
      if ((row >> k) & 1u) acc |= rk;
    }
    row |= acc & ~self;
  }
  if (lane < n) rows[sa + lane] = row & ~self;
}

__global__ void __launch_bounds__(DS_THREADS)
dataset_mask_epoch_kernel(const int* __restrict__ edge_index, const long long* __restrict__ atom_ptr,
                          const long long* __restrict__ bond_ptr, long long M, long long n_atoms, long long n_bonds,
                          unsigned long long seed_e, const int* __restrict__ keep_count, unsigned* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  long long m, sa, n, sb, nb;
  const bool ok = ds_wave_molecule(atom_ptr, bond_ptr, M, n_atoms, n_bonds, &m, &sa, &n, &sb, &nb);
  if (m >= M) return;
  unsigned kept = 0u;
  if (ok && n <= 32) {
    const unsigned row = ds_bond_row(edge_index, n_bonds, sb, nb, (int)n, lane);
    const unsigned full = ds_full((int)n);
    const int target = min(max(keep_count[n], 1), (int)n);
    const unsigned long long key = msde_mix64(seed_e, (unsigned long long)m);
    unsigned frontier = 0u;
    for (int d = 0; d < target; ++d) {            // (wave uniform: every lane walks the same draws)
      const unsigned set = frontier ? frontier : (full & ~kept);
      const unsigned u = (unsigned)(msde_mix64(key, (unsigned long long)d) >> 40);          // 24 bits
      const int pick = ds_nth_bit(set, (int)((u * (unsigned)__popc(set)) >> 24));
      kept |= 1u << pick;
      frontier = (frontier | __shfl(row, pick, 64)) & ~kept;
    }
  }
  if (lane == 0) keep[m] = kept;
}

extern "C" int msde_dataset_ext_rows(const int* edge_index, const long long* atom_ptr, const long long* bond_ptr, long long M,
                                     long long n_atoms, long long n_bonds, unsigned* rows, void* stream) {
  if (!atom_ptr || !bond_ptr || !rows || (n_bonds > 0 && !edge_index)) return MSDE_EINVAL;
  if (M <= 0 || n_atoms <= 0 || n_bonds < 0 || (M + 3) / 4 > 0x7fffffffLL) return MSDE_EINVAL;
  MSDE_LAUNCH(dataset_ext_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(DS_THREADS), 0, as_stream(stream), edge_index, atom_ptr,
              bond_ptr, M, n_atoms, n_bonds, rows);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_dataset_mask_epoch(const int* edge_index, const long long* atom_ptr, const long long* bond_ptr, long long M,
                                       long long n_atoms, long long n_bonds, unsigned long long mask_seed, long long epoch,
                                       const int* keep_count, unsigned* keep, void* stream) {
  if (!atom_ptr || !bond_ptr || !keep_count || !keep || (n_bonds > 0 && !edge_index)) return MSDE_EINVAL;
  if (M <= 0 || n_atoms <= 0 || n_bonds < 0 || (M + 3) / 4 > 0x7fffffffLL) return MSDE_EINVAL;
  const unsigned long long seed_e = mask_seed + DS_EPOCH_MIX * ((unsigned long long)epoch + 1ull);
  MSDE_LAUNCH(dataset_mask_epoch_kernel, dim3((unsigned)((M + 3) / 4)), dim3(DS_THREADS), 0, as_stream(stream), edge_index, atom_ptr,
              bond_ptr, M, n_atoms, n_bonds, seed_e, keep_count, keep);
  MSDE_CHECK_LAUNCH();
  return 0;
}
