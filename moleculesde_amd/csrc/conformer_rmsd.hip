// conformer_rmsd.hip — COV / MAT conformer evaluation: the aligned RMSD between every reference and every generated conformer
// of a molecule, and the coverage / matching scores built on it (the metrics the conformers of the 2D->3D sampler are judged
// by; neither the reference scripts nor this tree had them).
//
// RMSD.  For one pair (x = reference conformer, y = generated conformer, the same n kept atoms in stored order)
//   rmsd = min over rotations Q (det = +1) and translations of sqrt( mean_a |Q (x_a - c_x) - (y_a - c_y)|^2 )
//        = sqrt( max(0, (G_x + G_y - 2 lambda) / n) ),
// c = the centroids, G = the squared norms of the centred coordinates, lambda = the largest eigenvalue of Horn's symmetric
// 4 x 4 matrix of the cross-covariance S = sum_a (x_a - c_x)(y_a - c_y)^T (Horn 1987, closed-form absolute orientation with
// unit quaternions: the quaternion form only ever describes proper rotations, so a mirror image is NOT matched).  Atoms are
// taken as stored: no symmetry permutation, so this is an upper bound of a symmetry-aware RMSD.
//
// Everything behind the fp32 loads is fp64: centroids, the centring (before any product is formed), S, G and the solve.
//   (1) cr_prep_kernel: one wavefront per conformer: kept-atom count, centroid and G, once per conformer.
//   (2) cr_pair_kernel: one workgroup per 8 x 8 tile of pairs (host-built tile table).  Each of the four waves forms the S
//       of 16 pairs, one pair at a time: lane-strided partial sums over the atoms (any n), then an xor butterfly over the 64
//       lanes -- a fixed order, no atomics, so a pair's value depends on its own two conformers only.  The 64 S land in LDS
//       and the first wave solves them one pair per lane (the serial eigen-solve keeps 64 lanes busy, not one).
//   (2s) cr_sym_kernel: the symmetry-aware RMSD, the minimum of the above over a table of atom permutations per molecule
//       (the automorphisms of its graph, enumerated on the host): see the comment above the kernel.
// Eigen-solve: CR_SWEEPS cyclic Jacobi sweeps on the 4 x 4 (eigenvalues only).  A fixed count, no convergence test: repeated
// eigenvalues (identical, collinear, planar conformers, one or two atoms) leave it nothing to rotate and are harmless.
// A conformer with a non-finite kept coordinate has G = NaN, and every pair it takes part in is written as NaN.
//
// COV / MAT.  cr_cov_mat_kernel: one workgroup per molecule over its R x K block of the matrix; see include/msde_hip.h.
#include "msde_common.h"

#define CR_TR 8                    // tile: CR_TR references x CR_TK generated conformers
#define CR_TK 8
#define CR_PAIRS (CR_TR * CR_TK)   // = the wavefront width: one pair per lane in the solve
#define CR_SWEEPS 10               // cyclic Jacobi sweeps; 4 x 4 fp64 matrices are diagonal to round-off after 5 or 6
#define CR_REC 5                   // doubles per conformer record: cx, cy, cz, G, kept atoms
#define CR_MOL 8                   // int64 per molecule: n, R, K, ref_row0, gen_row0, out_off, mask_off, conf_off
#define CR_LDS 11                  // doubles per pair in LDS (9 of S, G_x + G_y, kept atoms): odd, so 32 lanes hit 32 slots

static_assert(CR_PAIRS == 64, "one pair per lane of a wavefront");

__device__ __forceinline__ double cr_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double cr_wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

// one Jacobi rotation that zeroes a[P][Q] of the symmetric a (both triangles kept, every index a compile-time constant)
template <int P, int Q>
__host__ __device__ inline void cr_rotate(double (&a)[4][4]) {
  const double apq = a[P][Q];
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // the smaller root: |angle| <= pi / 4
  t = apq == 0.0 ? 0.0 : t;                                                      // nothing to rotate (theta is inf or NaN)
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r != P && r != Q) {
      const double arp = a[r][P], arq = a[r][Q];
      a[r][P] = a[P][r] = arp - s * (arq + tau * arp);
      a[r][Q] = a[Q][r] = arq + s * (arp - tau * arq);
    }
}

// largest eigenvalue of Horn's matrix of S (row major: S[3 i + j] = sum_a x_i y_j of the centred coordinates)
__host__ __device__ inline double cr_horn_lambda(const double* S) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double a[4][4];
  a[0][0] = Sxx + Syy + Szz;
  a[1][1] = Sxx - Syy - Szz;
  a[2][2] = -Sxx + Syy - Szz;
  a[3][3] = -Sxx - Syy + Szz;
  a[0][1] = a[1][0] = Syz - Szy;
  a[0][2] = a[2][0] = Szx - Sxz;
  a[0][3] = a[3][0] = Sxy - Syx;
  a[1][2] = a[2][1] = Sxy + Syx;
  a[1][3] = a[3][1] = Szx + Sxz;
  a[2][3] = a[3][2] = Syz + Szy;
#pragma unroll 1
  for (int sweep = 0; sweep < CR_SWEEPS; ++sweep) {
    cr_rotate<0, 1>(a);
    cr_rotate<0, 2>(a);
    cr_rotate<0, 3>(a);
    cr_rotate<1, 2>(a);
    cr_rotate<1, 3>(a);
    cr_rotate<2, 3>(a);
  }
  return fmax(fmax(a[0][0], a[1][1]), fmax(a[2][2], a[3][3]));
}

// ---- (1) per conformer: kept atoms, centroid, squared norm of the centred coordinates --------------------------------------
// One wavefront per conformer, four per workgroup.  Conformer c of the launch belongs to the last molecule whose conf_off is
// <= c (bisection over the molecule table: at most 31 steps); a molecule's references come first, then its generated ones.
__global__ void __launch_bounds__(256) cr_prep_kernel(const float* __restrict__ ref_pos, const float* __restrict__ gen_pos,
                                                      const long long* __restrict__ mol, int G,
                                                      const unsigned char* __restrict__ mask, long long n_conf,
                                                      double* __restrict__ prep) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_conf) return;                                   // the whole wavefront leaves
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mol[(size_t)mid * CR_MOL + 7] <= c) lo = mid; else hi = mid - 1;
  }
  const long long* m = mol + (size_t)lo * CR_MOL;
  const long long n = m[0], R = m[1], j = c - m[7];
  const float* p = j < R ? ref_pos + 3 * (m[3] + j * n) : gen_pos + 3 * (m[4] + (j - R) * n);
  const unsigned char* mk = mask ? mask + m[6] : nullptr;
  double sx = 0.0, sy = 0.0, sz = 0.0, nk = 0.0;
  for (long long a = lane; a < n; a += 64)
    if (!mk || mk[a]) {
      sx += (double)p[3 * a]; sy += (double)p[3 * a + 1]; sz += (double)p[3 * a + 2];
      nk += 1.0;
    }
  sx = cr_wave_sum(sx); sy = cr_wave_sum(sy); sz = cr_wave_sum(sz); nk = cr_wave_sum(nk);
  const double cx = sx / nk, cy = sy / nk, cz = sz / nk;     // no kept atom: NaN, and so is every pair of this conformer
  double g = 0.0;
  for (long long a = lane; a < n; a += 64)
    if (!mk || mk[a]) {
      const double dx = (double)p[3 * a] - cx, dy = (double)p[3 * a + 1] - cy, dz = (double)p[3 * a + 2] - cz;
      g += dx * dx + dy * dy + dz * dz;
    }
  g = cr_wave_sum(g);
  if (lane == 0) {
    double* o = prep + (size_t)c * CR_REC;
    o[0] = cx; o[1] = cy; o[2] = cz; o[3] = g; o[4] = nk;
  }
}

// ---- (2) one 8 x 8 tile of pairs per workgroup ------------------------------------------------------------------------------
// tiles [n_tiles][3] = molecule, first reference, first generated conformer.  Pair p of the tile: reference r0 + (p >> 3),
// generated k0 + (p & 7); wave w forms S of pairs 16 w .. 16 w + 15 (valid or not is the same for the whole wave).
__global__ void __launch_bounds__(256) cr_pair_kernel(const float* __restrict__ ref_pos, const float* __restrict__ gen_pos,
                                                      const long long* __restrict__ mol, const int* __restrict__ tiles,
                                                      const unsigned char* __restrict__ mask,
                                                      const double* __restrict__ prep, double* __restrict__ out) {
  __shared__ double sS[CR_PAIRS * CR_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* tl = tiles + (size_t)blockIdx.x * 3;
  const long long* m = mol + (size_t)tl[0] * CR_MOL;
  const long long n = m[0], R = m[1], K = m[2], r0 = tl[1], k0 = tl[2];
  const unsigned char* mk = mask ? mask + m[6] : nullptr;
  for (int q = 0; q < CR_PAIRS / 4; ++q) {
    const int p = wave * (CR_PAIRS / 4) + q;
    const long long r = r0 + (p >> 3), k = k0 + (p & 7);
    if (r >= R || k >= K) continue;
    const double* px = prep + (size_t)(m[7] + r) * CR_REC;
    const double* py = prep + (size_t)(m[7] + R + k) * CR_REC;
    const double cxx = px[0], cxy = px[1], cxz = px[2], cyx = py[0], cyy = py[1], cyz = py[2];
    const float* x = ref_pos + 3 * (m[3] + r * n);
    const float* y = gen_pos + 3 * (m[4] + k * n);
    double s[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) s[e] = 0.0;
    for (long long a = lane; a < n; a += 64)
      if (!mk || mk[a]) {
        const double x0 = (double)x[3 * a] - cxx, x1 = (double)x[3 * a + 1] - cxy, x2 = (double)x[3 * a + 2] - cxz;
        const double y0 = (double)y[3 * a] - cyx, y1 = (double)y[3 * a + 1] - cyy, y2 = (double)y[3 * a + 2] - cyz;
        s[0] += x0 * y0; s[1] += x0 * y1; s[2] += x0 * y2;
        s[3] += x1 * y0; s[4] += x1 * y1; s[5] += x1 * y2;
        s[6] += x2 * y0; s[7] += x2 * y1; s[8] += x2 * y2;
      }
#pragma unroll
    for (int e = 0; e < 9; ++e) s[e] = cr_wave_sum(s[e]);
    if (lane == 0) {
      double* o = sS + p * CR_LDS;
#pragma unroll
      for (int e = 0; e < 9; ++e) o[e] = s[e];
      o[9] = px[3] + py[3];
      o[10] = px[4];
    }
  }
  __syncthreads();
  if (wave == 0) {
    const long long r = r0 + (lane >> 3), k = k0 + (lane & 7);
    if (r < R && k < K) {
      const double* o = sS + lane * CR_LDS;
      double S[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) S[e] = o[e];
      const double e0 = o[9], lam = cr_horn_lambda(S);
      double v = sqrt(fmax(0.0, (e0 - 2.0 * lam) / o[10]));
      if (!isfinite(e0)) v = __longlong_as_double(0x7ff8000000000000ll);   // one of the two conformers is not finite
      out[m[5] + r * K + k] = v;
    }
  }
}

// ---- (2s) symmetry-aware: one 8 x 8 tile of pairs per workgroup, every permutation of the molecule --------------------------
// rmsd = min over the P rows of the molecule's permutation table of the pair formula with S_p = sum_a x_{perm[p][a]} y_a^T
// (centred, kept atoms a): the count, the centroids and G do not move under a permutation of the kept atoms, so the records
// of cr_prep_kernel serve every p and min_p rmsd = the formula at max_p lambda.
// Layout: one ALIGNMENT (pair, p) per lane, serial over the atoms.  A wave takes one p at a time for all 64 pairs of the
// tile (wave w: p = w, w + 4, ...), so perm[p][a] is the same for the whole wave: 64 entries are fetched by one coalesced
// load and handed out by v_readlane.  The tile's 8 + 8 conformers are centred once, in fp64, into LDS ([16][stride] doubles,
// stride = 3 n made odd: the 4 reference and 8 generated rows a 32-lane group reads fall on different banks); a molecule of
// more than lds_atoms atoms reads the fp32 coordinates from global memory and centres on the fly -- (double)x - c is the
// same number either way, so the two paths agree bitwise.  Nothing crosses lanes until the maximum of lambda: each lane keeps
// its own over the p of its wave, four values per pair meet in LDS.  fmax is exact, so the order of the table, the split of
// the p over the waves and the path do not show in the result; the sum over the atoms runs a = 0, 1, ... for every p.
// A partial tile's missing conformers are clamped to the last valid one (computed, not written): no lane idles or diverges.
#define CS_LDS_ATOMS 160           // 16 (3 * 160 + 1) doubles = 61 568 bytes + 2 048 of lambda: inside the 64 KiB a launch may ask

__device__ __forceinline__ int cs_stride(int nl) { return (3 * nl) | 1; }

template <bool LDS>
__device__ __forceinline__ void cs_accumulate(double (&s)[9], const double* __restrict__ xs, const double* __restrict__ ys,
                                              const float* __restrict__ xg, const float* __restrict__ yg,
                                              const double (&cx)[3], const double (&cy)[3], long long pa, long long a) {
  double x0, x1, x2, y0, y1, y2;
  if (LDS) {                                                 // n <= CS_LDS_ATOMS here: 32-bit offsets
    const int ip = 3 * (int)pa, ia = 3 * (int)a;
    x0 = xs[ip]; x1 = xs[ip + 1]; x2 = xs[ip + 2];
    y0 = ys[ia]; y1 = ys[ia + 1]; y2 = ys[ia + 2];
  } else {
    x0 = (double)xg[3 * pa] - cx[0]; x1 = (double)xg[3 * pa + 1] - cx[1]; x2 = (double)xg[3 * pa + 2] - cx[2];
    y0 = (double)yg[3 * a] - cy[0]; y1 = (double)yg[3 * a + 1] - cy[1]; y2 = (double)yg[3 * a + 2] - cy[2];
  }
  s[0] += x0 * y0; s[1] += x0 * y1; s[2] += x0 * y2;
  s[3] += x1 * y0; s[4] += x1 * y1; s[5] += x1 * y2;
  s[6] += x2 * y0; s[7] += x2 * y1; s[8] += x2 * y2;
}

// the largest lambda of this lane's pair over the permutations p = wave, wave + 4, ... < P
template <bool LDS>
__device__ __forceinline__ double cs_best_lambda(const double* __restrict__ xs, const double* __restrict__ ys,
                                                 const float* __restrict__ xg, const float* __restrict__ yg,
                                                 const double (&cx)[3], const double (&cy)[3],
                                                 const unsigned char* __restrict__ mk, const int* __restrict__ pm,
                                                 long long n, long long P, int wave, int lane) {
  double best = -__longlong_as_double(0x7ff0000000000000ll);
  for (long long p = wave; p < P; p += 4) {
    const int* row = pm + p * n;
    double s[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) s[e] = 0.0;
    for (long long a0 = 0; a0 < n; a0 += 64) {
      const long long al = a0 + lane;
      const int mine = (al < n && (!mk || mk[al])) ? row[al] : -1;      // -1: past the end, or an atom the mask leaves out
      const int cnt = (int)(n - a0 < 64 ? n - a0 : 64);
      for (int j = 0; j < cnt; ++j) {
        const int pa = __builtin_amdgcn_readlane(mine, j);              // the same for the whole wave
        if (pa >= 0) cs_accumulate<LDS>(s, xs, ys, xg, yg, cx, cy, pa, a0 + j);
      }
    }
    best = fmax(best, cr_horn_lambda(s));
  }
  return best;
}

__global__ void __launch_bounds__(256) cr_sym_kernel(const float* __restrict__ ref_pos, const float* __restrict__ gen_pos,
                                                     const long long* __restrict__ mol, const int* __restrict__ tiles,
                                                     const unsigned char* __restrict__ mask,
                                                     const long long* __restrict__ sym, const int* __restrict__ perms,
                                                     int lds_atoms, const double* __restrict__ prep,
                                                     double* __restrict__ out) {
  extern __shared__ double cs_pos[];                         // [16][cs_stride(lds_atoms)]: the tile's centred conformers
  __shared__ double sL[4 * CR_PAIRS];                        // the best lambda of each wave, per pair
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int* tl = tiles + (size_t)blockIdx.x * 3;
  const long long* m = mol + (size_t)tl[0] * CR_MOL;
  const long long n = m[0], R = m[1], K = m[2], r0 = tl[1], k0 = tl[2];
  const long long P = sym[(size_t)tl[0] * 2], perm_off = sym[(size_t)tl[0] * 2 + 1];
  const unsigned char* mk = mask ? mask + m[6] : nullptr;
  const bool in_lds = n <= (long long)lds_atoms;             // the same for the whole workgroup
  const int stride = cs_stride(lds_atoms);
  if (in_lds) {
    const int per = 3 * (int)n;
    for (int i = threadIdx.x; i < 16 * per; i += 256) {
      const int c = i / per, e = i - c * per, d = e % 3;
      const long long j = c < 8 ? (r0 + c < R ? r0 + c : R - 1) : (k0 + c - 8 < K ? k0 + c - 8 : K - 1);
      const float* src = c < 8 ? ref_pos + 3 * (m[3] + j * n) : gen_pos + 3 * (m[4] + j * n);
      const double* rec = prep + (size_t)(m[7] + (c < 8 ? j : R + j)) * CR_REC;
      cs_pos[c * stride + e] = (double)src[e] - rec[d];
    }
  }
  __syncthreads();
  const long long r = r0 + (lane >> 3) < R ? r0 + (lane >> 3) : R - 1, k = k0 + (lane & 7) < K ? k0 + (lane & 7) : K - 1;
  const double* px = prep + (size_t)(m[7] + r) * CR_REC;
  const double* py = prep + (size_t)(m[7] + R + k) * CR_REC;
  const double cx[3] = {px[0], px[1], px[2]}, cy[3] = {py[0], py[1], py[2]};
  const float* xg = ref_pos + 3 * (m[3] + r * n);
  const float* yg = gen_pos + 3 * (m[4] + k * n);
  const double* xs = cs_pos + (int)(r - r0) * stride;
  const double* ys = cs_pos + (8 + (int)(k - k0)) * stride;
  const int* pm = perms + perm_off;
  const double best = in_lds ? cs_best_lambda<true>(xs, ys, xg, yg, cx, cy, mk, pm, n, P, wave, lane)
                             : cs_best_lambda<false>(xs, ys, xg, yg, cx, cy, mk, pm, n, P, wave, lane);
  sL[wave * CR_PAIRS + lane] = best;
  __syncthreads();
  if (wave == 0 && r0 + (lane >> 3) < R && k0 + (lane & 7) < K) {
    const double lam = fmax(fmax(sL[lane], sL[CR_PAIRS + lane]), fmax(sL[2 * CR_PAIRS + lane], sL[3 * CR_PAIRS + lane]));
    const double e0 = px[3] + py[3];
    double v = sqrt(fmax(0.0, (e0 - 2.0 * lam) / px[4]));
    if (!isfinite(e0)) v = __longlong_as_double(0x7ff8000000000000ll);     // one of the two conformers is not finite
    out[m[5] + r * K + k] = v;
  }
}

// ---- COV / MAT: one workgroup per molecule ----------------------------------------------------------------------------------
// conf_min [n_conf] in the order of the conformer records: a molecule's R row minima, then its K column minima (NaN entries
// count as +inf).  stats [G][2 T + 3] = COV-R [T], COV-P [T], MAT-R, MAT-P, finite generated conformers.
__global__ void __launch_bounds__(256) cr_cov_mat_kernel(const double* __restrict__ rmsd, const long long* __restrict__ mol,
                                                         const double* __restrict__ thr, int T, double* conf_min,
                                                         double* __restrict__ stats) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = __longlong_as_double(0x7ff8000000000000ll);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* m = mol + (size_t)blockIdx.x * CR_MOL;
  const long long R = m[1], K = m[2];
  const double* M = rmsd + m[5];
  double* rmin = conf_min + m[7];
  double* cmin = rmin + R;
  for (long long r = wave; r < R; r += 4) {                  // a row per wave: lanes along k (min is exact in any order)
    double v = inf;
    for (long long k = lane; k < K; k += 64) {
      const double e = M[r * K + k];
      v = fmin(v, e == e ? e : inf);
    }
    v = cr_wave_min(v);
    if (lane == 0) rmin[r] = v;
  }
  for (long long k = tid; k < K; k += 256) {                 // a column per thread: consecutive threads, consecutive k
    double v = inf;
    for (long long r = 0; r < R; ++r) {
      const double e = M[r * K + k];
      v = fmin(v, e == e ? e : inf);
    }
    cmin[k] = v;
  }
  __syncthreads();                                           // the minima of this workgroup are visible to all of it
  double* o = stats + (size_t)blockIdx.x * (2 * T + 3);
  for (int u = tid; u < 2 * T; u += 256) {
    const bool col = u >= T;
    const double d = thr[col ? u - T : u];
    const double* v = col ? cmin : rmin;
    const long long cnt = col ? K : R;
    long long hit = 0;
    for (long long i = 0; i < cnt; ++i) hit += v[i] <= d ? 1 : 0;
    o[u] = (double)hit / (double)cnt;
  }
  if (tid == 0) {                                            // the means: fp64, index order
    double sr = 0.0, sp = 0.0;
    long long fin = 0;
    for (long long r = 0; r < R; ++r) sr += rmin[r];
    for (long long k = 0; k < K; ++k)
      if (cmin[k] < inf) { sp += cmin[k]; ++fin; }
    o[2 * T] = fin > 0 ? sr / (double)R : nan;
    o[2 * T + 1] = fin > 0 ? sp / (double)fin : nan;
    o[2 * T + 2] = (double)fin;
  }
}

extern "C" int msde_conf_rmsd_matrix(const float* ref_pos, const float* gen_pos, const long long* mol, int G, const int* tiles,
                                     long long n_tiles, const unsigned char* atom_mask, long long n_conf, double* prep,
                                     double* rmsd, void* stream) {
  if (!ref_pos || !gen_pos || !mol || !tiles || !prep || !rmsd || G <= 0 || n_tiles <= 0 || n_conf < 2 * (long long)G)
    return MSDE_EINVAL;
  if (n_tiles > 0x7fffffffll || (n_conf + 3) / 4 > 0x7fffffffll) return MSDE_EUNSUP;
  MSDE_LAUNCH(cr_prep_kernel, dim3((unsigned)((n_conf + 3) / 4)), dim3(256), 0, as_stream(stream), ref_pos, gen_pos, mol, G,
              atom_mask, n_conf, prep);
  MSDE_CHECK_LAUNCH();
  MSDE_LAUNCH(cr_pair_kernel, dim3((unsigned)n_tiles), dim3(256), 0, as_stream(stream), ref_pos, gen_pos, mol, tiles,
              atom_mask, (const double*)prep, rmsd);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_conf_rmsd_matrix_sym(const float* ref_pos, const float* gen_pos, const long long* mol, int G,
                                         const int* tiles, long long n_tiles, const unsigned char* atom_mask, long long n_conf,
                                         const long long* sym, const int* perms, int lds_atoms, double* prep, double* rmsd,
                                         void* stream) {
  if (!ref_pos || !gen_pos || !mol || !tiles || !sym || !perms || !prep || !rmsd || G <= 0 || n_tiles <= 0 ||
      n_conf < 2 * (long long)G || lds_atoms < 0 || lds_atoms > CS_LDS_ATOMS)
    return MSDE_EINVAL;
  if (n_tiles > 0x7fffffffll || (n_conf + 3) / 4 > 0x7fffffffll) return MSDE_EUNSUP;
  MSDE_LAUNCH(cr_prep_kernel, dim3((unsigned)((n_conf + 3) / 4)), dim3(256), 0, as_stream(stream), ref_pos, gen_pos, mol, G,
              atom_mask, n_conf, prep);
  MSDE_CHECK_LAUNCH();
  const size_t lds = lds_atoms > 0 ? (size_t)16 * ((3 * lds_atoms) | 1) * sizeof(double) : 0;
  MSDE_LAUNCH(cr_sym_kernel, dim3((unsigned)n_tiles), dim3(256), lds, as_stream(stream), ref_pos, gen_pos, mol, tiles,
              atom_mask, sym, perms, lds_atoms, (const double*)prep, rmsd);
  MSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int msde_conf_cov_mat(const double* rmsd, const long long* mol, int G, const double* thresholds, int T,
                                 double* conf_min, double* stats, void* stream) {
  if (!rmsd || !mol || !thresholds || !conf_min || !stats || G <= 0 || T <= 0) return MSDE_EINVAL;
  MSDE_LAUNCH(cr_cov_mat_kernel, dim3((unsigned)G), dim3(256), 0, as_stream(stream), rmsd, mol, thresholds, T, conf_min,
              stats);
  MSDE_CHECK_LAUNCH();
  return 0;
}
