// Leave-one-out cross-validation of the kept posterior, point by point (gpg_loo, include/gpgrad.h).  With B = Kcov^-1 and
// alpha = Kcov^-1 (y - V beta) the residual of point a is B_aa^-1 alpha_a and its covariance varK B_aa^-1, B_aa the block of B
// on the rows of point a (its value row and its d gradient rows): no refit, and no more of B than its n point-diagonal blocks.
//     Kcov^-1 = P^-1 (L L^T)^-1 P^-1 = P^-1 W W^T P^-1,   W = L^-T (upper triangular: W[r, c] = 0 for c < r),
// so block a of B is  invp_i invp_j S_a[i, j],  S_a[i, j] = sum_c W[row_i(a), c] W[row_j(a), c].
//   1. W = L^-T into Wfull (the existing one-launch dataflow sweep, or the blocked sweep after a fallback).
//   2. loo_gram_kernel: S_a for every point, as K-chunk partials.  Lane <-> point: the entries of block row i at consecutive points
//      are contiguous in a column of W, so a wave reads 512 contiguous bytes per (column, block row).  Only what can be non-zero
//      is read: in the columns of block J (the columns that belong to d/dx_(J-1), or to the values for J = 0) only the block
//      rows <= J, and block row J itself only from the first row of the workgroup's 64 points on.
//   3. loo_finish_kernel, thread <-> point: partials added in chunk order, scaled by invp, with mean uncertainty the block of
//      Q = B - (B V) H^-1 (B V)' instead (Dubrule), Cholesky of the block, residual and covariance.
// Ordinary grids, no atomics, no workgroup waits for another: the results are a function of the shape only.
#include <climits>
#include <cmath>
#include <vector>
#include "gpg_internal.h"
#include "point_gram.h"   // loo_trip: the inner trip of the Gram kernel, shared with second.hip

namespace {

constexpr int kLooWorkgroups = 1024;   // (point tile, K-chunk) workgroups of one pair tile of loo_gram_kernel, about
constexpr int kLooChunksMax = 32;      // at most this many K-chunks
constexpr int kLooGroup = 6;           // block rows per group once the dim + 1 block rows no longer fit one lane's registers (dim > 8)
constexpr double kLooPivTol = 1e-12;   // the pivot rule of lkd_reduce_lin_kernel
constexpr int kLooFinishLds = 48 * 1024;

// first column of column block J: block 0 = the n value rows, block J >= 1 = the ng rows of d/dx_(J-1)
__device__ __forceinline__ int loo_blk_start(int J, int n, int ng) { return J == 0 ? 0 : n + (J - 1) * ng; }

// partial[(s npairs + p) npad + a] = sum over the columns c < N of K-chunk s of W[row_i(a), c] W[row_j(a), c], p = j (j + 1) / 2 + i
// for the block rows i <= j of pair tile blockIdx.z: groups of G block rows, tile (gi, gj) holds the rows [gi G, gi G + G) x
// [gj G, gj G + G); DIAG: the tiles gi = gj (all there is when dim + 1 <= G), else the tiles gi < gj.  grid = (point tiles, S, tiles).
// Chunk s holds the whole 64-column tiles [s ktiles / S, (s + 1) ktiles / S).  Wave w takes the columns = w (mod 4) of every
// segment, several per trip (their loads in flight together: the kernel is bound by the latency and the bandwidth of W); the four
// waves are added in wave order through LDS.  W[r, c] = 0 for c < r: the pair (i, j) starts at the first column of block j, and
// block row j of the workgroup's points at their first row.  Points beyond n and points without a gradient read the value row of a
// valid point instead (in bounds; loo_finish_kernel does not read those sums).
template <int G, bool DIAG>
__global__ void __launch_bounds__(256) loo_gram_kernel(const double* __restrict__ W, int ldw, int n, int ng, int N, int bs,
                                                       const int* __restrict__ gpos, int ktiles, int S, int npairs, int npad,
                                                       double* __restrict__ partial) {
  constexpr int NACC = loo_nacc(G, DIAG);
  __shared__ double sh[3][8][64];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int a = blockIdx.x * 64 + lane, ac = a < n ? a : n - 1, s = blockIdx.y;
  int gi, gj;
  if (DIAG) {
    gi = gj = blockIdx.z;
  } else {
    const int t = blockIdx.z;
    gj = 1;
    while ((gj + 1) * gj / 2 <= t) ++gj;
    gi = t - gj * (gj - 1) / 2;
  }
  const int I0 = gi * G, J0 = gj * G;
  const int gb = bs - J0 < G ? bs - J0 : G;
  const int g = bs > 1 ? gpos[ac] : -1;
  int gmin = g >= 0 ? g : INT_MAX;                     // gpos is monotone: the first gradient row of the 64 points
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(gmin, o); gmin = v < gmin ? v : gmin; }
  gmin = __builtin_amdgcn_readfirstlane(gmin);
  unsigned ra[G], rb[G];                               // byte offsets of the lane's rows in a column of W
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int bi = I0 + i, bj = J0 + i;
    ra[i] = 8u * (unsigned)((bi >= 1 && bi < bs && g >= 0) ? n + (bi - 1) * ng + g : ac);
    rb[i] = 8u * (unsigned)((bj >= 1 && bj < bs && g >= 0) ? n + (bj - 1) * ng + g : ac);
  }
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  const int c0 = (int)((long long)s * ktiles / S) * 64;
  int c1 = (int)((long long)(s + 1) * ktiles / S) * 64;
  if (c1 > N) c1 = N;
  // Segments in column order, two per column block Jc >= J0: the columns before and from the first row of block row Jc at the
  // workgroup's points (before it that block row is still zero).  Wave w takes the columns = w (mod 4) of a segment in ascending
  // order, U per trip.  The only branches are the two loops (an empty segment is a loop of no trips).
  constexpr int U = loo_unroll(DIAG ? G : 2 * G);
  const int nseg = 2 * (bs - J0);
#pragma unroll 1
  for (int q = 0; q < nseg; ++q) {
    const int Jc = J0 + (q >> 1), ph = q & 1;
    const int bstart = loo_blk_start(Jc, n, ng), bend = loo_blk_start(Jc + 1, n, ng);
    const int lo = bstart > c0 ? bstart : c0, hi = bend < c1 ? bend : c1;
    const bool own = Jc - J0 < gb;                     // block row Jc belongs to this pair tile
    int first = Jc == 0 ? (int)blockIdx.x * 64 : (gmin == INT_MAX ? bend : bstart + gmin);
    first = first < lo ? lo : first;
    const int split = own ? (first < hi ? first : hi) : lo;
    const int rows = own ? Jc - J0 + ph : (ph ? gb : 0);          // active block rows of B
    const int slo = ph ? split : lo;
    const int shi = rows < 1 ? slo : (ph ? hi : split);
    unsigned rbe[G];                                   // rb, or out of range for the block rows that are not active here
#pragma unroll
    for (int j = 0; j < G; ++j) rbe[j] = j < rows ? rb[j] : kLooOutOfRange;
    for (int c = slo + w; c < shi; c += 4 * U) loo_trip<G, DIAG, U>(W, ldw, c, shi, ra, rbe, acc);
  }
  // the four waves in wave order, eight sums per round
#pragma unroll
  for (int r0 = 0; r0 < NACC; r0 += 8) {
    if (w > 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (r0 + k < NACC) sh[w - 1][k][lane] = acc[r0 + k];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (r0 + k < NACC) {
          const int q = r0 + k;
          int i, j;
          if (DIAG) {
            j = 0;
            while ((j + 1) * (j + 2) / 2 <= q) ++j;
            i = q - j * (j + 1) / 2;
          } else {
            j = q / G;
            i = q - j * G;
          }
          if (j < gb) {
            const int bi = I0 + i, bj = J0 + j;
            partial[((size_t)s * npairs + (size_t)(bj * (bj + 1) / 2 + bi)) * npad + a] =
                ((acc[q] + sh[0][k][lane]) + sh[1][k][lane]) + sh[2][k][lane];
          }
        }
      }
    }
    __syncthreads();
  }
}

// h = H^-1 V' alpha [nb] by ONE workgroup: alpha = zvec invp; V' alpha coefficient by coefficient (value row r: [1, x_r], gradient
// row n + k ng + g: e_(k+1)), each thread its rows = tid (mod 256), the 256 sums by a tree in LDS; then R y = t, R' h = y by thread 0.
__global__ void __launch_bounds__(256) loo_vta_kernel(int n, int ng, int nb, const double* __restrict__ Xt, const double* __restrict__ zvec,
                                                      const double* __restrict__ invp, const double* __restrict__ small, double* __restrict__ h) {
  __shared__ double red[256];
  __shared__ double t[GPG_MAX_NBETA];
  const int tid = threadIdx.x;
  for (int i = 0; i < nb; ++i) {
    double s = 0.0;
    for (int r = tid; r < n; r += 256) s += (i == 0 ? 1.0 : Xt[(size_t)(i - 1) * n + r]) * (zvec[r] * invp[r]);
    if (i > 0)
      for (int q = tid; q < ng; q += 256) { const int r = n + (i - 1) * ng + q; s += zvec[r] * invp[r]; }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) t[i] = red[0];
    __syncthreads();
  }
  if (tid != 0) return;
  const double* R = small + GPG_MU_SMALL_R;
  for (int i = 0; i < nb; ++i) {
    double v = t[i];
    for (int k = 0; k < i; ++k) v -= R[i * nb + k] * t[k];
    t[i] = v / R[i * nb + i];
  }
  for (int i = nb - 1; i >= 0; --i) {
    double v = t[i];
    for (int k = i + 1; k < nb; ++k) v -= R[k * nb + i] * t[k];
    t[i] = v / R[i * nb + i];
    h[i] = t[i];
  }
}

struct LooFinish {
  const double* partial; int S, npairs, npad;
  int n, ng, bs, nb, munc, PW;
  const int* gpos;
  const double *invp, *zvec, *KV, *small, *h;
  double varK;
  double *prec, *cov, *resid, *qy;
  int* bad;
};

// Thread <-> point (PW points per workgroup; everything a thread keeps is in LDS with the point as the fastest index: runtime
// loops, no registers indexed at run time).  M: the block, lower packed (M(i, j) = m[i (i + 1) / 2 + j], j <= i).
__global__ void loo_finish_kernel(LooFinish f) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int PW = f.PW, bs = f.bs, nb = f.nb, t = threadIdx.x;
  double* Rsh = lds;                                              // [nb x nb]   (mean uncertainty only)
  double* m = Rsh + (f.munc ? ((nb * nb + 1) & ~1) : 0);          // [npairs][PW]
  double* qv = m + (size_t)f.npairs * PW;                         // [bs][PW]  qy of the point's rows
  double* yv = qv + (size_t)bs * PW;                              // [bs][PW]
  double* cv = yv + (size_t)bs * PW;                              // [nb bs][PW] R^-1 (B V)_a'  (mean uncertainty only)
  if (f.munc) {
    for (int k = t; k < nb * nb; k += PW) Rsh[k] = f.small[GPG_MU_SMALL_R + k];
    __syncthreads();
  }
  const int a = blockIdx.x * PW + t;
  if (a >= f.n) return;
#define M_(i, j) m[(size_t)((i) * ((i) + 1) / 2 + (j)) * PW + t]
#define ROW_(i) ((i) == 0 ? a : f.n + ((i) - 1) * f.ng + g)
  const int g = bs > 1 ? f.gpos[a] : -1;
  const int mb = g >= 0 ? bs : 1;                                 // rows of this point
  for (int i = 0; i < mb; ++i) {
    const double ipi = f.invp[ROW_(i)];
    for (int j = 0; j <= i; ++j) {
      const double* pp = f.partial + (size_t)(i * (i + 1) / 2 + j) * f.npad + a;
      const size_t stride = (size_t)f.npairs * f.npad;
      double s = 0.0;
#pragma unroll 8
      for (int q = 0; q < f.S; ++q) s += pp[(size_t)q * stride];  // chunk order
      M_(i, j) = (s * f.invp[ROW_(j)]) * ipi;
    }
  }
  for (int i = 0; i < mb; ++i) {
    const int r = ROW_(i);
    const double ip = f.invp[r];
    double q = f.zvec[r] * ip;                                    // alpha (alpha_kernel's product)
    if (f.munc) {
      const double* kv = f.KV + (size_t)r * nb;                   // row r of (L L^T)^-1 P^-1 V: invp times it is row r of Kcov^-1 V
      double corr = 0.0;
      for (int k = 0; k < nb; ++k) {
        corr += kv[k] * f.h[k];
        double v = kv[k] * ip;                                    // R c = (Kcov^-1 V)_r'
        for (int l = 0; l < k; ++l) v -= Rsh[k * nb + l] * cv[(size_t)(l * bs + i) * PW + t];
        cv[(size_t)(k * bs + i) * PW + t] = v / Rsh[k * nb + k];
      }
      q -= ip * corr;
      for (int j = 0; j <= i; ++j) {
        double s = 0.0;
        for (int k = 0; k < nb; ++k) s += cv[(size_t)(k * bs + i) * PW + t] * cv[(size_t)(k * bs + j) * PW + t];
        M_(i, j) -= s;
      }
    }
    qv[(size_t)i * PW + t] = q;
    if (f.qy) f.qy[r] = q;
  }
  if (f.prec) {
    double* out = f.prec + (size_t)a * bs * bs;
    for (int i = 0; i < bs; ++i)
      for (int j = 0; j < bs; ++j) out[i * bs + j] = (i < mb && j < mb) ? (i >= j ? M_(i, j) : M_(j, i)) : 0.0;
  }
  // M = C C^T in place (left-looking: column k is untouched until its turn, so M(k, k) is the entry the pivot rule refers to)
  bool bad = false;
  for (int k = 0; k < mb && !bad; ++k) {
    const double d0 = M_(k, k);
    double piv = d0;
    for (int l = 0; l < k; ++l) piv -= M_(k, l) * M_(k, l);
    if (!(piv > kLooPivTol * d0)) { bad = true; break; }
    const double ckk = sqrt(piv);
    M_(k, k) = ckk;
    for (int i = k + 1; i < mb; ++i) {
      double v = M_(i, k);
      for (int l = 0; l < k; ++l) v -= M_(i, l) * M_(k, l);
      M_(i, k) = v / ckk;
    }
  }
  f.bad[a] = bad ? 1 : 0;
  double* cout = f.cov ? f.cov + (size_t)a * bs * bs : nullptr;
  if (cout)
    for (int k = 0; k < bs * bs; ++k) cout[k] = 0.0;
  if (bad) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = 0; i < mb; ++i) {
      if (f.resid) f.resid[ROW_(i)] = nan;
      if (cout)
        for (int j = 0; j < mb; ++j) cout[i * bs + j] = nan;
    }
    return;
  }
  // X = C^-1 in place, column by column (column j needs the columns > j of C and its diagonal entries below j: still in place)
  for (int j = 0; j < mb; ++j) {
    M_(j, j) = 1.0 / M_(j, j);
    for (int i = j + 1; i < mb; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s += M_(i, k) * M_(k, j);
      M_(i, j) = -s / M_(i, i);
    }
  }
  // resid = M^-1 q = X' (X q);  cov = varK X' X, one sum per pair i >= j written to both places
  for (int k = 0; k < mb; ++k) {
    double s = 0.0;
    for (int j = 0; j <= k; ++j) s += M_(k, j) * qv[(size_t)j * PW + t];
    yv[(size_t)k * PW + t] = s;
  }
  for (int i = 0; i < mb; ++i) {
    if (f.resid) {
      double s = 0.0;
      for (int k = i; k < mb; ++k) s += M_(k, i) * yv[(size_t)k * PW + t];
      f.resid[ROW_(i)] = s;
    }
    if (cout)
      for (int j = 0; j <= i; ++j) {
        double s = 0.0;
        for (int k = i; k < mb; ++k) s += M_(k, i) * M_(k, j);
        s *= f.varK;
        cout[i * bs + j] = s;
        cout[j * bs + i] = s;
      }
  }
#undef M_
#undef ROW_
}

// K-chunks for T point tiles and Npad columns: a function of the shape only
int loo_chunks(int T, int Npad) {
  const int ktiles = Npad / 64;
  int s = (kLooWorkgroups + T - 1) / T;
  if (s > kLooChunksMax) s = kLooChunksMax;
  return s < 1 ? 1 : (s > ktiles ? ktiles : s);
}

// bytes of W loo_gram_kernel reads with groups of G block rows (the point tiles' skipped leading columns counted to the row)
double loo_gram_bytes(int n, int ng, int bs, int G) {
  const int ngroups = (bs + G - 1) / G;
  double elems = 0.0;
  auto rows = [&](int b) { return b == 0 ? (double)n : (double)ng; };
  for (int gj = 0; gj < ngroups; ++gj)
    for (int gi = 0; gi <= gj; ++gi) {
      const int J0 = gj * G, J1 = J0 + G < bs ? J0 + G : bs;
      double rows_a = 0.0;
      if (gi < gj) for (int b = gi * G; b < gi * G + G; ++b) rows_a += rows(b);
      for (int Jc = J0; Jc < bs; ++Jc) {
        const double cols = rows(Jc);
        double rows_b = 0.0;
        for (int b = J0; b < J1 && b < Jc; ++b) rows_b += rows(b);
        elems += cols * ((Jc == J0 ? 0.5 : 1.0) * rows_a + rows_b);   // (nothing to pair the rows of A with before block row J0 starts)
        if (Jc < J1) elems += cols * (cols + 1.0) / 2.0;   // block row Jc itself: its triangle
      }
    }
  return 8.0 * elems;
}

int loo_once(gpg_ctx* c, double varK, double* resid, double* cov, double* prec, double* qy, int* n_bad) {
  if (!c->eval_ready) { c->err = "gpg_setup_eval must succeed before gpg_loo"; return -1; }
  GPG_HIP_OK(c, hipSetDevice(c->device));
  if (gpg_ws_activate(c, 1) != 0) return -2;
  const bool munc = c->mean_unc != 0;
  if (munc) {
    if (int rc = gpg_meanunc_ensure(c)) return rc;
  }
  const int n = c->n, ng = c->use_grad ? c->ng : 0, N = c->N, Npad = c->Npad, nb = c->n_beta;
  const int bs = c->use_grad ? c->d + 1 : 1, npairs = bs * (bs + 1) / 2;
  const size_t nn = (size_t)Npad * Npad;
  if (!c->Wfull) {                                     // as the gradient path: the pair is allocated and released together
    if (hipMalloc(&c->Wfull, sizeof(double) * nn) != hipSuccess || hipMalloc(&c->Minv, sizeof(double) * nn) != hipSuccess) {
      (void)hipGetLastError();
      if (c->Wfull) (void)hipFree(c->Wfull);
      c->Wfull = c->Minv = nullptr;
      c->err = "out of device memory for W = L^-T of gpg_loo";
      return -2;
    }
  }
  const int T = (n + 63) / 64, npad = T * 64, S = loo_chunks(T, Npad), ktiles = Npad / 64;
  const size_t blk = (size_t)n * bs * bs;
  const size_t need = (size_t)S * npairs * npad + 2 * blk + 2 * (size_t)N + GPG_BETA_STRIDE + ((size_t)n + 1) / 2;
  if (need > c->loo_scr_elems) {
    if (c->loo_scr) (void)hipFree(c->loo_scr);
    c->loo_scr = nullptr; c->loo_scr_elems = 0;
    if (hipMalloc(&c->loo_scr, sizeof(double) * need) != hipSuccess) {
      (void)hipGetLastError();
      c->loo_scr = nullptr;
      c->err = "out of device memory for the leave-one-out scratch";
      return -2;
    }
    c->loo_scr_elems = need;
  }
  double* partial = c->loo_scr;
  double* prec_dev = partial + (size_t)S * npairs * npad;
  double* cov_dev = prec_dev + blk;
  double* resid_dev = cov_dev + blk;
  double* qy_dev = resid_dev + N;
  double* h_dev = qy_dev + N;
  int* bad_dev = reinterpret_cast<int*>(h_dev + GPG_BETA_STRIDE);
  GPG_HIP_OK(c, hipMemsetAsync(c->info, 0, sizeof(int), c->stream));
  gpg_inverse_from_factor(c, c->Wfull, nullptr);       // W = L^-T, upper triangular, leading dimension Npad
  const int G = bs <= 5 ? 5 : (bs <= 9 ? 9 : kLooGroup);
  const int ngroups = (bs + G - 1) / G;
  gpg_prof_begin(c, GPG_PROF_REDUCE, loo_gram_bytes(n, ng, bs, G));
#define LOO_GRAM(GV, DIAGV, TILES)                                                                                              \
  hipLaunchKernelGGL((loo_gram_kernel<GV, DIAGV>), dim3(T, S, TILES), dim3(256), 0, c->stream, (const double*)c->Wfull, Npad, n, ng, N, \
                     bs, (const int*)c->gpos, ktiles, S, npairs, npad, partial)
  if (G == 5) LOO_GRAM(5, true, 1);
  else if (G == 9) LOO_GRAM(9, true, 1);
  else {
    LOO_GRAM(kLooGroup, true, ngroups);
    LOO_GRAM(kLooGroup, false, ngroups * (ngroups - 1) / 2);
  }
#undef LOO_GRAM
  gpg_prof_end(c);
  const double* KV = munc ? c->mu_buf + (size_t)nb * Npad : nullptr;
  if (munc)
    hipLaunchKernelGGL(loo_vta_kernel, dim3(1), dim3(256), 0, c->stream, n, ng, nb, (const double*)c->Xt, (const double*)c->zvec,
                       (const double*)c->invp, (const double*)c->mu_small, h_dev);
  // points per workgroup of the finishing kernel: what fits the LDS budget
  const size_t per_point = sizeof(double) * ((size_t)npairs + 2 * bs + (munc ? (size_t)nb * bs : 0));
  const size_t fixed = munc ? sizeof(double) * (size_t)((nb * nb + 1) & ~1) : 0;
  int PW = 64;
  while (PW > 1 && fixed + per_point * PW > (size_t)kLooFinishLds) PW >>= 1;
  LooFinish f{partial, S, npairs, npad, n, ng, bs, nb, munc ? 1 : 0, PW, c->gpos, c->invp, c->zvec, KV, c->mu_small, h_dev,
              varK, prec_dev, cov_dev, resid_dev, qy_dev, bad_dev};
  hipLaunchKernelGGL(loo_finish_kernel, dim3((n + PW - 1) / PW), dim3(PW), fixed + per_point * PW, c->stream, f);
  std::vector<int> bad(n);
  if (resid) GPG_HIP_OK(c, hipMemcpyAsync(resid, resid_dev, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  if (qy) GPG_HIP_OK(c, hipMemcpyAsync(qy, qy_dev, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  if (prec) GPG_HIP_OK(c, hipMemcpyAsync(prec, prec_dev, sizeof(double) * blk, hipMemcpyDeviceToHost, c->stream));
  if (cov) GPG_HIP_OK(c, hipMemcpyAsync(cov, cov_dev, sizeof(double) * blk, hipMemcpyDeviceToHost, c->stream));
  GPG_HIP_OK(c, hipMemcpyAsync(bad.data(), bad_dev, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  GPG_HIP_OK(c, hipMemcpyAsync(c->h_info, c->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
  GPG_HIP_OK(c, hipGetLastError());
  GPG_LAUNCH_OK(c);
  if (gpg_solve_failure(c)) return -4;
  if (n_bad) {
    int cnt = 0;
    for (int a = 0; a < n; ++a) cnt += bad[a];
    *n_bad = cnt;
  }
  return 0;
}

}  // namespace

extern "C" {

int gpg_loo(gpg_ctx* c, double varK, double* resid, double* cov, double* prec, double* qy, int* n_bad) {
  if (!c) return -1;
  return gpg_with_fallback(c, [&] { return loo_once(c, varK, resid, cov, prec, qy, n_bad); });
}

}  // extern "C"
