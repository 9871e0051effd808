// Per-point covariance of [f, grad f] and batched Hessians of the posterior (gpg_predict_second, include/gpgrad.h).  For query
// point j with the cross-covariance rows k_j (value) and dk_j/dx_1 .. dk_j/dx_d (derivatives) against the training data,
//     Z_j = [k_j; dk_j/dx_1; ...; dk_j/dx_d] P^-1 L^-T            (bs = d + 1 forward-swept rows),
//     gcov_j = varK (K0 - Z_j Z_j')  [bs x bs],   K0 the prior block of one point with itself,
// which is the j-th diagonal block of the matrix gpg_predict_joint returns, without the other nx^2 - nx blocks.  gcov_j[0, 0] is
// sig^2, gcov_j[0, k + 1] = 1/2 d sig^2 / d x_k, and T_j = (Z_j Z_j')[1.., 1..] is the term of d2 sig^2 / dx2 that
// rows_gram_kernel (solve.hip) forms for one point: one per-point Gram kernel feeds the covariance and the Hessian of sig.
// The host loops over chunks of points whose rows fit Wt (at most 4096 rows; row r = blk * pc + j for the pc points of a chunk).
// Per chunk, all on the context's stream:
//   1. cross_joint_kernel writes the rows of Kqy P^-1, joint_mean_* their product with p * alpha (joint.hip): mu and dmudx;
//   2. gpg_forward_rows sweeps all rows at once;
//   3. second_gram_kernel: S_j[i, k] = sum_c Z[i pc + j, c] Z[k pc + j, c] as K-chunk partials.  Lane <-> query point: block row i
//      of consecutive points is contiguous in a column of Z, so a wave reads 512 contiguous bytes per (column, block row), the
//      layout of loo_gram_kernel (the inner trip is shared: point_gram.h).  Z is dense: every column, every block row.
//      second_finish_kernel adds the partials in chunk order, subtracts from K0, scales, adds the mean-uncertainty term and
//      writes both halves of the block;
//   4. Hessians only: gpg_backward_rows on the tiles that hold the value rows (after step 3 has read them), the mean-uncertainty
//      update of those rows, hess_contract_kernel (solve.hip: gpg_predict_hess runs it for one point) on a grid over
//      (row k, query point j), and second_hess_kernel, which assembles d2mudx2 and d2sigdx2 by the formulas of gpg_predict_hess;
//   5. one copy per output and one synchronisation.
// The K-chunk count is a function of Npad only (or gpg_set_gram_splits): a point's block does not depend on how many points ride
// along with it.  Ordinary grids, no atomics, no workgroup waits for another: the results are a function of the shape only.
//
// Registers of second_gram_kernel (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / scratch bytes / waves per SIMD) next to
// loo_gram_kernel's: G = 5: 62 / 0 / 8 (loo 68 / 0 / 7); G = 9: 126 / 0 / 4 (191 / 0 / 2); groups of 6, diagonal: 66 / 0 / 7 (70 / 0 / 7),
// off-diagonal: 126 / 0 / 4 (157 / 0 / 3).  No kernel of this file uses scratch.
// Measured on one MI355X (tools/second_time.py; host clock, median after warm-up, two runs; sweep and Gram from gpg_prof events):
//   (a) gcov alone at the largest nx gpg_predict_joint takes          n = 2000, d = 8, nx = 455      n = 500, d = 4, nx = 819
//       gpg_predict_second                                            26.5 - 26.6 ms                 0.87 - 0.88 ms
//         forward sweep                                               26.1 - 26.2 ms                 0.74 ms
//         second_gram_kernel                                          0.122 ms, 0.591 GB: 4.8 TB/s   20.8 us, 83.9 MB: 4.0 TB/s
//         rest (cross rows, finishing kernel, copies, launches)       0.24 - 0.26 ms                 0.11 - 0.12 ms
//       gpg_predict_joint (cov), same points, same build              37.3 - 37.4 ms                 4.37 ms
//       (loo_gram_kernel, the yardstick: 4.4 TB/s at N = 18000)
//   (b) Hessians of 64 points: one gpg_predict_second call            8.6 - 8.8 ms                   1.04 - 1.06 ms
//       64 gpg_predict_hess calls                                     267 - 268 ms                   41.3 - 41.6 ms
#include <algorithm>
#include <cmath>
#include <vector>
#include "gpg_internal.h"
#include "point_gram.h"

namespace {

constexpr int kSecondMaxRows = 4096;   // rows of a chunk, padded to 64: what Wt is sized for by the other posterior calls as well
constexpr int kSecondChunksMax = 64;   // K-chunks of the Gram kernel when gpg_set_gram_splits is not set: min(Npad / 64, this)
constexpr int kSecondGroup = 6;        // block rows per group once bs block rows no longer fit one lane's registers (dim > 8), as loo.hip

// partial[(s npairs + p) npad + j] = sum over the columns of K-chunk s of Z[bi pc + j, c] Z[bj pc + j, c], p = bj (bj + 1) / 2 + bi,
// for the block rows bi <= bj of pair tile blockIdx.z: groups of G block rows, tile (gi, gj) holds the rows [gi G, gi G + G) x
// [gj G, gj G + G); DIAG: the tiles gi = gj (all there is when bs <= G), else the tiles gi < gj.  grid = (point tiles, S, tiles).
// Chunk s holds the whole 64-column tiles [s ktiles / S, (s + 1) ktiles / S) of the Npad columns (the columns N .. Npad - 1 of Z
// are zero).  Wave w takes the columns = w (mod 4), several per trip; the four waves are added in wave order through LDS.
// Block rows >= bs of the last group are out of the descriptor's range (they read nothing and add +0.0); lanes beyond the pc
// points of the chunk read the last point instead (in bounds; second_finish_kernel does not read their sums).
template <int G, bool DIAG>
__global__ void __launch_bounds__(256) second_gram_kernel(const double* __restrict__ Z, int ldz, int pc, int bs, int ktiles, int S,
                                                          int npairs, int npad, double* __restrict__ partial) {
  constexpr int NACC = loo_nacc(G, DIAG);
  __shared__ double sh[3][8][64];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = blockIdx.x * 64 + lane, jc = j < pc ? j : pc - 1, s = blockIdx.y;
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
  unsigned ra[G], rb[G];                               // byte offsets of the lane's rows in a column of Z
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int bi = I0 + i, bj = J0 + i;
    ra[i] = bi < bs ? 8u * (unsigned)(bi * pc + jc) : kLooOutOfRange;
    rb[i] = bj < bs ? 8u * (unsigned)(bj * pc + jc) : kLooOutOfRange;
  }
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  const int c0 = (int)((long long)s * ktiles / S) * 64, c1 = (int)((long long)(s + 1) * ktiles / S) * 64;
  constexpr int U = loo_unroll(DIAG ? G : 2 * G);
  for (int c = c0 + w; c < c1; c += 4 * U) loo_trip<G, DIAG, U>(Z, ldz, c, c1, ra, rb, acc);
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
          int i, jj;
          if (DIAG) {
            jj = 0;
            while ((jj + 1) * (jj + 2) / 2 <= q) ++jj;
            i = q - jj * (jj + 1) / 2;
          } else {
            jj = q / G;
            i = q - jj * G;
          }
          if (jj < gb) {
            const int bi = I0 + i, bj = J0 + jj;
            partial[((size_t)s * npairs + (size_t)(bj * (bj + 1) / 2 + bi)) * npad + j] =
                ((acc[q] + sh[0][k][lane]) + sh[1][k][lane]) + sh[2][k][lane];
          }
        }
      }
    }
    __syncthreads();
  }
}

struct SecondFinish {
  const double* partial; int S, npairs, npad;
  int pc, bs, mp, nb, munc;
  const double *K0, *cf;
  double varK;
  double *gcov, *sraw;
};

// Pair p = k (k + 1) / 2 + i (i <= k) of point j = 64 blockIdx.x + threadIdx.x (grid = (point tiles, npairs)): the S partials in chunk
// order, gcov[j, i, k] = gcov[j, k, i] = varK (K0[k, i] - sum) (+ varK c'_i . c'_k with the mean uncertainty, c' = mu_cf of the
// chunk's rows), and the sum itself to sraw[p npad + j] for the Hessian of sig.
__global__ void __launch_bounds__(64) second_finish_kernel(SecondFinish f) {
  const int j = blockIdx.x * 64 + threadIdx.x, p = blockIdx.y;
  if (j >= f.pc) return;
  int k = 0;
  while ((k + 1) * (k + 2) / 2 <= p) ++k;
  const int i = p - k * (k + 1) / 2;
  const double* part = f.partial + (size_t)p * f.npad + j;
  const size_t stride = (size_t)f.npairs * f.npad;
  double g = 0.0;
  int s = 0;
  for (; s + 8 <= f.S; s += 8) {   // eight loads in flight, added in chunk order all the same
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(s + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) g += v[u];
  }
  for (; s < f.S; ++s) g += part[(size_t)s * stride];
  double v = f.varK * (f.K0[k * f.bs + i] - g);
  if (f.munc) {
    double t = 0.0;
    for (int a = 0; a < f.nb; ++a) t += f.cf[(size_t)a * f.mp + i * f.pc + j] * f.cf[(size_t)a * f.mp + k * f.pc + j];
    v = v + f.varK * t;
  }
  if (f.gcov) {
    double* out = f.gcov + (size_t)j * f.bs * f.bs;
    out[i * f.bs + k] = v;
    out[k * f.bs + i] = v;
  }
  if (f.sraw) f.sraw[(size_t)p * f.npad + j] = g;
}

// Thread <-> (point j, k, i): d2mudx2 = H1 and, by the arithmetic of gpg_predict_hess with sig and dsigdx taken from the block,
//   sig = sqrt(max(0, gcov_00)),  dsigdx_k = gcov_0,k+1 / sig,  d2sig2 = -2 varK (H2 + T) (+ 2 varK c'_k+1 . c'_i+1),
//   d2sigdx2 = (d2sig2 - 2 dsigdx_k dsigdx_i) / (2 sig),  NaN where sig == 0.
__global__ void __launch_bounds__(256) second_hess_kernel(int pc, int d, int npad, int mp, int nb, int munc, double varK,
                                                          const double* __restrict__ h1, const double* __restrict__ h2,
                                                          const double* __restrict__ sraw, const double* __restrict__ gcov,
                                                          const double* __restrict__ cf, double* __restrict__ d2mu,
                                                          double* __restrict__ d2sig) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= pc * d * d) return;
  const int j = t / (d * d), e = t - j * d * d, k = e / d, i = e - k * d;
  const int bs = d + 1;
  d2mu[t] = h1[t];
  const double* blk = gcov + (size_t)j * bs * bs;
  const double s2 = blk[0];
  const double sg = sqrt(s2 < 0.0 ? 0.0 : s2);
  const int lo = (i < k ? i : k) + 1, hi = (i < k ? k : i) + 1;
  double d2s2 = -2.0 * varK * (h2[t] + sraw[(size_t)(hi * (hi + 1) / 2 + lo) * npad + j]);
  if (munc) {
    double pk = 0.0;
    for (int a = 0; a < nb; ++a) pk += cf[(size_t)a * mp + (size_t)(1 + k) * pc + j] * cf[(size_t)a * mp + (size_t)(1 + i) * pc + j];
    d2s2 += 2.0 * varK * pk;
  }
  const double dsk = blk[1 + k] / sg, dsi = blk[1 + i] / sg;
  d2sig[t] = sg != 0.0 ? (d2s2 - 2.0 * dsk * dsi) / (2.0 * sg) : __longlong_as_double(0x7ff8000000000000LL);
}

// K-chunks of second_gram_kernel: a function of Npad only (never of nx or of the points per chunk), or what gpg_set_gram_splits asks for
int second_splits(int Npad, int requested) {
  const int ktiles = Npad / 64;
  int s = requested > 0 ? requested : (ktiles < kSecondChunksMax ? ktiles : kSecondChunksMax);
  return s < 1 ? 1 : (s > ktiles ? ktiles : s);
}

// points of the next chunk when `remaining` are left: what gpg_set_second_chunk asks for; else all of them if their rows fit (the
// last chunk), else the largest multiple of 64 whose rows fit (block rows then start on 512-byte boundaries of a column)
int second_points(const gpg_ctx* c, int remaining) {
  const int cap = kSecondMaxRows / (c->d + 1);
  if (c->second_chunk > 0) return std::min(c->second_chunk, remaining);
  return remaining <= cap ? remaining : (cap / 64) * 64;
}

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

int predict_second_once(gpg_ctx* c, int nx, const double* xq, double varK, double* mu, double* dmudx, double* gcov, double* d2mudx2,
                        double* d2sigdx2) {
  if (!c->eval_ready) { c->err = "gpg_setup_eval must succeed before gpg_predict_second"; return -1; }
  if (nx < 1 || !xq) { c->err = "bad gpg_predict_second arguments (nx >= 1, xq not NULL)"; return -1; }
  if (!mu && !dmudx && !gcov && !d2mudx2 && !d2sigdx2) { c->err = "gpg_predict_second: every output pointer is NULL"; return -1; }
  const int d = c->d, bs = d + 1, npairs = bs * (bs + 1) / 2;
  const bool want_mean = mu || dmudx, want_hess = d2mudx2 || d2sigdx2, want_gram = gcov || want_hess;
  const int pc_max = c->second_chunk > 0 ? std::min(c->second_chunk, nx) : std::min(kSecondMaxRows / bs, nx);   // of any chunk
  const int mp_max = ((pc_max * bs + 63) / 64) * 64, npad_max = ((pc_max + 63) / 64) * 64;
  GPG_HIP_OK(c, hipSetDevice(c->device));
  if (gpg_ws_activate(c, 1) != 0) return -2;
  if (int rc = gpg_predict_bufs(c, mp_max)) return rc;
  const bool munc = c->mean_unc != 0 && want_gram;
  if (munc) {
    if (int rc = gpg_meanunc_ensure(c)) return rc;
  }
  const int Npad = c->Npad, ktiles = Npad / 64, nb = c->n_beta;
  const int S = second_splits(Npad, c->gram_splits);
  const int Sm = gpg_joint_mean_slices(c);
  // scratch (the joint posterior's buffer): Gram partials | raw sums | blocks | H1 | H2 | d2mudx2 | d2sigdx2 | K0 | zero difference
  // tensor | mean partials | mean | gradient position
  const size_t b_part = want_gram ? round256(sizeof(double) * (size_t)S * npairs * npad_max) : 0;
  const size_t b_raw = want_hess ? round256(sizeof(double) * (size_t)npairs * npad_max) : 0;
  const size_t b_blk = want_gram ? round256(sizeof(double) * (size_t)pc_max * bs * bs) : 0;
  const size_t b_h = want_hess ? round256(sizeof(double) * (size_t)pc_max * d * d) : 0;
  const size_t b_k0 = round256(sizeof(double) * (size_t)bs * bs), b_rt = round256(sizeof(double) * d);
  const size_t b_mpart = want_mean ? round256(sizeof(double) * (size_t)Sm * mp_max) : 0, b_mean = round256(sizeof(double) * mp_max);
  const size_t need = b_part + b_raw + b_blk + 4 * b_h + b_k0 + b_rt + b_mpart + b_mean + 256;
  if (need > c->jbuf_bytes) {
    if (c->jbuf) (void)hipFree(c->jbuf);
    c->jbuf = nullptr; c->jbuf_bytes = 0;
    if (hipMalloc(&c->jbuf, need) != hipSuccess) {
      (void)hipGetLastError();
      c->jbuf = nullptr;
      c->err = "out of device memory for the scratch of gpg_predict_second (fewer gpg_set_gram_splits chunks or gpg_set_second_chunk points need less)";
      return -2;
    }
    c->jbuf_bytes = need;
  }
  char* base = reinterpret_cast<char*>(c->jbuf);
  auto take = [&](size_t bytes) { char* p = base; base += bytes; return p; };
  double* part = reinterpret_cast<double*>(take(b_part));
  double* sraw = want_hess ? reinterpret_cast<double*>(take(b_raw)) : nullptr;
  double* blk_dev = reinterpret_cast<double*>(take(b_blk));
  double* h1 = reinterpret_cast<double*>(take(b_h));
  double* h2 = reinterpret_cast<double*>(take(b_h));
  double* d2mu_dev = reinterpret_cast<double*>(take(b_h));
  double* d2sig_dev = reinterpret_cast<double*>(take(b_h));
  double* k0 = reinterpret_cast<double*>(take(b_k0));
  double* rt = reinterpret_cast<double*>(take(b_rt));
  double* mpart = reinterpret_cast<double*>(take(b_mpart));
  double* mean_dev = reinterpret_cast<double*>(take(b_mean));
  int* gpos = reinterpret_cast<int*>(take(256));

  const AsmParams p = c->eval_params;
  if (want_gram) {   // K0: the kernel table at a zero difference tensor, one point with itself (the entries gpg_predict_joint takes for Kqq)
    GPG_HIP_OK(c, hipMemsetAsync(rt, 0, b_rt, c->stream));
    GPG_HIP_OK(c, hipMemsetAsync(gpos, 0, sizeof(int), c->stream));
    if (gpg_kern_rtensor_run(p.kernel, d, 1, 1, 1, 1, 1, p.theta, p.hp_kernel, rt, gpos, gpos, k0, c->stream) != 0) {
      c->err = "gpg_predict_second: the kernel-table launch for K0 failed";
      return -2;
    }
  }
  const int G = bs <= 5 ? 5 : (bs <= 9 ? 9 : kSecondGroup);
  const int ngroups = (bs + G - 1) / G;
  std::vector<double> xt, hmean;
  for (int j0 = 0, pc = 0; j0 < nx; j0 += pc) {
    pc = second_points(c, nx - j0);
    const int m = pc * bs, mp = ((m + 63) / 64) * 64, T = (pc + 63) / 64, npad = T * 64;
    xt.assign((size_t)mp * d, 0.0);   // [d x mp], query point fastest
    for (int j = 0; j < pc; ++j)
      for (int k = 0; k < d; ++k) xt[(size_t)k * mp + j] = xq[(size_t)(j0 + j) * d + k];
    GPG_HIP_OK(c, hipMemcpyAsync(c->xq_dev, xt.data(), sizeof(double) * xt.size(), hipMemcpyHostToDevice, c->stream));
    GPG_HIP_OK(c, hipMemsetAsync(c->Wt, 0, sizeof(double) * (size_t)mp * Npad, c->stream));
    GPG_HIP_OK(c, hipMemsetAsync(c->info, 0, sizeof(int), c->stream));
    gpg_launch_cross_joint(c, p, pc, bs, mp);
    if (want_mean) {   // before the sweep: mean = prior + (Kqy P^-1) (p * alpha)
      gpg_launch_joint_mean(c, mp, m, pc, mpart, mean_dev);
      hmean.resize(m);
      GPG_HIP_OK(c, hipMemcpyAsync(hmean.data(), mean_dev, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_gram) {
      gpg_prof_begin(c, GPG_PROF_TRSM, (double)m * Npad * Npad);
      gpg_forward_rows(c, c->Wt, mp, mp, m);
      gpg_prof_end(c);
      if (munc) {
        if (int rc = gpg_meanunc_rows(c, c->Wt, mp, m, pc)) return rc;
      }
      double rows_read = m;                            // rows of Z the launches read: every row once, and both groups of every off-diagonal tile
      for (int gj = 1; gj < ngroups; ++gj) rows_read += (double)gj * pc * (G + std::min(G, bs - gj * G));
      gpg_prof_begin(c, GPG_PROF_REDUCE, 8.0 * rows_read * Npad);
#define SECOND_GRAM(GV, DIAGV, TILES)                                                                                             \
  hipLaunchKernelGGL((second_gram_kernel<GV, DIAGV>), dim3(T, S, TILES), dim3(256), 0, c->stream, (const double*)c->Wt, mp, pc, bs, \
                     ktiles, S, npairs, npad, part)
      if (G == 5) SECOND_GRAM(5, true, 1);
      else if (G == 9) SECOND_GRAM(9, true, 1);
      else {
        SECOND_GRAM(kSecondGroup, true, ngroups);
        SECOND_GRAM(kSecondGroup, false, ngroups * (ngroups - 1) / 2);
      }
#undef SECOND_GRAM
      gpg_prof_end(c);
      SecondFinish f{part, S, npairs, npad, pc, bs, mp, nb, munc ? 1 : 0, k0, munc ? c->mu_cf : nullptr, varK, blk_dev, sraw};
      hipLaunchKernelGGL(second_finish_kernel, dim3(T, npairs), dim3(64), 0, c->stream, f);
      if (gcov)
        GPG_HIP_OK(c, hipMemcpyAsync(gcov + (size_t)j0 * bs * bs, blk_dev, sizeof(double) * (size_t)pc * bs * bs, hipMemcpyDeviceToHost,
                                     c->stream));
    }
    if (want_hess) {
      // the 64-row tiles that hold the value rows, all of their rows solved (the derivative rows that share the last tile ride
      // along: the Gram kernel has read them)
      gpg_backward_rows(c, c->Wt, mp, std::min(npad, m), c->gradbuf + (size_t)2 * mp * GPG_MAX_DIM);
      if (munc) gpg_meanunc_update_rows(c, c->Wt, mp, pc);
      gpg_launch_hess_contract(c, p, pc, mp, h1, h2);
      const int total = pc * d * d;
      hipLaunchKernelGGL(second_hess_kernel, dim3((total + 255) / 256), dim3(256), 0, c->stream, pc, d, npad, mp, nb, munc ? 1 : 0, varK,
                         (const double*)h1, (const double*)h2, (const double*)sraw, (const double*)blk_dev,
                         munc ? (const double*)c->mu_cf : (const double*)nullptr, d2mu_dev, d2sig_dev);
      if (d2mudx2)
        GPG_HIP_OK(c, hipMemcpyAsync(d2mudx2 + (size_t)j0 * d * d, d2mu_dev, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream));
      if (d2sigdx2)
        GPG_HIP_OK(c, hipMemcpyAsync(d2sigdx2 + (size_t)j0 * d * d, d2sig_dev, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream));
    }
    GPG_HIP_OK(c, hipMemcpyAsync(c->h_info, c->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));   // the dataflow sweeps report here
    GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
    GPG_HIP_OK(c, hipGetLastError());
    GPG_LAUNCH_OK(c);
    if (gpg_solve_failure(c)) return -4;
    if (want_mean) {
      for (int j = 0; j < pc; ++j) {
        if (mu) mu[j0 + j] = hmean[j];
        if (dmudx)
          for (int k = 0; k < d; ++k) dmudx[(size_t)(j0 + j) * d + k] = hmean[(size_t)(k + 1) * pc + j];
      }
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int gpg_predict_second(gpg_ctx* c, int nx, const double* xq, double varK, double* mu, double* dmudx, double* gcov, double* d2mudx2,
                       double* d2sigdx2) {
  if (!c) return -1;
  return gpg_with_fallback(c, [&] { return predict_second_once(c, nx, xq, varK, mu, dmudx, gcov, d2mudx2, d2sigdx2); });
}

int gpg_set_second_chunk(gpg_ctx* c, int points) {
  if (!c) return -1;
  if (points < 0) { c->err = "points per chunk of gpg_predict_second must be >= 0 (0 = chosen from the dimension)"; return -1; }
  if ((long long)points * (c->d + 1) > kSecondMaxRows) {
    c->err = "points per chunk of gpg_predict_second: points (dim + 1) rows must not exceed 4096";
    return -1;
  }
  c->second_chunk = points;
  return 0;
}

}  // extern "C"
