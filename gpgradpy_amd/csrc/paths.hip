// Posterior sample paths by pathwise conditioning (gpg_paths_setup / gpg_paths_eval / gpg_paths_coeff, include/gpgrad.h):
// Matheron's rule on the factor kept by gpg_setup_eval*, with a random-Fourier-feature prior.  For path s
//     f_s(x) = m(x) + k(x, X) c_s + sqrt(varK) phi(x)' w_s,        c_s = alpha - sqrt(varK) Kcov^-1 (Phi_X w_s + D^(1/2) z_s),
// phi(x)_m = sqrt(2 / M) cos(omega_m . x + b_m), Phi_X its values (and x-derivatives on the gradient rows) at the training rows,
// D = diag(Kcov) - diag(Kern).  Given (omega, b, w, z) a path is one fixed smooth function of x: any number of calls at any
// points evaluate the same function.
//
// Set-up (once per draw, no factorisation), all on the context's stream:
//   1. paths_ddiag_kernel: D from dvec / invp / eta in the assembly's own operation order, so that Kern + D is the diagonal of the
//      matrix gpg_get_matrix(1) returns, bit for bit;
//   2. feature_rows_kernel on the training rows (gpos layout, masked points have no gradient rows): G_X = Phi_X W', never Phi_X;
//   3. paths_rhs_kernel: rows (G_X + D^(1/2) z) P^-1 in the RHS-rows layout U[c * Sp + s], Sp = S padded to 64;
//   4. gpg_forward_rows and gpg_backward_rows: U <- (L L')^-1 P^-1 (.), as alpha is formed from y - V beta.
// What is kept is U, not c_s: P c_s = zvec - sqrt(varK) U with zvec = P alpha of the posterior, and the evaluation uses the two
// terms separately.  The mean part k(x, X) alpha cancels by a factor ~ cond(Kcov) and is therefore summed with compensation by the
// kernels of gpg_predict_joint (joint_mean_*): a path's mean part is the `mean` of gpg_predict_joint / gpg_predict_second at that
// point, the same bits, and a zero draw returns exactly that mean.  Only the deviation goes through the plain MFMA sum.
//
// Evaluation (per chunk of query points as in gpg_predict_second, gpg_set_second_chunk applies; the automatic chunk holds
// 4096 / (Sp / 64) rows, at least 256: a function of S and d only; no sweep, no N^2 work):
//   1. cross_joint_kernel writes the rows of Kqy P^-1 into Wt (joint.hip), joint_mean_* their product with zvec plus the mean function;
//   2. rows_coeff_splitk_kernel: partial[r, s] = sum over the training columns c of one K-chunk of Wt[c, r] U[c, s] on fp64 MFMA,
//      64 x 64 output tiles over (query rows, paths), grid = (row tiles, path tiles, K-chunks).  Operand layouts as
//      rows_gram_splitk_kernel: both operands are "RHS rows" arrays, 16 consecutive rows of a column are contiguous;
//   3. feature_rows_kernel on the query rows (derivative-major like gpg_predict_joint): G_q = Phi_q W';
//   4. paths_finish_kernel adds the partials in chunk order, f = mean + sqrt(varK) (G_q - sum), and transposes to [S, nx] / [S, nx, d].
// One device-to-host copy per output and one synchronisation per call.  The K-chunk count is min(Npad / 64, 64) or
// gpg_set_gram_splits: never a function of nx, S or the device; the features are added in one fixed order.  Ordinary grids, no
// atomics: a point's result does not depend on the points that share its call, on the chunking or on gpg_set_max_workgroups.
// gpg_prof categories: cross rows under GPG_PROF_ASSEMBLY (bytes of Wt written), rows_coeff_splitk_kernel under GPG_PROF_GEMM_TRAIL
// (2 rows N S flops), feature_rows_kernel under GPG_PROF_REDUCE, the two sweeps of the set-up under GPG_PROF_TRSM.
//
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / scratch bytes / waves per SIMD): rows_coeff_splitk_kernel
// 50 / 0 / 5; feature_rows_kernel d = 1: 60 / 0 / 8, d = 4: 64 / 0 / 8, d = 8: 77 / 0 / 6, d = 16: 131 / 0 / 3; paths_finish_kernel
// 40 / 0 / 8.  No kernel of this file uses scratch.
// Measured on one MI355X (tools/paths_time.py, S = 64, M = 4096, n = 2000, d = 8; include/gpgrad.h and README.md hold the rest):
// set-up 11.2 ms (feature kernel 0.77 ms, two sweeps 6.45 ms); evaluation with gradients at nx = 64 0.57 ms: cross rows 18 us,
// product kernel 46 us (29 TFLOP/s), feature kernel 368 us -- the feature kernel on the query rows, one workgroup per point over
// all M features, is two thirds of the call; at nx = 448 1.22 ms (102 / 228 (40.8 TFLOP/s) / 484 us).
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>
#include "gpg_internal.h"
#include "kernel_fn.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kPathsMaxRows = 4096;    // rows of a chunk, padded to 64: what Wt is sized for by the other posterior calls as well
constexpr int kPathsChunksMax = 64;    // K-chunks of the product kernel when gpg_set_gram_splits is not set: min(Npad / 64, this)
constexpr int kPathsMaxS = 1024, kPathsMaxM = 65536;
constexpr int kFeatBlock = 256;        // features per trip of feature_rows_kernel (one per thread)

// The rows the feature kernel writes for point p.  Training rows (gpos != nullptr): value row p, derivative row n + k ng + gpos[p] when
// the point carries a gradient; query rows: value row p, derivative row (k + 1) npts + p.  Coordinate k of point p is X[k ldx + p].
struct FeatRows {
  const double* X;
  int ldx, npts, nblk;   // nblk = 1: value rows only, d + 1: derivative rows too
  const int* gpos;
  int n, ng;
};

// out[row * Sp + s] = sum_m Phi[row, m] w[s, m] for the nblk rows of point blockIdx.x and the 64 paths of tile blockIdx.y:
// value row sqrt(2 / M) cos(omega_m . x + b_m), derivative row k -sqrt(2 / M) omega_mk sin(.).  Per trip of 256 features every thread
// evaluates the phase and sincos of ONE feature into LDS (once per (point, feature), reused by the D + 1 rows and the 64 paths);
// then thread (lane <-> path, wave q) adds the 64 features of quarter q of the trip in ascending order, reading omega through
// wave-uniform loads and w^T [M x Sp] coalesced.  The four quarters are added in wave order at the end: one fixed order, whatever
// the grid.  Path columns S .. Sp - 1 of w^T are zero, so those columns of out are written as zeros.
template <int D>
__global__ void __launch_bounds__(256) feature_rows_kernel(FeatRows R, int M, const double* __restrict__ omega,
                                                           const double* __restrict__ phase, const double* __restrict__ wT, int Sp,
                                                           double scale, double* __restrict__ out) {
  __shared__ double cs[kFeatBlock], sn[kFeatBlock];
  __shared__ double red[3][D + 1][64];
  const int lane = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = blockIdx.x, s = blockIdx.y * 64 + lane;
  const bool deriv = R.nblk > 1;
  double x[D], acc[D + 1];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = R.X[(size_t)k * R.ldx + p];
#pragma unroll
  for (int k = 0; k <= D; ++k) acc[k] = 0.0;
  for (int m0 = 0; m0 < M; m0 += kFeatBlock) {
    {
      const int m = m0 + (int)threadIdx.x;
      double c = 0.0, sv = 0.0;
      if (m < M) {
        double arg = phase[m];
#pragma unroll
        for (int k = 0; k < D; ++k) arg += omega[(size_t)m * D + k] * x[k];
        sincos(arg, &sv, &c);
      }
      cs[threadIdx.x] = c;
      sn[threadIdx.x] = sv;
    }
    __syncthreads();
    const int mlo = m0 + q * 64, mhi = min(M, mlo + 64);
    for (int m = mlo; m < mhi; ++m) {
      const double wv = wT[(size_t)m * Sp + s];
      acc[0] += cs[m - m0] * wv;
      if (deriv) {
        const double t = sn[m - m0] * wv;
#pragma unroll
        for (int k = 0; k < D; ++k) acc[k + 1] += omega[(size_t)m * D + k] * t;
      }
    }
    __syncthreads();
  }
  if (q > 0) {
#pragma unroll
    for (int k = 0; k <= D; ++k) red[q - 1][k][lane] = acc[k];
  }
  __syncthreads();
  if (q != 0) return;
#pragma unroll
  for (int k = 0; k <= D; ++k) acc[k] = ((acc[k] + red[0][k][lane]) + red[1][k][lane]) + red[2][k][lane];
  out[(size_t)p * Sp + s] = scale * acc[0];
  if (!deriv) return;
  const int gp = R.gpos ? R.gpos[p] : p;
  if (gp < 0) return;   // a masked training point: no gradient rows
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const size_t row = R.gpos ? (size_t)R.n + (size_t)k * R.ng + gp : (size_t)(k + 1) * R.npts + p;
    out[row * Sp + s] = -scale * acc[k + 1];
  }
}

// dd[r] = diag(Kcov)[r] - diag(Kern)[r] for r < N (0 beyond), both diagonals rounded as assemble_kernel rounds them in modes 2 and 1
// (assembly.hip; no contraction, as that file is compiled): dvec = diag(Kern) + noise / varK is what prep_diag_kernel left.
// Clipped at zero (without noise and nugget the difference is rounding).
__global__ void __launch_bounds__(256) paths_ddiag_kernel(AsmParams P, const double* __restrict__ dvec, const double* __restrict__ invp,
                                                          double* __restrict__ dd) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= P.Npad) return;
  if (r >= P.N) { dd[r] = 0.0; return; }
  const int blk = (P.use_grad && r >= P.n) ? 1 + (r - P.n) / P.ng : 0;
  double kd = 1.0;
  if (blk > 0) kd = P.kernel == GPG_KERNEL_MA5F2 ? P.theta[blk - 1] * (5.0 / 3.0) : 2.0 * P.theta[blk - 1];
  const double dv = dvec[r];
  double o;
  if (P.precon) {
    const double ip = invp[r];
    const double kc = (ip * dv) * ip;
    o = P.varK * (kc + P.eta);
    const double p = sqrt(dv);
    o = (p * o) * p;
  } else {
    o = P.varK * (dv + P.eta);
  }
  const double v = o - kd;
  dd[r] = v > 0.0 ? v : 0.0;
}

// U[c * Sp + s] <- (G_X[c, s] + sqrt(dd[c]) z[s, c]) invp[c] for c < N, s < S; zero elsewhere (the sweeps skip rows >= S, and the product
// kernel reads all Npad columns).  zT [Npad x Sp] may be nullptr (no noise / nugget draw).
__global__ void __launch_bounds__(256) paths_rhs_kernel(int N, int Npad, int S, int Sp, const double* __restrict__ dd,
                                                        const double* __restrict__ zT, const double* __restrict__ invp,
                                                        double* __restrict__ U) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)Npad * Sp) return;
  const int c = (int)(t / Sp), s = (int)(t - (size_t)c * Sp);
  double v = 0.0;
  if (c < N && s < S) {
    v = U[t];
    if (zT) v += sqrt(dd[c]) * zT[t];
    v *= invp[c];
  }
  U[t] = v;
}

// Partial products of the cross rows with the kept solves (both in the RHS-rows layout, mp and Sp multiples of 64):
//   partial[((s nrt + ti) npt + tj)][q * 64 + p] = sum over the columns c of K-chunk s of Wt[c mp + ti 64 + p] U[c Sp + tj 64 + q]
// grid = (nrt row tiles, npt path tiles, splits); chunk s holds the whole 64-column tiles [s ktiles / splits, (s + 1) ktiles / splits).
// One workgroup = 4 waves, wave (wm, wn) owns the 32 x 32 quadrant as 2 x 2 MFMA 16 x 16 x 4 fp64 blocks, in the register layout
// of rows_gram_splitk_kernel (joint.hip): lane (l15, l4) feeds row l15 of k-slice l4 of either operand and holds
// C[l15, 4 r + l4] in element r.  Operands come straight from global memory: 16 consecutive rows are contiguous, so every 16-lane
// group reads 128 bytes; a k-step of 4 columns is 4 loads and 4 MFMAs per lane.  Columns N .. Npad - 1 of Wt and U are zero.
__global__ void __launch_bounds__(256) rows_coeff_splitk_kernel(const double* __restrict__ Wt, int mp, const double* __restrict__ U, int Sp,
                                                                int ktiles, int splits, double* __restrict__ partial) {
  const int ti = blockIdx.x, tj = blockIdx.y, s = blockIdx.z;
  const int k0 = (int)((long long)s * ktiles / splits) * 64, k1 = (int)((long long)(s + 1) * ktiles / splits) * 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wm = w & 1, wn = w >> 1, l15 = lane & 15, l4 = lane >> 4;
  const double* zp = Wt + (size_t)(k0 + l4) * mp + ti * 64 + wm * 32 + l15;
  const double* zq = U + (size_t)(k0 + l4) * Sp + tj * 64 + wn * 32 + l15;
  const size_t stp = (size_t)4 * mp, stq = (size_t)4 * Sp;
  d4 acc[2][2] = {};
  for (int k = k0; k < k1; k += 16) {   // chunks are whole 64-column tiles: four k-steps per trip, their 16 loads in flight together
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double fm0 = zp[0], fm1 = zp[16], fn0 = zq[0], fn1 = zq[16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn0, fm0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn0, fm1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn1, fm0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn1, fm1, acc[1][1], 0, 0, 0);
      zp += stp;
      zq += stq;
    }
  }
  double* out = partial + (((size_t)s * gridDim.x + ti) * gridDim.y + tj) * 4096 + wm * 32 + l15;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(wn * 32 + ni * 16 + 4 * r + l4) * 64 + mi * 16] = acc[ni][mi][r];
}

struct PathsFinish {
  const double* partial; int splits;
  const double *mean, *Gq;   // mean [rows] of the chunk (mean function included); G_q [rows x Sp]
  int m, pc, S, Sp, d;
  int nx, j0;                // points of the whole call, first point of the chunk
  double sv;                 // sqrt(varK)
  double *f, *dfdx;          // device [S, nx], [S, nx, d]
};

// Entry (row p of row tile blockIdx.x, path q of path tile blockIdx.y), one per thread (grid = (row tiles, path tiles, 16)): the
// K-chunk partials in chunk order, value = mean[row] + sqrt(varK) (G_q[row, s] - sum), written to f[s, j] (row block 0) or
// dfdx[s, j, blk - 1].
__global__ void __launch_bounds__(256) paths_finish_kernel(PathsFinish a) {
  const int e = blockIdx.z * 256 + threadIdx.x;
  const int p = e & 63, q = e >> 6;
  const int row = blockIdx.x * 64 + p, s = blockIdx.y * 64 + q;
  if (row >= a.m || s >= a.S) return;
  const double* part = a.partial + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 4096 + e;
  const size_t stride = (size_t)gridDim.x * gridDim.y * 4096;
  double g = 0.0;
  int c = 0;
  for (; c + 8 <= a.splits; c += 8) {   // eight loads in flight, added in chunk order all the same
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(c + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) g += v[u];
  }
  for (; c < a.splits; ++c) g += part[(size_t)c * stride];
  const double val = a.mean[row] + a.sv * (a.Gq[(size_t)row * a.Sp + s] - g);
  const int blk = row / a.pc, j = row - blk * a.pc;
  const size_t pt = (size_t)s * a.nx + a.j0 + j;
  if (blk == 0) a.f[pt] = val;
  else a.dfdx[pt * a.d + (blk - 1)] = val;
}

// c [S, N] row-major = (zvec - sqrt(varK) U) invp
__global__ void __launch_bounds__(256) paths_coeff_kernel(int N, int S, int Sp, double sv, const double* __restrict__ zvec,
                                                          const double* __restrict__ invp, const double* __restrict__ U,
                                                          double* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)N * S) return;
  const int s = (int)(t / N), c = (int)(t - (size_t)s * N);
  out[t] = (zvec[c] - sv * U[(size_t)c * Sp + s]) * invp[c];
}

int paths_splits(int Npad, int requested) {
  const int ktiles = Npad / 64;
  int s = requested > 0 ? requested : (ktiles < kPathsChunksMax ? ktiles : kPathsChunksMax);
  return s < 1 ? 1 : (s > ktiles ? ktiles : s);
}

// Most points of an automatic chunk: 4096 rows shared among the Sp / 64 path tiles, so that the product partials stay within
// 64 K-chunks x 64 (row, path) tiles x 32 KB = 128 MB whatever S is.  A function of S and the rows per point only, never of nx.
int paths_point_cap(const gpg_ctx* c, int qblk) {
  const int rows = std::max(256, kPathsMaxRows / (c->paths_Sp / 64));
  return std::max(1, rows / qblk);
}

// points of the next chunk when `remaining` are left: what gpg_set_second_chunk asks for; else all of them if they fit the cap (the
// last chunk), else the largest multiple of 64 within the cap (the cap itself below 64)
int paths_points(const gpg_ctx* c, int remaining, int qblk) {
  const int cap = paths_point_cap(c, qblk);
  if (c->second_chunk > 0) return std::min(c->second_chunk, remaining);
  return remaining <= cap ? remaining : (cap >= 64 ? (cap / 64) * 64 : cap);
}

// The host arrays that asynchronous copies read live in the calling function: a return before its final synchronisation waits for
// the stream first (declare this AFTER those arrays, so that it is destroyed before them).
struct StreamDrain {
  gpg_ctx* c; bool done = false;
  explicit StreamDrain(gpg_ctx* ctx) : c(ctx) {}
  ~StreamDrain() { if (!done) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); } }
};

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

int paths_scratch(gpg_ctx* c, size_t need, const char* what) {
  if (need <= c->paths_scr_bytes) return 0;
  if (c->paths_scr) (void)hipFree(c->paths_scr);
  c->paths_scr = nullptr; c->paths_scr_bytes = 0;
  if (hipMalloc(&c->paths_scr, need) != hipSuccess) {
    (void)hipGetLastError();
    c->paths_scr = nullptr;
    c->err = std::string("out of device memory for the scratch of ") + what;
    return -2;
  }
  c->paths_scr_bytes = need;
  return 0;
}

void launch_feature_rows(gpg_ctx* c, const FeatRows& R, double* out) {
  const int M = c->paths_M, Sp = c->paths_Sp;
  const double scale = std::sqrt(2.0 / M);
  gpg_for_kern_d(GPG_KERNEL_SQEXP, c->d, [&](auto, auto D) {
    hipLaunchKernelGGL((feature_rows_kernel<decltype(D)::value>), dim3(R.npts, Sp / 64), dim3(256), 0, c->stream, R, M,
                       (const double*)c->paths_omega, (const double*)c->paths_phase, (const double*)c->paths_wT, Sp, scale, out);
  });
}

int paths_setup_once(gpg_ctx* c, int S, int M, const double* omega, const double* phase, const double* w, const double* z, double varK) {
  if (!c->eval_ready) { c->err = "gpg_setup_eval must succeed before gpg_paths_setup"; return -1; }
  if (S < 1 || S > kPathsMaxS) { c->err = "gpg_paths_setup: n_paths must be in [1, 1024]"; return -1; }
  if (M < 1 || M > kPathsMaxM) { c->err = "gpg_paths_setup: n_feat must be in [1, 65536]"; return -1; }
  if (!omega || !phase || !w) { c->err = "gpg_paths_setup: omega / phase / w is NULL"; return -1; }
  if (!(varK >= 0.0) || std::isinf(varK)) { c->err = "gpg_paths_setup: varK must be finite and >= 0"; return -1; }
  if (c->mean_unc) {
    c->err = "gpg_paths_setup: paths with re-drawn mean coefficients are out of scope: switch gpg_set_mean_uncertainty off";
    return -1;
  }
  c->paths_ready = false;
  GPG_HIP_OK(c, hipSetDevice(c->device));
  if (gpg_ws_activate(c, 1) != 0) return -2;
  const int d = c->d, N = c->N, Npad = c->Npad, Sp = ((S + 63) / 64) * 64;
  // every part starts on a 256-byte boundary: the dataflow sweeps rely on 64 x 64 tiles of U that share no cache line (chol_device.h)
  auto pad32 = [](size_t n) { return (n + 31) & ~(size_t)31; };
  const size_t e_om = pad32((size_t)M * d), e_ph = pad32((size_t)M), e_w = (size_t)M * Sp, e_u = (size_t)Npad * Sp, e_dd = (size_t)Npad,
               e_tb = (size_t)Sp * 64;
  const size_t elems = e_om + e_ph + e_w + e_u + e_dd + e_tb;
  if (elems > c->paths_buf_elems) {
    GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
    if (c->paths_buf) (void)hipFree(c->paths_buf);
    c->paths_buf = nullptr; c->paths_buf_elems = 0;
    if (hipMalloc(&c->paths_buf, sizeof(double) * elems) != hipSuccess) {
      (void)hipGetLastError();
      c->paths_buf = nullptr;
      c->err = "out of device memory for the sample paths (features, draws and the kept solves)";
      return -2;
    }
    c->paths_buf_elems = elems;
  }
  c->paths_omega = c->paths_buf;
  c->paths_phase = c->paths_omega + e_om;
  c->paths_wT = c->paths_phase + e_ph;
  c->paths_U = c->paths_wT + e_w;
  c->paths_dd = c->paths_U + e_u;
  c->paths_tb = c->paths_dd + e_dd;
  c->paths_S = S; c->paths_Sp = Sp; c->paths_M = M; c->paths_sv = std::sqrt(varK);
  // the draws, path fastest: w^T [M x Sp]; z^T [Npad x Sp] in the scratch (read by paths_rhs_kernel only)
  std::vector<double> wT(e_w, 0.0), zT;
  for (int s = 0; s < S; ++s)
    for (int m = 0; m < M; ++m) wT[(size_t)m * Sp + s] = w[(size_t)s * M + m];
  StreamDrain drain(c);
  double* zT_dev = nullptr;
  if (z) {
    if (int rc = paths_scratch(c, round256(sizeof(double) * e_u), "gpg_paths_setup")) return rc;
    zT_dev = c->paths_scr;
    zT.assign(e_u, 0.0);
    for (int s = 0; s < S; ++s)
      for (int r = 0; r < N; ++r) zT[(size_t)r * Sp + s] = z[(size_t)s * N + r];
    GPG_HIP_OK(c, hipMemcpyAsync(zT_dev, zT.data(), sizeof(double) * e_u, hipMemcpyHostToDevice, c->stream));
  }
  GPG_HIP_OK(c, hipMemcpyAsync(c->paths_omega, omega, sizeof(double) * (size_t)M * d, hipMemcpyHostToDevice, c->stream));
  GPG_HIP_OK(c, hipMemcpyAsync(c->paths_phase, phase, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  GPG_HIP_OK(c, hipMemcpyAsync(c->paths_wT, wT.data(), sizeof(double) * e_w, hipMemcpyHostToDevice, c->stream));
  GPG_HIP_OK(c, hipMemsetAsync(c->info, 0, sizeof(int), c->stream));
  const AsmParams p = c->eval_params;
  hipLaunchKernelGGL(paths_ddiag_kernel, dim3((Npad + 255) / 256), dim3(256), 0, c->stream, p, (const double*)c->dvec,
                     (const double*)c->invp, c->paths_dd);
  const FeatRows R{c->Xt, c->n, c->n, c->use_grad ? d + 1 : 1, c->gpos, c->n, c->ng > 0 ? c->ng : 1};
  gpg_prof_begin(c, GPG_PROF_REDUCE, 2.0 * N * (double)M * S);
  launch_feature_rows(c, R, c->paths_U);
  gpg_prof_end(c);
  hipLaunchKernelGGL(paths_rhs_kernel, dim3((unsigned)((e_u + 255) / 256)), dim3(256), 0, c->stream, N, Npad, S, Sp,
                     (const double*)c->paths_dd, (const double*)zT_dev, (const double*)c->invp, c->paths_U);
  gpg_prof_begin(c, GPG_PROF_TRSM, (double)S * Npad * Npad);
  gpg_forward_rows(c, c->paths_U, Sp, Sp, S);
  gpg_prof_end(c);
  gpg_prof_begin(c, GPG_PROF_TRSM, (double)S * Npad * Npad);
  gpg_backward_rows(c, c->paths_U, Sp, S, c->paths_tb);
  gpg_prof_end(c);
  GPG_HIP_OK(c, hipMemcpyAsync(c->h_info, c->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));   // the dataflow sweeps report here
  GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
  drain.done = true;
  GPG_HIP_OK(c, hipGetLastError());
  GPG_LAUNCH_OK(c);
  if (gpg_solve_failure(c)) return -4;
  c->paths_ready = true;
  return 0;
}

int paths_check(gpg_ctx* c, const char* who) {
  if (!c->paths_ready || !c->eval_ready) {
    c->err = std::string(who) + ": no sample paths are set up for this posterior (gpg_paths_setup after the last gpg_setup_eval / "
             "gpg_set_data / gpg_set_grad_mask / gpg_set_mean_order)";
    return -1;
  }
  return 0;
}

struct XqSwap {   // the cross-row and mean launchers read the query points through c->xq_dev: point it at a chunk, put it back on return
  gpg_ctx* c; double* keep;
  explicit XqSwap(gpg_ctx* ctx) : c(ctx), keep(ctx->xq_dev) {}
  ~XqSwap() { c->xq_dev = keep; }
};

int paths_eval_once(gpg_ctx* c, int nx, const double* xq, double* f, double* dfdx) {
  if (int rc = paths_check(c, "gpg_paths_eval")) return rc;
  if (nx < 1 || !xq || !f) { c->err = "bad gpg_paths_eval arguments (nx >= 1, xq and f not NULL)"; return -1; }
  const int d = c->d, qblk = dfdx ? d + 1 : 1, S = c->paths_S, Sp = c->paths_Sp;
  const int pc_max = std::min(c->second_chunk > 0 ? c->second_chunk : paths_point_cap(c, qblk), nx);   // of any chunk
  const int mp_max = ((pc_max * qblk + 63) / 64) * 64;
  GPG_HIP_OK(c, hipSetDevice(c->device));
  if (gpg_ws_activate(c, 1) != 0) return -2;
  if (int rc = gpg_predict_bufs(c, mp_max)) return rc;
  const int N = c->N, Npad = c->Npad, ktiles = Npad / 64, npt = Sp / 64;
  const int splits = paths_splits(Npad, c->gram_splits);
  const int Sm = gpg_joint_mean_slices(c);
  // the query points of every chunk, [d x mp] each (point fastest), uploaded once
  std::vector<double> xt;
  std::vector<size_t> xoff;
  for (int j0 = 0, pc = 0; j0 < nx; j0 += pc) {
    pc = paths_points(c, nx - j0, qblk);
    const int mp = ((pc * qblk + 63) / 64) * 64;
    xoff.push_back(xt.size());
    xt.resize(xt.size() + (size_t)mp * d, 0.0);
    double* dst = xt.data() + xoff.back();
    for (int j = 0; j < pc; ++j)
      for (int k = 0; k < d; ++k) dst[(size_t)k * mp + j] = xq[(size_t)(j0 + j) * d + k];
  }
  // scratch: product partials | G_q | mean partials | mean | query points | f | dfdx
  const size_t b_part = round256(sizeof(double) * (size_t)splits * (mp_max / 64) * npt * 4096);
  const size_t b_gq = round256(sizeof(double) * (size_t)mp_max * Sp);
  const size_t b_mpart = round256(sizeof(double) * (size_t)Sm * mp_max), b_mean = round256(sizeof(double) * mp_max);
  const size_t b_xq = round256(sizeof(double) * xt.size());
  const size_t b_f = round256(sizeof(double) * (size_t)S * nx), b_df = dfdx ? round256(sizeof(double) * (size_t)S * nx * d) : 0;
  if (int rc = paths_scratch(c, b_part + b_gq + b_mpart + b_mean + b_xq + b_f + b_df,
                             "gpg_paths_eval (fewer gpg_set_second_chunk points or gpg_set_gram_splits chunks need less)"))
    return rc;
  char* base = reinterpret_cast<char*>(c->paths_scr);
  auto take = [&](size_t bytes) { char* q = base; base += bytes; return reinterpret_cast<double*>(q); };
  double* part = take(b_part);
  double* gq = take(b_gq);
  double* mpart = take(b_mpart);
  double* mean_dev = take(b_mean);
  double* xq_all = take(b_xq);
  double* f_dev = take(b_f);
  double* df_dev = dfdx ? take(b_df) : nullptr;
  StreamDrain drain(c);
  GPG_HIP_OK(c, hipMemcpyAsync(xq_all, xt.data(), sizeof(double) * xt.size(), hipMemcpyHostToDevice, c->stream));
  const AsmParams p = c->eval_params;
  XqSwap swap(c);
  int chunk = 0;
  for (int j0 = 0, pc = 0; j0 < nx; j0 += pc, ++chunk) {
    pc = paths_points(c, nx - j0, qblk);
    const int m = pc * qblk, mp = ((m + 63) / 64) * 64, nrt = mp / 64;
    c->xq_dev = xq_all + xoff[chunk];
    GPG_HIP_OK(c, hipMemsetAsync(c->Wt, 0, sizeof(double) * (size_t)mp * Npad, c->stream));
    gpg_prof_begin(c, GPG_PROF_ASSEMBLY, 8.0 * m * (double)N);
    gpg_launch_cross_joint(c, p, pc, qblk, mp);
    gpg_prof_end(c);
    gpg_launch_joint_mean(c, mp, m, pc, mpart, mean_dev);   // mean function + (Kqy P^-1) (P alpha): the mean of gpg_predict_joint
    gpg_prof_begin(c, GPG_PROF_GEMM_TRAIL, 2.0 * m * (double)N * S);
    hipLaunchKernelGGL(rows_coeff_splitk_kernel, dim3(nrt, npt, splits), dim3(256), 0, c->stream, (const double*)c->Wt, mp,
                       (const double*)c->paths_U, Sp, ktiles, splits, part);
    gpg_prof_end(c);
    const FeatRows R{c->xq_dev, mp, pc, qblk, nullptr, 0, 0};
    gpg_prof_begin(c, GPG_PROF_REDUCE, 2.0 * m * (double)c->paths_M * S);
    launch_feature_rows(c, R, gq);
    gpg_prof_end(c);
    const PathsFinish a{part, splits, mean_dev, gq, m, pc, S, Sp, d, nx, j0, c->paths_sv, f_dev, df_dev};
    hipLaunchKernelGGL(paths_finish_kernel, dim3(nrt, npt, 16), dim3(256), 0, c->stream, a);
  }
  GPG_HIP_OK(c, hipMemcpyAsync(f, f_dev, sizeof(double) * (size_t)S * nx, hipMemcpyDeviceToHost, c->stream));
  if (dfdx) GPG_HIP_OK(c, hipMemcpyAsync(dfdx, df_dev, sizeof(double) * (size_t)S * nx * d, hipMemcpyDeviceToHost, c->stream));
  GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
  drain.done = true;
  GPG_HIP_OK(c, hipGetLastError());
  GPG_LAUNCH_OK(c);
  return 0;
}

// host allocation failures of the staging arrays must not cross the C ABI
template <class F>
int paths_guarded(gpg_ctx* c, const char* who, F f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    c->err = std::string(who) + ": out of host memory for the staging arrays";
    return -2;
  }
}

}  // namespace

extern "C" {

int gpg_paths_setup(gpg_ctx* c, int n_paths, int n_feat, const double* omega, const double* phase, const double* w, const double* z,
                    double varK) {
  if (!c) return -1;
  return paths_guarded(c, "gpg_paths_setup",
                       [&] { return gpg_with_fallback(c, [&] { return paths_setup_once(c, n_paths, n_feat, omega, phase, w, z, varK); }); });
}

int gpg_paths_eval(gpg_ctx* c, int nx, const double* xq, double* f, double* dfdx) {
  if (!c) return -1;
  return paths_guarded(c, "gpg_paths_eval", [&] { return paths_eval_once(c, nx, xq, f, dfdx); });
}

int gpg_paths_coeff(gpg_ctx* c, double* coeff, double* ddiag) {
  if (!c) return -1;
  if (int rc = paths_check(c, "gpg_paths_coeff")) return rc;
  if (!coeff && !ddiag) { c->err = "gpg_paths_coeff: both outputs are NULL"; return -1; }
  GPG_HIP_OK(c, hipSetDevice(c->device));
  if (gpg_ws_activate(c, 1) != 0) return -2;
  const int N = c->N, S = c->paths_S;
  if (coeff) {
    const size_t total = (size_t)N * S;
    if (int rc = paths_scratch(c, round256(sizeof(double) * total), "gpg_paths_coeff")) return rc;
    hipLaunchKernelGGL(paths_coeff_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, N, S, c->paths_Sp, c->paths_sv,
                       (const double*)c->zvec, (const double*)c->invp, (const double*)c->paths_U, c->paths_scr);
    GPG_HIP_OK(c, hipMemcpyAsync(coeff, c->paths_scr, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream));
  }
  if (ddiag) GPG_HIP_OK(c, hipMemcpyAsync(ddiag, c->paths_dd, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
  GPG_HIP_OK(c, hipGetLastError());
  return 0;
}

}  // extern "C"
