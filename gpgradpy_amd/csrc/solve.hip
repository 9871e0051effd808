// Reductions and triangular sweeps around the factorisation (gfx950).
//   lkd_reduce      : ln det, GLS mean beta, r' K^-1 r from the diagonal of L and the two RHS rows
//                     (reference GpMeanFun.py:102-108, CalcLkd.py:153-168 / 220-226) -- wave-reduced
//   lkd_reduce_lin  : the same for the first-order mean: Gram matrix of the d + 2 RHS rows, (d+1) x (d+1) GLS solve
//   backward solve  : z = L^-T w for the single vector needed by alpha (GpEvalModel.py:57)
//   predict_reduce  : mu = beta + Kyx' alpha, sig2 = 1 - diag(Kxy K^-1 Kyx) (GpEvalModel.py:162-168)
//   extract         : dense N x N copies on request (tests / drop-in 7-tuple)
#include <algorithm>
#include "gpg_internal.h"
#include "device_util.h"
#include "kernel_fn.h"

namespace {

// orders the LDS accesses of ONE wave across a step of a wave-local algorithm (no workgroup barrier: the other waves are not involved)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// scal[0] = ln_det, [1] = beta, [2] = r'K^-1 r, [3] = V'K^-1 V, [4] = V'K^-1 y, [7] = the factorisation's info word (so that the
// host fetches ONE buffer per evaluation)
__global__ void __launch_bounds__(1024) lkd_reduce_kernel(const double* __restrict__ A, int ld, int N, int Npad,
                                                          const double* __restrict__ dvec, int precon,
                                                          double* __restrict__ scal, size_t v_stride, size_t a_stride,
                                                          const int* __restrict__ info) {
  A += blockIdx.x * a_stride; dvec += blockIdx.x * v_stride; scal += blockIdx.x * 8;   // batched: one workgroup per matrix
  __shared__ double sh[4 * 16];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = threadIdx.x; c < N; c += blockDim.x) {
    const size_t col = (size_t)c * ld;
    v[0] += log(A[col + c]);
    if (precon) v[1] += 0.5 * log(dvec[c]);
    const double w1 = A[col + Npad], w2 = A[col + Npad + 1];
    v[2] += w1 * w1;
    v[3] += w1 * w2;
  }
  block_sum<4>(v, sh);
  const double beta = v[3] / v[2];
  double rr[1] = {0.0};
  for (int c = threadIdx.x; c < N; c += blockDim.x) {
    const size_t col = (size_t)c * ld;
    const double t = A[col + Npad + 1] - beta * A[col + Npad];
    rr[0] += t * t;
  }
  block_sum<1>(rr, sh);
  if (threadIdx.x == 0) {
    scal[0] = 2.0 * (v[0] + v[1]);
    scal[1] = beta;
    scal[2] = rr[0];
    scal[3] = v[2];
    scal[4] = v[3];
    scal[7] = (double)info[blockIdx.x];
  }
}

// The same reduction for the first-order mean (V = calc_aug_vand, nb = d + 1 columns; GpMeanFun.py:69-122): the forward-solved
// right-hand-side rows w_0 .. w_(nb-1) (= L^-1 P^-1 V) and w_nb (= L^-1 P^-1 y) sit below the factor, nr = nb + 1 <= 18 contiguous
// doubles per matrix column.  One workgroup per matrix (batched launches as lkd_reduce_kernel):
//   pass 1  column chunks of kLinChunk columns x nr rows are staged in LDS (row stride kLinChunk + 1: the rows a wave reads at one
//           column sit in different banks, equal addresses are broadcast); thread (pair, slice) owns ONE entry (i, j), i <= j, of the
//           nr x nr Gram matrix of the rows over the columns = slice (mod kLinSlices) -- (d+2)(d+3)/2 <= 171 pairs x 4 slices, one
//           accumulator per thread; the slices are added in slice order.  G = W W' is its leading nb x nb block, b = W w_y its last
//           column.  The two log-det sums as in lkd_reduce_kernel.
//   solve   G = C C' by wave 0 alone (lane <-> row, wave-local ordering, no workgroup barrier), beta = C^-T C^-1 b by its lane 0.  A pivot that is not above kLinPivTol times the
//           diagonal entry it started from reports info = N + 1 + pivot: V has no full column rank in the K^-1 inner product.
//   pass 2  r'K^-1 r = sum_c (w_y - sum_i beta_i w_i)^2, the explicit residual (y'K^-1 y - b'G^-1 b cancels).
// Every sum has a fixed order: the result is reproducible and the same for a single and a batched launch.
// scal as lkd_reduce_kernel ([1] = beta_0, [3] = G_00, [4] = b_0); betav [nb] = the coefficients (NaN on a singular G).
constexpr int kLinChunk = 256, kLinSlices = 4, kLinRowsMax = GPG_MAX_NBETA + 1;
constexpr double kLinPivTol = 1e-12;
__global__ void __launch_bounds__(1024) lkd_reduce_lin_kernel(const double* __restrict__ A, int ld, int N, int Npad, int nb,
                                                              const double* __restrict__ dvec, int precon,
                                                              double* __restrict__ scal, double* __restrict__ betav,
                                                              size_t v_stride, size_t a_stride, const int* __restrict__ info) {
  A += blockIdx.x * a_stride; dvec += blockIdx.x * v_stride; scal += blockIdx.x * 8; betav += (size_t)blockIdx.x * GPG_BETA_STRIDE;
  __shared__ double sh[4 * 16];
  __shared__ double rows[kLinRowsMax][kLinChunk + 1];
  __shared__ double part[kLinSlices][256];
  __shared__ double G[GPG_MAX_NBETA][GPG_MAX_NBETA + 1];
  __shared__ double bsh[GPG_MAX_NBETA], beta_sh[GPG_MAX_NBETA], diag0[GPG_MAX_NBETA];
  __shared__ int sing;
  const int nr = nb + 1, npair = nr * (nr + 1) / 2;
  const int tid = threadIdx.x, pr = tid & 255, sl = tid >> 8;
  // pair index -> (pi, pj), pi <= pj, column by column of the upper triangle
  int pi = 0, pj = 0;
  if (pr < npair) {
    int q = pr;
    while (q > pj) { q -= pj + 1; ++pj; }
    pi = q;
  }
  if (tid == 0) sing = 0;
  double v[2] = {0.0, 0.0};
  for (int c = tid; c < N; c += blockDim.x) {
    v[0] += log(A[(size_t)c * ld + c]);
    if (precon) v[1] += 0.5 * log(dvec[c]);
  }
  double acc = 0.0;
  for (int c0 = 0; c0 < N; c0 += kLinChunk) {
    const int cn = min(kLinChunk, N - c0);
    __syncthreads();
    for (int t = tid; t < cn * nr; t += blockDim.x) {
      const int cc = t / nr, r = t - cc * nr;
      rows[r][cc] = A[(size_t)(c0 + cc) * ld + Npad + r];
    }
    __syncthreads();
    if (pr < npair)
      for (int cc = sl; cc < cn; cc += kLinSlices) acc += rows[pi][cc] * rows[pj][cc];
  }
  part[sl][pr] = acc;
  block_sum<2>(v, sh);                                   // (its barriers also order part[][])
  if (sl == 0 && pr < npair) {
    double s = part[0][pr];
    for (int q = 1; q < kLinSlices; ++q) s += part[q][pr];
    if (pj < nb) { G[pj][pi] = s; G[pi][pj] = s; }
    else if (pi < nb) bsh[pi] = s;
  }
  __syncthreads();
  const double g00 = G[0][0], b0 = bsh[0];
  // G = C C', lower triangle in place, and the two substitutions: wave 0 alone (lane <-> row, nb <= 17 < 64), the other fifteen
  // waves go straight to the barrier below.  Inside one wave the LDS operations complete in program order; wave_lds_sync keeps
  // the compiler from moving them across the steps.  `s` is uniform over the wave: every lane reads the same pivot.
  if (tid < 64) {
    if (tid < nb) diag0[tid] = G[tid][tid];
    int s = 0;
    for (int k = 0; k < nb; ++k) {
      wave_lds_sync();
      const double piv = G[k][k];
      if (!(piv > kLinPivTol * diag0[k])) { s = k + 1; break; }
      const double ckk = sqrt(piv);
      wave_lds_sync();                                    // every lane has read the pivot before lane k overwrites it
      if (tid > k && tid < nb) G[tid][k] = G[tid][k] / ckk;
      if (tid == k) G[k][k] = ckk;
      wave_lds_sync();
      if (tid > k && tid < nb)
        for (int j = k + 1; j <= tid; ++j) G[tid][j] -= G[tid][k] * G[j][k];
    }
    wave_lds_sync();
    if (tid == 0) {
      sing = s;
      if (s != 0) {
        for (int i = 0; i < nb; ++i) beta_sh[i] = __longlong_as_double(0x7ff8000000000000LL);
      } else {
        for (int i = 0; i < nb; ++i) {                    // C z = b
          double t = bsh[i];
          for (int j = 0; j < i; ++j) t -= G[i][j] * beta_sh[j];
          beta_sh[i] = t / G[i][i];
        }
        for (int i = nb - 1; i >= 0; --i) {               // C' beta = z
          double t = beta_sh[i];
          for (int j = i + 1; j < nb; ++j) t -= G[j][i] * beta_sh[j];
          beta_sh[i] = t / G[i][i];
        }
      }
    }
  }
  __syncthreads();
  double rr[1] = {0.0};
  for (int c = tid; c < N; c += blockDim.x) {
    const double* w = A + (size_t)c * ld + Npad;
    double t = w[nb];
    for (int i = 0; i < nb; ++i) t -= beta_sh[i] * w[i];
    rr[0] += t * t;
  }
  block_sum<1>(rr, sh);
  if (tid < nb) betav[tid] = beta_sh[tid];
  if (tid == 0) {
    const int finfo = info[blockIdx.x];
    scal[0] = 2.0 * (v[0] + v[1]);
    scal[1] = beta_sh[0];
    scal[2] = rr[0];
    scal[3] = g00;
    scal[4] = b0;
    scal[7] = (double)(finfo != 0 ? finfo : (sing != 0 ? N + sing : 0));
  }
}

// rows[64 c + r] = (r == 0) ? src[c ld] : 0 -- a vector as row 0 of a zeroed 64-row tile row (one launch instead of a fill and a
// strided copy)
__global__ void __launch_bounds__(256) vec_rows_load_kernel(double* __restrict__ rows, const double* __restrict__ src, int ld, int Npad) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 64 * (size_t)Npad) return;
  rows[i] = (i & 63) == 0 ? src[(i >> 6) * (size_t)ld] : 0.0;
}

// t[j] = sum_{i >= k0+64} L[i, k0+j] z[i]   (one workgroup per column j)
__global__ void __launch_bounds__(256) bs_dot_kernel(const double* __restrict__ A, int ld, int Npad, int k0,
                                                     const double* __restrict__ z, double* __restrict__ t) {
  __shared__ double sh[16];
  const int j = blockIdx.x;
  const double* colp = A + (size_t)(k0 + j) * ld;
  double v[1] = {0.0};
  for (int i = k0 + 64 + threadIdx.x; i < Npad; i += 256) v[0] += colp[i] * z[i];
  block_sum<1>(v, sh);
  if (threadIdx.x == 0) t[j] = v[0];
}

// solve L_kk^T z_k = w_k - t (one wave, lane j <-> unknown j)
__global__ void __launch_bounds__(64) bs_tri_kernel(const double* __restrict__ A, int ld, int Npad, int k0,
                                                    const double* __restrict__ t, int has_t, double* __restrict__ z) {
  __shared__ double Ls[64][65];
  const int j = threadIdx.x;
  for (int q = 0; q < 64; ++q) Ls[j][q] = A[(size_t)(k0 + j) + (size_t)(k0 + q) * ld];  // Ls[i][q] = L[i][q]
  __syncthreads();
  // right-hand side: forward-solved RHS row 0
  double rhs = A[(size_t)(k0 + j) * ld + Npad] - (has_t ? t[j] : 0.0);
  double zj = 0.0;
  for (int i = 63; i >= 0; --i) {
    double zi = __shfl(rhs, i, 64) / Ls[i][i];
    if (j == i) zj = zi;
    if (j < i) rhs -= Ls[i][j] * zi;
  }
  z[k0 + j] = zj;
}

__global__ void alpha_kernel(const double* __restrict__ z, const double* __restrict__ invp, int N,
                             double* __restrict__ alpha) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < N) alpha[r] = z[r] * invp[r];
}

// prior mean at query j: the constant beta, or with a first-order mean (betav != nullptr, device [d + 1]; Xq [d x nxp])
// beta_0 + xq_j . beta_1..d (GpMeanFun.py:14-67)
__device__ __forceinline__ double prior_mean(double beta, const double* __restrict__ betav, const double* __restrict__ Xq, int d, int nxp,
                                             int j) {
  if (betav == nullptr) return beta;
  double m = betav[0];
  for (int k = 0; k < d; ++k) m += betav[k + 1] * Xq[(size_t)k * nxp + j];
  return m;
}

// phase 0: out[j] = mean_j + sum_c Wt[j, c] z[c] ; phase 1: out[j] = 1 - sum_c Wt[j, c]^2
__global__ void __launch_bounds__(1024) predict_reduce_kernel(const double* __restrict__ Wt, int nxp, int N,
                                                              const double* __restrict__ z, double beta, int phase,
                                                              double* __restrict__ out, const double* __restrict__ betav,
                                                              const double* __restrict__ Xq, int d) {
  __shared__ double sh[16][64];
  const int jl = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jl;
  double acc = 0.0, comp = 0.0;
  if (phase == 0) {
    for (int c = cg; c < N; c += 16) kb_add(acc, comp, Wt[(size_t)c * nxp + j] * z[c]);
  } else {
    for (int c = cg; c < N; c += 16) { double w = Wt[(size_t)c * nxp + j]; acc += w * w; }
  }
  sh[cg][jl] = acc + comp;
  __syncthreads();
  if (cg == 0) {
    double s = 0.0, cs = 0.0;
    for (int q = 0; q < 16; ++q) kb_add(s, cs, sh[q][jl]);
    s += cs;
    out[j] = phase == 0 ? prior_mean(beta, betav, Xq, d, nxp, j) + s : 1.0 - s;
  }
}

// The same reductions for a few query rows, spread over S slices of the columns (grid = (nxp / 64, S)) so that a
// single-point evaluation is not one workgroup streaming the whole row set; the partial sums are added in slice order
// by predict_final_kernel (deterministic).
__global__ void __launch_bounds__(1024) predict_partial_kernel(const double* __restrict__ Wt, int nxp, int N, int chunk,
                                                               const double* __restrict__ z, int phase,
                                                               double* __restrict__ partial) {
  __shared__ double sh[16][64];
  const int jl = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jl;
  const int c0 = blockIdx.y * chunk, c1 = min(N, c0 + chunk);
  double acc = 0.0, comp = 0.0;
  if (phase == 0) {
    for (int c = c0 + cg; c < c1; c += 16) kb_add(acc, comp, Wt[(size_t)c * nxp + j] * z[c]);
  } else {
    for (int c = c0 + cg; c < c1; c += 16) { double w = Wt[(size_t)c * nxp + j]; acc += w * w; }
  }
  sh[cg][jl] = acc + comp;
  __syncthreads();
  if (cg == 0) {
    double s = 0.0, cs = 0.0;
    for (int q = 0; q < 16; ++q) kb_add(s, cs, sh[q][jl]);
    partial[(size_t)blockIdx.y * nxp + j] = s + cs;
  }
}

__global__ void __launch_bounds__(1024) predict_final_kernel(const double* __restrict__ partial, int nxp, int S, double beta,
                                                             int phase, double* __restrict__ out, const double* __restrict__ betav,
                                                             const double* __restrict__ Xq, int d) {
  __shared__ double sh[16][64];
  const int jl = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jl;
  double acc = 0.0, comp = 0.0;
  for (int q = cg; q < S; q += 16) kb_add(acc, comp, partial[(size_t)q * nxp + j]);
  sh[cg][jl] = acc + comp;
  __syncthreads();
  if (cg == 0) {
    double s = 0.0, cs = 0.0;
    for (int q = 0; q < 16; ++q) kb_add(s, cs, sh[q][jl]);
    s += cs;
    out[j] = phase == 0 ? prior_mean(beta, betav, Xq, d, nxp, j) + s : 1.0 - s;
  }
}

// ---- multi right-hand-side backward solve on the "RHS rows" layout Z[r + i * ldz] (in place) ----------
// t[r * 64 + j] = sum_{i >= k0+64} L[i, k0+j] Z[r, i]   (workgroup = column j x a group of 16 right-hand sides)
__global__ void __launch_bounds__(256) bs_dot_multi_kernel(const double* __restrict__ A, int ld, int Npad, int k0,
                                                           const double* __restrict__ Z, int ldz, int nrhs,
                                                           double* __restrict__ t) {
  __shared__ double sh[16 * 16];
  const int j = blockIdx.x, r0 = blockIdx.y * 16;
  const double* colp = A + (size_t)(k0 + j) * ld;
  double v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = 0.0;
  for (int i = k0 + 64 + threadIdx.x; i < Npad; i += 256) {
    const double l = colp[i];
    const double* zp = Z + (size_t)i * ldz + r0;
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] += l * zp[q];
  }
  block_sum<16>(v, sh);
  if (threadIdx.x < 16 && r0 + threadIdx.x < nrhs) t[(size_t)(r0 + threadIdx.x) * 64 + j] = v[threadIdx.x];
}

// solve L_kk^T z_k = w_k - t for right-hand side r = blockIdx.x (one wave, lane j <-> unknown j)
__global__ void __launch_bounds__(64) bs_tri_multi_kernel(const double* __restrict__ A, int ld, int k0,
                                                          const double* __restrict__ t, int has_t,
                                                          double* __restrict__ Z, int ldz) {
  __shared__ double Ls[64][65];
  const int j = threadIdx.x, r = blockIdx.x;
  for (int q = 0; q < 64; ++q) Ls[j][q] = A[(size_t)(k0 + j) + (size_t)(k0 + q) * ld];
  __syncthreads();
  double rhs = Z[(size_t)(k0 + j) * ldz + r] - (has_t ? t[(size_t)r * 64 + j] : 0.0);
  double zj = 0.0;
  for (int i = 63; i >= 0; --i) {
    double zi = __shfl(rhs, i, 64) / Ls[i][i];
    if (j == i) zj = zi;
    if (j < i) rhs -= Ls[i][j] * zi;
  }
  Z[(size_t)(k0 + j) * ldz + r] = zj;
}

// Posterior gradient reductions (reference GpEvalModel.py:135-140, 319-354): for query q and direction j'
//   g1[q, j'] = sum_c dKxy_dx[(j', q), c] alpha_c              -> dmu/dx
//   g2[q, j'] = sum_c dKxy_dx[(j', q), c] (K^-1 Kyx)[c, q]     -> d sig/dx = -varK g2 / sig
// dKxy_dx[(j', q), c] = block (I, j'+1) of the gradient-enhanced kernel at (x_a, xq_q), c = (I, a); it is
// recomputed on the fly (never stored).  zvec = p * alpha, Z = L^-T L^-1 P^-1 Kyx (RHS-rows layout).
template <int KERN, int D>
__global__ void __launch_bounds__(256) cross_grad_kernel(AsmParams P, const double* __restrict__ Xt,
                                                         const double* __restrict__ Xq, int nxp,
                                                         const double* __restrict__ invp, const double* __restrict__ zvec,
                                                         const double* __restrict__ Z, double* __restrict__ g1o,
                                                         double* __restrict__ g2o, const double* __restrict__ betav) {
  __shared__ double sh[2 * D * 16];
  const int q = blockIdx.x, n = P.n, ng = P.ng;
  const int nblk = P.use_grad ? D + 1 : 1;
  double g[2 * D];
#pragma unroll
  for (int k = 0; k < 2 * D; ++k) g[k] = 0.0;
  double xq[D], th[D];
#pragma unroll
  for (int k = 0; k < D; ++k) { xq[k] = Xq[(size_t)k * nxp + q]; th[k] = P.theta[k]; }
  const double rq_c = kern_rq_c(P.hp_kernel);
  for (int a = threadIdx.x; a < n; a += 256) {
    double R[D], s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) { R[k] = Xt[(size_t)k * n + a] - xq[k]; kern_s_add<KERN, true>(s, th[k], R[k]); }
    const KernRadial rad = kern_radial<KERN, true>(s, P.hp_kernel);
    const double E = rad.E, M1 = rad.M1;
    const int gpa = P.gpos[a];
    // I = 0 : block (0, j'+1)
    {
      const double wa = zvec[a] * invp[a], ws = Z[(size_t)a * nxp + q] * invp[a];
#pragma unroll
      for (int jp = 0; jp < D; ++jp) {
        const double v = kern_d01<KERN>(th[jp], R[jp], E, M1);
        g[jp] += v * wa;
        g[D + jp] += v * ws;
      }
    }
    if (nblk > 1 && gpa >= 0) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const size_t c = (size_t)n + (size_t)i * ng + gpa;
        const double ip = invp[c];
        const double wa = zvec[c] * ip, ws = Z[c * nxp + q] * ip;
#pragma unroll
        for (int jp = 0; jp < D; ++jp) {
          const double v = kern_d11<KERN>(i == jp, th[i], th[jp], R[i], R[jp], E, M1, rq_c);
          g[jp] += v * wa;
          g[D + jp] += v * ws;
        }
      }
    }
  }
  block_sum<2 * D>(g, sh);
  if (threadIdx.x < D) {
    // first-order mean: its gradient beta_1..d is the same at every query (GpMeanFun.py:14-67)
    g1o[(size_t)q * D + threadIdx.x] = betav ? g[threadIdx.x] + betav[threadIdx.x + 1] : g[threadIdx.x];
    g2o[(size_t)q * D + threadIdx.x] = g[D + threadIdx.x];
  }
}

// ------------------------------------------------------------------------------------------------
// Posterior Hessians (reference GpEvalModel.py:355-382; the kernel second / third derivatives d2K are kern_d2k_base and
// kern_d2k_grad of kernel_fn.h, with R = x_a - xq, this file's sign).
// hess_contract_kernel: workgroup (k, j) -> row k of  H1_j = sum_c d2K_j[k,:,c] alpha_c  and  H2_j = sum_c d2K_j[k,:,c] v_j,c  for
// query point j of the grid (gpg_predict_hess: one; gpg_predict_second: the points of a chunk), v_j = K^-1 Kyx of point j = row j
// of the backward-swept Z (with the mean uncertainty K^-1 k + K^-1 V H^-1 u).  h1o, h2o [points, D, D].  Xq is [D x ldz].
// Nothing of the [d, d, N] tensor is stored.
// ------------------------------------------------------------------------------------------------
template <int KERN, int D>
__global__ void __launch_bounds__(256) hess_contract_kernel(AsmParams P, const double* __restrict__ Xt, const double* __restrict__ Xq,
                                                              int ldz, const double* __restrict__ invp, const double* __restrict__ zvec,
                                                              const double* __restrict__ Z, double* __restrict__ h1o,
                                                              double* __restrict__ h2o) {
  __shared__ double sh[2 * D * 16];
  const int k = blockIdx.x, jq = blockIdx.y, n = P.n, ng = P.ng;
  const int nblk = P.use_grad ? D + 1 : 1;
  double g[2 * D];
#pragma unroll
  for (int i = 0; i < 2 * D; ++i) g[i] = 0.0;
  double xq[D], th[D];
#pragma unroll
  for (int i = 0; i < D; ++i) { xq[i] = Xq[(size_t)i * ldz + jq]; th[i] = P.theta[i]; }
  // row k's own coordinate and theta through memory (k is uniform): indexing xq / th / tR with it would put the arrays in scratch
  const double xqk = Xq[(size_t)k * ldz + jq], thk = P.theta[k];
  const double rq_s1 = 1.0 + 1.0 / P.hp_kernel, rq_s2 = rq_s1 * (1.0 + 2.0 / P.hp_kernel);   // RatQu only
  for (int a = threadIdx.x; a < n; a += 256) {
    double R[D], tR[D];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) { R[i] = Xt[(size_t)i * n + a] - xq[i]; tR[i] = th[i] * R[i]; s += tR[i] * R[i]; }
    const KernRadial rad = kern_radial<KERN>(s, P.hp_kernel);
    const double tRk = thk * (Xt[(size_t)k * n + a] - xqk);   // = tR[k], the same two operations
    {
      const double wa = zvec[a] * invp[a], ws = Z[(size_t)a * ldz + jq] * invp[a];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double v = kern_d2k_base<KERN>(i, k, th[i], thk, tR[i], tRk, rad.E, rad.M1, rq_s1);
        g[i] += v * wa;
        g[D + i] += v * ws;
      }
    }
    const int gpa = P.gpos[a];
    if (nblk > 1 && gpa >= 0) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const size_t c = (size_t)n + (size_t)j * ng + gpa;
        const double ip = invp[c];
        const double wa = zvec[c] * ip, ws = Z[c * ldz + jq] * ip;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const double v = kern_d2k_grad<KERN>(i, j, k, th[i], th[j], tR[i], tR[j], tRk, rad.E, rad.F3, rad.c3, rq_s1, rq_s2);
          g[i] += v * wa;
          g[D + i] += v * ws;
        }
      }
    }
  }
  block_sum<2 * D>(g, sh);
  if (threadIdx.x == 0) {   // (an index that differs by lane would put g in scratch for the whole loop)
#pragma unroll
    for (int i = 0; i < D; ++i) {
      h1o[((size_t)jq * D + k) * D + i] = g[i];
      h2o[((size_t)jq * D + k) * D + i] = g[D + i];
    }
  }
}

// Rows 1 .. d of Wt (RHS-rows layout, leading dimension nxp) <- P^-1 dKxy_dx[(j', q=0), :]: the d derivative rows
// of the cross-covariance at the query point (same entries as cross_grad_kernel), for the forward sweep that gives
// dKxy_dx K^-1 dKxy_dx^T (GpEvalModel.py:367).  Row 0 is cleared.
template <int KERN, int D>
__global__ void __launch_bounds__(256) cross_dx_rows_kernel(AsmParams P, const double* __restrict__ Xt,
                                                            const double* __restrict__ Xq, int nxp,
                                                            const double* __restrict__ invp, double* __restrict__ Wt) {
  const int a = blockIdx.x * 256 + threadIdx.x, n = P.n, ng = P.ng;
  if (a >= n) return;
  const int nblk = P.use_grad ? D + 1 : 1;
  double R[D], th[D], s = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) { th[i] = P.theta[i]; R[i] = Xt[(size_t)i * n + a] - Xq[(size_t)i * nxp]; kern_s_add<KERN, false>(s, th[i], R[i]); }
  const KernRadial rad = kern_radial<KERN>(s, P.hp_kernel);
  const double E = rad.E, M1 = rad.M1;
  {
    const double ip = invp[a];
    Wt[(size_t)a * nxp] = 0.0;
#pragma unroll
    for (int jp = 0; jp < D; ++jp)
      Wt[(size_t)a * nxp + 1 + jp] = ip * kern_d01<KERN>(th[jp], R[jp], E, M1);
  }
  const int gpa = P.gpos[a];
  if (nblk > 1 && gpa >= 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const size_t c = (size_t)n + (size_t)i * ng + gpa;
      const double ip = invp[c];
      Wt[c * nxp] = 0.0;
#pragma unroll
      for (int jp = 0; jp < D; ++jp)
        Wt[c * nxp + 1 + jp] = ip * kern_d11<KERN>(i == jp, th[i], th[jp], R[i], R[jp], E, M1, kern_rq_c(P.hp_kernel));
    }
  }
}

// T[i, i'] = sum_c W[1 + i, c] W[1 + i', c]  (workgroup i; rows of the RHS-rows layout after the forward sweep)
template <int D>
__global__ void __launch_bounds__(256) rows_gram_kernel(const double* __restrict__ Wt, int nxp, int Npad,
                                                        double* __restrict__ T) {
  __shared__ double sh[D * 16];
  const int i = blockIdx.x;
  double g[D];
#pragma unroll
  for (int q = 0; q < D; ++q) g[q] = 0.0;
  for (int c = threadIdx.x; c < Npad; c += 256) {
    const double* w = Wt + (size_t)c * nxp + 1;
    const double wi = w[i];
#pragma unroll
    for (int q = 0; q < D; ++q) g[q] += wi * w[q];
  }
  block_sum<D>(g, sh);
  if (threadIdx.x < D) T[(size_t)i * D + threadIdx.x] = g[threadIdx.x];
}

// which 0..2: symmetric copy of the lower triangle; which 3: P L (lower), zeros above
__global__ void extract_kernel(const double* __restrict__ A, int ld, int N, const double* __restrict__ dvec,
                               int precon, int which, double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (c >= N) return;
  double v;
  if (which == 3) {
    v = r >= c ? A[(size_t)r + (size_t)c * ld] * (precon ? sqrt(dvec[r]) : 1.0) : 0.0;
  } else {
    v = r >= c ? A[(size_t)r + (size_t)c * ld] : A[(size_t)c + (size_t)r * ld];
  }
  out[(size_t)r * N + c] = v;
}

}  // namespace

void gpg_launch_lkd_reduce(gpg_ctx* c, int slot) {
  gpg_prof_begin(c, GPG_PROF_REDUCE, 0.0);
  if (c->n_beta > 1)
    hipLaunchKernelGGL(lkd_reduce_lin_kernel, dim3(1), dim3(1024), 0, c->stream, c->A, c->ld, c->N, c->Npad, c->n_beta, c->dvec,
                       c->last_precon, c->scal + (size_t)slot * 8, c->betav + (size_t)slot * GPG_BETA_STRIDE, (size_t)0, (size_t)0, c->info);
  else
    hipLaunchKernelGGL(lkd_reduce_kernel, dim3(1), dim3(1024), 0, c->stream, c->A, c->ld, c->N, c->Npad, c->dvec,
                       c->last_precon, c->scal + (size_t)slot * 8, (size_t)0, (size_t)0, c->info);   // c->info: this evaluation's word
  gpg_prof_end(c);
}

void gpg_launch_lkd_reduce_batch(gpg_ctx* c, int slot0, int B, size_t v_stride, size_t a_stride, const int* info0) {
  gpg_prof_begin(c, GPG_PROF_REDUCE, 0.0);
  if (c->n_beta > 1)
    hipLaunchKernelGGL(lkd_reduce_lin_kernel, dim3(B), dim3(1024), 0, c->stream, c->A, c->ld, c->N, c->Npad, c->n_beta, c->dvec,
                       c->last_precon, c->scal + (size_t)slot0 * 8, c->betav + (size_t)slot0 * GPG_BETA_STRIDE, v_stride, a_stride, info0);
  else
    hipLaunchKernelGGL(lkd_reduce_kernel, dim3(B), dim3(1024), 0, c->stream, c->A, c->ld, c->N, c->Npad, c->dvec,
                       c->last_precon, c->scal + (size_t)slot0 * 8, v_stride, a_stride, info0);
  gpg_prof_end(c);
}

void gpg_backward_solve(gpg_ctx* c) {
  const int Npad = c->Npad;
  if (gpg_dataflow_solves(c)) {
    // the vector rides as row 0 of a zeroed 64-row tile through the dataflow backward solve (one launch instead of
    // 2 Npad / 64 dependent ones)
    if (!c->vec_rows) (void)gpg_dev_alloc(c, &c->vec_rows, sizeof(double) * 64 * (size_t)c->vec_rows_cols);
    if (c->vec_rows) {
      // right-hand side: the forward-solved RHS row 0 of the factorisation workspace (row Npad of A); rows 1..63 of the tile zero
      hipLaunchKernelGGL(vec_rows_load_kernel, dim3((unsigned)((64 * (size_t)Npad + 255) / 256)), dim3(256), 0, c->stream, c->vec_rows,
                         c->A + Npad, c->ld, Npad);
      if (gpg_launch_rows_bwd(c, c->vec_rows, 64, 64, 1)) {
        (void)hipMemcpy2DAsync(c->zvec, sizeof(double), c->vec_rows, 64 * sizeof(double), sizeof(double), Npad,
                               hipMemcpyDeviceToDevice, c->stream);
        return;
      }
    }
  }
  for (int k0 = Npad - 64; k0 >= 0; k0 -= 64) {
    const int has_t = (k0 + 64 < Npad);
    if (has_t)
      hipLaunchKernelGGL(bs_dot_kernel, dim3(64), dim3(256), 0, c->stream, c->A, c->ld, Npad, k0, c->zvec, c->tmpv);
    hipLaunchKernelGGL(bs_tri_kernel, dim3(1), dim3(64), 0, c->stream, c->A, c->ld, Npad, k0, c->tmpv, has_t, c->zvec);
  }
}

// Z (nrhs x Npad, RHS-rows layout, leading dimension ldz) <- Z L^-1, i.e. every row solved against L^T
void gpg_backward_rows(gpg_ctx* c, double* Z, int ldz, int nrhs, double* tbuf) {
  // one dataflow launch over the 64-row tiles that hold the nrhs rows (the other rows of a tile ride along)
  const int rows = ((nrhs + 63) / 64) * 64;
  if (gpg_dataflow_solves(c)) {
    if (gpg_launch_rows_bwd(c, Z, ldz, rows, nrhs)) return;
    // more row tiles than one dataflow launch takes: one launch per group of row tiles (rows are the fast index of Z)
    const int chunk = (c->rows_max_tasks / (c->Npad / 64)) * 64;
    if (chunk >= 64) {
      bool ok = true;
      for (int r0 = 0; r0 < rows && ok; r0 += chunk) {
        const int nr = std::min(chunk, rows - r0);
        ok = gpg_launch_rows_bwd(c, Z + r0, ldz, nr, std::min(nr, nrhs - r0));
      }
      if (ok) return;      // (a refusal can only come before the first launch: same shape every time)
    }
  }
  const int Npad = c->Npad;
  for (int k0 = Npad - 64; k0 >= 0; k0 -= 64) {
    const int has_t = (k0 + 64 < Npad);
    if (has_t)
      hipLaunchKernelGGL(bs_dot_multi_kernel, dim3(64, (nrhs + 15) / 16), dim3(256), 0, c->stream, c->A, c->ld, Npad, k0, Z,
                         ldz, nrhs, tbuf);
    hipLaunchKernelGGL(bs_tri_multi_kernel, dim3(nrhs), dim3(64), 0, c->stream, c->A, c->ld, k0, tbuf, has_t, Z, ldz);
  }
}

void gpg_launch_cross_grad(gpg_ctx* c, const AsmParams& p, int nx, int nxp, double* g1, double* g2) {
  gpg_for_kern_d(p.kernel, p.d, [&](auto K, auto D) {
    hipLaunchKernelGGL((cross_grad_kernel<decltype(K)::value, decltype(D)::value>), dim3(nx), dim3(256), 0, c->stream, p, c->Xt, c->xq_dev,
                       nxp, c->invp, c->zvec, c->Wt, g1, g2, c->eval_linear ? c->eval_beta_dev : (const double*)nullptr);
  });
}

// H1 / H2 of the pc query points in xq_dev [d x ldz], their K^-1 Kyx in rows 0 .. pc - 1 of Wt (leading dimension ldz): h1, h2 [pc, d, d]
void gpg_launch_hess_contract(gpg_ctx* c, const AsmParams& p, int pc, int ldz, double* h1, double* h2) {
  gpg_for_kern_d(p.kernel, p.d, [&](auto K, auto D) {
    constexpr int KERN = decltype(K)::value, DD = decltype(D)::value;
    hipLaunchKernelGGL((hess_contract_kernel<KERN, DD>), dim3(DD, pc), dim3(256), 0, c->stream, p, c->Xt, c->xq_dev, ldz, c->invp,
                       c->zvec, c->Wt, h1, h2);
  });
}

// stage 1: derivative rows into Wt rows 1..d, 2: Gram of those rows after the forward sweep
void gpg_launch_hess_stage(gpg_ctx* c, const AsmParams& p, int nxp, double* T, int stage) {
  gpg_for_kern_d(p.kernel, p.d, [&](auto K, auto D) {
    constexpr int KERN = decltype(K)::value, DD = decltype(D)::value;
    if (stage == 1)
      hipLaunchKernelGGL((cross_dx_rows_kernel<KERN, DD>), dim3((p.n + 255) / 256), dim3(256), 0, c->stream, p, c->Xt,
                         c->xq_dev, nxp, c->invp, c->Wt);
    else
      hipLaunchKernelGGL((rows_gram_kernel<DD>), dim3(DD), dim3(256), 0, c->stream, c->Wt, nxp, c->Npad, T);
  });
}

// ---- products with the factor in place (condition number) ------------------------------------
// w = L^T v: one wave per column j (column-major storage: the column is contiguous), w[j] = sum_{i >= j} L[i][j] v[i]
__global__ void __launch_bounds__(256) trmv_t_kernel(const double* __restrict__ A, int ld, int n, const double* __restrict__ v,
                                                     double* __restrict__ w) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= n) return;
  const double* col = A + (size_t)j * ld;
  double s = 0.0;
  for (int i = j + lane; i < n; i += 64) s += col[i] * v[i];
  s = wave_sum(s);
  if (lane == 0) w[j] = s;
}

// u = L w: thread <-> row i of a block of 256 rows, columns streamed in chunks of 256 (w chunk in LDS; every load of
// L is coalesced over the rows), u[i] = sum_{j <= i} L[i][j] w[j]
__global__ void __launch_bounds__(256) trmv_n_kernel(const double* __restrict__ A, int ld, int n, const double* __restrict__ w,
                                                     double* __restrict__ u) {
  __shared__ double ws[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int jend = min(n, (int)(blockIdx.x + 1) * 256);
  double s = 0.0;
  for (int j0 = 0; j0 < jend; j0 += 256) {
    __syncthreads();
    ws[threadIdx.x] = (j0 + (int)threadIdx.x < n) ? w[j0 + threadIdx.x] : 0.0;
    __syncthreads();
    if (i < n) {
      const int jm = min(256, i - j0 + 1);               // columns j0 .. j0 + jm - 1 are <= i
      const double* p = A + (size_t)i + (size_t)j0 * ld;
#pragma unroll 8
      for (int jj = 0; jj < jm; ++jj) s += p[(size_t)jj * ld] * ws[jj];
    }
  }
  if (i < n) u[i] = s;
}

// out (device, Npad) <- (L L^T) v (op 0) or (L L^T)^-1 v (op 1) with the factor in A; v (device, Npad, zero tail) is
// overwritten.  The solves run through the single-row dataflow kernels on a carrier tile.
int gpg_factor_apply_dev(gpg_ctx* c, int op, double* v, double* out) {
  const int Npad = c->Npad;
  if (op == 0) {
    hipLaunchKernelGGL(trmv_t_kernel, dim3((Npad + 3) / 4), dim3(256), 0, c->stream, c->A, c->ld, Npad, v, out);   // out = L^T v
    hipLaunchKernelGGL(trmv_n_kernel, dim3((Npad + 255) / 256), dim3(256), 0, c->stream, c->A, c->ld, Npad, out, v);  // v = L out
    return hipMemcpyAsync(out, v, sizeof(double) * Npad, hipMemcpyDeviceToDevice, c->stream) == hipSuccess ? 0 : -2;
  }
  if (!c->vec_rows && !gpg_dev_alloc(c, &c->vec_rows, sizeof(double) * 64 * (size_t)c->vec_rows_cols)) return -2;
  hipLaunchKernelGGL(vec_rows_load_kernel, dim3((unsigned)((64 * (size_t)Npad + 255) / 256)), dim3(256), 0, c->stream, c->vec_rows, v, 1,
                     Npad);                                                       // row 0 of the carrier <- v
  if (gpg_dataflow_solves(c)) {
    if (!gpg_launch_rows_fwd(c, c->vec_rows, 64, 64, 1) || !gpg_launch_rows_bwd(c, c->vec_rows, 64, 64, 1)) return -2;
  } else {
    gpg_forward_rows(c, c->vec_rows, 64, 64, 1);
    gpg_backward_rows(c, c->vec_rows, 64, 1, c->gradbuf ? c->gradbuf : v);
  }
  return hipMemcpy2DAsync(out, sizeof(double), c->vec_rows, 64 * sizeof(double), sizeof(double), Npad, hipMemcpyDeviceToDevice,
                          c->stream) == hipSuccess ? 0 : -2;
}

void gpg_launch_alpha(gpg_ctx* c, double* alpha_dev) {
  hipLaunchKernelGGL(alpha_kernel, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->zvec, c->invp, c->N,
                     alpha_dev);
}

void gpg_launch_predict_reduce(gpg_ctx* c, int nx, int nxp, double beta, double varK, int phase) {
  (void)nx; (void)varK;
  const double* bv = c->eval_linear ? c->eval_beta_dev : nullptr;
  const int S = std::min(128, c->Npad / nxp);      // slices; the partial sums live in tmpv [Npad]
  if (S >= 2) {
    const int chunk = (c->N + S - 1) / S;
    hipLaunchKernelGGL(predict_partial_kernel, dim3(nxp / 64, S), dim3(1024), 0, c->stream, c->Wt, nxp, c->N, chunk, c->zvec,
                       phase, c->tmpv);
    hipLaunchKernelGGL(predict_final_kernel, dim3(nxp / 64), dim3(1024), 0, c->stream, c->tmpv, nxp, S, beta, phase,
                       c->musig + (size_t)phase * nxp, bv, c->xq_dev, c->d);
    return;
  }
  hipLaunchKernelGGL(predict_reduce_kernel, dim3(nxp / 64), dim3(1024), 0, c->stream, c->Wt, nxp, c->N, c->zvec, beta,
                     phase, c->musig + (size_t)phase * nxp, bv, c->xq_dev, c->d);
}

void gpg_launch_extract(gpg_ctx* c, int which) {
  dim3 grid((c->N + 255) / 256, c->N);
  hipLaunchKernelGGL(extract_kernel, grid, dim3(256), 0, c->stream, c->A, c->ld, c->N, c->dvec, c->last_precon, which,
                     c->dense_tmp);
}
