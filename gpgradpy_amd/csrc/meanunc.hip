// Uncertainty of the GLS mean coefficients in the posterior (gpg_set_mean_uncertainty, include/gpgrad.h): the universal-kriging
// term  varK U H^-1 U^T  of the joint covariance, with
//     H = V^T K^-1 V  (n_beta x n_beta),      u_r = v_r - V^T K^-1 k_r  (row r of U),
// K = (P L)(P L)^T the matrix gpg_setup_eval factorised, V the augmented Vandermonde matrix of the model (gpg_set_mean_order), k_r
// the cross-covariance column of query row r and v_r its mean basis.  Only forward sweeps are needed per query:
//     Z = Kqy P^-1 L^-T  (what gpg_predict* / gpg_predict_joint already form),   W_V = L^-1 P^-1 V,
//     H = W_V^T W_V,   U = V_q - Z W_V.
// Per-model state, built by the first call that needs it after a gpg_setup_eval (gpg_meanunc_ensure): W_V and its backward-swept
// copy L^-T W_V (= K^-1 V in the scaling cross_grad_kernel expects of its row), both [Npad x n_beta] with the n_beta entries of a
// column contiguous, plus H and its Cholesky factor R.  The sweeps ride in rows 0 .. n_beta - 1 of one 64-row tile of Wt, which
// every predict clears before it writes its own rows.
// Per call (gpg_meanunc_rows): partial products of K-chunks of the columns, added in chunk order, then per row
//     c'_r = R^-1 u_r,  q_r = |c'_r|^2 = u_r^T H^-1 u_r,  c_r = R^-T c'_r = H^-1 u_r.
// Ordinary grids, no atomics, no workgroup waits for another: the results are a function of the shape only.
#include <cmath>
#include "gpg_internal.h"

namespace {

constexpr int kMuChunk = 256, kMuSlices = 4;
constexpr double kMuPivTol = 1e-12;          // the pivot rule of lkd_reduce_lin_kernel
constexpr int kMuWorkgroups = 512;           // (row tile, K-chunk) workgroups of mu_u_partial_kernel, about
constexpr int kMuChunksMax = 64;             // at most this many K-chunks: one sum of mu_u_finish_kernel is two rounds of loads at most
constexpr int kSmallH = 0, kSmallR = GPG_MU_SMALL_R, kSmallFlag = 2 * GPG_MAX_NBETA * GPG_MAX_NBETA;
constexpr int kSmallCount = GPG_MU_SMALL;

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rows 0 .. nb - 1 of the carrier tile W (RHS-rows layout, leading dimension 64) <- the columns of V P^-1: training column c < n
// (value of point c) holds [1, x_c], gradient column c = n + i ng + g (d/dx_i at the g-th point that carries a gradient) holds
// e_(i+1); with the constant mean (nb == 1) the single row is [1_n; 0].  As prep_rows_kernel writes them below the matrix.
__global__ void __launch_bounds__(256) mu_vand_rows_kernel(int n, int ng, int N, int nb, const double* __restrict__ Xt,
                                                           const double* __restrict__ invp, double* __restrict__ W) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const double ip = invp[c];
  double* w = W + (size_t)c * 64;
  if (c < n) {
    w[0] = ip;
    for (int j = 1; j < nb; ++j) w[j] = Xt[(size_t)(j - 1) * n + c] * ip;
  } else if (nb > 1) {
    w[(c - n) / ng + 1] = ip;
  }
}

// out[c * nb + i] = W[c * 64 + i]: the swept rows of the carrier tile, compact
__global__ void __launch_bounds__(256) mu_compact_kernel(const double* __restrict__ W, int Npad, int nb, double* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Npad * nb) return;
  const int c = t / nb, i = t - c * nb;
  out[t] = W[(size_t)c * 64 + i];
}

// H = W_V^T W_V over the N columns and its Cholesky factor, by ONE workgroup (the pattern of lkd_reduce_lin_kernel): column chunks
// of kMuChunk columns x nb rows are staged in LDS (row stride kMuChunk + 1), thread (pair, slice) owns one entry (i, j), i <= j, over
// the columns = slice (mod kMuSlices); the slices are added in slice order.  H = R R^T by wave 0 alone (lane <-> row); a pivot that
// is not above kMuPivTol times the diagonal entry it started from is reported as flag = pivot + 1.
// small: H [nb x nb] | R [nb x nb] (lower, zeros above) | flag
__global__ void __launch_bounds__(1024) mu_gram_chol_kernel(const double* __restrict__ WV, int N, int nb, double* __restrict__ small) {
  __shared__ double rows[GPG_MAX_NBETA][kMuChunk + 1];
  __shared__ double part[kMuSlices][256];
  __shared__ double G[GPG_MAX_NBETA][GPG_MAX_NBETA + 1];
  __shared__ double diag0[GPG_MAX_NBETA];
  const int npair = nb * (nb + 1) / 2;
  const int tid = threadIdx.x, pr = tid & 255, sl = tid >> 8;
  int pi = 0, pj = 0;
  if (pr < npair) {
    int q = pr;
    while (q > pj) { q -= pj + 1; ++pj; }
    pi = q;
  }
  double acc = 0.0;
  for (int c0 = 0; c0 < N; c0 += kMuChunk) {
    const int cn = min(kMuChunk, N - c0);
    __syncthreads();
    for (int t = tid; t < cn * nb; t += blockDim.x) {
      const int cc = t / nb, r = t - cc * nb;
      rows[r][cc] = WV[(size_t)c0 * nb + t];
    }
    __syncthreads();
    if (pr < npair)
      for (int cc = sl; cc < cn; cc += kMuSlices) acc += rows[pi][cc] * rows[pj][cc];
  }
  part[sl][pr] = acc;
  __syncthreads();
  if (sl == 0 && pr < npair) {
    double s = part[0][pr];
    for (int q = 1; q < kMuSlices; ++q) s += part[q][pr];
    G[pj][pi] = s;
    G[pi][pj] = s;
  }
  __syncthreads();
  if (tid < nb * nb) small[kSmallH + tid] = G[tid / nb][tid % nb];
  __syncthreads();
  if (tid < 64) {
    if (tid < nb) diag0[tid] = G[tid][tid];
    int s = 0;
    for (int k = 0; k < nb; ++k) {
      wave_lds_sync();
      const double piv = G[k][k];
      if (!(piv > kMuPivTol * diag0[k])) { s = k + 1; break; }
      const double ckk = sqrt(piv);
      wave_lds_sync();                                    // every lane has read the pivot before lane k overwrites it
      if (tid > k && tid < nb) G[tid][k] = G[tid][k] / ckk;
      if (tid == k) G[k][k] = ckk;
      wave_lds_sync();
      if (tid > k && tid < nb)
        for (int j = k + 1; j <= tid; ++j) G[tid][j] -= G[tid][k] * G[j][k];
    }
    wave_lds_sync();
    if (tid == 0) small[kSmallFlag] = (double)s;
  }
  __syncthreads();
  if (tid < nb * nb) {
    const int i = tid / nb, j = tid % nb;
    small[kSmallR + tid] = j <= i ? G[i][j] : 0.0;
  }
}

// partial[(s * NB + i) * mp + r] = sum over the columns c of K-chunk s of Z[c * ldz + r] W_V[c, i]  (grid = (mp / 64, S)): the skinny
// product [m x Npad] . [Npad x n_beta] behind U.  Chunk s holds the whole 64-column tiles [s ktiles / S, (s + 1) ktiles / S).
// Lane <-> query row (a wave reads 512 contiguous bytes of one column of Z), wave w takes the columns = w (mod 4) of the chunk,
// eight of them per trip (their loads in flight together: the kernel is bound by the latency and the bandwidth of Z); the n_beta
// entries of W_V at a column are the same address for every lane of the wave.  Every lane keeps NB accumulators; the four waves
// are added in wave order through LDS.  Z is read once: 8 m Npad bytes.
template <int NB>
__global__ void __launch_bounds__(256) mu_u_partial_kernel(const double* __restrict__ Z, int ldz, int ktiles, int S,
                                                           const double* __restrict__ WV, int mp, double* __restrict__ partial) {
  __shared__ double sh[3][NB][64];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the wave's column offset is uniform: W_V by scalar loads
  const int r = blockIdx.x * 64 + lane, s = blockIdx.y;
  const int c0 = (int)((long long)s * ktiles / S) * 64, c1 = (int)((long long)(s + 1) * ktiles / S) * 64;
  double acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) acc[i] = 0.0;
  for (int c = c0 + w; c < c1; c += 32) {   // chunks are whole 64-column tiles: two trips per tile
    double z[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) z[u] = Z[(size_t)(c + 4 * u) * ldz + r];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double* wv = WV + (size_t)(c + 4 * u) * NB;
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[i] += z[u] * wv[i];
    }
  }
  if (w > 0) {
#pragma unroll
    for (int i = 0; i < NB; ++i) sh[w - 1][i][lane] = acc[i];
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int i = 0; i < NB; ++i)
      partial[((size_t)s * NB + i) * mp + r] = ((acc[i] + sh[0][i][lane]) + sh[1][i][lane]) + sh[2][i][lane];
  }
}

// Rows 64 b .. 64 b + 63 of workgroup b, row r = blk nx + j < m.  First u = v_r - the S <= kMuChunksMax partials in chunk order: wave
// w takes the coefficients i = w, w + (waves), ..., lane <-> row, up to 32 loads of a sum in flight at a time.  v_r =
// [1, xq_j] on a value row (blk = 0) and e_blk on the row of d/dx_(blk-1) (first-order mean; with the constant mean [1] and [0]: the
// basis of the derivative rows is a constant and is never stored).  Then wave 0, lane <-> row: c' = R^-1 u, q = |c'|^2, c = R^-T c'.
// cf / cb [NB x mp], q [mp].  Xq is [d x ldq].
template <int NB>
__global__ void __launch_bounds__(512) mu_u_finish_kernel(const double* __restrict__ partial, int S, int mp, int m, int nx,
                                                           const double* __restrict__ Xq, int ldq, const double* __restrict__ small,
                                                           double* __restrict__ cf, double* __restrict__ cb, double* __restrict__ q) {
  __shared__ double ush[NB][64];
  __shared__ double R[NB * NB];
  for (int t = threadIdx.x; t < NB * NB; t += blockDim.x) R[t] = small[kSmallR + t];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int r = blockIdx.x * 64 + lane;                   // < mp
  const int blk = r / nx, j = r - blk * nx;
  for (int i = w; i < NB; i += nw) {
    const double* pp = partial + (size_t)i * mp + r;
    const size_t stride = (size_t)NB * mp;
    double g = 0.0;
    for (int t0 = 0; t0 < S; t0 += 32) {                  // 32 loads in flight, added in chunk order all the same
      double v[32];
#pragma unroll
      for (int t = 0; t < 32; ++t) v[t] = t0 + t < S ? pp[(size_t)(t0 + t) * stride] : 0.0;
#pragma unroll
      for (int t = 0; t < 32; ++t) g += v[t];             // (chunks >= S add +0.0)
    }
    double b = 0.0;
    if (r < m) {
      if (blk == 0) b = i == 0 ? 1.0 : Xq[(size_t)(i - 1) * ldq + j];
      else b = (NB > 1 && i == blk) ? 1.0 : 0.0;
    }
    ush[i][lane] = b - g;
  }
  __syncthreads();
  if (w != 0 || r >= m) return;
  // the two substitutions in place in the lane's own column of ush (rolled loops: R and u stay in LDS, R is a broadcast read)
  double qq = 0.0;
#pragma unroll 1
  for (int i = 0; i < NB; ++i) {          // R c' = u
    double t = ush[i][lane];
#pragma unroll 1
    for (int k = 0; k < i; ++k) t -= R[i * NB + k] * ush[k][lane];
    t /= R[i * NB + i];
    ush[i][lane] = t;
    qq += t * t;
    cf[(size_t)i * mp + r] = t;
  }
  q[r] = qq;
#pragma unroll 1
  for (int i = NB - 1; i >= 0; --i) {     // R^T c = c'
    double t = ush[i][lane];
#pragma unroll 1
    for (int k = i + 1; k < NB; ++k) t -= R[k * NB + i] * ush[k][lane];
    t /= R[i * NB + i];
    ush[i][lane] = t;
    cb[(size_t)i * mp + r] = t;
  }
}

// Z[c * ldz + j] += sum_i cb[i * mp + j] (K^-1 V)[c, i] for the nx backward-swept rows: K^-1 k becomes t = K^-1 k + K^-1 V H^-1 u,
// the row cross_grad_kernel (and the Hessian contraction) then read.  Thread <-> (column c, row j), j fastest.
template <int NB>
__global__ void __launch_bounds__(256) mu_row_update_kernel(double* __restrict__ Z, int ldz, int N, int nx, int nxs,
                                                            const double* __restrict__ KV, const double* __restrict__ cb, int mp) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int j = (int)(t % nxs);
  const long long c = t / nxs;
  if (c >= N || j >= nx) return;
  const double* kv = KV + (size_t)c * NB;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NB; ++i) s += cb[(size_t)i * mp + j] * kv[i];
  Z[(size_t)c * ldz + j] += s;
}

// lower tile t of a (T x T)-tile matrix (as joint.hip)
__device__ __forceinline__ void lower_tile(int t, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// cov[row, col] += varK sum_i cf[i, row] cf[i, col] for col <= row of every lower 64 x 64 tile (grid = (ntiles, 16), the mapping of
// gram_finish_kernel), written to both triangles: one sum in one order per pair, so cov stays exactly symmetric.
__global__ void __launch_bounds__(256) mu_cov_add_kernel(const double* __restrict__ cf, int nb, int mp, int m, double varK,
                                                         double* __restrict__ cov) {
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int p = e & 63, qd = e >> 6;
  const int row = ti * 64 + p, col = tj * 64 + qd;
  if (col > row || row >= m) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += cf[(size_t)i * mp + row] * cf[(size_t)i * mp + col];
  const double v = cov[(size_t)row * m + col] + varK * s;
  cov[(size_t)row * m + col] = v;
  cov[(size_t)col * m + row] = v;
}

#define MU_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17)

// K-chunks of mu_u_partial_kernel for mp rows and Npad columns: a function of the shape only
int mu_chunks(int mp, int Npad) {
  const int ktiles = Npad / 64, T = mp / 64;
  int s = (kMuWorkgroups + T - 1) / T;
  if (s > kMuChunksMax) s = kMuChunksMax;
  return s < 1 ? 1 : (s > ktiles ? ktiles : s);
}

}  // namespace

void gpg_meanunc_free(gpg_ctx* c) {
  if (c->mu_buf) (void)hipFree(c->mu_buf);
  if (c->mu_small) (void)hipFree(c->mu_small);
  if (c->mu_scr) (void)hipFree(c->mu_scr);
  c->mu_buf = c->mu_small = c->mu_scr = nullptr;
  c->mu_buf_elems = c->mu_scr_elems = 0;
  c->mu_ready = false;
}

// Builds W_V, K^-1 V, H and R for the posterior kept in workspace set 1 (which the caller has made the active one) unless they
// are there already.  0; -1: H is not positive definite (message names the pivot); -2: HIP / memory; -4: a dataflow sweep timed out.
int gpg_meanunc_ensure(gpg_ctx* c) {
  if (c->mu_ready) return 0;
  const int nb = c->n_beta, Npad = c->Npad;
  if (int rc = gpg_predict_bufs(c, 64)) return rc;
  const size_t need = (size_t)2 * nb * Npad;
  if (need > c->mu_buf_elems) {
    if (c->mu_buf) (void)hipFree(c->mu_buf);
    c->mu_buf = nullptr; c->mu_buf_elems = 0;
    if (hipMalloc(&c->mu_buf, sizeof(double) * need) != hipSuccess) {
      (void)hipGetLastError();
      c->mu_buf = nullptr;
      c->err = "out of device memory for the mean-uncertainty state";
      return -2;
    }
    c->mu_buf_elems = need;
  }
  if (!c->mu_small) GPG_HIP_OK(c, hipMalloc(&c->mu_small, sizeof(double) * kSmallCount));
  double* WV = c->mu_buf;
  double* KV = c->mu_buf + (size_t)nb * Npad;
  GPG_HIP_OK(c, hipMemsetAsync(c->Wt, 0, sizeof(double) * (size_t)64 * Npad, c->stream));
  GPG_HIP_OK(c, hipMemsetAsync(c->info, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(mu_vand_rows_kernel, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->n, c->ng > 0 ? c->ng : 1, c->N, nb, c->Xt,
                     c->invp, c->Wt);
  gpg_forward_rows(c, c->Wt, 64, 64, nb);
  const unsigned cgrid = (unsigned)(((size_t)Npad * nb + 255) / 256);
  hipLaunchKernelGGL(mu_compact_kernel, dim3(cgrid), dim3(256), 0, c->stream, c->Wt, Npad, nb, WV);
  gpg_backward_rows(c, c->Wt, 64, nb, c->gradbuf + (size_t)2 * 64 * GPG_MAX_DIM);
  hipLaunchKernelGGL(mu_compact_kernel, dim3(cgrid), dim3(256), 0, c->stream, c->Wt, Npad, nb, KV);
  hipLaunchKernelGGL(mu_gram_chol_kernel, dim3(1), dim3(1024), 0, c->stream, WV, c->N, nb, c->mu_small);
  GPG_HIP_OK(c, hipMemcpyAsync(c->mu_host, c->mu_small, sizeof(double) * kSmallCount, hipMemcpyDeviceToHost, c->stream));
  GPG_HIP_OK(c, hipMemcpyAsync(c->h_info, c->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
  GPG_HIP_OK(c, hipGetLastError());
  GPG_LAUNCH_OK(c);
  if (gpg_solve_failure(c)) return -4;
  const int flag = (int)c->mu_host[kSmallFlag];
  if (flag != 0) {
    c->err = "V' Kcov^-1 V of the kept posterior is not positive definite: pivot " + std::to_string(flag - 1) +
             " of " + std::to_string(nb) + " fails the 1e-12 rule (V has no full column rank in the K^-1 inner product)";
    return -1;
  }
  c->mu_ready = true;
  return 0;
}

// After the forward sweep of the m query rows Z (RHS-rows layout, leading dimension ldz, row r = blk nx + j, query coordinates in
// xq_dev [d x ldz]): c' -> mu_cf, c -> mu_cb [n_beta x ldz], q -> mu_q [ldz] (all inside mu_scr, contiguous in this order).
int gpg_meanunc_rows(gpg_ctx* c, const double* Z, int ldz, int m, int nx) {
  const int nb = c->n_beta, Npad = c->Npad, ktiles = Npad / 64;
  const int S = mu_chunks(ldz, Npad);
  const size_t need = (size_t)S * nb * ldz + (size_t)2 * nb * ldz + ldz;
  if (need > c->mu_scr_elems) {
    if (c->mu_scr) (void)hipFree(c->mu_scr);
    c->mu_scr = nullptr; c->mu_scr_elems = 0;
    if (hipMalloc(&c->mu_scr, sizeof(double) * need) != hipSuccess) {
      (void)hipGetLastError();
      c->mu_scr = nullptr;
      c->err = "out of device memory for the mean-uncertainty scratch";
      return -2;
    }
    c->mu_scr_elems = need;
  }
  c->mu_cf = c->mu_scr;
  c->mu_cb = c->mu_cf + (size_t)nb * ldz;
  c->mu_q = c->mu_cb + (size_t)nb * ldz;
  double* partial = c->mu_q + ldz;
  const double* WV = c->mu_buf;
  gpg_prof_begin(c, GPG_PROF_REDUCE, 8.0 * m * (double)Npad);   // the event time of the hot kernel, against the bytes of Z it reads
#define X(NBV)                                                                                                                  \
  case NBV:                                                                                                                     \
    hipLaunchKernelGGL((mu_u_partial_kernel<NBV>), dim3(ldz / 64, S), dim3(256), 0, c->stream, Z, ldz, ktiles, S, WV, ldz, partial); \
    break;
  switch (nb) { MU_CASES(X) }
#undef X
  gpg_prof_end(c);
#define X(NBV)                                                                                                                  \
  case NBV:                                                                                                                     \
    hipLaunchKernelGGL((mu_u_finish_kernel<NBV>), dim3((m + 63) / 64), dim3(64 * (NBV < 8 ? NBV : 8)), 0, c->stream, partial, S, ldz, m, nx, c->xq_dev, ldz, \
                       c->mu_small, c->mu_cf, c->mu_cb, c->mu_q);                                                               \
    break;
  switch (nb) { MU_CASES(X) }
#undef X
  return 0;
}

// rows 0 .. nx - 1 of the backward-swept Z += their c (mu_cb of the gpg_meanunc_rows call before) times K^-1 V
void gpg_meanunc_update_rows(gpg_ctx* c, double* Z, int ldz, int nx) {
  const int nxs = ((nx + 63) / 64) * 64;
  const long long total = (long long)c->N * nxs;
  const dim3 grid((unsigned)((total + 255) / 256));
  const double* KV = c->mu_buf + (size_t)c->n_beta * c->Npad;
#define X(NBV)                                                                                                                  \
  case NBV:                                                                                                                     \
    hipLaunchKernelGGL((mu_row_update_kernel<NBV>), grid, dim3(256), 0, c->stream, Z, ldz, c->N, nx, nxs, KV, c->mu_cb, ldz);       \
    break;
  switch (c->n_beta) { MU_CASES(X) }
#undef X
}

// cov_dev [m x m] += varK C' C'^T (mu_cf of the gpg_meanunc_rows call before, leading dimension mp)
void gpg_meanunc_add_cov(gpg_ctx* c, int m, int mp, double varK, double* cov_dev) {
  const int T = mp / 64, ntiles = T * (T + 1) / 2;
  hipLaunchKernelGGL(mu_cov_add_kernel, dim3(ntiles, 16), dim3(256), 0, c->stream, c->mu_cf, c->n_beta, mp, m, varK, cov_dev);
}

static int mean_gram_once(gpg_ctx* c, double* H) {
  if (!c->eval_ready) { c->err = "gpg_setup_eval must succeed before gpg_mean_gram"; return -1; }
  GPG_HIP_OK(c, hipSetDevice(c->device));
  if (gpg_ws_activate(c, 1) != 0) return -2;
  const int rc = gpg_meanunc_ensure(c);
  if (rc != 0 && rc != -1) return rc;                 // -1: H is not positive definite; it is in mu_host all the same
  const int nb = c->n_beta;
  for (int i = 0; i < nb * nb; ++i) H[i] = c->mu_host[kSmallH + i];
  return rc;
}

extern "C" {

int gpg_set_mean_uncertainty(gpg_ctx* c, int on) {
  if (!c) return -1;
  if (on != 0 && on != 1) { c->err = "mean uncertainty switch must be 0 (off) or 1 (on)"; return -1; }
  c->mean_unc = on;
  return 0;
}

int gpg_mean_gram(gpg_ctx* c, double* H) {
  if (!c) return -1;
  if (!H) { c->err = "H is NULL"; return -1; }
  return gpg_with_fallback(c, [&] { return mean_gram_once(c, H); });
}

}  // extern "C"
