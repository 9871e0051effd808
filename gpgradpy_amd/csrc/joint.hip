// Joint posterior at many query points (gpg_predict_joint, include/gpgrad.h): mean and full covariance of
//     [f(x_1..x_nx); d f / d x_1 (x_1..x_nx); ...; d f / d x_d (x_1..x_nx)]       (row r = blk * nx + j)
// from the factor kept by gpg_setup_eval:
//     cov = varK (Kqq - Kqy Kcov^-1 Kyq) = varK (Kqq - Z Z^T),   Z = Kqy P^-1 L^-T.
// Steps, all on the context's stream: cross_joint_kernel writes the m rows of Kqy P^-1 in the RHS-rows layout, the mean is
// their product with p * alpha (as gpg_predict's), gpg_forward_rows sweeps them, rows_gram_splitk_kernel forms the partial
// Gram matrices of K-chunks on fp64 MFMA, gram_finish_kernel adds them in chunk order and writes varK (Kqq - G) to both
// triangles.  Kqq comes from the kernel-table kernel (gpg_kern_rtensor_run) on a device-built difference tensor.
// The launches are ordinary grids: no workgroup waits for another one, nothing is accumulated with atomics.
// Compiled with -ffp-contract=off like assembly.hip: the kernel entries keep the operation order of cross_kernel /
// cross_dx_rows_kernel.
#include <cmath>
#include <cstring>
#include <vector>
#include "gpg_internal.h"
#include "device_util.h"
#include "kernel_fn.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kJointMaxRows = 4096;   // m padded to 64: cov is at most 4096 x 4096 (128 MiB)
constexpr int kMeanSlicesMax = 128;

// Wt[c * mp + r] = (Kqy P^-1)[r, c] for every training row c < N and every query row r = B * nx + j < m: value rows (B = 0) carry
// the entries of cross_kernel, derivative rows (B = 1 + jp) those of cross_dx_rows_kernel, for all nx query points.
// Thread <-> (training point a, query point j), j fastest: the 64 lanes of a wave store 512 contiguous bytes of one
// (column, block).  Rows m .. mp - 1 and columns N .. Npad - 1 are left as the caller cleared them.  Xq is [D x mp].
template <int KERN, int D>
__global__ void __launch_bounds__(256) cross_joint_kernel(AsmParams P, const double* __restrict__ Xt, const double* __restrict__ Xq,
                                                          int nx, int nxs, int qblk, int mp, const double* __restrict__ invp,
                                                          double* __restrict__ Wt) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int j = (int)(t % nxs);
  const long long a_ll = t / nxs;
  if (a_ll >= P.n || j >= nx) return;
  const int a = (int)a_ll, n = P.n, ng = P.ng;
  const int nblk = P.use_grad ? D + 1 : 1;
  double R[D], th[D], s = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) { th[i] = P.theta[i]; R[i] = Xt[(size_t)i * n + a] - Xq[(size_t)i * mp + j]; kern_s_add<KERN, false>(s, th[i], R[i]); }
  const KernRadial rad = kern_radial<KERN>(s, P.hp_kernel);
  const double E = rad.E, M1 = rad.M1, K00 = rad.K00;
  {   // value column of training point a
    const double ip = invp[a];
    double* w = Wt + (size_t)a * mp + j;
    w[0] = K00 * ip;
    if (qblk > 1) {
#pragma unroll
      for (int jp = 0; jp < D; ++jp)
        w[(size_t)(jp + 1) * nx] = ip * kern_d01<KERN>(th[jp], R[jp], E, M1);
    }
  }
  const int gpa = P.gpos[a];
  if (nblk > 1 && gpa >= 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) {   // gradient column (i, a)
      const size_t c = (size_t)n + (size_t)i * ng + gpa;
      const double ip = invp[c];
      double* w = Wt + c * mp + j;
      w[0] = kern_d10<KERN>(th[i], R[i], E, M1) * ip;
      if (qblk > 1) {
#pragma unroll
        for (int jp = 0; jp < D; ++jp)
          w[(size_t)(jp + 1) * nx] = ip * kern_d11<KERN>(i == jp, th[i], th[jp], R[i], R[jp], E, M1, kern_rq_c(P.hp_kernel));
      }
    }
  }
}

// partial[q * mp + r] = sum over the columns c of slice q of Wt[c * mp + r] z[c]   (grid = (mp / 64, S))
__global__ void __launch_bounds__(1024) joint_mean_partial_kernel(const double* __restrict__ Wt, int mp, int N, int chunk,
                                                                  const double* __restrict__ z, double* __restrict__ partial) {
  __shared__ double sh[16][64];
  const int rl = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const int r = blockIdx.x * 64 + rl;
  const int c0 = blockIdx.y * chunk, c1 = min(N, c0 + chunk);
  double acc = 0.0, comp = 0.0;
  for (int c = c0 + cg; c < c1; c += 16) kb_add(acc, comp, Wt[(size_t)c * mp + r] * z[c]);
  sh[cg][rl] = acc + comp;
  __syncthreads();
  if (cg == 0) {
    double s = 0.0, cs = 0.0;
    for (int q = 0; q < 16; ++q) kb_add(s, cs, sh[q][rl]);
    partial[(size_t)blockIdx.y * mp + r] = s + cs;
  }
}

// mean[r] = prior mean of row r + the slices in order.  Prior mean: value row j: beta (constant mean) or beta_0 + xq_j . beta_1..d;
// derivative row (k, j): 0 or beta_(k+1)
__global__ void __launch_bounds__(256) joint_mean_final_kernel(const double* __restrict__ partial, int mp, int m, int nx, int S, double beta,
                                                               const double* __restrict__ betav, const double* __restrict__ Xq, int d,
                                                               double* __restrict__ mean) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  double s = 0.0, cs = 0.0;
  for (int q = 0; q < S; ++q) kb_add(s, cs, partial[(size_t)q * mp + r]);
  s += cs;
  const int blk = r / nx, j = r - blk * nx;
  double pm;
  if (blk == 0) {
    pm = betav ? betav[0] : beta;
    if (betav) for (int k = 0; k < d; ++k) pm += betav[k + 1] * Xq[(size_t)k * mp + j];
  } else {
    pm = betav ? betav[blk] : 0.0;
  }
  mean[r] = pm + s;
}

// Difference tensor of the query points with themselves, R[k, a, b] = xq[a, k] - xq[b, k], and the identity gradient positions
__global__ void __launch_bounds__(256) joint_qdiff_kernel(const double* __restrict__ Xq, int mp, int nx, int d, double* __restrict__ Rt,
                                                          int* __restrict__ gpos) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long np = (long long)nx * nx;
  if (t < nx) gpos[t] = (int)t;
  if (t >= np) return;
  const int a = (int)(t / nx), b = (int)(t - (long long)a * nx);
  for (int k = 0; k < d; ++k) Rt[(size_t)k * np + t] = Xq[(size_t)k * mp + a] - Xq[(size_t)k * mp + b];
}

// lower tile t of a (T x T)-tile matrix, row-major over the triangle: t = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void lower_tile(int t, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// Partial Gram matrices of the swept rows Z (RHS-rows layout Z[c * mp + r], mp a multiple of 64):
//   partial[(s * ntiles + t)][q * 64 + p] = sum over the columns c of K-chunk s of Z[ti 64 + p, c] Z[tj 64 + q, c]
// for the lower 64 x 64 tile t = (ti, tj) (grid = (ntiles, splits)); chunk s holds the whole 64-column tiles
// [s ktiles / splits, (s + 1) ktiles / splits).  One workgroup = 4 waves, wave (wm, wn) owns the 32 x 32 quadrant as 2 x 2 MFMA
// 16 x 16 x 4 fp64 blocks (register layout of gemm_nt_minus_kernel: lane (l15, l4) feeds row l15 of k-slice l4 and holds
// C[l15, 4 r + l4] in element r).  Operands come straight from global memory: 16 consecutive rows are contiguous, so every
// 16-lane group reads 128 bytes; a k-step of 4 columns is 4 loads and 4 MFMAs per lane.  The contraction is skinny (m <= 4096
// rows, up to 68 000 columns), so the K split is what fills the device.
__global__ void __launch_bounds__(256) rows_gram_splitk_kernel(const double* __restrict__ Z, int mp, int ktiles, int splits,
                                                               double* __restrict__ partial) {
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int s = blockIdx.y;
  const int k0 = (int)((long long)s * ktiles / splits) * 64, k1 = (int)((long long)(s + 1) * ktiles / splits) * 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wm = w & 1, wn = w >> 1, l15 = lane & 15, l4 = lane >> 4;
  const double* zp = Z + (size_t)(k0 + l4) * mp + ti * 64 + wm * 32 + l15;
  const double* zq = Z + (size_t)(k0 + l4) * mp + tj * 64 + wn * 32 + l15;
  const size_t step = (size_t)4 * mp;
  d4 acc[2][2] = {};
  for (int k = k0; k < k1; k += 16) {   // chunks are whole 64-column tiles: four k-steps per trip, their 16 loads in flight together
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double fm0 = zp[0], fm1 = zp[16], fn0 = zq[0], fn1 = zq[16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn0, fm0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn0, fm1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn1, fm0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn1, fm1, acc[1][1], 0, 0, 0);
      zp += step;
      zq += step;
    }
  }
  double* out = partial + ((size_t)s * gridDim.x + blockIdx.x) * 4096 + wm * 32 + l15;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(wn * 32 + ni * 16 + 4 * r + l4) * 64 + mi * 16] = acc[ni][mi][r];
}

// cov = varK (Kqq - sum_s partial_s), the chunks added in order s = 0, 1, ...; entry (row, col), col <= row, of lower tile t
// goes to both triangles of the row-major [m, m] output (the diagonal tiles use their own lower half only: exactly symmetric)
__global__ void __launch_bounds__(256) gram_finish_kernel(const double* __restrict__ partial, int ntiles, int splits,
                                                          const double* __restrict__ Kqq, int m, double varK, double* __restrict__ cov) {
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int e = blockIdx.y * 256 + threadIdx.x;   // grid = (ntiles, 16): one entry of the tile per thread
  const int p = e & 63, q = e >> 6;
  const int row = ti * 64 + p, col = tj * 64 + q;
  if (col > row || row >= m) return;
  const double* part = partial + (size_t)blockIdx.x * 4096 + e;
  const size_t stride = (size_t)ntiles * 4096;
  double g = 0.0;
  int s = 0;
  for (; s + 8 <= splits; s += 8) {   // eight loads in flight, added in chunk order all the same
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(s + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) g += v[u];
  }
  for (; s < splits; ++s) g += part[(size_t)s * stride];
  const double v = varK * (Kqq[(size_t)row * m + col] - g);
  cov[(size_t)row * m + col] = v;
  cov[(size_t)col * m + row] = v;
}

// K-chunks of the Gram kernel for mp rows and Npad columns: about 2048 (tile, chunk) workgroups, a function of the shape only.
// Measured at Npad = 18048 (tools/joint_time.py --splits ... under a kernel trace): 3 tiles 992 us with one chunk, 27 us with 48,
// 16-17 us with 141 .. 282; 45 tiles 936 / 181 / 143 / 138 / 136 / 177 us with 1 / 12 / 16 / 48 / 96 / 282 chunks; 666 tiles
// 2278 / 2041 / 1950 / 1929 / 2591 us with 1 / 4 / 8 / 24 / 282.  The partials stay within ~2 x 2048 x 32 KB.
constexpr int kGramWorkgroups = 2048;
int gram_splits_for(int mp, int Npad, int requested) {
  const int ktiles = Npad / 64, T = mp / 64, ntiles = T * (T + 1) / 2;
  int s = requested > 0 ? requested : (kGramWorkgroups + ntiles - 1) / ntiles;
  return s < 1 ? 1 : (s > ktiles ? ktiles : s);
}

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

// The rows of Kqy P^-1 of nx query points (xq_dev [d x mp]) into Wt, qblk = 1 (values) or d + 1 (values and derivatives) blocks
void gpg_launch_cross_joint(gpg_ctx* c, const AsmParams& p, int nx, int qblk, int mp) {
  const int nxs = ((nx + 63) / 64) * 64;
  const long long total = (long long)p.n * nxs;
  const dim3 grid((unsigned)((total + 255) / 256));
  gpg_for_kern_d(p.kernel, p.d, [&](auto K, auto D) {
    hipLaunchKernelGGL((cross_joint_kernel<decltype(K)::value, decltype(D)::value>), grid, dim3(256), 0, c->stream, p, c->Xt, c->xq_dev, nx,
                       nxs, qblk, mp, c->invp, c->Wt);
  });
}

// slices of the mean reduction: mpart of gpg_launch_joint_mean holds this many times mp doubles
int gpg_joint_mean_slices(const gpg_ctx* c) {
  const int ktiles = c->Npad / 64;
  return ktiles < kMeanSlicesMax ? ktiles : kMeanSlicesMax;
}

// mean_dev[r] = prior mean + (Kqy P^-1)[r, :] (p * alpha) for the m rows that gpg_launch_cross_joint left in Wt (before the sweep)
void gpg_launch_joint_mean(gpg_ctx* c, int mp, int m, int nx, double* mpart, double* mean_dev) {
  const int S = gpg_joint_mean_slices(c);
  const int chunk = (c->N + S - 1) / S;
  hipLaunchKernelGGL(joint_mean_partial_kernel, dim3(mp / 64, S), dim3(1024), 0, c->stream, c->Wt, mp, c->N, chunk, c->zvec, mpart);
  hipLaunchKernelGGL(joint_mean_final_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, mpart, mp, m, nx, S, c->eval_beta,
                     c->eval_linear ? c->eval_beta_dev : (const double*)nullptr, c->xq_dev, c->d, mean_dev);
}

namespace {

int predict_joint_once(gpg_ctx* c, int nx, const double* xq, double varK, int with_grad, double* mean, double* cov) {
  if (!c) return -1;
  if (!c->eval_ready) { c->err = "gpg_setup_eval must succeed before gpg_predict_joint"; return -1; }
  if (nx < 1 || !xq) { c->err = "bad gpg_predict_joint arguments"; return -1; }
  const int d = c->d, qblk = with_grad ? d + 1 : 1;
  const long long m_ll = (long long)nx * qblk;
  if (((m_ll + 63) / 64) * 64 > kJointMaxRows) {
    c->err = "gpg_predict_joint: nx (dim + 1) rows (nx without gradients), padded to 64, must not exceed 4096";
    return -1;
  }
  const int m = (int)m_ll, mp = ((m + 63) / 64) * 64;
  GPG_HIP_OK(c, hipSetDevice(c->device));
  if (gpg_ws_activate(c, 1) != 0) return -2;
  if (int rc = gpg_predict_bufs(c, mp)) return rc;
  const bool munc = c->mean_unc != 0 && cov != nullptr;   // uncertainty of the mean coefficients (meanunc.hip): cov += varK U H^-1 U^T
  if (munc) {
    if (int rc = gpg_meanunc_ensure(c)) return rc;
  }
  const int Npad = c->Npad, ktiles = Npad / 64, T = mp / 64, ntiles = T * (T + 1) / 2;
  const int splits = gram_splits_for(mp, Npad, c->gram_splits);
  const int S = gpg_joint_mean_slices(c);
  // scratch: Gram partials | Kqq | cov | difference tensor | mean partials | mean | gradient positions
  const size_t b_part = cov ? round256(sizeof(double) * (size_t)splits * ntiles * 4096) : 0;
  const size_t b_mm = cov ? round256(sizeof(double) * (size_t)m * m) : 0;
  const size_t b_rt = cov ? round256(sizeof(double) * (size_t)d * nx * nx) : 0;
  const size_t b_mpart = round256(sizeof(double) * (size_t)S * mp), b_mean = round256(sizeof(double) * mp);
  const size_t b_gpos = round256(sizeof(int) * (size_t)nx);
  const size_t need = b_part + 2 * b_mm + b_rt + b_mpart + b_mean + b_gpos;
  if (need > c->jbuf_bytes) {
    if (c->jbuf) (void)hipFree(c->jbuf);
    c->jbuf = nullptr; c->jbuf_bytes = 0;
    if (hipMalloc(&c->jbuf, need) != hipSuccess) {
      (void)hipGetLastError();
      c->jbuf = nullptr;
      c->err = "out of device memory for the joint posterior's scratch (fewer gpg_set_gram_splits chunks need less)";
      return -2;
    }
    c->jbuf_bytes = need;
  }
  char* base = reinterpret_cast<char*>(c->jbuf);
  double* part = reinterpret_cast<double*>(base);
  double* kqq = reinterpret_cast<double*>(base + b_part);
  double* cov_dev = reinterpret_cast<double*>(base + b_part + b_mm);
  double* rt = reinterpret_cast<double*>(base + b_part + 2 * b_mm);
  double* mpart = reinterpret_cast<double*>(base + b_part + 2 * b_mm + b_rt);
  double* mean_dev = reinterpret_cast<double*>(base + b_part + 2 * b_mm + b_rt + b_mpart);
  int* gpos = reinterpret_cast<int*>(base + b_part + 2 * b_mm + b_rt + b_mpart + b_mean);

  std::vector<double> xt((size_t)mp * d, 0.0);   // [d x mp], query point fastest
  for (int j = 0; j < nx; ++j)
    for (int k = 0; k < d; ++k) xt[(size_t)k * mp + j] = xq[(size_t)j * d + k];
  GPG_HIP_OK(c, hipMemcpyAsync(c->xq_dev, xt.data(), sizeof(double) * xt.size(), hipMemcpyHostToDevice, c->stream));
  GPG_HIP_OK(c, hipMemsetAsync(c->Wt, 0, sizeof(double) * (size_t)mp * Npad, c->stream));
  GPG_HIP_OK(c, hipMemsetAsync(c->info, 0, sizeof(int), c->stream));
  const AsmParams p = c->eval_params;
  gpg_launch_cross_joint(c, p, nx, qblk, mp);
  if (mean) {   // before the sweep: mean = prior + (Kqy P^-1) (p * alpha)
    gpg_launch_joint_mean(c, mp, m, nx, mpart, mean_dev);
    GPG_HIP_OK(c, hipMemcpyAsync(mean, mean_dev, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
  }
  if (cov) {
    gpg_forward_rows(c, c->Wt, mp, mp, m);
    if (munc) {
      if (int rc = gpg_meanunc_rows(c, c->Wt, mp, m, nx)) return rc;
    }
    hipLaunchKernelGGL(joint_qdiff_kernel, dim3((unsigned)(((long long)nx * nx + 255) / 256)), dim3(256), 0, c->stream, c->xq_dev, mp, nx, d,
                       rt, gpos);
    if (gpg_kern_rtensor_run(p.kernel, d, nx, nx, nx, nx, with_grad ? 1 : 0, p.theta, p.hp_kernel, rt, gpos, gpos, kqq, c->stream) != 0) {
      c->err = "gpg_predict_joint: the kernel-table launch for Kqq failed";
      return -2;
    }
    hipLaunchKernelGGL(rows_gram_splitk_kernel, dim3(ntiles, splits), dim3(256), 0, c->stream, c->Wt, mp, ktiles, splits, part);
    hipLaunchKernelGGL(gram_finish_kernel, dim3(ntiles, 16), dim3(256), 0, c->stream, part, ntiles, splits, kqq, m, varK, cov_dev);
    if (munc) gpg_meanunc_add_cov(c, m, mp, varK, cov_dev);
    GPG_HIP_OK(c, hipMemcpyAsync(cov, cov_dev, sizeof(double) * (size_t)m * m, hipMemcpyDeviceToHost, c->stream));
  }
  GPG_HIP_OK(c, hipMemcpyAsync(c->h_info, c->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));   // the dataflow sweep reports here
  GPG_HIP_OK(c, hipStreamSynchronize(c->stream));
  GPG_HIP_OK(c, hipGetLastError());
  GPG_LAUNCH_OK(c);
  if (gpg_solve_failure(c)) return -4;
  return 0;
}

}  // namespace

extern "C" {

int gpg_predict_joint(gpg_ctx* c, int nx, const double* xq, double varK, int with_grad, double* mean, double* cov) {
  return gpg_with_fallback(c, [&] { return predict_joint_once(c, nx, xq, varK, with_grad, mean, cov); });
}

int gpg_set_gram_splits(gpg_ctx* c, int n) {
  if (!c) return -1;
  if (n < 0) { c->err = "gram splits must be >= 0 (0 = chosen from the shape)"; return -1; }
  c->gram_splits = n;
  return 0;
}

}  // extern "C"
