// Triangular solves for right-hand-side rows as dataflow launches: rows_fwd_kernel, rows_bwd_kernel (64-row tiles) and
// vec_solve_kernel (one to four rows).
#pragma once
#include "dataflow_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// rows_fwd_kernel: W <- W L^-T for right-hand-side rows held OUTSIDE the matrix (rows layout, leading dimension ldw,
// 64-row tiles) against the finished factor in A, as ONE dataflow launch: workgroup (rt, j) owns the 64 x 64 block of
// row tile rt and column block j, accumulates  W_j - sum_{k<j} X_k L_jk^T  on MFMA as the X_k of its own row tile are
// published (the L tiles are final), substitutes against L_jj and raises flag(rt, j).  The blocked version
// (gpg_forward_rows: panel solve + GEMM launch per 512 columns) is bound by ~70 dependent launches of 100+ us each;
// here the chain per 64 columns is one 64-deep MFMA block, one substitution and one flag hop.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool
rows_fwd_task(int tix, const double* __restrict__ A, int ld, const double* __restrict__ dinv, double* W, int ldw, int Mt, int nrt,
              int valid, int* flags, int* abort_word, int* info) {
  constexpr int KB = 16, SA = 80, BUF = KB * SA;
  __shared__ __attribute__((aligned(16))) double U[4 * BUF];
  __shared__ __attribute__((aligned(16))) double Ls[64][4][18];
  __shared__ double sdinv[64];
  __shared__ int sh_kr;
  double* const sA = U;
  double* const sB = U + 2 * BUF;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int tj = tix / nrt, rt = tix - tj * nrt;                    // column-block-major task order
  const size_t r0 = 64 * (size_t)rt, cj = 64 * (size_t)tj;
  const int q = tid & 3;
  const int sp = tid & 31, sk = tid >> 5;
  int* const frow = flags + (size_t)rt * Mt;

  d4 acc[4];
  {
    const double* Cw = W + r0 + 16 * w + l15 + (cj + l4) * (size_t)ldw;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[ni][r] = Cw[(size_t)(ni * 16 + 4 * r) * ldw];
  }
  {   // L_jj is final: its image is fetched before the first wait
    const double* Ljj = A + cj + cj * (size_t)ld;
    for (int t = tid; t < 64 * 64; t += 256) {
      const int jj = t >> 6, k = t & 63;
      Ls[jj][k & 3][k >> 2] = Ljj[k + (size_t)jj * ld];
    }
    if (tid < 64) sdinv[tid] = dinv[cj + tid];
  }
  int kdone = 0;
  while (kdone < tj) {
    if (tid == 0) {
      int kr = kdone;
      const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        while (kr < tj && __hip_atomic_load(frow + kr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ++kr;
        if (kr > kdone) break;
        if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS ||
            __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          atomicMax(info, GPG_INFO_INTERNAL);
          kr = -1;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      sh_kr = kr;
    }
    __syncthreads();
    const int kr = __builtin_amdgcn_readfirstlane(sh_kr);
    if (kr < 0) return false;
    GPG_ACQUIRE();
    const size_t ck = 64 * (size_t)kdone;
    wave_tile_gemm(acc, W + r0 + 2 * sp + (ck + sk) * (size_t)ldw, ldw, A + cj + 2 * sp + (ck + sk) * (size_t)ld, ld,
                   4 * (kr - kdone), sA, sB, w, l15, l4, sp, sk);
    __syncthreads();
    kdone = kr;
  }
  {
    double* Ts = U;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ts[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = acc[ni][r];
  }
  __syncthreads();
  double x[16];
  {
    const double* Tr = U + q * SA + (tid >> 2);
#pragma unroll
    for (int m = 0; m < 16; ++m) x[m] = Tr[(4 * m) * SA];
  }
  if (64 * rt + 16 * w < valid) {   // rows >= valid are zero (and stay zero): their waves skip the substitution
    GPG_QUAD_SUBST(x, Ls, sdinv, q)
  }
  double* Xr = W + r0 + (tid >> 2) + (cj + q) * (size_t)ldw;
#pragma unroll
  for (int m = 0; m < 16; ++m) GPG_ST(&Xr[(size_t)(4 * m) * ldw], x[m]);
  GPG_RELEASE();
  __syncthreads();
  if (tid == 0) GPG_FLAG_UP(frow + tj);
  return true;
}

__global__ void __launch_bounds__(256, 2)
rows_fwd_kernel(const double* __restrict__ A, int ld, const double* __restrict__ dinv, double* W, int ldw, int Mt, int nrt,
                int valid, int* flags, int* abort_word, int* ticket, int* info) {
  __shared__ int sh_tix;
  const int ntask = Mt * nrt;
  for (;;) {
    const int tix = next_ticket(ticket, &sh_tix);
    if (tix >= ntask) return;
    if (!rows_fwd_task(tix, A, ld, dinv, W, ldw, Mt, nrt, valid, flags, abort_word, info)) return;
  }
}

// ------------------------------------------------------------------------------------------------
// rows_bwd_kernel: Z <- Z L^-1 (every row solved against L^T) for right-hand-side rows in the rows layout, ONE
// dataflow launch, column blocks from the last to the first: workgroup (rt, j) accumulates
// Z_j - sum_{k>j} Z_k L_kj on MFMA (L_kj used untransposed: k-major staging) as the Z_k of its row tile are
// published, then runs the reverse substitution against L_jj.  Replaces 2 x Npad/64 dependent launches
// (gpg_backward_rows).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool
rows_bwd_task(int tix, const double* __restrict__ A, int ld, const double* __restrict__ dinv, double* Z, int ldz, int Mt, int nrt,
              int valid, int* flags, int* abort_word, int* info) {
  constexpr int KB = 16, SA = 80, BUF = KB * SA;
  __shared__ __attribute__((aligned(16))) double U[4 * BUF];
  __shared__ __attribute__((aligned(16))) double Ls[64][4][18];   // transposed image: Ls[j][q][m] = L_jj[j][4m + q]
  __shared__ double sdinv[64];
  __shared__ int sh_kr;
  double* const sA = U;
  double* const sB = U + 2 * BUF;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int jr = tix / nrt, rt = tix - jr * nrt;
  const int tj = Mt - 1 - jr;                                      // last column block first
  const size_t r0 = 64 * (size_t)rt, cj = 64 * (size_t)tj;
  const int q = tid & 3;
  const int sp = tid & 31, sk = tid >> 5;
  int* const frow = flags + (size_t)rt * Mt;

  d4 acc[4];
  {
    const double* Cw = Z + r0 + 16 * w + l15 + (cj + l4) * (size_t)ldz;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[ni][r] = Cw[(size_t)(ni * 16 + 4 * r) * ldz];
  }
  {
    const double* Ljj = A + cj + cj * (size_t)ld;
    for (int t = tid; t < 64 * 64; t += 256) {
      const int cc = t >> 6, rr = t & 63;                          // element L_jj[rr][cc], read down the column
      Ls[rr][cc & 3][cc >> 2] = Ljj[rr + (size_t)cc * ld];
    }
    if (tid < 64) sdinv[tid] = dinv[cj + tid];
  }
  int khi = Mt;                                                    // blocks [khi, Mt) are applied
  while (khi > tj + 1) {
    if (tid == 0) {
      int kr = khi;
      const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        while (kr > tj + 1 && __hip_atomic_load(frow + kr - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) --kr;
        if (kr < khi) break;
        if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS ||
            __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          atomicMax(info, GPG_INFO_INTERNAL);
          kr = -1;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      sh_kr = kr;
    }
    __syncthreads();
    const int kr = __builtin_amdgcn_readfirstlane(sh_kr);
    if (kr < 0) return false;
    GPG_ACQUIRE();
    const size_t ck = 64 * (size_t)kr;                             // contraction rows [64 kr, 64 khi)
    wave_tile_gemm_nn(acc, Z + r0 + 2 * sp + (ck + sk) * (size_t)ldz, ldz, A + ck + cj * (size_t)ld, ld, 4 * (khi - kr), sA, sB, w,
                      l15, l4, sp, sk);
    __syncthreads();
    khi = kr;
  }
  {
    double* Ts = U;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ts[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = acc[ni][r];
  }
  __syncthreads();
  double x[16];
  {
    const double* Tr = U + q * SA + (tid >> 2);
#pragma unroll
    for (int m = 0; m < 16; ++m) x[m] = Tr[(4 * m) * SA];
  }
  if (64 * rt + 16 * w < valid) {
    GPG_QUAD_SUBST_REV(x, Ls, sdinv, q)
  }
  double* Xr = Z + r0 + (tid >> 2) + (cj + q) * (size_t)ldz;
#pragma unroll
  for (int m = 0; m < 16; ++m) GPG_ST(&Xr[(size_t)(4 * m) * ldz], x[m]);
  GPG_RELEASE();
  __syncthreads();
  if (tid == 0) GPG_FLAG_UP(frow + tj);
  return true;
}

__global__ void __launch_bounds__(256, 2)
rows_bwd_kernel(const double* __restrict__ A, int ld, const double* __restrict__ dinv, double* Z, int ldz, int Mt, int nrt,
                int valid, int* flags, int* abort_word, int* ticket, int* info) {
  __shared__ int sh_tix;
  const int ntask = Mt * nrt;
  for (;;) {
    const int tix = next_ticket(ticket, &sh_tix);
    if (tix >= ntask) return;
    if (!rows_bwd_task(tix, A, ld, dinv, Z, ldz, Mt, nrt, valid, flags, abort_word, info)) return;
  }
}

// ------------------------------------------------------------------------------------------------
// vec_solve_kernel<BWD, RR>: the same dataflow solves for at most RR (1 or 4) right-hand-side rows (posterior
// evaluation at one point, the alpha vector): no MFMA tile, no 64-row substitution.  Workgroup j owns column block
// j; lane <-> column c of the block, wave w accumulates the quarter m in [16w, 16w+16) of every finished block k
//     FWD: t[r][c] -= x_k[r][m] L[64j + c][64k + m]   (k < j)        BWD: t[r][c] -= z_k[r][m] L[64k + m][64j + c]  (k > j)
// with L read straight from memory (the block applied next is prefetched while the wave polls).  The solution is
// exchanged through a compact copy xc[r][Npad] that the host fills with a NaN sentinel: THE DATA IS THE FLAG -- a
// producer publishes x_k with agent-scope atomic stores, a consumer wave re-reads the 16 values it needs (one line)
// until none is the sentinel; no separate flag, no release/acquire fence on the chain.  The values are broadcast by
// v_readlane.  No barrier until the four partial sums meet in LDS; wave r (< R) then runs the 64-step substitution
// of row r in the scaled variable u = v / L_cc (two dependent instructions per step: v_readlane, v_fma) with the
// diagonal block held in registers.
// ------------------------------------------------------------------------------------------------
#define GPG_VEC_SENTINEL 0x7ff8dead7ff8deadull     // quiet NaN that no arithmetic produces; both halves equal (memsetD32)
template <int BWD, int RR>
__device__ __forceinline__ bool
vec_solve_task(int tix, const double* __restrict__ A, int ld, const double* __restrict__ dinv, double* W, int ldw, int Mt, int R,
               unsigned long long* xc, int Npad, int* abort_word, int* info) {
  __shared__ double part[4][RR][64];     // [wave][row][column] partial sums
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tj = BWD ? Mt - 1 - tix : tix;
  const size_t cj = 64 * (size_t)tj;
  const int ktot = BWD ? Mt - 1 - tj : tj;
  const double dv = dinv[cj + lane];
  // diagonal block, scaled by the lane's own reciprocal pivot: FWD lane c keeps row c of L_jj, BWD column c
  double Ls[64];
  double v0 = 0.0;
  if (w < R) {
#pragma unroll
    for (int m = 0; m < 64; ++m)
      Ls[m] = (BWD ? A[cj + m + (cj + lane) * (size_t)ld] : A[cj + lane + (cj + m) * (size_t)ld]) * dv;
    v0 = W[w + (cj + lane) * (size_t)ldw];
  }
  double t[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) t[r] = 0.0;
  double lcur[16];
  const bool carrier = lane < 16 * RR && (lane >> 4) < R;     // lane 16 r + mm carries x_k[r][16 w + mm]
  bool dead = false;
  for (int kk = 0; kk < ktot; ++kk) {      // FWD: k = kk, BWD: k = Mt-1-kk
    const size_t ck = 64 * (size_t)(BWD ? Mt - 1 - kk : kk);
#pragma unroll
    for (int mm = 0; mm < 16; ++mm) {
      const int m = 16 * w + mm;
      lcur[mm] = BWD ? A[ck + m + (cj + lane) * (size_t)ld] : A[cj + lane + (ck + m) * (size_t)ld];
    }
    const unsigned long long* src = xc + (size_t)(carrier ? lane >> 4 : 0) * Npad + ck + 16 * w + (lane & 15);
    unsigned long long bits = 0;
    unsigned long long t_wait = 0;
    for (;;) {
      bits = carrier ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
      if (!__any(bits == GPG_VEC_SENTINEL)) break;
      const unsigned long long now = __builtin_amdgcn_s_memrealtime();
      if (t_wait == 0) t_wait = now;
      if (now - t_wait > GPG_TILE_WAIT_TICKS || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (lane == 0) {
          __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          atomicMax(info, GPG_INFO_INTERNAL);
        }
        dead = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (dead) break;
    const double xv = __longlong_as_double((long long)bits);
#pragma unroll
    for (int r = 0; r < RR; ++r)
#pragma unroll
      for (int mm = 0; mm < 16; ++mm) t[r] -= readlane_d(xv, 16 * r + mm) * lcur[mm];
  }
#pragma unroll
  for (int r = 0; r < RR; ++r) part[w][r][lane] = t[r];
  __syncthreads();
  if (w < R && !dead) {
    const int r = w < RR ? w : 0;
    double u = (v0 + part[0][r][lane] + part[1][r][lane] + part[2][r][lane] + part[3][r][lane]) * dv;
    double x = 0.0;
    if (!BWD) {
#pragma unroll
      for (int m = 0; m < 64; ++m) {
        const double xm = readlane_d(u, m);
        u -= xm * Ls[m];                 // meaningful in lanes c > m; finished lanes are never read again
        x = (lane == m) ? xm : x;
      }
    } else {
#pragma unroll
      for (int m = 63; m >= 0; --m) {
        const double xm = readlane_d(u, m);
        u -= xm * Ls[m];
        x = (lane == m) ? xm : x;
      }
    }
    __hip_atomic_store(xc + (size_t)w * Npad + cj + lane, (unsigned long long)__double_as_longlong(x), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    W[w + (cj + lane) * (size_t)ldw] = x;
  }
  return !__syncthreads_or(dead ? 1 : 0);      // a wave that timed out ends the workgroup (the abort word drains the others)
}

struct VecSolveArgs {
  const double* A; int ld; const double* dinv; double* W; int ldw, Mt, R; unsigned long long* xc; int Npad; int* abort_word; int* ticket;
  int* info;
};

template <int BWD, int RR>
__device__ __noinline__ int vec_solve_task_call(int tix_v, unsigned long long kernarg_bits) {
  GPG_KERNARGS_FROM(VecSolveArgs, ap, kernarg_bits);
  const int tix = __builtin_amdgcn_readfirstlane(tix_v);
  return vec_solve_task<BWD, RR>(tix, ap->A, ap->ld, ap->dinv, ap->W, ap->ldw, ap->Mt, ap->R, ap->xc, ap->Npad, ap->abort_word, ap->info) ? 1 : 0;
}

template <int BWD, int RR>
__global__ void __launch_bounds__(256) vec_solve_kernel(VecSolveArgs) {
  __shared__ int sh_tix;
  for (;;) {
    GPG_KERNARGS(VecSolveArgs, ap);
    const int tix = next_ticket(ap->ticket, &sh_tix);
    if (tix >= ap->Mt) return;
    if (!__builtin_amdgcn_readfirstlane((vec_solve_task_call<BWD, RR>(tix, (unsigned long long)ap)))) return;
  }
}

}  // namespace
