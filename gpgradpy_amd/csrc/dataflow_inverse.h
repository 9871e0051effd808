// Explicit inverse -(L L^T)^-1 as dataflow launches: W = L^-T (tile128_trinv_kernel, tile64_trinv_kernel), then -(W W^T)
// (tile128_wwt_kernel, tile64_wwt_kernel).
#pragma once
#include "dataflow_chol128.h"

namespace {

// ------------------------------------------------------------------------------------------------
// tile128_trinv_kernel: W = L^-T (upper triangular, Npad x Npad, leading dimension ldw) from the finished factor L in A,
// as ONE dataflow launch over 128 x 128 tiles -- the first N^3/3 sweep of the explicit inverse that the adjoint
// likelihood gradient contracts with (reference: adj_ln_detK = cho_solve(chofac, eye(N)), CalcLkd.py:174,234).
// W starts as the identity.  Workgroup task (j, i), j <= i (row tile j, column tile i of W; list order: tile column by
// tile column, longest accumulation first):
//     acc  = W_ji - sum_{k=j}^{i-1} W_jk L_ik^T    the MFMA loop of the factorisation (A operand: W row tile j, B operand:
//                                                  L row tile i, both read in fragment layout straight from memory),
//                                                  consumed in runs as the flags of W's row tile j come up
//     W_ji = acc L_ii^-T                           the 128-row substitution of the factorisation's off-diagonal tiles
//                                                  against the (final) diagonal tile of L
//     publish flag(j, i)
// Persistent workgroups and ticket order as in tile_chol_kernel: (j, i) waits only for (j, k), k < i -- earlier tile
// columns, i.e. smaller tickets.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool
tile128_trinv_task(int tix, const double* __restrict__ A, int ld, const double* __restrict__ dinv, double* W, int ldw, int Mt,
                   const int* __restrict__ tasks, int* flags, int* abort_word, int* ticket, int* info,
                   const int* __restrict__ batch_of, size_t a_stride, size_t w_stride, int d_stride, int f_stride, int* lflags, int lf_mt) {
  __shared__ int sh_kr;
  __shared__ int sh_ok;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w & 1, wn = w >> 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int task = tasks[tix];
  const int tj = task & 0xffff, ti = task >> 16;          // row tile j of W, column tile i
  // Overlapped with a 64-tile factorisation (gpg_overlap_inverse_*): column tile ti of W needs the 128 rows 128 ti .. of L up to the
  // diagonal; they are final once the factorisation's diagonal tile (2 ti + 1, 2 ti + 1) is (its task consumed the rest of its row, and the
  // tile row above went the same way before it).
  // (lf_mt == 0: the factorisation runs on the same 128 x 128 tiling: its diagonal tile (ti, ti).)  The abort word is looked at FIRST, on
  // every task: the host raises it when the factorisation it overlaps turns out to have failed (gpg_overlap_inverse_cancel), and the launch
  // then drains within one task instead of inverting a broken factor.
  if (lflags) {
    int* const fl = lf_mt > 0 ? lflags + (size_t)(2 * ti + 1) * lf_mt + (2 * ti + 1) : lflags + (size_t)ti * Mt + ti;
    if (tid == 0) sh_ok = __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    __syncthreads();
    const int go = sh_ok;
    __syncthreads();
    if (!go || !wg_wait_flag(fl, abort_word, info, &sh_ok)) return false;
  }
  if (batch_of) {   // batched launch: the factors of several matrices (restart rows) are inverted by one launch
    const int b = batch_of[tix];
    A += (size_t)b * a_stride;
    dinv += (size_t)b * d_stride;
    W += (size_t)b * w_stride;
    flags += (size_t)b * f_stride;
    info += b;
  }
  const size_t r0 = 128 * (size_t)tj, ci = 128 * (size_t)ti;
  int* const frow = flags + (size_t)tj * Mt;

  d4 acc[4][4];
  double* Cw = W + r0 + wm * 64 + 2 * l15 + (ci + wn * 64 + 2 * l4) * (size_t)ldw;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double2 v = *reinterpret_cast<const double2*>(Cw + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ldw);
        acc[ni][2 * g][r] = v.x;
        acc[ni][2 * g + 1][r] = v.y;
      }
  direct_tile_negate(acc);                                   // the loop adds the products to -W_ji (direct_tile_gemm_acc); sign restored below
  const unsigned lane_off_w = (unsigned)(2 * l15 + l4 * ldw) * 8u, lane_off_l = (unsigned)(2 * l15 + l4 * ld) * 8u;
  int kdone = tj;
  while (kdone < ti) {
    if (w == 0) {                                           // wave 0 scans the flag row, 64 tile columns per pass
      int* const frows[1] = {frow};
      int kr;
      const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        kr = wave_scan_flags<1>(frows, kdone, ti);
        if (kr > kdone) break;
        if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS ||
            __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          if (lane == 0) {
            __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicMax(info, GPG_INFO_INTERNAL);
          }
          kr = -1;
          break;
        }
        __builtin_amdgcn_s_sleep(8);
      }
      if (lane == 0) sh_kr = kr;
    }
    __syncthreads();
    const int kr = __builtin_amdgcn_readfirstlane(sh_kr);
    if (kr < 0) return false;
    GPG_ACQUIRE();
    const size_t ck = 128 * (size_t)kdone;
    direct_tile_gemm_acc<GPG_MFMA_PF>(acc, W + r0 + wm * 64 + ck * (size_t)ldw, lane_off_w, ldw,
                            A + ci + wn * 64 + ck * (size_t)ld, lane_off_l, ld, 32 * (kr - kdone));
    __syncthreads();   // sh_kr may be rewritten
    kdone = kr;
  }
  direct_tile_negate(acc);
  // (r03) the factorisation's one-piece finalisation: column block 0 handed over through LDS, column block 1 through memory; the diagonal
  // tile of L is final, so there is nothing to wait for
  {
    double* Cs = Cw;                                          // (store addresses formed here, see tile128_chol_task)
    asm volatile("" : "+v"(Cs));
    int l15s = l15, l4s = l4;
    asm volatile("" : "+v"(l15s), "+v"(l4s));
    if (wn == 0) fin128_handoff_block0<2>(acc, wm, l15s, l4s);
    else {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double2 v;
            v.x = acc[ni][2 * g][r];
            v.y = acc[ni][2 * g + 1][r];
            *reinterpret_cast<double2*>(Cs + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ldw) = v;
          }
    }
  }
  __syncthreads();
  GPG_PRIO(2);
#ifdef GPG_STAMP
  if (tid == 0) t128_fo = nullptr;
#endif
  fin128_onepiece<2>(W + r0 + ci * (size_t)ldw, ldw, A + ci + ci * (size_t)ld, ld, dinv + ci);
  GPG_PUBLISH_AND_NEXT(ticket, frow + ti)
  return true;
}

struct TrinvArgs {
  const double* A; int ld; const double* dinv; double* W; int ldw, Mt; const int* tasks; int ntask; int* flags;
  int* ones;   // nine words set to 1 behind the flags (launch_tile128_inverse_batch); the kernel does not read them
  int* abort_word; int* ticket; int* info; const int* batch_of; size_t a_stride, w_stride; int d_stride, f_stride;
  int* lflags; int lf_mt;   // non-null: the (64-tile, lf_mt tile columns) factorisation of this ONE matrix may still be running
};

__global__ void __launch_bounds__(256, 2) tile128_trinv_kernel(TrinvArgs) {
  int tix;
  {
    GPG_KERNARGS(TrinvArgs, ap);
    tix = next_ticket(ap->ticket, &g_next_ticket);
  }
  for (;;) {
    GPG_KERNARGS(TrinvArgs, ap);
    if (tix >= ap->ntask) return;
    if (!tile128_trinv_task(tix, ap->A, ap->ld, ap->dinv, ap->W, ap->ldw, ap->Mt, ap->tasks, ap->flags, ap->abort_word,
                            ap->ticket, ap->info, ap->batch_of, ap->a_stride, ap->w_stride, ap->d_stride, ap->f_stride, ap->lflags, ap->lf_mt))
      return;
    tix = __builtin_amdgcn_readfirstlane(g_next_ticket);
  }
}

// Frontier of a contraction over tile columns k of W that may still be in the making (W = L^-T running on the other stream): thread 0
// advances kr from kdone while BOTH flag rows show column kr finished, waits (bounded) until at least one column is; result through sh.
// Returns the new frontier, or -1 (timed out / aborted).  Whole workgroup; ends with an acquire.
__device__ __forceinline__ int wg_wait_two_rows(int* fa, int* fb, int kdone, int kend, int* abort_word, int* info, int* sh) {
  if (threadIdx.x == 0) {
    int kr = kdone;
    const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
    for (;;) {
      while (kr < kend && __hip_atomic_load(fa + kr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 &&
             __hip_atomic_load(fb + kr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
        ++kr;
      if (kr > kdone) break;
      if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicMax(info, GPG_INFO_INTERNAL);
        kr = -1;
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    *sh = kr;
  }
  __syncthreads();
  const int kr = *sh;
  __syncthreads();
  if (kr >= 0) GPG_ACQUIRE();
  return kr;
}

// ------------------------------------------------------------------------------------------------
// tile128_wwt_kernel: M = - W W^T, lower triangle (second N^3/3 sweep of the explicit inverse: -(L L^T)^-1 = -L^-T L^-1),
// W = L^-T upper triangular: tile (a, b), a >= b:  M_ab = - sum_{k >= a} W_ak W_bk^T -- independent tiles, no flags;
// persistent workgroups take them from the ticket counter, longest contraction (smallest a) first.  The same
// direct-fragment MFMA loop, accumulators start at zero.
// ------------------------------------------------------------------------------------------------
// Generalised for the Frobenius-norm condition number (gpg_cond_fro): M = - Sa Sb^T with two different full (symmetric) operands
// and the contraction over ALL tile columns when full_k != 0 (Sb0 == nullptr: Sb = Sa, the W W^T case).
__global__ void __launch_bounds__(256, 2)
tile128_wwt_kernel(const double* __restrict__ W0, int ldw, double* __restrict__ M0, int ldm, int Mt, const int* __restrict__ tasks,
                   int ntask, int* ticket, const int* __restrict__ batch_of, size_t w_stride, const double* __restrict__ Sb0, int full_k,
                   int* wflags /* non-null (one matrix, W W^T): tile flags [row * Mt + column] of a W still in the making */, int* abort_word,
                   int* info) {
  __shared__ int sh_tix;
  __shared__ int sh_kr;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w & 1, wn = w >> 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  for (;;) {
    const int tix = next_ticket(ticket, &sh_tix);
    if (tix >= ntask) return;
    const int task = tasks[tix];
    const int ta = task & 0xffff, tb = task >> 16;        // a >= b
    const size_t boff = batch_of ? (size_t)batch_of[tix] * w_stride : 0;
    const double* W = W0 + boff;
    const double* Wb = Sb0 ? Sb0 + boff : W;
    double* M = M0 + boff;
    const size_t r0 = 128 * (size_t)ta, c0 = 128 * (size_t)tb, ck = full_k ? 0 : 128 * (size_t)ta;
    d4 acc[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ni][mi][r] = 0.0;
    const unsigned lane_off = (unsigned)(2 * l15 + l4 * ldw) * 8u;
    if (!wflags) {
      direct_tile_gemm_acc<GPG_MFMA_PF>(acc, W + r0 + wm * 64 + ck * (size_t)ldw, lane_off, ldw,
                              Wb + c0 + wn * 64 + ck * (size_t)ldw, lane_off, ldw, 32 * (full_k ? Mt : Mt - ta));
    } else {   // the same sum in the same order, in runs of the tile columns of W that are finished
      int kdone = ta;
      while (kdone < Mt) {
        const int kr = wg_wait_two_rows(wflags + (size_t)ta * Mt, wflags + (size_t)tb * Mt, kdone, Mt, abort_word, info, &sh_kr);
        if (kr < 0) return;
        const size_t cc = 128 * (size_t)kdone;
        direct_tile_gemm_acc<GPG_MFMA_PF>(acc, W + r0 + wm * 64 + cc * (size_t)ldw, lane_off, ldw,
                                W + c0 + wn * 64 + cc * (size_t)ldw, lane_off, ldw, 32 * (kr - kdone));
        kdone = kr;
      }
    }
    direct_tile_negate(acc);                               // M = - Sa Sb^T: the loop accumulated + Sa Sb^T
    double* Cw = M + r0 + wm * 64 + 2 * l15 + (c0 + wn * 64 + 2 * l4) * (size_t)ldm;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double2 v;
          v.x = acc[ni][2 * g][r];
          v.y = acc[ni][2 * g + 1][r];
          *reinterpret_cast<double2*>(Cw + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ldm) = v;
        }
  }
}

// The same product on 64 x 64 tiles (wave_tile_gemm, the MFMA loop of tile_chol_kernel): for ONE small matrix the 128-tile list has fewer
// tasks than the device has workgroup slots (210 at 2560 columns) and its longest contraction is the whole launch; four times as many
// tiles of a quarter of the work fill the slots and halve the longest task.  tasks[t] = a | b << 16, a >= b, longest first.
__global__ void __launch_bounds__(256, 2)
tile64_wwt_kernel(const double* __restrict__ W, int ldw, double* __restrict__ M, int ldm, int Mt, const int* __restrict__ tasks, int ntask,
                  int* ticket, int* wflags /* non-null: tile flags [row * Mt + column] of a W still in the making */, int* abort_word, int* info) {
  constexpr int KB = 16, SA = 80, BUF = KB * SA;
  __shared__ __attribute__((aligned(16))) double U[4 * BUF];
  __shared__ int sh_tix;
  __shared__ int sh_kr;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4, sp = tid & 31, sk = tid >> 5;
  for (;;) {
    const int tix = next_ticket(ticket, &sh_tix);
    if (tix >= ntask) return;
    const int task = tasks[tix];
    const int ta = task & 0xffff, tb = task >> 16;        // a >= b
    const size_t r0 = 64 * (size_t)ta, c0 = 64 * (size_t)tb, ck = 64 * (size_t)ta;   // W is upper triangular: columns >= 64 a
    d4 acc[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[ni][r] = 0.0;
    if (!wflags) {
      wave_tile_gemm(acc, W + r0 + 2 * sp + (ck + sk) * (size_t)ldw, ldw, W + c0 + 2 * sp + (ck + sk) * (size_t)ldw, ldw, 4 * (Mt - ta), U,
                     U + 2 * BUF, w, l15, l4, sp, sk);
    } else {   // the same sum in the same order, in runs of the tile columns of W that are finished
      int kdone = ta;
      while (kdone < Mt) {
        const int kr = wg_wait_two_rows(wflags + (size_t)ta * Mt, wflags + (size_t)tb * Mt, kdone, Mt, abort_word, info, &sh_kr);
        if (kr < 0) return;
        const size_t cc = 64 * (size_t)kdone;
        wave_tile_gemm(acc, W + r0 + 2 * sp + (cc + sk) * (size_t)ldw, ldw, W + c0 + 2 * sp + (cc + sk) * (size_t)ldw, ldw, 4 * (kr - kdone), U,
                       U + 2 * BUF, w, l15, l4, sp, sk);
        __syncthreads();                                  // staging buffers free for the next run
        kdone = kr;
      }
    }
    double* Cw = M + r0 + 16 * w + l15 + (c0 + l4) * (size_t)ldm;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) Cw[(size_t)(ni * 16 + 4 * r) * ldm] = acc[ni][r];
    __syncthreads();                                      // staging buffers and sh_tix free for the next round
  }
}
// ------------------------------------------------------------------------------------------------
// tile64_trinv_kernel: W = L^-T with 64 x 64 tiles, for small matrices (the 128-tile version's dependency chain -- one
// 128-row substitution per tile column -- is what a 2560-column inverse spends its time on).  Task (rt, tj), rt <= tj (row
// tile rt, column tile tj of the upper triangular W, which starts as the identity; list order: tile column by tile
// column): acc = W_(rt,tj) - sum_{k=rt}^{tj-1} W_(rt,k) L_(tj,k)^T on MFMA as the tiles of W's row rt are published, then the
// quad-row substitution against L_(tj,tj): the body of rows_fwd_kernel restricted to the non-zero tiles, batched.
// ------------------------------------------------------------------------------------------------
struct Trinv64Args {
  const double* A; int ld; const double* dinv; double* W; int ldw, Mt; const int* tasks; int ntask; int* flags; int* abort_word;
  int* ticket; int* info; const int* batch_of; size_t a_stride, w_stride; int d_stride, f_stride;
  int* lflags;   // non-null: the factorisation may still be running; its tile flags [ti * Mt + tj] (64 x 64 tiles; matrix b at + b lf_stride)
  int lf_stride;
};

__device__ __forceinline__ bool
tile64_trinv_task(int tix, const double* __restrict__ A, int ld, const double* __restrict__ dinv, double* W, int ldw, int Mt,
                  const int* __restrict__ tasks, int* flags, int* abort_word, int* ticket, int* info,
                  const int* __restrict__ batch_of, size_t a_stride, size_t w_stride, int d_stride, int f_stride, int* lflags, int lf_stride) {
  constexpr int KB = 16, SA = 80, BUF = KB * SA;
  __shared__ __attribute__((aligned(16))) double U[4 * BUF];
  __shared__ __attribute__((aligned(16))) double Ls[64][4][18];
  __shared__ double sdinv[64];
  __shared__ int sh_kr;
  double* const sA = U;
  double* const sB = U + 2 * BUF;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int task = tasks[tix];
  const int rt = task & 0xffff, tj = task >> 16;
  if (batch_of) {
    const int b = batch_of[tix];
    A += (size_t)b * a_stride;
    dinv += (size_t)b * d_stride;
    W += (size_t)b * w_stride;
    flags += (size_t)b * f_stride;
    info += b;
    if (lflags) lflags += (size_t)b * lf_stride;
  }
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
  // Overlapped with the factorisation (lflags): column tile tj of W needs row tile tj of L, L_(tj,k) for k <= tj -- all of it is final once
  // the diagonal tile (tj, tj) is (its task consumed the others), so ONE wait on that flag covers the whole task.
  if (lflags && !wg_wait_flag(lflags + (size_t)tj * Mt + tj, abort_word, info, &sh_kr)) return false;
  {   // L_jj is final: its image is fetched before the first wait
    const double* Ljj = A + cj + cj * (size_t)ld;
    for (int t = tid; t < 64 * 64; t += 256) {
      const int jj = t >> 6, k = t & 63;
      Ls[jj][k & 3][k >> 2] = Ljj[k + (size_t)jj * ld];
    }
    if (tid < 64) sdinv[tid] = dinv[cj + tid];
  }
  int kdone = rt;
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
  GPG_PRIO(2);
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
  GPG_QUAD_SUBST(x, Ls, sdinv, q)
  double* Xr = W + r0 + (tid >> 2) + (cj + q) * (size_t)ldw;
#pragma unroll
  for (int m = 0; m < 16; ++m) GPG_ST(&Xr[(size_t)(4 * m) * ldw], x[m]);
  GPG_PUBLISH_AND_NEXT(ticket, frow + tj)
  return true;
}

__global__ void __launch_bounds__(256, 2) tile64_trinv_kernel(Trinv64Args) {
  int tix;
  {
    GPG_KERNARGS(Trinv64Args, ap);
    tix = next_ticket(ap->ticket, &g_next_ticket);
  }
  for (;;) {
    GPG_KERNARGS(Trinv64Args, ap);
    if (tix >= ap->ntask) return;
    if (!tile64_trinv_task(tix, ap->A, ap->ld, ap->dinv, ap->W, ap->ldw, ap->Mt, ap->tasks, ap->flags, ap->abort_word, ap->ticket,
                           ap->info, ap->batch_of, ap->a_stride, ap->w_stride, ap->d_stride, ap->f_stride, ap->lflags, ap->lf_stride))
      return;
    tix = __builtin_amdgcn_readfirstlane(g_next_ticket);
  }
}

}  // namespace
