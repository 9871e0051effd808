// Dataflow Cholesky on 64 x 64 tiles: tile_chol_kernel (small matrices, trailing blocks).
#pragma once
#include "dataflow_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// tile_chol_kernel: dataflow (left-looking) Cholesky of the trailing block A[c0:, c0:] in 64 x 64 tiles,
// ONE launch.  Used where the blocked algorithm is latency-bound: the last few thousand columns of a large
// matrix and small matrices as a whole.  Workgroup b owns tile (i, j) = tasks[b] (column-major task order,
// rows i >= j; the right-hand-side rows below the matrix are ordinary tile rows):
//     acc  = A_ij - sum_{k<j} L_ik L_jk^T      MFMA, k-blocks consumed as soon as their flags are up
//     i==j : L_jj = chol(acc) by wave 0 (potrf64_wave), reciprocal pivots to dinv
//     i> j : L_ij = acc L_jj^-T by the quad-row substitution, once flag(j, j) is up
//     publish: __threadfence, then flag(i, j) = 1 (agent-scope release)
// Scheduling: PERSISTENT workgroups.  The launch has at most as many workgroups as the device holds at once; each
// takes its next task from an atomic ticket counter, in list order, until the list is exhausted.  A task only ever
// waits for tasks with a smaller ticket.  Progress: let T be the smallest unfinished ticket.  If T has been taken,
// its workgroup is resident (it took the ticket while running) and everything T waits for has a smaller ticket, i.e.
// is finished -- T completes.  If T has not been taken, every resident workgroup holds a smaller ticket, all of those
// are finished, so one of them asks for its next ticket and gets T.  Nothing here depends on the order in which the
// hardware dispatches workgroups, on how many of them are resident, or on having the device alone: another process's
// launch on the same GPU can only delay this one, never block it.  Every wait still is bounded in time as a backstop:
// on timeout the kernel raises the abort word, all workgroups drain, and the host falls back on the blocked schedule.
// The serial chain per 64 columns is potrf -> substitution -> one 64-deep MFMA block (~20 us) instead of three
// dependent launches per step plus B_p and U_p.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool
tile_chol_task(int tix, double* A, int ld, int c0, int Mt, const int* __restrict__ tasks, int* flags, int* pieces, int* abort_word,
               int* ticket, double* __restrict__ dinv, int* __restrict__ info, int N, const int* __restrict__ batch_of, size_t a_stride,
               int d_stride, int f_stride, int fuse) {
  constexpr int KB = 16, SA = 80, BUF = KB * SA;
  __shared__ __attribute__((aligned(16))) double U[4 * BUF];      // staging sA[2] | sB[2]; later the tile Ts[64][SA]
  __shared__ __attribute__((aligned(16))) double Ls[64][4][18];   // L_jj image (i > j) / potrf scratch St[64][64] (i == j)
  __shared__ double sdinv[64];
  __shared__ int sh_kr;
  double* const sA = U;
  double* const sB = U + 2 * BUF;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int task = tasks[tix];
  const int ti = task & 0xffff, tj = task >> 16;
  if (batch_of) {   // batched launch: several independent matrices (restart rows) share the grid
    const int b = batch_of[tix];
    A += (size_t)b * a_stride;
    dinv += (size_t)b * d_stride;
    info += b;
    flags += (size_t)b * f_stride;
    pieces += (size_t)b * f_stride;
  }
  const size_t r0 = (size_t)c0 + 64 * (size_t)ti;        // first matrix row of the tile
  const size_t cj = (size_t)c0 + 64 * (size_t)tj;        // first matrix column of the tile
  const int q = tid & 3;
  const int sp = tid & 31, sk = tid >> 5;
  // Fused diagonal task (fuse != 0, tj > 0): this workgroup ALSO owns the sub-diagonal tile (tj, tj-1) -- the task list has no task of
  // its own for it.  It carries that tile's accumulators (acc1) next to its own, substitutes them against the pieces of the previous
  // diagonal tile as they are published, and applies the result to its own accumulators from LDS: the chain diagonal tile -> tile
  // (j+1, j) -> store / flag / poll / reload -> diagonal tile (j+1, j+1) loses its two trips through memory (~20.7 -> ~17 us per column).
  const bool fused = fuse != 0 && ti == tj && tj > 0;
  const int kend = fused ? tj - 1 : tj;                  // tile columns the MFMA loop covers (the fused task's last one comes from LDS)
  const size_t cjm = cj - 64;                            // first matrix column of tile column tj - 1 (fused only)
  int* const frow_i = flags + (size_t)ti * Mt;           // flags of tile row i
  int* const frow_j = flags + (size_t)(fused ? tj - 1 : tj) * Mt;

  // accumulators start as A_ij
  d4 acc[4];
  {
    const double* Cw = A + r0 + 16 * w + l15 + (cj + l4) * (size_t)ld;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[ni][r] = Cw[(size_t)(ni * 16 + 4 * r) * ld];
  }
  d4 acc1[4];                                            // fused: A(tj, tj-1), nobody else writes that tile
  if (fused) {
    const double* Cw = A + r0 + 16 * w + l15 + (cjm + l4) * (size_t)ld;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc1[ni][r] = Cw[(size_t)(ni * 16 + 4 * r) * ld];
  }

  // ---- (1) left-looking accumulation over the finished tile columns ------------------------------------------
#ifdef GPG_STAMP
  const unsigned long long tk_start = __builtin_amdgcn_s_memrealtime();
  unsigned long long tk_spin = 0, tk_gemm = 0, tk_runs = 0;
#endif
  GPG_PRIO_ACC(ti - tj)
  __shared__ int sh_kr1;
  int kdone = 0, kd1 = 0;                                // tile columns applied to acc / to the fused task's acc1
  while (kdone < kend || (fused && kd1 < kend)) {
    GPG_TR(q0)
    if (tid == 0) {
      int kr = kdone, kr1 = kd1;
      const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        if (fused) {   // own accumulators: tile row tj only; acc1: tile rows tj and tj - 1 -- the two frontiers advance independently
          while (kr < kend && __hip_atomic_load(frow_i + kr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ++kr;
          while (kr1 < kr && __hip_atomic_load(frow_j + kr1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ++kr1;
          if (kr > kdone || kr1 > kd1) break;
        } else {
          while (kr < kend && __hip_atomic_load(frow_i + kr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 &&
                 __hip_atomic_load(frow_j + kr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
            ++kr;
          if (kr > kdone) break;
        }
        if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          atomicMax(info, GPG_INFO_INTERNAL);
          kr = -1;
          break;
        }
        __builtin_amdgcn_s_sleep(4);
      }
      sh_kr = kr;
      sh_kr1 = kr1;
    }
    __syncthreads();
    const int kr = sh_kr, kr1 = sh_kr1;
    if (kr < 0) return false;                            // abort: drain
    GPG_ACQUIRE();   // the producers' tiles are visible from here on
    GPG_TR(q1)
    if (kr > kdone) {
      const size_t ck = (size_t)c0 + 64 * (size_t)kdone;
      wave_tile_gemm(acc, A + r0 + 2 * sp + (ck + sk) * (size_t)ld, ld, A + cj + 2 * sp + (ck + sk) * (size_t)ld, ld,
                     4 * (kr - kdone), sA, sB, w, l15, l4, sp, sk);
    }
    __syncthreads();                                     // staging buffers free again; sh_kr may be rewritten
    if (fused && kr1 > kd1) {                            // the sub-diagonal tile's share: rows tj against rows tj - 1
      const size_t ck = (size_t)c0 + 64 * (size_t)kd1;
      wave_tile_gemm(acc1, A + r0 + 2 * sp + (ck + sk) * (size_t)ld, ld, A + cjm + 2 * sp + (ck + sk) * (size_t)ld, ld,
                     4 * (kr1 - kd1), sA, sB, w, l15, l4, sp, sk);
      __syncthreads();
    }
    GPG_TR(q2)
#ifdef GPG_STAMP
    tk_spin += q1 - q0; tk_gemm += q2 - q1; ++tk_runs;
#endif
    kdone = kr;
    kd1 = kr1;
  }
#ifdef GPG_STAMP
  const unsigned long long tk_fin0 = __builtin_amdgcn_s_memrealtime();
#endif

  GPG_PRIO_FIN(ti - tj)
  // one 16-column piece of the diagonal tile of tile column PC (matrix column PCJ): wait, image, quad-row substitution of x
#define GPG_TC_PIECE(S, PC, PCJ)                                                             \
    {                                                                                       \
      if (!wg_wait_flag(pieces + 4 * (PC) + (S), abort_word, info, &sh_kr)) return false;    \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                        \
        const int t = tid + 256 * u, jj = 16 * (S) + (t >> 6), k = t & 63;                   \
        Ls[jj][k & 3][k >> 2] = (A + (PCJ) + (PCJ) * (size_t)ld)[k + (size_t)jj * ld];       \
      }                                                                                     \
      if (tid < 16) sdinv[16 * (S) + tid] = dinv[(PCJ) + 16 * (S) + tid];                    \
      __syncthreads();                                                                      \
      GPG_QUAD_SUBST_PIECE(x, Ls, sdinv, q, S)                                               \
      /* pin x: otherwise the FMAs of a piece are deferred into the next ones and everything spills */ \
      _Pragma("unroll") for (int m = 0; m < 16; ++m) asm volatile("" : "+v"(x[m]));              \
    }
  if (fused) {
    // ---- (1') the sub-diagonal tile: acc1 -> LDS -> quad rows, substitution against L(tj-1, tj-1) piece by piece, then out to memory
    //      (asynchronously) and, through the LDS tile, into this task's own accumulators: acc -= X X^T ------------------------------
    {
      double* Ts = U;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = acc1[ni][r];
    }
    __syncthreads();
    double x[16];
    {
      const double* Tr = U + q * SA + (tid >> 2);
#pragma unroll
      for (int m = 0; m < 16; ++m) x[m] = Tr[(4 * m) * SA];
    }
    GPG_TC_PIECE(0, tj - 1, cjm)
    GPG_TR(tq_p0)
    GPG_TC_PIECE(1, tj - 1, cjm)
    GPG_TC_PIECE(2, tj - 1, cjm)
    GPG_TR(tq_p2)
#ifdef GPG_STAMP
    if (!wg_wait_flag(pieces + 4 * (tj - 1) + 3, abort_word, info, &sh_kr)) return false;   // (diagnostic: when piece 3 is SEEN; the wait inside the piece macro then falls through)
#endif
    GPG_TR(tq_seen3)
    GPG_TC_PIECE(3, tj - 1, cjm)
    GPG_TR(tq_sub3)
    {
      double* Xr = A + r0 + (tid >> 2) + (cjm + q) * (size_t)ld;
      double* Tw = U + q * SA + (tid >> 2);
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        GPG_ST(&Xr[(size_t)(4 * m) * ld], x[m]);
        Tw[(4 * m) * SA] = x[m];                          // every thread rewrites exactly the entries it read: no barrier needed before
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 64; kk += 4) {
      const double fm = -U[(kk + l4) * SA + 16 * w + l15];
      double fn[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) fn[ni] = U[(kk + l4) * SA + ni * 16 + l15];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn[ni], fm, acc[ni], 0, 0, 0);
    }
    GPG_RELEASE();                                        // the stores of X have had the whole update to complete
    __syncthreads();                                      // ... and the LDS tile is free again
    if (tid == 0) GPG_FLAG_UP(frow_i + (tj - 1));          // tile (tj, tj-1) is final for everybody else
    GPG_TR(tq_upd)
#ifdef GPG_STAMP   // tools/timeline_chain64.py: the chain of the fused diagonal tasks, split at these stamps
    if (tid == 0 && g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) {
      unsigned long long* pz = g_stamp_buf + (size_t)GPG_STAMP_MAX * 16 + (size_t)tix * 16;
      pz[0] = tq_p0; pz[1] = tq_p2; pz[2] = tq_seen3; pz[3] = tq_sub3; pz[4] = tq_upd;
    }
#endif
  }
  // ---- (2) accumulators -> LDS tile Ts[col][row] --------------------------------------------------------------
  {
    double* Ts = U;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ts[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = acc[ni][r];
  }
  if (ti == tj) {
    __syncthreads();
    {   // diagonal tile: factor it (pivots on wave 0, the MFMA updates on all four; entries above the diagonal are garbage nobody reads)
      double* blk = A + r0 + cj * (size_t)ld;
#ifdef GPG_STAMP
      if (tid == 0 && g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) (g_stamp_buf + (size_t)GPG_STAMP_MAX * 16 + (size_t)tix * 16)[5] = __builtin_amdgcn_s_memrealtime();
#endif
      const int bad = potrf64_wg(U, SA, reinterpret_cast<double(*)[64]>(&Ls[0][0][0]), blk, ld, dinv + cj, pieces + 4 * tj);
#ifdef GPG_STAMP
      if (tid == 0 && g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) (g_stamp_buf + (size_t)GPG_STAMP_MAX * 16 + (size_t)tix * 16)[6] = __builtin_amdgcn_s_memrealtime();
#endif
      if (w == 0 && bad && lane == 0 && (int)cj + bad - 1 < N) atomicCAS(info, 0, (int)cj + bad);
    }
  } else {
    // substitute against the diagonal tile of this column piece by piece, as its 16-column pieces are published
    __syncthreads();
    double x[16];
    {
      const double* Tr = U + q * SA + (tid >> 2);
#pragma unroll
      for (int m = 0; m < 16; ++m) x[m] = Tr[(4 * m) * SA];
    }
    GPG_TC_PIECE(0, tj, cj)
    GPG_TC_PIECE(1, tj, cj)
    GPG_TC_PIECE(2, tj, cj)
    GPG_TC_PIECE(3, tj, cj)
#undef GPG_TC_PIECE
    double* Xr = A + r0 + (tid >> 2) + (cj + q) * (size_t)ld;
#pragma unroll
    for (int m = 0; m < 16; ++m) GPG_ST(&Xr[(size_t)(4 * m) * ld], x[m]);
  }
  // ---- (3) publish (and fetch the next ticket) --------------------------------------------------------------------
#ifdef GPG_STAMP
  const unsigned long long tk_pub0 = __builtin_amdgcn_s_memrealtime();
#endif
  GPG_PUBLISH_AND_NEXT(ticket, frow_i + tj)
#ifdef GPG_STAMP
  if (tid == 0 && g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) {
    unsigned long long* o = g_stamp_buf + (size_t)tix * 8;
    o[0] = tk_start; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = tk_spin; o[3] = tk_gemm; o[4] = tk_runs;
    o[5] = tk_fin0; o[6] = (unsigned long long)task; o[7] = (unsigned long long)blockIdx.x;
    unsigned long long* fo = g_stamp_buf + (size_t)GPG_STAMP_MAX * 8 + (size_t)tix * 8;
    fo[0] = tk_fin0; fo[1] = tk_pub0; fo[2] = fo[3] = fo[4] = fo[5] = fo[6] = fo[7] = 0;
  }
#endif
  return true;
}

__device__ __noinline__ int tile_chol_task_call(int tix_v, unsigned long long kernarg_bits) {
  GPG_KERNARGS_FROM(TileCholArgs, ap, kernarg_bits);
  const int tix = __builtin_amdgcn_readfirstlane(tix_v);
  return tile_chol_task(tix, ap->A, ap->ld, ap->c0, ap->Mt, ap->tasks, ap->flags, ap->pieces, ap->abort_word, ap->ticket, ap->dinv,
                        ap->info, ap->N, ap->batch_of, ap->a_stride, ap->d_stride, ap->f_stride, ap->fuse) ? 1 : 0;
}

__global__ void __launch_bounds__(256, 2) tile_chol_kernel(TileCholArgs) {
  int tix;
  {
    GPG_KERNARGS(TileCholArgs, ap);
    tix = next_ticket(ap->ticket, &g_next_ticket);       // the first ticket; every later one comes with a task's publish step
  }
  for (;;) {
    GPG_KERNARGS(TileCholArgs, ap);
    if (tix >= ap->ntask) return;
    if (!__builtin_amdgcn_readfirstlane(tile_chol_task_call(tix, (unsigned long long)ap))) return;   // aborted: every workgroup drains
    tix = __builtin_amdgcn_readfirstlane(g_next_ticket);                                    // written before the barrier of the publish step
  }
}

}  // namespace
