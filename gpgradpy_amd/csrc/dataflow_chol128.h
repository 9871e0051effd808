// Dataflow Cholesky on 128 x 128 tiles: tile128_chol_kernel, pair128_chol_kernel (two tiles per workgroup) and the fin128_*
// finalisation they share.
#pragma once
#include "dataflow_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// tile128_chol_kernel: the whole factorisation as ONE dataflow launch over 128 x 128 tiles (left-looking).
// Workgroup b owns tile (i, j) = tasks[b], column-major task order, rows i >= j (the right-hand-side rows
// below the matrix are one more tile row):
//     acc  = A_ij - sum_{k<j} L_ik L_jk^T   a direct-fragment MFMA loop (operands straight from global) over every finished tile
//                                          column, consumed in runs as the flags come up.  The C tile is read
//                                          once and written once per factorisation (the right-looking update
//                                          streams it once per panel) and there is no launch chain at all.
//     i==j : potrf of the 128 x 128 tile inside the workgroup (potrf64, 64-row substitution, 64 x 64 MFMA
//            update, potrf64)
//     i> j : L_ij = acc L_jj^-T, two 64-row passes of panel_solve_rows64 against the 128-wide diagonal tile
//     publish: __threadfence, flag(i, j) = 1 (agent-scope release)
// Persistent workgroups, ticket order, progress argument and bounded waits as in tile_chol_kernel.
// ------------------------------------------------------------------------------------------------
// The diagonal tile publishes its pieces as they are final -- L11 in four 16-column pieces (pa[0..3], while its first
// potrf64 is still running), L21 (flag_c, after its 64-row solve), L22 in four pieces (pb[0..3]): every column block of
// this tile is substituted piece by piece, and the MFMA update of block 1 runs while the diagonal tile is still in its
// second potrf64.
#ifdef GPG_STAMP
__shared__ unsigned long long* t128_fo;      // finalisation record of the running task (thread 0 writes and reads it)
__shared__ unsigned long long t128_wait_acc; // ticks thread 0 spent polling piece flags in this task's finalisation (wg_wait_flag2)
// piece-level record (third region of the stamp buffer, 16 words per task): per piece S of column block 0 -- after the flag wait,
// after the image is in LDS (barrier), after the 16 column steps
#define GPG_FS3(k) if (threadIdx.x == 0 && t128_fo) (g_stamp_buf + (size_t)GPG_STAMP_MAX * 16 + 2 * (t128_fo - (g_stamp_buf + (size_t)GPG_STAMP_MAX * 8)))[k] = __builtin_amdgcn_s_memrealtime();
#else
#define GPG_FS3(k)
#endif

// Finalisation of a 128 x 128 tile that already sits updated in memory (kept out of line so that its register
// needs do not leak into the MFMA loop of the kernel).  Returns 0 if the wait for the diagonal tile timed out.
__shared__ __attribute__((aligned(16))) double t128_U[4 * 16 * 80];   // staging / transposition tile of the finalisation
__shared__ __attribute__((aligned(16))) double t128_Ls[64][4][18];    // diagonal-block image / potrf scratch
__shared__ double t128_sdinv[64];
__shared__ int t128_sh_ok;
__shared__ int t128_sh2[2];           // verdict on the NEXT 16-column piece (fin128_offdiag; two words used alternately: a barrier lies between two uses of one)

// LDS of pair128_chol_kernel (512 threads = two teams; defined here because fin128_offdiag serves both 128-tile kernels)
__shared__ __attribute__((aligned(16))) double p128_U[2][4 * 16 * 80];    // per team: staging / transposition tile of the finalisation
__shared__ __attribute__((aligned(16))) double p128_Ls[2][64][4][18];     // per team: diagonal-block image / potrf scratch
__shared__ double p128_sdinv[2][64];
__shared__ int p128_sh2[2];
__shared__ int p128_sh_ok;            // result of the joint flag waits: ONE word for both teams (a function-local __shared__ would be one per template instance)

// Both flags up?  Thread 0 of the workgroup polls; 0 = timed out / aborted (both matrices are marked).
__device__ __forceinline__ int wg_wait_flag2(int* fa, int* fb, int* abort_word, int* info_a, int* info_b, int* sh) {
  if (threadIdx.x == 0) {
    int ok = 1;
    const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(fa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 ||
           __hip_atomic_load(fb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicMax(info_a, GPG_INFO_INTERNAL);
        atomicMax(info_b, GPG_INFO_INTERNAL);
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    *sh = ok;
#ifdef GPG_STAMP
    t128_wait_acc += __builtin_amdgcn_s_memrealtime() - t_wait;
#endif
  }
  __syncthreads();
  const int ok = *sh;
  __syncthreads();
  if (ok) GPG_ACQUIRE();
  return ok;
}

// ------------------------------------------------------------------------------------------------
// fin128_offdiag (round 3): finalisation X <- X L_jj^-T of an off-diagonal 128 x 128 tile of the factorisation, for both 128-tile
// kernels (SET 0 / 1: the two teams of pair128_chol_kernel, SET 2: tile128_chol_kernel; one instance each, because a team's LDS arrays
// must be addressed statically).  What the timeline of round 3 showed (tools/timeline_pieces.py, 64 matrices of 2560 columns): of
// ~100 us per task only ~40 are the 128 column steps; 34 us are the tile going to memory and coming back in the quad layout (store,
// s_waitcnt, barrier, 32 loads), 42 us are eight times (flag poll, two barriers, a dependent load of 16 columns of L_jj, a barrier).
//  * Column block 0 reaches this function THROUGH LDS: wave (wm, 0) of the team has written its 64 x 64 accumulator block as
//    [column][row] -- rows 0..63 into U (row stride 80), rows 64..127 into the region of the L image viewed as [64][72]
//    (fin128_handoff_block0) -- and every thread takes its two rows in the quad layout from there.  Column block 1 (waves (wm, 1))
//    went to memory as before and is read back for its MFMA update much later.
//  * When the diagonal tile is COMPLETE on entry (its tile flag; the rule in batched launches) there is one check instead of nine
//    waits: the image of L11 is loaded in one piece, the 64 column steps run without a barrier, the raw L22 is fetched into registers
//    while block 1 takes its update.  Otherwise the piecewise path of rounds 1 / 2 runs (16 columns at a time behind the diagonal
//    task's early flags).  Both paths do the same arithmetic in the same order.
// done0 / done1: tile flags of the diagonal tiles of the two teams' matrices (the same word twice for SET 2), every other flag
// argument likewise.  Returns 0 if a wait timed out.
// ------------------------------------------------------------------------------------------------
template <int SET> __device__ __forceinline__ double* fin128_U() { if constexpr (SET == 2) return t128_U; else return p128_U[SET]; }
template <int SET> __device__ __forceinline__ double (*fin128_Ls())[4][18] { if constexpr (SET == 2) return t128_Ls; else return p128_Ls[SET]; }
template <int SET> __device__ __forceinline__ double* fin128_sdinv() { if constexpr (SET == 2) return t128_sdinv; else return p128_sdinv[SET]; }
template <int SET> __device__ __forceinline__ int* fin128_sh() { if constexpr (SET == 2) return &t128_sh_ok; else return &p128_sh_ok; }
template <int SET> __device__ __forceinline__ int* fin128_sh2() { if constexpr (SET == 2) return t128_sh2; else return p128_sh2; }
// the caller's side of the LDS hand-over (inlined into the task: the accumulators are in its registers)
template <int SET>
__device__ __forceinline__ void fin128_handoff_block0(const d4 (&acc)[4][4], int wm, int l15, int l4) {
  double* const U = fin128_U<SET>();
  double* const L2 = &fin128_Ls<SET>()[0][0][0];
#define GPG_F128_HAND(dst, stride)                                                           \
  _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                                           \
    _Pragma("unroll") for (int g = 0; g < 2; ++g)                                            \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                        \
        double2 v;                                                                          \
        v.x = acc[ni][2 * g][r];                                                            \
        v.y = acc[ni][2 * g + 1][r];                                                        \
        *reinterpret_cast<double2*>((dst) + (32 * (ni >> 1) + 8 * r + 2 * l4 + (ni & 1)) * (stride) + 32 * g + 2 * l15) = v; \
      }
  if (wm == 0) { GPG_F128_HAND(U, 80) } else { GPG_F128_HAND(L2, 72) }
#undef GPG_F128_HAND
}
#ifdef GPG_STAMP
#define GPG_FS4(k) if (SET != 1 && threadIdx.x == 0 && t128_fo) t128_fo[k] = __builtin_amdgcn_s_memrealtime();
#else
#define GPG_FS4(k)
#endif
// fin128_onepiece: X <- X L^-T for a 128 x 128 tile whose column block 0 has been handed over in LDS (fin128_handoff_block0) and whose
// column block 1 sits in memory, against a COMPLETE diagonal tile L (reciprocal pivots dinv) -- the one-piece path of fin128_offdiag, also
// the finalisation of tile128_trinv_kernel (whose diagonal tiles are always complete).  The caller has synchronised the workgroup after
// the hand-over (and the stores of block 1); on return the stores of X are in flight: the caller's publish step waits for them.
// One-piece path (the diagonal tile was complete on entry).  Round 3, second half: the update of column block 1 no longer goes
// through memory.  Before: X1 stored, s_waitcnt vmcnt(0) + barrier (5.5 us of store acknowledgements), then wave_tile_gemm staging
// X1 and L21 from memory through LDS with three barriers per 16-deep chunk (14.8 us) -- for 128 MFMAs per wave.  Now L21 is brought
// in with L11 (one round trip) and parked k-major in the staging tile, the A operand -X1 comes straight out of the substitution's
// registers by a lane permutation (quad layout: lane 4 r + q holds row r, columns 4 m + q; MFMA layout: lane 16 k + r holds row r,
// column 4 s + k: source lane 4 l15 + l4, register m = s), the X1 store is left in flight until the task publishes, and the
// transposition back into the quad layout is wave-private (wave w owns rows 16 w .. 16 w + 15 in both layouts).  Two barriers
// instead of fourteen.  Same MFMA operands in the same order as GPG_F128_UPDATE (fn = L21 fragment, fm = -X1 fragment, accumulator
// preloaded with T2, k ascending): bit-identical with the piecewise path.
template <int SET>
__device__ __forceinline__ void fin128_onepiece(double* X, int ldx, const double* L, int ldl, const double* dinv) {
  constexpr int SA = 80, S2 = 72;
  double* const U = fin128_U<SET>();
  double (*const Ls)[4][18] = fin128_Ls<SET>();
  double* const sdinv = fin128_sdinv<SET>();
  int tid_raw = (int)threadIdx.x;
  asm volatile("" : "+v"(tid_raw));
  const int tid = SET == 2 ? tid_raw : (tid_raw & 255), lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int q = tid & 3, rr = tid >> 2;
  (void)l15; (void)l4;
  double x0[16], x1[16];
#define GPG_F128_TAKE_X()                                                                    \
  {                                                                                         \
    int tq = tid;                                                                           \
    asm volatile("" : "+v"(tq));                                                            \
    const double* T0 = U + (tq & 3) * SA + (tq >> 2);                                        \
    const double* T1 = &fin128_Ls<SET>()[0][0][0] + (tq & 3) * S2 + (tq >> 2);               \
    _Pragma("unroll") for (int m = 0; m < 16; ++m) {                                         \
      x0[m] = T0[(4 * m) * SA];                                                             \
      x1[m] = T1[(4 * m) * S2];                                                             \
    }                                                                                       \
  }
  GPG_ACQUIRE();
  GPG_F128_TAKE_X()
  double li[16], lj[16];                                     // raw 64 x 64 blocks of L, 16 entries per thread
#define GPG_F128_RAW(dst, LP)                                                                \
  _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                         \
    const int t = tid + 256 * i;                                                          \
    dst[i] = (LP)[(t & 63) + (size_t)(t >> 6) * ldl];                                      \
  }
#define GPG_F128_IMAGE(DOFF)                                                                 \
  _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                         \
    const int t = tid + 256 * i, jj = t >> 6, k = t & 63;                                  \
    Ls[jj][k & 3][k >> 2] = li[i];                                                        \
  }                                                                                       \
  if (tid < 64) sdinv[tid] = dinv[(DOFF) + tid];
  GPG_F128_RAW(li, L)
  GPG_F128_RAW(lj, L + 64)                                   // L21[n][k] = L[64 + n + k ldl]
  GPG_LDS_BARRIER();                                         // every thread has taken x0 / x1 out of the staging tile and the image region
  GPG_F128_IMAGE(0)
#pragma unroll
  for (int i = 0; i < 16; ++i) {                             // L21 k-major: U[k][n], row stride SA
    const int t = tid + 256 * i;
    U[(t >> 6) * SA + (t & 63)] = lj[i];
  }
  GPG_F128_RAW(li, L + 64 + (size_t)64 * ldl)                // L22: in flight through the column steps of block 0
  GPG_LDS_BARRIER();
  GPG_FS4(2)
  {
    double* const Xs = X + rr + (size_t)q * ldx;             // the finished columns of X1 leave behind the steps (no wait before the task publishes)
#define GPG_F128_HOOK(mj) GPG_ST(&Xs[(size_t)(4 * (mj)) * ldx], x0[mj]); GPG_ST(&Xs[64 + (size_t)(4 * (mj)) * ldx], x1[mj]);
    GPG_QUAD_SUBST2_HOOK(x0, x1, Ls, sdinv, q, GPG_F128_HOOK)
  }
  GPG_FS4(3)
  // (addresses used from here on are re-derived from an opaque copy of the thread index: computed ahead of the column steps -- they are
  // pure functions of it -- they were kept in ~50 registers across the steps and spilled around them)
  int tid2 = tid;
  asm volatile("" : "+v"(tid2));
#define GPG_F128_RELANE(t)  const int lane_ = (t) & 63, l15 = lane_ & 15, l4 = lane_ >> 4, q = (t) & 3, rr = (t) >> 2, tid = (t); (void)l15; (void)l4; (void)q; (void)rr; (void)tid;
  d4 c0[4], c1[4];                                           // T2 in the MFMA layout: rows 16 w + l15 (c0) and 64 + 16 w + l15 (c1), column 64 + 16 ni + 4 r + l4
  {
    GPG_F128_RELANE(tid2)
    const double* Cw = X + 16 * w + l15 + (size_t)(64 + l4) * ldx;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        c0[ni][r] = Cw[(size_t)(ni * 16 + 4 * r) * ldx];
        c1[ni][r] = Cw[64 + (size_t)(ni * 16 + 4 * r) * ldx];
      }
  }
  double a0[16], a1[16];
  {
    GPG_F128_RELANE(tid2)
    const int src = 4 * (4 * l15 + l4);
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int lo0 = __builtin_amdgcn_ds_bpermute(src, __double2loint(x0[m])), hi0 = __builtin_amdgcn_ds_bpermute(src, __double2hiint(x0[m]));
      const int lo1 = __builtin_amdgcn_ds_bpermute(src, __double2loint(x1[m])), hi1 = __builtin_amdgcn_ds_bpermute(src, __double2hiint(x1[m]));
      a0[m] = -__hiloint2double(hi0, lo0);
      a1[m] = -__hiloint2double(hi1, lo1);
    }
  }
  GPG_FS3(6)
  GPG_LDS_BARRIER();                                         // (1) every wave is through the column steps of block 0: the image region is free
  GPG_FS4(4)
  {
    GPG_F128_RELANE(tid2)
    GPG_F128_IMAGE(64)
#pragma unroll
    for (int s4 = 0; s4 < 16; ++s4) {
      double fn[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) fn[ni] = U[(4 * s4 + l4) * SA + ni * 16 + l15];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        c0[ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn[ni], a0[s4], c0[ni], 0, 0, 0);
        c1[ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fn[ni], a1[s4], c1[ni], 0, 0, 0);
      }
    }
  }
  GPG_LDS_BARRIER();                                         // (2) L21 is no longer read from the staging tile; the image of L22 is complete
  {
    GPG_F128_RELANE(tid2)
    const double* Tr = U + q * SA + rr;                      // rows 16 w .. 16 w + 15 are written and read by wave w only: no barrier
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) U[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = c0[ni][r];
#pragma unroll
    for (int m = 0; m < 16; ++m) x0[m] = Tr[(4 * m) * SA];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) U[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = c1[ni][r];
#pragma unroll
    for (int m = 0; m < 16; ++m) x1[m] = Tr[(4 * m) * SA];
  }
  GPG_FS4(5)
  {
    GPG_F128_RELANE(tid2)
    double* const Xs = X + rr + (size_t)(64 + q) * ldx;
    GPG_QUAD_SUBST2_HOOK(x0, x1, Ls, sdinv, q, GPG_F128_HOOK)
#undef GPG_F128_HOOK
  }
  GPG_FS4(6)
  GPG_FS3(0)
  GPG_FS3(1)
#undef GPG_F128_RELANE
#undef GPG_F128_RAW
#undef GPG_F128_IMAGE
#undef GPG_F128_TAKE_X
}

// The finalisations are inlined into the task: out of line, fin128_offdiag (which needs all 256 VGPRs) saved and reloaded the 112
// callee-saved ones through scratch per task, 2.6 us in and 4.2 us out (64 x 2560 columns 7.90 -> 7.31 ms inlined).
// Called with the ticket and the kernel's argument segment only: everything else is re-derived here by scalar loads.  What a task
// keeps alive across its MFMA loop is spilled, and every spill reload after the loop is a memory round trip under full load (the
// timeline of the first version of this function showed ~35 us of them in front of the call).
template <int SET>
__device__ __forceinline__ int fin128_offdiag(int tix_v, unsigned long long kernarg_bits) {
  constexpr int SA = 80, S2 = 72, BUF = 16 * SA;
  GPG_KERNARGS_FROM(TileCholArgs, ap, kernarg_bits);
  const int tix = __builtin_amdgcn_readfirstlane(tix_v);
  const int Mt = ap->Mt, ld = ap->ld;
  int task, b0, b1;
  if constexpr (SET == 2) {
    task = ap->tasks[tix];
    b0 = b1 = ap->batch_of ? ap->batch_of[tix] : 0;
  } else {
    task = ap->tasks[2 * tix + SET];
    b0 = ap->batch_of[2 * tix];
    b1 = ap->batch_of[2 * tix + 1];
  }
  const int ti = task & 0xffff, tj = task >> 16, b = SET == 1 ? b1 : b0;
  double* const A = ap->A + (size_t)b * ap->a_stride;
  double* const dinv_m = ap->dinv + (size_t)b * ap->d_stride;
  int* const info0 = ap->info + b0;
  int* const info1 = ap->info + b1;
  int* const fl0 = ap->flags + (size_t)b0 * ap->f_stride;
  int* const fl1 = ap->flags + (size_t)b1 * ap->f_stride;
  int* const ea0 = ap->pieces + (size_t)b0 * ap->f_stride;
  int* const ea1 = ap->pieces + (size_t)b1 * ap->f_stride;
  int* const pa0 = ea0 + 4 * tj; int* const pa1 = ea1 + 4 * tj;
  int* const pb0 = ea0 + 4 * Mt + 4 * tj; int* const pb1 = ea1 + 4 * Mt + 4 * tj;
  int* const fc0 = ea0 + 8 * Mt + tj; int* const fc1 = ea1 + 8 * Mt + tj;
  int* const done0 = fl0 + (size_t)tj * Mt + tj; int* const done1 = fl1 + (size_t)tj * Mt + tj;
  int* const abort_word = ap->abort_word;
  const size_t r0 = 128 * (size_t)ti, cj = 128 * (size_t)tj;
  double* const U = fin128_U<SET>();
  double (*const Ls)[4][18] = fin128_Ls<SET>();
  double* const sdinv = fin128_sdinv<SET>();
  int* const sh = fin128_sh<SET>();
  int* const sh2 = fin128_sh2<SET>();
  int tid_raw = (int)threadIdx.x;
  asm volatile("" : "+v"(tid_raw));                            // (inlined: nothing derived from the lane index may be hoisted above the task's MFMA loop)
  const int tid = SET == 2 ? tid_raw : (tid_raw & 255), lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int q = tid & 3, rr = tid >> 2;
  const int sp = tid & 31, sk = tid >> 5;
  const double* const L = A + cj + cj * (size_t)ld;            // the diagonal tile of this team's matrix
  const double* const dinv = dinv_m + cj;
  double* const X = A + r0 + cj * (size_t)ld;
  const int ldl = ld, ldx = ld;
  GPG_FS4(0)
  if (threadIdx.x == 0)
    *sh = __hip_atomic_load(done0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 &&
          __hip_atomic_load(done1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  __syncthreads();                                             // the hand-over is in LDS, the verdict on the diagonal tile in *sh
  const int fast = *sh;
  GPG_FS4(1)
#ifdef GPG_STAMP
  if (SET != 1 && threadIdx.x == 0 && t128_fo) t128_fo[7] = fast ? 2 : 1;
#endif
  double x0[16], x1[16];
  // (taken out of the hand-over tiles separately on each path, through an opaque copy of the thread index: loaded once ahead of the
  // branch, the initial values stayed live -- in scratch -- through the whole one-piece path)
#define GPG_F128_TAKE_X()                                                                    \
  {                                                                                         \
    int tq = tid;                                                                           \
    asm volatile("" : "+v"(tq));                                                            \
    const double* T0 = U + (tq & 3) * SA + (tq >> 2);                                        \
    const double* T1 = &fin128_Ls<SET>()[0][0][0] + (tq & 3) * S2 + (tq >> 2);               \
    _Pragma("unroll") for (int m = 0; m < 16; ++m) {                                         \
      x0[m] = T0[(4 * m) * SA];                                                             \
      x1[m] = T1[(4 * m) * S2];                                                             \
    }                                                                                       \
  }
  // column block 1 after its update: T2 -= X1 L21^T for the two row halves, each transposed through the LDS tile into x0 / x1
#define GPG_F128_UPDATE()                                                                    \
  _Pragma("unroll") for (int hh = 0; hh < 2; ++hh) {                                          \
    d4 acc[4];                                                                              \
    const double* Cw = X + 64 * hh + 16 * w + l15 + (size_t)(64 + l4) * ldx;                 \
    _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                                         \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) acc[ni][r] = Cw[(size_t)(ni * 16 + 4 * r) * ldx]; \
    wave_tile_gemm(acc, X + 64 * hh + 2 * sp + (size_t)sk * ldx, ldx, L + 64 + 2 * sp + (size_t)sk * ldl, ldl, 4, U, U + 2 * BUF, \
                   w, l15, l4, sp, sk);                                                     \
    __syncthreads();                                                                        \
    _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                                         \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) U[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = acc[ni][r]; \
    __syncthreads();                                                                        \
    const double* Tr = U + q * SA + rr;                                                     \
    if (hh == 0) { _Pragma("unroll") for (int m = 0; m < 16; ++m) x0[m] = Tr[(4 * m) * SA]; } \
    else { _Pragma("unroll") for (int m = 0; m < 16; ++m) x1[m] = Tr[(4 * m) * SA]; }        \
    __syncthreads();                                                                        \
  }
#define GPG_F128_STORE(COL0)                                                                 \
  {                                                                                         \
    double* Xr = X + rr + (size_t)((COL0) + q) * ldx;                                        \
    _Pragma("unroll") for (int m = 0; m < 16; ++m) {                                         \
      GPG_ST(&Xr[(size_t)(4 * m) * ldx], x0[m]);                                             \
      GPG_ST(&Xr[64 + (size_t)(4 * m) * ldx], x1[m]);                                        \
    }                                                                                       \
  }
  if (fast) {
    fin128_onepiece<SET>(X, ldx, L, ldl, dinv);
    return 1;                                                  // (the caller's publish step waits for the stores and synchronises the workgroup)
  }
  GPG_F128_TAKE_X()
  __syncthreads();                                             // x1 is out of the image region, *sh may be rewritten
  // piecewise: L11 / L22 arrive in four 16-column pieces each while the diagonal task is still at work
  // A piece whose flag is already up while the previous piece is being substituted is fetched into registers behind that
  // substitution (pf = 1): its turn then starts with the LDS write instead of a flag poll, two barriers and a dependent load.
  double lp4[4];
  int pf = 0;
#define GPG_F128_PIECE(FL, LP, DOFF, S)                                                      \
  {                                                                                         \
    if (!pf) {                                                                              \
      if (!wg_wait_flag2(FL##0 + (S), FL##1 + (S), abort_word, info0, info1, sh)) return 0;  \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                        \
        const int t = tid + 256 * u, jj = 16 * (S) + (t >> 6), k = t & 63;                   \
        lp4[u] = (LP)[k + (size_t)jj * ldl];                                                 \
      }                                                                                     \
    }                                                                                       \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                          \
      const int t = tid + 256 * u, jj = 16 * (S) + (t >> 6), k = t & 63;                     \
      Ls[jj][k & 3][k >> 2] = lp4[u];                                                        \
    }                                                                                       \
    if (tid < 16) sdinv[16 * (S) + tid] = dinv[(DOFF) + 16 * (S) + tid];                     \
    if ((S) < 3 && threadIdx.x == 0)                                                         \
      sh2[(S) & 1] = __hip_atomic_load(FL##0 + (S) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 && \
             __hip_atomic_load(FL##1 + (S) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;  \
    __syncthreads();                                                                        \
    pf = (S) < 3 ? sh2[(S) & 1] : 0;                                                        \
    if (pf) {                                                                               \
      GPG_ACQUIRE();                                                                        \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                        \
        const int t = tid + 256 * u, jj = 16 * ((S) + 1) + (t >> 6), k = t & 63;             \
        lp4[u] = (LP)[k + (size_t)jj * ldl];                                                 \
      }                                                                                     \
    }                                                                                       \
    GPG_QUAD_SUBST2_PIECE(x0, x1, Ls, sdinv, q, S)                                           \
    _Pragma("unroll") for (int m = 0; m < 16; ++m) { asm volatile("" : "+v"(x0[m])); asm volatile("" : "+v"(x1[m])); } \
  }
  GPG_F128_PIECE(pa, L, 0, 0)
  GPG_F128_PIECE(pa, L, 0, 1)
  GPG_F128_PIECE(pa, L, 0, 2)
  GPG_F128_PIECE(pa, L, 0, 3)
  GPG_FS4(2)
  GPG_F128_STORE(0)
  if (!wg_wait_flag2(fc0, fc1, abort_word, info0, info1, sh)) return 0;   // barrier inside: X1 in memory, L21 final
  GPG_FS4(3)
  GPG_F128_UPDATE()
  GPG_FS4(4)
  {
    const double* L22 = L + 64 + (size_t)64 * ldl;
    GPG_F128_PIECE(pb, L22, 64, 0)
    GPG_F128_PIECE(pb, L22, 64, 1)
    GPG_F128_PIECE(pb, L22, 64, 2)
    GPG_F128_PIECE(pb, L22, 64, 3)
  }
  GPG_FS4(5)
  GPG_F128_STORE(64)
  __syncthreads();
  GPG_FS4(6)
  return 1;
#undef GPG_F128_PIECE
#undef GPG_F128_UPDATE
#undef GPG_F128_STORE
#undef GPG_F128_TAKE_X
}


// fin128_diag: finalisation of a DIAGONAL 128 x 128 tile (both 128-tile kernels; SET as in fin128_offdiag).  On entry the top-left
// 64 x 64 block sits in the team's LDS tile (written by wave 0 of the team), A21 / A22 in memory:
//     L11 = chol(A11) (potrf64_wg; published in four 16-column pieces, early flags pa), L21 = A21 L11^-T (flag_c),
//     A22 -= L21 L21^T on MFMA, L22 = chol(A22) (pieces pb).
// Arguments as for fin128_offdiag: the ticket and the kernel's argument segment.
template <int SET>
__device__ __forceinline__ int fin128_diag(int tix_v, unsigned long long kernarg_bits) {
  constexpr int SA = 80;
  GPG_KERNARGS_FROM(TileCholArgs, ap, kernarg_bits);
  const int tix = __builtin_amdgcn_readfirstlane(tix_v);
  const int Mt = ap->Mt, ld = ap->ld, N = ap->N;
  int task, b;
  if constexpr (SET == 2) {
    task = ap->tasks[tix];
    b = ap->batch_of ? ap->batch_of[tix] : 0;
  } else {
    task = ap->tasks[2 * tix + SET];
    b = ap->batch_of[2 * tix + SET];
  }
  const int tj = task >> 16;
  double* const A = ap->A + (size_t)b * ap->a_stride;
  double* const dinv = ap->dinv + (size_t)b * ap->d_stride;
  int* const info = ap->info + b;
  int* const early = ap->pieces + (size_t)b * ap->f_stride;
  int* const pa = early + 4 * tj;
  int* const pb = early + 4 * Mt + 4 * tj;
  int* const flag_c = early + 8 * Mt + tj;
  const size_t cj = 128 * (size_t)tj;
  double* const U = fin128_U<SET>();
  double (*const Ls)[4][18] = fin128_Ls<SET>();
  double* const sdinv = fin128_sdinv<SET>();
  int tid_raw = (int)threadIdx.x;
  asm volatile("" : "+v"(tid_raw));
  const int tid = SET == 2 ? tid_raw : (tid_raw & 255), lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  double* blk = A + cj + cj * (size_t)ld;
  double (*St)[64] = reinterpret_cast<double(*)[64]>(&Ls[0][0][0]);   // potrf scratch over the image region
  __syncthreads();   // A11 was left in the LDS tile by wave 0; the other waves' stores of A21 / A22 are drained below
  GPG_FS4(0)
  {
    const int bad = potrf64_wg(U, SA, St, blk, ld, dinv + cj, pa, tid);   // L11 published in 16-column pieces pa[0..3]
    if (w == 0 && bad && lane == 0 && (int)cj + bad - 1 < N) atomicCAS(info, 0, (int)cj + bad);
  }
  __syncthreads();   // also drains the other waves' stores of A21 / A22
  GPG_FS4(1)
  panel_solve_rows64(blk, ld, dinv + cj, blk + 64, ld, 64, 64, U, Ls, sdinv, tid);   // L21 = A21 L11^-T
  GPG_RELEASE();     // L21 is final (every thread stored part of it; the solve ended with a barrier)
  __syncthreads();
  if (tid == 0) GPG_FLAG_UP(flag_c);
  GPG_FS4(2)
  const int sp = tid & 31, sk = tid >> 5;
  d4 a2[4];
  const double* C2 = blk + 64 + 16 * w + l15 + (size_t)(64 + l4) * ld;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) a2[ni][r] = C2[(size_t)(ni * 16 + 4 * r) * ld];
  const double* g21 = blk + 64 + 2 * sp + (size_t)sk * ld;
  wave_tile_gemm(a2, g21, ld, g21, ld, 4, U, U + 2 * 16 * SA, w, l15, l4, sp, sk);
  __syncthreads();
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) U[(ni * 16 + 4 * r + l4) * SA + 16 * w + l15] = a2[ni][r];
  __syncthreads();
  GPG_FS4(3)
  {
    const int bad = potrf64_wg(U, SA, St, blk + 64 + (size_t)64 * ld, ld, dinv + cj + 64, pb, tid);   // L22: pb[0..3]
    if (w == 0 && bad && lane == 0 && (int)cj + 64 + bad - 1 < N) atomicCAS(info, 0, (int)cj + 64 + bad);
  }
  GPG_FS4(4)
  return 1;
}

// ONE call site per task: with a call in each branch of `diagonal ? ... : ...` (and an early return after each) the compiler lays the two
// branches out one after the other, the accumulators of the second stay live across the call of the first, and all 240 live VGPRs
// are saved to scratch and reloaded around it (seen in the ISA, round 3).
template <int SET>
__device__ __forceinline__ int fin128_task(int tix_v, unsigned long long kernarg_bits, int is_diag) {
  return __builtin_amdgcn_readfirstlane(is_diag) ? fin128_diag<SET>(tix_v, kernarg_bits) : fin128_offdiag<SET>(tix_v, kernarg_bits);
}

__device__ __forceinline__ bool
tile128_chol_task(int tix, double* A, int ld, int Mt, const int* __restrict__ tasks, int* flags, int* early /* pa | pb | flag_c */, int* abort_word,
                  int* ticket, double* __restrict__ dinv, int* __restrict__ info, int N, const int* __restrict__ batch_of, size_t a_stride,
                  int d_stride, int f_stride, unsigned long long kbits) {
  __shared__ int sh_kr;
  int tid_task = threadIdx.x;
  asm volatile("" : "+v"(tid_task));   // per task: nothing derived from the lane index is kept alive from one task to the next (across its MFMA loop and finalisation)
  const int tid = tid_task, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w & 1, wn = w >> 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int task = tasks[tix];
  const int ti = task & 0xffff, tj = task >> 16;
  if (batch_of) {   // batched launch: several independent matrices (restart rows) share the grid
    const int b = batch_of[tix];
    A += (size_t)b * a_stride;
    dinv += (size_t)b * d_stride;
    info += b;
    flags += (size_t)b * f_stride;
    early += (size_t)b * f_stride;
  }
  const size_t r0 = 128 * (size_t)ti, cj = 128 * (size_t)tj;
  int* const frow_i = flags + (size_t)ti * Mt;
  int* const frow_j = flags + (size_t)tj * Mt;

#ifdef GPG_STAMP
  const unsigned long long tk_start = __builtin_amdgcn_s_memrealtime();
  unsigned long long tk_spin = 0, tk_gemm = 0, tk_runs = 0;
#endif
  // accumulator layout of direct_tile_gemm_acc: acc[2p + e][2g + m][r] <-> row 32 g + 2 l15 + m, column 32 p + 2 (4 r + l4) + e
  d4 acc[4][4];
  double* Cw = A + r0 + wm * 64 + 2 * l15 + (cj + wn * 64 + 2 * l4) * (size_t)ld;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double2 v = *reinterpret_cast<const double2*>(Cw + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ld);
        acc[ni][2 * g][r] = v.x;
        acc[ni][2 * g + 1][r] = v.y;
      }

  // ---- (1) left-looking accumulation ----------------------------------------------------------------------------
  GPG_PRIO_ACC(ti - tj)
  direct_tile_negate(acc);                                   // the loop ADDS the products to -A_ij (direct_tile_gemm_acc); sign restored below
  const unsigned lane_off = (unsigned)(2 * l15 + l4 * ld) * 8u;   // bytes: this lane's rows 2 t, 2 t + 1 of column l4 of a k-step
  int kdone = 0;
  while (kdone < tj) {
    GPG_TR(q0)
    if (w == 0) {                                           // wave 0 scans the two flag rows, 64 tile columns per pass
      int* const frows[2] = {frow_i, frow_j};
      int kr;
      const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        kr = wave_scan_flags<2>(frows, kdone, tj);
        if (kr > kdone) break;
        if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
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
    GPG_TR(q1)
    const size_t ck = 128 * (size_t)kdone;
    if (ti < Mt) {
      if (!(ti == tj && wm == 0 && wn == 1))   // diagonal tile: the block above the diagonal is never stored
        direct_tile_gemm_acc<GPG_MFMA_PF>(acc, A + r0 + wm * 64 + ck * (size_t)ld, lane_off, ld,
                                A + cj + wn * 64 + ck * (size_t)ld, lane_off, ld, 32 * (kr - kdone));
      else direct_tile_sync_only<GPG_MFMA_PF>(32 * (kr - kdone));
    } else if (wm == 0)   // right-hand-side tile row (prep_rows_kernel): rows 0 and 1 are real, the other 126 zero -- an eighth of the MFMAs
      direct_tile_gemm_acc<GPG_MFMA_PF, 2>(acc, A + r0 + ck * (size_t)ld, lane_off, ld,
                                 A + cj + wn * 64 + ck * (size_t)ld, lane_off, ld, 32 * (kr - kdone));
    else direct_tile_sync_only<GPG_MFMA_PF>(32 * (kr - kdone));
    __syncthreads();   // sh_kr may be rewritten
    GPG_TR(q2)
#ifdef GPG_STAMP
    tk_spin += q1 - q0; tk_gemm += q2 - q1; ++tk_runs;
#endif
    kdone = kr;
  }

#ifdef GPG_STAMP
  const unsigned long long tk_fin0 = __builtin_amdgcn_s_memrealtime();
#endif
  GPG_PRIO_FIN(ti - tj)
  direct_tile_negate(acc);
  // (the store addresses are formed HERE: derived from Cw before the loop, the compiler keeps all 32 of them alive across the MFMA
  // loop, spilled, and reloads them one memory round trip at a time)
  double* Cs = Cw;
  asm volatile("" : "+v"(Cs));
  // (likewise the lane indices: every LDS / memory address below is a pure function of the lane, i.e. invariant over the kernel's
  // task loop -- hoisted out of it, ~130 of them stay alive through every MFMA loop and every call, in scratch)
  int l15s = l15, l4s = l4;
  asm volatile("" : "+v"(l15s), "+v"(l4s));
  // ---- (2) Diagonal tile: the top-left 64 x 64 block goes straight into the LDS tile its own wave factors next, the strictly
  //      upper block is dropped, the rest goes to memory and is finalised in place (fin128_diag).  Tile below the diagonal:
  //      column block 0 is handed to fin128_offdiag through LDS, column block 1 goes to memory. -----------------------------------
  if (ti == tj) {
    if (w == 0) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            t128_U[(32 * (ni >> 1) + 8 * r + 2 * l4s + (ni & 1)) * 80 + 32 * (mi >> 1) + 2 * l15s + (mi & 1)] = acc[ni][mi][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else if (wm != 0) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double2 v;
            v.x = acc[ni][2 * g][r];
            v.y = acc[ni][2 * g + 1][r];
            *reinterpret_cast<double2*>(Cs + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ld) = v;
          }
    }
#ifdef GPG_STAMP
    if (tid == 0) t128_fo = nullptr;
#endif
  } else {
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
            *reinterpret_cast<double2*>(Cs + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ld) = v;
          }
    }
#ifdef GPG_STAMP
    if (tid == 0) t128_fo = (g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) ? g_stamp_buf + (size_t)GPG_STAMP_MAX * 8 + (size_t)tix * 8 : nullptr;
#endif
  }
  if (fin128_task<2>(tix, kbits, ti == tj) == 0) return false;
  // ---- (3) publish (and fetch the next ticket) --------------------------------------------------------------------
  GPG_PUBLISH_AND_NEXT(ticket, frow_i + tj)
#ifdef GPG_STAMP
  if (tid == 0 && g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) {
    unsigned long long* o = g_stamp_buf + (size_t)tix * 8;
    o[0] = tk_start; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = tk_spin; o[3] = tk_gemm; o[4] = tk_runs;
    o[5] = tk_fin0; o[6] = (unsigned long long)task; o[7] = (unsigned long long)blockIdx.x;
  }
#endif
  return true;
}

__global__ void __launch_bounds__(256, 2) tile128_chol_kernel(TileCholArgs) {   // c0 unused, pieces = early flags
  int tix;
  {
    GPG_KERNARGS(TileCholArgs, ap);
    tix = next_ticket(ap->ticket, &g_next_ticket);
  }
  for (;;) {
    GPG_KERNARGS(TileCholArgs, ap);
    if (tix >= ap->ntask) return;
    // inlined here (its MFMA loop wants every VGPR: a separate function would save / restore ~100 callee-saved registers
    // through scratch per task); re-reading the arguments per iteration keeps them out of the loop-carried SGPRs
    if (!tile128_chol_task(tix, ap->A, ap->ld, ap->Mt, ap->tasks, ap->flags, ap->pieces, ap->abort_word, ap->ticket, ap->dinv, ap->info,
                           ap->N, ap->batch_of, ap->a_stride, ap->d_stride, ap->f_stride, (unsigned long long)ap))
      return;                                             // aborted: every workgroup drains
    tix = __builtin_amdgcn_readfirstlane(g_next_ticket);
  }
}



// ------------------------------------------------------------------------------------------------
// pair128_chol_kernel (round 3): the same dataflow factorisation for BATCHED launches, 512 threads = two 256-thread teams per
// workgroup, ONE workgroup per compute unit.  A task is a PAIR of 128 x 128 tiles of one tile column j that go through the same
// control flow: team h owns tile (i_h, j) of matrix b_h.  Ordinary pairs are two consecutive rows of one matrix: both teams then
// read the SAME row panel L_j,0:j as their B operand, k-step by k-step at the same pace -- eight waves that start a run together and
// execute the same instruction stream stay together by themselves: a workgroup barrier in the loop (GPG_PAIR_KSYNC k-steps apart;
// 0 = none, the default) only adds its skew: 283.4 ms and 3.90e8 KiB FETCH_SIZE without, 289.0 ms and 4.08e8 with one every 8 k-steps
// -- so it crosses the L2 -> L1 path once per pair: the operand stream of a 256 x 128 footprint, 25 % fewer bytes than two independent
// 128 x 128 tiles.  Diagonal tiles pair with the diagonal tile of the NEXT matrix of the batch
// (same j, same barrier sequence, different data); what is left over in a tile column pairs with the next matrix's leftover,
// and a tile without any partner is simply given to both teams (identical instruction streams on identical data: the duplicate
// stores write identical values).  Every barrier is a full-workgroup barrier: the two teams never diverge in control flow, and
// every decision that depends on flags (how far the next MFMA run goes, which 16-column piece of L_jj is final) is taken by
// thread 0 for both tiles at once.  Flags, early flags, ticket order and the progress argument are those of tile128_chol_kernel:
// a pair waits only for tiles of earlier tile columns and for the diagonal tiles of its own column, which precede it in the list.
// What it gives up: with one workgroup per CU the finalisation of a pair is not overlapped with another workgroup's MFMA loop.
// ------------------------------------------------------------------------------------------------
constexpr int GPG_PAIR_KSYNC = 0;             // k-steps between two workgroup barriers in the pair kernel's MFMA loop: none (measured above)
constexpr int GPG_PAIR_PF = GPG_MFMA_PF;   // k-steps of operand prefetch in the pair kernel's MFMA loop (its eight waves run in lock step: nobody covers a late load)
__device__ __forceinline__ bool
pair128_chol_task(int tix, double* Abase, int ld, int Mt, const int* __restrict__ tasks, int* flags_base, int* early_base, int* abort_word,
                  int* ticket, double* __restrict__ dinv_base, int* __restrict__ info_base, int N, const int* __restrict__ batch_of,
                  size_t a_stride, int d_stride, int f_stride, unsigned long long kbits) {
  __shared__ int sh_kr;
  int tid_task = threadIdx.x;
  asm volatile("" : "+v"(tid_task));   // (see tile128_chol_task)
  const int tid = tid_task, h = __builtin_amdgcn_readfirstlane(tid >> 8), t = tid & 255, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w & 1, wn = w >> 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  // both teams' assignments (uniform values; [h] selects this thread's)
  const int task0 = tasks[2 * tix], task1 = tasks[2 * tix + 1];
  const int b0 = batch_of[2 * tix], b1 = batch_of[2 * tix + 1];
  const int tj = task0 >> 16;                                   // common tile column; both tiles diagonal or both below the diagonal
  const int ti0 = task0 & 0xffff, ti1 = task1 & 0xffff;
  const int ti = h ? ti1 : ti0, b = h ? b1 : b0;
  double* const A = Abase + (size_t)b * a_stride;
  double* const dinv = dinv_base + (size_t)b * d_stride;
  int* const fl0 = flags_base + (size_t)b0 * f_stride;
  int* const fl1 = flags_base + (size_t)b1 * f_stride;
  int* const ea0 = early_base + (size_t)b0 * f_stride;
  int* const ea1 = early_base + (size_t)b1 * f_stride;
  int* const info0 = info_base + b0;
  int* const info1 = info_base + b1;
  const size_t r0 = 128 * (size_t)ti, cj = 128 * (size_t)tj;

  d4 acc[4][4];
  double* Cw = A + r0 + wm * 64 + 2 * l15 + (cj + wn * 64 + 2 * l4) * (size_t)ld;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double2 v = *reinterpret_cast<const double2*>(Cw + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ld);
        acc[ni][2 * g][r] = v.x;
        acc[ni][2 * g + 1][r] = v.y;
      }

#ifdef GPG_STAMP
  const unsigned long long tk_start = __builtin_amdgcn_s_memrealtime();
  unsigned long long tk_spin = 0, tk_gemm = 0, tk_runs = 0;
#endif
  // ---- (1) left-looking accumulation: runs as far as the flags of BOTH tiles' rows (and of tile row j of both matrices) allow ----
  direct_tile_negate(acc);                                   // the loop adds the products to -A_ij; sign restored below
  const unsigned lane_off = (unsigned)(2 * l15 + l4 * ld) * 8u;
  int kdone = 0;
  while (kdone < tj) {
    GPG_TR(q0)
    if (tid < 64) {                                         // wave 0 of team 0 scans the four flag rows, 64 tile columns per pass
      int* const frows[4] = {fl0 + (size_t)ti0 * Mt, fl0 + (size_t)tj * Mt, fl1 + (size_t)ti1 * Mt, fl1 + (size_t)tj * Mt};
      int kr;
      const unsigned long long t_wait = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        kr = wave_scan_flags<4>(frows, kdone, tj);
        if (kr > kdone) break;
        if (__builtin_amdgcn_s_memrealtime() - t_wait > GPG_TILE_WAIT_TICKS || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          if (tid == 0) {
            __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicMax(info0, GPG_INFO_INTERNAL);
            atomicMax(info1, GPG_INFO_INTERNAL);
          }
          kr = -1;
          break;
        }
        __builtin_amdgcn_s_sleep(8);
      }
      if (tid == 0) sh_kr = kr;
    }
    __syncthreads();
    const int kr = __builtin_amdgcn_readfirstlane(sh_kr);
    if (kr < 0) return false;
    GPG_ACQUIRE();
    GPG_TR(q1)
    const size_t ck = 128 * (size_t)kdone;
    const int nstep = 32 * (kr - kdone);
    if (ti < Mt) {
      if (!(ti == tj && wm == 0 && wn == 1))
        direct_tile_gemm_acc<GPG_PAIR_PF, 4, GPG_PAIR_KSYNC>(acc, A + r0 + wm * 64 + ck * (size_t)ld, lane_off, ld,
                                                            A + cj + wn * 64 + ck * (size_t)ld, lane_off, ld, nstep);
      else direct_tile_sync_only<GPG_PAIR_PF, GPG_PAIR_KSYNC>(nstep);
    } else if (wm == 0)
      direct_tile_gemm_acc<GPG_PAIR_PF, 2, GPG_PAIR_KSYNC>(acc, A + r0 + ck * (size_t)ld, lane_off, ld,
                                                          A + cj + wn * 64 + ck * (size_t)ld, lane_off, ld, nstep);
    else direct_tile_sync_only<GPG_PAIR_PF, GPG_PAIR_KSYNC>(nstep);
    __syncthreads();
    GPG_TR(q2)
#ifdef GPG_STAMP
    tk_spin += q1 - q0; tk_gemm += q2 - q1; ++tk_runs;
#endif
    kdone = kr;
  }
#ifdef GPG_STAMP
  const unsigned long long tk_fin0 = __builtin_amdgcn_s_memrealtime();
#endif

  // ---- (2) diagonal tiles: top-left block into the team's LDS tile, the rest to memory; tiles below the diagonal: column block 0
  //      into LDS for fin128_offdiag, column block 1 to memory -----------------------------------------------------------------------
  direct_tile_negate(acc);
  double* Cs = Cw;                                            // (see tile128_chol_task)
  asm volatile("" : "+v"(Cs));
  int l15s = l15, l4s = l4;
  asm volatile("" : "+v"(l15s), "+v"(l4s));
  if (ti0 == tj) {
    if (w == 0) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            (h ? p128_U[1] : p128_U[0])[(32 * (ni >> 1) + 8 * r + 2 * l4s + (ni & 1)) * 80 + 32 * (mi >> 1) + 2 * l15s + (mi & 1)] = acc[ni][mi][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else if (wm != 0) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double2 v;
            v.x = acc[ni][2 * g][r];
            v.y = acc[ni][2 * g + 1][r];
            *reinterpret_cast<double2*>(Cs + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ld) = v;
          }
    }
  } else {
    if (wn == 0) {
      if (h) fin128_handoff_block0<1>(acc, wm, l15s, l4s); else fin128_handoff_block0<0>(acc, wm, l15s, l4s);
    } else {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double2 v;
            v.x = acc[ni][2 * g][r];
            v.y = acc[ni][2 * g + 1][r];
            *reinterpret_cast<double2*>(Cs + 32 * g + (size_t)(32 * (ni >> 1) + 8 * r + (ni & 1)) * ld) = v;
          }
    }
  }
#ifdef GPG_STAMP
  if (tid == 0) {
    t128_fo = (g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) ? g_stamp_buf + (size_t)GPG_STAMP_MAX * 8 + (size_t)tix * 8 : nullptr;
    t128_wait_acc = 0;
    if (t128_fo) for (int k = 0; k < 8; ++k) t128_fo[k] = 0;
  }
  GPG_FS3(5)
#endif
  if ((h ? fin128_task<1>(tix, kbits, ti0 == tj) : fin128_task<0>(tix, kbits, ti0 == tj)) == 0) return false;
#ifdef GPG_STAMP
  if (tid == 0 && t128_fo) (g_stamp_buf + (size_t)GPG_STAMP_MAX * 16 + (size_t)tix * 16)[15] = t128_wait_acc;
  GPG_FS3(2)
#endif
  // ---- (3) publish both tiles (and fetch the next ticket) --------------------------------------------------------------------------
  {
    int nxt_ = 0;
    if (tid == 0) nxt_ = GPG_TICKET_FETCH(ticket);
    GPG_RELEASE();
    GPG_FS3(3)
    if (tid == 0) g_next_ticket = nxt_;
    __syncthreads();
    GPG_FS3(4)
    if (tid == 0) {
      GPG_FLAG_UP(fl0 + (size_t)ti0 * Mt + tj);
      GPG_FLAG_UP(fl1 + (size_t)ti1 * Mt + tj);
    }
  }
#ifdef GPG_STAMP
  if (tid == 0 && g_stamp_buf != nullptr && tix < GPG_STAMP_MAX) {
    unsigned long long* o = g_stamp_buf + (size_t)tix * 8;
    o[0] = tk_start; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = tk_spin; o[3] = tk_gemm; o[4] = tk_runs;
    o[5] = tk_fin0; o[6] = (unsigned long long)task0; o[7] = (unsigned long long)blockIdx.x;
  }
#endif
  return true;
}

__global__ void __launch_bounds__(512, 1) pair128_chol_kernel(TileCholArgs) {   // tasks: two ints per task, batch_of: two per task
  int tix;
  {
    GPG_KERNARGS(TileCholArgs, ap);
    tix = next_ticket(ap->ticket, &g_next_ticket);
  }
  for (;;) {
    GPG_KERNARGS(TileCholArgs, ap);
    if (tix >= ap->ntask) return;
    if (!pair128_chol_task(tix, ap->A, ap->ld, ap->Mt, ap->tasks, ap->flags, ap->pieces, ap->abort_word, ap->ticket, ap->dinv, ap->info,
                           ap->N, ap->batch_of, ap->a_stride, ap->d_stride, ap->f_stride, (unsigned long long)ap))
      return;
    tix = __builtin_amdgcn_readfirstlane(g_next_ticket);
  }
}

}  // namespace
