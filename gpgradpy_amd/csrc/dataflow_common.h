// Dataflow kernels (cholesky_dataflow.hip), shared part: ticket scheduling of the persistent workgroups, wave priorities, the
// publish step, access to the kernel argument segment.  gfx950 only.
#pragma once
#include "chol_device.h"

namespace {

constexpr int GPG_MFMA_PF = 1;   // k-steps of operand fragments in flight ahead of the MFMAs (16 VGPRs each); PF + 1 a power of two.
                                 // Round 3, with exact waits in the loop (direct_tile_gemm_acc): 1 is as fast as 3 on ten cfg3 matrices per launch
                                 // (299.9 / 299.2 ms) and faster on short contractions (4608 columns x 16: 10.85 / 11.02 ms; 9216 x 1: 7.7 / 8.1) --
                                 // the second wave of the SIMD covers the latency, and a shallower queue keeps the shared slices in the 32-KB L1

// One ticket counter per launch.  (Eight of them, workgroup b drawing from queue b % 8 -- the static task -> XCD deal of a
// one-task-per-workgroup launch, kept persistent -- were no faster.)
#define GPG_TICKET_FETCH(ticket) __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// Next task of a persistent workgroup: one relaxed agent-scope fetch-add by thread 0, shared through LDS.  The two
// barriers also separate the LDS use of consecutive tasks.
__device__ __forceinline__ int next_ticket(int* ticket, int* sh) {
  __syncthreads();
  if (threadIdx.x == 0) *sh = GPG_TICKET_FETCH(ticket);
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*sh);   // the same word for every lane: said so, or every address derived from the task is per-lane arithmetic
}

// Wave priority by phase.  The two workgroups of a compute unit share every SIMD, and between equal priorities the
// OLDER wave wins the issue arbitration.  With one-task workgroups that order follows the task order by itself (the
// workgroup nearer its end is the older one); persistent workgroups keep their launch age for the whole factorisation,
// so half of the latency-bound finalisations (dependent fp64 VALU chains: pivots, substitutions) would queue behind the
// partner's MFMA stream whatever their place on the critical path.  The finalisation therefore raises its priority
// explicitly, the accumulation of a diagonal tile (the head of its tile column) runs above ordinary accumulation.
#define GPG_PRIO(n) __builtin_amdgcn_s_setprio(n)
// Priority by distance from the diagonal, dd = i - j of the tile: the head of a tile column (diagonal tile, the next few
// rows) is what the following columns' heads wait for.  Timelines (tools/timeline_compare.py) show tile (j+1, j) finishing
// 12 us after diag(j) with one-task workgroups (where the older = earlier task wins the arbitration) but 124 us after it
// with persistent ones at equal priorities.
constexpr int GPG_PRIO_NEAR = 3;   // tile rows below the diagonal that count as the head of their tile column
#define GPG_PRIO_ACC(dd) { if ((dd) == 0) { GPG_PRIO(2); } else if ((dd) <= GPG_PRIO_NEAR) { GPG_PRIO(1); } }
#define GPG_PRIO_FIN(dd) { if ((dd) <= GPG_PRIO_NEAR) { GPG_PRIO(3); } else { GPG_PRIO(2); } }

// Ticket of the NEXT task, fetched by the publish step of the current one (GPG_PUBLISH_AND_NEXT): the fetch-add travels
// with the drain of the tile's write-through stores, so a workgroup that finishes a task knows its next one without a
// further round trip.  That matters on the critical path of a factorisation: the diagonal tile of the next column
// usually gets its workgroup only when some task ends (all slots are busy), and whatever that workgroup spends finding
// out what to do next is added to every one of the Mt hops of the dependency chain (measured: 141 tile columns x ~6 us).
// The ticket is held without being worked on only for the duration of that drain.
__shared__ int g_next_ticket;
#define GPG_PUBLISH_AND_NEXT(ticket, flag_ptr)                                             \
  {                                                                                         \
    int nxt_ = 0;                                                                           \
    if (threadIdx.x == 0) nxt_ = GPG_TICKET_FETCH(ticket);                                  \
    GPG_RELEASE();                                                                          \
    if (threadIdx.x == 0) g_next_ticket = nxt_;                                             \
    __syncthreads();                                                                        \
    if (threadIdx.x == 0) GPG_FLAG_UP(flag_ptr);                                            \
    GPG_PRIO(0);                                                                            \
  }

// The task body of a persistent kernel is compiled as a function of its own (noinline) that fetches the kernel's
// arguments from the kernarg segment by scalar loads: inlined into the task loop, the arguments stay live in ~25 SGPRs
// across the back edge and the compiler spills the broadcast operands of the pivot chain (potrf64_wave) through
// v_writelane / v_readlane instead -- 400 extra pairs in tile_chol_kernel, 8 % on a chain-bound factorisation.  The
// kernel's formal parameter is only there to give the segment its layout.
#define GPG_KERNARGS(T, ap)                                                                                   \
  const __attribute__((address_space(4))) T* ap =                                                             \
      (const __attribute__((address_space(4))) T*)__builtin_amdgcn_kernarg_segment_ptr();                      \
  asm volatile("" : "+s"(ap))
// In a (noinline) device function the kernarg segment pointer is NOT available through the builtin (it reads as null
// there): the kernel passes it as an ordinary argument, which arrives in VGPRs; readfirstlane makes it scalar again so
// that the loads through it are s_load.
#define GPG_KERNARGS_FROM(T, ap, bits)                                                                        \
  const unsigned long long ap##_u =                                                                           \
      ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)((bits) >> 32)) << 32) |             \
      (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)((bits) & 0xffffffffull));            \
  const __attribute__((address_space(4))) T* ap = (const __attribute__((address_space(4))) T*)ap##_u

// Arguments of the three factorisation kernels (tile_chol_kernel, tile128_chol_kernel, pair128_chol_kernel).
struct TileCholArgs {
  double* A; int ld, c0, Mt; const int* tasks; int ntask; int* flags; int* pieces; int* abort_word; int* ticket; double* dinv;
  int* info; int N; const int* batch_of; size_t a_stride; int d_stride, f_stride, fuse;
};

}  // namespace
