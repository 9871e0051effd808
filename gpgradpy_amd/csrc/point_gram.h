// The inner trip shared by the per-point Gram kernels (loo_gram_kernel of loo.hip over W = L^-T, second_gram_kernel of second.hip
// over the swept rows Z of the query points): lane <-> point, a column of the rows layout is read by buffer loads with the column
// as the (uniform) descriptor and the lane's row as a 32-bit byte offset.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// byte offset beyond every column descriptor (a column has Npad * 8 < 2^31 bytes); offset + 8 does not wrap in 32 bits either
constexpr unsigned kLooOutOfRange = 0x80000000u;

constexpr int loo_nacc(int G, bool diag) { return diag ? G * (G + 1) / 2 : G * G; }
constexpr int loo_cdiv(int a, int b) { return (a + b - 1) / b; }
// columns per trip: about 18 load instructions of a lane in flight
constexpr int loo_unroll(int loads) { return loo_cdiv(18, loads); }

typedef unsigned int loo_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double loo_load(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
  return __builtin_bit_cast(double, (loo_u32x2)__builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)byte_off, 0, 0));
}

// U columns c, c + 4, ... < hi: the jm leading block rows of B (and, off the diagonal, all G block rows of A) at this lane's point.
// DIAG: acc[j (j + 1) / 2 + i] += b_i b_j, i <= j;  else acc[j G + i] += a_i b_j.
// Buffer loads: the column (uniform: scalar registers) is the descriptor, the lane's row a 32-bit byte offset -- one address
// register per block row for the whole kernel instead of a 64-bit pointer per load in flight.  What is not to be read is out of
// the descriptor's range -- a block row that is not active in this segment by its offset (kLooOutOfRange), a column >= hi of the
// last trip by a descriptor of zero bytes --: such a load touches no memory and returns 0.0, and its products add +0.0.  So the
// loop body is straight-line code however many block rows are active, and the sums stay in place in their registers (a switch
// over that number made the compiler keep several copies of them).
template <int G, bool DIAG, int U>
__device__ __forceinline__ void loo_trip(const double* __restrict__ W, int ldw, int c, int hi, const unsigned (&ra)[G],
                                         const unsigned (&rb)[G], double (&acc)[loo_nacc(G, DIAG)]) {
  double b[U][G];
  double a[U][DIAG ? 1 : G];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int cu = c + 4 * u;
    const __amdgpu_buffer_rsrc_t col = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(W + (size_t)(cu < hi ? cu : c) * ldw), 0,
                                                                         cu < hi ? ldw * 8 : 0, 0x00020000);
#pragma unroll
    for (int j = 0; j < G; ++j) b[u][j] = loo_load(col, rb[j]);
    if constexpr (!DIAG) {
#pragma unroll
      for (int i = 0; i < G; ++i) a[u][i] = loo_load(col, ra[i]);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if constexpr (DIAG) {
#pragma unroll
        for (int i = 0; i <= j; ++i) acc[j * (j + 1) / 2 + i] += b[u][i] * b[u][j];
      } else {
#pragma unroll
        for (int i = 0; i < G; ++i) acc[j * G + i] += a[u][i] * b[u][j];
      }
    }
  }
}

}  // namespace
