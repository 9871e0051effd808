// Small device helpers shared by the HIP translation units (gfx950): wave / workgroup sums and compensated accumulation.
#pragma once
#include <hip/hip_runtime.h>

namespace {   // internal to every includer, as the copies this header replaces were

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// block-wide sum of NV values per thread; result valid in every thread
template <int NV>
__device__ void block_sum(double (&v)[NV], double* sh /* [NV * 16] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double s = wave_sum(v[q]);
    if (lane == 0) sh[q * 16 + w] = s;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += sh[q * 16 + i];
    v[q] = s;
  }
  __syncthreads();
}

// Neumaier's compensated accumulation: s + comp carries the sum to ~eps |result| + eps^2 sum |terms|.  The mean
// mu = beta + sum_c Wt[j, c] z[c] cancels by a factor ~kappa on ill-conditioned cases (|alpha| ~ kappa |mu|), so the
// order of a plain summation shows up at eps kappa (measured 4e-8 .. 2e-7 at kappa = 7e9 depending on the slicing).
__device__ __forceinline__ void kb_add(double& s, double& comp, double x) {
  const double t = s + x;
  comp += (fabs(s) >= fabs(x)) ? (s - t) + x : (x - t) + s;
  s = t;
}

}  // namespace
