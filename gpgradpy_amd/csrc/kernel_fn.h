// The covariance functions (SqExp, Matern 5/2, RatQu) and their x-derivatives, written once, and the (kernel, d) dispatcher of
// the kernels that use them.  Included by assembly.hip, solve.hip, gradient.hip and joint.hip.
//
// Every function here is a __forceinline__ template on the covariance function: the text is compiled under the flags of
// whichever unit includes it.  assembly.hip and joint.hip are built with -ffp-contract=off, so that there the entries keep the
// operation order of the NumPy reference to the last ulp of exp() / sqrt() / pow(); the other units contract to fused
// multiply-adds.  The brackets below ARE that operation order (and the bitwise tests between the paths depend on it): a
// change here is a change of every kernel's bits.  tools/isa_diff.py compares the generated code of two builds.
//
// Not here, because they have one user each: the hyperparameter derivatives of grad_contract_kernel (gradient.hip) and of
// rtensor_kern_dhp_kernel (assembly.hip: it also forms the second-derivative block from R_i R_j multiplied first, a bracketing
// of its own), and the third-order columns of rtensor_kern_hess_x_kernel (below).
//
// Notation: R = x1 - x2 (each kernel says which point is which), s = sum_k theta_k R_k^2, and per covariance function
//              SqExp                Matern 5/2, nu = sqrt(s)                    RatQu, B = 1 + s / alpha
//   K00        exp(-s)              (1 + sqrt5 nu + 5/3 nu^2) exp(-sqrt5 nu)    B^(-alpha)
//   M1         --                   5/3 (1 + sqrt5 nu) exp(-sqrt5 nu)  (mat1)   B^(-alpha-1)
//   E          exp(-s)              exp(-sqrt5 nu)  (Abase)                     B^(-alpha-2)   (takes the place of E in the second derivatives)
//   F3         --                   --                                          B^(-alpha-3)
// Reference: KernelSqExp.py:338-408, KernelMatern5f2.py:369-448, KernelRatQuad.py:463-476, 523-554.
#pragma once
#include <type_traits>
#include <utility>
#include "gpg_internal.h"

// ---- radial part ------------------------------------------------------------------------------------------------------
// One term of s.  The kernels that follow KernelSqExp.py:381 accumulate the SqExp sum negatively (s -= ...; exp(s)), the others
// positively (exp(-s)): NEG_S says which, and kern_radial must be told the same.  Equal values, not equal code.
template <int KERN, bool NEG_S>
__device__ __forceinline__ void kern_s_add(double& s, double th, double R) {
  if (KERN == GPG_KERNEL_SQEXP && NEG_S) s -= th * (R * R);
  else s += th * (R * R);
}

// A caller pays for what it reads: the rest is dead code (cross_kernel computes no B^(-alpha-2), cross_dx_rows_kernel no K00).
struct KernRadial {
  double E, M1, K00, F3;
  double c3, inu;   // Matern 5/2: sqrt5 / nu (KernelMatern5f2.py:500) and 1 / nu (:592), nu clamped at 1e-16
  double Bq;        // RatQu: B
};

template <int KERN, bool NEG_S = false>
__device__ __forceinline__ KernRadial kern_radial(double s, double alpha /* RatQu only */) {
  KernRadial r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (KERN == GPG_KERNEL_SQEXP) {
    r.E = exp(NEG_S ? s : -s);
    r.K00 = r.E;
  } else if (KERN == GPG_KERNEL_RATQU) {   // KernelRatQuad.py:463-476: f_p = B^(-alpha-p): K00 = f_0, M1 = f_1, E = f_2, F3 = f_3
    r.Bq = 1.0 + s / alpha;
    r.K00 = pow(r.Bq, -alpha);
    r.M1 = pow(r.Bq, -alpha - 1.0);
    r.E = pow(r.Bq, -alpha - 2.0);
    r.F3 = pow(r.Bq, -alpha - 3.0);
  } else {
    const double sqrt5 = sqrt(5.0), nu = sqrt(s);
    r.E = exp(-sqrt5 * nu);                          // Abase
    r.M1 = ((5.0 / 3.0) * (1.0 + sqrt5 * nu)) * r.E;   // mat1
    r.K00 = (1.0 + sqrt5 * nu + (5.0 / 3.0) * (nu * nu)) * r.E;
    r.c3 = sqrt5 / fmax(nu, 1e-16);
    r.inu = 1.0 / fmax(nu, 1e-16);
  }
  return r;
}

// ---- first derivatives ------------------------------------------------------------------------------------------------
// block (i+1, 0): d K / d x1_i  (KernelRatQuad.py:540)
template <int KERN>
__device__ __forceinline__ double kern_d10(double th, double R, double E, double M1) {
  if (KERN == GPG_KERNEL_SQEXP) return ((-2.0 * th) * R) * E;
  if (KERN == GPG_KERNEL_RATQU) return ((-2.0 * th) * R) * M1;
  return ((-th) * R) * M1;
}

// block (0, i+1): d K / d x2_i, its negative as the reference writes it (KernelRatQuad.py:541)
template <int KERN>
__device__ __forceinline__ double kern_d01(double th, double R, double E, double M1) {
  if (KERN == GPG_KERNEL_SQEXP) return ((2.0 * th) * R) * E;
  if (KERN == GPG_KERNEL_RATQU) return ((2.0 * th) * R) * M1;
  return (th * R) * M1;
}

// ---- second derivatives: block (i+1, j+1) = d2 K / d x1_i d x2_j ---------------------------------------------------------
// rq_c: the constant of RatQu's second derivatives (KernelRatQuad.py:529), which the caller computes once; unused by the others
__device__ __forceinline__ double kern_rq_c(double alpha) { return 4.0 * (1.0 + 1.0 / alpha); }

template <int KERN>
__device__ __forceinline__ double kern_d11_diag(double th, double R, double E, double M1, double rq_c) {   // i == j  (KernelRatQuad.py:544)
  if (KERN == GPG_KERNEL_SQEXP) return (2.0 * th - (4.0 * (th * th)) * (R * R)) * E;
  if (KERN == GPG_KERNEL_RATQU) return (2.0 * th) * M1 - ((rq_c * (th * th)) * (R * R)) * E;
  return th * M1 - (((25.0 / 3.0) * (th * th)) * (R * R)) * E;
}

// i != j  (KernelRatQuad.py:554).  The value is symmetric in (i, j), the rounding is not: the kernels that walk the lower
// block triangle (assemble_kernel, rtensor_kern_kernel, grad_contract_kernel) pass the reference's (lo, hi) = (smaller, larger)
// index here, the cross-covariance kernels (training block i, query direction j).  One bracketing, two argument orders.
template <int KERN>
__device__ __forceinline__ double kern_d11_off(double th_i, double th_j, double R_i, double R_j, double E, double rq_c) {
  if (KERN == GPG_KERNEL_SQEXP) return ((-4.0 * th_i) * th_j) * ((R_i * R_j) * E);
  if (KERN == GPG_KERNEL_RATQU) return (((((-rq_c) * th_i) * th_j) * R_i) * R_j) * E;
  return (((((-(25.0 / 3.0)) * th_i) * th_j) * R_i) * R_j) * E;
}

template <int KERN>
__device__ __forceinline__ double kern_d11(bool same, double th_i, double th_j, double R_i, double R_j, double E, double M1, double rq_c) {
  return same ? kern_d11_diag<KERN>(th_i, R_i, E, M1, rq_c) : kern_d11_off<KERN>(th_i, th_j, R_i, R_j, E, rq_c);
}

// ---- entries of the Hessian contraction (hess_contract_kernel, solve.hip) ----------------------------------------------------
// Reference: kernel second / third derivatives KernelSqExp.py:48-88, 412-468, KernelMatern5f2.py:54-94, 453-530,
// KernelRatQuad.py:51-136, 556-632.  With R = x_train - x_query, tR_i = th_i R_i, d_ik = (i == k):
//   base column a          : d2K[k,i] = (-2 th_i d_ik + 4 th_i th_k R_i R_k) E                     (SqExp)
//                                       -th_k M1 d_ik + (25/3) th_i R_i th_k R_k E                 (Matern 5/2)
//                                       RatQu: KernelRatQuad.py:51-136
//   gradient column (j, a) : d2K[k,i] = (4 th_i th_j (d_ik R_j + d_jk R_i) + 4 d_ij th_i th_k R_k
//                                        - 8 th_i th_j th_k R_i R_j R_k) E                          (SqExp)
//                                       (25/3) (th_i d_ik th_j R_j + th_j d_jk th_i R_i + th_i d_ij th_k R_k
//                                        - sqrt5 / nu th_i R_i th_j R_j th_k R_k) E                 (Matern 5/2)
//                                       RatQu: KernelRatQuad.py:556-632
// th_k and tR_k come separately: hess_contract_kernel reads row k's coordinate through memory (k is its workgroup index).
// rtensor_kern_hess_x_kernel (assembly.hip) takes its base column from here as well; its gradient columns carry the opposite
// sign (R = X1 - X2 there) in an order of their own and stay in that kernel.
// rq_s1 = 1 + 1/alpha, rq_s2 = rq_s1 (1 + 2/alpha): RatQu's scalar1, scalar2, which the caller computes once; unused by the others
template <int KERN>
__device__ __forceinline__ double kern_d2k_base(int i, int k, double th_i, double th_k, double tR_i, double tR_k, double E, double M1, double rq_s1) {
  if (KERN == GPG_KERNEL_SQEXP) return (4.0 * tR_i * tR_k - (i == k ? 2.0 * th_i : 0.0)) * E;
  if (KERN == GPG_KERNEL_RATQU) return (4.0 * rq_s1) * tR_i * tR_k * E - (i == k ? 2.0 * th_i * M1 : 0.0);
  return (25.0 / 3.0) * tR_i * tR_k * E - (i == k ? th_k * M1 : 0.0);
}

template <int KERN>
__device__ __forceinline__ double kern_d2k_grad(int i, int j, int k, double th_i, double th_j, double tR_i, double tR_j, double tR_k,
                                                double E, double F3, double c3, double rq_s1, double rq_s2) {
  const double lin = (i == k ? th_i * tR_j : 0.0) + (j == k ? th_j * tR_i : 0.0) + (i == j ? th_i * tR_k : 0.0);
  double v;
  if (KERN == GPG_KERNEL_SQEXP) {
    v = 4.0 * lin - 8.0 * tR_i * tR_j * tR_k;
    v *= E;
  } else if (KERN == GPG_KERNEL_RATQU) {
    v = (4.0 * rq_s1) * lin * E - (8.0 * rq_s2) * tR_i * tR_j * tR_k * F3;
  } else {
    v = lin - c3 * tR_i * tR_j * tR_k;
    v *= (25.0 / 3.0) * E;
  }
  return v;
}

// ---- dispatch -----------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, KERN>, std::integral_constant<int, D>) for the run-time (kernel, d); d outside 1 .. GPG_MAX_DIM
// calls nothing (gpg_create refuses it).  Seen by the host and the device pass alike: the kernels f names are instantiated here.
template <int KERN, class F, int... DS>
inline void gpg_for_d(int d, F& f, std::integer_sequence<int, DS...>) {
  (void)((d == DS + 1 && (f(std::integral_constant<int, KERN>{}, std::integral_constant<int, DS + 1>{}), true)) || ...);
}

template <class F>
inline void gpg_for_kern_d(int kernel, int d, F f) {
  using Ds = std::make_integer_sequence<int, GPG_MAX_DIM>;
  if (kernel == GPG_KERNEL_SQEXP) gpg_for_d<GPG_KERNEL_SQEXP>(d, f, Ds{});
  else if (kernel == GPG_KERNEL_RATQU) gpg_for_d<GPG_KERNEL_RATQU>(d, f, Ds{});
  else gpg_for_d<GPG_KERNEL_MA5F2>(d, f, Ds{});
}
