"""Componentwise checks of a Cholesky factor and of products / solves through it.  Plain NumPy, float64; every
tolerance is a rounding-error bound, none is tuned.  u = 2^-53, gamma_k = k u / (1 - k u).

Rows and columns are 0-based here, so entry (i, j) of L L^T is a sum of k = min(i, j) + 1 products.

Roundings of the device's pivot step (gpgradpy_amd/csrc/chol_device.h: potrf64_wave and potrf64_wg run the same
sequence; the 128-tile kernels call potrf64_wg and, like the 64-tile and the blocked ones, scale their panels by
GPG_QUAD_SUBST* with the reciprocal pivots that sequence left in dinv -- one count serves every schedule):

    y0 = v_rsq_f64(a)                      seed, relative error e (|e| <= 2^-20 is all that is used)
    g = a y0 (d1), h = y0 / 2 (exact)      g ~ sqrt(a), h ~ 1 / (2 sqrt(a))
    r = 1/2 - h g; g = g + g r (d2); h = h + h r (d3)
    r = 1/2 - h g; dj = g + g r (d4); inv = 2 (h + h r) (d5)        each |d.| <= u; r is formed by one FMA and is
                                                                     so small that its own rounding is below 2^-70
    A coupled step maps the errors (e_g, e_h) of (g, h) to ((e_g - e_h) / 2 + O(e^2), (e_h - e_g) / 2 + O(e^2)):
    the common part is squared away, the difference -- born from d1 .. d3 -- is halved and handed on.  Hence
        dj  = sqrt(a)     (1 + ( d1 + d2 - d3) / 2 + d4 + O(e^4)),   |.| <= 2.5 u
        inv = 1 / sqrt(a) (1 + (-d1 - d2 + d3) / 2 + d5 + O(e^4)),   |.| <= 2.5 u,     dj inv = 1 + d4 + d5.
    Diagonal entry: L_jj^2 = a_hat (1 + .)^2 carries 5 roundings where a correctly rounded sqrt carries 2; a_hat, the
    updated pivot, is the usual chain of FMAs (k - 1 roundings).  Theorem 10.3's diagonal bound gamma_(k+1)
    becomes gamma_(k+4).
    Off-diagonal entry: L_ij = fl(t inv), so L_ij L_jj = t (1 + d)(1 + d4)(1 + d5): 3 roundings where the division
    carries 1 -- gamma_(k+2).
    One more unit pays for the O(e^4) remainders and the products of the d's, which are not multiples of u^2 that a
    gamma would absorb:  s = 5  (DEVICE_S).  The LAPACK factor of the host tests is checked with s = 0.

Extraction of a preconditioned factor (solve.hip: extract_kernel; assembly.hip: the epilogue of assemble_kernel).
which = 3 is fl(L_rj fl(sqrt(dvec_r))): 2 roundings per entry, 4 per product of two.  which = 1, Kcov, is formed
from the very value that is factorised (which = 2, Kp) as fl(fl(fl(1 / ip_r) Kp_rc) fl(1 / ip_c)) with
ip = fl(1 / fl(sqrt(dvec))): 3 + 3 + 2 = 8 roundings (diagonal: fl(fl(p Kp) p), p = fl(sqrt(dvec)): 4).  With
p = sqrt(dvec) exact,
    Kcov - (PL)(PL)^T = p_r p_c [ (Kp - L L^T) + theta_8 Kp - sum_j theta_4 L_rj L_cj ]_rc
so the bound is gamma_(k+s+4) on |PL||PL|^T (plus 4 more for expressing p_r p_c |L||L|^T by the rounded |PL||PL|^T
and for the second-order part of gamma_8):  s grows by PRECON_S = 8, and c u |Kcov| with c = PRECON_C = 8 is added.
"""
import numpy as np

U = 2.0 ** -53
DEVICE_S = 5
PRECON_S = 8
PRECON_C = 8
# un-scaling a downloaded P L by sqrt(diag Kern) on the host for check_apply: device sqrt and product (2), host sqrt
# and quotient (1), dvec against the downloaded diagonal of Kern under a square root (1): 4 per entry of L, 8 per
# product of two
UNSCALE_S = 8


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def check_factor(A, L, s=DEVICE_S, kcov_c=0):
    """|A - L L^T|_ij <= 2 gamma_(min(i,j)+1+s) (|L||L|^T)_ij  (+ kcov_c u |A|_ij), entry by entry.

    A: the symmetric matrix that was factorised; L: the factor, dense [N, N], lower triangular.
    The device side of the bound is Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3 with the pivot
    step counted in the module docstring; it holds for any order of accumulation and with FMA.  The factor 2 pays
    for the two float64 products formed here, which obey the same gamma whatever BLAS does with their sums.
    Also asserts: strict upper triangle exactly zero, all entries finite, diagonal positive.
    Returns the worst ratio of the left side to the right side (0 where both vanish)."""
    A = np.asarray(A, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    N = L.shape[0]
    assert A.shape == (N, N) and L.shape == (N, N)
    assert np.all(np.isfinite(L)), "factor has non-finite entries"
    assert np.all(np.isfinite(A)), "matrix has non-finite entries"
    assert not np.any(np.triu(L, 1)), "strict upper triangle of the factor is not exactly zero"
    assert np.all(np.diag(L) > 0.0), "factor has a non-positive diagonal entry"
    idx = np.arange(N)
    k = np.minimum(idx[:, None], idx[None, :]) + 1
    aL = np.abs(L)
    lhs = np.abs(A - L @ L.T)
    rhs = 2.0 * gamma(k + s) * (aL @ aL.T) + kcov_c * U * np.abs(A)
    bad = lhs > rhs
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(rhs > 0.0, lhs / rhs, np.where(lhs > 0.0, np.inf, 0.0))
    worst = float(ratio.max())
    if bad.any():
        i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"|A - L L^T| exceeds its bound at {int(bad.sum())} entries; worst ratio {worst:.3g} at ({i}, {j}): "
                             f"residual {lhs[i, j]:.3e}, bound {rhs[i, j]:.3e}")
    return worst


APPLY_C0 = 4
APPLY_C1 = 4


def check_apply(L, v, out, op, s=DEVICE_S):
    """Products and solves through the factor, entry by entry, N = len(v):

    op 0, out = (L L^T) v:   |out - L (L^T v)| <= c0 gamma_(N+s) (|L||L|^T|v|)
        The device forms w = L^T v and L w by dot products of at most N terms: |w_hat - L^T v| <= gamma_N |L|^T|v| and
        |out - L w_hat| <= gamma_N |L||w_hat|, together (2 gamma_N + gamma_N^2) |L||L|^T|v|.  The reference formed here
        the same way costs the same again: c0 = 4; the gamma_N^2 terms vanish in the step from gamma_N to gamma_(N+s).
    op 1, out = (L L^T)^-1 v:   |v - L (L^T out)| <= c1 gamma_(N+s) (|L||L|^T|out|)
        Two substitutions, Higham Thm 8.5: (L + D1) y = v, (L^T + D2) out = y with |D.| <= gamma_N |L| -- gamma_(N+2)
        on the device, which multiplies by the reciprocal pivot (inv L_jj = 1 + d4 + d5, module docstring, and the
        product) where the theorem divides.  v = (L + D1)(L^T + D2) out gives (2 gamma + gamma^2) |L||L|^T|out|, and
        forming L (L^T out) here costs 2 gamma_N more: c1 = 4, second-order terms covered by s = 5 against the 2 counted.
    Returns the worst ratio of the left side to the right side."""
    L = np.asarray(L, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    out = np.asarray(out, dtype=np.float64)
    N = v.size
    assert L.shape == (N, N) and out.shape == (N,) and op in (0, 1)
    assert np.all(np.isfinite(out)), "result has non-finite entries"
    aL = np.abs(L)
    if op == 0:
        lhs = np.abs(out - L @ (L.T @ v))
        rhs = APPLY_C0 * gamma(N + s) * (aL @ (aL.T @ np.abs(v)))
    else:
        lhs = np.abs(v - L @ (L.T @ out))
        rhs = APPLY_C1 * gamma(N + s) * (aL @ (aL.T @ np.abs(out)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(rhs > 0.0, lhs / rhs, np.where(lhs > 0.0, np.inf, 0.0))
    worst = float(ratio.max())
    if np.any(lhs > rhs):
        i = int(np.argmax(ratio))
        raise AssertionError(f"factor_apply op {op} exceeds its bound; worst ratio {worst:.3g} at row {i}: "
                             f"residual {lhs[i]:.3e}, bound {rhs[i]:.3e}")
    return worst


def lndet_tolerance(diagL, extra_abs=0.0):
    """|ln_det - 2 sum ln L_ii| <= N 4 u max|ln L_ii| (+ extra_abs): each logarithm on either side is good to an ulp or
    two of itself and the sums add N of them."""
    d = np.asarray(diagL, dtype=np.float64)
    return d.size * 4.0 * U * float(np.max(np.abs(np.log(d)))) + extra_abs
