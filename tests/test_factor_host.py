"""CPU: the case table of tests/factor_cases.py and the checker of tests/factor_checks.py are sound without the device --
LAPACK's factor of every case passes check_factor with s = 0, no case sits near breakdown, small corruptions of a factor
or of a solve are caught, LAPACK stops the failing-pivot matrices exactly where intended, and the two diagnostic setters
refuse a missing context."""
import functools

import numpy as np
import pytest
from scipy.linalg.lapack import dpotrf

import factor_cases as fc
import factor_checks as chk
from gpgradpy_amd import _lib


@functools.lru_cache(maxsize=None)
def _lapack(name):
    """(M, Kcov, pvec, L) of a case, computed once and shared (treated as read-only)."""
    c = next(c for c in fc.CASES if c.name == name)
    M, Kcov, pvec = fc.oracle_matrices(c)
    L, info = dpotrf(M, lower=1, clean=1)
    assert info == 0
    for a in (M, Kcov, L):
        a.setflags(write=False)
    return M, Kcov, pvec, L


CASE_IDS = [c.name for c in fc.CASES]


@pytest.mark.parametrize("name", CASE_IDS)
def test_lapack_factor_passes_with_s0(name):
    c = next(c for c in fc.CASES if c.name == name)
    M, Kcov, pvec, L = _lapack(name)
    assert M.shape == (fc.case_N(c),) * 2
    worst = chk.check_factor(M, L, s=0)
    assert worst <= 1.0
    d = np.diag(L)
    assert d.min() >= 1e-3 * d.max(), (d.min(), d.max())          # no case near breakdown
    if pvec is not None:
        # the scaled factor against Kcov, as the device test compares which = 3 with which = 1: host scaling is one rounding per
        # entry of P L and two per entry of Kcov, inside the device's allowance
        chk.check_factor(Kcov, pvec[:, None] * L, s=chk.PRECON_S, kcov_c=chk.PRECON_C)


@pytest.mark.parametrize("name", ["sqexp_n65", "sqexp_n257", "sqexp_n640", "ratqu_grad_N260"])
def test_checker_catches_corrupted_factors(name):
    M, _, _, L = _lapack(name)
    N = L.shape[0]
    aL = np.abs(L)
    # one sub-diagonal entry times (1 + 1e-10): in the last row, the entry that weighs most in its own residual bound
    i = N - 1
    share = aL[i, :i] * np.diag(aL)[:i] / (aL[i:i + 1] @ aL[:i].T).ravel()
    j = int(np.argmax(share))
    L1 = L.copy()
    L1[i, j] *= 1.0 + 1e-10
    with pytest.raises(AssertionError, match="exceeds its bound"):
        chk.check_factor(M, L1, s=chk.DEVICE_S)
    # a 4 x 4 patch zeroed (a stale or unwritten piece), strictly below the diagonal
    r0, c0 = N - 5, (N - 5) // 2
    L2 = L.copy()
    L2[r0:r0 + 4, c0:c0 + 4] = 0.0
    with pytest.raises(AssertionError, match="exceeds its bound"):
        chk.check_factor(M, L2, s=chk.DEVICE_S)
    # structure: something above the diagonal, a non-positive diagonal entry, a NaN
    L3 = L.copy(); L3[0, N - 1] = 1e-300
    with pytest.raises(AssertionError, match="upper triangle"):
        chk.check_factor(M, L3)
    L4 = L.copy(); L4[N // 2, N // 2] *= -1.0
    with pytest.raises(AssertionError, match="non-positive"):
        chk.check_factor(M, L4)
    L5 = L.copy(); L5[N - 1, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        chk.check_factor(M, L5)


@pytest.mark.parametrize("name", ["sqexp_n65", "sqexp_n640", "sqexp_grad_N387"])
def test_check_apply_accepts_host_results_and_catches_a_swap(name):
    from scipy.linalg import solve_triangular
    M, _, _, L = _lapack(name)
    N = L.shape[0]
    e_last = np.zeros(N); e_last[-1] = 1.0
    for v in (np.random.default_rng(5).standard_normal(N), e_last):
        out0 = L @ (L.T @ v)
        out1 = solve_triangular(L, solve_triangular(L, v, lower=True), lower=True, trans="T")
        assert chk.check_apply(L, v, out0, 0) <= 1.0
        assert chk.check_apply(L, v, out1, 1) <= 1.0
        for op, out in ((0, out0), (1, out1)):
            bad = out.copy()
            a, b = N - 1, N - 2                       # e_N: the only entries of (L L^T) e_N that matter sit at the end
            assert bad[a] != bad[b]
            bad[a], bad[b] = bad[b], bad[a]
            with pytest.raises(AssertionError, match="exceeds its bound"):
                chk.check_apply(L, v, bad, op)


@pytest.mark.parametrize("m", fc.FAIL_M)
def test_lapack_stops_at_the_intended_pivot(m):
    A = fc.failing_pivot_matrix(m)
    off = A - np.diag(np.diag(A))
    off[m - 1, 0] = off[0, m - 1] = 0.0
    assert np.abs(off).max() < 1e-6                    # well separated: only the planted pair is coupled
    _, info = dpotrf(A, lower=1)
    assert info == m
    # the failing pivot as a Schur complement, and the ones before it
    k = m - 1
    if k:
        Lk, info_k = dpotrf(A[:k, :k], lower=1, clean=1)
        assert info_k == 0 and np.all(np.diag(Lk) ** 2 > 0.4)
        w = np.linalg.solve(A[:k, :k], A[:k, k])
        piv = A[k, k] - A[k, :k] @ w
    else:
        piv = A[0, 0]
    assert piv < -0.1, piv


def test_setters_refuse_a_missing_context():
    """Without a device no context can be created; what the setters can be asked there is to refuse NULL (the argument checks on
    a live context are in tests/test_gpu_factor.py)."""
    lib = _lib.load()
    assert "gpg_set_fuse_max_tiles" in _lib.ABI_SYMBOLS and "gpg_set_task_order" in _lib.ABI_SYMBOLS
    for arg in (-2, -1, 0, 1, 48):
        assert lib.gpg_set_fuse_max_tiles(None, arg) == -1
        assert lib.gpg_set_task_order(None, arg) == -1
