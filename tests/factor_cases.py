"""The case table shared by tests/test_factor_host.py (LAPACK, no device) and tests/test_gpu_factor.py (every device
schedule): the matrices whose Cholesky factor is checked entry by entry, and the matrices whose factorisation must stop
at a chosen pivot."""
from collections import namedtuple

import numpy as np

from oracle import gp_oracle as orc

# name, kernel (device name), hp_kernel (alpha of RatQu or None), n, d, use_grad, wellcond, theta, etaK, seed
Case = namedtuple("Case", "name kernel hp_kernel n d use_grad wellcond theta etaK seed")

# Gradient-free, so N = n exactly: the matrix edge on a tile edge of either tile size, and one row to either side of it; one to
# five 128-tile columns, one to ten 64-tile columns, odd and even numbers of tile rows.
SIZES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 513, 640)
# Points are uniform in [-2, 2]^2; with these length scales every point has a few strongly correlated neighbours, and the nugget
# keeps every pivot above 1e-4 (diag(L) >= 1e-2) however they cluster.
BASE_THETA = (1.5, 2.5)
BASE_ETA = 1e-4

BASE_CASES = tuple(Case(f"sqexp_n{n}", "SqExp", None, n, 2, False, "base", BASE_THETA, BASE_ETA, 100 + n) for n in SIZES)
# gradient-enhanced twins: the P L extraction and the gradient blocks
TWIN_CASES = (
    Case("ma5f2_grad_N192", "Ma5f2", None, 64, 2, True, "precon", (0.8, 1.7), 1e-4, 7),
    Case("ratqu_grad_N260", "RatQu", 2.0, 65, 3, True, "precon", (0.6, 1.1, 0.4), 1e-4, 8),
    Case("sqexp_grad_N387", "SqExp", None, 43, 8, True, "precon", (0.30, 0.12, 0.45, 0.20, 0.08, 0.25, 0.15, 0.35), 1e-4, 9),
)
CASES = BASE_CASES + TWIN_CASES


def case_N(c):
    return c.n * (c.d + 1) if c.use_grad else c.n


def case_data(c):
    """X [n, d], f [n], g [n, d] of the case."""
    return orc.synthetic_design(c.n, c.d, seed=c.seed)


def oracle_matrices(c):
    """(M, Kcov, pvec): the matrix that is factorised -- Kcov itself for 'base', Kcor + eta I for 'precon' (varK = 1, no
    noise) --, Kcov, and the diagonal preconditioner (None for 'base'); reference Kernel.py:213-237 / 268-277."""
    X = case_data(c)[0]
    theta = np.asarray(c.theta, dtype=np.float64)
    kern = (c.kernel, c.hp_kernel) if c.hp_kernel is not None else c.kernel
    K = orc.kern_grad(X, X, theta, kern) if c.use_grad else orc.kern_base(X, X, theta, kern)
    N = K.shape[0]
    if c.wellcond == "precon":
        pvec = np.sqrt(np.diag(K))
        M = K / np.outer(pvec, pvec)
        M[np.diag_indices(N)] += c.etaK
        return M, M * np.outer(pvec, pvec), pvec
    M = K + c.etaK * np.eye(N)
    return M, M, None


# ---- failing pivot -------------------------------------------------------------------------------------------------------
# 300 points on a unit grid, theta = 15: off-diagonal entries are at most exp(-15) = 3e-7.  With the nugget -0.5 every pivot is
# about 0.5 -- until point m - 1, a copy of point 0 displaced by 1e-3 (K = exp(-1.5e-5)): pivot m = 0.5 - K^2 / 0.5, about -1.5.
# m = 1 has no earlier point to copy; there the nugget is -1.5 and the first pivot itself is -0.5.
FAIL_N = 300
FAIL_M = (1, 16, 17, 64, 65, 128, 129, 257, 300)
FAIL_THETA = (15.0, 15.0)


def failing_pivot_case(m):
    """(X [300, 2], etaK) whose base matrix K + etaK I stops the factorisation at pivot m (1-based)."""
    assert 1 <= m <= FAIL_N
    gx, gy = np.meshgrid(np.arange(20.0), np.arange(15.0), indexing="ij")
    X = np.column_stack((gx.ravel(), gy.ravel()))
    assert X.shape == (FAIL_N, 2)
    if m == 1:
        return X, -1.5
    X[m - 1] = X[0] + np.array([1e-3, 0.0])
    return X, -0.5


def failing_pivot_matrix(m):
    X, eta = failing_pivot_case(m)
    return orc.kern_base(X, X, np.asarray(FAIL_THETA), "SqExp") + eta * np.eye(FAIL_N)
