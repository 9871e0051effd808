"""Uncertainty of the GLS mean coefficients in the posterior (gpg_set_mean_uncertainty / mean_unc=True): the parts that need no device.

The yardstick of tests/test_gpu_meanunc.py is meanunc_reference() below: the oracle construction of tests/test_joint_host.py
(joint_model / joint_reference, imported unchanged) plus the universal-kriging term in plain NumPy,
    cov_tot = cov_ref + varK U H^-1 U',   H = V' K^-1 V,   U = V_q - Kqy K^-1 V,
K^-1 by cho_solve with the factor the joint reference uses, V the augmented Vandermonde matrix of the model ([1_n; 0], or with the
first-order mean value row a: [1, x_a], gradient row (i, a): e_(i+1), masked points without gradient rows), V_q the same basis at
the query rows.

Metric: E = max_ij |cov - cov_ref|_ij / (varK sqrt(S_ii S_jj)), S = diag(Kqq + U H^-1 U') -- the added term can exceed Kqq, so Kqq
alone is the wrong scale.  Bound: the project's standing E_BOUND = 2e-7.

Checked here, on all sixteen fixtures at two point sets each (the fixture's own xq; six "outside" points on the faces of a box
twice the size of the design's bounding box):
  * the reference agrees with the forward-only route the device takes (Z = Kqy P^-1 L^-T and W_V = L^-1 V by triangular solves,
    H = W_V' W_V, U = V_q - Z W_V) to E <= 2e-8: two orderings of the same arithmetic, a tenth of E_BOUND (measured 5.4e-13 or less);
  * at the outside points the value rows of the added term are >= 1e-4 S on thirteen fixtures (measured 1.2e-4 .. 0.6): there the
    device tests can tell "term present" from "term missing"; on the other three it is negligible and they are not counted;
  * 2 cov_tot[f_j, d_k f_j] equals central differences of diag(cov_tot): the gradient rows of U and the cross blocks are consistent
    with the value rows.  Step h = 1e-5 of the box half-width in each coordinate: truncation ~ h^2 and rounding ~ 1e-16 / h = 1e-11
    relative to the E scale, so 1e-6 of that scale leaves four orders for the third derivatives (measured 1e-8 or better);
  * the two new symbols are declared in include/gpgrad.h, listed in _lib.ABI_SYMBOLS and exported by the built library.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve, solve_triangular

from conftest import ROOT
from test_joint_host import E_BOUND, PARITY, joint_model, joint_reference  # noqa: F401  (E_BOUND: the bound the device tests hold E to)

LINMEAN_MORE = ("linmean/linmean_RatQu_none_n14_d3", "linmean/linmean_SqExp_none_n12_d3", "linmean/linmean_SqExp_none_n17_d4_mask",
                "linmean/linmean_SqExp_none_n30_d2_nograd", "linmean/linmean_SqExp_none_n9_d16")
FIXTURES = PARITY + LINMEAN_MORE
NEGLIGIBLE = ("SqExp_none_n5_d2", "SqExp_none_n200_d4", "SqExp_none_n20_d2_neardup")     # added term < 1e-4 S at the outside points
MUST_DIFFER = tuple(n for n in FIXTURES if n not in NEGLIGIBLE)
NEW_SYMBOLS = ("gpg_set_mean_uncertainty", "gpg_mean_gram")
TERM_MIN = 1e-4
assert len(FIXTURES) == 16 and len(MUST_DIFFER) == 13


def outside_points(c):
    """Six points on the faces of the box twice the size of the design's bounding box."""
    nx, d = 6, c["d"]
    lo, hi = c["x"].min(axis=0), c["x"].max(axis=0)
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    x = ctr + 2.0 * half * np.random.default_rng(5).uniform(-1.0, 1.0, (nx, d))
    for j in range(nx):
        k = j % d
        x[j, k] = ctr[k] + (2.0 if (j // d) % 2 == 1 else -2.0) * half[k]
    return x


def point_sets(jm):
    return (("xq", jm.c["xq"]), ("outside", outside_points(jm.c)))


def aug_vand(jm):
    """V [N, n_beta] of the model in the derivative-major row order of the training data."""
    c = jm.c
    n, d = c["n"], c["d"]
    nb = d + 1 if jm.linear else 1
    ng = 0 if not c["use_grad"] else (n if jm.mask is None else int(np.sum(jm.mask)))
    V = np.zeros((n + ng * d, nb))
    V[:n, 0] = 1.0
    if jm.linear:
        V[:n, 1:] = c["x"]
        for i in range(d):
            V[n + i * ng:n + (i + 1) * ng, i + 1] = 1.0
    return V


def query_basis(jm, xq, calc_grad):
    """V_q [m, n_beta]: value row j [1, x_j] (or [1]), row of d/dx_k at any point e_(k+1) (or 0)."""
    nx, d = xq.shape
    nb = d + 1 if jm.linear else 1
    Vq = np.zeros((nx * (d + 1) if calc_grad else nx, nb))
    Vq[:nx, 0] = 1.0
    if jm.linear:
        Vq[:nx, 1:] = xq
        if calc_grad:
            for k in range(d):
                Vq[(k + 1) * nx:(k + 2) * nx, k + 1] = 1.0
    return Vq


def _kqy(jm, xq, calc_grad):
    from oracle import gp_oracle as orc
    c = jm.c
    Kg = orc.kern_grad(c["x"], xq, c["theta"], c["kernel_o"], grad_cols=True, mask1=jm.mask)
    if not c["use_grad"]:
        Kg = Kg[:c["n"]]
    return Kg if calc_grad else Kg[:, :xq.shape[0]]


def mean_gram_reference(jm):
    V = aug_vand(jm)
    return V.T @ cho_solve(jm.chofac, V)


def meanunc_reference(jm, xq, calc_grad=True):
    """(mean_ref [m], cov_tot [m, m], S [m], term [m, m]): the joint posterior with the uncertainty of the mean coefficients,
    S = diag(Kqq + U H^-1 U') the scale of the metric, term = U H^-1 U' (without varK)."""
    mean, cov, Kqq = joint_reference(jm, xq, calc_grad)
    V, Vq, Kg = aug_vand(jm), query_basis(jm, xq, calc_grad), _kqy(jm, xq, calc_grad)
    KiV = cho_solve(jm.chofac, V)
    H = V.T @ KiV
    U = Vq - Kg.T @ KiV
    term = U @ cho_solve(cho_factor(H, lower=True), U.T)
    term = 0.5 * (term + term.T)
    return mean, cov + jm.varK * term, np.diag(Kqq) + np.diag(term), term


def meanunc_error(cov, cov_ref, S, varK):
    s = np.sqrt(S)
    return float(np.max(np.abs(cov - cov_ref) / (varK * np.outer(s, s))))


def forward_only(jm, xq, calc_grad=True):
    """The same covariance by the route of the device: forward substitutions only."""
    _, _, Kqq = joint_reference(jm, xq, calc_grad)
    L = np.tril(jm.chofac[0]) if jm.chofac[1] else np.triu(jm.chofac[0]).T
    Z = solve_triangular(L, _kqy(jm, xq, calc_grad), lower=True).T
    WV = solve_triangular(L, aug_vand(jm), lower=True)
    H = WV.T @ WV
    U = query_basis(jm, xq, calc_grad) - Z @ WV
    C = solve_triangular(np.linalg.cholesky(H), U.T, lower=True).T
    return jm.varK * (Kqq - Z @ Z.T + C @ C.T)


def test_new_symbols_declared_listed_exported():
    from gpgradpy_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpgrad.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpg_[a-z_]+)\s*\(", txt))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/gpgrad.h"
        assert s in _lib.ABI_SYMBOLS, f"{s} is not listed in _lib.ABI_SYMBOLS"
        assert hasattr(lib, s), f"{s} is not exported by the library"


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_agrees_with_forward_only_route(name):
    jm = joint_model(name)
    for tag, xq in point_sets(jm):
        _, cov_tot, S, _ = meanunc_reference(jm, xq)
        E = meanunc_error(forward_only(jm, xq), cov_tot, S, jm.varK)
        print(f"{name} {tag}: forward-only against cho_solve  E = {E:.2e}")
        assert E <= 2e-8
        assert np.max(np.abs(cov_tot - cov_tot.T)) <= 1e-12 * jm.varK * S.max()


@pytest.mark.parametrize("name", FIXTURES)
def test_added_term_at_the_outside_points(name):
    jm = joint_model(name)
    xq = outside_points(jm.c)
    nx = xq.shape[0]
    _, _, S, term = meanunc_reference(jm, xq)
    ratio = np.diag(term)[:nx] / S[:nx]
    print(f"{name}: added term / S on the value rows  {ratio.min():.2e} .. {ratio.max():.2e}")
    assert np.all(np.diag(term) >= -1e-12 * S)
    if name in MUST_DIFFER:
        assert ratio.min() >= TERM_MIN
    else:
        assert ratio.min() < TERM_MIN          # stays a "term negligible" case


@pytest.mark.parametrize("name", MUST_DIFFER)
def test_cross_block_is_half_the_gradient_of_the_variance(name):
    jm = joint_model(name)
    c = jm.c
    xq = outside_points(c)
    nx, d = xq.shape
    half = 0.5 * (c["x"].max(axis=0) - c["x"].min(axis=0))
    _, cov_tot, S, _ = meanunc_reference(jm, xq)
    j = np.arange(nx)
    worst = 0.0
    for k in range(d):
        h = 1e-5 * half[k]
        xp, xm = xq.copy(), xq.copy()
        xp[:, k] += h
        xm[:, k] -= h
        vp = np.diag(meanunc_reference(jm, xp, False)[1])
        vm = np.diag(meanunc_reference(jm, xm, False)[1])
        fd = (vp - vm) / (xp[:, k] - xm[:, k])
        scale = jm.varK * np.sqrt(S[j] * S[(k + 1) * nx + j])
        worst = max(worst, float(np.max(np.abs(2.0 * cov_tot[j, (k + 1) * nx + j] - fd) / scale)))
    print(f"{name}: |2 cov[f, d f] - central differences of var f| = {worst:.2e} of the E scale")
    assert worst <= 1e-6
