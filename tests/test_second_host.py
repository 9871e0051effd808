"""Per-point gradient covariance and batched Hessians (gpg_predict_second / eval_model_second, gpgradpy_amd/second.py): the parts
that need no device.

* ABI: the two new symbols are declared in include/gpgrad.h, listed in _lib.ABI_SYMBOLS and exported by the built library.
* The yardstick of tests/test_gpu_second.py is block_reference() below: block_ref_j[i, k] = cov_ref[i nx + j, k nx + j] of
  joint_reference (tests/test_joint_host.py, imported unchanged; with mean_unc the cov_tot of meanunc_reference).  On every fixture
  of PARITY it is pinned here to
    - what the fixtures store from the reference: sqrt(block_00) against `sig`, block_0,k+1 against sig dsigdx (the SIG_* and
      DSIG_RTOL rules of tests/tolerances.py, as tests/test_joint_host.py holds the full matrix to them);
    - orc.eval_model_hess: d2sig2 = -2 varK (H2 + T) with T = K0_gg - block_gg / varK taken from the block and H2 formed as the
      oracle forms it, against the d2sig2 that the oracle's d2sigdx2 stands for, 2 sig d2sigdx2 + 2 dsigdx dsigdx'.  The two differ
      by the rounding of the block alone, which E_BOUND bounds on the normalised scale: |difference|_ik <= 2 E_BOUND varK
      sqrt(K0_ii K0_kk) (measured 2.0e-8 of that bound or less; printed, pytest -s).
* The helpers of gpgradpy_amd/second.py on hand-made inputs, a zero directional variance in prob_descent included.
"""
import ctypes
import os
import re
from math import erf, sqrt

import numpy as np
import pytest
from scipy.linalg import cho_solve

import tolerances as tol
from conftest import ROOT
from oracle import gp_oracle as orc
from test_joint_host import E_BOUND, PARITY, joint_model, joint_reference
from test_meanunc_host import meanunc_reference

NEW_SYMBOLS = ("gpg_predict_second", "gpg_set_second_chunk")


def blocks_of(mat, nx):
    """[nx, bs, bs] point-diagonal blocks of a joint matrix in the derivative-major row order (row blk * nx + j)."""
    bs = mat.shape[0] // nx
    idx = np.arange(bs)[None, :] * nx + np.arange(nx)[:, None]                  # [nx, bs]
    return mat[idx[:, :, None], idx[:, None, :]]


def block_reference(jm, xq, mean_unc=False):
    """(mean_ref [m], block_ref [nx, bs, bs], scale [nx, bs]): the blocks of the oracle's joint covariance at xq and the diagonal
    the metric normalises with (K0 = diag Kqq; with mean_unc S = diag(Kqq + U H^-1 U') of tests/test_meanunc_host.py)."""
    nx = xq.shape[0]
    if mean_unc:
        mean, cov, S, _ = meanunc_reference(jm, xq, True)
    else:
        mean, cov, Kqq = joint_reference(jm, xq, True)
        S = np.diag(Kqq)
    bs = cov.shape[0] // nx
    return mean, blocks_of(cov, nx), S.reshape(bs, nx).T.copy()


def block_error(got, ref, scale, varK):
    """E = max |got - ref|_jik / (varK sqrt(scale_ji scale_jk))."""
    s = np.sqrt(scale)
    return float(np.max(np.abs(got - ref) / (varK * s[:, :, None] * s[:, None, :])))


def oracle_model(jm):
    """The oracle's EvalModel of a JointModel (the same factor and alpha; beta[0] alone enters its mu)."""
    c = jm.c
    return orc.EvalModel(c["x"], np.asarray(c["theta"], float), c["kernel_o"], c["use_grad"], np.ravel(jm.beta), jm.varK, jm.chofac,
                         jm.alpha, jm.mask)


def hess_reference(jm, xq, points=None):
    """What tests/test_posterior_hess._check reads, from orc.eval_model_hess at the rows `points` of xq (all by default): mu (from
    joint_reference: the first-order mean is part of it), sig, d2mudx2, d2sigdx2 [nx, ...] (NaN rows where not asked), varK."""
    nx, d = xq.shape
    m = oracle_model(jm)
    ref = dict(mu=joint_reference(jm, xq, False)[0], sig=np.full(nx, np.nan), varK=jm.varK, dsigdx=np.full((nx, d), np.nan),
               d2mudx2=np.full((nx, d, d), np.nan), d2sigdx2=np.full((nx, d, d), np.nan))
    for j in (range(nx) if points is None else points):
        o = orc.eval_model_hess(m, xq[j])
        ref["sig"][j], ref["dsigdx"][j], ref["d2mudx2"][j], ref["d2sigdx2"][j] = o[1][0], o[3][0], o[4][0], o[5][0]
    return ref


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_listed_exported():
    from gpgradpy_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpgrad.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpg_[a-z_]+)\s*\(", txt))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/gpgrad.h"
        assert s in _lib.ABI_SYMBOLS, f"{s} is not listed in _lib.ABI_SYMBOLS"
        assert hasattr(lib, s), f"{s} is not exported by the library"


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_block_reference_reproduces_fixture_and_oracle_hessian(name):
    jm = joint_model(name)
    c, xq = jm.c, jm.c["xq"]
    nx, d = xq.shape
    _, blk, K0 = block_reference(jm, xq)
    assert blk.shape == (nx, d + 1, d + 1) and K0.shape == (nx, d + 1)
    sig = np.sqrt(np.maximum(blk[:, 0, 0], 0.0))
    want = c["sig"][:, None] * c["dsigdx"]
    np.testing.assert_allclose(sig, c["sig"], rtol=tol.SIG_RTOL, atol=tol.SIG_ATOL_SCALE * np.sqrt(jm.varK))
    np.testing.assert_allclose(blk[:, 0, 1:], want, rtol=tol.DSIG_RTOL, atol=tol.DSIG_RTOL * max(1e-12, np.abs(want).max()))
    # d2sig2 from the block against the oracle's Hessian of sig
    m = oracle_model(jm)
    worst = 0.0
    for j in range(nx):
        o = orc.eval_model_hess(m, xq[j])
        sg, dsg, d2sg = o[1][0], o[3][0], o[5][0]
        if sg == 0.0:
            continue
        Kg = orc.kern_grad(m.X, xq[j:j + 1], m.theta, m.kernel, grad_cols=True, mask1=m.grad_mask if m.use_grad else None)
        if not m.use_grad:
            Kg = Kg[:m.X.shape[0], :]
        H2 = orc.kern_hess_x(xq[j], m.X, m.theta, m.kernel, m.use_grad, m.grad_mask) @ cho_solve(m.chofac, Kg[:, :1])[:, 0]
        K0gg = orc.kern_grad(xq[j:j + 1], xq[j:j + 1], m.theta, m.kernel, grad_cols=True)[1:, 1:]
        T = K0gg - blk[j, 1:, 1:] / jm.varK
        lhs = -2.0 * jm.varK * (H2 + T)
        rhs = 2.0 * sg * d2sg + 2.0 * np.outer(dsg, dsg)
        s = np.sqrt(K0[j, 1:])
        worst = max(worst, float(np.max(np.abs(lhs - rhs) / (2.0 * jm.varK * np.outer(s, s)))))
    print(f"{name}: |-2 varK (H2 + T) - d2sig2 of the oracle| = {worst / E_BOUND:.2e} of 2 E_BOUND varK sqrt(K0_ii K0_kk)")
    assert worst <= E_BOUND


# ---- gpgradpy_amd/second.py --------------------------------------------------------------------------------------------------------
def _hand_made():
    from gpgradpy_amd.second import second_from_blocks
    mu = np.array([1.0, -2.0])
    dmudx = np.array([[3.0, 4.0], [0.0, -1.0]])
    cov = np.zeros((2, 3, 3))
    cov[0] = [[4.0, 1.0, -2.0], [1.0, 2.0, 0.5], [-2.0, 0.5, 3.0]]
    cov[1] = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 9.0]]           # sig = 0 and no variance along x_0
    return second_from_blocks(mu, dmudx, cov)


def test_second_from_blocks():
    from gpgradpy_amd.second import second_from_blocks
    r = _hand_made()
    np.testing.assert_array_equal(r.sig, [2.0, 0.0])
    np.testing.assert_array_equal(r.dsigdx, [[0.5, -1.0], [0.0, 0.0]])       # 0 where sig == 0, as eval_model
    np.testing.assert_allclose(r.grad_std, [[np.sqrt(2.0), np.sqrt(3.0)], [0.0, 3.0]], rtol=1e-15)
    assert r.d2mudx2 is None and r.d2sigdx2 is None
    assert set(r.fields) == {"mu", "sig", "dmudx", "dsigdx", "cov", "grad_std", "d2mudx2", "d2sigdx2"}
    with pytest.raises(ValueError):
        second_from_blocks(np.zeros(2), np.zeros((2, 3)), np.zeros((2, 3, 3)))


def test_expected_sq_grad_norm_and_active_subspace():
    from gpgradpy_amd.second import active_subspace, expected_sq_grad_norm
    r = _hand_made()
    np.testing.assert_allclose(expected_sq_grad_norm(r), [25.0 + 5.0, 1.0 + 9.0], rtol=1e-15)
    Cm, lam, vec = active_subspace(r)
    want = 0.5 * (np.array([[9.0, 12.0], [12.0, 16.0]]) + np.array([[0.0, 0.0], [0.0, 1.0]])
                  + np.array([[2.0, 0.5], [0.5, 3.0]]) + np.array([[0.0, 0.0], [0.0, 9.0]]))
    np.testing.assert_allclose(Cm, want, rtol=1e-15)
    assert lam[0] >= lam[1] and np.isclose(lam.sum(), np.trace(want))
    np.testing.assert_allclose((vec * lam) @ vec.T, want, rtol=1e-13, atol=1e-13)


def test_prob_descent():
    from gpgradpy_amd.second import prob_descent
    r = _hand_made()
    phi = lambda z: 0.5 * (1.0 + erf(z / sqrt(2.0)))  # noqa: E731
    p = prob_descent(r, np.array([1.0, 0.0]))
    # point 0: slope 3, variance 2; point 1: variance 0 along x_0 and slope 0 -> 1/2
    np.testing.assert_allclose(p, [phi(-3.0 / np.sqrt(2.0)), 0.5], rtol=1e-15)
    p = prob_descent(r, np.array([[-1.0, -1.0], [1.0, 0.0]]))
    np.testing.assert_allclose(p[0], phi(7.0 / np.sqrt(2.0 + 3.0 + 1.0)), rtol=1e-15)
    r.dmudx = np.array([[3.0, 4.0], [-2.0, -1.0]])                           # zero variance, negative slope: certainly descent
    assert prob_descent(r, np.array([1.0, 0.0]))[1] == 1.0
    assert prob_descent(r, np.array([-1.0, 0.0]))[1] == 0.0
    np.testing.assert_allclose(prob_descent(r, np.array([0.0, 1.0]))[1], phi(1.0 / 3.0), rtol=1e-15)
    with pytest.raises(ValueError):
        prob_descent(r, np.zeros(3))
