"""Joint posterior (gpg_predict_joint / eval_model_joint / sample_posterior): the parts that need no device.

* ABI: the two new symbols are declared in include/gpgrad.h, listed in _lib.ABI_SYMBOLS and exported by the built library.
* The yardstick of tests/test_gpu_joint.py -- joint_reference() below, built from the unchanged oracle -- reproduces what the
  fixtures store from the reference: sqrt(diag) against `sig` and Cov(f_j, d f_j / d x_k) against sig * dsigdx
  (d Var f = 2 Cov(f, d f)), with the SIG_* / DSIG_RTOL rules of tests/tolerances.py; the gradient rows of its mean against dmudx.
* gpgradpy_amd.joint.draw_from_joint on oracle-built (mean, cov): z = I reproduces cov to 1e-10 lambda_max -- the negative
  eigenvalues it clips on these inputs are rounding (at most 7.5e-13 lambda_max in magnitude, printed below), so the cap is
  kept by the reference on its own --, an indefinite input is clipped and stays finite, shapes, and a z of the wrong width raises.
  The comparison is with the symmetric part of cov_ref: Kg' cho_solve(., Kg) is not symmetric in floating point, and on the
  near-duplicate fixture, where varK (Kqq - ...) cancels by 1e4, cov_ref - cov_ref' reaches 6.7e-9 lambda_max.  A draw
  reproduces a symmetric matrix, so no draw_from_joint can come closer than half of that to the unsymmetrised array (measured
  3.3e-9 lambda_max there, 3.0e-11 and 1.2e-13 on the other two); against the symmetric part all three are at 2.9e-13
  lambda_max or below.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

import tolerances as tol
from conftest import GOLDEN_DIR, ROOT, load_case
from oracle import gp_oracle as orc

PARITY = ("SqExp_none_n5_d2", "SqExp_none_n64_d8", "SqExp_none_n200_d4", "Ma5f2_known_n17_d4", "RatQu_unknown_n12_d3",
          "SqExp_unknown_n40_d5_mask", "Ma5f2_known_n23_d3_mask", "SqExp_none_n50_d2_nograd", "RatQu_none_n40_d2_nograd",
          "SqExp_none_n20_d2_neardup", "linmean/linmean_Ma5f2_known_n40_d4")
NEW_SYMBOLS = ("gpg_predict_joint", "gpg_set_gram_splits")
E_BOUND = 2e-7            # max |cov - cov_ref|_ij / (varK sqrt(Kqq_ii Kqq_jj)): SIG_ATOL_SCALE on sig is <= 2e-7 on the normalised variance


def case(name):
    return load_case(os.path.join(GOLDEN_DIR, name + ".npz"))


class JointModel:
    """What the reference keeps after setup_eval_model, from the oracle: factor of Kcov (varK = 1), alpha, beta, varK."""

    def __init__(self, c):
        self.c = c
        self.linear = c["name"].startswith("linmean")
        self.mask = None if (not c["use_grad"] or c["bvec_use_grad"].all()) else c["bvec_use_grad"]
        if self.linear:
            from test_linmean_golden import dense_linmean
            r = dense_linmean(c)
            self.chofac = cho_factor(r["Kcov_model"], lower=True)
            self.alpha, self.beta, self.varK = r["alpha"], r["beta"], float(r["varK"])
            return
        # exactly as tests/test_oracle_golden.py
        y = orc.make_data_vec(c["f"], c["g"] if c["use_grad"] else None)
        vf = None if np.isnan(c["var_fval"]) else c["var_fval"]
        vg = None if np.isnan(c["var_fgrad"]) else c["var_fgrad"]
        nv = orc.calc_noise_vec(c["n"], c["d"], c["use_grad"], c["std_f"], c["std_g"] if c["use_grad"] else None, vf, vg,
                                n_grad=int(c["bvec_use_grad"].sum()))
        noisy = c["b_has_noisy_data"]
        wc = c["wellcond"] if c["use_grad"] else "base"
        r = orc.calc_lkd(c["x"], y, c["theta"], c["kernel_o"], c["use_grad"], wc, c["etaK"], nv, noisy,
                         varK=c["varK_in"] if noisy else None, grad_mask=self.mask)
        assert r.ok
        self.varK = float(c["varK_in"] if noisy else r.hp_varK)
        m = orc.setup_eval_model(c["x"], y, c["theta"], c["kernel_o"], c["use_grad"], wc, c["etaK"], nv, r.hp_beta, self.varK, self.mask)
        self.chofac, self.alpha, self.beta = m.chofac, m.alpha, np.ravel(r.hp_beta)


_MODELS = {}


def joint_model(name):
    if name not in _MODELS:
        _MODELS[name] = JointModel(case(name))
    return _MODELS[name]


def joint_reference(jm, xq, calc_grad=True):
    """(mean_ref [m], cov_ref [m, m], Kqq [m, m]) in the derivative-major row order of gpg_predict_joint."""
    c = jm.c
    nx, d = xq.shape
    Kg = orc.kern_grad(c["x"], xq, c["theta"], c["kernel_o"], grad_cols=True, mask1=jm.mask)
    if not c["use_grad"]:
        Kg = Kg[:c["n"]]
    Kqq = orc.kern_grad(xq, xq, c["theta"], c["kernel_o"], grad_cols=True)
    if not calc_grad:
        Kg, Kqq = Kg[:, :nx], Kqq[:nx, :nx]
    cov = jm.varK * (Kqq - Kg.T @ cho_solve(jm.chofac, Kg))
    mean = Kg.T @ jm.alpha
    mean[:nx] += jm.beta[0] + (xq @ jm.beta[1:] if jm.linear else 0.0)
    if jm.linear and calc_grad:
        mean[nx:] += np.repeat(jm.beta[1:], nx)
    return mean, cov, Kqq


def joint_error(cov, cov_ref, Kqq, varK):
    s = np.sqrt(np.diag(Kqq))
    return float(np.max(np.abs(cov - cov_ref) / (varK * np.outer(s, s))))


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


# ---- the yardstick reproduces the reference's stored outputs --------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_reference_construction_satisfies_fixture_identities(name):
    jm = joint_model(name)
    c, xq = jm.c, jm.c["xq"]
    nx, d = xq.shape
    mean, cov, Kqq = joint_reference(jm, xq)
    assert cov.shape == (nx * (d + 1),) * 2 and np.max(np.abs(cov - cov.T)) <= 1e-12 * jm.varK
    np.testing.assert_allclose(jm.varK, c["varK_model"], rtol=tol.VARK_RTOL)
    sig = np.sqrt(np.maximum(np.diag(cov)[:nx], 0.0))
    j = np.arange(nx)
    half_dvar = np.stack([cov[j, (k + 1) * nx + j] for k in range(d)], axis=1)          # [nx, d]
    want = c["sig"][:, None] * c["dsigdx"]
    g_rows = mean[nx:].reshape(d, nx).T
    print(f"{name}: sig {np.max(np.abs(sig - c['sig'])) / np.sqrt(jm.varK):.2e} sqrt(varK)   "
          f"sig dsigdx {np.max(np.abs(half_dvar - want)) / max(1e-300, np.abs(want).max()):.2e} of max   "
          f"dmudx {np.max(np.abs(g_rows - c['dmudx'])) / np.abs(c['dmudx']).max():.2e} of max")
    np.testing.assert_allclose(sig, c["sig"], rtol=tol.SIG_RTOL, atol=tol.SIG_ATOL_SCALE * np.sqrt(jm.varK))
    np.testing.assert_allclose(half_dvar, want, rtol=tol.DSIG_RTOL, atol=tol.DSIG_RTOL * max(1e-12, np.abs(want).max()))
    np.testing.assert_allclose(mean[:nx], c["mu"], rtol=tol.MU_RTOL, atol=tol.MU_ATOL_SCALE * max(1.0, np.abs(c["mu"]).max()))
    np.testing.assert_allclose(g_rows, c["dmudx"], rtol=tol.DMU_RTOL, atol=tol.DMU_RTOL * max(1e-12, np.abs(c["dmudx"]).max()))


# ---- draw_from_joint -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("SqExp_none_n5_d2", "RatQu_unknown_n12_d3", "SqExp_none_n20_d2_neardup"))
def test_draw_identity_normals_reproduce_cov(name):
    from gpgradpy_amd.joint import draw_from_joint
    jm = joint_model(name)
    mean, cov, _ = joint_reference(jm, jm.c["xq"])
    m = mean.size
    lam = np.linalg.eigvalsh(0.5 * (cov + cov.T))
    print(f"{name}: most negative eigenvalue {min(lam.min(), 0.0) / lam.max():.2e} lambda_max")
    D = draw_from_joint(mean, cov, np.eye(m)) - mean
    assert D.shape == (m, m)
    sym = 0.5 * (cov + cov.T)
    print(f"{name}: |D'D - sym(cov_ref)| {np.max(np.abs(D.T @ D - sym)) / lam.max():.2e}   |D'D - cov_ref| "
          f"{np.max(np.abs(D.T @ D - cov)) / lam.max():.2e}   asymmetry of cov_ref {np.max(np.abs(cov - cov.T)) / lam.max():.2e}   (lambda_max)")
    assert np.max(np.abs(D.T @ D - sym)) <= 1e-10 * lam.max()
    np.testing.assert_array_equal(draw_from_joint(mean, cov, np.zeros((3, m))), np.tile(mean, (3, 1)))


def test_draw_clips_an_indefinite_input():
    from gpgradpy_amd.joint import draw_from_joint
    V = np.linalg.qr(np.random.default_rng(0).standard_normal((3, 3)))[0]
    cov = (V * np.array([2.0, 0.5, -0.3])) @ V.T
    s = draw_from_joint(np.zeros(3), cov, np.eye(3))
    assert np.all(np.isfinite(s))
    np.testing.assert_allclose(s.T @ s, (V * np.array([2.0, 0.5, 0.0])) @ V.T, atol=1e-14)


def test_draw_shapes_and_wrong_width():
    from gpgradpy_amd.joint import draw_from_joint
    jm = joint_model("SqExp_none_n5_d2")
    xq = jm.c["xq"]
    nx, d = xq.shape
    z = np.random.default_rng(1).standard_normal((5, nx * (d + 1)))
    for calc_grad, m in ((False, nx), (True, nx * (d + 1))):
        mean, cov, _ = joint_reference(jm, xq, calc_grad)
        assert mean.shape == (m,) and cov.shape == (m, m)
        assert draw_from_joint(mean, cov, z[:, :m]).shape == (5, m)
        with pytest.raises(ValueError):
            draw_from_joint(mean, cov, z[:, :m - 1])
    with pytest.raises(ValueError):
        draw_from_joint(np.zeros(3), np.eye(4), np.zeros((2, 3)))
