"""Leave-one-out cross-validation (gpg_loo / GaussianProcess.loo_cv): the parts that need no device.

The yardstick of tests/test_gpu_loo.py is loo_reference() below -- brute force: for every point delete its rows from
Kcov = (P L)(P L)' (the factor of tests/test_joint_host.joint_model), factorise the rest in NumPy and predict the deleted rows,
    e_ref = r_I - K_IJ K_JJ^-1 r_J,   C_ref = varK (K_II - K_IJ K_JJ^-1 K_JI),   r = Kcov alpha = y - V beta,
and with mean_unc the universal-kriging form: beta by GLS on the remaining rows, the residual against that mean, and
C_ref += varK U H_J^-1 U', U = V_I - K_IJ K_JJ^-1 V_J, H_J = V_J' K_JJ^-1 V_J.

Second CPU route, loo_blocks_numpy(): the block formulas the device uses (include/gpgrad.h) from a dense cho_solve(chofac, I).

Metrics, the project's prior-normalised form with E_BOUND = 2e-7 of tests/test_joint_host.py:
    E_e = max_r |e - e_ref|_r / sqrt(varK Kcov_rr),     E_C = max_ij |C - C_ref|_ij / (varK sqrt(Kcov_ii Kcov_jj)).

Checked here, and every figure printed (pytest -s):
  * the two CPU routes agree to E_BOUND / 10 in both metrics and both modes on every fixture of FIXTURES, so the bound of the
    device tests cannot hide the yardstick's own error.  Measured: E_e <= 1.4e-9 (SqExp_none_n5_d2), E_C <= 5.4e-11
    (linmean_RatQu_none_n14_d3).  The gradient-free fixtures SqExp_none_n50_d2_nograd, RatQu_none_n40_d2_nograd and
    Ma5f2_known_n50_d2_nograd are NOT used: cond(Kcov) >= 2e17 there, the refits are not positive definite and the CPU routes
    disagree by up to O(1).
  * gpgradpy_amd.loo on NumPy inputs: ln_pseudo_lkd_pt against scipy.stats.multivariate_normal.logpdf of the brute-force mean
    and covariance, z'z = e' C^-1 e, by='row' against single-row deletion, and a NaN block stays NaN, is counted, and makes
    the total NaN instead of being left out of a finite sum.
  * gpg_loo is declared in include/gpgrad.h, listed in _lib.ABI_SYMBOLS and exported by the built library.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve
from scipy.stats import multivariate_normal

from conftest import ROOT
from test_joint_host import E_BOUND, joint_model
from test_meanunc_host import aug_vand

FIXTURES = ("SqExp_none_n5_d2", "SqExp_none_n64_d8", "SqExp_none_n200_d4", "Ma5f2_known_n17_d4", "RatQu_unknown_n12_d3",
            "SqExp_unknown_n40_d5_mask", "Ma5f2_known_n23_d3_mask", "SqExp_none_n20_d2_neardup", "Ma5f2_known_n130_d8",
            "linmean/linmean_Ma5f2_known_n40_d4", "linmean/linmean_RatQu_none_n14_d3", "linmean/linmean_SqExp_none_n12_d3",
            "linmean/linmean_SqExp_none_n17_d4_mask", "linmean/linmean_SqExp_none_n30_d2_nograd", "linmean/linmean_SqExp_none_n9_d16")
SMALL = ("SqExp_none_n5_d2", "RatQu_unknown_n12_d3")
NEW_SYMBOLS = ("gpg_loo",)
CPU_BOUND = E_BOUND / 10


class LooProblem:
    """Dense pieces of one fixture: Kcov, r = y - V beta, V, y, the rows of every point."""

    def __init__(self, jm):
        from gpgradpy_amd.loo import point_rows
        c = jm.c
        PL = np.tril(jm.chofac[0]) if jm.chofac[1] else np.triu(jm.chofac[0]).T
        self.Kcov = PL @ PL.T
        self.N = self.Kcov.shape[0]
        self.varK = jm.varK
        self.r = self.Kcov @ jm.alpha
        self.V = aug_vand(jm)
        self.y = self.r + self.V @ np.ravel(jm.beta)[:self.V.shape[1]]
        self.rows = point_rows(c["n"], c["d"], bool(c["use_grad"]), jm.mask)
        self.n, self.bs = self.rows.shape
        self.kd = np.sqrt(np.diag(self.Kcov))
        assert self.V.shape[0] == self.N and jm.alpha.shape == (self.N,)
        assert sorted(self.rows[self.rows >= 0].tolist()) == list(range(self.N))


_PROBLEMS, _REFS, _ROW_REFS = {}, {}, {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = LooProblem(joint_model(name))
    return _PROBLEMS[name]


def _delete_and_predict(p, I, mean_unc_modes=(False, True)):
    """{mode: (e [|I|], C [|I|, |I|])} for the rows I left out, by refitting on the others."""
    J = np.setdiff1d(np.arange(p.N), I)
    K = p.Kcov
    fac = cho_factor(K[np.ix_(J, J)], lower=True)
    nb = p.V.shape[1]
    S = cho_solve(fac, np.column_stack([p.r[J], p.y[J], p.V[J], K[np.ix_(J, I)]]))
    KIJ = K[np.ix_(I, J)]
    C0 = K[np.ix_(I, I)] - KIJ @ S[:, 2 + nb:]
    C0 = 0.5 * (C0 + C0.T)
    out = {}
    if False in mean_unc_modes:
        out[False] = (p.r[I] - KIJ @ S[:, 0], p.varK * C0)
    if True in mean_unc_modes:
        HJ = p.V[J].T @ S[:, 2:2 + nb]
        hfac = cho_factor(0.5 * (HJ + HJ.T), lower=True)
        beta = cho_solve(hfac, p.V[J].T @ S[:, 1])                                  # GLS on the remaining rows
        U = p.V[I] - KIJ @ S[:, 2:2 + nb]
        e = (p.y[I] - p.V[I] @ beta) - KIJ @ (S[:, 1] - S[:, 2:2 + nb] @ beta)
        T = U @ cho_solve(hfac, U.T)
        out[True] = (e, p.varK * (C0 + 0.5 * (T + T.T)))
    return out


def loo_reference(jm_or_name, mean_unc):
    """(e_ref [N] in data_vec order, C_ref [n, bs, bs], zeros outside the live rows) by brute force; cached per fixture."""
    name = jm_or_name if isinstance(jm_or_name, str) else jm_or_name.c["name"]
    if name not in _REFS:
        p = problem(_fixture_key(name))
        e = {m: np.full(p.N, np.nan) for m in (False, True)}
        C = {m: np.zeros((p.n, p.bs, p.bs)) for m in (False, True)}
        for a in range(p.n):
            I = p.rows[a][p.rows[a] >= 0]
            for m, (ea, Ca) in _delete_and_predict(p, I).items():
                e[m][I] = ea
                C[m][a, :I.size, :I.size] = Ca
        _REFS[name] = (e, C)
    e, C = _REFS[name]
    return e[bool(mean_unc)], C[bool(mean_unc)]


def _fixture_key(name):
    for f in FIXTURES:
        if f == name or f.split("/")[-1] == name:
            return f
    raise KeyError(name)


def row_reference(name, mean_unc):
    """(e_ref [N], var_ref [N]): every single row deleted on its own."""
    key = (name, bool(mean_unc))
    if key not in _ROW_REFS:
        p = problem(name)
        e, v = np.empty(p.N), np.empty(p.N)
        for r in range(p.N):
            er, Cr = _delete_and_predict(p, np.array([r]), (bool(mean_unc),))[bool(mean_unc)]
            e[r], v[r] = er[0], Cr[0, 0]
        _ROW_REFS[key] = (e, v)
    return _ROW_REFS[key]


def loo_blocks_numpy(name, mean_unc):
    """The block formulas of gpg_loo from a dense inverse: (resid [N], cov [n, bs, bs], prec [n, bs, bs], qy [N])."""
    jm, p = joint_model(name), problem(name)
    B = cho_solve(jm.chofac, np.eye(p.N))
    B = 0.5 * (B + B.T)
    qy = jm.alpha.copy()
    if mean_unc:
        BV = B @ p.V
        hfac = cho_factor(p.V.T @ BV, lower=True)
        B = B - BV @ cho_solve(hfac, BV.T)
        B = 0.5 * (B + B.T)
        qy = jm.alpha - BV @ cho_solve(hfac, p.V.T @ jm.alpha)
    resid = np.full(p.N, np.nan)
    cov, prec = np.zeros((p.n, p.bs, p.bs)), np.zeros((p.n, p.bs, p.bs))
    for a in range(p.n):
        I = p.rows[a][p.rows[a] >= 0]
        Pa = B[np.ix_(I, I)]
        prec[a, :I.size, :I.size] = Pa
        fac = cho_factor(Pa, lower=True)
        resid[I] = cho_solve(fac, qy[I])
        Ci = cho_solve(fac, np.eye(I.size))
        cov[a, :I.size, :I.size] = p.varK * 0.5 * (Ci + Ci.T)
    return resid, cov, prec, qy


def err_e(p, e, e_ref):
    return float(np.max(np.abs(e - e_ref) / (np.sqrt(p.varK) * p.kd)))


def err_c(p, C, C_ref):
    worst = 0.0
    for a in range(p.n):
        I = p.rows[a][p.rows[a] >= 0]
        m = I.size
        worst = max(worst, float(np.max(np.abs(C[a, :m, :m] - C_ref[a, :m, :m]) / (p.varK * np.outer(p.kd[I], p.kd[I])))))
    return worst


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


# ---- the yardstick is sharp ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_routes_agree(name):
    p = problem(name)
    for mean_unc in (False, True):
        e_ref, C_ref = loo_reference(name, mean_unc)
        resid, cov, _, _ = loo_blocks_numpy(name, mean_unc)
        Ee, Ec = err_e(p, resid, e_ref), err_c(p, cov, C_ref)
        print(f"{name} mean_unc={mean_unc}: N = {p.N}  E_e = {Ee:.2e}  E_C = {Ec:.2e}")
        assert Ee <= CPU_BOUND and Ec <= CPU_BOUND


def test_point_rows_layout():
    from gpgradpy_amd.loo import point_rows
    assert point_rows(3, 2, False).tolist() == [[0], [1], [2]]
    assert point_rows(3, 2, True).tolist() == [[0, 3, 6], [1, 4, 7], [2, 5, 8]]
    assert point_rows(4, 2, True, [True, False, True, False]).tolist() == [[0, 4, 6], [1, -1, -1], [2, 5, 7], [3, -1, -1]]
    with pytest.raises(ValueError):
        point_rows(3, 2, True, [True, False])


# ---- gpgradpy_amd.loo on NumPy inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("SqExp_none_n5_d2", "RatQu_unknown_n12_d3", "Ma5f2_known_n23_d3_mask",
                                  "linmean/linmean_SqExp_none_n30_d2_nograd"))
def test_point_scores_against_scipy(name):
    from gpgradpy_amd.loo import loo_by_point
    p = problem(name)
    for mean_unc in (False, True):
        e_ref, C_ref = loo_reference(name, mean_unc)
        res = loo_by_point(p.y, p.rows, e_ref, C_ref)
        assert res.n_bad == 0 and res.cov is not None
        total = 0.0
        for a in range(p.n):
            I = p.rows[a][p.rows[a] >= 0]
            m = I.size
            Ca = C_ref[a, :m, :m]
            want = multivariate_normal.logpdf(p.y[I], mean=p.y[I] - e_ref[I], cov=Ca)
            total += want
            np.testing.assert_allclose(res.ln_pseudo_lkd_pt[a], want, rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(res.z[a, :m] @ res.z[a, :m], e_ref[I] @ np.linalg.solve(Ca, e_ref[I]), rtol=1e-8)
            assert np.all(np.isnan(res.z[a, m:]))
            np.testing.assert_array_equal(res.resid_f[a], e_ref[I[0]])
            np.testing.assert_array_equal(res.mu_f[a], p.y[I[0]] - e_ref[I[0]])
            if p.bs > 1:
                if m > 1:
                    np.testing.assert_array_equal(res.resid_g[a], e_ref[I[1:]])
                    np.testing.assert_array_equal(res.mu_g[a], p.y[I[1:]] - e_ref[I[1:]])
                else:
                    assert np.all(np.isnan(res.resid_g[a])) and np.all(np.isnan(res.mu_g[a]))
        if p.bs == 1:
            assert res.mu_g is None and res.resid_g is None
        np.testing.assert_allclose(res.ln_pseudo_lkd, total, rtol=1e-10)


@pytest.mark.parametrize("name", SMALL)
def test_by_row_against_single_row_deletion(name):
    from gpgradpy_amd.loo import loo_by_row
    p = problem(name)
    for mean_unc in (False, True):
        e_ref, v_ref = row_reference(name, mean_unc)
        _, _, prec, qy = loo_blocks_numpy(name, mean_unc)
        res = loo_by_row(p.y, p.rows, prec, qy, p.varK)
        Ee = float(np.max(np.abs(res.resid - e_ref) / (np.sqrt(p.varK) * p.kd)))
        Ev = float(np.max(np.abs(res.var - v_ref) / (p.varK * p.kd ** 2)))
        print(f"{name} mean_unc={mean_unc} by row: E_e = {Ee:.2e}  E_var = {Ev:.2e}")
        assert Ee <= CPU_BOUND and Ev <= CPU_BOUND and res.n_bad == 0
        np.testing.assert_allclose(res.mu, p.y - res.resid, rtol=0, atol=0)
        np.testing.assert_allclose(res.z, res.resid / np.sqrt(res.var), rtol=1e-15)
        want = np.array([multivariate_normal.logpdf(p.y[r], mean=p.y[r] - e_ref[r], cov=v_ref[r]) for r in range(p.N)])
        np.testing.assert_allclose(res.ln_pseudo_lkd_row, want, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(res.ln_pseudo_lkd, res.ln_pseudo_lkd_row.sum(), rtol=1e-14)


def test_bad_block_stays_nan_and_is_counted():
    from gpgradpy_amd.loo import loo_by_point, loo_by_row
    name = "RatQu_unknown_n12_d3"
    p = problem(name)
    resid, cov, prec, qy = loo_blocks_numpy(name, False)
    good = loo_by_point(p.y, p.rows, resid, cov)
    assert good.n_bad == 0 and np.isfinite(good.ln_pseudo_lkd)
    I = p.rows[3]
    resid_b, cov_b = resid.copy(), cov.copy()
    resid_b[I] = np.nan                                        # what the device writes for a bad block
    cov_b[3] = np.nan
    cov_b[7] = -cov_b[7]                                       # finite but not positive definite: caught on the host
    res = loo_by_point(p.y, p.rows, resid_b, cov_b)
    assert res.n_bad == 2
    for a in (3, 7):
        assert np.isnan(res.ln_pseudo_lkd_pt[a]) and np.all(np.isnan(res.z[a])) and np.isnan(res.resid_f[a]) and np.isnan(res.mu_f[a])
        assert np.all(np.isnan(res.resid_g[a])) and np.all(np.isnan(res.mu_g[a]))
    keep = np.setdiff1d(np.arange(p.n), (3, 7))
    np.testing.assert_array_equal(res.ln_pseudo_lkd_pt[keep], good.ln_pseudo_lkd_pt[keep])
    assert np.isnan(res.ln_pseudo_lkd)                         # not a finite total without the bad points
    prec_b = prec.copy()
    prec_b[2, 1, 1] = np.nan
    prec_b[4, 0, 0] = -1.0
    rr = loo_by_row(p.y, p.rows, prec_b, qy, p.varK)
    assert rr.n_bad == 2 and np.isnan(rr.ln_pseudo_lkd)
    assert np.isnan(rr.resid[p.rows[2, 1]]) and np.isnan(rr.var[p.rows[4, 0]]) and np.isnan(rr.ln_pseudo_lkd_row[p.rows[4, 0]])
    assert np.sum(np.isnan(rr.ln_pseudo_lkd_row)) == 2
