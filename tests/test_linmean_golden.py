"""First-order polynomial mean ('poly_ord_1'): the fixtures captured from the reference (tests/golden/gen_golden_linmean.py,
stored under tests/golden/linmean/) against a dense NumPy restatement -- Kcov and its factor from
oracle.gp_oracle.calc_all_K_w_chofac, V = calc_aug_vand (GpMeanFun.py:172-191), the reference's GLS for beta
(GpMeanFun.py:98-107) and the scalar formulas of CalcLkd.py:149-168 / 220-226.  CPU only.

This pins the fixtures and measures how much two CPU paths disagree; every figure is printed before it is asserted
(pytest -s).  Measured (largest over the six fixtures, all on linmean_SqExp_none_n30_d2_nograd or linmean_RatQu_none_n14_d3;
next to each the constant of tests/tolerances.py it is held to):
    beta normwise 2.8e-10 (BETA_RTOL 1e-8), ln_lkd 1.6e-10 rel (LN_LKD_RTOL 1e-8), ln_det 2.9e-8 abs (LN_DET_ATOL 2e-6),
    varK 2.3e-10 (VARK_RTOL 1e-8), alpha normwise 2.8e-8 (ALPHA_NORMWISE 1e-5), mu 3.7e-3 of its bound, sig 8.0e-5 of its bound;
    affine shift through the dense restatement (n40_d4 data): beta moves by (c0, c) to 1.3e-16 normwise, ln_lkd 3.8e-16,
    alpha 3.1e-14, sig unchanged to the last bit.
None is above a tenth of its constant, so the GPU tests (tests/test_gpu_linmean.py) use the constants unchanged.
"""
import glob
import os

import numpy as np
import pytest
from scipy.linalg import cho_solve

import tolerances as tol
from conftest import GOLDEN_DIR, load_case

LINMEAN_DIR = os.path.join(GOLDEN_DIR, "linmean")
CASES = sorted(p for p in glob.glob(os.path.join(LINMEAN_DIR, "linmean_*.npz")) if "_optz_" not in os.path.basename(p))
EXPECTED = ("linmean_Ma5f2_known_n40_d4", "linmean_RatQu_none_n14_d3", "linmean_SqExp_none_n12_d3", "linmean_SqExp_none_n17_d4_mask",
            "linmean_SqExp_none_n30_d2_nograd", "linmean_SqExp_none_n9_d16")


def case_name(path):
    return os.path.basename(path)[:-4]


def aug_vand(x, use_grad, mask=None):
    """calc_aug_vand with n_beta_coeff = d + 1 (GpMeanFun.py:124-191): value row a: [1, x_a]; gradient row (i, a): e_(i+1);
    rows of masked points left out."""
    n, d = x.shape
    ng = n if mask is None else int(np.sum(mask))
    V = np.zeros((n + (ng * d if use_grad else 0), d + 1))
    V[:n, 0] = 1.0
    V[:n, 1:] = x
    if use_grad:
        for i in range(d):
            V[n + i * ng:n + (i + 1) * ng, i + 1] = 1.0
    return V


def dense_linmean(c, f=None, g=None, xq=None):
    """The likelihood and the posterior of fixture c (optionally with other values f / gradients g) with dense NumPy / SciPy."""
    from oracle import gp_oracle as orc
    f = c["f"] if f is None else f
    g = c["g"] if g is None else g
    xq = c["xq"] if xq is None else xq
    n, d, use_grad, noisy = c["n"], c["d"], c["use_grad"], c["b_has_noisy_data"]
    mask = None if (not use_grad or c["bvec_use_grad"].all()) else c["bvec_use_grad"]
    y = orc.make_data_vec(f, g if use_grad else None)
    nv = orc.calc_noise_vec(n, d, use_grad, c["std_f"], c["std_g"] if use_grad else None, None, None,
                            n_grad=int(c["bvec_use_grad"].sum()))
    wc = c["wellcond"] if use_grad else "base"
    fac = orc.calc_all_K_w_chofac(c["x"], c["theta"], c["kernel_o"], use_grad, wc, c["etaK"], nv,
                                  varK=c["varK_in"] if noisy else 1.0, grad_mask=mask)
    V = aug_vand(c["x"], use_grad, mask)
    N = y.size
    KiV = cho_solve(fac.chofac, V)
    beta = np.linalg.solve(V.T @ KiV, KiV.T) @ y                            # GpMeanFun.py:102-107
    res = y - V @ beta
    alpha_l = cho_solve(fac.chofac, res)
    ln_det = 2.0 * np.sum(np.log(np.diag(fac.chofac[0])))
    rKr = res @ alpha_l
    if noisy:
        varK, ln_lkd = c["varK_in"], -(ln_det + rKr) / 2.0                  # CalcLkd.py:226
    else:
        varK = max(1e-32, rKr / N)                                          # CalcLkd.py:159
        ln_lkd = -(N * np.log(varK) + ln_det) / 2.0                         # CalcLkd.py:168
    # posterior: matrix built with varK = 1 and the noise undivided (Kernel.py:196-197, 218), GpEvalModel.py:17-57
    fac1 = fac if not noisy else orc.calc_all_K_w_chofac(c["x"], c["theta"], c["kernel_o"], use_grad, wc, c["etaK"], nv, varK=1.0,
                                                         grad_mask=mask)
    alpha = cho_solve(fac1.chofac, res)
    if use_grad:
        Kyx = orc.kern_grad(c["x"], xq, c["theta"], c["kernel_o"], grad_cols=False, mask1=mask)
    else:
        Kyx = orc.kern_base(c["x"], xq, c["theta"], c["kernel_o"])
    sol = cho_solve(fac1.chofac, Kyx)
    sig2 = np.maximum(0.0, 1.0 - np.einsum("ij,ij->j", Kyx, sol))
    mu = beta[0] + xq @ beta[1:] + Kyx.T @ alpha                            # GpMeanFun.py:49, GpEvalModel.py:168
    return dict(beta=beta, ln_det=ln_det, ln_lkd=ln_lkd, varK=varK, alpha=alpha, alpha_lkd=alpha_l, mu=mu, sig=np.sqrt(sig2) * np.sqrt(varK),
                Kcov=fac.Kcov, Kcov_model=fac1.Kcov, V=V, y=y)


def normwise(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_fixture_set_is_complete():
    assert tuple(case_name(p) for p in CASES) == EXPECTED
    assert os.path.isfile(os.path.join(LINMEAN_DIR, "linmean_optz_SqExp_n20_d2.npz"))
    for p in glob.glob(os.path.join(LINMEAN_DIR, "*.npz")):
        assert os.path.getsize(p) <= 100 * 1024                               # what the other tests/golden/*.npz keep to


@pytest.mark.parametrize("path", CASES, ids=case_name)
def test_dense_restatement_reproduces_fixture(path):
    c = load_case(path)
    r = dense_linmean(c)
    N, noisy = c["n_data"], c["b_has_noisy_data"]
    assert c["hp_beta"].shape == (c["d"] + 1,)
    assert c["ln_lkd"] > float(c["ln_lkd_const_mean"])                       # the data carry a slope: the trend pays
    d_beta = normwise(r["beta"], c["hp_beta"])
    d_ln = abs(r["ln_lkd"] - c["ln_lkd"]) / abs(c["ln_lkd"])
    d_det = abs(r["ln_det"] - c["ln_det_Kmat"])
    d_varK = 0.0 if noisy else abs(r["varK"] - c["hp_varK"]) / c["hp_varK"]
    d_alpha = float(np.linalg.norm(r["alpha"] - c["alpha"]) / np.linalg.norm(c["alpha"]))
    mu_bound = tol.MU_RTOL * np.abs(c["mu"]) + tol.MU_ATOL_SCALE * max(1.0, np.abs(c["mu"]).max())
    sig_bound = tol.SIG_RTOL * np.abs(c["sig"]) + tol.SIG_ATOL_SCALE * np.sqrt(c["varK_model"])
    d_mu = float(np.max(np.abs(r["mu"] - c["mu"]) / mu_bound))
    d_sig = float(np.max(np.abs(r["sig"] - c["sig"]) / sig_bound))
    print(f"{c['name']}: beta {d_beta:.2e} ln_lkd {d_ln:.2e} ln_det {d_det:.2e} varK {d_varK:.2e} alpha {d_alpha:.2e} "
          f"mu/bound {d_mu:.2e} sig/bound {d_sig:.2e}")
    assert d_beta <= tol.BETA_RTOL
    assert d_ln <= tol.LN_LKD_RTOL
    assert d_det <= tol.LN_DET_ATOL + tol.LN_DET_ATOL_PER_N * N
    assert d_varK <= tol.VARK_RTOL
    assert d_alpha <= tol.ALPHA_NORMWISE
    assert d_mu <= 1.0 and d_sig <= 1.0
    # V' alpha = 0 at the GLS optimum, column by column, on the scale ALPHA_RESIDUAL is defined on.  alpha of the LIKELIHOOD's
    # matrix: with known noise the posterior's matrix is another one (built with varK = 1, Kernel.py:196-197), beta is not its optimum
    Kn, al = np.linalg.norm(r["Kcov"], 2), r["alpha_lkd"]
    for j in range(r["V"].shape[1]):
        assert abs(r["V"][:, j] @ al) <= tol.ALPHA_RESIDUAL * np.linalg.norm(r["V"][:, j]) * Kn * np.linalg.norm(al)


def affine_shift(c):
    """c0 + x . cv with the norm of the values; the same slope goes to every gradient."""
    rng = np.random.default_rng(5)
    cv, c0 = rng.standard_normal(c["d"]), rng.standard_normal()
    aff = c0 + c["x"] @ cv
    s = np.linalg.norm(c["f"]) / np.linalg.norm(aff)
    g2 = c["g"] + s * cv[None, :] if c["use_grad"] else c["g"]
    return c["f"] + s * aff, g2, np.concatenate(([s * c0], s * cv))


def test_affine_shift_dense():
    """Adding c0 + x . c to the values and c to the gradients moves beta by exactly (c0, c) and leaves the residual, hence
    ln_lkd, varK, alpha and sig, unchanged -- through the dense restatement, before the device is held to it."""
    c = load_case(os.path.join(LINMEAN_DIR, "linmean_Ma5f2_known_n40_d4.npz"))
    f2, g2, shift = affine_shift(c)
    a, b = dense_linmean(c), dense_linmean(c, f2, g2)
    d_beta = normwise(b["beta"] - shift, a["beta"])
    d_ln = abs(b["ln_lkd"] - a["ln_lkd"]) / abs(a["ln_lkd"])
    d_alpha = float(np.linalg.norm(b["alpha"] - a["alpha"]) / np.linalg.norm(a["alpha"]))
    d_sig = float(np.max(np.abs(b["sig"] - a["sig"]) / (tol.SIG_RTOL * np.abs(a["sig"]) + tol.SIG_ATOL_SCALE * np.sqrt(a["varK"]))))
    print(f"affine shift (dense): beta {d_beta:.2e} ln_lkd {d_ln:.2e} alpha {d_alpha:.2e} sig/bound {d_sig:.2e}")
    assert d_beta <= tol.BETA_RTOL and d_ln <= tol.LN_LKD_RTOL and d_alpha <= tol.ALPHA_NORMWISE and d_sig <= 1.0


def test_mirror_accepts_the_option_on_the_host():
    """Constructor contract (no device needed): 'poly_ord_1' gives d + 1 coefficients, anything else still raises."""
    import gpgradpy_amd
    GP = gpgradpy_amd.GaussianProcess(3, True, 'SqExp', 'precon', mean_fun_type='poly_ord_1')
    assert GP.n_beta_coeff == 4 and GP.beta_var_npara == 4 and GP.mean_fun_type == 'poly_ord_1'
    assert gpgradpy_amd.GaussianProcess(3, True).n_beta_coeff == 1
    with pytest.raises(Exception, match='not available'):
        gpgradpy_amd.GaussianProcess(3, True, mean_fun_type='poly_ord_2')
