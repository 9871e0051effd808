"""Uncertainty of the mean coefficients on the device (gpg_set_mean_uncertainty, gpg_mean_gram; mean_unc=True of eval_model,
eval_model_var, eval_model_joint, sample_posterior; GaussianProcess.calc_beta_cov) against meanunc_reference of
tests/test_meanunc_host.py, which that file pins to the forward-only route and to central differences on the CPU.

Metric and bound: E = max |cov - cov_ref|_ij / (varK sqrt(S_ii S_jj)), S = diag(Kqq + U H^-1 U'), E <= E_BOUND = 2e-7 (the project's
standing bound on the normalised variance; not moved to what the code gives).  Every figure is printed (pytest -s) before it is
asserted.  The sixteen fixtures cover N = 30, 48, 56, 65 (one past a 64-tile), 153 with n_beta = 17, 200, 576 and 1000, gradient
masks, gradient-free models with calc_grad=True, all three kernels, noisy and noise-free data.

Other bounds, and where they come from:
  * H = V' K^-1 V against NumPy: normwise BETA_RTOL (tests/tolerances.py), the rule the GLS coefficients formed from the same
    matrix are held to; calc_beta_cov = varK H^-1 against varK inv(H_ref): normwise n_beta cond(H_ref) BETA_RTOL, the first-order
    perturbation bound of an inverse for a BETA_RTOL perturbation of H (n_beta: max norm against 2-norm).
  * Hessian: the rule of tests/test_posterior_hess.py (eps 1e-5, rtol 1e-3, atol 1e-4 max(1, |H|max)); symmetry 1e-9 relative.
  * sampling: 1e-10 lambda_max as test_sample_posterior.

Largest values measured on an MI355X (one run of this file):
    joint parity, E: SqExp_none_n200_d4 outside 9.4e-10, SqExp_none_n20_d2_neardup outside 5.5e-10, linmean_RatQu_none_n14_d3 1.4e-10,
                SqExp_none_n50_d2_nograd 1.3e-10, every other case 1.6e-11 or less; least gain of a value row on the must-differ
                fixtures 1.24e-4 S (Ma5f2_known_n23_d3_mask) .. 0.60 S (linmean_SqExp_none_n9_d16);
    marginals: 6.5e-13 or less (SqExp_none_n64_d8, nx = 64), 2.6e-15 or less on the linear-mean fixture;
    Hessian: asymmetry 6e-17 relative, |H_k - central differences| 2.4e-8 at |H|max = 146; the switch changes d2sigdx2 by 0.23-0.31 |H|max;
    H normwise 1.8e-9 (SqExp_none_n5_d2) or less, calc_beta_cov 3.9e-9 or less; sampling |D'D - cov| = 7.4e-14 lambda_max.

All of these fail without the feature: the keyword and the symbols do not exist there.
"""
import ctypes as C

import numpy as np
import pytest

import tolerances as tol
from test_gpu_joint import _build, _no_fallbacks
from test_joint_host import E_BOUND, case, joint_model
from test_meanunc_host import (FIXTURES, MUST_DIFFER, TERM_MIN, mean_gram_reference, meanunc_error, meanunc_reference,
                               outside_points, point_sets)

pytestmark = pytest.mark.gpu

N5, N17, N64 = "SqExp_none_n5_d2", "Ma5f2_known_n17_d4", "SqExp_none_n64_d8"
LIN40, LIN12, LIN17M = ("linmean/linmean_Ma5f2_known_n40_d4", "linmean/linmean_SqExp_none_n12_d3",
                        "linmean/linmean_SqExp_none_n17_d4_mask")
_GPS = {}


def _gp(name):
    """One device model per fixture, shared by the tests of this file (every eval_* call sets the switch for itself)."""
    if name not in _GPS:
        _GPS[name] = _build(name)
    return _GPS[name]


def _wide_points(c, nx, seed):
    lo, hi = c["x"].min(axis=0), c["x"].max(axis=0)
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return ctr + 2.0 * half * np.random.default_rng(seed).uniform(-1.0, 1.0, (nx, c["d"]))


# ---- 1. joint parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_joint_parity(name):
    jm, GP = joint_model(name), _gp(name)
    varK = float(GP.hp_vals.varK)
    np.testing.assert_allclose(varK, jm.varK, rtol=tol.VARK_RTOL)
    for tag, xq in point_sets(jm):
        nx = xq.shape[0]
        mean_off, cov_off = GP.eval_model_joint(xq, True)
        mean, cov = GP.eval_model_joint(xq, True, mean_unc=True)
        _, cov_ref, S, _ = meanunc_reference(jm, xq, True)
        assert cov.shape == cov_ref.shape
        E = meanunc_error(cov, cov_ref, S, jm.varK)
        gain = (np.diag(cov - cov_off)[:nx] / (jm.varK * S[:nx])).min()
        print(f"{name} {tag}: m = {cov.shape[0]}  E = {E:.2e}  least gain of a value row {gain:.2e} S")
        assert E <= E_BOUND
        assert np.array_equal(cov, cov.T)
        assert np.array_equal(mean, mean_off)
        if tag == "outside" and name in MUST_DIFFER:
            assert gain >= TERM_MIN
    _no_fallbacks(GP)


# ---- 2. marginals: the 1-4-row vector solve against the tile sweeps, row padding -----------------------------------------------------
@pytest.mark.parametrize("name", (N64, LIN40))
@pytest.mark.parametrize("nx", (1, 4, 5, 64, 65))
def test_marginals(name, nx):
    jm, GP = joint_model(name), _gp(name)
    xq = _wide_points(jm.c, nx, 100 + nx)
    d = xq.shape[1]
    _, cov_ref, S, _ = meanunc_reference(jm, xq, True)
    j = np.arange(nx)
    var_ref = np.diag(cov_ref)[:nx]
    half_dvar_ref = np.stack([cov_ref[j, (k + 1) * nx + j] for k in range(d)], axis=1)
    s_var = jm.varK * S[:nx]
    s_dvar = jm.varK * np.stack([np.sqrt(S[j] * S[(k + 1) * nx + j]) for k in range(d)], axis=1)
    mu_off = GP.eval_model(xq, calc_grad=True)[:3:2]
    mu, sig, dmudx, dsigdx = GP.eval_model(xq, calc_grad=True, mean_unc=True)[:4]
    sig2, dsig2dx = GP.eval_model_var(xq, calc_grad=True, mean_unc=True)[:2]
    sig_only = GP.eval_model(xq, mean_unc=True)[1]
    e = (np.max(np.abs(sig ** 2 - var_ref) / s_var), np.max(np.abs(sig[:, None] * dsigdx - half_dvar_ref) / s_dvar),
         np.max(np.abs(sig2 - var_ref) / s_var), np.max(np.abs(0.5 * dsig2dx - half_dvar_ref) / s_dvar),
         np.max(np.abs(sig_only ** 2 - var_ref) / s_var))
    print(f"{name} nx={nx}: sig^2 {e[0]:.2e}  sig dsigdx {e[1]:.2e}  sig2 {e[2]:.2e}  dsig2dx / 2 {e[3]:.2e}  sig^2 (no gradients) {e[4]:.2e}")
    assert max(e) <= E_BOUND
    assert np.array_equal(mu, mu_off[0]) and np.array_equal(dmudx, mu_off[1])          # the mean does not change
    _no_fallbacks(GP)


# ---- 3. Hessian -----------------------------------------------------------------------------------------------------------------
def _hess(GP, x0, masked):
    """(dsigdx [d], d2sigdx2 [d, d]) at x0 with the switch on; a masked model goes through the C ABI (the mirror refuses Hessians
    with a mask because the reference has nothing to pin them against; the device path honours the mask)."""
    if not masked:
        out = GP.eval_model(x0, calc_grad=True, calc_hess=True, squeeze_nx=True, mean_unc=True)
        return out[3], out[5]
    from gpgradpy_amd import _lib
    d = x0.size
    GP.eval_model(x0[None, :], calc_grad=True, mean_unc=True)                      # leaves the switch on
    mu, sig, dmu, dsig, d2mu, d2sig = np.empty(1), np.empty(1), np.empty(d), np.empty(d), np.empty((d, d)), np.empty((d, d))
    x0 = np.ascontiguousarray(x0)
    rc = GP._lib.gpg_predict_hess(GP._ctx, _lib.as_dp(x0), float(GP.hp_vals.varK), _lib.as_dp(mu), _lib.as_dp(sig), _lib.as_dp(dmu),
                                  _lib.as_dp(dsig), _lib.as_dp(d2mu), _lib.as_dp(d2sig))
    assert rc == 0, GP._err()
    return dsig, d2sig


@pytest.mark.parametrize("name", (N17, LIN12, LIN17M))
def test_hessian(name):
    jm, GP = joint_model(name), _gp(name)
    masked = jm.mask is not None
    x0 = outside_points(jm.c)[0]
    d = x0.size
    dsig0, H = _hess(GP, x0, masked)
    dsig_grad = GP.eval_model(x0[None, :], calc_grad=True, mean_unc=True)[3][0]
    assert np.array_equal(dsig0, dsig_grad)
    H_off = GP.eval_model(x0, calc_grad=True, calc_hess=True, squeeze_nx=True)[5] if not masked else None
    print(f"{name}: |d2sigdx2|max = {np.abs(H).max():.3e}  asymmetry {np.abs(H - H.T).max() / np.abs(H).max():.2e}"
          + ("" if masked else f"  change by the switch {np.abs(H - H_off).max() / np.abs(H).max():.2e}"))
    np.testing.assert_allclose(H, H.T, rtol=1e-9, atol=1e-9 * np.abs(H).max())
    eps = 1e-5
    for k in range(d):
        xp, xm = x0.copy(), x0.copy()
        xp[k] += eps
        xm[k] -= eps
        gp_ = GP.eval_model(xp[None, :], calc_grad=True, mean_unc=True)
        gm_ = GP.eval_model(xm[None, :], calc_grad=True, mean_unc=True)
        fd = (gp_[3][0] - gm_[3][0]) / (2 * eps)
        print(f"{name} k={k}: |H_k - fd| = {np.abs(H[k] - fd).max():.2e}")
        np.testing.assert_allclose(H[k], fd, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(H).max()))
    _no_fallbacks(GP)


# ---- 4. isolation -------------------------------------------------------------------------------------------------------------
def _all_outputs(GP, xq, mean_unc):
    a = GP.eval_model(xq, calc_grad=True, mean_unc=mean_unc)[:4]
    b = GP.eval_model_var(xq, calc_grad=True, mean_unc=mean_unc)[:2]
    c = GP.eval_model_joint(xq, True, mean_unc=mean_unc)
    h = GP.eval_model(xq[0], calc_grad=True, calc_hess=True, squeeze_nx=True, mean_unc=mean_unc)
    return tuple(a) + tuple(b) + tuple(c) + tuple(h)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_isolation():
    name = LIN40
    jm = joint_model(name)
    GP = _build(name)                                                       # a context that never had the switch on
    xq = outside_points(jm.c)
    off0 = _all_outputs(GP, xq, False)
    on0 = _all_outputs(GP, xq, True)
    assert not _same(off0, on0)
    assert _same(off0, _all_outputs(GP, xq, False))                         # off after on: the bits from before it was ever on
    assert _same(on0, _all_outputs(GP, xq, True))                           # on -> off -> on
    for cap in (1, 3):
        GP.set_max_workgroups(cap)
        assert _same(on0, _all_outputs(GP, xq, True)), cap
    GP.set_max_workgroups(0)
    c = jm.c
    hp_other = GP.make_hp_class(theta=2.0 * c["theta"], varK=c["varK_in"] if c["b_has_noisy_data"] else None,
                                var_fval=None if np.isnan(c["var_fval"]) else c["var_fval"],
                                var_fgrad=None if np.isnan(c["var_fgrad"]) else c["var_fgrad"])
    GP.calc_lkd_all(hp_other)                                               # likelihood calls in between change nothing
    assert _same(on0, _all_outputs(GP, xq, True))
    GP.calc_lkd_all(hp_other, calc_grad=True)
    assert _same(off0, _all_outputs(GP, xq, False))
    assert _same(on0, _all_outputs(GP, xq, True))
    # another theta: the state of the old factor must not survive gpg_setup_eval
    hp2 = GP.optz_closed_form_hp(hp_other)
    GP.set_hpara('set', 0, hp_vals=hp2)
    on_new = _all_outputs(GP, xq, True)
    fresh = _build(name, setup=False)
    fresh.set_hpara('set', 0, hp_vals=fresh.optz_closed_form_hp(hp_other))
    on_fresh = _all_outputs(fresh, xq, True)
    assert _same(on_new, on_fresh)
    assert not np.array_equal(on_new[1], on0[1])
    _no_fallbacks(GP)
    _no_fallbacks(fresh)
    GP.close()
    fresh.close()


# ---- 5. gpg_mean_gram, calc_beta_cov ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_mean_gram(name):
    from gpgradpy_amd import _lib
    jm, GP = joint_model(name), _gp(name)
    H_ref = mean_gram_reference(jm)
    nb = H_ref.shape[0]
    H = np.empty((nb, nb))
    assert GP._lib.gpg_mean_gram(GP._ctx, _lib.as_dp(H)) == 0, GP._err()
    dH = np.abs(H - H_ref).max() / np.abs(H_ref).max()
    cov_ref = jm.varK * np.linalg.inv(H_ref)
    cov = GP.calc_beta_cov()
    dC = np.abs(cov - cov_ref).max() / np.abs(cov_ref).max()
    bound = nb * np.linalg.cond(H_ref) * tol.BETA_RTOL
    print(f"{name}: n_beta = {nb}  H normwise {dH:.2e}  calc_beta_cov normwise {dC:.2e} (bound {bound:.2e})")
    assert np.array_equal(H, H.T)
    assert dH <= tol.BETA_RTOL
    assert cov.shape == (nb, nb) and dC <= bound
    _no_fallbacks(GP)


# ---- 6. sampling ------------------------------------------------------------------------------------------------------------------
def test_sample_posterior():
    jm, GP = joint_model(LIN40), _gp(LIN40)
    xq = outside_points(jm.c)
    nx, d = xq.shape
    m = nx * (d + 1)
    mean, cov = GP.eval_model_joint(xq, True, mean_unc=True)
    f, g = GP.sample_posterior(xq, m, calc_grad=True, z=np.eye(m), mean_unc=True)
    D = np.concatenate([f, np.transpose(g, (0, 2, 1)).reshape(m, d * nx)], axis=1) - mean
    lam_max = np.linalg.eigvalsh(cov)[-1]
    err = np.max(np.abs(D.T @ D - cov))
    cov_off = GP.eval_model_joint(xq, True)[1]
    print(f"{LIN40}: |D'D - cov| = {err / lam_max:.2e} lambda_max   (cov - cov_off: {np.max(np.abs(cov - cov_off)) / lam_max:.2e} lambda_max)")
    assert err <= 1e-10 * lam_max
    assert np.max(np.abs(D.T @ D - cov_off)) > 1e-6 * lam_max                # the draws are those of the wider posterior
    _no_fallbacks(GP)


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------
def test_errors():
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    c = case(N5)
    xq = np.ascontiguousarray(c["xq"])
    nx = xq.shape[0]
    GP = _build(N5, setup=False)
    lib, ctx = GP._lib, GP._ctx
    assert lib.gpg_set_mean_uncertainty(ctx, 1) == 0                          # before gpg_setup_eval: accepted
    mu, sig = np.empty(nx), np.empty(nx)
    assert lib.gpg_predict(ctx, nx, _lib.as_dp(xq), 1.0, _lib.as_dp(mu), _lib.as_dp(sig), None) == -1
    assert "gpg_setup_eval" in GP._err()
    H = np.empty((1, 1))
    assert lib.gpg_mean_gram(ctx, _lib.as_dp(H)) == -1
    assert "gpg_setup_eval" in GP._err()
    assert lib.gpg_set_mean_uncertainty(ctx, 2) == -1
    assert "0" in GP._err() and "1" in GP._err()
    assert lib.gpg_set_mean_uncertainty(ctx, -1) == -1
    assert lib.gpg_set_mean_uncertainty(None, 1) == -1
    assert lib.gpg_mean_gram(ctx, C.POINTER(C.c_double)()) == -1
    _no_fallbacks(GP)
    GP.close()
    GP = _gp(N5)                                                              # the switch set before the set-up takes effect after it
    assert GP._lib.gpg_set_mean_uncertainty(GP._ctx, 1) == 0
    s_on = np.empty(nx)
    assert GP._lib.gpg_predict(GP._ctx, nx, _lib.as_dp(xq), 1.0, _lib.as_dp(mu), _lib.as_dp(sig), _lib.as_dp(s_on)) == 0
    assert GP._lib.gpg_set_mean_uncertainty(GP._ctx, 0) == 0
    s_off = np.empty(nx)
    assert GP._lib.gpg_predict(GP._ctx, nx, _lib.as_dp(xq), 1.0, _lib.as_dp(mu), _lib.as_dp(sig), _lib.as_dp(s_off)) == 0
    assert np.all(s_on >= s_off) and np.any(s_on > s_off)
    _no_fallbacks(GP)
    # V' K^-1 V that is not positive definite: first-order mean in two dimensions (three coefficients) on two points without
    # gradients -- rank 2.  The factor of K itself is fine, so the set-up succeeds; gpg_mean_gram and a switched-on predict refuse.
    lib = _lib.load()
    ctx = C.c_void_p()
    assert lib.gpg_create(C.byref(ctx), 0, 2, 2, 0, _lib.GPG_KERNEL["SqExp"]) == 0
    try:
        assert lib.gpg_set_mean_order(ctx, 1) == 0
        x2, y2 = np.array([[0.0, 0.0], [1.0, 0.5]]), np.array([1.0, 2.0])
        assert lib.gpg_set_data(ctx, _lib.as_dp(x2), _lib.as_dp(y2), None) == 0
        theta = np.array([0.5, 0.5])
        hp = _lib.GpgHp()
        hp.theta, hp.varK_mat, hp.var_fval, hp.var_fgrad = _lib.as_dp(theta), 1.0, -1.0, -1.0
        hp.eta, hp.wellcond, hp.closed_form_varK, hp.hp_kernel = 1e-10, _lib.GPG_WELLCOND["base"], 1, 0.0
        beta = np.zeros(3)
        assert lib.gpg_setup_eval_mean(ctx, C.byref(hp), _lib.as_dp(beta), None) == 0
        H3 = np.full((3, 3), np.nan)
        assert lib.gpg_mean_gram(ctx, _lib.as_dp(H3)) == -1
        msg = lib.gpg_last_error(ctx).decode()
        assert "pivot 2" in msg and "positive definite" in msg
        assert np.all(np.isfinite(H3)) and np.array_equal(H3, H3.T)             # H is written all the same
        q2, m2, s2 = np.array([[0.3, 0.3]]), np.empty(1), np.empty(1)
        assert lib.gpg_set_mean_uncertainty(ctx, 1) == 0
        assert lib.gpg_predict(ctx, 1, _lib.as_dp(q2), 1.0, _lib.as_dp(m2), _lib.as_dp(s2), None) == -1
        assert "pivot 2" in lib.gpg_last_error(ctx).decode()
        assert lib.gpg_set_mean_uncertainty(ctx, 0) == 0
        assert lib.gpg_predict(ctx, 1, _lib.as_dp(q2), 1.0, _lib.as_dp(m2), _lib.as_dp(s2), None) == 0   # switched off it still answers
        assert lib.gpg_factor_fallbacks(ctx) == 0 and lib.gpg_solve_fallbacks(ctx) == 0
    finally:
        lib.gpg_destroy(ctx)
    GP = gpgradpy_amd.GaussianProcess(c["d"], True, 'SqExp', 'rescale_origin')
    GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"])
    assert GP.b_use_data_scl
    GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(GP.make_hp_class(theta=c["theta"])))
    for call in (lambda: GP.eval_model(xq, mean_unc=True), lambda: GP.eval_model_var(xq, mean_unc=True),
                 lambda: GP.eval_model_joint(xq, mean_unc=True), lambda: GP.sample_posterior(xq, 2, mean_unc=True)):
        with pytest.raises(Exception, match="not setup for cases where data must be rescaled"):
            call()
    assert GP.eval_model(xq)[1].shape == (nx,)                               # the default still answers on a rescaled model
    _no_fallbacks(GP)
    GP.close()
