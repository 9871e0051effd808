"""First-order polynomial mean ('poly_ord_1', gpg_set_mean_order) on the device, against the fixtures captured from the
reference (tests/golden/linmean/, tests/golden/gen_golden_linmean.py).

Tolerances are the constants and helpers of tests/tolerances.py, the ones every other fixture is held to.  The CPU test
(tests/test_linmean_golden.py) measures how much the dense NumPy restatement and the reference disagree on these fixtures and on
the affine-shift property: every figure is below a tenth of its constant (largest: beta 2.8e-10 of 1e-8, ln_lkd 1.6e-10 of 1e-8,
ln_det 2.9e-8 of 2e-6, alpha 2.8e-8 of 1e-5; affine shift 1e-13 or less), so nothing is widened here.  beta is compared normwise,
max |d beta| / max |beta| <= BETA_RTOL; hp_beta_grad with check_lkd_grad's rule, row by row.

All of these fail without the feature: the constructor raises and the library has no gpg_set_mean_order.
"""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.optimize import Bounds

import tolerances as tol
from conftest import GOLDEN_DIR, load_case
from test_linmean_golden import CASES, LINMEAN_DIR, affine_shift, aug_vand, case_name, dense_linmean, normwise

pytestmark = pytest.mark.gpu

N40 = os.path.join(LINMEAN_DIR, "linmean_Ma5f2_known_n40_d4.npz")
N9 = os.path.join(LINMEAN_DIR, "linmean_SqExp_none_n9_d16.npz")


def _gp(c, f=None, g=None, linear=True):
    import gpgradpy_amd
    GP = gpgradpy_amd.GaussianProcess(c["d"], c["use_grad"], c["kernel"], c["wellcond"] if c["use_grad"] else "base",
                                      mean_fun_type='poly_ord_1' if linear else 'poly_ord_0')
    f = c["f"] if f is None else f
    g = c["g"] if g is None else g
    if c["use_grad"]:
        bvec = None if c["bvec_use_grad"].all() else c["bvec_use_grad"]
        GP.set_data(c["x"], f, c["std_f"], g, c["std_g"], bvec)
    else:
        GP.set_data(c["x"], f, c["std_f"])
    return GP


def _hp(GP, c):
    return GP.make_hp_class(theta=c["theta"], kernel=float(c["hp_kernel"]) if "hp_kernel" in c else None,
                            varK=c["varK_in"] if c["b_has_noisy_data"] else None)


def _cond(c):
    return float(np.linalg.cond(dense_linmean(c)["Kcov"]))


def _check_value(info, c, N):
    assert info.hp_beta.shape == (c["d"] + 1,)
    d_beta = normwise(info.hp_beta, c["hp_beta"])
    print(f"{c['name']}: beta normwise {d_beta:.2e}  ln_lkd rel {abs(info.ln_lkd - c['ln_lkd']) / abs(c['ln_lkd']):.2e}  "
          f"ln_det abs {abs(info.ln_det_Kmat - c['ln_det_Kmat']):.2e}")
    assert d_beta <= tol.BETA_RTOL
    tol.check_scalars(info.hp_beta[0], info.hp_varK, info.ln_det_Kmat, info.ln_lkd, c, N, c["b_has_noisy_data"])


def _check_grad(info_g, c, cond):
    assert info_g.ln_lkd_grad.shape == c["ln_lkd_grad"].shape
    tol.check_lkd_grad(info_g.ln_lkd_grad, c["ln_lkd_grad"], tol.lkd_grad_slots_to_check(c), cond=cond)
    if "hp_beta_grad" in c:                                                     # noisy path (CalcLkd.py:216-217)
        assert info_g.hp_beta_grad.shape == c["hp_beta_grad"].shape == (c["d"] + 1, c["ln_lkd_grad"].size)
        for row_got, row_ref in zip(info_g.hp_beta_grad, c["hp_beta_grad"]):
            tol.check_lkd_grad(row_got, row_ref, cond=cond)


# ---- 1. parity with the reference, every fixture -------------------------------------------------------------------------------
@pytest.mark.parametrize("path", CASES, ids=case_name)
def test_parity_with_reference(path):
    c = load_case(path)
    GP = _gp(c)
    assert GP.n_data == c["n_data"] and GP.n_beta_coeff == c["d"] + 1
    assert np.isclose(GP._etaK, c["etaK"], rtol=1e-14)
    hp = _hp(GP, c)
    info, ok = GP.calc_lkd_all(hp)
    assert ok
    _check_value(info, c, GP.n_data)
    masked = c["use_grad"] and not c["bvec_use_grad"].all()
    if not masked:
        info_g, ok_g = GP.calc_lkd_all(hp, calc_grad=True)
        assert ok_g and np.isclose(info_g.ln_lkd, info.ln_lkd, rtol=1e-12)
        np.testing.assert_array_equal(info_g.hp_beta, info.hp_beta)
        _check_grad(info_g, c, _cond(c))
    hp2 = GP.optz_closed_form_hp(hp)
    assert np.ravel(hp2.beta).size == c["d"] + 1
    np.testing.assert_allclose(hp2.varK, c["varK_model"], rtol=tol.VARK_RTOL)
    GP.set_hpara('set', 0, hp_vals=hp2)
    alpha = GP.invKernEta_fdiff
    assert np.linalg.norm(alpha - c["alpha"]) <= tol.ALPHA_NORMWISE * np.linalg.norm(c["alpha"])
    mu, sig = GP.eval_model(c["xq"])[:2]
    np.testing.assert_allclose(mu, c["mu"], rtol=tol.MU_RTOL, atol=tol.MU_ATOL_SCALE * max(1.0, np.abs(c["mu"]).max()))
    np.testing.assert_allclose(sig, c["sig"], rtol=tol.SIG_RTOL, atol=tol.SIG_ATOL_SCALE * np.sqrt(hp2.varK))
    mu_g, sig_g, dmudx, dsigdx = GP.eval_model(c["xq"], calc_grad=True)[:4]
    np.testing.assert_allclose(mu_g, mu, rtol=1e-12)
    tol.check_post_grad(dmudx, dsigdx, c)
    if masked:
        return
    # Hessians, one point per call, with the rule of tests/test_posterior_hess.py::_check (d2sig divides by sig: its error scales
    # with kappa * eps / sig).  d2mudx2 is the kernel part alone: the Hessian of a first-order mean is zero.
    varK = hp2.varK
    for i in range(c["xq"].shape[0]):
        m1, s1, dm, ds, h_mu, h_sig = GP.eval_model(c["xq"][i], calc_grad=True, calc_hess=True, squeeze_nx=True)
        assert np.isclose(m1, mu[i], rtol=1e-12) and np.allclose(dm, dmudx[i], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(h_mu, c["d2mudx2"][i], rtol=1e-6, atol=1e-7 * np.abs(c["d2mudx2"][i]).max())
        ref = c["d2sigdx2"][i]
        np.testing.assert_allclose(h_sig, ref, rtol=1e-4,
                                   atol=1e-6 * max(1.0, np.abs(ref).max()) / min(1.0, c["sig"][i] / np.sqrt(varK) + 1e-12))


# ---- 2. every schedule carries the right-hand-side rows ------------------------------------------------------------------------
def _rows5(GP, c):
    """Five start rows in the optimiser's encoding (GpHpara.py:56-103): row 0 is the fixture's hyperparameter vector."""
    hi = GP.hp_info_optz_lkd
    v = np.zeros(hi.n_hp)
    v[hi.idx_theta] = c["theta"]
    if hi.has_varK:
        v[hi.idx_varK] = c["varK_in"]
    rows = np.tile(v, (5, 1))
    rows[1:, hi.idx_theta] *= np.random.default_rng(9).uniform(0.6, 1.6, (4, c["d"]))
    rows[:, hi.bvec_log_optz] = np.log10(rows[:, hi.bvec_log_optz])
    return rows


@pytest.mark.parametrize("path", (N40, N9), ids=case_name)
@pytest.mark.parametrize("mode", ("blocked", "tile64", "tile128"))
def test_every_schedule_carries_the_rows(path, mode):
    c = load_case(path)
    cond = _cond(c)
    GP = _gp(c)
    GP.set_factor_mode(mode)
    hp = _hp(GP, c)
    info, ok = GP.calc_lkd_all(hp)
    assert ok and GP.last_factor()[0] == mode
    _check_value(info, c, GP.n_data)
    info_g, ok_g = GP.calc_lkd_all(hp, calc_grad=True)
    assert ok_g
    _check_grad(info_g, c, cond)
    # pair mode 1: every 128-tile launch, also of ONE matrix, goes to the pair kernel (its right-hand-side tile rows are "light tasks")
    assert GP._lib.gpg_set_pair_mode(GP._ctx, 1) == 0
    info_p, ok_p = GP.calc_lkd_all(hp)
    assert ok_p and GP.last_factor()[0] == ('pair128' if mode == 'tile128' else mode)
    assert info_p.ln_lkd == info.ln_lkd
    np.testing.assert_array_equal(info_p.hp_beta, info.hp_beta)
    rows = _rows5(GP, c)
    ln_b = GP.calc_lkd_batch(rows)
    ln_gb, grad_b, ok_b = GP.calc_lkd_grad_batch(rows)
    assert np.all(ok_b)
    for i in range(5):
        one, ok1 = GP.calc_lkd_all(GP.hp_vec2dataclass(GP.hp_info_optz_lkd, rows[i]), calc_grad=True)
        assert ok1
        assert ln_b[i] == one.ln_lkd and ln_gb[i] == one.ln_lkd, (i, ln_b[i], ln_gb[i], one.ln_lkd)
        np.testing.assert_array_equal(grad_b[i], one.ln_lkd_grad)
    np.testing.assert_allclose(ln_b[0], c["ln_lkd"], rtol=tol.LN_LKD_RTOL)
    tol.check_lkd_grad(grad_b[0], c["ln_lkd_grad"], tol.lkd_grad_slots_to_check(c), cond=cond)
    assert GP.factor_fallbacks() == 0 and GP.overlap_fallbacks() == 0 and GP.solve_fallbacks() == 0


def test_batched_gradient_groups_bitwise():
    """N = 550 (Npad = 640): large enough for gpg_lkd_grad_batch to form groups (one launch per step for several matrices, the
    combine step reading each matrix's own coefficient slot); 5 rows, an odd count.  Bit-identical to single calls."""
    import gpgradpy_amd
    from oracle import gp_oracle as orc
    n, d = 110, 4
    X, f, g = orc.synthetic_design(n, d, seed=12)
    f = f + 40.0 * (X @ np.arange(1.0, d + 1.0)) - 25.0
    g = g + 40.0 * np.arange(1.0, d + 1.0)[None, :]
    GP = gpgradpy_amd.GaussianProcess(d, True, 'SqExp', 'precon', mean_fun_type='poly_ord_1')
    GP.set_data(X, f, np.zeros(n), g, np.zeros((n, d)))
    rows = np.random.default_rng(13).uniform(-2.0, -0.6, (5, d))
    ln_b, outs = GP.calc_lkd_batch(rows, return_all=True)
    ln_gb, grad_b, ok_b = GP.calc_lkd_grad_batch(rows)
    assert np.all(ok_b) and GP.last_factor()[1] > 1
    for i in range(5):
        one, ok1 = GP.calc_lkd_all(GP.hp_vec2dataclass(GP.hp_info_optz_lkd, rows[i]), calc_grad=True)
        assert ok1 and ln_b[i] == one.ln_lkd and ln_gb[i] == one.ln_lkd and outs[i].beta == one.hp_beta[0]
        np.testing.assert_array_equal(grad_b[i], one.ln_lkd_grad)
    assert GP.factor_fallbacks() == 0 and GP.overlap_fallbacks() == 0 and GP.solve_fallbacks() == 0


# ---- 3. order 0 is untouched ---------------------------------------------------------------------------------------------------
def test_order_zero_is_untouched():
    c = load_case(os.path.join(GOLDEN_DIR, "SqExp_none_n200_d4.npz"))
    res = []
    for toggle in (False, True):
        GP = _gp(c, linear=False)
        if toggle:
            assert GP._lib.gpg_set_mean_order(GP._ctx, 1) == 0
            assert GP.calc_lkd_all(_hp(GP, c))[1]                               # one evaluation with the linear mean in between
            assert GP._lib.gpg_set_mean_order(GP._ctx, 0) == 0
        hp = _hp(GP, c)
        a, ok = GP.calc_lkd_all(hp)
        b, okb = GP.calc_lkd_all(hp, calc_grad=True)
        assert ok and okb
        GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(hp))
        post = GP.eval_model(c["xq"], calc_grad=True)[:4]
        res.append((a.ln_lkd, a.hp_beta, a.hp_varK, a.ln_det_Kmat, b.ln_lkd, b.ln_lkd_grad, GP.invKernEta_fdiff) + tuple(post))
        GP.close()
    for x, y in zip(*res):
        np.testing.assert_array_equal(x, y)
    tol.check_scalars(res[0][1][0], res[0][2], res[0][3], res[0][0], c, c["n_data"], False)


# ---- 4. properties that need no reference (n40_d4 data) ------------------------------------------------------------------------
def _lkd_alpha(GP):
    from gpgradpy_amd import _lib
    alpha = np.empty(GP.n_data)
    assert GP._lib.gpg_lkd_alpha(GP._ctx, _lib.as_dp(alpha)) == 0
    return alpha


def test_orthogonality_of_alpha():
    c = load_case(N40)
    GP = _gp(c)
    info, ok = GP.calc_lkd_all(_hp(GP, c), calc_grad=True)
    assert ok
    alpha = _lkd_alpha(GP)                                                      # Kcov^-1 (y - V beta) of the likelihood's matrix
    V = aug_vand(c["x"], True)
    Kn = np.linalg.norm(dense_linmean(c)["Kcov"], 2)
    for j in range(V.shape[1]):
        lhs, rhs = abs(V[:, j] @ alpha), tol.ALPHA_RESIDUAL * np.linalg.norm(V[:, j]) * Kn * np.linalg.norm(alpha)
        print(f"column {j}: |V_j' alpha| = {lhs:.3e}  bound {rhs:.3e}")
        assert lhs <= rhs


def test_affine_shift():
    c = load_case(N40)
    f2, g2, shift = affine_shift(c)                                             # the added part has the norm of the values
    out = []
    for f, g in ((c["f"], c["g"]), (f2, g2)):
        GP = _gp(c, f, g)
        hp = _hp(GP, c)
        info, ok = GP.calc_lkd_all(hp, calc_grad=True)
        assert ok
        alpha_l = _lkd_alpha(GP)
        GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(hp))
        sig = GP.eval_model(c["xq"])[1]
        out.append((info, alpha_l, GP.invKernEta_fdiff.copy(), sig))
        GP.close()
    (a, al_a, am_a, sig_a), (b, al_b, am_b, sig_b) = out
    d_beta = normwise(b.hp_beta - shift, a.hp_beta)
    print(f"affine shift: beta {d_beta:.2e}  ln_lkd {abs(b.ln_lkd - a.ln_lkd) / abs(a.ln_lkd):.2e}  "
          f"alpha {np.linalg.norm(al_b - al_a) / np.linalg.norm(al_a):.2e}")
    assert d_beta <= tol.BETA_RTOL
    np.testing.assert_allclose(b.ln_lkd, a.ln_lkd, rtol=tol.LN_LKD_RTOL)
    np.testing.assert_allclose(b.ln_det_Kmat, a.ln_det_Kmat, rtol=0, atol=tol.LN_DET_ATOL + tol.LN_DET_ATOL_PER_N * c["n_data"])
    assert np.linalg.norm(al_b - al_a) <= tol.ALPHA_NORMWISE * np.linalg.norm(al_a)
    assert np.linalg.norm(am_b - am_a) <= tol.ALPHA_NORMWISE * np.linalg.norm(am_a)
    np.testing.assert_allclose(sig_b, sig_a, rtol=tol.SIG_RTOL, atol=tol.SIG_ATOL_SCALE * np.sqrt(c["varK_in"]))
    # noise-free data: varK is the closed-form one and must not move either
    c3 = load_case(os.path.join(LINMEAN_DIR, "linmean_SqExp_none_n12_d3.npz"))
    f3, g3, shift3 = affine_shift(c3)
    v = []
    for f, g in ((c3["f"], c3["g"]), (f3, g3)):
        GP = _gp(c3, f, g)
        v.append(GP.calc_lkd_all(_hp(GP, c3))[0])
        GP.close()
    np.testing.assert_allclose(v[1].hp_varK, v[0].hp_varK, rtol=tol.VARK_RTOL)
    assert normwise(v[1].hp_beta - shift3, v[0].hp_beta) <= tol.BETA_RTOL


def test_affine_shift_with_data_rescaling():
    """A data-rescaling method: the device sees scaled points, V is built from them (as the reference uses get_scl_x_w_dist) and the
    query points are scaled the same way.  In the caller's coordinates the shift c0 + x . c must then move mu by c0 + xq . c and
    dmudx by c and leave sig alone."""
    import gpgradpy_amd
    c = load_case(os.path.join(LINMEAN_DIR, "linmean_SqExp_none_n12_d3.npz"))
    f2, g2, shift = affine_shift(c)
    res = []
    for f, g in ((c["f"], c["g"]), (f2, g2)):
        GP = gpgradpy_amd.GaussianProcess(c["d"], True, 'SqExp', 'rescale_origin', mean_fun_type='poly_ord_1')
        GP.set_data(c["x"], f, c["std_f"], g, c["std_g"])
        assert GP.b_use_data_scl
        hp = GP.optz_closed_form_hp(GP.make_hp_class(theta=c["theta"]))
        GP.set_hpara('set', 0, hp_vals=hp)
        res.append(GP.eval_model(c["xq"], calc_grad=True)[:4])
        GP.close()
    (mu_a, sig_a, dmu_a, dsig_a), (mu_b, sig_b, dmu_b, dsig_b) = res
    want_mu = mu_a + shift[0] + c["xq"] @ shift[1:]
    np.testing.assert_allclose(mu_b, want_mu, rtol=tol.MU_RTOL, atol=tol.MU_ATOL_SCALE * max(1.0, np.abs(want_mu).max()))
    want_dmu = dmu_a + shift[1:][None, :]
    np.testing.assert_allclose(dmu_b, want_dmu, rtol=tol.DMU_RTOL, atol=tol.DMU_RTOL * np.abs(want_dmu).max())
    np.testing.assert_allclose(sig_b, sig_a, rtol=tol.SIG_RTOL, atol=tol.SIG_ATOL_SCALE * np.abs(sig_a).max())


# ---- 5. singular trend -----------------------------------------------------------------------------------------------------------
def _check_singular_grad_batch(GP, rows):
    """gpg_lkd_grad_batch on rows whose GLS system is singular: info > N, NaN ln_lkd and gradients; the mirror reports ok False."""
    from gpgradpy_amd import _lib
    ln, grad, ok = GP.calc_lkd_grad_batch(rows)
    assert not np.any(ok) and np.all(np.isnan(ln)) and np.all(np.isnan(grad))
    r = GP._rows_with_eta(np.ascontiguousarray(GP._rows_from_hp_x0(rows)))
    m, d = r.shape[0], GP.dim
    outs = (_lib.GpgLkdOut * m)()
    g_aa, g_inv = np.zeros((m, d + 4)), np.zeros((m, d + 4))
    rc = GP._lib.gpg_lkd_grad_batch(GP._ctx, m, _lib.as_dp(r), r.shape[1], float(GP._etaK), GP._wellcond_code,
                                    int(not GP.b_has_noisy_data), outs, _lib.as_dp(g_aa), _lib.as_dp(g_inv))
    assert rc == 0
    for o in outs:
        assert GP.n_data < o.info <= GP.n_data + d + 1 and np.isnan(o.ln_lkd) and np.isnan(o.varK)
    assert np.all(np.isnan(g_aa[:, :d])) and np.all(np.isnan(g_inv[:, :d]))


def test_singular_trend_is_a_failed_factorisation():
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (3, 3))                                               # 3 points, 4 coefficients, no gradients
    GP = gpgradpy_amd.GaussianProcess(3, False, 'SqExp', mean_fun_type='poly_ord_1')
    GP.set_data(x, np.array([1.0, -2.0, 0.5]), np.zeros(3))
    hp_vals = GP.make_hp_class(theta=np.full(3, 0.4))
    hp, keep = GP._make_hp(hp_vals, 1.0, closed_form=True)
    out = _lib.GpgLkdOut()
    rc = GP._lib.gpg_lkd(GP._ctx, C.byref(hp), C.byref(out))
    assert rc == out.info and out.info > GP.n_data and out.info <= GP.n_data + 4 and np.isnan(out.ln_lkd)
    info, ok = GP.calc_lkd_all(hp_vals)                                          # the mirror: a failed factorisation, nothing raises
    assert ok is False and info.ln_lkd is None
    info_g, ok_g = GP.calc_lkd_all(hp_vals, calc_grad=True)
    assert ok_g is False
    rows = np.log10(np.array([[0.4, 0.4, 0.4], [0.1, 0.2, 0.3]]))
    ln = GP.calc_lkd_batch(rows)
    assert np.all(np.isnan(ln))
    _check_singular_grad_batch(GP, rows)
    # affinely dependent points (all on one line) with enough of them
    t = np.linspace(-1, 1, 6)
    xl = np.outer(t, [1.0, 0.5, -0.25]) + 0.1
    GP2 = gpgradpy_amd.GaussianProcess(3, False, 'SqExp', mean_fun_type='poly_ord_1')
    GP2.set_data(xl, np.sin(t), np.zeros(6))
    info2, ok2 = GP2.calc_lkd_all(GP2.make_hp_class(theta=np.full(3, 0.4)))
    assert ok2 is False
    # the same on a matrix large enough for gpg_lkd_grad_batch to form groups (Npad = 640): 520 well-separated points on a line,
    # the covariance matrix itself factorises, the trend does not
    t3 = np.linspace(-200.0, 200.0, 520)
    GP3 = gpgradpy_amd.GaussianProcess(3, False, 'SqExp', mean_fun_type='poly_ord_1')
    GP3.set_data(np.outer(t3, [1.0, 0.5, -0.25]) + 0.1, np.sin(t3), np.zeros(520))
    rows3 = np.log10(np.array([[0.4, 0.4, 0.4], [0.3, 0.5, 0.2], [0.6, 0.3, 0.4]]))
    ln3, outs3 = GP3.calc_lkd_batch(rows3, return_all=True)
    assert np.all(np.isnan(ln3)) and all(o.info > GP3.n_data for o in outs3)
    _check_singular_grad_batch(GP3, rows3)
    assert GP3.last_factor()[1] == 3


# ---- 6. gpg_setup_eval guard, several contexts ---------------------------------------------------------------------------------
def test_setup_eval_guard_and_multi():
    from gpgradpy_amd import _lib
    c = load_case(N40)
    GP = _gp(c)
    hp_vals = GP.optz_closed_form_hp(_hp(GP, c))
    hp, keep = GP._make_hp(hp_vals, 1.0, closed_form=False)
    rc = GP._lib.gpg_setup_eval(GP._ctx, C.byref(hp), float(hp_vals.beta[0]), None)
    assert rc == -1 and "gpg_setup_eval_mean" in GP._err()
    beta = np.ascontiguousarray(hp_vals.beta, dtype=np.float64)
    assert GP._lib.gpg_setup_eval_mean(GP._ctx, C.byref(hp), _lib.as_dp(beta), None) == 0
    assert GP._lib.gpg_set_mean_order(GP._ctx, 2) == -1
    # one device listed twice
    rows = np.ascontiguousarray(GP._rows_from_hp_x0(_rows5(GP, c)))
    ln_b, outs = GP.calc_lkd_batch(_rows5(GP, c), return_all=True)
    lib = GP._lib
    m = C.c_void_p()
    devs = (C.c_int * 2)(GP.device, GP.device)
    assert lib.gpg_multi_create(C.byref(m), 2, devs, c["n"], c["d"], 1, _lib.GPG_KERNEL[c["kernel"]]) == 0
    try:
        assert lib.gpg_multi_set_mean_order(m, 1) == 0
        x = np.ascontiguousarray(c["x"], dtype=np.float64)
        assert lib.gpg_multi_set_data(m, _lib.as_dp(x), _lib.as_dp(GP._data_vec), _lib.as_dp(GP._noise_known)) == 0
        mo = (_lib.GpgLkdOut * 5)()
        best = C.c_int(-1)
        rc = lib.gpg_multi_lkd_batch(m, 5, _lib.as_dp(rows), rows.shape[1], float(GP._etaK), GP._wellcond_code, 0, mo, C.byref(best))
        assert rc == 0, lib.gpg_multi_last_error(m)
        for i in range(5):
            assert mo[i].info == 0 and mo[i].ln_lkd == outs[i].ln_lkd and mo[i].beta == outs[i].beta
        assert best.value == int(np.argmax(ln_b))
    finally:
        lib.gpg_multi_destroy(m)


# ---- 7. optimisation -----------------------------------------------------------------------------------------------------------
def test_optz_flow_matches_reference():
    """One set_hpara('optz') run from the fixture's explicit start rows, with the comparison and the tolerances
    tests/test_hpara_optz.py applies to its reference runs (TIGHT)."""
    import gpgradpy_amd
    from test_hpara_optz import TIGHT as T
    with np.load(os.path.join(LINMEAN_DIR, "linmean_optz_SqExp_n20_d2.npz"), allow_pickle=False) as z:
        c = {k: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files}
    n, d = int(c["n"]), int(c["d"])
    GP = gpgradpy_amd.GaussianProcess(d, True, str(c["kernel"]), 'precon', mean_fun_type='poly_ord_1')
    GP.optz_n_x0 = 3
    GP.init_optz_surr(3)
    assert GP.hp_beta_all.shape[1] == d + 1
    GP.set_data(c["x"][:1], c["f"][:1], np.zeros(1), c["g"][:1], np.zeros((1, d)))
    GP.set_hpara('optz', 0)
    np.testing.assert_allclose(GP.hp_theta_all[0], c["theta_hist0"], rtol=1e-14)
    GP.set_data(c["x"], c["f"], np.zeros(n), c["g"], np.zeros((n, d)))
    box = GP.get_hp_x0_lhs_median(1, GP.hp_info_optz_lkd, 3)[1]
    np.testing.assert_allclose(box.lb, c["box_lb"], rtol=1e-13)
    np.testing.assert_allclose(box.ub, c["box_ub"], rtol=1e-13)
    GP.select_hp_optz_x0 = lambda i_optz, hp_info: (c["hp_x0"].copy(), Bounds(c["box_lb"], c["box_ub"]), 0.0)
    GP.set_hpara('optz', 1)
    hv = GP.hp_vals
    mu, sig = GP.eval_model(c["x"][:2])[:2]
    assert np.all(np.isfinite(mu)) and np.all(sig >= 0)
    ln_here = GP.calc_lkd_all(GP.make_hp_class(theta=hv.theta, kernel=hv.kernel))[0].ln_lkd
    ln_ref = c["ln_lkd"]
    assert abs(ln_here - ln_ref) <= T["ln"] * abs(ln_ref) + 1e-6, (ln_here, ln_ref)
    np.testing.assert_allclose(np.log10(hv.theta), np.log10(c["theta"]), atol=T["log_theta"])
    assert np.isclose(hv.varK, c["varK"], rtol=T["varK"])
    assert np.ravel(hv.beta).shape == (d + 1,)
    for got, ref in zip(np.ravel(hv.beta), c["beta"]):
        assert np.isclose(got, ref, rtol=T["beta"], atol=1e-6 * max(1.0, abs(ref))), (hv.beta, c["beta"])
    assert GP.hp_optz_success[1] == c["success"]
    np.testing.assert_array_equal(GP.hp_beta_all[1], np.ravel(hv.beta))
    GP.set_hpara('stored', 1)
    np.testing.assert_allclose(GP.hp_vals.beta, GP.hp_beta_all[1])
