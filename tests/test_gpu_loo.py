"""Leave-one-out cross-validation on the device (gpg_loo, GaussianProcess.loo_cv) against the brute force of
tests/test_loo_host.py (loo_reference: delete the rows of a point, refit in NumPy, predict), which that file pins to a second
CPU route at a tenth of the bound used here.

Metrics and bound (the project's prior-normalised form, E_BOUND = 2e-7 of tests/test_joint_host.py):
    E_e = max_r |e - e_ref|_r / sqrt(varK Kcov_rr),     E_C = max_ij |C - C_ref|_ij / (varK sqrt(Kcov_ii Kcov_jj)).
That bound says nothing where the leave-one-out variance is 1e-9 of the prior, so the fixtures with cond(Kcov) <= 1e5 (WELL) also
carry two relative checks: sqrt(diag C) to tolerances.SIG_RTOL and the per-row standardised residual e / sqrt(diag C) to
SIG_RTOL max(1, |z_ref|_max).  Every figure is printed (pytest -s) before it is asserted.

Largest values measured on an MI355X (one run of this file), the same to two digits with mean_unc False and True:
    parity:  E_e 1.3e-9 (SqExp_none_n5_d2), 1.3e-9 (linmean_RatQu_none_n14_d3), 4.5e-10 (Ma5f2_known_n130_d8), 3.7e-10 (near-duplicate
             fixture), 2.4e-10 (SqExp_none_n200_d4), 1.6e-10 or less elsewhere (linmean_SqExp_none_n9_d16: 3.2e-15);
             E_C 2.0e-10 (linmean_RatQu_none_n14_d3), 6.8e-12 (SqExp_none_n5_d2), 5.5e-13 or less elsewhere;
    WELL:    sqrt(diag C) relative 1.1e-12 or less; standardised residual 5.1e-9 or less at |z_ref|max up to 8.2e3 (bound 1e-5 |z_ref|max);
    switch:  mean_unc on against off on the linear-mean fixtures E_e 9.5e-3 .. 68, E_C 2.0e-4 .. 1.4;
    prec / qy normwise against NumPy: 1.8e-7 or less (qy, near-duplicate fixture; 7.8e-8 and 4.3e-8 on the next two);
    blocked W (the fallback route): E_e 4.5e-10, E_C 3.0e-13 (the figures of the dataflow route to two digits);
    by row:  E_e 2.2e-10, E_var 4.8e-13;  ln_pseudo_lkd against the brute force: 7.8e-13 relative or less.
Timing (recorded, not gated), one MI355X, per gpg_loo call after warm-up:
    n=2000, d=8 (N=18000): 33.5 ms = W launch 32.8 ms + block Gram kernel 0.29 ms (1.296 GB of W: 4.4 TB/s) + finishing kernel
                           0.16 ms + copies; the parent's route to the same blocks (W, then -(W W^T)): 32.6 + 27.5 ms;
    n=500, d=4 (N=2500):   0.69 ms = 0.49 ms + 12 us (25 MB: 2.1 TB/s) + 45 us + copies; parent 0.49 + 0.22 ms.

Every test here fails without the feature: the library has no gpg_loo and the mirror no loo_cv.
"""
import ctypes

import numpy as np
import pytest

import tolerances as tol
from test_gpu_joint import _build, _no_fallbacks
from test_joint_host import E_BOUND, case, joint_model
from test_loo_host import FIXTURES, SMALL, err_c, err_e, loo_blocks_numpy, loo_reference, problem, row_reference

pytestmark = pytest.mark.gpu

WELL = tuple(f for f in FIXTURES if any(k in f for k in ("known", "_mask"))
             or f.endswith(("linmean_SqExp_none_n12_d3", "linmean_SqExp_none_n9_d16")))
LINMEAN = tuple(f for f in FIXTURES if f.startswith("linmean"))
N64, N130 = "SqExp_none_n64_d8", "Ma5f2_known_n130_d8"
assert len(FIXTURES) == 15 and len(WELL) == 9 and len(LINMEAN) == 6
_GPS, _RAW = {}, {}


def _gp(name):
    """One device model per fixture, shared by the tests of this file (they restore every setting they change)."""
    if name not in _GPS:
        _GPS[name] = _build(name)
    return _GPS[name]


def _raw(GP, mean_unc):
    """gpg_loo itself: (resid [N], cov [n, bs, bs], prec [n, bs, bs], qy [N], n_bad)."""
    from gpgradpy_amd import _lib
    GP._set_mean_unc(mean_unc)
    n, N = GP.n_eval, GP.n_data
    bs = GP.dim + 1 if GP.use_grad else 1
    resid, qy = np.full(N, -7.0), np.full(N, -7.0)
    cov, prec = np.full((n, bs, bs), -7.0), np.full((n, bs, bs), -7.0)
    n_bad = ctypes.c_int(-1)
    rc = GP._lib.gpg_loo(GP._ctx, float(GP.hp_vals.varK), _lib.as_dp(resid), _lib.as_dp(cov), _lib.as_dp(prec), _lib.as_dp(qy),
                         ctypes.byref(n_bad))
    assert rc == 0, GP._err()
    return resid, cov, prec, qy, n_bad.value


def _raw_cached(name, mean_unc):
    if (name, mean_unc) not in _RAW:
        _RAW[(name, mean_unc)] = _raw(_gp(name), mean_unc)
    return _RAW[(name, mean_unc)]


def _live_diag(p, C):
    """diag of every block in data_vec order [N]."""
    d = np.empty(p.N)
    live = p.rows >= 0
    d[p.rows[live]] = np.diagonal(C, axis1=1, axis2=2)[live]
    return d


def _hp_like_build(GP, c, theta):
    noisy = c["b_has_noisy_data"]
    vf = None if np.isnan(c["var_fval"]) else c["var_fval"]
    vg = None if np.isnan(c["var_fgrad"]) else c["var_fgrad"]
    return GP.make_hp_class(theta=theta, kernel=float(c["hp_kernel"]) if "hp_kernel" in c else None,
                            varK=c["varK_in"] if noisy else None, var_fval=vf, var_fgrad=vg)


# ---- 1. parity with the brute force ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_unc", (False, True))
@pytest.mark.parametrize("name", FIXTURES)
def test_parity(name, mean_unc):
    jm, p, GP = joint_model(name), problem(name), _gp(name)
    np.testing.assert_allclose(float(GP.hp_vals.varK), jm.varK, rtol=tol.VARK_RTOL)
    e_ref, C_ref = loo_reference(name, mean_unc)
    resid, cov, _, _, n_bad = _raw_cached(name, mean_unc)
    Ee, Ec = err_e(p, resid, e_ref), err_c(p, cov, C_ref)
    print(f"{name} mean_unc={mean_unc}: N = {p.N}  E_e = {Ee:.2e}  E_C = {Ec:.2e}  n_bad = {n_bad}")
    assert n_bad == 0
    assert Ee <= E_BOUND and Ec <= E_BOUND
    if name in WELL:
        sd, sd_ref = np.sqrt(_live_diag(p, cov)), np.sqrt(_live_diag(p, C_ref))
        z, z_ref = resid / sd, e_ref / sd_ref
        zmax = max(1.0, float(np.abs(z_ref).max()))
        print(f"{name} mean_unc={mean_unc}: sqrt(diag C) rel {np.max(np.abs(sd / sd_ref - 1.0)):.2e}   "
              f"standardised residual {np.max(np.abs(z - z_ref)):.2e} (|z_ref|max = {zmax:.2e})")
        np.testing.assert_allclose(sd, sd_ref, rtol=tol.SIG_RTOL, atol=0)
        np.testing.assert_allclose(z, z_ref, rtol=0, atol=tol.SIG_RTOL * zmax)
    if mean_unc and name in LINMEAN:                                   # the switch does something
        resid0, cov0 = _raw_cached(name, False)[:2]
        De, Dc = err_e(p, resid, resid0), err_c(p, cov, cov0)
        print(f"{name}: mean_unc on against off  E_e = {De:.2e}  E_C = {Dc:.2e}")
        assert max(De, Dc) > E_BOUND
    _no_fallbacks(GP)


# ---- 2. prec and qy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_unc", (False, True))
@pytest.mark.parametrize("name", FIXTURES)
def test_prec_and_qy(name, mean_unc):
    p, GP = problem(name), _gp(name)
    _, cov, prec, qy, _ = _raw_cached(name, mean_unc)
    _, _, prec_np, qy_np = loo_blocks_numpy(name, mean_unc)
    dp = np.linalg.norm(prec - prec_np) / np.linalg.norm(prec_np)
    dq = np.linalg.norm(qy - qy_np) / np.linalg.norm(qy_np)
    print(f"{name} mean_unc={mean_unc}: normwise  prec {dp:.2e}  qy {dq:.2e}")
    assert dp <= tol.ALPHA_NORMWISE and dq <= tol.ALPHA_NORMWISE
    if not mean_unc:
        assert np.array_equal(qy, GP.invKernEta_fdiff)                 # the bits of alpha_out of gpg_setup_eval*
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1))) and np.array_equal(prec, np.transpose(prec, (0, 2, 1)))
    nograd = np.flatnonzero(p.rows[:, -1] < 0) if p.bs > 1 else np.array([], dtype=int)
    assert (nograd.size > 0) == ("_mask" in name)
    for a in nograd:                                                   # only [0, 0] is set
        for M in (prec, cov):
            blk = M[a].copy()
            assert blk[0, 0] > 0.0
            blk[0, 0] = 0.0
            assert np.array_equal(blk, np.zeros_like(blk))
    _no_fallbacks(GP)


# ---- 3. the same bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", (N64, N130))
def test_same_bits(name):
    c = case(name)
    GP = _build(name)                                                  # a fresh context
    xq = c["xq"]
    before = GP.eval_model(xq, calc_grad=True)[:4]
    for mean_unc in (False, True):
        first = _raw(GP, mean_unc)
        second = _raw(GP, mean_unc)
        for u, v in zip(first, second):
            assert np.array_equal(u, v)
        for cap in (1, 3, 17):
            GP.set_max_workgroups(cap)
            for u, v in zip(first, _raw(GP, mean_unc)):
                assert np.array_equal(u, v), cap
        GP.set_max_workgroups(0)
        # a likelihood gradient in between (another matrix through the same W scratch) changes no bit
        info, ok = GP.calc_lkd_all(_hp_like_build(GP, c, 1.3 * c["theta"]), calc_grad=True)
        assert ok
        for u, v in zip(first, _raw(GP, mean_unc)):
            assert np.array_equal(u, v)
        for u, v in zip(first[:4], _raw_cached(name, mean_unc)[:4]):   # and the shared context of the other tests agrees
            assert np.array_equal(u, v)
    GP._set_mean_unc(False)
    for u, v in zip(before, GP.eval_model(xq, calc_grad=True)[:4]):
        assert np.array_equal(u, v)
    _no_fallbacks(GP)
    GP.close()


@pytest.mark.parametrize("name", (N64, N130))
def test_blocked_route(name):
    """W = L^-T by the blocked sweep (what a timed-out dataflow launch falls back on): other summation orders, the same bound."""
    p = problem(name)
    GP = _build(name)
    try:
        GP.set_factor_mode('blocked')
        for mean_unc in (False, True):
            e_ref, C_ref = loo_reference(name, mean_unc)
            resid, cov, _, _, n_bad = _raw(GP, mean_unc)
            Ee, Ec = err_e(p, resid, e_ref), err_c(p, cov, C_ref)
            print(f"{name} mean_unc={mean_unc} blocked W: E_e = {Ee:.2e}  E_C = {Ec:.2e}")
            assert n_bad == 0 and Ee <= E_BOUND and Ec <= E_BOUND
    finally:
        GP.set_factor_mode('auto')
    _no_fallbacks(GP)
    GP.close()


# ---- 4. the mirror ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_unc", (False, True))
@pytest.mark.parametrize("name", SMALL)
def test_by_row(name, mean_unc):
    p, GP = problem(name), _gp(name)
    e_ref, v_ref = row_reference(name, mean_unc)
    res = GP.loo_cv(mean_unc=mean_unc, by='row')
    Ee = float(np.max(np.abs(res.resid - e_ref) / (np.sqrt(p.varK) * p.kd)))
    Ev = float(np.max(np.abs(res.var - v_ref) / (p.varK * p.kd ** 2)))
    print(f"{name} mean_unc={mean_unc} by row: E_e = {Ee:.2e}  E_var = {Ev:.2e}")
    assert Ee <= E_BOUND and Ev <= E_BOUND and res.n_bad == 0
    assert res.mu.shape == (p.N,) and np.array_equal(res.mu, GP.data_vec - res.resid)
    _no_fallbacks(GP)


@pytest.mark.parametrize("mean_unc", (False, True))
@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_by_point(name, mean_unc):
    from gpgradpy_amd.loo import loo_by_point
    p, GP = problem(name), _gp(name)
    res = GP.loo_cv(mean_unc=mean_unc)
    resid, cov = _raw_cached(name, mean_unc)[:2]
    assert res.n_bad == 0 and np.array_equal(res.cov, cov)
    assert res.mu_f.shape == (p.n,) and np.array_equal(res.resid_f, resid[:p.n]) and np.array_equal(res.mu_f, GP.data_vec[:p.n] - resid[:p.n])
    if p.bs > 1:
        assert res.mu_g.shape == (p.n, p.bs - 1)
        live = p.rows[:, 1:] >= 0
        assert np.array_equal(res.resid_g[live], resid[p.rows[:, 1:][live]]) and np.all(np.isnan(res.mu_g[~live]))
    else:
        assert res.mu_g is None
    assert res.z.shape == (p.n, p.bs) and res.ln_pseudo_lkd_pt.shape == (p.n,)
    if name in WELL:
        e_ref, C_ref = loo_reference(name, mean_unc)
        want = loo_by_point(p.y, p.rows, e_ref, C_ref).ln_pseudo_lkd
        print(f"{name} mean_unc={mean_unc}: ln_pseudo_lkd {res.ln_pseudo_lkd:.12e}  brute force {want:.12e}  "
              f"rel {abs(res.ln_pseudo_lkd - want) / abs(want):.2e}")
        assert abs(res.ln_pseudo_lkd - want) <= tol.LN_LKD_RTOL * abs(want)
    _no_fallbacks(GP)


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors():
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    name = SMALL[0]
    c = case(name)
    GP = _build(name, setup=False)
    n, bs = c["n"], c["d"] + 1
    out = np.zeros(n * bs * bs)
    n_bad = ctypes.c_int(0)
    assert GP._lib.gpg_loo(GP._ctx, 1.0, None, _lib.as_dp(out), None, None, ctypes.byref(n_bad)) == -1
    assert "gpg_setup_eval" in GP._err()
    with pytest.raises((AssertionError, Exception)):
        GP.loo_cv()
    GP.close()
    GP = _build(name)
    assert GP.loo_cv().n_bad == 0
    assert GP._lib.gpg_loo(GP._ctx, 1.0, None, None, None, None, None) == 0          # every output may be NULL
    with pytest.raises(ValueError):
        GP.loo_cv(by='column')
    GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"])
    with pytest.raises(Exception, match="setup_eval_model|Cholesky"):
        GP.loo_cv()
    GP.close()
    GP = gpgradpy_amd.GaussianProcess(c["d"], True, 'SqExp', 'rescale_origin')
    GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"])
    assert GP.b_use_data_scl
    GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(GP.make_hp_class(theta=c["theta"])))
    with pytest.raises(Exception, match="not setup for cases where data must be rescaled"):
        GP.loo_cv()
    GP.close()
