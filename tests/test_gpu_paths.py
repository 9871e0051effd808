"""Posterior sample paths on the device (gpg_paths_setup / gpg_paths_eval / gpg_paths_coeff, GaussianProcess.sample_paths) against the
NumPy restatement of the path formula in tests/paths_cases.py (Matheron's rule with the oracle's kern_grad, setup_eval_model and
calc_all_K_w_chofac), on the six models listed there.  Shapes: S = 5 and S = 70 paths (less than / more than one 64-column path tile),
M = 37 features (no multiple of the 256-feature trip or its 64-feature quarters), nx = 70 points (with gradients 70 (d + 1) rows: several
row tiles, the last one partial).

Bounds (none fitted to what the device gives; every figure is printed, pytest -s, before it is asserted):
  1. parity   f: MU_RTOL / MU_ATOL_SCALE max(1, |f|max); dfdx: DMU_RTOL with the dmudx rule of tests/test_gpu_joint.py; coeff normwise
              ALPHA_NORMWISE per path; ddiag against diag(gpg_get_matrix(1)) - diag(gpg_get_matrix(0)) at rtol 1e-13.
  2. zero draw    w = 0, z = 0: every path against mu, dmudx of gpg_predict_grad, the MU_* / DMU_RTOL rules (tests/test_gpu_second.py).
  3. linearity    |dev(w1 + w2, z1 + z2) - dev(w1, z1) - dev(w2, z2)| <= 1e-10 of the largest deviation: exact in exact arithmetic, the
              margin covers reassociation over at most N_pad + M terms.
  4. one function across calls: bitwise per point in one call of 70, two calls of 30 + 40, chunks of 64, and under 1 / 3 / 17 workgroups.
  5. gradient     dfdx against central differences of f through separate calls, h = 1e-5 of the data range, 1e-6 of the largest |dfdx|.
  6. training rows    f_s(X) = mu_rows + sqrt(varK) (D v_s - D^(1/2) z_s), v_s = (alpha - c_s) / sqrt(varK) from gpg_paths_coeff, at the
              parity tolerance (the random features cancel in this identity).
  7. errors and invalidation.

Largest values measured on an MI355X (one run of this file: 32 tests in 1.5 s):
    parity, fraction of the bound used: f 3.6e-2 (sqexp_n17_d4, S = 70), dfdx 4.7e-5; coeff normwise 1.1e-10 (sqexp_n17_d4_lin), 6.5e-12
                or less on the other four models; ddiag against the two diagonals: equal bits (against the oracle's 2.1e-12 relative);
    zero draw   |f - mu| 1.4e-9 at |mu| ~ 1.5e3 (sqexp_n17_d4), 5.3e-11 or less elsewhere;
    linearity   1.4e-12 of the largest deviation or less;
    gradient    1.4e-8 of |dfdx|max or less;
    training rows   f 2.2e-5, dfdx 1.5e-7 of the bound.

All of these fail without the feature: the library has no gpg_paths_* and the mirror no sample_paths.
"""
import ctypes as C

import numpy as np
import pytest

import paths_cases as pc
import tolerances as tol

pytestmark = pytest.mark.gpu

_GPS, _REF = {}, {}


def _gp(name):
    """One device model per case, shared by the tests of this file (they restore every setting they change)."""
    if name not in _GPS:
        _GPS[name] = pc.build_gp(pc.model(name))
    return _GPS[name]


def _ref(name, S):
    """Draws, query points and the NumPy reference of (model, S); computed once and left unchanged."""
    key = (name, S)
    if key not in _REF:
        pm = pc.model(name)
        omega, phase, w, z = pc.draws(pm, S, 100 + S)
        xq = pm.box_points(pc.NX, 7)
        coeff = pc.coeff_reference(pm, omega, phase, w, z)
        f, dfdx = pc.path_reference(pm, omega, phase, w, z, xq, coeff)
        _REF[key] = dict(omega=omega, phase=phase, w=w, z=z, xq=xq, coeff=coeff, f=f, dfdx=dfdx)
    return _REF[key]


def _no_fallbacks(GP):
    assert GP.factor_fallbacks() == 0 and GP.overlap_fallbacks() == 0 and GP.solve_fallbacks() == 0


def _paths(GP, r):
    return GP.sample_paths(r["w"].shape[0], omega=r["omega"], phase=r["phase"], w=r["w"], z=r["z"])


def _check_f(tag, f, dfdx, f_ref, dfdx_ref):
    at_f = tol.MU_ATOL_SCALE * max(1.0, np.abs(f_ref).max())
    at_g = tol.DMU_RTOL * max(1e-12, np.abs(dfdx_ref).max())
    u_f = float(np.max(np.abs(f - f_ref) / (at_f + tol.MU_RTOL * np.abs(f_ref))))
    u_g = float(np.max(np.abs(dfdx - dfdx_ref) / (at_g + tol.DMU_RTOL * np.abs(dfdx_ref))))
    print(f"{tag}: fraction of the bound used  f {u_f:.2e}  dfdx {u_g:.2e}")
    np.testing.assert_allclose(f, f_ref, rtol=tol.MU_RTOL, atol=at_f)
    np.testing.assert_allclose(dfdx, dfdx_ref, rtol=tol.DMU_RTOL, atol=at_g)


# ---- 1. parity with the NumPy formula ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", pc.S_VALUES)
@pytest.mark.parametrize("name", pc.NAMES)
def test_parity(name, S):
    from gpgradpy_amd import _lib
    pm, GP, r = pc.model(name), _gp(name), _ref(name, S)
    np.testing.assert_allclose(float(GP.hp_vals.varK), pm.varK, rtol=tol.VARK_RTOL)
    paths = _paths(GP, r)
    f, dfdx = paths(r["xq"], calc_grad=True)
    assert f.shape == (S, pc.NX) and dfdx.shape == (S, pc.NX, pm.c["d"])
    _check_f(f"{name} S={S}", f, dfdx, r["f"], r["dfdx"])
    assert np.array_equal(paths(r["xq"]), f)                                   # without the derivative rows: the same values
    coeff, dd = paths.coeff, paths.ddiag
    e_c = float(np.max(np.linalg.norm(coeff - r["coeff"], axis=1) / np.linalg.norm(r["coeff"], axis=1)))
    hp, keep = GP._make_hp(GP.hp_vals, 1.0, closed_form=not GP.b_has_noisy_data)
    K0, K1 = np.empty((pm.N, pm.N)), np.empty((pm.N, pm.N))
    assert GP._lib.gpg_get_matrix(GP._ctx, C.byref(hp), 0, _lib.as_dp(K0)) == 0
    assert GP._lib.gpg_get_matrix(GP._ctx, C.byref(hp), 1, _lib.as_dp(K1)) == 0
    dd_ref = np.diag(K1) - np.diag(K0)
    e_d = float(np.max(np.abs(dd - dd_ref) / np.abs(dd_ref)))
    print(f"{name} S={S}: coeff normwise {e_c:.2e}   ddiag rel {e_d:.2e}   ddiag against the oracle's rel "
          f"{np.max(np.abs(dd - pm.D) / pm.D):.2e}")
    assert e_c <= tol.ALPHA_NORMWISE
    np.testing.assert_allclose(dd, dd_ref, rtol=1e-13, atol=0)
    _no_fallbacks(GP)


# ---- 2. zero draw ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NAMES)
def test_zero_draw_is_the_posterior_mean(name):
    pm, GP, r = pc.model(name), _gp(name), _ref(name, 5)
    paths = GP.sample_paths(5, omega=r["omega"], phase=r["phase"], w=np.zeros_like(r["w"]), z=np.zeros_like(r["z"]))
    f, dfdx = paths(r["xq"], calc_grad=True)
    mu, _, dmudx, _ = GP.eval_model(r["xq"], calc_grad=True)[:4]
    print(f"{name}: zero draw  |f - mu| {np.max(np.abs(f - mu[None])):.2e}  |dfdx - dmudx| {np.max(np.abs(dfdx - dmudx[None])):.2e}")
    for s in range(5):
        np.testing.assert_allclose(f[s], mu, rtol=tol.MU_RTOL, atol=tol.MU_ATOL_SCALE * max(1.0, np.abs(mu).max()))
        np.testing.assert_allclose(dfdx[s], dmudx, rtol=tol.DMU_RTOL, atol=tol.DMU_RTOL * max(1e-12, np.abs(dmudx).max()))
    nodraw = GP.sample_paths(5, omega=r["omega"], phase=r["phase"], w=np.zeros_like(r["w"]), noise_draw=False)   # z = NULL
    assert np.array_equal(nodraw(r["xq"]), f)
    _no_fallbacks(GP)


# ---- 3. linearity in the draws ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sqexp_n17_d4", "ma5f2_n23_d3_mask", "ratqu_n12_d3_base", "sqexp_n40_d2_nograd"))
def test_linearity(name):
    GP, r = _gp(name), _ref(name, 5)
    r2 = _ref(name, 70)
    w2, z2 = r2["w"][:5], r2["z"][:5]
    xq = r["xq"]

    def dev(w, z):
        p = GP.sample_paths(5, omega=r["omega"], phase=r["phase"], w=w, z=z)
        f, g = p(xq, calc_grad=True)
        return f, g

    f0, g0 = dev(np.zeros_like(w2), np.zeros_like(z2))
    fa, ga = dev(r["w"], r["z"])
    fb, gb = dev(w2, z2)
    fs, gs = dev(r["w"] + w2, r["z"] + z2)
    big_f = max(np.abs(fa - f0).max(), np.abs(fb - f0).max(), np.abs(fs - f0).max())
    big_g = max(np.abs(ga - g0).max(), np.abs(gb - g0).max(), np.abs(gs - g0).max())
    e_f = float(np.max(np.abs((fs - f0) - (fa - f0) - (fb - f0))) / big_f)
    e_g = float(np.max(np.abs((gs - g0) - (ga - g0) - (gb - g0))) / big_g)
    print(f"{name}: linearity  f {e_f:.2e}  dfdx {e_g:.2e} of the largest deviation ({big_f:.2e}, {big_g:.2e})")
    assert e_f <= 1e-10 and e_g <= 1e-10
    _no_fallbacks(GP)


# ---- 4. one function across calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", (("ma5f2_n33_d3", 70), ("sqexp_n40_d2_nograd", 5)))
def test_one_function_across_calls(name, S):
    GP, r = _gp(name), _ref(name, S)
    xq = r["xq"]
    paths = _paths(GP, r)
    f, g = paths(xq, calc_grad=True)
    assert np.array_equal(paths(xq, calc_grad=True)[0], f)
    fa, ga = paths(xq[:30], calc_grad=True)
    fb, gb = paths(xq[30:], calc_grad=True)
    assert np.array_equal(np.concatenate((fa, fb), axis=1), f) and np.array_equal(np.concatenate((ga, gb), axis=1), g)
    try:
        GP.set_second_chunk(64)                                                # two chunks: 64 and 6 points
        fc, gc = paths(xq, calc_grad=True)
    finally:
        GP.set_second_chunk(0)
    assert np.array_equal(fc, f) and np.array_equal(gc, g)
    try:
        for cap in (1, 3, 17):
            GP.set_max_workgroups(cap)
            p2 = _paths(GP, r)                                                 # the sweeps of the set-up run under the cap as well
            f2, g2 = p2(xq, calc_grad=True)
            assert np.array_equal(f2, f) and np.array_equal(g2, g), cap
    finally:
        GP.set_max_workgroups(0)
    _no_fallbacks(GP)


# ---- 5. dfdx is the gradient of f --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", (("sqexp_n17_d4", 70), ("ma5f2_n23_d3_mask", 5), ("ratqu_n12_d3_base", 5), ("sqexp_n40_d2_nograd", 5),
                                    ("sqexp_n17_d4_lin", 5)))
def test_gradient_against_central_differences(name, S):
    pm, GP, r = pc.model(name), _gp(name), _ref(name, S)
    d = pm.c["d"]
    xq = r["xq"][:6]
    paths = _paths(GP, r)
    g = paths(xq, calc_grad=True)[1]
    h = 1e-5 * (pm.c["x"].max(axis=0) - pm.c["x"].min(axis=0))
    fd = np.empty_like(g)
    for k in range(d):
        e = np.zeros(d)
        e[k] = h[k]
        fd[:, :, k] = (paths(xq + e) - paths(xq - e)) / (2.0 * h[k])
    err = float(np.max(np.abs(g - fd)) / np.abs(g).max())
    print(f"{name} S={S}: |dfdx - central differences| = {err:.2e} of |dfdx|max = {np.abs(g).max():.3e}")
    assert err <= 1e-6
    _no_fallbacks(GP)


# ---- 6. the identity at the training rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ma5f2_n33_d3", "ma5f2_n23_d3_mask"))
def test_training_row_identity(name):
    pm, GP, r = pc.model(name), _gp(name), _ref(name, 5)
    c = pm.c
    n, d, X = c["n"], c["d"], c["x"]
    paths = _paths(GP, r)
    f, g = paths(X, calc_grad=True)
    mu, _, dmudx, _ = GP.eval_model(X, calc_grad=True)[:4]
    sv = np.sqrt(float(GP.hp_vals.varK))
    v = (GP.invKernEta_fdiff[None, :] - paths.coeff) / sv
    dd = paths.ddiag
    corr = sv * (dd[None, :] * v - np.sqrt(dd)[None, :] * r["z"])                                  # [S, N], rows of the model
    got = np.concatenate((f, np.transpose(g, (0, 2, 1)).reshape(5, -1)), axis=1)[:, pm.rows]
    mu_rows = np.concatenate((mu, dmudx.T.reshape(-1)))[pm.rows]
    want = mu_rows[None, :] + corr
    _check_f(f"{name} training rows", got[:, :n], got[:, n:], want[:, :n], want[:, n:])
    _no_fallbacks(GP)


# ---- 7. errors and invalidation ---------------------------------------------------------------------------------------------------
def test_errors_and_invalidation():
    from gpgradpy_amd import _lib
    name = "sqexp_n17_d4"
    pm, r = pc.model(name), _ref(name, 5)
    GP = pc.build_gp(pm)                                                         # a context of its own: it is set up again below
    lib, ctx = GP._lib, GP._ctx
    xq = np.ascontiguousarray(r["xq"][:3])
    f = np.empty((5, 3))
    om, ph, w, z = (np.ascontiguousarray(r[k]) for k in ("omega", "phase", "w", "z"))
    setup = lambda S, M: lib.gpg_paths_setup(ctx, S, M, _lib.as_dp(om), _lib.as_dp(ph), _lib.as_dp(w), _lib.as_dp(z), 1.0)
    assert lib.gpg_paths_eval(ctx, 3, _lib.as_dp(xq), _lib.as_dp(f), None) == -1
    assert "gpg_paths_setup" in GP._err()
    assert lib.gpg_paths_coeff(ctx, _lib.as_dp(np.empty((5, pm.N))), None) == -1
    for S, M in ((0, 37), (1025, 37), (5, 0)):
        assert setup(S, M) == -1 and GP._err()
    assert lib.gpg_set_mean_uncertainty(ctx, 1) == 0
    assert setup(5, 37) == -1 and "mean" in GP._err()
    assert lib.gpg_set_mean_uncertainty(ctx, 0) == 0
    with pytest.raises(Exception, match="mean_unc"):
        GP.sample_paths(5, mean_unc=True)
    paths = _paths(GP, r)
    f0 = paths(xq)
    info, ok = GP.calc_lkd_all(GP.hp_vals)                                       # a likelihood call in between changes nothing
    assert ok
    assert np.array_equal(paths(xq), f0)
    # drawn paths (nothing explicit): shapes, reproducible from the seed, and they differ from path to path
    drawn = GP.sample_paths(3, n_features=64, seed=5)
    fd = drawn(xq)
    assert fd.shape == (3, 3) and np.all(np.isfinite(fd)) and np.abs(fd[0] - fd[1]).max() > 0
    assert np.array_equal(GP.sample_paths(3, n_features=64, seed=5)(xq), fd)
    with pytest.raises(Exception, match="no longer belong"):
        paths(xq)                                                                # another set was drawn on the model
    paths = _paths(GP, r)
    GP.setup_eval_model()
    with pytest.raises(Exception, match="no longer belong"):
        paths(xq)
    assert lib.gpg_paths_eval(ctx, 3, _lib.as_dp(xq), _lib.as_dp(f), None) == -1  # the device refuses as well
    assert "gpg_paths_setup" in GP._err()
    # before gpg_setup_eval
    GP.close()
    c = pm.c
    import gpgradpy_amd
    GP = gpgradpy_amd.GaussianProcess(c["d"], True, 'SqExp', 'precon')
    GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"])
    assert GP._lib.gpg_paths_setup(GP._ctx, 5, 37, _lib.as_dp(om), _lib.as_dp(ph), _lib.as_dp(w), _lib.as_dp(z), 1.0) == -1
    assert "gpg_setup_eval" in GP._err()
    GP.close()
    GP = gpgradpy_amd.GaussianProcess(c["d"], True, 'SqExp', 'rescale_origin')
    GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"])
    assert GP.b_use_data_scl
    GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(GP.make_hp_class(theta=c["theta"])))
    with pytest.raises(Exception, match="not setup for cases where data must be rescaled"):
        GP.sample_paths(5)
    GP.close()
