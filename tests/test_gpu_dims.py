"""Every (kernel, dimension) instantiation of the device code, and the gradient-mask paths only a C caller reaches.

The kernels of assembly.hip, gradient.hip, joint.hip and solve.hip are compiled once per (KERN, D), meanunc.hip once per n_beta
(1 .. 17), and loo.hip picks its Gram kernel from bs = d + 1 (G = 5, G = 9, groups of 6 with an off-diagonal launch above).  The
other device files reach a thin slice of these; this file runs all 48 (kernel, d) pairs, d = 1 .. 16, on the seeded cases of
tests/dims_cases.py (n = 9 points, N <= 153, noise model by d % 3, a twin with points 2 and 5 stripped of their gradient), whose
conditions tests/test_dims_host.py asserts on the CPU.  The reference is the oracle throughout; where the mirror refuses
(likelihood gradient and Hessian with a mask: the reference itself fails there) the device is called through the C ABI and held to
the oracle's masked forms, which tests/test_dims_host.py pins to central differences of what the mask fixtures pin.

Checks and bounds (nothing here is fitted to what the device gives; every figure is printed, pytest -s, before it is asserted):
  a  assembly: Kern, Kcov (gpg_get_matrix 0 / 1) at KERN_RTOL / KERN_ATOL; beta, varK, ln det, ln_lkd by tolerances.check_scalars;
  b  posterior: mu, sig, dmudx, dsigdx by the MU / SIG rules and check_post_grad, alpha normwise; eval_model_var: sig2 to
     E_BOUND varK (the project's bound on the normalised variance) and dsig2dx by the dsigdx rule of check_post_grad;
  c  joint posterior, with and without the mean uncertainty, E <= E_BOUND; H = V' K^-1 V and calc_beta_cov by the rules of
     tests/test_gpu_meanunc.py; all with the constant and with the first-order mean (n_beta = 1 and d + 1: every MU_CASES entry);
  d  leave-one-out by point, mean_unc off and on: E_e, E_C <= E_BOUND, n_bad = 0, and below cond 1e5 the two relative checks of
     tests/test_gpu_loo.py (G = 5 for d <= 4, G = 9 for d <= 8, groups of 6 for bs = 10 .. 17: 6+4, 6+5, 6+6, 6+6+1, ..., 6+6+5);
  e  likelihood gradient, unmasked: calc_lkd_all(calc_grad=True) by tolerances.check_lkd_grad; g_aa and g_inv of gpg_lkd_grad each
     to LKD_GRAD_RTOL of its own largest component (sharper than their sum, in which they cancel);
  f  likelihood gradient, masked twin, through gpg_lkd_grad: parts and sum as in e; gpg_lkd_grad_batch with two rows gives the
     bits of two single calls;
  g  Hessians d2mudx2, d2sigdx2 at an outside point and at a training point, by the rule of tests/test_posterior_hess.py; masked
     twin through gpg_predict_hess.
Every test ends with factor / overlap / solve fallbacks == 0.

Measured on an MI355X (one run of this file: 288 tests in 7.8 s, the first 0.30 s, every other one 0.11 s or less), worst case over
the 96 cases as a fraction of its bound (1 = at the bound):
    a  Kern 0.17, Kcov 0.22 (RatQu d = 1: pow), every SqExp / Ma5f2 case 0.09 or less; scalars 2.7e-5;
    b  mu 8.0e-5, sig 2.2e-7, dmudx 1.5e-7, dsigdx 7.2e-8, alpha 8.6e-8, sig2 1.9e-8, dsig2dx 2.6e-8;
    c  joint E 1.5e-7, with the mean uncertainty 2.3e-7, mean 8.1e-5, its gradient rows 1.7e-7, H 2.1e-5, calc_beta_cov 1.2e-5;
    d  E_e 1.9e-4, E_C 1.8e-7, sqrt(diag C) 8.4e-8, standardised residual 9.3e-8;
    e  sum 9.0e-3, g_aa 1.4e-2, g_inv 1.2e-2;      f  sum 9.3e-3, g_aa 1.1e-2, g_inv 1.1e-2
       (1e-8 of the largest component: the level of the oracle's own differenced d Kcov / d theta, tests/test_dims_host.py);
    g  d2mudx2 1.0e-6, d2sigdx2 2.7e-8 unmasked; 2.0e-6, 2.7e-8 masked.
Mutation (run once, not kept): with (I - 1) * n in place of (I - 1) * ng in the row index of grad_contract_kernel, check f fails
on all 36 masked twins run with d >= 2, by 2.8e3 times its bound or more (d = 1 has no second gradient block, so the change is
none there), while a - e pass unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import dims_cases as dc
import tolerances as tol
from oracle import gp_oracle as orc
from test_joint_host import E_BOUND, joint_error, joint_reference
from test_loo_host import err_c, err_e
from test_meanunc_host import mean_gram_reference, meanunc_error, meanunc_reference
from test_posterior_hess import _check as check_hess

pytestmark = pytest.mark.gpu

PAIRS = pytest.mark.parametrize("pair", dc.PAIRS, ids=dc.pair_id)


def _hp(GP, c):
    _, _, vf, vg, varK = dc.noise_args(c)
    return GP.make_hp_class(theta=c["theta"].copy(), kernel=c.get("hp_kernel"), varK=varK, var_fval=vf, var_fgrad=vg)


def _build(c, linear=False, setup=True):
    import gpgradpy_amd
    GP = gpgradpy_amd.GaussianProcess(c["d"], True, c["kernel"], "precon", mean_fun_type="poly_ord_1" if linear else "poly_ord_0")
    GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"], None if c["bvec_use_grad"].all() else c["bvec_use_grad"])
    GP._etaK = GP._eta_Kgrad = c["etaK"]
    assert GP.n_data == c["n_data"] and GP.b_has_noisy_data == c["b_has_noisy_data"]
    if setup:
        GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(_hp(GP, c)))
    return GP


def _done(GP):
    assert GP.factor_fallbacks() == 0 and GP.overlap_fallbacks() == 0 and GP.solve_fallbacks() == 0
    GP.close()


def _used(got, want, rtol, atol):
    """Largest |got - want| / (atol + rtol |want|): the fraction of an assert_allclose bound that is used."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))


def _say(c, tag, **figs):
    print(f"{c['name']} [{tag}] " + "  ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    return figs


def _hold(figs):
    for k, v in figs.items():
        assert v <= 1.0, f"{k}: {v:.3e} of its bound"


# ---- a. assembly, b. posterior ---------------------------------------------------------------------------------------------------------
@PAIRS
def test_assembly_and_posterior(pair):
    for masked in (False, True):
        jm = dc.model(*pair, masked)
        c, r = jm.c, jm.lkd
        noisy, N, xq = c["b_has_noisy_data"], c["n_data"], c["xq"]
        GP = _build(c, setup=False)
        hp = _hp(GP, c)
        info, ok = GP.calc_lkd_all(hp)
        assert ok
        ref = dict(hp_beta=r.hp_beta, hp_varK=r.hp_varK, ln_det_Kmat=r.ln_det_Kmat, ln_lkd=r.ln_lkd)
        tol.check_scalars(info.hp_beta[0], info.hp_varK, info.ln_det_Kmat, info.ln_lkd, ref, N, noisy)
        scal = max(abs(info.hp_beta[0] / r.hp_beta[0] - 1) / tol.BETA_RTOL, abs(info.ln_lkd / r.ln_lkd - 1) / tol.LN_LKD_RTOL,
                   abs(info.ln_det_Kmat - r.ln_det_Kmat) / (tol.LN_DET_ATOL + tol.LN_DET_ATOL_PER_N * N),
                   0.0 if noisy else abs(info.hp_varK / r.hp_varK - 1) / tol.VARK_RTOL)
        if noisy:
            Kern, _, Kcov = GP.calc_all_K_w_chofac(None, hp, materialize=True)[:3]
        else:
            Kern, _, Kcov = GP.calc_Kern_w_chofac(None, hp, materialize=True)[:3]
        _hold(_say(c, "a", Kern=_used(Kern, r.factor.Kern, tol.KERN_RTOL, tol.KERN_ATOL),
                   Kcov=_used(Kcov, r.factor.Kcov, tol.KERN_RTOL, tol.KERN_ATOL), scalars=scal))

        hp2 = GP.optz_closed_form_hp(hp)
        np.testing.assert_allclose(hp2.varK, jm.varK, rtol=tol.VARK_RTOL)
        GP.set_hpara('set', 0, hp_vals=hp2)
        varK = jm.varK
        mu_o, sig_o, dmu_o, dsig_o = orc.eval_model_grad(jm.eval_model(), xq)
        mu0, sig0 = GP.eval_model(xq)[:2]
        mu, sig, dmu, dsig, h1, h2 = GP.eval_model(xq, calc_grad=True)
        assert h1 is None and h2 is None
        mu_atol, sig_atol = tol.MU_ATOL_SCALE * max(1.0, np.abs(mu_o).max()), tol.SIG_ATOL_SCALE * np.sqrt(varK)
        nx = xq.shape[0]
        _, cov_ref, _ = joint_reference(jm, xq, True)
        j = np.arange(nx)
        var_ref = np.diag(cov_ref)[:nx]
        dvar_ref = 2.0 * np.stack([cov_ref[j, (k + 1) * nx + j] for k in range(c["d"])], axis=1)
        sig2, dsig2dx, _ = GP.eval_model_var(xq, calc_grad=True)
        figs = _say(c, "b", mu=max(_used(mu, mu_o, tol.MU_RTOL, mu_atol), _used(mu0, mu_o, tol.MU_RTOL, mu_atol)),
                    sig=max(_used(sig, sig_o, tol.SIG_RTOL, sig_atol), _used(sig0, sig_o, tol.SIG_RTOL, sig_atol)),
                    dmudx=_used(dmu, dmu_o, tol.DMU_RTOL, tol.DMU_RTOL * max(1e-12, np.abs(dmu_o).max())),
                    dsigdx=_used(dsig, dsig_o, tol.DSIG_RTOL, tol.DSIG_RTOL * max(1e-12, np.abs(dsig_o).max())),
                    alpha=float(np.linalg.norm(GP.invKernEta_fdiff - jm.alpha) / (tol.ALPHA_NORMWISE * np.linalg.norm(jm.alpha))),
                    sig2=_used(sig2, var_ref, 0.0, E_BOUND * varK),
                    dsig2dx=_used(dsig2dx, dvar_ref, tol.DSIG_RTOL, tol.DSIG_RTOL * max(1e-12, np.abs(dvar_ref).max())))
        tol.check_post_grad(dmu, dsig, dict(dmudx=dmu_o, dsigdx=dsig_o))
        _hold(figs)
        _done(GP)


# ---- c. joint posterior, mean uncertainty, V' K^-1 V: both mean orders --------------------------------------------------------------
@PAIRS
def test_joint_and_mean_uncertainty(pair):
    from gpgradpy_amd import _lib
    for masked in (False, True):
        for linear in (False, True):
            jm = dc.model(*pair, masked, linear)
            c = jm.c
            xq, d = c["xq"], c["d"]
            nx = xq.shape[0]
            GP = _build(c, linear)
            varK = float(GP.hp_vals.varK)
            np.testing.assert_allclose(varK, jm.varK, rtol=tol.VARK_RTOL)
            mean, cov = GP.eval_model_joint(xq, calc_grad=True)
            mean_ref, cov_ref, Kqq = joint_reference(jm, xq, True)
            assert cov.shape == cov_ref.shape == (nx * (d + 1),) * 2 and np.array_equal(cov, cov.T)
            mean_u, cov_u = GP.eval_model_joint(xq, calc_grad=True, mean_unc=True)
            _, cov_tot, S, _ = meanunc_reference(jm, xq, True)
            assert np.array_equal(cov_u, cov_u.T) and np.array_equal(mean_u, mean)
            H_ref = mean_gram_reference(jm)
            nb = H_ref.shape[0]
            assert nb == (d + 1 if linear else 1) == GP.n_beta_coeff
            H = np.empty((nb, nb))
            assert GP._lib.gpg_mean_gram(GP._ctx, _lib.as_dp(H)) == 0, GP._err()
            assert np.array_equal(H, H.T)
            bcov, bcov_ref = GP.calc_beta_cov(), jm.varK * np.linalg.inv(H_ref)
            figs = _say(c, f"c n_beta={nb}", E=joint_error(cov, cov_ref, Kqq, jm.varK) / E_BOUND,
                        E_unc=meanunc_error(cov_u, cov_tot, S, jm.varK) / E_BOUND,
                        mean=_used(mean[:nx], mean_ref[:nx], tol.MU_RTOL, tol.MU_ATOL_SCALE * max(1.0, np.abs(mean_ref[:nx]).max())),
                        dmean=_used(mean[nx:], mean_ref[nx:], tol.DMU_RTOL, tol.DMU_RTOL * np.abs(mean_ref[nx:]).max()),
                        H=float(np.abs(H - H_ref).max() / np.abs(H_ref).max() / tol.BETA_RTOL),
                        beta_cov=float(np.abs(bcov - bcov_ref).max() / np.abs(bcov_ref).max() / (nb * np.linalg.cond(H_ref) * tol.BETA_RTOL)))
            _hold(figs)
            _done(GP)


# ---- d. leave-one-out ----------------------------------------------------------------------------------------------------------------
@PAIRS
def test_loo(pair):
    for masked in (False, True):
        jm = dc.model(*pair, masked)
        c = jm.c
        p, refs = dc.loo_problem_and_reference(*pair, masked)
        assert p.bs == c["d"] + 1
        cond = np.linalg.cond(p.Kcov)
        GP = _build(c)
        for mean_unc in (False, True):
            e_ref, C_ref = refs[mean_unc]
            res = GP.loo_cv(mean_unc=mean_unc, by='point')
            assert res.n_bad == 0 and res.cov.shape == C_ref.shape
            live = p.rows[:, 1:] >= 0
            assert np.all(np.isnan(res.resid_g[~live])) and int((~live).all(axis=1).sum()) == (len(dc.STRIPPED) if masked else 0)
            resid = np.full(p.N, np.nan)
            resid[p.rows[:, 0]] = res.resid_f
            resid[p.rows[:, 1:][live]] = res.resid_g[live]
            figs = dict(E_e=err_e(p, resid, e_ref) / E_BOUND, E_C=err_c(p, res.cov, C_ref) / E_BOUND)
            if cond <= 1e5:                                            # the WELL rule of tests/test_gpu_loo.py
                sd, sd_ref = np.empty(p.N), np.empty(p.N)
                for a in range(p.n):
                    I = p.rows[a][p.rows[a] >= 0]
                    sd[I], sd_ref[I] = np.sqrt(np.diag(res.cov[a])[:I.size]), np.sqrt(np.diag(C_ref[a])[:I.size])
                z, z_ref = resid / sd, e_ref / sd_ref
                figs["sd"] = _used(sd, sd_ref, tol.SIG_RTOL, 0.0)
                figs["z"] = _used(z, z_ref, 0.0, tol.SIG_RTOL * max(1.0, float(np.abs(z_ref).max())))
            _hold(_say(c, f"d mean_unc={int(mean_unc)} bs={p.bs} cond={cond:.1e}", **figs))
        _done(GP)


# ---- e, f. likelihood gradient -------------------------------------------------------------------------------------------------------
def _abi_lkd_grad(GP, hp_vals):
    """gpg_lkd_grad itself: (out, g_aa, g_inv) with the dim + 4 slots of the C ABI."""
    from gpgradpy_amd import _lib
    noisy = GP.b_has_noisy_data
    hp, keep = GP._make_hp(hp_vals, hp_vals.varK if noisy else 1.0, closed_form=not noisy)
    out = _lib.GpgLkdOut()
    g_aa, g_inv = np.full(GP.dim + 4, np.nan), np.full(GP.dim + 4, np.nan)
    rc = GP._lib.gpg_lkd_grad(GP._ctx, C.byref(hp), C.byref(out), _lib.as_dp(g_aa), _lib.as_dp(g_inv))
    assert rc == 0 and out.info == 0, GP._err()
    return out, g_aa, g_inv


def _check_parts(GP, c, tag, out, g_aa, g_inv, ref, cond):
    g_ref, aa_ref, inv_ref = ref
    s = 0.5 if c["b_has_noisy_data"] else 1.0 / (2.0 * out.varK)
    got = GP._slots_to_hp(s * g_aa + g_inv)
    aa, inv = GP._slots_to_hp(g_aa), GP._slots_to_hp(g_inv)
    assert got.shape == g_ref.shape == (GP.hp_info_optz_lkd.n_hp,)
    rt = tol.lkd_grad_rtol(cond)
    assert rt == tol.LKD_GRAD_RTOL
    figs = _say(c, tag, sum=_used(got, g_ref, rt, rt * np.abs(g_ref).max()),
                g_aa=float(np.abs(aa - aa_ref).max() / (tol.LKD_GRAD_RTOL * np.abs(aa_ref).max())),
                g_inv=float(np.abs(inv - inv_ref).max() / (tol.LKD_GRAD_RTOL * np.abs(inv_ref).max())))
    tol.check_lkd_grad(got, g_ref, cond=cond)
    _hold(figs)
    return got


@PAIRS
def test_lkd_grad_unmasked(pair):
    jm = dc.model(*pair, False)
    c = jm.c
    cond = float(np.linalg.cond(jm.lkd.factor.Kcov))
    ref = dc.lkd_grad_reference(*pair, False)
    GP = _build(c, setup=False)
    hp = _hp(GP, c)
    info, ok = GP.calc_lkd_all(hp, calc_grad=True)
    assert ok and np.isclose(info.ln_lkd, jm.lkd.ln_lkd, rtol=tol.LN_LKD_RTOL)
    tol.check_lkd_grad(info.ln_lkd_grad, ref[0], cond=cond)
    out, g_aa, g_inv = _abi_lkd_grad(GP, hp)
    got = _check_parts(GP, c, "e", out, g_aa, g_inv, ref, cond)
    assert np.array_equal(got, info.ln_lkd_grad)                       # the mirror combines the same two vectors
    _done(GP)


def _hp_row(GP, c, theta):
    """One row of gpg_lkd_batch / gpg_lkd_grad_batch: [theta(d), varK_mat, var_fval, var_fgrad, hp_kernel]."""
    _, _, vf, vg, varK = dc.noise_args(c)
    return np.concatenate((theta, [varK if GP.b_has_noisy_data else 1.0, -1.0 if vf is None else vf, -1.0 if vg is None else vg,
                                   c.get("hp_kernel", 0.0)]))


@PAIRS
def test_lkd_grad_masked_through_the_abi(pair):
    from gpgradpy_amd import _lib
    jm = dc.model(*pair, True)
    c, d = jm.c, jm.c["d"]
    cond = float(np.linalg.cond(jm.lkd.factor.Kcov))
    GP = _build(c, setup=False)
    assert GP.n_grad == c["n"] - len(dc.STRIPPED)
    hp = _hp(GP, c)
    with pytest.raises(NotImplementedError):                           # the mirror stays at reference parity
        GP.calc_lkd_all(hp, calc_grad=True)
    out, g_aa, g_inv = _abi_lkd_grad(GP, hp)
    np.testing.assert_allclose(out.ln_lkd, jm.lkd.ln_lkd, rtol=tol.LN_LKD_RTOL)
    _check_parts(GP, c, "f", out, g_aa, g_inv, dc.lkd_grad_reference(*pair, True), cond)
    # two rows in one batched call: the bits of two single calls
    hp_b = _hp(GP, c)
    hp_b.theta = 1.3 * c["theta"]
    out_b, g_aa_b, g_inv_b = _abi_lkd_grad(GP, hp_b)
    rows = np.ascontiguousarray(np.stack((_hp_row(GP, c, c["theta"]), _hp_row(GP, c, hp_b.theta))))
    outs = (_lib.GpgLkdOut * 2)()
    G_aa, G_inv = np.full((2, d + 4), np.nan), np.full((2, d + 4), np.nan)
    rc = GP._lib.gpg_lkd_grad_batch(GP._ctx, 2, _lib.as_dp(rows), d + 4, float(GP._etaK), GP._wellcond_code,
                                    int(not GP.b_has_noisy_data), outs, _lib.as_dp(G_aa), _lib.as_dp(G_inv))
    assert rc == 0, GP._err()
    for i, (o, a, b) in enumerate(((out, g_aa, g_inv), (out_b, g_aa_b, g_inv_b))):
        assert outs[i].info == 0 and outs[i].ln_lkd == o.ln_lkd and outs[i].ln_det == o.ln_det and outs[i].varK == o.varK
        assert np.array_equal(G_aa[i], a) and np.array_equal(G_inv[i], b), i
    assert not np.array_equal(G_aa[0], G_aa[1])
    _done(GP)


# ---- g. Hessians ---------------------------------------------------------------------------------------------------------------------
def _abi_hess(GP, x0):
    from gpgradpy_amd import _lib
    d = x0.size
    GP._set_mean_unc(False)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    mu, sig, dmu, dsig = np.empty(1), np.empty(1), np.empty(d), np.empty(d)
    d2mu, d2sig = np.full((d, d), np.nan), np.full((d, d), np.nan)
    rc = GP._lib.gpg_predict_hess(GP._ctx, _lib.as_dp(x0), float(GP.hp_vals.varK), _lib.as_dp(mu), _lib.as_dp(sig), _lib.as_dp(dmu),
                                  _lib.as_dp(dsig), _lib.as_dp(d2mu), _lib.as_dp(d2sig))
    assert rc == 0, GP._err()
    return mu[0], sig[0], dmu, dsig, d2mu, d2sig


@PAIRS
def test_hessians(pair):
    for masked in (False, True):
        jm = dc.model(*pair, masked)
        c, m = jm.c, jm.eval_model()
        d = c["d"]
        GP = _build(c)
        for i in dc.HESS_POINTS:
            x0 = c["xq"][i]
            o = orc.eval_model_hess(m, x0)
            if masked:
                with pytest.raises(NotImplementedError):               # the mirror stays at reference parity
                    GP.eval_model(x0, calc_grad=True, calc_hess=True, squeeze_nx=True)
                got = _abi_hess(GP, x0)
            else:
                got = GP.eval_model(x0, calc_grad=True, calc_hess=True, squeeze_nx=True)
            ref = dict(mu=o[0], sig=o[1], varK=jm.varK, d2mudx2=o[4], d2sigdx2=o[5])
            assert got[4].shape == (d, d) and got[5].shape == (d, d)
            H_mu, H_sig = o[4][0], o[5][0]
            sig_atol = 1e-6 * max(1.0, np.abs(H_sig).max()) / min(1.0, o[1][0] / np.sqrt(jm.varK) + 1e-12)
            figs = _say(c, f"g point {i}", d2mudx2=_used(got[4], H_mu, 1e-6, 1e-7 * np.abs(H_mu).max()),
                        d2sigdx2=_used(got[5], H_sig, 1e-4, sig_atol), sig_over_sqrt_varK=float(o[1][0] / np.sqrt(jm.varK)))
            np.testing.assert_allclose(got[4], got[4].T, rtol=1e-9, atol=1e-9 * np.abs(got[4]).max())
            check_hess(ref, 0, got)
            tol.check_post_grad(got[2][None, :], got[3][None, :], dict(dmudx=o[2], dsigdx=o[3]))
            _hold({k: v for k, v in figs.items() if k != "sig_over_sqrt_varK"})
        _done(GP)
