"""The parts of tests/test_gpu_dims.py that need no device: the oracle's gradient masks in the likelihood gradient and the
posterior Hessian, and the conditions the seeded cases of tests/dims_cases.py have to keep so that the device tests can hold
every quantity to the project's tightest tolerance.  Every figure is printed (pytest -s) before it is asserted.

Oracle (oracle/gp_oracle.py: calc_lkd_grad / _kcov_only with grad_mask and return_parts, kern_hess_x / eval_model_hess with a
training-side mask):
  * an all-true mask gives the bits of no mask; the two parts recombine to the gradient, s g_aa + g_inv, to 1e-12 of its largest
    component (the same products summed in another order);
  * a masked kern_hess_x is the column selection of the full one, and the masked eval_model_hess agrees with central differences
    of the oracle's own masked posterior gradients (eval_model_grad, pinned by the mask fixtures) by the rule of
    tests/test_posterior_hess.py;
  * the masked adjoint gradient against central differences of the oracle's own masked ln_lkd (calc_lkd(grad_mask=...), what the
    mask fixtures pin), relative steps 1e-4, 1e-5, 1e-6 in every hyperparameter, error = max |g - fd| / max |g|, best of the three
    steps per case.  Measured over the 48 masked twins: worst case 1.9e-8 (RatQu d = 9), median 1.8e-9; per step the worst
    cases are 4.4e-8 (1e-4: truncation), 8.8e-8 (1e-5) and 1.3e-6 (1e-6: rounding of ln_lkd).  FD_BOUND = 1.9e-7 is ten times the
    measured worst case and 50 times below the 1e-5 of the largest component that the bound may not exceed.
    The oracle gradient is taken with the inner steps of dims_cases.lkd_grad_reference (1e-4 theta for d Kcov / d theta, half the
    value for the three variances, in which Kcov is linear): with calc_lkd_grad's default 1e-6 for every slot the same
    comparison stalls at 5e-7 whatever the outer step, because d Kcov / d var_fval is then a difference of 2e-10 between
    entries of size varK.

Conditions of the 96 cases (48 (kernel, d) pairs and their masked twins), measured here:
    cond(Kcov) 7.2e2 .. 3.0e5 (<= COND_MAX = 1e6, and below 3.3e5, so tolerances.lkd_grad_rtol is at its floor of 1e-6);
    least sig2_raw over the five query points 3.7e-5 (>= SIG2_MIN = 1e-8; the same with the mean uncertainty on, which only adds);
    least pivot / diagonal entry of V' Kcov^-1 V with the first-order mean 0.71 (>= PIVOT_MIN = 1e-6; the device refuses at 1e-12);
    every factorisation succeeds: the likelihood's and the posterior's matrix, constant and first-order mean, and the 9 refits
    of the brute-force leave-one-out with their GLS systems.
The oracle pass of one (kernel, d) pair with its twin -- models of both mean orders, joint / mean-uncertainty / leave-one-out
references, likelihood gradient with parts, Hessians -- takes 0.01 s (d = 1) to 0.8 s (d = 16), 7.4 s for all 48; the whole file 18 s.
"""
import time

import numpy as np
import pytest

import dims_cases as dc
import tolerances as tol
from oracle import gp_oracle as orc
from test_joint_host import joint_reference
from test_meanunc_host import mean_gram_reference, meanunc_reference

FD_STEPS = (1e-4, 1e-5, 1e-6)
FD_BOUND = 1.9e-7
SAME_BITS = (("SqExp", 2), ("Ma5f2", 5), ("RatQu", 3), ("SqExp", 7))       # noise models unknown, unknown, none, known


def _lkd_grad_args(c, mask):
    std_f, std_g, vf, vg, varK = dc.noise_args(c)
    args = (c["x"], orc.make_data_vec(c["f"], c["g"]), c["theta"], c["kernel_o"], True, "precon", c["etaK"], std_f, std_g,
            c["b_has_noisy_data"])
    return args, dict(varK=varK, var_fval=vf, var_fgrad=vg, grad_mask=mask)


def _hp_vector(c):
    """The optimised hyperparameters in hp_info_optz_lkd order: [theta(d), alpha? (RatQu), varK?, var_fval?, var_fgrad?]."""
    _, _, vf, vg, varK = dc.noise_args(c)
    v = list(c["theta"])
    if c["kernel"] == "RatQu":
        v.append(c["hp_kernel"])
    if c["b_has_noisy_data"]:
        v.append(varK)
        v += [x for x in (vf, vg) if x is not None]
    return np.array(v, dtype=float)


def _ln_lkd(c, v, mask):
    d = c["d"]
    k = d
    kernel = c["kernel_o"]
    if c["kernel"] == "RatQu":
        kernel = ("RatQu", v[k])
        k += 1
    std_f, std_g, vf, vg, varK = dc.noise_args(c)
    if c["b_has_noisy_data"]:
        varK = v[k]
        k += 1
        if vf is not None:
            vf, vg = v[k], v[k + 1]
    nv = orc.calc_noise_vec(c["n"], d, True, std_f, std_g, vf, vg, n_grad=int(c["bvec_use_grad"].sum()))
    r = orc.calc_lkd(c["x"], orc.make_data_vec(c["f"], c["g"]), v[:d], kernel, True, "precon", c["etaK"], nv, c["b_has_noisy_data"],
                     varK=varK, grad_mask=mask)
    assert r.ok
    return r.ln_lkd


# ---- 1. the oracle's masks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,d", SAME_BITS)
def test_all_true_mask_gives_the_bits_of_no_mask(kernel, d):
    c = dc.case(kernel, d, False)
    full = np.ones(c["n"], dtype=bool)
    args, kw = _lkd_grad_args(c, None)
    g0 = orc.calc_lkd_grad(*args, **kw)
    p0 = orc.calc_lkd_grad(*args, return_parts=True, **kw)
    kw["grad_mask"] = full
    assert np.array_equal(g0, orc.calc_lkd_grad(*args, **kw))
    p1 = orc.calc_lkd_grad(*args, return_parts=True, **kw)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])
    assert g0.shape == p0[0].shape == p0[1].shape == _hp_vector(c).shape
    m0 = dc.model(kernel, d, False).eval_model()
    m1 = orc.EvalModel(m0.X, m0.theta, m0.kernel, True, m0.beta, m0.varK, m0.chofac, m0.alpha, full)
    for x in c["xq"]:
        assert np.array_equal(orc.kern_hess_x(x, c["x"], c["theta"], c["kernel_o"], True),
                              orc.kern_hess_x(x, c["x"], c["theta"], c["kernel_o"], True, full))
        for u, v in zip(orc.eval_model_hess(m0, x), orc.eval_model_hess(m1, x)):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("pair", dc.PAIRS, ids=dc.pair_id)
def test_parts_recombine_to_the_gradient(pair, both):
    jm = dc.model(*pair, both)
    g, g_aa, g_inv = dc.lkd_grad_reference(*pair, both)
    s = 0.5 if jm.c["b_has_noisy_data"] else 1.0 / (2.0 * jm.lkd.hp_varK)
    err = np.abs(s * g_aa + g_inv - g).max() / np.abs(g).max()
    cancel = np.abs(g).max() / max(np.abs(s * g_aa).max(), np.abs(g_inv).max())
    print(f"{jm.c['name']}: |s g_aa + g_inv - g| = {err:.2e} of max   (|g|max / largest part = {cancel:.2e})")
    assert err <= 1e-12 / min(1.0, cancel)


@pytest.mark.parametrize("kernel,d", SAME_BITS + (("Ma5f2", 1), ("RatQu", 16)))
def test_masked_kern_hess_x_is_the_column_selection(kernel, d):
    c = dc.case(kernel, d, True)
    mask, n = c["bvec_use_grad"], c["n"]
    idx = orc._mask_index(n, d, mask)
    assert idx.size == c["n_data"] == n + (n - len(dc.STRIPPED)) * d
    for x in c["xq"]:
        H = orc.kern_hess_x(x, c["x"], c["theta"], c["kernel_o"], True)
        Hm = orc.kern_hess_x(x, c["x"], c["theta"], c["kernel_o"], True, mask)
        assert Hm.shape == (d, d, c["n_data"]) and np.array_equal(Hm, H[:, :, idx])
        assert np.all(np.isfinite(Hm))


@pytest.mark.parametrize("pair", dc.PAIRS, ids=dc.pair_id)
def test_masked_hessian_against_central_differences_of_the_masked_gradients(pair):
    """eval_model_hess with a mask against (eval_model_grad(x + h e_k) - eval_model_grad(x - h e_k)) / 2h of the same masked model,
    at the outside point, by the rule tests/test_posterior_hess.py holds the device to (h = 1e-5; rtol 1e-4 / 1e-3,
    atol 1e-5 |H_mu|max / 1e-4 max(1, |H_sig|max))."""
    jm = dc.model(*pair, True)
    m, d = jm.eval_model(), jm.c["d"]
    x0 = jm.c["xq"][dc.HESS_POINTS[0]]
    H_mu, H_sig = (h[0] for h in orc.eval_model_hess(m, x0)[4:6])
    np.testing.assert_allclose(H_mu, H_mu.T, rtol=1e-9, atol=1e-9 * np.abs(H_mu).max())
    np.testing.assert_allclose(H_sig, H_sig.T, rtol=1e-9, atol=1e-9 * np.abs(H_sig).max())
    eps, worst = 1e-5, [0.0, 0.0]
    for k in range(d):
        xp, xm = x0.copy(), x0.copy()
        xp[k] += eps
        xm[k] -= eps
        gp_, gm_ = orc.eval_model_grad(m, xp), orc.eval_model_grad(m, xm)
        fd_mu, fd_sig = (gp_[2][0] - gm_[2][0]) / (2 * eps), (gp_[3][0] - gm_[3][0]) / (2 * eps)
        worst = [max(worst[0], np.abs(H_mu[k] - fd_mu).max() / np.abs(H_mu).max()),
                 max(worst[1], np.abs(H_sig[k] - fd_sig).max() / max(1.0, np.abs(H_sig).max()))]
        np.testing.assert_allclose(H_mu[k], fd_mu, rtol=1e-4, atol=1e-5 * np.abs(H_mu).max())
        np.testing.assert_allclose(H_sig[k], fd_sig, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(H_sig).max()))
    print(f"{jm.c['name']}: |H_mu - fd| {worst[0]:.2e} of max   |H_sig - fd| {worst[1]:.2e} of max(1, max)")


@pytest.mark.parametrize("pair", dc.PAIRS, ids=dc.pair_id)
def test_masked_adjoint_gradient_against_central_differences(pair):
    jm = dc.model(*pair, True)
    c = jm.c
    g = dc.lkd_grad_reference(*pair, True)[0]
    v = _hp_vector(c)
    assert g.shape == v.shape
    errs = []
    for step in FD_STEPS:
        fd = np.empty_like(v)
        for k in range(v.size):
            h = step * v[k]
            vp, vm = v.copy(), v.copy()
            vp[k] += h
            vm[k] -= h
            fd[k] = (_ln_lkd(c, vp, jm.mask) - _ln_lkd(c, vm, jm.mask)) / (vp[k] - vm[k])
        errs.append(float(np.abs(g - fd).max() / np.abs(g).max()))
    print(f"{c['name']}: n_hp = {v.size}  |g - fd| / |g|max at steps {FD_STEPS}: " + "  ".join(f"{e:.2e}" for e in errs)
          + f"   best {min(errs):.2e}")
    assert FD_BOUND <= 1e-5
    assert min(errs) <= FD_BOUND


# ---- 2. the conditions of the cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", dc.PAIRS, ids=dc.pair_id)
def test_case_conditions(pair):
    kernel, d = pair
    t0 = time.perf_counter()
    for masked in (False, True):
        jm, jl = dc.model(kernel, d, masked), dc.model(kernel, d, masked, linear=True)
        c = jm.c
        n, xq = c["n"], c["xq"]
        assert c["n_data"] <= 170 and xq.shape == (5, d) and c["noise"] == ("none", "known", "unknown")[d % 3]
        assert c["bvec_use_grad"][0] and c["bvec_use_grad"][-1] and (not c["bvec_use_grad"].all()) == masked
        assert np.array_equal(xq[0], c["x"][0]) and np.array_equal(xq[1], c["x"][dc.STRIPPED[0]])
        lo, hi = c["x"].min(axis=0), c["x"].max(axis=0)
        assert all(np.any((x < lo) | (x > hi)) for x in xq[3:]) and np.all((xq[2] >= lo) & (xq[2] <= hi))
        cond = float(np.linalg.cond(jm.lkd.factor.Kcov))
        s2 = []
        for m_, lin in ((jm, False), (jl, True)):
            for unc in (False, True):
                cov = (meanunc_reference(m_, xq, False)[1] if unc else joint_reference(m_, xq, False)[1]) / m_.varK
                s2.append(float(np.diag(cov).min()))
        H1 = mean_gram_reference(jl)
        piv = min(dc.gls_pivot_margin(H1), dc.gls_pivot_margin(mean_gram_reference(jm)))
        p, refs = dc.loo_problem_and_reference(kernel, d, masked)                       # raises if a refit is not positive definite
        assert all(np.all(np.isfinite(e[p.rows[p.rows >= 0]])) and np.all(np.isfinite(C)) for e, C in refs.values())
        g, g_aa, g_inv = dc.lkd_grad_reference(kernel, d, masked)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(g_aa)) and np.all(np.isfinite(g_inv))
        em = jm.eval_model()
        for i in dc.HESS_POINTS:
            assert all(np.all(np.isfinite(h)) for h in orc.eval_model_hess(em, xq[i]))
        print(f"{c['name']}: N = {c['n_data']}  cond(Kcov) = {cond:.2e}  least sig2_raw = {min(s2):.2e}  least GLS pivot / diagonal = {piv:.2e}")
        assert cond <= dc.COND_MAX and tol.lkd_grad_rtol(cond) == tol.LKD_GRAD_RTOL
        assert min(s2) >= dc.SIG2_MIN
        assert piv >= dc.PIVOT_MIN
    print(f"{kernel} d = {d}: oracle pass of the pair {time.perf_counter() - t0:.2f} s")


def test_every_pair_and_every_noise_model_is_there():
    assert len(dc.PAIRS) == 48 and len(set(dc.PAIRS)) == 48
    assert {d + 1 for d in dc.DIMS} | {1} == set(range(1, 18))                           # n_beta of the two mean orders: every MU_CASES entry
    assert {dc.case("SqExp", d, False)["noise"] for d in dc.DIMS} == {"none", "known", "unknown"}
    assert {d + 1 for d in dc.DIMS} >= {5, 9, 10, 11, 12, 13, 17}                         # block sizes of the leave-one-out routes
