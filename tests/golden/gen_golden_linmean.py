#!/usr/bin/env python3
"""Golden vectors for the first-order polynomial mean ('poly_ord_1'), captured by running the *reference* in the build
container (import recipe of gen_golden.py / gen_golden_optz.py).

The reference carries the whole algebra of the linear mean (calc_vand, calc_aug_vand, calc_model_max_lkd_poly,
eval_mean_fun_poly: GpMeanFun.py:14-191); only set_mean_fun_op refuses the option (GpMeanFun.py:195-204).  After
construction this script therefore sets the three attributes that option would set,

    n_beta_coeff = beta_var_npara = dim + 1,   mean_fun_type = 'poly_ord_1',

and runs the usual hot path (calc_lkd_all -> optz_closed_form_hp -> set_hpara('set') -> eval_model).  The data are
Rosenbrock values plus an affine part of comparable norm, so that the trend matters.

The fixtures go to tests/golden/linmean/ (a directory of their own: the case list of the existing parity tests takes
every tests/golden/*.npz that has none of its known prefixes).

Usage:  python tests/golden/gen_golden_linmean.py      # rewrites tests/golden/linmean/linmean_*.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'linmean')
sys.path.insert(0, HERE)
from gen_golden import rosenbrock  # noqa: E402
from gen_golden_optz import _import_reference  # noqa: E402  (numba stub + the SciPy Latin hypercube behind smt.LHS)


def linear_mean(GP):
    GP.n_beta_coeff = GP.dim + 1
    GP.beta_var_npara = GP.dim + 1
    GP.mean_fun_type = 'poly_ord_1'
    return GP


def trend_data(rng, x):
    """Rosenbrock + c0 + x . c with ||c0 + x . c|| = ||Rosenbrock values||."""
    f, g = rosenbrock(x)
    c = rng.standard_normal(x.shape[1])
    c0 = rng.standard_normal()
    aff = c0 + x @ c
    s = np.linalg.norm(f) / np.linalg.norm(aff)
    return f + s * aff, g + s * c[None, :], s * c0, s * c


def run_case(GaussianProcess, name, n, d, kernel, noise, seed, use_grad=True, mask=False, hp_kernel=None):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, (n, d))
    f, g, c0, cvec = trend_data(rng, x)
    theta = 10.0 ** rng.uniform(-1.5, -0.3, d)
    if noise == 'none':
        std_f, std_g = np.zeros(n), np.zeros((n, d))
    else:
        std_f = 1e-2 * (1 + rng.uniform(0, 1, n))
        std_g = 1e-1 * (1 + rng.uniform(0, 1, (n, d)))
        f = f + std_f * rng.standard_normal(n)
        g = g + std_g * rng.standard_normal((n, d))
    bvec = None
    if mask:
        bvec = rng.random(n) > 0.35
        bvec[0], bvec[-1] = True, False
        g, std_g = g[bvec], std_g[bvec]
    GP = linear_mean(GaussianProcess(d, use_grad, kernel, 'precon'))
    if use_grad:
        GP.set_data(x, f, std_f, g, std_g, bvec)
    else:
        GP.set_data(x, f, std_f)
    noisy = bool(GP.b_has_noisy_data)
    varK_in = 2.5 if noisy else None
    hp = GP.make_hp_class(theta=theta, kernel=hp_kernel if hp_kernel is not None else GP.hp_kernel_default, varK=varK_in)
    lkd, ok = GP.calc_lkd_all(hp, calc_lkd=True, calc_cond=False, calc_grad=False)
    assert ok
    out = dict(name=name, n=n, d=d, kernel=kernel, noise=noise, use_grad=use_grad, wellcond=GP.wellcond_mtd, x=x, f=f,
               g=g if use_grad else np.zeros((0, d)), std_f=std_f, std_g=std_g if use_grad else np.array([]),
               theta=theta, varK_in=np.nan if varK_in is None else varK_in, var_fval=np.nan, var_fgrad=np.nan, etaK=GP._etaK,
               b_has_noisy_data=noisy, b_chofac_good=True, n_data=GP.n_data,
               bvec_use_grad=np.ones(n, dtype=bool) if bvec is None else bvec, trend_c0=c0, trend_c=cvec,
               hp_beta=np.asarray(lkd.hp_beta, dtype=float), hp_varK=np.nan if lkd.hp_varK is None else float(lkd.hp_varK),
               ln_det_Kmat=float(lkd.ln_det_Kmat), ln_lkd=float(lkd.ln_lkd))
    if hp.kernel is not None:
        out['hp_kernel'] = float(hp.kernel)
    if not mask:                                               # the reference's masked gradient is broken (KernelSqExp.py:552-554)
        lkd_g, ok_g = GP.calc_lkd_all(hp, calc_lkd=True, calc_cond=False, calc_grad=True)
        assert ok_g
        out['ln_lkd_grad'] = np.asarray(lkd_g.ln_lkd_grad, dtype=float)
        if lkd_g.hp_beta_grad is not None:                     # noisy path (CalcLkd.py:216-217)
            out['hp_beta_grad'] = np.asarray(lkd_g.hp_beta_grad, dtype=float)
    # ln_lkd of the same data with the constant mean, for the record: the trend must pay
    GP0 = GaussianProcess(d, use_grad, kernel, 'precon')
    if use_grad:
        GP0.set_data(x, f, std_f, g, std_g, bvec)
    else:
        GP0.set_data(x, f, std_f)
    out['ln_lkd_const_mean'] = float(GP0.calc_lkd_all(GP0.make_hp_class(theta=theta, kernel=hp.kernel, varK=varK_in))[0].ln_lkd)
    hp2 = GP.optz_closed_form_hp(hp)
    GP.set_hpara('set', 0, hp_vals=hp2)
    out['alpha'] = np.asarray(GP.invKernEta_fdiff, dtype=float)
    out['varK_model'] = float(hp2.varK)
    xq = rng.uniform(-2, 2, (4, d))
    xq[3] = x[0] + 1e-3                                        # close to a data point: small sig
    out['xq'] = xq
    if mask:                                                   # no Hessians with a mask (reference shape bug, KernelSqExp.py:451-452)
        mu, sig, dmudx, dsigdx = GP.eval_model(xq, calc_grad=True)[:4]
        out.update(mu=mu, sig=sig, dmudx=dmudx, dsigdx=dsigdx)
    else:
        res = [GP.eval_model(xq[i:i + 1], calc_grad=True, calc_hess=True) for i in range(xq.shape[0])]
        for k, key in enumerate(('mu', 'sig', 'dmudx', 'dsigdx', 'd2mudx2', 'd2sigdx2')):
            out[key] = np.array([r[k][0] for r in res])
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **out)
    print(f"{name}: N={GP.n_data} beta={out['hp_beta'][:3]}... ln_lkd={out['ln_lkd']:.8e} (constant mean {out['ln_lkd_const_mean']:.8e})"
          f" hp_beta_grad {'hp_beta_grad' in out}")


def run_optz(GaussianProcess, name, n, d, kernel, seed, n_x0=3):
    """One set_hpara('optz') run from explicit start rows hp_x0 (select_hp_optz_x0 replaced by them): inputs, start rows, box,
    optimum and the closed-form (beta, varK) there."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, (n, d))
    f, g, c0, cvec = trend_data(rng, x)
    GP = linear_mean(GaussianProcess(d, True, kernel, 'precon'))
    GP.optz_n_x0 = n_x0
    GP.init_optz_surr(3)
    # iteration 0: a single evaluation -> the initial hyperparameters are stored (GpHparaOptz.py:152-157), as gen_golden_optz.py
    z1 = np.zeros(1)
    GP.set_data(x[:1], f[:1], z1, g[:1], np.zeros((1, d)))
    GP.set_hpara('optz', 0)
    # iteration 1: the whole data set from explicit start rows inside the box the history gives
    GP.set_data(x, f, np.zeros(n), g, np.zeros((n, d)))
    box = GP.get_hp_x0_lhs_median(1, GP.hp_info_optz_lkd, n_x0)[1]
    hp_x0 = rng.uniform(box.lb + 0.2, box.ub - 0.2, (n_x0, d))   # log10(theta) start rows
    GP.select_hp_optz_x0 = lambda i_optz, hp_info: (hp_x0.copy(), box, 0.0)
    GP.set_hpara('optz', 1)
    hv = GP.hp_vals
    hp_final = GP.make_hp_class(theta=hv.theta, kernel=hv.kernel)
    out = dict(name=name, n=n, d=d, kernel=kernel, noise='none', x=x, f=f, g=g, hp_x0=hp_x0, box_lb=box.lb, box_ub=box.ub,
               theta=np.array(hv.theta, dtype=float), varK=float(hv.varK), beta=np.array(hv.beta, dtype=float),
               ln_lkd=float(GP.calc_lkd_all(hp_final)[0].ln_lkd), success=GP.hp_optz_success[1], iter_max=GP.hp_optz_iter_max[1],
               theta_hist0=GP.hp_theta_all[0], varK_hist0=GP.hp_varK_all[0], beta_hist0=GP.hp_beta_all[0])
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **out)
    print(f"{name}: theta={hv.theta} varK={hv.varK:.6e} beta={hv.beta} ln_lkd={out['ln_lkd']:.10e}")


def main():
    GaussianProcess = _import_reference()
    run_case(GaussianProcess, 'linmean_SqExp_none_n12_d3', 12, 3, 'SqExp', 'none', 61)
    run_case(GaussianProcess, 'linmean_Ma5f2_known_n40_d4', 40, 4, 'Ma5f2', 'known', 62)
    run_case(GaussianProcess, 'linmean_RatQu_none_n14_d3', 14, 3, 'RatQu', 'none', 63, hp_kernel=1.7)
    run_case(GaussianProcess, 'linmean_SqExp_none_n9_d16', 9, 16, 'SqExp', 'none', 64)
    run_case(GaussianProcess, 'linmean_SqExp_none_n30_d2_nograd', 30, 2, 'SqExp', 'none', 65, use_grad=False)
    run_case(GaussianProcess, 'linmean_SqExp_none_n17_d4_mask', 17, 4, 'SqExp', 'none', 66, mask=True)
    run_optz(GaussianProcess, 'linmean_optz_SqExp_n20_d2', 20, 2, 'SqExp', 67)


if __name__ == '__main__':
    main()
