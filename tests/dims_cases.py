"""Seeded cases, one per (kernel, d) for the three kernels and d = 1 .. 16, shared by tests/test_dims_host.py (CPU) and
tests/test_gpu_dims.py (device).  No fixture files: the design is oracle.gp_oracle.synthetic_design and every reference value
comes from the oracle.

build_case(kernel, d, masked) returns a dict with the keys tests/test_joint_host.JointModel reads (the layout conftest.load_case
gives a fixture), so joint_reference, meanunc_reference, aug_vand and the brute-force leave-one-out of tests/test_loo_host.py take
it as they are.  Per case:
  * n = 9 points (N = 9 (d + 1) <= 153: one padded tile), theta_k = U(0.5, 2) * THETA_SCALE[d] / (d span^2) (THETA_SCALE is 1 except
    at d = 1, 2, 3 and 6: there the nine points are close in units of the correlation length and theta is raised until cond(Kcov)
    is below 3.3e5, where tolerances.lkd_grad_rtol is at its floor; COND_MAX is what the tests assert), alpha = 1.4 for RatQu;
  * noise model by d % 3: 'none' / 'known' (std_f 1e-2, std_g 1e-1, varK 2.5) / 'unknown' (var_fval 1e-4, var_fgrad 1e-2, varK 0.7),
    so the closed-form varK, the varK slot, and the var_fval / var_fgrad slots are all met;
  * nugget ETA = 1e-4 instead of the default of the design size (~1e-9): a noise-free model has sig2_raw ~ eta at a training point
    that carries its gradient, and the cases keep sig2_raw above SIG2_MIN there so that dsigdx and d2sigdx2 are on their regular
    branch;
  * the masked twin strips points 2 and 5 of their gradient (neither the first nor the last point, so gpos is -1 in the middle and
    shifted after it);
  * five query points: training point 0 (carries a gradient in both twins), training point 2 (its gradient is masked out in the
    twin), the midpoint of points 1 and 3, and two points outside the bounding box of the design.

DimsModel is JointModel for these cases; with linear=True it is the first-order-mean model (n_beta = d + 1) built the way
tests/test_linmean_golden.dense_linmean builds it, with the noise vector of the case (dense_linmean takes known noise only).
"""
import numpy as np
from scipy.linalg import cho_solve

from oracle import gp_oracle as orc
from test_joint_host import JointModel
from test_loo_host import LooProblem, _delete_and_predict
from test_meanunc_host import aug_vand

KERNELS = ("SqExp", "Ma5f2", "RatQu")
DIMS = tuple(range(1, 17))
PAIRS = tuple((k, d) for k in KERNELS for d in DIMS)
N_POINTS = 9
STRIPPED = (2, 5)
ETA = 1e-4
RATQU_ALPHA = 1.4
SPAN = 4.0                                  # synthetic_design draws from [-2, 2]^d
THETA_SCALE = {1: 6.0, 2: 4.0, 3: 3.0, 6: 2.0}      # every other d: 1
COND_MAX = 1e6                              # cond(Kcov) of every case
SIG2_MIN = 1e-8                             # sig2_raw at every query point
PIVOT_MIN = 1e-6                            # least pivot / diagonal entry of V' Kcov^-1 V (the device's rule refuses at 1e-12)
GRAD_REL_STEP = 1e-4                        # inner step of the oracle's d Kcov / d theta, see lkd_grad_reference
HESS_POINTS = (3, 0)                        # rows of xq: an outside point and the coincident training point


def pair_id(p):
    return f"{p[0]}-d{p[1]}"


def build_case(kernel, d, masked):
    n = N_POINTS
    X, f, g = orc.synthetic_design(n, d, seed=1000 + 17 * d + KERNELS.index(kernel))
    rng = np.random.default_rng(5000 + 17 * d + KERNELS.index(kernel))
    theta = rng.uniform(0.5, 2.0, d) * THETA_SCALE.get(d, 1.0) / (d * SPAN ** 2)
    mask = np.ones(n, dtype=bool)
    if masked:
        mask[list(STRIPPED)] = False
    ng = int(mask.sum())
    noise = ("none", "known", "unknown")[d % 3]
    std_f = std_g = None
    var_fval = var_fgrad = varK_in = np.nan
    if noise == "none":
        std_f, std_g = np.zeros(n), np.zeros((ng, d))
    elif noise == "known":
        std_f, std_g, varK_in = np.full(n, 1e-2), np.full((ng, d), 1e-1), 2.5
    else:
        var_fval, var_fgrad, varK_in = 1e-4, 1e-2, 0.7
    lo, hi = X.min(axis=0), X.max(axis=0)
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    sgn = np.where(rng.random((2, d)) < 0.5, -1.0, 1.0)
    out = ctr + sgn * half * rng.uniform(0.2, 0.9, (2, d))
    out[0, 0] = ctr[0] + sgn[0, 0] * 1.3 * half[0]                # outside the box through one face ...
    out[1, d - 1] = ctr[d - 1] + sgn[1, d - 1] * 1.6 * half[d - 1]
    out[1, 0] = ctr[0] - sgn[1, 0] * 1.2 * half[0]                # ... and through a corner (an edge of it for d > 2; d = 1: one face)
    xq = np.vstack((X[0], X[STRIPPED[0]], 0.5 * (X[1] + X[3]), out))
    c = dict(name=f"dims_{kernel}_{noise}_n{n}_d{d}" + ("_mask" if masked else ""), kernel=kernel, noise=noise, wellcond="precon",
             n=n, d=d, n_data=n + ng * d, use_grad=True, b_has_noisy_data=noise != "none", bvec_use_grad=mask,
             x=X, f=f, g=g[mask], std_f=std_f, std_g=std_g, var_fval=var_fval, var_fgrad=var_fgrad, varK_in=varK_in,
             theta=theta, etaK=ETA, xq=xq)
    if kernel == "RatQu":
        c["hp_kernel"] = RATQU_ALPHA
    c["kernel_o"] = ("RatQu", RATQU_ALPHA) if kernel == "RatQu" else kernel
    return c


def noise_args(c):
    """(std_f, std_g, var_fval, var_fgrad, varK) as the oracle takes them (None where the fixture layout has NaN / empty)."""
    vf = None if np.isnan(c["var_fval"]) else c["var_fval"]
    vg = None if np.isnan(c["var_fgrad"]) else c["var_fgrad"]
    return c["std_f"], c["std_g"], vf, vg, (c["varK_in"] if c["b_has_noisy_data"] else None)


def noise_vec(c):
    std_f, std_g, vf, vg, _ = noise_args(c)
    return orc.calc_noise_vec(c["n"], c["d"], True, std_f, std_g, vf, vg, n_grad=int(c["bvec_use_grad"].sum()))


class DimsModel(JointModel):
    """JointModel of a case of this file; linear=True: the model with the first-order mean (beta by GLS, n_beta = d + 1)."""

    def __init__(self, c, linear=False):
        if not linear:
            JointModel.__init__(self, c)
            assert not self.linear
            self.lkd = self._lkd(c)
            return
        self.c, self.linear = c, True
        self.mask = None if c["bvec_use_grad"].all() else c["bvec_use_grad"]
        y = orc.make_data_vec(c["f"], c["g"])
        nv, noisy = noise_vec(c), c["b_has_noisy_data"]
        fac = orc.calc_all_K_w_chofac(c["x"], c["theta"], c["kernel_o"], True, "precon", c["etaK"], nv,
                                      varK=c["varK_in"] if noisy else 1.0, grad_mask=self.mask)
        assert fac.chofac is not None
        V = aug_vand(self)
        KiV = cho_solve(fac.chofac, V)
        beta = np.linalg.solve(V.T @ KiV, KiV.T) @ y                            # GpMeanFun.py:102-107
        res = y - V @ beta
        self.varK = float(c["varK_in"]) if noisy else max(1e-32, (res @ cho_solve(fac.chofac, res)) / y.size)
        fac1 = fac if not noisy else orc.calc_all_K_w_chofac(c["x"], c["theta"], c["kernel_o"], True, "precon", c["etaK"], nv,
                                                             varK=1.0, grad_mask=self.mask)
        assert fac1.chofac is not None
        self.chofac, self.alpha, self.beta = fac1.chofac, cho_solve(fac1.chofac, res), beta
        self.lkd = None

    def _lkd(self, c):
        """The likelihood evaluation of the constant-mean model (LkdResult of the oracle; .factor.Kcov is the matrix factorised)."""
        r = orc.calc_lkd(c["x"], orc.make_data_vec(c["f"], c["g"]), c["theta"], c["kernel_o"], True, "precon", c["etaK"], noise_vec(c),
                         c["b_has_noisy_data"], varK=noise_args(c)[4], grad_mask=self.mask)
        assert r.ok
        return r

    def eval_model(self):
        """The oracle's EvalModel of the constant-mean model (the same factor and alpha as this object)."""
        c = self.c
        return orc.EvalModel(c["x"], np.asarray(c["theta"], float), c["kernel_o"], True, np.ravel(self.beta), self.varK,
                             self.chofac, self.alpha, self.mask)


_CASES, _MODELS, _LOO, _LKD_GRAD = {}, {}, {}, {}


def case(kernel, d, masked):
    key = (kernel, d, bool(masked))
    if key not in _CASES:
        _CASES[key] = build_case(*key)
    return _CASES[key]


def model(kernel, d, masked, linear=False):
    key = (kernel, d, bool(masked), bool(linear))
    if key not in _MODELS:
        _MODELS[key] = DimsModel(case(kernel, d, masked), linear)
    return _MODELS[key]


def loo_problem_and_reference(kernel, d, masked):
    """(LooProblem, {mean_unc: (e_ref [N], C_ref [n, bs, bs])}) of the constant-mean model: the brute force of
    tests/test_loo_host.py (delete the rows of a point, refit, predict)."""
    key = (kernel, d, bool(masked))
    if key not in _LOO:
        p = LooProblem(model(kernel, d, masked))
        e = {m: np.full(p.N, np.nan) for m in (False, True)}
        C = {m: np.zeros((p.n, p.bs, p.bs)) for m in (False, True)}
        for a in range(p.n):
            I = p.rows[a][p.rows[a] >= 0]
            for m, (ea, Ca) in _delete_and_predict(p, I).items():
                e[m][I] = ea
                C[m][a, :I.size, :I.size] = Ca
        _LOO[key] = (p, {m: (e[m], C[m]) for m in (False, True)})
    return _LOO[key]


def lkd_grad_reference(kernel, d, masked):
    """(gradient, g_aa, g_inv) of the oracle in hp_info_optz_lkd order [theta(d), alpha? (RatQu), varK?, var_fval?, var_fgrad?].
    Inner steps of the oracle's d Kcov / d hp: GRAD_REL_STEP = 1e-4 of theta and alpha (theta_k R_k^2 is O(1 / d) here, so the
    truncation (1e-4 theta R^2)^2 / 6 and the rounding eps / (1e-4 theta) per entry are both ~1e-10 of the entries; the default 1e-6
    has rounding 2e-8 at theta = 5e-3), and half the value for the variances, in which Kcov is linear (exact at any step)."""
    key = (kernel, d, bool(masked))
    if key not in _LKD_GRAD:
        c = case(kernel, d, masked)
        std_f, std_g, vf, vg, varK = noise_args(c)
        mask = None if c["bvec_use_grad"].all() else c["bvec_use_grad"]
        args = (c["x"], orc.make_data_vec(c["f"], c["g"]), c["theta"], c["kernel_o"], True, "precon", c["etaK"], std_f, std_g,
                c["b_has_noisy_data"])
        kw = dict(varK=varK, var_fval=vf, var_fgrad=vg, grad_mask=mask, rel_step=GRAD_REL_STEP, rel_step_var=0.5)
        _LKD_GRAD[key] = (orc.calc_lkd_grad(*args, **kw),) + orc.calc_lkd_grad(*args, return_parts=True, **kw)
    return _LKD_GRAD[key]


def gls_pivot_margin(H):
    """Least pivot of the Cholesky factorisation of H over the diagonal entry it started from."""
    L = np.linalg.cholesky(H)
    return float(np.min(np.diag(L) ** 2 / np.diag(H)))
