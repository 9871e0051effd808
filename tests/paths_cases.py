"""Models and the NumPy restatement of the path formula shared by tests/test_paths_host.py (CPU) and tests/test_gpu_paths.py (device).

path_reference() is Matheron's rule written out with the oracle's pieces (oracle.gp_oracle.kern_grad, setup_eval_model through
tests/test_joint_host.JointModel, calc_all_K_w_chofac):
    f_s(x) = m(x) + k(x, X) c_s + sqrt(varK) phi(x)' w_s,       c_s = alpha - sqrt(varK) Kcov^-1 (Phi_X w_s + D^(1/2) z_s),
    phi(x)_m = sqrt(2 / M) cos(omega_m . x + b_m),   D = diag(Kcov) - diag(Kern)  (the matrices of the model, built with varK = 1).

The six models (include the tile and padding edges of the device code):
    sqexp_n17_d4          fixture SqExp_none_n17_d4: N = 85
    ma5f2_n23_d3_mask     fixture Ma5f2_known_n23_d3_mask: gradient mask, known noise
    ratqu_n12_d3_base     the data of fixture RatQu_unknown_n12_d3 (unknown noise) with wellcond 'base' and that method's nugget
    ma5f2_n33_d3          fixture Ma5f2_known_n33_d3_spread: N = 132 crosses the padding to 128
    sqexp_n40_d2_nograd   the first 40 points of fixture SqExp_none_n50_d2_nograd: use_grad = 0
    sqexp_n17_d4_lin      the data of SqExp_none_n17_d4 with the first-order mean (beta by GLS, as tests/dims_cases.DimsModel builds it)
"""
import numpy as np
from scipy.linalg import cho_solve

from oracle import gp_oracle as orc
from test_joint_host import JointModel, case

NAMES = ("sqexp_n17_d4", "ma5f2_n23_d3_mask", "ratqu_n12_d3_base", "ma5f2_n33_d3", "sqexp_n40_d2_nograd", "sqexp_n17_d4_lin")
N_FEAT, NX = 37, 70
S_VALUES = (5, 70)


def _case(name):
    if name == "sqexp_n17_d4":
        return dict(case("SqExp_none_n17_d4")), False
    if name == "ma5f2_n23_d3_mask":
        return dict(case("Ma5f2_known_n23_d3_mask")), False
    if name == "ma5f2_n33_d3":
        return dict(case("Ma5f2_known_n33_d3_spread")), False
    if name == "ratqu_n12_d3_base":
        c = dict(case("RatQu_unknown_n12_d3"))
        c["wellcond"] = "base"
        c["etaK"] = orc.calc_nugget(c["n"], c["d"], c["kernel_o"], True, "base")[1]
        c["name"] = name
        return c, False
    if name == "sqexp_n40_d2_nograd":
        c = dict(case("SqExp_none_n50_d2_nograd"))
        n = 40
        c.update(n=n, n_data=n, x=c["x"][:n], f=c["f"][:n], std_f=c["std_f"][:n], bvec_use_grad=np.ones(n, dtype=bool), name=name,
                 etaK=orc.calc_nugget(n, c["d"], c["kernel_o"], False)[0])
        return c, False
    if name == "sqexp_n17_d4_lin":
        c = dict(case("SqExp_none_n17_d4"))
        c["name"] = name
        return c, True
    raise KeyError(name)


class PathModel:
    """The oracle's posterior of one of the models above plus what the path formula needs: Kern, Kcov (varK = 1), D, the mask rows."""

    def __init__(self, name):
        from dims_cases import DimsModel
        self.name = name
        c, self.linear = _case(name)
        self.c = c
        jm = DimsModel(c, linear=True) if self.linear else JointModel(c)
        self.jm = jm
        self.mask, self.varK, self.chofac, self.alpha, self.beta = jm.mask, jm.varK, jm.chofac, jm.alpha, np.ravel(jm.beta)
        n, d = c["n"], c["d"]
        vf = None if np.isnan(c["var_fval"]) else c["var_fval"]
        vg = None if np.isnan(c["var_fgrad"]) else c["var_fgrad"]
        nv = orc.calc_noise_vec(n, d, c["use_grad"], c["std_f"], c["std_g"] if c["use_grad"] else None, vf, vg,
                                n_grad=int(c["bvec_use_grad"].sum()))
        wc = c["wellcond"] if c["use_grad"] else "base"
        fac = orc.calc_all_K_w_chofac(c["x"], c["theta"], c["kernel_o"], c["use_grad"], wc, c["etaK"], nv, varK=1.0, grad_mask=self.mask)
        assert fac.chofac is not None
        self.Kern, self.Kcov = fac.Kern, fac.Kcov
        self.D = np.diag(fac.Kcov) - np.diag(fac.Kern)
        assert np.all(self.D > 0)
        self.N = self.Kern.shape[0]
        assert self.N == c["n_data"] == self.alpha.size
        # rows of the full [n (d + 1)] derivative-major ordering the model holds
        if not c["use_grad"]:
            self.rows = np.arange(n)
        elif self.mask is None:
            self.rows = np.arange(n * (d + 1))
        else:
            g = np.flatnonzero(self.mask)
            self.rows = np.concatenate([np.arange(n)] + [n * (k + 1) + g for k in range(d)])

    def box_points(self, nx, seed):
        x = self.c["x"]
        return np.random.default_rng(seed).uniform(x.min(axis=0), x.max(axis=0), (nx, self.c["d"]))


_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = PathModel(name)
    return _MODELS[name]


def features(P, omega, phase, with_grad):
    """Phi [np (d + 1) or np, M]: value rows sqrt(2 / M) cos(omega . x + b), then d phi / d x_k for k = 0 .. d - 1 (derivative-major)."""
    M, d = omega.shape
    arg = P @ omega.T + phase[None, :]
    s = np.sqrt(2.0 / M)
    val = s * np.cos(arg)
    if not with_grad:
        return val
    sn = np.sin(arg)
    return np.vstack([val] + [-s * omega[:, k][None, :] * sn for k in range(d)])


def draws(pm, S, seed, M=N_FEAT):
    """Explicit (omega, phase, w, z) for S paths on model pm, frequencies by the kernel's own law (gpgradpy_amd.paths)."""
    from gpgradpy_amd.paths import draw_frequencies
    c = pm.c
    rng = np.random.default_rng(seed)
    omega, phase = draw_frequencies(c["kernel"], c["theta"], float(c["hp_kernel"]) if "hp_kernel" in c else None, M, rng)
    return omega, phase, rng.standard_normal((S, M)), rng.standard_normal((S, pm.N))


def coeff_reference(pm, omega, phase, w, z):
    """c [S, N] of the formula."""
    c = pm.c
    PhiX = features(c["x"], omega, phase, bool(c["use_grad"]))[pm.rows]
    rhs = PhiX @ w.T
    if z is not None:
        rhs = rhs + np.sqrt(pm.D)[:, None] * z.T
    return (pm.alpha[:, None] - np.sqrt(pm.varK) * cho_solve(pm.chofac, rhs)).T


def path_reference(pm, omega, phase, w, z, xq, coeff=None):
    """(f [S, nx], dfdx [S, nx, d]) of the formula at xq."""
    c = pm.c
    nx, d = xq.shape
    S = w.shape[0]
    if coeff is None:
        coeff = coeff_reference(pm, omega, phase, w, z)
    Kg = orc.kern_grad(c["x"], xq, c["theta"], c["kernel_o"], grad_cols=True, mask1=pm.mask)
    if not c["use_grad"]:
        Kg = Kg[:c["n"]]
    F = Kg.T @ coeff.T + np.sqrt(pm.varK) * (features(xq, omega, phase, True) @ w.T)       # [nx (d + 1), S]
    if pm.linear:
        F[:nx] += (pm.beta[0] + xq @ pm.beta[1:])[:, None]
        F[nx:] += np.repeat(pm.beta[1:], nx)[:, None]
    else:
        F[:nx] += pm.beta[0]
    return F[:nx].T.copy(), np.transpose(F[nx:].reshape(d, nx, S), (2, 1, 0)).copy()


def build_gp(pm):
    """The device model of pm, posterior set up (tests/test_gpu_joint._build for a case dict)."""
    import gpgradpy_amd
    c = pm.c
    GP = gpgradpy_amd.GaussianProcess(c["d"], c["use_grad"], c["kernel"], c["wellcond"] if c["use_grad"] else "base",
                                      mean_fun_type='poly_ord_1' if pm.linear else 'poly_ord_0')
    if c["use_grad"]:
        GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"], None if c["bvec_use_grad"].all() else c["bvec_use_grad"])
    else:
        GP.set_data(c["x"], c["f"], c["std_f"])
    noisy = c["b_has_noisy_data"]
    vf = None if np.isnan(c["var_fval"]) else c["var_fval"]
    vg = None if np.isnan(c["var_fgrad"]) else c["var_fgrad"]
    hp = GP.make_hp_class(theta=c["theta"], kernel=float(c["hp_kernel"]) if "hp_kernel" in c else None,
                          varK=c["varK_in"] if noisy else None, var_fval=vf, var_fgrad=vg)
    GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(hp))
    return GP
