"""Posterior sample paths: the host side of gpg_paths_setup / gpg_paths_eval / gpg_paths_coeff (include/gpgrad.h).

A path is a draw from the posterior AS A FUNCTION (pathwise conditioning, Matheron's rule, on a random-Fourier-feature prior):
    f_s(x) = m(x) + k(x, X) c_s + sqrt(varK) phi(x)' w_s,       c_s = alpha - sqrt(varK) Kcov^-1 (Phi_X w_s + D^(1/2) z_s),
    phi(x)_m = sqrt(2 / M) cos(omega_m . x + phase_m).
The device needs (omega, phase, w, z) only; the frequency law of each kernel lives here:
    SqExp   k = exp(-sum_k theta_k r_k^2):                     omega_k = sqrt(2 theta_k) z_k
    RatQu   k = (1 + s / alpha)^-alpha, a Gamma mixture of SqExp: tau ~ Gamma(shape alpha, scale 1 / alpha) per feature,
                                                               omega_k = sqrt(2 theta_k tau) z_k
    Ma5f2   a multivariate Student-t spectrum with 5 degrees of freedom: g ~ chi^2_5 per feature,
                                                               omega_k = sqrt(theta_k) z_k sqrt(5 / g)
with z ~ N(0, I) and the phase uniform on [0, 2 pi), so that E[phi(x) . phi(x')] is the unit-variance kernel.
Functions of plain NumPy arrays except PosteriorPaths.__call__ and its two properties, which go to the device.
"""
import numpy as np

KERNELS = ('SqExp', 'Ma5f2', 'RatQu')
MAX_PATHS, MAX_FEATURES = 1024, 65536


def draw_frequencies(kernel_type, theta, hp_kernel, n_features, rng):
    """(omega [M, dim], phase [M]) of M = n_features random Fourier features of the unit-variance kernel `kernel_type` with
    length-scale parameters theta [dim] (hp_kernel: alpha of RatQu, ignored by the others).  rng: a numpy Generator, or a seed."""
    if kernel_type not in KERNELS:
        raise ValueError(f'kernel_type must be one of {KERNELS}, got {kernel_type!r}')
    theta = np.asarray(theta, dtype=np.float64)
    if theta.ndim != 1 or theta.size < 1 or not np.all(np.isfinite(theta)) or np.any(theta <= 0):
        raise ValueError(f'theta must be a vector of positive numbers, got {theta!r}')
    M = int(n_features)
    if M != n_features or not 1 <= M <= MAX_FEATURES:
        raise ValueError(f'n_features must be an integer in [1, {MAX_FEATURES}], got {n_features!r}')
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    z = rng.standard_normal((M, theta.size))
    if kernel_type == 'SqExp':
        omega = np.sqrt(2.0 * theta)[None, :] * z
    elif kernel_type == 'RatQu':
        if hp_kernel is None or not np.isfinite(hp_kernel) or hp_kernel <= 0:
            raise ValueError(f'RatQu needs its hyperparameter alpha > 0 in hp_kernel, got {hp_kernel!r}')
        tau = rng.gamma(shape=float(hp_kernel), scale=1.0 / float(hp_kernel), size=M)
        omega = np.sqrt(2.0 * theta[None, :] * tau[:, None]) * z
    else:
        g = rng.chisquare(5.0, size=M)
        omega = np.sqrt(theta)[None, :] * z * np.sqrt(5.0 / g)[:, None]
    phase = rng.uniform(0.0, 2.0 * np.pi, M)
    return np.ascontiguousarray(omega), phase


def _as_shape(name, a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f'{name} must have shape {shape}, got {a.shape}')
    if not np.all(np.isfinite(a)):
        raise ValueError(f'{name} has entries that are not finite')
    return a


def prepare_draws(kernel_type, theta, hp_kernel, n_data, n_paths, n_features=4096, seed=None, omega=None, phase=None, w=None, z=None,
                  noise_draw=True):
    """What gpg_paths_setup takes, validated: (omega [M, dim], phase [M], w [S, M], z [S, n_data] or None).  Whatever is not given
    is drawn from np.random.default_rng(seed), in the order frequencies, w, z; omega and phase come together or not at all, and
    then M is their length.  noise_draw=False: z is None (no noise / nugget draw: paths of the noise-free part only)."""
    S = int(n_paths)
    if S != n_paths or not 1 <= S <= MAX_PATHS:
        raise ValueError(f'n_paths must be an integer in [1, {MAX_PATHS}], got {n_paths!r}')
    dim = np.asarray(theta).size
    rng = np.random.default_rng(seed)
    if (omega is None) != (phase is None):
        raise ValueError('omega and phase must be given together')
    if omega is None:
        omega, phase = draw_frequencies(kernel_type, theta, hp_kernel, n_features, rng)
    else:
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        if omega.ndim != 2 or omega.shape[1] != dim or not 1 <= omega.shape[0] <= MAX_FEATURES:
            raise ValueError(f'omega must have shape (M, {dim}) with 1 <= M <= {MAX_FEATURES}, got {omega.shape}')
        omega = _as_shape('omega', omega, omega.shape)
        phase = _as_shape('phase', phase, (omega.shape[0],))
    M = omega.shape[0]
    w = rng.standard_normal((S, M)) if w is None else _as_shape('w', w, (S, M))
    if not noise_draw:
        if z is not None:
            raise ValueError('z given together with noise_draw=False')
    else:
        z = rng.standard_normal((S, int(n_data))) if z is None else _as_shape('z', z, (S, int(n_data)))
    return omega, phase, w, z


class PosteriorPaths:
    """S sample paths of the posterior a GaussianProcess had set up when sample_paths() made this object.  paths(xq) evaluates the
    same S functions at any points, in any number of calls; the object raises once the model's posterior has been set up again (or
    another set of paths was drawn on it: the device keeps one set)."""

    def __init__(self, gp, n_paths, dim, n_data, omega, phase, w, z):
        self._gp, self.n_paths, self.dim, self.n_data = gp, int(n_paths), int(dim), int(n_data)
        self.omega, self.phase, self.w, self.z = omega, phase, w, z

    def _live(self):
        gp = self._gp
        if gp is None or getattr(gp, '_paths_current', None) is not self:
            raise Exception('these sample paths no longer belong to the model: its posterior was set up again (or other paths were '
                            'drawn on it); call sample_paths() again')
        return gp

    def _points(self, xq):
        xq = np.asarray(xq, dtype=np.float64)
        if xq.ndim == 1:
            xq = xq[None, :]
        if xq.ndim != 2 or xq.shape[1] != self.dim or xq.shape[0] < 1:
            raise ValueError(f'xq must have shape (nx, {self.dim}) with nx >= 1, got {xq.shape}')
        if not np.all(np.isfinite(xq)):
            raise ValueError('xq has entries that are not finite')
        return np.ascontiguousarray(xq)

    def __call__(self, xq, calc_grad=False):
        """f [S, nx], or (f, dfdx [S, nx, dim]) with calc_grad: the exact gradient of each path."""
        xq = self._points(xq)
        gp = self._live()
        return gp._paths_eval(self, xq, bool(calc_grad))

    @property
    def coeff(self):
        """c [S, n_data]: the coefficient vectors c_s of the formula above (gpg_paths_coeff)."""
        return self._live()._paths_coeff(self)[0]

    @property
    def ddiag(self):
        """D [n_data]: the diagonal the model adds to the kernel matrix (noise / varK plus the nugget), as it was used."""
        return self._live()._paths_coeff(self)[1]
