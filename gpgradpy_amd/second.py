"""Host arithmetic on the per-point posterior of [f, grad f]: what `GaussianProcess.eval_model_second` returns (the blocks come
from gpg_predict_second, include/gpgrad.h) and three quantities people build on the gradient covariance.  Functions of plain
NumPy arrays, so they can be checked without a device.

With m_j = dmudx[j] the posterior mean of grad f at x_j and C_j = cov[j, 1:, 1:] its covariance:
    expected_sq_grad_norm:  E |grad f(x_j)|^2 = |m_j|^2 + tr C_j                      (stationarity tests)
    active_subspace:        mean_j E[grad f grad f'] = mean_j (m_j m_j' + C_j)        and its eigendecomposition
    prob_descent:           P(dir . grad f(x_j) < 0) = Phi(-(dir . m_j) / sqrt(dir' C_j dir))
"""
from math import erf, sqrt

import numpy as np


class SecondResult:
    """Plain container: the attributes are listed in `fields`."""

    def __init__(self, **kw):
        self.fields = tuple(kw)
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        return 'SecondResult(' + ', '.join(self.fields) + ')'


def second_from_blocks(mu, dmudx, cov, d2mudx2=None, d2sigdx2=None):
    """SecondResult from the device arrays: sig = sqrt(max(0, cov_00)), dsigdx_k = cov_0,k+1 / sig (0 where sig == 0, as
    eval_model), grad_std_k = sqrt(max(0, cov_k+1,k+1))."""
    cov = np.asarray(cov, dtype=np.float64)
    nx, bs = cov.shape[0], cov.shape[1]
    if cov.shape != (nx, bs, bs) or np.shape(mu) != (nx,) or np.shape(dmudx) != (nx, bs - 1):
        raise ValueError(f'shapes do not match: mu {np.shape(mu)}, dmudx {np.shape(dmudx)}, cov {cov.shape}')
    sig = np.sqrt(np.maximum(cov[:, 0, 0], 0.0))
    inv_sig = np.divide(1.0, sig, out=np.zeros_like(sig), where=sig != 0)
    dsigdx = cov[:, 0, 1:] * inv_sig[:, None]
    grad_std = np.sqrt(np.maximum(np.diagonal(cov, axis1=1, axis2=2)[:, 1:], 0.0))
    return SecondResult(mu=mu, sig=sig, dmudx=dmudx, dsigdx=dsigdx, cov=cov, grad_std=grad_std, d2mudx2=d2mudx2,
                        d2sigdx2=d2sigdx2)


def _grad_parts(res):
    dmudx = np.asarray(res.dmudx, dtype=np.float64)
    cgg = np.asarray(res.cov, dtype=np.float64)[:, 1:, 1:]
    if dmudx.ndim != 2 or cgg.shape != (dmudx.shape[0],) + (dmudx.shape[1],) * 2:
        raise ValueError(f'shapes do not match: dmudx {dmudx.shape}, cov {np.shape(res.cov)}')
    return dmudx, cgg


def expected_sq_grad_norm(res):
    """[nx]: |dmudx_j|^2 + tr Cov_j(grad f)."""
    dmudx, cgg = _grad_parts(res)
    return np.sum(dmudx * dmudx, axis=1) + np.trace(cgg, axis1=1, axis2=2)


def active_subspace(res):
    """(C [d, d], eigenvalues [d] in descending order, eigenvectors [d, d] in columns) of
    C = mean_j (dmudx_j dmudx_j' + Cov_j(grad f)), the posterior expectation of the active-subspace matrix over the points."""
    dmudx, cgg = _grad_parts(res)
    Cm = (dmudx.T @ dmudx + np.sum(cgg, axis=0)) / dmudx.shape[0]
    Cm = 0.5 * (Cm + Cm.T)
    lam, vec = np.linalg.eigh(Cm)
    return Cm, lam[::-1].copy(), vec[:, ::-1].copy()


def prob_descent(res, direction):
    """[nx]: the posterior probability that `direction` [d] (or one direction per point, [nx, d]) is a descent direction at x_j,
    Phi(-(dir . dmudx_j) / sqrt(dir' Cov_j(grad f) dir)).  Where the directional variance is zero (or rounds below it) the
    gradient along the direction is known: 1 if dir . dmudx_j < 0, 0 if > 0, 0.5 if it is zero."""
    dmudx, cgg = _grad_parts(res)
    nx, d = dmudx.shape
    dirs = np.asarray(direction, dtype=np.float64)
    if dirs.shape == (d,):
        dirs = np.broadcast_to(dirs, (nx, d))
    if dirs.shape != (nx, d):
        raise ValueError(f'direction must have shape ({d},) or ({nx}, {d}), got {np.shape(direction)}')
    slope = np.einsum('jk,jk->j', dirs, dmudx)
    var = np.einsum('jk,jkl,jl->j', dirs, cgg, dirs)
    out = np.where(slope < 0, 1.0, np.where(slope > 0, 0.0, 0.5))
    ok = var > 0
    z = -slope[ok] / np.sqrt(var[ok])
    out[ok] = [0.5 * (1.0 + erf(v / sqrt(2.0))) for v in z]
    return out
