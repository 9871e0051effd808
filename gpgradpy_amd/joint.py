"""Host arithmetic of posterior sampling: draws from the joint Gaussian that `GaussianProcess.eval_model_joint` returns.

The covariance has at most 4096 rows (include/gpgrad.h: gpg_predict_joint), so one symmetric eigendecomposition on the
host is not on any hot path; the device Cholesky is not used for it (a posterior covariance is routinely singular to
rounding -- at a training point, for instance -- which an eigendecomposition with clipping handles and a Cholesky does not).
"""
import numpy as np


def draw_from_joint(mean, cov, z):
    """Samples mean + z A^T with A A^T = cov: mean [m], cov [m, m], z [n_samples, m] standard normals -> [n_samples, m].

    cov is symmetrised, decomposed as V diag(lam) V^T (np.linalg.eigh), negative eigenvalues (rounding of a positive
    semi-definite matrix) are clipped to zero and A = V sqrt(lam)."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    m = mean.size
    if mean.ndim != 1 or cov.shape != (m, m):
        raise ValueError(f'mean must be [m] and cov [m, m], got {mean.shape} and {cov.shape}')
    if z.ndim != 2 or z.shape[1] != m:
        raise ValueError(f'z must be [n_samples, {m}], got {z.shape}')
    lam, V = np.linalg.eigh(0.5 * (cov + cov.T))
    A = V * np.sqrt(np.clip(lam, 0.0, None))
    return mean + z @ A.T
