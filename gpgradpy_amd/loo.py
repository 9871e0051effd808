"""Host arithmetic of leave-one-out cross-validation: what `GaussianProcess.loo_cv` makes of the four arrays gpg_loo returns
(include/gpgrad.h).  Functions of plain NumPy arrays, so they can be checked without a device.

With B = Kcov^-1 (or Q = B - B V (V' B V)^-1 V' B when the mean coefficients are re-estimated without the point) and
qy = B (y - V beta) (or Q y):
    point a, rows I_a:  e_a = prec_a^-1 qy_a,  C_a = varK prec_a^-1   (prec_a the block of B / Q on I_a; both from the device)
    single row r:       e_r = qy_r / prec_rr,  var_r = varK / prec_rr
e = observed data minus its prediction from everything else, C / var the covariance of that prediction of the observed rows.
The log pseudo-likelihood is the sum of the Gaussian log densities of the left-out data under those predictions.
"""
import numpy as np

_LN_2PI = float(np.log(2.0 * np.pi))


class LooResult:
    """Plain container: the attributes are listed in `fields`."""

    def __init__(self, **kw):
        self.fields = tuple(kw)
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        return 'LooResult(' + ', '.join(self.fields) + ')'


def point_rows(n, dim, use_grad, bvec_use_grad=None):
    """rows [n, bs] (bs = dim + 1 with use_grad, else 1): the data_vec rows of every point, value row first, then d/dx_0 ..
    d/dx_(dim-1); -1 where a point carries no gradient.  The row layout of gpg_set_data: value rows 0 .. n - 1, the row of
    d/dx_k at the g-th gradient point is n + k ng + g."""
    if not use_grad:
        return np.arange(n, dtype=np.int64)[:, None]
    mask = np.ones(n, dtype=bool) if bvec_use_grad is None else np.asarray(bvec_use_grad, dtype=bool)
    if mask.shape != (n,):
        raise ValueError(f'bvec_use_grad must have {n} entries, got shape {mask.shape}')
    ng = int(mask.sum())
    gpos = np.where(mask, np.cumsum(mask) - 1, -1)
    rows = np.full((n, dim + 1), -1, dtype=np.int64)
    rows[:, 0] = np.arange(n)
    for k in range(dim):
        rows[mask, k + 1] = n + k * ng + gpos[mask]
    return rows


def loo_by_point(data_vec, rows, resid, cov):
    """Leave-one-point-out summary.  data_vec, resid [N]; rows [n, bs] (point_rows); cov [n, bs, bs] = C_a on the live rows.
    Returns a LooResult with mu_f, resid_f [n]; mu_g, resid_g [n, dim] (None without gradients; NaN where a point has no
    gradient); cov; z [n, bs] = Lc^-1 e_a with C_a = Lc Lc' (Cholesky whitening, NaN in the unused places);
    ln_pseudo_lkd_pt [n] = -1/2 (ln det(2 pi C_a) + e_a' C_a^-1 e_a), their sum ln_pseudo_lkd, and n_bad: the points whose
    block is NaN (marked bad on the device) or not positive definite here.  A bad point stays NaN everywhere, the total included."""
    data_vec = np.asarray(data_vec, dtype=np.float64)
    resid = np.asarray(resid, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    rows = np.asarray(rows)
    n, bs = rows.shape
    if cov.shape != (n, bs, bs) or data_vec.shape != resid.shape or data_vec.ndim != 1:
        raise ValueError(f'shapes do not match: data_vec {data_vec.shape}, resid {resid.shape}, rows {rows.shape}, cov {cov.shape}')
    live = rows >= 0
    e = np.full((n, bs), np.nan)
    e[live] = resid[rows[live]]
    y = np.full((n, bs), np.nan)
    y[live] = data_vec[rows[live]]
    z = np.full((n, bs), np.nan)
    lnp = np.full(n, np.nan)
    for a in range(n):
        m = int(live[a].sum())                     # the live rows are the leading ones: value row, then all dim gradient rows or none
        Ca, ea = cov[a, :m, :m], e[a, :m]
        if not (np.all(np.isfinite(Ca)) and np.all(np.isfinite(ea))):
            continue
        try:
            Lc = np.linalg.cholesky(Ca)
        except np.linalg.LinAlgError:
            continue
        za = np.linalg.solve(Lc, ea) if m > 1 else ea / Lc[0, 0]
        z[a, :m] = za
        lnp[a] = -0.5 * (m * _LN_2PI + 2.0 * float(np.sum(np.log(np.diag(Lc)))) + float(za @ za))
    bad = np.isnan(lnp)
    e[bad] = np.nan
    mu = y - e
    has_g = bs > 1
    return LooResult(mu_f=mu[:, 0], mu_g=mu[:, 1:] if has_g else None, resid_f=e[:, 0], resid_g=e[:, 1:] if has_g else None,
                     cov=cov, z=z, ln_pseudo_lkd_pt=lnp, ln_pseudo_lkd=float(np.sum(lnp)), n_bad=int(bad.sum()))


def loo_by_row(data_vec, rows, prec, qy, varK):
    """Every data row left out alone, from the same device call.  prec [n, bs, bs], qy [N].  Returns a LooResult with, in
    data_vec order [N]: mu, resid (e_r = qy_r / prec_rr), var (varK / prec_rr), z = e_r / sqrt(var_r), ln_pseudo_lkd_row
    = -1/2 (ln(2 pi var_r) + z_r^2), and their sum ln_pseudo_lkd; n_bad counts the rows with a diagonal entry that is not a
    positive finite number (NaN there and in the total)."""
    data_vec = np.asarray(data_vec, dtype=np.float64)
    qy = np.asarray(qy, dtype=np.float64)
    prec = np.asarray(prec, dtype=np.float64)
    rows = np.asarray(rows)
    n, bs = rows.shape
    if prec.shape != (n, bs, bs) or data_vec.shape != qy.shape or data_vec.ndim != 1:
        raise ValueError(f'shapes do not match: data_vec {data_vec.shape}, qy {qy.shape}, rows {rows.shape}, prec {prec.shape}')
    live = rows >= 0
    d = np.full(data_vec.size, np.nan)
    d[rows[live]] = np.diagonal(prec, axis1=1, axis2=2)[live]
    ok = np.isfinite(d) & (d > 0.0) & np.isfinite(qy)
    d = np.where(ok, d, np.nan)
    e = qy / d
    var = float(varK) / d
    z = e / np.sqrt(var)
    lnp = -0.5 * (_LN_2PI + np.log(var) + z * z)
    return LooResult(mu=data_vec - e, resid=e, var=var, z=z, ln_pseudo_lkd_row=lnp, ln_pseudo_lkd=float(np.sum(lnp)),
                     n_bad=int((~ok).sum()))
