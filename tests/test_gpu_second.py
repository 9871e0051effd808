"""Per-point gradient covariance and batched Hessians on the device (gpg_predict_second, gpg_set_second_chunk,
GaussianProcess.eval_model_second) against block_reference of tests/test_second_host.py -- the point-diagonal blocks of the oracle's
joint covariance, which that file pins to the fixtures and to orc.eval_model_hess -- and against orc.eval_model_hess itself.

Metric and bounds (none fitted to what the device gives; every figure is printed, pytest -s, before it is asserted):
    blocks:    E = max |gcov - block_ref|_jik / (varK sqrt(K0_ii K0_kk)) <= E_BOUND = 2e-7, the project's standing bound on the
               normalised covariance (tests/test_joint_host.py); with mean_unc the scale is S = diag(Kqq + U H^-1 U') as in
               tests/test_gpu_meanunc.py.  Blocks are exactly symmetric.
    mu, dmudx: the MU_* / DMU_RTOL rules of tests/tolerances.py, as tests/test_gpu_joint.py holds the joint mean.
    Hessians:  tests/test_posterior_hess._check against orc.eval_model_hess (d2mudx2 rtol 1e-6 / atol 1e-7 |H|max; d2sigdx2 rtol 1e-4 /
               atol 1e-6 max(1, |H|max) / min(1, sig / sqrt(varK))); with mean_unc the central-difference rule of
               tests/test_gpu_meanunc.py (eps 1e-5, rtol 1e-3, atol 1e-4 max(1, |H|max)).

Largest values measured on an MI355X (one run of this file: 75 tests in 4.7 s, the slowest 0.34 s):
    parity, E:  SqExp_none_n5_d2 1.4e-11 (1.6e-11 with mean_unc), SqExp_none_n50_d2_nograd 3.4e-12, SqExp_none_n64_d8 1.9e-13, every
                other fixture 2.4e-14 or less; against the diagonal blocks of eval_model_joint on the same context 1.4e-15 or less;
    Hessians, as a fraction of the bound of _check: d2mudx2 0.25 (SqExp_none_n5_d2), 0.10 (SqExp_none_n200_d4 at box points),
                7.4e-4 or less elsewhere; d2sigdx2 6.9e-5 or less; with mean_unc |H - central differences| 3.9e-8 at |H|max = 146,
                the switch changes d2sigdx2 by 0.17-0.45 |H|max;
    point tiles and chunks (SqExp_none_n200_d4): E 2.7e-14 or less for nx = 1 .. 130, 9.1e-14 at nx = 460 and 900; nx = 130 in
                chunks of 64 is the one-chunk result bit for bit, every field;
    every block size (96 cases, bs = 2 .. 17): E 3.1e-14 or less, d2mudx2 2.0e-6 and d2sigdx2 2.7e-8 of their bounds or less;
    K-chunks 1, 3, Npad / 64: E as with the automatic count to three digits (3.0e-15 on cfg5_combo_n120_d16, 1.9e-13 on
                SqExp_none_n64_d8); a point's block alone (nx = 1) and inside nx = 65 are the same bits (the forward sweep is
                row-independent in bits), so that assertion is on bits.

All of these fail without the feature: the library has no gpg_predict_second and the mirror no eval_model_second.
"""
import numpy as np
import pytest

import dims_cases as dc
import tolerances as tol
from oracle import gp_oracle as orc
from test_gpu_dims import _build as build_dims
from test_gpu_joint import _box_points, _build, _gp, _no_fallbacks
from test_joint_host import E_BOUND, PARITY, case, joint_model
from test_meanunc_host import outside_points
from test_posterior_hess import _check as check_hess
from test_second_host import block_error, block_reference, blocks_of, hess_reference

pytestmark = pytest.mark.gpu

N64, N200, N5, N17 = "SqExp_none_n64_d8", "SqExp_none_n200_d4", "SqExp_none_n5_d2", "Ma5f2_known_n17_d4"
CFG5 = "cfg5_combo_n120_d16"
LIN12, LIN17M = "linmean/linmean_SqExp_none_n12_d3", "linmean/linmean_SqExp_none_n17_d4_mask"


def _got(res, j):
    return res.mu[j], res.sig[j], res.dmudx[j], res.dsigdx[j], res.d2mudx2[j], res.d2sigdx2[j]


def _hess_used(res, ref, points):
    """Largest fraction of the two Hessian bounds of _check that is used at the rows `points` (for the printed figures)."""
    u_mu = u_sig = 0.0
    for j in points:
        Hm, Hs = ref["d2mudx2"][j], ref["d2sigdx2"][j]
        u_mu = max(u_mu, float(np.max(np.abs(res.d2mudx2[j] - Hm) / (1e-7 * np.abs(Hm).max() + 1e-6 * np.abs(Hm)))))
        at = 1e-6 * max(1.0, np.abs(Hs).max()) / min(1.0, ref["sig"][j] / np.sqrt(ref["varK"]) + 1e-12)
        u_sig = max(u_sig, float(np.max(np.abs(res.d2sigdx2[j] - Hs) / (at + 1e-4 * np.abs(Hs)))))
    return u_mu, u_sig


def _check_blocks(tag, res, jm, xq, mean_unc=False, ref=None):
    """E of the device blocks at xq against the oracle, printed, then asserted; returns (mean_ref, block_ref, scale)."""
    mean_ref, blk, scale = ref if ref is not None else block_reference(jm, xq, mean_unc)
    nx, d = xq.shape
    assert res.cov.shape == blk.shape == (nx, d + 1, d + 1)
    E = block_error(res.cov, blk, scale, jm.varK)
    print(f"{tag}: nx = {nx}  bs = {d + 1}  E = {E:.2e}")
    assert E <= E_BOUND
    assert np.array_equal(res.cov, np.transpose(res.cov, (0, 2, 1)))
    return mean_ref, blk, scale


def _check_hessians(tag, res, ref, points):
    u_mu, u_sig = _hess_used(res, ref, points)
    print(f"{tag}: Hessians at {len(list(points))} points, fraction of the bound used  d2mudx2 {u_mu:.2e}  d2sigdx2 {u_sig:.2e}")
    for j in points:
        check_hess(ref, j, _got(res, j))


def _check_mean(res, mean_ref, nx, d):
    np.testing.assert_allclose(res.mu, mean_ref[:nx], rtol=tol.MU_RTOL, atol=tol.MU_ATOL_SCALE * max(1.0, np.abs(mean_ref[:nx]).max()))
    np.testing.assert_allclose(res.dmudx, mean_ref[nx:].reshape(d, nx).T, rtol=tol.DMU_RTOL,
                               atol=tol.DMU_RTOL * max(1e-12, np.abs(mean_ref[nx:]).max()))


# ---- 1. parity with the oracle, the fixture's own query points ---------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_parity(name):
    jm, GP = joint_model(name), _gp(name)
    c, xq = jm.c, jm.c["xq"]
    nx, d = xq.shape
    np.testing.assert_allclose(float(GP.hp_vals.varK), jm.varK, rtol=tol.VARK_RTOL)
    res = GP.eval_model_second(xq)
    mean_ref, _, K0 = _check_blocks(name, res, jm, xq)
    np.testing.assert_allclose(res.mu, c["mu"], rtol=tol.MU_RTOL, atol=tol.MU_ATOL_SCALE * max(1.0, np.abs(c["mu"]).max()))
    np.testing.assert_allclose(res.dmudx, c["dmudx"], rtol=tol.DMU_RTOL, atol=tol.DMU_RTOL * max(1e-12, np.abs(c["dmudx"]).max()))
    _check_mean(res, mean_ref, nx, d)
    _check_hessians(name, res, hess_reference(jm, xq), range(nx))
    # the diagonal blocks of the joint matrix, on the same context
    cov_joint = GP.eval_model_joint(xq, calc_grad=True)[1]
    E = block_error(res.cov, blocks_of(cov_joint, nx), K0, jm.varK)
    print(f"{name}: against the diagonal blocks of eval_model_joint  E = {E:.2e}")
    assert E <= E_BOUND
    # without the Hessians: the same blocks and means
    res_c = GP.eval_model_second(xq, calc_hess=False)
    assert res_c.d2mudx2 is None and res_c.d2sigdx2 is None
    assert np.array_equal(res_c.cov, res.cov) and np.array_equal(res_c.mu, res.mu) and np.array_equal(res_c.dmudx, res.dmudx)
    # with the uncertainty of the mean coefficients
    res_u = GP.eval_model_second(xq, mean_unc=True)
    _check_blocks(f"{name} mean_unc", res_u, jm, xq, mean_unc=True)
    assert np.array_equal(res_u.mu, res.mu) and np.array_equal(res_u.dmudx, res.dmudx) and np.array_equal(res_u.d2mudx2, res.d2mudx2)
    assert np.all(np.diagonal(res_u.cov - res.cov, axis1=1, axis2=2) >= -E_BOUND * jm.varK * K0)
    _no_fallbacks(GP)


@pytest.mark.parametrize("name", (N17, LIN12, LIN17M))
def test_hessian_with_mean_uncertainty(name):
    """d2sigdx2 with the switch on: central differences of the device's own dsigdx (the rule of tests/test_gpu_meanunc.py), and the
    single-point path where the mirror offers it (no mask)."""
    jm, GP = joint_model(name), _gp(name)
    xq = outside_points(jm.c)[:2]
    d = xq.shape[1]
    res = GP.eval_model_second(xq, mean_unc=True)
    res_off = GP.eval_model_second(xq)
    eps = 1e-5
    for j in range(2):
        H = res.d2sigdx2[j]
        np.testing.assert_allclose(H, H.T, rtol=1e-9, atol=1e-9 * np.abs(H).max())
        pts = np.repeat(xq[j][None, :], 2 * d, axis=0)
        pts[np.arange(d), np.arange(d)] += eps
        pts[d + np.arange(d), np.arange(d)] -= eps
        dsig = GP.eval_model(pts, calc_grad=True, mean_unc=True)[3]
        fd = (dsig[:d] - dsig[d:]) / (2 * eps)
        print(f"{name} point {j}: |d2sigdx2|max = {np.abs(H).max():.3e}  |H - fd| = {np.abs(H - fd).max():.2e}  change by the switch "
              f"{np.abs(H - res_off.d2sigdx2[j]).max() / np.abs(H).max():.2e}")
        np.testing.assert_allclose(H, fd, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(H).max()))
        if jm.mask is None:
            one = GP.eval_model(xq[j], calc_grad=True, calc_hess=True, squeeze_nx=True, mean_unc=True)
            ref = dict(mu=[one[0]], sig=[one[1]], varK=jm.varK, d2mudx2=[one[4]], d2sigdx2=[one[5]])
            check_hess(ref, 0, _got(res, j))
    _no_fallbacks(GP)


# ---- 2. point-tile and chunk edges ----------------------------------------------------------------------------------------------
_EDGE = {}


def _edge_reference():
    """460 box points of SqExp_none_n200_d4 (every smaller set is a prefix: a block depends on its own point only), their block
    reference and the oracle's Hessians at a spread of them; computed once."""
    if not _EDGE:
        jm = joint_model(N200)
        xq = _box_points(jm.c, 460, 4242)
        pts = sorted(set(range(0, 460, 23)) | {1, 62, 63, 64, 65, 127, 128, 129, 447, 448, 459})
        _EDGE.update(jm=jm, xq=xq, blocks=block_reference(jm, xq), hess=hess_reference(jm, xq, pts), pts=pts)
    return _EDGE


def _prefix(e, nx):
    mean_ref, blk, K0 = e["blocks"]
    bs, n_all = blk.shape[1], blk.shape[0]
    mean = mean_ref.reshape(bs, n_all)[:, :nx].reshape(-1)
    return (mean, blk[:nx], K0[:nx]), [j for j in e["pts"] if j < nx]


@pytest.mark.parametrize("nx", (1, 63, 64, 65, 130))
def test_point_tile_edges(nx):
    e, GP = _edge_reference(), _gp(N200)
    jm, xq = e["jm"], e["xq"][:nx]
    ref, pts = _prefix(e, nx)
    res = GP.eval_model_second(xq)
    _check_blocks(f"{N200} nx={nx}", res, jm, xq, ref=ref)
    _check_mean(res, ref[0], nx, xq.shape[1])
    _check_hessians(f"{N200} nx={nx}", res, e["hess"], pts)
    _no_fallbacks(GP)


def test_chunks():
    e, GP = _edge_reference(), _gp(N200)
    jm, d = e["jm"], e["xq"].shape[1]
    xq = e["xq"][:130]
    ref, pts = _prefix(e, 130)
    whole = GP.eval_model_second(xq)
    try:
        GP.set_second_chunk(64)                                               # three chunks: 64, 64 and 2 points
        parts = GP.eval_model_second(xq)
        _check_blocks(f"{N200} nx=130 in chunks of 64", parts, jm, xq, ref=ref)
        _check_mean(parts, ref[0], 130, d)
        _check_hessians(f"{N200} nx=130 in chunks of 64", parts, e["hess"], pts)
        E = block_error(parts.cov, whole.cov, ref[2], jm.varK)
        same = all(np.array_equal(getattr(parts, f), getattr(whole, f), equal_nan=True) for f in whole.fields)
        print(f"{N200} nx=130: chunks of 64 against one chunk  E = {E:.2e}  bit-identical: {same}")
        assert E <= E_BOUND
        as_ref = dict(mu=whole.mu, sig=whole.sig, varK=jm.varK, d2mudx2=whole.d2mudx2, d2sigdx2=whole.d2sigdx2)
        for j in range(130):
            check_hess(as_ref, j, _got(parts, j))
        # nx = 460 (more than the 455 points gpg_predict_joint takes at d = 8): eight chunks, the last of 12 points
        big = GP.eval_model_second(e["xq"])
        _check_blocks(f"{N200} nx=460 in chunks of 64", big, jm, e["xq"], ref=e["blocks"])
        _check_mean(big, e["blocks"][0], 460, d)
        _check_hessians(f"{N200} nx=460 in chunks of 64", big, e["hess"], e["pts"])
    finally:
        GP.set_second_chunk(0)
    auto = GP.eval_model_second(e["xq"])                                      # the automatic chunk: 460 points at d = 4 are one chunk
    _check_blocks(f"{N200} nx=460, automatic chunk", auto, jm, e["xq"], ref=e["blocks"])
    _check_hessians(f"{N200} nx=460, automatic chunk", auto, e["hess"], e["pts"])
    # more points than gpg_predict_joint takes at d = 4 (819): 900 = the 460 points and the first 440 again (a block depends on its
    # own point only, so the reference is the one above); automatic chunks of 768 and 132 points
    from gpgradpy_amd import _lib
    xq2 = np.ascontiguousarray(np.vstack((e["xq"], e["xq"][:440])))
    assert 900 * (d + 1) > 4096
    with pytest.raises(_lib.GpgError):
        GP.eval_model_joint(xq2, calc_grad=True)
    two = GP.eval_model_second(xq2)
    mean_ref, blk, K0 = e["blocks"]
    E = max(block_error(two.cov[:460], blk, K0, jm.varK), block_error(two.cov[460:], blk[:440], K0[:440], jm.varK))
    print(f"{N200} nx=900, automatic chunks of 768 + 132  E = {E:.2e}")
    assert E <= E_BOUND
    for j in e["pts"]:
        check_hess(e["hess"], j, _got(two, j))
        if j < 440:
            check_hess(e["hess"], j, _got(two, 460 + j))
    _no_fallbacks(GP)


# ---- 3. every block size: bs = 2 .. 17, every register grouping and its off-diagonal launch ------------------------------------------
@pytest.mark.parametrize("pair", dc.PAIRS, ids=dc.pair_id)
def test_every_block_size(pair):
    for masked in (False, True):
        jm = dc.model(*pair, masked)
        c, m = jm.c, jm.eval_model()
        d = c["d"]
        xq = np.vstack((c["xq"], _box_points(c, 3, 77 + d)))
        nx = xq.shape[0]
        GP = build_dims(c)
        res = GP.eval_model_second(xq)                                        # the mirror takes the mask; the device honours it
        mean_ref, _, _ = _check_blocks(c["name"], res, jm, xq)
        _check_mean(res, mean_ref, nx, d)
        ref = dict(mu=mean_ref[:nx], sig=np.full(nx, np.nan), varK=jm.varK, d2mudx2=np.full((nx, d, d), np.nan),
                   d2sigdx2=np.full((nx, d, d), np.nan))
        for j in dc.HESS_POINTS:
            o = orc.eval_model_hess(m, xq[j])
            ref["sig"][j], ref["d2mudx2"][j], ref["d2sigdx2"][j] = o[1][0], o[4][0], o[5][0]
        _check_hessians(c["name"], res, ref, dc.HESS_POINTS)
        assert GP.factor_fallbacks() == 0 and GP.overlap_fallbacks() == 0 and GP.solve_fallbacks() == 0
        GP.close()


# ---- 4. K-chunks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", (CFG5, N64))
def test_k_chunks(name):
    jm, GP = joint_model(name), _gp(name)
    xq = jm.c["xq"]
    ktiles = ((jm.c["n_data"] + 127) // 128) * 128 // 64
    assert ktiles == {CFG5: 32, N64: 10}[name]
    ref = block_reference(jm, xq)
    hess = hess_reference(jm, xq, (0, 1))
    try:
        for n in (1, 3, ktiles):
            GP.set_gram_splits(n)
            res = GP.eval_model_second(xq)
            _check_blocks(f"{name} K-chunks={n}", res, jm, xq, ref=ref)
            _check_hessians(f"{name} K-chunks={n}", res, hess, (0, 1))
    finally:
        GP.set_gram_splits(0)
    _no_fallbacks(GP)


def test_automatic_k_chunks_depend_on_npad_only():
    """A point's block is the same bits alone (nx = 1) and as point 40 of 65 (another point tile count, other rows in the sweep)."""
    e, GP = _edge_reference(), _gp(N200)
    xq = e["xq"][:65]
    many = GP.eval_model_second(xq)
    for j in (0, 40, 64):
        alone = GP.eval_model_second(xq[j:j + 1])
        same = np.array_equal(alone.cov[0], many.cov[j])
        E = block_error(alone.cov, many.cov[j:j + 1], e["blocks"][2][j:j + 1], e["jm"].varK)
        print(f"{N200} point {j}: alone against inside nx = 65  E = {E:.2e}  bit-identical: {same}")
        assert same
        assert np.array_equal(alone.mu[0], many.mu[j]) and np.array_equal(alone.dmudx[0], many.dmudx[j])
    _no_fallbacks(GP)


# ---- 5. determinism and isolation -----------------------------------------------------------------------------------------------
def _others(GP, xq):
    a = GP.eval_model(xq, calc_grad=True)[:4]
    b = GP.eval_model_joint(xq, calc_grad=True)
    loo = GP.loo_cv()
    return tuple(a) + tuple(b) + (loo.resid_f, loo.resid_g, loo.cov)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_determinism_and_isolation():
    jm = joint_model(N64)
    GP = _build(N64)                                                            # a fresh context: the call grows the shared buffers
    xq = jm.c["xq"]
    before = _others(GP, xq)
    res = GP.eval_model_second(xq)
    _check_blocks(f"{N64} fresh context", res, jm, xq)
    res2 = GP.eval_model_second(xq)
    assert _same([getattr(res, f) for f in res.fields], [getattr(res2, f) for f in res.fields])
    assert _same(before, _others(GP, xq))
    for cap in (1, 3, 17):
        GP.set_max_workgroups(cap)
        res_c = GP.eval_model_second(xq)
        assert _same([getattr(res, f) for f in res.fields], [getattr(res_c, f) for f in res.fields]), cap
    GP.set_max_workgroups(0)
    GP.eval_model_second(xq, mean_unc=True)
    assert _same(before, _others(GP, xq))
    _no_fallbacks(GP)
    GP.close()


# ---- 6. batched equals single ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", (N17, N64))
def test_batched_equals_single(name):
    jm, GP = joint_model(name), _gp(name)
    xq = _box_points(jm.c, 5, 9)
    res = GP.eval_model_second(xq)
    for j in range(5):
        one = GP.eval_model(xq[j], calc_grad=True, calc_hess=True, squeeze_nx=True)    # the single-point path of the parent
        ref = dict(mu=[one[0]], sig=[one[1]], varK=jm.varK, d2mudx2=[one[4]], d2sigdx2=[one[5]])
        check_hess(ref, 0, _got(res, j))
        tol.check_post_grad(res.dmudx[j][None, :], res.dsigdx[j][None, :], dict(dmudx=one[2][None, :], dsigdx=one[3][None, :]))
    _no_fallbacks(GP)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors():
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    c = case(N5)
    xq = np.ascontiguousarray(c["xq"])
    nx, d = xq.shape
    mu = np.empty(nx)
    GP = _build(N5, setup=False)
    assert GP._lib.gpg_predict_second(GP._ctx, nx, _lib.as_dp(xq), 1.0, _lib.as_dp(mu), None, None, None, None) == -1
    assert "gpg_setup_eval" in GP._err()
    with pytest.raises((AssertionError, _lib.GpgError)):
        GP.eval_model_second(xq)
    GP.close()
    GP = _gp(N5)
    lib, ctx = GP._lib, GP._ctx
    assert lib.gpg_predict_second(ctx, 0, _lib.as_dp(xq), 1.0, _lib.as_dp(mu), None, None, None, None) == -1
    assert "nx" in GP._err()
    assert lib.gpg_predict_second(ctx, nx, _lib.as_dp(xq), 1.0, None, None, None, None, None) == -1
    assert "NULL" in GP._err()
    assert lib.gpg_predict_second(None, nx, _lib.as_dp(xq), 1.0, _lib.as_dp(mu), None, None, None, None) == -1
    assert lib.gpg_set_second_chunk(ctx, -1) == -1
    assert ">= 0" in GP._err()
    assert lib.gpg_set_second_chunk(ctx, 4096 // (d + 1) + 1) == -1
    assert "4096" in GP._err()
    with pytest.raises(_lib.GpgError):
        GP.set_second_chunk(-3)
    assert lib.gpg_predict_second(ctx, nx, _lib.as_dp(xq), 1.0, _lib.as_dp(mu), None, None, None, None) == 0   # the context still answers
    assert np.array_equal(mu, GP.eval_model_second(xq, calc_hess=False).mu)
    _no_fallbacks(GP)
    GP = gpgradpy_amd.GaussianProcess(c["d"], True, 'SqExp', 'rescale_origin')
    GP.set_data(c["x"], c["f"], c["std_f"], c["g"], c["std_g"])
    assert GP.b_use_data_scl
    GP.set_hpara('set', 0, hp_vals=GP.optz_closed_form_hp(GP.make_hp_class(theta=c["theta"])))
    with pytest.raises(Exception, match="not setup for cases where data must be rescaled"):
        GP.eval_model_second(xq)
    with pytest.raises(AssertionError):
        GP.eval_model(xq[:2], calc_grad=True, calc_hess=True)                  # eval_model keeps its one-point rule
    GP.close()
