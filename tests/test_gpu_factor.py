"""GPU (MI355X): the Cholesky factor itself, on every device schedule, with the matrix edge on and next to the tile edges.

Every (case, schedule) downloads the matrix that is factorised and the factor and checks A = L L^T entry by entry
against the rounding-error bound of tests/factor_checks.py, then (L L^T) v and (L L^T)^-1 v through gpg_factor_apply
and ln det against the downloaded factor.  Schedules that must agree bit for bit are compared on the factor, and a
factorisation that must stop is asked for the exact pivot.  Cases: tests/factor_cases.py (their LAPACK twins run in
tests/test_factor_host.py).

Each test prints one line `FACTOR_RATIO ...` with its worst ratios to the bounds (pytest -s shows them)."""
import ctypes as C
import functools

import numpy as np
import pytest

import factor_cases as fc
import factor_checks as chk

pytestmark = pytest.mark.gpu

# name -> (factor mode, panel, fuse_max_tiles, task order, pair mode, kernel that must have run)
SCHEDULES = {
    "blocked128":      ("blocked", 128, 48, -1, 2, "blocked"),
    "tile64_fuse_o0":  ("tile64", None, 48, 0, 2, "tile64"),
    "tile64_fuse_o1":  ("tile64", None, 48, 1, 2, "tile64"),
    "tile64_split_o0": ("tile64", None, 0, 0, 2, "tile64"),
    "tile64_split_o1": ("tile64", None, 0, 1, 2, "tile64"),
    "tile128_o0":      ("tile128", None, 48, 0, 0, "tile128"),
    "tile128_o1":      ("tile128", None, 48, 1, 0, "tile128"),
    "pair128_o0":      ("tile128", None, 48, 0, 1, "pair128"),
    "pair128_o1":      ("tile128", None, 48, 1, 1, "pair128"),
    "auto":            ("auto", None, 48, -1, 2, "tile64"),
}
CASES = {c.name: c for c in fc.CASES}


def _apply_schedule(GP, name, max_wg=0):
    mode, panel, fuse, order, pair, _ = SCHEDULES[name]
    GP.set_factor_mode(mode)
    GP.set_panel(panel if panel else 128)
    GP.set_fuse_max_tiles(fuse)
    GP.set_task_order(order)
    assert GP._lib.gpg_set_pair_mode(GP._ctx, pair) == 0
    GP.set_max_workgroups(max_wg)


@functools.lru_cache(maxsize=None)
def _gp(name):
    """One device model per case, shared by the schedules (each test sets every switch it depends on)."""
    import gpgradpy_amd
    c = CASES[name]
    X, f, g = fc.case_data(c)
    GP = gpgradpy_amd.GaussianProcess(c.d, c.use_grad, c.kernel, c.wellcond)
    if c.use_grad:
        GP.set_data(X, f, np.zeros(c.n), g, np.zeros((c.n, c.d)))
    else:
        GP.set_data(X, f, np.zeros(c.n))
    assert GP.n_data == fc.case_N(c) and GP.wellcond_mtd == c.wellcond
    GP._etaK = GP._eta_Kgrad = c.etaK
    return GP


def _hp(GP, theta, hp_kernel=None):
    """(gpg_hp, keep-alive) of a noise-free evaluation: varK_mat = 1, closed-form varK."""
    return GP._make_hp(GP.make_hp_class(theta=np.asarray(theta, dtype=np.float64), kernel=hp_kernel), 1.0, closed_form=True)


def _matrix(GP, hp, which):
    from gpgradpy_amd import _lib
    out = np.empty((GP.n_data, GP.n_data))
    rc = GP._lib.gpg_get_matrix(GP._ctx, C.byref(hp) if hp is not None else None, which, _lib.as_dp(out))
    assert rc == 0, (rc, GP._err())
    return out


def _lkd(GP, hp):
    from gpgradpy_amd import _lib
    out = _lib.GpgLkdOut()
    rc = GP._lib.gpg_lkd(GP._ctx, C.byref(hp), C.byref(out))
    return rc, out


def _apply(GP, op, v):
    from gpgradpy_amd import _lib
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.full(v.size, np.nan)
    rc = GP._lib.gpg_factor_apply(GP._ctx, op, _lib.as_dp(v), _lib.as_dp(out))
    assert rc == 0, (rc, GP._err())
    return out


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name", list(CASES))
def test_factor_entrywise(name, sched):
    """A = L L^T entry by entry, products and solves through the factor, ln det -- one case on one schedule.

    'base': which = 3 is L itself and is compared with which = 2.  'precon': which = 3 is P L and is compared with which = 1
    (Kcov) under the wider count of factor_checks (PRECON_S, PRECON_C); gpg_factor_apply works with L, recovered here as
    (P L) / sqrt(diag Kern) at UNSCALE_S more roundings.  ln det: the device reports 2 (sum ln L_ii + sum ln p_i), p = sqrt(dvec),
    which is 2 sum ln (P L)_ii up to the two roundings of each extracted diagonal entry (4 N u in all); the tolerance takes the
    larger logarithms of the two sums it is made of."""
    c = CASES[name]
    GP = _gp(name)
    N = GP.n_data
    GP._etaK = GP._eta_Kgrad = c.etaK
    _apply_schedule(GP, sched)
    hp, keep = _hp(GP, c.theta, c.hp_kernel)
    precon = c.wellcond == "precon"
    # (downloads of which = 0 .. 2 re-assemble the workspace: they come before the factorisation)
    A = _matrix(GP, hp, 1 if precon else 2)
    p = np.sqrt(np.diag(_matrix(GP, hp, 0))) if precon else None
    rc, out = _lkd(GP, hp)
    assert rc == 0 and out.info == 0, (rc, GP._err())
    assert GP.last_factor() == (SCHEDULES[sched][5], 1)
    assert GP.factor_fallbacks() == 0
    F = _matrix(GP, None, 3)
    s = chk.DEVICE_S + (chk.PRECON_S if precon else 0)
    r_fac = chk.check_factor(A, F, s=s, kcov_c=chk.PRECON_C if precon else 0)

    L = F / p[:, None] if precon else F
    s_app = chk.DEVICE_S + (chk.UNSCALE_S if precon else 0)
    e_last = np.zeros(N)
    e_last[-1] = 1.0                                          # the last real row: the one next to the padding
    r_app = [0.0, 0.0]
    for v in (np.random.default_rng(1234).standard_normal(N), e_last):
        for op in (0, 1):
            r_app[op] = max(r_app[op], chk.check_apply(L, v, _apply(GP, op, v), op, s=s_app))

    dL = np.diag(L)
    if precon:
        ref = 2.0 * np.sum(np.log(np.diag(F)))
        tol = N * 4.0 * chk.U * (np.abs(np.log(dL)).max() + np.abs(np.log(p)).max()) + 4.0 * N * chk.U
    else:
        ref = 2.0 * np.sum(np.log(dL))
        tol = chk.lndet_tolerance(dL)
    err = abs(out.ln_det - ref)
    print(f"FACTOR_RATIO case={name} sched={sched} factor={r_fac:.4f} apply0={r_app[0]:.4f} apply1={r_app[1]:.4f} lndet={err / tol:.4f}")
    assert err <= tol, (out.ln_det, ref, tol)


BITWISE_N = ("sqexp_n193", "sqexp_n385", "sqexp_n640")
BITWISE_GROUPS = {
    "tile64_fuse": ("tile64_fuse_o0", "tile64_fuse_o1"),
    "tile64_split": ("tile64_split_o0", "tile64_split_o1"),
    "tile128": ("tile128_o0", "tile128_o1", "pair128_o0", "pair128_o1"),
}


@pytest.mark.parametrize("group", list(BITWISE_GROUPS))
@pytest.mark.parametrize("name", BITWISE_N)
def test_factor_bitwise_across_orders_caps_and_pairs(name, group):
    """With the tile size and the fuse setting fixed, the factor must be the same bits under both ticket orders, under 0
    (all), 1 and 3 persistent workgroups -- which change which finalisation path a tile takes and when -- and, on 128-tiles,
    with and without tile pairs."""
    c = CASES[name]
    GP = _gp(name)
    GP._etaK = GP._eta_Kgrad = c.etaK
    hp, keep = _hp(GP, c.theta, c.hp_kernel)
    ref = ref_ln = None
    for sched in BITWISE_GROUPS[group]:
        for cap in (0, 1, 3):
            _apply_schedule(GP, sched, max_wg=cap)
            rc, out = _lkd(GP, hp)
            assert rc == 0 and GP.last_factor() == (SCHEDULES[sched][5], 1) and GP.factor_fallbacks() == 0
            F = _matrix(GP, None, 3)
            if ref is None:
                ref, ref_ln = F, out.ln_lkd
                continue
            diff = np.flatnonzero(F.view(np.uint64) != ref.view(np.uint64))
            assert diff.size == 0, (sched, cap, diff.size, np.unravel_index(diff[0], F.shape))
            assert out.ln_lkd == ref_ln
    GP.set_max_workgroups(0)


@functools.lru_cache(maxsize=None)
def _gp_fail():
    import gpgradpy_amd
    GP = gpgradpy_amd.GaussianProcess(2, False, "SqExp", "base")
    return GP


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("m", fc.FAIL_M)
def test_failing_pivot_index(m, sched):
    """The factorisation stops at pivot m exactly (LAPACK's info, tests/test_factor_host.py), whichever code computes the
    index -- inside a 16-column sub-block, across a 64- or 128-tile edge, in the last, partly padded tile, in the last row --
    and the next well-posed evaluation on the same context succeeds."""
    GP = _gp_fail()
    X, eta = fc.failing_pivot_case(m)
    GP.set_data(X, np.sin(X[:, 0]) + 0.1 * X[:, 1], np.zeros(fc.FAIL_N))
    assert GP.n_data == fc.FAIL_N
    _apply_schedule(GP, sched)
    GP._etaK = GP._eta_Kgrad = eta
    hp, keep = _hp(GP, fc.FAIL_THETA)
    rc, out = _lkd(GP, hp)
    assert rc == m and out.info == m, (rc, out.info, m, GP._err())
    assert GP.last_factor() == (SCHEDULES[sched][5], 1) and GP.factor_fallbacks() == 0
    GP._etaK = GP._eta_Kgrad = 0.5
    hp2, keep2 = _hp(GP, fc.FAIL_THETA)
    rc2, out2 = _lkd(GP, hp2)
    assert rc2 == 0 and out2.info == 0 and np.isfinite(out2.ln_lkd)
    # K + I/2 with K = I up to 1e-6 and one coupled pair: ln det is N ln 1.5 to first order
    assert abs(out2.ln_det - fc.FAIL_N * np.log(1.5)) < 1.0
    assert GP.factor_fallbacks() == 0


ROUTING_N = 2048      # gradient-free: 2048 padded columns, where GPG_FACTOR_AUTO sends 20 matrices per launch to 128-tiles and 19 to 64-tiles
# steps of (factor mode, restart rows of calc_lkd_batch, last_factor() afterwards).  The tuples are what the build before the
# schedule became one field (commit 5783a75) returned for the same calls on the device; they are not derived from this build.
ROUTING = {
    "auto_19_rows":      (("auto", 19, ("tile64", 19)),),
    "auto_20_rows":      (("auto", 20, ("pair128", 20)),),
    "tile64_20_rows":    (("tile64", 20, ("tile64", 20)),),
    "tile128_19_rows":   (("tile128", 19, ("pair128", 19)),),
    "blocked_then_auto": (("blocked", 2, ("blocked", 1)), ("auto", 1, ("tile64", 1)), ("auto", 20, ("pair128", 20))),
}


@functools.lru_cache(maxsize=None)
def _gp_routing():
    import gpgradpy_amd
    from oracle import gp_oracle as orc
    X, f, _ = orc.synthetic_design(ROUTING_N, 2, seed=31)
    GP = gpgradpy_amd.GaussianProcess(2, False, "SqExp", "base")
    GP.set_data(X, f, np.zeros(ROUTING_N))
    assert GP.n_data == ROUTING_N
    GP._etaK = GP._eta_Kgrad = fc.BASE_ETA
    return GP


@pytest.mark.parametrize("steps", list(ROUTING))
def test_factor_mode_routing(steps):
    """Which kernel a factor mode sends one matrix and a batch of restart rows to, at the size where the batch rule of
    GPG_FACTOR_AUTO switches tile size (B Npad / 128 >= 320 at Npad = 2048: 20 rows), with both forced modes on the other
    side of that rule, and the blocked mode (one matrix per launch) handing back to the dataflow route."""
    GP = _gp_routing()
    GP.set_fuse_max_tiles(48)
    GP.set_task_order(-1)
    assert GP._lib.gpg_set_pair_mode(GP._ctx, 2) == 0
    GP.set_max_workgroups(0)
    GP.set_batch(-1)
    try:
        for mode, rows, expect in ROUTING[steps]:
            GP.set_factor_mode(mode)
            ln = GP.calc_lkd_batch(np.random.default_rng(32).uniform(1.0, 1.7, (rows, 2)))   # theta in [10, 50]
            assert np.all(np.isfinite(ln))
            assert GP.last_factor() == expect, (mode, rows, GP.last_factor())
            assert GP.factor_fallbacks() == 0
    finally:
        GP.set_factor_mode("auto")


def test_setters_check_their_arguments():
    GP = _gp("sqexp_n65")
    lib, ctx = GP._lib, GP._ctx
    for bad in (-2, 2, 7):
        assert lib.gpg_set_task_order(ctx, bad) == -1
        assert b"task order" in lib.gpg_last_error(ctx)
    for ok in (0, 1, -1):
        assert lib.gpg_set_task_order(ctx, ok) == 0
    assert lib.gpg_set_fuse_max_tiles(ctx, -1) == -1
    assert b"fuse_max_tiles" in lib.gpg_last_error(ctx)
    for ok in (0, 1, 1 << 20, 48):
        assert lib.gpg_set_fuse_max_tiles(ctx, ok) == 0
