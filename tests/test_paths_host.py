"""Posterior sample paths, the parts that need no device (gpgradpy_amd/paths.py; the device side is tests/test_gpu_paths.py).

* The three frequency laws of draw_frequencies at fixed seeds, M = 16384, d = 3, six points in [-1, 1]^3, theta = (0.7, 2.0, 0.3),
  alpha = 1.7: the value-value entries of Phi Phi' are within 6 / sqrt(M) = 0.047 of the oracle's kern_base (each entry is a mean of
  M terms 2 cos(.) cos(.) of variance <= 1, so six standard deviations; a wrong scale or mixture is off by 0.1 or more), and the column
  means of omega^2 are within 5 % of 2 theta (SqExp, RatQu) and 5 theta / 3 (Ma5f2).  Every figure is printed (pytest -s) before it is
  asserted.  Measured: SqExp 0.014, RatQu 0.009, Ma5f2 0.022.
* The reference of the device tests is self-consistent: at the training rows path_reference reproduces the identity
  f_s(X) = mu_rows + sqrt(varK) (D v_s - D^(1/2) z_s) in which the features cancel (tests/test_gpu_paths.py, test 6).
* Shape and argument errors of draw_frequencies, prepare_draws and the PosteriorPaths wrapper.
* The three symbols are declared, listed and exported.

All of these fail without the feature: gpgradpy_amd.paths does not exist on the parent commit.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import paths_cases as pc
from conftest import ROOT
from oracle import gp_oracle as orc

M_LAW, THETA, ALPHA = 16384, np.array([0.7, 2.0, 0.3]), 1.7
LAWS = {"SqExp": ("SqExp", None, 2.0 * THETA), "RatQu": (("RatQu", ALPHA), ALPHA, 2.0 * THETA), "Ma5f2": ("Ma5f2", None, 5.0 * THETA / 3.0)}


@pytest.mark.parametrize("kernel", sorted(LAWS))
def test_frequency_law(kernel):
    from gpgradpy_amd.paths import draw_frequencies
    kernel_o, hp_kernel, second_moment = LAWS[kernel]
    X = np.random.default_rng(11).uniform(-1.0, 1.0, (6, 3))
    omega, phase = draw_frequencies(kernel, THETA, hp_kernel, M_LAW, np.random.default_rng(2024))
    assert omega.shape == (M_LAW, 3) and phase.shape == (M_LAW,)
    assert phase.min() >= 0.0 and phase.max() < 2.0 * np.pi
    Phi = pc.features(X, omega, phase, False)
    err = float(np.max(np.abs(Phi @ Phi.T - orc.kern_base(X, X, THETA, kernel_o))))
    ratio = np.mean(omega ** 2, axis=0) / second_moment
    print(f"{kernel}: max |Phi Phi' - K| = {err:.4f} (bound {6 / np.sqrt(M_LAW):.4f})   E omega^2 / expected = {ratio}")
    assert err <= 6.0 / np.sqrt(M_LAW)
    assert np.all(np.abs(ratio - 1.0) <= 0.05)


def test_frequencies_are_a_function_of_the_seed():
    from gpgradpy_amd.paths import draw_frequencies
    a = draw_frequencies("Ma5f2", THETA, None, 50, 7)
    b = draw_frequencies("Ma5f2", THETA, None, 50, np.random.default_rng(7))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ("ma5f2_n33_d3", "ma5f2_n23_d3_mask", "sqexp_n17_d4_lin"))
def test_reference_training_row_identity(name):
    """The NumPy restatement against the identity in which the random features cancel: a wrong sign, a missing sqrt(varK) or a
    wrong row order in path_reference or coeff_reference does not survive it.  Bound: 1e-7 of the largest |f| resp. |dfdx|, the
    conditioning budget of two cho_solve calls on a matrix regularised to cond ~ 1e10 (tests/tolerances.py)."""
    pm = pc.model(name)
    c = pm.c
    n, d = c["n"], c["d"]
    omega, phase, w, z = pc.draws(pm, 5, 31)
    coeff = pc.coeff_reference(pm, omega, phase, w, z)
    f, dfdx = pc.path_reference(pm, omega, phase, w, z, c["x"], coeff)
    sv = np.sqrt(pm.varK)
    v = (pm.alpha[None, :] - coeff) / sv
    mu_rows = pm.Kern @ pm.alpha
    mu_rows[:n] += pm.beta[0] + (c["x"] @ pm.beta[1:] if pm.linear else 0.0)
    if pm.linear:
        mu_rows[n:] += np.repeat(pm.beta[1:], (pm.N - n) // d)
    want = mu_rows[None, :] + sv * (pm.D[None, :] * v - np.sqrt(pm.D)[None, :] * z)           # [S, N]
    got = np.concatenate((f, np.transpose(dfdx, (0, 2, 1)).reshape(5, -1)), axis=1)[:, pm.rows]
    e_f = np.max(np.abs(got[:, :n] - want[:, :n])) / np.abs(want[:, :n]).max()
    e_g = np.max(np.abs(got[:, n:] - want[:, n:])) / np.abs(want[:, n:]).max()
    print(f"{name}: training-row identity of the reference  f {e_f:.2e}  dfdx {e_g:.2e}")
    assert e_f <= 1e-7 and e_g <= 1e-7


def test_draw_frequencies_errors():
    from gpgradpy_amd.paths import draw_frequencies
    with pytest.raises(ValueError, match="kernel_type"):
        draw_frequencies("Gauss", THETA, None, 8, 0)
    with pytest.raises(ValueError, match="theta"):
        draw_frequencies("SqExp", np.array([1.0, -1.0]), None, 8, 0)
    with pytest.raises(ValueError, match="theta"):
        draw_frequencies("SqExp", np.ones((2, 2)), None, 8, 0)
    with pytest.raises(ValueError, match="n_features"):
        draw_frequencies("SqExp", THETA, None, 0, 0)
    with pytest.raises(ValueError, match="n_features"):
        draw_frequencies("SqExp", THETA, None, 65537, 0)
    with pytest.raises(ValueError, match="alpha"):
        draw_frequencies("RatQu", THETA, None, 8, 0)
    with pytest.raises(ValueError, match="alpha"):
        draw_frequencies("RatQu", THETA, -2.0, 8, 0)


def test_prepare_draws_shapes_and_errors():
    from gpgradpy_amd.paths import prepare_draws
    om, ph, w, z = prepare_draws("SqExp", THETA, None, 20, 4, n_features=16, seed=3)
    assert om.shape == (16, 3) and ph.shape == (16,) and w.shape == (4, 16) and z.shape == (4, 20)
    again = prepare_draws("SqExp", THETA, None, 20, 4, n_features=16, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip((om, ph, w, z), again))
    assert prepare_draws("SqExp", THETA, None, 20, 4, n_features=16, seed=3, noise_draw=False)[3] is None
    om2, ph2, w2, z2 = prepare_draws("SqExp", THETA, None, 20, 4, omega=om[:5], phase=ph[:5], w=np.zeros((4, 5)), z=np.zeros((4, 20)))
    assert om2.shape == (5, 3) and np.array_equal(om2, om[:5]) and not w2.any() and not z2.any()
    for kw, msg in ((dict(n_paths=0), "n_paths"), (dict(n_paths=1025), "n_paths"), (dict(n_paths=2.5), "n_paths"),
                    (dict(omega=om), "together"), (dict(phase=ph), "together"),
                    (dict(omega=om[:, :2], phase=ph), "omega"), (dict(omega=om, phase=ph[:3]), "phase"),
                    (dict(w=np.zeros((4, 15))), "w must"), (dict(z=np.zeros((3, 20))), "z must"),
                    (dict(z=np.zeros((4, 20)), noise_draw=False), "noise_draw"),
                    (dict(w=np.full((4, 16), np.nan)), "finite")):
        args = dict(n_paths=4, n_features=16, seed=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            prepare_draws("SqExp", THETA, None, 20, **args)


class _Owner:
    _paths_current = None


def test_wrapper_errors_without_a_device():
    from gpgradpy_amd.paths import PosteriorPaths
    gp = _Owner()
    p = PosteriorPaths(gp, 3, 2, 10, None, None, None, None)
    gp._paths_current = p
    for bad in (np.zeros((4, 3)), np.zeros((2, 2, 2)), np.zeros((0, 2)), np.full((1, 2), np.inf)):
        with pytest.raises(ValueError, match="xq"):
            p(bad)
    gp._paths_current = None                                          # the posterior was set up again
    with pytest.raises(Exception, match="no longer belong"):
        p(np.zeros((1, 2)))
    with pytest.raises(Exception, match="no longer belong"):
        p.coeff
    with pytest.raises(Exception, match="no longer belong"):
        p.ddiag


def test_new_symbols_declared_listed_exported():
    from gpgradpy_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpgrad.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpg_[a-z_]+)\s*\(", txt))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("gpg_paths_setup", "gpg_paths_eval", "gpg_paths_coeff"):
        assert s in declared, f"{s} is not declared in include/gpgrad.h"
        assert s in _lib.ABI_SYMBOLS, f"{s} is not listed in _lib.ABI_SYMBOLS"
        assert hasattr(lib, s), f"{s} is not exported by the library"
