#!/usr/bin/env python
"""Time of the per-point gradient covariance and the batched Hessians (GaussianProcess.eval_model_second, gpg_predict_second)
next to the two paths that gave these numbers before, on one device model.

    python tools/second_time.py [--n 2000] [--d 8] [--reps 20] [--hess-nx 64]

(a) gcov alone at the largest nx gpg_predict_joint accepts, (4096 // 64 * 64) // (d + 1) points, against gpg_predict_joint (cov alone)
    at the same points; the event times of the forward sweep and of the Gram kernel of gpg_predict_second (gpg_prof_enable: 'trsm'
    and 'reduce'), the bytes of Z the Gram kernel reads over its time, and what is left of the call (cross rows, finishing kernel,
    copies, launches) from a second run without the events.
(b) the Hessians of --hess-nx points in one gpg_predict_second call against as many gpg_predict_hess calls.

Host clock around calls that end in a stream synchronise (all do), after two warm-up calls of every shape; one JSON line per
variant with the median and the minimum over the repetitions.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(f, reps):
    f()
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hess-nx", type=int, default=64)
    a = ap.parse_args()
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    from oracle import gp_oracle as orc
    d, bs = a.d, a.d + 1
    X, f, g = orc.synthetic_design(a.n, d, seed=3)
    GP = gpgradpy_amd.GaussianProcess(d, True, 'SqExp', 'precon')
    GP.set_data(X, f, np.zeros(a.n), g, np.zeros((a.n, d)))
    hp = GP.optz_closed_form_hp(GP.make_hp_class(theta=np.full(d, 0.05)))
    GP.set_hpara('set', 0, hp_vals=hp)
    varK = float(hp.varK)
    lib, ctx = GP._lib, GP._ctx
    rng = np.random.default_rng(4)
    base = dict(n=a.n, d=d, N=GP.n_data)

    def say(**kw):
        print(json.dumps({**base, **kw}), flush=True)

    # ---- (a) the blocks against the full joint matrix ---------------------------------------------------------------------------
    nx = 4096 // bs
    xq = np.ascontiguousarray(rng.uniform(X.min(axis=0), X.max(axis=0), (nx, d)))
    gcov, cov = np.empty((nx, bs, bs)), np.empty((nx * bs, nx * bs))

    def second_gcov():
        assert lib.gpg_predict_second(ctx, nx, _lib.as_dp(xq), varK, None, None, _lib.as_dp(gcov), None, None) == 0, GP._err()

    def joint_cov():
        assert lib.gpg_predict_joint(ctx, nx, _lib.as_dp(xq), varK, 1, None, _lib.as_dp(cov)) == 0, GP._err()

    med_s, min_s = timed(second_gcov, a.reps)
    say(variant="second_gcov", nx=nx, median_ms=round(med_s, 3), min_ms=round(min_s, 3))
    med_j, min_j = timed(joint_cov, a.reps)
    say(variant="joint_cov", nx=nx, median_ms=round(med_j, 3), min_ms=round(min_j, 3))
    GP.prof_enable(("trsm", "reduce"))
    GP.prof_read()
    for _ in range(a.reps):
        second_gcov()
    pr = GP.prof_read()
    GP.prof_enable(())
    sweep, gram = pr["trsm"]["ms"] / pr["trsm"]["count"], pr["reduce"]["ms"] / pr["reduce"]["count"]
    nbytes = pr["reduce"]["work"] / pr["reduce"]["count"]
    say(variant="second_gcov_split", nx=nx, chunks=int(pr["trsm"]["count"] // a.reps), sweep_ms=round(sweep, 4), gram_ms=round(gram, 4),
        gram_GB=round(nbytes / 1e9, 4), gram_TBps=round(nbytes / (gram * 1e-3) / 1e12, 3),
        rest_of_call_ms=round(med_s - (sweep + gram) * (pr["trsm"]["count"] / a.reps), 3))

    # ---- (b) batched Hessians against one call per point ----------------------------------------------------------------------------
    nh = a.hess_nx
    xh = np.ascontiguousarray(xq[:nh])
    mu, dmu, blk = np.empty(nh), np.empty((nh, d)), np.empty((nh, bs, bs))
    h_mu, h_sig = np.empty((nh, d, d)), np.empty((nh, d, d))

    def second_hess():
        assert lib.gpg_predict_second(ctx, nh, _lib.as_dp(xh), varK, _lib.as_dp(mu), _lib.as_dp(dmu), _lib.as_dp(blk), _lib.as_dp(h_mu),
                                      _lib.as_dp(h_sig)) == 0, GP._err()

    o = [np.empty(1), np.empty(1), np.empty(d), np.empty(d), np.empty((d, d)), np.empty((d, d))]

    def single_hess():
        for j in range(nh):
            assert lib.gpg_predict_hess(ctx, _lib.as_dp(xh[j]), varK, *[_lib.as_dp(v) for v in o]) == 0, GP._err()

    med, best = timed(second_hess, a.reps)
    say(variant="second_hess_one_call", nx=nh, median_ms=round(med, 3), min_ms=round(best, 3))
    med1, best1 = timed(single_hess, max(3, a.reps // 4))
    say(variant="predict_hess_per_point", nx=nh, calls=nh, median_ms=round(med1, 3), min_ms=round(best1, 3), ratio=round(med1 / med, 1))
    assert GP.factor_fallbacks() == 0 and GP.solve_fallbacks() == 0


if __name__ == "__main__":
    main()
