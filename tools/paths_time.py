#!/usr/bin/env python
"""Time of the posterior sample paths (GaussianProcess.sample_paths: gpg_paths_setup, gpg_paths_eval) on one device model, next to
the posterior calls that give moments at the same points.

    python tools/paths_time.py [--n 2000] [--d 8] [--paths 64] [--features 4096] [--reps 20]

(a) gpg_paths_setup, and from gpg_prof events its feature kernel ('reduce') and its two sweeps ('trsm');
(b) gpg_paths_eval with gradients at nx = 64 and nx = 448, and from the events the cross rows ('assembly'), the product kernel
    ('gemm_trail': 2 nx (d + 1) N S flops; it reads the nx (d + 1) x N_pad doubles of Wt once per 64 paths) and the feature kernel
    ('reduce');
(c) for scale, gpg_predict_grad and gpg_predict_joint (mean and covariance) at the same points.

Host clock around calls that end in a stream synchronise (all do), after two warm-up calls of every shape; one JSON line per
variant with the median and the minimum over the repetitions.  The event times come from a second run with the events on.
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
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--features", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    from gpgradpy_amd.paths import prepare_draws
    from oracle import gp_oracle as orc
    d, bs, S, M = a.d, a.d + 1, a.paths, a.features
    X, f, g = orc.synthetic_design(a.n, d, seed=3)
    GP = gpgradpy_amd.GaussianProcess(d, True, 'SqExp', 'precon')
    GP.set_data(X, f, np.zeros(a.n), g, np.zeros((a.n, d)))
    hp = GP.optz_closed_form_hp(GP.make_hp_class(theta=np.full(d, 0.05)))
    GP.set_hpara('set', 0, hp_vals=hp)
    varK = float(hp.varK)
    lib, ctx = GP._lib, GP._ctx
    N, Npad = GP.n_data, ((GP.n_data + 127) // 128) * 128
    rng = np.random.default_rng(4)
    base = dict(n=a.n, d=d, N=N, S=S, M=M)

    def say(**kw):
        print(json.dumps({**base, **kw}), flush=True)

    def events(fn, cats):
        GP.prof_enable(cats)
        GP.prof_read()
        for _ in range(a.reps):
            fn()
        pr = GP.prof_read()
        GP.prof_enable(())
        return {c: pr[c]["ms"] / a.reps for c in cats}, {c: pr[c]["count"] / a.reps for c in cats}

    # ---- (a) set-up -------------------------------------------------------------------------------------------------------------------
    om, ph, w, z = prepare_draws('SqExp', np.ravel(hp.theta), None, N, S, n_features=M, seed=5)

    def setup():
        assert lib.gpg_paths_setup(ctx, S, M, _lib.as_dp(om), _lib.as_dp(ph), _lib.as_dp(w), _lib.as_dp(z), varK) == 0, GP._err()

    med, best = timed(setup, a.reps)
    ev, cnt = events(setup, ("reduce", "trsm"))
    say(variant="paths_setup", median_ms=round(med, 3), min_ms=round(best, 3), feature_kernel_ms=round(ev["reduce"], 4),
        two_sweeps_ms=round(ev["trsm"], 4), sweeps_per_call=cnt["trsm"])

    # ---- (b) evaluation, (c) the moment calls at the same points -----------------------------------------------------------------
    for nx in (64, 448):
        xq = np.ascontiguousarray(rng.uniform(X.min(axis=0), X.max(axis=0), (nx, d)))
        fo, go = np.empty((S, nx)), np.empty((S, nx, d))

        def ev_grad():
            assert lib.gpg_paths_eval(ctx, nx, _lib.as_dp(xq), _lib.as_dp(fo), _lib.as_dp(go)) == 0, GP._err()

        def ev_val():
            assert lib.gpg_paths_eval(ctx, nx, _lib.as_dp(xq), _lib.as_dp(fo), None) == 0, GP._err()

        med, best = timed(ev_grad, a.reps)
        ev, cnt = events(ev_grad, ("assembly", "gemm_trail", "reduce"))
        flops = 2.0 * nx * bs * N * S
        wt_bytes = 8.0 * (((nx * bs + 63) // 64) * 64) * Npad * ((S + 63) // 64)
        say(variant="paths_eval_grad", nx=nx, median_ms=round(med, 3), min_ms=round(best, 3), cross_rows_ms=round(ev["assembly"], 4),
            product_kernel_ms=round(ev["gemm_trail"], 4), feature_kernel_ms=round(ev["reduce"], 4),
            product_TFLOPs=round(flops / (ev["gemm_trail"] * 1e-3) / 1e12, 3),
            product_Wt_TBps=round(wt_bytes / (ev["gemm_trail"] * 1e-3) / 1e12, 3), chunks=cnt["gemm_trail"])
        med, best = timed(ev_val, a.reps)
        say(variant="paths_eval_values", nx=nx, median_ms=round(med, 3), min_ms=round(best, 3))
        mu, sig, s2, dmu, dsig = np.empty(nx), np.empty(nx), np.empty(nx), np.empty((nx, d)), np.empty((nx, d))

        def predict_grad():
            assert lib.gpg_predict_grad(ctx, nx, _lib.as_dp(xq), varK, _lib.as_dp(mu), _lib.as_dp(sig), _lib.as_dp(s2), _lib.as_dp(dmu),
                                        _lib.as_dp(dsig)) == 0, GP._err()

        med, best = timed(predict_grad, a.reps)
        say(variant="predict_grad", nx=nx, median_ms=round(med, 3), min_ms=round(best, 3))
        mean, cov = np.empty(nx * bs), np.empty((nx * bs, nx * bs))

        def predict_joint():
            assert lib.gpg_predict_joint(ctx, nx, _lib.as_dp(xq), varK, 1, _lib.as_dp(mean), _lib.as_dp(cov)) == 0, GP._err()

        med, best = timed(predict_joint, max(5, a.reps // 2))
        say(variant="predict_joint", nx=nx, median_ms=round(med, 3), min_ms=round(best, 3))
    assert GP.factor_fallbacks() == 0 and GP.solve_fallbacks() == 0


if __name__ == "__main__":
    main()
