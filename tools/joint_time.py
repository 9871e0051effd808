#!/usr/bin/env python
"""Time of the joint posterior (GaussianProcess.eval_model_joint, gpg_predict_joint) next to the marginal posterior with
gradients (eval_model(calc_grad=True), gpg_predict_grad) at the same query points, on one device model.

    python tools/joint_time.py [--n 2000] [--d 8] [--nx 8 64] [--reps 20] [--splits 0 1]

Host clock around calls that end in a stream synchronise (both do), after warm-up calls of every shape; prints one JSON
line per (nx, variant) with the median and the minimum over the repetitions.  Variants: the marginal call, the joint call with
each --splits value (gpg_set_gram_splits: 0 = the automatic number of K-chunks, 1 = one chunk: what the split of the Gram kernel
buys), and the joint mean alone.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--nx", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--splits", type=int, nargs="+", default=[0, 1])
    a = ap.parse_args()
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    from oracle import gp_oracle as orc
    X, f, g = orc.synthetic_design(a.n, a.d, seed=3)
    GP = gpgradpy_amd.GaussianProcess(a.d, True, 'SqExp', 'precon')
    GP.set_data(X, f, np.zeros(a.n), g, np.zeros((a.n, a.d)))
    hp = GP.optz_closed_form_hp(GP.make_hp_class(theta=np.full(a.d, 0.05)))
    GP.set_hpara('set', 0, hp_vals=hp)
    rng = np.random.default_rng(4)
    for nx in a.nx:
        xq = np.ascontiguousarray(rng.uniform(X.min(axis=0), X.max(axis=0), (nx, a.d)))
        m = nx * (a.d + 1)
        mean = np.empty(m)
        variants = [("predict_grad", lambda: GP.eval_model(xq, calc_grad=True))]
        for label, splits in [("joint_auto" if k == 0 else f"joint_{k}chunk", k) for k in a.splits]:
            def call(splits=splits):
                GP.set_gram_splits(splits)
                return GP.eval_model_joint(xq, calc_grad=True)
            variants.append((label, call))
        variants.append(("joint_mean_only", lambda: GP._lib.gpg_predict_joint(GP._ctx, nx, _lib.as_dp(xq), float(hp.varK), 1,
                                                                              _lib.as_dp(mean), C.POINTER(C.c_double)())))
        for label, call in variants:
            med, best = timed(call, a.reps)
            print(json.dumps(dict(n=a.n, d=a.d, N=GP.n_data, nx=nx, m=m, variant=label, median_ms=round(med, 3), min_ms=round(best, 3))))
        GP.set_gram_splits(0)
    assert GP.factor_fallbacks() == 0 and GP.solve_fallbacks() == 0


if __name__ == "__main__":
    main()
