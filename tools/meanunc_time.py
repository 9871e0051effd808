#!/usr/bin/env python
"""What gpg_set_mean_uncertainty costs (sibling of tools/joint_time.py): gpg_predict_grad and gpg_predict_joint with the switch off
and on, the one-time build of the per-model state, and the event time of the hot kernel (mu_u_partial_kernel).

    python tools/meanunc_time.py [--n 2000] [--d 8] [--order 0 1] [--reps 20] [--other-lib libgpgrad_other.so]

Host clock around whole C-ABI calls (each ends in a stream synchronise), median and minimum of --reps after two warm-up calls, on
one device model per mean order: gpg_predict_grad at nx = 1 and 64, gpg_predict_joint with gradients at nx = 8 and 64.
--other-lib: another build of the library inside gpgradpy_amd/ (for instance one made from the commit before this switch existed),
driven through the same C ABI on a context of its own with the same data and hyperparameters; its calls alternate with the
switch-off calls of this build, repetition by repetition, so both see the same box in the same state.
State build: the first switched-on call after a gpg_setup_eval_mean minus the median of the later ones.
Kernel time: category 'reduce' of gpg_prof_enable holds nothing but mu_u_partial_kernel during a predict call; printed with the
bytes of Z it reads (8 m Npad) and the bandwidth that amounts to.  One JSON line per figure.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def alternate(calls, reps):
    """median / minimum in ms of each call, the calls taking turns within every repetition"""
    for f in calls:
        f()
        f()
    ts = [[] for _ in calls]
    for _ in range(reps):
        for i, f in enumerate(calls):
            t0 = time.perf_counter()
            f()
            ts[i].append(time.perf_counter() - t0)
    return [(float(np.median(t)) * 1e3, float(np.min(t)) * 1e3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--order", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None)
    a = ap.parse_args()
    import gpgradpy_amd
    from gpgradpy_amd import _lib
    from oracle import gp_oracle as orc
    dp = C.POINTER(C.c_double)
    other = None
    if a.other_lib:
        other = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), os.path.basename(a.other_lib)))
        other.gpg_predict_grad.argtypes = [C.c_void_p, C.c_int, dp, C.c_double, dp, dp, dp, dp, dp]
        other.gpg_predict_joint.argtypes = [C.c_void_p, C.c_int, dp, C.c_double, C.c_int, dp, dp]
        other.gpg_setup_eval_mean.argtypes = [C.c_void_p, C.POINTER(_lib.GpgHp), dp, dp]
        other.gpg_set_data.argtypes = [C.c_void_p, dp, dp, dp]
        other.gpg_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        other.gpg_set_mean_order.argtypes = [C.c_void_p, C.c_int]
        other.gpg_destroy.argtypes = [C.c_void_p]
        other.gpg_destroy.restype = None
    X, f, g = orc.synthetic_design(a.n, a.d, seed=3)
    rng = np.random.default_rng(4)
    for order in a.order:
        GP = gpgradpy_amd.GaussianProcess(a.d, True, 'SqExp', 'precon', mean_fun_type='poly_ord_1' if order else 'poly_ord_0')
        GP.set_data(X, f, np.zeros(a.n), g, np.zeros((a.n, a.d)))
        hp_vals = GP.optz_closed_form_hp(GP.make_hp_class(theta=np.full(a.d, 0.05)))
        GP.set_hpara('set', 0, hp_vals=hp_vals)
        lib, ctx, varK = GP._lib, GP._ctx, float(hp_vals.varK)
        hp, keep = GP._make_hp(hp_vals, 1.0, closed_form=True)
        beta = np.ascontiguousarray(np.ravel(hp_vals.beta), dtype=np.float64)
        octx = None
        if other is not None:
            octx = C.c_void_p()
            assert other.gpg_create(C.byref(octx), 0, a.n, a.d, 1, 0) == 0
            assert other.gpg_set_mean_order(octx, order) == 0
            y = np.ascontiguousarray(GP._data_vec)
            assert other.gpg_set_data(octx, _lib.as_dp(np.ascontiguousarray(X)), _lib.as_dp(y), None) == 0
            assert other.gpg_setup_eval_mean(octx, C.byref(hp), _lib.as_dp(beta), None) == 0
        Npad = ((GP.n_data + 127) // 128) * 128
        base = dict(n=a.n, d=a.d, N=GP.n_data, mean_order=order, n_beta=beta.size)

        def switch(on):
            assert lib.gpg_set_mean_uncertainty(ctx, on) == 0

        # one-time state build: first switched-on call after a set-up against the later ones
        xq1 = np.ascontiguousarray(rng.uniform(X.min(axis=0), X.max(axis=0), (1, a.d)))
        o1 = [np.empty(1), np.empty(1), np.empty(1), np.empty((1, a.d)), np.empty((1, a.d))]

        def grad1():
            assert lib.gpg_predict_grad(ctx, 1, _lib.as_dp(xq1), varK, *[_lib.as_dp(o) for o in o1]) == 0
        switch(1)
        grad1()
        builds = []
        for _ in range(5):
            assert lib.gpg_setup_eval_mean(ctx, C.byref(hp), _lib.as_dp(beta), None) == 0
            t0 = time.perf_counter()
            grad1()
            t1 = time.perf_counter()
            grad1()
            t2 = time.perf_counter()
            builds.append((t1 - t0) - (t2 - t1))
        print(json.dumps(dict(base, figure="state_build", median_ms=round(float(np.median(builds)) * 1e3, 3),
                              min_ms=round(float(np.min(builds)) * 1e3, 3))))

        for kind, nxs in (("predict_grad", (1, 64)), ("predict_joint", (8, 64))):
            for nx in nxs:
                xq = np.ascontiguousarray(rng.uniform(X.min(axis=0), X.max(axis=0), (nx, a.d)))
                m = nx * (a.d + 1) if kind == "predict_joint" else nx
                if kind == "predict_grad":
                    outs = [np.empty(nx), np.empty(nx), np.empty(nx), np.empty((nx, a.d)), np.empty((nx, a.d))]

                    def call(L, cx):
                        assert L.gpg_predict_grad(cx, nx, _lib.as_dp(xq), varK, *[_lib.as_dp(o) for o in outs]) == 0
                else:
                    mean, cov = np.empty(m), np.empty((m, m))

                    def call(L, cx):
                        assert L.gpg_predict_joint(cx, nx, _lib.as_dp(xq), varK, 1, _lib.as_dp(mean), _lib.as_dp(cov)) == 0

                def off():
                    switch(0)
                    call(lib, ctx)

                def on():
                    switch(1)
                    call(lib, ctx)
                calls, labels = [off, on], ["off", "on"]
                if other is not None:
                    calls.insert(0, lambda: call(other, octx))
                    labels.insert(0, "other_lib")
                for label, (med, best) in zip(labels, alternate(calls, a.reps)):
                    print(json.dumps(dict(base, figure=kind, nx=nx, m=m, variant=label, median_ms=round(med, 3), min_ms=round(best, 3))))
                # event time of the hot kernel
                GP.prof_enable(("reduce",))
                switch(1)
                for _ in range(a.reps):
                    call(lib, ctx)
                prof = GP.prof_read()
                GP.prof_enable(())
                ms, count = prof["reduce"]["ms"], prof["reduce"]["count"]
                if count:
                    us = ms / count * 1e3
                    nbytes = 8.0 * m * Npad
                    print(json.dumps(dict(base, figure="mu_u_partial_kernel", call=kind, nx=nx, m=m, launches=int(count),
                                          mean_us=round(us, 2), z_bytes=int(nbytes), gb_per_s=round(nbytes / us * 1e-3, 1))))
                switch(0)
        assert GP.factor_fallbacks() == 0 and GP.solve_fallbacks() == 0
        if octx is not None:
            other.gpg_destroy(octx)
        GP.close()


if __name__ == "__main__":
    main()
