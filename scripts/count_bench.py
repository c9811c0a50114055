"""Step time of adagrad_optimize for the two count regressions at D = 32, M = 100 000,
N = 128 with the mean-field Gaussian family: targets.regression with poisson_log and
neg_binomial_2_log on the device, beside the host callback of the same model
(tests/count_cases.py) and the device's bernoulli_logit target at the same shape, all in
one session.  Prints one JSON line per likelihood.  Modelled on scripts/glm_bench.py: a
timing is a whole adagrad_optimize call of --steps iterations divided by the step count,
the device synchronised before both clocks; --warmup untimed calls, then the median of
--reps.  A measurement, not a gate.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from glm_bench import _time  # noqa: E402
from tests import count_cases as cc  # noqa: E402
from tests import glm_cases as gc  # noqa: E402

D, M, N = 32, 100000, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--callback-steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from viabel_amd import vb, targets, _native as nat
    sync = nat.context().synchronize
    init = np.zeros(2 * D)

    def step_us(tgt, steps, warmup, reps):
        obj = vb.black_box_klvi(vb.mean_field_gaussian_variational_family(D, rng='numpy'), tgt, N)
        ts = _time(lambda: vb.adagrad_optimize(steps, obj, init), sync, warmup, reps)
        return 1e6 * statistics.median(ts) / steps, [round(1e6 * t / steps, 2) for t in ts]

    xb, yb = gc.make_data(D, M, 'bernoulli_logit', seed=1)
    logit_us, logit_all = step_us(targets.logistic_regression(xb, yb, prior_scale=3.0), a.steps,
                                  a.warmup, a.reps)
    for lik in cc.LIKELIHOODS:
        x, y, off = cc.make_data(D, M, lik, seed=1)
        kw = cc.model_kwargs(lik)
        dev_us, dev_all = step_us(targets.regression(x, y, offset=off, **kw), a.steps, a.warmup,
                                  a.reps)
        cb = targets.callback(cc.restatement(x, y, offset=off, **kw), D)
        cb_us, cb_all = step_us(cb, a.callback_steps, 1, 3)
        print(json.dumps(dict(
            likelihood=lik, D=D, M=M, N=N, family='mf_gauss', steps=a.steps, warmup=a.warmup,
            reps=a.reps, device_us_per_step=dev_us, device_us_per_step_all=dev_all,
            callback_us_per_step=cb_us, callback_us_per_step_all=cb_all,
            callback_steps=a.callback_steps, callback_reps=3,
            bernoulli_logit_us_per_step=logit_us, bernoulli_logit_us_per_step_all=logit_all,
            device_over_bernoulli_logit=dev_us / logit_us, callback_over_device=cb_us / dev_us)),
            flush=True)


if __name__ == '__main__':
    main()
