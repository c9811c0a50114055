"""Step time of adagrad_optimize for the regression target with a learned scale or
dispersion at p = 32, M = 100 000, N = 128 with the mean-field Gaussian family: the learned
gaussian, student_t and neg_binomial_2_log targets (dim 33) beside the fixed-parameter
target of the same likelihood on the same data (dim 32: the kernels as they were before
the learned mode) and the host callback of the learned model (tests/aux_cases.py), all in
one session.  Prints one JSON line per likelihood.  Modelled on scripts/count_bench.py: a
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
from tests import aux_cases as ac  # noqa: E402

P, M, N = 32, 100000, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--callback-steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from viabel_amd import vb, targets, _native as nat
    sync = nat.context().synchronize

    def step_us(tgt, dim, steps, warmup, reps):
        init = np.zeros(2 * dim)
        obj = vb.black_box_klvi(vb.mean_field_gaussian_variational_family(dim, rng='numpy'), tgt, N)
        ts = _time(lambda: vb.adagrad_optimize(steps, obj, init), sync, warmup, reps)
        return 1e6 * statistics.median(ts) / steps, [round(1e6 * t / steps, 2) for t in ts]

    for lik in ac.LIKELIHOODS:
        x, y, off = ac.make_data(P, M, lik, seed=1)
        if lik == 'neg_binomial_2_log':
            y = np.minimum(y, 50.0)              # J = 50: the table of a typical count model
        kw = ac.model_kwargs(lik)
        learned = targets.regression(x, y, offset=off, **ac.target_kwargs(kw))
        fkw = {k: v for k, v in kw.items() if k != 'hyper_scale'}
        if lik == 'neg_binomial_2_log':
            fixed = targets.regression(x, y, offset=off, phi=3.0, **fkw)
        else:
            fixed = targets.regression(x, y, scale=0.7, **fkw)
        fix_us, fix_all = step_us(fixed, P, a.steps, a.warmup, a.reps)
        dev_us, dev_all = step_us(learned, P + 1, a.steps, a.warmup, a.reps)
        cb = targets.callback(ac.restatement(x, y, offset=off, **kw), P + 1)
        cb_us, cb_all = step_us(cb, P + 1, a.callback_steps, 1, 3)
        print(json.dumps(dict(
            likelihood=lik, p=P, M=M, N=N, J=int(y.max()) if lik == 'neg_binomial_2_log' else None,
            family='mf_gauss', steps=a.steps, warmup=a.warmup, reps=a.reps,
            learned_us_per_step=dev_us, learned_us_per_step_all=dev_all,
            fixed_us_per_step=fix_us, fixed_us_per_step_all=fix_all,
            callback_us_per_step=cb_us, callback_us_per_step_all=cb_all,
            callback_steps=a.callback_steps, callback_reps=3,
            learned_over_fixed=dev_us / fix_us, callback_over_learned=cb_us / dev_us)),
            flush=True)


if __name__ == '__main__':
    main()
