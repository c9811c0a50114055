"""Step time of adagrad_optimize for the multilevel regression target with a learned scale or
dispersion at DESIGN §7d's shape ii (p = 8, G = 2 000, M = 200 000, N = 128, mean-field
Gaussian, non-centred): the learned gaussian, student_t and neg_binomial_2_log targets (dim
p + 2 + G) beside the fixed-parameter target of the same likelihood on the same data (dim
p + 1 + G) and the host callback of the learned model (tests/mlm_aux_cases.py), all in one
session.  Prints one JSON line per likelihood.  Modelled on scripts/aux_bench.py: a timing
is a whole adagrad_optimize call of --steps iterations divided by the step count, the device
synchronised before both clocks; --warmup untimed calls, then the median of --reps.
--fixed-only times the fixed targets alone, which a build without the learned mode can run:
the baseline for "the fixed path did not get slower".  A measurement, not a gate.
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
from tests import mlm_aux_cases as mac  # noqa: E402

P, G, M, N = 8, 2000, 200000, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--callback-steps', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fixed-only', action='store_true')
    ap.add_argument('--label', default='')
    a = ap.parse_args()
    from viabel_amd import vb, targets, _native as nat
    sync = nat.context().synchronize

    def step_us(tgt, dim, steps, warmup, reps):
        init = np.zeros(2 * dim)
        obj = vb.black_box_klvi(vb.mean_field_gaussian_variational_family(dim, rng='numpy'), tgt, N)
        ts = _time(lambda: vb.adagrad_optimize(steps, obj, init), sync, warmup, reps)
        return 1e6 * statistics.median(ts) / steps, [round(1e6 * t / steps, 2) for t in ts]

    for lik in mac.LIKELIHOODS:
        x, y, g, off = mac.make_data(P, G, M, lik, seed=1)
        if lik == 'neg_binomial_2_log':
            y = np.minimum(y, 50.0)              # J = 50: the table of a typical count model
        kw = mac.model_kwargs(lik, False)
        fkw = {k: v for k, v in kw.items() if k != 'hyper_scale'}
        if lik == 'neg_binomial_2_log':
            fixed = targets.multilevel_regression(x, y, g, n_groups=G, offset=off, phi=3.0, **fkw)
        else:
            fixed = targets.multilevel_regression(x, y, g, n_groups=G, scale=0.7, **fkw)
        fix_us, fix_all = step_us(fixed, P + 1 + G, a.steps, a.warmup, a.reps)
        out = dict(likelihood=lik, label=a.label, p=P, G=G, M=M, N=N, centered=False,
                   J=int(y.max()) if lik == 'neg_binomial_2_log' else None, family='mf_gauss',
                   steps=a.steps, warmup=a.warmup, reps=a.reps,
                   fixed_us_per_step=fix_us, fixed_us_per_step_all=fix_all)
        if not a.fixed_only:
            D = P + 2 + G
            learned = targets.multilevel_regression(x, y, g, n_groups=G, offset=off,
                                                    **mac.target_kwargs(kw))
            dev_us, dev_all = step_us(learned, D, a.steps, a.warmup, a.reps)
            cb = targets.callback(mac.restatement(x, y, g, offset=off, n_groups=G, **kw), D)
            cb_us, cb_all = step_us(cb, D, a.callback_steps, 1, 3)
            out.update(learned_us_per_step=dev_us, learned_us_per_step_all=dev_all,
                       callback_us_per_step=cb_us, callback_us_per_step_all=cb_all,
                       callback_steps=a.callback_steps, callback_reps=3,
                       learned_over_fixed=dev_us / fix_us, callback_over_learned=cb_us / dev_us)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
