"""Step time of adagrad_optimize for one multilevel regression model evaluated two
ways: through targets.callback (the numpy restatement, on the host once per step) and
through targets.multilevel_regression (on the device).  Prints one JSON line per case.

  case i   p = 3, G = 8,     M = 200,     N = 100, mean-field t, centred, bernoulli_logit
  case ii  p = 8, G = 2 000, M = 200 000, N = 128, mean-field Gaussian, non-centred, gaussian

Each timing is a whole adagrad_optimize call of --steps iterations divided by the
step count; the device is synchronised before both clocks; --warmup untimed calls,
then the median of --reps.  --device-only skips the callback path (for a kernel
trace of the device path alone).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import mlm_cases as mc  # noqa: E402

CASES = {
    'i': dict(p=3, G=8, M=200, N=100, family='mf_t', df=40.0, centered=True,
              likelihood='bernoulli_logit', steps=200),
    'ii': dict(p=8, G=2000, M=200000, N=128, family='mf_gauss', df=None, centered=False,
               likelihood='gaussian', steps=10),
}


def _time(fn, sync, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return out


def run_case(name, steps, warmup, reps, device_only):
    from viabel_amd import vb, targets, _native as nat
    c = CASES[name]
    p, G, M, N = c['p'], c['G'], c['M'], c['N']
    D = p + 1 + G
    steps = steps or c['steps']
    x, y, group = mc.make_data(p, G, M, c['likelihood'], 1)
    kw = mc.model_kwargs(c['likelihood'], c['centered'])

    def family():
        if c['family'] == 'mf_t':
            return vb.mean_field_t_variational_family(D, c['df'], rng='numpy')
        return vb.mean_field_gaussian_variational_family(D, rng='numpy')

    init = np.zeros(2 * D)
    sync = nat.context().synchronize
    paths = {'device': targets.multilevel_regression(x, y, group, n_groups=G, **kw)}
    if not device_only:
        paths['callback'] = targets.callback(mc.restatement(x, y, group, n_groups=G, **kw), D)
    res = dict(case=name, p=p, G=G, M=M, D=D, N=N, family=c['family'], centered=c['centered'],
               likelihood=c['likelihood'], steps=steps, warmup=warmup, reps=reps)
    for label, tgt in paths.items():
        obj = vb.black_box_klvi(family(), tgt, N)
        ts = _time(lambda: vb.adagrad_optimize(steps, obj, init), sync, warmup, reps)
        res[label + '_us_per_step'] = 1e6 * statistics.median(ts) / steps
        res[label + '_us_per_step_all'] = [round(1e6 * t / steps, 2) for t in ts]
    if not device_only:
        res['callback_over_device'] = res['callback_us_per_step'] / res['device_us_per_step']
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['all', 'i', 'ii'])
    ap.add_argument('--steps', type=int, default=0, help='iterations per call (0: the case default)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--device-only', action='store_true')
    a = ap.parse_args()
    for name in (['i', 'ii'] if a.case == 'all' else [a.case]):
        run_case(name, a.steps, a.warmup, a.reps, a.device_only)


if __name__ == '__main__':
    main()
