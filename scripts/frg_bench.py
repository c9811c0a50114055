"""Step time of adagrad_optimize with the Cholesky full-rank Gaussian family
(vb.cholesky_gaussian_variational_family) beside its former stand-in,
t_variational_family(D, 1e6), on the same build.  Prints one JSON line per case.

  eight_schools   eight_schools_ncp, D = 10, N = 100, KLVI
  corr512_klvi    corr_gauss, D = 512, N = 128, KLVI
  corr512_chivi   corr_gauss, D = 512, N = 128, CHIVI alpha = 2 (config 4's shape)
  regression      student-t regression, D = 32, M = 100 000, N = 100, KLVI

rng='philox' throughout.  Each timing is a whole adagrad_optimize call of --steps
iterations divided by the step count; the device is synchronised before both clocks;
--warmup untimed calls, then the median of --reps.
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

from tests import glm_cases as gc  # noqa: E402

CASES = {
    'eight_schools': dict(target='eight_schools_ncp', D=10, N=100, obj='klvi', steps=500),
    'corr512_klvi': dict(target='corr_gauss', D=512, N=128, obj='klvi', steps=200),
    'corr512_chivi': dict(target='corr_gauss', D=512, N=128, obj='chivi', steps=200),
    'regression': dict(target='regression', D=32, N=100, obj='klvi', steps=50, M=100000),
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


def run_case(name, steps, warmup, reps):
    from viabel_amd import vb, targets, _native as nat
    os.environ['VIABEL_AMD_PROGRESS'] = '0'
    c = CASES[name]
    D, N = c['D'], c['N']
    steps = steps or c['steps']
    if c['target'] == 'regression':
        x, y = gc.make_data(D, c['M'], 'student_t', seed=1)
        tgt = targets.regression(x, y, **gc.model_kwargs('student_t'))
    elif c['target'] == 'corr_gauss':
        tgt = targets.corr_gauss(D)
    else:
        tgt = targets.eight_schools_ncp()
    fams = {'cholesky_gaussian': vb.cholesky_gaussian_variational_family(D, rng='philox'),
            't_df1e6': vb.t_variational_family(D, 1e6, rng='philox')}
    init = np.zeros(fams['t_df1e6'].var_param_dim)
    sync = nat.context().synchronize
    res = dict(case=name, target=c['target'], D=D, N=N, objective=c['obj'], steps=steps,
               warmup=warmup, reps=reps)
    for label, fam in fams.items():
        obj = (vb.black_box_klvi(fam, tgt, N) if c['obj'] == 'klvi'
               else vb.black_box_chivi(2.0, fam, tgt, N))
        ts = _time(lambda: vb.adagrad_optimize(steps, obj, init, learning_rate=1e-3), sync, warmup,
                   reps)
        res[label + '_us_per_step'] = round(1e6 * statistics.median(ts) / steps, 2)
        res[label + '_us_per_step_all'] = [round(1e6 * t / steps, 2) for t in ts]
    res['t_over_cholesky'] = round(res['t_df1e6_us_per_step'] / res['cholesky_gaussian_us_per_step'], 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['all'] + list(CASES))
    ap.add_argument('--steps', type=int, default=0, help='iterations per call (0: the case default)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    for name in (list(CASES) if a.case == 'all' else [a.case]):
        run_case(name, a.steps, a.warmup, a.reps)


if __name__ == '__main__':
    main()
