"""Step time of adagrad_optimize with the low-rank-plus-diagonal Gaussian family
(vb.low_rank_gaussian_variational_family) beside the Cholesky full-rank Gaussian and the
materialised mean-field Gaussian at equal D, on the same build and in the same process.
Prints one JSON line per case (and appends it to --out).

  eight_schools     eight_schools_ncp, D = 10, N = 100, KLVI; R = 2; beside cholesky
  corr512_klvi      corr_gauss, D = 512, N = 128, KLVI; R = 4, 16, 64; beside cholesky
  corr512_chivi     the same with CHIVI alpha = 2
  funnel1e4         funnel, D = 10 000, N = 128, KLVI; R = 4, 16; beside mean-field Gaussian
                    (non-separable target at D > 16: the materialised path)
  regression        student-t regression, D = 32, M = 100 000, N = 100, KLVI; R = 4; beside
                    cholesky

The cholesky times of eight_schools, corr512_* and regression are scripts/frg_bench.py's
cases (profiles/frg/frg_bench.jsonl): they show whether anything else moved.

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
    'eight_schools': dict(target='eight_schools_ncp', D=10, N=100, obj='klvi', steps=500,
                          ranks=(2,), beside='cholesky'),
    'corr512_klvi': dict(target='corr_gauss', D=512, N=128, obj='klvi', steps=200,
                         ranks=(4, 16, 64), beside='cholesky'),
    'corr512_chivi': dict(target='corr_gauss', D=512, N=128, obj='chivi', steps=200,
                          ranks=(4, 16, 64), beside='cholesky'),
    'funnel1e4': dict(target='funnel', D=10000, N=128, obj='klvi', steps=100,
                      ranks=(4, 16), beside='mean_field'),
    'regression': dict(target='regression', D=32, N=100, obj='klvi', steps=50, M=100000,
                       ranks=(4,), beside='cholesky'),
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
    elif c['target'] == 'funnel':
        tgt = targets.funnel(D)
    else:
        tgt = targets.eight_schools_ncp()
    fams = {'low_rank_r%d' % r: vb.low_rank_gaussian_variational_family(D, r, rng='philox')
            for r in c['ranks']}
    if c['beside'] == 'cholesky':
        fams['cholesky_gaussian'] = vb.cholesky_gaussian_variational_family(D, rng='philox')
    else:
        fams['mean_field_gaussian'] = vb.mean_field_gaussian_variational_family(D, rng='philox')
    sync = nat.context().synchronize
    res = dict(case=name, target=c['target'], D=D, N=N, objective=c['obj'], steps=steps,
               warmup=warmup, reps=reps)
    for label, fam in fams.items():
        obj = (vb.black_box_klvi(fam, tgt, N) if c['obj'] == 'klvi'
               else vb.black_box_chivi(2.0, fam, tgt, N))
        init = np.zeros(fam.var_param_dim)
        ts = _time(lambda: vb.adagrad_optimize(steps, obj, init, learning_rate=1e-3), sync, warmup,
                   reps)
        res[label + '_us_per_step'] = round(1e6 * statistics.median(ts) / steps, 2)
        res[label + '_us_per_step_all'] = [round(1e6 * t / steps, 2) for t in ts]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['all'] + list(CASES))
    ap.add_argument('--steps', type=int, default=0, help='iterations per call (0: the case default)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='', help='append the JSON lines to this file')
    a = ap.parse_args()
    for name in (list(CASES) if a.case == 'all' else [a.case]):
        res = run_case(name, a.steps, a.warmup, a.reps)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
