"""Times a KLVI adagrad fit of the robust-regression model through its three routes:

  callback   targets.callback of the numpy restatement (host round trip per step)
  plugin     targets.example_model('robust_regression'): the model as a code object
  builtin    targets.robust_regression (VB_TARGET_REGRESSION)

for the notebook's shape (D = 2, M = 25, N = 100, 5000 steps) and a wider one (D = 32,
M = 4096, N = 128, 500 steps).  Philox draws on the device, so the routes differ in the
target alone.  Each figure is the median of 5 timed fits after one warm-up fit; a fit ends
with its results on the host, so the clock stops after the device has finished.  Writes
one JSON line per setup to profiles/plugin/plugin_bench.jsonl (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def restatement(x, y, nu):
    def f(b):
        r = y[None, :] - b @ x.T
        lp = (-0.5 * np.sum((b / 10.0) ** 2, axis=1)
              - (nu + 1) / 2 * np.sum(np.log1p(r ** 2 / nu), axis=1))
        return lp, -b / 100.0 + ((nu + 1) * r / (nu + r ** 2)) @ x
    return f


def fit_seconds(target, D, N, n_iters, reps, warmup):
    from viabel_amd import vb, _native as nat
    times = []
    for k in range(warmup + reps):
        fam = vb.mean_field_gaussian_variational_family(D, rng='philox')
        obj = vb.black_box_klvi(fam, target, N)
        nat.context().synchronize()
        t0 = time.perf_counter()
        vb.adagrad_optimize(n_iters, obj, np.zeros(2 * D), learning_rate=0.01)
        nat.context().synchronize()
        if k >= warmup:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plugin', 'plugin_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    a = ap.parse_args()
    os.environ.setdefault('VIABEL_AMD_PROGRESS', '0')
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_plugin.py measures on the GPU: no device visible')
    from viabel_amd import targets, _native as nat
    setups = [dict(name='notebook', D=2, M=25, N=100, n_iters=5000, nu=40.0),
              dict(name='wide', D=32, M=4096, N=128, n_iters=500, nu=4.0)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as out:
        for s in setups:
            rs = np.random.RandomState(7)
            x = rs.randn(s['M'], s['D'])
            y = x @ rs.randn(s['D']) / np.sqrt(s['D']) + rs.standard_t(5, s['M'])
            routes = {
                'callback': targets.callback(restatement(x, y, s['nu']), s['D']),
                'plugin': targets.example_model('robust_regression', x, y, s['nu']),
                'builtin': targets.robust_regression(x, y, s['nu'], prior_scale=10.0),
            }
            rec = dict(s, reps=a.reps, warmup=a.warmup, build_id=nat.lib().vb_build_id().decode(),
                       device=torch.cuda.get_device_name(0))
            for route, target in routes.items():
                med, lo, hi = fit_seconds(target, s['D'], s['N'], s['n_iters'], a.reps, a.warmup)
                rec[route + '_s'] = med
                rec[route + '_us_per_step'] = 1e6 * med / s['n_iters']
                rec[route + '_range_s'] = [lo, hi]
            rec['plugin_over_callback'] = rec['plugin_s'] / rec['callback_s']
            rec['plugin_over_builtin'] = rec['plugin_s'] / rec['builtin_s']
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + '\n')


if __name__ == '__main__':
    main()
