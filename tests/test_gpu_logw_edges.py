"""The Philox log-weight kernels against the 50-digit reference of tests/logw_mp.py,
which starts from the draws' integers: logw_row_kernel<.., HOST = false> (its four
register instances, the t family's product-of-(1 + y) log q and the Gaussian family's
normal_pair_tab draws), logw_sep_kernel<.., HOST = false>, and sample_bailey_kernel
followed by the target and launch_family_logdensity, on every case of
tests/logw_cases.py: launch edges (m around 256 rows, 4 rows, 256 (row, pair) threads; D
around the 64-pair pass, odd D), df from 2.000001 to 1e6, log sigma in [-30, 30] and
|mu| = 30, and the planted tail draws (U1 < 2^-28, U1 -> 1, cos(2 pi U2) at and beside its
zeros and extrema).

Every entry of x is held to 8 x the oracle's 'sample' figure and every row's log
weight to 8 x its 'log_w' figure, each in units of 2^-53 of its own condition sum
(logw_mp's docstring): no row is scaled by the call's largest.  The t family on the row
kernel takes log q at the draw itself and is held to the smaller 'direct' sum; every
other path reads log q back from the rounded x ('back').  A case's second call is
compared with step 1's draws.

Measured on an MI355X (worst over all cases; bar):
  row  sample 2.66 (20.96)   log_w 1.36 (14.64)
  sep  sample 2.48 (20.96)   log_w 0.65 (14.64)
  mat  sample 1.90 (20.96)   log_w 0.65 (14.64)
The row kernel's product form at df = 1e3 and 1e6 stays inside the bar (0.71 and 0.69
units, both the rounding of the t density's constant): lgamma((df + 1) / 2) - lgamma(df /
2) puts ~df (log(df / 2) - 1) per coordinate into the condition sum, as its own double
rounding demands (1e-9 D at df = 1e6), and the product's (df + 1) / 2 roundings of 2^-53
stay below 1.5 units of it at every df.

VIABEL_AMD_LOGW_EDGE_RECORD=<path> writes the worst error per kernel and class beside
its bar and the oracle's figure (profiles/logw_mp/errors.json)."""
import json
import os

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests import logw_cases as lc
from tests import logw_mp as lm
from tests import mf_mp as mm

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not lm.available(), reason='needs mpmath')]

WORST = {}
ABS_ROW_T = {}     # the row kernel's t branch: worst |lw - ref| per df (reported, not asserted)


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    path = os.environ.get('VIABEL_AMD_LOGW_EDGE_RECORD')
    if path:
        out = {'_note': 'worst error over the cases of tests/logw_cases.py in units of 2^-53 S: '
                        '[error, bar, oracle figure, case]; row_t_abs: worst absolute error of the '
                        'row kernel\'s t-family log weights per df'}
        for (kernel, cls), (e, cid) in sorted(WORST.items()):
            out.setdefault(kernel, {})[cls] = [float('%.4g' % e), lm.bar(cls),
                                               lm.oracle_figure(cls), cid]
        out['row_t_abs'] = {'%.7g' % df: float('%.3g' % v) for df, v in sorted(ABS_ROW_T.items())}
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


def _note(kernel, cls, err, cid):
    if err >= WORST.get((kernel, cls), (-1.0, ''))[0]:
        WORST[(kernel, cls)] = (float(err), cid)


def _family(c):
    from viabel_amd import vb
    if c['kind'] == 'gauss':
        fam = vb.mean_field_gaussian_variational_family(c['D'], rng='philox')
    else:
        fam = vb.mean_field_t_variational_family(c['D'], c['df'], rng='philox')
    fam.seed, fam.stream, fam.step = lc.SEED, c['stream'], c['step0']
    return fam


def _target(c):
    from viabel_amd import targets
    if c['target'] == 'eight_schools_ncp':
        return targets.eight_schools_ncp()
    return getattr(targets, c['target'])(c['D'])


@pytest.mark.parametrize('c', lc.CASES, ids=[c['id'] for c in lc.CASES])
def test_log_weights_match_multiprecision(c):
    from viabel_amd import experiments
    direct = c['kernel'] == 'row' and c['kind'] == 't'
    tgt = _target(c)
    for m, n in c['calls']:
        fam = _family(c)
        prev = None
        for k in range(n):
            step = c['step0'] + k
            ref = lm.case_reference(c, step)
            x, lw = experiments.log_weights(tgt, fam, c['lam'], m)
            assert x.shape == (m, c['D']) and lw.shape == (m,)
            rlw = lm.rows_of(ref.lw_direct if direct else ref.lw_back, m)
            ex = float(mm.units(x, lm.rows_of(ref.x, m)).max())
            ew = float(mm.units(lw, rlw).max())
            print('LOGW_EDGE %s m %d step %d: sample %.3f log_w %.3f' % (c['id'], m, step, ex, ew))
            _note(c['kernel'], 'sample', ex, c['id'])
            _note(c['kernel'], 'log_w', ew, c['id'])
            if direct and not c['id'].startswith('edge/'):     # central lam: |lw| of order D
                ABS_ROW_T[c['df']] = max(ABS_ROW_T.get(c['df'], 0.0),
                                         float(np.max(np.abs((lw - rlw.hi) - rlw.lo))))
            assert ex <= lm.bar('sample'), ('sample', ex, lm.bar('sample'))
            assert ew <= lm.bar('log_w'), ('log_w', ew, lm.bar('log_w'))
            # the second call drew anew (and matched step 1's reference above)
            assert prev is None or not np.array_equal(prev, x)
            prev = x
        assert fam.step == c['step0'] + n
