"""vb_rhat.hip at edge shapes, against the 50-digit reference of tests/rhat_mp.py:
every case runs as one batched launch (all its segments together); the nan pattern
of half-chains of one draw is compared exactly, var_hat and R-hat within

    8 x RHAT_ORACLE_ERR[quantity]   in units of 2^-53 S

and never looser than the rtol of 1e-12 tests/test_gpu_ia.py already uses.  The
two-stage form (rhat_stats, then rhat_combine) must give vb_rhat's bits, and
stochastic_iterate_averaging numpy's cumulative means bit for bit (the same
summation order)."""
import numpy as np
import pytest

from tests import rhat_mp as rm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not rm.available(), reason='needs mpmath')]


def _within(quantity, got, hi, lo, S, what):
    e = rm.err(got, hi, lo, S)
    bound = rm.device_bound(quantity, hi, S)
    print('RHAT_EDGE %s %s err %.3g x 2^-53 S (bound %.1f)'
          % (what, quantity, float(np.max(e)), rm.MARGIN * rm.RHAT_ORACLE_ERR[quantity][0]))
    with np.errstate(invalid='ignore'):
        d = np.abs((np.asarray(got, dtype=float) - hi) - lo)
    bad = ~((d <= bound) | (e == 0))
    assert not np.any(bad), (what, quantity, float(np.max(e)))


@pytest.mark.parametrize('name', rm.CASES)
def test_rhat_matches_multiprecision(name):
    from viabel_amd import functions as F
    rm.check_case(name)
    x, segs = rm.case(name)
    var, rhat = F._rhat_batch(x.copy(), list(segs), return_var=True)
    assert var.shape == rhat.shape == (len(segs), x.shape[2])
    for j, ((s, ln), (vref, rref)) in enumerate(zip(segs, rm.reference(name))):
        what = '%s [%d, +%d)' % (name, s, ln)
        np.testing.assert_array_equal(np.isnan(var[j]), np.isnan(vref[0]))
        np.testing.assert_array_equal(np.isnan(rhat[j]), np.isnan(rref[0]))
        if ln == 2:
            assert np.all(np.isnan(var[j])) and np.all(np.isnan(rhat[j]))
            continue
        _within('var_hat', var[j], *vref, what=what)
        _within('rhat', rhat[j], *rref, what=what)
        # each segment alone: the same bits as in the batch
        v1, r1 = F._rhat_batch(x.copy(), [(s, ln)], return_var=True)
        np.testing.assert_array_equal(v1[0], var[j])
        np.testing.assert_array_equal(r1[0], rhat[j])
    if len(segs) == 1 and segs[0][1] > 2:
        v, r = F.compute_R_hat(x.copy(), warmup=0)
        np.testing.assert_array_equal(v, var[0])
        np.testing.assert_array_equal(r, rhat[0])
    # two stages (as chains held by several ranks combine): the same bits
    mean, ss = F.rhat_stats(x.copy(), list(segs))
    v2, r2 = F.rhat_combine(mean, ss, [ln for _, ln in segs], return_var=True)
    np.testing.assert_array_equal(v2, var)
    np.testing.assert_array_equal(r2, rhat)


@pytest.mark.parametrize('cols', [1, 257])
@pytest.mark.parametrize('start', ['0', '1', 'n-1'])
def test_iterate_averaging_is_numpy_cumsum_bit_for_bit(start, cols):
    from viabel_amd import functions as F
    n = 37
    x = np.random.RandomState(700 + cols).randn(n, cols) * 3.0 + 0.7
    s = {'0': 0, '1': 1, 'n-1': n - 1}[start]
    iters, last = F.stochastic_iterate_averaging(x.copy(), s)
    expect = np.cumsum(x[s:], axis=0) / np.arange(1, n - s + 1)[:, None]
    np.testing.assert_array_equal(iters, expect)
    np.testing.assert_array_equal(last, expect[-1])
