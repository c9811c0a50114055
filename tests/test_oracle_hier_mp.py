"""The numpy restatement of the hierarchical normal-means target
(tests/hier_cases.py), the reference of tests/test_gpu_hier.py, pinned: over the edge
sets of tests/hier_mp.py its values and gradients stay within twice the recorded
HIER_ORACLE_ERR of a 50-digit mpmath restatement, in units of 2^-53 S; its gradient
is the derivative of its value; and its non-centred form at the eight-schools data
is the oracle's eight-schools function.  CPU only."""
import numpy as np
import pytest

from tests import hier_cases as hc
from tests import hier_mp as hm

needs_mp = pytest.mark.skipif(not hm.available(), reason='needs mpmath')


def _errors(J, centered):
    x, ref = hm.edge_reference(J, centered)
    y, sigma = hm.data(J)
    # the restatement must not overflow or divide by zero on the way
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = hc.restatement(y, sigma, centered)(np.array(x))
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    return x, hm.errors(lp, g, ref)


@needs_mp
@pytest.mark.parametrize('J,centered', hm.CASES)
def test_restatement_matches_multiprecision(J, centered):
    x, (e_lp, e_g) = _errors(J, centered)
    r, (gr, gc) = int(np.argmax(e_lp)), np.unravel_index(int(np.argmax(e_g)), e_g.shape)
    print('HIER ORACLE J=%d centred=%d: value %.3f (row %d, x[:2] = %r), gradient %.3f (row %d, '
          'column %d, x[:2] = %r) x 2^-53 S'
          % (J, centered, e_lp[r], r, x[r, :2].tolist(), e_g[gr, gc], gr, gc, x[gr, :2].tolist()))
    assert max(e_lp[r], e_g[gr, gc]) <= 2.0 * hm.HIER_ORACLE_ERR[centered]


@needs_mp
@pytest.mark.parametrize('centered', hm.FORMS)
def test_recorded_figures_are_the_measured_ones(centered):
    """HIER_ORACLE_ERR is the measured worst case, not a loose cap."""
    worst = max(max(float(e.max()) for e in _errors(J, centered)[1]) for J in hm.SIZES)
    assert 0.5 * hm.HIER_ORACLE_ERR[centered] <= worst <= hm.HIER_ORACLE_ERR[centered] * 1.001


@needs_mp
def test_edge_sets_cover_the_documented_points():
    for J, centered in hm.CASES:
        x = hm.edge_points(J, centered)
        assert x.shape[1] == J + 2 and x.shape[0] <= 600
        for lt in hm.ES_LOG_TAU:
            assert np.sum(x[:, 1] == lt) >= (6 if centered else 3)
        for m in (30.0, -30.0):
            assert np.sum(np.abs(x[:, 0] - m) <= hm.tm.JITTER * 30.0) >= 7 * hm.BLOCK_ROWS
        if centered:
            # the posterior's own region: th within a few tau of mu at a tiny tau
            z = (x[:, 2:] - x[:, :1]) / np.exp(x[:, 1:2])
            small = x[:, 1] < -39.0
            assert np.sum(small & (np.abs(z).max(axis=1) < 6.0)) >= 3 * hm.BLOCK_ROWS - 3
            assert np.sum(small & (np.abs(z).max(axis=1) > 1e10)) >= 3 * hm.BLOCK_ROWS - 3


@pytest.mark.parametrize('centered', hm.FORMS)
def test_restatement_gradient_matches_central_differences(centered):
    J = 3
    y, sigma = hc.make_data(J, 5)
    f = hc.restatement(y, sigma, centered, mu_scale=3.0, tau_scale=2.0)
    b = np.random.RandomState(6).randn(5, J + 2)
    lp, g = f(b)
    assert lp.shape == (5,) and g.shape == (5, J + 2)
    h = 1e-5
    for d in range(J + 2):
        e = np.zeros(J + 2)
        e[d] = h
        fd = (f(b + e)[0] - f(b - e)[0]) / (2 * h)
        # central differences: O(h^2) truncation + rounding of |log p| ~ 1e2 over 2h
        np.testing.assert_allclose(g[:, d], fd, rtol=1e-6, atol=1e-7)


def test_non_centred_restatement_is_the_oracle_eight_schools():
    from oracle import targets_oracle
    f = hc.restatement(hc.ES_Y, hc.ES_SIGMA, False)
    x = np.random.RandomState(7).randn(200, 10)
    lp, g = f(x)
    lp0, g0 = targets_oracle.TARGETS['eight_schools_ncp'](x)
    np.testing.assert_allclose(lp, lp0, rtol=1e-13, atol=0)
    assert np.max(np.abs(g - g0)) <= 1e-13 * np.max(np.abs(g0))
