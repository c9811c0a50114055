"""The hierarchical normal-means kernels (vb_hier.hip) away from the origin: the
device values at the edge sets of tests/hier_mp.py, both forms and every J (the
lane-per-row kernel's three instances at J = 1, 8, 14; the wave-per-row kernel at
J = 15 and 65), against the 50-digit reference: value and every gradient entry
within 8 x HIER_ORACLE_ERR in units of 2^-53 S.  The factor 8 is the margin the
target kernels have over their numpy oracle (tests/test_gpu_targets_edges.py): the
device helpers are ~1 ulp forms where libm is ~0.5, reciprocals replace divisions,
and the wave tree sums in another order.  Then log tau = +-400, where tau^2 or
1 / tau^2 leaves the double range.

Measured worst errors on MI355X are in DESIGN.md §7c.
"""
import numpy as np
import pytest

from tests import hier_cases as hc
from tests import hier_mp as hm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

MARGIN = 8.0


@pytest.mark.skipif(not hm.available(), reason='needs mpmath')
@pytest.mark.parametrize('J,centered', hm.CASES)
def test_kernels_at_edge_points(J, centered):
    from viabel_amd import targets
    x, ref = hm.edge_reference(J, centered)
    y, sigma = hm.data(J)
    t = targets.hierarchical_normal(y, sigma, centered=centered)
    lp, g = t.logdensity_and_grad(np.array(x))
    e_lp, e_g = hm.errors(lp, g, ref)
    r, (gr, gc) = int(np.argmax(e_lp)), np.unravel_index(int(np.argmax(e_g)), e_g.shape)
    bound = MARGIN * hm.HIER_ORACLE_ERR[centered]
    print('HIER EDGE J=%d centred=%d: value %.3f (row %d, x[:2] = %r), gradient %.3f (row %d, '
          'column %d, x[:2] = %r); bound %.2f x 2^-53 S'
          % (J, centered, e_lp[r], r, x[r, :2].tolist(), e_g[gr, gc], gr, gc, x[gr, :2].tolist(),
             bound))
    assert e_lp[r] <= bound
    assert e_g[gr, gc] <= bound


@pytest.mark.parametrize('centered', hm.FORMS)
@pytest.mark.parametrize('J', hm.SIZES + (600,))
def test_log_tau_at_plus_minus_400(centered, J):
    """u = +-400 with the other coordinates standard normal: no NaN in log p, and
    -inf only where the restatement also leaves the double range."""
    from viabel_amd import targets
    y, sigma = hc.make_data(J, 31)
    t = targets.hierarchical_normal(y, sigma, centered=centered)
    f = hc.restatement(y, sigma, centered)
    x = np.random.RandomState(32 + J).randn(40, J + 2)
    x[:20, 1] = 400.0
    x[20:, 1] = -400.0
    lp, _ = t.logdensity_and_grad(x)
    with np.errstate(all='ignore'):
        lp0, _ = f(x)
    assert not np.any(np.isnan(lp0))
    assert not np.any(np.isnan(lp))
    assert np.all(lp < np.inf)
    fin = np.isfinite(lp0)
    assert np.all(np.isfinite(lp[fin]))
    np.testing.assert_allclose(lp[fin], lp0[fin], rtol=1e-11)
