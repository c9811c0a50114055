"""The multilevel regression kernels (vb_mlm.hip) away from the origin: the device values
at the edge sets of tests/mlm_mp.py, both forms, the three links and every shape (the
lane-per-row kernel's four instances at G = 1, 8 and 70 over one, two, three and six
observation chunks, a group spanning chunks, empty groups; the tile kernel at p = 17 and
40), against the 50-digit reference: value and every gradient entry within
8 x MLM_ORACLE_ERR in units of 2^-53 S, the margin the regression and hierarchical
kernels have over their numpy oracles.  Then log tau = +-400, where tau^2 or 1 / tau^2
leaves the double range.

Measured worst errors on MI355X are in DESIGN.md §7d.
"""
import numpy as np
import pytest

from tests import mlm_cases as mc
from tests import mlm_mp as mm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

MARGIN = 8.0


@pytest.mark.skipif(not mm.available(), reason='needs mpmath')
@pytest.mark.parametrize('lik,centered,p,G,M', mm.cases())
def test_kernels_at_edge_points(lik, centered, p, G, M):
    from viabel_amd import targets
    c, ref = mm.edge_reference(lik, centered, p, G, M)
    t = targets.multilevel_regression(c.x, c.y, c.group, n_groups=G, **c.kw)
    lp, g = t.logdensity_and_grad(np.array(c.z))
    e_lp, e_g = mm.errors(lp, g, ref)
    r, (gr, gc) = int(np.argmax(e_lp)), np.unravel_index(int(np.argmax(e_g)), e_g.shape)
    bound = MARGIN * mm.MLM_ORACLE_ERR[centered]
    print('MLM EDGE %s centred=%d p=%d G=%d M=%d: value %.3f (row %d, u = %r), gradient %.3f '
          '(row %d, column %d, u = %r); bound %.2f x 2^-53 S'
          % (lik, centered, p, G, M, e_lp[r], r, float(c.z[r, p]), e_g[gr, gc], gr, gc,
             float(c.z[gr, p]), bound))
    assert e_lp[r] <= bound
    assert e_g[gr, gc] <= bound


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('lik', mc.LIKELIHOODS)
@pytest.mark.parametrize('p,G,M', [(3, 8, 129), (17, 3, 65)])
def test_log_tau_at_plus_minus_400(p, G, M, lik, centered):
    """u = +-400 with the other coordinates standard normal: no NaN in log p, and -inf
    only where the restatement also leaves the double range."""
    from viabel_amd import targets
    x, y, g = mc.make_data(p, G, M, lik, 31)
    kw = mc.model_kwargs(lik, centered)
    t = targets.multilevel_regression(x, y, g, n_groups=G, **kw)
    f = mc.restatement(x, y, g, n_groups=G, **kw)
    z = np.random.RandomState(32 + G).randn(40, p + 1 + G)
    z[:20, p] = 400.0
    z[20:, p] = -400.0
    lp, _ = t.logdensity_and_grad(z)
    with np.errstate(all='ignore'):
        lp0, _ = f(z)
    assert not np.any(np.isnan(lp0))
    assert not np.any(np.isnan(lp))
    assert np.all(lp < np.inf)
    fin = np.isfinite(lp0)
    assert np.all(np.isfinite(lp[fin]))
    assert np.all(np.isneginf(lp[~fin]))
    np.testing.assert_allclose(lp[fin], lp0[fin], rtol=1e-11)
