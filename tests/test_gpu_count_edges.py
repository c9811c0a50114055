"""The poisson_log and neg_binomial_2_log instances of the regression and multilevel
kernels (viabel_amd/csrc/vb_glm.hip, vb_mlm.hip) at the edge data and rows of
tests/count_mp.py, against the 50-digit reference written from the probability mass
functions: the value and every gradient entry within MARGIN = 8 x COUNT_ORACLE_ERR in
units of 2^-53 S (the factor tests/test_gpu_glm_edges.py grants device kernels, for the
same reasons), an exact 0 where S = 0.  Which instance a shape reaches is in the
docstrings of tests/test_gpu_glm_edges.py and tests/mlm_mp.py.  Measured worst errors
on MI355X are in DESIGN.md §7b."""
import numpy as np
import pytest

from tests import count_cases as cc
from tests import count_mp as cm
from tests import mlm_cases as mc
from tests.conftest import gpu_available
from tests.test_gpu_glm_edges import _value_only

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not cm.available(), reason='needs mpmath')]

MARGIN = 8.0


def _target(c):
    from viabel_amd import targets
    return targets.regression(c.x, c.y, offset=c.offset, **c.kw)


def _check(tag, key, shape, lp, g, ref):
    bound = MARGIN * cm.COUNT_ORACLE_ERR[key]
    e_lp, e_g = cm.errors(lp, np.zeros_like(ref.g_hi) if g is None else g, ref)
    r = int(np.argmax(e_lp))
    msg = 'EDGE %s %s %s %r: value %.3f (row %d)' % (tag, key[0], key[1], shape, e_lp[r], r)
    if g is not None:
        gr, gcol = np.unravel_index(int(np.argmax(e_g)), e_g.shape)
        msg += ', gradient %.3f (row %d, column %d)' % (e_g[gr, gcol], gr, gcol)
    print(msg + '; bound %.2f x 2^-53 S' % bound)
    assert e_lp[r] <= bound
    if g is not None:
        assert e_g[gr, gcol] <= bound


def _run(tag, lik, D, M, n):
    c, ref = cm.edge_reference(lik, D, M, n)
    lp, g = _target(c).logdensity_and_grad(np.array(c.beta))
    assert lp.shape == (n,) and g.shape == (n, D)
    _check(tag, ('regression', lik), (D, M, n), lp, g, ref)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', cm.SHAPES_SMALL)
def test_lane_per_row_kernel(lik, D, M, n):
    _run('small', lik, D, M, n)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', cm.SHAPES_MFMA)
def test_matrix_kernel(lik, D, M, n):
    _run('mfma', lik, D, M, n)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', cm.SHAPES_CHUNK)
def test_six_observation_chunks(lik, D, M, n):
    _run('chunks', lik, D, M, n)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', cm.SHAPES_VALUE)
def test_value_only(lik, D, M, n):
    """GRAD = false (a null grad_out), and the with-gradient call beside it: the same
    value bit for bit."""
    c, ref = cm.edge_reference(lik, D, M, n)
    t = _target(c)
    lp = _value_only(t, np.array(c.beta))
    _check('value-only', ('regression', lik), (D, M, n), lp, None, ref)
    lp_g, g = t.logdensity_and_grad(np.array(c.beta))
    _check('value-only shape, with gradient', ('regression', lik), (D, M, n), lp_g, g, ref)
    assert np.array_equal(lp, lp_g)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('p,G,M', cm.MLM_SHAPES)
def test_multilevel_kernels(lik, centered, p, G, M):
    """(2, 1, 40), (3, 8, 129), (16, 70, 321): the lane kernel at PP = 2, 4, 16 over one,
    three and six chunks, groups spanning chunk boundaries, empty groups; (17, 3, 65):
    the tile kernel with two column slices."""
    from viabel_amd import targets
    c, ref = cm.mlm_edge_reference(lik, centered, p, G, M)
    t = targets.multilevel_regression(c.x, c.y, c.group, n_groups=G, offset=c.offset, **c.kw)
    lp, g = t.logdensity_and_grad(np.array(c.z))
    _check('mlm', ('multilevel', lik), (int(centered), p, G, M), lp, g, ref)
    assert np.array_equal(_value_only(t, np.array(c.z)), lp)


@pytest.mark.parametrize('D', [3, 20])
@pytest.mark.parametrize('eta', [710.0, 800.0])
@pytest.mark.parametrize('y0', [0.0, 3.0])
def test_poisson_value_is_minus_inf_beyond_exps_range(D, eta, y0):
    """No clamp: -inf on the device and in the restatement; the other rows stay finite
    and close.  The gradient there is whatever IEEE gives and is not asserted."""
    from viabel_amd import targets
    x, y, off = cc.make_data(D, 65, 'poisson_log', seed=5)
    off[0], y[0] = 0.0, y0
    t = targets.poisson_regression(x, y, offset=off, prior_scale=3.0)
    f = cc.restatement(x, y, 'poisson_log', offset=off, prior_scale=3.0)
    b = np.random.RandomState(6).randn(4, D) * 0.3
    b[0] = eta * x[0] / (x[0] @ x[0])
    lp, _ = t.logdensity_and_grad(b)
    lp0, _ = f(b)
    assert lp[0] == -np.inf and lp0[0] == -np.inf
    assert np.all(np.isfinite(lp[1:]))
    np.testing.assert_allclose(lp[1:], lp0[1:], rtol=1e-11)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
def test_two_calls_give_the_same_bits(lik):
    c = cm.edge_case(lik, 130, 321, 10)
    t = _target(c)
    lp1, g1 = t.logdensity_and_grad(np.array(c.beta))
    lp2, g2 = t.logdensity_and_grad(np.array(c.beta))
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('D', [3, 40])
def test_zero_offset_equals_no_offset(lik, D):
    from viabel_amd import targets
    x, y, _ = cc.make_data(D, 130, lik, seed=9)
    kw = cc.model_kwargs(lik)
    b = np.random.RandomState(10).randn(20, D) * 0.3
    lp1, g1 = targets.regression(x, y, **kw).logdensity_and_grad(b)
    lp2, g2 = targets.regression(x, y, offset=np.zeros(130), **kw).logdensity_and_grad(b)
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)


@pytest.mark.parametrize('D', [3, 40])
def test_negative_binomial_tends_to_poisson(D):
    """At phi = 1e6 the gradient agrees with the Poisson's on the same data to 1e-5
    relative to its largest entry: a check of the limit, not an accuracy bar.  The two
    l' differ by mu (mu - y) / (phi + mu), a share ~ mu / phi of the gradient, so the data
    keep the means small: exposures at most 1 and |x . beta| ~ 0.3, mu < 3."""
    from viabel_amd import targets
    x, y, off = cc.make_data(D, 130, 'poisson_log', seed=11)
    off = off - np.log(4.0)
    y = np.minimum(y, 5.0)
    b = np.random.RandomState(12).randn(20, D) * 0.3 / np.sqrt(D)
    _, g1 = targets.poisson_regression(x, y, offset=off).logdensity_and_grad(b)
    _, g2 = targets.negative_binomial_regression(x, y, 1e6, offset=off).logdensity_and_grad(b)
    print('limit D=%d: max |g_nb - g_pois| / max |g_pois| = %.3g'
          % (D, float(np.max(np.abs(g1 - g2))) / float(np.max(np.abs(g1)))))
    assert float(np.max(np.abs(g1 - g2))) <= 1e-5 * float(np.max(np.abs(g1)))
