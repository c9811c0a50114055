"""The learned instances of the regression kernels (viabel_amd/csrc/vb_glm.hip: a learned
sigma for gaussian and student_t, a learned phi for neg_binomial_2_log) at the edge data
and rows of tests/aux_mp.py, against the 50-digit reference written from the densities,
the lambda gradient by mp.diff: the value and every gradient entry within MARGIN = 8 x
AUX_ORACLE_ERR in units of 2^-53 S (the factor tests/test_gpu_glm_edges.py grants device
kernels, for the same reasons), an exact 0 where S = 0, a finite result where S = inf.
Which instance a shape reaches is beside aux_mp.SHAPES: the kernel, DP and NCT are chosen
by p as a fixed block with D = p chooses them.  Measured worst errors on MI355X are in
DESIGN.md §7b."""
import numpy as np
import pytest

from tests import aux_cases as ac
from tests import aux_mp as am
from tests.conftest import gpu_available
from tests.test_gpu_glm_edges import _value_only

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not am.available(), reason='needs mpmath')]

MARGIN = 8.0


def _target(c):
    from viabel_amd import targets
    return targets.regression(c.x, c.y, offset=c.offset, **ac.target_kwargs(c.kw))


def _check(tag, lik, shape, lp, g, ref):
    bound = MARGIN * am.AUX_ORACLE_ERR[lik]
    e_lp, e_g = am.errors(lp, np.zeros_like(ref.g_hi) if g is None else g, ref)
    r = int(np.argmax(e_lp))
    msg = 'EDGE %s %s %r: value %.3f (row %d)' % (tag, lik, shape, e_lp[r], r)
    if g is not None:
        gr, gcol = np.unravel_index(int(np.argmax(e_g[:, :-1])), e_g[:, :-1].shape)
        lr = int(np.argmax(e_g[:, -1]))
        msg += ', coefficients %.3f (row %d, column %d), lambda %.3f (row %d)' % (
            e_g[gr, gcol], gr, gcol, e_g[lr, -1], lr)
    print(msg + '; bound %.2f x 2^-53 S' % bound)
    assert e_lp[r] <= bound
    if g is not None:
        assert e_g[gr, gcol] <= bound
        assert e_g[lr, -1] <= bound


def _run(tag, lik, p, M, n, kind=None):
    c, ref = am.edge_reference(lik, p, M, n, kind)
    lp, g = _target(c).logdensity_and_grad(np.array(c.z))
    assert lp.shape == (n,) and g.shape == (n, p + 1)
    _check(tag, lik, (p, M, n) + ((kind,) if kind else ()), lp, g, ref)


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
@pytest.mark.parametrize('p,M,n', am.SHAPES)
def test_value_and_gradient(lik, p, M, n):
    _run('lane' if p <= 16 else 'matrix', lik, p, M, n)


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
@pytest.mark.parametrize('p,M,n', am.SHAPES_VALUE)
def test_value_only(lik, p, M, n):
    """GRAD = false (a null grad_out), and the with-gradient call beside it: the same
    value bit for bit."""
    c, ref = am.edge_reference(lik, p, M, n)
    t = _target(c)
    lp = _value_only(t, np.array(c.z))
    _check('value-only', lik, (p, M, n), lp, None, ref)
    lp_g, g = t.logdensity_and_grad(np.array(c.z))
    _check('value-only shape, with gradient', lik, (p, M, n), lp_g, g, ref)
    assert np.array_equal(lp, lp_g)


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
def test_two_calls_give_the_same_bits(lik):
    c = am.edge_case(lik, 130, 321, 10)
    t = _target(c)
    lp1, g1 = t.logdensity_and_grad(np.array(c.z))
    lp2, g2 = t.logdensity_and_grad(np.array(c.z))
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)


@pytest.mark.parametrize('kind', am.TABLE_KINDS)
def test_dispersion_tables(kind):
    """J = 0 (no table), J = 1 (an empty sum) and J = 65536 at (2, 40, 17), value only
    beside it, and twice for the bits."""
    lik = 'neg_binomial_2_log'
    p, M, n = am.SHAPE_TABLE
    _run('table', lik, p, M, n, kind)
    c = am.edge_case(lik, p, M, n, kind)
    t = _target(c)
    assert t.params[8 + M * p + 2 * M + 1] == {'zero': 0, 'binary': 1, 'big': 65536}[kind]
    lp1, g1 = t.logdensity_and_grad(np.array(c.z))
    lp2, g2 = t.logdensity_and_grad(np.array(c.z))
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)
    assert np.array_equal(_value_only(t, np.array(c.z)), lp1)


@pytest.mark.parametrize('lik', ['gaussian', 'student_t'])
@pytest.mark.parametrize('p', [3, 20])
def test_zero_residuals_give_minus_m(lik, p):
    """Residuals of exactly 0: d/dlambda is -M plus the prior's 1 - 2 logistic(w), the
    coefficient gradient is the prior's -beta / s^2, to the last bit."""
    from viabel_amd import targets
    M = 65
    x = np.random.RandomState(3).randn(M, p)
    y = x[:, 0].copy()
    t = targets.regression(x, y, lik, df=4.0, prior_scale=3.0, learn_scale=True, hyper_scale=2.0)
    z = np.zeros((3, p + 1))
    z[:, 0] = 1.0
    z[:, p] = (np.log(2.0), -3.0, 5.0)
    _, g = t.logdensity_and_grad(z)
    w = 2.0 * (z[:, p] - np.log(2.0))
    e = np.exp(-np.abs(w))
    lg = np.where(w >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    np.testing.assert_allclose(g[:, p], -M + (1.0 - 2.0 * lg), rtol=4e-16)
    assert g[0, p] == -M                  # w = 0: 1 - 2 / 2
    assert np.array_equal(g[:, 0], np.full(3, -1.0 / 9.0)) and np.all(g[:, 1:p] == 0.0)
