"""The learned instances of the multilevel kernels (viabel_amd/csrc/vb_mlm.hip, LIK = 5, 6,
7: a learned sigma for gaussian and student_t, a learned phi for neg_binomial_2_log) at the
edge data and rows of tests/mlm_aux_mp.py, both forms and every shape (the lane-per-row
kernel's four instances, the tile kernel, groups split across chunks, empty groups), against
the 50-digit reference written from the literal densities, the lambda gradient by mp.diff:
vb_target_logdensity's value and every gradient entry within MARGIN = 8 x
MLM_AUX_ORACLE_ERR in units of 2^-53 S, the project's standing margin of the device kernels
over the numpy restatement (fused operations, a different sum order).  The value-only
instances give the with-gradient bits, two calls give the same bits, and at lambda -
log s_aux = +-400 and u = +-400 log p has no NaN and is -inf only where the restatement is.

Measured worst errors on MI355X are in DESIGN.md §7d.
"""
import numpy as np
import pytest

from tests import mlm_aux_cases as mac
from tests import mlm_aux_mp as mam
from tests.conftest import gpu_available
from tests.test_gpu_mlm import _value_only

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not mam.available(), reason='needs mpmath')]

MARGIN = 8.0


def _target(c, G):
    from viabel_amd import targets
    return targets.multilevel_regression(c.x, c.y, c.group, n_groups=G, offset=c.offset,
                                         **mac.target_kwargs(c.kw))


def _instance(lik, p):
    lid = {'gaussian': 5, 'student_t': 6, 'neg_binomial_2_log': 7}[lik]
    return 'tile LIK=%d' % lid if p > 16 else 'lane LIK=%d PP=%d' % (lid, 2 if p <= 2 else 4 if p <= 4
                                                                     else 8 if p <= 8 else 16)


def _check(tag, key, c, lp, g, ref):
    lik, centered, p = key[0], key[1], key[2]
    bound = MARGIN * mam.MLM_AUX_ORACLE_ERR[centered]
    e_lp, e_g = mam.errors(lp, np.zeros_like(ref.g_hi) if g is None else g, ref)
    r = int(np.argmax(e_lp))
    msg = 'MLM AUX EDGE %s [%s] %r: value %.3f (row %d)' % (tag, _instance(lik, p), key, e_lp[r], r)
    if g is not None:
        gr, gc = np.unravel_index(int(np.argmax(e_g[:, :-1])), e_g[:, :-1].shape)
        lr = int(np.argmax(e_g[:, -1]))
        msg += ', beta / u / group %.3f (row %d, column %d), lambda %.3f (row %d)' % (
            e_g[gr, gc], gr, gc, e_g[lr, -1], lr)
    print(msg + '; bound %.2f x 2^-53 S' % bound)
    assert e_lp[r] <= bound
    if g is not None:
        assert e_g[gr, gc] <= bound
        assert e_g[lr, -1] <= bound


@pytest.mark.parametrize('lik,centered,p,G,M', mam.cases())
def test_value_and_gradient(lik, centered, p, G, M):
    """Every new instance with GRAD = true and, beside it, GRAD = false: the same value
    bits; and a second call: the same bits."""
    key = (lik, centered, p, G, M)
    c, ref = mam.edge_reference(*key)
    t = _target(c, G)
    z = np.array(c.z)
    lp, g = t.logdensity_and_grad(z)
    assert lp.shape == (z.shape[0],) and g.shape == z.shape
    _check('grad', key, c, lp, g, ref)
    lp_v = _value_only(t, z)
    _check('value-only', key, c, lp_v, None, ref)
    assert np.array_equal(lp_v, lp)
    lp2, g2 = t.logdensity_and_grad(z)
    assert np.array_equal(lp, lp2) and np.array_equal(g, g2)


@pytest.mark.parametrize('lik,centered,p,G,M,kind', mam.table_cases())
def test_dispersion_tables(lik, centered, p, G, M, kind):
    """J = 0 (no table), J = 1 (an empty sum) and J = 65536."""
    key = (lik, centered, p, G, M, kind)
    c, ref = mam.edge_reference(*key)
    t = _target(c, G)
    assert t.params[8 + M * p + 2 * M + G + 1 + 2] == {'zero': 0, 'binary': 1, 'big': 65536}[kind]
    z = np.array(c.z)
    lp, g = t.logdensity_and_grad(z)
    _check('table', key, c, lp, g, ref)
    lp2, g2 = t.logdensity_and_grad(z)
    assert np.array_equal(lp, lp2) and np.array_equal(g, g2)
    assert np.array_equal(_value_only(t, z), lp)


@pytest.mark.parametrize('centered', mac.FORMS)
@pytest.mark.parametrize('lik', mac.LIKELIHOODS)
@pytest.mark.parametrize('p,G,M', [(3, 8, 129), (17, 3, 65)])
def test_rows_at_plus_minus_400(p, G, M, lik, centered):
    """lambda - log s_aux = +-400 and u = +-400, the other coordinates standard normal: no
    NaN in log p, and -inf only where the restatement also leaves the double range."""
    c = mam.edge_case(lik, centered, p, G, M)
    t = _target(c, G)
    f = mac.restatement(c.x, c.y, c.group, offset=c.offset, n_groups=G, **c.kw)
    z = np.concatenate([mam.far_rows(c, p, G, seed=s) for s in range(5)])
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
