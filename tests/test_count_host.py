"""The count likelihoods of targets.regression and targets.multilevel_regression, host
side: argument checks, the parameter block's layout and length, the group sorting of
the offset, and the packer's constant.  No GPU.  (The C side's VB_EINVAL messages for a
bad phi and a wrong length need a context, so they are in tests/test_gpu_count.py.)"""
import math

import numpy as np
import pytest

from tests import count_cases as cc


def _data(D=3, M=9, lik='poisson_log'):
    return cc.make_data(D, M, lik, seed=1)


def test_regression_block_layout():
    from viabel_amd import targets
    x, y, off = _data()
    M, D = x.shape
    for lik, phi, lid in (('poisson_log', None, 3), ('neg_binomial_2_log', 2.5, 4)):
        t = targets.regression(x, y, lik, offset=off, phi=phi, prior_scale=3.0)
        p = t.params
        assert p.size == 8 + M * D + M + M + 1 and t.dim == D
        assert p[0] == lid and p[1] == M and p[3] == 0.0 and p[4] == 3.0
        assert p[2] == (phi or 0.0) and np.all(p[5:8] == 0.0)
        assert np.array_equal(p[8:8 + M * D].reshape(M, D), x)
        assert np.array_equal(p[8 + M * D:8 + M * D + M], y)
        assert np.array_equal(p[8 + M * D + M:8 + M * D + 2 * M], off)
        assert p[-1] == cc.count_constant(y, lik, phi)
        t0 = targets.regression(x, y, lik, phi=phi)
        assert np.all(t0.params[8 + M * D + M:-1] == 0.0)
    # the existing likelihoods keep their length
    assert targets.regression(x, y * 0.5, 'gaussian').params.size == 8 + M * D + M


def test_multilevel_block_layout_and_offset_sorting():
    from viabel_amd import targets
    p, G, M = 2, 4, 11
    x, y, group, off = cc.mlm_make_data(p, G, M, 'neg_binomial_2_log', seed=2)
    t = targets.multilevel_regression(x, y, group, 'neg_binomial_2_log', phi=0.7, offset=off,
                                      n_groups=G + 1)
    P, e = t.params, 8 + M * p + M + (G + 1) + 1
    assert P.size == e + M + 1 and t.dim == p + 1 + G + 1
    assert P[0] == 4 and P[2] == 0.7
    order = np.argsort(group, kind='stable')
    assert np.array_equal(t.order, order)
    assert np.array_equal(P[8:8 + M * p].reshape(M, p), x[order])
    assert np.array_equal(P[8 + M * p:8 + M * p + M], y[order])
    assert np.array_equal(P[e:e + M], off[order])
    assert P[-1] == cc.count_constant(y, 'neg_binomial_2_log', 0.7)
    t2 = targets.multilevel_poisson_regression(x, y, group)
    assert t2.params.size == 8 + M * p + M + G + 1 + M + 1 and t2.params[0] == 3
    assert np.all(t2.params[-1 - M:-1] == 0.0)
    assert t2.params[-1] == -math.fsum(math.lgamma(v + 1.0) for v in y)


@pytest.mark.parametrize('multilevel', [False, True])
def test_argument_errors(multilevel):
    from viabel_amd import targets
    x, y, off = _data()
    g = np.arange(x.shape[0]) % 3

    def make(yy, lik, **kw):
        if multilevel:
            return targets.multilevel_regression(x, yy, g, lik, **kw)
        return targets.regression(x, yy, lik, **kw)

    for lik, kw in (('poisson_log', {}), ('neg_binomial_2_log', dict(phi=2.0))):
        for bad in (-1.0, 0.5):
            yb = y.copy()
            yb[2] = bad
            with pytest.raises(ValueError, match='non-negative integer'):
                make(yb, lik, **kw)
        yb = y.copy()
        yb[0] = 2.0 ** 53 + 2
        with pytest.raises(ValueError, match='2\\^53'):
            make(yb, lik, **kw)
        yb[0] = 2.0 ** 53
        make(yb, lik, **kw)
        with pytest.raises(ValueError, match='offset must have shape'):
            make(y, lik, offset=off[:-1], **kw)
        with pytest.raises(ValueError, match='offset must have shape'):
            make(y, lik, offset=off[:, None], **kw)
        for bad in (np.nan, np.inf):
            ob = off.copy()
            ob[1] = bad
            with pytest.raises(ValueError, match='offset must be finite'):
                make(y, lik, offset=ob, **kw)
    for bad in (None, 0.0, -2.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='phi'):
            make(y, 'neg_binomial_2_log', phi=bad)
    with pytest.raises(ValueError, match='phi'):
        make(y, 'poisson_log', phi=2.0)
    yb = (y > 0).astype(float)
    for lik, kw in (('gaussian', {}), ('student_t', dict(df=4.0)), ('bernoulli_logit', {})):
        with pytest.raises(ValueError, match='offset'):
            make(yb, lik, offset=off, **kw)
        with pytest.raises(ValueError, match='phi'):
            make(yb, lik, phi=2.0, **kw)
    with pytest.raises(ValueError, match='likelihood'):
        make(y, 'poisson')


def test_wrappers():
    from viabel_amd import targets
    x, y, off = _data()
    g = np.arange(x.shape[0]) % 3
    a = targets.poisson_regression(x, y, offset=off, prior_scale=2.0)
    b = targets.regression(x, y, 'poisson_log', offset=off, prior_scale=2.0)
    assert np.array_equal(a.params, b.params) and a.likelihood == 'poisson_log'
    a = targets.negative_binomial_regression(x, y, 1.5)
    b = targets.regression(x, y, 'neg_binomial_2_log', phi=1.5)
    assert np.array_equal(a.params, b.params)
    a = targets.multilevel_poisson_regression(x, y, g, offset=off, centered=True)
    b = targets.multilevel_regression(x, y, g, 'poisson_log', offset=off, centered=True)
    assert np.array_equal(a.params, b.params)
    a = targets.multilevel_negative_binomial_regression(x, y, g, 1.5, offset=off)
    b = targets.multilevel_regression(x, y, g, 'neg_binomial_2_log', phi=1.5, offset=off)
    assert np.array_equal(a.params, b.params)
    with pytest.raises(TypeError):
        targets.negative_binomial_regression(x, y)


def test_restatement_gradient_is_the_derivative():
    """Central differences of the restatement's value, both likelihoods and targets."""
    x, y, off = _data(3, 12)
    g = np.arange(12) % 3
    for lik in cc.LIKELIHOODS:
        for f, D in ((cc.restatement(x, y, offset=off, **cc.model_kwargs(lik)), 3),
                     (cc.mlm_restatement(x, y, g, offset=off, **cc.mlm_model_kwargs(lik, False)), 7),
                     (cc.mlm_restatement(x, y, g, offset=off, **cc.mlm_model_kwargs(lik, True)), 7)):
            z = np.random.RandomState(5).randn(1, D) * 0.3
            _, gr = f(z)
            for d in range(D):
                h = np.zeros((1, D))
                h[0, d] = 1e-6
                num = (f(z + h)[0][0] - f(z - h)[0][0]) / 2e-6
                assert abs(num - gr[0, d]) <= 1e-6 * max(1.0, abs(gr[0, d]))
