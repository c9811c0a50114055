"""Multilevel regression target (targets.multilevel_regression), host side: argument
checks, the parameter block's layout, the ABI constant, the routes that refuse or pass
the new kind, and the numpy restatement of tests/mlm_cases.py against its own central
differences, against the regression restatement on the one-hot design and against the
hierarchical normal-means restatement.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from tests import glm_cases as gc
from tests import hier_cases as hc
from tests import mlm_cases as mc
from tests.conftest import ROOT


def _data(lik='gaussian', p=3, G=5, M=20, seed=1):
    return mc.make_data(p, G, M, lik, seed)


def test_argument_errors():
    from viabel_amd import targets
    x, y, g = _data()
    f = targets.multilevel_regression
    with pytest.raises(ValueError, match='unknown likelihood'):
        f(x, y, g, 'poisson')
    for bad in (x[0], x[:0], x[:, :0], x.reshape(20, 3, 1)):
        with pytest.raises(ValueError, match='non-empty'):
            f(bad, y, g)
    with pytest.raises(ValueError, match='y must have shape'):
        f(x, y[:-1], g)
    with pytest.raises(ValueError, match='group must have shape'):
        f(x, y, g[:-1])
    with pytest.raises(ValueError, match='group must have shape'):
        f(x, y, g.reshape(-1, 1))
    for v in (np.nan, np.inf, -np.inf):
        xb, yb = x.copy(), y.copy()
        xb[3, 1] = yb[2] = v
        with pytest.raises(ValueError, match='finite'):
            f(xb, y, g)
        with pytest.raises(ValueError, match='finite'):
            f(x, yb, g)
    # labels: negative, fractional, non-finite, not numbers, past n_groups
    gb = g.copy()
    gb[4] = -1
    with pytest.raises(ValueError, match='>= 0'):
        f(x, y, gb)
    gf = g.astype(float)
    gf[4] = 1.5
    with pytest.raises(ValueError, match='integer labels'):
        f(x, y, gf)
    gf[4] = np.nan
    with pytest.raises(ValueError, match='integer labels'):
        f(x, y, gf)
    with pytest.raises(ValueError, match='integer labels'):
        f(x, y, np.array(['a'] * 20))
    with pytest.raises(ValueError, match='not below n_groups'):
        f(x, y, g, n_groups=int(g.max()))
    for v in (0, -1, 2.5):
        with pytest.raises(ValueError, match='n_groups'):
            f(x, y, g, n_groups=v)
    for v in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='prior_scale'):
            f(x, y, g, prior_scale=v)
        with pytest.raises(ValueError, match='tau_scale'):
            f(x, y, g, tau_scale=v)
        with pytest.raises(ValueError, match='scale must be positive'):
            f(x, y, g, scale=v)
        with pytest.raises(ValueError, match='df > 0'):
            f(x, y, g, 'student_t', df=v)
    with pytest.raises(ValueError, match='df > 0'):
        f(x, y, g, 'student_t')
    with pytest.raises(ValueError, match=r'y in \{0, 1\}'):
        f(x, y, g, 'bernoulli_logit')
    # integral float labels are accepted
    assert f(x, y, g.astype(float)).n_groups == int(g.max()) + 1


def test_block_layout_and_stable_sort():
    from viabel_amd import targets, _native as nat
    rs = np.random.RandomState(3)
    # groups 0, 3 and 6 (first, middle, last) are empty
    g = np.array([5, 1, 2, 5, 1, 4, 2, 1, 5, 4, 1])
    M, p, G = g.size, 2, 7
    x, y = rs.randn(M, p), rs.randn(M)
    t = targets.multilevel_regression(x, y, g, 'student_t', df=4.0, scale=0.5, prior_scale=3.0,
                                      tau_scale=2.0, centered=True, n_groups=G)
    assert t.kind == nat.TARGET_MULTILEVEL == 8
    assert t.dim == p + 1 + G and t.name == 'multilevel_regression' and not t.separable
    assert t.n_groups == G and t.n_obs == M and t.centered is True and t.likelihood == 'student_t'
    np.testing.assert_array_equal(t.order, np.argsort(g, kind='stable'))
    np.testing.assert_array_equal(t.order, [1, 4, 7, 10, 2, 6, 5, 9, 0, 3, 8])
    pr = t.params
    assert pr.dtype == np.float64 and pr.flags['C_CONTIGUOUS']
    assert targets.MULTILEVEL_HEADER == 8
    assert pr.size == 8 + M * p + M + G + 1
    np.testing.assert_array_equal(pr[:8], [1.0, M, 4.0, 0.5, 3.0, G, 2.0, 1.0])
    np.testing.assert_array_equal(pr[8:8 + M * p].reshape(M, p), x[t.order])
    np.testing.assert_array_equal(pr[8 + M * p:8 + M * p + M], y[t.order])
    np.testing.assert_array_equal(pr[8 + M * p + M:], [0, 0, 4, 6, 6, 8, 11, 11])
    s1 = t._struct()
    assert s1.n_params == pr.size and s1.dim == p + 1 + G and s1.kind == 8
    # defaults: gaussian, non-centred, G from the labels
    d = targets.multilevel_regression(x, y, g)
    assert d.likelihood == 'gaussian' and d.centered is False and d.n_groups == 6
    np.testing.assert_array_equal(d.params[:8], [0.0, M, 0.0, 1.0, 10.0, 6, 5.0, 0.0])
    # the logit link stores neither df nor scale
    b = targets.multilevel_regression(x, (y > 0).astype(float), g, 'bernoulli_logit')
    np.testing.assert_array_equal(b.params[:8], [2.0, M, 0.0, 0.0, 10.0, 6, 5.0, 0.0])


def test_conveniences_and_exports():
    from viabel_amd import targets
    x, y, g = _data('bernoulli_logit')
    a = targets.multilevel_logistic_regression(x, y, g, prior_scale=2.0, tau_scale=1.5, centered=True)
    b = targets.multilevel_regression(x, y, g, 'bernoulli_logit', prior_scale=2.0, tau_scale=1.5,
                                      centered=True)
    np.testing.assert_array_equal(a.params, b.params)
    x, y, g = _data('student_t')
    a = targets.multilevel_robust_regression(x, y, g, 7.0, scale=0.3, n_groups=9)
    b = targets.multilevel_regression(x, y, g, 'student_t', df=7.0, scale=0.3, n_groups=9)
    np.testing.assert_array_equal(a.params, b.params)
    assert a.dim == 3 + 1 + 9
    for name in ('multilevel_regression', 'multilevel_logistic_regression',
                 'multilevel_robust_regression'):
        assert name in targets.__all__ and name in targets.__doc__
        assert callable(getattr(targets, name))
    assert targets.as_target(a, a.dim) is a


def test_header_declares_the_kind():
    from viabel_amd import _native as nat
    h = open(os.path.join(ROOT, 'include', 'viabel_amd.h')).read()
    m = re.search(r'VB_TARGET_MULTILEVEL\s*=\s*(\d+)', h)
    assert m and int(m.group(1)) == 8 == nat.TARGET_MULTILEVEL
    assert re.search(r'#define VB_ABI_VERSION 1\b', h)


def test_rows_kernel_not_used():
    from viabel_amd import targets, vb
    from viabel_amd.restarts import _rows_supported
    x, y, g = _data()
    t = targets.multilevel_regression(x, y, g)
    fam = vb.mean_field_t_variational_family(t.dim, 40.0, rng='philox')
    assert t.dim <= 16 and not _rows_supported(fam, t)
    assert _rows_supported(vb.mean_field_t_variational_family(10, 40.0, rng='philox'),
                           targets.eight_schools_ncp())


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('lik', mc.LIKELIHOODS)
def test_restatement_gradient_matches_central_differences(lik, centered):
    p, G, M = 2, 4, 15
    x, y, g = mc.make_data(p, G, M, lik, 5)
    f = mc.restatement(x, y, g, n_groups=G, **mc.model_kwargs(lik, centered))
    D = p + 1 + G
    z = mc.rows(5, D, p, 6)
    lp, gr = f(z)
    assert lp.shape == (5,) and gr.shape == (5, D)
    h = 1e-5
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd = (f(z + e)[0] - f(z - e)[0]) / (2 * h)
        # central differences: O(h^2) truncation + rounding of |log p| ~ 1e2 over 2h
        np.testing.assert_allclose(gr[:, d], fd, rtol=1e-6, atol=2e-7)


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('lik', mc.LIKELIHOODS)
def test_restatement_is_the_regression_on_the_one_hot_design(lik, centered):
    """log p of the regression restatement (tests/glm_cases.py) on X' = [x | onehot(group)]
    at [beta | a], its N(0, s^2) prior on the intercept columns exchanged by hand for the
    groups' prior, tau's prior and the Jacobian; the gradient in beta and in the
    intercepts by the chain rule."""
    p, G, M = 3, 6, 40
    x, y, g = mc.make_data(p, G, M, lik, 8)
    kw = mc.model_kwargs(lik, centered)
    f = mc.restatement(x, y, g, n_groups=G, **kw)
    s, st = kw['prior_scale'], kw['tau_scale']
    onehot = np.zeros((M, G))
    onehot[np.arange(M), g] = 1.0
    glm = gc.restatement(np.concatenate([x, onehot], axis=1), y,
                         **{k: v for k, v in kw.items() if k not in ('tau_scale', 'centered')})
    z = mc.rows(9, p + 1 + G, p, 9)
    beta, u, a = z[:, :p], z[:, p], z[:, p + 1:]
    tau = np.exp(u)
    aeff = a if centered else tau[:, None] * a
    lp0, g0 = glm(np.concatenate([beta, aeff], axis=1))
    # take the regression's prior on the intercept columns out again
    c_s = 0.5 * math.log(2 * math.pi) + math.log(s)
    lp0 = lp0 + np.sum(0.5 * (aeff / s) ** 2, axis=1) + G * c_s
    S = g0[:, p:] + aeff / s ** 2
    w = (tau / st) ** 2
    lp0 = lp0 + math.log(2 / (math.pi * st)) - np.log1p(w) + u - G * 0.5 * math.log(2 * math.pi)
    if centered:
        lp0 = lp0 - G * u - 0.5 * np.sum((a / tau[:, None]) ** 2, axis=1)
        ga = S - a / tau[:, None] ** 2
        gu = 1 - 2 * w / (1 + w) + np.sum((a / tau[:, None]) ** 2, axis=1) - G
    else:
        lp0 = lp0 - 0.5 * np.sum(a * a, axis=1)
        ga = tau[:, None] * S - a
        gu = 1 - 2 * w / (1 + w) + tau * np.sum(S * a, axis=1)
    lp, gr = f(z)
    np.testing.assert_allclose(lp, lp0, rtol=1e-12)
    np.testing.assert_allclose(gr[:, :p], g0[:, :p], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(gr[:, p], gu, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(gr[:, p + 1:], ga, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize('centered', mc.FORMS)
def test_reduces_to_hierarchical_normal_means(centered):
    """p = 1, x = 0, the gaussian link and one observation per group: the hierarchical
    normal-means restatement (tests/hier_cases.py) with sigma_j = scale at mu = 0, plus the
    constants that one drops (Stan's convention) and the beta prior; the gradients in
    log tau and in the group coordinates are equal."""
    J, scale, s, st = 6, 1.3, 3.0, 2.0
    y, _ = hc.make_data(J, 4)
    f = mc.restatement(np.zeros((J, 1)), y, np.arange(J), 'gaussian', scale=scale, prior_scale=s,
                       tau_scale=st, centered=centered)
    h = hc.restatement(y, np.full(J, scale), centered, mu_scale=5.0, tau_scale=st)
    rs = np.random.RandomState(10)
    z = rs.randn(7, 1 + 1 + J)
    zh = np.concatenate([np.zeros((7, 1)), z[:, 1:]], axis=1)          # mu = 0
    lp, g = f(z)
    lph, gh = h(zh)
    half = 0.5 * math.log(2 * math.pi)
    const = (-half - math.log(s)) + math.log(2 / (math.pi * st)) - J * half \
        + J * (-half - math.log(scale))
    np.testing.assert_allclose(lp, lph - 0.5 * (z[:, 0] / s) ** 2 + const, rtol=1e-13)
    np.testing.assert_allclose(g[:, 0], -z[:, 0] / s ** 2, rtol=1e-13)
    np.testing.assert_allclose(g[:, 1:], gh[:, 1:], rtol=1e-12, atol=1e-13)
