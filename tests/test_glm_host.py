"""Regression targets (targets.regression), host side: argument checks, the
parameter block's layout, the ABI constant, and the numpy restatement
(tests/glm_cases.py) that the device tests compare against.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import glm_cases as gc
from tests import notebook_cases as nc
from tests.conftest import ROOT


def _data(D=3, M=7, lik='student_t'):
    return gc.make_data(D, M, lik, seed=1)


def test_argument_errors():
    from viabel_amd import targets
    x, y = _data()
    with pytest.raises(ValueError, match='likelihood'):
        targets.regression(x, y, 'poisson')
    with pytest.raises(ValueError, match='shape'):
        targets.regression(x, y[:-1], 'gaussian')
    with pytest.raises(ValueError, match='shape'):
        targets.regression(x[:, 0], y, 'gaussian')
    bad = x.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match='finite'):
        targets.regression(bad, y, 'gaussian')
    ybad = y.copy()
    ybad[0] = np.inf
    with pytest.raises(ValueError, match='finite'):
        targets.regression(x, ybad, 'gaussian')
    with pytest.raises(ValueError, match='df'):
        targets.regression(x, y, 'student_t')
    with pytest.raises(ValueError, match='df'):
        targets.regression(x, y, 'student_t', df=0.0)
    with pytest.raises(ValueError, match='df'):
        targets.robust_regression(x, y, -1.0)
    with pytest.raises(ValueError, match='scale'):
        targets.regression(x, y, 'gaussian', scale=0.0)
    with pytest.raises(ValueError, match='scale'):
        targets.robust_regression(x, y, 4.0, scale=-2.0)
    with pytest.raises(ValueError, match='prior_scale'):
        targets.regression(x, y, 'gaussian', prior_scale=0.0)
    with pytest.raises(ValueError, match='prior_scale'):
        targets.logistic_regression(x, (y > 0).astype(float), prior_scale=-1.0)
    with pytest.raises(ValueError, match=r'\{0, 1\}'):
        targets.logistic_regression(x, y)


@pytest.mark.parametrize('lik', gc.LIKELIHOODS)
def test_parameter_layout(lik):
    from viabel_amd import targets, _native as nat
    D, M = 3, 7
    x, y = _data(D, M, lik)
    kw = gc.model_kwargs(lik, df=6.0, scale=0.5, prior_scale=2.5)
    t = targets.regression(x, y, **kw)
    assert t.kind == nat.TARGET_REGRESSION == 6
    assert t.dim == D and not t.separable
    p = t.params
    assert p.dtype == np.float64 and p.flags['C_CONTIGUOUS']
    assert p.size == 8 + M * D + M
    assert p[0] == gc.LIKELIHOODS.index(lik) and p[1] == M
    assert p[2] == (6.0 if lik == 'student_t' else 0.0)
    assert p[3] == (0.5 if lik != 'bernoulli_logit' else 0.0)
    assert p[4] == 2.5
    assert np.all(p[5:8] == 0.0)
    np.testing.assert_array_equal(p[8:8 + M * D].reshape(M, D), x)
    np.testing.assert_array_equal(p[8 + M * D:], y)
    # one array for the target's lifetime: the descriptor points into it every time
    s1, s2 = t._struct(), t._struct()
    assert t.params is p and s1.n_params == s2.n_params == p.size
    assert nat.as_f64(t.params) is t.params


def test_conveniences_and_exports():
    from viabel_amd import targets
    x, y = _data()
    a = targets.robust_regression(x, y, 40.0)
    b = targets.regression(x, y, 'student_t', df=40.0, scale=1.0, prior_scale=10.0)
    np.testing.assert_array_equal(a.params, b.params)
    yb = (y > 0).astype(float)
    np.testing.assert_array_equal(targets.logistic_regression(x, yb).params,
                                  targets.regression(x, yb, 'bernoulli_logit').params)
    for name in ('regression', 'robust_regression', 'logistic_regression'):
        assert name in targets.__all__ and name in targets.__doc__


def test_header_declares_the_kind():
    from viabel_amd import _native as nat
    h = open(os.path.join(ROOT, 'include', 'viabel_amd.h')).read()
    m = re.search(r'VB_TARGET_REGRESSION\s*=\s*(\d+)', h)
    assert m and int(m.group(1)) == 6 == nat.TARGET_REGRESSION
    assert re.search(r'#define VB_ABI_VERSION 1\b', h)


def test_rows_kernel_not_used():
    from viabel_amd import targets, vb
    from viabel_amd.restarts import _rows_supported
    x, y = _data(2, 5)
    fam = vb.mean_field_t_variational_family(2, 40.0, rng='philox')
    assert _rows_supported(fam, targets.funnel(2))
    assert not _rows_supported(fam, targets.robust_regression(x, y, 40.0))


@pytest.mark.parametrize('lik', gc.LIKELIHOODS)
def test_restatement_gradient_matches_central_differences(lik):
    D, M = 4, 30
    x, y = gc.make_data(D, M, lik, seed=2)
    f = gc.restatement(x, y, **gc.model_kwargs(lik))
    b = np.random.RandomState(3).randn(5, D)
    lp, g = f(b)
    assert lp.shape == (5,) and g.shape == (5, D)
    h = 1e-5
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd = (f(b + e)[0] - f(b - e)[0]) / (2 * h)
        # central differences: O(h^2) truncation + rounding of |log p| ~ 1e2 over 2h
        np.testing.assert_allclose(g[:, d], fd, rtol=1e-6, atol=1e-7)


def test_restatement_matches_the_notebook_model_up_to_a_constant():
    x, y = nc.robust_regression_data()
    f = gc.restatement(x, y, 'student_t', df=40.0, scale=1.0, prior_scale=10.0)
    ref = nc.robust_regression_target()
    b = np.random.RandomState(4).randn(50, 2) * 2.0
    lp, g = f(b)
    lp0, g0 = ref(b)
    shift = lp - lp0
    assert abs(shift[0]) > 1.0          # Stan drops the constants this target keeps
    np.testing.assert_allclose(shift, shift[0], rtol=0, atol=1e-11 * abs(shift[0]) + 1e-11)
    np.testing.assert_allclose(g, g0, rtol=1e-13, atol=1e-13)
