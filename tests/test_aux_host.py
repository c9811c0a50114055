"""targets.regression with a learned scale (learn_scale) or dispersion (learn_phi), host
side: the target's dimension and attributes, the parameter block's layout (fields 5 and 6,
the zeroed sigma / phi, J and T against a brute-force count, the reduced c_data), every
refused combination and the cap on max y, and the wrappers' old calls, whose blocks must
stay byte for byte what they were.  No GPU and no library call.  (The C side's refusals
need a context, so they are in tests/test_gpu_aux.py.)"""
import math

import numpy as np
import pytest

from tests import aux_cases as ac
from tests import count_cases as cc
from tests import glm_cases as gc


def _located(p=3, M=9):
    return gc.make_data(p, M, 'gaussian', seed=1)


def _counts(p=3, M=9):
    return cc.make_data(p, M, 'neg_binomial_2_log', seed=1)


@pytest.mark.parametrize('lik,df,lid', [('gaussian', None, 0), ('student_t', 4.0, 1)])
def test_learned_scale_block(lik, df, lid):
    from viabel_amd import targets
    x, y = _located()
    M, p = x.shape
    t = targets.regression(x, y, lik, df=df, scale=123.0, prior_scale=3.0, learn_scale=True,
                           hyper_scale=2.5)
    assert t.dim == p + 1 and t.n_coef == p and t.learned == 'scale' and t.n_obs == M
    P = t.params
    assert P.size == 8 + M * p + M
    assert P[0] == lid and P[1] == M and P[2] == (df or 0.0) and P[4] == 3.0
    assert P[3] == 0.0                      # the scale argument is not used
    assert P[5] == 1.0 and P[6] == 2.5 and P[7] == 0.0
    assert np.array_equal(P[8:8 + M * p].reshape(M, p), x)
    assert np.array_equal(P[8 + M * p:], y)
    # a fixed target keeps fields 5..7 zero and its dimension
    t0 = targets.regression(x, y, lik, df=df, scale=0.5)
    assert t0.dim == p and np.all(t0.params[5:8] == 0.0) and not hasattr(t0, 'learned')
    assert 'last' in targets.regression.__doc__ and 'log' in targets.regression.__doc__


@pytest.mark.parametrize('kind', ['plain', 'zero', 'binary', 'big'])
def test_learned_dispersion_block(kind):
    from viabel_amd import targets
    x, y, off = _counts(3, 40)
    if kind == 'zero':
        y = np.zeros_like(y)
    elif kind == 'binary':
        y = np.minimum(y, 1.0)
        y[0] = 1.0
    elif kind == 'big':
        y[7] = 65536.0
    M, p = x.shape
    t = targets.regression(x, y, 'neg_binomial_2_log', offset=off, prior_scale=3.0,
                           learn_phi=True, hyper_scale=0.5)
    J = int(y.max())
    assert J == {'zero': 0, 'binary': 1, 'big': 65536}.get(kind, J)
    assert t.dim == p + 1 and t.n_coef == p and t.learned == 'phi'
    P = t.params
    e = 8 + M * p + 2 * M
    assert P.size == e + 1 + 1 + J
    assert P[0] == 4 and P[1] == M and P[2] == 0.0 and P[3] == 0.0 and P[4] == 3.0
    assert P[5] == 1.0 and P[6] == 0.5 and P[7] == 0.0
    assert np.array_equal(P[8:8 + M * p].reshape(M, p), x)
    assert np.array_equal(P[8 + M * p:8 + M * p + M], y)
    assert np.array_equal(P[8 + M * p + M:e], off)
    T, c_data = ac.dispersion_table(y)      # brute force: T[j] = #{m : y_m > j}
    assert P[e] == c_data == math.fsum(-math.lgamma(v + 1.0) for v in y)
    assert P[e + 1] == J
    assert np.array_equal(P[e + 2:], T)
    # the helper beside count_constant, and count_constant itself unchanged
    T2, c2 = targets.dispersion_table(y)
    assert np.array_equal(T2, T) and c2 == c_data
    if kind != 'big':
        assert targets.count_constant(y, 2.5) == cc.count_constant(y, 'neg_binomial_2_log', 2.5)
        # sum_j T_j log1p(j / phi) is the part of the fixed-phi constant that moved out
        A = math.fsum((T * np.log1p(np.arange(J) / 2.5)).tolist())
        assert abs((c_data + A) - targets.count_constant(y, 2.5)) <= 1e-12 * max(1.0, abs(c_data))


def test_refused_combinations():
    from viabel_amd import targets
    x, y = _located()
    xc, yc, off = _counts()
    yb = (y > 0).astype(float)
    for lik, yy, kw in (('bernoulli_logit', yb, {}), ('poisson_log', yc, {}),
                        ('neg_binomial_2_log', yc, dict(phi=2.0))):
        with pytest.raises(ValueError, match='learn_scale.*gaussian and student_t'):
            targets.regression(x, yy, lik, learn_scale=True, **kw)
    for lik, yy, kw in (('gaussian', y, {}), ('student_t', y, dict(df=4.0)),
                        ('bernoulli_logit', yb, {}), ('poisson_log', yc, {})):
        with pytest.raises(ValueError, match='learn_phi.*neg_binomial_2_log'):
            targets.regression(x, yy, lik, learn_phi=True, **kw)
    with pytest.raises(ValueError, match='phi must be None'):
        targets.regression(xc, yc, 'neg_binomial_2_log', phi=2.0, learn_phi=True)
    with pytest.raises(ValueError, match='phi must be None'):
        targets.negative_binomial_regression(xc, yc, 2.0, learn_phi=True)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='hyper_scale'):
            targets.regression(x, y, 'gaussian', learn_scale=True, hyper_scale=bad)
        with pytest.raises(ValueError, match='hyper_scale'):
            targets.regression(xc, yc, 'neg_binomial_2_log', learn_phi=True, hyper_scale=bad)
    with pytest.raises(ValueError, match='df > 0'):
        targets.regression(x, y, 'student_t', learn_scale=True)
    # an unused scale is not checked; a used one still is
    targets.regression(x, y, 'gaussian', scale=-1.0, learn_scale=True)
    with pytest.raises(ValueError, match='scale must be positive'):
        targets.regression(x, y, 'gaussian', scale=-1.0)
    with pytest.raises(ValueError, match='phi'):
        targets.regression(xc, yc, 'neg_binomial_2_log')


def test_max_y_cap_names_the_fixed_phi_target():
    from viabel_amd import targets
    x, y, off = _counts()
    y[3] = 65536.0
    targets.regression(x, y, 'neg_binomial_2_log', learn_phi=True)
    y[3] = 65537.0
    with pytest.raises(ValueError, match=r'65536.*fixed-phi.*negative_binomial_regression\(x, y, phi\)'):
        targets.regression(x, y, 'neg_binomial_2_log', learn_phi=True)
    targets.regression(x, y, 'neg_binomial_2_log', phi=2.0)      # the fixed target takes it


def test_wrappers():
    from viabel_amd import targets
    x, y = _located()
    xc, yc, off = _counts()
    a = targets.linear_regression(x, y)
    b = targets.regression(x, y, 'gaussian', prior_scale=10.0, learn_scale=True, hyper_scale=5.0)
    assert np.array_equal(a.params, b.params) and a.dim == x.shape[1] + 1
    a = targets.linear_regression(x, y, 2.0, 0.5)
    assert a.params[4] == 2.0 and a.params[6] == 0.5
    a = targets.robust_regression(x, y, 4.0, learn_scale=True, hyper_scale=2.0)
    b = targets.regression(x, y, 'student_t', df=4.0, learn_scale=True, hyper_scale=2.0)
    assert np.array_equal(a.params, b.params) and a.learned == 'scale'
    a = targets.negative_binomial_regression(xc, yc, learn_phi=True, offset=off, hyper_scale=2.0)
    b = targets.regression(xc, yc, 'neg_binomial_2_log', offset=off, learn_phi=True, hyper_scale=2.0)
    assert np.array_equal(a.params, b.params) and a.learned == 'phi'
    for t in (targets.linear_regression, targets.robust_regression,
              targets.negative_binomial_regression):
        assert 'last' in t.__doc__ and 'log' in t.__doc__


def test_old_positional_calls_give_the_old_blocks():
    """The blocks of the calls that existed before, rebuilt here field by field as the
    packer wrote them then."""
    from viabel_amd import targets
    x, y = _located()
    xc, yc, off = _counts()
    M, p = x.shape

    def old(lid, p2, p3, prior, xx, yy, tail=()):
        return np.concatenate([[lid, M, p2, p3, prior, 0.0, 0.0, 0.0], xx.ravel(), yy, *tail])

    t = targets.robust_regression(x, y, 4.0, 0.7, 3.0)
    assert t.params.tobytes() == old(1, 4.0, 0.7, 3.0, x, y).tobytes() and t.dim == p
    t = targets.robust_regression(x, y, 40.0)
    assert t.params.tobytes() == old(1, 40.0, 1.0, 10.0, x, y).tobytes()
    t = targets.negative_binomial_regression(xc, yc, 2.5, off, 3.0)
    c = cc.count_constant(yc, 'neg_binomial_2_log', 2.5)
    assert t.params.tobytes() == old(4, 2.5, 0.0, 3.0, xc, yc, (off, [c])).tobytes() and t.dim == p
    t = targets.regression(x, y, 'gaussian', None, 0.5, 2.0)
    assert t.params.tobytes() == old(0, 0.0, 0.5, 2.0, x, y).tobytes()
    t = targets.regression(xc, yc, 'neg_binomial_2_log', None, 1.0, 2.0, off, 1.5)
    c = cc.count_constant(yc, 'neg_binomial_2_log', 1.5)
    assert t.params.tobytes() == old(4, 1.5, 0.0, 2.0, xc, yc, (off, [c])).tobytes()
    with pytest.raises(TypeError):
        targets.negative_binomial_regression(xc, yc)


def test_restatement_takes_the_table_the_packer_builds():
    """The numpy restatement's table sums equal the per-observation sums they replace."""
    x, y, off = _counts(2, 30)
    phi = 1.7
    T, _ = ac.dispersion_table(y)
    js = np.arange(T.size)
    A = float(np.sum(T * np.log1p(js / phi)))
    brute = sum(math.log1p(j / phi) for v in y for j in range(int(v)))
    assert abs(A - brute) <= 1e-12 * max(1.0, brute)
    dA = float(np.sum(T * js / (phi + js)))
    brute = sum(j / (phi + j) for v in y for j in range(int(v)))
    assert abs(dA - brute) <= 1e-12 * max(1.0, brute)
