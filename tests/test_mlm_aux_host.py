"""The packer of the multilevel target with a learned scale or dispersion
(targets.multilevel_regression(..., learn_scale=True) / (..., learn_phi=True)): the layout
of the learned block documented in include/viabel_amd.h, the argument errors, the wrappers,
and that a call without the new arguments packs the bytes of the fixed layout.  No GPU."""
import numpy as np
import pytest

from tests import mlm_aux_cases as mac
from tests import mlm_cases as mc
from viabel_amd import targets

P, G, M = 3, 5, 40


def _data(lik, seed=1):
    return mac.make_data(P, G, M, lik, seed=seed)


@pytest.mark.parametrize('centered', mac.FORMS)
@pytest.mark.parametrize('lik', mac.LIKELIHOODS)
def test_learned_block_layout(lik, centered):
    x, y, g, off = _data(lik)
    kw = mac.model_kwargs(lik, centered)
    t = targets.multilevel_regression(x, y, g, n_groups=G, offset=off, **mac.target_kwargs(kw))
    pr = t.params
    nb = lik == 'neg_binomial_2_log'
    assert t.dim == P + 2 + G
    assert t.learned == ('phi' if nb else 'scale')
    assert t.n_coef == P and t.n_groups == G and t.n_obs == M and t.centered == centered
    assert t.likelihood == lik and np.array_equal(np.sort(t.order), np.arange(M))
    assert pr[0] == {'gaussian': 0, 'student_t': 1, 'neg_binomial_2_log': 4}[lik]
    assert pr[1] == M and pr[4] == kw['prior_scale'] and pr[5] == G and pr[6] == kw['tau_scale']
    assert pr[7] == (1.0 if centered else 0.0) + 2.0
    # the vacated constant is zero; nu stays
    assert pr[2] == (kw['df'] if lik == 'student_t' else 0.0)
    assert pr[3] == 0.0
    o = t.order
    e = 8 + M * P
    assert np.array_equal(pr[8:e].reshape(M, P), x[o])
    assert np.array_equal(pr[e:e + M], y[o])
    offsets = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=G))])
    assert np.array_equal(pr[e + M:e + M + G + 1], offsets)
    e += M + G + 1
    if nb:
        T, c_data = targets.dispersion_table(y)
        assert np.array_equal(pr[e:e + M], off[o])
        assert pr[e + M] == c_data
        assert pr[e + M + 1] == kw['hyper_scale']
        assert pr[e + M + 2] == T.size
        assert np.array_equal(pr[e + M + 3:], T)
        assert pr.size == 8 + M * P + 2 * M + G + 1 + 1 + 1 + 1 + T.size
    else:
        assert pr[e] == kw['hyper_scale']
        assert pr.size == 8 + M * P + M + G + 1 + 1


def test_argument_errors():
    x, y, g, _ = _data('gaussian')
    xc, yc, gc_, off = _data('neg_binomial_2_log')
    f = targets.multilevel_regression
    for lik in ('bernoulli_logit', 'poisson_log', 'neg_binomial_2_log'):
        with pytest.raises(ValueError, match='learn_scale=True is valid for the gaussian and student_t'):
            f(x, y, g, lik, learn_scale=True)
    for lik in ('gaussian', 'student_t', 'bernoulli_logit', 'poisson_log'):
        with pytest.raises(ValueError, match='learn_phi=True is valid for the neg_binomial_2_log'):
            f(x, y, g, lik, df=4.0, learn_phi=True)
    with pytest.raises(ValueError, match='phi must be None'):
        f(xc, yc, gc_, 'neg_binomial_2_log', phi=2.0, learn_phi=True)
    with pytest.raises(ValueError, match='needs a finite phi > 0'):
        f(xc, yc, gc_, 'neg_binomial_2_log')
    for hs in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='hyper_scale must be positive'):
            f(x, y, g, 'gaussian', learn_scale=True, hyper_scale=hs)
    big = yc.copy()
    big[0] = targets.DISPERSION_TABLE_MAX + 1
    with pytest.raises(ValueError, match='learn_phi=True needs max'):
        f(xc, big, gc_, 'neg_binomial_2_log', learn_phi=True)
    big[0] = targets.DISPERSION_TABLE_MAX
    assert f(xc, big, gc_, 'neg_binomial_2_log', learn_phi=True).params[-1] == 1.0   # T[J - 1]
    # scale is not looked at when it is learned
    assert f(x, y, g, 'gaussian', scale=-1.0, learn_scale=True).learned == 'scale'
    with pytest.raises(ValueError, match='scale must be positive'):
        f(x, y, g, 'gaussian', scale=-1.0)
    with pytest.raises(TypeError, match='needs phi, or learn_phi=True'):
        targets.multilevel_negative_binomial_regression(xc, yc, gc_)


def test_wrappers():
    x, y, g, _ = _data('gaussian')
    t = targets.multilevel_linear_regression(x, y, g, prior_scale=2.0, tau_scale=3.0, hyper_scale=4.0,
                                             centered=True, n_groups=G + 1)
    t0 = targets.multilevel_regression(x, y, g, 'gaussian', prior_scale=2.0, tau_scale=3.0,
                                       centered=True, n_groups=G + 1, learn_scale=True,
                                       hyper_scale=4.0)
    assert t.dim == P + 2 + G + 1 and t.learned == 'scale' and np.array_equal(t.params, t0.params)
    assert t.params[7] == 3.0 and t.params[-1] == 4.0
    t = targets.multilevel_robust_regression(x, y, g, 4.0, learn_scale=True, hyper_scale=1.5)
    assert t.learned == 'scale' and t.params[0] == 1 and t.params[2] == 4.0 and t.params[-1] == 1.5
    xc, yc, gc_, off = _data('neg_binomial_2_log')
    t = targets.multilevel_negative_binomial_regression(xc, yc, gc_, offset=off, learn_phi=True)
    assert t.learned == 'phi' and t.params[2] == 0.0 and t.params[7] == 2.0
    t = targets.multilevel_negative_binomial_regression(xc, yc, gc_, 2.5, offset=off)
    assert not hasattr(t, 'learned') and t.params[2] == 2.5 and t.params[7] == 0.0


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('lik', ['gaussian', 'student_t', 'bernoulli_logit', 'poisson_log',
                                 'neg_binomial_2_log'])
def test_fixed_blocks_keep_their_bytes(lik, centered):
    """A call without the new arguments: the block assembled here from the documented fixed
    layout [header | X | y | off | (eta0, c_data)], byte for byte."""
    from tests import count_cases as cc
    count = lik in ('poisson_log', 'neg_binomial_2_log')
    if count:
        x, y, g, off = cc.mlm_make_data(P, G, M, lik, seed=2)
        kw = cc.mlm_model_kwargs(lik, centered)
        t = targets.multilevel_regression(x, y, g, n_groups=G, offset=off, **kw)
    else:
        x, y, g = mc.make_data(P, G, M, lik, seed=2)
        kw = mc.model_kwargs(lik, centered)
        t = targets.multilevel_regression(x, y, g, n_groups=G, **kw)
    o = np.argsort(g, kind='stable')
    head = np.zeros(8)
    head[0] = ('gaussian', 'student_t', 'bernoulli_logit', 'poisson_log', 'neg_binomial_2_log').index(lik)
    head[1] = M
    head[2] = kw['df'] if lik == 'student_t' else kw['phi'] if lik == 'neg_binomial_2_log' else 0.0
    head[3] = kw['scale'] if lik in ('gaussian', 'student_t') else 0.0
    head[4], head[5], head[6], head[7] = kw['prior_scale'], G, kw['tau_scale'], float(centered)
    parts = [head, x[o].ravel(), y[o], np.concatenate([[0.0], np.cumsum(np.bincount(g, minlength=G))])]
    if count:
        parts += [off[o], [targets.count_constant(y, kw.get('phi'))]]
    want = np.concatenate(parts).astype(np.float64)
    assert t.dim == P + 1 + G and not hasattr(t, 'learned')
    assert t.params.dtype == np.float64 and t.params.tobytes() == want.tobytes()
