"""The count likelihoods (poisson_log, neg_binomial_2_log) of targets.regression and
targets.multilevel_regression through the fit routes, against the host callback of the
numpy restatement of the same model (tests/count_cases.py) on identical numpy-stream
draws, at the tolerances tests/test_gpu_glm.py uses for the same comparison: only the
summation order and libm-vs-device exp / log1p differ."""
import numpy as np
import pytest

from tests import count_cases as cc
from tests.conftest import gpu_available
from tests.test_gpu_glm import _close

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

M = 50


def _pair(D, lik, seed=0):
    from viabel_amd import targets
    x, y, off = cc.make_data(D, M, lik, seed=seed)
    kw = cc.model_kwargs(lik)
    return targets.regression(x, y, offset=off, **kw), cc.restatement(x, y, offset=off, **kw)


def _family(kind, D):
    from viabel_amd import vb
    if kind == 'mf_gauss':
        return vb.mean_field_gaussian_variational_family(D, rng='numpy'), 2 * D
    if kind == 'cholesky':
        return vb.cholesky_gaussian_variational_family(D, rng='numpy'), D + D * (D + 1) // 2
    if kind == 'low_rank':
        return vb.low_rank_gaussian_variational_family(D, 2, rng='numpy'), D * 4
    return vb.t_variational_family(D, 100.0, rng='numpy'), D + D * (D + 1) // 2


def _objective(obj, kind, D, target):
    from viabel_amd import vb
    fam, P = _family(kind, D)
    if obj == 'klvi':
        return vb.black_box_klvi(fam, target, 64), P
    return vb.black_box_chivi(2.0, fam, target, 64), P


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('obj', ['klvi', 'chivi'])
@pytest.mark.parametrize('kind', ['mf_gauss', 'cholesky', 'low_rank', 'fr_t'])
@pytest.mark.parametrize('D', [5, 20])
def test_estimators_match_callback_of_same_model(lik, obj, kind, D):
    from viabel_amd import targets
    t, f = _pair(D, lik, seed=11)
    o1, P = _objective(obj, kind, D, t)
    o2, _ = _objective(obj, kind, D, targets.callback(f, D))
    lam = np.random.RandomState(12).randn(P) * 0.05
    np.random.seed(1)
    v1, g1 = o1(lam)
    np.random.seed(1)
    v2, g2 = o2(lam)
    np.testing.assert_allclose(v1, v2, rtol=1e-11)
    _close(g1, g2, 1e-10)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
def test_adagrad_trajectory_matches_callback(lik):
    from viabel_amd import vb, targets
    D = 5
    t, f = _pair(D, lik, seed=13)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    init = np.zeros(2 * D)
    r1 = vb.adagrad_optimize(30, vb.black_box_klvi(f1, t, 30), init)
    r2 = vb.adagrad_optimize(30, vb.black_box_klvi(f2, targets.callback(f, D), 30), init)
    _close(r1[1], r2[1], 1e-10)
    _close(r1[2], r2[2], 1e-10)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('D', [5, 20])
def test_log_weights_match_callback(lik, D):
    from viabel_amd import vb, targets, experiments
    t, f = _pair(D, lik, seed=14)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    lam = np.concatenate([np.linspace(-0.1, 0.1, D), np.linspace(-2.5, -2.0, D)])
    x1, lw1 = experiments.log_weights(t, f1, lam, 1000)
    x2, lw2 = experiments.log_weights(targets.callback(f, D), f2, lam, 1000)
    _close(x1, x2, 1e-14)
    _close(lw1, lw2, 1e-11)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
def test_device_resident_parameter_block(lik):
    """The block in device memory (read in place, c_data fetched from its last value)
    gives the bits of the host block."""
    import torch
    from viabel_amd import _native as nat
    D = 20
    t, _ = _pair(D, lik, seed=15)
    b = nat.as_f64(np.random.RandomState(16).randn(10, D) * 0.3)
    lp0, g0 = t.logdensity_and_grad(b)
    dev = torch.from_numpy(t.params).cuda()
    s = nat.Target(t.kind, 0, t.dim, nat.dptr(dev), t.params.size, nat.TARGET_CALLBACK_T(), None)
    lp, g = np.empty(10), np.empty_like(b)
    nat.check(nat.lib().vb_target_logdensity(nat.context().handle, s, nat.dptr(b), 10,
                                             nat.dptr(lp), nat.dptr(g)))
    assert np.array_equal(lp, lp0) and np.array_equal(g, g0)


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
def test_bad_blocks_are_rejected(lik):
    from viabel_amd import _native as nat
    t, _ = _pair(5, lik, seed=17)
    b = np.zeros((1, 5))
    good = t.params
    t.params = good[:-1].copy()
    with pytest.raises(ValueError, match=r'8 \+ M\*D \+ M \+ M \+ 1'):
        t.logdensity_and_grad(b)
    if lik == 'neg_binomial_2_log':
        for bad in (0.0, -1.0, np.inf, np.nan):
            t.params = good.copy()
            t.params[2] = bad
            with pytest.raises(ValueError, match=r'params\[2\] \(phi\)'):
                t.logdensity_and_grad(b)
    t.params = good.copy()
    t.params[0] = 5.0
    with pytest.raises(ValueError, match='must be 0, 1, 2, 3 or 4'):
        t.logdensity_and_grad(b)
    assert nat is not None


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
@pytest.mark.parametrize('centered', [False, True])
@pytest.mark.parametrize('kind', ['mf_gauss', 'cholesky'])
def test_multilevel_estimators_match_callback(lik, centered, kind):
    from viabel_amd import vb, targets
    p, G = 3, 6
    x, y, group, off = cc.mlm_make_data(p, G, M, lik, seed=21)
    kw = cc.mlm_model_kwargs(lik, centered)
    t = targets.multilevel_regression(x, y, group, n_groups=G, offset=off, **kw)
    f = cc.mlm_restatement(x, y, group, n_groups=G, offset=off, **kw)
    D = p + 1 + G
    z = np.random.RandomState(22).randn(30, D) * 0.5
    lp, g = t.logdensity_and_grad(z)
    lp0, g0 = f(z)
    _close(lp, lp0, 1e-11)
    _close(g, g0, 1e-11)
    fam1, P = _family(kind, D)
    fam2, _ = _family(kind, D)
    lam = np.random.RandomState(23).randn(P) * 0.05
    lam[D:2 * D] -= 2.0 if kind == 'mf_gauss' else 0.0
    np.random.seed(1)
    v1, g1 = vb.black_box_klvi(fam1, t, 64)(lam)
    np.random.seed(1)
    v2, g2 = vb.black_box_klvi(fam2, targets.callback(f, D), 64)(lam)
    np.testing.assert_allclose(v1, v2, rtol=1e-11)
    _close(g1, g2, 1e-10)


def test_wrappers_build_the_same_targets():
    from viabel_amd import targets
    x, y, off = cc.make_data(5, M, 'poisson_log', seed=3)
    g = np.arange(M) % 4
    pairs = [
        (targets.poisson_regression(x, y, offset=off, prior_scale=3.0),
         targets.regression(x, y, 'poisson_log', offset=off, prior_scale=3.0)),
        (targets.negative_binomial_regression(x, y, 2.5, offset=off),
         targets.regression(x, y, 'neg_binomial_2_log', phi=2.5, offset=off)),
        (targets.multilevel_poisson_regression(x, y, g, offset=off),
         targets.multilevel_regression(x, y, g, 'poisson_log', offset=off)),
        (targets.multilevel_negative_binomial_regression(x, y, g, 2.5, offset=off, centered=True),
         targets.multilevel_regression(x, y, g, 'neg_binomial_2_log', phi=2.5, offset=off,
                                       centered=True)),
    ]
    for a, b in pairs:
        assert np.array_equal(a.params, b.params)
        z = np.random.RandomState(4).randn(3, a.dim) * 0.2
        assert np.array_equal(a(z), b(z))
