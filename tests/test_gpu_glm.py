"""Device-resident regression targets (targets.regression, VB_TARGET_REGRESSION)
against the numpy restatement of the same models (tests/glm_cases.py) and
against the host callback of that restatement on identical numpy-stream draws.
Tolerances: 1e-11 relative to max |expected| (1e-10 at M = 1000): only the
summation order and libm-vs-device log1p / exp differ."""
import warnings

import numpy as np
import pytest

from tests import glm_cases as gc
from tests import notebook_cases as nc
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.max(np.abs(b))))
    assert float(np.max(np.abs(a - b))) / scale <= rtol


def _pair(D, M, lik, seed=0):
    """(device target, restatement) of one seeded model."""
    from viabel_amd import targets
    x, y = gc.make_data(D, M, lik, seed=seed)
    kw = gc.model_kwargs(lik)
    return targets.regression(x, y, **kw), gc.restatement(x, y, **kw)


# every D, every M and every n at least once per likelihood; D <= 16 is the
# lane-per-row kernel, D > 16 the matrix-core kernel (40: two column tiles + a
# partial slice), M = 63 / 64 / 65 around the 64-observation tile, M = 1000 more
# than one chunk, n = 257 more than one row tile on both paths
SHAPES = [(1, 1, 1), (2, 25, 10), (3, 63, 64), (16, 64, 100), (17, 65, 257),
          (40, 1000, 100), (40, 25, 1), (2, 1000, 257), (17, 1, 10), (3, 65, 64)]


@pytest.mark.parametrize('lik', gc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', SHAPES)
def test_parity_with_restatement(lik, D, M, n):
    t, f = _pair(D, M, lik, seed=D + M)
    b = np.random.RandomState(n).randn(n, D) * 0.8
    lp, g = t.logdensity_and_grad(b)
    lp0, g0 = f(b)
    assert lp.shape == (n,) and g.shape == (n, D)
    tol = 1e-10 if M == 1000 else 1e-11
    print('max err', float(np.max(np.abs(lp - lp0))), float(np.max(np.abs(g - g0))))
    _close(lp, lp0, tol)
    _close(g, g0, tol)


@pytest.mark.parametrize('D', [3, 20])
def test_logistic_saturated_rows_stay_finite(D):
    from viabel_amd import targets
    M, n = 65, 10
    x, y = gc.make_data(D, M, 'bernoulli_logit', seed=5)
    t = targets.logistic_regression(x, y, prior_scale=3.0)
    f = gc.restatement(x, y, 'bernoulli_logit', prior_scale=3.0)
    b = np.random.RandomState(6).randn(n, D)
    # rows along +-x_0: eta_0 = +-800, the other observations spread around it
    b[0] = 800.0 * x[0] / (x[0] @ x[0])
    b[1] = -b[0]
    assert abs(abs((b[:2] @ x.T)[0, 0]) - 800.0) < 1e-9
    lp, g = t.logdensity_and_grad(b)
    lp0, g0 = f(b)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    _close(lp, lp0, 1e-11)
    _close(g, g0, 1e-11)


@pytest.mark.parametrize('D', [3, 20])
def test_student_t_huge_residuals_stay_finite(D):
    from viabel_amd import targets
    M, n = 65, 10
    x, y = gc.make_data(D, M, 'student_t', seed=7)
    y = y + 1e6 * np.where(np.arange(M) % 2 == 0, 1.0, -1.0)
    t = targets.robust_regression(x, y, 5.0, scale=0.7, prior_scale=3.0)
    f = gc.restatement(x, y, 'student_t', df=5.0, scale=0.7, prior_scale=3.0)
    b = np.random.RandomState(8).randn(n, D)
    lp, g = t.logdensity_and_grad(b)
    lp0, g0 = f(b)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    _close(lp, lp0, 1e-11)
    _close(g, g0, 1e-11)


def _objective(kind, D, target):
    from viabel_amd import vb
    if kind == 'mf_gauss_klvi':
        fam = vb.mean_field_gaussian_variational_family(D, rng='numpy')
        return vb.black_box_klvi(fam, target, 64), 2 * D
    if kind == 'mf_t_chivi':
        fam = vb.mean_field_t_variational_family(D, 40.0, rng='numpy')
        return vb.black_box_chivi(2.0, fam, target, 64), 2 * D
    fam = vb.t_variational_family(D, 100.0, rng='numpy')
    return vb.black_box_klvi(fam, target, 64), D + D * (D + 1) // 2


@pytest.mark.parametrize('kind', ['mf_gauss_klvi', 'mf_t_chivi', 'fr_t_klvi'])
@pytest.mark.parametrize('D', [3, 20])
def test_estimators_match_callback_of_same_model(kind, D):
    from viabel_amd import targets
    t, f = _pair(D, 65, 'student_t', seed=11)
    o1, P = _objective(kind, D, t)
    o2, _ = _objective(kind, D, targets.callback(f, D))
    lam = np.random.RandomState(12).randn(P) * 0.05
    np.random.seed(1)
    v1, g1 = o1(lam)
    np.random.seed(1)
    v2, g2 = o2(lam)
    np.testing.assert_allclose(v1, v2, rtol=1e-11)
    _close(g1, g2, 1e-10)


def test_adagrad_trajectory_matches_callback():
    from viabel_amd import vb, targets
    D = 3
    t, f = _pair(D, 25, 'student_t', seed=13)
    f1 = vb.mean_field_t_variational_family(D, 40.0, rng='numpy')
    f2 = vb.mean_field_t_variational_family(D, 40.0, rng='numpy')
    init = np.zeros(2 * D)
    r1 = vb.adagrad_optimize(40, vb.black_box_klvi(f1, t, 30), init)
    r2 = vb.adagrad_optimize(40, vb.black_box_klvi(f2, targets.callback(f, D), 30), init)
    _close(r1[1], r2[1], 1e-10)
    _close(r1[2], r2[2], 1e-10)


@pytest.mark.parametrize('D', [3, 20])
def test_log_weights_match_callback(D):
    from viabel_amd import vb, targets, experiments
    t, f = _pair(D, 65, 'bernoulli_logit', seed=14)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    lam = np.concatenate([np.linspace(-0.3, 0.3, D), np.linspace(-0.5, 0.1, D)])
    x1, lw1 = experiments.log_weights(t, f1, lam, 1000)
    x2, lw2 = experiments.log_weights(targets.callback(f, D), f2, lam, 1000)
    _close(x1, x2, 1e-14)
    _close(lw1, lw2, 1e-11)


def test_two_calls_give_the_same_bits():
    t, _ = _pair(20, 1000, 'student_t', seed=15)     # more than one observation chunk
    b = np.random.RandomState(16).randn(100, 20)
    lp1, g1 = t.logdensity_and_grad(b)
    lp2, g2 = t.logdensity_and_grad(b)
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)


def test_multi_problem_run():
    from viabel_amd import vb
    D, n_iters, seed = 2, 20, 77
    t, _ = _pair(D, 25, 'student_t', seed=17)
    fam = vb.mean_field_t_variational_family(D, 40.0, rng='philox')
    obj = vb.black_box_klvi(fam, t, 30)
    inits = np.random.RandomState(18).randn(4, 2 * D) * 0.3

    def run(rows, stream):
        r = vb.DeviceRun(obj, n_iters, inits[rows])
        r.advance_philox(n_iters, seed, stream, 0)
        return r.result()

    lam, hist, vals, smooth = run(slice(0, 4), 0)
    assert lam.shape == (4, 2 * D) and smooth.shape == (4, 2 * D)
    assert vals.shape == (4, n_iters) and hist.shape == (4, n_iters - 3 * n_iters // 4, 2 * D)
    for a in (lam, hist, vals, smooth):
        assert np.all(np.isfinite(a))
    assert np.all(np.abs(lam - inits) > 0)
    for rows, stream in ((slice(0, 2), 0), (slice(2, 4), 2)):
        for whole, part in zip((lam, hist, vals, smooth), run(rows, stream)):
            np.testing.assert_array_equal(whole[rows], part)


def _notebook(case, fam, target, spec):
    from viabel_amd import vb, experiments, bounds
    obj = vb.black_box_klvi(fam, target, spec['N'])
    opt = vb.adagrad_optimize(spec['n_iters'], obj, spec['init'], **spec['kw'])[0]
    mean, cov = fam.mean_and_cov(opt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, lw = experiments.get_samples_and_log_weights(target, fam, opt, spec['M_bounds'])
        b = bounds.all_bounds(lw, q_var=cov, moment_bound_fn=lambda p: fam.pth_moment(p, opt))
        D = spec['D']
        res, am, ac = experiments.improve_with_psis(target, fam, opt, spec['M_psis'],
                                                    np.zeros(D), np.eye(D))
    nc.check(case, mean, np.sqrt(np.diag(cov)), b, res['khat'], am, np.sqrt(np.diag(ac)))


def test_robust_regression_mean_field_klvi_notebook_on_device():
    from viabel_amd import vb, targets
    s = nc.RR_MF
    x, y = nc.robust_regression_data()
    _notebook('robust_regression_mf_klvi',
              vb.mean_field_t_variational_family(s['D'], s['df'], rng='numpy'),
              targets.robust_regression(x, y, 40.0), s)


def test_robust_regression_full_rank_klvi_notebook_on_device():
    from viabel_amd import vb, targets
    s = nc.RR_FR
    x, y = nc.robust_regression_data()
    _notebook('robust_regression_fullrank_klvi',
              vb.t_variational_family(s['D'], s['df'], rng='numpy'),
              targets.robust_regression(x, y, 40.0), s)
