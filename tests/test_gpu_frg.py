"""GPU parity of the Cholesky full-rank Gaussian family
(vb.cholesky_gaussian_variational_family, vb_frg.hip) with its numpy restatement
(tests/frg_cases.py) on identical draws.

Tolerances are those of tests/test_gpu_fullrank.py: helpers 1e-10, samples 1e-11,
values 1e-10 (CHIVI 1e-9), gradients 1e-8 of the largest entry, trajectories 1e-7.
The Cholesky path has no iterative solve, so it has no reason to need more."""
import warnings

import numpy as np
import pytest

from tests import frg_cases as fc
from tests import glm_cases as gc
from tests import mlm_cases as mc
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


def _mods():
    from viabel_amd import vb, targets
    from oracle import fullrank_oracle as fo, rng_oracle, vb_oracle
    return vb, targets, fo, rng_oracle, vb_oracle


def _lam(D, seed, scale=0.05):
    rs = np.random.RandomState(seed)
    tri = np.tril_indices(D)
    free = rs.randn(len(tri[0])) * scale
    free[tri[0] == tri[1]] = rs.randn(D) * 0.2
    return np.concatenate([rs.randn(D) * 0.3, free])


def _pair(name, D):
    """(device target, restatement x -> (log p, grad)) of a named target at D."""
    _, targets, fo, _, _ = _mods()
    if name == 'regression':
        x, y = gc.make_data(D, 65, 'student_t', seed=D)
        kw = gc.model_kwargs('student_t')
        return targets.regression(x, y, **kw), gc.restatement(x, y, **kw)
    if name == 'multilevel_regression':
        G = 10
        p = D - 1 - G
        x, y, g = mc.make_data(p, G, 70, 'gaussian', 1)
        kw = mc.model_kwargs('gaussian', mc.FORMS[0])
        return (targets.multilevel_regression(x, y, g, n_groups=G, **kw),
                mc.restatement(x, y, g, n_groups=G, **kw))
    dev = {'isogauss': lambda: targets.isogauss(D), 'funnel': lambda: targets.funnel(D),
           'eight_schools_ncp': targets.eight_schools_ncp,
           'corr_gauss': lambda: targets.corr_gauss(D)}[name]()
    return dev, fo.target_fn(name, D)


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.isfinite(b))
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b))) / scale
    print('max scaled error %.3e' % err)
    assert err <= rtol, 'max scaled error %.3e > %.1e' % (err, rtol)


# every D of {1, 15, 16, 17, 31, 32, 33, 65, 130} and every N of {1, 3, 16, 17, 64, 65,
# 130}; D = 130 with N = 65 (nine tile rows and a partial one, a partial last k group);
# eight_schools_ncp has its own D = 10
CALLS = [('isogauss', 1, 1), ('corr_gauss', 15, 3), ('corr_gauss', 16, 16), ('funnel', 17, 17),
         ('corr_gauss', 31, 64), ('isogauss', 32, 65), ('corr_gauss', 33, 130), ('funnel', 65, 16),
         ('corr_gauss', 130, 65), ('eight_schools_ncp', 10, 17), ('regression', 17, 64),
         ('multilevel_regression', 15, 3)]


# ---------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 5, 16, 17, 33, 100])
def test_moments_and_helpers(D):
    vb = _mods()[0]
    fam = vb.cholesky_gaussian_variational_family(D)
    ofam = fc.CholeskyGaussian(D)
    lam = _lam(D, D)
    m, cov = fam.mean_and_cov(lam)
    om, ocov = ofam.mean_and_cov(lam)
    _close(m, om, 0)
    _close(cov, ocov, 1e-13)
    np.testing.assert_allclose(fam.entropy(lam), ofam.entropy(lam), rtol=1e-14)
    for p in (2, 4):
        np.testing.assert_allclose(fam.pth_moment(p, lam), ofam.pth_moment(p, lam), rtol=1e-10)
    x = np.random.RandomState(1).randn(50, D) + om
    _close(fam.logdensity(x, lam), ofam.logdensity(x, lam), 1e-10)
    one = fam.logdensity(x[0], lam)
    assert np.ndim(one) == 0
    _close(one, ofam.logdensity(x[0], lam), 1e-10)
    # more points than one block of the substitution kernel
    x = np.random.RandomState(2).randn(300, D) * 2 + om
    _close(fam.logdensity(x, lam), ofam.logdensity(x, lam), 1e-10)
    assert fam.var_param_dim == ofam.var_param_dim == D * (D + 3) // 2


@pytest.mark.parametrize('D', [1, 2, 16, 17, 33])
def test_sample_numpy_stream(D):
    """sample() draws randn(n, D) from the family's RandomState(0) (vb.py:105)."""
    vb = _mods()[0]
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    lam = _lam(D, 3)
    for n in (1, 40, 257):
        _close(fam.sample(lam, n), ofam.sample(lam, n), 1e-11)
    _close(fam.sample(lam, 33, seed=9), ofam.sample(lam, 33, seed=9), 1e-11)


@pytest.mark.parametrize('target,D,N', CALLS)
def test_klvi_and_klvi_pd_calls_numpy_stream(target, D, N):
    vb = _mods()[0]
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    tgt, otgt = _pair(target, D)
    obj = vb.black_box_klvi(fam, tgt, N)
    pd = vb.black_box_klvi_pd(fam, tgt, N)
    pd2 = vb.black_box_klvi_pd2(fam, tgt, N)
    for call in range(2):
        lam = _lam(D, 10 + call)
        v, g = obj(lam)
        ov, og = fc.klvi_value_grad(ofam, otgt, lam, N)
        np.testing.assert_allclose(v, ov, rtol=1e-10, atol=1e-10)
        _close(g, og, 1e-8)
        for o in (pd, pd2):
            v, g = o(lam)
            ov, og = fc.klvi_pd_value_grad(ofam, otgt, lam, N)
            np.testing.assert_allclose(v, ov, rtol=1e-10, atol=1e-10)
            _close(g, og, 1e-8)


@pytest.mark.parametrize('alpha', [2.0, 1.5])
@pytest.mark.parametrize('target,D,N', CALLS)
def test_chivi_call_numpy_stream(target, D, N, alpha):
    vb = _mods()[0]
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    tgt, otgt = _pair(target, D)
    obj = vb.black_box_chivi(alpha, fam, tgt, N)
    for call in range(2):
        lam = _lam(D, 20 + call)
        np.random.seed(100 + call)
        v, g = obj(lam)
        np.random.seed(100 + call)
        ov, og = fc.chivi_value_grad(ofam, otgt, lam, N, alpha)
        np.testing.assert_allclose(v, ov, rtol=1e-9, atol=1e-9)
        _close(g, og, 1e-8)


@pytest.mark.parametrize('D', [3, 16, 65])
def test_philox_noise_equals_c_oracle(D):
    """In-kernel draws: the full-rank t family's z (normal pairs, purpose 0); no s."""
    vb, targets, fo, ro, _ = _mods()
    fam = vb.cholesky_gaussian_variational_family(D, rng='philox')
    ofam = fc.CholeskyGaussian(D)
    lam = _lam(D, 5)
    stream, step = fam.stream, fam.step
    x = fam.sample(lam, 300)
    z = ro.fr_noise(0, stream, step, 300, D, 100.0)[1]
    _close(x, ofam.transform(lam, z), 1e-11)
    obj = vb.black_box_klvi(fam, targets.corr_gauss(D), 64)
    stream, step = fam.stream, fam.step
    v, g = obj(lam)
    z = ro.fr_noise(0, stream, step, 64, D, 100.0)[1]
    ov, og = fc.klvi_value_grad(ofam, fo.target_fn('corr_gauss', D), lam, 64, draws=z)
    np.testing.assert_allclose(v, ov, rtol=1e-10)
    _close(g, og, 1e-8)
    # a sample's bits do not depend on how many rows are drawn beside it
    a = fam.sample(lam, 5, seed=11)
    b = fam.sample(lam, 70, seed=11)
    assert np.array_equal(a, b[:5])


@pytest.mark.parametrize('objective', ['klvi', 'chivi'])
@pytest.mark.parametrize('lr_end', [None, 0.002])
def test_adagrad_trajectory_numpy_stream(objective, lr_end):
    vb, targets, fo, _, vo = _mods()
    D, N, n_iters = 9, 50, 60
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    otgt = fo.target_fn('corr_gauss', D)
    tgt = targets.corr_gauss(D)
    lam0 = _lam(D, 2)
    if objective == 'klvi':
        obj = vb.black_box_klvi(fam, tgt, N)
        ofn = lambda lam: fc.klvi_value_grad(ofam, otgt, lam, N)
    else:
        obj = vb.black_box_chivi(2.0, fam, tgt, N)
        ofn = lambda lam: fc.chivi_value_grad(ofam, otgt, lam, N, 2.0)
    np.random.seed(3)
    sm, hist, vals, _ = vb.adagrad_optimize(n_iters, obj, lam0, learning_rate=.05,
                                            learning_rate_end=lr_end)
    np.random.seed(3)
    osm, ohist, ovals = vo.adagrad_optimize(n_iters, ofn, lam0, learning_rate=.05,
                                            learning_rate_end=lr_end)[:3]
    _close(vals, ovals, 1e-7)
    _close(hist, ohist, 1e-7)
    _close(sm, osm, 1e-7)


@pytest.mark.parametrize('objective', ['klvi', 'chivi', 'klvi_pd'])
@pytest.mark.parametrize('D', [40, 64])
def test_fused_philox_advances_are_bit_identical(objective, D):
    """Fused Philox runs (the adagrad step in the gradient kernel's epilogue): three
    advances of 7 steps equal one advance of 21 bit for bit, and follow the
    restatement's adagrad on the C oracle's draws."""
    vb, targets, fo, ro, vo = _mods()
    N, n_iters = 24, 21
    lam0 = _lam(D, 7)
    tgt, otgt = _pair('corr_gauss', D)

    def run(chunks):
        fam = vb.cholesky_gaussian_variational_family(D, rng='philox')
        obj = {'klvi': lambda: vb.black_box_klvi(fam, tgt, N),
               'chivi': lambda: vb.black_box_chivi(2.0, fam, tgt, N),
               'klvi_pd': lambda: vb.black_box_klvi_pd(fam, tgt, N)}[objective]()
        r = vb.DeviceRun(obj, n_iters, lam0, learning_rate=0.02)
        done = 0
        for c in chunks:
            r.advance_philox(c, 3, 5, done)
            done += c
        return r.result()

    lam_a, hist_a, vals_a, sm_a = run([7, 7, 7])
    lam_b, hist_b, vals_b, sm_b = run([21])
    assert np.array_equal(vals_a, vals_b)
    assert np.array_equal(hist_a, hist_b)
    assert np.array_equal(lam_a, lam_b) and np.array_equal(sm_a, sm_b)

    ofam = fc.CholeskyGaussian(D)
    step = [0]

    def f(l):
        z = ro.fr_noise(3, 5, step[0], N, D, 30.0)[1]
        step[0] += 1
        if objective == 'klvi':
            return fc.klvi_value_grad(ofam, otgt, l, N, draws=z)
        if objective == 'chivi':
            return fc.chivi_value_grad(ofam, otgt, l, N, 2.0, draws=z)
        return fc.klvi_pd_value_grad(ofam, otgt, l, N, draws=z)
    _, ohist, ovals, _ = vo.adagrad_optimize(n_iters, f, lam0, learning_rate=0.02)
    _close(vals_a[0], ovals, 1e-7)
    _close(hist_a[0], ohist, 1e-7)
    _close(lam_a[0], ohist[-1], 1e-7)


def test_rmsprop_ia_equals_the_restatement_through_the_foreign_path():
    """The native RMSProp-IA run against the same optimiser driving the restatement's
    objective as a caller-supplied function (vb._ia_host_chains)."""
    vb, targets, fo, _, _ = _mods()
    D, N, n_iters = 4, 30, 120
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    otgt = fo.target_fn('corr_gauss', D)
    obj = vb.black_box_klvi(fam, targets.corr_gauss(D), N)
    ofn = lambda lam: fc.klvi_value_grad(ofam, otgt, lam, N)
    init = np.zeros(fam.var_param_dim)
    kw = dict(window=500, learning_rate=.01, rhat_window=30, n_optimisers=2, tail_avg_iters=30)
    res = vb.rmsprop_IA_optimize_with_rhat(n_iters, obj, init, D, **kw)
    ores = vb.rmsprop_IA_optimize_with_rhat(n_iters, ofn, init, D, **kw)
    _close(res[1], ores[1], 1e-7)
    _close(res[4], ores[4], 1e-7)
    _close(res[0], ores[0], 1e-7)


def test_adam_ia_runs():
    vb, targets, _, _, _ = _mods()
    D = 5
    fam = vb.cholesky_gaussian_variational_family(D, rng='philox')
    obj = vb.black_box_klvi(fam, targets.corr_gauss(D), 20)
    res = vb.adam_IA_optimize_with_rhat(100, obj, np.zeros(fam.var_param_dim), D, rhat_window=20,
                                        n_optimisers=2, tail_avg_iters=20)
    assert res[1].shape == (2, 100, fam.var_param_dim) and np.all(np.isfinite(res[1]))


@pytest.mark.parametrize('D', [6, 40])
def test_log_weights_vanish_at_the_exact_fit(D):
    """corr_gauss at lambda* = (0, chol Sigma*): q = p, so every log weight is ~0 on both
    sides; compared absolutely, 1e-10 max(1, |log q|)."""
    vb, targets, fo, _, _ = _mods()
    from viabel_amd import experiments
    otgt = fo.target_fn('corr_gauss', D)
    Sig = np.linalg.inv(-otgt(np.eye(D))[1] + otgt(np.zeros((1, D)))[1])
    L = np.linalg.cholesky(0.5 * (Sig + Sig.T))
    M = L.copy()
    M[np.diag_indices(D)] = np.log(np.diag(L))
    lam = np.concatenate([np.zeros(D), M[np.tril_indices(D)]])
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    xs, lw = experiments.log_weights(targets.corr_gauss(D), fam, lam, 500)
    ox, olw = fc.log_weights(ofam, otgt, lam, 500)
    _close(xs, ox, 1e-11)
    bar = 1e-10 * np.maximum(1.0, np.abs(ofam.logdensity(ox, lam)))
    assert np.all(np.abs(olw) <= 1e-9)
    assert np.all(np.abs(lw - olw) <= bar), float(np.max(np.abs(lw - olw) / bar))
    # psis_correction / improve_with_psis accept the family
    samples, slw, khat = experiments.psis_correction(targets.corr_gauss(D), fam, lam, 400)
    assert samples.shape == (D, 400) and np.all(np.isfinite(slw))


@pytest.mark.parametrize('target,D', [('funnel', 12), ('regression', 17)])
def test_log_weights(target, D):
    vb = _mods()[0]
    from viabel_amd import experiments
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    tgt, otgt = _pair(target, D)
    lam = _lam(D, 8)
    xs, lw = experiments.log_weights(tgt, fam, lam, 500)
    ox, olw = fc.log_weights(ofam, otgt, lam, 500)
    _close(xs, ox, 1e-11)
    _close(lw, olw, 1e-9)
    # log q of the samples through the substitution kernel agrees with the draws' form
    _close(fam.logdensity(xs, lam), ofam.logdensity(ox, lam), 1e-10)


def test_rows_refused_and_restarts_complete():
    vb, targets, _, _, _ = _mods()
    from viabel_amd import experiments, restarts
    D = 6
    fac = lambda: vb.cholesky_gaussian_variational_family(D, rng='philox')
    tgt = targets.corr_gauss(D)
    P = fac().var_param_dim
    with pytest.raises(NotImplementedError, match='mean-field families only'):
        experiments.log_weights_rows(tgt, fac(), np.zeros((2, P)), 100, stream=7)
    R, n_iters, N, M = 3, 25, 16, 3000
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        table = restarts.run_restarts(fac, tgt, R, n_iters, n_samples=N, n_bounds=M)
    assert table.shape == (R, 10 + P) and np.all(np.isfinite(table[:, [1, 9]]))
    # column 1 is the mean log weight of restart r at its lambda* on stream 2^20 + r
    for r in range(R):
        f = fac()
        f.stream = (1 << 20) + r
        _, lw = experiments.log_weights(tgt, f, table[r, 10:], M, return_samples=False)
        np.testing.assert_allclose(table[r, 1], np.mean(lw), rtol=1e-12, atol=1e-14)


def test_two_calls_give_the_same_bits():
    vb, targets, _, _, _ = _mods()
    D, N = 33, 65
    lam = _lam(D, 4)
    out = []
    for _ in range(2):
        fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
        np.random.seed(5)
        v1, g1 = vb.black_box_klvi(fam, targets.corr_gauss(D), N)(lam)
        v2, g2 = vb.black_box_chivi(1.5, fam, targets.funnel(D), N)(lam)
        x = fam.sample(lam, 40)
        out.append((v1, g1, v2, g2, x, fam.logdensity(x, lam)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_errors():
    vb, targets, _, _, _ = _mods()
    fam = vb.cholesky_gaussian_variational_family(4)
    with pytest.raises(ValueError, match=r'var_param must have shape \(14,\)'):
        fam.sample(np.zeros(8), 3)
    with pytest.raises(ValueError, match='only p = 2 or 4 supported'):
        fam.pth_moment(3, np.zeros(14))
    with pytest.raises(ValueError, match=r'var_param must have shape \(14,\)'):
        vb.black_box_klvi(fam, targets.corr_gauss(4), 10)(np.zeros(8))
