"""GPU parity of the low-rank-plus-diagonal Gaussian family
(vb.low_rank_gaussian_variational_family, vb_lrg.hip) with its numpy restatement
(tests/lrg_cases.py) on identical draws.

Tolerances are those of tests/test_gpu_frg.py for the same quantities: helpers 1e-10,
samples 1e-11, values 1e-10 (CHIVI 1e-9), gradients 1e-8 of the largest entry,
trajectories 1e-7."""
import warnings

import numpy as np
import pytest

from tests import glm_cases as gc
from tests import lrg_cases as lc
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


def _mods():
    from viabel_amd import vb, targets
    from oracle import fullrank_oracle as fo, rng_oracle, vb_oracle
    return vb, targets, fo, rng_oracle, vb_oracle


def _lam(D, R, seed, scale=0.3):
    rs = np.random.RandomState(seed)
    return lc.pack(rs.randn(D) * 0.3, rs.randn(D) * 0.2, rs.randn(D, R) * scale)


def _pair(name, D):
    """(device target, restatement x -> (log p, grad)) of a named target at D."""
    _, targets, fo, _, _ = _mods()
    if name == 'regression':
        x, y = gc.make_data(D, 65, 'student_t', seed=D)
        kw = gc.model_kwargs('student_t')
        return targets.regression(x, y, **kw), gc.restatement(x, y, **kw)
    dev = {'isogauss': lambda: targets.isogauss(D), 'funnel': lambda: targets.funnel(D),
           'corr_gauss': lambda: targets.corr_gauss(D)}[name]()
    return dev, fo.target_fn(name, D)


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.isfinite(b))
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b))) / scale
    print('max scaled error %.3e' % err)
    assert err <= rtol, 'max scaled error %.3e > %.1e' % (err, rtol)


SHAPES = [(D, R) for D in (1, 2, 16, 17, 33) for R in (1, 3, 4, 5, 16, 17) if R <= D]
# (target, D, R, N)
CALLS = [('isogauss', 1, 1, 1), ('corr_gauss', 15, 3, 3), ('corr_gauss', 16, 4, 16),
         ('funnel', 17, 5, 17), ('regression', 33, 17, 65)]


@pytest.mark.parametrize('D,R', SHAPES)
def test_sample_and_logdensity_numpy_stream(D, R):
    """sample() draws randn(n, D + R) from the family's RandomState(0)."""
    vb = _mods()[0]
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    ofam = lc.LowRankGaussian(D, R)
    lam = _lam(D, R, 3)
    for n in (1, 40, 257):
        _close(fam.sample(lam, n), ofam.sample(lam, n), 1e-11)
    _close(fam.sample(lam, 33, seed=9), ofam.sample(lam, 33, seed=9), 1e-11)
    x = np.random.RandomState(1).randn(70, D) * 2 + lam[:D]
    _close(fam.logdensity(x, lam), ofam.logdensity(x, lam), 1e-10)
    one = fam.logdensity(x[0], lam)
    assert np.ndim(one) == 0
    _close(one, ofam.logdensity(x[0], lam), 1e-10)
    np.testing.assert_allclose(fam.entropy(lam), ofam.entropy(lam), rtol=1e-13)
    for p in (2, 4):
        np.testing.assert_allclose(fam.pth_moment(p, lam), ofam.pth_moment(p, lam), rtol=1e-12)


@pytest.mark.parametrize('target,D,R,N', CALLS)
def test_klvi_and_klvi_pd_calls_numpy_stream(target, D, R, N):
    vb = _mods()[0]
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    ofam = lc.LowRankGaussian(D, R)
    tgt, otgt = _pair(target, D)
    obj = vb.black_box_klvi(fam, tgt, N)
    pd = vb.black_box_klvi_pd(fam, tgt, N)
    for call in range(2):
        lam = _lam(D, R, 10 + call)
        v, g = obj(lam)
        ov, og = lc.klvi_value_grad(ofam, otgt, lam, N)
        np.testing.assert_allclose(v, ov, rtol=1e-10, atol=1e-10)
        _close(g, og, 1e-8)
        v, g = pd(lam)
        ov, og = lc.klvi_pd_value_grad(ofam, otgt, lam, N)
        np.testing.assert_allclose(v, ov, rtol=1e-10, atol=1e-10)
        _close(g, og, 1e-8)


@pytest.mark.parametrize('alpha', [2.0, 1.5])
@pytest.mark.parametrize('target,D,R,N', CALLS)
def test_chivi_call_numpy_stream(target, D, R, N, alpha):
    vb = _mods()[0]
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    ofam = lc.LowRankGaussian(D, R)
    tgt, otgt = _pair(target, D)
    obj = vb.black_box_chivi(alpha, fam, tgt, N)
    for call in range(2):
        lam = _lam(D, R, 20 + call)
        np.random.seed(100 + call)
        v, g = obj(lam)
        np.random.seed(100 + call)
        ov, og = lc.chivi_value_grad(ofam, otgt, lam, N, alpha)
        np.testing.assert_allclose(v, ov, rtol=1e-9, atol=1e-9)
        _close(g, og, 1e-8)


@pytest.mark.parametrize('D,R', [(3, 2), (16, 4), (65, 17)])
def test_philox_noise_equals_c_oracle(D, R):
    """In-kernel draws: the generator's Gaussian z row at width D + R."""
    vb, targets, fo, ro, _ = _mods()
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='philox')
    ofam = lc.LowRankGaussian(D, R)
    lam = _lam(D, R, 5)
    stream, step = fam.stream, fam.step
    x = fam.sample(lam, 300)
    eps = ro.fr_noise(0, stream, step, 300, D + R, 100.0)[1]
    _close(x, ofam.transform(lam, eps), 1e-11)
    obj = vb.black_box_klvi(fam, targets.corr_gauss(D), 64)
    stream, step = fam.stream, fam.step
    v, g = obj(lam)
    eps = ro.fr_noise(0, stream, step, 64, D + R, 100.0)[1]
    ov, og = lc.klvi_value_grad(ofam, fo.target_fn('corr_gauss', D), lam, 64, draws=eps)
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
    D, R, N, n_iters = 9, 3, 50, 60
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    ofam = lc.LowRankGaussian(D, R)
    otgt = fo.target_fn('corr_gauss', D)
    tgt = targets.corr_gauss(D)
    lam0 = _lam(D, R, 2)
    if objective == 'klvi':
        obj = vb.black_box_klvi(fam, tgt, N)
        ofn = lambda lam: lc.klvi_value_grad(ofam, otgt, lam, N)
    else:
        obj = vb.black_box_chivi(2.0, fam, tgt, N)
        ofn = lambda lam: lc.chivi_value_grad(ofam, otgt, lam, N, 2.0)
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
@pytest.mark.parametrize('nprob', [1, 2])
def test_fused_philox_advances_are_bit_identical(objective, nprob):
    """Fused Philox runs (the adagrad step in the gradient kernel's epilogue): three
    advances of 7 steps equal one advance of 21 bit for bit, with one and two problems,
    and problem 0 follows the restatement's adagrad on the C oracle's draws."""
    vb, targets, fo, ro, vo = _mods()
    D, R, N, n_iters = 40, 5, 24, 21
    lam0 = np.stack([_lam(D, R, 7 + q) for q in range(nprob)])
    tgt, otgt = _pair('corr_gauss', D)

    def run(chunks):
        fam = vb.low_rank_gaussian_variational_family(D, R, rng='philox')
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

    ofam = lc.LowRankGaussian(D, R)
    step = [0]

    def f(l):
        eps = ro.fr_noise(3, 5, step[0], N, D + R, 30.0)[1]
        step[0] += 1
        if objective == 'klvi':
            return lc.klvi_value_grad(ofam, otgt, l, N, draws=eps)
        if objective == 'chivi':
            return lc.chivi_value_grad(ofam, otgt, l, N, 2.0, draws=eps)
        return lc.klvi_pd_value_grad(ofam, otgt, l, N, draws=eps)
    _, ohist, ovals, _ = vo.adagrad_optimize(n_iters, f, lam0[0], learning_rate=0.02)
    _close(vals_a[0], ovals, 1e-7)
    _close(hist_a[0], ohist, 1e-7)
    _close(lam_a[0], ohist[-1], 1e-7)


def test_ia_optimisers_run():
    vb, targets, _, _, _ = _mods()
    D, R = 5, 2
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='philox')
    obj = vb.black_box_klvi(fam, targets.corr_gauss(D), 20)
    for opt in (vb.adam_IA_optimize_with_rhat, vb.rmsprop_IA_optimize_with_rhat):
        res = opt(100, obj, np.zeros(fam.var_param_dim), D, rhat_window=20, n_optimisers=2,
                  tail_avg_iters=20)
        assert res[1].shape == (2, 100, fam.var_param_dim) and np.all(np.isfinite(res[1]))


@pytest.mark.parametrize('D', [6, 40])
def test_log_weights_vanish_at_the_exact_fit(D):
    """corr_gauss has Sigma* = A A^T / D + I = B* B*^T + diag(1) with B* = A / sqrt(D) of
    rank D: at lambda* = (0, 0, B*) q = p, so every log weight is ~0; compared absolutely,
    1e-9 max(1, |log q|)."""
    vb, targets, _, _, _ = _mods()
    from viabel_amd import experiments
    R = D
    Bs = np.random.RandomState(512).randn(D, D) / np.sqrt(D)
    lam = lc.pack(np.zeros(D), np.zeros(D), Bs)
    tgt = targets.corr_gauss(D)
    np.testing.assert_allclose(Bs @ Bs.T + np.eye(D), tgt.sigma, rtol=1e-12, atol=1e-12)
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    ofam = lc.LowRankGaussian(D, R)
    xs, lw = experiments.log_weights(tgt, fam, lam, 500)
    ox = ofam.sample(lam, 500)
    _close(xs, ox, 1e-11)
    bar = 1e-10 * np.maximum(1.0, np.abs(ofam.logdensity(ox, lam)))
    assert np.all(np.abs(lw) <= 10 * bar), float(np.max(np.abs(lw) / bar))
    samples, slw, khat = experiments.psis_correction(tgt, fam, lam, 400)
    assert samples.shape == (D, 400) and np.all(np.isfinite(slw))


@pytest.mark.parametrize('target,D,R', [('funnel', 12, 3), ('regression', 17, 5)])
def test_log_weights(target, D, R):
    vb = _mods()[0]
    from viabel_amd import experiments
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    ofam = lc.LowRankGaussian(D, R)
    tgt, otgt = _pair(target, D)
    lam = _lam(D, R, 8)
    xs, lw = experiments.log_weights(tgt, fam, lam, 500)
    ox, olw = lc.log_weights(ofam, otgt, lam, 500)
    _close(xs, ox, 1e-11)
    _close(lw, olw, 1e-9)
    # log q of the samples as arbitrary points agrees with the draws' form
    _close(fam.logdensity(xs, lam), ofam.logdensity(ox, lam), 1e-10)


def test_rows_refused_and_restarts_complete():
    vb, targets, _, _, _ = _mods()
    from viabel_amd import experiments, restarts
    D, R = 6, 2
    fac = lambda: vb.low_rank_gaussian_variational_family(D, R, rng='philox')
    tgt = targets.corr_gauss(D)
    P = fac().var_param_dim
    with pytest.raises(NotImplementedError, match='mean-field families only'):
        experiments.log_weights_rows(tgt, fac(), np.zeros((2, P)), 100, stream=7)
    n_r, n_iters, N, M = 3, 25, 16, 3000
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        table = restarts.run_restarts(fac, tgt, n_r, n_iters, n_samples=N, n_bounds=M)
    assert table.shape == (n_r, 10 + P) and np.all(np.isfinite(table[:, [1, 9]]))


def test_two_calls_give_the_same_bits():
    vb, targets, _, _, _ = _mods()
    D, R, N = 33, 5, 65
    lam = _lam(D, R, 4)
    out = []
    for _ in range(2):
        fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
        np.random.seed(5)
        v1, g1 = vb.black_box_klvi(fam, targets.corr_gauss(D), N)(lam)
        v2, g2 = vb.black_box_chivi(1.5, fam, targets.funnel(D), N)(lam)
        x = fam.sample(lam, 40)
        out.append((v1, g1, v2, g2, x, fam.logdensity(x, lam)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('D,R,N', [(5, 2, 7), (33, 4, 65)])
def test_zero_factor_equals_the_mean_field_gaussian(D, R, N):
    """B = 0: the device results equal the mean-field Gaussian's device results on the
    same z columns."""
    vb, targets, _, _, _ = _mods()
    rs = np.random.RandomState(D)
    mu, ld = rs.randn(D) * 0.3, rs.randn(D) * 0.2
    lam = lc.pack(mu, ld, np.zeros((D, R)))
    mlam = np.concatenate([mu, ld])
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    mf = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    eps = np.random.RandomState(0).randn(N, D + R)
    mf.rs = np.random.RandomState(0)
    mf._draw = lambda n, seed=None: eps[:n, :D]
    x = fam.sample(lam, N)
    _close(x, mu + np.exp(ld) * eps[:, :D], 1e-11)
    _close(fam.logdensity(x, lam), mf.logdensity(x, mlam), 1e-10)
    np.testing.assert_allclose(fam.entropy(lam), mf.entropy(mlam), rtol=1e-13)
    tgt = targets.funnel(D)
    fam.rs = np.random.RandomState(0)
    v, g = vb.black_box_klvi(fam, tgt, N)(lam)
    mv, mg = vb.black_box_klvi(mf, tgt, N)(mlam)
    np.testing.assert_allclose(v, mv, rtol=1e-10, atol=1e-10)
    _close(g[:2 * D], mg, 1e-8)


def test_errors():
    vb, targets, _, _, _ = _mods()
    from viabel_amd import _native as nat
    fam = vb.low_rank_gaussian_variational_family(4, 2)
    with pytest.raises(ValueError, match=r'var_param must have shape \(16,\)'):
        fam.sample(np.zeros(8), 3)
    with pytest.raises(ValueError, match=r'var_param must have shape \(16,\)'):
        vb.black_box_klvi(fam, targets.corr_gauss(4), 10)(np.zeros(8))
    # the library validates the rank itself
    out = np.empty((1, 4))
    nz = nat.Noise(nat.NOISE_PHILOX, 0, 0, 0, None)
    for rank in (0, 5, 65):
        rc = nat.lib().vb_family_sample(nat.context().handle, nat.Family(4, rank, 4, 0.0),
                                        nat.dptr(np.zeros(4 * (rank + 2))), 1, nz, nat.dptr(out))
        assert rc == nat.VB_EINVAL
    # vb_family_moments does not take this kind
    rc = nat.lib().vb_family_moments(nat.context().handle, fam._struct(), nat.dptr(np.zeros(16)),
                                     nat.dptr(np.empty((4, 4))), None)
    assert rc == nat.VB_EUNSUPPORTED
