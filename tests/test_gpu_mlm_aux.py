"""The multilevel regression target with a learned scale or dispersion
(targets.multilevel_linear_regression, multilevel_robust_regression(..., learn_scale=True),
multilevel_negative_binomial_regression(..., learn_phi=True)) through every route that
accepts targets.multilevel_regression, against the numpy restatement of the same model
(tests/mlm_aux_cases.py) and its host callback on identical numpy-stream draws, on the
pattern of tests/test_gpu_aux.py and at the tolerance tests/test_gpu_mlm.py holds these
kernels to (1e-10 relative to max |expected|: only the summation order and libm-vs-device
exp / log1p / reciprocals differ); and the library's refusals of a bad learned block."""
import numpy as np
import pytest

from tests import mlm_aux_cases as mac
from tests.conftest import gpu_available
from tests.test_gpu_count import _family
from tests.test_gpu_mlm import _close

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

G, M = 6, 50


def _pair(p, lik, centered, seed=0, M=M, G=G):
    """(device target, restatement) of one seeded model; dim = p + 2 + G."""
    from viabel_amd import targets
    x, y, g, off = mac.make_data(p, G, M, lik, seed=seed)
    kw = mac.model_kwargs(lik, centered)
    return (targets.multilevel_regression(x, y, g, n_groups=G, offset=off, **mac.target_kwargs(kw)),
            mac.restatement(x, y, g, offset=off, n_groups=G, **kw))


def _lam(kind, D, lik, seed):
    """Variational parameters whose mean sits at a plausible fit (lambda near the data
    makers' log scale), so the draws are where a fit's are."""
    _, P = _family(kind, D)
    lam = np.random.RandomState(seed).randn(P) * 0.05
    lam[D - 1] += np.log(3.0 if lik == 'neg_binomial_2_log' else 0.7)
    if kind == 'mf_gauss':
        lam[D:2 * D] -= 1.5
    return lam


def _objective(obj, kind, D, target):
    from viabel_amd import vb
    fam, _ = _family(kind, D)
    if obj == 'klvi':
        return vb.black_box_klvi(fam, target, 64)
    return vb.black_box_chivi(2.0, fam, target, 64)


@pytest.mark.parametrize('centered', mac.FORMS)
@pytest.mark.parametrize('lik', mac.LIKELIHOODS)
@pytest.mark.parametrize('p,G_,M_,n', [(4, 6, 50, 30), (19, 6, 50, 30), (5, 9, 321, 257)])
def test_parity_with_restatement(lik, centered, p, G_, M_, n):
    t, f = _pair(p, lik, centered, seed=p, M=M_, G=G_)
    z = mac.start_rows(np.random.RandomState(n), n, p, G_, lik, spread=0.5)
    lp, g = t.logdensity_and_grad(z)
    lp0, g0 = f(z)
    assert lp.shape == (n,) and g.shape == (n, p + 2 + G_)
    _close(lp, lp0, 1e-10)
    _close(g, g0, 1e-10)


@pytest.mark.parametrize('lik', mac.LIKELIHOODS)
@pytest.mark.parametrize('obj', ['klvi', 'chivi'])
@pytest.mark.parametrize('kind', ['mf_gauss', 'cholesky', 'low_rank', 'fr_t'])
@pytest.mark.parametrize('p,centered', [(4, False), (19, True)])
def test_estimators_match_callback_of_same_model(lik, obj, kind, p, centered):
    from viabel_amd import targets
    D = p + 2 + G
    t, f = _pair(p, lik, centered, seed=11)
    o1 = _objective(obj, kind, D, t)
    o2 = _objective(obj, kind, D, targets.callback(f, D))
    lam = _lam(kind, D, lik, 12)
    np.random.seed(1)
    v1, g1 = o1(lam)
    np.random.seed(1)
    v2, g2 = o2(lam)
    np.testing.assert_allclose(v1, v2, rtol=1e-10)
    _close(g1, g2, 1e-10)


@pytest.mark.parametrize('centered', mac.FORMS)
@pytest.mark.parametrize('lik', mac.LIKELIHOODS)
def test_adagrad_trajectory_matches_callback(lik, centered):
    from viabel_amd import vb, targets
    p = 4
    D = p + 2 + G
    t, f = _pair(p, lik, centered, seed=13)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    init = np.zeros(2 * D)
    np.random.seed(3)
    r1 = vb.adagrad_optimize(30, vb.black_box_klvi(f1, t, 30), init)
    np.random.seed(3)
    r2 = vb.adagrad_optimize(30, vb.black_box_klvi(f2, targets.callback(f, D), 30), init)
    _close(r1[1], r2[1], 1e-10)
    _close(r1[2], r2[2], 1e-10)


@pytest.mark.parametrize('lik', mac.LIKELIHOODS)
@pytest.mark.parametrize('p,centered', [(4, True), (19, False)])
def test_log_weights_match_callback(lik, p, centered):
    from viabel_amd import vb, targets, experiments
    D = p + 2 + G
    t, f = _pair(p, lik, centered, seed=14)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    lam = np.concatenate([np.linspace(-0.1, 0.1, D), np.linspace(-2.5, -2.0, D)])
    x1, lw1 = experiments.log_weights(t, f1, lam, 1000)
    x2, lw2 = experiments.log_weights(targets.callback(f, D), f2, lam, 1000)
    _close(x1, x2, 1e-14)
    _close(lw1, lw2, 1e-10)


@pytest.mark.parametrize('lik', mac.LIKELIHOODS)
def test_device_resident_parameter_block(lik):
    """The block in device memory (read in place; s_aux, c_data and J fetched from it)
    gives the bits of the host block."""
    import torch
    from viabel_amd import _native as nat
    p = 19
    t, _ = _pair(p, lik, True, seed=15)
    z = nat.as_f64(mac.start_rows(np.random.RandomState(16), 10, p, G, lik))
    lp0, g0 = t.logdensity_and_grad(z)
    dev = torch.from_numpy(t.params).cuda()
    s = nat.Target(t.kind, 0, t.dim, nat.dptr(dev), t.params.size, nat.TARGET_CALLBACK_T(), None)
    lp, g = np.empty(10), np.empty_like(z)
    nat.check(nat.lib().vb_target_logdensity(nat.context().handle, s, nat.dptr(z), 10,
                                             nat.dptr(lp), nat.dptr(g)))
    assert np.array_equal(lp, lp0) and np.array_equal(g, g0)


def test_wrappers_fit_on_the_device():
    """The three wrappers through a short fit: finite, and lambda moves."""
    from viabel_amd import vb, targets
    p = 4
    for lik, make in (
            ('gaussian', lambda x, y, g, o: targets.multilevel_linear_regression(x, y, g)),
            ('student_t', lambda x, y, g, o: targets.multilevel_robust_regression(
                x, y, g, 5.0, learn_scale=True)),
            ('neg_binomial_2_log', lambda x, y, g, o: targets.multilevel_negative_binomial_regression(
                x, y, g, learn_phi=True, offset=o))):
        x, y, g, off = mac.make_data(p, G, 200, lik, seed=21)
        t = make(x, y, g, off)
        D = p + 2 + G
        assert t.dim == D
        fam = vb.mean_field_gaussian_variational_family(D, rng='philox')
        res = vb.adagrad_optimize(200, vb.black_box_klvi(fam, t, 64), np.zeros(2 * D),
                                  learning_rate=0.05)
        assert np.all(np.isfinite(res[0])) and res[0][D - 1] != 0.0


def test_rows_of_log_weights_refuse_the_kind():
    from viabel_amd import vb, experiments
    t, _ = _pair(3, 'gaussian', False)
    D = 3 + 2 + G
    fam = vb.mean_field_gaussian_variational_family(D, rng='philox')
    with pytest.raises(NotImplementedError, match='rows of log weights'):
        experiments.log_weights_rows(t, fam, np.zeros((2, 2 * D)), 8, 1)


def test_library_refuses_bad_learned_blocks():
    from viabel_amd import targets
    p, Mo = 3, 20
    x, y, g, _ = mac.make_data(p, G, Mo, 'gaussian', seed=17)
    t = targets.multilevel_linear_regression(x, y, g, n_groups=G)
    dim = p + 2 + G
    good = t.params
    assert np.all(np.isfinite(t.logdensity_and_grad(np.zeros((1, dim)))[0]))

    def expect(match, params, dim=dim):
        bad = targets.Target(t.kind, dim, 'multilevel_regression', params)
        with pytest.raises(ValueError, match=match):
            bad.logdensity_and_grad(np.zeros((1, dim)))

    def put(i, v, base=None):
        pr = (good if base is None else base).copy()
        pr[i] = v
        return pr

    for v in (4.0, 2.5, -1.0):
        expect(r'params\[7\] \(form \+ 2 learn\) must be 0, 1, 2 or 3', put(7, v))
    for lid in (2.0, 3.0):
        expect(r'learn = 1, which is valid for the likelihoods 0, 1 and 4', put(0, lid))
    # dim leaves no coefficient: p = dim - 2 - G
    expect(r'does not leave p >= 1 beside 1 \+ G \+ 1 \(learn\)', good, dim=G + 2)
    # a fixed block of the same length is one value too long, and needs its sigma
    expect(r'params\[3\] \(sigma\)', put(7, 0.0))
    for v in (0.0, -1.0, np.inf, np.nan):
        expect(r's_aux \(after the group offsets\) must be positive', put(good.size - 1, v))
    expect(r'n_params \d+ is shorter than', good[:-1].copy(), dim=dim)
    expect(r'n_params \d+ does not match 8 \+ M\*p \+ M \+ G \+ 1 \+ 1',
           np.concatenate([good, [0.0]]))
    # the negative binomial's tail: c_data, s_aux, J, T [J]
    xc, yc, gc_, off = mac.make_data(p, G, Mo, 'neg_binomial_2_log', seed=17)
    tn = targets.multilevel_negative_binomial_regression(xc, yc, gc_, offset=off, n_groups=G,
                                                         learn_phi=True)
    goodn = tn.params
    e = 8 + Mo * p + 2 * Mo + G + 1          # c_data
    assert goodn[e + 2] == goodn.size - (e + 3)
    for v in (0.0, -2.0, np.nan):
        expect(r's_aux \(after c_data\) must be positive', put(e + 1, v, goodn))
    for v in (-1.0, 0.5, 65537.0, np.nan):
        expect(r'J \(the table', put(e + 2, v, goodn))
    expect(r'n_params \d+ does not match .* \+ J', goodn[:-1].copy())
    expect(r'n_params \d+ does not match .* \+ J', np.concatenate([goodn, [0.0]]))
    expect(r'n_params \d+ is shorter than', goodn[:e + 2].copy())
    assert np.all(np.isfinite(tn.logdensity_and_grad(np.zeros((1, dim)))[0]))
