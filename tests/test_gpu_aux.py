"""The regression target with a learned scale or dispersion (targets.linear_regression,
robust_regression(..., learn_scale=True), negative_binomial_regression(..., learn_phi=True))
through every route that accepts targets.regression, against the host callback of the
numpy restatement of the same model (tests/aux_cases.py) on identical numpy-stream draws,
at the tolerances tests/test_gpu_glm.py uses for the same comparison; the library's
refusals of a bad learned block; and the bits of fixed-parameter blocks (learn = 0)
against tests/golden/aux_parent_bits.npz, recorded on an MI355X with the build before the
learned mode existed."""
import os

import numpy as np
import pytest

from tests import aux_cases as ac
from tests.conftest import ROOT, gpu_available
from tests.test_gpu_count import _family
from tests.test_gpu_glm import _close

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

M = 50


def _pair(p, lik, seed=0):
    """(device target, restatement) of one seeded model; dim = p + 1."""
    from viabel_amd import targets
    x, y, off = ac.make_data(p, M, lik, seed=seed)
    kw = ac.model_kwargs(lik)
    return (targets.regression(x, y, offset=off, **ac.target_kwargs(kw)),
            ac.restatement(x, y, offset=off, **kw))


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


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
@pytest.mark.parametrize('p,n', [(4, 30), (19, 30), (40, 257)])
def test_parity_with_restatement(lik, p, n):
    t, f = _pair(p, lik, seed=p)
    z = ac.start_rows(np.random.RandomState(n), n, p, lik, spread=0.5)
    lp, g = t.logdensity_and_grad(z)
    lp0, g0 = f(z)
    assert lp.shape == (n,) and g.shape == (n, p + 1)
    _close(lp, lp0, 1e-11)
    _close(g, g0, 1e-11)


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
@pytest.mark.parametrize('obj', ['klvi', 'chivi'])
@pytest.mark.parametrize('kind', ['mf_gauss', 'cholesky', 'low_rank', 'fr_t'])
@pytest.mark.parametrize('p', [4, 19])
def test_estimators_match_callback_of_same_model(lik, obj, kind, p):
    from viabel_amd import targets
    D = p + 1
    t, f = _pair(p, lik, seed=11)
    o1 = _objective(obj, kind, D, t)
    o2 = _objective(obj, kind, D, targets.callback(f, D))
    lam = _lam(kind, D, lik, 12)
    np.random.seed(1)
    v1, g1 = o1(lam)
    np.random.seed(1)
    v2, g2 = o2(lam)
    np.testing.assert_allclose(v1, v2, rtol=1e-11)
    _close(g1, g2, 1e-10)


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
def test_adagrad_trajectory_matches_callback(lik):
    from viabel_amd import vb, targets
    p = 4
    D = p + 1
    t, f = _pair(p, lik, seed=13)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    init = np.zeros(2 * D)
    r1 = vb.adagrad_optimize(30, vb.black_box_klvi(f1, t, 30), init)
    r2 = vb.adagrad_optimize(30, vb.black_box_klvi(f2, targets.callback(f, D), 30), init)
    _close(r1[1], r2[1], 1e-10)
    _close(r1[2], r2[2], 1e-10)


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
@pytest.mark.parametrize('p', [4, 19])
def test_log_weights_match_callback(lik, p):
    from viabel_amd import vb, targets, experiments
    D = p + 1
    t, f = _pair(p, lik, seed=14)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    lam = np.concatenate([np.linspace(-0.1, 0.1, D), np.linspace(-2.5, -2.0, D)])
    x1, lw1 = experiments.log_weights(t, f1, lam, 1000)
    x2, lw2 = experiments.log_weights(targets.callback(f, D), f2, lam, 1000)
    _close(x1, x2, 1e-14)
    _close(lw1, lw2, 1e-11)


@pytest.mark.parametrize('lik', ac.LIKELIHOODS)
def test_device_resident_parameter_block(lik):
    """The block in device memory (read in place; c_data and J fetched from it) gives the
    bits of the host block."""
    import torch
    from viabel_amd import _native as nat
    p = 19
    t, _ = _pair(p, lik, seed=15)
    z = nat.as_f64(ac.start_rows(np.random.RandomState(16), 10, p, lik))
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
    for lik, make in (('gaussian', lambda x, y, o: targets.linear_regression(x, y)),
                      ('student_t', lambda x, y, o: targets.robust_regression(x, y, 5.0, learn_scale=True)),
                      ('neg_binomial_2_log',
                       lambda x, y, o: targets.negative_binomial_regression(x, y, learn_phi=True, offset=o))):
        x, y, off = ac.make_data(p, 200, lik, seed=21)
        t = make(x, y, off)
        fam = vb.mean_field_gaussian_variational_family(p + 1, rng='philox')
        res = vb.adagrad_optimize(200, vb.black_box_klvi(fam, t, 64), np.zeros(2 * (p + 1)),
                                  learning_rate=0.05)
        assert np.all(np.isfinite(res[0])) and res[0][p] != 0.0


def test_library_refuses_bad_learned_blocks():
    from viabel_amd import targets
    x, y, _ = ac.make_data(3, 20, 'gaussian', seed=17)
    t = targets.linear_regression(x, y)
    z = np.zeros((1, 4))
    good = t.params

    def expect(match, params, dim=4):
        t.params, t.dim = params, dim
        with pytest.raises(ValueError, match=match):
            t.logdensity_and_grad(np.zeros((1, dim)))
        t.params, t.dim = good, 4

    bad = good.copy()
    bad[5] = 2.0
    expect(r'params\[5\] \(learn\) must be 0 or 1', bad)
    for lid in (2.0, 3.0):
        bad = good.copy()
        bad[0] = lid
        expect(r'learn\) = 1 is valid for the likelihoods 0, 1 and 4', bad)
    expect(r'learn\) = 1 needs dim >= 2', np.concatenate([good[:8], y]), dim=1)
    for v in (0.0, -1.0, np.inf, np.nan):
        bad = good.copy()
        bad[6] = v
        expect(r'params\[6\] \(s_aux\)', bad)
    bad = good.copy()
    bad[7] = 1.0
    expect(r'params\[7\] \(reserved\)', bad)
    bad = good.copy()
    bad[5] = 0.0               # a fixed block: sigma is needed and s_aux must be zero
    expect(r'params\[3\] \(sigma\)', bad)
    expect(r'n_params', good[:-1].copy())
    # the negative binomial's table
    xc, yc, off = ac.make_data(3, 20, 'neg_binomial_2_log', seed=17)
    tn = targets.negative_binomial_regression(xc, yc, learn_phi=True, offset=off)
    goodn = tn.params
    e = 8 + 20 * 3 + 2 * 20
    for v in (-1.0, 0.5, 65537.0, np.nan):
        bad = goodn.copy()
        bad[e + 1] = v
        tn.params = bad
        with pytest.raises(ValueError, match='J \\(the table'):
            tn.logdensity_and_grad(z)
    tn.params = goodn[:-1].copy()
    with pytest.raises(ValueError, match='n_params'):
        tn.logdensity_and_grad(z)
    tn.params = goodn
    assert np.all(np.isfinite(tn.logdensity_and_grad(z)[0]))


def _fixture():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'make_aux_parent_bits', os.path.join(ROOT, 'tests', 'golden', 'make_aux_parent_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, np.load(os.path.join(ROOT, 'tests', 'golden', 'aux_parent_bits.npz'))


def test_fixed_blocks_give_the_bits_they_gave_before():
    """learn = 0, every likelihood, both kernels, one and several chunks and slabs."""
    mod, gold = _fixture()
    assert len(mod.cases()) == 20
    for lik, D, Mo, n in mod.cases():
        t = mod.build(lik, D, Mo)
        assert t.params[5] == 0.0
        lp, g = t.logdensity_and_grad(mod.rows(D, n))
        k = mod.key(lik, D, Mo, n)
        assert np.array_equal(lp, gold[k + '_lp']), k
        assert np.array_equal(g, gold[k + '_g']), k
