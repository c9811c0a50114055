"""Device-resident hierarchical normal-means target (targets.hierarchical_normal,
VB_TARGET_HIERARCHICAL) against the numpy restatement of the same model
(tests/hier_cases.py), against the host callback of that restatement on identical
numpy-stream draws, and against the built-in eight-schools target.  Tolerances:
1e-11 relative to max |expected|, as tests/test_gpu_glm.py uses: only the summation
order and libm-vs-device exp / log1p / reciprocals differ."""
import numpy as np
import pytest

from tests import hier_cases as hc
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

FORMS = [False, True]


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.isfinite(b))
    scale = max(1.0, float(np.max(np.abs(b))))
    assert float(np.max(np.abs(a - b))) / scale <= rtol


def _pair(J, centered, seed=0):
    """(device target, restatement) of one seeded model."""
    from viabel_amd import targets
    y, sigma = hc.make_data(J, seed)
    return (targets.hierarchical_normal(y, sigma, centered=centered),
            hc.restatement(y, sigma, centered))


def _rows(n, J, seed):
    """Sample rows in the region a fit visits: mu and log tau a few units wide."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, J + 2)
    x[:, 0] *= 3.0
    return x


# J <= 4, <= 8, <= 14: the lane-per-row kernel's three instances (D <= 16); J = 15
# to 509 (D < 512): one wave per row, 62 / 63 / 64 / 65 around one pass of its 64
# lanes, 257 / 509 past one round of four passes; J >= 510 (D >= 512): one block
# per row, 1000 below and 1030 above one round of its 1024 columns.  n = 257: more
# than one block of rows on every path.
SHAPES = [(1, 1), (8, 10), (14, 64), (14, 257), (15, 1), (15, 257), (62, 100), (63, 64),
          (64, 65), (65, 257), (1000, 33),
          (4, 65), (5, 65), (8, 257), (9, 65), (257, 9), (509, 9), (510, 9), (1030, 5)]


@pytest.mark.parametrize('centered', FORMS)
@pytest.mark.parametrize('J,n', SHAPES)
def test_parity_with_restatement(centered, J, n):
    t, f = _pair(J, centered, seed=J + n)
    x = _rows(n, J, n)
    lp, g = t.logdensity_and_grad(x)
    lp0, g0 = f(x)
    assert lp.shape == (n,) and g.shape == (n, J + 2)
    print('max err', float(np.max(np.abs(lp - lp0))), float(np.max(np.abs(g - g0))))
    _close(lp, lp0, 1e-11)
    _close(g, g0, 1e-11)


def test_non_default_scales():
    from viabel_amd import targets
    y, sigma = hc.make_data(20, 3)
    for centered in FORMS:
        t = targets.hierarchical_normal(y, sigma, centered=centered, mu_scale=2.5, tau_scale=0.75)
        f = hc.restatement(y, sigma, centered, mu_scale=2.5, tau_scale=0.75)
        x = _rows(33, 20, 4)
        lp, g = t.logdensity_and_grad(x)
        lp0, g0 = f(x)
        _close(lp, lp0, 1e-11)
        _close(g, g0, 1e-11)


@pytest.mark.parametrize('centered', FORMS)
@pytest.mark.parametrize('J', [8, 65, 600])
def test_same_bits_alone_and_in_a_batch(centered, J):
    t, _ = _pair(J, centered, seed=21)
    x = _rows(257, J, 22)
    lp1, g1 = t.logdensity_and_grad(x)
    lp2, g2 = t.logdensity_and_grad(x)
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)
    for i in (0, 63, 64, 130, 255, 256):
        lpi, gi = t.logdensity_and_grad(x[i:i + 1])
        assert lpi[0] == lp1[i] and np.array_equal(gi[0], g1[i])


def test_agrees_with_the_built_in_eight_schools():
    from viabel_amd import targets
    t = targets.hierarchical_normal(hc.ES_Y, hc.ES_SIGMA)
    x = np.random.RandomState(23).randn(33, 10)
    lp, g = t.logdensity_and_grad(x)
    lp0, g0 = targets.eight_schools_ncp().logdensity_and_grad(x)
    _close(lp, lp0, 1e-12)
    _close(g, g0, 1e-12)


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
@pytest.mark.parametrize('centered', FORMS)
@pytest.mark.parametrize('J', [8, 20])
def test_estimators_match_callback_of_same_model(kind, centered, J):
    from viabel_amd import targets
    D = J + 2
    t, f = _pair(J, centered, seed=11)
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
    D = 10
    t = targets.eight_schools_cp()
    f = hc.restatement(hc.ES_Y, hc.ES_SIGMA, True)
    f1 = vb.mean_field_t_variational_family(D, 40.0, rng='numpy')
    f2 = vb.mean_field_t_variational_family(D, 40.0, rng='numpy')
    init = np.zeros(2 * D)
    r1 = vb.adagrad_optimize(40, vb.black_box_klvi(f1, t, 30), init)
    r2 = vb.adagrad_optimize(40, vb.black_box_klvi(f2, targets.callback(f, D), 30), init)
    _close(r1[1], r2[1], 1e-10)
    _close(r1[2], r2[2], 1e-10)


@pytest.mark.parametrize('centered', FORMS)
@pytest.mark.parametrize('J', [8, 65])
def test_log_weights_match_callback(centered, J):
    from viabel_amd import vb, targets, experiments
    D = J + 2
    t, f = _pair(J, centered, seed=14)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    lam = np.concatenate([np.linspace(-0.3, 0.3, D), np.linspace(-0.5, 0.1, D)])
    x1, lw1 = experiments.log_weights(t, f1, lam, 1000)
    x2, lw2 = experiments.log_weights(targets.callback(f, D), f2, lam, 1000)
    _close(x1, x2, 1e-14)
    _close(lw1, lw2, 1e-10)


def test_rows_of_log_weights_refuse_the_kind():
    from viabel_amd import vb, targets, experiments
    fam = vb.mean_field_gaussian_variational_family(10, rng='philox')
    with pytest.raises(NotImplementedError, match='rows of log weights'):
        experiments.log_weights_rows(targets.eight_schools_cp(), fam, np.zeros((2, 20)), 8, 1)


def test_parameter_block_is_validated():
    """vb_capi.hip's checks of the block: n_params == 8 + 2 J, D == J + 2, the form
    flag in {0, 1}, scales > 0, reserved entries zero."""
    from viabel_amd import targets
    good = targets.eight_schools_cp()
    x = np.zeros((1, 10))
    good.logdensity_and_grad(x)

    def bad(edit, dim=10, cut=None):
        p = good.params.copy()
        edit(p)
        t = targets.Target(good.kind, dim, 'hierarchical_normal', p if cut is None else p[:cut])
        with pytest.raises(ValueError, match='hierarchical target'):
            t.logdensity_and_grad(np.zeros((1, dim)))

    bad(lambda p: p.__setitem__(0, 2.0))
    bad(lambda p: p.__setitem__(0, 0.5))
    bad(lambda p: p.__setitem__(1, 7.0))          # n_params no longer 8 + 2 J
    bad(lambda p: p.__setitem__(1, 8.5))
    bad(lambda p: p.__setitem__(1, 0.0))
    bad(lambda p: p.__setitem__(2, 0.0))
    bad(lambda p: p.__setitem__(2, np.inf))
    bad(lambda p: p.__setitem__(3, -1.0))
    bad(lambda p: p.__setitem__(3, np.nan))
    bad(lambda p: p.__setitem__(5, 1.0))
    bad(lambda p: None, dim=11)                   # D != J + 2
    bad(lambda p: None, cut=4)                    # shorter than the header
    bad(lambda p: None, cut=23)
