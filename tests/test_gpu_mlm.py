"""Device-resident multilevel regression target (targets.multilevel_regression,
VB_TARGET_MULTILEVEL) against the numpy restatement of the same model
(tests/mlm_cases.py), against the device regression target on the one-hot design, and
against the host callback of the restatement on identical numpy-stream draws.
Single calls are held to 1e-10 relative to max |expected|, the suite's bar for one
evaluation: only the summation order and libm-vs-device exp / log1p / reciprocals
differ."""
import numpy as np
import pytest

from tests import mlm_cases as mc
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.isfinite(b))
    scale = max(1.0, float(np.max(np.abs(b))))
    assert float(np.max(np.abs(a - b))) / scale <= rtol


def _pair(p, G, M, lik, centered, seed=0):
    """(device target, restatement, data) of one seeded model."""
    from viabel_amd import targets
    x, y, g = mc.make_data(p, G, M, lik, seed)
    kw = mc.model_kwargs(lik, centered)
    return (targets.multilevel_regression(x, y, g, n_groups=G, **kw),
            mc.restatement(x, y, g, n_groups=G, **kw), (x, y, g, kw))


# (p, G, M, n).  (1, 1, 1, 1): the smallest; (3, 4, 7, 5): an empty and a singleton group;
# (3, 5, 65, 65) / (4, 3, 129, 10): two / three observation chunks, a group covering the
# whole middle chunk; (16, 9, 321, 10): six chunks at p = 16; (2, 70, 130, 64): more groups
# than an observation tile; (2, 600, 700, 4): D > 512; (17, 3, 65, 17) / (40, 5, 130, 10):
# the tile kernel (p > 16); (2, 3, 25, 4097): many row tiles, the 256-thread launch.
SHAPES = [(1, 1, 1, 1), (3, 4, 7, 5), (3, 5, 65, 65), (4, 3, 129, 10), (16, 9, 321, 10),
          (2, 70, 130, 64), (2, 600, 700, 4), (17, 3, 65, 17), (40, 5, 130, 10), (2, 3, 25, 4097)]


def test_shapes_have_the_documented_groups():
    sizes = np.bincount(mc.make_data(3, 4, 7, 'gaussian', 0)[2], minlength=4)
    assert sizes.min() == 0 and np.sum(sizes == 1) >= 1
    off = np.concatenate([[0], np.cumsum(np.bincount(mc.make_data(4, 3, 129, 'gaussian', 0)[2],
                                                     minlength=3))])
    assert any(off[g] <= 64 and off[g + 1] >= 128 for g in range(3))


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('lik', mc.LIKELIHOODS)
@pytest.mark.parametrize('p,G,M,n', SHAPES)
def test_parity_with_restatement(p, G, M, n, lik, centered):
    t, f, _ = _pair(p, G, M, lik, centered)
    D = p + 1 + G
    z = mc.rows(n, D, p, n + M)
    lp, g = t.logdensity_and_grad(z)
    lp0, g0 = f(z)
    assert lp.shape == (n,) and g.shape == (n, D)
    print('max err', float(np.max(np.abs(lp - lp0))), float(np.max(np.abs(g - g0))))
    _close(lp, lp0, 1e-10)
    _close(g, g0, 1e-10)


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('lik', mc.LIKELIHOODS)
@pytest.mark.parametrize('p,G,M', [(3, 5, 129), (20, 4, 70)])
def test_agrees_with_the_device_regression_on_the_one_hot_design(p, G, M, lik, centered):
    """Two kernels: vb_mlm.hip against vb_glm.hip on X' = [x | onehot(group)] at
    [beta | a_eff]; the host only exchanges the priors (as tests/test_mlm_host.py)."""
    import math
    from viabel_amd import targets
    t, _, (x, y, g, kw) = _pair(p, G, M, lik, centered, seed=3)
    s, st = kw['prior_scale'], kw['tau_scale']
    onehot = np.zeros((M, G))
    onehot[np.arange(M), g] = 1.0
    glm = targets.regression(np.concatenate([x, onehot], axis=1), y,
                             **{k: v for k, v in kw.items() if k not in ('tau_scale', 'centered')})
    z = mc.rows(33, p + 1 + G, p, 4)
    beta, u, a = z[:, :p], z[:, p], z[:, p + 1:]
    tau = np.exp(u)
    aeff = a if centered else tau[:, None] * a
    lp0, g0 = glm.logdensity_and_grad(np.concatenate([beta, aeff], axis=1))
    lp0 = lp0 + np.sum(0.5 * (aeff / s) ** 2, axis=1) + G * (0.5 * math.log(2 * math.pi) + math.log(s))
    S = g0[:, p:] + aeff / s ** 2
    w = (tau / st) ** 2
    lp0 = lp0 + math.log(2 / (math.pi * st)) - np.log1p(w) + u - G * 0.5 * math.log(2 * math.pi)
    if centered:
        lp0 = lp0 - G * u - 0.5 * np.sum((a / tau[:, None]) ** 2, axis=1)
        ga = S - a / tau[:, None] ** 2
        gu = 1 - 2 * w / (1 + w) + np.sum((a / tau[:, None]) ** 2, axis=1) - G
    else:
        lp0 = lp0 - 0.5 * np.sum(a * a, axis=1)
        ga = tau[:, None] * S - a
        gu = 1 - 2 * w / (1 + w) + tau * np.sum(S * a, axis=1)
    lp, gr = t.logdensity_and_grad(z)
    _close(lp, lp0, 1e-10)
    _close(gr, np.concatenate([g0[:, :p], gu[:, None], ga], axis=1), 1e-10)


def _value_only(t, z):
    """log p of the rows z through the value-only instances: vb_target_logdensity
    without a gradient array, the call the log-weight routes make."""
    from viabel_amd import _native as nat
    n, D = z.shape
    lp = np.empty(n)
    nat.check(nat.lib().vb_target_logdensity(nat.context().handle, t._struct(), nat.dptr(z), n,
                                             nat.dptr(lp), None))
    return lp


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('p,G,M,n', [(3, 5, 129, 65), (16, 9, 321, 10), (17, 3, 130, 17)])
def test_value_only_call_has_the_same_bits(p, G, M, n, centered):
    for lik in mc.LIKELIHOODS:
        t, _, _ = _pair(p, G, M, lik, centered, seed=5)
        z = np.ascontiguousarray(mc.rows(n, p + 1 + G, p, 6))
        lp, _ = t.logdensity_and_grad(z)
        assert np.array_equal(_value_only(t, z), lp)


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('p,G,M,n', [(3, 5, 129, 65), (16, 70, 321, 10), (40, 5, 130, 10)])
def test_two_calls_give_the_same_bits(p, G, M, n, centered):
    for lik in mc.LIKELIHOODS:
        t, _, _ = _pair(p, G, M, lik, centered, seed=7)
        z = mc.rows(n, p + 1 + G, p, 8)
        lp1, g1 = t.logdensity_and_grad(z)
        lp2, g2 = t.logdensity_and_grad(z)
        assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)


def _family(kind, D):
    from viabel_amd import vb
    if kind == 'mf_gauss':
        return vb.mean_field_gaussian_variational_family(D, rng='numpy'), 2 * D
    if kind == 'mf_t':
        return vb.mean_field_t_variational_family(D, 40.0, rng='numpy'), 2 * D
    return vb.t_variational_family(D, 100.0, rng='numpy'), D + D * (D + 1) // 2


@pytest.mark.parametrize('kind,rtol', [('mf_gauss', 1e-10), ('mf_t', 1e-10), ('fr_t', 1e-7)])
@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('p,G,M,lik', [(3, 6, 129, 'bernoulli_logit'),      # D = 10
                                       (4, 20, 200, 'student_t')])          # D = 25
def test_adagrad_trajectory_matches_callback(p, G, M, lik, centered, kind, rtol):
    """40 adagrad steps on the numpy stream: the history and the values of the device
    target and of the host callback of the restatement (the full-rank family at the
    tolerance of tests/test_gpu_fullrank.py's trajectories)."""
    from viabel_amd import vb, targets
    D = p + 1 + G
    t, f, _ = _pair(p, G, M, lik, centered, seed=9)
    f1, P = _family(kind, D)
    f2, _ = _family(kind, D)
    init = np.zeros(P)
    if kind == 'fr_t':
        # distinct log-diagonal entries, as tests/test_gpu_fullrank.py starts its runs
        rs = np.random.RandomState(2)
        tri = np.tril_indices(D)
        free = rs.randn(len(tri[0])) * 0.05
        free[tri[0] == tri[1]] = rs.randn(D) * 0.2
        init = np.concatenate([rs.randn(D) * 0.3, free])
    np.random.seed(3)
    r1 = vb.adagrad_optimize(40, vb.black_box_klvi(f1, t, 30), init)
    np.random.seed(3)
    r2 = vb.adagrad_optimize(40, vb.black_box_klvi(f2, targets.callback(f, D), 30), init)
    _close(r1[1], r2[1], rtol)
    _close(r1[2], r2[2], rtol)


@pytest.mark.parametrize('centered', mc.FORMS)
@pytest.mark.parametrize('p,G,M,lik', [(3, 6, 129, 'gaussian'), (4, 70, 200, 'bernoulli_logit')])
def test_log_weights_match_callback(p, G, M, lik, centered):
    from viabel_amd import vb, targets, experiments
    D = p + 1 + G
    t, f, _ = _pair(p, G, M, lik, centered, seed=14)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    lam = np.concatenate([np.linspace(-0.3, 0.3, D), np.linspace(-0.5, 0.1, D)])
    x1, lw1 = experiments.log_weights(t, f1, lam, 1000)
    x2, lw2 = experiments.log_weights(targets.callback(f, D), f2, lam, 1000)
    _close(x1, x2, 1e-14)
    _close(lw1, lw2, 1e-10)


@pytest.mark.parametrize('centered', mc.FORMS)
def test_philox_fit_runs(centered):
    from viabel_amd import vb
    p, G, M = 3, 8, 200
    t, _, _ = _pair(p, G, M, 'gaussian', centered, seed=15)
    D = p + 1 + G
    fam = vb.mean_field_gaussian_variational_family(D, rng='philox')
    res = vb.adagrad_optimize(40, vb.black_box_klvi(fam, t, 30), np.zeros(2 * D))
    assert all(np.all(np.isfinite(np.asarray(r))) for r in res[:3])


def test_rows_of_log_weights_refuse_the_kind():
    from viabel_amd import vb, experiments
    t, _, _ = _pair(3, 6, 20, 'gaussian', False)
    fam = vb.mean_field_gaussian_variational_family(10, rng='philox')
    with pytest.raises(NotImplementedError, match='rows of log weights'):
        experiments.log_weights_rows(t, fam, np.zeros((2, 20)), 8, 1)


def test_parameter_block_is_validated():
    """Every check of vb_capi.hip's multilevel_head."""
    from viabel_amd import targets
    good, _, _ = _pair(2, 4, 9, 'student_t', True)
    dim = good.dim
    good.logdensity_and_grad(np.zeros((1, dim)))
    noff = good.params.size - 5            # index of the first group offset

    def bad(edit, dim=dim, cut=None):
        pr = good.params.copy()
        edit(pr)
        t = targets.Target(good.kind, dim, 'multilevel_regression', pr if cut is None else pr[:cut])
        with pytest.raises(ValueError, match='multilevel target'):
            t.logdensity_and_grad(np.zeros((1, dim)))

    def put(i, v):
        return lambda pr: pr.__setitem__(i, v)

    for v in (3.0, 0.5, -1.0):
        bad(put(0, v))                     # likelihood
    for v in (0.0, 8.0, 9.5):
        bad(put(1, v))                     # M: < 1, n_params no longer fits, fractional
    for v in (0.0, -1.0, np.inf):
        bad(put(2, v))                     # nu (student_t)
    for v in (0.0, np.nan):
        bad(put(3, v))                     # sigma
    for v in (0.0, np.inf):
        bad(put(4, v))                     # prior_scale
    for v in (0.0, 3.0, 4.5):
        bad(put(5, v))                     # G: < 1, sizes no longer fit, fractional
    for v in (0.0, -2.0, np.nan):
        bad(put(6, v))                     # tau_scale
    for v in (2.0, 0.5):
        bad(put(7, v))                     # form
    bad(put(noff, 1.0))                    # first offset not 0
    bad(put(noff + 4, 8.0))                # last offset not M
    bad(lambda pr: pr.__setitem__(slice(noff + 1, noff + 3), [6.0, 2.0]))   # decreasing
    bad(put(noff + 1, 0.5))                # fractional
    bad(put(noff + 2, np.nan))
    bad(lambda pr: None, dim=dim + 1)      # p + 1 + G != dim
    bad(lambda pr: None, dim=5)            # no room for p >= 1
    bad(lambda pr: None, cut=4)            # shorter than the header
    bad(lambda pr: None, cut=good.params.size - 1)
