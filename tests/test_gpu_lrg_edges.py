"""The 50-digit edge sets of tests/lrg_mp.py through the kernels of vb_lrg.hip: sample,
logdensity and the three objectives on host draws, against the numpy restatement
(tests/lrg_cases.py).  The allowance is 8 x LRG_ORACLE_ERR in units of 2^-53 S (S as
lrg_mp.np_scales defines it), the margin this project gives every kernel over its
restatement; every entry is compared and every instance prints its measured error beside
its allowance (kept in profiles/lrg/gpu_lrg_tests.log)."""
import numpy as np
import pytest

from oracle import targets_oracle
from tests import lrg_cases as lc
from tests import lrg_mp as lm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

ISO = targets_oracle.isogauss
U = 2.0 ** -53
# every D of {1, 16, 17, 33, 65}, R of {1, 3, 4, 5, 17} and N of {1, 17, 65}
SHAPES = [(1, 1, 1), (16, 3, 17), (17, 4, 65), (33, 5, 17), (65, 17, 65), (65, 1, 1)]


def _check(tag, key, got, ref, S):
    got, ref, S = (np.atleast_1d(np.asarray(a, dtype=float)).ravel() for a in (got, ref, S))
    assert got.shape == ref.shape == S.shape
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got)), tag
    diff = np.abs(got - ref)
    den = U * np.maximum(S, np.abs(ref))
    units = np.where(diff == 0.0, 0.0, diff / np.where(den > 0.0, den, 1.0))   # 0 / 0: exact
    worst = float(np.max(units))
    bar = 8.0 * lm.LRG_ORACLE_ERR[key]
    print('%-32s %-14s worst %.2f units (allowed %.2f)' % (tag, key, worst, bar))
    assert worst <= bar, (tag, key, worst, bar)


def _with_draws(fam, eps, call):
    """Run `call` with the family's next host draws being eps (its RandomState stands in)."""
    class _RS:
        def randn(self, n, d):
            assert (n, d) == eps.shape
            return eps.copy()
    fam.rs = _RS()
    return call()


def _chivi_with_draws(obj, eps, lam):
    obj._eps_one_call = lambda: eps.copy()
    return obj(lam)


@pytest.mark.parametrize('kind', lm.EDGE_KINDS)
@pytest.mark.parametrize('D,R,N', SHAPES)
def test_edge_sets(kind, D, R, N):
    from viabel_amd import vb, targets
    lam, eps = lm.edge_lam(kind, D, R), lm.edge_draws(N, D, R)
    tag = '%s D=%d R=%d N=%d' % (kind, D, R, N)
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    tgt = targets.isogauss(D)
    ofam = lc.LowRankGaussian(D, R)
    ox = ofam.transform(lam, eps)
    pts = ox + np.random.RandomState(D + N).randn(N, D) * 0.5 * np.exp(lam[D:2 * D])
    S = lm.np_scales(ofam, lam, eps, None, pts)
    _check(tag, 'sample', _with_draws(fam, eps, lambda: fam.sample(lam, N)), ox, S['sample'])
    _check(tag, 'logdensity', fam.logdensity(pts, lam), ofam.logdensity(pts, lam), S['logdensity'])
    v, g = _with_draws(fam, eps, lambda: vb.black_box_klvi(fam, tgt, N)(lam))
    ov, og = lc.klvi_value_grad(ofam, ISO, lam, N, draws=eps)
    _check(tag, 'klvi_value', v, ov, S['klvi_value'])
    _check(tag, 'klvi_grad', g, og, S['klvi_grad'])
    v, g = _with_draws(fam, eps, lambda: vb.black_box_klvi_pd(fam, tgt, N)(lam))
    ov, og = lc.klvi_pd_value_grad(ofam, ISO, lam, N, draws=eps)
    _check(tag, 'klvi_pd_value', v, ov, S['klvi_pd_value'])
    _check(tag, 'klvi_pd_grad', g, og, S['klvi_pd_grad'])
    for alpha in (2.0, 1.5):
        Sa = lm.np_scales(ofam, lam, eps, alpha)
        v, g = _chivi_with_draws(vb.black_box_chivi(alpha, fam, tgt, N), eps, lam)
        ov, og = lc.chivi_value_grad(ofam, ISO, lam, N, alpha, draws=eps)
        _check(tag, 'chivi_value', v, ov, Sa['chivi_value'])
        _check(tag, 'chivi_grad', g, og, Sa['chivi_grad'])


@pytest.mark.parametrize('D,R,N', [(16, 3, 17), (65, 17, 65)])
@pytest.mark.parametrize('alpha', [2.0, 1.5])
def test_chivi_rows_with_one_dominant_weight(D, R, N, alpha):
    from viabel_amd import vb, targets
    lam, eps = lm.dominant_lam_draws(N, D, R)
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    ofam = lc.LowRankGaussian(D, R)
    lw = lc.log_weights(ofam, ISO, lam, N, draws=eps)[1]
    assert lw[0] - np.max(lw[1:]) >= 700.0
    S = lm.np_scales(ofam, lam, eps, alpha)
    v, g = _chivi_with_draws(vb.black_box_chivi(alpha, fam, targets.isogauss(D), N), eps, lam)
    ov, og = lc.chivi_value_grad(ofam, ISO, lam, N, alpha, draws=eps)
    tag = 'dominant D=%d R=%d N=%d a=%g' % (D, R, N, alpha)
    _check(tag, 'chivi_value', v, ov, S['chivi_value'])
    _check(tag, 'chivi_grad', g, og, S['chivi_grad'])


@pytest.mark.parametrize('case', ['log_d=300', 'log_d=-300', 'B=1e150'])
@pytest.mark.parametrize('D,R,N', [(1, 1, 1), (17, 4, 17), (65, 17, 65)])
def test_extremes_stay_free_of_nan(case, D, R, N):
    """At log_d = +-300 and at |B| = 1e150 nothing is NaN, and +-inf appears only where
    the restatement has it."""
    from viabel_amd import vb, targets
    lam = lm.edge_lam('plain', D, R)
    if case == 'B=1e150':
        lam[2 * D:] = np.where(lam[2 * D:] < 0, -1e150, 1e150)
    else:
        lam[D:2 * D] = 300.0 if case == 'log_d=300' else -300.0
    eps = lm.edge_draws(N, D, R)
    fam = vb.low_rank_gaussian_variational_family(D, R, rng='numpy')
    tgt = targets.isogauss(D)
    ofam = lc.LowRankGaussian(D, R)
    with np.errstate(all='ignore'):
        ox = ofam.transform(lam, eps)
        outs = [(_with_draws(fam, eps, lambda: fam.sample(lam, N)), ox)]
        pts = ox * 1.5
        outs.append((fam.logdensity(pts, lam), ofam.logdensity(pts, lam)))
        for make, f in ((vb.black_box_klvi, lc.klvi_value_grad),
                        (vb.black_box_klvi_pd, lc.klvi_pd_value_grad)):
            outs.extend(zip(_with_draws(fam, eps, lambda: make(fam, tgt, N)(lam)),
                            f(ofam, ISO, lam, N, draws=eps)))
        outs.extend(zip(_chivi_with_draws(vb.black_box_chivi(2.0, fam, tgt, N), eps, lam),
                        lc.chivi_value_grad(ofam, ISO, lam, N, 2.0, draws=eps)))
    for got, ref in outs:
        got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
        assert not np.any(np.isnan(got) & ~np.isnan(ref))
        assert np.array_equal(np.isinf(got) & ~np.isnan(ref), np.isinf(ref) & ~np.isnan(ref))
