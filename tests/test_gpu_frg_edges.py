"""The 50-digit edge sets of tests/frg_mp.py through the kernels of vb_frg.hip: sample,
logdensity and the three objectives on host draws, against the numpy restatement
(tests/frg_cases.py).  The allowance is 8 x FRG_ORACLE_ERR in units of 2^-53 S (S as
in tests/frg_mp.py), the margin this project gives every kernel over its restatement;
every entry is compared.

Measured on an MI355X, worst over all instances in units (allowance in brackets): sample
4.52 (23.92), logdensity 1.81 (6.32), KLVI value 1.32 (11.36), KLVI / KLVI_PD gradient
2.62 (17.28), KLVI_PD value 2.66 (20.00), CHIVI value 0.43 (4.00), CHIVI gradient 0.59
(7.04); every instance's printed line is kept in profiles/frg/gpu_frg_tests.log."""
import numpy as np
import pytest

from oracle import targets_oracle
from tests import frg_cases as fc
from tests import frg_mp as fm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

ISO = targets_oracle.isogauss
U = fm.U
# every D of {1, 16, 17, 33, 65} and every N / n of {1, 17, 65}
SHAPES = [(1, 1), (16, 17), (17, 65), (33, 17), (65, 65), (65, 1)]


def _check(tag, key, got, ref, S):
    got, ref, S = (np.atleast_1d(np.asarray(a, dtype=float)).ravel() for a in (got, ref, S))
    assert got.shape == ref.shape == S.shape
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got)), tag
    diff = np.abs(got - ref)
    den = U * np.maximum(S, np.abs(ref))
    units = np.where(diff == 0.0, 0.0, diff / np.where(den > 0.0, den, 1.0))   # 0 / 0: exact
    worst = float(np.max(units))
    bar = 8.0 * fm.FRG_ORACLE_ERR[key]
    print('%-28s %-14s worst %.2f units (allowed %.2f)' % (tag, key, worst, bar))
    assert worst <= bar, (tag, key, worst, bar)


def _objs(D, N):
    from viabel_amd import vb, targets
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    t = targets.isogauss(D)
    return fam, vb.black_box_klvi(fam, t, N), vb.black_box_klvi_pd(fam, t, N), t


def _with_draws(fam, z, call):
    """Run `call` with the family's next host draws being z (its RandomState stands in)."""
    class _RS:
        def randn(self, n, d):
            assert (n, d) == z.shape
            return z.copy()
    fam.rs = _RS()
    return call()


@pytest.mark.parametrize('kind', fm.EDGE_KINDS)
@pytest.mark.parametrize('D,N', SHAPES)
def test_edge_sets(kind, D, N):
    from viabel_amd import vb
    lam = fm.edge_lam(kind, D)
    z = fm.edge_draws(N, D)
    tag = '%s D=%d N=%d' % (kind, D, N)
    fam, klvi, pd, tgt = _objs(D, N)
    ofam = fc.CholeskyGaussian(D)
    S = fm.np_scales(lam, z, alpha=2.0)
    xs = _with_draws(fam, z, lambda: fam.sample(lam, N))
    ox = ofam.transform(lam, z)
    _check(tag, 'sample', xs, ox, S['sample'])
    pts = ox + np.random.RandomState(D + N).randn(N, D) * 0.5
    _check(tag, 'logdensity', fam.logdensity(pts, lam), ofam.logdensity(pts, lam),
           fm.np_logdensity_scale(pts, lam))
    v, g = _with_draws(fam, z, lambda: klvi(lam))
    ov, og = fc.klvi_value_grad(ofam, ISO, lam, N, draws=z)
    _check(tag, 'klvi_value', v, ov, S['klvi_value'])
    _check(tag, 'klvi_grad', g, og, S['klvi_grad'])
    v, g = _with_draws(fam, z, lambda: pd(lam))
    ov, og = fc.klvi_pd_value_grad(ofam, ISO, lam, N, draws=z)
    _check(tag, 'klvi_pd_value', v, ov, S['klvi_pd_value'])
    _check(tag, 'klvi_grad', g, og, S['klvi_grad'])
    for alpha in (2.0, 1.5):
        Sa = fm.np_scales(lam, z, alpha=alpha)
        chivi = vb.black_box_chivi(alpha, fam, tgt, N)
        v, g = _chivi_with_draws(fam, z, chivi, lam)
        ov, og = fc.chivi_value_grad(ofam, ISO, lam, N, alpha, draws=z)
        _check(tag, 'chivi_value', v, ov, Sa['chivi_value'])
        _check(tag, 'chivi_grad', g, og, Sa['chivi_grad'])


def _chivi_with_draws(fam, z, obj, lam):
    """CHIVI draws from RandomState(seed) of its own (vb.py:251): hand it z through
    the objective's draw hook."""
    obj._eps_one_call = lambda: z.copy()
    return obj(lam)


@pytest.mark.parametrize('D,N', [(16, 17), (65, 65)])
@pytest.mark.parametrize('alpha', [2.0, 1.5])
def test_chivi_rows_with_one_dominant_weight(D, N, alpha):
    from viabel_amd import vb, targets
    lam, z = fm.dominant_pair(N, D)
    fam = vb.cholesky_gaussian_variational_family(D, rng='numpy')
    ofam = fc.CholeskyGaussian(D)
    lw = fc.log_weights(ofam, ISO, lam, N, draws=z)[1]
    assert lw[0] - np.max(lw[1:]) >= 700.0
    S = fm.np_scales(lam, z, alpha=alpha)
    v, g = _chivi_with_draws(fam, z, vb.black_box_chivi(alpha, fam, targets.isogauss(D), N), lam)
    ov, og = fc.chivi_value_grad(ofam, ISO, lam, N, alpha, draws=z)
    tag = 'dominant D=%d N=%d a=%g' % (D, N, alpha)
    _check(tag, 'chivi_value', v, ov, S['chivi_value'])
    _check(tag, 'chivi_grad', g, og, S['chivi_grad'])


@pytest.mark.parametrize('m', [300.0, -300.0])
@pytest.mark.parametrize('D,N', [(1, 1), (17, 17), (65, 65)])
def test_extreme_log_diagonal_stays_finite(m, D, N):
    """At M_ii = +-300 nothing is NaN, and +-inf appears only where the restatement has it."""
    from viabel_amd import vb
    lam = fm.edge_lam('plain', D)
    lam[fc.diag_index(D)] = m
    z = fm.edge_draws(N, D)
    fam, klvi, pd, tgt = _objs(D, N)
    ofam = fc.CholeskyGaussian(D)
    outs = [(_with_draws(fam, z, lambda: fam.sample(lam, N)), ofam.transform(lam, z))]
    pts = ofam.transform(lam, z) * 1.5
    outs.append((fam.logdensity(pts, lam), ofam.logdensity(pts, lam)))
    with np.errstate(all='ignore'):
        for o, f in ((klvi, fc.klvi_value_grad), (pd, fc.klvi_pd_value_grad)):
            outs.extend(zip(_with_draws(fam, z, lambda: o(lam)), f(ofam, ISO, lam, N, draws=z)))
        chivi = vb.black_box_chivi(2.0, fam, tgt, N)
        outs.extend(zip(_chivi_with_draws(fam, z, chivi, lam),
                        fc.chivi_value_grad(ofam, ISO, lam, N, 2.0, draws=z)))
    for got, ref in outs:
        got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
        assert not np.any(np.isnan(got) & ~np.isnan(ref))
        assert np.array_equal(np.isinf(got) & ~np.isnan(ref), np.isinf(ref) & ~np.isnan(ref))
