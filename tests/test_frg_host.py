"""Host-side checks of the Cholesky full-rank Gaussian family (no GPU): the numpy
restatement (tests/frg_cases.py) against the 50-digit reference (tests/frg_mp.py) and
against central differences, the measured FRG_ORACLE_ERR, and the public interface's
shape, entropy and argument errors, which fire before any device call."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import targets_oracle
from tests import frg_cases as fc
from tests import frg_mp as fm

ROOT = Path(__file__).resolve().parents[1]
ISO = targets_oracle.isogauss

# (kind, D, n): every edge kind at one-entry, sub-tile and multi-row shapes, and at the
# largest dimensions of the GPU edge test (rounding grows with the length of the sums)
INSTANCES = [(k, D, n) for k in fm.EDGE_KINDS + ('plain',)
             for D, n in ((1, 1), (3, 5), (9, 4), (33, 17), (65, 3))]


def _measure():
    worst = {k: 0.0 for k in fm.FRG_ORACLE_ERR}

    def up(key, got, ref, S):
        worst[key] = max(worst[key], fm.units(got, ref, S))

    for kind, D, n in INSTANCES:
        lam = fm.edge_lam(kind, D)
        z = fm.edge_draws(n, D)
        fam = fc.CholeskyGaussian(D)
        x, Sx = fm.sample(lam, z)
        xs = fam.transform(lam, z)
        up('sample', xs, x, Sx)
        pts = xs + np.random.RandomState(D + n).randn(n, D) * 0.5
        lq, Slq = fm.logdensity(pts, lam)
        up('logdensity', fam.logdensity(pts, lam), lq, Slq)
        v, sv, g, sg = fm.klvi(lam, z)
        ov, og = fc.klvi_value_grad(fam, ISO, lam, n, draws=z)
        up('klvi_value', ov, [v], [sv])
        up('klvi_grad', og, g, sg)
        v, sv, g, sg = fm.klvi(lam, z, pd=True)
        ov, og = fc.klvi_pd_value_grad(fam, ISO, lam, n, draws=z)
        up('klvi_pd_value', ov, [v], [sv])
        up('klvi_grad', og, g, sg)
        for alpha in (2.0, 1.5):
            v, sv, g, sg = fm.chivi(lam, z, alpha)
            ov, og = fc.chivi_value_grad(fam, ISO, lam, n, alpha, draws=z)
            up('chivi_value', ov, [v], [sv])
            up('chivi_grad', og, g, sg)
    for D, n in ((3, 5), (9, 4)):
        lam, z = fm.dominant_pair(n, D)
        fam = fc.CholeskyGaussian(D)
        lw = fc.log_weights(fam, ISO, lam, n, draws=z)[1]
        assert lw[0] - np.max(lw[1:]) >= 700.0
        for alpha in (2.0, 1.5):
            v, sv, g, sg = fm.chivi(lam, z, alpha)
            ov, og = fc.chivi_value_grad(fam, ISO, lam, n, alpha, draws=z)
            up('chivi_value', ov, [v], [sv])
            up('chivi_grad', og, g, sg)
    return worst


def test_restatement_against_the_mp_reference():
    worst = _measure()
    print({k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 2.0 * fm.FRG_ORACLE_ERR[k], (k, v, fm.FRG_ORACLE_ERR[k])


def test_np_scales_equal_the_mp_scales():
    lam, z = fm.edge_lam('offd', 5), fm.edge_draws(4, 5)
    S = fm.np_scales(lam, z, alpha=1.5)
    np.testing.assert_allclose(S['sample'], np.array(fm.sample(lam, z)[1], dtype=float), rtol=1e-12)
    _, sv, _, sg = fm.klvi(lam, z)
    np.testing.assert_allclose(S['klvi_value'], float(sv), rtol=1e-12)
    np.testing.assert_allclose(S['klvi_grad'], np.array(sg, dtype=float), rtol=1e-12)
    np.testing.assert_allclose(S['klvi_pd_value'], float(fm.klvi(lam, z, pd=True)[1]), rtol=1e-12)
    _, sv, _, sg = fm.chivi(lam, z, 1.5)
    np.testing.assert_allclose(S['chivi_value'], float(sv), rtol=1e-9)
    np.testing.assert_allclose(S['chivi_grad'], np.array(sg, dtype=float), rtol=1e-9)
    pts = fc.CholeskyGaussian(5).transform(lam, z) + 0.3
    np.testing.assert_allclose(fm.np_logdensity_scale(pts, lam),
                               np.array(fm.logdensity(pts, lam)[1], dtype=float), rtol=1e-9)
    # where y grows by orders of magnitude from row to row
    for kind in ('diag', 'offd'):
        lam, z = fm.edge_lam(kind, 33), fm.edge_draws(2, 33)
        pts = fc.CholeskyGaussian(33).transform(lam, z) + 0.3
        np.testing.assert_allclose(fm.np_logdensity_scale(pts, lam),
                                   np.array(fm.logdensity(pts, lam)[1], dtype=float), rtol=1e-9)


@pytest.mark.parametrize('name', ['klvi', 'klvi_pd', 'chivi'])
def test_restatement_gradient_against_central_differences(name):
    D, N = 5, 7
    fam = fc.CholeskyGaussian(D)
    lam = fm.edge_lam('plain', D)
    z = fm.edge_draws(N, D)
    tgt = targets_oracle.TARGETS['funnel']
    if name == 'chivi':
        # the reference's CHIVI gradient is alpha / N times the VJP of the log weights
        # against the weights held fixed (vb.py:259-264): difference sum_n r_n lw_n(lam)
        lw0 = fc.log_weights(fam, tgt, lam, N, draws=z)[1]
        r = 1.5 * np.exp(1.5 * (lw0 - np.max(lw0))) / N
        f = lambda l: float(np.sum(r * fc.log_weights(fam, tgt, l, N, draws=z)[1]))
        g = fc.chivi_value_grad(fam, tgt, lam, N, 1.5, draws=z)[1]
    elif name == 'klvi':
        f = lambda l: fc.klvi_value_grad(fam, tgt, l, N, draws=z)[0]
        g = fc.klvi_value_grad(fam, tgt, lam, N, draws=z)[1]
    else:
        f = lambda l: fc.klvi_pd_value_grad(fam, tgt, l, N, draws=z)[0]
        g = fc.klvi_pd_value_grad(fam, tgt, lam, N, draws=z)[1]
    h = 1e-6
    fd = np.array([(f(lam + h * e) - f(lam - h * e)) / (2 * h) for e in np.eye(lam.size)])
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6)


def test_public_interface_without_a_device():
    from viabel_amd import vb, _native as nat
    assert 'cholesky_gaussian_variational_family' in vb.__all__
    assert nat.FAMILY_FR_GAUSSIAN == 3
    header = (ROOT / 'include' / 'viabel_amd.h').read_text()
    assert int(re.search(r'VB_FAMILY_FR_GAUSSIAN\s*=\s*(\d+)', header).group(1)) == 3
    for D in (1, 4, 33):
        fam = vb.cholesky_gaussian_variational_family(D)
        assert fam.var_param_dim == D * (D + 3) // 2
        assert fam.kind == nat.FAMILY_FR_GAUSSIAN and fam.dim == D
        lam = fm.edge_lam('diag', D)
        ref = fm.mpf(D) / 2 * (1 + fm.LOG2PI) + sum(fm._unpack(lam, D)[2])
        assert abs(fm.mpf(float(fam.entropy(lam))) - ref) <= 4 * fm.U * (abs(ref) + 8 * D)
    fam = vb.cholesky_gaussian_variational_family(4)
    bad = np.zeros(8)
    for call in (lambda: fam.sample(bad, 3), lambda: fam.logdensity(np.zeros((2, 4)), bad),
                 lambda: fam.entropy(bad), lambda: fam.mean_and_cov(bad),
                 lambda: fam.pth_moment(2, bad)):
        with pytest.raises(ValueError, match=r'var_param must have shape \(14,\)'):
            call()
    with pytest.raises(ValueError, match='only p = 2 or 4 supported'):
        fam.pth_moment(3, np.zeros(14))
    with pytest.raises(ValueError, match="rng must be 'numpy' or 'philox'"):
        vb.cholesky_gaussian_variational_family(3, rng='mt')
    with pytest.raises(NotImplementedError, match='cholesky_gaussian_variational_family'):
        vb.full_rank_gaussian_variational_family(3)
