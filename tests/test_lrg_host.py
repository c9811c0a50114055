"""Host-side checks of the low-rank-plus-diagonal Gaussian family (no GPU): the numpy
restatement (tests/lrg_cases.py) against the 50-digit reference (tests/lrg_mp.py, every
quantity from the dense Sigma) on every edge set, recording LRG_ORACLE_ERR per function in
units of 2^-53 S; value gradients against 50-digit central differences; the B = 0 case
against the mean-field Gaussian oracle; and the public interface's shapes, closed forms
and argument errors, which fire before any device call."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import targets_oracle, vb_oracle
from tests import lrg_cases as lc
from tests import lrg_mp as lm

ROOT = Path(__file__).resolve().parents[1]
ISO = targets_oracle.isogauss
# (D, R, n): every D of {1, 16, 17, 33, 65} and R of {1, 3, 4, 5, 17} of the GPU edge test;
# n is kept small where D is large (the 50-digit sums are slow; S carries the length)
INSTANCES = [(1, 1, 1), (16, 3, 17), (17, 4, 5), (33, 5, 17), (65, 17, 3)]


def _f(v):
    return np.array([float(e) for e in v]) if np.ndim(v) else float(v)


def _tol(fam, lam, mag):
    """Closed forms of the public interface: 64 cond(C) 2^-53 of the magnitude."""
    W, _, _ = fam.capacitance(lam)
    cond = np.linalg.cond(np.eye(fam.rank) + W.T @ W)
    return 64 * cond * 2.0 ** -53 * mag


def _measure_instance(worst, lam, eps, D, R, alphas, with_rest=True):
    n = eps.shape[0]
    fam = lc.LowRankGaussian(D, R)
    ref = lm.reference(lam, eps, D, R, alphas)

    def up(key, got, want, S):
        got = np.asarray(got, dtype=float)
        assert np.all(np.isfinite(got)), key        # the restatement is finite everywhere
        worst[key] = max(worst[key], lm.units(got, want, S))

    if with_rest:
        x = fam.transform(lam, eps)
        pts = x + np.random.RandomState(D + n).randn(n, D) * 0.5 * np.exp(lam[D:2 * D])
        S = lm.np_scales(fam, lam, eps, None, pts)
        up('sample', x, ref['sample'], S['sample'])
        up('logdensity', fam.logdensity(pts, lam), ref['dense'].logdensity(pts), S['logdensity'])
        v, g = lc.klvi_value_grad(fam, ISO, lam, n, draws=eps)
        up('klvi_value', v, [ref['klvi_value']], [S['klvi_value']])
        up('klvi_grad', g, ref['klvi_grad'], S['klvi_grad'])
        v, g = lc.klvi_pd_value_grad(fam, ISO, lam, n, draws=eps)
        up('klvi_pd_value', v, [ref['klvi_pd_value']], [S['klvi_pd_value']])
        up('klvi_pd_grad', g, ref['klvi_pd_grad'], S['klvi_pd_grad'])
    for al in alphas:
        Sa = lm.np_scales(fam, lam, eps, al)
        v, g = lc.chivi_value_grad(fam, ISO, lam, n, al, draws=eps)
        up('chivi_value', v, [ref['chivi_value', al]], [Sa['chivi_value']])
        up('chivi_grad', g, ref['chivi_grad', al], Sa['chivi_grad'])


def test_restatement_against_the_mp_reference():
    """Every edge set at every instance; the measured worst errors are LRG_ORACLE_ERR."""
    worst = {k: 0.0 for k in lm.LRG_ORACLE_ERR}
    for kind in lm.EDGE_KINDS:
        for D, R, n in INSTANCES:
            _measure_instance(worst, lm.edge_lam(kind, D, R), lm.edge_draws(n, D, R), D, R,
                              (2.0, 1.5))
    for D, R, n in ((16, 3, 17), (65, 17, 3)):
        lam, eps = lm.dominant_lam_draws(n, D, R)
        lw = lc.log_weights(lc.LowRankGaussian(D, R), ISO, lam, n, draws=eps)[1]
        assert lw[0] - np.max(lw[1:]) >= 700.0
        _measure_instance(worst, lam, eps, D, R, (2.0, 1.5), with_rest=False)
    print({k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 2.0 * lm.LRG_ORACLE_ERR[k], (k, v, lm.LRG_ORACLE_ERR[k])


def test_woodbury_reference_equals_the_dense_reference():
    for D, R in ((3, 2), (33, 5), (65, 17)):
        lam, eps = lm.edge_lam('plain', D, R), lm.edge_draws(2, D, R)
        x = lm.sample(lam, eps, D, R)
        dense = lm.Dense(lam, D, R).logdensity(x)
        for a, b, c in zip(lm.logdensity(x, lam, D, R), lm.woodbury_logdensity(x, lam, D, R), dense):
            assert abs(a - b) <= lm.mpf(10) ** -40 * (1 + abs(a))
            assert abs(a - c) <= lm.mpf(10) ** -40 * (1 + abs(a))


@pytest.mark.parametrize('name', ['klvi', 'klvi_pd', 'chivi'])
def test_restatement_gradient_against_mp_central_differences(name):
    """Fixed target (standard normal), fixed draws; CHIVI's gradient is the weights, held
    fixed, against the gradient of the log weights (sum_n r_n lw_n(lambda))."""
    D, R, N = 4, 2, 5
    fam = lc.LowRankGaussian(D, R)
    lam, eps = lm.edge_lam('plain', D, R), lm.edge_draws(N, D, R)
    if name == 'chivi':
        r = lm.chivi_weights(lam, eps, D, R, lm.mpf(1.5))
        f = lambda l: sum(a * b for a, b in zip(r, lm.log_weights(l, eps, D, R)))
        g = lc.chivi_value_grad(fam, ISO, lam, N, 1.5, draws=eps)[1]
    elif name == 'klvi':
        f = lambda l: lm.klvi_value(l, eps, D, R)
        g = lc.klvi_value_grad(fam, ISO, lam, N, draws=eps)[1]
    else:
        f = lambda l: lm.klvi_value(l, eps, D, R, pd=True)
        g = lc.klvi_pd_value_grad(fam, ISO, lam, N, draws=eps)[1]
    fd = _f(lm.central_gradient(f, lam))
    # truncation h^2 ~ 1e-24; what remains is the restatement's own rounding
    np.testing.assert_allclose(g, fd, rtol=1e-11, atol=1e-11)


def test_zero_factor_equals_the_mean_field_gaussian_oracle():
    D, R, N = 7, 3, 9
    rs = np.random.RandomState(1)
    mu, ld = rs.randn(D), rs.randn(D) * 0.3
    lam, mlam = lc.pack(mu, ld, np.zeros((D, R))), np.concatenate([mu, ld])
    fam, mf = lc.LowRankGaussian(D, R), vb_oracle.Family('gauss', D)
    eps = rs.randn(N, D + R)
    z = eps[:, :D]
    x = fam.transform(lam, eps)
    np.testing.assert_array_equal(x, mf.transform(mlam, z))
    np.testing.assert_allclose(fam.logdensity(x + 0.1, lam), mf.logdensity(x + 0.1, mlam), rtol=1e-13)
    np.testing.assert_allclose(fam.entropy(lam), mf.entropy(mlam), rtol=1e-14)
    tgt = targets_oracle.TARGETS['funnel']
    v, g = lc.klvi_value_grad(fam, tgt, lam, N, draws=eps)
    mv, mg = vb_oracle.klvi_value_grad(mf, tgt, mlam, N, eps=z)
    np.testing.assert_allclose(v, mv, rtol=1e-13)
    np.testing.assert_allclose(g[:2 * D], mg, rtol=1e-12, atol=1e-13)


def test_public_interface_without_a_device():
    from viabel_amd import vb, _native as nat
    assert 'low_rank_gaussian_variational_family' in vb.__all__
    assert nat.FAMILY_LR_GAUSSIAN == 4
    header = (ROOT / 'include' / 'viabel_amd.h').read_text()
    assert int(re.search(r'VB_FAMILY_LR_GAUSSIAN\s*=\s*(\d+)', header).group(1)) == 4
    assert re.search(r'int32_t rank;', header) and [n for n, _ in nat.Family._fields_][1] == 'rank'
    for D, R in ((1, 1), (4, 2), (33, 17)):
        fam = vb.low_rank_gaussian_variational_family(D, R)
        assert fam.var_param_dim == D * (R + 2)
        assert fam.kind == nat.FAMILY_LR_GAUSSIAN and fam.dim == D and fam.rank == R
        assert fam._struct().rank == R
        assert fam._draw(5).shape == (5, D + R)
        ofam = lc.LowRankGaussian(D, R)
        for kind in ('plain', 'mixed_log_d', 'large_factor'):
            lam = lm.edge_lam(kind, D, R)
            ref = float(lm.entropy(lam, D, R))
            assert abs(fam.entropy(lam) - ref) <= _tol(ofam, lam, max(1.0, abs(ref)) + 8 * D)
            S = lm.dense_sigma(lam, D, R)
            tr = sum(S[i, i] for i in range(D))
            fro = sum(S[i, j] ** 2 for i in range(D) for j in range(D))
            np.testing.assert_allclose(fam.pth_moment(2, lam), float(tr), rtol=1e-13)
            np.testing.assert_allclose(fam.pth_moment(4, lam), float(2 * fro + tr ** 2), rtol=1e-12)
            m, cov = fam.mean_and_cov(lam)
            np.testing.assert_array_equal(m, lam[:D])
            ref_cov = np.array([[float(S[i, j]) for j in range(D)] for i in range(D)])
            np.testing.assert_allclose(cov, ref_cov, rtol=1e-13, atol=1e-13 * np.max(ref_cov))
    fam = vb.low_rank_gaussian_variational_family(4, 2)
    bad = np.zeros(8)
    for call in (lambda: fam.sample(bad, 3), lambda: fam.logdensity(np.zeros((2, 4)), bad),
                 lambda: fam.entropy(bad), lambda: fam.mean_and_cov(bad),
                 lambda: fam.pth_moment(2, bad)):
        with pytest.raises(ValueError, match=r'var_param must have shape \(16,\)'):
            call()
    with pytest.raises(ValueError, match='only p = 2 or 4 supported'):
        fam.pth_moment(3, np.zeros(16))
    with pytest.raises(ValueError, match="rng must be 'numpy' or 'philox'"):
        vb.low_rank_gaussian_variational_family(3, 1, rng='mt')
    for D, R in ((3, 0), (3, 4), (100, 65), (3, 1.5), (3, -1)):
        with pytest.raises(ValueError, match='rank must be an integer'):
            vb.low_rank_gaussian_variational_family(D, R)
