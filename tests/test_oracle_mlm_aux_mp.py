"""The numpy restatement of the multilevel regression target with a learned scale or
dispersion (tests/mlm_aux_cases.py), the reference of tests/test_gpu_mlm_aux.py, pinned: over
the edge sets of tests/mlm_aux_mp.py its values and gradients stay within twice the recorded
MLM_AUX_ORACLE_ERR of a 50-digit mpmath restatement written from the literal densities, in
units of 2^-53 S; and with lambda held at log sigma it is the fixed-scale restatement of
tests/mlm_cases.py plus the prior of lambda.  CPU only."""
import math

import numpy as np
import pytest

from tests import mlm_aux_cases as mac
from tests import mlm_aux_mp as mam
from tests import mlm_cases as mc

needs_mp = pytest.mark.skipif(not mam.available(), reason='needs mpmath')

_CACHE = {}     # the errors of a case, computed once and shared by the tests below


def _errors(*key):
    if key not in _CACHE:
        c, ref = mam.edge_reference(*key)
        G = key[3]
        # the restatement must not overflow or divide by zero on the way
        with np.errstate(over='raise', divide='raise', invalid='raise'):
            lp, g = mac.restatement(c.x, c.y, c.group, offset=c.offset, n_groups=G, **c.kw)(
                np.array(c.z))
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
        _CACHE[key] = (c, mam.errors(lp, g, ref))
    return _CACHE[key]


def _report(tag, key, c, e_lp, e_g):
    p = key[2]
    r = int(np.argmax(e_lp))
    gr, gc = np.unravel_index(int(np.argmax(e_g[:, :-1])), e_g[:, :-1].shape)
    lr = int(np.argmax(e_g[:, -1]))
    print('%s %r: value %.3f (row %d), beta / u / group entries %.3f (row %d, column %d, u = %r), '
          'lambda %.3f (row %d, lambda = %r) x 2^-53 S'
          % (tag, key, e_lp[r], r, e_g[gr, gc], gr, gc, float(c.z[gr, p]), e_g[lr, -1], lr,
             float(c.z[lr, -1])))
    return max(e_lp[r], e_g[gr, gc], e_g[lr, -1])


@needs_mp
@pytest.mark.parametrize('lik,centered,p,G,M', mam.cases())
def test_restatement_matches_multiprecision(lik, centered, p, G, M):
    key = (lik, centered, p, G, M)
    c, (e_lp, e_g) = _errors(*key)
    assert c.z.shape[0] <= 40
    assert _report('MLM AUX ORACLE', key, c, e_lp, e_g) <= 2.0 * mam.MLM_AUX_ORACLE_ERR[centered]


@needs_mp
@pytest.mark.parametrize('lik,centered,p,G,M,kind', mam.table_cases())
def test_dispersion_tables(lik, centered, p, G, M, kind):
    key = (lik, centered, p, G, M, kind)
    c, (e_lp, e_g) = _errors(*key)
    assert int(c.y.max()) == {'zero': 0, 'binary': 1, 'big': 65536}[kind]
    assert _report('MLM AUX ORACLE table', key, c, e_lp, e_g) <= 2.0 * mam.MLM_AUX_ORACLE_ERR[centered]


@needs_mp
@pytest.mark.parametrize('centered', mac.FORMS)
def test_recorded_figures_are_the_measured_ones(centered):
    """MLM_AUX_ORACLE_ERR is the measured worst case, not a loose cap."""
    keys = [k for k in mam.cases() + mam.table_cases() if k[1] == centered]
    worst = max(max(float(e.max()) for e in _errors(*k)[1]) for k in keys)
    print('MLM AUX ORACLE worst centred=%d: %.4f' % (centered, worst))
    assert 0.5 * mam.MLM_AUX_ORACLE_ERR[centered] <= worst <= mam.MLM_AUX_ORACLE_ERR[centered] * 1.001


@needs_mp
def test_edge_sets_cover_the_documented_points():
    for lik, centered, p, G, M in mam.cases():
        c = mam.edge_case(lik, centered, p, G, M)
        z, D = c.z, p + 2 + G
        assert z.shape[1] == D
        lams = mam.LAMS['phi' if lik == 'neg_binomial_2_log' else 'scale']
        for uc in mam.U_CENTRES:
            for lam in lams:
                assert np.any((z[:, p] == uc) & (z[:, D - 1] == lam))
        for uw in mam.U_WIDE:
            assert np.sum(z[:, p] == uw) == 1
        eta = np.array([mam._eta(c.x, c.group, zr, p, G, centered, c.offset) for zr in z])
        if lik == 'neg_binomial_2_log':
            zeta = eta - z[:, D - 1:]
            for v in mam.ZETAS:
                assert np.any(np.abs(zeta[:, c.offset == 0.0] - v) <= 1e-9 * max(1.0, abs(v)) + 1e-12)
        else:
            assert np.sum(np.max(np.abs(c.y - eta), axis=1) > 0.5 * mam.RESID_FAR) >= 3
        far = mam.far_rows(c, p, G)
        ls = math.log(c.kw['hyper_scale'])
        assert sorted(far[:2, D - 1] - ls) == [-mam.TAIL, mam.TAIL] and sorted(far[2:, p]) == [-400.0, 400.0]
    dfs = {mam.case_kwargs('student_t', False, i)['df'] for i in range(len(mam.SHAPES))}
    assert dfs == {0.5, 5.0, 1e6}
    for name, vals in (('prior_scale', mam.PRIOR_SCALES), ('hyper_scale', mam.HYPER_SCALES),
                       ('tau_scale', mam.TAU_SCALES)):
        seen = {mam.case_kwargs(lik, c, i)[name] for lik in mac.LIKELIHOODS for c in mac.FORMS
                for i in range(len(mam.SHAPES))}
        assert {1e-3, 1e3} <= seen and seen == set(vals)


@pytest.mark.parametrize('centered', mac.FORMS)
@pytest.mark.parametrize('lik', ['gaussian', 'student_t'])
def test_lambda_fixed_is_the_fixed_scale_model_plus_the_prior(lik, centered):
    """lambda = log sigma in every row: the learned restatement is
    mlm_cases.restatement(scale=sigma) plus log p(lambda), and their gradients agree on
    every shared coordinate."""
    p, G, M, sigma = 3, 5, 70, 0.6
    x, y, group = mc.make_data(p, G, M, lik, seed=4)
    kw = mac.model_kwargs(lik, centered)
    fixed = {k: v for k, v in kw.items() if k != 'hyper_scale'}
    z0 = mc.rows(12, p + 1 + G, p, 5)
    z = np.concatenate([z0, np.full((12, 1), math.log(sigma))], axis=1)
    lp, g = mac.restatement(x, y, group, n_groups=G, **kw)(z)
    lp0, g0 = mc.restatement(x, y, group, n_groups=G, scale=sigma, **fixed)(z0)
    prior = mac.lambda_prior(z[:, -1], kw['hyper_scale'])
    np.testing.assert_allclose(lp, lp0 + prior, rtol=1e-12)
    np.testing.assert_allclose(g[:, :-1], g0, rtol=1e-10, atol=1e-10)
