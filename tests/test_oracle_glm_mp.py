"""The numpy restatement of the regression targets (tests/glm_cases.py), the
reference of tests/test_gpu_glm.py, pinned at the edges: over every case of
tests/glm_mp.py its values and gradients stay within twice the recorded
GLM_ORACLE_ERR[likelihood] of a 50-digit mpmath restatement, in units of 2^-53 S (S
the condition sum of the result; see tests/glm_mp.py).  CPU only."""
import time

import numpy as np
import pytest

from tests import glm_cases as gc
from tests import glm_mp as gm

pytestmark = pytest.mark.skipif(not gm.available(), reason='needs mpmath')

CASES = gm.cases()


def _restatement_errors(case):
    c, ref = gm.edge_reference(*case)
    # the restatement must not overflow or divide by zero on the way
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = gc.restatement(c.x, c.y, **c.kw)(c.beta[c.rows])
    return gm.errors(lp, g, ref)


def test_all_references_compute_within_a_minute():
    """Runs first: every reference of every case, which the later tests and the GPU
    tests then share through the per-process cache."""
    t0 = time.perf_counter()
    for case in CASES:
        gm.edge_reference(*case)
    dt = time.perf_counter() - t0
    print('all %d references: %.1f s' % (len(CASES), dt))
    assert dt < 60.0


@pytest.mark.parametrize('lik,D,M,n', CASES)
def test_restatement_matches_multiprecision(lik, D, M, n):
    e_lp, e_g = _restatement_errors((lik, D, M, n))
    worst = max(float(e_lp.max()), float(e_g.max()))
    print('%s D=%d M=%d n=%d: restatement worst error %.3f (value %.3f, gradient %.3f) x 2^-53 S'
          % (lik, D, M, n, worst, e_lp.max(), e_g.max()))
    assert worst <= 2.0 * gm.GLM_ORACLE_ERR[lik]


def test_recorded_figures_are_the_measured_ones():
    """GLM_ORACLE_ERR is the measured worst case, not a loose cap."""
    for lik in gc.LIKELIHOODS:
        worst = max(max(float(e.max()) for e in _restatement_errors(case))
                    for case in CASES if case[0] == lik)
        assert 0.5 * gm.GLM_ORACLE_ERR[lik] <= worst <= gm.GLM_ORACLE_ERR[lik] * 1.0005, (lik, worst)


def test_student_t_without_scipy_is_as_close(monkeypatch):
    """The written-out student_t density of glm_cases (used where scipy is absent;
    its constant is formed as vb_glm.hip forms it) meets the same bound.  With the
    constant as lgamma((nu+1)/2) - lgamma(nu/2) it missed it by a factor ~10 at
    nu = 1e6 (value error 205 at D = 128, M = 70)."""
    monkeypatch.setattr(gc, '_stats', None)
    for case in CASES:
        if case[0] == 'student_t':
            e_lp, e_g = _restatement_errors(case)
            assert max(float(e_lp.max()), float(e_g.max())) <= 2.0 * gm.GLM_ORACLE_ERR['student_t'], case


@pytest.mark.parametrize('lik,D,M,n', CASES)
def test_condition_sums_are_positive_and_finite(lik, D, M, n):
    """S > 0 and finite for every value and gradient entry, but for the one entry
    where S is 0 by construction: the beta = 0 row at the all-zero column of X, whose
    gradient -beta_d / s^2 + sum_m l'_m 0 is exactly 0 (reference hi = lo = 0)."""
    c, ref = gm.edge_reference(lik, D, M, n)
    assert np.all(np.isfinite(ref.lp_S)) and np.all(ref.lp_S > 0)
    assert np.all(np.isfinite(ref.g_S))
    zero = np.argwhere(ref.g_S == 0)
    expected = []
    if 'zero' in c.info['cols'] and c.info['n_edge'] >= 1:
        expected = [[0, c.info['cols']['zero']]]
    assert zero.tolist() == expected
    for r, d in zero:
        assert c.rows[r] == 0 and ref.g_hi[r, d] == 0.0 and ref.g_lo[r, d] == 0.0
    assert np.all(ref.g_S[ref.g_S != 0] > 0)


def test_model_constants_cover_the_documented_values():
    seen = {lik: dict(prior_scale=set(), scale=set(), df=set()) for lik in gc.LIKELIHOODS}
    for lik, D, M, n in CASES:
        for k, v in gm.case_kwargs(lik, D, M, n).items():
            if k != 'likelihood':
                seen[lik][k].add(v)
    for lik in gc.LIKELIHOODS:
        assert seen[lik]['prior_scale'] == set(gm.PRIOR_SCALES)
        if lik != 'bernoulli_logit':
            assert seen[lik]['scale'] == set(gm.SCALES)
    assert seen['student_t']['df'] == set(gm.DFS)
    pairs = {(k['df'], k['scale']) for k in (gm.case_kwargs(*c) for c in CASES if c[0] == 'student_t')}
    assert len(pairs) == 9


@pytest.mark.parametrize('lik,D,M,n', CASES)
def test_edge_data_hold_the_documented_points(lik, D, M, n):
    c = gm.edge_case(lik, D, M, n)
    x, y, beta, cols = c.x, c.y, c.beta, c.info['cols']
    n_rand = n - c.info['n_edge']
    assert n_rand >= 1 and abs(n_rand - gm.RANDOM_SHARE * n) <= 1
    if D >= 5:
        assert set(cols) == {'ortho', 'zero', 'small', 'big'}
    if c.info['n_edge'] >= 1:
        assert np.all(beta[0] == 0.0)
    if 'zero' in cols:
        assert np.all(x[:, cols['zero']] == 0.0)
    if M >= 3:
        assert np.all(x[1] == 0.0)
    if 'big' in cols:
        ordinary = np.abs(x[:, 0]).mean()
        assert 300 < np.abs(x[:, cols['big']]).mean() / ordinary < 3000
        assert 3e-7 < np.abs(x[:, cols['small']]).mean() / ordinary < 3e-6
    if 'ortho_row' in c.info:
        keep = np.arange(M) != 1
        dl = gm._dl64(lik, c.kw, x @ beta[1], y)[keep]
        v = x[keep, cols['ortho']]
        assert beta[1, cols['ortho']] == 0.0
        cosine = abs(float(dl @ v)) / (np.linalg.norm(dl) * np.linalg.norm(v))
        assert 1e-13 < cosine < 1e-11
    if D >= 5 and M >= 15 and n >= 8:
        assert 'ortho_row' in c.info
    if lik != 'bernoulli_logit' and c.info['n_edge'] >= 3:
        res = y - x @ beta[2]
        if M >= 3:
            assert y[1] == 0.0 and np.all((y - beta @ x.T)[:, 1] == 0.0)
        for m, (kind, v) in c.info['resid'].items():
            want = v if kind == 'abs' else v * y[m]
            assert abs(res[m] - want) <= 1e-3 * abs(want) + 4 * np.spacing(abs(y[m])), (m, res[m], want)
        if M >= 8:
            want = {2, 3, 4, 5} | ({6, 7} if lik == 'student_t' else set())
            assert set(c.info['resid']) == want
    if lik == 'bernoulli_logit':
        eta = beta @ x.T
        if c.info['n_edge'] >= 1:
            assert np.all(eta[0] == 0.0)
        if M >= 3:
            assert np.all(eta[:, 1] == 0.0)
        for r, m, v, yv in c.info['slots']:
            assert abs(eta[r, m] - v) <= 1e-3 * abs(v) and y[m] == yv
        if (D, M, n) in gm.BERN_Y:
            assert np.all(y == gm.BERN_Y[(D, M, n)])
            want = {(sg * v, gm.BERN_Y[(D, M, n)]) for v in gm.BERN_ETAS for sg in (1.0, -1.0)}
        else:
            want = {(sg * v, yv) for v in gm.BERN_ETAS for sg in (1.0, -1.0) for yv in (0.0, 1.0)}
            if M >= 4:
                assert set(y) == {0.0, 1.0}
                assert {y[m] for m in range(M) if np.all(x[m] == 0)} <= {0.0, 1.0}
        if D >= 2 and n >= 8 and M >= 15:
            assert {(v, yv) for _, _, v, yv in c.info['slots']} == want
            # each once
            assert len(c.info['slots']) == len(want)
