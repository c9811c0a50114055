"""The numpy restatement of the count likelihoods (tests/count_cases.py), the reference
of tests/test_gpu_count.py, and the packer's c_data (targets.count_constant), pinned at
the edges: over every case of tests/count_mp.py their values and gradients stay within
twice the recorded COUNT_ORACLE_ERR of a 50-digit mpmath restatement written from the
probability mass functions, in units of 2^-53 S (S the condition sum of the result; see
tests/count_mp.py).  The Poisson overflow points (eta > 709.78) have a test of their
own.  CPU only."""
import time

import numpy as np
import pytest

from tests import count_cases as cc
from tests import count_mp as cm

pytestmark = pytest.mark.skipif(not cm.available(), reason='needs mpmath')

CASES = cm.cases()
MLM_CASES = cm.mlm_cases()


def _errors(case):
    c, ref = cm.edge_reference(*case)
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = cc.restatement(c.x, c.y, offset=c.offset, **c.kw)(c.beta[c.rows])
    return cm.errors(lp, g, ref)


def _mlm_errors(case):
    c, ref = cm.mlm_edge_reference(*case)
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = cc.mlm_restatement(c.x, c.y, c.group, offset=c.offset, n_groups=case[3], **c.kw)(c.z)
    return cm.errors(lp, g, ref)


def _c_data_error(lik, y, phi):
    from viabel_amd import targets
    (hi, lo), S = cm.c_data_reference(y, lik, phi)
    got = targets.count_constant(y, phi if lik == 'neg_binomial_2_log' else None)
    if S == 0.0:
        return 0.0 if got == 0.0 and hi == 0.0 else np.inf
    return abs((got - hi) - lo) / (cm.UNIT * S)


def _all_c_data(lik):
    out = [_c_data_error(lik, cm.edge_case(*c).y, cm.edge_case(*c).kw.get('phi'))
           for c in CASES if c[0] == lik]
    out += [_c_data_error(lik, cm.mlm_edge_case(*c).y, cm.mlm_edge_case(*c).kw.get('phi'))
            for c in MLM_CASES if c[0] == lik]
    return out


def test_all_references_compute_within_two_minutes():
    """Runs first: every reference of every case, which the later tests and the GPU tests
    then share through the per-process cache."""
    t0 = time.perf_counter()
    for case in CASES:
        cm.edge_reference(*case)
    for case in MLM_CASES:
        cm.mlm_edge_reference(*case)
    dt = time.perf_counter() - t0
    print('all %d references: %.1f s' % (len(CASES) + len(MLM_CASES), dt))
    assert dt < 120.0


@pytest.mark.parametrize('lik,D,M,n', CASES)
def test_restatement_matches_multiprecision(lik, D, M, n):
    e_lp, e_g = _errors((lik, D, M, n))
    worst = max(float(e_lp.max()), float(e_g.max()))
    print('%s D=%d M=%d n=%d: restatement worst error %.3f (value %.3f row %d, gradient %.3f at %r) '
          'x 2^-53 S' % (lik, D, M, n, worst, e_lp.max(), int(e_lp.argmax()), e_g.max(),
                         np.unravel_index(int(e_g.argmax()), e_g.shape)))
    assert worst <= 2.0 * cm.COUNT_ORACLE_ERR[('regression', lik)]


@pytest.mark.parametrize('lik,centered,p,G,M', MLM_CASES)
def test_multilevel_restatement_matches_multiprecision(lik, centered, p, G, M):
    e_lp, e_g = _mlm_errors((lik, centered, p, G, M))
    worst = max(float(e_lp.max()), float(e_g.max()))
    print('%s centred=%d p=%d G=%d M=%d: restatement worst error %.3f (value %.3f row %d, '
          'gradient %.3f at %r) x 2^-53 S'
          % (lik, centered, p, G, M, worst, e_lp.max(), int(e_lp.argmax()), e_g.max(),
             np.unravel_index(int(e_g.argmax()), e_g.shape)))
    assert worst <= 2.0 * cm.COUNT_ORACLE_ERR[('multilevel', lik)]


@pytest.mark.parametrize('lik', cc.LIKELIHOODS)
def test_packer_constant_matches_multiprecision(lik):
    errs = _all_c_data(lik)
    print('%s: c_data worst error %.3f x 2^-53 S_c over %d cases' % (lik, max(errs), len(errs)))
    assert max(errs) <= 2.0 * cm.COUNT_ORACLE_ERR[('c_data', lik)]


@pytest.mark.parametrize('phi', [1e-3, 1.0, 20.5, 1e6, 1e12])
@pytest.mark.parametrize('y', [4096.0, 4097.0, 1e5, 1e9, 2.0 ** 53])
def test_packer_constant_beyond_the_product(phi, y):
    """Past y = 4096 the packer leaves the product for Stirling's difference series; the
    same metric, within 2 x 2^-53 S_c (measured: 1.2 at the worst, y = 1e5, phi = 1e12)."""
    assert _c_data_error('neg_binomial_2_log', np.array([y, 3.0]), phi) <= 2.0


def test_lgamma_differences_would_miss_the_bar_at_phi_1e6():
    """What count_constant's docstring says of math.lgamma differences: tens of units
    (measured: 81) where the bar is 2 x COUNT_ORACLE_ERR = 1.5."""
    import math
    y, phi = np.array([7.0, 1000.0] * 50), 1e6
    naive = sum(math.lgamma(v + phi) - math.lgamma(phi) - v * math.log(phi) - math.lgamma(v + 1)
                for v in y)
    (hi, lo), S = cm.c_data_reference(y, 'neg_binomial_2_log', phi)
    assert abs((naive - hi) - lo) / (cm.UNIT * S) > 10.0


def test_recorded_figures_are_the_measured_ones():
    """COUNT_ORACLE_ERR is the measured worst case, not a loose cap."""
    for lik in cc.LIKELIHOODS:
        worst = {
            'regression': max(max(float(e.max()) for e in _errors(c)) for c in CASES if c[0] == lik),
            'multilevel': max(max(float(e.max()) for e in _mlm_errors(c))
                              for c in MLM_CASES if c[0] == lik),
            'c_data': max(_all_c_data(lik)),
        }
        for k, w in worst.items():
            rec = cm.COUNT_ORACLE_ERR[(k, lik)]
            assert 0.5 * rec <= w <= rec * 1.0005, (k, lik, w)


@pytest.mark.parametrize('eta', [710.0, 800.0])
@pytest.mark.parametrize('y', [0.0, 3.0])
def test_poisson_value_is_minus_inf_beyond_exps_range(eta, y):
    """The restatement gives -inf where exp(eta) overflows, with no clamp; the gradient
    there is whatever IEEE gives and is not asserted."""
    x = np.array([[1.0, 0.0], [0.5, 1.0]])
    f = cc.restatement(x, np.array([y, 1.0]), 'poisson_log', prior_scale=3.0)
    lp, _ = f(np.array([[eta, 0.0], [0.1, 0.2]]))
    assert lp[0] == -np.inf and np.isfinite(lp[1])


@pytest.mark.parametrize('lik,D,M,n', CASES)
def test_condition_sums_are_positive_and_finite(lik, D, M, n):
    """S > 0 and finite, but for the one entry where it is 0 by construction: the
    beta = 0 row at the all-zero column of X, whose gradient is exactly 0."""
    c, ref = cm.edge_reference(lik, D, M, n)
    assert np.all(np.isfinite(ref.lp_S)) and np.all(ref.lp_S > 0)
    assert np.all(np.isfinite(ref.g_S))
    zero = np.argwhere(ref.g_S == 0)
    expected = []
    if 'zero' in c.info['cols'] and c.info['n_edge'] >= 1:
        expected = [[0, c.info['cols']['zero']]]
    assert zero.tolist() == expected
    for r, d in zero:
        assert ref.g_hi[r, d] == 0.0 and ref.g_lo[r, d] == 0.0


def test_edge_data_hold_the_documented_points():
    placed = {lik: set() for lik in cc.LIKELIHOODS}
    seen = {lik: dict(prior_scale=set(), phi=set()) for lik in cc.LIKELIHOODS}
    for lik, D, M, n in CASES:
        c = cm.edge_case(lik, D, M, n)
        cols = c.info['cols']
        for k in seen[lik]:
            if k in c.kw:
                seen[lik][k].add(c.kw[k])
        if c.info['n_edge'] >= 1:
            assert np.all(c.beta[0] == 0.0)
        if 'zero' in cols:
            assert np.all(c.x[:, cols['zero']] == 0.0)
        if M >= 3:
            assert np.all(c.x[1] == 0.0)
        if (D, M, n) in cm.ZERO_Y:
            assert np.all(c.y == 0.0)
        elif M >= 6:
            assert tuple(c.y[2:6]) == cm.Y_EDGE
        if M >= 6:
            assert tuple(c.offset[[0, 2, 3, 4, 5]]) == cm.OFFSET_EDGE
        assert np.all((c.y >= 0) & (c.y == np.floor(c.y)))
        eta = c.beta @ c.x.T + c.offset[None, :]
        for r, m, v in c.info['slots']:
            assert abs(eta[r, m] - v) <= 1e-3 * abs(v) and c.offset[m] == 0.0
            base = np.log(c.kw['phi']) if lik == 'neg_binomial_2_log' and abs(v - np.log(c.kw['phi'])) < 1e-6 else None
            placed[lik].add(('zeta', round((v - base) * 1e9)) if base is not None and base != 0.0
                            else ('eta', v))
        if D >= 3 and n >= 15 and M >= 15 and lik == 'poisson_log':   # (D = 2: no direction for -800)
            assert len(c.info['slots']) == len(cm.POIS_ETAS)
    for lik in cc.LIKELIHOODS:
        assert seen[lik]['prior_scale'] == set(cm.PRIOR_SCALES)
    assert seen['neg_binomial_2_log']['phi'] == set(cm.PHIS)
    assert {v for k, v in placed['poisson_log'] if k == 'eta'} == set(cm.POIS_ETAS) | {690.0}
    assert {v for k, v in placed['neg_binomial_2_log'] if k == 'eta'} >= set(cm.NB_ETAS)
    assert {v for k, v in placed['neg_binomial_2_log'] if k == 'zeta'} == {1, -1}
    groups = [cm.mlm_edge_case(*c) for c in MLM_CASES]
    assert any(np.any(np.bincount(c.group, minlength=G) == 0)
               for c, (_, _, _, G, _) in zip(groups, MLM_CASES))
