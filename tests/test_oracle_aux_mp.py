"""The numpy restatement of the regression target with a learned scale or dispersion
(tests/aux_cases.py), the reference of tests/test_gpu_aux.py, pinned at the edges: over
every case of tests/aux_mp.py its values and gradients (the lambda entry included) stay
within twice the recorded AUX_ORACLE_ERR of a 50-digit mpmath restatement written from the
densities literally, the lambda gradient by mp.diff, in units of 2^-53 S (S the condition
sum of the result; see tests/aux_mp.py).  CPU only."""
import math
import time

import numpy as np
import pytest

from tests import aux_cases as ac
from tests import aux_mp as am

pytestmark = pytest.mark.skipif(not am.available(), reason='needs mpmath')

CASES = am.cases()
TABLE_CASES = am.table_cases()


def _errors(case):
    c, ref = am.edge_reference(*case)
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = ac.restatement(c.x, c.y, offset=c.offset, **c.kw)(c.z)
    return am.errors(lp, g, ref)


def test_all_references_compute_within_two_minutes():
    """Runs first: every reference of every case, which the later tests and the GPU tests
    then share through the per-process cache."""
    t0 = time.perf_counter()
    for case in CASES + TABLE_CASES:
        am.edge_reference(*case)
    dt = time.perf_counter() - t0
    print('all %d references: %.1f s' % (len(CASES) + len(TABLE_CASES), dt))
    assert dt < 120.0


@pytest.mark.parametrize('case', CASES + TABLE_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_restatement_matches_multiprecision(case):
    e_lp, e_g = _errors(case)
    worst = max(float(e_lp.max()), float(e_g.max()))
    p = case[1]
    print('%r: restatement worst error %.3f (value %.3f row %d, coefficients %.3f at %r, lambda '
          '%.3f row %d) x 2^-53 S'
          % (case, worst, e_lp.max(), int(e_lp.argmax()), e_g[:, :p].max(),
             np.unravel_index(int(e_g[:, :p].argmax()), e_g[:, :p].shape), e_g[:, p].max(),
             int(e_g[:, p].argmax())))
    assert worst <= 2.0 * am.AUX_ORACLE_ERR[case[0]]


def test_recorded_figures_are_the_measured_ones():
    """AUX_ORACLE_ERR is the measured worst case, not a loose cap."""
    for lik in ac.LIKELIHOODS:
        worst = max(max(float(e.max()) for e in _errors(c)) for c in CASES + TABLE_CASES
                    if c[0] == lik)
        rec = am.AUX_ORACLE_ERR[lik]
        assert 0.5 * rec <= worst <= rec * 1.0005, (lik, worst)


@pytest.mark.parametrize('case', CASES + TABLE_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_condition_sums_are_positive_and_finite(case):
    """S > 0 and finite, but where it is 0 by construction: a beta_d = 0 entry at the
    all-zero column of X, whose gradient is exactly 0.  The coefficient entries of the
    zero-residual row at lambda = log s_aux - 400 have S = inf (|l''| = 1 / sigma^2 is past
    the range): there only a finite result is asked."""
    c, ref = am.edge_reference(*case)
    assert np.all(np.isfinite(ref.lp_S)) and np.all(ref.lp_S > 0)
    far = np.array([lab == 'zero residual, tail -' for lab in c.info['labels']]
                   + [False] * (c.z.shape[0] - len(c.info['labels'])))
    assert np.all(np.isfinite(ref.g_S[~far])) and np.all(ref.g_S[:, -1] > 0)
    assert np.all(np.isfinite(ref.g_S[:, -1]))
    for r, d in np.argwhere(ref.g_S == 0):
        # beta_d = 0 at the all-zero column, or in a zero-residual row at lambda = log s_aux
        # + 400, where |l''| = 1 / sigma^2 underflows: the entry is exactly 0
        label = c.info['labels'][r] if r < len(c.info['labels']) else ''
        assert c.z[r, d] == 0.0
        assert d == c.info['cols'].get('zero') or label == 'zero residual, tail +'
        assert ref.g_hi[r, d] == 0.0 and ref.g_lo[r, d] == 0.0


def test_edge_data_hold_the_documented_points():
    seen = {lik: dict(hyper_scale=set(), prior_scale=set(), labels=set(), lam=set(), zeta=set())
            for lik in ac.LIKELIHOODS}
    kinds = set()
    for case in CASES + TABLE_CASES:
        lik, p, M = case[0], case[1], case[2]
        c = am.edge_case(*case)
        s = seen[lik]
        s['hyper_scale'].add(c.kw['hyper_scale'])
        s['prior_scale'].add(c.kw['prior_scale'])
        s['labels'].update(c.info['labels'])
        ls = math.log(c.kw['hyper_scale'])
        for r, lab in enumerate(c.info['labels']):
            lam = c.z[r, p]
            if lab.startswith('zero residual'):
                assert np.all(c.y - c.z[r, :p] @ c.x.T == 0.0)
            if lab.endswith('tail -'):
                assert lam == ls - am.TAIL
            if lab.endswith('tail +'):
                assert lam == ls + am.TAIL
            if lab == 'at s_aux':
                assert lam == ls
            if lab in ('zero beta', 'zero residual', 'residual 1e-9'):
                s['lam'].add(lam)
        if lik == 'neg_binomial_2_log':
            kinds.add(c.info['kind'])
            T, _ = ac.dispersion_table(c.y)
            assert T.size == {'zero': 0, 'binary': 1, 'big': 65536}.get(c.info['kind'], T.size)
            s['zeta'].update(v for _, v in c.info['slots'])
            assert np.all((c.y >= 0) & (c.y == np.floor(c.y)))
    for lik in ac.LIKELIHOODS:
        assert seen[lik]['hyper_scale'] == set(am.HYPER_SCALES)
        assert seen[lik]['prior_scale'] == set(am.PRIOR_SCALES)
        assert {'zero beta', 'at s_aux', 'tail +'} <= seen[lik]['labels']
    for lik in ('gaussian', 'student_t'):
        assert {'zero residual', 'zero residual, tail -', 'zero residual, tail +',
                'residual 1e-9', 'residual 1e-12'} <= seen[lik]['labels']
        assert seen[lik]['lam'] == set(am.LAMS['scale'])
    assert 'tail -' in seen['neg_binomial_2_log']['labels']
    assert seen['neg_binomial_2_log']['lam'] == set(am.LAMS['phi'])
    assert seen['neg_binomial_2_log']['zeta'] == set(am.ZETAS)
    assert kinds == {None, 'zero', 'binary', 'big'}


def test_restatement_gradient_is_the_derivative():
    """Central differences of the restatement's value, every likelihood."""
    for lik in ac.LIKELIHOODS:
        x, y, off = ac.make_data(3, 12, lik, seed=1)
        f = ac.restatement(x, y, offset=off, **ac.model_kwargs(lik))
        z = ac.start_rows(np.random.RandomState(5), 1, 3, lik)
        _, gr = f(z)
        for d in range(4):
            h = np.zeros((1, 4))
            h[0, d] = 1e-6
            num = (f(z + h)[0][0] - f(z - h)[0][0]) / 2e-6
            assert abs(num - gr[0, d]) <= 1e-6 * max(1.0, abs(gr[0, d]))


def test_fixed_lambda_equals_the_fixed_parameter_restatements():
    """At a given lambda the learned density is the fixed-parameter one (tests/glm_cases.py,
    tests/count_cases.py) plus the prior of lambda: the two restatements agree."""
    from tests import count_cases as cc
    from tests import glm_cases as gc
    for lik in ac.LIKELIHOODS:
        x, y, off = ac.make_data(4, 30, lik, seed=2)
        kw = ac.model_kwargs(lik)
        z = ac.start_rows(np.random.RandomState(6), 5, 4, lik)
        lp, g = ac.restatement(x, y, offset=off, **kw)(z)
        for r in range(5):
            lam = z[r, 4]
            w = 2.0 * (lam - math.log(kw['hyper_scale']))
            prior = math.log(2.0 / (math.pi * kw['hyper_scale'])) - math.log1p(math.exp(w)) + lam
            if lik == 'neg_binomial_2_log':
                f0 = cc.restatement(x, y, lik, phi=math.exp(lam), offset=off,
                                    prior_scale=kw['prior_scale'])
            else:
                f0 = gc.restatement(x, y, lik, df=kw.get('df'), scale=math.exp(lam),
                                    prior_scale=kw['prior_scale'])
            lp0, g0 = f0(z[r:r + 1, :4])
            assert abs(lp[r] - (lp0[0] + prior)) <= 1e-11 * max(1.0, abs(lp[r]))
            np.testing.assert_allclose(g[r, :4], g0[0], rtol=1e-10, atol=1e-10)
