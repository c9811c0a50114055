"""The numpy restatements behind tests/test_gpu_bounds_psis.py and
tests/test_gpu_switches.py (oracle/bounds_oracle.py divergence_stats and
centered_moments; np.cov / np.average) pinned over the edge cases of
tests/bounds_mp.py: every quantity stays within twice the recorded
BOUNDS_ORACLE_ERR of a 50-digit mpmath restatement, in units of 2^-53 S (S as in
tests/bounds_mp.py), and the non-finite patterns are the ones the reference states.
CPU only."""
import time
import warnings

import numpy as np
import pytest

from oracle import bounds_oracle as bo
from tests import bounds_mp as bm

pytestmark = pytest.mark.skipif(not bm.available(), reason='needs mpmath')


def _div_errors(name):
    lw, alpha, elbo = bm.div_case(name)
    ref = bm.div_reference(name)
    got = dict(zip(bm.OUT7, bo.divergence_stats(lw, alpha, elbo)))
    assert got['max'] == ref['max'][0] or (np.isnan(got['max']) and np.isnan(ref['max'][0]))
    e = {}
    for q in bm.QUANTITIES:
        hi, lo, S = ref[q]
        v = float(bm.err(got[q], hi, lo, S))
        if np.isfinite(hi):
            e[q] = v
        else:
            assert v == 0.0, (name, q, got[q], hi)         # the same inf, or both nan
    return e


def _moment_errors(name):
    ref = bm.moment_reference(name)
    c2, c4 = bo.centered_moments(bm.moment_case(name))
    return {bm.moment_quantity(name, 2): float(bm.err(c2, *ref['c2'])),
            bm.moment_quantity(name, 4): float(bm.err(c4, *ref['c4']))}


def numpy_mean_cov(x, w, lw, ddof):
    if lw is not None:
        with np.errstate(under='ignore'):
            w = np.exp(lw - np.max(lw))
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        cov = np.cov(x.T, aweights=w, ddof=ddof).reshape(x.shape[1], x.shape[1])
    return np.average(x, axis=0, weights=w), cov


def _cov_errors(name):
    x, w, lw, ddof = bm.cov_case(name)
    (m_hi, m_lo, m_S), (hi, lo, S) = bm.cov_reference(name)
    m, cov = numpy_mean_cov(x, w, lw, ddof)
    ec = bm.err(cov, hi, lo, S)
    if np.all(np.isnan(hi)):
        assert np.all(np.isnan(cov)), name           # 0 / 0 normaliser: nan everywhere
        return {'mean_w': float(bm.err(m, m_hi, m_lo, m_S).max())}
    return {'mean_w': float(bm.err(m, m_hi, m_lo, m_S).max()), 'cov': float(ec.max())}


def _check(errors, what):
    print(what, ' '.join('%s %.3g' % kv for kv in sorted(errors.items())), 'x 2^-53 S')
    for q, v in errors.items():
        assert v <= 2.0 * bm.BOUNDS_ORACLE_ERR[q][0], (what, q, v)


def test_all_references_compute_within_a_minute():
    """Runs first: every reference, which the later tests then share through the
    per-process cache."""
    t0 = time.perf_counter()
    for name in bm.DIV_CASES:
        bm.div_reference(name)
    for name in bm.MOMENT_CASES:
        bm.moment_reference(name)
    for name in bm.COV_CASES:
        bm.cov_reference(name)
    dt = time.perf_counter() - t0
    print('all %d references: %.1f s' % (len(bm.DIV_CASES + bm.MOMENT_CASES + bm.COV_CASES), dt))
    assert dt < 60.0


@pytest.mark.parametrize('name', bm.DIV_CASES)
def test_div_case_holds_what_it_claims(name):
    bm.check_div_case(name)


@pytest.mark.parametrize('name', bm.MOMENT_CASES)
def test_moment_case_holds_what_it_claims(name):
    bm.check_moment_case(name)


@pytest.mark.parametrize('name', bm.COV_CASES)
def test_cov_case_holds_what_it_claims(name):
    bm.check_cov_case(name)


def test_case_set_covers_the_sizes_and_values():
    sizes = {bm.div_case(n)[0].size for n in bm.DIV_CASES}
    assert sizes >= {1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 65535, 65536, 65537,
                     1024 * 2048 + 257, 1024 * 8192 + 4097}
    for n in sizes:
        for a in (2.0, 1.5):
            assert 'normal_%d_a%g' % (n, a) in bm.DIV_CASES
    for kind in bm.VALUE_KINDS:
        assert '%s_2049' % kind in bm.DIV_CASES and '%s_65537' % kind in bm.BOTH_FORMS
    assert {bm.div_case(n)[1] for n in bm.DIV_CASES} == {2.0, 1.5, 3.0, 1.0001, 50.0}
    assert {bm.COV_SPECS[n][1] for n in bm.COV_CASES} == {1, 2, 3, 63, 64, 65, 66}
    assert {bm.COV_SPECS[n][0] for n in bm.COV_CASES} == {2, 3, 255, 257, 4097}


@pytest.mark.parametrize('name', bm.DIV_CASES)
def test_divergence_stats_match_multiprecision(name):
    _check(_div_errors(name), name)


def test_non_finite_patterns_of_the_oracle():
    """numpy's values for -inf log weights, as the reference states them."""
    for n in (2049, 65537):
        d, lnb, mean_r, se_r, mean_lw, se_lw, top = bo.divergence_stats(
            *bm.div_case('one_ninf_%d' % n))
        assert d == np.inf and lnb == mean_lw == -np.inf and np.isnan(se_lw)
        assert np.isfinite([mean_r, se_r, top]).all() and mean_r > 0
        d, lnb, mean_r, se_r, mean_lw, se_lw, top = bo.divergence_stats(
            *bm.div_case('one_ninf_%d_elbo' % n))
        assert np.isfinite([d, lnb, mean_r, se_r]).all() and mean_lw == -np.inf and np.isnan(se_lw)
        d, lnb, mean_r, se_r, mean_lw, se_lw, top = bo.divergence_stats(
            *bm.div_case('all_ninf_%d' % n))
        assert top == mean_lw == -np.inf and np.isnan([d, mean_r, se_r, se_lw]).all()
    # the reference's statement for +inf and nan entries is numpy's too
    for bad in (np.inf, np.nan):
        lw = np.array([0.1, bad, -0.4])
        ref = bm.div_reference_of(lw, 2.0)
        got = dict(zip(bm.OUT7, bo.divergence_stats(lw, 2.0)))
        for q in bm.QUANTITIES:
            assert bm.err(got[q], *ref[q]) == 0.0, (bad, q)
            assert np.isnan(got[q]) or (q == 'mean_lw' and bad == np.inf and got[q] == np.inf)
    for name in bm.NAN_CASES:
        lw, alpha, elbo = bm.nan_case(name)
        assert np.sum(np.isnan(lw)) == 1 and np.sum(np.isneginf(lw)) == 2
        ref = bm.div_reference_of(lw, alpha)
        got = dict(zip(bm.OUT7, bo.divergence_stats(lw, alpha)))
        assert all(np.isnan(got[q]) and np.isnan(ref[q][0]) for q in bm.QUANTITIES), name
    # ... and the ELBO warning is not raised when se_lw is nan (a comparison with nan)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        lw = np.array([0.1, -np.inf, -0.4, 0.2] * 50)
        with np.errstate(all='ignore'):
            assert bo.mc_mean(lw, 'ELBO') == -np.inf


@pytest.mark.parametrize('name', bm.MOMENT_CASES)
def test_centered_moments_match_multiprecision(name):
    _check(_moment_errors(name), 'moments ' + name)


@pytest.mark.parametrize('name', bm.COV_CASES)
def test_np_cov_matches_multiprecision(name):
    _check(_cov_errors(name), 'cov ' + name)


def test_uniform_weights_equal_the_unweighted_reference():
    x, w, lw, ddof = bm.cov_case('uniform_n255_d2')
    (_, _, _), (hi, lo, S) = bm.cov_reference('uniform_n255_d2')
    (_, _, _), (uhi, ulo, _) = bm._cov_ref(x, None, None, ddof)
    assert np.all(np.abs((hi - uhi) + (lo - ulo)) <= 1e-30 * S)


def test_recorded_figures_are_the_measured_ones():
    """BOUNDS_ORACLE_ERR is the measured worst case and names its case."""
    worst = {q: (0.0, None) for q in bm.BOUNDS_ORACLE_ERR}
    runs = [(n, _div_errors(n)) for n in bm.DIV_CASES]
    runs += [(n, _moment_errors(n)) for n in bm.MOMENT_CASES]
    runs += [(n, _cov_errors(n)) for n in bm.COV_CASES]
    for name, e in runs:
        for q, v in e.items():
            if v > worst[q][0]:
                worst[q] = (v, name)
    print(worst)
    for q, (v, name) in worst.items():
        rec, rec_name = bm.BOUNDS_ORACLE_ERR[q]
        assert 0.5 * rec <= v <= rec * 1.0005 and name == rec_name, (q, v, name)
