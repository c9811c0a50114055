"""The numpy restatement of PSIS (oracle/psis_oracle.py), the reference of
tests/test_gpu_bounds_psis.py, pinned over the edge cases of tests/psis_mp.py:
k, sigma, the smoothed log weights, the quadrature, gpinv and sumlogs stay within
twice the recorded PSIS_ORACLE_ERR of a 50-digit mpmath restatement, in units of
2^-53 S (S as in tests/psis_mp.py).  CPU only.

Where the oracle's np.argsort orders equal tail values differently from the
reference's index rule (psis_mp.TIED_TAILS), the smoothed weights are the same
set of numbers placed on different members of the tie: they are compared as
sorted multisets."""
import time
import warnings

import numpy as np
import pytest

from oracle import psis_oracle as po
from tests import psis_mp as pm

pytestmark = pytest.mark.skipif(not pm.available(), reason='needs mpmath')


def _psislw_errors(name):
    lw, reff = pm.case(name)
    ref = pm.reference(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out, k, tails = po.psislw(lw.copy(), Reff=reff, return_tail=True)
    assert len(tails[0]) == ref.n2
    e = {'k': float(pm.err(k, ref.k_hi, ref.k_lo, ref.k_S))}
    if ref.n2 > 4:
        # sigma as psislw forms it: the fit of y = exp(tail) - exp(cutoff)
        x, cut, order = pm.shifted_tail(lw, reff)
        sigma = po.gpdfit(np.exp(x[order]) - np.exp(cut), order=np.arange(ref.n2))[1]
        e['sigma'] = float(pm.err(sigma, ref.sigma_hi, ref.sigma_lo, ref.sigma_S))
    assert np.array_equal(np.isneginf(out), np.isneginf(ref.lw_hi)) and not np.any(np.isnan(out))
    if np.array_equal(tails[0], ref.tail) or not ref.smoothed:
        e['lw'] = float(pm.err(out, ref.lw_hi, ref.lw_lo, ref.lw_S).max())
    else:
        assert name in pm.TIED_TAILS
        o = np.argsort(ref.lw_hi, kind='stable')
        e['lw'] = float(pm.err(np.sort(out), ref.lw_hi[o], ref.lw_lo[o], ref.lw_S[o]).max())
    return e


def _gpdfit_errors(name):
    x = pm.gpd_case(name)
    ref = pm.gpd_reference(name)
    k, sigma, ks, w = po.gpdfit(x.copy(), return_quadrature=True)
    assert len(ks) == len(w) == len(ref.ks_hi) == len(ref.w_hi)
    return {'k': float(pm.err(k, ref.k_hi, ref.k_lo, ref.k_S)),
            'sigma': float(pm.err(sigma, ref.sigma_hi, ref.sigma_lo, ref.sigma_S)),
            'quad_ks': float(pm.err(ks, ref.ks_hi, ref.ks_lo, ref.ks_S).max()),
            'quad_w': float(pm.err(w, ref.w_hi, ref.w_lo, ref.w_S).max())}


def _gpinv_error(k, sigma):
    hi, lo, S = pm.gpinv_ref(pm.GPINV_P, k, sigma)
    got = po.gpinv(pm.GPINV_P, k, sigma)
    assert got[0] == 0.0 and got[1] == hi[1]            # p = 0, p = 1: exact
    return float(pm.err(got, hi, lo, S).max())


def _sumlogs_error(name):
    x = pm.sumlogs_case(name)
    return float(pm.err(po.sumlogs(x), *pm.sumlogs_ref(x)))


def _check(errors, what):
    print(what, ' '.join('%s %.2f' % kv for kv in sorted(errors.items())), 'x 2^-53 S')
    for q, v in errors.items():
        assert v <= 2.0 * pm.PSIS_ORACLE_ERR[q], (what, q, v)


def test_all_references_compute_within_a_minute():
    """Runs first: every reference, which the later tests and the GPU tests then
    share through the per-process cache."""
    t0 = time.perf_counter()
    for name in pm.CASES:
        pm.reference(name)
    for name in pm.GPD_CASES:
        pm.gpd_reference(name)
    dt = time.perf_counter() - t0
    print('all %d references: %.1f s' % (len(pm.CASES) + len(pm.GPD_CASES), dt))
    assert dt < 60.0


@pytest.mark.parametrize('name', pm.CASES + pm.BIG_CASES)
def test_case_holds_what_it_claims(name):
    pm.check_case(name)


@pytest.mark.parametrize('name', pm.CASES)
def test_psislw_matches_multiprecision(name):
    _check(_psislw_errors(name), name)


@pytest.mark.parametrize('name', pm.GPD_CASES)
def test_gpdfit_matches_multiprecision(name):
    _check(_gpdfit_errors(name), 'gpdfit ' + name)


@pytest.mark.parametrize('k,sigma', pm.GPINV_CASES)
def test_gpinv_matches_multiprecision(k, sigma):
    _check({'gpinv': _gpinv_error(k, sigma)}, 'gpinv k=%g sigma=%g' % (k, sigma))


def test_gpinv_nonpositive_sigma_is_nan():
    assert np.all(np.isnan(po.gpinv(pm.GPINV_P, 0.2, -1.0)))
    assert np.all(np.isnan(pm.gpinv_ref(pm.GPINV_P, 0.2, -1.0)[0]))


@pytest.mark.parametrize('name', pm.SUMLOGS_CASES)
def test_sumlogs_matches_multiprecision(name):
    _check({'sumlogs': _sumlogs_error(name)}, 'sumlogs ' + name)


def test_recorded_figures_are_the_measured_ones():
    """PSIS_ORACLE_ERR is the measured worst case, not a loose cap."""
    worst = {q: 0.0 for q in pm.PSIS_ORACLE_ERR}
    runs = [_psislw_errors(n) for n in pm.CASES] + [_gpdfit_errors(n) for n in pm.GPD_CASES]
    runs += [{'gpinv': _gpinv_error(k, s)} for k, s in pm.GPINV_CASES]
    runs += [{'sumlogs': _sumlogs_error(n)} for n in pm.SUMLOGS_CASES]
    for e in runs:
        for q, v in e.items():
            worst[q] = max(worst[q], v)
    print(worst)
    for q, v in worst.items():
        assert 0.5 * pm.PSIS_ORACLE_ERR[q] <= v <= pm.PSIS_ORACLE_ERR[q] * 1.0005, (q, v)
