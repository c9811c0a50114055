"""vb_psis.hip at small edge shapes, against the 50-digit reference of
tests/psis_mp.py: every case of psis_mp.CASES runs psislw_with_tail and psis_khat
on the device; n2 and the tail order are compared exactly, k, sigma, the
quadrature, the smoothed log weights, gpinv and sumlogs within

    8 x PSIS_ORACLE_ERR[quantity]   in units of 2^-53 S

(the project's margin of a kernel over its restatement), and never looser than the
tolerance tests/test_gpu_bounds_psis.py already uses (psis_mp.device_bound).  The
cases whose tails hold 8192 draws and more (psis_mp.BIG_CASES, GPD_BIG) are not
given to mpmath; they are compared with the numpy oracle at those tolerances.

Each case's data are checked on the host first (psis_mp.check_case: sizes, n2,
the select route the column takes, ties, k on the stated side of 1/3)."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import psis_mp as pm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not pm.available(), reason='needs mpmath')]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _within(quantity, got, hi, lo, S, what):
    e = pm.err(got, hi, lo, S)
    bound = pm.device_bound(quantity, hi, S)
    print('PSIS_EDGE %s %s err %.2f x 2^-53 S (bound %.1f)'
          % (what, quantity, float(np.max(e)), pm.MARGIN * pm.PSIS_ORACLE_ERR[quantity]))
    with np.errstate(invalid='ignore'):
        d = np.abs((np.asarray(got, dtype=float) - hi) - lo)
    bad = ~((d <= bound) | (e == 0))
    assert not np.any(bad), (what, quantity, float(np.max(e)))


@functools.lru_cache(maxsize=None)
def _device(name):
    """One device run of a named case: (out, k, tail)."""
    from viabel_amd import psis
    pm.check_case(name)
    lw, reff = pm.case(name)
    out, k, tails = psis.psislw_with_tail(lw.copy(), Reff=reff)
    return out[:, 0], k[0], tails[0]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import psis_oracle
    lw, reff = pm.case(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out, k, tails = psis_oracle.psislw(lw.copy(), Reff=reff, return_tail=True)
    return out, k, tails[0]


@pytest.mark.parametrize('name', pm.CASES)
def test_psislw_matches_multiprecision(name):
    from viabel_amd import psis
    out, k, tail = _device(name)
    ref = pm.reference(name)
    lw, reff = pm.case(name)
    assert len(tail) == ref.n2
    np.testing.assert_array_equal(tail, ref.tail)
    # psis_khat stops after the fit: the same k, bit for bit
    np.testing.assert_array_equal(np.float64(psis.psis_khat(lw.copy(), Reff=reff)), np.float64(k))
    assert not np.any(np.isnan(out))
    np.testing.assert_array_equal(np.isneginf(out), np.isneginf(ref.lw_hi))
    if np.isinf(ref.k_hi):
        assert k == np.inf
    else:
        _within('k', k, ref.k_hi, ref.k_lo, ref.k_S, name)
        assert (k >= pm.K_MIN) == ref.smoothed        # both take the same branch
    _within('lw', out, ref.lw_hi, ref.lw_lo, ref.lw_S, name)
    if name.startswith('all_equal'):
        np.testing.assert_allclose(out, -np.log(len(lw)), rtol=0, atol=8 * pm.UNIT * np.log(len(lw)))


_CHILD = '''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests import psis_mp as pm
from viabel_amd import psis
res = {}
for name in pm.BOTH_ROUTES:
    lw, reff = pm.case(name)
    out, k, tails = psis.psislw_with_tail(lw.copy(), Reff=reff)
    res[name + '/out'], res[name + '/k'], res[name + '/tail'] = out[:, 0], k, tails[0]
np.savez(sys.argv[2], **res)
'''


@pytest.fixture(scope='module')
def radix_select_run(tmp_path_factory):
    """psis_mp.BOTH_ROUTES in one child process with the fast select switched off
    (VIABEL_AMD_PSIS_FAST_SELECT=0 is read once per process)."""
    f = str(tmp_path_factory.mktemp('psis_routes') / 'radix.npz')
    env = dict(os.environ, VIABEL_AMD_PSIS_FAST_SELECT='0')
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, f], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(f)


@pytest.mark.parametrize('name', pm.BOTH_ROUTES)
def test_both_select_routes_agree_bit_for_bit(name, radix_select_run):
    out, k, tail = _device(name)
    np.testing.assert_array_equal(radix_select_run[name + '/out'], out)
    np.testing.assert_array_equal(radix_select_run[name + '/k'], [k])
    np.testing.assert_array_equal(radix_select_run[name + '/tail'], tail)


@pytest.mark.parametrize('name', pm.BIG_CASES)
def test_large_tails_match_the_oracle(name):
    """Mt = 8192 (the LDS sort at full size), 8193 (the device radix sort, one
    +inf pad slot; with a tie block n2 < Mt and the pads sort behind the tail) and
    the fits of 51 528 / 51 529 draws (256 / 257 quadrature points)."""
    from viabel_amd import psis
    out, k, tail = _device(name)
    oout, ok, otail = _oracle(name)
    lw, reff = pm.case(name)
    assert len(tail) == pm.SHAPES[name][2]
    np.testing.assert_array_equal(tail, otail)
    print('PSIS_EDGE %s k rel err %.3g, lw max err %.3g' % (name, abs(k - ok) / abs(ok),
                                                            np.max(np.abs(out - oout))))
    np.testing.assert_allclose(k, ok, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(out, oout, rtol=1e-11, atol=1e-11)
    np.testing.assert_array_equal(np.float64(psis.psis_khat(lw.copy(), Reff=reff)), np.float64(k))


def _layouts(lw, layout):
    if layout == 'C':
        return np.ascontiguousarray(lw)
    if layout == 'F':
        return np.asfortranarray(lw)
    import torch
    return torch.tensor(lw.T.copy(), dtype=torch.float64, device='cuda').t()


@pytest.mark.parametrize('layout', ['C', 'F', 'device_T'])
def test_mixed_routes_in_one_call(layout):
    """Two columns whose candidates fit the workgroup sort and two whose do not:
    one 0 flag sends the whole call down the radix route, and every column must
    equal its own single-column result (whichever route that took) bit for bit."""
    from viabel_amd import psis
    routes = [pm.ROUTES[n] for n in pm.MIXED]
    assert sorted(routes) == ['fast', 'fast', 'radix', 'radix']
    lw = np.stack([pm.case(n)[0] for n in pm.MIXED], axis=1)
    out, k, tails = psis.psislw_with_tail(_layouts(lw, layout))
    khat = psis.psis_khat(_layouts(lw, layout))
    if layout == 'device_T':
        out = out.cpu().numpy()
    out = np.asarray(out)
    for c, name in enumerate(pm.MIXED):
        sout, sk, stail = _device(name)
        np.testing.assert_array_equal(out[:, c], sout)
        assert k[c] == sk and khat[c] == sk
        np.testing.assert_array_equal(tails[c], stail)


@pytest.mark.parametrize('layout', ['C', 'F'])
def test_column_groups(layout):
    """1500 columns of 40 draws (Mt = 8): more than one scratch group of
    psislw_impl (256 MiB / column stride: 765 columns a group, 739 before the
    quadrature arrays were sized from the tail capacity).  Every column against the
    oracle; the columns on either side of both boundaries, the first and the last
    also against their single-column calls, bit for bit."""
    from viabel_amd import psis
    from oracle import psis_oracle
    n, m = 40, 1500
    rs = np.random.RandomState(97)
    lw = rs.standard_t(3, (n, m)) * (0.5 + rs.uniform(size=m)) + rs.randn(m) * 5
    assert pm.tail_len(n) == 8
    out, k, tails = psis.psislw_with_tail(_layouts(lw, layout))
    out = np.asarray(out)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        oout, ok, otails = psis_oracle.psislw(lw.copy(), return_tail=True)
    np.testing.assert_allclose(k, ok, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(out, oout, rtol=1e-11, atol=1e-11)
    for t, ot in zip(tails, otails):
        np.testing.assert_array_equal(t, ot)
    np.testing.assert_array_equal(psis.psis_khat(_layouts(lw, layout)), k)
    for c in (0, 738, 739, 764, 765, 1499):
        sout, sk, stail = psis.psislw_with_tail(lw[:, c].copy())
        np.testing.assert_array_equal(out[:, c], sout[:, 0])
        assert k[c] == sk[0]
        np.testing.assert_array_equal(tails[c], stail[0])


@pytest.mark.parametrize('name', pm.GPD_CASES)
def test_gpdfitnew_matches_multiprecision(name):
    """n = 2, 3, 5, unsorted input and input with repeated values; the quadrature
    of return_quadrature in length and value."""
    from viabel_amd import psis
    x = pm.gpd_case(name)
    ref = pm.gpd_reference(name)
    if name == 'unsorted_700':
        assert np.any(np.diff(x) < 0)
    if name == 'repeated_700':
        assert len(np.unique(x)) < len(x) // 2
    k, sigma, ks, w = psis.gpdfitnew(x.copy(), return_quadrature=True)
    k2, sigma2 = psis.gpdfitnew(x.copy())
    assert (k2, sigma2) == (k, sigma)
    assert len(ks) == len(w) == len(ref.w_hi)
    _within('k', k, ref.k_hi, ref.k_lo, ref.k_S, 'gpdfit ' + name)
    _within('sigma', sigma, ref.sigma_hi, ref.sigma_lo, ref.sigma_S, 'gpdfit ' + name)
    _within('quad_ks', ks, ref.ks_hi, ref.ks_lo, ref.ks_S, 'gpdfit ' + name)
    _within('quad_w', w, ref.w_hi, ref.w_lo, ref.w_S, 'gpdfit ' + name)
    # sorted input, sort=False: the same fit
    assert psis.gpdfitnew(np.sort(x), sort=False) == (k, sigma)


@pytest.mark.parametrize('name', sorted(pm.GPD_BIG))
def test_gpdfitnew_large_matches_the_oracle(name):
    """n = 8192 / 8193 (LDS sort / device radix sort) and 51 528 / 51 529 values
    (256 / 257 quadrature points: the capacity the arrays used to have, and one
    more)."""
    from viabel_amd import psis
    from oracle import psis_oracle
    x = pm.gpd_case(name)
    n = len(x)
    assert n == pm.GPD_BIG[name][1] and np.any(np.diff(x) < 0)
    if name[0] == 'm':
        assert 30 + int(np.sqrt(n)) == int(name[1:])
    k, sigma, ks, w = psis.gpdfitnew(x.copy(), return_quadrature=True)
    ok, osigma, oks, ow = psis_oracle.gpdfit(x.copy(), return_quadrature=True)
    print('PSIS_EDGE gpdfit %s k rel err %.3g sigma rel err %.3g' % (name, abs(k - ok) / abs(ok),
                                                                 abs(sigma - osigma) / osigma))
    np.testing.assert_allclose([k, sigma], [ok, osigma], rtol=1e-10, atol=1e-12)
    assert len(ks) == len(oks) and len(w) == len(ow)
    np.testing.assert_allclose(ks, oks, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(w, ow, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('k,sigma', pm.GPINV_CASES)
def test_gpinv_matches_multiprecision(k, sigma):
    from viabel_amd import psis
    hi, lo, S = pm.gpinv_ref(pm.GPINV_P, k, sigma)
    got = psis.gpinv(pm.GPINV_P, k, sigma)
    _within('gpinv', got, hi, lo, S, 'gpinv k=%g sigma=%g' % (k, sigma))
    assert got[0] == 0.0 and got[1] == hi[1]            # p = 0, p = 1
    assert np.all(np.isnan(psis.gpinv(pm.GPINV_P, k, -sigma)))


@pytest.mark.parametrize('name', pm.SUMLOGS_CASES)
def test_sumlogs_matches_multiprecision(name):
    from viabel_amd import psis
    x = pm.sumlogs_case(name)
    hi, lo, S = pm.sumlogs_ref(x)
    _within('sumlogs', psis.sumlogs(x.copy()), hi, lo, S, 'sumlogs ' + name)
