"""vb_bounds.hip at edge shapes, against the 50-digit reference of
tests/bounds_mp.py: every case of bounds_mp.DIV_CASES, MOMENT_CASES and COV_CASES
runs on the device; log max, the non-finite patterns and the zeros of a constant
vector are compared exactly, everything else within

    8 x BOUNDS_ORACLE_ERR[quantity]   in units of 2^-53 S

(the project's margin of a kernel over its restatement), and never looser than the
tolerance tests/test_gpu_bounds_psis.py and tests/test_gpu_switches.py already use
(bounds_mp.device_bound).  Each case's data are checked on the host first
(bounds_mp.check_*_case: which side of a constant the size sits on, the form or
path taken, what the values are named for)."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import bounds_mp as bm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not bm.available(), reason='needs mpmath')]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _within(quantity, got, hi, lo, S, what):
    e = bm.err(got, hi, lo, S)
    bound = bm.device_bound(quantity, hi, S)
    print('BOUNDS_EDGE %s %s err %.3g x 2^-53 S (bound %.1f)'
          % (what, quantity, float(np.max(e)), bm.MARGIN * bm.BOUNDS_ORACLE_ERR[quantity][0]))
    with np.errstate(invalid='ignore'):
        d = np.abs((np.asarray(got, dtype=float) - hi) - lo)
    bad = ~((d <= bound) | (e == 0))
    assert not np.any(bad), (what, quantity, float(np.max(e)))


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _compare7(out, ref, elbo, what):
    """One out7 (d_alpha, lnb, mean_r, se_r, mean_lw, se_lw, log max) against the
    reference of its log weights."""
    got = dict(zip(bm.OUT7, out))
    assert _same(got['max'], ref['max'][0]), (what, got['max'])
    if elbo is None:
        assert _same(got['lnb'], got['mean_lw'])
    else:
        assert got['lnb'] == elbo and np.isnan(got['se_lw'])     # not computed with a bound given
    for q in bm.QUANTITIES:
        if q == 'se_lw' and elbo is not None:
            continue
        hi, lo, S = ref[q]
        if not np.isfinite(hi):
            assert _same(got[q], hi), (what, q, got[q], hi)
            print('BOUNDS_EDGE %s %s %r as the reference' % (what, q, got[q]))
        else:
            _within(q, got[q], hi, lo, S, what)


@functools.lru_cache(maxsize=None)
def _device(name):
    from viabel_amd import bounds
    bm.check_div_case(name)
    lw, alpha, elbo = bm.div_case(name)
    return bounds._device_divergence(lw.copy(), alpha, elbo)


@pytest.mark.parametrize('name', bm.DIV_CASES)
def test_divergence_matches_multiprecision(name):
    from viabel_amd import bounds
    lw, alpha, elbo = bm.div_case(name)
    out = _device(name)
    ref = bm.div_reference(name)
    _compare7(out, ref, elbo, name)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        d, lnb = bounds.divergence_bound(lw.copy(), alpha=alpha, log_norm_bound=elbo,
                                         return_log_norm_bound=True)
    assert _same(d, out[0]) and _same(lnb, out[1])
    texts = [str(w.message) for w in caught]
    # bounds.py:183-192 on the reference's values: warned exactly when s > 0.01 holds
    # (a comparison with nan is false); asserted where s is well clear of 0.01
    for tag, q in (('CUBO', 'se_r'), ('ELBO', 'se_lw')):
        if tag == 'ELBO' and elbo is not None:
            assert not any('ELBO' in t for t in texts)
            continue
        s = ref[q][0]
        if np.isnan(s) or abs(s - 0.01) > 1e-3:
            assert any(tag in t for t in texts) == bool(s > 0.01), (name, tag, s, texts)
    kind = name.rsplit('_', 1)[0]
    if kind in ('const', 'const_inexact'):
        assert out[3] == 0.0 and out[2] == 1.0
    if kind == 'const':
        assert out[5] == 0.0 and out[4] == lw[0]


_CHILD = '''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests import bounds_mp as bm
from viabel_amd import bounds
res = {}
for name in bm.BOTH_FORMS + bm.FORM_EDGE:
    lw, alpha, elbo = bm.div_case(name)
    res[name] = bounds._device_divergence(lw.copy(), alpha, elbo)
for name in bm.NAN_CASES:
    lw, alpha, elbo = bm.nan_case(name)
    res[name] = bounds._device_divergence(lw.copy(), alpha, elbo)
np.savez(sys.argv[2], **res)
'''


@pytest.fixture(scope='module')
def three_pass_run(tmp_path_factory):
    """bounds_mp.BOTH_FORMS in one child process with the Welford form switched off
    (VIABEL_AMD_DIV_TWO_PASS=0 is read once per process)."""
    f = str(tmp_path_factory.mktemp('div_forms') / 'three_pass.npz')
    env = dict(os.environ, VIABEL_AMD_DIV_TWO_PASS='0')
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, f], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(f)


@pytest.mark.parametrize('name', bm.BOTH_FORMS)
def test_both_forms_match_multiprecision(name, three_pass_run):
    """From 2^16 draws on: the three-pass form held to the same bound as the Welford
    form, and the same non-finite pattern from both."""
    lw, alpha, elbo = bm.div_case(name)
    three = three_pass_run[name]
    _compare7(three, bm.div_reference(name), elbo, name + ' three-pass')
    two = _device(name)
    np.testing.assert_array_equal(np.isnan(two), np.isnan(three))
    np.testing.assert_array_equal(np.isinf(two), np.isinf(three))


def test_the_form_changes_at_two_to_the_sixteen(three_pass_run):
    """65535 draws: the default is the three-pass form (the bits of the run with the
    Welford form switched off).  65536 draws: it is not (different last bits)."""
    for name in bm.FORM_EDGE:
        assert bm.div_case(name)[0].size == bm.DIV_TWO_PASS_MIN_N - 1
        np.testing.assert_array_equal(three_pass_run[name], _device(name))
    for name in ('normal_65536_a2',):            # (65536 distinct draws)
        assert bm.div_case(name)[0].size == bm.DIV_TWO_PASS_MIN_N
        assert not np.array_equal(three_pass_run[name], _device(name)), name


@pytest.mark.parametrize('name', bm.NAN_CASES)
def test_nan_beside_neg_inf_is_nan_in_both_forms(name, three_pass_run):
    """numpy's nan for every statistic; not the -inf of a vector that holds -inf
    alone."""
    from viabel_amd import bounds
    lw, alpha, elbo = bm.nan_case(name)
    assert (lw.size >= bm.DIV_TWO_PASS_MIN_N) == name.endswith('65537')
    ref = bm.div_reference_of(lw, alpha)
    for tag, out in (('welford/default', bounds._device_divergence(lw.copy(), alpha, None)),
                     ('three-pass', three_pass_run[name])):
        got = dict(zip(bm.OUT7, out))
        for q in bm.QUANTITIES:
            assert np.isnan(ref[q][0]) and np.isnan(got[q]), (name, tag, q, got[q])


@functools.lru_cache(maxsize=None)
def _rows(n):
    names = ('normal_%d_a2' % n, 't_%d' % n, 'off1e6_%d' % n)
    rows = np.stack([bm.div_case(k)[0] for k in names])
    assert rows.shape == (3, n)
    return rows


@functools.lru_cache(maxsize=None)
def _row_reference(n, r, alpha):
    return bm.div_reference_of(_rows(n)[r], alpha)


@pytest.mark.parametrize('alpha', [2.0, 1.5])
@pytest.mark.parametrize('n', [bm.SMALL_SIDE, bm.BIG_SIDE])
@pytest.mark.parametrize('where', ['device_slice', 'host'])
def test_divergence_rows_strided(where, n, alpha):
    """Three rows in one launch chain; on the device a slice t[:, :n] of a
    [3, n + 5] tensor (ld = n + 5) whose padding holds +inf."""
    import torch
    from viabel_amd import bounds
    assert (n >= bm.DIV_TWO_PASS_MIN_N) == (n == bm.BIG_SIDE)
    rows = _rows(n)
    if where == 'device_slice':
        t = torch.full((3, n + 5), float('inf'), dtype=torch.float64, device='cuda')
        t[:, :n] = torch.tensor(rows)
        arg = t[:, :n]
        assert arg.stride() == (n + 5, 1)
    else:
        arg = rows.copy()
    out = bounds.divergence_rows(arg, alpha=alpha)
    assert out.shape == (3, 7)
    for r in range(3):
        single = bounds._device_divergence(rows[r].copy(), alpha, None)
        np.testing.assert_array_equal(out[r], single)
        _compare7(out[r], _row_reference(n, r, alpha), None, 'rows %s n=%d row %d' % (where, n, r))


@pytest.mark.parametrize('name', ['off1e8_2049', 'off1e8_65537', 'off1e6_2049', 'off1e6_65537',
                                  'off700_2049', 'off700_65537'])
def test_mean_and_check_mc_error_on_offsets(name):
    from viabel_amd import bounds
    lw = bm.div_case(name)[0]
    ref = bm.div_reference(name)
    s, _, S = ref['se_lw']
    width = float(bm.device_bound('se_lw', s, S))
    for atol, warns in ((2.0 * s, False), (0.5 * s, True)):
        assert abs(s - atol) >= 100.0 * width and (s > atol) == warns
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            m = bounds.mean_and_check_mc_error(lw.copy(), atol=atol, quantity_name='offset')
        assert bool(caught) == warns, (name, atol, [str(w.message) for w in caught])
        _within('mean_lw', m, *ref['mean_lw'], what='mc_error ' + name)


def _centered_moments(x):
    from viabel_amd import _native as nat
    c2, c4 = np.empty(1), np.empty(1)
    nat.check(nat.lib().vb_centered_moments(nat.context().handle, nat.dptr(x), x.shape[0],
                                            x.shape[1], nat.dptr(c2), nat.dptr(c4)))
    return c2[0], c4[0]


@pytest.mark.parametrize('name', bm.MOMENT_CASES)
def test_centered_moments_match_multiprecision(name):
    from viabel_amd import bounds
    bm.check_moment_case(name)
    x = bm.moment_case(name)
    ref = bm.moment_reference(name)
    c2, c4 = _centered_moments(np.ascontiguousarray(x))
    _within(bm.moment_quantity(name, 2), c2, *ref['c2'], what='moments ' + name)
    _within(bm.moment_quantity(name, 4), c4, *ref['c4'], what='moments ' + name)
    # wasserstein_bounds (bounds.py:103-139) is scalar algebra on the same two values
    res = bounds.wasserstein_bounds(0.3, x.copy())
    assert res['W1'] == 2 * c2 ** .5 * np.expm1(0.3) ** .5
    assert res['W2'] == 2 * c4 ** .25 * np.expm1(0.3) ** .25


@functools.lru_cache(maxsize=None)
def _device_cov(name):
    from viabel_amd import experiments
    bm.check_cov_case(name)
    x, w, lw, ddof = bm.cov_case(name)
    return experiments.weighted_mean_and_cov(x.copy(), weights=None if w is None else w.copy(),
                                             ddof=ddof,
                                             log_weights=None if lw is None else lw.copy())


@pytest.mark.parametrize('name', bm.COV_CASES)
def test_covariance_matches_multiprecision(name):
    from viabel_amd import bounds
    x, w, lw, ddof = bm.cov_case(name)
    (m_hi, m_lo, m_S), (hi, lo, S) = bm.cov_reference(name)
    mean, cov = _device_cov(name)
    np.testing.assert_array_equal(cov, cov.T)
    _within('mean_w', mean, m_hi, m_lo, m_S, 'cov ' + name)
    if np.all(np.isnan(hi)):
        assert np.all(np.isnan(cov)), name        # numpy's pattern of a zero normaliser
    else:
        _within('cov', cov, hi, lo, S, 'cov ' + name)
    if w is None and lw is None and ddof == 1:
        sc = bounds._sample_cov(x.copy())
        np.testing.assert_array_equal(sc, sc.T)
        _within('cov', sc, hi, lo, S, 'sample_cov ' + name)
        if 2 <= x.shape[1] <= bm.COV_D_MAX:
            # from d = 2 (d = 1 has a mean kernel of its own) up to d = 64 both entry
            # points run the column-sum and pair kernels: the same bits
            np.testing.assert_array_equal(sc, cov)


def test_pair_path_and_gemm_path_agree_on_a_shared_block():
    """d = 64 (2080 pairs) and d = 65 (MFMA GEMM) on the same 257 rows."""
    a, b = bm.PREFIX_PAIR
    (_, _, _), (hi, lo, S) = bm.cov_reference(a)
    c64, c65 = _device_cov(a)[1], _device_cov(b)[1]
    bound = bm.device_bound('cov', hi, S)
    d = np.abs(c64 - c65[:64, :64])
    print('BOUNDS_EDGE pairs against gemm: %.3g x 2^-53 S' % float(np.max(d / (bm.UNIT * S))))
    assert np.all(d <= bound)


def test_all_neg_inf_log_weights_sum_to_zero():
    from viabel_amd import experiments
    x = bm.cov_case('n3_d2')[0]
    with pytest.raises(ValueError, match='weights sum to zero'):
        experiments.weighted_mean_and_cov(x.copy(), log_weights=np.full(3, -np.inf), ddof=0)
    with pytest.raises(ValueError, match='weights sum to zero'):
        experiments.weighted_mean_and_cov(x.copy(), weights=np.zeros(3), ddof=0)
