"""The numpy restatement of split-chain R-hat (oracle/functions_oracle.py
compute_R_hat), the reference of tests/test_gpu_ia.py, pinned over the edge cases
of tests/rhat_mp.py: var_hat and R-hat stay within twice the recorded
RHAT_ORACLE_ERR of a 50-digit mpmath restatement, in units of 2^-53 S (S as in
tests/rhat_mp.py), with numpy's nan pattern at half-chains of one draw.  CPU only."""
import warnings

import numpy as np
import pytest

from oracle import functions_oracle as fo
from tests import rhat_mp as rm

pytestmark = pytest.mark.skipif(not rm.available(), reason='needs mpmath')


def oracle_rhat(x, s, ln):
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')          # 0 / 0 and 'Mean of empty slice' at h = 1
        return fo.compute_R_hat(x[:, s:s + ln, :], warmup=0)


def _errors(name):
    x, segs = rm.case(name)
    e = {'var_hat': 0.0, 'rhat': 0.0}
    for (s, ln), (vref, rref) in zip(segs, rm.reference(name)):
        var, rhat = oracle_rhat(x, s, ln)
        for q, got, ref in (('var_hat', var, vref), ('rhat', rhat, rref)):
            np.testing.assert_array_equal(np.isnan(got), np.isnan(ref[0]))
            e[q] = max(e[q], float(rm.err(got, *ref).max()))
    return e


@pytest.mark.parametrize('name', rm.CASES)
def test_case_holds_what_it_claims(name):
    rm.check_case(name)


def test_case_set_covers_the_shapes():
    shapes = [rm.case(n)[0].shape for n in rm.CASES]
    assert {s[0] for s in shapes} == {1, 2, 3} and {s[2] for s in shapes} >= {1, 255, 256, 257}
    assert {ln for n in rm.CASES for _, ln in rm.case(n)[1]} >= {2, 4, 6, 64}


@pytest.mark.parametrize('name', rm.CASES)
def test_compute_r_hat_matches_multiprecision(name):
    e = _errors(name)
    print(name, ' '.join('%s %.3g' % kv for kv in sorted(e.items())), 'x 2^-53 S')
    for q, v in e.items():
        assert v <= 2.0 * rm.RHAT_ORACLE_ERR[q][0], (name, q, v)


def test_half_chains_of_one_draw_are_nan():
    """len = 2: ss / (h - 1) = 0 / 0 for every half-chain and the nanmean is empty."""
    for name in ('nc1_len2_K1', 'nc2_len2_K1', 'nc3_len2_K257'):
        x, ((s, ln),) = rm.case(name)
        var, rhat = oracle_rhat(x, s, ln)
        assert np.all(np.isnan(var)) and np.all(np.isnan(rhat))
        assert np.all(np.isnan(rm.reference(name)[0][0][0]))


def test_recorded_figures_are_the_measured_ones():
    worst = {q: (0.0, None) for q in rm.RHAT_ORACLE_ERR}
    for name in rm.CASES:
        for q, v in _errors(name).items():
            if v > worst[q][0]:
                worst[q] = (v, name)
    print(worst)
    for q, (v, name) in worst.items():
        rec, rec_name = rm.RHAT_ORACLE_ERR[q]
        assert 0.5 * rec <= v <= rec * 1.0005 and name == rec_name, (q, v, name)
