"""The oracle of the Philox log-weight draws pinned against the 50-digit restatement of
tests/logw_mp.py, which starts from the draws' integers: the C oracle's libm draws
(oracle/vbrng.c, families 0 and 2), and the numpy oracle's transform and log_weights on
them (oracle/vb_oracle.py), over every case of tests/logw_cases.py, per class, in units
of 2^-53 S.  The measured worst errors are recorded as logw_mp.LOGW_ORACLE_ERR and
asserted at twice the record; the device test allows 8 times the figure.  CPU only.

Every reference is asserted finite, and lies inside every device bar by construction
(it is what the bars are measured from), so no case of tests/test_gpu_logw_edges.py is
there only to be skipped."""
import numpy as np
import pytest

from tests import logw_cases as lc
from tests import logw_mp as lm
from tests import mf_mp as mm

pytestmark = pytest.mark.skipif(not lm.available(), reason='needs mpmath')

WORST = {}


def _note(cls, err, cid):
    if err > WORST.get(cls, (0.0, ''))[0]:
        WORST[cls] = (float(err), cid)


def oracle_errors(c, step):
    from oracle import rng_oracle as ro, vb_oracle as vo
    ref = lm.case_reference(c, step)
    for v in ref:
        assert mm.finite(v), c['id']
    m = c['rows'][step]
    eps = ro.noise(lc.SEED, c['stream'], step, m, c['D'],
                   'gauss' if c['kind'] == 'gauss' else 't_bailey', c['df'] or 0.0)
    with np.errstate(over='ignore', invalid='ignore'):
        x, lw = vo.log_weights(vo.Family(c['kind'], c['D'], c['df']), c['target'], c['lam'], m,
                               eps=eps)
    return {'draw': float(mm.units(eps, ref.eps).max()),
            'sample': float(mm.units(x, ref.x).max()),
            'log_w': float(mm.units(lw, ref.lw_back).max())}


@pytest.mark.parametrize('c', lc.CASES, ids=[c['id'] for c in lc.CASES])
def test_oracle_matches_multiprecision(c):
    for step in sorted(c['rows']):
        err = oracle_errors(c, step)
        print('LOGW_ORACLE %s step %d: %s' % (c['id'], step,
                                              ' '.join('%s %.3f' % kv for kv in err.items())))
        for cls, e in err.items():
            _note(cls, e, c['id'])
            assert e <= 2.0 * lm.LOGW_ORACLE_ERR[cls], (cls, e)


def test_planted_tails_are_where_the_cases_say():
    """Each TAILS entry: the variate's integers are the recorded ones and lie in the
    class's range; the c = 0 hits sit in the last, odd column of their row-kernel case."""
    from oracle import rng_oracle as ro
    odd = 0
    for cls, stream, step, row, pair, cc, a, b in lc.TAILS:
        D = 2 * pair + cc + 1
        ia, ib, _, _ = ro.draw_ints(lc.SEED, stream, step, row + 1, D)
        assert (ia[row, D - 1], ib[row, D - 1]) == (a, b), cls
        assert row < 256 and 2 * pair + cc != 1
        if cls == 'a_lo':
            assert a < 1 << 12
        elif cls == 'a_hi':
            assert a > (1 << 40) - (1 << 12)
        else:
            k = {'b0': 0, 'bq1': 1 << 22, 'bh': 1 << 23, 'bq3': 3 << 22}[cls.rstrip('+-')]
            d = {'+': 1, '-': -1}.get(cls[-1], 0)
            assert b == (k + d) % (1 << 24), cls
        odd += cc == 0 and D % 2 == 1
    assert odd >= 1
    assert {t[0][:2] for t in lc.TAILS} == {'a_', 'b0', 'bq', 'bh'}


def test_recorded_figures_are_the_measured_ones():
    """LOGW_ORACLE_ERR is the measured worst case (at least half of each record is
    reached); runs after the cases of this file."""
    if not all(cls in WORST for cls in lm.LOGW_ORACLE_ERR):
        return    # a partial run of this file: nothing to compare
    for cls in lm.LOGW_ORACLE_ERR:
        print('LOGW_ORACLE record %r: %.2f,' % (cls, WORST[cls][0] + 0.005))
    for cls, rec in lm.LOGW_ORACLE_ERR.items():
        print('LOGW_ORACLE worst %s: %.3f at %s (recorded %.3f)' % (cls, *WORST[cls], rec))
        assert WORST[cls][0] >= 0.5 * rec, (cls, WORST[cls])
