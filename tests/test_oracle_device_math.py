"""The measuring stick of tests/test_gpu_device_math.py pinned on the CPU: the
long-double references of exp, expm1, log, log1p, sqrt and the reciprocals agree
with mpmath (40 digits) on 2 000 of each helper's own arguments to 2^-8 of a
double ulp -- the x87 forms are good to a few units of their 64-bit mantissa,
2^-11 double ulps each -- so the stick's error is invisible beside the 1 ulp margin
the GPU test allows."""
import numpy as np
import pytest

from tests import device_math_cases as dm

mpmath = pytest.importorskip('mpmath')
pytestmark = pytest.mark.skipif(not dm.longdouble_ok(), reason='needs a 64-bit-mantissa long double')

MP_FUNCS = {'exp': mpmath.exp, 'expm1': mpmath.expm1, 'log': mpmath.log, 'log1p': mpmath.log1p,
            'sqrt': mpmath.sqrt, 'rcp': lambda x: 1 / x, 'rsqrt': lambda x: 1 / mpmath.sqrt(x)}


@pytest.mark.parametrize('helper', dm.ULP_HELPERS)
def test_longdouble_reference_against_mpmath(helper):
    x, ref = dm.args(helper), dm.reference_ld(helper)
    pick = np.random.RandomState(5).choice(x.size, size=2000, replace=False)
    worst = 0.0
    with mpmath.workdps(40):
        for i in pick:
            exact = MP_FUNCS[dm.LIBRARY[helper]](mpmath.mpf(float(x[i])))
            sp = float(np.spacing(abs(float(ref[i]))))
            # the long double exactly, as a 64-bit integer times a power of two
            m, e = np.frexp(ref[i])
            have = mpmath.ldexp(mpmath.mpf(int(np.ldexp(m, 64))), int(e) - 64)
            err = abs(have - exact) / mpmath.mpf(sp)
            worst = max(worst, float(err))
    print('%s: long double vs mpmath, worst %.2e double ulps' % (helper, worst))
    assert worst <= 2.0 ** -8


def test_argument_sets():
    """Sizes (about 2^18 per ulp-measured helper, at most 2^14 for sin / cos), the
    domains the probe's table forms accept, and the seams that must be present."""
    for h in dm.ULP_HELPERS:
        assert 1 << 17 <= dm.args(h).size <= 5 << 16, (h, dm.args(h).size)
        assert np.all(np.isfinite(dm.reference_ld(h).astype(np.float64)))
    for h in dm.TRIG_HELPERS:
        assert dm.args(h).size <= 1 << 14
    u = dm.args('log_u01_tab')
    assert u.min() == 5e-324 and u.max() == 1.0 - 2.0 ** -53 and 2.0 ** -53 in u
    x = dm.args('sincospi_tab')
    assert x.min() == 0.0 and x.max() == 2.0 and np.all(np.isin(np.arange(257) / 128.0, x))
    b = dm.args('cospi_tab_u24')
    assert np.all((b == np.rint(b)) & (b >= 0) & (b < 2 ** 24))
    e = dm.args('exp_fast')
    assert np.exp(e.min()) < 2.0 ** -1073 and e.max() == dm.EXP_MAX_ARG
    assert np.any(np.exp(e) < 2.0 ** -1022)
    assert dm.args('log_unit').max() > 1e308 and dm.args('log1p_pos_fast').min() == 0.0
