"""The numpy oracle of the mean-field estimators (oracle/vb_oracle.py: Family, the
KLVI / KLVI_PD / CHIVI value and gradient, log_weights, adagrad_optimize's update)
pinned against the 50-digit restatement of tests/mf_mp.py on every case of
tests/mf_cases.py, per class, in units of 2^-53 S (S the condition sum of each
result).  The measured worst errors are recorded as mf_mp.MF_ORACLE_ERR and
asserted at twice the record; the device tests allow 8 times it.  CPU only.

Every case's multiprecision reference is asserted finite here.

The oracle was changed by this file's first run: Family.logdensity of the t family
formed z * z, which overflows from |z| = 1.34e154 on (log q = -inf where the true
value is ~ -(df + 1) 355); it now switches to 2 log|z| - log df + log1p(df / z^2)
above |z| = 2^500 (test_t_logdensity_past_the_overflow_of_z_squared)."""
import numpy as np
import pytest

from tests import mf_cases as mc
from tests import mf_mp as mm

pytestmark = pytest.mark.skipif(not mm.available(), reason='needs mpmath')

CLASSES = ('value', 'mean', 'log_sigma', 'log_q', 'log_w')
CASES = mc.all_cases()
WORST = {}


def _note(cls, err, cid):
    if err > WORST.get(cls, (0.0, ''))[0]:
        WORST[cls] = (float(err), cid)


def oracle_estimate(vo, c):
    fam = vo.Family(c['kind'], c['D'], c['df'])
    a = (fam, c['target'], c['lam'], c['N'])
    with np.errstate(over='ignore', invalid='ignore'):
        if c['objective'] == 'klvi':
            v, g = vo.klvi_value_grad(*a, eps=c['eps'])
        elif c['objective'] == 'klvi_pd':
            v, g = vo.klvi_pd_value_grad(*a, eps=c['eps'])
        else:
            v, g = vo.chivi_value_grad(*a, c['alpha'], eps=c['eps'])
        x, lw = vo.log_weights(*a, eps=c['eps'])
        lq = fam.logdensity(x, c['lam'])
    return v, g, lw, lq, x


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_oracle_matches_multiprecision(c):
    from oracle import vb_oracle as vo
    v, g, lw, lq, x = oracle_estimate(vo, c)
    err = mm.case_errors(c, v, g, lw, (lq, x))
    print('MF_ORACLE %s: %s' % (c['id'], ' '.join('%s %.3f' % kv for kv in err.items())))
    for cls, e in err.items():
        _note(cls, e, c['id'])
        assert e <= 2.0 * mm.MF_ORACLE_ERR[cls], (cls, e)


@pytest.mark.parametrize('W,steps,eps,lr_end', mc.UPDATE_CASES)
def test_oracle_adagrad_update(W, steps, eps, lr_end):
    """Each step of adagrad_optimize on a scripted gradient sequence (entries over
    twelve decades, one exactly 0) against the multiprecision update applied to the
    oracle's own previous lam and the same window."""
    from oracle import vb_oracle as vo
    rs = np.random.RandomState(W * 1000 + steps)
    P = 6
    gs = rs.randn(steps, P) * 10.0 ** rs.randint(-8, 4, size=(steps, P))
    gs[:, 3] = 0.0
    gs[steps // 2, 1] = 0.0
    seen = []

    def obj(lam):
        seen.append(lam.copy())
        return 0.0, gs[len(seen) - 1]
    lam0 = rs.randn(P)
    lam0[0] = 0.0
    res = vo.adagrad_optimize(steps, obj, lam0, window=W, learning_rate=0.01, epsilon=eps,
                              learning_rate_end=lr_end)
    lams = seen + [res[1][-1]]
    lrs = vo.learning_rate_schedule(steps, 0.01, lr_end)
    worst = 0.0
    for i in range(steps):
        ref, _ = mm.adagrad_update(lams[i], gs[max(0, i + 1 - W):i + 1], lrs[i], eps)
        assert mm.finite(ref)
        worst = max(worst, float(mm.units(lams[i + 1], ref).max()))
    # a zero gradient entry leaves lam exactly where it was
    assert np.all(np.array(lams)[:, 3] == lam0[3])
    print('MF_ORACLE adagrad W=%d eps=%g: %.3f' % (W, eps, worst))
    _note('adagrad', worst, 'W%d/eps%g' % (W, eps))
    assert worst <= 2.0 * mm.MF_ORACLE_ERR['adagrad']


@pytest.mark.parametrize('eps', [0.1, 1e-6, 1e-300])
@pytest.mark.parametrize('which', ['rmsprop', 'adam'])
def test_oracle_ia_update(which, eps):
    """The first steps of the oracle's RMSProp-IA / Adam-IA chain (i = 0 is special-cased,
    Adam corrects with the power i + 2) on a scripted gradient sequence, each step
    against the multiprecision update applied to the oracle's own previous lam."""
    from oracle import functions_oracle as fo
    rs = np.random.RandomState(7)
    P, steps = 6, 100   # (the chain's R-hat windows need 100 iterations; the first 10 are checked)
    gs = rs.randn(steps, P) * 10.0 ** rs.randint(-8, 4, size=(steps, P))
    gs[:, 3] = 0.0
    seen = []

    def obj(lam):
        seen.append(lam.copy())
        return 0.0, gs[len(seen) - 1]
    lam0 = rs.randn(P)
    res = fo._ia_optimize(which, steps, obj, lam0, P // 2, learning_rate=0.01, epsilon=eps,
                          rhat_window=50, tail_avg_iters=50)
    lams = seen + [res[0]]
    worst = 0.0
    for i in range(10):
        ref, _ = mm.ia_update(which, lams[i], gs[:i + 1], 0.01, eps)
        assert mm.finite(ref)
        worst = max(worst, float(mm.units(lams[i + 1], ref).max()))
    assert np.all(np.array(lams)[:, 3] == lam0[3])
    print('MF_ORACLE %s eps=%g: %.3f' % (which, eps, worst))
    _note(which, worst, 'eps%g' % eps)
    assert worst <= 2.0 * mm.MF_ORACLE_ERR[which]


@pytest.mark.parametrize('f', mc.family_cases(), ids=[f['id'] for f in mc.family_cases()])
def test_oracle_family_functions(f):
    from oracle import vb_oracle as vo
    fam = vo.Family(f['kind'], f['D'], f['df'])
    lam = f['lam']
    x = fam.transform(lam, f['eps'])
    xr = mm.transform(lam, f['eps'])
    e_x = float(mm.units(x, xr).max())
    e_q = float(mm.units(fam.logdensity(x, lam), mm.logdensity(f['kind'], f['df'], lam, x)).max())
    e_h = float(mm.units(fam.entropy(lam), mm.entropy(f['kind'], lam)))
    e_c = float(mm.units(np.diag(fam.mean_and_cov(lam)[1]),
                         mm.mean_and_cov_diag(f['kind'], f['df'], lam)).max())
    e_m = float(mm.units(fam.pth_moment(2, lam), mm.pth_moment(f['kind'], f['df'], 2, lam)))
    if f['df'] is None or f['df'] > 4:
        e_m = max(e_m, float(mm.units(fam.pth_moment(4, lam),
                                      mm.pth_moment(f['kind'], f['df'], 4, lam))))
    print('MF_ORACLE %s: x %.3f log_q %.3f entropy %.3f cov %.3f moments %.3f'
          % (f['id'], e_x, e_q, e_h, e_c, e_m))
    _note('log_q', e_q, f['id'])
    for cls, e in (('transform', e_x), ('entropy', e_h), ('moments', max(e_c, e_m))):
        _note(cls, e, f['id'])
        assert e <= 2.0 * mm.MF_ORACLE_ERR[cls], (cls, e)
    assert e_q <= 2.0 * mm.MF_ORACLE_ERR['log_q']


@pytest.mark.parametrize('df', [2.000001, 8.0, 1e6])
def test_t_logdensity_past_the_overflow_of_z_squared(df):
    """log sigma = -400 and |x - mu| = z e^-400: log q stays within the log_q bar up
    to |z| = 1e300, on both sides of the overflow of z * z and of the switch at 2^500."""
    from oracle import vb_oracle as vo
    ls = -400.0
    lam = np.array([0.0, ls])
    x = np.array(mc.Z_EDGES)[:, None] * np.exp(ls) * np.array([1.0, -1.0])[None, :]
    x = x.reshape(-1, 1)
    ref = mm.logdensity('t', df, lam, x)
    assert mm.finite(ref)
    e = mm.units(vo.Family('t', 1, df).logdensity(x, lam), ref)
    print('MF_ORACLE z-overflow df=%g: %s' % (df, np.round(e, 3).tolist()))
    assert e.max() <= 2.0 * mm.MF_ORACLE_ERR['log_q']


@pytest.mark.parametrize('objective,kind,df,target,D', [
    ('klvi', 'gauss', None, 'funnel', 3), ('klvi_pd', 't', 5.0, 'mixture', 2),
    ('chivi', 'gauss', None, 'eight_schools_ncp', 10), ('chivi', 't', 2.5, 'funnel', 3),
    ('klvi', 't', 8.0, 'eight_schools_ncp', 10), ('klvi_pd', 'gauss', None, 'isogauss', 2)])
def test_restatement_against_its_own_central_differences(objective, kind, df, target, D):
    """The gradient formulas of mf_mp (the +1 of the log sigma block included) equal
    multiprecision central differences of mf_mp's own value."""
    rs = np.random.RandomState(D)
    lam = np.concatenate([0.3 * rs.randn(D), -0.5 + 0.3 * rs.randn(D)])
    gap = mm.fd_check(objective, kind, df, target, lam, rs.randn(4, D), 1.5)
    assert gap <= 1e-25, gap


def test_recorded_figures_are_the_measured_ones():
    """MF_ORACLE_ERR is the measured worst case (at least half of each record is
    reached); runs after the cases of this file."""
    if not all(cls in WORST for cls in mm.MF_ORACLE_ERR):
        return    # a partial run of this file: nothing to compare
    for cls, rec in mm.MF_ORACLE_ERR.items():
        print('MF_ORACLE record %r: %.2f,' % (cls, WORST[cls][0] + 0.005))
    for cls, rec in mm.MF_ORACLE_ERR.items():
        print('MF_ORACLE worst %s: %.3f at %s (recorded %.3f)' % (cls, *WORST[cls], rec))
        assert WORST[cls][0] >= 0.5 * rec, (cls, WORST[cls])
