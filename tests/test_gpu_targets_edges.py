"""The target kernels away from the origin.

Part 1: every direct target kernel (vb_target_logdensity: target_row_kernel at
DMAX 16, target_sep_kernel, funnel_wide_kernel and the row-block kernels from
D = 512) over the edge point set of tests/targets_mp.py, against the 50-digit
reference, value and every gradient entry within 8 x ORACLE_ERR[target] in units
of 2^-53 S (S the condition sum of the result).  The factor 8 over the double
oracle's own error: the device helpers are ~1 ulp forms where libm is ~0.5,
compile-time-rounded reciprocals replace divisions, and the wave / block trees
sum in another order.

Part 2: the other written forms of the same targets (the log-weight kernels, the
block kernel's row / row_half instances, the column-pair kernel, the materialised
path) at off-centre variational parameters, against oracle.vb_oracle on identical
numpy-stream draws with the suite's tolerances: single calls 1e-10 of the largest
entry, log weights rtol = atol = 1e-11, trajectories 1e-7.  The numpy oracle these
rest on is pinned off-centre by tests/test_oracle_targets_mp.py.

Measured worst errors of part 1 on MI355X (units of 2^-53 S; bound in brackets)
are in DESIGN.md §2.
"""
import numpy as np
import pytest

from tests import targets_mp as tm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not tm.available(), reason='needs mpmath')]

MARGIN = 8.0


def _mods():
    from viabel_amd import vb, targets, experiments
    from oracle import vb_oracle
    return vb, targets, experiments, vb_oracle


def _target(targets, name, D):
    return {'isogauss': lambda: targets.isogauss(D), 'mixture': lambda: targets.mixture(D),
            'funnel': lambda: targets.funnel(D),
            'eight_schools_ncp': targets.eight_schools_ncp}[name]()


def _family(vb, kind, df, D):
    if kind == 'gauss':
        return vb.mean_field_gaussian_variational_family(D, rng='numpy')
    return vb.mean_field_t_variational_family(D, df, rng='numpy')


def _close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.isfinite(b)), 'oracle not finite'
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b))) / scale
    assert err <= tol, 'max scaled error %.3e > %.1e' % (err, tol)


# ---- part 1: the direct kernels at the edge set --------------------------------
@pytest.mark.parametrize('target,D', tm.CASES)
def test_direct_kernel_at_edge_points(target, D):
    _, targets, _, _ = _mods()
    x, ref = tm.edge_reference(target, D)
    lp, g = _target(targets, target, D).logdensity_and_grad(np.array(x))
    e_lp, e_g = tm.errors(lp, g, ref)
    r, (gr, gc) = int(np.argmax(e_lp)), np.unravel_index(int(np.argmax(e_g)), e_g.shape)
    bound = MARGIN * tm.ORACLE_ERR[target]
    print('EDGE %s D=%d: value %.3f (row %d, x[:2] = %r), gradient %.3f (row %d, column %d, '
          'x[:2] = %r); bound %.2f x 2^-53 S'
          % (target, D, e_lp[r], r, x[r, :2].tolist(), e_g[gr, gc], gr, gc, x[gr, :2].tolist(),
             bound))
    assert e_lp[r] <= bound
    assert e_g[gr, gc] <= bound


def _switch_lam(log_tau, mu):
    """q concentrated on one switch row with theta_tilde ~ 1e-174 (log sigma = -400:
    tau theta_tilde vanishes beside y - mu), so that log1p(w) ~ 700 is a leading term
    of every log weight; log tau stays on its side of the switch (sigma = e^-12)."""
    mean = np.zeros(10)
    mean[0], mean[1] = mu, log_tau
    ls = np.full(10, -400.0)
    ls[0], ls[1] = -3.0, -12.0
    return np.concatenate([mean, ls])


@pytest.mark.parametrize('log_tau', tm.ES_SWITCH)
def test_eight_schools_both_sides_of_the_lp_tab_switch(log_tau):
    """EightSchools::lp_tab takes the table log1p below w = (tau / 5)^2 = 2^1000 and
    the library's above; ::row uses the library's on both sides.  Beside the switch
    both agree with the references: row with the multiprecision one at the switch
    rows (theta_tilde = 0, where log1p is not drowned by tau^2), the log weights with
    the oracle's."""
    vb, targets, experiments, vo = _mods()
    tgt = targets.eight_schools_ncp()
    rows = tm.es_switch_rows()
    rows = rows[rows[:, 1] == log_tau]
    assert len(rows) == 4
    ref = tm.reference('eight_schools_ncp', rows)
    lp, g = tgt.logdensity_and_grad(rows)
    e_lp, e_g = tm.errors(lp, g, ref)
    bound = MARGIN * tm.ORACLE_ERR['eight_schools_ncp']
    print('SWITCH row log tau %.1f: value %.3f gradient %.3f; bound %.2f'
          % (log_tau, e_lp.max(), e_g.max(), bound))
    assert e_lp.max() <= bound and e_g.max() <= bound
    w_side = (np.exp(log_tau) * 0.2) ** 2 < 2.0 ** 1000
    for mu in (0.0, 30.0):
        lam = _switch_lam(log_tau, mu)
        fam, ofam = _family(vb, 'gauss', None, 10), vo.Family('gauss', 10)
        x, lw = experiments.log_weights(tgt, fam, lam, 2000)
        ox, olw = vo.log_weights(ofam, 'eight_schools_ncp', lam, 2000)
        assert np.all(((np.exp(ox[:, 1]) * 0.2) ** 2 < 2.0 ** 1000) == w_side)
        np.testing.assert_allclose(x, ox, rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(lw, olw, rtol=1e-11, atol=1e-11)
        # and against the multiprecision log p at the drawn rows
        sub = ox[:64]
        mref = tm.reference('eight_schools_ncp', sub)
        lq = ofam.logdensity(sub, lam)
        err = np.abs(((lw[:64] + lq) - mref.lp_hi) - mref.lp_lo) / (tm.UNIT * (mref.lp_S + np.abs(lq)))
        assert err.max() <= bound, err.max()


# ---- part 2: off-centre variational parameters -------------------------------
FAMS = [('gauss', None), ('t', 8.0)]
LOG_SIGMAS = [-3.0, -0.2]
# start points: the means of q sit at a subset of the edge centres
STARTS = {
    'mixture': ['mean0', 'mean+10', 'mean-10'],
    'funnel': ['x1-6', 'x1+5'],
    'eight_schools_ncp': ['logtau-8_mu30', 'logtau+4_mu30'],
}
ALL_STARTS = [(t, s) for t in STARTS for s in STARTS[t]]


def hash_name(s):
    """A process-independent hash of a start's name (str hashes are salted)."""
    h = 0
    for ch in s.encode():
        h = (h * 131 + ch) % 1000003
    return h


def start_lam(target, start, D, log_sigma):
    """The named off-centre start: [means, log sigmas]."""
    rs = np.random.RandomState(hash_name(start))
    if target == 'mixture':
        mean = np.full(D, {'mean0': 0.0, 'mean+10': 10.0, 'mean-10': -10.0}[start])
    elif target == 'funnel':
        mean = 0.3 * rs.randn(D)
        mean[1] = {'x1-6': -6.0, 'x1+5': 5.0}[start]
    else:
        mean = 0.3 * rs.randn(D)
        mean[0] = 30.0
        mean[1] = {'logtau-8_mu30': -8.0, 'logtau+4_mu30': 4.0}[start]
    return np.concatenate([mean, np.full(D, log_sigma)])


LOGW_CASES = [('eight_schools_ncp', 10), ('funnel', 10), ('funnel', 40), ('mixture', 2),
              ('mixture', 40)]


@pytest.mark.parametrize('kind,df', FAMS)
@pytest.mark.parametrize('log_sigma', LOG_SIGMAS)
@pytest.mark.parametrize('target,D,start', [(t, D, s) for t, D in LOGW_CASES for s in STARTS[t]])
def test_log_weights_off_centre(kind, df, log_sigma, target, D, start):
    """8-schools reaches lp_tab and log1p_pos_tab, the funnel its row (D = 10) and
    wide (D = 40) forms, the mixture logw_row_kernel (D = 2) and logw_sep_kernel."""
    vb, targets, experiments, vo = _mods()
    fam, ofam = _family(vb, kind, df, D), vo.Family(kind, D, df)
    lam = start_lam(target, start, D, log_sigma)
    x, lw = experiments.log_weights(_target(targets, target, D), fam, lam, 2000)
    ox, olw = vo.log_weights(ofam, target, lam, 2000)
    assert np.all(np.isfinite(olw))
    np.testing.assert_allclose(x, ox, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(lw, olw, rtol=1e-11, atol=1e-11)


def _value_grad(vb, vo, objective, fam, ofam, tgt, target, lam, N):
    if objective == 'klvi':
        v, g = vb.black_box_klvi(fam, tgt, N)(lam)
        ov, og = vo.klvi_value_grad(ofam, target, lam, N)
    else:
        np.random.seed(31)
        v, g = vb.black_box_chivi(2.0, fam, tgt, N)(lam)
        np.random.seed(31)
        ov, og = vo.chivi_value_grad(ofam, target, lam, N, 2.0)
    return v, g, ov, og


# block kernel (D <= 16; N = 100 and 300: the overlapped and the chunked layout),
# column-pair kernel (separable, D = 64), materialised path (funnel D = 40; the
# mixture at D = 600 under CHIVI)
CALL_CASES = ([(t, D, N, o) for t, D in [('mixture', 2), ('funnel', 10), ('eight_schools_ncp', 10),
                                          ('funnel', 16)]
               for N in (100, 300) for o in ('klvi', 'chivi')]
              + [('mixture', 64, 128, 'klvi'), ('mixture', 64, 128, 'chivi'),
                 ('funnel', 40, 128, 'klvi'), ('funnel', 40, 128, 'chivi'),
                 ('mixture', 600, 128, 'chivi')])


@pytest.mark.parametrize('kind,df', FAMS)
@pytest.mark.parametrize('log_sigma', LOG_SIGMAS)
@pytest.mark.parametrize('target,D,N,objective,start',
                         [(t, D, N, o, s) for t, D, N, o in CALL_CASES for s in STARTS[t]])
def test_value_and_gradient_off_centre(kind, df, log_sigma, target, D, N, objective, start):
    vb, targets, _, vo = _mods()
    fam, ofam = _family(vb, kind, df, D), vo.Family(kind, D, df)
    lam = start_lam(target, start, D, log_sigma)
    v, g, ov, og = _value_grad(vb, vo, objective, fam, ofam, _target(targets, target, D), target,
                               lam, N)
    assert np.isfinite(ov) and np.all(np.isfinite(og))
    assert abs(v - ov) <= 1e-10 * max(1.0, abs(ov)), (v, ov)
    _close(g, og, 1e-10)


RUN_CASES = [('funnel', 10), ('eight_schools_ncp', 10), ('mixture', 2)]
RUN_STEPS, RUN_N, RUN_LR = 20, 128, 0.05


def oracle_run(vo, kind, df, target, D, objective, lam0, nudge=False):
    """The oracle's 20 adagrad steps from lam0 (CHIVI seeds from np.random.seed(4)).
    nudge: every draw moved by one ulp -- the conditioning probe of a start point
    (tests/test_oracle_targets_mp.py keeps the committed starts well conditioned)."""
    ofam = vo.Family(kind, D, df)
    draw = ofam.draw
    if nudge:
        ofam.draw = lambda n, seed=None: np.nextafter(draw(n, seed), np.inf)
    if objective == 'klvi':
        fn = lambda lam: vo.klvi_value_grad(ofam, target, lam, RUN_N)
    else:
        fn = lambda lam: vo.chivi_value_grad(ofam, target, lam, RUN_N, 2.0)
    np.random.seed(4)
    return vo.adagrad_optimize(RUN_STEPS, fn, lam0, learning_rate=RUN_LR)


@pytest.mark.parametrize('kind,df', FAMS)
@pytest.mark.parametrize('log_sigma', LOG_SIGMAS)
@pytest.mark.parametrize('objective', ['klvi', 'chivi'])
@pytest.mark.parametrize('target,D,start', [(t, D, s) for t, D in RUN_CASES for s in STARTS[t]])
def test_short_run_off_centre(kind, df, log_sigma, objective, target, D, start):
    """20 adagrad steps at N = 128 (the split-row instances: row_half, lane_const,
    the hot KLVI and CHIVI instances) from the off-centre start."""
    vb, targets, _, vo = _mods()
    fam = _family(vb, kind, df, D)
    tgt = _target(targets, target, D)
    lam0 = start_lam(target, start, D, log_sigma)
    obj = (vb.black_box_klvi(fam, tgt, RUN_N) if objective == 'klvi'
           else vb.black_box_chivi(2.0, fam, tgt, RUN_N))
    np.random.seed(4)
    res = vb.adagrad_optimize(RUN_STEPS, obj, lam0, learning_rate=RUN_LR)
    ores = oracle_run(vo, kind, df, target, D, objective, lam0)
    _close(res[2], ores[2], 1e-7)
    _close(res[1], ores[1], 1e-7)
