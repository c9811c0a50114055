"""The numpy oracle of the four built-in targets (oracle/targets_oracle.py), the
reference of every GPU target test, pinned off-centre: over the whole edge point
set of tests/targets_mp.py its values and gradients stay within twice the recorded
ORACLE_ERR[target] of a 50-digit mpmath restatement, in units of 2^-53 S (S the
condition sum of the result; see tests/targets_mp.py).  CPU only."""
import numpy as np
import pytest

from tests import targets_mp as tm

pytestmark = pytest.mark.skipif(not tm.available(), reason='needs mpmath')


def _oracle_errors(target, D):
    from oracle import targets_oracle
    x, ref = tm.edge_reference(target, D)
    # the oracle must not overflow or divide by zero on the way
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = targets_oracle.TARGETS[target](np.array(x))
    return tm.errors(lp, g, ref)


@pytest.mark.parametrize('target,D', tm.CASES)
def test_oracle_matches_multiprecision(target, D):
    e_lp, e_g = _oracle_errors(target, D)
    worst = max(float(e_lp.max()), float(e_g.max()))
    print('%s D=%d: oracle worst error %.3f (value %.3f, gradient %.3f) x 2^-53 S'
          % (target, D, worst, e_lp.max(), e_g.max()))
    assert worst <= 2.0 * tm.ORACLE_ERR[target]


def test_recorded_figures_are_the_measured_ones():
    """ORACLE_ERR is the measured worst case, not a loose cap: the worst error over
    a target's cases reaches at least half of the recorded figure."""
    for target in tm.ORACLE_ERR:
        worst = max(max(float(e.max()) for e in _oracle_errors(t, D))
                    for t, D in tm.CASES if t == target)
        assert worst >= 0.5 * tm.ORACLE_ERR[target], (target, worst)


def test_edge_set_covers_the_documented_points():
    """The point set itself: no degenerate point, the exact centres present, the
    two sides of lp_tab's switch on their sides."""
    pool = tm.sep_pool()
    assert np.sum(pool == 0.0) == 1
    for c in tm.SEP_CENTRES[1:]:
        for s in (1.0, -1.0):
            near = np.abs(pool - s * c) <= tm.JITTER * c
            assert near.sum() >= 24
    # |4x| on both sides of exp_fast's -746 clamp, and exp(-|4x|) subnormal at 177.5
    assert (4 * np.abs(pool) > 746).any() and ((4 * np.abs(pool) < 746) & (np.abs(pool) > 186)).any()
    sub = pool[np.abs(np.abs(pool) - 177.5) < 1]
    assert np.all((np.exp(-4 * np.abs(sub)) < 2.0 ** -1022) & (np.exp(-4 * np.abs(sub)) > 0))
    for D in tm.FUNNEL_DIMS:
        x = tm.edge_points('funnel', D)
        for c in tm.FUNNEL_X1:
            at = x[x[:, 1] == c]
            assert len(at) >= 2 and (np.delete(at, 1, axis=1) == 0).all(axis=1).any()
    sw = tm.es_switch_rows()
    w = (np.exp(sw[:, 1]) * 0.2) ** 2
    assert np.all(np.isfinite(w))
    assert set(sw[w < 2.0 ** 1000, 1]) == {348.0} and set(sw[w >= 2.0 ** 1000, 1]) == {352.0, 354.5, 348.4}


def test_short_run_start_points_are_well_conditioned():
    """Every off-centre start of tests/test_gpu_targets_edges.py's 20-step runs: two
    oracle runs, the second with every draw moved by one ulp, stay within 1e-9 of
    each other (scaled as the GPU test scales), so the GPU comparison at 1e-7
    measures the kernels and not the start point."""
    from oracle import vb_oracle as vo
    from tests import test_gpu_targets_edges as te

    def scaled(a, b):
        return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))
    for target, D in te.RUN_CASES:
        for start in te.STARTS[target]:
            for log_sigma in te.LOG_SIGMAS:
                for kind, df in te.FAMS:
                    for objective in ('klvi', 'chivi'):
                        lam0 = te.start_lam(target, start, D, log_sigma)
                        a = te.oracle_run(vo, kind, df, target, D, objective, lam0)
                        b = te.oracle_run(vo, kind, df, target, D, objective, lam0, nudge=True)
                        assert np.all(np.isfinite(a[1])) and np.all(np.isfinite(a[2]))
                        d = max(scaled(a[1], b[1]), scaled(a[2], b[2]))
                        assert d <= 1e-9, (target, start, log_sigma, kind, objective, d)
