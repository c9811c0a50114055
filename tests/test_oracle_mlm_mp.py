"""The numpy restatement of the multilevel regression target (tests/mlm_cases.py), the
reference of tests/test_gpu_mlm.py, pinned: over the edge sets of tests/mlm_mp.py its
values and gradients stay within twice the recorded MLM_ORACLE_ERR of a 50-digit mpmath
restatement, in units of 2^-53 S.  CPU only."""
import numpy as np
import pytest

from tests import mlm_cases as mc
from tests import mlm_mp as mm

needs_mp = pytest.mark.skipif(not mm.available(), reason='needs mpmath')


_CACHE = {}     # the errors of a case, computed once and shared by the tests below


def _errors(lik, centered, p, G, M):
    key = (lik, centered, p, G, M)
    if key not in _CACHE:
        c, ref = mm.edge_reference(*key)
        # the restatement must not overflow or divide by zero on the way
        with np.errstate(over='raise', divide='raise', invalid='raise'):
            lp, g = mc.restatement(c.x, c.y, c.group, n_groups=G, **c.kw)(np.array(c.z))
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
        _CACHE[key] = (c, mm.errors(lp, g, ref))
    return _CACHE[key]


@needs_mp
@pytest.mark.parametrize('lik,centered,p,G,M', mm.cases())
def test_restatement_matches_multiprecision(lik, centered, p, G, M):
    c, (e_lp, e_g) = _errors(lik, centered, p, G, M)
    r, (gr, gc) = int(np.argmax(e_lp)), np.unravel_index(int(np.argmax(e_g)), e_g.shape)
    print('MLM ORACLE %s centred=%d p=%d G=%d M=%d: value %.3f (row %d, u = %r), gradient %.3f '
          '(row %d, column %d, u = %r) x 2^-53 S'
          % (lik, centered, p, G, M, e_lp[r], r, float(c.z[r, p]), e_g[gr, gc], gr, gc,
             float(c.z[gr, p])))
    assert max(e_lp[r], e_g[gr, gc]) <= 2.0 * mm.MLM_ORACLE_ERR[centered]


@needs_mp
@pytest.mark.parametrize('centered', mc.FORMS)
def test_recorded_figures_are_the_measured_ones(centered):
    """MLM_ORACLE_ERR is the measured worst case, not a loose cap."""
    worst = max(max(float(e.max()) for e in _errors(*case)[1])
                for case in mm.cases() if case[1] == centered)
    assert 0.5 * mm.MLM_ORACLE_ERR[centered] <= worst <= mm.MLM_ORACLE_ERR[centered] * 1.001


@needs_mp
def test_edge_sets_cover_the_documented_points():
    for lik, centered, p, G, M in mm.cases():
        c = mm.edge_case(lik, centered, p, G, M)
        z = c.z
        assert z.shape[1] == p + 1 + G and z.shape[0] <= 80
        for uc in mm.U_CENTRES:
            assert np.sum(z[:, p] == uc) >= (2 if centered else 1)
        eta = np.array([mm._eta(c.x, c.group, zr, p, centered) for zr in z])
        if lik == 'bernoulli_logit':
            assert np.sum(np.abs(np.max(np.abs(eta), axis=1) - mm.ETA_FAR) < 1e-6) >= len(mm.U_CENTRES)
        else:
            assert np.sum(np.max(np.abs(c.y - eta), axis=1) > 0.5 * mm.RESID_FAR) >= len(mm.U_CENTRES)
        if centered:
            # the prior's own region: a within a few tau of 0 at a tiny tau
            zg = z[:, p + 1:] / np.exp(z[:, p:p + 1])
            small = z[:, p] < -39.0
            assert np.sum(small & (np.abs(zg).max(axis=1) < 6.0)) >= mm.BLOCK_ROWS - 1
        sizes = np.bincount(c.group, minlength=G)
        if G >= 3:
            assert sizes.min() == 0 and np.sum(sizes == 1) >= 1 and sizes.max() > M // 2
