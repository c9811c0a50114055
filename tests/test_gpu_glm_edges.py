"""Every kernel variant of the regression target (viabel_amd/csrc/vb_glm.hip) at the
edge data and rows of tests/glm_mp.py, against the 50-digit reference: the value and
every gradient entry of targets.regression(...).logdensity_and_grad within
8 x GLM_ORACLE_ERR[likelihood] in units of 2^-53 S (S the condition sum of the
result).  The factor 8 over the numpy restatement's own error is the one
tests/test_gpu_targets_edges.py grants device kernels, for the same reasons: device
log1p / exp of ~1 ulp where libm is ~0.5, reciprocals formed once on the host in place
of divisions, and sums taken in tile, wave and chunk order.

Which instance a shape reaches is read from glm_plan and glm_launch (the device has
256 compute units, so the plan aims at 1024 blocks):
  D <= 16   glm_rows_small_kernel<LIK, GRAD, DP>, DP = 2 / 4 / 8 / 16 for D <= 2 / 4 / 8 /
            16, 64 threads up to n = 4096 and 256 above
  D > 16    glm_rows_mfma_kernel<LIK, GRAD, NCT>, NCT = 2 / 4 / 8 for D <= 32 / <= 64 /
            above; ceil(D / 32) LDS slices; ceil(D / (16 NCT)) column slabs with a
            gradient, one without (then always NCT = 2)
  chunks    min(ceil(M / 64), ceil(1024 / row tiles)) of a whole number of 64
            observations: with n <= 16 (one row tile of either kernel) every 64
            observations are a chunk, and from two chunks on glm_combine_kernel adds
            the partials
Measured worst errors on MI355X are in DESIGN.md §7b.
"""
import numpy as np
import pytest

from tests import glm_cases as gc
from tests import glm_mp as gm
from tests.conftest import gpu_available
from tests.test_gpu_glm import _close, _objective, _pair

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not gm.available(), reason='needs mpmath')]

MARGIN = 8.0


def _target(c):
    from viabel_amd import targets
    return targets.regression(c.x, c.y, **c.kw)


def _value_only(t, beta):
    """log p with a null grad_out, the way Target.logdensity_and_grad calls the
    library (the Python layer has no value-only entry for a target)."""
    from viabel_amd import _native as nat
    x = nat.as_f64(np.atleast_2d(beta))
    lp = np.empty(x.shape[0])
    nat.check(nat.lib().vb_target_logdensity(nat.context().handle, t._struct(), nat.dptr(x),
                                             x.shape[0], nat.dptr(lp), None))
    return lp


def _check(tag, lik, D, M, n, lp, g, c, ref):
    """The EDGE line and the two assertions; g None: value only."""
    bound = MARGIN * gm.GLM_ORACLE_ERR[lik]
    if g is None:
        e_lp, _ = gm.errors(lp[c.rows], np.zeros_like(ref.g_hi), ref)
        e_g = None
    else:
        e_lp, e_g = gm.errors(lp[c.rows], g[c.rows], ref)
    r = int(np.argmax(e_lp))
    eta = lambda k: (c.x[:2] @ c.beta[c.rows[k]]).tolist()
    msg = ('EDGE %s %s D=%d M=%d n=%d: value %.3f (row %d, eta[:2] = %r)'
           % (tag, lik, D, M, n, e_lp[r], c.rows[r], eta(r)))
    if e_g is not None:
        gr, gcol = np.unravel_index(int(np.argmax(e_g)), e_g.shape)
        msg += (', gradient %.3f (row %d, column %d, eta[:2] = %r)'
                % (e_g[gr, gcol], c.rows[gr], gcol, eta(gr)))
    print(msg + '; bound %.2f x 2^-53 S' % bound)
    assert e_lp[r] <= bound
    if e_g is not None:
        assert e_g[gr, gcol] <= bound


def _run(tag, lik, D, M, n):
    c, ref = gm.edge_reference(lik, D, M, n)
    lp, g = _target(c).logdensity_and_grad(np.array(c.beta))
    assert lp.shape == (n,) and g.shape == (n, D)
    _check(tag, lik, D, M, n, lp, g, c, ref)
    return c, lp, g


@pytest.mark.parametrize('lik', gc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', gm.SHAPES_SMALL)
def test_lane_per_row_kernel(lik, D, M, n):
    """DP = 2 (D = 1, 2), 4 (4), 8 (5, 8: both ends of 5..8) and 16 (9, 16); M = 63 / 64 /
    65 around the 64-observation LDS tile and 129 / 130 (three chunks, the last of one and
    of two observations); n = 63 / 64 / 65 / 70 around one 64-lane block (the second block
    of n = 65 has one live lane)."""
    _run('small', lik, D, M, n)


def test_lane_per_row_kernel_with_256_threads():
    """n = 4097 > 4096: glm_plan takes tb = 256, 17 row blocks, the last with one live
    row; M = 25 is one chunk.  The multiprecision reference is taken on 64 rows (0, 1,
    2 and 61 evenly spaced ones, so every block, the last row included); all rows are
    also held to the float64 restatement at test_gpu_glm.py's 1e-11."""
    lik, (D, M, n) = 'student_t', gm.SHAPE_256
    c, lp, g = _run('small-256', lik, D, M, n)
    assert len(c.rows) <= gm.SAMPLE_ROWS and c.rows[-1] == n - 1
    assert len(set(c.rows // 256)) == 17
    lp0, g0 = gc.restatement(c.x, c.y, **c.kw)(c.beta)
    _close(lp, lp0, 1e-11)
    _close(g, g0, 1e-11)


@pytest.mark.parametrize('lik', gc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', gm.SHAPES_MFMA)
def test_matrix_kernel_at_the_D_boundaries(lik, D, M, n):
    """17, 32: NCT = 2, one slice (the staged slice serves both products); 33: NCT = 4,
    two slices, the second with one live column; 64: NCT = 4 full; 65: NCT = 8, three
    slices; 96; 128: one full slab, four slices; 129: a second slab (blockIdx.z = 1) of
    one column; 130; 257: three slabs, the last of one column.  n = 15 / 16 / 17: a
    partial tile, a full one, a second tile of one row.  M = 65 / 70 / 129: a last chunk
    of 1, 6 and 1 observations, whose single MFMA tile leaves three waves idle."""
    _run('mfma', lik, D, M, n)


@pytest.mark.parametrize('lik', gc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', gm.SHAPES_CHUNK)
def test_six_observation_chunks(lik, D, M, n):
    """M = 321, n = 10: ceil(321 / 64) = 6 chunks of 64 (four MFMA tiles: one round with
    every wave busy), the last of one observation; D = 40 (NCT = 4, one slab) and 130
    (NCT = 8, two slabs, only slab 0 writing log p)."""
    _run('chunks', lik, D, M, n)


@pytest.mark.parametrize('lik', gc.LIKELIHOODS)
@pytest.mark.parametrize('D,M,n', gm.SHAPES_VALUE)
def test_value_only(lik, D, M, n):
    """GRAD = false through vb_target_logdensity with a null grad_out (_value_only): the
    lane-per-row kernel (D = 3; n = 64 is one full 64-lane block) and
    glm_rows_mfma_kernel<LIK, false, 2> with one (D = 20), two (40) and five (130) LDS
    slices, nK > 1 with GRAD = false included; M = 65 two chunks, 321 six.

    The value equals the with-gradient call's bit for bit at all four shapes: both run
    the same eta, link and sums, and take the same chunks, because glm_plan's chunk count
    depends on `grad` only through the scratch cap nc n (1 + D) <= 32 Mi doubles, which
    6 x 64 x 131 is far below."""
    c, ref = gm.edge_reference(lik, D, M, n)
    t = _target(c)
    lp = _value_only(t, np.array(c.beta))
    _check('value-only', lik, D, M, n, lp, None, c, ref)
    lp_g, g = t.logdensity_and_grad(np.array(c.beta))
    _check('value-only shape, with gradient', lik, D, M, n, lp_g, g, c, ref)
    assert np.array_equal(lp, lp_g)


@pytest.mark.parametrize('kind,D', [('mf_gauss_klvi', 70), ('mf_gauss_klvi', 130),
                                    ('fr_t_klvi', 70)])
def test_estimators_match_callback_of_same_model_at_wide_D(kind, D):
    """test_gpu_glm.py's test_estimators_match_callback_of_same_model at NCT = 8 (D = 70)
    and two column slabs (130), on the materialised mean-field path and the full-rank
    path, with its tolerances."""
    from viabel_amd import targets
    t, f = _pair(D, 65, 'student_t', seed=11)
    o1, P = _objective(kind, D, t)
    o2, _ = _objective(kind, D, targets.callback(f, D))
    lam = np.random.RandomState(12).randn(P) * 0.05
    np.random.seed(1)
    v1, g1 = o1(lam)
    np.random.seed(1)
    v2, g2 = o2(lam)
    np.testing.assert_allclose(v1, v2, rtol=1e-11)
    _close(g1, g2, 1e-10)


def test_two_calls_give_the_same_bits_with_slabs_and_chunks():
    """(D, M, n) = (130, 321, 10): two column slabs x six chunks and the combine."""
    t, _ = _pair(130, 321, 'student_t', seed=15)
    b = np.random.RandomState(16).randn(10, 130)
    lp1, g1 = t.logdensity_and_grad(b)
    lp2, g2 = t.logdensity_and_grad(b)
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)


def test_scratch_cap_falls_back_to_fewer_chunks():
    """(D, M, n) = (2100, 1024, 1024), student_t, with gradient.  By glm_plan: 64 row
    tiles; aim 4 x 256 CUs = 1024 blocks; max_chunks = ceil(1024 / 64) = 16; nc = min(16,
    ceil(1024 / 64)) = 16.  per = n (1 + D) = 1024 x 2101 = 2 151 424 doubles, and
    16 x per = 34 422 784 > kGlmScratchMax = 32 x 2^20 = 33 554 432, so nc becomes
    floor(33 554 432 / 2 151 424) = 15, a chunk ceil(1024 / 15) = 69 -> 128 observations,
    and the call runs 8 chunks (17 211 392 doubles of partials) x 17 slabs, the last slab
    of 52 columns (a full slice and one of 20).  No materially smaller shape reaches the
    branch: row tiles x chunks <= ~1024 bounds nc n by ~16 400, so nc n (1 + D) > 2^25
    needs D >= 2047 whatever n and M.  The reference is the float64 restatement (a
    multiprecision one is too slow here) under test_gpu_glm.py's metric at its M = 1000
    tolerance."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count >= 241, \
        'the arithmetic above needs ceil(4 CUs / 64 row tiles) >= 16 chunks'
    D, M, n = 2100, 1024, 1024
    t, f = _pair(D, M, 'student_t', seed=19)
    b = np.random.RandomState(20).randn(n, D) * 0.8
    lp, g = t.logdensity_and_grad(b)
    lp0, g0 = f(b)
    print('max err', float(np.max(np.abs(lp - lp0))), float(np.max(np.abs(g - g0))))
    _close(lp, lp0, 1e-10)
    _close(g, g0, 1e-10)
