"""The device runs of the Cholesky full-rank Gaussian family (vb_frg.hip) and of the
low-rank-plus-diagonal family (vb_lrg.hip), one step at a time: every update route of
advance_fr_steps (vb_capi.hip) against the multiprecision update of tests/mf_mp.py, at
the shapes of tests/fr_run_cases.py.

Routes.  Philox draws with adagrad: the windowed step rides in the gradient kernel's
epilogue (lam updated in place, ring slot and history row written there).  Host draws
with adagrad: launch_adagrad_update after the gradient kernel.  RMSProp-IA / Adam-IA:
launch_ia_update with the ring as the two moment vectors and the history row as the
pre-update parameters.

Method (tests/test_gpu_mf_edges.py test_adagrad_update_step_by_step).  lam after k steps
comes from a fresh DeviceRun advanced k steps in one call, for every k.  The draws of
step i of problem q are the C oracle's, rng_oracle.fr_noise(seed, stream + q stride, i, N,
width)[1], width D or D + R; on the host route the same arrays go through advance_host.
The reference gradient at the device's own lam_i is the numpy restatement's on isogauss
(tests/frg_cases.py, tests/lrg_cases.py) with its condition sums from np_scales; the
reference update is mf_mp.adagrad_update / mf_mp.ia_update applied to the device's own
lam_i and those gradients, so one step's rounding is measured, not a trajectory.  Bars:
fr_run_cases' docstring (8 x MF_ORACLE_ERR[update] units of S_u = |lam'| + |step| + r G).
values[i] is held to 8 x the family's value record in units of the value's S.

Every measured error is printed beside its bar (FR_RUN_EDGE lines) and, when
VIABEL_AMD_FR_RUN_EDGE_RECORD names a file, collected there as JSON."""
import json
import os

import numpy as np
import pytest

from tests import fr_run_cases as rc
from tests import mf_mp as mm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not mm.available(), reason='needs mpmath')]

RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    path = os.environ.get('VIABEL_AMD_FR_RUN_EDGE_RECORD')
    if path:
        with open(path, 'w') as f:
            f.write('{\n"_note": "per case and class: [error, bar] in units of 2^-53 S",\n'
                    + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v))
                                 for k, v in RECORD.items()) + '\n}\n')


def _check(cid, errs, bars):
    bad = []
    for cls, e in errs.items():
        bar = bars[cls]
        RECORD.setdefault(cid, {})[cls] = [float('%.4g' % e), float('%.4g' % bar)]
        print('FR_RUN_EDGE %s %s err %.3f (bar %.2f)' % (cid, cls, e, bar))
        if not e <= bar:
            bad.append((cls, e, bar))
    assert not bad, bad


def _objective(kind, shape, objective, N, rng):
    from viabel_amd import vb, targets
    fam = (vb.cholesky_gaussian_variational_family(shape[0], rng=rng) if kind == 'frg'
           else vb.low_rank_gaussian_variational_family(shape[0], shape[1], rng=rng))
    tgt = targets.isogauss(shape[0])
    if objective == 'klvi':
        return vb.black_box_klvi(fam, tgt, N)
    if objective == 'klvi_pd':
        return vb.black_box_klvi_pd(fam, tgt, N)
    return vb.black_box_chivi(rc.ALPHA, fam, tgt, N)


def _oracle_draws(kind, shape, N, steps, nprob=1, stride=1):
    """[nprob][steps][N][width]: the C oracle's draws of the streams STREAM + q stride."""
    from oracle import rng_oracle as ro
    w = rc.noise_width(kind, shape)
    return np.stack([np.stack([ro.fr_noise(rc.SEED, rc.STREAM + q * stride, i, N, w, 30.0)[1]
                               for i in range(steps)]) for q in range(nprob)])


def _device_draws(kind, shape, N, steps):
    """[1][steps][N][width]: the in-kernel draws of stream STREAM themselves, read back
    through sample() at parameters that make x a copy of them: mu = 0 and L = I (Cholesky),
    mu = 0, d = 1, B = 0 for the z columns and d = exp(-1000) = 0, B = [I_R; 0] for the u
    columns (low-rank).  Every product is by 1 or 0, so x holds the draws exactly.  sample()
    and the run share the noise kernel (frg_noise_kernel, lrg_noise_kernel)."""
    from viabel_amd import vb
    from tests import lrg_cases as lc
    D, P = shape[0], rc.n_free(kind, shape)
    out = np.empty((1, steps, N, rc.noise_width(kind, shape)))
    for i in range(steps):
        fam = (vb.cholesky_gaussian_variational_family(D, rng='philox') if kind == 'frg'
               else vb.low_rank_gaussian_variational_family(D, shape[1], rng='philox'))
        fam.seed, fam.stream, fam.step = rc.SEED, rc.STREAM, i
        out[0, i, :, :D] = fam.sample(np.zeros(P), N)
        if kind == 'lrg':
            R = shape[1]
            B = np.zeros((D, R))
            B[np.arange(R), np.arange(R)] = 1.0
            fam.step = i
            out[0, i, :, D:] = fam.sample(lc.pack(np.zeros(D), np.full(D, -1000.0), B), N)[:, :R]
    return out


class _Runs:
    """Fresh runs of one configuration: lam0 [nprob][P]; route 'philox' (in-kernel draws
    of the streams STREAM + q stride) or 'host' (draws [nprob][steps][N][width])."""

    def __init__(self, kind, shape, objective, N, lam0, W, n_iters, eps, lr_end, route,
                 draws=None, stride=1, stream=rc.STREAM, optimizer=None):
        self.args = (kind, shape, objective, N, 'philox' if route == 'philox' else 'numpy')
        self.lam0 = np.atleast_2d(lam0)
        self.W, self.n_iters, self.eps, self.lr_end = W, n_iters, eps, lr_end
        self.route, self.draws, self.stride, self.stream = route, draws, stride, stream
        self.optimizer = optimizer

    def advanced(self, k):
        """A fresh run advanced k steps in one call."""
        from viabel_amd import vb
        kw = {} if self.optimizer is None else {'optimizer': self.optimizer}
        run = vb.DeviceRun(_objective(*self.args), self.n_iters, self.lam0, window=self.W,
                           learning_rate=rc.LR0, epsilon=self.eps,
                           learning_rate_end=self.lr_end, **kw)
        if self.route == 'philox':
            run.advance_philox(k, rc.SEED, self.stream, 0, stream_stride=self.stride)
        else:
            run.advance_host(self.draws[:, :k])
        return run

    def lams(self, steps):
        """[steps + 1][nprob][P]: lam after k steps, k = 0 ... steps, and the last run."""
        out = [self.lam0.copy()]
        run = None
        for k in range(1, steps + 1):
            run = self.advanced(k)
            out.append(run.result(history=False)[0].copy())
        return out, run


def _reference_grads(kind, shape, objective, lams, draws):
    """Per step i: the restatement's (value, S value, gradient, S gradient) at lams[i] on
    draws[i], every figure asserted finite."""
    ofam = rc.restatement(kind, shape)
    out = []
    for i in range(len(draws)):
        v, g = rc.value_grad(kind, ofam, objective, lams[i], draws[i])
        Sv, Sg = rc.scales(kind, ofam, objective, lams[i], draws[i])
        assert np.isfinite(v) and np.isfinite(Sv) and np.all(np.isfinite(g)) \
            and np.all(np.isfinite(Sg)), (i, v, Sv)
        out.append((float(v), Sv, np.asarray(g, dtype=float), Sg))
    return out


def _adagrad_errors(kind, shape, objective, lams, draws, values, W, eps, lr_end, n_iters):
    """Worst step error (units of S_u) and worst value error (units of the value's S) of
    one problem: lams [steps + 1][P], draws [steps][N][width], values [steps]."""
    from oracle import vb_oracle as vo
    steps = len(draws)
    refs = _reference_grads(kind, shape, objective, lams, draws)
    lrs = vo.learning_rate_schedule(n_iters, rc.LR0, lr_end)
    r = rc.grad_weight(kind, objective, 'adagrad')
    worst, worst_v = 0.0, 0.0
    for i in range(steps):
        win = range(max(0, i + 1 - W), i + 1)
        G = np.array([refs[k][2] for k in win])
        GS = np.array([refs[k][3] for k in win])
        ref, step = mm.adagrad_update(lams[i], G, lrs[i], eps)
        assert mm.finite(ref)
        carried = rc.adagrad_carried(G, GS, step, lrs[i], eps)
        assert np.all(np.isfinite(carried))
        e = mm.units(lams[i + 1], mm.Val(ref.hi, ref.lo, ref.S + r * carried))
        worst = max(worst, float(e.max()))
        worst_v = max(worst_v, float(mm.units(values[i], mm.Val(refs[i][0], 0.0, refs[i][1]))))
    return worst, worst_v


def _bars(kind, objective, update='adagrad'):
    return {update: rc.MARGIN * mm.MF_ORACLE_ERR[update],
            'value': rc.MARGIN * rc.records(kind, objective)[0]}


FUSED = rc.fused_cases()


@pytest.mark.parametrize('c', FUSED, ids=[rc.case_id(c) for c in FUSED])
def test_fused_adagrad_step_by_step(c):
    """Philox draws, one problem: the step in the gradient kernel's epilogue.  W = 1, the
    wrap at periods 2, 10 and 17, W past the step count, eps << g^2 and
    learning_rate_end, at block shapes on both sides of every tile / block limit of the
    two gradient kernels (fr_run_cases.FRG_SHAPES, LRG_SHAPES); CHIVI and KLVI_PD at one
    single-block and one several-block shape, CHIVI once at N = 17."""
    kind, shape, objective, N, W, steps, eps, lr_end = c
    lam0 = rc.lam0(kind, shape)
    runs = _Runs(kind, shape, objective, N, lam0, W, steps, eps, lr_end, 'philox')
    lams, last = runs.lams(steps)
    draws = _oracle_draws(kind, shape, N, steps)[0]
    values = last.result(history=False)[2][0]
    e, ev = _adagrad_errors(kind, shape, objective, [l[0] for l in lams], draws, values, W, eps,
                            lr_end, steps)
    _check('fused/' + rc.case_id(c), {'adagrad': e, 'value': ev}, _bars(kind, objective))


@pytest.mark.parametrize('stride', [1, 7])
@pytest.mark.parametrize('kind', ['frg', 'lrg'])
def test_fused_adagrad_three_problems(kind, stride):
    """Three problems with different lam0 in one run (ring offset q P W, history offset
    (q n_hist + step - hist_start) P, value offset q n_iters + step, stream STREAM + q
    stride): every problem against its own reference on its own stream's draws, and
    problem q equal bit for bit -- lam, history, values, smooth -- to a one-problem run on
    stream STREAM + q stride from lam0[q]."""
    shape, N, W, steps, eps = rc.ONE_SHAPE[kind], 5, 2, 5, 0.1
    lam0 = np.stack([rc.lam0(kind, shape, seed=q) for q in range(3)])
    assert not np.array_equal(lam0[0], lam0[1]) and not np.array_equal(lam0[1], lam0[2])
    runs = _Runs(kind, shape, 'klvi', N, lam0, W, steps, eps, None, 'philox', stride=stride)
    lams, last = runs.lams(steps)
    lam3, hist3, vals3, sm3 = last.result()
    draws = _oracle_draws(kind, shape, N, steps, 3, stride)
    errs = {}
    for q in range(3):
        e, ev = _adagrad_errors(kind, shape, 'klvi', [l[q] for l in lams], draws[q], vals3[q], W,
                                eps, None, steps)
        errs['adagrad'] = max(errs.get('adagrad', 0.0), e)
        errs['value'] = max(errs.get('value', 0.0), ev)
        one = _Runs(kind, shape, 'klvi', N, lam0[q], W, steps, eps, None, 'philox',
                    stream=rc.STREAM + q * stride).advanced(steps)
        lam1, hist1, vals1, sm1 = one.result()
        assert np.array_equal(lam1[0], lam3[q]), q
        assert np.array_equal(hist1[0], hist3[q]), q
        assert np.array_equal(vals1[0], vals3[q]), q
        assert np.array_equal(sm1[0], sm3[q]), q
    _check('three/%s/stride%d' % (rc.tag(kind, shape), stride), errs, _bars(kind, 'klvi'))


@pytest.mark.parametrize('n_iters', [1, 2, 3, 5, 21])
@pytest.mark.parametrize('kind', ['frg', 'lrg'])
def test_history_values_and_smooth(kind, n_iters):
    """Fused route.  The run returns n_iters - (3 n_iters) // 4 history rows; row j equals
    bit for bit the lam of a fresh run advanced hist_start + j + 1 steps (the post-update
    parameters of step hist_start + j, vb.py:374-376 of the reference); values[i] is
    within the value bar of the restatement's value at lam_i on step i's draws; smooth is
    the mean of the history rows.  vb_run_result forms it in row_mean_kernel: one thread
    per entry adds the rows in order, first row first, from 0.0 (numpy's axis-0 order),
    and divides by the row count.  With n rows that is n - 1 rounded additions (0 + h_0 is
    exact) and one rounded division, so |smooth - mean| <= n 2^-53 (sum_r |h_r|) / n to
    first order: the error is quoted in units of 2^-53 (sum_r |h_r|) / n against the bar n."""
    from mpmath import mp, mpf
    shape, N, W, eps = rc.ONE_SHAPE[kind], 5, 2, 0.1
    lam0 = rc.lam0(kind, shape)
    runs = _Runs(kind, shape, 'klvi', N, lam0, W, n_iters, eps, None, 'philox')
    lams, last = runs.lams(n_iters)
    lam, hist, vals, smooth = last.result()
    hist_start = (3 * n_iters) // 4
    rows = n_iters - hist_start
    assert hist.shape == (1, rows, rc.n_free(kind, shape))
    for j in range(rows):
        assert np.array_equal(hist[0, j], lams[hist_start + j + 1][0]), j
    assert np.array_equal(lam[0], lams[n_iters][0])
    draws = _oracle_draws(kind, shape, N, n_iters)[0]
    e, ev = _adagrad_errors(kind, shape, 'klvi', [l[0] for l in lams], draws, vals[0], W, eps,
                            None, n_iters)
    with mp.workdps(50):
        worst = 0.0
        for p in range(hist.shape[2]):
            col = [mpf(float(v)) for v in hist[0, :, p]]
            mean, S = mp.fsum(col) / rows, mp.fsum(abs(v) for v in col) / rows
            d = abs(mpf(float(smooth[0, p])) - mean)
            assert np.isfinite(smooth[0, p])
            if d != 0:
                worst = max(worst, float(d / (S * mpf(2) ** -53)))
    bars = _bars(kind, 'klvi')
    bars['smooth'] = float(rows)
    _check('history/%s/n%d' % (rc.tag(kind, shape), n_iters),
           {'adagrad': e, 'value': ev, 'smooth': worst}, bars)


@pytest.mark.parametrize('W,steps,eps,lr_end', rc.SHORT)
@pytest.mark.parametrize('kind', ['frg', 'lrg'])
def test_unfused_adagrad_on_host_noise(kind, W, steps, eps, lr_end):
    """The C oracle's draws through advance_host: the gradient kernel writes grad and
    launch_adagrad_update applies the step.  Within the same bar of the same reference as
    the fused route.  Whether the result equals the fused run's lam bit for bit is
    printed, not asserted (FR_RUN_EDGE ... fused-bits).

    Finding: it does not, by ~1e-16 in lam.  The cause is the draws, not the update: about
    60 % of the in-kernel draws differ from the C oracle's in their last bits (measured: by
    up to 1.8e-15 absolutely, a few ulps of the largest draws and many ulps of a z near 0;
    presumably normal_pair's device log / sincos against libm's), which the parity tests'
    1e-11 cannot see.  The fused route's measured step errors on the oracle's draws are
    accordingly larger than the host route's (3.4 against 0.9 units at worst) and stay
    within the same bar.  So the comparison is made a second time on draws both routes do
    share: the in-kernel draws read back exactly (_device_draws) and fed through
    advance_host.  On those the unfused run equals the fused run bit for bit, lam, history
    and values, and that is asserted."""
    shape, N = rc.ONE_SHAPE[kind], 5
    lam0 = rc.lam0(kind, shape)
    draws = _oracle_draws(kind, shape, N, steps)
    host = _Runs(kind, shape, 'klvi', N, lam0, W, steps, eps, lr_end, 'host', draws=draws)
    lams, last = host.lams(steps)
    values = last.result(history=False)[2][0]
    e, ev = _adagrad_errors(kind, shape, 'klvi', [l[0] for l in lams], draws[0], values, W, eps,
                            lr_end, steps)
    fused = _Runs(kind, shape, 'klvi', N, lam0, W, steps, eps, lr_end, 'philox').advanced(steps)
    res_f = fused.result()
    same = np.array_equal(res_f[0][0], lams[steps][0])
    cid = 'host/%s/W%d/s%d/end%s' % (rc.tag(kind, shape), W, steps, lr_end)
    print('FR_RUN_EDGE %s fused-bits %s (max |fused - unfused| %.3e)'
          % (cid, 'equal' if same else 'differ',
             float(np.max(np.abs(res_f[0][0] - lams[steps][0])))))
    own = _device_draws(kind, shape, N, steps)
    print('FR_RUN_EDGE %s draws: %d of %d in-kernel draws differ from the C oracle\'s, max %.3e'
          % (cid, int(np.sum(own != draws)), own.size, float(np.max(np.abs(own - draws)))))
    RECORD.setdefault(cid, {})['fused_bits_equal'] = bool(same)
    res_o = _Runs(kind, shape, 'klvi', N, lam0, W, steps, eps, lr_end, 'host',
                  draws=own).advanced(steps).result()
    for a, b in zip(res_f[:3], res_o[:3]):
        assert np.array_equal(a, b)
    _check(cid, {'adagrad': e, 'value': ev}, _bars(kind, 'klvi'))


@pytest.mark.parametrize('eps_ia', [1e-6, 1e-300])
@pytest.mark.parametrize('which', ['rmsprop', 'adam'])
@pytest.mark.parametrize('kind', ['frg', 'lrg'])
def test_native_ia_step_by_step(kind, which, eps_ia):
    """RMSProp-IA and Adam-IA through DeviceRun(..., optimizer=...) on Philox draws, 6
    steps, as test_gpu_mf_edges.test_ia_update_step_by_step: each step against
    mf_mp.ia_update applied to the device's own previous lam with the moments rebuilt from
    the restatement's gradients at the device's own lams.  History: the reference's IA
    loops append old_variational_param, the copy taken before the update (vb.py:462-466,
    vb.py:624-628), so row i holds the pre-update parameters of step i: row 0 is lam0 and
    row i the lam of a fresh run advanced i steps, bit for bit."""
    from viabel_amd import _native as nat
    shape, N, steps, window = rc.ONE_SHAPE[kind], 5, 6, 500
    opt = nat.OPT_RMSPROP_IA if which == 'rmsprop' else nat.OPT_ADAM_IA
    lam0 = rc.lam0(kind, shape)
    runs = _Runs(kind, shape, 'klvi', N, lam0, window, steps, eps_ia, None, 'philox', optimizer=opt)
    lams, last = runs.lams(steps)
    lam, hist, vals, _ = last.result()
    assert hist.shape == (1, steps, rc.n_free(kind, shape))
    for i in range(steps):
        assert np.array_equal(hist[0, i], lams[i][0]), i
    assert np.array_equal(lam[0], lams[steps][0])
    draws = _oracle_draws(kind, shape, N, steps)[0]
    refs = _reference_grads(kind, shape, 'klvi', [l[0] for l in lams], draws)
    r = rc.grad_weight(kind, 'klvi', which)
    worst, worst_v = 0.0, 0.0
    for i in range(steps):
        G = np.array([t[2] for t in refs[:i + 1]])
        GS = np.array([t[3] for t in refs[:i + 1]])
        ref, step = mm.ia_update(which, lams[i][0], G, rc.LR0, eps_ia)
        assert mm.finite(ref)
        carried = rc.ia_carried(which, G, GS, step, rc.LR0, eps_ia)
        assert np.all(np.isfinite(carried))
        e = mm.units(lams[i + 1][0], mm.Val(ref.hi, ref.lo, ref.S + r * carried))
        worst = max(worst, float(e.max()))
        worst_v = max(worst_v, float(mm.units(vals[0, i], mm.Val(refs[i][0], 0.0, refs[i][1]))))
    _check('%s/%s/eps%g' % (which, rc.tag(kind, shape), eps_ia), {which: worst, 'value': worst_v},
           _bars(kind, 'klvi', which))


@pytest.mark.parametrize('eps', [0.1, 1e-300])
@pytest.mark.parametrize('kind', ['frg', 'lrg'])
def test_exact_zero_mean_entry_stays_zero(kind, eps):
    """Host route, mu_0 = 0 and z column 0 = 0 in every draw (low-rank: B = 0 at the start
    as well, so row 0 of B, whose gradient g_0 u + (sum r) H_B[0] is 0 when x_0 = 0 and
    W[0] = 0, stays 0 while the other rows move): x_0 = 0 in every row, d/dmu_0 = sum r_n
    (-x_n0) is exactly 0 and mu_0 stays exactly 0.0 through every step, whatever ring slot
    0 holds.  The other entries stay within the step bar."""
    shape, N, W, steps = rc.ONE_SHAPE[kind], 5, 2, 5
    D = shape[0]
    lam0 = rc.lam0(kind, shape)
    lam0[0] = 0.0
    if kind == 'lrg':
        lam0[2 * D:] = 0.0
    draws = _oracle_draws(kind, shape, N, steps)
    draws[:, :, :, 0] = 0.0
    host = _Runs(kind, shape, 'klvi', N, lam0, W, steps, eps, None, 'host', draws=draws)
    lams, last = host.lams(steps)
    assert all(l[0][0] == 0.0 for l in lams), [l[0][0] for l in lams]
    one = [l[0] for l in lams]
    refs = _reference_grads(kind, shape, 'klvi', one, draws[0])
    assert all(t[2][0] == 0.0 and t[3][0] == 0.0 for t in refs)
    if kind == 'lrg':
        assert any(np.any(l[2 * D + shape[1]:] != 0.0) for l in one[1:])     # B moves
        assert all(np.all(l[2 * D:2 * D + shape[1]] == 0.0) for l in one)    # its row 0 does not
    values = last.result(history=False)[2][0]
    e, ev = _adagrad_errors(kind, shape, 'klvi', one, draws[0], values, W, eps, None, steps)
    _check('zero/%s/eps%g' % (rc.tag(kind, shape), eps), {'adagrad': e, 'value': ev},
           _bars(kind, 'klvi'))
