"""The mean-field estimators, family functions and the fused adagrad update of the
device against the 50-digit restatement of tests/mf_mp.py, at the edge shapes and
parameters of tests/mf_cases.py, every entry against its own condition sum (units
of 2^-53 S).

Noise is host noise throughout (the family's _draw replaced by the case's draws, or
DeviceRun.advance_host), so the device and the reference see the same doubles.  The
in-kernel Philox draws are not compared here: sample_kernel draws with normal_pair
/ gamma_pair and a library sqrt where the block kernel draws with the table forms
and rsqrt_pos, so vb_family_sample does not return the step kernels' bits.

Bars.  Estimators, log weights, log q: 8 x mf_mp.MF_ORACLE_ERR[class], the numpy
oracle's measured error on the same cases (tests/test_oracle_mf_mp.py) times the
factor tests/test_gpu_targets_edges.py derives (1-ulp helpers, reciprocal
constants, tree order).  The update: each step is compared with the multiprecision
update applied to the device's own previous lam and the multiprecision gradients
at the device's own lams, so one step's rounding is measured, not a trajectory.
Its error has two parts: the update's own arithmetic, within 8 x
MF_ORACLE_ERR['adagrad'] units of |lam'| + |step| (rsqrt_pos in place of the
oracle's IEEE sqrt and division), and the device gradient's error e_k <= 8 x
MF_ORACLE_ERR[mean | log_sigma] units of S_g,k carried through
d step / d g = lr / sqrt(eps + q) and d step / d q = -step / (2 (eps + q)),
q = sum g_k^2, G = lr S_g / sqrt(eps + q) + |step| / (eps + q) sum_k |g_k| S_g,k.  The
two parts keep their own factors: the step's error is at most 8 x MF_ORACLE_ERR['adagrad']
units of S_u = |lam'| + |step| + r G, r the ratio of the gradient's record to the update's.

Every measured error is printed beside its bar (MF_EDGE lines) and, when
VIABEL_AMD_MF_EDGE_RECORD names a file, collected there as JSON."""
import json
import os

import numpy as np
import pytest

from tests import mf_cases as mc
from tests import mf_mp as mm
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not mm.available(), reason='needs mpmath')]

MARGIN = 8.0
RECORD = {}
CASES = mc.all_cases()


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    path = os.environ.get('VIABEL_AMD_MF_EDGE_RECORD')
    if path:
        with open(path, 'w') as f:
            f.write('{\n"_note": "per case and class: [error, bar] in units of 2^-53 S",\n'
                    + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v))
                                 for k, v in RECORD.items()) + '\n}\n')


def _check(cid, errs, bars=None):
    bad = []
    for cls, e in errs.items():
        bar = (bars or {}).get(cls, MARGIN * mm.MF_ORACLE_ERR.get(cls, 0.0))
        RECORD.setdefault(cid, {})[cls] = [float('%.4g' % e), float('%.4g' % bar)]
        print('MF_EDGE %s %s err %.3f (bar %.2f)' % (cid, cls, e, bar))
        if not e <= bar:
            bad.append((cls, e, bar))
    assert not bad, bad


def _family(vb, kind, df, D, eps_list):
    """A numpy-noise family whose next draws are the arrays of eps_list, in order."""
    fam = (vb.mean_field_gaussian_variational_family(D, rng='numpy') if kind == 'gauss'
           else vb.mean_field_t_variational_family(D, df, rng='numpy'))
    it = iter(eps_list)
    fam.__dict__['_draw'] = lambda n, seed=None: next(it)
    return fam


def _target(targets, name, D):
    return {'isogauss': lambda: targets.isogauss(D), 'mixture': lambda: targets.mixture(D),
            'funnel': lambda: targets.funnel(D),
            'eight_schools_ncp': targets.eight_schools_ncp}[name]()


def _objective(vb, c, fam, tgt):
    if c['objective'] == 'klvi':
        return vb.black_box_klvi(fam, tgt, c['N'])
    if c['objective'] == 'klvi_pd':
        return vb.black_box_klvi_pd(fam, tgt, c['N'])
    return vb.black_box_chivi(c['alpha'], fam, tgt, c['N'])


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_value_gradient_and_log_weights(c):
    """One NativeObjective call (block, column-pair or materialised path by shape)
    and experiments.log_weights (row form at D <= 16, sep form for the separable
    targets past it) on the case's draws."""
    from viabel_amd import vb, targets, experiments
    tgt = _target(targets, c['target'], c['D'])
    fam = _family(vb, c['kind'], c['df'], c['D'], [c['eps'], c['eps']])
    v, g = _objective(vb, c, fam, tgt)(c['lam'])
    assert np.isfinite(v) and np.all(np.isfinite(g)), (v, g)      # never NaN
    x, lw = experiments.log_weights(tgt, fam, c['lam'], c['N'])
    lq = fam.logdensity(x, c['lam'])
    _check(c['id'], mm.case_errors(c, v, g, lw, (lq, x)))


@pytest.mark.parametrize('f', mc.family_cases(), ids=[f['id'] for f in mc.family_cases()])
def test_family_functions(f):
    """sample, logdensity (one wave per row below 512 columns, one block per row
    from 512 on), mean_and_cov and pth_moment at mixed log sigma -30 ... 30."""
    from viabel_amd import vb
    fam = _family(vb, f['kind'], f['df'], f['D'], [f['eps']])
    lam = f['lam']
    x = fam.sample(lam, f['eps'].shape[0])
    errs = {'transform': float(mm.units(x, mm.transform(lam, f['eps'])).max()),
            'log_q': float(mm.units(fam.logdensity(x, lam),
                                    mm.logdensity(f['kind'], f['df'], lam, x)).max()),
            'entropy': float(mm.units(fam.entropy(lam), mm.entropy(f['kind'], lam)))}
    e_m = float(mm.units(np.diag(fam.mean_and_cov(lam)[1]),
                         mm.mean_and_cov_diag(f['kind'], f['df'], lam)).max())
    for p in (2, 4):
        if f['df'] is None or f['df'] > p:
            e_m = max(e_m, float(mm.units(fam.pth_moment(p, lam),
                                          mm.pth_moment(f['kind'], f['df'], p, lam))))
    errs['moments'] = e_m
    _check(f['id'], errs)


@pytest.mark.parametrize('df', [2.000001, 8.0, 1e6])
@pytest.mark.parametrize('D', [1, 513])
def test_t_logdensity_past_the_overflow_of_z_squared(df, D):
    """family_logdensity_kernel (D = 1) and the row-block form (D = 513) at log sigma
    = -400, |z| up to 1e300 in the first column: within the log_q bar on both sides
    of |z| = 1.34e154, where z * z overflows (both forms returned -inf there before
    they switched to 2 log|z| - log df + log1p(df / z^2) above 2^500)."""
    from viabel_amd import vb
    fam = vb.mean_field_t_variational_family(D, df, rng='numpy')
    lam = np.concatenate([np.zeros(D), np.full(D, -400.0)])
    x = np.zeros((2 * len(mc.Z_EDGES), D))
    x[:, 0] = (np.array(mc.Z_EDGES)[:, None] * np.exp(-400.0) * np.array([1.0, -1.0])).ravel()
    ref = mm.logdensity('t', df, lam, x)
    assert mm.finite(ref)
    got = fam.logdensity(x, lam)
    assert not np.any(np.isnan(got))
    _check('zsq/df%g/D%d' % (df, D), {'log_q': float(mm.units(got, ref).max())})


@pytest.mark.parametrize('df', [8.0])
def test_t_log_weights_past_the_overflow_of_z_squared(df):
    """The log-weight kernels' host-noise form (logq1s at D = 2, logq1 at D = 18) reads
    z back from x: at log sigma = -400 and draws up to 1e300 the log weight stays
    finite and within the log_w bar."""
    from viabel_amd import vb, targets, experiments
    for D in (2, 18):
        lam = np.concatenate([np.zeros(D), np.full(D, -400.0)])
        eps = np.zeros((len(mc.Z_EDGES), D))
        eps[:, 0] = mc.Z_EDGES
        fam = _family(vb, 't', df, D, [eps])
        x, lw = experiments.log_weights(targets.isogauss(D), fam, lam, eps.shape[0])
        ref = mm.estimate('klvi', 't', df, 'isogauss', lam, eps)
        assert mm.finite(ref.lw)
        _check('zsq-logw/df%g/D%d' % (df, D), {'log_w': float(mm.units(lw, ref.lw).max())})


UPD_SHAPES = [('mixture', 2, 2, 'klvi', 'block'), ('mixture', 2, 2, 'chivi', 'block'),
              ('isogauss', 2, 2, 'klvi', 'block'),       # a gradient entry of exactly 0
              ('mixture', 18, 2, 'klvi', 'pair'), ('funnel', 17, 2, 'klvi', 'wide')]
UPD = [u + s for s in UPD_SHAPES for u in mc.UPDATE_CASES]


@pytest.mark.parametrize('W,steps,eps_ada,lr_end,target,D,N,objective,path', UPD)
def test_adagrad_update_step_by_step(W, steps, eps_ada, lr_end, target, D, N, objective, path):
    """Window wrap, W = 1, W past the step count, both sides of kBlockQpreMaxW = 16,
    eps << g^2, learning_rate_end, on every path.  lam after k steps comes from a
    fresh run advanced k steps in one launch chain (the fused multi-step forms: qpre,
    qnext, the ring loop, CHIVI's qo_pre), for every k.  The isogauss shape has
    mu_0 = 0 and eps_0 = 0 in every draw: d/dmu_0 = -mean x_0 is exactly 0 and mu_0
    must stay exactly 0.  The error of a step is measured in units of
    S_u = |lam'| + |step| + r G, G the gradient-carried terms of the module docstring
    and r = max(MF_ORACLE_ERR[mean], [log_sigma]) / MF_ORACLE_ERR[adagrad], against the
    bar 8 x MF_ORACLE_ERR[adagrad]: the update's own arithmetic gets 8 x its own
    record, the gradient's error 8 x the gradient's."""
    from viabel_amd import vb, targets
    from oracle import vb_oracle as vo
    rs = np.random.RandomState(W * 131 + D)
    eps = rs.randn(steps, N, D)
    lam0 = np.concatenate([0.3 * rs.randn(D), -0.5 + 0.1 * rs.randn(D)])
    if target == 'isogauss':
        eps[:, :, 0] = 0.0
        lam0[0] = 0.0
    tgt = _target(targets, target, D)
    lr0 = 0.05
    c = dict(objective=objective, kind='gauss', df=None, target=target, D=D, N=N, alpha=2.0)
    lams = [lam0]
    for k in range(1, steps + 1):
        fam = _family(vb, 'gauss', None, D, [])
        run = vb.DeviceRun(_objective(vb, c, fam, tgt), steps, lam0[None, :], window=W,
                           learning_rate=lr0, epsilon=eps_ada, learning_rate_end=lr_end)
        run.advance_host(eps[None, :k])
        lams.append(run.result(history=False)[0][0].copy())
    if target == 'isogauss':
        assert all(l[0] == 0.0 for l in lams)
    lrs = vo.learning_rate_schedule(steps, lr0, lr_end)
    grads = [mm.estimate(objective, 'gauss', None, target, lams[i], eps[i], 2.0).grad
             for i in range(steps)]
    if target == 'isogauss':
        assert all(g.hi[0] == 0.0 and g.lo[0] == 0.0 for g in grads)
    r = max(mm.MF_ORACLE_ERR['mean'], mm.MF_ORACLE_ERR['log_sigma']) / mm.MF_ORACLE_ERR['adagrad']
    worst = 0.0
    for i in range(steps):
        win = range(max(0, i + 1 - W), i + 1)
        G = np.array([grads[k].hi for k in win])
        ref, step = mm.adagrad_update(lams[i], G, lrs[i], eps_ada)
        assert mm.finite(ref)
        q = eps_ada + np.sum(G * G, axis=0)
        carried = (lrs[i] * grads[i].S / np.sqrt(q)
                   + np.abs(step) / q * sum(np.abs(grads[k].hi) * grads[k].S for k in win))
        e = mm.units(lams[i + 1], mm.Val(ref.hi, ref.lo, ref.S + r * carried))
        worst = max(worst, float(e.max()))
    _check('update/%s/%s/%s/D%d/W%d/eps%g/end%s' % (path, target, objective, D, W, eps_ada, lr_end),
           {'adagrad': worst})


BOUNDARY = [('block', 'mixture', 2, 5), ('pair', 'mixture', 18, 5), ('wide', 'funnel', 17, 5)]


@pytest.mark.parametrize('path,target,D,N', BOUNDARY)
def test_step_kernels_t_log_q_domain(path, target, D, N):
    """The step kernels (block_kernel, sep_kernel, mfw_rows_kernel) form the t
    family's log1p(eps^2 / df) from the draw itself and were not changed: eps * eps
    overflows from |eps| = 1.34e154 on.  KLVI_PD (the value holds mean log q) with one
    host draw planted at eps = 1e153 and at 1e155, log sigma = -400 in that column so
    that x stays small: below the boundary the value is within the value bar and
    finite; above it the fused kernels' value is infinite, never NaN, the materialised
    path's (measured: its host-noise log q goes through the form that switches above
    2^500) stays within the bar, and the gradient (which does not hold log q) stays
    finite."""
    from viabel_amd import vb, targets
    rs = np.random.RandomState(D)
    lam = np.concatenate([0.3 * rs.randn(D), np.full(D, -0.7)])
    # mu_0 = 0: x_0 = sigma_0 eps_0 exactly, so the materialised path, which reads z
    # back from x, sees the same z as the fused kernels
    lam[0], lam[D] = 0.0, -400.0
    tgt = _target(targets, target, D)
    for z in (1e153, 1e155):
        eps = rs.standard_t(8.0, size=(N, D))
        eps[N // 2, 0] = z
        fam = _family(vb, 't', 8.0, D, [eps])
        v, g = vb.black_box_klvi_pd(fam, tgt, N)(lam)
        ref = mm.estimate('klvi_pd', 't', 8.0, target, lam, eps)
        assert mm.finite(ref.value)
        print('MF_EDGE domain/%s |eps| = %g: value %r (reference %r)' % (path, z, v, ref.value.hi))
        assert not np.isnan(v) and np.all(np.isfinite(g))
        if z < 1.3e154 or path == 'wide':
            # (the materialised path's host-noise log q is the switched form: within the
            # bar on both sides)
            _check('domain/%s/%s' % (path, 'below' if z < 1.3e154 else 'above'),
                   {'value': float(mm.units(v, ref.value))})
        else:
            assert np.isinf(v)


@pytest.mark.parametrize('eps_ia', [1e-6, 1e-300])
@pytest.mark.parametrize('which', ['rmsprop', 'adam'])
@pytest.mark.parametrize('target,D,N,objective,path', UPD_SHAPES)
def test_ia_update_step_by_step(target, D, N, objective, path, which, eps_ia):
    """RMSProp-IA and Adam-IA for 3 steps (i = 0 is special-cased; Adam corrects with
    the power i + 2), as test_adagrad_update_step_by_step: lam after k steps from a
    fresh run of k steps, each step against the multiprecision update applied to the
    device's own previous lam with the moments rebuilt from the multiprecision
    gradients at the device's own lams.  With s = sum_k c_k g_k^2 (RMSProp; Adam:
    v-hat likewise with weights b_k, m-hat = sum_k a_k g_k) the gradient-carried
    terms are  lr S_g,i / sqrt(eps + s) + |step| / (eps + s) sum_k c_k |g_k| S_g,k
    (Adam: lr sum_k a_k S_g,k / sqrt(eps + v-hat) + |step| / (eps + v-hat) sum_k b_k
    |g_k| S_g,k), weighted as in the adagrad test."""
    from viabel_amd import vb, targets, _native as nat
    steps = 3
    rs = np.random.RandomState(D + len(which))
    eps = rs.randn(steps, N, D)
    lam0 = np.concatenate([0.3 * rs.randn(D), -0.5 + 0.1 * rs.randn(D)])
    if target == 'isogauss':
        eps[:, :, 0] = 0.0
        lam0[0] = 0.0
    tgt = _target(targets, target, D)
    lr = 0.05
    c = dict(objective=objective, kind='gauss', df=None, target=target, D=D, N=N, alpha=2.0)
    opt = nat.OPT_RMSPROP_IA if which == 'rmsprop' else nat.OPT_ADAM_IA
    lams = [lam0]
    for k in range(1, steps + 1):
        fam = _family(vb, 'gauss', None, D, [])
        run = vb.DeviceRun(_objective(vb, c, fam, tgt), steps, lam0[None, :], window=500,
                           learning_rate=lr, epsilon=eps_ia, optimizer=opt)
        run.advance_host(eps[None, :k])
        lams.append(run.result(history=False)[0][0].copy())
    grads = [mm.estimate(objective, 'gauss', None, target, lams[i], eps[i], 2.0).grad
             for i in range(steps)]
    r = max(mm.MF_ORACLE_ERR['mean'], mm.MF_ORACLE_ERR['log_sigma']) / mm.MF_ORACLE_ERR[which]
    worst = 0.0
    for i in range(steps):
        G = np.array([g.hi for g in grads[:i + 1]])
        GS = np.array([g.S for g in grads[:i + 1]])
        ref, step = mm.ia_update(which, lams[i], G, lr, eps_ia)
        assert mm.finite(ref)
        if which == 'rmsprop':
            ck = np.array([1.0 if i == 0 else (0.9 ** i if k == 0 else 0.1 * 0.9 ** (i - k))
                           for k in range(i + 1)])
            den = eps_ia + np.sum(ck[:, None] * G * G, axis=0)
            carried = (lr * GS[i] / np.sqrt(den)
                       + np.abs(step) / den * np.sum(ck[:, None] * np.abs(G) * GS, axis=0))
        else:
            ak = np.array([(0.9 ** (i + 1) if k == 0 else 0.1 * 0.9 ** (i - k)) for k in range(i + 1)])
            bk = np.array([(0.9 * 0.999 ** i if k == 0 else 0.001 * 0.999 ** (i - k))
                           for k in range(i + 1)])
            ak, bk = ak / (1 - 0.9 ** (i + 2)), bk / (1 - 0.999 ** (i + 2))
            den = eps_ia + np.sum(bk[:, None] * G * G, axis=0)
            carried = (lr * np.sum(ak[:, None] * GS, axis=0) / np.sqrt(den)
                       + np.abs(step) / den * np.sum(bk[:, None] * np.abs(G) * GS, axis=0))
        e = mm.units(lams[i + 1], mm.Val(ref.hi, ref.lo, ref.S + r * carried))
        worst = max(worst, float(e.max()))
    if target == 'isogauss':
        assert all(l[0] == 0.0 for l in lams)
    _check('%s/%s/%s/%s/D%d/eps%g' % (which, path, target, objective, D, eps_ia), {which: worst})


# ---- Philox instances and the block kernel's layout switches -------------------
PHILOX = [(kind, df, target, D, N, obj)
          for kind, df in [('gauss', None), ('t', 8.0)]
          for target, D, N in [('mixture', 2, 64), ('funnel', 10, 128), ('eight_schools_ncp', 10, 100),
                               ('mixture', 9, 129), ('mixture', 18, 128)]
          for obj in (['klvi', 'klvi_pd'] if D > 16 else ['klvi', 'klvi_pd', 'chivi'])]
SEED, STREAM = 11, 9


def _philox_one_step(cases):
    """Per case: (value of step 0, lam after it) of a one-step Philox run (in-kernel
    draws; the t family's log q through log1p_pos_tab)."""
    from viabel_amd import vb, targets
    out = []
    for kind, df, target, D, N, obj in cases:
        fam = (vb.mean_field_gaussian_variational_family(D, rng='philox') if kind == 'gauss'
               else vb.mean_field_t_variational_family(D, df, rng='philox'))
        c = dict(objective=obj, N=N, alpha=2.0)
        rs = np.random.RandomState(D * 1000 + N)
        lam0 = np.concatenate([0.3 * rs.randn(D), -0.5 + 0.1 * rs.randn(D)])
        run = vb.DeviceRun(_objective(vb, c, fam, _target(targets, target, D)), 1, lam0[None, :],
                           window=10, learning_rate=0.05, epsilon=0.1)
        run.advance_philox(1, SEED, STREAM, 0)
        lam, _, vals, _ = run.result(history=False)
        out.append((lam0, float(vals[0, 0]), lam[0].copy()))
    return out


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import test_gpu_mf_edges as t
res = t._philox_one_step(t.PHILOX)
np.savez(sys.argv[2], vals=np.array([r[1] for r in res]),
         **{'lam%d' % k: r[2] for k, r in enumerate(res)})
"""


@pytest.fixture(scope='module')
def philox_refs():
    """The draws of oracle/vbrng.c for (SEED, STREAM, step 0) and the multiprecision
    one-step reference on them, once for every switch setting."""
    from oracle import rng_oracle as ro
    refs = []
    for kind, df, target, D, N, obj in PHILOX:
        rs = np.random.RandomState(D * 1000 + N)
        lam0 = np.concatenate([0.3 * rs.randn(D), -0.5 + 0.1 * rs.randn(D)])
        eps = ro.noise(SEED, STREAM, 0, N, D, kind, df or 0.0)
        est = mm.estimate(obj, kind, df, target, lam0, eps, 2.0)
        upd, step = mm.adagrad_update(lam0, est.grad.hi[None, :], 0.05, 0.1)
        refs.append((lam0, est, upd, step))
    return refs


@pytest.mark.parametrize('switch', ['default', 'PREDRAW=0', 'PREDRAW=all', 'BLOCK_SPLIT=0',
                                    'BLOCK_SPLIT=0,PREDRAW=0'])
def test_philox_instances_under_the_layout_switches(switch, philox_refs, monkeypatch, tmp_path):
    """One Philox step of the block kernel (D <= 10 with N <= 128: split rows unless
    VIABEL_AMD_BLOCK_SPLIT=0; N = 129: several samples per thread) and of the
    column-pair kernel, in-kernel draws (VIABEL_AMD_PREDRAW=0) and pre-drawn (=all;
    the t family always pre-draws), against the multiprecision estimator on the draws
    of oracle/vbrng.c.  sample_kernel does not share the step kernels' draw routine
    (normal_pair / library sqrt against the table forms and rsqrt_pos), so
    vb_family_sample is not the source of the draws; the C restatement's differ from
    the kernels' by ~1 ulp of eps, that is 2 units of |sigma eps| in x, which every
    condition sum already holds (dx_d = |mu_d| + |sigma_d eps_nd| weighs |g| in S of
    log p and the curvature in S of g; eps^2 / 2 and the log1p term weigh log q), so
    no further term is added and the bars are the host-noise ones.
    VIABEL_AMD_BLOCK_SPLIT is read once per process: those settings run in a child."""
    env = dict(kv.split('=') for kv in switch.split(',')) if switch != 'default' else {}
    env = {'VIABEL_AMD_' + k: v for k, v in env.items()}
    if 'VIABEL_AMD_BLOCK_SPLIT' in env:
        import subprocess
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        f = str(tmp_path / 'child.npz')
        r = subprocess.run([sys.executable, '-c', _CHILD, root, f], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        z = np.load(f)
        res = [(None, float(z['vals'][k]), z['lam%d' % k]) for k in range(len(PHILOX))]
    else:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res = _philox_one_step(PHILOX)
    r_g = max(mm.MF_ORACLE_ERR['mean'], mm.MF_ORACLE_ERR['log_sigma']) / mm.MF_ORACLE_ERR['adagrad']
    bad = []
    for case, (_, v, lam1), (lam0, est, upd, step) in zip(PHILOX, res, philox_refs):
        q = 0.1 + est.grad.hi ** 2
        carried = 0.05 * est.grad.S / np.sqrt(q) + np.abs(step) / q * np.abs(est.grad.hi) * est.grad.S
        errs = {'value': float(mm.units(v, est.value)),
                'adagrad': float(mm.units(lam1, mm.Val(upd.hi, upd.lo, upd.S + r_g * carried)).max())}
        try:
            _check('philox/%s/%s%s/%s/D%d/N%d/%s' % ((switch, case[0], case[1] or '') + case[2:]), errs)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad
