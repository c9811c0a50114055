"""Device model plugins (VB_TARGET_PLUGIN) on the GPU: the shipped models of
viabel_amd/models, loaded as code objects, give the numpy restatement's values,
gradients and trajectories through every family, objective and optimiser of the
materialised path.  The reference side is targets.callback of the restatement on the
same numpy-stream draws, so only the target's evaluation order differs: 1e-11 relative
for one call's value and gradient, 1e-10 for trajectories (tests/test_gpu_callback.py's
tolerances for the same kind of comparison).  Shapes are the edges of the two launch
forms (256 rows per block; 4 rows per block and 64 lanes per row), not workloads.  No
test loads a deliberately faulty kernel."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import notebook_cases as nc
from tests import plugin_cases as pc
from tests.conftest import ROOT, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b))) / scale
    assert err <= rtol, err


def _lam(D, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([0.3 * rs.randn(D), -0.5 + 0.2 * rs.randn(D)])


def _direct(plug, ref, D, n, seed=3):
    """log weights (null gradient) and one KLVI value + gradient of `plug` against the
    callback of the restatement `ref`, on the same draws."""
    from viabel_amd import vb, targets, experiments
    lam = _lam(D, seed)
    f1 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    f2 = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    cb = targets.callback(ref, D)
    np.random.seed(seed)
    x1, lw1 = experiments.log_weights(plug, f1, lam, n)
    np.random.seed(seed)
    x2, lw2 = experiments.log_weights(cb, f2, lam, n)
    _close(x1, x2, 1e-14)
    _close(lw1, lw2, 1e-11)
    np.random.seed(seed + 1)
    v1, g1 = vb.black_box_klvi(f1, plug, n)(lam)
    np.random.seed(seed + 1)
    v2, g2 = vb.black_box_klvi(f2, cb, n)(lam)
    np.testing.assert_allclose(v1, v2, rtol=1e-11)
    _close(g1, g2, 1e-11)


@pytest.mark.parametrize('D', [1, 3, 17])
def test_rows_form_direct(D):
    from viabel_amd import targets
    plug = targets.example_model('banana', D)
    assert plug.launch == pc.LAUNCH['banana']
    for n in (1, 255, 256, 257):
        _direct(plug, pc.banana(), D, n)


@pytest.mark.parametrize('D', [1, 2, pc.RR_DMAX])
def test_sum_form_direct(D):
    from viabel_amd import targets
    for M in (1, 63, 64, 65, 130):
        x, y = pc.robust_regression_data(M, D)
        plug = targets.example_model('robust_regression', x, y, 4.0)
        assert plug.launch == pc.LAUNCH['robust_regression']
        for n in (1, 3, 4, 5):
            _direct(plug, pc.robust_regression(x, y, 4.0), D, n)


def test_raw_kernel_direct():
    """The hand-written kernel with its own launch record (blocks of 128 rows)."""
    from viabel_amd import targets
    plug = targets.example_model('isogauss_raw', 5)
    assert plug.launch == pc.LAUNCH['isogauss_raw']
    for n in (1, 127, 128, 129):
        _direct(plug, pc.isogauss, 5, n)
    lp, g = plug.logdensity_and_grad(np.linspace(-1, 1, 15).reshape(3, 5))
    rlp, rg = pc.isogauss(np.linspace(-1, 1, 15).reshape(3, 5))
    _close(lp, rlp, 1e-13)
    _close(g, rg, 1e-13)


def test_device_resident_data_used_in_place():
    import torch
    from viabel_amd import targets
    D, M = 2, 65
    x, y = pc.robust_regression_data(M, D)
    block = torch.tensor(pc.robust_regression_block(x, y, 4.0), dtype=torch.float64, device='cuda')
    plug = targets.device_model(pc.hsaco('robust_regression'), D, data=block)
    assert plug.params is None and plug.data_device is block
    _direct(plug, pc.robust_regression(x, y, 4.0), D, 5)


# ---- the same answer through every family, objective and optimiser --------------------

RR_D, RR_M, RR_NU, RR_N = 3, 65, 4.0, 30


@pytest.fixture(scope='module')
def rr():
    from viabel_amd import targets
    x, y = pc.robust_regression_data(RR_M, RR_D)
    return (targets.example_model('robust_regression', x, y, RR_NU),
            targets.callback(pc.robust_regression(x, y, RR_NU), RR_D))


def _families():
    from viabel_amd import vb
    D = RR_D
    tril = 0.05 * np.random.RandomState(2).randn(D * (D + 1) // 2)
    return {
        'mf_gauss': (lambda: vb.mean_field_gaussian_variational_family(D, rng='numpy'), _lam(D, 5)),
        'mf_t': (lambda: vb.mean_field_t_variational_family(D, 40.0, rng='numpy'), _lam(D, 6)),
        'fr_t': (lambda: vb.t_variational_family(D, 100.0, rng='numpy'),
                 np.concatenate([0.1 * np.ones(D), tril])),
        'cholesky': (lambda: vb.cholesky_gaussian_variational_family(D, rng='numpy'),
                     np.concatenate([0.1 * np.ones(D), tril])),
        'low_rank': (lambda: vb.low_rank_gaussian_variational_family(D, 1, rng='numpy'),
                     np.concatenate([0.1 * np.ones(D), -0.4 * np.ones(D),
                                     0.2 * np.random.RandomState(4).randn(D)])),
    }


@pytest.mark.parametrize('family,objective', [
    ('mf_gauss', 'klvi'), ('mf_gauss', 'chivi'), ('mf_gauss', 'klvi_pd'), ('mf_t', 'klvi'),
    ('fr_t', 'klvi'), ('cholesky', 'klvi'), ('low_rank', 'klvi')])
def test_same_answer_through_every_family(rr, family, objective):
    from viabel_amd import vb
    make, lam = _families()[family]
    out = []
    for target in rr:
        fam = make()
        if objective == 'klvi':
            obj = vb.black_box_klvi(fam, target, RR_N)
        elif objective == 'klvi_pd':
            obj = vb.black_box_klvi_pd(fam, target, RR_N)
        else:
            obj = vb.black_box_chivi(2.0, fam, target, RR_N)
        np.random.seed(11)
        out.append(obj(lam))
    (v1, g1), (v2, g2) = out
    np.testing.assert_allclose(v1, v2, rtol=1e-11)
    _close(g1, g2, 1e-11)


def test_adagrad_trajectory(rr):
    from viabel_amd import vb
    res = []
    for target in rr:
        fam = vb.mean_field_gaussian_variational_family(RR_D, rng='numpy')
        np.random.seed(21)
        res.append(vb.adagrad_optimize(40, vb.black_box_klvi(fam, target, RR_N),
                                       np.zeros(2 * RR_D), learning_rate=0.05))
    _close(res[0][1], res[1][1], 1e-10)   # history
    _close(res[0][0], res[1][0], 1e-10)   # final (smoothed) parameters
    _close(res[0][2], res[1][2], 1e-10)   # values


def test_rmsprop_ia_trajectory(rr):
    from viabel_amd import vb
    kw = dict(window=10, rhat_window=10, n_optimisers=2, tail_avg_iters=10)
    res = []
    for target in rr:
        fam = vb.mean_field_gaussian_variational_family(RR_D, rng='numpy')
        np.random.seed(22)
        res.append(vb.rmsprop_IA_optimize_with_rhat(40, vb.black_box_klvi(fam, target, RR_N),
                                                    np.zeros(2 * RR_D), RR_D, **kw))
    _close(res[0][1], res[1][1], 1e-10)   # history chains
    _close(res[0][0], res[1][0], 1e-10)   # final parameters
    _close(res[0][4], res[1][4], 1e-10)   # values


# ---- the notebook's runs through the plugin (the printed digits) ------------------------

def _notebook_target():
    from viabel_amd import targets
    x, y = nc.robust_regression_data()
    return targets.example_model('robust_regression', x, y, 40.0)


def test_robust_regression_mean_field_klvi_notebook_plugin():
    from viabel_amd import vb
    from tests.test_gpu_notebooks import _run
    s = nc.RR_MF
    _run('robust_regression_mf_klvi',
         vb.mean_field_t_variational_family(s['D'], s['df'], rng='numpy'), _notebook_target(), s)


def test_robust_regression_full_rank_klvi_notebook_plugin():
    from viabel_amd import vb
    from tests.test_gpu_notebooks import _run
    s = nc.RR_FR
    _run('robust_regression_fullrank_klvi', vb.t_variational_family(s['D'], s['df'], rng='numpy'),
         _notebook_target(), s)


# ---- repeatability, refusals, lifetime -------------------------------------------------

def test_same_call_same_bits(rr):
    from viabel_amd import vb, experiments
    plug = rr[0]
    lam = _lam(RR_D, 9)
    out = []
    for _ in range(2):
        fam = vb.mean_field_gaussian_variational_family(RR_D, rng='numpy')
        np.random.seed(31)
        _, lw = experiments.log_weights(plug, fam, lam, 257)
        np.random.seed(32)
        v, g = vb.black_box_klvi(fam, plug, 130)(lam)
        out.append((lw, v, g))
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2])


def test_refuses_dim_above_dmax():
    from viabel_amd import vb, targets
    D = pc.RR_DMAX + 1
    x, y = pc.robust_regression_data(5, D)
    plug = targets.example_model('robust_regression', x, y, 4.0)
    fam = vb.mean_field_gaussian_variational_family(D, rng='numpy')
    with pytest.raises(ValueError, match='dmax'):
        vb.black_box_klvi(fam, plug, 8)(np.zeros(2 * D))
    with pytest.raises(ValueError, match='dmax'):
        plug.logdensity_and_grad(np.zeros((2, D)))


def test_refuses_family_of_another_dimension():
    from viabel_amd import vb, targets
    plug = targets.example_model('banana', 3)
    with pytest.raises(ValueError, match='dimension'):
        vb.black_box_klvi(vb.mean_field_gaussian_variational_family(4, rng='numpy'), plug, 8)
    # dim=None binds to the family's dimension, as callback does
    open_dim = targets.device_model(pc.hsaco('banana'))
    assert open_dim.dim is None
    fam = vb.mean_field_gaussian_variational_family(4, rng='numpy')
    v, g = vb.black_box_klvi(fam, open_dim, 8)(np.zeros(8))
    assert np.isfinite(v) and g.shape == (8,)


def test_refuses_handle_of_another_device():
    import ctypes
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs more than one visible device')
    from viabel_amd import _native as nat
    image = open(pc.hsaco('banana'), 'rb').read()
    other = nat.Context(1)
    p = nat.Plugin(other, image)
    try:
        t = nat.Target(nat.TARGET_PLUGIN, 0, 2, None, 0, nat.TARGET_CALLBACK_T(),
                       ctypes.c_void_p(p.handle.value))
        x, lp = np.zeros((1, 2)), np.zeros(1)
        with pytest.raises(ValueError, match='GPU'):
            nat.check(nat.lib().vb_target_logdensity(nat.context(0).handle, t, nat.dptr(x), 1,
                                                     nat.dptr(lp), None))
    finally:
        assert p.release() == nat.VB_OK


def test_run_outlives_the_python_target():
    """A vb_run holds its own reference: it keeps working after the target object (and
    with it the caller's reference) is gone, and the handle's last reference goes with
    the run."""
    from viabel_amd import vb, targets, _native as nat
    x, y = pc.robust_regression_data(RR_M, RR_D)
    ref = targets.callback(pc.robust_regression(x, y, RR_NU), RR_D)
    fam = vb.mean_field_gaussian_variational_family(RR_D, rng='numpy')
    plug = targets.example_model('robust_regression', x, y, RR_NU)
    run = vb.DeviceRun(vb.black_box_klvi(fam, plug, RR_N), 6, np.zeros((1, 2 * RR_D)))
    handle = plug.plugin()
    run.obj = None
    del plug
    gc.collect()
    handle_value = handle.handle.value
    assert handle.release() == nat.VB_OK       # the caller's reference
    del handle
    gc.collect()
    eps = np.random.RandomState(41).randn(1, 6, RR_N, RR_D)
    run.advance_host(eps)
    got = run.result()
    rrun = vb.DeviceRun(vb.black_box_klvi(fam, ref, RR_N), 6, np.zeros((1, 2 * RR_D)))
    rrun.advance_host(eps)
    want = rrun.result()
    _close(got[0], want[0], 1e-10)
    _close(got[2], want[2], 1e-10)
    # the run's reference is the last: destroying the run releases it with VB_OK, after
    # which the handle is no longer live
    h, run.handle = run.handle, None
    assert nat.lib().vb_run_destroy(h) == nat.VB_OK
    assert nat.lib().vb_plugin_info(handle_value, None, None, None) == nat.VB_EINVAL


def test_last_release_after_run_destroyed():
    import ctypes
    from viabel_amd import vb, targets, _native as nat
    fam = vb.mean_field_gaussian_variational_family(3, rng='numpy')
    plug = targets.example_model('banana', 3)
    run = vb.DeviceRun(vb.black_box_klvi(fam, plug, 8), 2, np.zeros((1, 6)))
    run.advance_host(np.random.RandomState(1).randn(1, 2, 8, 3))
    h, run.handle = run.handle, None
    assert nat.lib().vb_run_destroy(h) == nat.VB_OK
    p = plug.plugin()
    assert p.info() == pc.LAUNCH['banana']
    assert p.release() == nat.VB_OK
    assert p.release() == nat.VB_OK            # idempotent on the Python object
    del ctypes


_RELOAD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from viabel_amd import vb, targets, _native as nat
from tests import plugin_cases as pc
plug = targets.example_model('banana', 3)
x = np.linspace(-1, 1, 12).reshape(4, 3)
a = plug.logdensity_and_grad(x)
nat.release_all()
assert not plug._plugins or all(not p.handle for p in plug._plugins.values())
b = plug.logdensity_and_grad(x)          # a new context: the module is loaded again
fresh = targets.device_model(pc.hsaco('banana'), 3, data=np.array([10.0, 0.03]))
c = fresh.logdensity_and_grad(x)
ref = pc.banana()(x)
for got in (a, b, c):
    assert np.allclose(got[0], ref[0], rtol=1e-12) and np.allclose(got[1], ref[1], rtol=1e-12)
print('RELOAD OK')
'''


def test_device_model_reloads_after_release_all():
    """release_all ends the process's use of the library, so this runs in a child."""
    r = subprocess.run([sys.executable, '-c', _RELOAD % ROOT], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and b'RELOAD OK' in r.stdout, r.stdout.decode('utf-8', 'replace')
