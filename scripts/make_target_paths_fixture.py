"""Write tests/golden/target_paths_parent_bits.npz: every target kind through every entry
point and path that evaluates it, from the library that is loaded (VIABEL_AMD_LIB selects
a build).  Recorded once on an MI355X from the build of the commit before the host side
got one target descriptor (vbk::Target) and one evaluation entry (target_eval);
tests/test_gpu_target_paths.py asks the current build for the same bits ever after.

  VIABEL_AMD_LIB=$PWD/viabel_amd/libviabel_amd_parent.so \
      python scripts/make_target_paths_fixture.py [OUT.npz]

Per case: vb_target_logdensity with and without the gradient, and per family that accepts
the target one value-and-gradient, three adagrad steps and vb_log_weights with samples.
The families are the mean-field Gaussian on the materialised path, the full-rank t, the
Cholesky Gaussian and the low-rank Gaussian at rank 2.  Data, parameters and draws (host
noise, numpy streams) are seeded here, so the file holds the results only.

Shapes: N = 5 samples per step, m = 7 log-weight draws and rows, M = 6 observations,
D = 3 to 5.  What takes another route at another size has a case there:
  * the mean-field Gaussian evaluates a target with a parameter block, a plugin or a
    callback on the materialised path at any D; a built-in target only at D > 16, and a
    separable one (isogauss, mixture) only under CHIVI, so those legs run at D = 17;
    eight_schools_ncp has D = 10, and only a run whose window exceeds 64 steps is
    materialised there;
  * glm_scratch_doubles (csrc/vb_glm.hip) is zero while the observations fit one
    64-observation chunk and first positive at M = 65 (two chunks), at any D;
    mlm_scratch_doubles (csrc/vb_mlm.hip) is positive at every M and grows to two chunks
    at M = 65.  Both have a case at M = 65.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M_DRAWS, M_OBS, M_CHUNKED, STEPS = 5, 7, 6, 65, 3
FAMILIES = ('mf', 'frt', 'chol', 'lr2')
OBJ_KLVI, OBJ_CHIVI = 'klvi', 'chivi'


def _data(p, m, lik, seed=41):
    rs = np.random.RandomState(seed)
    x = rs.randn(m, p)
    eta = x @ (0.4 * rs.randn(p))
    if lik == 'bernoulli_logit':
        y = (rs.rand(m) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif lik in ('poisson_log', 'neg_binomial_2_log'):
        y = 1.0 + rs.poisson(np.exp(eta + 0.5)).astype(np.float64)   # max y >= 1: a table
    else:
        y = eta + 0.3 * rs.randn(m)
    return x, y, 0.1 * rs.randn(m)


def _regression(lik, m=M_OBS, **kw):
    def build():
        from viabel_amd import targets
        x, y, off = _data(3, m, lik)
        if lik in ('poisson_log', 'neg_binomial_2_log'):
            kw.setdefault('offset', off)
        if lik == 'neg_binomial_2_log' and not kw.get('learn_phi'):
            kw.setdefault('phi', 2.5)
        if lik == 'student_t':
            kw.setdefault('df', 4.0)
        return targets.regression(x, y, lik, **kw)
    return build


def _multilevel(lik, centered, m=M_OBS):
    def build():
        from viabel_amd import targets
        x, y, off = _data(1, m, lik)
        group = np.arange(m) % 2
        kw = {'offset': off} if lik == 'poisson_log' else {}
        return targets.multilevel_regression(x, y, group, lik, centered=centered, n_groups=2, **kw)
    return build


def _hierarchical(centered):
    def build():
        from viabel_amd import targets
        return targets.hierarchical_normal([1.5, -0.5], [1.0, 2.0], centered=centered)
    return build


def _plugin():
    from viabel_amd import targets
    x, y, _ = _data(3, M_OBS, 'student_t')
    return targets.example_model('robust_regression', x, y, 4.0)


def callback_fn(x):
    """The one host callback: N(0.3, I) without its constant, in plain numpy."""
    r = x - 0.3
    return -0.5 * np.sum(r * r, axis=1), -r


def _callback():
    from viabel_amd import targets
    return targets.callback(callback_fn, 3)


def _builtin(name, dim=None):
    def build():
        from viabel_amd import targets
        return getattr(targets, name)(*(() if dim is None else (dim,)))
    return build


# (key, target builder, families, objective of the value-and-gradient and the run,
#  adagrad window)
CASES = [
    ('isogauss3', _builtin('isogauss', 3), ('frt', 'chol', 'lr2'), OBJ_KLVI, 10),
    ('mixture3', _builtin('mixture', 3), ('frt', 'chol', 'lr2'), OBJ_KLVI, 10),
    ('funnel3', _builtin('funnel', 3), ('frt', 'chol', 'lr2'), OBJ_KLVI, 10),
    ('isogauss17', _builtin('isogauss', 17), ('mf',), OBJ_CHIVI, 10),
    ('mixture17', _builtin('mixture', 17), ('mf',), OBJ_CHIVI, 10),
    ('funnel17', _builtin('funnel', 17), ('mf',), OBJ_KLVI, 10),
    ('eight_schools_ncp', _builtin('eight_schools_ncp'), FAMILIES, OBJ_KLVI, 65),
    ('corr_gauss4', _builtin('corr_gauss', 4), ('frt', 'chol', 'lr2'), OBJ_KLVI, 10),
    ('reg_gaussian', _regression('gaussian'), FAMILIES, OBJ_KLVI, 10),
    ('reg_student_t', _regression('student_t'), FAMILIES, OBJ_KLVI, 10),
    ('reg_bernoulli_logit', _regression('bernoulli_logit'), FAMILIES, OBJ_KLVI, 10),
    ('reg_poisson_log', _regression('poisson_log'), FAMILIES, OBJ_KLVI, 10),
    ('reg_neg_binomial_2_log', _regression('neg_binomial_2_log'), FAMILIES, OBJ_KLVI, 10),
    ('reg_learn_scale', _regression('gaussian', learn_scale=True), FAMILIES, OBJ_KLVI, 10),
    ('reg_learn_phi', _regression('neg_binomial_2_log', learn_phi=True), FAMILIES, OBJ_KLVI, 10),
    ('reg_gaussian_m65', _regression('gaussian', M_CHUNKED), FAMILIES, OBJ_KLVI, 10),
    ('hier_nc', _hierarchical(False), FAMILIES, OBJ_KLVI, 10),
    ('hier_c', _hierarchical(True), FAMILIES, OBJ_KLVI, 10),
    ('mlm_gaussian_nc', _multilevel('gaussian', False), FAMILIES, OBJ_KLVI, 10),
    ('mlm_gaussian_c', _multilevel('gaussian', True), FAMILIES, OBJ_KLVI, 10),
    ('mlm_poisson_log_nc', _multilevel('poisson_log', False), FAMILIES, OBJ_KLVI, 10),
    ('mlm_gaussian_nc_m65', _multilevel('gaussian', False, M_CHUNKED), FAMILIES, OBJ_KLVI, 10),
    ('plugin_robust_regression', _plugin, FAMILIES, OBJ_KLVI, 10),
    ('callback', _callback, FAMILIES, OBJ_KLVI, 10),
]


def _family(name, dim):
    from viabel_amd import vb
    if name == 'mf':
        return vb.mean_field_gaussian_variational_family(dim, rng='numpy')
    if name == 'frt':
        return vb.t_variational_family(dim, 8.0, rng='numpy')
    if name == 'chol':
        return vb.cholesky_gaussian_variational_family(dim, rng='numpy')
    return vb.low_rank_gaussian_variational_family(dim, 2, rng='numpy')


def _objective(kind, fam, target):
    from viabel_amd import vb
    if kind == OBJ_CHIVI:
        return vb.black_box_chivi(2.0, fam, target, N)
    return vb.black_box_klvi(fam, target, N)


def _logdensity(target, x, with_grad):
    from viabel_amd import _native as nat
    lp = np.empty(x.shape[0])
    g = np.empty_like(x) if with_grad else None
    nat.check(nat.lib().vb_target_logdensity(nat.context().handle, target._struct(), nat.dptr(x),
                                             x.shape[0], nat.dptr(lp),
                                             nat.dptr(g) if with_grad else None))
    return lp, g


def _value_grad(obj, lam, eps):
    from viabel_amd import _native as nat
    f, t, o = obj._structs()
    eps = nat.as_f64(eps)
    nz = nat.Noise(nat.NOISE_HOST, 0, 0, 0, nat.dptr(eps))
    val, grad = np.empty(1), np.empty(lam.size)
    nat.check(nat.lib().vb_objective_value_grad(nat.context().handle, f, t, o, nat.dptr(lam), nz,
                                                nat.dptr(val), nat.dptr(grad)))
    return val, grad


def _log_weights(fam, target, lam, eps):
    from viabel_amd import _native as nat
    eps = nat.as_f64(eps)
    nz = nat.Noise(nat.NOISE_HOST, 0, 0, 0, nat.dptr(eps))
    lw, xs = np.empty(M_DRAWS), np.empty((M_DRAWS, fam.dim))
    nat.check(nat.lib().vb_log_weights(nat.context().handle, fam._struct(), target._struct(),
                                       nat.dptr(lam), M_DRAWS, nz, nat.dptr(lw), nat.dptr(xs)))
    return lw, xs


def evaluate_case(key, build, fams, objective, window):
    """{array name: array} of one case on the loaded build."""
    from viabel_amd import _native as nat
    from viabel_amd import vb
    target = build()
    dim = target.dim
    res = {}
    x = nat.as_f64(0.5 * np.random.RandomState(5).randn(M_DRAWS, dim))
    res[key + '.ld.lp'], res[key + '.ld.g'] = _logdensity(target, x, True)
    res[key + '.ld_nograd.lp'] = _logdensity(target, x, False)[0]
    for name in fams:
        fam = _family(name, dim)
        lam = nat.as_f64(0.1 * np.random.RandomState(7).randn(fam.var_param_dim))
        obj = _objective(objective, fam, target)
        pre = '%s.%s.' % (key, name)
        res[pre + 'value'], res[pre + 'grad'] = _value_grad(obj, lam, fam._draw(N, 11))
        run = vb.DeviceRun(obj, STEPS, lam, window=window, learning_rate=0.05)
        run.advance_host(np.stack([np.asarray(fam._draw(N, 21 + s)) for s in range(STEPS)])[None])
        out = run.result()
        for part, arr in zip(('run_lam', 'run_hist', 'run_vals', 'run_smooth'), out):
            res[pre + part] = arr
        del run
        res[pre + 'lw'], res[pre + 'lw_x'] = _log_weights(fam, target, lam, fam._draw(M_DRAWS, 13))
    return res


def evaluate():
    res = {}
    for case in CASES:
        res.update(evaluate_case(*case))
    return res


def main(out=os.path.join(ROOT, 'tests', 'golden', 'target_paths_parent_bits.npz')):
    from viabel_amd import _native as nat
    res = evaluate()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **res)
    print('wrote %s (%d arrays, %d bytes) from %s build %s'
          % (out, len(res), os.path.getsize(out), nat.LIB_PATH, nat.lib().vb_build_id().decode()))


if __name__ == '__main__':
    main(*sys.argv[1:])
