"""Every target kind through every entry point and path that evaluates it, bit for bit
against tests/golden/target_paths_parent_bits.npz: vb_target_logdensity with and without
the gradient, one value-and-gradient, three adagrad steps and vb_log_weights with samples,
on the materialised mean-field path, the full-rank t, the Cholesky Gaussian and the
low-rank Gaussian (rank 2).  The fixture was recorded on an MI355X by
scripts/make_target_paths_fixture.py with the build of the commit before the host side got
one target descriptor (vbk::Target) and one evaluation entry (target_eval); the cases,
shapes and seeds are that script's."""
import importlib.util
import os

import numpy as np
import pytest

from tests.conftest import ROOT, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


def _load():
    spec = importlib.util.spec_from_file_location(
        'make_target_paths_fixture', os.path.join(ROOT, 'scripts', 'make_target_paths_fixture.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MOD = _load()


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'target_paths_parent_bits.npz'))


def test_the_cases_cover_every_kind_and_path(gold):
    keys = [c[0] for c in MOD.CASES]
    assert len(set(keys)) == len(keys) == 24
    for kind in ('isogauss', 'mixture', 'funnel', 'eight_schools_ncp', 'corr_gauss', 'hier_nc',
                 'hier_c', 'mlm_gaussian_nc', 'mlm_gaussian_c', 'plugin', 'callback',
                 'reg_learn_scale', 'reg_learn_phi', 'reg_gaussian_m65', 'mlm_gaussian_nc_m65',
                 'reg_gaussian', 'reg_student_t', 'reg_bernoulli_logit', 'reg_poisson_log',
                 'reg_neg_binomial_2_log'):
        assert any(k.startswith(kind) for k in keys), kind
    # every family leg of every case, and both logdensity legs, are in the fixture
    want = set()
    for key, _, fams, _, _ in MOD.CASES:
        want |= {key + '.ld.lp', key + '.ld.g', key + '.ld_nograd.lp'}
        for f in fams:
            want |= {'%s.%s.%s' % (key, f, part) for part in
                     ('value', 'grad', 'run_lam', 'run_hist', 'run_vals', 'run_smooth', 'lw', 'lw_x')}
    assert want == set(gold.files)
    # the learned dispersion's table is not empty
    assert MOD.CASES[keys.index('reg_learn_phi')][1]().params.size > 8 + 6 * 3 + 6 + 6 + 1 + 1


@pytest.mark.parametrize('case', MOD.CASES, ids=[c[0] for c in MOD.CASES])
def test_every_path_gives_the_bits_it_gave_before(case, gold):
    got = MOD.evaluate_case(*case)
    assert got and all(k in gold.files for k in got)
    for k in sorted(got):
        assert np.all(np.isfinite(got[k])), k
        np.testing.assert_array_equal(got[k], gold[k], err_msg=k)
