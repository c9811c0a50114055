"""The column-pair kernel keeps every output bit (tests/sep_bits_cases.py has the
shapes and why; tests/golden/sep_bits.npz was recorded by
scripts/make_sep_bits_fixture.py from the build before the kernel's instruction-count
work).  Every case: lam, vals, smooth and the history rows equal the recorded ones
exactly -- at the stored columns value by value, over all columns by sha256."""
import os

import numpy as np
import pytest

from tests import sep_bits_cases as sc
from tests.conftest import ROOT, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


@pytest.fixture(scope='module')
def recorded():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'sep_bits.npz'))
    assert [tuple(c) for c in z['cases']] == sc.CASES
    np.testing.assert_array_equal(z['cols'], sc.PCOLS)
    return z


@pytest.mark.parametrize('k', range(len(sc.CASES)), ids=['N%d-W%d' % c for c in sc.CASES])
def test_sep_kernel_bits(recorded, k):
    n, w = sc.CASES[k]
    got = sc.record(n, w)
    for name in ('vals', 'lam', 'smooth', 'hist'):
        assert np.all(np.isfinite(got[name])), name
        np.testing.assert_array_equal(got[name], recorded[name][k], err_msg=name)
        # (assert_array_equal takes -0 == +0: the bytes settle it)
        assert got[name].tobytes() == np.ascontiguousarray(recorded[name][k]).tobytes(), name
    np.testing.assert_array_equal(got['sha256'], recorded['sha256'][k],
                                  err_msg='a column outside the stored ones differs')
