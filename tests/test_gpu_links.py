"""The bits of the multilevel regression target (every likelihood, centred and non-centred,
lane and tile kernel, two chunks with a group on both sides of the chunk boundary) and of
the regression target with a learned scale or dispersion (lane and matrix kernel, two
chunks) against tests/golden/links_parent_bits.npz, recorded on an MI355X with the build
before the observation links moved into csrc/vb_links.hpp.  The fixed regression blocks are
pinned the same way by tests/test_gpu_aux.py (tests/golden/aux_parent_bits.npz)."""
import importlib.util
import os

import numpy as np
import pytest

from tests.conftest import ROOT, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]


def _fixture():
    spec = importlib.util.spec_from_file_location(
        'make_links_parent_bits', os.path.join(ROOT, 'tests', 'golden', 'make_links_parent_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, np.load(os.path.join(ROOT, 'tests', 'golden', 'links_parent_bits.npz'))


def test_multilevel_and_learned_blocks_give_the_bits_they_gave_before():
    mod, gold = _fixture()
    assert len(mod.mlm_cases()) == 20 and len(mod.aux_cases()) == 6
    # the lane kernel's case has a group that continues across observation 64
    off = np.cumsum(np.bincount(mod.mlm_data('gaussian', 3, 4, 70)[2], minlength=4))
    assert any(a < 64 < b for a, b in zip(np.concatenate([[0], off[:-1]]), off))
    got = mod.evaluate()
    assert sorted(got) == sorted(gold.files) and len(got) == 52
    for k in sorted(got):
        np.testing.assert_array_equal(got[k], gold[k], err_msg=k)
