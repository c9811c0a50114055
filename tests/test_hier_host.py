"""Hierarchical normal-means target (targets.hierarchical_normal), host side:
argument checks, the parameter block's layout, the ABI constant and the routes that
refuse or pass the new kind.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import hier_cases as hc
from tests.conftest import ROOT


def test_argument_errors():
    from viabel_amd import targets
    y, s = hc.make_data(5, 1)
    for bad_y, bad_s in ((y[:-1], s), (y, s[:-1]), (y.reshape(5, 1), s.reshape(5, 1)),
                         (np.zeros(0), np.zeros(0)), (3.0, 2.0)):
        with pytest.raises(ValueError, match='1-D|shape'):
            targets.hierarchical_normal(bad_y, bad_s)
    for v in (np.nan, np.inf, -np.inf):
        ybad, sbad = y.copy(), s.copy()
        ybad[2] = sbad[3] = v
        with pytest.raises(ValueError, match='finite'):
            targets.hierarchical_normal(ybad, s)
        with pytest.raises(ValueError, match='finite'):
            targets.hierarchical_normal(y, sbad)
    for v in (0.0, -1.0):
        sbad = s.copy()
        sbad[0] = v
        with pytest.raises(ValueError, match='sigma must be positive'):
            targets.hierarchical_normal(y, sbad)
    for v in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='mu_scale'):
            targets.hierarchical_normal(y, s, mu_scale=v)
        with pytest.raises(ValueError, match='tau_scale'):
            targets.hierarchical_normal(y, s, centered=True, tau_scale=v)


@pytest.mark.parametrize('centered', [False, True])
@pytest.mark.parametrize('J', [1, 7])
def test_parameter_layout(centered, J):
    from viabel_amd import targets, _native as nat
    y, s = hc.make_data(J, 2)
    t = targets.hierarchical_normal(y, s, centered=centered, mu_scale=2.5, tau_scale=0.75)
    assert t.kind == nat.TARGET_HIERARCHICAL == 7
    assert t.dim == J + 2 and t.name == 'hierarchical_normal' and not t.separable
    assert t.n_groups == J and t.centered is centered
    p = t.params
    assert p.dtype == np.float64 and p.flags['C_CONTIGUOUS']
    assert p.size == 8 + 2 * J
    assert p[0] == (1.0 if centered else 0.0)
    assert p[1] == J
    assert p[2] == 2.5
    assert p[3] == 0.75
    assert np.all(p[4:8] == 0.0)
    np.testing.assert_array_equal(p[8:8 + J], y)
    np.testing.assert_array_equal(p[8 + J:], s)
    # one array for the target's lifetime: the descriptor points into it every time
    s1, s2 = t._struct(), t._struct()
    assert t.params is p and s1.n_params == s2.n_params == p.size
    assert s1.dim == s2.dim == J + 2 and s1.kind == 7
    assert nat.as_f64(t.params) is t.params


def test_defaults_and_eight_schools_cp():
    from viabel_amd import targets
    y, s = hc.make_data(3, 4)
    t = targets.hierarchical_normal(y, s)
    assert t.centered is False and t.params[0] == 0.0
    assert t.params[2] == 5.0 and t.params[3] == 5.0
    cp = targets.eight_schools_cp()
    explicit = targets.hierarchical_normal(hc.ES_Y, hc.ES_SIGMA, centered=True)
    np.testing.assert_array_equal(cp.params, explicit.params)
    assert cp.dim == 10 and cp.centered is True and cp.n_groups == 8
    np.testing.assert_array_equal(cp.params[8:16], [28, 8, -3, 7, -1, 1, 18, 12])
    np.testing.assert_array_equal(cp.params[16:], [15, 10, 16, 11, 9, 11, 10, 18])
    # eight_schools_ncp stays the built-in kind
    assert targets.eight_schools_ncp().kind == 3 and targets.eight_schools_ncp().params is None


def test_exports():
    from viabel_amd import targets
    for name in ('hierarchical_normal', 'eight_schools_cp'):
        assert name in targets.__all__ and name in targets.__doc__
        assert callable(getattr(targets, name))


def test_header_declares_the_kind():
    from viabel_amd import _native as nat
    h = open(os.path.join(ROOT, 'include', 'viabel_amd.h')).read()
    m = re.search(r'VB_TARGET_HIERARCHICAL\s*=\s*(\d+)', h)
    assert m and int(m.group(1)) == 7 == nat.TARGET_HIERARCHICAL
    assert re.search(r'#define VB_ABI_VERSION 1\b', h)


def test_rows_kernel_not_used():
    from viabel_amd import targets, vb
    from viabel_amd.restarts import _rows_supported
    fam = vb.mean_field_t_variational_family(10, 40.0, rng='philox')
    assert _rows_supported(fam, targets.eight_schools_ncp())
    assert not _rows_supported(fam, targets.eight_schools_cp())
    assert not _rows_supported(fam, targets.hierarchical_normal(hc.ES_Y, hc.ES_SIGMA))


def test_as_target_passes_it_through():
    from viabel_amd import targets
    t = targets.eight_schools_cp()
    assert targets.as_target(t, 10) is t
