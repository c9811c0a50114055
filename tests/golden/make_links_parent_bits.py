"""Records tests/golden/links_parent_bits.npz: Target.logdensity_and_grad of the multilevel
regression blocks (every likelihood, centred and non-centred) and of the regression blocks
with a learned scale or dispersion on the device, made with the build of the commit before
the observation links moved into csrc/vb_links.hpp.  tests/test_gpu_links.py asks the
current build for the same bits; tests/golden/aux_parent_bits.npz holds the fixed
regression blocks.

    python tests/golden/make_links_parent_bits.py OUT.npz

The data and rows are seeded (tests/mlm_cases.py, tests/count_cases.py,
tests/aux_cases.py), so the file holds the results only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import aux_cases as ac     # noqa: E402
from tests import count_cases as cc   # noqa: E402
from tests import mlm_cases as mc     # noqa: E402

# (p, G, M, n): lane kernel, two chunks, a group on both sides of observation 64; tile kernel
MLM_SHAPES = ((3, 4, 70, 65), (17, 3, 70, 10))
# (p, M, n): lane kernel; matrix kernel; two chunks each
AUX_SHAPES = ((3, 65, 64), (20, 65, 17))
SEED = 41


def mlm_data(lik, p, G, M):
    """(x, y, group, offset or None) of one multilevel case."""
    if lik in mc.LIKELIHOODS:
        return mc.make_data(p, G, M, lik, seed=SEED) + (None,)
    return cc.mlm_make_data(p, G, M, lik, seed=SEED)


def mlm_build(lik, centered, p, G, M):
    from viabel_amd import targets
    x, y, g, off = mlm_data(lik, p, G, M)
    if off is None:
        return targets.multilevel_regression(x, y, g, n_groups=G, **mc.model_kwargs(lik, centered))
    return targets.multilevel_regression(x, y, g, n_groups=G, offset=off,
                                         **cc.mlm_model_kwargs(lik, centered))


def mlm_rows(p, G, n):
    return mc.rows(n, p + 1 + G, p, 2000 + 7 * p + n)


def aux_build(lik, p, M):
    from viabel_amd import targets
    x, y, off = ac.make_data(p, M, lik, seed=SEED)
    return targets.regression(x, y, offset=off, **ac.target_kwargs(ac.model_kwargs(lik)))


def aux_rows(lik, p, n):
    return ac.start_rows(np.random.RandomState(3000 + 7 * p + n), n, p, lik)


def mlm_cases():
    return [(lik, centered, p, G, M, n) for lik in mc.LIKELIHOODS + cc.LIKELIHOODS
            for centered in mc.FORMS for p, G, M, n in MLM_SHAPES]


def aux_cases():
    return [(lik, p, M, n) for lik in ac.LIKELIHOODS for p, M, n in AUX_SHAPES]


def mlm_key(lik, centered, p, G, M, n):
    return 'mlm_%s_%s_%d_%d_%d_%d' % (lik, 'c' if centered else 'nc', p, G, M, n)


def aux_key(lik, p, M, n):
    return 'aux_%s_%d_%d_%d' % (lik, p, M, n)


def evaluate():
    """{key + '_lp' / '_g': array} of every case on the current build."""
    res = {}
    for lik, centered, p, G, M, n in mlm_cases():
        lp, g = mlm_build(lik, centered, p, G, M).logdensity_and_grad(mlm_rows(p, G, n))
        res[mlm_key(lik, centered, p, G, M, n) + '_lp'] = lp
        res[mlm_key(lik, centered, p, G, M, n) + '_g'] = g
    for lik, p, M, n in aux_cases():
        lp, g = aux_build(lik, p, M).logdensity_and_grad(aux_rows(lik, p, n))
        res[aux_key(lik, p, M, n) + '_lp'] = lp
        res[aux_key(lik, p, M, n) + '_g'] = g
    return res


def main(out):
    res = evaluate()
    np.savez_compressed(out, **res)
    print('wrote %s: %d arrays' % (out, len(res)))


if __name__ == '__main__':
    main(sys.argv[1])
