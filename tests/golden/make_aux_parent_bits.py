"""Records tests/golden/aux_parent_bits.npz: Target.logdensity_and_grad of fixed-parameter
regression blocks (learn = 0, every likelihood) on the device, made with the build of the
commit before the learned-scale mode was added.  tests/test_gpu_aux.py asks the current
build for the same bits.

    python tests/golden/make_aux_parent_bits.py OUT.npz

The data and rows are seeded (tests/glm_cases.py, tests/count_cases.py), so the file
holds the results only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import count_cases as cc   # noqa: E402
from tests import glm_cases as gc     # noqa: E402

# lane-per-row kernel (one and three chunks), matrix kernel with one slice, two slabs and
# six chunks
SHAPES = ((3, 65, 64), (16, 130, 70), (20, 65, 17), (130, 321, 10))


def build(lik, D, M):
    """The fixed-parameter target of one (likelihood, D, M)."""
    from viabel_amd import targets
    if lik in gc.LIKELIHOODS:
        x, y = gc.make_data(D, M, lik, seed=31)
        return targets.regression(x, y, **gc.model_kwargs(lik))
    x, y, off = cc.make_data(D, M, lik, seed=31)
    return targets.regression(x, y, offset=off, **cc.model_kwargs(lik))


def rows(D, n):
    return np.random.RandomState(1000 + 7 * D + n).randn(n, D) * 0.4


def cases():
    return [(lik, D, M, n) for lik in gc.LIKELIHOODS + cc.LIKELIHOODS for D, M, n in SHAPES]


def key(lik, D, M, n):
    return '%s_%d_%d_%d' % (lik, D, M, n)


def main(out):
    res = {}
    for lik, D, M, n in cases():
        lp, g = build(lik, D, M).logdensity_and_grad(rows(D, n))
        res[key(lik, D, M, n) + '_lp'] = lp
        res[key(lik, D, M, n) + '_g'] = g
    np.savez_compressed(out, **res)
    print('wrote %s: %d arrays' % (out, len(res)))


if __name__ == '__main__':
    main(sys.argv[1])
