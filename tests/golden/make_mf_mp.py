"""Generator of tests/golden/mf_mp.npz: the 50-digit references (tests/mf_mp.py) of
the cases of tests/mf_cases.py whose reference takes more than a few seconds -- the
mixture at D >= 511 with N >= 127 -- with SHA-256 digests of each case's seeded
lam and eps.  Every entry of value, gradient and log weights is kept (no subset is
needed under 1 MiB).  Run from the repository root:

    python tests/golden/make_mf_mp.py
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from tests import mf_cases as mc      # noqa: E402
from tests import mf_mp as mm         # noqa: E402


def main():
    out = {}
    for c in mc.all_cases():
        if not c.get('golden'):
            continue
        ref = mm.estimate(c['objective'], c['kind'], c['df'], c['target'], c['lam'], c['eps'],
                          c['alpha'])
        k = c['id']
        out[k + '|value'] = np.array(ref.value)
        out[k + '|grad'] = np.array(ref.grad)
        out[k + '|lw'] = np.array(ref.lw)
        out[k + '|sha'] = np.frombuffer(mc.digest(c).encode(), dtype=np.uint8)
        print(k, flush=True)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mf_mp.npz'), **out)


if __name__ == '__main__':
    main()
