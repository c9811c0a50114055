"""Write tests/golden/sep_bits.npz: the column-pair kernel's results at the shapes of
tests/sep_bits_cases.py, from the library that is loaded (VIABEL_AMD_LIB selects a
build).  Recorded once from the build whose bits are the standard -- the one before
the kernel's instruction-count work -- and compared bit for bit by
tests/test_gpu_sep_bits.py ever after.  Results only.  Needs the GPU:

  VIABEL_AMD_LIB=$PWD/viabel_amd/libviabel_amd_base.so \
      python scripts/make_sep_bits_fixture.py [OUT.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out=os.path.join(ROOT, 'tests', 'golden', 'sep_bits.npz')):
    from tests import sep_bits_cases as sc
    from viabel_amd import _native as nat
    rec = {k: [] for k in ('lam', 'hist', 'vals', 'smooth', 'sha256')}
    for n, w in sc.CASES:
        for k, v in sc.record(n, w).items():
            rec[k].append(v)
    arrays = {k: np.stack(v) for k, v in rec.items()}
    arrays['cases'] = np.array(sc.CASES, dtype=np.int64)
    arrays['cols'] = sc.PCOLS.astype(np.int64)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print('wrote %s (%d bytes) from %s build %s' % (out, os.path.getsize(out), nat.LIB_PATH,
                                                    nat.lib().vb_build_id().decode()))


if __name__ == '__main__':
    main(*sys.argv[1:])
