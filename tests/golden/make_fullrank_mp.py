"""Generator of tests/golden/fullrank_mp.npz: the 50-digit references of
tests/fullrank_mp.py at the dimensions too slow to compute inside a test
(D = 63, 64, 65, 96, 128; mp.eigsy takes 13 s at D = 65, over a minute at 128).

    python -m tests.golden.make_fullrank_mp [processes]

One work item per (D, Sigma kind): its root and every value-and-gradient case on
it, so the eigendecomposition is computed once.  The inputs are the seeded
cases of tests/fullrank_mp.py (lam_case, draws); the fixture stores a SHA-256
of each item's inputs under `inputs/...`, the references (hi, lo, condition
sums) and, for every case at every D, the numpy oracle's measured error against
the mp reference under `oracle_err/...` (absolute; the layout of
fullrank_mp.block_errors), which tests/test_oracle_fullrank_mp.py re-measures."""
import hashlib
import multiprocessing
import os
import sys

import numpy as np

from tests import fullrank_mp as fm

FIXTURE_DIMS = tuple(D for D in fm.DIMS if D > fm.LIVE_MAX)
ROOT_KINDS = ('eye', 'two', 'generic', 'cond1e4')


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def oracle_grad(t, D, kind, N, obj, special=None):
    """oracle/fullrank_oracle.py on the case's draws: (value, grad)."""
    from oracle import fullrank_oracle as fo
    fam, tgt = fo.FullRankT(D, fm.DF), fo.target_fn(t, D)
    lam, dr = fm.lam_case(D, kind), fm.case_draws(t, D, kind, N, special)
    if obj == 'klvi':
        return fo.klvi_value_grad(fam, tgt, lam, N, draws=dr)
    if obj == 'klvi_pd':
        return fo.klvi_pd_value_grad(fam, tgt, lam, N, draws=dr)
    return fo.chivi_value_grad(fam, tgt, lam, N, float(obj[5:]), draws=dr)


def oracle_root_err(D, kind, ref):
    """|oracle - mp| of entropy, 2nd and 4th moment."""
    from oracle import fullrank_oracle as fo
    fam, lam = fo.FullRankT(D, fm.DF), fm.lam_case(D, kind)
    got = (fam.entropy(lam), fam.pth_moment(2, lam), fam.pth_moment(4, lam))
    return np.array([abs((g - ref[q][0]) - ref[q][1]) for g, q in zip(got, ('entropy', 'm2', 'm4'))])


def oracle_logq_err(D, which, ref):
    """max over the points of |oracle - mp| / S."""
    from oracle import fullrank_oracle as fo
    lam, x = fm.logq_case(D, which)
    got = fo.FullRankT(D, fm.DF).logdensity(x, lam)
    return float(np.max(np.abs((got - ref['hi']) - ref['lo']) / ref['S']))


ERR_KEYS = ('value', 'gmu', 'gmu_max', 'gL', 'gL_max')


def item(args):
    D, kind = args
    out = {}
    stored = D > fm.LIVE_MAX
    root = fm.compute_root(D, kind)
    out['oracle_err/' + fm.root_key(D, kind)] = oracle_root_err(D, kind, root)
    if kind == 'generic' and D in fm.LOGQ_DIMS:
        for which in fm.logq_whiches(D):
            ref = fm.compute_logq(D, which)
            out['oracle_err/logq/%d/%s' % (D, which)] = oracle_logq_err(D, which, ref)
    if kind in fm.GRAD_KINDS:
        for (t, _, _, N) in sorted(set(c for c in fm.grad_cases() if c[1] == D and c[2] == kind)):
            for obj in fm.OBJECTIVES:
                ref = fm.compute_grad(t, D, kind, N, obj)
                v, g = oracle_grad(t, D, kind, N, obj)
                e = fm.block_errors(v, g, ref, D)
                out['oracle_err/' + fm.grad_key(t, D, kind, N, obj)] = np.array(
                    [e[q] for q in ERR_KEYS])
    if not stored:
        print('done', D, kind, flush=True)
        return out
    for k, v in root.items():
        out[fm.root_key(D, kind) + '/' + k] = v
    out['inputs/' + fm.root_key(D, kind)] = digest(fm.lam_case(D, kind))
    cases = [c for c in fm.grad_cases() + fm.HOOK_CASES if c[1] == D and c[2] == kind]
    for (t, _, _, N) in sorted(set(cases)):
        s, z = fm.case_draws(t, D, kind, N)
        out['inputs/draws/%s/%d/%s/%d' % (t, D, kind, N)] = digest(s, z)
        hook_only = (t, D, kind, N) not in fm.grad_cases()
        for obj in (('chivi2',) if hook_only else fm.OBJECTIVES):
            r = fm.compute_grad(t, D, kind, N, obj)
            if obj == 'klvi_pd':                   # KLVI's gradient: the value only
                r = {'value': r['value']}
            for k, v in r.items():
                out[fm.grad_key(t, D, kind, N, obj) + '/' + k] = v
    if kind == 'generic' and D in fm.LOGQ_DIMS:
        for which in fm.logq_whiches(D):
            lam, x = fm.logq_case(D, which)
            out['inputs/logq/%d/%s' % (D, which)] = digest(lam, x)
            for k, v in fm.compute_logq(D, which).items():
                out['logq/%d/%s/%s' % (D, which, k)] = v
    print('done', D, kind, flush=True)
    return out


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1)
    work = sorted(((D, k) for D in fm.DIMS for k in fm.KINDS
                   if (D <= fm.LIVE_MAX or k in ROOT_KINDS) and (D >= 2 or k != 'two')),
                  reverse=True)
    keep = {}
    with multiprocessing.Pool(procs) as pool:
        for out in pool.imap_unordered(item, work):
            keep.update(out)
    keep = {k: v for k, v in keep.items() if not k.endswith('_idx')}     # recomputed on load
    fm.pack_fixture(fm.FIXTURE, keep)
    print('%d arrays, %d bytes' % (len(keep), os.path.getsize(fm.FIXTURE)))


if __name__ == '__main__':
    main()
