"""The 50-digit reference of the full-rank family (tests/fullrank_mp.py) checked on
its own, and oracle/fullrank_oracle.py pinned against it.  CPU only.

  * the mp gradient against mp central differences of the mp value function (step
    1e-20 at 50 digits): every coordinate at D <= 4, 6 random directions at D = 8,
    to 1e-25 of the largest gradient entry; CHIVI on fixed draws, its max log
    weight held (the reference's gradient is that function's, vb.py:263);
  * log q of the draws through the z.z / s^2 invariant equals the eigenvector route;
  * the numpy oracle on the cases of tests/test_gpu_fullrank_edges.py: its error
    per case and block stays within twice the figure stored in
    tests/golden/fullrank_mp.npz under oracle_err/ (the GPU tests' eigensolver bars
    are 8 times those figures);
  * one fixture case recomputed live equals the stored pair exactly."""
import numpy as np
import pytest

from oracle import fullrank_oracle as fo
from tests import fullrank_mp as fm

pytestmark = pytest.mark.skipif(not fm.available(), reason='needs mpmath')

ERR_KEYS = ('value', 'gmu', 'gmu_max', 'gL', 'gL_max')


def _fd_check(D, kind, coords, N=5):
    from mpmath import mp, mpf
    lam = fm.lam_case(D, kind)
    s, z = fm.draws(D, N, fm.DF)
    h = mpf('1e-20')
    worst = 0.0
    with mp.workdps(fm.DIGITS):
        for obj in fm.OBJECTIVES:
            for t in fm.TARGETS:
                r = fm.evaluate(obj, lam, D, fm.DF, s, z, t)
                g = np.concatenate([r['gmu'], r['gL']])
                scale = max(abs(v) for v in g)
                for d in coords(len(lam)):
                    d = fm._obj(d)
                    f = [fm.evaluate(obj, fm._obj(lam) + sg * h * d, D, fm.DF, s, z, t, grad=False,
                                     top=r['top'])['surrogate'] for sg in (1, -1)]
                    fd = (f[0] - f[1]) / (2 * h)
                    ex = mp.fsum(a * b for a, b in zip(g, d))
                    worst = max(worst, float(abs(fd - ex) / scale))
    print('FD %d %s worst %.3g' % (D, kind, worst))
    assert worst <= 1e-25


@pytest.mark.parametrize('D,kind', [(1, 'generic'), (2, 'eye'), (3, 'cond1e4'), (4, 'two'),
                                    (4, 'generic')])
def test_gradient_equals_central_differences_every_coordinate(D, kind):
    _fd_check(D, kind, lambda P: np.eye(P))


def test_gradient_equals_central_differences_d8():
    rs = np.random.RandomState(8)
    _fd_check(8, 'generic', lambda P: rs.randn(6, P))


def test_logq_invariant_equals_the_eigenvector_route():
    from mpmath import mp
    D, N = 5, 7
    with mp.workdps(fm.DIGITS):
        lam = fm.lam_case(D, 'cond1e4')
        s, z = fm.draws(D, N, fm.DF)
        mu, L, Sig, _ = fm.unpack(lam, D)
        w, Q, S = fm.eig(Sig)
        x, _ = fm.transform(S, mu, s, z)
        a, _ = fm.logdensity(x, mu, w, Q, fm.DF)
        b = fm.logq_draws(w, s, z, fm.DF)
        c, _ = fm.logq_draws_lam(lam, D, s, z, fm.DF)       # .5 log det = sum of the log-diagonal
        assert max(abs(u - v) for u, v in zip(a, b)) < 1e-40
        assert max(abs(u - v) for u, v in zip(a, c)) < 1e-40


def _oracle_cases():
    """Every value-and-gradient case of the GPU tests: a file read on the mp side at
    the fixture dimensions, live (memoised, ~0.4 s per gradient at D ~ 32) below."""
    return fm.grad_cases()


@pytest.mark.parametrize('tname,D,kind,N', _oracle_cases())
def test_oracle_value_and_gradient(tname, D, kind, N):
    from tests.golden.make_fullrank_mp import oracle_grad
    for obj in fm.OBJECTIVES:
        ref = fm.grad_ref(tname, D, kind, N, obj)
        v, g = oracle_grad(tname, D, kind, N, obj)
        e = fm.block_errors(v, g, ref, D)
        stored = fm._fixture()['oracle_err/' + fm.grad_key(tname, D, kind, N, obj)]
        for q, st in zip(ERR_KEYS, stored):
            # twice the stored figure; 2^-50 of the block's scale for figures at 0
            scale = abs(ref['value'][0]) if q == 'value' else ref[q[:3].rstrip('_') + '_fro']
            assert e[q] <= 2 * st + 2.0 ** -50 * max(scale, 1.0), (obj, q, e[q], st)
        # and the oracle's documented accuracy: 1e-7 of each block's largest entry
        assert e['value'] <= 1e-9 * max(1.0, abs(ref['value'][0]))
        assert e['gmu_max'] <= 1e-7 * max(1.0, ref['gmu_max'])
        assert e['gL_max'] <= 1e-7 * max(1.0, ref['gL_max'])


@pytest.mark.parametrize('D', fm.LOGQ_DIMS)
def test_oracle_logdensity_at_the_pinv_cutoff(D):
    """The Sigma with eigenvalues 1e-8 and 1e-12 in decoupled directions: numpy's eigh
    returns both to relative precision, so the oracle agrees with mp to rounding in
    units of the condition sum, log(1e-12) in log_pdet included."""
    from tests.golden.make_fullrank_mp import oracle_logq_err
    for which in fm.logq_whiches(D):
        ref = fm.logq_ref(D, which)
        e = oracle_logq_err(D, which, ref)
        st = float(fm._fixture()['oracle_err/logq/%d/%s' % (D, which)])
        print('LOGQ %d %s oracle err %.3g S' % (D, which, e))
        assert e <= 2 * st + 2.0 ** -50
        assert e <= 1e-9
        if which == 'cutoff':
            assert ref['w_min'] < 2e-12 and ref['w_min'] > 0.5e-12


def test_oracle_entropy_and_moments():
    from tests.golden.make_fullrank_mp import oracle_root_err, ROOT_KINDS
    for D in fm.DIMS:
        for kind in (fm.KINDS if D <= fm.LIVE_MAX else ROOT_KINDS):
            if D == 1 and kind == 'two':
                continue
            ref = fm.root_ref(D, kind)
            e = oracle_root_err(D, kind, ref)
            st = fm._fixture()['oracle_err/' + fm.root_key(D, kind)]
            for q, a, b in zip(('entropy', 'm2', 'm4'), e, st):
                assert a <= 2 * b + 2.0 ** -50 * max(1.0, ref[q][2]), (D, kind, q, a, b)


def test_fixture_case_recomputed_live_equals_the_stored_pair():
    """D = 63, KLVI, corr_gauss, generic Sigma, N = 64: the generator's code and the
    committed fixture agree bit for bit (hi as double, lo as float)."""
    key = ('corr_gauss', 63, 'generic', 64, 'klvi')
    live = fm.compute_grad(*key)
    stored = fm._from_fixture(fm.grad_key(*key))
    for q in ('value', 'gmu_hi', 'gmu_lo', 'gL_hi', 'gL_lo', 'sens'):
        assert np.array_equal(live[q], stored[q]), q
    assert live['gL_lo'].dtype == stored['gL_lo'].dtype == np.float32


def test_fixture_inputs_are_the_seeded_cases():
    from tests.golden.make_fullrank_mp import digest
    fx = fm._fixture()
    for D in (63, 128):
        assert np.array_equal(fx['inputs/' + fm.root_key(D, 'generic')],
                              digest(fm.lam_case(D, 'generic')))
    s, z = fm.case_draws('corr_gauss', 64, 'generic', 512)
    assert np.array_equal(fx['inputs/draws/corr_gauss/64/generic/512'], digest(s, z))
