"""The full-rank Student-t kernels (vb_fr.hip, vb_gemm.hpp, vb_symsum.hpp) against
the 50-digit reference of tests/fullrank_mp.py, at the smallest shapes on each
side of every path switch: D in {1, 2, 31, 32, 33, 63, 64, 65, 96, 128} (GEMM tile
32; LDS-DMA loop at M, N % 32 == 0 and K % 64 == 0, else the register-staged loop
-- D = 96 takes whole tiles through it; symmetric-sum PCG at D % 64 == 0; D = 128
the first symmetric grid with more than one k stage), N on both sides of the
weights hook's N <= 512, N % 64 == 0, and Sigma with repeated eigenvalues
(lambda = 0 among them), where an eigh-based gradient is undefined.

Host noise only: the flat eps [s (n), z (n x D)] is built here and passed as
nat.Noise(nat.NOISE_HOST, ...), so the device and the reference see identical
doubles.  References at D <= 33 are computed live (memoised), larger D come from
tests/golden/fullrank_mp.npz.

Tolerances (fullrank_mp.root_bar, solve_bar, grad_bars; nothing is tuned on the
device's output): results with no iterative solver behind them carry an
operation-count bound in units of 2^-53 of their condition sum; results through
the device eigensolver 8 times the numpy oracle's own measured error on the same
case; results behind Newton-Schulz and PCG 4 times the first-order effect of the
solvers' own stopping thresholds (tau = 1e-10 sqrt(D), 1e-9 ||E||) plus the
block's rounding term.  The Newton-Schulz stall clause (1e-8 sqrt(D)) passes none
of these bars.

Every measured error is printed beside its bar (FR_EDGE lines) and, when
VIABEL_AMD_FR_EDGE_RECORD names a file, collected there as JSON, one line per case."""
import json
import os

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests import fullrank_mp as fm

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X'),
              pytest.mark.skipif(not fm.available(), reason='needs mpmath')]

U = fm.UNIT
RECORD = []


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    path = os.environ.get('VIABEL_AMD_FR_EDGE_RECORD')
    if path:
        # one line per case: {block: [error, bar, the oracle's error or null]}, 4 digits
        cases = {}
        for r in RECORD:
            cases.setdefault(r['case'], {})[r['block']] = [
                None if v is None else float('%.4g' % v) for v in (r['err'], r['bar'], r['oracle_err'])]
        with open(path, 'w') as f:
            note = ('errors and bars as printed; at D >= 63 the packed-L (gL) errors, and off the '
                    'generic kind at D >= 63 (every kind at D >= 96) the root\'s forward error, '
                    'run over the fixture\'s subset of entries while the max / Frobenius scales '
                    'are the whole block\'s')
            f.write('{\n"_note": %s,\n' % json.dumps(note) + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v))
                                        for k, v in cases.items()) + '\n}\n')


def _note(case, block, err, bar, oracle=None):
    RECORD.append({'case': case, 'block': block, 'err': float(err), 'bar': float(bar),
                   'oracle_err': None if oracle is None else float(oracle)})
    print('FR_EDGE %s %s err %.3g (bar %.3g%s)'
          % (case, block, err, bar, '' if oracle is None else ', oracle %.3g' % oracle))


def _mods():
    from viabel_amd import vb, targets, _native as nat
    return vb, targets, nat


def _sample(D, df, lam, s, z):
    """vb_family_sample on explicit draws: x = mu + (z S) / s as the device forms it."""
    vb, _, nat = _mods()
    fam = vb.t_variational_family(D, df, rng='numpy')
    n = len(s)
    lam = nat.as_f64(lam)
    eps = nat.as_f64(np.concatenate([s, np.asarray(z).ravel()]))
    out = np.empty((n, D))
    nz = nat.Noise(nat.NOISE_HOST, 0, 0, 0, nat.dptr(eps))
    nat.check(nat.lib().vb_family_sample(nat.context().handle, fam._struct(), nat.dptr(lam), n, nz,
                                         nat.dptr(out)))
    return out


def _value_grad(obj, tname, D, N, lam, s, z):
    """vb_objective_value_grad (one cold call) on explicit draws."""
    vb, targets, nat = _mods()
    fam = vb.t_variational_family(D, fm.DF, rng='numpy')
    tgt = targets.isogauss(D) if tname == 'isogauss' else targets.corr_gauss(D)
    if obj == 'klvi':
        o = vb.black_box_klvi(fam, tgt, N)
    elif obj == 'klvi_pd':
        o = vb.black_box_klvi_pd(fam, tgt, N)
    else:
        o = vb.black_box_chivi(float(obj[5:]), fam, tgt, N)
    lam = nat.as_f64(lam)
    eps = nat.as_f64(np.concatenate([s, np.asarray(z).ravel()]))
    nz = nat.Noise(nat.NOISE_HOST, 0, 0, 0, nat.dptr(eps))
    f, t, ob = o._structs()
    val, grad = np.empty(1), np.empty(lam.size)
    nat.check(nat.lib().vb_objective_value_grad(nat.context().handle, f, t, ob, nat.dptr(lam), nz,
                                                nat.dptr(val), nat.dptr(grad)))
    return val[0], grad


def _oracle_err(key):
    return fm._fixture().get('oracle_err/' + key)


# ---- a. Sigma = L L^T ---------------------------------------------------------------
@pytest.mark.parametrize('D', fm.DIMS)
def test_sigma_product_to_the_dot_product_bound(D):
    """mean_and_cov: the NT symmetric GEMM with its mirrored tiles.  Off-diagonals
    of L at scale 1, so the terms of an entry cancel.  Each entry is a length-D dot
    product (D roundings in any summation order) times df / (df - 2) (the quotient's
    and the product's rounding): |got - ref| <= (D + 2) 2^-53 S_ij, S_ij = c sum_k
    |L_ik L_jk|.  cov is symmetric bit for bit and the mean comes back exactly."""
    vb, _, _ = _mods()
    rs = np.random.RandomState(fm.SEED + D)
    tri = np.tril_indices(D)
    free = rs.randn(len(tri[0]))
    free[tri[0] == tri[1]] = rs.randn(D) * 0.2
    lam = np.concatenate([rs.randn(D), free])
    m, cov = vb.t_variational_family(D, fm.DF).mean_and_cov(lam)
    with fm.mp.workdps(fm.DIGITS):
        mu, ref, S = fm.mean_and_cov(lam, D, fm.DF)
        hi, lo = fm.pair(ref)
    assert np.array_equal(m, lam[:D])
    assert np.array_equal(cov, cov.T)
    err = float(np.max(np.abs((cov - hi) - lo) / (U * S)))
    _note('sigma/%d' % D, 'cov', err, D + 2)
    assert err <= D + 2


# ---- b. the root -------------------------------------------------------------------------
def _root_cases():
    out = [(D, k) for D in fm.DIMS for k in ('eye', 'two', 'generic', 'cond1e4')
           if not (D == 1 and k == 'two')]
    return out + [(D, 'cond1e8') for D in fm.DIMS if 2 <= D <= fm.LIVE_MAX]


@pytest.mark.parametrize('D,kind', _root_cases())
def test_root(D, kind):
    """sample(lam, D) with z = I, s = 1, mu = 0 returns S as the device holds it
    (products with 0 and 1 are exact).  In mp: ||S - S^T||_F / ||S||_2 and the forward
    error ||S - S_ref||_F / ||S_ref||_2 within fullrank_mp.root_bar; the residual
    ||S^2 - Sigma||_F / ||Sigma||_2 within twice it (d(S^2) = S dS + dS S).  At D >= 96,
    and at 63..65 off the generic kind, the forward error runs over the fixture's
    subset of entries (every diagonal entry, the last row, the first column and
    128 seeded others).  lambda = 0 must give S = I to the same bar.  Kind (v),
    cond(Sigma) ~1e8 at D <= 33, is kept: it passes on the tau-based bar (errors
    ~1e-15) since vb_family_sample reads the Newton-Schulz status and runs again with
    a larger count; before, the cold 12-iteration root came back unconverged
    (forward error 8.6e-5 at D = 2, 4.5e-4 at D = 31..33) without an error."""
    lam = fm.lam_case(D, kind).copy()
    lam[:D] = 0.0
    S = _sample(D, fm.DF, lam, np.ones(D), np.eye(D))
    assert np.all(np.isfinite(S))
    ref = fm.root_ref(D, kind)
    bar = fm.root_bar(D, ref['k'], ref['gamma'])
    with fm.mp.workdps(fm.DIGITS):
        Sd = fm._obj(S)
        _, _, Sig, _ = fm.unpack(lam, D)
        resid = float(fm._frob(fm.mm(Sd, Sd) - Sig)) / ref['w_max']
        sym = float(fm._frob(Sd - Sd.T)) / ref['S_norm2']
    d = (S.ravel()[ref['S_idx']] - ref['S_hi']) - ref['S_lo']
    fwd = float(np.linalg.norm(d)) / ref['S_norm2']
    case = 'root/%d/%s' % (D, kind)
    _note(case, 'symmetry', sym, bar)
    _note(case, 'residual', resid, 2 * bar)
    _note(case, 'forward', fwd, bar)
    assert sym <= bar and resid <= 2 * bar and fwd <= bar


# ---- c. sample: row divide and column bias ------------------------------------------------
@pytest.mark.parametrize('df', [2.1, 1e6])
@pytest.mark.parametrize('D', [1, 33, 64, 65])
@pytest.mark.parametrize('n', [1, 31, 33, 64, 65])
def test_sample_epilogue(n, D, df):
    """x = mu + (z S) / s at row counts on both sides of the tile, |mu| up to 1e6 in
    every third column, s heavy-tailed (df = 2.1) and ~1 (df = 1e6).  Per entry
    against the generic root's reference: the root's error moves entry (n, j) by at
    most ||z_n|| ||dS||_2 / s_n <= root_bar ||S||_2 ||z_n|| / s_n, and the sum, the
    scaling by sqrt(c), the divide and the bias round D + 3 times on the scale
    |mu_j| + sum_k |z_nk S_kj| / s_n."""
    lam = fm.lam_case(D, 'generic').copy()
    rs = np.random.RandomState(fm.SEED + 100 * D + n)
    lam[:D:3] = rs.uniform(-1e6, 1e6, size=len(lam[:D:3]))
    s = np.sqrt(rs.chisquare(df, n) / df)
    z = rs.randn(n, D)
    x = _sample(D, df, lam, s, z)
    ref = fm.root_ref(D, 'generic')
    assert ref['S_hi'].size == D * D
    with fm.mp.workdps(fm.DIGITS):
        Sr = fm._obj(ref['S_hi']).reshape(D, D) + fm._obj(ref['S_lo'].astype(float)).reshape(D, D)
        xr, scale = fm.transform(Sr, fm._obj(lam[:D]), s, z)
        hi, lo = fm.pair(xr)
    bar = (fm.root_bar(D, ref['k'], ref['gamma']) * ref['S_norm2']
           * (np.linalg.norm(z, axis=1) / s)[:, None] + (D + 3) * U * scale)
    worst = float(np.max(np.abs((x - hi) - lo) / bar))
    _note('sample/%d/%d/%g' % (n, D, df), 'x (fraction of bar)', worst, 1.0)
    assert worst <= 1.0


# ---- d / e. value and gradient ---------------------------------------------------------------
def _check_grad(tname, D, kind, N, obj, special=None):
    ref = fm.grad_ref(tname, D, kind, N, obj, special)
    s, z = fm.case_draws(tname, D, kind, N, special)
    v, g = _value_grad(obj, tname, D, N, fm.lam_case(D, kind), s, z)
    assert np.isfinite(v) and np.all(np.isfinite(g))
    err = fm.block_errors(v, g, ref, D)
    bars = fm.grad_bars(ref, D, N, obj)
    key = fm.grad_key(tname, D, kind, N, obj, special)
    oe = _oracle_err(key)
    oe = dict(zip(('value', 'gmu', 'gmu_max', 'gL', 'gL_max'), oe)) if oe is not None else {}
    _note(key, 'value', err['value'], bars['value'], oe.get('value'))
    for blk in ('gmu', 'gL'):
        # max norm against the block's largest entry, 2-norm against its Frobenius norm
        # (at D >= 63 the packed-L errors run over the fixture's subset of entries,
        # the scales over the whole block)
        _note(key, blk + ' max/max', err[blk + '_max'] / ref[blk + '_max'],
              bars[blk][0] / ref[blk + '_max'],
              oe[blk + '_max'] / ref[blk + '_max'] if oe else None)
        _note(key, blk + ' fro/fro', err[blk] / ref[blk + '_fro'], bars[blk][1] / ref[blk + '_fro'],
              oe[blk] / ref[blk + '_fro'] if oe else None)
    assert err['value'] <= bars['value']
    for blk in ('gmu', 'gL'):
        assert err[blk + '_max'] <= bars[blk][0] and err[blk] <= bars[blk][1]


@pytest.mark.parametrize('obj', fm.OBJECTIVES)
@pytest.mark.parametrize('tname,D,kind,N', fm.grad_cases())
def test_value_and_gradient(tname, D, kind, N, obj):
    """One cold vb_objective_value_grad call (fr_value_grad without an update): the
    value, the mean block and the packed-L block each against its own scale, within
    fullrank_mp.grad_bars.  Launches reached: D = 32, 64, 96, 128 take whole tiles.
    The D x D products (K = D) have LDS-DMA shapes at D = 64 and 128 only: there
    iteration 0 of the root carries the schedule hook (SchedHook); at D = 32 and 96
    (K % 64 != 0) the products run the register-staged loop and fr_sched_kernel
    runs on its own, as at every ragged D.  The G_S product has M = N = D and K = N
    draws, so WeightsHook is taken at every D % 32 == 0 once N % 64 == 0 -- D = 32,
    64, 96, 128 at N = 64, D = 64 at N = 128 -- and fr_weights_kernel with a plain
    product everywhere else, the D = 96, N = 65 case among them (whole tiles, no
    hook at all).  D % 64 == 0 takes the symmetric-sum PCG, else the GEMM PCG.  At
    D >= 63 the packed-L block is checked on the fixture's subset (every diagonal
    entry, the last row, the first column, 64 seeded others, 256 from D = 96)."""
    _check_grad(tname, D, kind, N, obj)


@pytest.mark.parametrize('special', ['equal', 'dominant'])
def test_chivi_weight_edges(special):
    """CHIVI alpha = 2 at D = 33, lambda = 0, isogauss: every log weight equal to
    rounding (all rows the same draw), and one log weight ahead of every other by
    more than 800 nats (every other weight underflows to 0)."""
    _check_grad('isogauss', 33, 'eye', 64, 'chivi2', special)


@pytest.mark.parametrize('tname,D,kind,N', fm.HOOK_CASES)
def test_weights_hook_boundary(tname, D, kind, N):
    """CHIVI alpha = 2 at D = 64: the single call reaches WeightsHook when N <= 512
    and the G_S product (M = N = 64, K = N) has LDS-DMA shapes, K % 64 == 0 -- taken
    at N = 64 and 512, fr_weights_kernel and a plain product at N = 65 and 576."""
    _check_grad(tname, D, kind, N, 'chivi2')


# ---- f. log q of arbitrary points ----------------------------------------------------------------
@pytest.mark.parametrize('D,which', [(D, w) for D in fm.LOGQ_DIMS for w in fm.logq_whiches(D)])
def test_logdensity_far_points_and_pinv_cutoff(D, which):
    """logdensity (dsyevd route) at points up to 1e3 scale units out, and at a Sigma
    with eigenvalues 1e-8 and 1e-12 on the two sides of the 1e-10 pinv cutoff.  Bar:
    8 times the numpy oracle's measured error on the case, never below D 2^-53
    ||Sigma||_2, in units of the result's condition sum."""
    vb, _, _ = _mods()
    lam, x = fm.logq_case(D, which)
    got = vb.t_variational_family(D, fm.DF).logdensity(x, lam)
    ref = fm.logq_ref(D, which)
    err = float(np.max(np.abs((got - ref['hi']) - ref['lo']) / ref['S']))
    oe = float(_oracle_err('logq/%d/%s' % (D, which)))
    bar = max(8 * oe, D * U * ref['w_max'])
    _note('logq/%d/%s' % (D, which), 'log q / S', err, bar, oe)
    assert np.all(np.isfinite(got)) and err <= bar


@pytest.mark.parametrize('tname', fm.TARGETS)
@pytest.mark.parametrize('D', fm.LOGQ_DIMS)
def test_log_weights_invariant(D, tname):
    """vb_log_weights on host draws (df = 7, 2.1-heavy s mixed in): lw = log p(x) -
    log q, log q through the invariant maha = z.z / s^2 and .5 log det Sigma = sum log
    L_ii.  The reference evaluates log p in mp at the x the device returned (x itself is
    test_sample_epilogue's), so only the algebra is measured, with no solver behind it:
    each of log p (D terms), z.z (D terms), the log-diagonal sum (D terms) and the
    dozen scalar operations rounds once per term on its share of the condition sum
    S = S_logp + S_logq, hence |got - ref| <= (D + 16) 2^-53 S; corr_gauss forms
    G = -x P first (D more roundings per entry, S_logp = .5 |x| |P| |x|^T + |const|):
    (2 D + 16) 2^-53 S."""
    vb, targets, nat = _mods()
    from tests import targets_mp as tm
    n = 48
    lam = fm.lam_case(D, 'generic')
    rs = np.random.RandomState(fm.SEED + 5 * D)
    s = np.sqrt(np.concatenate([rs.chisquare(fm.DF, n // 2) / fm.DF, rs.chisquare(2.1, n // 2) / 2.1]))
    z = rs.randn(n, D)
    fam = vb.t_variational_family(D, fm.DF, rng='numpy')
    tgt = (targets.isogauss(D) if tname == 'isogauss' else targets.corr_gauss(D)).bind(D)
    lamd = nat.as_f64(lam)
    eps = nat.as_f64(np.concatenate([s, z.ravel()]))
    nz = nat.Noise(nat.NOISE_HOST, 0, 0, 0, nat.dptr(eps))
    lw, xs = np.empty(n), np.empty((n, D))
    nat.check(nat.lib().vb_log_weights(nat.context().handle, fam._struct(), tgt._struct(),
                                       nat.dptr(lamd), n, nz, nat.dptr(lw), nat.dptr(xs)))
    assert np.all(np.isfinite(lw)) and np.all(np.isfinite(xs))
    with fm.mp.workdps(fm.DIGITS):
        xo = fm._obj(xs)
        lp, g = fm.target(tname, xo)
        if tname == 'isogauss':
            Sp = tm.reference('isogauss', xs).lp_S
        else:      # .5 |x| |P| |x|^T + |const|: the products inside G = -x P cancel too
            prec, const = fm.corr_gauss_params(D)
            ax = np.abs(xs)
            Sp = 0.5 * np.sum((ax @ np.abs(prec)) * ax, axis=1) + abs(const)
        lq, Sq = fm.logq_draws_lam(lam, D, s, z, fm.DF)
        hi, lo = fm.pair(lp - lq)
    err = float(np.max(np.abs((lw - hi) - lo) / (U * (Sp + Sq))))
    bar = D + 16 if tname == 'isogauss' else 2 * D + 16
    _note('log_weights/%s/%d' % (tname, D), 'lw', err, bar)
    assert err <= bar


# ---- g. entropy and moments ------------------------------------------------------------------------
@pytest.mark.parametrize('D,kind', [c for c in _root_cases() if c[1] != 'cond1e8'])
def test_entropy_and_moments(D, kind):
    """entropy, pth_moment(2), pth_moment(4) from the device eigenvalues: 8 times the
    numpy oracle's measured error, never below D 2^-53 ||Sigma||_2 of the condition
    sum."""
    vb, _, _ = _mods()
    fam = vb.t_variational_family(D, fm.DF)
    lam = fm.lam_case(D, kind)
    ref = fm.root_ref(D, kind)
    oe = _oracle_err(fm.root_key(D, kind))
    got = (fam.entropy(lam), fam.pth_moment(2, lam), fam.pth_moment(4, lam))
    for g, q, o in zip(got, ('entropy', 'm2', 'm4'), oe):
        hi, lo, S = ref[q]
        err = abs((g - hi) - lo)
        bar = max(8 * o, D * U * ref['w_max'] * S)
        _note('moments/%d/%s' % (D, kind), q, err, bar, o)
        assert np.isfinite(g) and err <= bar
