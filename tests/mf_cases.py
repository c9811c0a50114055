"""The case list of the mean-field multiprecision tests (tests/test_oracle_mf_mp.py
on the numpy oracle, tests/test_gpu_mf_edges.py on the device), each case with the
reason it is there.  The shapes are the smallest on each side of each switch of
vb_mf.hip and the mf_wide path; every case's draws are host noise seeded from its
id, so the oracle, the device and the 50-digit reference see the same doubles.

A case is a dict: id, path, target, D, N, objective, kind, df, alpha, lam, eps, why.
"""
import hashlib
import zlib

import numpy as np

FAMS = [('gauss', None), ('t', 8.0)]
OBJECTIVES = ['klvi', 'klvi_pd', 'chivi']
LS_EDGES = (-30.0, -3.0, 0.0, 5.0, 30.0)
DF_EDGES = (2.000001, 2.5, 40.0, 1e6)
ALPHA_EDGES = (1.0001, 1.5, 2.0, 8.0)


def _seed(cid):
    return zlib.crc32(cid.encode()) & 0x7FFFFFFF


def _mean(target, D, rs):
    mean = 0.3 * rs.randn(D)
    if target == 'mixture':
        mean += np.where(np.arange(D) % 3 == 0, 2.0, -1.0)   # both modes and the saddle between
    return mean


def _draws(kind, df, N, D, rs):
    return rs.randn(N, D) if kind == 'gauss' else rs.standard_t(df, size=(N, D))


def make(path, target, D, N, objective, kind, df, why, alpha=2.0, ls=-0.7, tag=''):
    """ls: one value for every coordinate, or 'mixed' (LS_EDGES cycled over the
    coordinates)."""
    cid = '%s/%s/D%d/N%d/%s/%s%s/a%g/ls%s%s' % (path, target, D, N, objective, kind,
                                                 '' if df is None else '%g' % df, alpha, ls, tag)
    rs = np.random.RandomState(_seed(cid))
    lsv = (np.array([LS_EDGES[d % len(LS_EDGES)] for d in range(D)]) if ls == 'mixed'
           else np.full(D, float(ls)) + (0.1 * rs.randn(D) if abs(ls) < 3 else 0.0))
    lam = np.concatenate([_mean(target, D, rs), lsv])
    return dict(id=cid, path=path, target=target, D=D, N=N, objective=objective, kind=kind, df=df,
                alpha=alpha, lam=lam, eps=_draws(kind, df, N, D, rs), why=why)


def digest(c):
    """SHA-256 of a case's seeded inputs (kept beside its precomputed reference)."""
    return hashlib.sha256(np.ascontiguousarray(c['lam']).tobytes()
                          + np.ascontiguousarray(c['eps']).tobytes()).hexdigest()


def _golden(c):
    """Mark a case whose reference comes from tests/golden/mf_mp.npz."""
    c['golden'] = True
    return c


def _rot(k, seq):
    return seq[k % len(seq)]


def block_cases():
    """block_kernel: D <= kBlockDMax = 16, split rows up to kBlockSplitMaxD = 10; N:
    one draw, two, a partly filled wave (63), a full one, one draw past it, several
    per thread (100, 128, 129) and the chunked layout (300).  Every (D, N) once, the
    target / objective / family rotating so that each appears at each D and each N."""
    out, k = [], 0
    for D in (1, 2, 9, 10, 11, 15, 16):
        for N in (1, 2, 63, 64, 65, 100, 128, 129, 300):
            targets = ['mixture'] + (['funnel'] if D >= 2 else []) + (
                ['eight_schools_ncp'] if D == 10 else [])
            kind, df = _rot(k // 3, FAMS)
            out.append(make('block', _rot(k, targets), D, N, _rot(k + k // 7, OBJECTIVES), kind, df,
                            'block kernel: D on a side of the split (10) / DMax (16) limits, N '
                            'on a side of the wave and per-thread sample counts'))
            k += 1
    return out


def pair_cases():
    """sep_kernel (separable target, not CHIVI): odd D leaves half a column pair,
    kRowChunkPairs = 256 pairs per chunk (D = 511 ... 514 around it); N around the
    128 rows of a pass with the kRowsPerBlock = 4 remainder.  D >= 511 at N >= 127
    costs a multiprecision reference of ~10 s: those references are precomputed
    (tests/golden/make_mf_mp.py -> mf_mp.npz, every entry kept: 0 % unchecked for
    value, gradient and log weights; log q at the device's own x is checked live on
    the first 4 rows, 97 % of the rows unchecked)."""
    out, k = [], 0
    for D in (17, 18, 19, 64):
        for N in (1, 127, 128, 129):
            kind, df = _rot(k, FAMS)
            out.append(make('pair', 'mixture', D, N, _rot(k // 2, ['klvi', 'klvi_pd']), kind, df,
                            'column-pair kernel: odd D tail, N around 128 with the 4-row remainder'))
            k += 1
    for D in (511, 512, 513, 514):
        for N in (1, 5, 127, 128, 129):
            kind, df = _rot(k, FAMS)
            c = make('pair', 'mixture', D, N, _rot(k // 2, ['klvi', 'klvi_pd']), kind, df,
                     'column-pair kernel: both sides of the 256-pair chunk')
            out.append(_golden(c) if N >= 127 else c)
            k += 1
    return out


def wide_cases():
    """The materialised path: the funnel past D = 16 and the mixture under CHIVI
    (kWideRowD = 512 switches the row kernels)."""
    out, k = [], 0
    for D in (17, 40):
        for N in (1, 128, 129):
            kind, df = _rot(k, FAMS)
            out.append(make('wide', 'funnel', D, N, _rot(k, OBJECTIVES), kind, df,
                            'materialised path: funnel past the block kernel'))
            k += 1
    for D, Ns in ((17, (1, 128, 129)), (511, (1, 5, 128, 129)), (512, (1, 5, 128, 129)),
                  (513, (1, 5, 128, 129))):
        for N in Ns:
            kind, df = _rot(k, FAMS)
            c = make('wide', 'mixture', D, N, 'chivi', kind, df,
                     'materialised path: separable target under CHIVI, both sides of '
                     'kWideRowD = 512', alpha=_rot(k, (2.0, 1.5)))
            out.append(_golden(c) if D >= 511 and N >= 128 else c)
            k += 1
    return out


# one shape per path for the parameter edges (the mixture: finite at every sigma)
EDGE_SHAPES = [('block', 10, 129), ('pair', 19, 5), ('wide', 17, 5)]


def edge_cases():
    out = []
    for path, D, N in EDGE_SHAPES:
        objs = ['chivi'] if path == 'wide' else (['klvi', 'klvi_pd'] if path == 'pair' else OBJECTIVES)
        for ls in LS_EDGES + ('mixed',):
            for k, obj in enumerate(objs):
                kind, df = _rot(k + int(ls == 'mixed'), FAMS)
                out.append(make(path, 'mixture', D, N, obj, kind, df,
                                'log sigma edge %s (uniform, or mixed per coordinate)' % ls,
                                ls=ls, tag='/edge'))
        for df in DF_EDGES:
            for obj in objs:
                out.append(make(path, 'mixture', D, N, obj, 't', df,
                                'df edge %g (just above 2; the Gaussian limit)' % df, tag='/edge'))
        if 'chivi' in objs:
            for alpha in ALPHA_EDGES:
                for ls in (-0.7, 1.2):
                    out.append(make(path, 'mixture', D, N, 'chivi', 'gauss', None,
                                    'alpha edge %g; at ls 1.2 the log weights spread wide' % alpha,
                                    alpha=alpha, ls=ls, tag='/edge'))
    return out


def spread_cases():
    """CHIVI log weights planted around exp_fast's -746 clamp: isogauss, mu = 0,
    sigma^2 = 3, so lw = -sum eps^2 + const exactly; row 0 is eps = 0 (the maximum)
    and planted rows sit alpha (M - lw) = s below it, s on both sides of 745.13 (the
    smallest subnormal) -- first and last of a wave, first of the next, the last
    row.  'under': every planted weight > 0 in double; 'over': some exactly 0."""
    out = []
    for alpha in (1.5, 2.0, 8.0):
        for name, spans in (('under', (600.0, 700.0, 740.0, 744.0)),
                            ('over', (700.0, 744.0, 745.5, 747.0, 900.0, 5000.0))):
            for D, N, path in ((2, 129, 'block'), (2, 300, 'block'), (17, 129, 'wide')):
                c = make(path, 'isogauss', D, N, 'chivi', 'gauss', None,
                         'planted log-weight spread %s the clamp at 746 / alpha' % name,
                         alpha=alpha, ls=0.0, tag='/spread-' + name)
                c['lam'] = np.concatenate([np.zeros(D), np.full(D, 0.5 * np.log(3.0))])
                eps = 0.05 * c['eps']
                eps[0] = 0.0
                for j, row in enumerate((1, 63, 64, 65, N - 1, N // 2)[:len(spans)]):
                    eps[row] = 0.0
                    eps[row, j % D] = np.sqrt(spans[j] / alpha)
                c['eps'] = eps
                c['spans'] = spans
                out.append(c)
    return out


def neginf_cases():
    """A CHIVI thread whose first draw has log weight -inf in double while others are
    finite.  The isogauss target forms -0.5 * x * x as (-0.5 x) x, which overflows
    from |x| = sqrt(2 DBL_MAX) = 1.8961e154 on (x * x alone already from 1.34e154,
    which is not enough).  mu_0 = 1.896e154 and sigma_0 = e^350 = 1.0e152: eps_0 = +2
    gives x_0 = 1.916e154, log p = -inf; eps_0 = -2 gives 1.876e154, log p =
    -1.76e308, finite; g sigma eps ~ 3.8e306 stays finite in both.  Every third draw
    and draws 0 and 64 overflow ('over'), so whatever the layout some thread starts
    on one.  The true log weights are ~ -1.8e308: below the double range on the
    planted rows (-inf is their correct rounding), finite on the others."""
    out = []
    for D, N, path in ((2, 129, 'block'), (2, 300, 'block'), (17, 129, 'wide')):
        c = make(path, 'isogauss', D, N, 'chivi', 'gauss', None,
                 'first sample of a thread with lw = -inf, others finite', tag='/neginf')
        lam = np.zeros(2 * D)
        lam[0], lam[D] = 1.896e154, 350.0
        eps = 0.3 * c['eps']
        over = (np.arange(N) % 3 == 0) | (np.arange(N) == 64)
        eps[:, 0] = np.where(over, 2.0, -2.0) + 0.01 * eps[:, 0]
        c['lam'], c['eps'], c['over'] = lam, eps, over
        out.append(c)
    return out


def all_cases():
    return (block_cases() + pair_cases() + wide_cases() + edge_cases() + spread_cases()
            + neginf_cases())


# ---- family functions ---------------------------------------------------------
def family_cases():
    """logdensity (family_logdensity_kernel below 512 columns, the row-block form
    from 512 on), sample, moments: (kind, df, D, n, lam, x)."""
    out = []
    for D in (1, 10, 65, 511, 512, 513):
        for kind, df in FAMS + [('t', 2.000001), ('t', 4.000001), ('t', 1e6)]:
            rs = np.random.RandomState(_seed('fam/%d/%s%s' % (D, kind, df)))
            lsv = np.array([LS_EDGES[d % 5] for d in range(D)]) if D > 1 else np.array([-3.0])
            lam = np.concatenate([rs.randn(D), lsv])
            n = 6 if D < 511 else 2
            eps = _draws(kind, df, n, D, rs)
            out.append(dict(id='fam/%s%s/D%d' % (kind, '' if df is None else '%g' % df, D),
                            kind=kind, df=df, D=D, lam=lam, eps=eps))
    return out


# |z| of the t family's log q: both sides of where z * z overflows (1.34e154)
Z_EDGES = (1e100, 1e150, 1e153, 1.3e154, 1.4e154, 1e160, 1e200, 1e300)

# ---- update forms --------------------------------------------------------------
# (W, steps, eps, lr_end): 2 W + 1 steps wrap the ring twice; W on both sides of
# kBlockQpreMaxW = 16; W = 50 never fills (W larger than the step count)
UPDATE_CASES = ([(W, 2 * W + 1, eps, None) for W in (1, 2, 10, 16, 17, 64) for eps in (0.1, 1e-300)]
                + [(50, 12, 0.1, None), (10, 21, 0.1, 0.002), (17, 35, 1e-300, 0.002)])
