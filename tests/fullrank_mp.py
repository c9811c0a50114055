"""Multiprecision restatement of the full-rank Student-t family and its KLVI /
KLVI-PD / CHIVI value and gradient (mpmath, 50 digits), the edge cases built on
it, and the error model of their GPU tests; shared by the CPU test that pins
oracle/fullrank_oracle.py (tests/test_oracle_fullrank_mp.py), the fixture
generator (tests/golden/make_fullrank_mp.py) and the GPU tests
(tests/test_gpu_fullrank_edges.py).

Written from the definitions in the docstrings of oracle/fullrank_oracle.py and
viabel_amd/csrc/vb_fr.hip:

  lambda = [mu (D), tril(M) row-major], L = M with exp on the diagonal,
  Sigma = L L^T, S = sqrtm(Sigma) = Q diag(sqrt w) Q^T (mp.eigsy),
  x = mu + (z S) / s,  entropy = .5 log det Sigma,
  cov = df / (df - 2) Sigma,  log q = multivariate_t_logpdf (absolute pinv
  cutoff 1e-10 on the eigenvalues).

  KLVI      value -(entropy + mean log p)            r_n = -1/N,  c = -1/2
  KLVI-PD   value -(mean log p - mean log q(x))      gradient as KLVI
  CHIVI     lw = log p - log q, w = exp(alpha (lw - max lw)),
            value log(mean w) / alpha + max lw       r_n = alpha w_n / N,
                                                     c = 1/2 sum r
  gradient  g_mu = sum_n r_n g_n (g = d log p / dx);  G_S = Z^T diag(r / s) G,
            E = G_S + G_S^T;  S X + X S = E solved in the eigenbasis,
            X~_ij = E~_ij / (sqrt w_i + sqrt w_j) (defined at repeated
            eigenvalues);  H = X + 2 c Sigma^-1;  G_L = H L;  packed lower
            triangle with the diagonal times L_ii.

The CHIVI gradient is the reference's (vb.py:263): the derivative of
mean(exp(alpha (lw - top))) with top held at max lw, NOT of the reported value;
`surrogate` returns that function for the finite-difference check.

Matrix products run on fixed-point integers (entries scaled by 2^FIX_BITS in
numpy object arrays): exact products and sums, one truncation of 2^-FIX_BITS
absolute per input entry -- below 1e-75 against entries between 1e-12 and 1e12
here -- and ~100 times faster than mpmath's matrix product.

References come back as double pairs (hi, lo), ref = hi + lo to ~2^-106, with a
condition sum S (sum of the absolute values of the added terms) where a
rounding-level comparison |got - ref| / (2^-53 S) applies.
"""
import functools
import math
import os

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mpmath = None

from tests import targets_mp as tm

DIGITS = 50
FIX_BITS = 320
UNIT = 2.0 ** -53
SEED = 20240611
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fullrank_mp.npz')

DIMS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 128)
LIVE_MAX = 33            # larger D come from the fixture (mp.eigsy: 13 s at 65, 28 s at 96)
KINDS = ('eye', 'two', 'generic', 'cond1e4', 'cond1e8')
OBJECTIVES = ('klvi', 'klvi_pd', 'chivi2', 'chivi1.5')
TARGETS = ('isogauss', 'corr_gauss')
DF = 7.0

# the device's stopping constants (vb_fr.hip fr_sqrt, fr_pcg)
NS_TAU = 1e-10           # ||I - Z Y||_F <= NS_TAU sqrt(D)   (conv_tol2 = 1e-20 D)
PCG_TOL = 1e-9           # ||R|| <= PCG_TOL ||E||, cold calls (pcg_tol2 = 1e-18)


def available():
    return mpmath is not None


# ---- arithmetic helpers -------------------------------------------------------
def _obj(a):
    """Doubles (or mpf) -> object array of mpf."""
    a = np.asarray(a, dtype=object)
    out = np.empty(a.shape, dtype=object)
    for i, v in np.ndenumerate(a):
        out[i] = v if isinstance(v, mpf) else mpf(float(v))
    return out


def _fix(A):
    out = np.empty(A.shape, dtype=object)
    for i, v in np.ndenumerate(A):
        out[i] = int(mp.ldexp(v, FIX_BITS))
    return out


def mm(A, B):
    """A @ B of object arrays of mpf, on fixed-point integers."""
    C = _fix(A).dot(_fix(B))
    out = np.empty(C.shape, dtype=object)
    for i, v in np.ndenumerate(C):
        out[i] = mp.ldexp(mpf(v), -2 * FIX_BITS)
    return out


def pair(v):
    """mpf or object array -> (hi, lo) doubles."""
    if isinstance(v, np.ndarray):
        hi = np.empty(v.shape)
        lo = np.empty(v.shape)
        for i, e in np.ndenumerate(v):
            hi[i] = float(e)
            lo[i] = float(e - mpf(hi[i]))
        return hi, lo
    hi = float(v)
    return hi, float(v - mpf(hi))


def _f(A):
    return np.array(A, dtype=float)


def _frob(A):
    return mp.sqrt(mp.fsum(v * v for v in A.ravel()))


# ---- the family -----------------------------------------------------------------
def unpack(lam, D):
    """mu (D), L, Sigma = L L^T (object arrays of mpf) and the condition sums
    Sabs_ij = sum_k |L_ik L_jk| (doubles).  lam: doubles or mpf."""
    lam = _obj(lam)
    mu = lam[:D].copy()
    L = np.full((D, D), mpf(0), dtype=object)
    t = D
    for i in range(D):
        for j in range(i + 1):
            L[i, j] = mp.exp(lam[t]) if i == j else lam[t]
            t += 1
    Sig = mm(L, L.T)
    aL = np.abs(L)
    return mu, L, Sig, _f(mm(aL, aL.T))


def eig(Sig):
    """w ascending (object array), Q (columns = eigenvectors), S = Q diag(sqrt w) Q^T."""
    D = Sig.shape[0]
    E, Q = mp.eigsy(mp.matrix(Sig.tolist()))
    w = np.array([E[i] for i in range(D)], dtype=object)
    Qa = np.array(Q.tolist(), dtype=object).reshape(D, D)
    rw = np.array([mp.sqrt(v) for v in w], dtype=object)
    return w, Qa, mm(Qa * rw[None, :], Qa.T)


def transform(S, mu, s, z):
    """x = mu + (z S) / s (n x D, mpf) and its per-entry scale
    |mu_j| + sum_k |z_nk S_kj| / s_n (doubles)."""
    z, s = _obj(z), _obj(s)
    x = mm(z, S) / s[:, None] + mu[None, :]
    scale = mm(np.abs(z), np.abs(S)) / s[:, None] + np.abs(mu)[None, :]
    return x, _f(scale)


def entropy(w):
    """.5 log det Sigma and its condition sum."""
    lg = [mp.log(v) for v in w]
    return mp.fsum(lg) / 2, float(mp.fsum(abs(v) for v in lg) / 2)


def mean_and_cov(lam, D, df):
    """(mu doubles, cov (mpf), condition sums): cov = df / (df - 2) Sigma."""
    mu, L, Sig, Sabs = unpack(lam, D)
    c = mpf(df) / (mpf(df) - 2)
    return _f(mu), Sig * c, float(c) * Sabs


def pth_moment(p, w, df):
    """c sum w (p = 2), c^2 (2 (df - 1) / (df - 4) sum w^2 + (sum w)^2) (p = 4); every
    term is positive, so the condition sum is the value."""
    df = mpf(df)
    c = df / (df - 2)
    if p == 2:
        v = c * mp.fsum(w)
    else:
        v = c ** 2 * (2 * (df - 1) / (df - 4) * mp.fsum(e * e for e in w) + mp.fsum(w) ** 2)
    return v, float(v)


def t_const(D, df):
    df = mpf(df)
    return mp.loggamma((df + D) / 2) - mp.loggamma(df / 2) - mpf(D) / 2 * mp.log(mp.pi * df)


def logdensity(x, mu, w, Q, df):
    """multivariate_t_logpdf rows (mpf) with the absolute 1e-10 pinv cutoff, and
    condition sums |const| + .5 sum |log w| + .5 (df + D) log1p(maha / df)."""
    D = len(w)
    x = _obj(x)
    pinv = np.array([mpf(0) if abs(v) <= mpf('1e-10') else 1 / v for v in w], dtype=object)
    y = mm(x - mu[None, :], Q)
    lg = [mp.log(v) for v in w]
    tc = t_const(D, df)
    e = (mpf(df) + D) / 2
    out = np.empty(x.shape[0], dtype=object)
    S = np.empty(x.shape[0])
    for n in range(x.shape[0]):
        maha = mp.fsum(y[n, k] * y[n, k] * pinv[k] for k in range(D))
        tail = e * mp.log1p(maha / mpf(df))
        out[n] = tc - mp.fsum(lg) / 2 - tail
        S[n] = float(abs(tc) + mp.fsum(abs(v) for v in lg) / 2 + tail)
    return out, S


def logq_draws(w, s, z, df):
    """log q at x = mu + z S / s through the invariant maha = z.z / s^2."""
    D = len(w)
    z, s = _obj(z), _obj(s)
    base = t_const(D, df) - mp.fsum(mp.log(v) for v in w) / 2
    e = (mpf(df) + D) / 2
    return np.array([base - e * mp.log1p(mp.fsum(v * v for v in z[n]) / (s[n] * s[n]) / mpf(df))
                     for n in range(len(s))], dtype=object)


def logq_draws_lam(lam, D, s, z, df):
    """log q at the draws without an eigendecomposition: .5 log det Sigma = sum log
    L_ii = the sum of lambda's log-diagonal, maha = z.z / s^2.  Returns (rows (mpf),
    condition sums |lgamma((df + D) / 2)| + |lgamma(df / 2)| + D / 2 |log(pi df)| +
    sum (|lambda_ii| + 1) + .5 (df + D) log1p(maha / df); the + 1 per diagonal entry is
    the device's exp and log round trip, one rounding of L_ii each)."""
    z, s, lam = _obj(z), _obj(s), _obj(lam)
    diag = [lam[D + i * (i + 1) // 2 + i] for i in range(D)]
    dfm = mpf(df)
    parts = (mp.loggamma((dfm + D) / 2), mp.loggamma(dfm / 2), mpf(D) / 2 * mp.log(mp.pi * dfm))
    base = parts[0] - parts[1] - parts[2] - mp.fsum(diag)
    Sb = mp.fsum(abs(v) for v in parts) + mp.fsum(abs(v) + 1 for v in diag)
    e = (dfm + D) / 2
    out = np.empty(len(s), dtype=object)
    S = np.empty(len(s))
    for n in range(len(s)):
        tail = e * mp.log1p(mp.fsum(v * v for v in z[n]) / (s[n] * s[n]) / dfm)
        out[n] = base - tail
        S[n] = float(Sb + tail)
    return out, S


# ---- targets ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corr_gauss_params(D, seed=512):
    """The CorrGauss set-up in doubles (Sigma* = A A^T / D + I; precision
    symmetrised; log normaliser): model data, exact inputs of both sides."""
    a = np.random.RandomState(seed).randn(D, D)
    sigma = a @ a.T / D + np.eye(D)
    prec = np.linalg.inv(sigma)
    prec = 0.5 * (prec + prec.T)
    _, logdet = np.linalg.slogdet(sigma)
    return prec, -0.5 * logdet - 0.5 * D * np.log(2 * np.pi)


def target(name, x):
    """log p (n) and d log p / dx (n x D) at mpf rows x."""
    n, D = x.shape
    if name == 'isogauss':
        lp = np.empty(n, dtype=object)
        g = np.empty((n, D), dtype=object)
        for r in range(n):
            one = [tm._iso1(v) for v in x[r]]
            lp[r] = mp.fsum(o[0] for o in one)
            g[r] = [o[2] for o in one]
        return lp, g
    prec, const = corr_gauss_params(D)
    g = -mm(x, _obj(prec))
    lp = np.array([mp.fsum(x[r, d] * g[r, d] for d in range(D)) / 2 + mpf(float(const))
                   for r in range(n)], dtype=object)
    return lp, g


# ---- objectives ---------------------------------------------------------------------
def _alpha(obj):
    return mpf(obj[5:]) if obj.startswith('chivi') else None


def _weights(obj, lp, lq, top=None):
    """(value, r (n), c, top): the objective's value and its weights."""
    N = len(lp)
    if obj == 'klvi':
        return None, np.array([mpf(-1) / N] * N, dtype=object), mpf(-1) / 2, None
    if obj == 'klvi_pd':
        v = -(mp.fsum(lp) / N - mp.fsum(lq) / N)
        return v, np.array([mpf(-1) / N] * N, dtype=object), mpf(-1) / 2, None
    a = _alpha(obj)
    lw = lp - lq
    if top is None:
        top = max(lw)
    w = np.array([mp.exp(a * (v - top)) for v in lw], dtype=object)
    r = w * a / N
    return mp.log(mp.fsum(w) / N) / a + top, r, mp.fsum(r) / 2, top


def evaluate(obj, lam, D, df, s, z, tname, grad=True, top=None, root=None):
    """Value and gradient of one objective at lam on the draws (s, z).
    Returns a dict of mpf objects: value, surrogate (the function whose
    derivative the gradient is), gmu (D), gL (packed D (D + 1) / 2), k = cond(S),
    top (CHIVI's max log weight)."""
    mu, L, Sig, _ = unpack(lam, D)
    w, Q, S = root if root is not None else eig(Sig)
    x, _ = transform(S, mu, s, z)
    lp, g = target(tname, x)
    lq = logq_draws(w, s, z, df)
    value, r, c, top = _weights(obj, lp, lq, top)
    ent, _ = entropy(w)
    if obj == 'klvi':
        value = -(ent + mp.fsum(lp) / len(lp))
    out = {'value': value, 'top': top, 'k': mp.sqrt(w[-1] / w[0]),
           'surrogate': value if top is None else mp.fsum(r) / _alpha(obj)}
    if not grad:
        return out
    zs, ss = _obj(z), _obj(s)
    # first-order sensitivities to a relative error of the root (see grad_bars)
    nrm = lambda v: mp.sqrt(mp.fsum(e * e for e in v))
    dx = [nrm(x[n] - mu) for n in range(len(r))]
    gn = [nrm(g[n]) for n in range(len(r))]
    zn = [nrm(zs[n]) / ss[n] for n in range(len(r))]
    ar = [abs(v) for v in r]
    vn = [a * b for a, b in zip(gn, dx)]                 # |d log p_n| <= t vn
    if top is not None:                                  # r_n moves with lw_n and with max lw
        itop = max(range(len(r)), key=lambda n: lp[n] - lq[n])
        vr = [v + vn[itop] for v in vn]
    else:
        vr = [mpf(0)] * len(r)
    out['sens'] = {
        'vS': abs(ent) + (mp.fsum(abs(v) for v in lp) + (0 if obj == 'klvi' else
                                                         mp.fsum(abs(v) for v in lq))) / len(r),
        'Vw': mp.fsum(a * b for a, b in zip(ar, vn)) / mp.fsum(ar),
        'A': mp.fsum(a * b for a, b in zip(ar, dx)),
        'Rg': mp.fsum(a * b for a, b in zip(ar, gn)),
        'RgV': mp.fsum(a * b * v for a, b, v in zip(ar, gn, vr)),
        'Ez': mp.fsum(a * b * c_ for a, b, c_ in zip(ar, zn, dx)),
        'Eg': mp.fsum(a * b * c_ for a, b, c_ in zip(ar, zn, gn)),
        'EgV': mp.fsum(a * b * c_ * v for a, b, c_, v in zip(ar, zn, gn, vr)),
        'rV': mp.fsum(a * v for a, v in zip(ar, vr)),
        'c': abs(c), 's_min': mp.sqrt(w[0]), 'L_norm2': mp.sqrt(w[-1]),
        'Lii_max': max(L[i, i] for i in range(D))}
    out['gmu'] = np.array([mp.fsum(r[n] * g[n, d] for n in range(len(r))) for d in range(D)],
                          dtype=object)
    GS = mm((zs * (r / ss)[:, None]).T, g)
    E = GS + GS.T
    Et = mm(mm(Q.T, E), Q)
    rw = np.array([mp.sqrt(v) for v in w], dtype=object)
    Xt = Et / (rw[:, None] + rw[None, :])
    H = mm(mm(Q, Xt + np.diag(2 * c / w)), Q.T)          # X + 2 c Sigma^-1
    out['sens']['X_fro'] = _frob(Xt)
    GL = mm(H, L)
    out['gL'] = np.array([GL[i, j] * (L[i, i] if i == j else 1)
                          for i in range(D) for j in range(i + 1)], dtype=object)
    return out


# ---- cases ----------------------------------------------------------------------------
def lam_case(D, kind):
    """lambda of Sigma kind (i)-(v) at D (doubles).
      eye      lambda = 0: Sigma = I, every eigenvalue equal
      two      Sigma = Q diag(1/4 x ceil(D/2), 4 x floor(D/2)) Q^T, Q random
               orthogonal, L its Cholesky factor: two eigenvalues, each repeated
               to the rounding of L (split ~1e-16; D = 1 has the one)
      generic  log-diagonal 0.2 randn, off-diagonal 0.5 / sqrt(D) randn
      cond1e4  log-diagonal spread over [-2.3, 2.3], off-diagonal 0.01 randn
      cond1e8  log-diagonal spread over [-4.6, 4.6], row i's off-diagonals
               0.01 L_ii randn"""
    rs = np.random.RandomState(SEED + 1000 * KINDS.index(kind) + D)
    P = D + D * (D + 1) // 2
    if kind == 'eye':
        return np.zeros(P)
    tri = np.tril_indices(D)
    diag = tri[0] == tri[1]
    mu = rs.randn(D) * 0.3
    if kind == 'two':
        q, _ = np.linalg.qr(rs.randn(D, D))
        ev = np.array([0.25] * ((D + 1) // 2) + [4.0] * (D // 2))
        Lc = np.linalg.cholesky((q * ev) @ q.T)
        free = Lc[tri]
        free[diag] = np.log(free[diag])
    elif kind == 'generic':
        free = rs.randn(len(tri[0])) * 0.5 / math.sqrt(D)
        free[diag] = rs.randn(D) * 0.2
    else:
        half = 2.3 if kind == 'cond1e4' else 4.6
        ld = np.linspace(-half, half, D)[rs.permutation(D)] if D > 1 else np.array([half])
        free = rs.randn(len(tri[0])) * 0.01
        if kind == 'cond1e8':
            free *= np.exp(ld)[tri[0]]
        free[diag] = ld
    return np.concatenate([mu, free])


def draws(D, N, df, seed=0):
    """(s, z) in the reference's order (chisquare first, then randn)."""
    rs = np.random.RandomState(SEED + 7919 * seed + 31 * D + N)
    s = np.sqrt(rs.chisquare(df, N) / df)
    return s, rs.randn(N, D)


def special_draws(which, D=33, N=64):
    """CHIVI's weight edges at D = 33 (isogauss, lambda = 0):
      equal     every row the same (s, z): all log weights equal to rounding
      dominant  s = 0.01 in every row but one: x = 100 z there, log p ~ -5000 |z|^2
                against the one row with s = 1 -- it dominates by far more than
                800 nats and every other weight underflows to 0"""
    s, z = draws(D, N, DF, seed=5)
    if which == 'equal':
        return np.full(N, s[0]), np.tile(z[0], (N, 1))
    s = np.full(N, 0.01)
    s[N // 2] = 1.0
    return s, z


def subset(D, n_extra=None):
    """Packed-L indices kept in the fixture at D > LIVE_MAX: every diagonal
    entry, the last row, the first column and n_extra seeded others (64 below
    D = 96, 256 from there on, where the triangle has 6 and 10 tiles)."""
    P = D * (D + 1) // 2
    if n_extra is None:
        n_extra = 64 if D < 96 else 256
    rowstart = lambda i: i * (i + 1) // 2
    keep = {rowstart(i) + i for i in range(D)} | {rowstart(D - 1) + j for j in range(D)}
    keep |= {rowstart(i) for i in range(D)}
    rs = np.random.RandomState(SEED + D)
    keep |= set(rs.choice(P, size=min(P, n_extra), replace=False).tolist())
    return np.array(sorted(keep), dtype=np.int64)


def root_subset(D, n_extra=128):
    """Flat indices of S kept in the fixture where the whole root is too large."""
    keep = {i * D + i for i in range(D)} | {(D - 1) * D + j for j in range(D)}
    keep |= {i * D for i in range(D)}
    rs = np.random.RandomState(SEED + 3 * D)
    keep |= set(rs.choice(D * D, size=n_extra, replace=False).tolist())
    return np.array(sorted(keep), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _root(D, kind):
    with mp.workdps(DIGITS):
        mu, L, Sig, Sabs = unpack(lam_case(D, kind), D)
        return (mu, L, Sig, Sabs) + eig(Sig)


def compute_root(D, kind):
    """Reference of the root and the eigenvalue helpers of (D, kind), as doubles:
    S (whole, or at `S_idx` for D >= 96 and for D >= 63 off the generic kind),
    ||S||_2, k = cond(S), ||Sigma||_2, ||Sigma||_F, gamma = || |L||L|^T ||_F / ||Sigma||_2,
    entropy / 2nd / 4th moment as (hi, lo, S)."""
    with mp.workdps(DIGITS):
        mu, L, Sig, Sabs, w, Q, S = _root(D, kind)
        whole = D <= LIVE_MAX or (D <= 65 and kind == 'generic')
        idx = np.arange(D * D) if whole else root_subset(D)
        hi, lo = pair(S.ravel()[idx])
        out = {'S_idx': idx, 'S_hi': hi, 'S_lo': lo.astype(np.float32),
               'S_norm2': float(mp.sqrt(w[-1])), 'S_fro': float(_frob(S)),
               'k': float(mp.sqrt(w[-1] / w[0])), 'w_min': float(w[0]), 'w_max': float(w[-1]),
               'gamma': float(np.linalg.norm(Sabs)) / float(w[-1])}
        e, eS = entropy(w)
        out['entropy'] = np.array(pair(e) + (eS,))
        for p in (2, 4):
            v, vS = pth_moment(p, w, DF)
            out['m%d' % p] = np.array(pair(v) + (vS,))
        return out


def case_draws(tname, D, kind, N, special=None):
    if special:
        return special_draws(special, D, N)
    return draws(D, N, DF, seed=TARGETS.index(tname))


@functools.lru_cache(maxsize=None)
def compute_grad(tname, D, kind, N, obj, special=None):
    """Reference of one value-and-gradient case as doubles: value (hi, lo), the
    mean block whole, the packed-L block whole (D <= LIVE_MAX) or at subset(D),
    each block's largest entry and Frobenius norm over the whole block, k."""
    with mp.workdps(DIGITS):
        s, z = case_draws(tname, D, kind, N, special)
        r = evaluate(obj, lam_case(D, kind), D, DF, s, z, tname, root=_root(D, kind)[4:])
        idx = np.arange(D * (D + 1) // 2) if D <= LIVE_MAX else subset(D)
        out = {'value': np.array(pair(r['value'])), 'k': float(r['k']), 'gL_idx': idx}
        out['gamma'] = float(np.linalg.norm(_root(D, kind)[3])) / float(_root(D, kind)[4][-1])
        out['sens'] = np.array([float(r['sens'][q]) for q in SENS])
        for name, blk in (('gmu', r['gmu']), ('gL', r['gL'])):
            out[name + '_max'] = float(max(abs(v) for v in blk))
            out[name + '_fro'] = float(_frob(blk))
            hi, lo = pair(blk if name == 'gmu' else blk[idx])
            out[name + '_hi'], out[name + '_lo'] = hi, lo.astype(np.float32)
        return out


SENS = ('vS', 'Vw', 'A', 'Rg', 'RgV', 'Ez', 'Eg', 'EgV', 'rV', 'c', 's_min', 'L_norm2', 'Lii_max',
        'X_fro')


def grad_key(tname, D, kind, N, obj, special=None):
    return 'grad/%s/%d/%s/%d/%s%s' % (tname, D, kind, N, obj, '/' + special if special else '')


def root_key(D, kind):
    return 'root/%d/%s' % (D, kind)


@functools.lru_cache(maxsize=1)
def _fixture():
    return unpack_fixture(FIXTURE)


_BUFFERS = (('f64', np.float64), ('f32', np.float32), ('u8', np.uint8))


def pack_fixture(path, arrays):
    """One buffer per dtype and a JSON index (name -> buffer, offset, shape): a
    zip member per array would cost more than the data."""
    import json
    bufs = {b: [] for b, _ in _BUFFERS}
    used = {b: 0 for b, _ in _BUFFERS}
    index = {}
    for k in sorted(arrays):
        a = np.asarray(arrays[k])
        b = 'u8' if a.dtype == np.uint8 else 'f32' if a.dtype == np.float32 else 'f64'
        a = a.astype(dict(_BUFFERS)[b])
        index[k] = [b, used[b], list(a.shape)]
        bufs[b].append(a.ravel())
        used[b] += a.size
    out = {b: np.concatenate(v) if v else np.zeros(0, dtype=dict(_BUFFERS)[b])
           for b, v in bufs.items()}
    out['index'] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    np.savez_compressed(path, **out)


def unpack_fixture(path):
    import json
    with np.load(path) as f:
        index = json.loads(f['index'].tobytes().decode())
        bufs = {b: f[b] for b, _ in _BUFFERS}
    out = {}
    for k, (b, off, shape) in index.items():
        n = int(np.prod(shape)) if shape else 1
        out[k] = bufs[b][off:off + n].reshape(shape)
    return out


def _from_fixture(prefix):
    fx = _fixture()
    out = {k[len(prefix) + 1:]: v for k, v in fx.items() if k.startswith(prefix + '/')}
    if not out:
        raise KeyError('no fixture entry %s' % prefix)
    out = {k: (v if v.ndim else float(v)) for k, v in out.items()}
    D = int(prefix.split('/')[2 if prefix.startswith('grad') else 1])
    if 'gL_hi' in out:                         # the index sets are not stored
        out['gL_idx'] = subset(D)
    if 'S_hi' in out:
        out['S_idx'] = np.arange(D * D) if out['S_hi'].size == D * D else root_subset(D)
    return out


@functools.lru_cache(maxsize=None)
def root_ref(D, kind):
    """compute_root's dict: live (memoised) at D <= LIVE_MAX, else the fixture's."""
    return compute_root(D, kind) if D <= LIVE_MAX else _from_fixture(root_key(D, kind))


@functools.lru_cache(maxsize=None)
def grad_ref(tname, D, kind, N, obj, special=None):
    """compute_grad's dict: live (memoised) at D <= LIVE_MAX, else the fixture's.
    KLVI-PD shares KLVI's gradient; only its value is its own."""
    if D <= LIVE_MAX:
        return compute_grad(tname, D, kind, N, obj, special)
    if obj == 'klvi_pd':
        out = dict(_from_fixture(grad_key(tname, D, kind, N, 'klvi')))
        out['value'] = _from_fixture(grad_key(tname, D, kind, N, obj))['value']
        return out
    return _from_fixture(grad_key(tname, D, kind, N, obj))


# the value-and-gradient cases of the GPU tests (§d of the issue) ------------------------
GRAD_KINDS = ('eye', 'generic', 'cond1e4')


def grad_cases():
    out = [(t, D, k, 64) for t in TARGETS for D in DIMS for k in GRAD_KINDS]
    out += [(t, D, k, N) for t in TARGETS for D in (33, 64) for k in GRAD_KINDS
            for N in (1, 63, 65, 128)]
    # whole tiles with a G_S product off the LDS-DMA shapes: fr_weights_kernel
    out += [(t, 96, 'generic', 65) for t in TARGETS]
    return out


HOOK_CASES = [('corr_gauss', 64, 'generic', N) for N in (64, 65, 512, 576)]


# ---- the error model (GPU tests) ----------------------------------------------------------
def root_bar(D, k, gamma):
    """Bar on ||S_dev - S||_F / ||S||_2.  First order: Newton-Schulz stops at
    ||I - Z Y||_F <= tau = NS_TAU sqrt(D), and Y = Sigma'^(1/2) (I - E)^(1/2), so the
    root's relative error is <= tau (tau / 2 per eigenvalue); factor 4 for the
    second-order terms and the rounding of the products inside the iteration.
    Rounding term: Sigma = L L^T carries (D + 2) 2^-53 of its condition sums,
    gamma relative to ||Sigma||_2, and the square root's relative condition number
    is k / 2."""
    return 4.0 * NS_TAU * math.sqrt(D) + 0.5 * k * (D + 2) * UNIT * gamma


def solve_bar(D, k, gamma):
    """Bar on the relative error of the Sylvester solution X: kappa PCG_TOL from
    the accepted residual (kappa = (2 + k + 1/k) / 4 the preconditioned condition
    number) plus k tau from the root (a relative perturbation eps of S moves X by
    at most ||dS|| / s_min = k eps); factor 4 as above."""
    kappa = (2.0 + k + 1.0 / k) / 4.0
    return 4.0 * (kappa * PCG_TOL + k * NS_TAU * math.sqrt(D)) + k * (D + 2) * UNIT * gamma


# ---- log q of arbitrary points (§f) ----------------------------------------------------------
LOGQ_DIMS = (1, 33, 64, 65)


def logq_case(D, which):
    """(lam, x): 24 points up to 1e3 scale units from mu.
      generic  the generic Sigma
      cutoff   (D >= 3) the generic Sigma of D - 2 dimensions, and two decoupled
               directions (rows of L with the diagonal entry only) with eigenvalues
               1e-8 and 1e-12, one on each side of the 1e-10 pinv cutoff and a
               factor 100 from it.  The block structure keeps both eigenvalues
               exact products of doubles, so an fp64 eigensolver returns them to
               relative precision and log(1e-12) in log_pdet is stable; the
               points move along the dropped direction too."""
    rs = np.random.RandomState(SEED + 17 * D + (which == 'cutoff'))
    if which == 'generic':
        lam = lam_case(D, 'generic')
    else:
        sub = lam_case(D - 2, 'generic')
        M = np.zeros((D, D))
        M[np.tril_indices(D - 2)] = sub[D - 2:]
        M[D - 2, D - 2] = 0.5 * math.log(1e-8)
        M[D - 1, D - 1] = 0.5 * math.log(1e-12)
        lam = np.concatenate([sub[:D - 2], rs.randn(2), M[np.tril_indices(D)]])
    _, L, _ = _np_unpack(lam, D)
    far = 10.0 ** rs.uniform(-1, 3, size=24)
    x = lam[:D] + (rs.randn(24, D) * far[:, None] / math.sqrt(D)) @ L.T
    return lam, x


def _np_unpack(lam, D):
    M = np.zeros((D, D))
    M[np.tril_indices(D)] = lam[D:]
    L = M - np.diag(np.diag(M)) + np.diag(np.exp(np.diag(M)))
    return lam[:D], L, L @ L.T


def logq_whiches(D):
    return ('generic', 'cutoff') if D >= 3 else ('generic',)


def compute_logq(D, which):
    with mp.workdps(DIGITS):
        lam, x = logq_case(D, which)
        mu, L, Sig, _ = unpack(lam, D)
        w, Q, _ = eig(Sig)
        v, S = logdensity(x, mu, w, Q, DF)
        hi, lo = pair(v)
        return {'hi': hi, 'lo': lo, 'S': S, 'w_min': float(w[0]), 'w_max': float(w[-1])}


@functools.lru_cache(maxsize=None)
def logq_ref(D, which):
    if D <= LIVE_MAX:
        return compute_logq(D, which)
    return _from_fixture('logq/%d/%s' % (D, which))


def grad_bars(ref, D, N, obj):
    """Bars of one value-and-gradient case, each block against its own scale:
    {'value': absolute, 'gmu': (max bar, 2-norm bar), 'gL': (max bar, 2-norm bar)}.
    With t = NS_TAU sqrt(D) the root's relative error, k = cond(S) and kappa =
    (2 + k + 1/k) / 4 (root_bar, solve_bar):
      value, mean block   x inherits t:                 4 t            x scale
      packed-L block      X inherits kappa PCG_TOL + k t: 4 (kappa 1e-9 + k t) x scale
    where scale is |value|, the mp block's largest entry (max norm) or its Frobenius
    norm (2-norm), plus the block's rounding term, taken once:
      value   (N + D + 8) 2^-53 vS, vS = |entropy| + mean |log p| (+ mean |log q|)
      mean    (N + 8) 2^-53 Rg, Rg = sum |r_n| |g_n|
      packed  (2 D + 8) 2^-53 (||X||_F ||L||_2 max(1, max L_ii) + 2 |c| sqrt(D))
    One term was missing for the value, found on five recorded cases (isogauss,
    CHIVI and KLVI-PD at D = 1, 31, 33 with lambda = 0 or N = 1; errors 3e-12..5e-11
    against 1e-12..3e-11): there log p - log q nearly cancels, |value| is ~1e-3 of
    its terms, and the root's error does not shrink with it.  To first order
    d value = sum_n (|r_n| / sum |r|) g_n . dx_n, at most t Vw with Vw the weighted
    mean of |g_n| |x_n - mu|; the value's scale is max(|value|, Vw).  No other block
    needed a further term (profiles/fullrank_mp/errors.json)."""
    q = dict(zip(SENS, ref['sens']))
    t = NS_TAU * math.sqrt(D)
    k = ref['k']
    kappa = (2.0 + k + 1.0 / k) / 4.0
    rx, rX = 4.0 * t, 4.0 * (kappa * PCG_TOL + k * t)
    lmax = q['L_norm2'] * max(1.0, q['Lii_max'])
    rnd_m = (N + 8) * UNIT * q['Rg']
    rnd_l = (2 * D + 8) * UNIT * (q['X_fro'] * lmax + 2.0 * q['c'] * math.sqrt(D))
    return {'value': rx * max(abs(ref['value'][0]), q['Vw']) + (N + D + 8) * UNIT * q['vS'],
            'gmu': (rx * ref['gmu_max'] + rnd_m, rx * ref['gmu_fro'] + rnd_m),
            'gL': (rX * ref['gL_max'] + rnd_l, rX * ref['gL_fro'] + rnd_l)}


def block_errors(value, grad, ref, D):
    """2-norm and max errors of (value, grad) against a reference dict, absolute:
    {'value', 'gmu', 'gmu_max', 'gL', 'gL_max'} (the packed-L block over the
    reference's indices)."""
    grad = np.asarray(grad, dtype=np.float64)
    dm = (grad[:D] - ref['gmu_hi']) - ref['gmu_lo']
    dl = (grad[D:][ref['gL_idx']] - ref['gL_hi']) - ref['gL_lo']
    out = {'value': abs((float(value) - ref['value'][0]) - ref['value'][1]),
           'gmu': float(np.linalg.norm(dm)), 'gmu_max': float(np.max(np.abs(dm))),
           'gL': float(np.linalg.norm(dl)), 'gL_max': float(np.max(np.abs(dl)))}
    if not (np.isfinite(value) and np.all(np.isfinite(grad))):
        out = {k: np.inf for k in out}
    return out
