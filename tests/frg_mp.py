"""50-digit reference (mpmath) of the Cholesky full-rank Gaussian family and its three
estimators on the isogauss target, with seeded edge sets, for tests/test_frg_host.py
(the numpy restatement tests/frg_cases.py against it) and tests/test_gpu_frg_edges.py
(the kernels of vb_frg.hip against the restatement).

Errors are in units of 2^-53 S.  S follows the project's rule: the absolute terms of
every cancelling inner sum, carried through the term's derivative.

  x_ni = mu_i + sum_j L_ij z_nj          Sx_ni = |mu_i| + sum_j |L_ij| |z_nj|
  log p(x_n) = sum_i -(x_ni^2 + log 2 pi) / 2   (isogauss; g_ni = -x_ni, Sg = Sx)
                                         Slp_n = sum_i (x_ni^2 + log 2 pi) / 2 + |x_ni| Sx_ni
  log q of arbitrary x: y = L^-1 (x - mu).  The cancelling sums are x - mu and the
  forward substitution; its error is bounded through the comparison matrix M(L)
  (|L_ii| on the diagonal, -|L_ij| off it): Sy = M(L)^-1 (|L| |y| + |x| + |mu|), and
                                         Slq = D/2 log 2 pi + sum |M_ii| + sum_i (y_i^2 / 2 + |y_i| Sy_i)
  lw_n = log p(x_n) + D/2 log 2 pi + sum M_ii + zz_n / 2
                                         Slw_n = Slp_n + D/2 log 2 pi + sum |M_ii| + zz_n / 2
  KLVI value                             D/2 (1 + log 2 pi) + sum |M_ii| + mean Slp
  KLVI_PD value                          mean Slw
  CHIVI value                            |max lw| + Slw_max + sum_n (w_n / sum w) (Slw_n + Slw_max)
  weights r_n: exact for KLVI; CHIVI r_n = alpha w_n / N carries the relative error
  er_n = alpha (Slw_n + Slw_max) (in units), so
  grad mu_i                              sum_n |r_n| (Sg_ni + |g_ni| (1 + er_n))
  G_L[i][j]                              sum_n |r_n| |z_nj| (Sg_ni + |g_ni| (1 + er_n))
  packed diagonal                        S(G_L[i][i]) L_ii + sum_n |r_n| (1 + er_n)
"""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50
LOG2PI = mp.log(2 * mp.pi)
U = 2.0 ** -53


def _unpack(lam, D):
    lam = [mpf(float(v)) for v in lam]
    mu = lam[:D]
    L = [[mpf(0)] * D for _ in range(D)]
    k = D
    Mdiag = []
    for i in range(D):
        for j in range(i + 1):
            L[i][j] = mp.exp(lam[k]) if i == j else lam[k]
            if i == j:
                Mdiag.append(lam[k])
            k += 1
    return mu, L, Mdiag


def sample(lam, z):
    """x [n][D] and Sx [n][D]."""
    n, D = z.shape
    mu, L, _ = _unpack(lam, D)
    x = [[mu[i] + sum(L[i][j] * mpf(float(z[r, j])) for j in range(i + 1)) for i in range(D)]
         for r in range(n)]
    S = [[abs(mu[i]) + sum(abs(L[i][j]) * abs(mpf(float(z[r, j]))) for j in range(i + 1))
          for i in range(D)] for r in range(n)]
    return x, S


def logdensity(x, lam):
    """log q [n] of arbitrary points and Slq [n]."""
    n, D = x.shape
    mu, L, Md = _unpack(lam, D)
    out, S = [], []
    for r in range(n):
        y, sy = [], []
        for i in range(D):
            xi = mpf(float(x[r, i]))
            acc = xi - mu[i]
            sa = abs(xi) + abs(mu[i])
            for j in range(i):
                acc -= L[i][j] * y[j]
                sa += abs(L[i][j]) * (abs(y[j]) + sy[j])
            y.append(acc / L[i][i])
            sy.append(sa / L[i][i] + abs(y[-1]))   # M(L)^-1 (|L||y| + |x| + |mu|), row i
        out.append(-mpf(D) / 2 * LOG2PI - sum(Md) - sum(v * v for v in y) / 2)
        S.append(mpf(D) / 2 * LOG2PI + sum(abs(m) for m in Md) +
                 sum(y[i] * y[i] / 2 + abs(y[i]) * sy[i] for i in range(D)))
    return out, S


def _rows(lam, z):
    n, D = z.shape
    mu, L, Md = _unpack(lam, D)
    x, Sx = sample(lam, z)
    lp = [sum(-(v * v + LOG2PI) / 2 for v in x[r]) for r in range(n)]
    Slp = [sum((x[r][i] ** 2 + LOG2PI) / 2 + abs(x[r][i]) * Sx[r][i] for i in range(D))
           for r in range(n)]
    zz = [sum(mpf(float(v)) ** 2 for v in z[r]) for r in range(n)]
    c = mpf(D) / 2 * LOG2PI
    lw = [lp[r] + c + sum(Md) + zz[r] / 2 for r in range(n)]
    Slw = [Slp[r] + c + sum(abs(m) for m in Md) + zz[r] / 2 for r in range(n)]
    return dict(n=n, D=D, L=L, Md=Md, x=x, Sx=Sx, lp=lp, Slp=Slp, zz=zz, lw=lw, Slw=Slw)


def _pack(R, z, r, er):
    """The packed gradient of weights r (relative error er, in units) and its S."""
    n, D, L, x, Sx = R['n'], R['D'], R['L'], R['x'], R['Sx']
    zm = [[mpf(float(v)) for v in z[k]] for k in range(n)]
    g = [[-v for v in x[k]] for k in range(n)]
    t = [[abs(r[k]) * (Sx[k][i] + abs(g[k][i]) * (1 + er[k])) for i in range(D)] for k in range(n)]
    grad = [sum(r[k] * g[k][i] for k in range(n)) for i in range(D)]
    S = [sum(t[k][i] for k in range(n)) for i in range(D)]
    rs = sum(r)
    srs = sum(abs(r[k]) * (1 + er[k]) for k in range(n))
    for i in range(D):
        for j in range(i + 1):
            v = sum(r[k] * g[k][i] * zm[k][j] for k in range(n))
            s = sum(t[k][i] * abs(zm[k][j]) for k in range(n))
            if i == j:
                v = v * L[i][i] + rs
                s = s * L[i][i] + srs
            grad.append(v)
            S.append(s)
    return grad, S


def klvi(lam, z, pd=False):
    """(value, S value, grad [P], S grad [P]) of KLVI (pd: KLVI_PD) on isogauss."""
    R = _rows(lam, z)
    n, D = R['n'], R['D']
    r = [-mpf(1) / n] * n
    if pd:
        v = -sum(R['lw']) / n
        sv = sum(R['Slw']) / n
    else:
        v = -(mpf(D) / 2 * (1 + LOG2PI) + sum(R['Md']) + sum(R['lp']) / n)
        sv = mpf(D) / 2 * (1 + LOG2PI) + sum(abs(m) for m in R['Md']) + sum(R['Slp']) / n
    g, sg = _pack(R, z, r, [mpf(0)] * n)
    return v, sv, g, sg


def chivi(lam, z, alpha):
    R = _rows(lam, z)
    n = R['n']
    lw, Slw = R['lw'], R['Slw']
    im = max(range(n), key=lambda k: lw[k])
    mx = lw[im]
    a = mpf(alpha)
    w = [mp.exp(a * (lw[k] - mx)) for k in range(n)]
    sw = sum(w)
    v = mp.log(sw / n) / a + mx
    sv = abs(mx) + Slw[im] + sum(w[k] / sw * (Slw[k] + Slw[im]) for k in range(n))
    r = [a * w[k] / n for k in range(n)]
    er = [a * (Slw[k] + Slw[im]) for k in range(n)]
    g, sg = _pack(R, z, r, er)
    return v, sv, g, sg


def units(got, ref, S):
    """max |got - ref| / (2^-53 S) over the entries (S floored at |ref|)."""
    got = np.atleast_1d(np.asarray(got, dtype=float)).ravel()
    ref = list(np.ravel(np.array(ref, dtype=object)))
    S = list(np.ravel(np.array(S, dtype=object)))
    worst = 0.0
    for a, b, s in zip(got, ref, S):
        s = max(s, abs(b), mpf(10) ** -300)
        worst = max(worst, float(abs(mpf(float(a)) - b) / (s * mpf(U))))
    return worst


# ---- edge sets --------------------------------------------------------------
def edge_lam(kind, D, seed=0):
    """Seeded var_param [D (D + 3) / 2] of an edge instance.
    diag:   M_ii cycling through {-8, 0, 4} within one L
    offd:   off-diagonals exactly zero, ~1e-6 and ~1e3, cycling by entry
    cond:   cond(L) ~ 1e8 (log diagonal from 0 down to log 1e-8, rows scaled with it)
    mu:     mu = +-1e6 (x - mu cancels in log q)
    plain:  a benign L"""
    rs = np.random.RandomState(1000 + 17 * D + seed)
    M = np.tril(rs.randn(D, D) * 0.1)
    mu = rs.randn(D) * 0.3
    dg = rs.randn(D) * 0.2
    if kind == 'diag':
        dg = np.array([(-8.0, 0.0, 4.0)[i % 3] for i in range(D)])
    elif kind == 'offd':
        ii, jj = np.tril_indices(D, -1)
        sc = np.array([0.0, 1e-6, 1e3])[(ii + 2 * jj) % 3]
        M[ii, jj] = rs.randn(len(ii)) * sc
    elif kind == 'cond':
        dg = np.linspace(0.0, np.log(1e-8), D) if D > 1 else np.array([np.log(1e-8)])
        M = np.tril(rs.randn(D, D) * 0.1) * np.exp(dg)[:, None]   # L = diag (I + 0.1 strict tril)
    elif kind == 'mu':
        mu = np.where(np.arange(D) % 2 == 0, 1e6, -1e6) + rs.randn(D)
    elif kind != 'plain':
        raise ValueError(kind)
    M[np.diag_indices(D)] = dg
    return np.concatenate([mu, M[np.tril_indices(D)]])


EDGE_KINDS = ('diag', 'offd', 'cond', 'mu')


def edge_draws(n, D, seed=0):
    """Seeded z [n][D]; row n // 2 is all zeros."""
    z = np.random.RandomState(2000 + 31 * D + n + seed).randn(n, D)
    z[n // 2] = 0.0
    return z


def dominant_pair(n, D, seed=0):
    """(lam, z): CHIVI rows with one log weight >= 700 above the rest on isogauss.
    lam has mu = 0, M_ii = 1 and no off-diagonals, so lw_n = const - (e^2 - 1) |z_n|^2 / 2;
    row 0 of z is zero and every other row has |z_n|^2 >= 1400 / (e^2 - 1)."""
    M = np.zeros((D, D))
    M[np.diag_indices(D)] = 1.0
    lam = np.concatenate([np.zeros(D), M[np.tril_indices(D)]])
    z = np.random.RandomState(3000 + 31 * D + n + seed).randn(n, D)
    z[0] = 0.0
    for k in range(1, n):
        need = np.sqrt(1400.0 / (np.e ** 2 - 1.0)) * (1.0 + 0.02 * k)
        z[k] *= need / np.sqrt(np.sum(z[k] ** 2))
    return lam, z


# ---- the same S in float64 numpy (vectorised), for shapes too large for mpmath -----
def np_scales(lam, z, alpha=None):
    """dict of S for sample [n, D], klvi_value, klvi_pd_value, klvi_grad [P] and, with
    alpha, chivi_value / chivi_grad [P]: the module docstring's formulas."""
    from oracle.fullrank_oracle import unpack
    n, D = z.shape
    mu, L, _ = unpack(np.asarray(lam, dtype=float), D)
    l2p = float(LOG2PI)
    aL, az = np.abs(L), np.abs(z)
    x = mu + z @ L.T
    Sx = np.abs(mu) + az @ aL.T
    Slp = np.sum((x * x + l2p) / 2 + np.abs(x) * Sx, axis=1)
    sM = float(np.sum(np.abs(np.log(np.diag(L)))))
    Slw = Slp + D / 2 * l2p + sM + np.sum(z * z, axis=1) / 2
    out = {'sample': Sx, 'klvi_value': D / 2 * (1 + l2p) + sM + np.mean(Slp),
           'klvi_pd_value': np.mean(Slw)}

    def pack(r, er):
        t = np.abs(r)[:, None] * (Sx + np.abs(x) * (1 + er)[:, None])
        SG = t.T @ az
        SG[np.diag_indices(D)] = np.diag(SG) * np.diag(L) + np.sum(np.abs(r) * (1 + er))
        return np.concatenate([t.sum(axis=0), SG[np.tril_indices(D)]])

    out['klvi_grad'] = pack(np.full(n, 1.0 / n), np.zeros(n))
    if alpha is not None:
        lw = np.sum(-(x * x + l2p) / 2, axis=1) + D / 2 * l2p + np.sum(np.log(np.diag(L))) \
            + np.sum(z * z, axis=1) / 2
        im = int(np.argmax(lw))
        w = np.exp(alpha * (lw - lw[im]))
        out['chivi_value'] = abs(lw[im]) + Slw[im] + np.sum(w / np.sum(w) * (Slw + Slw[im]))
        out['chivi_grad'] = pack(alpha * w / n, alpha * (Slw + Slw[im]))
    return out


def np_logdensity_scale(x, lam):
    """S [n] of log q at arbitrary points x [n, D]."""
    from oracle.fullrank_oracle import unpack
    n, D = x.shape
    mu, L, _ = unpack(np.asarray(lam, dtype=float), D)
    y = np.zeros((n, D))
    sy = np.zeros((n, D))
    for i in range(D):
        y[:, i] = (x[:, i] - mu[i] - y[:, :i] @ L[i, :i]) / L[i, i]   # forward substitution
        sa = np.abs(x[:, i]) + abs(mu[i]) + (np.abs(y[:, :i]) + sy[:, :i]) @ np.abs(L[i, :i])
        sy[:, i] = sa / L[i, i] + np.abs(y[:, i])
    return (D / 2 * float(LOG2PI) + np.sum(np.abs(np.log(np.diag(L)))) +
            np.sum(y * y / 2 + np.abs(y) * sy, axis=1))


# Worst error of the numpy restatement (tests/frg_cases.py) against this reference over
# the edge instances of tests/test_frg_host.py, in units of 2^-53 S, per function;
# measured by that test, which asserts twice these figures.  The GPU edge test allows
# the kernels 8 times them.
FRG_ORACLE_ERR = {
    'sample': 2.99,         # D = 65
    'logdensity': 0.79,
    'klvi_value': 1.42,
    'klvi_grad': 2.16,      # also the KLVI_PD gradient (the same weights)
    'klvi_pd_value': 2.50,
    'chivi_value': 0.50,
    'chivi_grad': 0.88,
}
