"""Device target log densities (the model plug-in boundary).

In the reference, ``logdensity`` is an arbitrary autograd-differentiable
callable or ``make_stan_log_density(fit)`` (viabel/vb.py:314-321).  A Python
callable cannot run inside a HIP kernel, so the device path takes targets
from this registry; each carries the kernel-side target id.  Calling a target
evaluates log p(x) for x of shape (N, D) on the GPU, like the reference's
``logdensity(samples)``.

Targets:
  isogauss(D)            N(0, I_D)                                  config 3
  mixture(D)             per-coordinate 0.5 N(-2,1) + 0.5 N(2,1)    normal-mixture.ipynb
  funnel(D)              Neal's funnel, x[1] = log sigma            funnel-distribution.ipynb
  eight_schools_ncp()    eight_schools_ncp.stan log_prob (D = 10)   eight-schools.ipynb
  corr_gauss(D)          N(0, A A^T / D + I), A = RandomState(512).randn(D, D)
                         (full-rank family)
  regression(x, y, ...)  generalised linear model over a data matrix held on the
                         device: beta ~ N(0, s^2 I), y_m | beta through a gaussian,
                         student_t or bernoulli_logit link of x_m . beta
                         (robust-regression.ipynb; VB_TARGET_REGRESSION)
  robust_regression(x, y, df)   regression with the student_t likelihood
  logistic_regression(x, y)     regression with the bernoulli_logit likelihood
  poisson_regression(x, y, offset=None)
                         regression with the poisson_log likelihood: counts y_m with mean
                         exp(x_m . beta + offset_m), offset = log exposure
  negative_binomial_regression(x, y, phi, offset=None)
                         ... with the neg_binomial_2_log likelihood (variance mu + mu^2 / phi)
  regression(..., learn_scale=True) / regression(..., learn_phi=True)
                         the same models with the gaussian / student_t scale sigma, or the
                         negative binomial's dispersion phi, learned on the device: x = [beta
                         (p), lambda], lambda = log sigma or log phi, D = p + 1, e^lambda ~
                         half-Cauchy(0, hyper_scale)
  linear_regression(x, y)       gaussian regression with learned sigma
  robust_regression(x, y, df, learn_scale=True)
  negative_binomial_regression(x, y, learn_phi=True)
  hierarchical_normal(y, sigma, centered=False, ...)
                         hierarchical normal means over J groups held on the device,
                         x = [mu, log tau, theta or theta_tilde (J)], D = J + 2, centred
                         or non-centred (VB_TARGET_HIERARCHICAL)
  eight_schools_cp()     eight_schools_cp.stan log_prob (D = 10): hierarchical_normal
                         with the eight-schools data, centred       eight-schools.ipynb
  multilevel_regression(x, y, group, likelihood='gaussian', centered=False, ...)
                         regression with group intercepts a_g sharing a learned scale tau,
                         held on the device: x = [beta (p), log tau, a or a_tilde (G)],
                         D = p + 1 + G, the three likelihoods of regression, centred or
                         non-centred (VB_TARGET_MULTILEVEL)
  multilevel_logistic_regression(x, y, group)     ... with the bernoulli_logit likelihood
  multilevel_robust_regression(x, y, group, df)   ... with the student_t likelihood
  multilevel_poisson_regression(x, y, group, offset=None)         ... poisson_log
  multilevel_negative_binomial_regression(x, y, group, phi, offset=None)
                                                  ... neg_binomial_2_log

User models (the reference's make_stan_log_density, vb.py:314-321, and autograd
callables): callback(fn, D), from_stan(fit, D) and torch_target(f, D) evaluate
the model on the HOST once per optimisation step on the whole batch of samples
(VB_TARGET_CALLBACK); sampling, weights, gradient reductions and the optimiser
stay on the device.  This is the model boundary, not a fallback of the VI
computation: the model is the user's code and runs where that code runs.

Device model plugins (VB_TARGET_PLUGIN): device_model(code_object, dim, data) runs the
user's model ON THE DEVICE -- a gfx950 code object with the kernel contract of
include/viabel_amd.h, written with include/viabel_amd_model.h and compiled with
viabel_amd.plugin.compile -- in place of the host callback: no copy, synchronisation or
Python call per step.  example_model(name, ...) wraps the shipped models of
viabel_amd/models (robust_regression, banana, isogauss_raw).
"""
import numpy as np

from . import _native as nat

__all__ = ['Target', 'isogauss', 'mixture', 'funnel', 'eight_schools_ncp', 'corr_gauss',
           'regression', 'linear_regression', 'robust_regression', 'logistic_regression',
           'poisson_regression', 'negative_binomial_regression',
           'multilevel_poisson_regression', 'multilevel_negative_binomial_regression',
           'hierarchical_normal', 'eight_schools_cp',
           'multilevel_regression', 'multilevel_logistic_regression',
           'multilevel_robust_regression',
           'callback', 'from_stan', 'torch_target', 'as_target',
           'device_model', 'example_model']


class Target:
    def __init__(self, kind, dim, name, params=None):
        # dim None: a user model whose dimension is taken from the variational
        # family it is used with (like the reference's make_stan_log_density)
        self.kind, self.dim, self.name = int(kind), None if dim is None else int(dim), name
        self.params = None if params is None else nat.as_f64(params)

    def bind(self, dim):
        """This target for dimension `dim` (a copy when the dimension was left open)."""
        if self.dim is None:
            import copy
            t = copy.copy(self)
            t.dim = int(dim)
            return t
        return self

    _cfunc = None   # ctypes callback of a host target (kept alive with the target)

    @property
    def separable(self):
        return self.kind in (nat.TARGET_ISOGAUSS, nat.TARGET_MIXTURE)

    def _struct(self):
        cb = self._cfunc if self._cfunc is not None else nat.TARGET_CALLBACK_T()
        if self.params is None:
            return nat.Target(self.kind, 0, self.dim, None, 0, cb, None)
        return nat.Target(self.kind, 0, self.dim, nat.dptr(self.params), self.params.size, cb, None)

    def logdensity_and_grad(self, x):
        x = nat.as_f64(np.atleast_2d(x))
        if self.dim is None:
            return self.bind(x.shape[1]).logdensity_and_grad(x)
        if x.shape[1] != self.dim:
            raise ValueError('expected x with %d columns, got %s' % (self.dim, x.shape))
        n = x.shape[0]
        lp = np.empty(n)
        g = np.empty_like(x)
        t = self._struct()
        nat.check(nat.lib().vb_target_logdensity(nat.context().handle, t, nat.dptr(x), n,
                                                 nat.dptr(lp), nat.dptr(g)))
        return lp, g

    def __call__(self, x):
        return self.logdensity_and_grad(x)[0]

    def __repr__(self):
        return 'viabel_amd.targets.%s(D=%d)' % (self.name, self.dim)


def isogauss(dim):
    return Target(nat.TARGET_ISOGAUSS, dim, 'isogauss')


def mixture(dim=1):
    return Target(nat.TARGET_MIXTURE, dim, 'mixture')


def funnel(dim=2):
    if dim < 2:
        raise ValueError('funnel needs dim >= 2')
    return Target(nat.TARGET_FUNNEL, dim, 'funnel')


def eight_schools_ncp():
    return Target(nat.TARGET_EIGHT_SCHOOLS_NCP, 10, 'eight_schools_ncp')


def corr_gauss(dim, seed=512):
    """N(0, Sigma*) with Sigma* = A A^T / dim + I, A = RandomState(seed).randn(dim, dim).
    The precision and log normaliser are formed once here (model set-up); every
    evaluation runs on the device."""
    a = np.random.RandomState(seed).randn(dim, dim)
    sigma = a @ a.T / dim + np.eye(dim)
    prec = np.linalg.inv(sigma)
    prec = 0.5 * (prec + prec.T)
    _, logdet = np.linalg.slogdet(sigma)
    const = -0.5 * logdet - 0.5 * dim * np.log(2 * np.pi)
    t = Target(nat.TARGET_CORR_GAUSS, dim, 'corr_gauss', np.concatenate([prec.ravel(), [const]]))
    t.sigma = sigma
    return t


_LIKELIHOODS = {'gaussian': 0, 'student_t': 1, 'bernoulli_logit': 2, 'poisson_log': 3,
                'neg_binomial_2_log': 4}
_COUNT_LIKELIHOODS = ('poisson_log', 'neg_binomial_2_log')
REGRESSION_HEADER = 8   # doubles before X in a regression target's parameter block


def count_constant(y, phi=None):
    """c_data = sum_m c_m, the data-only constants of the count likelihoods:
      poisson_log         c_m = -lgamma(y_m + 1)
      neg_binomial_2_log  c_m = lgamma(y_m + phi) - lgamma(phi) - y_m log(phi) - lgamma(y_m + 1)
    The negative binomial's first three terms are log prod_{j<y} (1 + j / phi) =
    sum_{j<y} log1p(j / phi): a sum of non-negative terms, taken as it stands up to
    y = 4096 (the lgamma differences lose it as phi grows: each is ~phi log phi at
    phi = 1e6).  Above that, Stirling's series for both lgamma with the leading terms
    cancelled in closed form: with t = y / phi,
      phi ((1 + t) log1p(t) - t) - log1p(t) / 2 + s(phi + y) - s(phi),
      s(z) = 1/(12 z) - 1/(360 z^3) + 1/(1260 z^5) - 1/(1680 z^7)
    (z >= 32: next term below 1e-16; a smaller phi climbs there with y by the
    product's first factors), (1 + t) log1p(t) - t by its series t^2/2 - t^3/6 + ...
    below t = 0.1.  Each distinct y is evaluated once and the sum over m is math.fsum."""
    import math
    y = np.asarray(y, dtype=np.float64)
    vals, counts = np.unique(y, return_counts=True)

    def stirling_tail(z):
        t = 1.0 / z
        t2 = t * t
        return t * (1.0 / 12 + t2 * (-1.0 / 360 + t2 * (1.0 / 1260 + t2 * (-1.0 / 1680))))

    def rising(yv):                  # lgamma(y + phi) - lgamma(phi) - y log(phi)
        if yv <= 4096:
            return math.fsum(np.log1p(np.arange(int(yv)) / phi).tolist())
        head, f, k = [], phi, 0
        while f < 32.0:              # the factors (1 + j / phi) below phi + j = 32
            head.append(math.log1p(k / phi))
            f += 1.0
            k += 1
        # the rest: prod_{k <= j < y} (1 + j / phi) = Gamma(phi + y) / Gamma(f) / phi^(y - k)
        n = yv - k
        t = n / f
        if t < 0.1:
            q, tk, i = 0.0, t * t, 2
            while True:
                term = tk / (i * (i - 1))
                q += term if i % 2 == 0 else -term
                if term <= 1e-20 * abs(q):
                    break
                tk *= t
                i += 1
        else:
            q = (1.0 + t) * math.log1p(t) - t
        body = f * q - 0.5 * math.log1p(t) + (stirling_tail(f + n) - stirling_tail(f))
        # Gamma(f + n) / Gamma(f) / f^n, then f^n / phi^n
        return math.fsum(head + [body, n * math.log1p(k / phi)])

    terms = []
    for v, c in zip(vals.tolist(), counts.tolist()):
        cm = -math.lgamma(v + 1.0)
        if phi is not None and v > 0:
            cm = math.fsum([rising(v), cm])
        terms += [cm] * c
    return math.fsum(terms)


DISPERSION_TABLE_MAX = 65536   # largest count y that regression(..., learn_phi=True) takes


def dispersion_table(y):
    """(T, c_data) of the negative binomial with a learned dispersion.  The data term
    sum_m sum_{j < y_m} log1p(j / phi) of count_constant then depends on the coordinate
    log phi, so the device forms it per sample row from
      T[j] = #{m : y_m > j},  j = 0 .. J - 1,  J = max y
    (sum_m sum_{j<y_m} f(j) = sum_j T[j] f(j); f(0) = 0, so the device's sum starts at j = 1;
    J = 0 gives an empty table), and c_data keeps only sum_m -lgamma(y_m + 1), each distinct
    y evaluated once and the sum over m by math.fsum, as count_constant does."""
    import math
    y = np.asarray(y, dtype=np.float64)
    vals, counts = np.unique(y, return_counts=True)
    jmax = int(vals[-1]) if vals.size else 0
    above = np.zeros(jmax + 1)                 # above[v] = #{m : y_m == v}
    above[vals.astype(np.int64)] = counts
    # T[j] = #{y > j} = M - #{y <= j}
    table = (y.size - np.cumsum(above))[:jmax].astype(np.float64)
    terms = []
    for v, c in zip(vals.tolist(), counts.tolist()):
        terms += [-math.lgamma(v + 1.0)] * c
    return table, math.fsum(terms)


def _check_counts(likelihood, y, offset, phi, m, learn_phi=False):
    """Validation shared by regression and multilevel_regression for the count
    likelihoods' arguments; returns the offset as a float64 (M,) array (or None)."""
    count = likelihood in _COUNT_LIKELIHOODS
    if not count:
        if offset is not None:
            raise ValueError('offset is taken by the poisson_log and neg_binomial_2_log '
                             'likelihoods only, not by %r' % (likelihood,))
        if phi is not None:
            raise ValueError('phi is taken by the neg_binomial_2_log likelihood only, not by %r'
                             % (likelihood,))
        return None
    if likelihood == 'neg_binomial_2_log' and learn_phi:
        if phi is not None:
            raise ValueError('learn_phi=True learns the dispersion: phi must be None, got %r'
                             % (phi,))
    elif likelihood == 'neg_binomial_2_log':
        if phi is None or not (np.isfinite(phi) and phi > 0):
            raise ValueError('the neg_binomial_2_log likelihood needs a finite phi > 0')
    elif phi is not None:
        raise ValueError('phi is taken by the neg_binomial_2_log likelihood only, not by %r'
                         % (likelihood,))
    if not np.all((y >= 0) & (y == np.floor(y))):
        raise ValueError('the %s likelihood needs non-negative integer y' % likelihood)
    if np.any(y > 2.0 ** 53):
        raise ValueError('the %s likelihood needs y <= 2^53' % likelihood)
    if offset is None:
        return np.zeros(m)
    offset = np.asarray(offset, dtype=np.float64)
    if offset.shape != (m,):
        raise ValueError('offset must have shape (%d,), got %s' % (m, offset.shape))
    if not np.all(np.isfinite(offset)):
        raise ValueError('offset must be finite')
    return offset


def _check_likelihood(likelihood):
    if likelihood not in _LIKELIHOODS:
        raise ValueError('unknown likelihood %r (expected one of %s)'
                         % (likelihood, ', '.join(sorted(_LIKELIHOODS))))


def _check_design_shape(x, y, dims):
    """The shape checks shared by regression and multilevel_regression (dims: how the
    message names x's shape); returns x and y as float64 arrays."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError('x must be a non-empty %s matrix, got shape %s' % (dims, x.shape))
    if y.shape != (x.shape[0],):
        raise ValueError('y must have shape (%d,), got %s' % (x.shape[0], y.shape))
    return x, y


def _check_design(x, y, likelihood, df, scale, prior_scale, tau_scale=None, learn_scale=False):
    """The value checks shared by regression and multilevel_regression, after the shape
    checks (and, in the multilevel target, the group checks between the two); tau_scale
    is the multilevel target's, learn_scale says that `scale` is not used.  Returns whether
    the likelihood is a count likelihood."""
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError('x and y must be finite')
    if not (np.isfinite(prior_scale) and prior_scale > 0):
        raise ValueError('prior_scale must be positive')
    if tau_scale is not None and not (np.isfinite(tau_scale) and tau_scale > 0):
        raise ValueError('tau_scale must be positive')
    if likelihood == 'student_t':
        if df is None or not (np.isfinite(df) and df > 0):
            raise ValueError('the student_t likelihood needs df > 0')
    if likelihood in ('gaussian', 'student_t'):
        if not learn_scale and not (np.isfinite(scale) and scale > 0):
            raise ValueError('scale must be positive')
    elif likelihood == 'bernoulli_logit' and not np.all((y == 0) | (y == 1)):
        raise ValueError('the bernoulli_logit likelihood needs y in {0, 1}')
    return likelihood in _COUNT_LIKELIHOODS


def _fill_link_params(params, likelihood, m, df, phi, scale, prior_scale):
    """params[0..4] of a regression or multilevel block (include/viabel_amd.h); phi / scale
    None: learned, the slot stays 0."""
    params[0] = _LIKELIHOODS[likelihood]
    params[1] = m
    if likelihood == 'student_t':
        params[2] = df
    elif likelihood == 'neg_binomial_2_log' and phi is not None:
        params[2] = phi
    if likelihood in ('gaussian', 'student_t') and scale is not None:
        params[3] = scale
    params[4] = prior_scale


def regression(x, y, likelihood='student_t', df=None, scale=1.0, prior_scale=10.0, offset=None,
               phi=None, learn_scale=False, learn_phi=False, hyper_scale=5.0):
    """A generalised linear model evaluated on the device: beta_d ~ N(0,
    prior_scale^2) independently and, with eta_m = x_m . beta,
      gaussian         y_m ~ N(eta_m, scale^2)
      student_t        y_m ~ t_df(eta_m, scale)
      bernoulli_logit  y_m ~ Bernoulli(logistic(eta_m)), y_m in {0, 1}
    or, for counts y_m with eta_m = x_m . beta + offset_m (offset = log exposure,
    default 0),
      poisson_log         y_m ~ Poisson(exp(eta_m))
      neg_binomial_2_log  y_m ~ NB(mean mu = exp(eta_m), variance mu + mu^2 / phi), phi
                          fixed
    with every normalising constant kept.  x is (M, D), y is (M,).  The data are
    packed once into one parameter array (layout in include/viabel_amd.h) that
    the library uploads per run, so no host call happens inside a fit.

    Learned scale or dispersion.  learn_scale=True (gaussian, student_t; `scale` is then
    not used) or learn_phi=True (neg_binomial_2_log; `phi` must then be None) makes the
    parameter a coordinate: with x of shape (M, p) the target has dim = p + 1 and its
    coordinate vector is [beta (p), lambda], the last coordinate being the log: lambda =
    log sigma, or lambda = log phi, with e^lambda ~ half-Cauchy(0, hyper_scale) and the
    Jacobian of the log kept.  Such a target carries n_coef = p and learned = 'scale' or
    'phi'; learn_phi needs max(y) <= 65536."""
    _check_likelihood(likelihood)
    if learn_scale and likelihood not in ('gaussian', 'student_t'):
        raise ValueError('learn_scale=True is valid for the gaussian and student_t likelihoods '
                         'only, not for %r' % (likelihood,))
    if learn_phi and likelihood != 'neg_binomial_2_log':
        raise ValueError('learn_phi=True is valid for the neg_binomial_2_log likelihood only, '
                         'not for %r' % (likelihood,))
    learn = bool(learn_scale or learn_phi)
    if learn and not (np.isfinite(hyper_scale) and hyper_scale > 0):
        raise ValueError('hyper_scale must be positive')
    x, y = _check_design_shape(x, y, '(M, D)')
    count = _check_design(x, y, likelihood, df, scale, prior_scale, learn_scale=learn_scale)
    m, d = x.shape
    offset = _check_counts(likelihood, y, offset, phi, m, learn_phi)
    table = None
    if learn_phi:
        if np.any(y > DISPERSION_TABLE_MAX):
            raise ValueError('learn_phi=True needs max(y) <= %d, got %g: use the fixed-phi target '
                             '(negative_binomial_regression(x, y, phi)) for larger counts'
                             % (DISPERSION_TABLE_MAX, float(np.max(y))))
        table, c_data = dispersion_table(y)
    h = REGRESSION_HEADER
    params = np.zeros(h + m * d + m + (m + 1 if count else 0)
                      + (1 + table.size if table is not None else 0))
    _fill_link_params(params, likelihood, m, df, phi, None if learn_scale else scale, prior_scale)
    if learn:
        params[5] = 1.0
        params[6] = hyper_scale
    params[h:h + m * d] = x.ravel()
    params[h + m * d:h + m * d + m] = y
    if count:
        e = h + m * d + 2 * m
        params[h + m * d + m:e] = offset
        if learn_phi:
            params[e] = c_data
            params[e + 1] = table.size
            params[e + 2:] = table
        else:
            params[e] = count_constant(y, phi)
    t = Target(nat.TARGET_REGRESSION, d + 1 if learn else d, 'regression', params)
    t.likelihood = likelihood
    t.n_obs = m
    if learn:
        t.n_coef = d
        t.learned = 'scale' if learn_scale else 'phi'
    return t


def linear_regression(x, y, prior_scale=10.0, hyper_scale=5.0):
    """Bayesian linear regression with unknown noise: y ~ normal(x beta, sigma), beta ~
    normal(0, prior_scale), sigma ~ half-Cauchy(0, hyper_scale).  The coordinates are
    [beta (p), log sigma]: the last one is the log."""
    return regression(x, y, 'gaussian', prior_scale=prior_scale, learn_scale=True,
                      hyper_scale=hyper_scale)


def robust_regression(x, y, df, scale=1.0, prior_scale=10.0, learn_scale=False, hyper_scale=5.0):
    """The reference's robust-regression model: y ~ student_t(df, x beta, scale),
    beta ~ normal(0, prior_scale).  learn_scale=True: scale ~ half-Cauchy(0, hyper_scale) is
    learned, the coordinates are [beta (p), log scale] (the last one is the log) and the
    `scale` argument is not used."""
    return regression(x, y, 'student_t', df=df, scale=scale, prior_scale=prior_scale,
                      learn_scale=learn_scale, hyper_scale=hyper_scale)


def logistic_regression(x, y, prior_scale=10.0):
    """y ~ bernoulli_logit(x beta), beta ~ normal(0, prior_scale)."""
    return regression(x, y, 'bernoulli_logit', prior_scale=prior_scale)


def poisson_regression(x, y, offset=None, prior_scale=10.0):
    """y ~ poisson_log(x beta + offset), beta ~ normal(0, prior_scale)."""
    return regression(x, y, 'poisson_log', prior_scale=prior_scale, offset=offset)


def negative_binomial_regression(x, y, phi=None, offset=None, prior_scale=10.0, learn_phi=False,
                                 hyper_scale=5.0):
    """y ~ neg_binomial_2_log(x beta + offset, phi), beta ~ normal(0, prior_scale).
    learn_phi=True (phi left None): phi ~ half-Cauchy(0, hyper_scale) is learned and the
    coordinates are [beta (p), log phi] (the last one is the log)."""
    if phi is None and not learn_phi:
        raise TypeError('negative_binomial_regression() needs phi, or learn_phi=True')
    return regression(x, y, 'neg_binomial_2_log', prior_scale=prior_scale, offset=offset, phi=phi,
                      learn_phi=learn_phi, hyper_scale=hyper_scale)


HIERARCHICAL_HEADER = 8   # doubles before y in a hierarchical target's parameter block
EIGHT_SCHOOLS_Y = (28., 8., -3., 7., -1., 1., 18., 12.)
EIGHT_SCHOOLS_SIGMA = (15., 10., 16., 11., 9., 11., 10., 18.)


def hierarchical_normal(y, sigma, centered=False, mu_scale=5.0, tau_scale=5.0):
    """Hierarchical normal means evaluated on the device: J groups with estimates
    y_j and standard errors sigma_j,
      mu ~ N(0, mu_scale^2), tau ~ half-Cauchy(0, tau_scale), y_j ~ N(theta_j, sigma_j^2)
      centred       theta_j ~ N(mu, tau^2),          x = [mu, log tau, theta (J)]
      non-centred   theta_j = mu + tau theta_tilde_j, theta_tilde_j ~ N(0, 1),
                                                     x = [mu, log tau, theta_tilde (J)]
    in Stan's log_prob convention (constants of the ~ statements dropped, the
    Jacobian of tau = exp(log tau) kept), so D = J + 2.  The data are packed once
    into one parameter array (layout in include/viabel_amd.h) that the library
    uploads per run, so no host call happens inside a fit."""
    y = np.asarray(y, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    if y.ndim != 1 or y.shape[0] < 1:
        raise ValueError('y must be a non-empty 1-D array, got shape %s' % (y.shape,))
    if sigma.shape != y.shape:
        raise ValueError('sigma must have shape %s, got %s' % (y.shape, sigma.shape))
    if not (np.all(np.isfinite(y)) and np.all(np.isfinite(sigma))):
        raise ValueError('y and sigma must be finite')
    if not np.all(sigma > 0):
        raise ValueError('sigma must be positive')
    if not (np.isfinite(mu_scale) and mu_scale > 0):
        raise ValueError('mu_scale must be positive')
    if not (np.isfinite(tau_scale) and tau_scale > 0):
        raise ValueError('tau_scale must be positive')
    j = y.shape[0]
    params = np.zeros(HIERARCHICAL_HEADER + 2 * j)
    params[0] = 1.0 if centered else 0.0
    params[1] = j
    params[2] = mu_scale
    params[3] = tau_scale
    params[HIERARCHICAL_HEADER:HIERARCHICAL_HEADER + j] = y
    params[HIERARCHICAL_HEADER + j:] = sigma
    t = Target(nat.TARGET_HIERARCHICAL, j + 2, 'hierarchical_normal', params)
    t.n_groups = j
    t.centered = bool(centered)
    return t


def eight_schools_cp():
    """eight_schools_cp.stan: the centred eight-schools model (D = 10)."""
    return hierarchical_normal(EIGHT_SCHOOLS_Y, EIGHT_SCHOOLS_SIGMA, centered=True)


MULTILEVEL_HEADER = 8   # doubles before X in a multilevel target's parameter block


def multilevel_regression(x, y, group, likelihood='gaussian', df=None, scale=1.0,
                          prior_scale=10.0, tau_scale=5.0, centered=False, n_groups=None,
                          offset=None, phi=None, learn_scale=False, learn_phi=False,
                          hyper_scale=5.0):
    """A regression whose intercept varies by group, evaluated on the device:
      beta_d ~ N(0, prior_scale^2), tau ~ half-Cauchy(0, tau_scale)
      centred       a_g ~ N(0, tau^2),               x = [beta (p), log tau, a (G)]
      non-centred   a_g = tau a_tilde_g, a_tilde_g ~ N(0, 1),
                                                     x = [beta (p), log tau, a_tilde (G)]
      eta_m = x_m . beta + a_group[m] (+ offset_m for the count likelihoods),
      y_m | eta_m as in `regression`
    with every normalising constant and the Jacobian of tau = exp(log tau) kept, so
    D = p + 1 + G.  x is (M, p), y is (M,), group is (M,) integer labels in 0 .. G - 1
    with G = n_groups, or max(group) + 1; a group without observations has its prior
    only.  The observations are sorted by group once (a stable sort, the permutation
    kept as `order`) and packed with the group offsets into one parameter array
    (layout in include/viabel_amd.h) that the library uploads per run, so no host call
    happens inside a fit.

    Learned scale or dispersion, as in `regression`.  learn_scale=True (gaussian, student_t;
    `scale` is then not used) or learn_phi=True (neg_binomial_2_log; `phi` must then be
    None) appends one coordinate: x = [beta (p), log tau, G more, lambda], D = p + 2 + G,
    lambda = log sigma or log phi with e^lambda ~ half-Cauchy(0, hyper_scale) and the
    Jacobian of the log kept.  Every other coordinate stays where it is.  Such a target
    carries learned = 'scale' or 'phi'; learn_phi needs max(y) <= 65536."""
    _check_likelihood(likelihood)
    if learn_scale and likelihood not in ('gaussian', 'student_t'):
        raise ValueError('learn_scale=True is valid for the gaussian and student_t likelihoods '
                         'only, not for %r' % (likelihood,))
    if learn_phi and likelihood != 'neg_binomial_2_log':
        raise ValueError('learn_phi=True is valid for the neg_binomial_2_log likelihood only, '
                         'not for %r' % (likelihood,))
    learn = bool(learn_scale or learn_phi)
    if learn and not (np.isfinite(hyper_scale) and hyper_scale > 0):
        raise ValueError('hyper_scale must be positive')
    x, y = _check_design_shape(x, y, '(M, p)')
    m, p = x.shape
    graw = np.asarray(group)
    if graw.shape != (m,):
        raise ValueError('group must have shape (%d,), got %s' % (m, graw.shape))
    if graw.dtype.kind not in 'iuf':
        raise ValueError('group must hold integer labels, got dtype %s' % graw.dtype)
    if graw.dtype.kind == 'f' and not (np.all(np.isfinite(graw)) and np.all(graw == np.floor(graw))):
        raise ValueError('group must hold integer labels')
    if np.any(graw < 0):
        raise ValueError('group labels must be >= 0')
    if np.any(graw >= 2 ** 31):
        raise ValueError('group labels must be below 2^31')
    g = graw.astype(np.int64)
    if n_groups is None:
        n_groups = int(g.max()) + 1
    elif not (isinstance(n_groups, (int, np.integer)) and n_groups >= 1):
        raise ValueError('n_groups must be an integer >= 1')
    n_groups = int(n_groups)
    if int(g.max()) >= n_groups:
        raise ValueError('group label %d is not below n_groups = %d' % (int(g.max()), n_groups))
    count = _check_design(x, y, likelihood, df, scale, prior_scale, tau_scale=tau_scale,
                          learn_scale=learn_scale)
    offset = _check_counts(likelihood, y, offset, phi, m, learn_phi)
    table = None
    if learn_phi:
        if np.any(y > DISPERSION_TABLE_MAX):
            raise ValueError('learn_phi=True needs max(y) <= %d, got %g: use the fixed-phi target '
                             '(multilevel_negative_binomial_regression(x, y, group, phi)) for '
                             'larger counts' % (DISPERSION_TABLE_MAX, float(np.max(y))))
        table, c_data = dispersion_table(y)
    order = np.argsort(g, kind='stable')
    offsets = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=n_groups))])
    h = MULTILEVEL_HEADER
    # a learned block appends s_aux and, for the dispersion, J and T [J]
    e = h + m * p + m + n_groups + 1
    fixed = e + (m + 1 if count else 0)
    params = np.zeros(fixed + (1 + (1 + table.size if table is not None else 0) if learn else 0))
    _fill_link_params(params, likelihood, m, df, phi, None if learn_scale else scale, prior_scale)
    params[5] = n_groups
    params[6] = tau_scale
    params[7] = (1.0 if centered else 0.0) + (2.0 if learn else 0.0)
    params[h:h + m * p] = x[order].ravel()
    params[h + m * p:h + m * p + m] = y[order]
    params[h + m * p + m:e] = offsets
    if count:
        params[e:e + m] = offset[order]
        params[fixed - 1] = c_data if learn_phi else count_constant(y, phi)
    if learn:
        params[fixed] = hyper_scale
        if learn_phi:
            params[fixed + 1] = table.size
            params[fixed + 2:] = table
    t = Target(nat.TARGET_MULTILEVEL, p + 1 + n_groups + (1 if learn else 0),
               'multilevel_regression', params)
    t.likelihood = likelihood
    t.n_obs = m
    t.n_groups = n_groups
    t.centered = bool(centered)
    t.order = order
    if learn:
        t.n_coef = p
        t.learned = 'scale' if learn_scale else 'phi'
    return t


def multilevel_linear_regression(x, y, group, prior_scale=10.0, tau_scale=5.0, hyper_scale=5.0,
                                 centered=False, n_groups=None):
    """The varying-intercept linear model with unknown noise (the radon model): y ~
    normal(x beta + a_group, sigma), sigma ~ half-Cauchy(0, hyper_scale):
    multilevel_regression with the gaussian likelihood and learn_scale=True.  The last
    coordinate is log sigma."""
    return multilevel_regression(x, y, group, 'gaussian', prior_scale=prior_scale,
                                 tau_scale=tau_scale, centered=centered, n_groups=n_groups,
                                 learn_scale=True, hyper_scale=hyper_scale)


def multilevel_logistic_regression(x, y, group, prior_scale=10.0, tau_scale=5.0, centered=False,
                                   n_groups=None):
    """Random-intercept logistic regression: multilevel_regression with the
    bernoulli_logit likelihood."""
    return multilevel_regression(x, y, group, 'bernoulli_logit', prior_scale=prior_scale,
                                 tau_scale=tau_scale, centered=centered, n_groups=n_groups)


def multilevel_robust_regression(x, y, group, df, scale=1.0, prior_scale=10.0, tau_scale=5.0,
                                 centered=False, n_groups=None, learn_scale=False,
                                 hyper_scale=5.0):
    """multilevel_regression with the student_t likelihood.  learn_scale=True: scale ~
    half-Cauchy(0, hyper_scale) is learned, the last coordinate is log scale and the `scale`
    argument is not used."""
    return multilevel_regression(x, y, group, 'student_t', df=df, scale=scale,
                                 prior_scale=prior_scale, tau_scale=tau_scale, centered=centered,
                                 n_groups=n_groups, learn_scale=learn_scale,
                                 hyper_scale=hyper_scale)


def multilevel_poisson_regression(x, y, group, offset=None, prior_scale=10.0, tau_scale=5.0,
                                  centered=False, n_groups=None):
    """Random-intercept Poisson regression: multilevel_regression with the poisson_log
    likelihood."""
    return multilevel_regression(x, y, group, 'poisson_log', prior_scale=prior_scale,
                                 tau_scale=tau_scale, centered=centered, n_groups=n_groups,
                                 offset=offset)


def multilevel_negative_binomial_regression(x, y, group, phi=None, offset=None, prior_scale=10.0,
                                            tau_scale=5.0, centered=False, n_groups=None,
                                            learn_phi=False, hyper_scale=5.0):
    """multilevel_regression with the neg_binomial_2_log likelihood.  learn_phi=True (phi
    left None): phi ~ half-Cauchy(0, hyper_scale) is learned and the last coordinate is
    log phi."""
    if phi is None and not learn_phi:
        raise TypeError('multilevel_negative_binomial_regression() needs phi, or learn_phi=True')
    return multilevel_regression(x, y, group, 'neg_binomial_2_log', prior_scale=prior_scale,
                                 tau_scale=tau_scale, centered=centered, n_groups=n_groups,
                                 offset=offset, phi=phi, learn_phi=learn_phi,
                                 hyper_scale=hyper_scale)


def callback(logdensity_and_grad, dim=None, name='callback'):
    """A user model: logdensity_and_grad(x) -> (log p (n,), d log p / dx (n, d)) for
    x of shape (n, dim) (numpy, host).  dim None: the dimension of the family
    the target is used with."""

    def _cb(user, xp, n, d, lpp, gp):
        try:
            x = np.ctypeslib.as_array(xp, shape=(n, d)).copy()
            lp, g = logdensity_and_grad(x)
            np.ctypeslib.as_array(lpp, shape=(n,))[:] = np.asarray(lp, dtype=float).reshape(n)
            np.ctypeslib.as_array(gp, shape=(n, d))[:] = np.asarray(g, dtype=float).reshape(n, d)
            return 0
        except BaseException as e:          # re-raised by _native.check after the call
            nat.PENDING_CALLBACK_ERRORS.append(e)
            return 1

    t = Target(nat.TARGET_CALLBACK, dim, name)
    t._cfunc = nat.TARGET_CALLBACK_T(_cb)
    t.fn = logdensity_and_grad
    return t


def from_stan(fitobj, dim=None):
    """make_stan_log_density (vb.py:314-321): log_prob / grad_log_prob of a fitted
    Stan model (pystan 2 fit object), applied row by row on the host."""
    def f(x):
        lp = np.array([fitobj.log_prob(row) for row in x])
        g = np.array([fitobj.grad_log_prob(row) for row in x])
        return lp, g
    return callback(f, dim, 'stan')


def torch_target(logdensity, dim=None, device=None):
    """A model written in torch: logdensity(x: tensor (n, dim)) -> (n,); the
    gradient comes from torch.autograd (on `device`, default the GPU when present)."""
    import torch
    dev = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))

    def f(x):
        xt = torch.tensor(x, dtype=torch.float64, device=dev, requires_grad=True)
        lp = logdensity(xt)
        g, = torch.autograd.grad(lp.sum(), xt)
        return lp.detach().cpu().numpy(), g.cpu().numpy()
    return callback(f, dim, 'torch')


def as_target(logdensity, dim):
    """The reference accepts any differentiable callable as logdensity
    (vb.py:236-241, 249-253).  A device target passes through; a plain callable
    that torch can differentiate (logdensity(x: tensor (n, dim)) -> tensor (n,)
    with a grad_fn) is wrapped with torch_target; anything else -- e.g. an
    autograd.numpy function, whose derivatives only autograd can take -- raises
    TypeError."""
    if isinstance(logdensity, Target):
        return logdensity
    msg = ('logdensity must be a viabel_amd.targets target, a user model wrapped with '
           'targets.callback / targets.from_stan, or a callable that torch can differentiate '
           '(x: tensor (n, dim) -> tensor (n,)); got %r' % (logdensity,))
    if not callable(logdensity) or dim is None:
        raise TypeError(msg)
    try:
        import torch
        dev = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        x = torch.zeros((2, int(dim)), dtype=torch.float64, device=dev, requires_grad=True)
        out = logdensity(x)
        ok = (isinstance(out, torch.Tensor) and out.requires_grad and tuple(out.shape) == (2,))
    except Exception as e:       # the probe failed: not a torch-differentiable callable
        raise TypeError(msg + ' (probe: %s: %s)' % (type(e).__name__, e)) from None
    if not ok:
        raise TypeError(msg)
    return torch_target(logdensity, int(dim))


class DeviceModel(Target):
    """A device model plugin as a target (see device_model)."""

    def __init__(self, image, dim, data, kernel, name):
        Target.__init__(self, nat.TARGET_PLUGIN, dim, name)
        self.image, self.kernel = image, kernel
        # a device tensor is used in place; anything else is packed as a host block
        self.data_device = nat.device_tensor(data) if data is not None else None
        if data is not None and self.data_device is None:
            self.params = nat.as_f64(np.ravel(np.asarray(data, dtype=np.float64)))
        # context -> loaded handle; shared by the copies bind() makes
        self._plugins = {}

    def plugin(self):
        """The handle loaded on the current context's device (loaded on first use)."""
        ctx = nat.context()
        p = self._plugins.get(id(ctx))
        if p is None or not p.usable_on(ctx):
            for k in [k for k, v in self._plugins.items() if not v.handle]:
                del self._plugins[k]      # released with their contexts (release_all)
            p = self._plugins[id(ctx)] = nat.Plugin(ctx, self.image, self.kernel)
        return p

    @property
    def launch(self):
        """(block, rows_per_block, dmax) as the loaded module reports it."""
        return self.plugin().info()

    def _struct(self):
        import ctypes
        user = ctypes.c_void_p(self.plugin().handle.value)
        cb = nat.TARGET_CALLBACK_T()
        if self.data_device is not None:
            d = self.data_device
            return nat.Target(self.kind, 0, self.dim, nat.dptr(d), d.numel(), cb, user)
        if self.params is None:
            return nat.Target(self.kind, 0, self.dim, None, 0, cb, user)
        return nat.Target(self.kind, 0, self.dim, nat.dptr(self.params), self.params.size, cb, user)


def device_model(code_object, dim=None, data=None, kernel='vb_model', name=None):
    """A user model evaluated on the device: `code_object` is a gfx950 code object (a
    path, or its bytes) exporting the kernel `kernel` and the launch record
    `kernel`_launch (include/viabel_amd.h, "Device model plugins"; write it with
    include/viabel_amd_model.h and build it with viabel_amd.plugin.compile).

    data   the model's block of doubles, passed to the kernel as (data, n_data): an array
           (uploaded per run) or a float64 device tensor (used in place), or None
    dim    the model's dimension; None: the dimension of the family it is used with

    The image is checked here (vb_plugin_check_image), so a file that is not a gfx950 code
    object with these symbols raises ValueError before any GPU call.  The module is loaded
    on first use, once per context, and released with it.  The library checks the image,
    the launch record and the dimension; it cannot check the kernel, which must write
    logp [n] and grad [n][D] and nothing else."""
    import os
    if isinstance(code_object, (bytes, bytearray, memoryview)):
        image = bytes(code_object)
    elif isinstance(code_object, (str, os.PathLike)):
        with open(os.fspath(code_object), 'rb') as f:
            image = f.read()
        if name is None:
            name = os.path.splitext(os.path.basename(os.fspath(code_object)))[0]
    else:
        raise TypeError('code_object must be a path or bytes, got %r' % (type(code_object),))
    if not isinstance(kernel, str):
        raise TypeError('kernel must be a string')
    if dim is not None and int(dim) < 1:
        raise ValueError('dim must be positive')
    nat.check_plugin_image(image, kernel)
    return DeviceModel(image, dim, data, kernel, name or 'device_model')


def robust_regression_block(x, y, df):
    """The data block of models/robust_regression.hip: [M, nu, X [M][D], y [M]]."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError('x must be a non-empty (M, D) matrix, got shape %s' % (x.shape,))
    if y.shape != (x.shape[0],):
        raise ValueError('y must have shape (%d,), got %s' % (x.shape[0], y.shape))
    if not (np.isfinite(df) and df > 0):
        raise ValueError('df must be positive')
    return np.concatenate([[float(x.shape[0]), float(df)], x.ravel(), y])


def example_model(name, *args, **kwargs):
    """The shipped example models (viabel_amd/models/*.hip) as device_model targets:
      example_model('robust_regression', x, y, df)   beta ~ normal(0, 10), y ~ student_t(df,
                                                     x beta, 1), Stan's constants dropped;
                                                     D = x.shape[1] <= 32
      example_model('banana', dim, scale=10.0, curvature=0.03)    a twisted Gaussian, dim >= 1
      example_model('isogauss_raw', dim)             N(0, I), the hand-written raw kernel"""
    from . import plugin
    if name == 'robust_regression':
        def pack(x, y, df):
            return int(np.shape(x)[1]), robust_regression_block(x, y, df)
        dim, data = pack(*args, **kwargs)
    elif name == 'banana':
        def pack(dim, scale=10.0, curvature=0.03):
            if not (np.isfinite(scale) and scale > 0):
                raise ValueError('scale must be positive')
            return int(dim), np.array([scale, curvature], dtype=np.float64)
        dim, data = pack(*args, **kwargs)
    elif name == 'isogauss_raw':
        def pack(dim):
            return int(dim), None
        dim, data = pack(*args, **kwargs)
    else:
        raise ValueError("unknown example model %r (expected 'robust_regression', 'banana' or "
                         "'isogauss_raw')" % (name,))
    return device_model(plugin.shipped(name), dim, data, name=name)
