"""Arguments and references for the accuracy tests of the device math helpers of
viabel_amd/csrc/vb_device.hpp (tests/test_gpu_device_math.py on the GPU through
vb_math_probe; tests/test_oracle_device_math.py pins the reference on the CPU).

Reference: numpy.longdouble (x87 extended, 64-bit mantissa: 2^-11 of a double ulp)
for exp, expm1, log, log1p, sqrt and the reciprocals; mpmath (40 digits) for sin /
cos of pi x.  Errors of the first group are in ulps of the double result (of the
subnormal spacing where the result is subnormal), those of sin / cos absolute in
units of 2^-53 (Box-Muller multiplies them by a radius).

Each helper gets a dense sweep of its documented domain plus its own seams:
range-reduction ties, polynomial / table cell edges, the clamps, subnormal
arguments or results.
"""
import functools

import numpy as np

LD = np.longdouble
SEED = 987
LN2 = float(np.log(2.0))
SQRT_HALF = float(np.sqrt(0.5))
EXP_MAX_ARG = float.fromhex('0x1.62e42fefa39efp+9')   # 709.78271289338397: the last finite exp


def longdouble_ok():
    return np.finfo(LD).nmant >= 63


def _rs(k):
    return np.random.RandomState(SEED + k)


def _logu(rs, lo, hi, n):
    """n log-uniform values in [lo, hi] (also across the subnormals)."""
    return np.exp(rs.uniform(np.log(LD(lo)), np.log(LD(hi)), size=n).astype(LD)).astype(np.float64)


def _steps(x, js):
    """x moved by j ulps for every j of js."""
    out = []
    for j in js:
        y = np.float64(x)
        for _ in range(abs(j)):
            y = np.nextafter(y, np.inf if j > 0 else -np.inf)
        out.append(y)
    return np.array(out)


def _around(x, n):
    return _steps(x, range(-n, n + 1))


def _finish(parts):
    x = np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in parts])
    x.setflags(write=False)
    return x


# ---- arguments --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def args(helper):
    rs = _rs(sorted(ARGS).index(helper))
    return _finish(ARGS[helper](rs))


def _exp(rs):
    parts = [rs.uniform(-745.2, 709.78, 1 << 17), _logu(rs, 1e-300, 700.0, 1 << 15),
             -_logu(rs, 1e-300, 700.0, 1 << 15),
             rs.uniform(-745.2, -708.0, 1 << 14),            # subnormal results
             _around(709.78, 8), _steps(EXP_MAX_ARG, range(-8, 1))]
    for k in (-1075, -1023, -1022, -1, 0, 1, 52, 53, 1023):  # reduction ties (k + 1/2) ln 2
        t = (k + 0.5) * LN2
        parts.append(np.concatenate([_steps(t, (0, 1, 2, 8)), _steps(t, (-1, -2, -8))]))
    x = np.concatenate(parts)
    return [x[(x >= -745.2) & (x <= EXP_MAX_ARG)]]


# (argument, documented result) of exp_fast outside the sweep: the clamps themselves,
# beyond them, signed zeros, infinities, NaN
EXP_SPECIAL = [(-746.0, 0.0), (710.0, np.inf), (-747.0, 0.0), (-1e4, 0.0), (-1e308, 0.0),
               (710.5, np.inf), (1e4, np.inf), (1e308, np.inf), (0.0, 1.0), (-0.0, 1.0),
               (np.inf, np.inf), (-np.inf, 0.0), (np.nan, np.nan)]


def _expm1(rs):
    return [rs.uniform(0.0, 700.0, 1 << 16), _logu(rs, 1e-300, 700.0, 1 << 16),
            rs.uniform(51.5 * LN2, 54.5 * LN2, 1 << 14),        # k = 52, 53, 54
            np.concatenate([_around((k + 0.5) * LN2, 8) for k in (0, 1, 52, 53, 54)]),
            [0.0, 700.0]]


def _log_seams(exps):
    """1 - j 2^-53 and 1 + j 2^-52 (j <= 64); mantissas within 64 ulp of sqrt(1/2) at
    the binary exponents `exps` (u = 2 m 2^E)."""
    j = np.arange(0, 65)
    parts = [1.0 - j * 2.0 ** -53, 1.0 + j * 2.0 ** -52]
    m = _around(SQRT_HALF, 64)
    for e in exps:
        parts.append(np.ldexp(m, e + 1))
    return parts


def _subnormals(rs, n):
    return np.concatenate([_logu(rs, 5e-324, 2.2e-308, n), [5e-324, 2.0 ** -1023, 2.2250738585072009e-308]])


def _log_unit(rs):
    return ([_logu(rs, 2.3e-308, 1.0, 1 << 17), _logu(rs, 1.0, 1.7e308, 1 << 15), _subnormals(rs, 1 << 10)]
            + _log_seams((-1022, -500, -1, 0, 500, 1023)))


def _log_unit_tab(rs):
    # every table cell edge: m = 1 + (i +- 1/2) / 64, +- 1 ulp
    i = np.arange(-19, 28)
    edges = np.concatenate([_around(1.0 + (k + s) / 64.0, 1) for k in i for s in (-0.5, 0.5)])
    return ([_logu(rs, 2.3e-308, 1.0, 1 << 17), _logu(rs, 1.0, 1.7e308, 1 << 15), _subnormals(rs, 1 << 10),
             edges, edges * 2.0 ** -37, edges * 2.0 ** 200]
            + _log_seams((-1022, -500, -1, 0)))


def _log_u01_tab(rs):
    # the uniforms the kernels feed it: (2 m + 1) 2^-53 of the normal pairs, (w + 1/2)
    # 2^-32 of the gamma proposals, (a + 1/2) 2^-40 of the Bailey draws; smallest and
    # largest of each
    m = rs.randint(0, 1 << 52, size=1 << 15, dtype=np.int64).astype(np.float64)
    forms = [(2.0 * m + 1.0) * 2.0 ** -53, [2.0 ** -53, 1.0 - 2.0 ** -53],
             (rs.randint(0, 1 << 32, size=1 << 13, dtype=np.int64) + 0.5) * 2.0 ** -32,
             [2.0 ** -33, 1.0 - 2.0 ** -33],
             (rs.randint(0, 1 << 40, size=1 << 13, dtype=np.int64) + 0.5) * 2.0 ** -40,
             [2.0 ** -41, 1.0 - 2.0 ** -41]]
    j = np.arange(1, 65)
    cells = np.concatenate([_around(0.5 + (k + s) / 256.0, 1) for k in range(0, 128) for s in (0.0, 0.5)])
    x = np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in
                        [_logu(rs, 2.3e-308, 1.0, 1 << 17), _subnormals(rs, 1 << 10), 1.0 - j * 2.0 ** -53,
                         cells, cells * 2.0 ** -20] + forms
                        + [np.ldexp(_around(SQRT_HALF, 64), e + 1) for e in (-1022, -500, -1)]])
    return [x[(x > 0.0) & (x < 1.0)]]


def _log1p(rs):
    j = np.arange(-64, 65)
    return [_logu(rs, 1e-320, 1e300, 1 << 17), rs.uniform(2.0 ** 52, 2.0 ** 54, 1 << 14),
            2.0 ** 53 + 2.0 * j, 2.0 ** 53 * (1.0 + j * 2.0 ** -40), _logu(rs, 1e-3, 1e3, 1 << 15),
            [0.0, 1e-320, 1e300]]


def _sqrt(rs):
    k = rs.randint(1, 1 << 26, size=1 << 14, dtype=np.int64).astype(np.float64)
    e = np.arange(-485, 486)
    # perfect squares: k^2, 4^e and k^2 4^e
    return [_logu(rs, 2.3e-308, 1.7e308, 1 << 17), k * k, np.ldexp(1.0, 2 * e),
            np.ldexp(k[:e.size] ** 2, 2 * e), _around(1.0, 8), [2.2250738585072014e-308, 1.7976931348623157e308]]


def _rcp(rs):
    x = _logu(rs, 2.0 ** -1020, 2.0 ** 1020, 1 << 17)
    return [x, -x[:1 << 12], _around(1.0, 8), _around(2.0, 8), rs.uniform(1.0, 2.0, 1 << 15)]


def _rsqrt(rs):
    return [_logu(rs, 2.3e-308, 1.7e308, 1 << 17), _around(1.0, 8), rs.uniform(1.0, 4.0, 1 << 15),
            [2.2250738585072014e-308, 1.7976931348623157e308]]


def _sincos(rs):
    # every octant edge and every table point q / 128 (+- 1 ulp), and a dense sweep;
    # 2^14 arguments at the most (the mpmath reference)
    q = np.arange(0, 257) / 128.0
    x = np.concatenate([q, np.nextafter(q, 3.0), np.nextafter(q, -1.0), (np.arange(0, 256) + 0.5) / 128.0,
                        np.nextafter((np.arange(0, 256) + 0.5) / 128.0, 3.0),
                        np.nextafter((np.arange(0, 256) + 0.5) / 128.0, -1.0),
                        rs.uniform(0.0, 2.0, 12000), _logu(rs, 1e-300, 1.0, 1024), [5e-324]])
    return [x[(x >= 0.0) & (x <= 2.0)]]


def _cos_u24(rs):
    # every b whose low half is at the rounding seam of q = (b + 0x8000) >> 16, and
    # random b; the argument travels as an integer-valued double
    hi = np.arange(0, 256, dtype=np.int64) << 16
    b = np.concatenate([hi | 0x7FFF, hi | 0x8000, hi | 0x8001, hi, hi | 0xFFFF,
                        rs.randint(0, 1 << 24, size=1 << 13, dtype=np.int64)])
    return [b.astype(np.float64)]


ARGS = {'exp_fast': _exp, 'expm1_pos': _expm1, 'log_unit': _log_unit, 'log_unit_tab': _log_unit_tab,
        'log_u01_tab': _log_u01_tab, 'log1p_pos_fast': _log1p, 'log1p_pos_tab': _log1p,
        'sqrt_pos': _sqrt, 'rcp_refined': _rcp, 'rsqrt_pos': _rsqrt,
        'sincospi_unit': _sincos, 'sincospi_tab': _sincos, 'cospi_tab_u24': _cos_u24}

# hand-written form -> (library form of the same probe, reference function)
LIBRARY = {'exp_fast': 'exp', 'expm1_pos': 'expm1', 'log_unit': 'log', 'log_unit_tab': 'log',
           'log_u01_tab': 'log', 'log1p_pos_fast': 'log1p', 'log1p_pos_tab': 'log1p',
           'sqrt_pos': 'sqrt', 'rcp_refined': 'rcp', 'rsqrt_pos': 'rsqrt',
           'sincospi_unit': 'sincospi', 'sincospi_tab': 'sincospi', 'cospi_tab_u24': 'sincospi'}
ULP_HELPERS = [h for h in ARGS if LIBRARY[h] != 'sincospi']
TRIG_HELPERS = [h for h in ARGS if LIBRARY[h] == 'sincospi']

LD_FUNCS = {'exp': np.exp, 'expm1': np.expm1, 'log': np.log, 'log1p': np.log1p, 'sqrt': np.sqrt,
            'rcp': lambda x: LD(1) / x, 'rsqrt': lambda x: LD(1) / np.sqrt(x)}


# ---- references -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_ld(helper):
    """The long-double reference of an ulp-measured helper at args(helper)."""
    with np.errstate(all='ignore'):
        r = LD_FUNCS[LIBRARY[helper]](args(helper).astype(LD))
    r.setflags(write=False)
    return r


def ulp_errors(got, ref):
    """|got - ref| in ulps of the double nearest ref (subnormal spacing for subnormal
    results)."""
    refd = ref.astype(np.float64)
    assert np.all(np.isfinite(refd)), 'argument set reaches a non-finite result'
    sp = np.spacing(np.abs(refd)).astype(LD)
    with np.errstate(invalid='ignore'):
        e = (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref) / sp).astype(np.float64)
    return np.where(np.isfinite(got), e, np.inf)


@functools.lru_cache(maxsize=None)
def trig_arguments(helper):
    """The argument x of sin(pi x) / cos(pi x) (cospi_tab_u24's b is x = b 2^-23)."""
    a = args(helper)
    return a * 2.0 ** -23 if helper == 'cospi_tab_u24' else a


@functools.lru_cache(maxsize=None)
def reference_trig(helper):
    """(sin(pi x), cos(pi x)) as double pairs ((hi, lo), (hi, lo)), mpmath 40 digits."""
    from mpmath import mp, mpf
    x = trig_arguments(helper)
    assert x.size <= 1 << 14
    out = np.empty((4, x.size))
    with mp.workdps(40):
        for k, v in enumerate(x):
            t = mp.pi * mpf(float(v))
            for c, f in ((0, mp.sin(t)), (2, mp.cos(t))):
                hi = float(f)
                out[c, k], out[c + 1, k] = hi, float(f - mpf(hi))
    out.setflags(write=False)
    return out


def trig_errors(got, hi, lo):
    """Absolute error in units of 2^-53."""
    e = np.abs((np.asarray(got, dtype=np.float64) - hi) - lo) * 2.0 ** 53
    return np.where(np.isfinite(got), e, np.inf)
