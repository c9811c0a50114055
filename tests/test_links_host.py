"""The host part of viabel_amd/csrc/vb_links.hpp (the one definition of the regression
likelihoods' constants), through the stand-alone program tests/links_main.cc built by the
host C++ compiler with no HIP, plain and under AddressSanitizer + UndefinedBehaviorSanitizer
(run as its own process):

  lgamma_half_step(x) = lgamma(x + 1/2) - lgamma(x) - log(x) / 2 against 50-digit mpmath on
  both sides of its branches at x = 1 and x = 32.  The bar is the one the multiprecision
  tests hold the Student-t constant to: c_obs = lgamma_half_step(nu / 2) - log(2 pi) / 2
  (sigma = 1) enters the condition sum of log p as M |c_obs| (tests/aux_mp.py), and
  tests/test_oracle_aux_mp.py allows 2 AUX_ORACLE_ERR['student_t'] = 7.88 units of 2^-53 S,
  the tightest of the regression restatements' bars; so |error| <= 7.88 x 2^-53 |c_obs|.
  |c_obs| <= 1.32 over these x, which makes it 10.4 x 2^-53 absolute at most, the function's
  "a few 2^-53 absolute".  Measured (the formula is the one vb_glm.hip and vb_mlm.hip each
  carried): 3.40 at x = 1, 1.70 at 1.5, 0.53 at 31.5, 0.43 at 0.25, below 0.05 elsewhere.

  link_consts(lik, nu, sigma, phi) for each of the five likelihoods: k0 .. k3 and c_obs
  equal, bit for bit, the formulas that launch_glm_rows and launch_mlm_rows carried, written
  here in Python floats in the same operation order (math.log and math.log1p are the C
  library's).  nu >= 2 in these cases: below it lgamma_half_step calls the C library's
  lgamma, which math.lgamma does not wrap.

CPU only."""
import math
import os
import shutil
import struct
import subprocess

import pytest

from tests import aux_mp as am
from tests import glm_cases as gc
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'viabel_amd', 'csrc')
LOG2PI = 1.8378770664093454835606594728112

# the small-x branch; just below, at and just above x = 1; just below and at the series
# threshold x = 32; large; very large
XS = (0.25, 0.999, 1.0, 1.5, 31.5, 32.0, 5e5, 1e15)
# (lik, nu, sigma, phi): every likelihood, student_t on both sides of nu / 2 = 32
CONSTS = ((0, 0.0, 0.7, 0.0), (0, 0.0, 1e3, 0.0), (1, 5.0, 0.7, 0.0), (1, 2.0, 1.0, 0.0),
          (1, 63.0, 2.5, 0.0), (1, 64.0, 1.0, 0.0), (1, 1e6, 1e3, 0.0), (2, 0.0, 0.0, 0.0),
          (3, 0.0, 0.0, 0.0), (4, 0.0, 0.0, 3.0), (4, 0.0, 0.0, 1e-3))


def _hex(v):
    return '%016x' % struct.unpack('<Q', struct.pack('<d', v))[0]


def _val(w):
    return struct.unpack('<d', struct.pack('<Q', int(w, 16)))[0]


def _expected_consts(lik, nu, sigma, phi):
    """(k0, k1, k2, k3, c_obs) as the launchers formed them before vb_links.hpp."""
    k0 = k1 = k2 = k3 = c_obs = 0.0
    if lik == 0:
        k0 = 1.0 / (sigma * sigma)
        c_obs = -0.5 * LOG2PI - math.log(sigma)
    elif lik == 1:
        k3 = nu * (sigma * sigma)
        k0 = 1.0 / k3
        k1 = 0.5 * (nu + 1.0)
        k2 = nu + 1.0
        c_obs = gc.lgamma_half_step(0.5 * nu) - 0.5 * LOG2PI - math.log(sigma)
    elif lik == 4:
        k0 = phi
        k1 = math.log(phi)
    return k0, k1, k2, k3, c_obs


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """{'plain' / 'sanitized': CompletedProcess} of links_main over XS and CONSTS."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('links')
    args = []
    for x in XS:
        args += ['h', _hex(x)]
    for lik, nu, sigma, phi in CONSTS:
        args += ['c', str(lik), _hex(nu), _hex(sigma), _hex(phi)]
    out = {}
    for name, flags in (('plain', ['-O2']),
                        ('sanitized', ['-g', '-O1', '-fsanitize=address,undefined',
                                       '-fno-sanitize-recover=all'])):
        exe = str(d / ('links_main_' + name))
        subprocess.check_call([cxx, '-std=c++17', '-ffp-contract=off'] + flags +
                              ['-I', CSRC, os.path.join(ROOT, 'tests', 'links_main.cc'), '-o', exe])
        out[name] = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   text=True, timeout=120)
    return out


def _lines(run):
    assert run.returncode == 0, run.stderr[-3000:]
    lines = run.stdout.split('\n')[:-1]
    assert len(lines) == 1 + len(XS) + len(CONSTS)
    return lines


def test_sanitized_program_runs_clean_and_prints_the_same_bits(runs):
    r = runs['sanitized']
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    assert _lines(r) == _lines(runs['plain'])


def test_log_2_pi(runs):
    assert _lines(runs['plain'])[0] == _hex(LOG2PI)
    assert abs(LOG2PI - math.log(2 * math.pi)) <= 2.0 ** -52


@pytest.mark.skipif(not am.available(), reason='needs mpmath')
def test_lgamma_half_step_against_multiprecision(runs):
    from mpmath import mp, mpf
    bar = 2.0 * am.AUX_ORACLE_ERR['student_t']
    got = [_val(w) for w in _lines(runs['plain'])[1:1 + len(XS)]]
    with mp.workdps(am.DIGITS):
        for x, v in zip(XS, got):
            xm = mpf(x)
            ref = mp.loggamma(xm + mpf(1) / 2) - mp.loggamma(xm) - mp.log(xm) / 2
            c_obs = abs(ref - mp.log(2 * mp.pi) / 2)
            err = float(abs(mpf(v) - ref) / (mpf(am.UNIT) * c_obs))
            print('lgamma_half_step(%g) = %r: error %.3f x 2^-53 |c_obs|, |c_obs| %.4f'
                  % (x, v, err, float(c_obs)))
            assert err <= bar, (x, v, err)


@pytest.mark.parametrize('i', range(len(CONSTS)), ids=lambda i: 'lik%d-%d' % (CONSTS[i][0], i))
def test_link_consts_have_the_launchers_bits(runs, i):
    words = _lines(runs['plain'])[1 + len(XS) + i].split()
    want = [_hex(v) for v in _expected_consts(*CONSTS[i])]
    print(CONSTS[i], words, want)
    assert words == want
