"""Compile a device model plugin: HIP source -> gfx950 code object.

A model is a kernel with the contract of include/viabel_amd.h ("Device model plugins"),
usually one device function and a macro of include/viabel_amd_model.h:

    from viabel_amd import plugin, targets
    hsaco = plugin.compile('model.hip')
    target = targets.device_model(hsaco, dim=3, data=my_block)

The library does not compile at run time (no hiprtc): this calls the ROCm compiler
driver as a build step, with the flags the shipped models are built with.
"""
import os
import subprocess

HIPCC = os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
ARCH = 'gfx950'
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'models')


def compile(source, out=None, include_dirs=(), bundle=True):   # noqa: A001 (the issue's name)
    """Compile `source` (a .hip file) to a gfx950 code object and return its path.

    out           output path (default: the source's path with the suffix .hsaco)
    include_dirs  further -I directories; the package's include/ is always there
    bundle        False: a raw ELF (--no-gpu-bundle-output) instead of an offload bundle

    No fast-math, as the library's own Makefile explains: PSIS and the estimators rely on
    IEEE inf / NaN semantics.  An output newer than its source (and than
    viabel_amd_model.h) is reused.  Raises RuntimeError with the compiler's stderr when
    the compilation fails, and when the compiler is absent."""
    source = os.fspath(source)
    if not os.path.isfile(source):
        raise FileNotFoundError(source)
    if out is None:
        out = os.path.splitext(source)[0] + '.hsaco'
    out = os.fspath(out)
    deps = [source, os.path.join(INCLUDE, 'viabel_amd_model.h')]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d)
                                   for d in deps if os.path.exists(d)):
        return out
    cmd = [HIPCC, '--genco', '--offload-arch=' + ARCH, '-O3', '-std=c++17', '-I', INCLUDE]
    for d in include_dirs:
        cmd += ['-I', os.fspath(d)]
    if not bundle:
        cmd.append('--no-gpu-bundle-output')
    cmd += [source, '-o', out]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except OSError as e:
        raise RuntimeError('viabel_amd.plugin.compile: cannot run %s: %s' % (HIPCC, e)) from None
    if r.returncode != 0:
        try:
            os.remove(out)
        except OSError:
            pass
        raise RuntimeError('viabel_amd.plugin.compile: %s failed (exit %d):\n%s'
                           % (' '.join(cmd), r.returncode, r.stderr.decode('utf-8', 'replace')))
    return out


def shipped(name):
    """Path of a shipped example model's code object (viabel_amd/models/NAME.hsaco),
    compiled from its source when the library's build has not made it."""
    src = os.path.join(MODELS, name + '.hip')
    if not os.path.isfile(src):
        raise ValueError('no shipped model %r (have: %s)' % (name, ', '.join(sorted(
            f[:-4] for f in os.listdir(MODELS) if f.endswith('.hip')))))
    return compile(src)
