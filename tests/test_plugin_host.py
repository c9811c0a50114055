"""Device model plugins without a GPU: the model header and the shipped models compile for
gfx950, their code objects (offload bundle and raw ELF) pass the image checker and carry the
launch records, and the checker -- through the C ABI, through targets.device_model, and
alone under the address / undefined-behaviour sanitizers -- refuses damaged input with a
message naming the fault."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import plugin_cases as pc
from tests.conftest import ROOT

HIPCC = '/opt/rocm/bin/hipcc'
INCLUDE = os.path.join(ROOT, 'include')
CSRC = os.path.join(ROOT, 'viabel_amd', 'csrc')
MODELS = ('robust_regression', 'banana', 'isogauss_raw')
BUNDLE_ID = b'hipv4-amdgcn-amd-amdhsa--gfx950'

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs the ROCm compiler')

KERNEL_ONLY = r'''
#include <hip/hip_runtime.h>
extern "C" __global__ void vb_model(const double* x, long long n, int D, const double* data,
                                    long long n_data, double* logp, double* grad) {
  const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
  if (r < n) logp[r] = 0.0;
}
'''
BAD_RECORD = KERNEL_ONLY + r'''
extern "C" __device__ __attribute__((used, visibility("default"))) const int vb_model_launch[3] = {
    100, 1, 0};
'''
HEADER_ONLY = '#include "viabel_amd_model.h"\n'


@pytest.fixture(scope='module')
def built(tmp_path_factory):
    """Every code object the tests use, compiled once through plugin.compile."""
    from viabel_amd import plugin
    d = tmp_path_factory.mktemp('plugin')
    out = {}
    for m in MODELS:
        src = os.path.join(ROOT, 'viabel_amd', 'models', m + '.hip')
        out[m, 'bundle'] = plugin.compile(src, str(d / (m + '.hsaco')))
        out[m, 'raw'] = plugin.compile(src, str(d / (m + '.raw.hsaco')), bundle=False)
    for name, text in (('kernel_only', KERNEL_ONLY), ('bad_record', BAD_RECORD),
                       ('header_only', HEADER_ONLY)):
        src = d / (name + '.hip')
        src.write_text(text)
        out[name] = plugin.compile(str(src), bundle=False)
    exe = d / 'x86'
    (d / 'x86.c').write_text('int main(){}\n')
    subprocess.check_call(['gcc', str(d / 'x86.c'), '-o', str(exe)])
    out['x86'] = str(exe)
    out['dir'] = d
    return out


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _check(image, kernel='vb_model'):
    """(status, message) of vb_plugin_check_image."""
    from viabel_amd import _native as nat
    rc = nat.lib().vb_plugin_check_image(image, len(image), kernel.encode())
    return rc, nat.lib().vb_last_error().decode() if rc else ''


def _bundle_entries(b):
    """[(position of the offset field, offset, size, id)] of an offload bundle."""
    assert b[:24] == b'__CLANG_OFFLOAD_BUNDLE__'
    n, = struct.unpack_from('<Q', b, 24)
    pos, out = 32, []
    for _ in range(n):
        off, size, idl = struct.unpack_from('<QQQ', b, pos)
        out.append((pos, off, size, b[pos + 24:pos + 24 + idl]))
        pos += 24 + idl
    return out


def _symbol_bytes(elf, name, count):
    """`count` bytes at the file offset of symbol `name` of an ELF64 image."""
    shoff, = struct.unpack_from('<Q', elf, 40)
    shentsize, shnum = struct.unpack_from('<HH', elf, 58)
    secs = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + i * shentsize) for i in range(shnum)]
    for s in secs:
        if s[1] != 2:        # SHT_SYMTAB
            continue
        strtab = secs[s[6]]
        for k in range(s[5] // 24):
            st_name, _, _, shndx, value, _ = struct.unpack_from('<IBBHQQ', elf, s[4] + 24 * k)
            end = elf.index(b'\0', strtab[4] + st_name)
            if elf[strtab[4] + st_name:end] == name:
                sec = secs[shndx]
                off = sec[4] + value - sec[3]
                return elf[off:off + count]
    raise KeyError(name)


def test_header_and_models_compile(built):
    for key, path in built.items():
        if key not in ('dir', 'x86'):
            assert os.path.getsize(path) > 0, key
    # a second call reuses an output newer than its source
    from viabel_amd import plugin
    path = built['banana', 'bundle']
    before = os.path.getmtime(path)
    assert plugin.compile(os.path.join(ROOT, 'viabel_amd', 'models', 'banana.hip'), path) == path
    assert os.path.getmtime(path) == before


def test_header_pulls_nothing_from_csrc():
    text = open(os.path.join(INCLUDE, 'viabel_amd_model.h')).read()
    includes = [ln for ln in text.splitlines() if ln.lstrip().startswith('#include')]
    assert includes == ['#include <hip/hip_runtime.h>']


def test_compile_failure_carries_the_compiler_message(built):
    from viabel_amd import plugin
    src = built['dir'] / 'broken.hip'
    src.write_text('#include "viabel_amd_model.h"\nthis is not HIP\n')
    with pytest.raises(RuntimeError, match='error'):
        plugin.compile(str(src))
    saved, plugin.HIPCC = plugin.HIPCC, str(built['dir'] / 'no_such_hipcc')
    try:
        with pytest.raises(RuntimeError, match='cannot run'):
            plugin.compile(str(src))
    finally:
        plugin.HIPCC = saved


@pytest.mark.parametrize('model', MODELS)
def test_bundle_and_raw_elf_pass_the_check(built, model):
    bundle, raw = _read(built[model, 'bundle']), _read(built[model, 'raw'])
    assert bundle[:24] == b'__CLANG_OFFLOAD_BUNDLE__' and raw[:4] == b'\x7fELF'
    assert BUNDLE_ID in [e[3] for e in _bundle_entries(bundle)]
    assert _check(bundle) == (0, '')
    assert _check(raw) == (0, '')
    # what the library's own build made, where it has
    assert _check(_read(pc.hsaco(model))) == (0, '')


@pytest.mark.parametrize('model', MODELS)
def test_elf_holds_the_launch_record(built, model):
    raw = _read(built[model, 'raw'])
    # e_machine 224 (AMDGPU), e_flags' machine byte 0x4f (gfx950)
    assert struct.unpack_from('<H', raw, 18)[0] == 224
    assert struct.unpack_from('<I', raw, 48)[0] & 0xff == 0x4f
    rec = struct.unpack('<3i', _symbol_bytes(raw, b'vb_model_launch', 12))
    assert rec == pc.LAUNCH[model]
    # and the gfx950 entry of the bundle is the same kind of object
    bundle = _read(built[model, 'bundle'])
    _, off, size, _ = [e for e in _bundle_entries(bundle) if e[3] == BUNDLE_ID][0]
    inner = bundle[off:off + size]
    assert struct.unpack('<3i', _symbol_bytes(inner, b'vb_model_launch', 12)) == pc.LAUNCH[model]


def _damaged(built):
    """name -> (image, kernel, a word the message must hold)"""
    raw = _read(built['banana', 'raw'])
    bundle = bytearray(_read(built['banana', 'bundle']))
    pos = [e for e in _bundle_entries(bytes(bundle)) if e[3] == BUNDLE_ID][0][0]
    struct.pack_into('<Q', bundle, pos, len(bundle) + 4096)
    cases = {
        'empty': (b'', 'vb_model', 'empty'),
        'three_bytes': (b'\x7fEL', 'vb_model', 'short'),
        'x86_elf': (_read(built['x86']), 'vb_model', 'e_machine'),
        'bundle_offset_past_end': (bytes(bundle), 'vb_model', 'outside'),
        'wrong_kernel_name': (raw, 'other_model', "'other_model'"),
        'no_launch_record': (_read(built['kernel_only']), 'vb_model', 'launch record'),
        'header_only': (_read(built['header_only']), 'vb_model', 'vb_model'),
        'bad_launch_record': (_read(built['bad_record']), 'vb_model', 'multiple of 64'),
    }
    for k in range(512, len(raw), 512):
        cases['truncated_at_%d' % k] = (raw[:k], 'vb_model', 'truncated')
    return cases


def test_checker_refuses_damaged_images(built):
    from viabel_amd import _native as nat
    cases = _damaged(built)
    assert sum(k.startswith('truncated') for k in cases) >= 5
    for name, (image, kernel, word) in cases.items():
        rc, msg = _check(image, kernel)
        assert rc == nat.VB_EINVAL, name
        assert word in msg and '\n' not in msg, (name, msg)
    # a truncated bundle as well
    bundle = _read(built['banana', 'bundle'])
    for k in range(512, len(bundle), 512):
        rc, msg = _check(bundle[:k])
        assert rc == nat.VB_EINVAL and msg, k


def test_device_model_refuses_before_any_gpu_call(built):
    from viabel_amd import targets
    for name, (image, kernel, word) in _damaged(built).items():
        with pytest.raises(ValueError) as e:
            targets.device_model(image, 2, kernel=kernel)
        assert word in str(e.value), name
    path = built['dir'] / 'damaged.hsaco'
    path.write_bytes(_read(built['banana', 'raw'])[:1024])
    with pytest.raises(ValueError, match='truncated'):
        targets.device_model(str(path), 2)
    for bad in (3, None, 2.5, ['x']):
        with pytest.raises(TypeError):
            targets.device_model(bad, 2)
    # good input: a target, with nothing loaded yet
    t = targets.device_model(built['banana', 'bundle'], 2)
    assert t.kind == 9 and t.dim == 2 and t._plugins == {}
    assert targets.example_model('robust_regression', [[1.0, 2.0]], [0.5], 4.0).params.tolist() == \
        [1.0, 4.0, 1.0, 2.0, 0.5]


def test_image_checker_alone_under_sanitizers(built):
    """tests/plugin_image_main.cc: its own main, only vb_plugin_image.hpp, run as its own
    process on the same good and damaged images."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = built['dir']
    exe = str(d / 'plugin_image_main')
    subprocess.check_call([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC,
                           os.path.join(ROOT, 'tests', 'plugin_image_main.cc'), '-o', exe])
    args = []
    for m in MODELS:
        for kind in ('bundle', 'raw'):
            args += ['ok', 'vb_model', built[m, kind], 'trunc', 'vb_model', built[m, kind]]
    for name, (image, kernel, _) in _damaged(built).items():
        if name.startswith('truncated'):
            continue
        path = d / (name + '.img')
        path.write_bytes(image)
        args += ['bad', kernel, str(path)]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = r.stdout.decode('utf-8', 'replace')
    assert r.returncode == 0, text
    assert 'FAIL' not in text and 'runtime error' not in text and 'AddressSanitizer' not in text, text
