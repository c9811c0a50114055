"""Compiles viabel_amd/csrc/vb_glm.hip for gfx950 with the compiler's resource remarks and
prints one line per kernel: name VGPRs AGPRs scratch-bytes/lane waves/SIMD LDS-bytes/block.

    python scripts/aux_resource_usage.py            # every kernel of the file
    python scripts/aux_resource_usage.py --check    # also compares the instances recorded in
        profiles/glm_regression/vb_glm_resource_usage.txt and
        profiles/count_regression/count_resource_usage.txt, and asks for 0 scratch everywhere

Needs hipcc only (a cross-compile; no GPU)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
RECORDED = ('profiles/glm_regression/vb_glm_resource_usage.txt',
            'profiles/count_regression/count_resource_usage.txt')
FIELDS = (('VGPRs', r'VGPRs: (\d+)'), ('AGPRs', r'AGPRs: (\d+)'),
          ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
          ('waves', r'Occupancy \[waves/SIMD\]: (\d+)'), ('LDS', r'LDS Size \[bytes/block\]: (\d+)'))


def remarks():
    src = os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_glm.hip')
    out = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
                          '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', src,
                          '-o', os.devnull], stderr=subprocess.PIPE, stdout=subprocess.PIPE,
                         universal_newlines=True, check=True).stderr
    table, name = {}, None
    for line in out.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            table[name] = {}
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m and name is not None:
                table[name][key] = int(m.group(1))
    return table


def recorded():
    rec = {}
    for rel in RECORDED:
        with open(os.path.join(ROOT, rel)) as f:
            for line in f:
                parts = line.split()
                if len(parts) == 6 and parts[0].startswith('_ZN3vbk') and 'glm_' in parts[0]:
                    rec[parts[0]] = tuple(int(v) for v in parts[1:])
    return rec


def main():
    table = remarks()
    for name, r in table.items():
        print(name, *(r[k] for k, _ in FIELDS))
    if '--check' not in sys.argv[1:]:
        return 0
    bad = [n for n, r in table.items() if r['scratch'] != 0]
    for name, want in recorded().items():
        got = tuple(table[name][k] for k, _ in FIELDS) if name in table else None
        if got != want:
            bad.append('%s: recorded %r, now %r' % (name, want, got))
    print('check: %d recorded instances compared, %s' % (len(recorded()), 'all equal, no scratch'
                                                         if not bad else 'DIFFERENCES'))
    for b in bad:
        print('  ', b)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
