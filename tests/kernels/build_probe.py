"""TEST INFRASTRUCTURE: builds tests/kernels/stagei_probe.hip (single-kernel launchers around the UNCHANGED moshpp_amd/csrc/stagei.hip)
into a shared library, on demand:

  gpu: hipcc for gfx950 with the flags moshpp_amd/build.py compiles stagei.hip with (build.compile_flags);
  emu: g++ against tests/emu/fakehip with the defines tests/emu/build_chain_emu.py gives stagei.hip, linked with the fiber scheduler.

Outputs are cached under a name that carries a hash of the probe, stagei.hip, its headers and the flags."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from moshpp_amd import build as product_build  # noqa: E402
from tests.emu import build_chain_emu  # noqa: E402

PROBE = os.path.join(HERE, 'stagei_probe.hip')
STAGEI = os.path.join(product_build.CSRC, 'stagei.hip')
EMU = os.path.dirname(build_chain_emu.__file__)
DEPS = [PROBE, STAGEI, os.path.join(product_build.CSRC, 'stagei_views.h'), os.path.join(product_build.CSRC, 'stagei_plan.h'), os.path.join(product_build.CSRC, 'dev_mem.h'), os.path.join(ROOT, 'include', 'moshii.h')]
EMU_DEPS = [os.path.join(EMU, 'fakehip', 'hip', 'hip_runtime.h'), os.path.join(EMU, 'hip_emu_runtime.cpp')]


def _emu_defines():
    for src, extra, _cxx in build_chain_emu.UNITS:
        if os.path.basename(src) == 'stagei.hip':
            return list(extra)
    raise RuntimeError('tests/emu/build_chain_emu.py no longer builds stagei.hip')


def _commands(target, out):
    if target == 'gpu':
        return [[product_build._hipcc()] + product_build.compile_flags('stagei.hip') + ['-shared', PROBE, '-o', out]]
    if target == 'emu':
        inc = ['-I', os.path.join(EMU, 'fakehip'), '-I', os.path.join(ROOT, 'include'), '-I', EMU]
        obj_p, obj_r = out + '.probe.o', out + '.rt.o'
        return [['g++', '-O2', '-std=c++17', '-fPIC', '-w'] + inc + ['-x', 'c++', '-c', PROBE, '-o', obj_p] + _emu_defines(),
                ['g++', '-O2', '-std=c++17', '-fPIC', '-w'] + inc + ['-x', 'c++', '-c', EMU_DEPS[1], '-o', obj_r],
                ['g++', '-shared', '-fPIC', '-o', out, obj_p, obj_r]]
    raise ValueError(target)


def _hash(target):
    h = hashlib.sha256()
    for fn in DEPS + (EMU_DEPS if target == 'emu' else []):
        h.update(os.path.basename(fn).encode())
        with open(fn, 'rb') as fh:
            h.update(fh.read())
    h.update(repr(_commands(target, 'OUT')).encode())
    return h.hexdigest()[:16]


def build(target):
    """Path of the probe library for `target` ('gpu' or 'emu'), compiled if no cached build of these sources exists."""
    tag = _hash(target)
    out = os.path.join(HERE, f'_stagei_probe_{target}_{tag}.so')
    if os.path.exists(out):
        return out
    tmp = out + f'.{os.getpid()}.tmp'
    for cmd in _commands(target, tmp):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'probe build ({target}) failed: {" ".join(cmd)}\n{r.stdout}\n{r.stderr}')
    for leftover in (tmp + '.probe.o', tmp + '.rt.o'):
        if os.path.exists(leftover):
            os.remove(leftover)
    os.replace(tmp, out)
    for fn in os.listdir(HERE):     # stale builds of older sources
        if fn.startswith(f'_stagei_probe_{target}_') and fn.endswith('.so') and os.path.join(HERE, fn) != out:
            os.remove(os.path.join(HERE, fn))
    return out


if __name__ == '__main__':
    for t in sys.argv[1:] or ['emu', 'gpu']:
        print(build(t))
