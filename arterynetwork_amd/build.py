"""Build libvrg_hip.so (hipcc, gfx950 only) in-tree so that it travels with the repo snapshot.

The one recipe for the product library and for its diagnostic builds (-DVRG_CHAOS, -DVRG_FENCES, -DVRG_STAMPS, -DVRG_MUTANT):
every translation unit is compiled to an object, in parallel, then they are linked; the library appears under its name only
once it is complete, and a failed build leaves none behind.
    python -m arterynetwork_amd.build [--define VRG_CHAOS ...] [--out libvrg_hip_chaos.so]"""
from __future__ import annotations

import argparse
import glob
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(CSRC, 'libvrg_hip.so')
SOURCES = ['vrg_chain.hip', 'vrg_device.hip', 'vrg_init.hip', 'vrg_follow.hip', 'vmask_device.hip', 'vskel_device.hip', 'vrg_engine.cpp', 'vseg_device.hip', 'vves_device.hip', 'vter_device.hip', 'vgeo_device.hip', 'vbr_device.hip', 'vmor_device.hip', 'vcl_device.hip', 'vcomp_device.hip', 'vflow_device.hip', 'vden_device.hip', 'vbias_device.hip', 'vreg_device.hip', 'vbrain_device.hip', 'vwarp_device.hip', 'vbridge_device.hip', 'vtube_device.hip']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17']


def hipcc():
    return os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def jobs():
    """Compiles that run at once: at most 16, fewer when MAX_JOBS says so."""
    try:
        return max(1, min(16, int(os.environ.get('MAX_JOBS', 16))))
    except ValueError:
        return 16


def needs_build(out=LIB):
    if not os.path.exists(out):
        return True
    inputs = [f for ext in ('hip', 'cpp', 'h') for f in glob.glob(os.path.join(CSRC, '*.' + ext))]
    inputs += glob.glob(os.path.join(os.path.dirname(HERE), 'include', '*.h'))
    t = os.path.getmtime(out)
    return any(os.path.getmtime(f) > t for f in inputs)


def build(force=False, verbose=False, out=LIB, defines=()):
    """Compile SOURCES with -D<name> for every name in `defines` into `out` (a bare file name lands in csrc/); returns its path."""
    out = os.path.join(CSRC, out)
    if not force and not needs_build(out):
        return out
    flags = FLAGS + ['-D' + d for d in defines]
    tmp = out + '.tmp'

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)

    try:
        with tempfile.TemporaryDirectory() as objdir:
            def compile_one(src):
                obj = os.path.join(objdir, os.path.splitext(src)[0] + '.o')
                run([hipcc()] + flags + ['-fPIC', '-c', '-o', obj, src])
                return obj
            with ThreadPoolExecutor(min(jobs(), len(SOURCES))) as pool:
                objects = list(pool.map(compile_one, SOURCES))
            run([hipcc(), '-shared', '-o', tmp] + objects + ['-L/opt/rocm/lib', '-lrccl'])
        os.replace(tmp, out)
    except BaseException:
        for f in (out, tmp):            # (never a stale library with an older VrgCtx layout)
            if os.path.exists(f):
                os.remove(f)
        raise
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='Build libvrg_hip.so, or a diagnostic variant of it.')
    ap.add_argument('--define', action='append', default=[], metavar='NAME', help='compile with -DNAME (VRG_CHAOS, VRG_FENCES, VRG_STAMPS, VRG_MUTANT)')
    ap.add_argument('--out', default=LIB, help='the library to write (a bare file name lands in csrc/)')
    a = ap.parse_args()
    print(build(force=True, verbose=True, out=a.out, defines=a.define))
