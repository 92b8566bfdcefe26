"""Automatic 16-bit intensity storage (option storage16 = -1, the default).

The engine (vrg_engine.cpp) is shared by the product library and the sequential host model, so what the engine decides -
when the level-index volume is built, kept, rebuilt, and when the stored type stays - is checked on the CPU through the
host model and on the GPU through the product."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from arterynetwork_amd import phantoms
from arterynetwork_amd._capi import Session, VrgError, VrgLib

HM_DIR = os.path.join(ROOT, 'tests', 'hostmodel')
BACKENDS = ['hostmodel', pytest.param('gpu', marks=pytest.mark.gpu)]


@functools.lru_cache(maxsize=None)
def _lib(kind):
    if kind == 'gpu':
        from arterynetwork_amd._capi import product_lib
        return product_lib()
    subprocess.check_call(['make', '-C', HM_DIR, '-s', 'libvrg_hostmodel.so'])
    return VrgLib(os.path.join(HM_DIR, 'libvrg_hostmodel.so'), 'vrgm_')


@functools.lru_cache(maxsize=None)
def _bench_volume(levels=255):
    d, v = phantoms.bench_volume((256, 192, 96), seed=4, levels=levels)
    return d, v.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _scattered(excluded=True):
    """The 83x61x47 volume of test_skip_excluded_is_bit_identical: seeds and excluded voxels scattered, so that every group of
    four voxels is mixed; excluded = False: the same seeds with nothing excluded."""
    rng = np.random.default_rng(21)
    shape = (83, 61, 47)
    u = rng.random(shape)
    vm = np.full(shape, 3, dtype=np.uint8); vm[u < 0.03] = 0
    if excluded:
        vm[u > 0.55] = 4
    return rng.integers(0, 7, size=shape).astype(np.float64), vm


def _results(s):
    return (s.labels(), s.segmented(), s.band(0), s.band(1), s.trace().tobytes())


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for w in (2, 3):
        for x, y in zip(a[w], b[w]):
            assert np.array_equal(x, y)
    assert a[4] == b[4]                                      # the trace with its f64 intensity sums: bit-identical


def _run(lib, data, vmap, sweeps, options, H=2.25):
    s = Session(data.shape, lib=lib)
    for k, v in options.items():
        s.set_option(k, v)
    s.set_volume(data); s.set_labels(vmap); s.init(H)
    r = s.run(sweeps, 10 ** 9, None)
    assert r.sweeps > 0
    out = _results(s), s.stats()
    s.close()
    return out


@pytest.mark.parametrize('volume', ['brain_mask', 'scattered'])
@pytest.mark.parametrize('backend', BACKENDS)
def test_auto_engages_above_threshold(backend, volume):
    lib = _lib(backend)
    data, vmap = _bench_volume() if volume == 'brain_mask' else _scattered()
    sweeps = 12 if backend == 'gpu' or volume == 'scattered' else 4
    ref, st0 = _run(lib, data, vmap, sweeps, {'storage16': 0})
    got, st1 = _run(lib, data, vmap, sweeps, {'storage16': -1, 'narrow_above': 0})
    assert st0['dense_storage'].startswith('fp32') and st0['storage16_option'] == 0 and st0['storage16_auto'] is None
    assert st1['dense_storage'].startswith('u16') and st1['storage16_option'] == -1 and st1['storage16_auto'] is True
    assert st1['level_index_bytes'] > 0
    _same(ref, got)
    # default options: these volumes are far below the 300-MiB threshold - the fp32 pass still runs
    dflt, st2 = _run(lib, data, vmap, sweeps, {})
    assert st2['dense_storage'].startswith('fp32') and st2['storage16_option'] == -1 and st2['storage16_auto'] is False
    if backend == 'gpu':
        assert st2['dense_kernel'].startswith('k_recount_pipe<3,') and st1['dense_kernel'].startswith('k_recount_bits<3,')
    _same(ref, dflt)


@pytest.mark.parametrize('backend', BACKENDS)
def test_auto_falls_back_on_continuous_values(backend):
    """More than 16384 distinct values: the automatic mode keeps the stored type, silently; storage16 = 1 still fails loudly."""
    lib = _lib(backend)
    data, vmap = phantoms.config1()
    sweeps = 10 if backend == 'gpu' else 3
    ref, st0 = _run(lib, data, vmap, sweeps, {'storage16': 0})
    got, st1 = _run(lib, data, vmap, sweeps, {'storage16': -1, 'narrow_above': 0})
    assert st1['dense_storage'] == st0['dense_storage'] and not st1['dense_storage'].startswith('u16')
    assert st1['storage16_auto'] is False
    _same(ref, got)
    s = Session(data.shape, lib=lib)
    s.set_option('storage16', 1)
    s.set_volume(data); s.set_labels(vmap)
    with pytest.raises(VrgError):
        s.init(2.25)
    s.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_index_volume_follows_the_volume(backend):
    """One handle: a re-init after set_labels reuses the level-index volume (same results); set_volume with other data of the
    same shape rebuilds it (results of a fresh handle, not of stale indices)."""
    lib = _lib(backend)
    data, vmap = _scattered()
    other = np.random.default_rng(5).integers(0, 9, size=data.shape).astype(np.float64)
    assert not np.array_equal(other, data)
    opts = {'storage16': -1, 'narrow_above': 0}
    sweeps = 8
    fresh_a, _ = _run(lib, data, vmap, sweeps, opts)
    fresh_b, _ = _run(lib, other, vmap, sweeps, opts)
    assert fresh_a[4] != fresh_b[4]                          # (the two volumes do give different runs)
    s = Session(data.shape, lib=lib)
    for k, v in opts.items():
        s.set_option(k, v)
    s.set_volume(data); s.set_labels(vmap); s.init(2.25); s.run(sweeps, 10 ** 9, None)
    _same(fresh_a, _results(s))
    st = s.stats()
    bytes0 = st['level_index_bytes']
    assert bytes0 > 0 and st['level_index_builds'] == 1
    s.set_labels(vmap); s.init(2.25); s.run(sweeps, 10 ** 9, None)
    st = s.stats()
    assert st['dense_storage'].startswith('u16') and st['level_index_bytes'] == bytes0
    assert st['level_index_builds'] == 1                     # reused, not rebuilt
    _same(fresh_a, _results(s))
    s.set_volume(other); s.set_labels(vmap); s.init(2.25); s.run(sweeps, 10 ** 9, None)
    st = s.stats()
    assert st['dense_storage'].startswith('u16') and st['level_index_builds'] == 2
    _same(fresh_b, _results(s))
    # an init that does not use the index volume gives its memory back
    s.set_option('storage16', 0)
    s.set_labels(vmap); s.init(2.25); s.run(sweeps, 10 ** 9, None)
    st = s.stats()
    assert st['dense_storage'].startswith('fp32') and st['level_index_bytes'] == 0
    _same(fresh_b, _results(s))
    s.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_auto_falls_back_when_the_index_volume_cannot_be_allocated(backend):
    """Option narrow_alloc_fault (tests only) makes the 2 B/voxel allocation fail: the automatic mode keeps the stored type, the
    init succeeds and leaves no error message behind; storage16 = 1 reports the failure."""
    lib = _lib(backend)
    data, vmap = _scattered()
    ref, _ = _run(lib, data, vmap, 8, {'storage16': 0})
    s = Session(data.shape, lib=lib)
    s.set_option('storage16', -1); s.set_option('narrow_above', 0); s.set_option('narrow_alloc_fault', 1)
    s.set_volume(data); s.set_labels(vmap); s.init(2.25)
    assert s.lib.last_error(s._h) == b''
    s.run(8, 10 ** 9, None)
    st = s.stats()
    assert st['dense_storage'].startswith('fp32') and st['storage16_auto'] is False and st['level_index_bytes'] == 0
    _same(ref, _results(s))
    s.set_option('storage16', 1)
    s.set_labels(vmap)
    with pytest.raises(VrgError):
        s.init(2.25)
    s.close()


@pytest.mark.gpu
def test_default_equals_fp32_storage_above_the_threshold():
    """512x512x300: the padded volume stores 316 MiB of fp32 intensities - above narrow_above, so the default chooses 16-bit
    storage.  Non-temporal loads are switched on for both runs (by itself the pass takes them above 300 MB fetched; the kernels
    are the ones a 880x880x640 volume runs).  storage16 = 0 against the default: labels, `segmented`, both bands and the trace
    with its f64 sums, bit for bit."""
    shape = (512, 512, 300)
    assert (shape[0] + 2 + 15) // 16 * 16 * (shape[1] + 4) * (shape[2] + 4) * 4 > 300 << 20
    data, vmap = phantoms.bench_volume(shape, seed=5)
    vmap = vmap.astype(np.uint8)
    (ref, st0), (got, st1) = [_run(_lib('gpu'), data, vmap, 40, dict(opts, nt_loads=1, batch=32)) for opts in ({'storage16': 0}, {})]
    assert st0['dense_storage'].startswith('fp32') and st0['dense_kernel'].startswith('k_recount_pipe<3,true')
    assert st1['dense_storage'].startswith('u16') and st1['storage16_option'] == -1 and st1['storage16_auto'] is True
    assert st1['dense_kernel'].startswith('k_recount_bits<3,true,3,')
    assert len(ref[1]) > 0
    _same(ref, got)
