"""Rigid and affine registration on the GPU: step 1 of the reference's Usage, "Register multiple sets of images if any".

The reference pipeline leaves this step to FSL ``flirt`` and holds no code for it.  Here it is a multi-resolution search over
6, 7, 9 or 12 parameters that minimises a cost of the joint histogram of the two images - correlation ratio by default, as in
``flirt``, or (normalised) mutual information - by a definition of our own: include/vmask.h ``vmask_reg_*``, DESIGN.md section 9
entry f16.  One cost evaluation - the moving volume sampled at every voxel of the fixed grid through the affine map, scattered
into the histogram - is one HIP kernel; the search, a deterministic pattern search, is host Python and takes its histogram
function as an argument (``registerWith``), which is how tests/registration_model.py replaces the GPU.  Agreement with FSL is
not claimed.  No CPU path.

Matrices.  ``W`` is 4 x 4 and takes WORLD coordinates of the moving image to WORLD coordinates of the fixed image, "world"
being what the NIfTI voxel -> world affines of ``nifti.loadVolume`` give.  The ``.mat`` file that ``main`` writes holds this
matrix as text.  It is NOT FSL's convention: a ``flirt`` matrix acts between scaled-millimetre voxel coordinates of the two
grids and cannot be exchanged with this one without both headers.

Volumes stay where they are given: tensors on the GPU are used in place and give tensors; host arrays are copied to the device
by every call of the single entries.  ``register`` (and so ``main``) converts and copies its host arrays once and keeps the
pyramid and the bin images on the device for its whole search.

Nonlinear registration (``registerNonlinear``, in ``fnirt``'s place) refines what the matrix leaves: a displacement field on the
fixed grid, a B-spline demons warp by a definition of our own - include/vmask.h ``vmask_warp_*``, DESIGN.md section 9 entry f18.
Per level of the pyramid one C entry iterates force pass, three-component B-spline fit and update on the device; the pyramid and
the levels are ``registerNonlinearWith``, host Python over operations that tests/warp_model.py restates in numpy.  A warp is
float64 ``[3, n0, n1, n2]``: component c is the displacement along axis c of the fixed grid, in fixed voxels.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
import types

import numpy as np

from . import bias as _B
from . import generateVesselVolume as _G
from ._capi import DTYPE_CODES
from .nifti import loadVolume, saveVolume
from .vesselness import BRAIN_FILE

COSTS = {'corratio': 0, 'mi': 1, 'nmi': 2}
DOFS = (6, 7, 9, 12)
SHRINK = np.array([[2.0, 0.0, 0.0, 0.5], [0.0, 2.0, 0.0, 0.5], [0.0, 0.0, 2.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
# the first steps of a level: translations (in voxels of the level), rotations (rad), scales, shears; the steps halve down to
# below 1 / FINE of these at the finest level and 1 / COARSE at the others, which the next level refines anyway
FIRST_STEPS = (2.0, 0.04, 0.02, 0.02)
FINE, COARSE = 32.0, 4.0
NEAREST_TYPES = (np.uint8, np.int16, np.int32, np.float32, np.float64)


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_reg_joint_hist, 'argtypes', None):
        p, i64, d, i = C.c_void_p, C.c_int64, C.c_double, C.c_int
        dll.vmask_reg_minmax.argtypes = [i, p, i, p, i64, i64, i64, p]
        dll.vmask_reg_quantise.argtypes = [i, p, i, p, i64, i64, i64, i, d, d, p, p]
        dll.vmask_reg_joint_hist.argtypes = [i, p, i64, i64, i64, p, i, i64, i64, i64, p, i, d, d, p]
        dll.vmask_reg_cost.argtypes = [p, i, i, d, i64, p]
        dll.vmask_reg_shrink.argtypes = [i, p, i, i64, i64, i64, p]
        dll.vmask_reg_resample.argtypes = [i, p, i, i64, i64, i64, p, i, d, p, i64, i64, i64]
        dll.vmask_reg_hold.argtypes = [i, p, i64, p]
        dll.vmask_reg_release.argtypes = [p]
        dll.vmask_reg_release.restype = None
        dll.vmask_reg_fetch.argtypes = [p, p, i64]
        dll.vmask_warp_force.argtypes = [i, p, i, p, i64, i64, i64, p, p, i, i64, i64, i64, p, d, d, d, d, d, p, p, p, p]
        dll.vmask_warp_fit.argtypes = [i, p, p, i64, i64, i64, p, p]
        dll.vmask_warp_upsample.argtypes = [i, p, i64, i64, i64, p, i64, i64, i64]
        dll.vmask_warp_resample.argtypes = [i, p, i, i64, i64, i64, p, p, i, d, p, i64, i64, i64]
        dll.vmask_warp_field.argtypes = [i, p, i, p, i64, i64, i64, p, i, i64, i64, i64, p, d, d, d, d, p, i, d, d, p, p, p]
    return dll


# ------------------------------------------------------------------ host: parameters and matrices
def _affine(a, name):
    if a is None:
        return np.eye(4)
    a = np.array(a, dtype=np.float64)
    if a.shape != (4, 4) or not np.isfinite(a).all() or abs(np.linalg.det(a[:3, :3])) == 0.0:
        raise ValueError('{}: a finite, invertible 4 x 4 matrix'.format(name))
    return a


def paramsToMatrix(params, dof, centre):
    """W = C . Trans(t) . Rz . Ry . Rx . Scale . Shear . C^-1 about the world point `centre`.  params: (tx, ty, tz) in world
    units, (rx, ry, rz) in radians; dof 7 adds one scale s (Scale = (1 + s) I), dof 9 three (sx, sy, sz), dof 12 three shears
    (a, b, c), Shear = [[1, a, b], [0, 1, c], [0, 0, 1]].  Zero parameters give the identity for every dof."""
    if dof not in DOFS:
        raise ValueError('dof: 6, 7, 9 or 12')
    p = np.asarray(params, dtype=np.float64)
    centre = np.asarray(centre, dtype=np.float64)
    if p.shape != (dof,) or not np.isfinite(p).all() or centre.shape != (3,) or not np.isfinite(centre).all():
        raise ValueError('params: {} finite numbers; centre: 3'.format(dof))

    def hom(m3=None, t=None):
        m = np.eye(4)
        if m3 is not None:
            m[:3, :3] = m3
        if t is not None:
            m[:3, 3] = t
        return m
    cx, sx, cy, sy, cz, sz = np.cos(p[3]), np.sin(p[3]), np.cos(p[4]), np.sin(p[4]), np.cos(p[5]), np.sin(p[5])
    Rx = hom([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = hom([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = hom([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    scale = np.ones(3)
    if dof == 7:
        scale = scale + p[6]
    elif dof >= 9:
        scale = scale + p[6:9]
    shear = np.eye(3)
    if dof == 12:
        shear[0, 1], shear[0, 2], shear[1, 2] = p[9], p[10], p[11]
    return hom(t=centre) @ hom(t=p[:3]) @ Rz @ Ry @ Rx @ hom(np.diag(scale)) @ hom(shear) @ hom(t=-centre)


def voxelMap(W, fixedAffine, movingAffine):
    """T = inv(movingAffine) . inv(W) . fixedAffine, 4 x 4: a voxel index of the fixed grid to one of the moving grid."""
    return np.linalg.inv(_affine(movingAffine, 'movingAffine')) @ np.linalg.inv(_affine(W, 'W')) @ _affine(fixedAffine, 'fixedAffine')


def _map12(T):
    """The 12 doubles the C entries take, from a 3 x 4 or 4 x 4 array or a (W, fixedAffine, movingAffine) triple."""
    if isinstance(T, (tuple, list)) and len(T) == 3 and np.ndim(T[0]) == 2:
        T = voxelMap(*T)
    T = np.asarray(T, dtype=np.float64)
    if T.shape not in ((3, 4), (4, 4)) or not np.isfinite(T[:3]).all():
        raise ValueError('T: a finite 3 x 4 or 4 x 4 voxel map, or (W, fixedAffine, movingAffine)')
    return np.ascontiguousarray(T[:3])


def costFromHistogram(H, cost='corratio', minOverlap=0.0, nmask=0):
    """``vmask_reg_cost`` (host code): the cost of a joint histogram of B x B counts; +inf when it holds fewer than
    `minOverlap` * `nmask` voxels, or none."""
    H = np.ascontiguousarray(np.asarray(H), dtype=np.uint64)
    if H.ndim != 2 or H.shape[0] != H.shape[1] or not 8 <= H.shape[0] <= 128:
        raise ValueError('H: B x B counts, 8 <= B <= 128')
    if cost not in COSTS:
        raise ValueError('cost: one of {}'.format(sorted(COSTS)))
    minOverlap, nmask = float(minOverlap), int(nmask)
    if not 0.0 <= minOverlap <= 1.0 or nmask < 0:
        raise ValueError('minOverlap in [0, 1], nmask >= 0')
    out = C.c_double(0.0)
    _G._check(_lib().vmask_reg_cost(H.ctypes.data, H.shape[0], COSTS[cost], minOverlap, nmask, C.addressof(out)))
    return out.value


def binScale(lo, hi, bins):
    """s of the quantisation b(v) = clamp(floor((v - lo) s), 0, bins - 1): bins / (hi - lo), 0 when hi == lo."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError('no finite voxel to take the extrema of (an empty mask?)')
    return 0.0 if hi == lo else float(bins) / (hi - lo)


# ------------------------------------------------------------------ the device entries
class _Held:
    """A device copy that this module owns: what ``register`` makes of host arrays, so that the volumes, the pyramid and the bin
    images cross to the device once and not with every evaluation.  (A torch tensor cannot stand in: torch has to be imported
    before the library is loaded, INTEGRATION.md, which a caller with host arrays has not done.)"""

    def __init__(self, shape, dtype, source=None, device=0):
        self.shape, self.dtype, self.device, self.ptr = tuple(int(n) for n in shape), np.dtype(dtype), int(device), None
        p = C.c_void_p()
        nbytes = max(1, int(np.prod(self.shape))) * self.dtype.itemsize
        _G._check(_lib().vmask_reg_hold(self.device, None if source is None else source.ctypes.data, nbytes, C.byref(p)))
        self.ptr = p.value

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        if out.size:
            _G._check(_lib().vmask_reg_fetch(C.c_void_p(self.ptr), out.ctypes.data, out.nbytes))
        return out

    def __del__(self):
        if self.ptr:
            try:
                _lib().vmask_reg_release(C.c_void_p(self.ptr))
            except Exception:                      # (the interpreter is shutting down)
                pass
            self.ptr = None


def _take(volume, mask=False):
    """(the array as the library takes it, its address, 'held' / 'tensor' / 'host')"""
    if isinstance(volume, _Held):
        return volume, volume.ptr, 'held'
    if mask:
        v, on_device = (_G._u8t(volume), True) if _G._on_device(volume) else (_G._u8c(volume), False)
    else:
        v, on_device = _B._volume(volume, (np.float32, np.float64))
    return v, _B._ptr(v, on_device), 'tensor' if on_device else 'host'


def _take_mask(mask, v, kind):
    if mask is None:
        return None, None
    if isinstance(mask, _Held):
        if mask.shape != tuple(v.shape):
            raise ValueError('mask: the shape of the volume')
        return mask, mask.ptr
    m = _B._mask(mask, v, kind == 'tensor')
    return m, _B._ptr(m, kind == 'tensor')


def _make(shape, dtype, like, kind):
    """(a new array where `like` lives, its address)"""
    if kind == 'held':
        out = _Held(shape, dtype, None, like.device)
        return out, out.ptr
    out = _empty(shape, dtype, like, kind == 'tensor')
    return out, _B._ptr(out, kind == 'tensor')


def _device(v, kind, device):
    return v.device if kind == 'held' else _B._sync(v, kind == 'tensor', device)


def _code(v, kind):
    return 5 if (v.element_size() if kind == 'tensor' else v.dtype.itemsize) == 4 else 6


def _empty(shape, dtype, like, on_device):
    if on_device:
        import torch
        return torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=like.device)
    return np.empty(tuple(shape), dtype)


def _bins(bins):
    bins = int(bins)
    if bins < 8 or bins > 128:
        raise ValueError('bins: 8 to 128')
    return bins


def extrema(volume, mask=None, device=0):
    """``vmask_reg_minmax``: (min, max) of the finite voxels - of those inside `mask` where one is given; (inf, -inf) if none."""
    dll = _lib()
    v, ptr, kind = _take(volume)
    m, mptr = _take_mask(mask, v, kind)
    out = np.empty(2, np.float64)
    _G._check(dll.vmask_reg_minmax(_device(v, kind, device), ptr, _code(v, kind), mptr, *v.shape, out.ctypes.data))
    return float(out[0]), float(out[1])


def quantise(volume, lo, s, bins=64, mask=None, device=0):
    """``vmask_reg_quantise``: (the uint8 bin image of `volume`, the number of voxels in it that take part).  255 marks a voxel
    outside `mask` or one that is not finite."""
    dll = _lib()
    bins, lo, s = _bins(bins), float(lo), float(s)
    if not (np.isfinite(lo) and np.isfinite(s) and s >= 0.0):
        raise ValueError('lo finite, s finite and not negative')
    v, ptr, kind = _take(volume)
    m, mptr = _take_mask(mask, v, kind)
    out, optr = _make(v.shape, np.uint8, v, kind)
    inside = C.c_int64(0)
    _G._check(dll.vmask_reg_quantise(_device(v, kind, device), ptr, _code(v, kind), mptr, *v.shape, bins, lo, s, optr, C.addressof(inside)))
    return out, inside.value


def _bin_image(a):
    """(a uint8 bin image as the library takes it, its address, where it lives)"""
    if isinstance(a, _Held):
        return a, a.ptr, 'held'
    if _G._on_device(a):
        import torch
        if a.dim() != 3 or a.dtype != torch.uint8:
            raise ValueError('fixedBins: a 3-D uint8 bin image')
        a = a.contiguous()
        return a, a.data_ptr(), 'tensor'
    a = np.asarray(a)
    if a.ndim != 3 or a.dtype != np.uint8:
        raise ValueError('fixedBins: a 3-D uint8 bin image')
    a = np.ascontiguousarray(a)
    return a, a.ctypes.data, 'host'


def jointHistogram(fixedBins, moving, T, bins=64, mlo=0.0, ms=1.0, device=0):
    """``vmask_reg_joint_hist``: the bins x bins uint64 counts H[bf, bm] over the voxels of the bin image `fixedBins` (see
    ``quantise``) whose sample of `moving` through the voxel map `T` is inside, bm the sample's bin with (mlo, ms).  An image of
    255 only gives H = 0."""
    dll = _lib()
    bins, mlo, ms = _bins(bins), float(mlo), float(ms)
    if not (np.isfinite(mlo) and np.isfinite(ms)):
        raise ValueError('mlo, ms: finite')
    t12 = _map12(T)
    fb, fptr, fkind = _bin_image(fixedBins)
    mv, mptr, mkind = _take(moving)
    H = np.empty((bins, bins), np.uint64)
    dev = _device(mv, mkind, _device(fb, fkind, device))
    _G._check(dll.vmask_reg_joint_hist(dev, fptr, *fb.shape, mptr, _code(mv, mkind), *mv.shape, t12.ctypes.data, bins, mlo, ms, H.ctypes.data))
    return H


def shrink(volume, mask=False, device=0):
    """``vmask_reg_shrink``: one level of the pyramid, extents ceil(n / 2).  A volume (any dtype; float32 and float64 go in as
    they are, others as float64) gives the float64 block mean, indices clamped at the far faces; with mask=True the array is a
    mask and gives the uint8 "any non-zero" of every 2 x 2 x 2 block.  The output's voxel -> world affine is the input's times
    ``SHRINK``."""
    dll = _lib()
    v, ptr, kind = _take(volume, mask)
    out, optr = _make([(int(n) + 1) // 2 for n in v.shape], np.uint8 if mask else np.float64, v, kind)
    _G._check(dll.vmask_reg_shrink(_device(v, kind, device), ptr, 0 if mask else _code(v, kind), *v.shape, optr))
    return out


def resample(moving, T, shape, order=1, fill=0, device=0):
    """``vmask_reg_resample``: `moving` on a grid of `shape` through the voxel map `T` - a 3 x 4 or 4 x 4 array, or the triple
    (W, fixedAffine, movingAffine).  order 1 is trilinear and gives float64 (float32 and float64 volumes go in as they are,
    others as float64); order 0 takes the nearest voxel and keeps the type (uint8, int16, int32, float32, float64; bool goes in
    as uint8).  `fill` is written where the voxel falls outside the moving volume."""
    dll = _lib()
    shape = tuple(int(x) for x in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError('shape: three extents')
    t12 = _map12(T)
    v, on_device, code, dtype, fill = _resample_input(moving, order, fill)
    out = _empty(shape, dtype, v, on_device)
    dev = _B._sync(v, on_device, device)
    _G._check(dll.vmask_reg_resample(dev, _B._ptr(v, on_device), code, *v.shape, t12.ctypes.data, order, fill, _B._ptr(out, on_device), *shape))
    return out


def _resample_input(moving, order, fill):
    """(the volume as ``vmask_reg_resample`` / ``vmask_warp_resample`` take it, on the device?, its dtype code, the output's dtype, fill)"""
    if order not in (0, 1):
        raise ValueError('order: 0 or 1')
    fill = float(fill)
    if order == 1:
        v, on_device = _B._volume(moving, (np.float32, np.float64))
        return v, on_device, _code(v, 'tensor' if on_device else 'host'), np.float64, fill
    if _G._on_device(moving):
        import torch
        v, on_device = (moving.to(torch.uint8) if moving.dtype == torch.bool else moving).contiguous(), True
        dtype = np.dtype(str(v.dtype).replace('torch.', ''))
    else:
        v, on_device = np.asarray(moving), False
        v = np.ascontiguousarray(v.astype(np.uint8) if v.dtype == np.bool_ else v)
        dtype = v.dtype
    if (v.dim() if on_device else v.ndim) != 3:
        raise ValueError('expected a 3-D volume')
    if dtype not in NEAREST_TYPES:
        raise ValueError('order 0: uint8, int16, int32, float32 or float64')
    if np.dtype(dtype).kind in 'iu' and not (np.isfinite(fill) and fill == np.floor(fill) and np.iinfo(dtype).min <= fill <= np.iinfo(dtype).max):
        raise ValueError('fill: a value of the volume\'s type')
    return v, on_device, DTYPE_CODES[np.dtype(dtype)], dtype, fill


# ------------------------------------------------------------------ host: the search
def _spacing(affine):
    return np.sqrt((affine[:3, :3] ** 2).sum(axis=0))


def _steps(dof, voxel):
    kinds = [0] * 3 + [1] * 3 + [2] * (1 if dof == 7 else 3 if dof >= 9 else 0) + [3] * (3 if dof == 12 else 0)
    first = np.array(FIRST_STEPS)
    first[0] = first[0] * voxel
    return first[kinds]


def patternSearch(evaluate, params, steps, tolerances, maxEvaluations, record):
    """The deterministic search of one level.  `evaluate(params)` is the cost.  The parameters are visited in order; each tries
    +step and, only if that was not accepted, -step; a candidate is accepted iff its cost is strictly lower (`record(params,
    cost)` is called); a full cycle without an acceptance halves every step; the search ends when every step is below its
    tolerance, or after `maxEvaluations` evaluations, in the midst of a cycle if need be.  Returns (params, cost, evaluations)."""
    params, steps = np.array(params, dtype=np.float64), np.array(steps, dtype=np.float64)
    best = evaluate(params)
    count = 1
    while count < maxEvaluations:
        improved = False
        for k in range(len(params)):
            for sign in (1.0, -1.0):
                if count >= maxEvaluations:
                    return params, best, count
                cand = params.copy()
                cand[k] = cand[k] + sign * steps[k]
                c = evaluate(cand)
                count += 1
                if c < best:
                    params, best, improved = cand, c, True
                    record(params, best)
                    break
        if not improved:
            steps = steps * 0.5
            if (steps < tolerances).all():
                break
    return params, best, count


def registerWith(ops, fixed, moving, fixedAffine=None, movingAffine=None, fixedMask=None, dof=6, cost='corratio', bins=64, levels=3,
                 minOverlap=0.25, search=None, maxEvaluations=2000, initial=None):
    """``register`` over the operations of `ops`: ``extrema(volume, mask)``, ``quantise(volume, lo, s, bins, mask)``,
    ``shrink(array, mask)``, ``jointHistogram(fixedBins, moving, T, bins, mlo, ms)`` and ``cost(H, name, minOverlap, nmask)``; an
    optional ``hold(array)`` may move an array to where the operations want it.  The library passes its GPU entries, the tests'
    model its numpy restatements; everything else - the volumes' conversion, the pyramid's bookkeeping, the parameters, the
    search - is this function for both.  Volumes of any dtype are converted once, before the pyramid: float32 and float64
    stay, everything else becomes float64; the mask becomes uint8 0 / 1."""
    if dof not in DOFS:
        raise ValueError('dof: 6, 7, 9 or 12')
    if cost not in COSTS:
        raise ValueError('cost: one of {}'.format(sorted(COSTS)))
    bins, levels, maxEvaluations, minOverlap = _bins(bins), int(levels), int(maxEvaluations), float(minOverlap)
    if levels < 1 or levels > 8:
        raise ValueError('levels: 1 to 8')
    if maxEvaluations < 1:
        raise ValueError('maxEvaluations: at least 1')
    if not 0.0 <= minOverlap <= 1.0:
        raise ValueError('minOverlap: 0 to 1')
    fA, mA = _affine(fixedAffine, 'fixedAffine'), _affine(movingAffine, 'movingAffine')
    if len(fixed.shape) != 3 or len(moving.shape) != 3:
        raise ValueError('expected 3-D volumes')
    if fixedMask is not None and tuple(fixedMask.shape) != tuple(fixed.shape):
        raise ValueError('fixedMask: the shape of the fixed volume')
    params = np.zeros(dof) if initial is None else np.array(initial, dtype=np.float64)
    if params.shape != (dof,) or not np.isfinite(params).all():
        raise ValueError('initial: {} finite parameters'.format(dof))
    grid = None
    if search is not None:
        if len(search) != 2 or not (np.isfinite(search[0]) and np.isfinite(search[1]) and search[0] >= 0 and search[1] > 0):
            raise ValueError('search: (rangeDeg >= 0, stepDeg > 0)')
        k = int(np.floor(float(search[0]) / float(search[1]) + 1e-9))
        if (2 * k + 1) ** 3 > 100000:
            raise ValueError('search: more than 100000 rotations')
        grid = np.deg2rad(float(search[1]) * np.arange(-k, k + 1))
    centre = (fA @ np.append((np.array(fixed.shape, dtype=np.float64) - 1.0) / 2.0, 1.0))[:3]
    fixed, on_device = _B._volume(fixed, (np.float32, np.float64))
    moving = _B._volume(moving, (np.float32, np.float64))[0]
    if fixedMask is not None:
        fixedMask = _B._mask(fixedMask, fixed, on_device)
    hold = getattr(ops, 'hold', lambda a: a)
    fixed, moving, fixedMask = hold(fixed), hold(moving), None if fixedMask is None else hold(fixedMask)
    # the pyramid: index 0 is the full resolution
    F, M = [(fixed, fA, fixedMask)], [(moving, mA)]
    for _ in range(levels - 1):
        (f, a, m), (g, b) = F[-1], M[-1]
        if min((int(n) + 1) // 2 for n in tuple(f.shape) + tuple(g.shape)) < 8:
            break
        F.append((ops.shrink(f, False), a @ SHRINK, None if m is None else ops.shrink(m, True)))
        M.append((ops.shrink(g, False), b @ SHRINK))
    F.reverse()
    M.reverse()
    rows, evaluations = [], []
    for level, ((f, a, m), (g, b)) in enumerate(zip(F, M)):
        flo, fhi = ops.extrema(f, m)
        fbins, nmask = ops.quantise(f, flo, binScale(flo, fhi, bins), bins, m)
        mlo, mhi = ops.extrema(g, None)
        ms = binScale(mlo, mhi, bins)
        if nmask == 0:
            raise ValueError('the fixed mask is empty at level {}'.format(level))

        def evaluate(p):
            try:
                T = voxelMap(paramsToMatrix(p, dof, centre), a, b)
            except (np.linalg.LinAlgError, ValueError):
                return float('inf')
            if not np.isfinite(T).all():
                return float('inf')
            return ops.cost(ops.jointHistogram(fbins, g, T, bins, mlo, ms), cost, minOverlap, nmask)

        extra = 0
        if grid is not None and level == 0:
            best = None
            for r in itertools.product(grid, repeat=3):
                cand = params.copy()
                cand[3:6] = params[3:6] + np.array(r)
                c = evaluate(cand)
                extra += 1
                if best is None or c < best[0]:
                    best = (c, cand)
            params = best[1]
            rows.append(np.concatenate(([float(level)], params, [best[0]])))
        steps = _steps(dof, float(_spacing(a).min()))
        finest = level == len(F) - 1
        params, _, count = patternSearch(evaluate, params, steps, steps / (FINE if finest else COARSE), maxEvaluations,
                                         lambda p, c: rows.append(np.concatenate(([float(level)], p, [c]))))
        evaluations.append(count + extra)
    trace = {'steps': np.array(rows, dtype=np.float64).reshape(len(rows), dof + 2), 'evaluations': np.array(evaluations, dtype=np.int64),
             'params': params.copy()}
    return paramsToMatrix(params, dof, centre), trace


def register(fixed, moving, fixedAffine=None, movingAffine=None, fixedMask=None, dof=6, cost='corratio', bins=64, levels=3, minOverlap=0.25,
             search=None, maxEvaluations=2000, initial=None, device=0):
    """The 4 x 4 matrix W that takes world coordinates of `moving` to world coordinates of `fixed`, and the search's trace.

    `fixedAffine` / `movingAffine` are the volumes' voxel -> world matrices (None: the identity); `fixedMask` limits the voxels of
    the fixed grid that are counted.  dof 6 is rigid, 7 adds a global scale, 9 three scales, 12 three shears (``paramsToMatrix``),
    about the world centre of the fixed grid.  `levels` block-mean pyramids levels are searched coarse to fine (fewer when an extent
    would fall below 8); per level the intensities over the mask are cut into `bins` bins between their extrema and a pattern search
    (``patternSearch``) of at most `maxEvaluations` evaluations minimises `cost` - 'corratio', 'mi' or 'nmi' - of the joint
    histogram, +inf where fewer than `minOverlap` of the mask's voxels fall inside the moving volume.  search=(rangeDeg, stepDeg)
    first evaluates every rotation of that grid about the three axes at the coarsest level and starts from the best (ties: the first).
    `initial`: the starting parameters.  trace: {'steps': one row (level, parameters, cost) per accepted step, 'evaluations': their
    number per level, 'params': the final parameters}.  An empty mask raises ValueError.  Volumes of any dtype are taken (float32 and
    float64 as they are, others as float64), host arrays are copied to the device once."""
    ops = types.SimpleNamespace(extrema=lambda v, m: extrema(v, m, device), quantise=lambda v, lo, s, b, m: quantise(v, lo, s, b, m, device),
                                shrink=lambda v, m: shrink(v, m, device), cost=costFromHistogram,
                                jointHistogram=lambda fb, g, T, b, mlo, ms: jointHistogram(fb, g, T, b, mlo, ms, device),
                                hold=lambda a: a if _G._on_device(a) else _Held(a.shape, a.dtype, a, device))
    _lib()
    return registerWith(ops, fixed, moving, fixedAffine, movingAffine, fixedMask, dof, cost, bins, levels, minOverlap, search, maxEvaluations, initial)


# ------------------------------------------------------------------ the files
def _stem(name):
    for ext in ('.nii.gz', '.nii'):
        if name.endswith(ext):
            return name[:-len(ext)]
    return name


def main(baseFolder=None, movingName=None, fixedName=BRAIN_FILE, outputName=None, matrixName=None, **parameters):
    """File-level step: `movingName` registered to `fixedName` (both in `baseFolder`) by ``register(**parameters)`` with the
    files' affines.  Writes `<moving>Registered.nii.gz` (`outputName`): the moving volume on the fixed grid, trilinear, float32,
    with the fixed file's affine; and `<moving>ToFixed.mat` (`matrixName`): W as a 4 x 4 text matrix in %.17g - moving world to
    fixed world, NOT FSL's scaled-millimetre convention (see the module's text).  Returns (W, the registered volume)."""
    if baseFolder is None:
        baseFolder = os.getcwd()
    if movingName is None:
        raise ValueError('movingName: the file to register')
    if 'fixedAffine' in parameters or 'movingAffine' in parameters:
        raise ValueError('main takes the affines from the files')
    fixed, fA = loadVolume(baseFolder, fixedName)
    moving, mA = loadVolume(baseFolder, movingName)
    fixed, moving = np.ascontiguousarray(fixed), np.ascontiguousarray(moving)
    W, _ = register(fixed, moving, fixedAffine=fA, movingAffine=mA, **parameters)
    result = resample(moving, (W, fA, mA), fixed.shape, order=1, fill=0, device=parameters.get('device', 0))
    outputName = outputName or _stem(movingName) + 'Registered.nii.gz'
    matrixName = matrixName or _stem(movingName) + 'ToFixed.mat'
    path = os.path.join(baseFolder, outputName)
    saveVolume(result, fA, path, astype=np.float32)
    print('{} saved to {}.'.format(outputName, path))
    path = os.path.join(baseFolder, matrixName)
    np.savetxt(path, W, fmt='%.17g')
    print('{} saved to {}.'.format(matrixName, path))
    return W, result


def applyTransform(baseFolder, volumeName, matrixName, referenceName=BRAIN_FILE, order=0, outputName=None):
    """Carry a mask or another series of the moving image's space over a matrix that ``main`` wrote: `volumeName` resampled onto
    the grid of `referenceName` through W of `matrixName`, nearest voxel and the file's type by default (int8 and uint16 widen to
    int16 and int32), trilinear float32 with order=1; written as `<volume>Transformed.nii.gz` (`outputName`) with the reference's
    affine.  Returns the volume."""
    volume, vA = loadVolume(baseFolder, volumeName)
    reference, rA = loadVolume(baseFolder, referenceName)
    W = np.loadtxt(os.path.join(baseFolder, matrixName)).reshape(4, 4)
    volume = np.ascontiguousarray(volume)
    if order == 0:
        widen = {np.dtype(np.int8): np.int16, np.dtype(np.uint16): np.int32, np.dtype(np.bool_): np.uint8}
        volume = volume.astype(widen.get(volume.dtype, volume.dtype))
    result = resample(volume, (W, rA, vA), reference.shape, order=order, fill=0)
    outputName = outputName or _stem(volumeName) + 'Transformed.nii.gz'
    path = os.path.join(baseFolder, outputName)
    saveVolume(result, rA, path, astype=result.dtype if order == 0 else np.float32)
    print('{} saved to {}.'.format(outputName, path))
    return result


# ------------------------------------------------------------------ nonlinear: the device entries
def _take_warp(u, grid=None, name='warp'):
    """(a float64 [3, n0, n1, n2] array as the library takes it, its address, 'held' / 'tensor' / 'host')"""
    if isinstance(u, _Held):
        shape, a, ptr, kind = u.shape, u, u.ptr, 'held'
        if u.dtype != np.float64:
            raise ValueError('{}: float64'.format(name))
    elif _G._on_device(u):
        import torch
        a = u.to(torch.float64).contiguous()
        shape, ptr, kind = tuple(a.shape), a.data_ptr(), 'tensor'
    else:
        a = np.ascontiguousarray(np.asarray(u), dtype=np.float64)
        shape, ptr, kind = a.shape, a.ctypes.data, 'host'
    if len(shape) != 4 or shape[0] != 3 or (grid is not None and tuple(shape[1:]) != tuple(int(x) for x in grid)):
        raise ValueError('{}: float64 [3, n0, n1, n2] on the fixed grid'.format(name))
    return a, ptr, kind


def _finite(x, name):
    x = float(x)
    if not np.isfinite(x):
        raise ValueError('{}: finite'.format(name))
    return x


def _force_args(fixed, moving, T, flo, fs, mlo, ms, maxStep, mask):
    f, fptr, fkind = _take(fixed)
    g, gptr, gkind = _take(moving)
    m, mptr = _take_mask(mask, f, fkind)
    scales = [_finite(x, name) for x, name in ((flo, 'flo'), (fs, 'fs'), (mlo, 'mlo'), (ms, 'ms'))]
    return (f, fptr, fkind), (g, gptr, gkind), (m, mptr), _map12(T), scales, _B._positive(maxStep, 'maxStep')


def forcePass(fixed, moving, T, warp, flo, fs, mlo, ms, maxStep=0.5, mask=None, device=0):
    """``vmask_warp_force``: (delta float64 [3, n0, n1, n2], part uint8 [n0, n1, n2], S, count) - the demons force at every voxel of
    the fixed grid that takes part (inside `mask`, finite, its sample of `moving` through `T` and `warp` inside), which those
    are, and the sum of their squared residuals and their number.  fs and ms are ``binScale(lo, hi, 1)`` of the two volumes."""
    dll = _lib()
    (f, fptr, fkind), (g, gptr, gkind), (m, mptr), t12, scales, maxStep = _force_args(fixed, moving, T, flo, fs, mlo, ms, maxStep, mask)
    u, uptr, ukind = _take_warp(warp, f.shape)
    delta, dptr = _make((3,) + tuple(f.shape), np.float64, f, fkind)
    part, pptr = _make(f.shape, np.uint8, f, fkind)
    S, count = C.c_double(0.0), C.c_int64(0)
    dev = _device(g, gkind, _device(f, fkind, device))
    if ukind == 'tensor':
        _B._sync(u, True, device)
    _G._check(dll.vmask_warp_force(dev, fptr, _code(f, fkind), mptr, *f.shape, uptr, gptr, _code(g, gkind), *g.shape, t12.ctypes.data, *scales, maxStep,
                                   dptr, pptr, C.addressof(S), C.addressof(count)))
    return delta, part, S.value, count.value


def fitForces(delta, part, spans, device=0):
    """``vmask_warp_fit``: float64 [3, spans + 3 per axis], ``bias.bsplineFit(delta[c], part, spans)`` for the three components."""
    dll = _lib()
    M = _B._spans(spans, 64, 'spans')
    d, dptr, kind = _take_warp(delta, None, 'delta')
    p, pptr, _ = _take(part, True)
    if tuple(p.shape) != tuple(d.shape[1:]):
        raise ValueError('part: the shape of a component of delta')
    phi, optr = _make([3] + [int(k) + 3 for k in M], np.float64, d, kind)
    _G._check(dll.vmask_warp_fit(_device(d, kind, device), dptr, pptr, *p.shape, M.ctypes.data, optr))
    return phi


def upsampleWarp(coarse, shape, device=0):
    """``vmask_warp_upsample``: the warp of a coarser level of the pyramid on the grid of `shape`, in that grid's voxels."""
    dll = _lib()
    shape = tuple(int(x) for x in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError('shape: three extents')
    c, cptr, kind = _take_warp(coarse)
    fine, fptr = _make((3,) + shape, np.float64, c, kind)
    _G._check(dll.vmask_warp_upsample(_device(c, kind, device), cptr, *c.shape[1:], fptr, *shape))
    return fine


def warpLevel(fixed, moving, T, warp, flo, fs, mlo, ms, spans, iterations=30, maxStep=0.5, convergenceThreshold=0.01, mask=None, device=0):
    """``vmask_warp_field``: the iterations of one level from `warp`.  Returns (the warp, one row (cost, count, max |dphi|) per
    iteration).  A warp on the device (a tensor, a held array) is updated in place; a host array is copied first.  ValueError
    when no voxel takes part at the first iteration."""
    from ._capi import VrgError
    dll = _lib()
    (f, fptr, fkind), (g, gptr, gkind), (m, mptr), t12, scales, maxStep = _force_args(fixed, moving, T, flo, fs, mlo, ms, maxStep, mask)
    M = _B._spans(spans, 64, 'spans')
    iterations, threshold = int(iterations), _B._positive(convergenceThreshold, 'convergenceThreshold')
    if iterations < 1 or iterations > 200:
        raise ValueError('iterations: 1 to 200')
    u, uptr, ukind = _take_warp(np.array(warp, dtype=np.float64) if isinstance(warp, np.ndarray) else warp, f.shape)
    rows = np.zeros((iterations, 3), np.float64)
    count = C.c_int64(0)
    dev = _device(g, gkind, _device(f, fkind, device))
    if ukind == 'tensor':
        _B._sync(u, True, device)
    try:
        _G._check(dll.vmask_warp_field(dev, fptr, _code(f, fkind), mptr, *f.shape, gptr, _code(g, gkind), *g.shape, t12.ctypes.data, *scales, M.ctypes.data,
                                       iterations, maxStep, threshold, uptr, rows.ctypes.data, C.addressof(count)))
    except VrgError as e:
        if e.code == -1:                                     # (what the host can check has passed: no voxel takes part)
            raise ValueError(str(e))
        raise
    return u, rows[:count.value].copy()


def warpResample(moving, W, warp, fixedAffine=None, movingAffine=None, order=1, fill=0, device=0):
    """``vmask_warp_resample``: `moving` on the fixed grid - the grid of `warp`, float64 [3, n0, n1, n2] - through the matrix `W`
    that ``register`` returns (None: the identity), the two voxel -> world affines and the warp that ``registerNonlinear`` returns.
    order, fill and the types as ``resample``; a zero warp gives ``resample``'s bytes.  A tensor on the GPU gives a tensor."""
    dll = _lib()
    t12 = _map12((np.eye(4) if W is None else W, fixedAffine, movingAffine))
    v, on_device, code, dtype, fill = _resample_input(moving, order, fill)
    if on_device and not _G._on_device(warp) and not isinstance(warp, _Held):
        import torch
        warp = torch.as_tensor(np.asarray(warp, dtype=np.float64), device=v.device)
    u, uptr, ukind = _take_warp(warp)
    shape = tuple(int(x) for x in u.shape[1:])
    out = _empty(shape, dtype, v, on_device)
    dev = _B._sync(v, on_device, device)
    if ukind == 'tensor':
        _B._sync(u, True, device)
    _G._check(dll.vmask_warp_resample(dev, _B._ptr(v, on_device), code, *v.shape, t12.ctypes.data, uptr, order, fill, _B._ptr(out, on_device), *shape))
    return out


# ------------------------------------------------------------------ nonlinear: the levels
def registerNonlinearWith(ops, fixed, moving, W=None, fixedAffine=None, movingAffine=None, fixedMask=None, splineSpans=(2, 2, 2), levels=3,
                          iterations=30, maxStep=0.5, convergenceThreshold=0.01):
    """``registerNonlinear`` over the operations of `ops`: ``extrema(volume, mask)``, ``shrink(array, mask)``, ``zeros(like)`` (a
    zero warp on the grid of a volume), ``upsample(warp, shape)``, ``level(fixed, moving, T, warp, flo, fs, mlo, ms, spans,
    iterations, maxStep, threshold, mask)`` (the iterations of one level: the warp and one row (cost, count, max |dphi|) per
    iteration) and ``result(warp)``; an optional ``hold(array)`` may move an array to where the operations want it.  The library
    passes its GPU entries, the tests' model (tests/warp_model.py) its numpy restatements; the conversion of the volumes, the
    pyramid, the maps and scales of the levels and the trace are this function for both."""
    m0 = _B._spans(splineSpans, 64, 'splineSpans')
    levels, iterations = int(levels), int(iterations)
    if levels < 1 or levels > 8:
        raise ValueError('levels: 1 to 8')
    if iterations < 1 or iterations > 200:
        raise ValueError('iterations: 1 to 200')
    maxStep, threshold = _B._positive(maxStep, 'maxStep'), _B._positive(convergenceThreshold, 'convergenceThreshold')
    W = _affine(W, 'W')
    fA, mA = _affine(fixedAffine, 'fixedAffine'), _affine(movingAffine, 'movingAffine')
    if len(fixed.shape) != 3 or len(moving.shape) != 3:
        raise ValueError('expected 3-D volumes')
    if fixedMask is not None and tuple(fixedMask.shape) != tuple(fixed.shape):
        raise ValueError('fixedMask: the shape of the fixed volume')
    fixed, on_device = _B._volume(fixed, (np.float32, np.float64))
    moving = _B._volume(moving, (np.float32, np.float64))[0]
    if fixedMask is not None:
        fixedMask = _B._mask(fixedMask, fixed, on_device)
    hold = getattr(ops, 'hold', lambda a: a)
    fixed, moving, fixedMask = hold(fixed), hold(moving), None if fixedMask is None else hold(fixedMask)
    # the pyramid of registerWith: index 0 is the full resolution
    F, M = [(fixed, fA, fixedMask)], [(moving, mA)]
    for _ in range(levels - 1):
        (f, a, m), (g, b) = F[-1], M[-1]
        if min((int(n) + 1) // 2 for n in tuple(f.shape) + tuple(g.shape)) < 8:
            break
        F.append((ops.shrink(f, False), a @ SHRINK, None if m is None else ops.shrink(m, True)))
        M.append((ops.shrink(g, False), b @ SHRINK))
    F.reverse()
    M.reverse()
    warp, rows = None, []
    for level, ((f, a, m), (g, b)) in enumerate(zip(F, M)):
        spans = [min(64, int(k) * 2 ** level) for k in m0]
        flo, fhi = ops.extrema(f, None)                      # (of the whole volumes: the mask limits the forces, not the scaling)
        mlo, mhi = ops.extrema(g, None)
        fs, ms = binScale(flo, fhi, 1), binScale(mlo, mhi, 1)
        T = voxelMap(W, a, b)
        warp = ops.zeros(f) if warp is None else ops.upsample(warp, tuple(int(n) for n in f.shape))
        warp, r = ops.level(f, g, T, warp, flo, fs, mlo, ms, spans, iterations, maxStep, threshold, m)
        rows.extend((float(level), float(c), float(n), float(top)) for c, n, top in r)
    return ops.result(warp), np.array(rows, dtype=np.float64).reshape(len(rows), 4)


def registerNonlinear(fixed, moving, W=None, fixedAffine=None, movingAffine=None, fixedMask=None, splineSpans=(2, 2, 2), levels=3, iterations=30,
                      maxStep=0.5, convergenceThreshold=0.01, device=0):
    """The warp that brings `moving` onto `fixed` where the matrix `W` of ``register`` (None: the identity) leaves a smooth
    deformation, and the trace: (warp, trace).

    warp is float64 [3, n0, n1, n2]: at fixed voxel v the moving volume is sampled at T (v + warp[:, v]), T = ``voxelMap(W,
    fixedAffine, movingAffine)`` - displacements in fixed voxels (``warpResample`` applies it).  `levels` block-mean pyramid levels
    run coarse to fine (fewer when an extent would fall below 8), the warp doubled and resampled in between; at level L the update
    lives on a cubic B-spline lattice of `splineSpans` 2^L spans per axis (at most 64).  Per iteration, at most `iterations` a level:
    the demons force of the squared difference of the two volumes, each scaled to [0, 1] between its extrema (over `fixedMask` for
    the fixed one) - no single force exceeds `maxStep` voxels -, its B-spline fit over the voxels that take part, and the fit's
    evaluation added to the warp.  A level ends when the largest control-point update falls below `convergenceThreshold` (voxels of
    that level).  trace: one row (level, cost before the step, voxels that took part, max |update|) per iteration.  ValueError when
    no voxel takes part at a level's first iteration (an empty mask, volumes that do not overlap).  The cost is a sum of squared
    differences: both volumes must be of one modality.  Volumes of any dtype are taken (float32 and float64 as they are, others
    as float64); host arrays are copied to the device once and give a host array; tensors on the GPU are used in place and give a
    tensor."""
    def zeros(f):
        if isinstance(f, _Held):
            return _Held((3,) + f.shape, np.float64, np.zeros((3,) + f.shape), f.device)
        import torch
        return torch.zeros((3,) + tuple(f.shape), dtype=torch.float64, device=f.device)
    ops = types.SimpleNamespace(extrema=lambda v, m: extrema(v, m, device), shrink=lambda v, m: shrink(v, m, device), zeros=zeros,
                                upsample=lambda u, shape: upsampleWarp(u, shape, device),
                                level=lambda f, g, T, u, flo, fs, mlo, ms, spans, it, step, thr, m: warpLevel(f, g, T, u, flo, fs, mlo, ms, spans, it, step, thr, m, device),
                                result=lambda u: u.numpy() if isinstance(u, _Held) else u,
                                hold=lambda a: a if _G._on_device(a) else _Held(a.shape, a.dtype, a, device))
    _lib()
    return registerNonlinearWith(ops, fixed, moving, W, fixedAffine, movingAffine, fixedMask, splineSpans, levels, iterations, maxStep, convergenceThreshold)


# ------------------------------------------------------------------ nonlinear: the files
def mainNonlinear(baseFolder=None, movingName=None, fixedName=BRAIN_FILE, matrixName=None, outputName=None, warpName=None, **parameters):
    """File-level step after ``main``: `movingName` warped onto `fixedName` (both in `baseFolder`).  The matrix W is read from
    `<moving>ToFixed.mat` (`matrixName`) where ``main`` has left one; where not, ``register`` runs first with its defaults and the
    matrix is written there.  Then ``registerNonlinear(W=W, **parameters)`` with the files' affines.  Writes
    `<moving>Warped.nii.gz` (`outputName`): the moving volume through W and the warp on the fixed grid, trilinear, float32, the
    fixed file's affine; and `<moving>Warp.nii.gz` (`warpName`): the warp as a 4-D float32 volume [n0, n1, n2, 3] with that
    affine, displacements in fixed voxels.  Returns (warp, the warped volume), both float64."""
    if baseFolder is None:
        baseFolder = os.getcwd()
    if movingName is None:
        raise ValueError('movingName: the file to register')
    if 'fixedAffine' in parameters or 'movingAffine' in parameters or 'W' in parameters:
        raise ValueError('mainNonlinear takes the affines and the matrix from the files')
    device = parameters.get('device', 0)
    fixed, fA = loadVolume(baseFolder, fixedName)
    moving, mA = loadVolume(baseFolder, movingName)
    fixed, moving = np.ascontiguousarray(fixed), np.ascontiguousarray(moving)
    matrixName = matrixName or _stem(movingName) + 'ToFixed.mat'
    path = os.path.join(baseFolder, matrixName)
    if os.path.exists(path):
        W = np.loadtxt(path).reshape(4, 4)
    else:
        W, _ = register(fixed, moving, fixedAffine=fA, movingAffine=mA, device=device)
        np.savetxt(path, W, fmt='%.17g')
        print('{} saved to {}.'.format(matrixName, path))
    warp, _ = registerNonlinear(fixed, moving, W=W, fixedAffine=fA, movingAffine=mA, **parameters)
    result = warpResample(moving, W, warp, fA, mA, order=1, fill=0, device=device)
    outputName = outputName or _stem(movingName) + 'Warped.nii.gz'
    path = os.path.join(baseFolder, outputName)
    saveVolume(result, fA, path, astype=np.float32)
    print('{} saved to {}.'.format(outputName, path))
    warpName = warpName or _stem(movingName) + 'Warp.nii.gz'
    path = os.path.join(baseFolder, warpName)
    saveVolume(np.moveaxis(warp, 0, 3), fA, path, astype=np.float32)
    print('{} saved to {}.'.format(warpName, path))
    return warp, result


def applyWarp(baseFolder, volumeName, matrixName, warpName, referenceName=BRAIN_FILE, order=0, outputName=None, device=0):
    """Carry a mask or another series of the moving image's space over the matrix and the warp that ``mainNonlinear`` wrote:
    `volumeName` resampled onto the grid of `referenceName` through W of `matrixName` and the (float32) warp of `warpName`,
    nearest voxel and the file's type by default (int8 and uint16 widen to int16 and int32), trilinear float32 with order=1;
    written as `<volume>Warped.nii.gz` (`outputName`) with the reference's affine.  Returns the volume."""
    volume, vA = loadVolume(baseFolder, volumeName)
    reference, rA = loadVolume(baseFolder, referenceName)
    stored, _ = loadVolume(baseFolder, warpName)
    if stored.ndim != 4 or stored.shape[3] != 3 or stored.shape[:3] != reference.shape:
        raise ValueError('{}: a 4-D warp [n0, n1, n2, 3] on the grid of {}'.format(warpName, referenceName))
    warp = np.ascontiguousarray(np.moveaxis(stored, 3, 0), dtype=np.float64)
    W = np.loadtxt(os.path.join(baseFolder, matrixName)).reshape(4, 4)
    volume = np.ascontiguousarray(volume)
    if order == 0:
        widen = {np.dtype(np.int8): np.int16, np.dtype(np.uint16): np.int32, np.dtype(np.bool_): np.uint8}
        volume = volume.astype(widen.get(volume.dtype, volume.dtype))
    result = warpResample(volume, W, warp, rA, vA, order=order, fill=0, device=device)
    outputName = outputName or _stem(volumeName) + 'Warped.nii.gz'
    path = os.path.join(baseFolder, outputName)
    saveVolume(result, rA, path, astype=result.dtype if order == 0 else np.float32)
    print('{} saved to {}.'.format(outputName, path))
    return result
