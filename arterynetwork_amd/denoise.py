"""Edge-preserving denoising on the GPU: the "MR image denoising" step in front of ``vesselness.main``.

The reference pipeline leaves this step to an external GUI tool (its README, Pre-processing) and holds no code for it.  Here
it is Perona-Malik diffusion over the 6 neighbours in float64, or a median over a window of at most 3 x 3 x 3 voxels, by
definitions of our own - include/vmask.h ``vmask_diffuse`` / ``vmask_median``, DESIGN.md section 9 entry f14 - computed by HIP
kernels.  Agreement with the external tool's filters is not claimed: their discretisation differs.  No CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import generateVesselVolume as _G
from .nifti import loadVolume, saveVolume
from .vesselness import BRAIN_FILE

DENOISED_FILE = 'brainVolumeDenoised.nii.gz'
FUNCTIONS = {'rational': 0, 'exponential': 1}


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_diffuse, 'argtypes', None):
        p, i64, d = C.c_void_p, C.c_int64, C.c_double
        dll.vmask_diffuse.argtypes = [C.c_int, p, C.c_int, i64, i64, i64, p, d, C.c_int, d, C.c_int, p]
        dll.vmask_median.argtypes = [C.c_int, p, C.c_int, i64, i64, i64, C.c_int, C.c_int, C.c_int, p]
    return dll


def stabilityBound(spacing=None):
    """The largest stable time step of ``anisotropicDiffusion``: 1 / (2 sum 1 / h_a^2), 1/6 at unit spacing - the same float64
    operations as the library's."""
    h = np.ones(3) if spacing is None else np.asarray(spacing, dtype=np.float64)
    ih = 1.0 / h
    return float(1.0 / (2.0 * ((ih[0] * ih[0] + ih[1] * ih[1]) + ih[2] * ih[2])))


def _volume(volume):
    """(array or tensor as the library takes it, dtype code, on the device?)"""
    if _G._on_device(volume):
        import torch
        if volume.dim() != 3:
            raise ValueError('expected a 3-D volume')
        v = volume.contiguous()
        if v.dtype not in (torch.float32, torch.float64):
            v = v.to(torch.float64)
        return v, (5 if v.dtype == torch.float32 else 6), True
    v = np.asarray(volume)
    if v.ndim != 3:
        raise ValueError('expected a 3-D volume')
    if v.dtype not in (np.float32, np.float64):
        v = v.astype(np.float64)
    return np.ascontiguousarray(v), (5 if v.dtype == np.float32 else 6), False


def anisotropicDiffusion(volume, conductance, iterations=5, timeStep=None, spacing=None, function='rational', device=0):
    """Perona-Malik diffusion of a 3-D volume: `iterations` explicit steps over the 6 neighbours with the conductance
    1 / (1 + (g / K)^2) (`function` 'rational') or exp(-(g / K)^2) ('exponential'), g the difference to the neighbour over
    the spacing and K = `conductance` in intensity per unit of the spacing: differences well below K are smoothed away,
    edges well above it stay.  `timeStep` None is automatic, half the stability bound ``stabilityBound(spacing)``; a larger
    step than the bound is refused.  Returns float64.  float32 and float64 volumes go in as they are, anything else as
    float64; the voxels must be finite.  A tensor that lives on the GPU gives a float64 tensor on the same device."""
    dll = _lib()
    if function not in FUNCTIONS:
        raise ValueError("function: 'rational' or 'exponential'")
    iterations = int(iterations)
    if iterations < 1 or iterations > 1000:
        raise ValueError('iterations: 1 to 1000')
    K = float(conductance)
    if not (np.isfinite(K) and K > 0):
        raise ValueError('conductance: finite and positive')
    sp = None
    if spacing is not None:
        sp = np.ascontiguousarray(np.asarray(spacing, dtype=np.float64))
        if sp.shape != (3,):
            raise ValueError('spacing: three numbers, one per axis')
        if not (np.isfinite(sp).all() and (sp > 0).all()):
            raise ValueError('spacing: finite and positive')
    dt = 0.0 if timeStep is None else float(timeStep)
    if not np.isfinite(dt) or dt > stabilityBound(sp):
        raise ValueError('timeStep: finite and at most stabilityBound(spacing)')
    v, code, on_device = _volume(volume)
    args = (sp.ctypes.data if sp is not None else None, K, iterations, dt, FUNCTIONS[function])
    if on_device:
        import torch
        out = torch.empty(v.shape, dtype=torch.float64, device=v.device)
        torch.cuda.synchronize(v.device)
        _G._check(dll.vmask_diffuse(_G._dev_index(v), v.data_ptr(), code, *v.shape, *args, out.data_ptr()))
    else:
        out = np.empty(v.shape, np.float64)
        _G._check(dll.vmask_diffuse(device, v.ctypes.data, code, *v.shape, *args, out.ctypes.data))
    return out


def medianFilter(volume, radius=1, device=0):
    """scipy.ndimage.median_filter(volume, size=2 radius + 1, mode='nearest') for `radius` 0 or 1 per axis (an int or three
    ints): (1, 1, 0) is the in-plane 3 x 3 median of a thick-slice volume.  The median is one of the window's values, so the
    result is exact and integer data stay integer data.  float32 gives float32, everything else float64.  A tensor that lives
    on the GPU gives a tensor on the same device."""
    dll = _lib()
    r = np.asarray(radius)
    if r.ndim == 0:
        r = np.repeat(r, 3)
    if r.shape != (3,) or not all(x in (0, 1) for x in r.tolist()):
        raise ValueError('radius: 0 or 1, or three of them')
    r = [int(x) for x in r]
    v, code, on_device = _volume(volume)
    if on_device:
        import torch
        out = torch.empty_like(v)
        torch.cuda.synchronize(v.device)
        _G._check(dll.vmask_median(_G._dev_index(v), v.data_ptr(), code, *v.shape, *r, out.data_ptr()))
    else:
        out = np.empty_like(v)
        _G._check(dll.vmask_median(device, v.ctypes.data, code, *v.shape, *r, out.ctypes.data))
    return out


def main(baseFolder=None, method='diffusion', outputName=DENOISED_FILE, volumeName=BRAIN_FILE, **parameters):
    """File-level step in front of ``vesselness.main``: `volumeName` (``brainVolume.nii.gz``; the output of ``bias.main`` behind
    a bias-field correction) denoised by `method` 'diffusion'
    (``anisotropicDiffusion``; `parameters` must name `conductance`; the spacing is the norms of the affine's columns) or
    'median' (``medianFilter``), written as float32 `outputName` with the input's affine into the same folder.  Feed it on with
    ``vesselness.main(baseFolder, volumeName=outputName)``.  Returns the denoised volume."""
    if method not in ('diffusion', 'median'):
        raise ValueError("method: 'diffusion' or 'median'")
    if baseFolder is None:
        baseFolder = os.getcwd()
    volume, affine = loadVolume(baseFolder, volumeName)
    if method == 'diffusion':
        spacing = np.sqrt((np.asarray(affine, dtype=np.float64)[:3, :3] ** 2).sum(axis=0))
        result = anisotropicDiffusion(volume, spacing=spacing, **parameters)
    else:
        result = medianFilter(volume, **parameters)
    path = os.path.join(baseFolder, outputName)
    saveVolume(result, affine, path, astype=np.float32)
    print('{} saved to {}.'.format(outputName, path))
    return result
