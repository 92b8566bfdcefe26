"""Multiscale Hessian vesselness filter on the GPU: the step that produces ``vesselnessFiltered.nii.gz``.

The reference pipeline gets this volume from an external GUI tool (3D Slicer / VMTK, README.md:61-67) and holds no code
for it; ``generateVesselVolume.main`` reads the file next.  Here it is Frangi's measure (Frangi et al. 1998) by a
definition of our own - include/vmask.h ``vmask_vesselness``, DESIGN.md section 9 entry f7 - computed in float64 by HIP
kernels; the README's "suppress plates / suppress blobs / vessel contrast" are alpha / beta / gamma.  Agreement with the
external tool's output is not claimed: its discretisation differs.  No CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import generateVesselVolume as _G
from .nifti import loadVolume, saveVolume

VESSELNESS_FILE = 'vesselnessFiltered.nii.gz'
BRAIN_FILE = 'brainVolume.nii.gz'
BRAIN_MASK_FILE = 'brainVolumeMask.nii.gz'


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_vesselness, 'argtypes', None):
        p, i64, d = C.c_void_p, C.c_int64, C.c_double
        dll.vmask_vesselness.argtypes = [C.c_int, p, C.c_int, i64, i64, i64, p, p, C.c_int, p, d, d, d, C.c_int, p, p, p]
    return dll


def sigmasFromDiameters(minDiameter, maxDiameter, steps):
    """`steps` scales, logarithmically spaced, for vessels of diameter `minDiameter` .. `maxDiameter` (in the units of the
    spacing): sigma = diameter / 2.  This is the package's own policy - the reference only names the external tool's
    minimum / maximum vessel diameter parameters - chosen because a tube with a Gaussian profile of width s responds most
    at sigma = s."""
    steps = int(steps)
    if steps < 1 or not (np.isfinite(minDiameter) and np.isfinite(maxDiameter)) or minDiameter <= 0 or maxDiameter < minDiameter:
        raise ValueError('sigmasFromDiameters: 0 < minDiameter <= maxDiameter, steps >= 1')
    if steps == 1:
        return np.array([0.5 * minDiameter])
    return 0.5 * np.exp(np.linspace(np.log(minDiameter), np.log(maxDiameter), steps))


def vesselnessFilter(volume, sigmas, alpha=0.5, beta=0.5, gamma=None, brainVolumeMask=None, spacing=None, bright=True, device=0, info=None):
    """Frangi vesselness of a 3-D volume, the maximum over the scales `sigmas` (physical units; `spacing` per axis, default
    1): a float64 array in [0, 1], 0 outside `brainVolumeMask` when one is given.  `gamma` None (or <= 0) is automatic:
    per scale, half the largest Frobenius norm of the scaled Hessian over the (masked) volume.  `bright` False looks for
    dark vessels.  float32 and float64 volumes go in as they are, anything else as float64; the voxels must be finite.  A
    tensor that lives on the GPU gives a float64 tensor on the same device.  `info`, when a dict, receives ``gammas``
    (the gamma used per scale) and, when it holds the key ``scale`` beforehand, ``scale``: per voxel the index of the first
    scale that attains the maximum (uint8; 0 where the result is 0)."""
    dll = _lib()
    sig = np.ascontiguousarray(np.atleast_1d(np.asarray(sigmas, dtype=np.float64)))
    if sig.ndim != 1 or sig.size < 1:
        raise ValueError('sigmas: a non-empty sequence of scales')
    sp = None
    if spacing is not None:
        sp = np.ascontiguousarray(np.asarray(spacing, dtype=np.float64))
        if sp.shape != (3,):
            raise ValueError('spacing: three numbers, one per axis')
    g = 0.0 if gamma is None else float(gamma)
    gammas = np.zeros(sig.size, np.float64)
    want_scale = info is not None and 'scale' in info
    if _G._on_device(volume):
        import torch
        if volume.dim() != 3:
            raise ValueError('expected a 3-D volume')
        v = volume.contiguous()
        if v.dtype not in (torch.float32, torch.float64):
            v = v.to(torch.float64)
        m = None
        if brainVolumeMask is not None:
            m = _G._u8t(brainVolumeMask if _G._on_device(brainVolumeMask) else torch.as_tensor(np.asarray(brainVolumeMask), device=v.device))
            if tuple(m.shape) != tuple(v.shape):
                raise ValueError('brainVolumeMask and volume must have the same shape')
        out = torch.empty(v.shape, dtype=torch.float64, device=v.device)
        scale = torch.empty(v.shape, dtype=torch.uint8, device=v.device) if want_scale else None
        torch.cuda.synchronize(v.device)
        _G._check(dll.vmask_vesselness(_G._dev_index(v), v.data_ptr(), 5 if v.dtype == torch.float32 else 6, *v.shape,
                                       m.data_ptr() if m is not None else None, sig.ctypes.data, sig.size,
                                       sp.ctypes.data if sp is not None else None, float(alpha), float(beta), g, 1 if bright else 0,
                                       out.data_ptr(), scale.data_ptr() if want_scale else None, gammas.ctypes.data))
    else:
        v = np.asarray(volume)
        if v.ndim != 3:
            raise ValueError('expected a 3-D volume')
        if v.dtype not in (np.float32, np.float64):
            v = v.astype(np.float64)
        v = np.ascontiguousarray(v)
        m = None
        if brainVolumeMask is not None:
            m = _G._u8c(brainVolumeMask)
            if m.shape != v.shape:
                raise ValueError('brainVolumeMask and volume must have the same shape')
        out = np.empty(v.shape, np.float64)
        scale = np.empty(v.shape, np.uint8) if want_scale else None
        _G._check(dll.vmask_vesselness(device, v.ctypes.data, 5 if v.dtype == np.float32 else 6, *v.shape,
                                       m.ctypes.data if m is not None else None, sig.ctypes.data, sig.size,
                                       sp.ctypes.data if sp is not None else None, float(alpha), float(beta), g, 1 if bright else 0,
                                       out.ctypes.data, scale.ctypes.data if want_scale else None, gammas.ctypes.data))
    if info is not None:
        info['gammas'] = gammas
        if want_scale:
            info['scale'] = scale
    return out


def main(baseFolder=None, sigmas=(0.5, 1.0, 1.5, 2.0), alpha=0.5, beta=0.5, gamma=None, bright=True, volumeName=BRAIN_FILE):
    """File-level step in front of ``generateVesselVolume.main``: the vesselness of ``brainVolume.nii.gz`` (or `volumeName`,
    ``denoise.main``'s output for one) - inside
    ``brainVolumeMask.nii.gz`` when that file exists - written as float32 ``vesselnessFiltered.nii.gz`` with the input's
    affine into the same folder; `sigmas` in the units of the affine (millimetres), the voxel spacing being the norms of the
    affine's columns.  Returns the float64 volume."""
    if baseFolder is None:
        baseFolder = os.getcwd()
    volume, affine = loadVolume(baseFolder, volumeName)
    mask = None
    if os.path.exists(os.path.join(baseFolder, BRAIN_MASK_FILE)):
        mask, _ = loadVolume(baseFolder, BRAIN_MASK_FILE)
    spacing = np.sqrt((np.asarray(affine, dtype=np.float64)[:3, :3] ** 2).sum(axis=0))
    ves = vesselnessFilter(volume, sigmas, alpha=alpha, beta=beta, gamma=gamma, brainVolumeMask=mask, spacing=spacing, bright=bright)
    path = os.path.join(baseFolder, VESSELNESS_FILE)
    saveVolume(ves, affine, path, astype=np.float32)
    print('{} saved to {}.'.format(VESSELNESS_FILE, path))
    return ves
