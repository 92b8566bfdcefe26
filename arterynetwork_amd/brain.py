"""Skull stripping on the GPU: ``headVolume.nii.gz`` -> ``brainVolumeMask.nii.gz`` and ``brainVolume.nii.gz``, the two files that
every voxel stage of the package reads.

The reference pipeline leaves this step to an external GUI tool (its README, Pre-processing: an atlas-based skull-stripping
plugin) and holds no code for it.  Here it is an atlas-free, edge-based extraction by a definition of our own, after the Brain
Surface Extractor recipe - include/vmask.h ``vmask_brain_*``, DESIGN.md section 9 entry f17 - computed by HIP kernels: an
optional Perona-Malik diffusion, an intensity floor from Otsu's threshold over a 256-bin histogram, Marr-Hildreth edges (the
scale-normalised Laplacian of Gaussian against ``edge`` times the contrast of the two classes), an opening around the main
6-connected component, a closing, and hole filling.  Agreement with the external tool is not claimed.  Only a brain that is
brighter than its surroundings is supported.  The edge term needs the diffusion on noisy data: without it, noise of a few
percent of the contrast lets the scalp and the brain merge (tests/brain_model.py measures it).  No CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import generateVesselVolume as _G
from .denoise import _volume, anisotropicDiffusion
from .nifti import loadVolume, saveVolume
from .vesselness import BRAIN_FILE

HEAD_FILE = 'headVolume.nii.gz'
MASK_FILE = 'brainVolumeMask.nii.gz'
STAGES = ('candidate', 'eroded', 'main', 'closed', 'final')
TIMED = ('edges', 'erosion', 'mainComponent', 'dilationClosing', 'fillHoles', 'unpack', 'sizePass')


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_brain_extract, 'argtypes', None):
        p, i64, d, i = C.c_void_p, C.c_int64, C.c_double, C.c_int
        dll.vmask_brain_histogram.argtypes = [i, p, i, i64, i64, i64, p, p, p]
        dll.vmask_brain_log.argtypes = [i, p, i, i64, i64, i64, p, d, p]
        dll.vmask_binary_morph.argtypes = [i, p, i64, i64, i64, i, i, i, p]
        dll.vmask_largest_component.argtypes = [i, p, i64, i64, i64, i, i64, p, p]
        dll.vmask_fill_holes.argtypes = [i, p, i64, i64, i64, p]
        dll.vmask_brain_extract.argtypes = [i, p, i, i64, i64, i64, p, d, d, d, i, i, i64, p, p, p]
    return dll


def _spacing(spacing):
    if spacing is None:
        return None
    sp = np.ascontiguousarray(np.asarray(spacing, dtype=np.float64))
    if sp.shape != (3,):
        raise ValueError('spacing: three numbers, one per axis')
    if not (np.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError('spacing: finite and positive')
    return sp


def _sigma(sigma, sp):
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError('sigma: finite and positive')
    for h in (np.ones(3) if sp is None else sp):
        rr = 4.0 * (sigma / h) + 0.5
        if not (1.0 <= rr < 65.0):
            raise ValueError('sigma: the tap radius int(4 sigma / spacing + 0.5) must lie in 1..64 on every axis')
    return sigma


def _steps(name, n, most):
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= most:
        raise ValueError('{}: an integer in 0..{}'.format(name, most))
    return int(n)


def _mask(mask):
    """(uint8 array or tensor, on the device?)  A contiguous uint8 volume goes in as it is: the library reads non-zero as set."""
    if _G._on_device(mask):
        import torch
        if mask.dim() == 3 and mask.dtype == torch.uint8 and mask.is_contiguous():
            return mask, True
        return _G._u8t(mask), True
    m = np.asarray(mask)
    if m.ndim == 3 and m.dtype == np.uint8 and m.flags.c_contiguous:
        return m, False
    return _G._u8c(mask), False


def _ptr(a, on_device):
    return a.data_ptr() if on_device else a.ctypes.data


def _like(v, on_device, dtype, lead=()):
    """A new array or tensor of v's shape (behind `lead`), where v lives."""
    shape = tuple(lead) + tuple(v.shape)
    if on_device:
        import torch
        out = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=v.device)
        torch.cuda.synchronize(v.device)
        return out
    return np.empty(shape, dtype)


def _index(v, on_device, device):
    return _G._dev_index(v) if on_device else device


def otsu(counts):
    """(t*, contrast in bins per t = 0..254) from 256 counts, in float64: the between-class variance
    (m W1 - (M - m) W0)^2 / (W0 W1), 0 where a class is empty; t* its first maximum; mu1 - mu0 at every t (0 where a class is
    empty)."""
    c = np.asarray(counts, dtype=np.float64)
    if c.shape != (256,):
        raise ValueError('counts: 256 numbers')
    k = np.arange(256, dtype=np.float64)
    W0 = np.cumsum(c)
    m = np.cumsum(k * c)
    N, M = W0[255], m[255]
    W0, m = W0[:255], m[:255]
    W1 = N - W0
    both = (W0 > 0) & (W1 > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        num = m * W1 - (M - m) * W0
        between = np.where(both, (num * num) / (W0 * W1), 0.0)
        gap = np.where(both, (M - m) / W1 - m / W0, 0.0)
    return int(np.argmax(between)), gap


def intensityFloor(volume, floor=None, device=0):
    """(floor, contrast, lo, hi, counts) of a volume: its extrema, the 256 counts of b = min(255, floor((v - lo) 256 / (hi - lo)))
    from the GPU, Otsu's threshold t* over them, floor = lo + (t* + 1) w and contrast = (mu1 - mu0) w, w the bin width, mu the
    class means in bins.  A given `floor` is kept, and the contrast is taken at the largest t with lo + (t + 1) w <= floor
    (clamped to 0..254).  A constant volume and voxels that are not finite are refused."""
    dll = _lib()
    if floor is not None and not np.isfinite(float(floor)):
        raise ValueError('floor: finite')
    v, code, on_device = _volume(volume)
    lohi = np.empty(2, np.float64)
    counts = np.zeros(256, np.uint64)
    if on_device:
        import torch
        torch.cuda.synchronize(v.device)
    _G._check(dll.vmask_brain_histogram(_index(v, on_device, device), _ptr(v, on_device), code, *v.shape,
                                        lohi[0:].ctypes.data, lohi[1:].ctypes.data, counts.ctypes.data))
    lo, hi = float(lohi[0]), float(lohi[1])
    w = (hi - lo) / 256.0
    t, gap = otsu(counts)
    if floor is None:
        floor = lo + (t + 1) * w
    else:
        floor = float(floor)
        ok = np.nonzero(lo + (np.arange(255, dtype=np.float64) + 1.0) * w <= floor)[0]
        t = int(ok[-1]) if len(ok) else 0
    return floor, float(gap[t] * w), lo, hi, counts


def laplacianOfGaussian(volume, sigma=1.0, spacing=None, device=0):
    """E = sum_a (sigma^2 / h_a^2) d_a^2 (G_sigma * volume), float64: the scale-normalised Laplacian of Gaussian with the taps of
    ``vesselness`` (radius int(4 sigma / h_a + 0.5), indices clamped at the faces).  A tensor that lives on the GPU gives a
    tensor on the same device."""
    dll = _lib()
    sp = _spacing(spacing)
    sigma = _sigma(sigma, sp)
    v, code, on_device = _volume(volume)
    out = _like(v, on_device, np.float64)
    _G._check(dll.vmask_brain_log(_index(v, on_device, device), _ptr(v, on_device), code, *v.shape,
                                  sp.ctypes.data if sp is not None else None, sigma, _ptr(out, on_device)))
    return out


def _morph(mask, op, steps, border, device):
    dll = _lib()
    steps = _steps('steps', steps, 100000)
    if border not in (0, 1):
        raise ValueError('border: 0 or 1')
    m, on_device = _mask(mask)
    out = _like(m, on_device, np.uint8)
    _G._check(dll.vmask_binary_morph(_index(m, on_device, device), _ptr(m, on_device), *m.shape, op, steps, int(border), _ptr(out, on_device)))
    return out


def binaryErosion(mask, steps=1, border=0, device=0):
    """scipy.ndimage.binary_erosion(mask, generate_binary_structure(3, 1), iterations=steps, border_value=border) as uint8:
    `steps` steps of the 6-neighbour cross, voxels outside the volume counting as `border` (0 or 1)."""
    return _morph(mask, 0, steps, border, device)


def binaryDilation(mask, steps=1, device=0):
    """scipy.ndimage.binary_dilation(mask, generate_binary_structure(3, 1), iterations=steps) as uint8."""
    return _morph(mask, 1, steps, 0, device)


def _seed(seed, shape):
    if seed is None:
        return -1
    s = tuple(seed)
    if len(s) != 3 or any(isinstance(x, bool) or int(x) != x for x in s) or not all(0 <= int(x) < n for x, n in zip(s, shape)):
        raise ValueError('seed: a voxel (i, j, k) of the volume')
    return int(np.ravel_multi_index(tuple(int(x) for x in s), tuple(shape)))


def largestComponent(mask, connectivity=1, seed=None, device=0, size=None):
    """The largest connected component of the mask as uint8 (`connectivity` 1, 2, 3: 6, 18, 26 neighbours); among equals the one
    that scipy.ndimage.label numbers first.  `seed` (i, j, k): the component that holds that voxel instead - an error when the
    voxel is not set.  `size`: a list that receives the component's number of voxels."""
    dll = _lib()
    if connectivity not in (1, 2, 3):
        raise ValueError('connectivity: 1, 2 or 3')
    m, on_device = _mask(mask)
    s = _seed(seed, m.shape)
    out = _like(m, on_device, np.uint8)
    n = C.c_int64(0)
    _G._check(dll.vmask_largest_component(_index(m, on_device, device), _ptr(m, on_device), *m.shape, int(connectivity), s,
                                          _ptr(out, on_device), C.addressof(n)))
    if size is not None:
        size.append(n.value)
    return out


def fillHoles(mask, device=0):
    """scipy.ndimage.binary_fill_holes(mask) as uint8."""
    dll = _lib()
    m, on_device = _mask(mask)
    out = _like(m, on_device, np.uint8)
    _G._check(dll.vmask_fill_holes(_index(m, on_device, device), _ptr(m, on_device), *m.shape, _ptr(out, on_device)))
    return out


def brainExtraction(volume, sigma=1.0, edge=0.05, floor=None, erosion=1, closing=1, diffusion=None, spacing=None, seed=None, device=0, info=None):
    """The brain mask (uint8) of a head volume.

    `diffusion` dict(conductance=..., iterations=...): ``denoise.anisotropicDiffusion`` first (needed on noisy data, see the
    module's text).  Then the voxels above the `floor` (None: Otsu's threshold, ``intensityFloor``) whose Laplacian of Gaussian
    at `sigma` (units of the `spacing`) is at most `edge` times the contrast; `erosion` steps of erosion, the largest 6-connected
    component (or the one that holds `seed` = (i, j, k)), `erosion` steps of dilation; `closing` steps of closing; the holes
    filled.  `info`: a dict that receives floor, contrast, lo, hi, the voxel counts of the five stages (``STAGES``), the
    number of components after the erosion, the kept one's size, the peak of the call's device allocations and the microseconds
    of the stages (``TIMED``, between HIP events); info['stages'] = True on entry asks
    for the five stage volumes as well.  A tensor that lives on the GPU stays there and gives a tensor on the same device."""
    dll = _lib()
    sp = _spacing(spacing)
    sigma = _sigma(sigma, sp)
    edge = float(edge)
    if np.isnan(edge):
        raise ValueError('edge: a number')
    if floor is not None and not np.isfinite(float(floor)):
        raise ValueError('floor: finite')
    erosion, closing = _steps('erosion', erosion, 1000), _steps('closing', closing, 1000)
    if diffusion is not None and not (isinstance(diffusion, dict) and 'conductance' in diffusion and set(diffusion) <= {'conductance', 'iterations', 'timeStep', 'function'}):
        raise ValueError("diffusion: a dict with 'conductance' and optionally 'iterations', 'timeStep', 'function'")
    if info is not None and not isinstance(info, dict):
        raise ValueError('info: a dict')
    v, code, on_device = _volume(volume)
    s = _seed(seed, v.shape)
    J = v
    if diffusion is not None:
        J = anisotropicDiffusion(v, spacing=sp, device=device, **diffusion)
        code = 6
    fl, contrast, lo, hi, _ = intensityFloor(J, floor, device=device)
    threshold = edge * contrast
    if np.isnan(threshold):
        raise ValueError('edge: edge times the contrast is not a number')
    out = _like(J, on_device, np.uint8)
    want_stages = bool(info is not None and info.get('stages'))
    stages = _like(J, on_device, np.uint8, lead=(5,)) if want_stages else None
    numbers = np.zeros(16, np.int64)
    _G._check(dll.vmask_brain_extract(_index(J, on_device, device), _ptr(J, on_device), code, *J.shape, sp.ctypes.data if sp is not None else None,
                                      sigma, threshold, fl, erosion, closing, s, _ptr(out, on_device),
                                      _ptr(stages, on_device) if want_stages else None, numbers.ctypes.data))
    if info is not None:
        info.update(floor=fl, contrast=contrast, lo=lo, hi=hi, threshold=threshold, counts={k: int(n) for k, n in zip(STAGES, numbers[:5])},
                    components=int(numbers[6]), mainSize=int(numbers[7]), peakBytes=int(numbers[5]),
                    microseconds=dict(zip(TIMED, (int(x) for x in numbers[8:15]))))
        if want_stages:
            info['stages'] = {k: stages[i] for i, k in enumerate(STAGES)}
    return out


def main(baseFolder=None, headName=HEAD_FILE, maskName=MASK_FILE, brainName=BRAIN_FILE, **parameters):
    """File-level step in front of ``bias.main`` / ``denoise.main`` / ``vesselness.main``: `headName` (the head volume as
    acquired) -> `maskName` (uint8, ``brainExtraction`` with `parameters`; the spacing is the norms of the affine's columns) and
    `brainName` (float32: the head volume times the mask), both with the input's affine, in the same folder.  Returns the mask."""
    if 'spacing' in parameters:
        raise ValueError('spacing: taken from the affine of the file')
    if baseFolder is None:
        baseFolder = os.getcwd()
    volume, affine = loadVolume(baseFolder, headName)
    spacing = np.sqrt((np.asarray(affine, dtype=np.float64)[:3, :3] ** 2).sum(axis=0))
    mask = brainExtraction(volume, spacing=spacing, **parameters)
    path = os.path.join(baseFolder, maskName)
    saveVolume(mask, affine, path, astype=np.uint8)
    print('{} saved to {}.'.format(maskName, path))
    path = os.path.join(baseFolder, brainName)
    saveVolume(np.asarray(volume) * mask, affine, path, astype=np.float32)
    print('{} saved to {}.'.format(brainName, path))
    return mask
