"""Bias-field correction on the GPU: the "MR image bias field correction" step in front of ``denoise.main``.

The reference pipeline leaves this step to an external tool (its README, Pre-processing: "N4ITK MRI Bias correction") and holds
no code for it.  Here it is an N4-style estimate by a definition of our own - include/vmask.h ``vmask_bias_*``, DESIGN.md
section 9 entry f15: log domain, histogram sharpening by Wiener deconvolution, an incremental cubic B-spline fit of the
residual over a lattice that doubles per level - computed by HIP kernels; the 200-bin deconvolution runs on the host.
Agreement with ITK / Slicer is not claimed.  No CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import generateVesselVolume as _G
from .nifti import loadVolume, saveVolume
from .vesselness import BRAIN_FILE

CORRECTED_FILE = 'brainVolumeBiasCorrected.nii.gz'
MASK_FILE = 'brainVolumeMask.nii.gz'


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_bias_correct, 'argtypes', None):
        p, i64, d, i = C.c_void_p, C.c_int64, C.c_double, C.c_int
        dll.vmask_bias_axis_table.argtypes = [i, i, p, p, p, p]
        dll.vmask_bias_sharpen.argtypes = [p, i, d, d, d, d, p]
        dll.vmask_bias_fit.argtypes = [i, p, p, i64, i64, i64, p, p]
        dll.vmask_bias_eval.argtypes = [i, p, p, i64, i64, i64, p]
        dll.vmask_bias_log_field.argtypes = [i, p, p, i64, i64, i64, p, i, i, d, i, d, d, p, p, p]
        dll.vmask_bias_correct.argtypes = [i, p, i, p, i64, i64, i64, p, i, i, d, i, d, d, p, p, p, p]
    return dll


def _spans(spans, hi, name):
    s = np.asarray(spans)
    if s.shape != (3,) or not all(float(x).is_integer() and 1 <= x <= hi for x in s.tolist()):
        raise ValueError('{}: three whole numbers, 1 to {}'.format(name, hi))
    return np.ascontiguousarray(s.astype(np.intc))


def _positive(x, name):
    x = float(x)
    if not (np.isfinite(x) and x > 0):
        raise ValueError('{}: finite and positive'.format(name))
    return x


def _loop_args(splineSpans, levels, iterations, convergenceThreshold, bins, fwhm, noise):
    """What the host can check of the loop's parameters - the same conditions as the C entries."""
    m0 = _spans(splineSpans, 32, 'splineSpans')
    levels, iterations, bins = int(levels), int(iterations), int(bins)
    if levels < 1 or levels > 6:
        raise ValueError('levels: 1 to 6')
    if int(m0.max()) * 2 ** (levels - 1) > 64:
        raise ValueError('splineSpans * 2^(levels - 1): at most 64')
    if iterations < 1 or iterations > 200:
        raise ValueError('iterations: 1 to 200')
    if bins < 8 or bins > 256:
        raise ValueError('bins: 8 to 256')
    return m0, (levels, iterations, _positive(convergenceThreshold, 'convergenceThreshold'), bins, _positive(fwhm, 'fwhm'), _positive(noise, 'noise'))


def _volume(volume, floats):
    """(array or tensor as the library takes it, on the device?): the dtypes of `floats` go in as they are, others as float64."""
    if _G._on_device(volume):
        import torch
        if volume.dim() != 3:
            raise ValueError('expected a 3-D volume')
        v = volume.contiguous()
        if v.dtype not in [getattr(torch, np.dtype(f).name) for f in floats]:
            v = v.to(torch.float64)
        return v, True
    v = np.asarray(volume)
    if v.ndim != 3:
        raise ValueError('expected a 3-D volume')
    if v.dtype not in floats:
        v = v.astype(np.float64)
    return np.ascontiguousarray(v), False


def _mask(mask, like, on_device):
    """The mask as uint8 where the volume lives; its shape must be the volume's."""
    if on_device:
        import torch
        m = mask if _G._on_device(mask) else torch.as_tensor(np.asarray(mask), device=like.device)
        if tuple(m.shape) != tuple(like.shape):
            raise ValueError('mask: the shape of the volume')
        return (m != 0).to(torch.uint8).contiguous()
    if _G._on_device(mask):
        mask = mask.cpu().numpy()
    m = np.asarray(mask)
    if m.shape != tuple(like.shape):
        raise ValueError('mask: the shape of the volume')
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def _ptr(a, on_device):
    return a.data_ptr() if on_device else a.ctypes.data


def _empty(shape, like, on_device):
    if on_device:
        import torch
        return torch.empty(tuple(shape), dtype=torch.float64, device=like.device)
    return np.empty(tuple(shape), np.float64)


def _sync(t, on_device, device):
    if on_device:
        import torch
        torch.cuda.synchronize(t.device)
        return _G._dev_index(t)
    return device


def axisTable(n, spans):
    """The library's table of one axis of extent `n` with `spans` spans: (s[n] int32, w[n][4], c2[n][4], c3[n][4])."""
    n, spans = int(n), int(spans)
    if n < 1 or n > 32000 or spans < 1 or spans > 64:
        raise ValueError('an extent of 1 to 32000 and 1 to 64 spans')
    s = np.empty(n, np.int32)
    w, c2, c3 = (np.empty((n, 4), np.float64) for _ in range(3))
    _G._check(_lib().vmask_bias_axis_table(n, spans, s.ctypes.data, w.ctypes.data, c2.ctypes.data, c3.ctypes.data))
    return s, w, c2, c3


def sharpeningMap(counts, umin, umax, fwhm=0.15, noise=0.01):
    """The library's host function ``vmask_bias_sharpen``: for every bin of a histogram of log intensities (centres `umin` ..
    `umax`) the expected value of the sharpened intensity, the histogram deconvolved by a Gaussian of width `fwhm`."""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.float64))
    if c.ndim != 1 or c.size < 8 or c.size > 256:
        raise ValueError('counts: 8 to 256 bins')
    umin, umax = float(umin), float(umax)
    if not (np.isfinite(umin) and np.isfinite(umax) and umax > umin):
        raise ValueError('umin < umax, both finite')
    fwhm, noise = _positive(fwhm, 'fwhm'), _positive(noise, 'noise')
    E = np.empty(c.size, np.float64)
    _G._check(_lib().vmask_bias_sharpen(c.ctypes.data, c.size, umin, umax, fwhm, noise, E.ctypes.data))
    return E


def bsplineFit(residual, mask, spans, device=0):
    """``vmask_bias_fit``: the lattice of (spans + 3) control points per axis that approximates the float64 `residual` over
    `mask`; 0.0 where no mask voxel reaches a control point."""
    dll = _lib()
    M = _spans(spans, 64, 'spans')
    r, on_device = _volume(residual, (np.float64,))
    m = _mask(mask, r, on_device)
    phi = _empty([int(k) + 3 for k in M], r, on_device)
    dev = _sync(r, on_device, device)
    _G._check(dll.vmask_bias_fit(dev, _ptr(r, on_device), _ptr(m, on_device), *r.shape, M.ctypes.data, _ptr(phi, on_device)))
    return phi


def bsplineEval(phi, spans, shape, device=0):
    """``vmask_bias_eval``: the lattice `phi` of `spans` spans per axis evaluated at the voxels of a volume of `shape`."""
    dll = _lib()
    M = _spans(spans, 64, 'spans')
    shape = tuple(int(x) for x in shape)
    if len(shape) != 3:
        raise ValueError('shape: three extents')
    p, on_device = _volume(phi, (np.float64,))
    if tuple(p.shape) != tuple(int(k) + 3 for k in M):
        raise ValueError('phi: spans + 3 control points per axis')
    out = _empty(shape, p, on_device)
    dev = _sync(p, on_device, device)
    _G._check(dll.vmask_bias_eval(dev, _ptr(p, on_device), M.ctypes.data, *shape, _ptr(out, on_device)))
    return out


def logBiasField(logVolume, mask, splineSpans=(1, 1, 1), levels=3, iterations=20, convergenceThreshold=1e-3, bins=200, fwhm=0.15,
                 noise=0.01, device=0):
    """``vmask_bias_log_field``: the loop on float64 log intensities over `mask`.  Returns (b, trace): the log field, float64,
    and one row (level, max |phi|, umin, umax) per iteration that ran."""
    dll = _lib()
    m0, args = _loop_args(splineSpans, levels, iterations, convergenceThreshold, bins, fwhm, noise)
    v, on_device = _volume(logVolume, (np.float64,))
    m = _mask(mask, v, on_device)
    b = _empty(v.shape, v, on_device)
    trace = np.zeros((args[0] * args[1], 4), np.float64)
    count = C.c_int64(0)
    dev = _sync(v, on_device, device)
    _G._check(dll.vmask_bias_log_field(dev, _ptr(v, on_device), _ptr(m, on_device), *v.shape, m0.ctypes.data, *args, _ptr(b, on_device),
                                       trace.ctypes.data, C.addressof(count)))
    return b, trace[:count.value].copy()


def biasFieldCorrection(volume, mask=None, splineSpans=(1, 1, 1), levels=3, iterations=20, convergenceThreshold=1e-3, bins=200,
                        fwhm=0.15, noise=0.01, returnField=False, device=0):
    """N4-style correction of a smooth multiplicative intensity inhomogeneity: the volume divided by exp of a cubic B-spline
    field that is fitted, in the log domain, to the difference between the intensities and their sharpened histogram -
    `levels` lattices of `splineSpans` 2^level spans per axis, at most `iterations` steps on each, a level ending when its
    largest control-point update falls below `convergenceThreshold`.  `mask` None is volume > 0; voxels of a mask that are
    not positive leave it.  Returns float64, with `returnField` the pair (corrected, field).  float32 and float64 volumes go
    in as they are, anything else as float64.  A tensor that lives on the GPU gives tensors on the same device."""
    dll = _lib()
    m0, args = _loop_args(splineSpans, levels, iterations, convergenceThreshold, bins, fwhm, noise)
    v, on_device = _volume(volume, (np.float32, np.float64))
    code = 5 if (v.dtype == np.float32 if not on_device else v.element_size() == 4) else 6
    m = None if mask is None else _mask(mask, v, on_device)
    out = _empty(v.shape, v, on_device)
    field = _empty(v.shape, v, on_device) if returnField else None
    dev = _sync(v, on_device, device)
    _G._check(dll.vmask_bias_correct(dev, _ptr(v, on_device), code, None if m is None else _ptr(m, on_device), *v.shape, m0.ctypes.data, *args,
                                     _ptr(out, on_device), None if field is None else _ptr(field, on_device), None, None))
    return (out, field) if returnField else out


def main(baseFolder=None, outputName=CORRECTED_FILE, fieldName=None, **parameters):
    """File-level step in front of ``denoise.main``: ``brainVolume.nii.gz`` corrected by ``biasFieldCorrection`` over
    ``brainVolumeMask.nii.gz`` where the folder holds one (over the positive voxels where not), written as float32 `outputName`
    with the input's affine into the same folder, and the field as `fieldName` when that is given.  Feed it on with
    ``denoise.main(baseFolder, volumeName=outputName, ...)``.  Returns the corrected volume."""
    if baseFolder is None:
        baseFolder = os.getcwd()
    if 'returnField' in parameters or 'mask' in parameters:
        raise ValueError('main takes the mask from {} and the field by fieldName'.format(MASK_FILE))
    volume, affine = loadVolume(baseFolder, BRAIN_FILE)
    mask = None
    if os.path.exists(os.path.join(baseFolder, MASK_FILE)):
        mask, _ = loadVolume(baseFolder, MASK_FILE)
    result, field = biasFieldCorrection(volume, mask=mask, returnField=True, **parameters)
    path = os.path.join(baseFolder, outputName)
    saveVolume(result, affine, path, astype=np.float32)
    print('{} saved to {}.'.format(outputName, path))
    if fieldName is not None:
        path = os.path.join(baseFolder, fieldName)
        saveVolume(field, affine, path, astype=np.float32)
        print('{} saved to {}.'.format(fieldName, path))
    return result
