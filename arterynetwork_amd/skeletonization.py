"""Hand-off to the external skeletoniser.

The reference's ``skeletonization.analyze()`` (skeletonization.py:97-146) prepares three files for A. Tabb's
curve-skeleton tool before it starts the Docker image (:148-162, host plumbing outside this path).  This module
produces the same three files from a vessel mask; only their *format* is the contract:

``BB.txt``      three lines - ``1``, the lower corner ``0 0 0``, the upper corner = the volume's shape in the tool's
                axis order (z, y, x: the reference swaps axes 0 and 2 first); no trailing newline
``xyz.txt``     first line the number of vessel voxels, then one ``z y x`` row per voxel in raster order of the
                swapped volume, unsigned integers
``vesselVolumeMaskLabelInfo.npz``
                the 26-connected component labels of the swapped volume and the per-component (label, size) table,
                under the reference's key names (its later stages read them back)

Component labelling runs on the GPU (``vmask_label``).

The centrelines themselves - what the reference reads back from that tool and saves as ``skeleton.nii.gz`` (:783-790) -
are computed here on the GPU: ``skeletonize`` (``vmask_skeleton``: subfield-sequential thinning),
``skeletonRadii`` and the file-level ``main``.  They work in the caller's axis order; the axis swap above belongs to
the external tool's file format and is not applied.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import generateVesselVolume as _G
from .generateVesselVolume import labelVolume, loadVolume, saveVolume

RESULT_DIR = 'skeletonizationResult'
LABEL_CACHE = 'vesselVolumeMaskLabelInfo.npz'


def to_tool_axes(vesselVolumeMask):
    """Binary uint8 volume in the skeletoniser's (z, y, x) axis order."""
    return np.swapaxes((np.asarray(vesselVolumeMask) != 0).astype(np.uint8), 0, 2)


def write_bb(path, shape):
    """Bounding-box file: one box, from the origin to `shape`."""
    lines = ['1', '0 0 0', ' '.join(str(int(n)) for n in shape)]
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def write_xyz(path, mask):
    """Voxel list: count, then the coordinates of every non-zero voxel of `mask` in raster order."""
    coords = np.argwhere(mask)
    with open(path, 'w') as f:
        f.write('%d\n' % len(coords))
        np.savetxt(f, coords, fmt='%1u')
    return len(coords)


def write_label_cache(path, labeled, label_result):
    np.savez_compressed(path, vesselVolumeMaskLabeled=labeled, vesselVolumeMaskLabelResult=label_result)


def analyze_export(vesselVolumeMask, baseFolder, device=0):
    """Write BB.txt, xyz.txt and the label cache into <baseFolder>/skeletonizationResult; returns that directory."""
    mask = to_tool_axes(vesselVolumeMask)
    out_dir = os.path.join(baseFolder, RESULT_DIR)
    if not os.path.isdir(out_dir):
        os.makedirs(out_dir)
        print('Directory {} created.'.format(out_dir))
    labeled, label_result = labelVolume(mask, minSize=1, device=device)
    cache = os.path.join(out_dir, LABEL_CACHE)
    write_label_cache(cache, labeled, label_result)
    print('{} saved to {}.'.format(LABEL_CACHE, cache))
    write_bb(os.path.join(out_dir, 'BB.txt'), mask.shape)
    write_xyz(os.path.join(out_dir, 'xyz.txt'), mask)
    return out_dir


SKELETON_FILE = 'skeleton.nii.gz'


def _skeleton_lib():
    dll = _G._lib()
    if not getattr(dll.vmask_skeleton, 'argtypes', None):
        p, i64 = C.c_void_p, C.c_int64
        dll.vmask_skeleton.argtypes = [C.c_int, p, i64, i64, i64, p, C.POINTER(i64), C.POINTER(i64)]
    return dll


def skeletonize(vesselVolumeMask, device=0, info=None):
    """Curve skeleton of ``vesselVolumeMask != 0``: a uint8 0/1 volume of the same shape, a subset of the mask with the
    mask's 26-components, cavities and tunnels, one voxel thin, curve end points kept.  A tensor
    that lives on the GPU gives a uint8 tensor on the same device.  `info`, when a dict, receives ``kept`` (voxels left)
    and ``cycles`` (thinning cycles run)."""
    dll = _skeleton_lib()
    kept, cycles = C.c_int64(), C.c_int64()
    if _G._on_device(vesselVolumeMask):
        import torch
        m = _G._u8t(vesselVolumeMask)
        out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
        torch.cuda.synchronize(m.device)
        _G._check(dll.vmask_skeleton(_G._dev_index(m), m.data_ptr(), *m.shape, out.data_ptr(), C.byref(kept), C.byref(cycles)))
    else:
        m = _G._u8c(vesselVolumeMask)
        out = np.empty(m.shape, np.uint8)
        _G._check(dll.vmask_skeleton(device, m.ctypes.data, *m.shape, out.ctypes.data, C.byref(kept), C.byref(cycles)))
    if info is not None:
        info['kept'], info['cycles'] = kept.value, cycles.value
    return out


def skeletonRadii(skeleton, vesselVolumeMask, device=0):
    """Vessel radius at every skeleton voxel, by the convention of manualCorrectionGUI.py:248: the Euclidean distance
    transform of the mask (on the GPU) looked up at the voxel.  Returns (coords int64 N x 3 in raster order, radii float64 N)."""
    sk = np.asarray(skeleton.cpu() if _G._on_device(skeleton) else skeleton)
    if sk.ndim != 3:
        raise ValueError('expected a 3-D volume')
    dt = _G.distance_transform_edt(vesselVolumeMask, device=device)
    if _G._on_device(dt):
        dt = dt.cpu().numpy()
    if dt.shape != sk.shape:
        raise ValueError('skeleton and vesselVolumeMask must have the same shape')
    coords = np.argwhere(sk).astype(np.int64)
    return coords, dt[tuple(coords.T)].astype(np.float64)


def main(baseFolder=None):
    """File-level equivalent of what the reference's skeleton stage leaves behind (:783-790): the skeleton of
    ``vesselVolumeMask.nii.gz`` as ``skeleton.nii.gz`` (uint8, the mask's affine) in the same folder."""
    if baseFolder is None:
        baseFolder = os.getcwd()
    vesselVolumeMask, affine = loadVolume(baseFolder, 'vesselVolumeMask.nii.gz')
    skeleton = skeletonize(vesselVolumeMask)
    path = os.path.join(baseFolder, SKELETON_FILE)
    saveVolume(skeleton, affine, path, astype=np.uint8)
    print('{} saved to {}.'.format(SKELETON_FILE, path))
    return skeleton
