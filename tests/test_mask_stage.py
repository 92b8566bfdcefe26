"""Stage-1 voxel passes: GPU EDT / component labelling / vessel-mask pipeline / skeletoniser
export against the CPU oracle (oracle/mask_oracle.py: scipy.ndimage, the reference's own dependency)."""
import os

import numpy as np
import pytest

from oracle import mask_oracle as MO


def _volumes(seed, shape):
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    c = [(n - 1) / 2.0 for n in shape]
    brain = (((x - c[0]) / (0.45 * shape[0])) ** 2 + ((y - c[1]) / (0.45 * shape[1])) ** 2
             + ((z - c[2]) / (0.45 * shape[2])) ** 2) <= 1.0
    tube = ((y - c[1] - 0.2 * shape[1] * np.sin(2 * np.pi * x / shape[0])) ** 2 + (z - c[2]) ** 2) <= 6.0
    tube2 = ((x - 0.3 * shape[0]) ** 2 + (y - 0.6 * shape[1]) ** 2) <= 4.0
    ves = (tube | tube2).astype(np.float32) + 0.25 * rng.random(shape).astype(np.float32)
    ves[rng.random(shape) < 0.002] = 1.2          # specks: small components to be dropped
    return brain.astype(np.uint8), ves


# ------------------------------------------------------------------ CPU: the oracle itself
def test_oracle_pipeline_properties():
    brain, ves = _volumes(0, (40, 36, 30))
    m = MO.vesselVolumeMask(brain, ves)
    assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1} and 50 < m.sum() < m.size // 4
    lab, res = MO.labelVolume(m)
    assert all(size > 150 for label, size in res if label != 0)      # :197-199
    assert res[0][0] == 0 and sum(s for _, s in res) == m.size       # bincount includes the background (:131-134)
    edt = MO.distance_transform_edt(brain)
    assert edt[brain == 0].max() == 0 and edt.max() > 5


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(40, 36, 30), (17, 64, 9), (1, 50, 33), (96, 80, 72), (3, 700, 5), (2, 6, 900), (130, 150, 140),
                                   (37, 9, 7), (70, 5, 6),       # (rows of 63 / 30 voxels: the axis-0 scans one column per thread, whole batches + a tail)
                                   (2, 3, 20000), (2, 20000, 3), # (the longest lines of the 32-bit envelope pass: quotients near 2^15, numerators near 2^30)
                                   (2, 5, 23200),       # (squared diagonal >= 2^29: the envelope pass in 64-bit arithmetic)
                                   (20000, 3, 2), (20011, 3, 2)])      # (a long axis 0: the scans run hundreds of whole batches of 32 / 16 rows; 20011: and a tail of 11)
def test_edt_bit_exact(shape):
    from arterynetwork_amd.generateVesselVolume import distance_transform_edt
    brain, _ = _volumes(1, shape)
    rng = np.random.default_rng(2)
    # (long lines with few zeros: the envelope stacks get deeper than the part of them the kernel keeps in LDS)
    for mask in (brain, (rng.random(shape) < 0.97).astype(np.uint8), (rng.random(shape) < 0.5).astype(np.uint8),
                 (rng.random(shape) < 0.9995).astype(np.uint8), np.ones(shape, np.uint8) * (np.arange(shape[1])[None, :, None] > 0)):
        if mask.all():                  # (a volume without a zero voxel has no distance transform: scipy's answer is arbitrary)
            mask = mask.copy(); mask.flat[mask.size // 3] = 0
        got = distance_transform_edt(mask)
        ref = MO.distance_transform_edt(mask)
        assert got.dtype == np.float64 and np.array_equal(got, ref)      # sqrt of the exact integer squared distance


@pytest.mark.gpu
def test_edt_random_shapes():
    """Sixty random small volumes (every dimension 1..70, zero fractions from one voxel to most of the volume, solid blocks
    with holes): the distances are scipy's, bit for bit - row lengths of every residue modulo 4 and 64, lines shorter and
    longer than a batch of the envelope pass, columns with and without a zero."""
    from arterynetwork_amd.generateVesselVolume import distance_transform_edt
    rng = np.random.default_rng(77)
    for case in range(60):
        shape = tuple(int(v) for v in rng.integers(1, 71, 3))
        kind = case % 4
        if kind == 0:
            mask = (rng.random(shape) < rng.choice([0.3, 0.8, 0.97, 0.995])).astype(np.uint8)
        elif kind == 1:
            mask = np.ones(shape, np.uint8)
            for _ in range(int(rng.integers(1, 4))):
                mask[tuple(int(rng.integers(0, n)) for n in shape)] = 0
        elif kind == 2:
            mask = np.zeros(shape, np.uint8)
            lo = [int(rng.integers(0, max(1, n // 2))) for n in shape]
            mask[lo[0]:, lo[1]:, lo[2]:] = 1                       # a solid block against three faces of the volume
            mask[rng.random(shape) < 0.002] = 0
        else:
            mask = (rng.random(shape) < 0.9).astype(np.uint8)
            mask[:, :, shape[2] // 2] = 1                          # a plane without a zero
        if mask.all():
            mask.flat[mask.size // 3] = 0
        got = distance_transform_edt(mask)
        assert np.array_equal(got, MO.distance_transform_edt(mask)), (case, shape, kind)


@pytest.mark.gpu
@pytest.mark.parametrize('maxHop', [1, 2, 3])
def test_label_volume_matches_raster_numbering(maxHop):
    from arterynetwork_amd.generateVesselVolume import labelVolume
    rng = np.random.default_rng(3)
    for shape, p in (((30, 28, 26), 0.25), ((9, 70, 5), 0.45), ((64, 64, 48), 0.12)):
        vol = (rng.random(shape) < p).astype(int)
        lab, res = labelVolume(vol, maxHop=maxHop)
        olab, ores = MO.labelVolume(vol, maxHop=maxHop)
        assert np.array_equal(lab, olab)
        assert res == ores
    lab, res = labelVolume(np.zeros((4, 5, 6), int))
    assert lab.max() == 0 and res == [(0, 120)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_vessel_mask_pipeline(dtype, capsys):
    from arterynetwork_amd.generateVesselVolume import vesselVolumeMask
    for seed, shape in ((0, (40, 36, 30)), (5, (72, 64, 56))):
        brain, ves = _volumes(seed, shape)
        ves = ves.astype(dtype)
        got = vesselVolumeMask(brain * 7, ves)            # any non-zero value means "inside the brain"
        ref = MO.vesselVolumeMask(brain, ves)
        assert got.dtype == np.uint8 and np.array_equal(got, ref)
        assert 'Number of voxels in segmentation: {}'.format(int(ref.sum())) in capsys.readouterr().out


@pytest.mark.gpu
def test_skeletoniser_export(tmp_path):
    from arterynetwork_amd.skeletonization import analyze_export
    brain, ves = _volumes(0, (40, 36, 30))
    mask = MO.vesselVolumeMask(brain, ves) * 255
    d = analyze_export(mask, str(tmp_path))
    sw = np.swapaxes((mask != 0).astype(np.uint8), 0, 2)
    assert open(os.path.join(d, 'BB.txt')).read() == '1\n0 0 0\n{} {} {}'.format(*sw.shape)
    lines = open(os.path.join(d, 'xyz.txt')).read().splitlines()
    coords = np.array(np.where(sw)).T
    assert int(lines[0]) == len(coords) == len(lines) - 1
    assert lines[1] == '{} {} {}'.format(*coords[0]) and lines[-1] == '{} {} {}'.format(*coords[-1])
    z = np.load(os.path.join(d, 'vesselVolumeMaskLabelInfo.npz'))
    olab, ores = MO.labelVolume(sw)
    assert np.array_equal(z['vesselVolumeMaskLabeled'], olab)
    assert [tuple(r) for r in z['vesselVolumeMaskLabelResult']] == ores


@pytest.mark.gpu
def test_vessel_distance_transform_cache(tmp_path):
    """Row f4: the distance transform of the vessel mask under the reference's cache file name and key; radius look-up."""
    from arterynetwork_amd.generateVesselVolume import vesselDistanceTransform, DISTANCE_CACHE
    brain, ves = _volumes(3, (40, 36, 30))
    mask = MO.vesselVolumeMask(brain, ves)
    ref = MO.distance_transform_edt(mask)
    dt = vesselDistanceTransform(mask, str(tmp_path))
    assert np.array_equal(dt, ref)
    z = np.load(os.path.join(str(tmp_path), DISTANCE_CACHE))
    assert list(z.keys()) == ['distanceTransform'] and np.array_equal(z['distanceTransform'], ref)
    again = vesselDistanceTransform(np.zeros_like(mask), str(tmp_path))          # (the cache wins, as in the reference)
    assert np.array_equal(again, ref)
    coords = np.argwhere(mask)[::50]
    assert np.array_equal(dt[tuple(coords.T)], ref[tuple(coords.T)]) and (dt[tuple(coords.T)] >= 1).all()


@pytest.mark.gpu
def test_nifti_main_round_trip(tmp_path):
    from arterynetwork_amd import nifti, generateVesselVolume as G
    brain, ves = _volumes(7, (48, 40, 32))
    aff = np.diag([0.4, 0.4, 0.6, 1.0])
    nifti.saveVolume(ves * 100, aff, str(tmp_path / '401 3D MRA BRAIN.nii.gz'), astype=np.float32)
    nifti.saveVolume(brain, aff, str(tmp_path / 'brainVolumeMask.nii.gz'))
    nifti.saveVolume(ves, aff, str(tmp_path / 'vesselnessFiltered.nii.gz'), astype=np.float32)
    m = G.main(str(tmp_path))
    out, aff2 = nifti.loadVolume(str(tmp_path), 'vesselVolumeMask.nii.gz')
    assert out.dtype == np.uint8 and np.array_equal(out, m) and np.allclose(aff2, aff)
    assert np.array_equal(m, MO.vesselVolumeMask(brain, ves))


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import generateVesselVolume as G
rng = np.random.default_rng(12)
shape = (40, 36, 31)
ves = rng.random(shape).astype(np.float32)
brain = np.zeros(shape, np.uint8); brain[3:-3, 4:-2, 2:-4] = 1
dev = torch.device('cuda', 0)
m_host = G.vesselVolumeMask(brain, ves, minSize=5)
m_dev = G.vesselVolumeMask(torch.as_tensor(brain, device=dev), torch.as_tensor(ves, device=dev), minSize=5)
assert m_dev.is_cuda and m_dev.dtype == torch.uint8 and np.array_equal(m_dev.cpu().numpy(), m_host)
assert m_host.sum() > 0
lab_h, res_h = G.labelVolume(m_host)
lab_d, res_d = G.labelVolume(m_dev)
assert lab_d.is_cuda and np.array_equal(lab_d.cpu().numpy().astype(np.int64), lab_h) and res_d == res_h
d_h = G.distance_transform_edt(m_host)
d_d = G.distance_transform_edt(m_dev)
assert d_d.is_cuda and np.array_equal(d_d.cpu().numpy(), d_h)
# (a mask that starts at an odd device address: the 4-voxel accesses of the axis-0 scans do not apply)
flat = torch.zeros(m_dev.numel() + 1, dtype=torch.uint8, device=dev)
odd = flat[1:].view(m_dev.shape); odd.copy_(m_dev)
out = torch.empty(odd.shape, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
assert odd.data_ptr() % 4 != 0 and G._lib().vmask_edt(0, odd.data_ptr(), *odd.shape, out.data_ptr()) == 0
assert np.array_equal(out.cpu().numpy(), d_h)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_device_resident_volumes_in_and_out():
    """Tensors that live on the GPU go to the C-ABI by their device pointers and the results stay on the GPU: the same
    mask, labels and distances as with host arrays (no PCIe round trip per call).  Own process: torch is imported
    before the HIP library there."""
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, '-c', DEVICE_RESIDENT_SCRIPT.format(root=ROOT)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
