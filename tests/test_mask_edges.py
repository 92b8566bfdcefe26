"""Directed edge cases for the stage-1 voxel passes (vmask_device.hip): component labelling on structured volumes,
device pointers that are not aligned (inside guard bands), the 4-loads-in-flight loop of the min/max reduction, and every
comparison of the vessel-mask pipeline at its boundary (x <= thr1, x <= thr2, sqrt(G) <= edtMax, size > minSize).

References are oracle/mask_oracle.py (scipy.ndimage) and plain numpy; every comparison is exact.  The inputs are built by
the functions at the top of this file and the CPU tests below check that each of them is what it claims to be (component
counts, ties that survive the dtype, distances that are hit exactly), so a GPU test cannot pass on a degenerate input.

Not tested here, on purpose:
  * NaN vesselness: numpy propagates a NaN through amin / amax (every threshold becomes NaN), the reduction kernel's
    `x < lo` comparisons skip it - the two disagree by construction and the reference never feeds one in.
  * a brain mask without any zero voxel: it has no distance transform, scipy's answer there is arbitrary.
"""
import math

import numpy as np
import pytest

from oracle import mask_oracle as MO

HOPS = [1, 2, 3]


# ------------------------------------------------------------------ section 1: structured volumes for the labelling
def _serpentine(shape=(12, 14, 70)):
    """One 6-connected boustrophedon path: along i2, a step in i1 at the row end, a step in i0 at the plane end; every
    other row and every other plane stays empty.  Returns the volume and the path (in walking order)."""
    n0, n1, n2 = shape
    rows, path, cur = list(range(0, n1, 2)), [], 0
    for k, i0 in enumerate(range(0, n0, 2)):
        order = rows if k % 2 == 0 else rows[::-1]
        for r, i1 in enumerate(order):
            if r:
                path.append((i0, (i1 + order[r - 1]) // 2, cur))
            path += [(i0, i1, j) for j in (range(n2) if cur == 0 else range(n2 - 1, -1, -1))]
            cur = n2 - 1 - cur
        if i0 + 2 < n0:
            path.append((i0 + 1, order[-1], cur))
    v = np.zeros(shape, np.uint8)
    v[tuple(np.array(path).T)] = 1
    return v, path


def _comb(shape=(20, 21, 22)):
    """Two combs.  The first: teeth along i0 on a grid of every other (i1, i2), joined only by a plate in the last plane
    i0 = n0-1.  The second: teeth along i0 that turn along i1 in the last plane and meet only in its last row.  Every
    tooth starts as a provisional root of its own at i0 = 0; all of them collapse at the very end of the raster order."""
    n0, n1, n2 = shape
    v = np.zeros(shape, np.uint8)
    h = n2 // 2
    v[:, 0:n1 - 4:2, 0:h - 1:2] = 1
    v[n0 - 1, 0:n1 - 4, 0:h - 1] = 1
    bs = list(range(h + 1, n2, 2))
    for k, b in enumerate(bs):
        a = 1 + 3 * k
        assert a < n1 - 1
        v[:, a, b] = 1
        v[n0 - 1, a:, b] = 1
    v[n0 - 1, n1 - 1, bs[0]:] = 1
    return v


def _diagonals(shape=(10, 10, 12)):
    """The anti-raster face diagonals i1 = n1-1-i0 (in the plane i2 = n2-1) and i2 = n2-1-i1 (in the plane i0 = 0):
    connected from maxHop = 2; and the body diagonal, connected only at maxHop = 3."""
    n0, n1, n2 = shape
    n = min(n0, n1)
    t = np.arange(n)
    v = np.zeros(shape, np.uint8)
    v[t, n1 - 1 - t, n2 - 1] = 1
    v[0, t, n2 - 1 - t] = 1
    v[t, t, t] = 1
    return v, n


def _checkerboard(shape):
    i = np.indices(shape).sum(0)
    return (i % 2 == 0).astype(np.uint8)


def _lattice(shape=(96, 96, 64)):
    v = np.zeros(shape, np.uint8)
    v[::2, ::2, ::2] = 1
    return v


TINY_SHAPES = [(1, 1, 63), (1, 1, 64), (1, 1, 65), (1, 2, 2), (1, 65, 1), (65, 1, 1),
               (1, 1, 129), (1, 2, 65), (1, 1, 131),          # V % 4 = 1, 2, 3, and a voxel 127 and 128
               (1, 7, 32)]                                    # (0, 63, 64, 127, 128 and V-1 are all isolated here)


def _tiny_volumes():
    """(name, volume): voxels exactly at the flat indices 0, 63, 64, 127, 128 and V-1 - the bits 0 and 63 of a word of the
    root bitmap, and the last voxel of a partly filled last word - all together, the two ends of a word apart, and the
    last voxel alone."""
    out = [('1x1x1-zero', np.zeros((1, 1, 1), np.uint8)), ('1x1x1-one', np.ones((1, 1, 1), np.uint8))]
    for shape in TINY_SHAPES:
        V = int(np.prod(shape))
        for tag, idx in (('all', (0, 63, 64, 127, 128, V - 1)), ('bit63', (0, 63, 127, V - 1)), ('bit0', (64, 128)), ('last', (V - 1,))):
            idx = sorted({i for i in idx if 0 <= i < V})
            if not idx:
                continue
            v = np.zeros(V, np.uint8)
            v[idx] = 1
            out.append(('{}-{}'.format('x'.join(map(str, shape)), tag), v.reshape(shape)))
    return out


def _no_wrap(shape):
    """Voxels that are neighbours in memory and not in space: the last voxel of a row and the first of the next one, the
    last of a plane and the first of the next one; and the first and last voxel of every other row."""
    n0, n1, n2 = shape
    a = np.zeros((n0 * n1, n2), np.uint8)
    a[0::2, n2 - 1] = 1
    a[1::2, 0] = 1
    b = np.zeros(shape, np.uint8)
    b[0::2, n1 - 1, n2 - 1] = 1
    b[1::2, 0, 0] = 1
    c = np.zeros((n0 * n1, n2), np.uint8)
    c[0::2, 0] = 1
    c[0::2, n2 - 1] = 1
    return [a.reshape(shape), b, c.reshape(shape)]


def _flip(v):
    return np.ascontiguousarray(v[::-1, ::-1, ::-1])


def _label_cases():
    cases = {}
    s, _ = _serpentine()
    cases['serpentine'] = s
    cases['serpentine-reversed'] = _flip(s)
    c = _comb()
    cases['comb'] = c
    cases['comb-reversed'] = _flip(c)
    cases['comb-along-i2'] = np.ascontiguousarray(c.transpose(2, 1, 0))      # (the teeth along i2, joined in the last column)
    cases['diagonals'] = _diagonals()[0]
    cases['checkerboard-5x7x9'] = _checkerboard((5, 7, 9))
    cases['checkerboard-4x6x8'] = _checkerboard((4, 6, 8))
    cases['ones-64x64x48'] = np.ones((64, 64, 48), np.uint8)
    cases['ones-3x5x7'] = np.ones((3, 5, 7), np.uint8)
    for name, v in _tiny_volumes():
        cases['tiny-' + name] = v
    cases['lattice-96x96x64'] = _lattice()
    for shape in ((6, 5, 2), (6, 2, 5), (2, 6, 5)):
        for k, v in enumerate(_no_wrap(shape)):
            cases['nowrap-{}-{}'.format('x'.join(map(str, shape)), 'abc'[k])] = v
    return cases


LABEL_CASES = _label_cases()


def _ncomp(v, hop):
    return len([1 for label, size in MO.labelVolume(v, maxHop=hop)[1] if label != 0])


# ------------------------------------------------------------------ CPU: the inputs are what they claim to be
def test_serpentine_is_one_long_path():
    v, path = _serpentine()
    p = np.array(path)
    assert len(set(path)) == len(path) == int(v.sum())
    assert (np.abs(np.diff(p, axis=0)).sum(1) == 1).all()               # every step is one voxel along one axis
    assert v.size // 4 <= len(path) <= v.size // 4 + v.size // 50
    assert path[0] == (0, 0, 0)                                          # (the root is the first voxel; reversed: the path's end)
    for hop in HOPS:
        assert _ncomp(v, hop) == 1 and _ncomp(_flip(v), hop) == 1
    # nothing but the path's own steps touches: each voxel has at most two 6-neighbours
    q = np.pad(v, 1).astype(int)
    nb = q[:-2, 1:-1, 1:-1] + q[2:, 1:-1, 1:-1] + q[1:-1, :-2, 1:-1] + q[1:-1, 2:, 1:-1] + q[1:-1, 1:-1, :-2] + q[1:-1, 1:-1, 2:]
    assert nb[v != 0].max() == 2 and (nb[v != 0] == 1).sum() == 2


def test_comb_collapses_in_the_last_plane():
    v = _comb()
    n0 = v.shape[0]
    for hop in HOPS:
        assert _ncomp(v, hop) == 2
        assert _ncomp(v[:n0 - 1], hop) == 9 * 5 + 5                      # without the last plane: every tooth on its own
        last = v.copy(); last[n0 - 1, v.shape[1] - 1, :] = 0
        assert _ncomp(last, hop) == 1 + 5                                # without the last row: the second comb falls apart


def test_diagonals_connect_by_hop():
    v, n = _diagonals()
    assert int(v.sum()) == 3 * n
    assert _ncomp(v, 1) == 3 * n
    assert _ncomp(v, 2) == 2 + n
    assert _ncomp(v, 3) == 3


def test_checkerboard_fills_the_sizes_buffer():
    for shape, n in (((5, 7, 9), 158), ((4, 6, 8), 96)):
        v = _checkerboard(shape)
        assert _ncomp(v, 1) == n == int(v.sum()) and _ncomp(v, 2) == 1 and _ncomp(v, 3) == 1
    assert 158 == (5 * 7 * 9) // 2 + 1                                   # the capacity labelVolume allocates for `sizes`


def test_lattice_has_more_than_65536_components():
    v = _lattice()
    for hop in HOPS:
        assert _ncomp(v, hop) == 73728 > 2 ** 16


def test_tiny_volumes_hit_the_word_edges():
    names = dict(_tiny_volumes())
    assert {int(np.prod(s)) % 4 for s in TINY_SHAPES} == {0, 1, 2, 3}
    v = names['1x7x32-all']
    assert list(np.flatnonzero(v)) == [0, 63, 64, 127, 128, 223] and _ncomp(v, 3) == 6      # roots at bit 0 and bit 63
    v = names['1x1x131-last']
    assert list(np.flatnonzero(v)) == [130] and 131 % 64 != 0            # a root in the partly filled last word
    assert _ncomp(names['1x1x65-all'], 1) == 2                           # (63 and 64 touch there: one root at bit 63)


def test_no_wrap_volumes_have_memory_neighbours_that_do_not_touch():
    for shape in ((6, 5, 2), (6, 2, 5), (2, 6, 5)):
        a, b, c = _no_wrap(shape)
        for v in (a, b):
            lab = MO.labelVolume(v, maxHop=1)[0].ravel()
            f = v.ravel()
            pairs = np.flatnonzero((f[:-1] != 0) & (f[1:] != 0))
            assert len(pairs) >= shape[0] // 2
            assert (lab[pairs] != lab[pairs + 1]).all()                  # consecutive in memory, different components
        assert c.reshape(-1, shape[2])[0::2, [0, -1]].all() and int(c.sum()) == shape[0] * shape[1]


# ------------------------------------------------------------------ GPU: labelling
@pytest.mark.gpu
@pytest.mark.parametrize('maxHop', HOPS)
@pytest.mark.parametrize('case', sorted(LABEL_CASES))
def test_label_structured_volumes(case, maxHop):
    from arterynetwork_amd.generateVesselVolume import labelVolume
    vol = LABEL_CASES[case]
    lab, res = labelVolume(vol, maxHop=maxHop)
    olab, ores = MO.labelVolume(vol, maxHop=maxHop)
    assert lab.shape == vol.shape and np.array_equal(lab, olab)
    assert res == ores


# ------------------------------------------------------------------ section 2: misaligned device pointers
MISALIGNED_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import ctypes as C
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import generateVesselVolume as G
from oracle import mask_oracle as MO
dev = torch.device('cuda', 0)
lib = G._lib()
PAD = 64                          # elements on either side: a multiple of 16 bytes for every dtype used here
SENT = {{torch.uint8: 0xA5, torch.int32: -7777, torch.float32: 3.0e30, torch.float64: 3.0e300}}


class Carved:
    '''`numel` elements at element offset `off` inside an allocation of numel + 2 * PAD, the rest holding a sentinel
    (a correct kernel may touch the view only; every byte near it is owned all the same).'''
    def __init__(self, numel, dtype, off, src=None):
        assert 0 <= off < PAD
        self.whole = torch.full((numel + 2 * PAD,), SENT[dtype], dtype=dtype, device=dev)
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.hi = PAD + off, PAD + off + numel
        self.view = self.whole[self.lo:self.hi]
        if src is not None:
            self.view.copy_(torch.as_tensor(np.ascontiguousarray(src).ravel()))
        self.ptr = self.view.data_ptr()
        assert self.ptr == self.whole.data_ptr() + self.lo * self.whole.element_size()

    def intact(self):
        s = SENT[self.whole.dtype]
        return bool((self.whole[:self.lo] == s).all()) and bool((self.whole[self.hi:] == s).all())

    def numpy(self):
        return self.view.cpu().numpy()


def label(vol, hop, voff, loff):
    V = vol.size
    v, l = Carved(V, torch.uint8, voff, vol), Carved(V, torch.int32, loff)
    assert (v.ptr % 4 != 0) == bool(voff) and (l.ptr % 16 != 0) == bool(loff)
    n = C.c_int64(); cap = V // 2 + 1; sizes = np.zeros(cap, np.int64)
    torch.cuda.synchronize()
    rc = lib.vmask_label(0, v.ptr, *vol.shape, hop, l.ptr, sizes.ctypes.data, cap, C.byref(n))
    torch.cuda.synchronize()
    assert rc == 0, lib.vmask_last_error()
    assert v.intact() and l.intact(), ('guard band overwritten', vol.shape, hop, voff, loff)
    assert np.array_equal(v.numpy(), vol.ravel())
    return l.numpy().reshape(vol.shape), n.value, sizes[:n.value].tolist()


def mask(brain, ves, boff, voff, ooff, **kw):
    V = ves.size
    tdt = torch.float32 if ves.dtype == np.float32 else torch.float64
    b, v, o = Carved(V, torch.uint8, boff, brain), Carved(V, tdt, voff, ves), Carved(V, torch.uint8, ooff)
    assert (b.ptr % 4 != 0) == bool(boff) and (v.ptr % 16 != 0) == bool(voff) and (o.ptr % 4 != 0) == bool(ooff)
    kept = C.c_int64()
    torch.cuda.synchronize()
    rc = lib.vmask_vessel_mask(0, b.ptr, v.ptr, 5 if ves.dtype == np.float32 else 6, *ves.shape, kw['edtMax'], kw['frac1'], kw['frac2'],
                               kw['minSize'], o.ptr, C.byref(kept))
    torch.cuda.synchronize()
    assert rc == 0, lib.vmask_last_error()
    assert b.intact() and v.intact() and o.intact(), ('guard band overwritten', ves.shape, ves.dtype, boff, voff, ooff)
    assert np.array_equal(b.numpy(), brain.ravel()) and np.array_equal(v.numpy(), ves.ravel())
    return o.numpy().reshape(ves.shape), kept.value


rng = np.random.default_rng(31)
for shape in ((9, 7, 5), (8, 7, 5)):              # V % 4 == 3, and V % 4 == 0: there the pointer alone decides the branch
    vol = (rng.random(shape) < 0.15).astype(np.uint8)
    vol.flat[0] = 0; vol.flat[-1] = 1
    for hop in (1, 3):
        ref = label(vol, hop, 0, 0)
        olab, ores = MO.labelVolume(vol, maxHop=hop)
        assert np.array_equal(ref[0], olab) and [(0, vol.size - sum(ref[2]))] + list(zip(range(1, ref[1] + 1), ref[2])) == ores
        assert ref[1] > 3
        for voff, loff in ((1, 0), (0, 1), (1, 1), (3, 3)):
            got = label(vol, hop, voff, loff)
            assert np.array_equal(got[0], ref[0]) and got[1:] == ref[1:], (shape, hop, voff, loff)
    brain = np.zeros(shape, np.uint8); brain[1:-1, 1:-1, :-1] = 1
    kw = dict(edtMax=1.0, frac1=0.8, frac2=0.5, minSize=2)
    for dt in (np.float32, np.float64):
        ves = rng.random(shape).astype(dt)
        ves.flat[-1] = 2.0; ves.flat[0] = -1.0     # (the extremes at the two ends: the reduction's first load and its scalar tail)
        ref = mask(brain, ves, 0, 0, 0, **kw)
        oref = MO.vesselVolumeMask(brain, ves, **kw)
        assert np.array_equal(ref[0], oref) and ref[1] == int(oref.sum())
        assert 0 < ref[1] < ves.size
        for boff, voff, ooff in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 3, 3)):
            got = mask(brain, ves, boff, voff, ooff, **kw)
            assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], (shape, dt, boff, voff, ooff)
print('MISALIGNED OK')
"""


@pytest.mark.gpu
def test_misaligned_device_pointers_with_guard_bands():
    """vmask_label and vmask_vessel_mask with device pointers that are not 4- / 16-byte aligned (the scalar branches of
    k_cc_init, k_cc_labels, k_cc_filter, k_minmax and k_edt_axis0): every view lies inside a larger allocation with a
    sentinel on either side; the sentinels survive and the result is that of the aligned call (and the oracle's).  Own
    process: torch is imported before the HIP library there."""
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, '-c', MISALIGNED_SCRIPT.format(root=ROOT)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'MISALIGNED OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ------------------------------------------------------------------ section 3: min/max over the unrolled loop
MINMAX_BLOCKS, MINMAX_TPB = 1024, 256             # the launch of k_minmax (vessel_mask_impl)
MINMAX_SHAPES = {np.float32: (149, 147, 147), np.float64: (117, 117, 117)}


def _thresholds(ves, frac1, frac2):
    """numpy scalar arithmetic in the volume's dtype, as generateVesselVolume.py:187-190 does it."""
    t = ves.dtype.type
    lo, hi = np.amin(ves), np.amax(ves)
    return lo + t(frac1) * (hi - lo), lo + t(frac2) * (hi - lo)


def _minmax_plan(dtype):
    """Shape, and the flat indices an extreme has to be found at: element 0, the last one (scalar tail), one that a thread
    reaches only as the 2nd, 3rd and 4th load of the unrolled turn, and one in the leftover loop after it."""
    shape = MINMAX_SHAPES[dtype]
    V = int(np.prod(shape))
    W = 16 // np.dtype(dtype).itemsize                  # elements per 16-byte word
    nth = MINMAX_BLOCKS * MINMAX_TPB
    nq = V // W
    assert nq > 3 * nth and V % W != 0                  # the unrolled turn runs, and there is a scalar tail
    unrolled = nq - 3 * nth                             # threads 0 .. unrolled-1 take one unrolled turn, the others the leftover loop
    assert 0 < unrolled < nth and nq < 4 * nth
    t = unrolled // 3
    pos = {'first': 0, 'last': V - 1,
           'load1': (t + 1 * nth) * W + 1, 'load2': (t + 2 * nth) * W + W - 1, 'load3': (t + 3 * nth) * W,
           'leftover': (unrolled + 7 + 2 * nth) * W + 1}
    assert pos['load3'] < nq * W and pos['leftover'] < nq * W and nq * W <= pos['last']
    return shape, V, pos


def _minmax_volume(dtype, at_min, at_max):
    shape, V, pos = _minmax_plan(dtype)
    ves = np.full(V, 1.0, dtype)
    rng = np.random.default_rng(5)
    lo, hi = dtype(-2.0), dtype(5.0)
    thr1 = lo + dtype(0.8) * (hi - lo)
    # voxels around the threshold, and around the ones a missed minimum (lo = 1: 4.2) or maximum (hi = 1: 0.4) would give
    values = [thr1, np.nextafter(thr1, dtype(np.inf)), np.nextafter(thr1, dtype(-np.inf)), 3.0, 3.5, 3.8, 4.0, 4.1, 4.3, 4.9, 0.3, 0.5, -1.5]
    where = rng.choice(V - 2, size=40 * len(values), replace=False) + 1
    where = np.array([w for w in where if w not in set(pos.values())])
    for k, val in enumerate(values):
        ves[where[k::len(values)]] = val
    ves[pos[at_min]] = lo
    ves[pos[at_max]] = hi
    return ves.reshape(shape)


def test_minmax_plan_exceeds_the_unrolled_bound():
    for dtype in (np.float32, np.float64):
        shape, V, pos = _minmax_plan(dtype)
        assert len(set(pos.values())) == 6
        ves = _minmax_volume(dtype, 'load2', 'leftover')
        assert np.amin(ves) == -2.0 and np.amax(ves) == 5.0 and (ves == -2.0).sum() == 1 and (ves == 5.0).sum() == 1
        thr1, thr2 = _thresholds(ves, 0.8, 0.7)
        assert thr1 > thr2 and (ves == thr1).sum() >= 30 and (ves > thr1).sum() > 100 and ((ves > thr2) & (ves <= thr1)).sum() > 100
    assert V % 2 == 1 and int(np.prod(MINMAX_SHAPES[np.float32])) % 4 != 0


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_minmax_unrolled_loop_finds_the_extremes(dtype, capsys):
    """A unique minimum and a unique maximum over a constant background, in a volume large enough for the four-loads-in-flight
    turn of k_minmax, at every kind of position the kernel reaches differently.  All-zero brain mask (distance 0 everywhere)
    and minSize = 0: the mask is (ves > max(thr1, thr2)) & (ves != 0), plain numpy."""
    from arterynetwork_amd.generateVesselVolume import vesselVolumeMask
    order = ['first', 'last', 'load1', 'load2', 'load3', 'leftover']
    brain = np.zeros(MINMAX_SHAPES[dtype], np.uint8)
    for k, at_min in enumerate(order):
        at_max = order[(k + 1) % len(order)]
        ves = _minmax_volume(dtype, at_min, at_max)
        thr1, thr2 = _thresholds(ves, 0.8, 0.7)
        ref = ((ves > max(thr1, thr2)) & (ves != 0)).astype(np.uint8)
        got = vesselVolumeMask(brain, ves, minSize=0)
        assert np.array_equal(got, ref), (at_min, at_max)
        assert 'Number of voxels in segmentation: {}'.format(int(ref.sum())) in capsys.readouterr().out


# ------------------------------------------------------------------ section 4: the pipeline's comparisons at their boundaries
SHAPE4 = (40, 36, 30)
LO, HI = -3.25, 11.625                              # (not round; exact in float32; see test_tie_volumes_... for why these two)
TIE_EDT_MAX, TIE_MIN_SIZE = 6, 20
FRACS = [(0.8, 0.7), (0.1, 1.0 / 3.0)]
BLOB_VALUES = ['thr2', 'thr2+', 'thr2-', 'thr1', 'thr1+', 'thr1-']


def _tie_volumes(dtype, frac1, frac2):
    """Background at LO, one voxel at HI, and 3x3x3 blobs (27 > TIE_MIN_SIZE voxels) that sit exactly at thr2, one ulp above
    and below it, and the same for thr1 - each once within TIE_EDT_MAX of the brain mask's boundary and once deeper.
    Returns brain, ves, {name: (slices, value, inside the band)}."""
    t = np.dtype(dtype).type
    brain = np.zeros(SHAPE4, np.uint8)
    brain[2:-2, 2:-2, 2:-2] = 1
    ves = np.full(SHAPE4, LO, dtype)
    ves[38, 1, 1] = HI
    thr1, thr2 = _thresholds(ves, frac1, frac2)
    vals = {'thr2': thr2, 'thr2+': np.nextafter(thr2, t(np.inf)), 'thr2-': np.nextafter(thr2, t(-np.inf)),
            'thr1': thr1, 'thr1+': np.nextafter(thr1, t(np.inf)), 'thr1-': np.nextafter(thr1, t(-np.inf))}
    blobs = {}
    for k, name in enumerate(BLOB_VALUES):
        band = (slice(3, 6), slice(3 + 5 * k, 6 + 5 * k), slice(4, 7))
        deep = (slice(12 + 8 * (k // 3), 15 + 8 * (k // 3)), slice(9 + 5 * (k % 3), 12 + 5 * (k % 3)), slice(13, 16))
        for sl, inside in ((band, True), (deep, False)):
            ves[sl] = vals[name]
            blobs[(name, inside)] = (sl, vals[name], inside)
    return brain, ves, blobs


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('fracs', FRACS)
def test_tie_volumes_sit_exactly_at_the_thresholds(dtype, fracs):
    brain, ves, blobs = _tie_volumes(dtype, *fracs)
    assert ves.dtype == dtype and np.amin(ves) == dtype(LO) and np.amax(ves) == dtype(HI)
    thr1, thr2 = _thresholds(ves, *fracs)
    assert type(thr1) is np.dtype(dtype).type
    edt = MO.distance_transform_edt(brain)
    for (name, inside), (sl, val, _) in blobs.items():
        assert (ves[sl] == val).all() and ves[sl].size == 27 > TIE_MIN_SIZE
        assert (edt[sl] <= TIE_EDT_MAX).all() if inside else (edt[sl] > TIE_EDT_MAX).all()
    assert blobs[('thr2', True)][1] == thr2 and blobs[('thr1', False)][1] == thr1
    assert blobs[('thr2-', True)][1] < thr2 < blobs[('thr2+', True)][1] and blobs[('thr1-', True)][1] < thr1 < blobs[('thr1+', True)][1]
    ref = MO.vesselVolumeMask(brain, ves, edtMax=TIE_EDT_MAX, frac1=fracs[0], frac2=fracs[1], minSize=TIE_MIN_SIZE)
    kept = {key for key, (sl, _, _) in blobs.items() if ref[sl].all()}
    assert all(ref[sl].all() or not ref[sl].any() for sl, _, _ in blobs.values()) and int(ref.sum()) == 27 * len(kept)
    if fracs == (0.8, 0.7):       # thr2 < thr1: inside the band only what exceeds thr1 stays, deeper everything that exceeds thr2
        assert kept == {('thr1+', True), ('thr2+', False), ('thr1', False), ('thr1+', False), ('thr1-', False)}
    else:                         # thr1 < thr2: the second comparison alone decides
        assert thr1 < thr2 and kept == {('thr2+', True), ('thr2+', False)}
    if dtype == np.float32 and fracs == (0.8, 0.7):
        # with these extremes the float32 threshold is not the rounded float64 one, whether only the product or the whole
        # expression is evaluated in double: arithmetic in the wrong precision moves thr1 by an ulp, onto or off a blob
        lo64, hi64 = np.float64(LO), np.float64(HI)
        assert np.float32(lo64 + fracs[0] * (hi64 - lo64)) != thr1
        assert np.float32(LO) + np.float32(fracs[0] * (hi64 - lo64)) != thr1


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('fracs', FRACS)
def test_pipeline_threshold_ties(dtype, fracs, capsys):
    from arterynetwork_amd.generateVesselVolume import vesselVolumeMask
    brain, ves, _ = _tie_volumes(dtype, *fracs)
    kw = dict(edtMax=TIE_EDT_MAX, frac1=fracs[0], frac2=fracs[1], minSize=TIE_MIN_SIZE)
    ref = MO.vesselVolumeMask(brain, ves, **kw)
    got = vesselVolumeMask(brain, ves, **kw)
    assert np.array_equal(got, ref)
    assert 'Number of voxels in segmentation: {}'.format(int(ref.sum())) in capsys.readouterr().out


EDT_ZERO = (14, 13, 12)
EDT_MAXES = [10, 7.5, math.sqrt(50)]


def _edt_volumes(dtype):
    """A brain mask whose only zero voxel is EDT_ZERO: the squared distance of a voxel is the squared length of its offset
    from there - 100 along an axis and as (6, 8, 0), 101, 56 and 57, 50 and 51 are all hit.  Vesselness: halfway between
    thr2 and thr1 everywhere (one voxel at LO, one at HI), so a voxel stays exactly when its distance exceeds edtMax."""
    brain = np.ones(SHAPE4, np.uint8)
    brain[EDT_ZERO] = 0
    ves = np.full(SHAPE4, LO + 0.75 * (HI - LO), dtype)
    ves[0, 0, 0] = LO
    ves[39, 35, 29] = HI
    return brain, ves


def test_edt_volumes_hit_the_distances_exactly():
    brain, ves = _edt_volumes(np.float32)
    thr1, thr2 = _thresholds(ves, 0.8, 0.7)
    assert thr2 < ves[5, 5, 5] < thr1
    edt = MO.distance_transform_edt(brain)
    z = np.array(EDT_ZERO)
    for off, sq in (((10, 0, 0), 100), ((0, 10, 0), 100), ((0, 0, 10), 100), ((6, 8, 0), 100), ((10, 1, 0), 101), ((6, 4, 2), 56),
                    ((7, 2, 2), 57), ((5, 5, 0), 50), ((7, 1, 0), 50), ((7, 1, 1), 51)):
        assert edt[tuple(z + off)] == math.sqrt(sq) and sum(o * o for o in off) == sq
    for edtMax in EDT_MAXES:
        ref = MO.vesselVolumeMask(brain, ves, edtMax=edtMax, minSize=0)
        d2 = np.rint(edt ** 2).astype(int)
        inner = d2 <= int(edtMax * edtMax + 1e-9)
        assert not ref[inner].any() and ref[~inner].sum() == (~inner).sum() - 1          # (the voxel at LO lies outside and goes)
        for sq, kept in ((100, edtMax < 10), (101, edtMax < 10.04), (56, edtMax < 7.4), (57, edtMax < 7.54), (50, edtMax < 7.07), (51, edtMax < 7.1)):
            assert (ref[d2 == sq] == int(kept)).all() and (d2 == sq).sum() >= 6


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('edtMax', EDT_MAXES)
def test_pipeline_edt_boundary(dtype, edtMax, capsys):
    from arterynetwork_amd.generateVesselVolume import vesselVolumeMask
    brain, ves = _edt_volumes(dtype)
    ref = MO.vesselVolumeMask(brain, ves, edtMax=edtMax, minSize=0)
    got = vesselVolumeMask(brain, ves, edtMax=edtMax, minSize=0)
    assert np.array_equal(got, ref)
    assert 'Number of voxels in segmentation: {}'.format(int(ref.sum())) in capsys.readouterr().out


MIN_SIZES = [150, 1, 0]


def _size_volumes(dtype, minSize):
    """Separate components of minSize-1, minSize and minSize+1 voxels (those that exist), all at HI over a background at LO:
    the first k voxels, in raster order, of a 16-voxel-wide strip of one plane - straight up to 16 voxels, L-shaped after."""
    brain = np.zeros(SHAPE4, np.uint8)
    brain[2:-2, 2:-2, 2:-2] = 1
    ves = np.full(SHAPE4, LO, dtype)
    sizes = [s for s in (minSize - 1, minSize, minSize + 1) if s > 0]
    for k, s in enumerate(sizes):
        strip = np.zeros((SHAPE4[1] - 6) * 16, bool)
        strip[:s] = True
        ves[4 + 12 * k, 3:-3, 5:21][strip.reshape(-1, 16)] = HI
    return brain, ves, sizes


@pytest.mark.parametrize('minSize', MIN_SIZES)
def test_size_volumes_have_components_at_the_boundary(minSize):
    brain, ves, sizes = _size_volumes(np.float32, minSize)
    assert sizes == {150: [149, 150, 151], 1: [1, 2], 0: [1]}[minSize]
    assert [s for label, s in MO.labelVolume(ves == np.float32(HI))[1] if label] == sizes
    ref = MO.vesselVolumeMask(brain, ves, minSize=minSize)
    assert int(ref.sum()) == minSize + 1


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('minSize', MIN_SIZES)
def test_pipeline_size_boundary(dtype, minSize, capsys):
    from arterynetwork_amd.generateVesselVolume import vesselVolumeMask
    brain, ves, _ = _size_volumes(dtype, minSize)
    ref = MO.vesselVolumeMask(brain, ves, minSize=minSize)
    got = vesselVolumeMask(brain, ves, minSize=minSize)
    assert np.array_equal(got, ref) and int(got.sum()) == minSize + 1
    assert 'Number of voxels in segmentation: {}'.format(minSize + 1) in capsys.readouterr().out


def _degenerate_cases(dtype):
    """name -> (brain, ves, keyword arguments)."""
    rng = np.random.default_rng(41)
    brain = np.zeros(SHAPE4, np.uint8)
    brain[2:-2, 2:-2, 2:-2] = 1
    cases = {'constant': (brain, np.full(SHAPE4, 2.5, dtype), {}),
             'constant-zero': (brain, np.zeros(SHAPE4, dtype), {}),
             'constant-negative': (brain, np.full(SHAPE4, -2.5, dtype), {'minSize': 0})}
    neg = (-10.0 + 0.5 * rng.random(SHAPE4)).astype(dtype)
    neg[10:30, 16:20, 13:17] = (-1.5 + 0.4 * rng.random((20, 4, 4))).astype(dtype)       # a bar deep inside: kept
    neg[3:6, 5:30, 4:7] = (-3.5 + 0.4 * rng.random((3, 25, 3))).astype(dtype)            # between thr2 and thr1 near the boundary: goes
    neg[12:28, 21:24, 13:17] = (-3.5 + 0.4 * rng.random((16, 3, 4))).astype(dtype)        # ... and deep inside: stays
    neg[20, 30, 20] = -1.0
    cases['all-negative'] = (brain, neg, {})
    z = (0.2 + 0.8 * rng.random(SHAPE4)).astype(dtype)
    z[0, 0, 0] = -1.0
    z[39, 35, 29] = 1.0
    z[5:35:3, 7:30:4, 6:25:5] = 0.0                  # exactly zero and minus zero: background whatever the thresholds are
    z[6:35:3, 8:30:4, 7:25:5] = -0.0
    cases['negative-fractions'] = (brain, z, {'frac1': -0.05, 'frac2': -0.1, 'minSize': 0})
    cases['negative-frac2'] = (brain, z, {'frac2': -0.1, 'edtMax': 3, 'minSize': 0})
    return cases


DEGENERATE = sorted(_degenerate_cases(np.float32))


def test_degenerate_inputs_are_what_they_claim():
    cases = _degenerate_cases(np.float32)
    for name in ('constant', 'constant-zero', 'constant-negative'):
        brain, ves, kw = cases[name]
        assert not MO.vesselVolumeMask(brain, ves, **kw).any()
    brain, ves, kw = cases['all-negative']
    ref = MO.vesselVolumeMask(brain, ves, **kw)
    assert ves.max() < 0 and ref[10:30, 16:20, 13:17].all() and ref[12:28, 21:24, 13:17].all() and not ref[3:6, 5:30, 4:7].any()
    assert int(ref.sum()) == 320 + 192
    brain, ves, kw = cases['negative-fractions']
    zeros = ves == 0
    assert np.signbit(ves[zeros]).sum() > 100 and (~np.signbit(ves[zeros])).sum() > 100
    thr1, thr2 = _thresholds(ves, kw['frac1'], kw['frac2'])
    assert thr2 < thr1 < ves.min() == -1.0
    ref = MO.vesselVolumeMask(brain, ves, **kw)
    assert np.array_equal(ref != 0, ~zeros)
    brain, ves, kw = cases['negative-frac2']
    ref = MO.vesselVolumeMask(brain, ves, **kw)
    assert not ref[zeros].any() and 0 < ref.sum() < (~zeros).sum()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('case', DEGENERATE)
def test_pipeline_degenerate_inputs(dtype, case, capsys):
    from arterynetwork_amd.generateVesselVolume import vesselVolumeMask
    brain, ves, kw = _degenerate_cases(dtype)[case]
    ref = MO.vesselVolumeMask(brain, ves, **kw)
    got = vesselVolumeMask(brain, ves, **kw)
    assert np.array_equal(got, ref)
    assert 'Number of voxels in segmentation: {}'.format(int(ref.sum())) in capsys.readouterr().out
    if case.startswith('constant'):
        assert not got.any()
