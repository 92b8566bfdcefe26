"""Edge-preserving denoising (DESIGN.md section 9 entry f14): the numpy model tests/denoise_model.py is checked on the CPU
(what the filters are for, range, mean, fixed points, the explicit median against scipy), the median's exchange networks are proved on
every 0/1 input, then vmask_diffuse must return
the model's bits with the rational conductance and stay within 1e-9 of the input's span with the exponential one, and
vmask_median must equal scipy.ndimage.median_filter(mode='nearest')."""
import functools
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

import denoise_model as M
from conftest import ROOT
from arterynetwork_amd import denoise as DN
from arterynetwork_amd._capi import VrgError

BAR = 1e-9                                               # of the input's span: the project's bar for float64 quantities against their oracle
RADII = list(itertools.product((0, 1), repeat=3))
SPACINGS = (None, (1.0, 1.0, 2.0), (0.5, 0.7, 1.3))

# the tile extents of the kernels (csrc/vden_device.hip): k_den_diffuse DZ, DY, DX; k_den_median MZ, MY, MX
E_DIFFUSE = (32, 16, 64)
E_MEDIAN = (32, 4, 64)


def _tile_shapes():
    """Per axis and tile extent E: E - 1, E, E + 1 and 2 E + 1 on that axis, the other two extents small."""
    shapes = []
    for axis in range(3):
        for E in sorted({E_DIFFUSE[axis], E_MEDIAN[axis]}):
            for n in (E - 1, E, E + 1, 2 * E + 1):
                s = [3, 5, 6]
                s[axis] = n
                shapes.append(tuple(s))
    return shapes


SHAPES = [(1, 1, 1), (1, 1, 7), (1, 6, 1), (5, 1, 1), (2, 2, 2), (3, 4, 5), (17, 64, 9), (20, 18, 16), (9, 17, 65), (4, 3, 130), (33, 30, 41)]
SHAPES += [s for s in _tile_shapes() if s not in SHAPES]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def _noisy(shape, seed=0):
    """A step of 100 across the middle of axis 1, a ramp along axis 2, Gaussian noise of sigma 5 on every voxel."""
    v = np.random.default_rng(seed).normal(0.0, 5.0, shape)
    v[:, shape[1] // 2:, :] += 100.0
    return v + 0.5 * np.arange(shape[2])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------ CPU: the model itself
@pytest.mark.parametrize('radius', RADII, ids=lambda r: ''.join(map(str, r)))
def test_model_explicit_median_equals_scipy(radius):
    for shape in ((6, 7, 5), (1, 4, 9), (2, 1, 3)):
        I = _noisy(shape, seed=3)
        for vol in (I, I.astype(np.float32), np.round(I / 40.0)):
            a, b = M.median_explicit(vol, radius), M.median_scipy(vol, radius)
            assert a.dtype == b.dtype == vol.dtype and np.array_equal(a, b)


def _step_scores(u, clean):
    flat = np.concatenate([(u - clean)[:, :8].ravel(), (u - clean)[:, 12:].ravel()])
    return float(flat.std()), float((u[:, 10] - u[:, 9]).mean())


@pytest.mark.parametrize('function,spacing', [('rational', None), ('exponential', None), ('rational', (1.0, 1.0, 2.0))])
def test_model_keeps_the_edge_and_removes_the_noise(function, spacing):
    """What the filter is for.  Measured when this was written: 0.684 / 97.6 rational, 0.695 / 100.4 exponential, 0.790 / 96.9
    at spacing (1, 1, 2); a Gaussian of sigma 1 leaves 40.0 of the jump."""
    clean, noisy = M.step_phantom()
    sd, jump = _step_scores(M.diffuse(noisy, 15.0, 10, spacing=spacing, function=function), clean)
    print('{} {}: sd {:.3f} (5.0 before), jump {:.1f}'.format(function, spacing, sd, jump))
    assert sd < 1.0 and jump > 95.0
    _, blurred = _step_scores(ndi.gaussian_filter(noisy, 1.0), clean)
    assert blurred < 50.0


@pytest.mark.parametrize('function', ['rational', 'exponential'])
def test_model_range_mean_and_constant(function):
    _, noisy = M.step_phantom()
    span = noisy.max() - noisy.min()
    for spacing in SPACINGS:
        u = M.diffuse(noisy, 15.0, 10, time_step=M.bound(spacing), spacing=spacing, function=function)      # dt at the bound
        assert u.min() >= noisy.min() - 1e-12 * span and u.max() <= noisy.max() + 1e-12 * span
        assert abs(u.mean() - noisy.mean()) <= 1e-12 * span
        const = np.full((5, 6, 7), 37.3)
        assert _bits(M.diffuse(const, 15.0, 7, time_step=M.bound(spacing), spacing=spacing, function=function)).tobytes() == _bits(const).tobytes()


def test_model_slabs_do_not_change_the_bits():
    """The large GPU case computes its model slab by slab along axis 0: the per-voxel arithmetic does not know."""
    I = _noisy((13, 6, 7), seed=5)
    for slab in (1, 4, 13):
        assert np.array_equal(_bits(M.diffuse(I, 15.0, 3, slab=slab)), _bits(M.diffuse(I, 15.0, 3)))


def test_model_median_removes_spikes():
    clean, _ = M.step_phantom()
    spiked = clean.copy()
    keep = []                                            # forty isolated spikes: no two within one 3 x 3 x 3 window
    for p in np.stack(np.unravel_index(np.random.default_rng(11).permutation(clean.size), clean.shape), axis=1):
        if len(keep) < 40 and all(np.abs(p - q).max() > 2 for q in keep):
            keep.append(p)
    assert len(keep) == 40
    for p in keep:
        spiked[tuple(p)] = 1000.0
    assert np.array_equal(M.median_explicit(spiked, (1, 1, 1)), clean)
    assert np.array_equal(M.median_explicit(clean, (1, 1, 1)), clean)


def test_bound_is_the_models():
    for spacing in SPACINGS:
        assert DN.stabilityBound(spacing) == M.bound(spacing)
    assert DN.stabilityBound() == 1.0 / 6.0


def test_argument_errors_raise():
    """What the host can check is refused before a device is looked for: no GPU needed."""
    I = np.zeros((6, 5, 4))
    bad = [dict(volume=np.zeros((6, 5))), dict(volume=np.zeros((2, 6, 5, 4))), dict(iterations=0), dict(iterations=1001),
           dict(conductance=0.0), dict(conductance=-1.0), dict(conductance=float('nan')), dict(conductance=float('inf')),
           dict(spacing=(1.0, 1.0)), dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, float('nan'), 1.0)), dict(spacing=(1.0, 1.0, float('inf'))),
           dict(timeStep=float('nan')), dict(timeStep=float('inf')), dict(timeStep=np.nextafter(1.0 / 6.0, 1.0)),
           dict(timeStep=0.23, spacing=(1.0, 1.0, 2.0)), dict(function='linear')]
    for kw in bad:
        args = dict(volume=I, conductance=15.0)
        args.update(kw)
        with pytest.raises(ValueError):
            DN.anisotropicDiffusion(**args)
    for radius in (2, -1, (1, 1), (1, 2, 0), (1, 1, 1, 1)):
        with pytest.raises(ValueError):
            DN.medianFilter(I, radius)
    with pytest.raises(ValueError):
        DN.medianFilter(np.zeros((6, 5)))
    with pytest.raises(ValueError):
        DN.main('.', method='gaussian')


def _refusals(dll, inp, f32, out, shape):
    """Every refused input of the two C entries: (label, return code).  `inp`, `f32` and `out` are addresses of a float64
    volume, a float32 volume and the output of that shape."""
    sp = lambda *h: np.array(h, dtype=np.float64)
    keep = []                                            # (the spacing arrays must outlive the calls)

    def diffuse(label, volume=inp, dtype=6, dims=shape, spacing=None, K=15.0, iterations=3, dt=0.0, function=0, to=out):
        if spacing is not None:
            keep.append(spacing)
        return label, dll.vmask_diffuse(0, volume, dtype, *dims, spacing.ctypes.data if spacing is not None else None, K, iterations, dt, function, to)

    def median(label, volume=inp, dtype=6, dims=shape, r=(1, 1, 1), to=out):
        return label, dll.vmask_median(0, volume, dtype, *dims, *r, to)
    inf, nan = float('inf'), float('nan')
    return [diffuse('iterations 0', iterations=0), diffuse('iterations 1001', iterations=1001), diffuse('iterations -1', iterations=-1),
            diffuse('K 0', K=0.0), diffuse('K < 0', K=-2.0), diffuse('K nan', K=nan), diffuse('K inf', K=inf),
            diffuse('spacing 0', spacing=sp(1, 0, 1)), diffuse('spacing < 0', spacing=sp(-1, 1, 1)), diffuse('spacing nan', spacing=sp(1, 1, nan)),
            diffuse('spacing inf', spacing=sp(inf, 1, 1)),
            diffuse('dt nan', dt=nan), diffuse('dt inf', dt=inf), diffuse('dt above the bound', dt=float(np.nextafter(1.0 / 6.0, 1.0))),
            diffuse('dt above the bound of the spacing', dt=0.23, spacing=sp(1, 1, 2)),
            diffuse('function 2', function=2), diffuse('function -1', function=-1),
            diffuse('dtype 4', dtype=4), diffuse('dtype 7', dtype=7),
            diffuse('null volume', volume=None), diffuse('null out', to=None),
            diffuse('shape 0', dims=(0, shape[1], shape[2])), diffuse('shape envelope', dims=(2000, 2000, 600)),
            median('radius 2', r=(2, 1, 1)), median('radius -1', r=(1, -1, 1)), median('radius 2 on axis 2', r=(0, 0, 2)),
            median('dtype 4', dtype=4), median('dtype 7', volume=f32, dtype=7),
            median('null volume', volume=None), median('null out', to=None),
            median('shape 0', dims=(shape[0], 0, shape[2])), median('shape envelope', dims=(2000, 2000, 600))]


def test_c_entries_refuse_before_a_device_is_looked_for():
    """Host pointers, no GPU needed: every refusal is VRG_E_ARG and leaves the output alone."""
    dll = DN._lib()
    shape = (4, 5, 6)
    I = _noisy(shape)
    I32 = I.astype(np.float32)
    out = np.full(shape, -12345.0)
    res = _refusals(dll, I.ctypes.data, I32.ctypes.data, out.ctypes.data, shape)
    assert len(res) == 32
    for label, rc in res:
        assert rc == -1, label                           # VRG_E_ARG
    assert (out == -12345.0).all() and np.array_equal(I, _noisy(shape))


# ------------------------------------------------------------------ no GPU needed: the kernels' resource records
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_denoise_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vden_device.hip' in build.SOURCES
    out = tmp_path / 'vden_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vden_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1)),
                            int(re.search(r'\.vgpr_count:\s+(\d+)', m.group(2)).group(1)))
    assert sum('k_den_diffuse' in k for k in recs) == 4 and sum('k_den_median' in k for k in recs) == 16, sorted(recs)
    for name, (scratch, vgprs) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        # the first build: k_den_diffuse 82 (rational) and 98 (exponential); k_den_median 8 .. 64 for the windows of 1, 3 and 9
        # values, 127 (float32) and 126 (float64) for the window of 27
        assert vgprs <= 128, '%s uses %d VGPRs' % (name, vgprs)


# ------------------------------------------------------------------ no GPU needed: the median's exchange networks, proved
NET_COMPARATORS = {3: 3, 9: 24, 27: 126}                 # a change to a table is a decision: it shows up here


def _networks():
    """NET3, NET9 and NET27 as they stand in vden_device.hip: {N: [(a, b), ...]}."""
    text = open(os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vden_device.hip')).read()
    nets = {}
    for m in re.finditer(r'constexpr CE NET(\d+)\[\] = \{(.*?)\};', text, re.S):
        body = m.group(2)
        pairs = [(int(a), int(b)) for a, b in re.findall(r'\{\s*(\d+)\s*,\s*(\d+)\s*\}', body)]
        assert not re.sub(r'\{\s*\d+\s*,\s*\d+\s*\}|[\s,]', '', body), 'NET%s holds something that is no comparator' % m.group(1)
        nets[int(m.group(1))] = pairs
    return text, nets


def _popcounts(x):
    x = x.astype(np.uint64)
    c = np.zeros(x.shape, np.int64)
    for s in range(0, 32):
        c += ((x >> np.uint64(s)) & np.uint64(1)).astype(np.int64)
    return c


@pytest.mark.parametrize('N', [3, 9, 27])
def test_median_network_selects_the_median_of_every_01_input(N):
    """The 0-1 principle, exhaustively: the pruned Batcher network NET<N> of vden_device.hip is applied to all 2^N inputs of zeros
    and ones, bit-sliced (one bit per input, a comparator (a, b) is (a & b, a | b) since `exchange` leaves the minimum in a), and
    wire N // 2 must be 1 exactly where the input holds at least N // 2 + 1 ones.  A network of min / max exchanges commutes with
    every monotone map, so a network that selects the median of every 0/1 input selects it for every input of totally ordered
    values: this proves the median for every finite window, ties included.  It covers orderings only - a NaN is not ordered, and
    include/vmask.h says of vmask_median's volume "assumed finite".  NET27 (2^27 inputs) takes about 1 s."""
    text, nets = _networks()
    assert sorted(nets) == [3, 9, 27]
    net = nets[N]
    assert len(net) == NET_COMPARATORS[N]
    assert all(a < b < N for a, b in net), [c for c in net if not c[0] < c[1] < N]
    assert re.search(r'a = lo; b = hi;', text) and 'return v[N / 2];' in text            # what the proof assumes of exchange and median_of
    # input x (an N-bit number) has bit i on wire i; bit b of word w is input 64 w + b
    low = [np.uint64(sum(1 << b for b in range(64) if (b >> i) & 1)) for i in range(6)]
    at_least = [np.uint64(sum(1 << b for b in range(64) if bin(b).count('1') >= k)) for k in range(8)]      # [7] = 0
    words = max(1, (1 << N) >> 6)
    valid = np.uint64((1 << min(64, 1 << N)) - 1)                                        # N = 3: one word, 8 inputs
    chunk = min(words, 1 << 16)
    ones, checked = np.uint64(0xFFFFFFFFFFFFFFFF), 0
    for start in range(0, words, chunk):
        w = np.arange(start, start + chunk, dtype=np.uint64)
        wires = []
        for i in range(N):
            if i < 6:
                wires.append(np.full(chunk, low[i], np.uint64))
            else:
                wires.append(np.where((w >> np.uint64(i - 6)) & np.uint64(1), ones, np.uint64(0)))
        for a, b in net:
            wires[a], wires[b] = wires[a] & wires[b], wires[a] | wires[b]
        need = np.clip(N // 2 + 1 - _popcounts(w), 0, 7)                                  # ones still needed among the word's 6 low wires
        want = np.array(at_least, np.uint64)[need]
        wrong = (wires[N // 2] ^ want) & valid
        assert not wrong.any(), 'NET{}: input {:#x} gives the wrong middle value'.format(N, int(np.flatnonzero(wrong)[0] + start) * 64)
        checked += chunk * min(64, 1 << N)
    assert checked == 1 << N


# ------------------------------------------------------------------ GPU: diffusion against the model
# (iterations, spacing, input dtype, dt at the bound?, K): both ping-pong parities, every spacing, every input type, both time
# steps; K = 1e-3 (next to nothing moves) and 1e6 (the linear heat equation)
VARIANTS = [(1, None, np.float64, False, 15.0), (2, (1.0, 1.0, 2.0), np.float32, True, 15.0), (3, (0.5, 0.7, 1.3), np.int16, False, 15.0),
            (6, None, np.float64, True, 15.0), (3, (1.0, 1.0, 2.0), np.float64, False, 1e-3), (2, (0.5, 0.7, 1.3), np.float32, True, 1e6)]


def _typed(I, dtype):
    return np.round(10.0 * I).astype(dtype) if dtype == np.int16 else I.astype(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_diffusion_rational_is_the_model(shape):
    for iterations, spacing, dtype, at_bound, K in VARIANTS:
        I = _typed(_noisy(shape), dtype)
        before = I.copy()
        dt = M.bound(spacing) if at_bound else None
        got = DN.anisotropicDiffusion(I, K, iterations, timeStep=dt, spacing=spacing)
        ref = M.diffuse(I, K, iterations, time_step=dt, spacing=spacing)
        label = '{} x{} {} {} dt {} K {}'.format(shape, iterations, spacing, np.dtype(dtype).name, dt, K)
        assert got.dtype == np.float64 and got.shape == tuple(shape), label
        assert np.array_equal(_bits(got), _bits(ref)), '{}: {} voxels differ, max {:.3e}'.format(label, int((got != ref).sum()), np.abs(got - ref).max())
        assert np.array_equal(I, before), label
        if K == 1e-3 and I.size > 1:
            assert np.abs(got - I).max() < 1e-3 * max(np.ptp(I.astype(np.float64)), 1.0), label     # next to nothing moves


@pytest.mark.gpu
def test_diffusion_rational_256x256x192():
    shape = (256, 256, 192)
    I = _noisy(shape, seed=2).astype(np.float32)
    got = DN.anisotropicDiffusion(I, 15.0, 4)
    ref = M.diffuse(I, 15.0, 4, slab=8)
    assert np.array_equal(_bits(got), _bits(ref))
    assert got.min() >= I.min() and got.max() <= I.max()


@pytest.mark.gpu
def test_diffusion_constant_volume_keeps_its_bits():
    for function in ('rational', 'exponential'):
        for shape, value, dtype in (((33, 17, 70), 37.3, np.float64), ((5, 6, 7), -1e-300, np.float64), ((9, 20, 65), 1234.5678, np.float32)):
            I = np.full(shape, value, dtype)
            for spacing in SPACINGS:
                got = DN.anisotropicDiffusion(I, 15.0, 5, timeStep=M.bound(spacing), spacing=spacing, function=function)
                assert _bits(got).tobytes() == _bits(I.astype(np.float64)).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_diffusion_exponential_is_near_the_model(shape):
    """The device's exp is not the host's: |delta| <= 1e-9 of the input's span.  The largest deviation seen is in DESIGN.md."""
    worst = 0.0
    for spacing, dtype, at_bound in ((None, np.float64, False), ((1.0, 1.0, 2.0), np.float32, True), ((0.5, 0.7, 1.3), np.int16, False)):
        I = _typed(_noisy(shape), dtype)
        dt = M.bound(spacing) if at_bound else None
        got = DN.anisotropicDiffusion(I, 15.0, 3, timeStep=dt, spacing=spacing, function='exponential')
        ref = M.diffuse(I, 15.0, 3, time_step=dt, spacing=spacing, function='exponential')
        span = max(float(np.ptp(I.astype(np.float64))), 1.0)
        dev = float(np.abs(got - ref).max()) / span
        worst = max(worst, dev)
        assert got.dtype == np.float64 and dev <= BAR, (shape, spacing, dev)
    print('exponential {}: max |delta| / span {:.3e}'.format(shape, worst))


# ------------------------------------------------------------------ GPU: the median against scipy
@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_median_is_scipys(shape):
    I = _noisy(shape, seed=1)
    levels = np.random.default_rng(4).integers(0, 3, shape)                # three levels: mostly ties
    for vol in (I, I.astype(np.float32), levels.astype(np.int16), levels.astype(np.float32)):
        before = vol.copy()
        for radius in RADII:
            got = DN.medianFilter(vol, radius)
            ref = M.median_scipy(vol.astype(got.dtype), radius)
            assert got.dtype == (np.float32 if vol.dtype == np.float32 else np.float64) and got.shape == tuple(shape)
            assert np.array_equal(got, ref), (shape, radius, vol.dtype, int((got != ref).sum()))
        assert np.array_equal(vol, before)
    assert np.array_equal(DN.medianFilter(I, 1), M.median_scipy(I, (1, 1, 1)))                   # an int radius
    assert np.array_equal(DN.medianFilter(I, 0), I)


@pytest.mark.gpu
def test_median_removes_spikes_and_keeps_the_value_set():
    clean, noisy = M.step_phantom()
    spiked = clean.copy()
    spiked[::5, ::6, ::7] = 1000.0                                          # isolated spikes
    assert np.array_equal(DN.medianFilter(spiked, 1), clean) and np.array_equal(DN.medianFilter(clean, 1), clean)
    q = np.round(noisy).astype(np.int16)
    assert set(np.unique(DN.medianFilter(q, (1, 1, 0)))) <= set(np.unique(q).astype(np.float64))


@pytest.mark.gpu
def test_both_filters_are_deterministic():
    I = _noisy((33, 30, 41), seed=6)
    for function in ('rational', 'exponential'):
        a, b = (DN.anisotropicDiffusion(I, 15.0, 4, function=function) for _ in range(2))
        assert a.tobytes() == b.tobytes()
    for vol in (I, I.astype(np.float32)):
        a, b = (DN.medianFilter(vol) for _ in range(2))
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ GPU: device pointers, in a process of their own
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import denoise as DN
from test_denoise import _noisy, _refusals, RADII
dev = torch.device('cuda', 0)
I = _noisy((21, 19, 67), seed=8)
for dtype in (np.float32, np.float64):
    host = I.astype(dtype)
    t = torch.as_tensor(host, device=dev)
    for function in ('rational', 'exponential'):
        for iterations in (1, 4):
            got = DN.anisotropicDiffusion(t, 15.0, iterations, spacing=(1.0, 1.0, 2.0), function=function)
            assert got.is_cuda and got.device == t.device and got.dtype == torch.float64 and tuple(got.shape) == I.shape
            ref = DN.anisotropicDiffusion(host, 15.0, iterations, spacing=(1.0, 1.0, 2.0), function=function)
            assert got.cpu().numpy().tobytes() == ref.tobytes()
            again = DN.anisotropicDiffusion(t, 15.0, iterations, spacing=(1.0, 1.0, 2.0), function=function)
            assert again.cpu().numpy().tobytes() == ref.tobytes()
    for radius in RADII:
        got = DN.medianFilter(t, radius)
        assert got.is_cuda and got.dtype == t.dtype and tuple(got.shape) == I.shape
        assert got.cpu().numpy().tobytes() == DN.medianFilter(host, radius).tobytes()
    assert t.cpu().numpy().tobytes() == host.tobytes()          # the input is unchanged
q = torch.as_tensor(np.round(I).astype(np.int16), device=dev)   # an integer tensor goes in as float64
assert DN.medianFilter(q).dtype == torch.float64 and DN.anisotropicDiffusion(q, 15.0, 2).cpu().numpy().tobytes() == DN.anisotropicDiffusion(np.round(I), 15.0, 2).tobytes()
print('DEVICE RESIDENT OK')

shape = (4, 5, 6)
a = torch.as_tensor(_noisy(shape), device=dev)
a32 = a.to(torch.float32)
out = torch.full(shape, -12345.0, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
res = _refusals(DN._lib(), a.data_ptr(), a32.data_ptr(), out.data_ptr(), shape)
assert len(res) == 32
for label, rc in res:
    assert rc == -1, label
torch.cuda.synchronize()
assert bool((out == -12345.0).all()) and a.cpu().numpy().tobytes() == _noisy(shape).tobytes()
print('REFUSALS OK')
"""


@functools.lru_cache(maxsize=None)
def _device_run():
    script = DEVICE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    return out.returncode, out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_denoise_device_resident():
    """A tensor on the GPU goes in by its device pointer and a tensor on the same device comes out, bit-identical to the
    host call and to a second run; the input is unchanged.  Own process: torch is imported before the HIP library there."""
    rc, stdout, tail = _device_run()
    assert 'DEVICE RESIDENT OK' in stdout, tail


@pytest.mark.gpu
def test_denoise_refusals_with_device_pointers():
    """Every refused input of the two C entries, with device pointers: VRG_E_ARG, the sentinel in the output untouched."""
    rc, stdout, tail = _device_run()
    assert rc == 0 and 'REFUSALS OK' in stdout, tail


# ------------------------------------------------------------------ GPU: the files
@pytest.mark.gpu
@pytest.mark.parametrize('method', ['diffusion', 'median'])
def test_denoise_main_feeds_vesselness(tmp_path, capsys, method):
    from arterynetwork_amd import nifti, vesselness as VS
    shape = (24, 20, 16)
    I = _noisy(shape, seed=9)
    aff = np.array([[0.5, 0, 0, -10.0], [0, 0.5, 0, 3.0], [0, 0, 0.75, 7.5], [0, 0, 0, 1.0]])
    nifti.saveVolume(I, aff, str(tmp_path / 'brainVolume.nii.gz'), astype=np.float32)
    kw = dict(conductance=15.0, iterations=3) if method == 'diffusion' else dict(radius=(1, 1, 0))
    res = DN.main(str(tmp_path), method=method, **kw)
    path = os.path.join(str(tmp_path), 'brainVolumeDenoised.nii.gz')
    assert 'brainVolumeDenoised.nii.gz saved to {}.'.format(path) in capsys.readouterr().out
    stored, aff2 = nifti.loadVolume(str(tmp_path), 'brainVolumeDenoised.nii.gz')
    assert stored.dtype == np.float32 and np.array_equal(stored, res.astype(np.float32)) and np.allclose(aff2, aff)
    I32 = I.astype(np.float32)
    if method == 'diffusion':
        assert res.dtype == np.float64 and np.array_equal(_bits(res), _bits(M.diffuse(I32, 15.0, 3, spacing=(0.5, 0.5, 0.75))))
    else:
        assert res.dtype == np.float32 and np.array_equal(res, M.median_scipy(I32, (1, 1, 0)))
    # vesselness.main reads the denoised file when told to - and brainVolume.nii.gz when not
    ves = VS.main(str(tmp_path), sigmas=(0.5,), volumeName='brainVolumeDenoised.nii.gz')
    assert np.array_equal(ves, VS.vesselnessFilter(stored, (0.5,), spacing=(0.5, 0.5, 0.75)))
    plain = VS.main(str(tmp_path), sigmas=(0.5,))
    assert np.array_equal(plain, VS.vesselnessFilter(I32, (0.5,), spacing=(0.5, 0.5, 0.75))) and not np.array_equal(plain, ves)
