"""Bias-field correction (DESIGN.md section 9 entry f15): the numpy model tests/bias_model.py is checked on the CPU (what the
step is for, the axis tables, the library's host sharpening map against np.fft), then vmask_bias_fit, vmask_bias_eval and the
whole loop vmask_bias_log_field must return the model's bits, and biasFieldCorrection must stay within a measured distance of
the model, whose log and exp are numpy's."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bias_model as M
from conftest import ROOT
from arterynetwork_amd import bias as B

# the extents at which the kernels of csrc/vbias_device.hip change workgroup: EZ planes of axis 0 in k_bias_expand0, and BT = 256
# consecutive columns of the flattened (axis 1, axis 2) plane everywhere else (test_tile_extents_are_the_kernels reads them)
E_BIAS = (32, 256, 256)

# largest |E - E_fft| seen over SHARPEN_CASES in units of the bin width, and what is allowed: ten times it.  It is rounding of
# the 512-point transforms divided by den, which the definition lets fall to 1e-12 of its maximum: the one-bin histogram at
# nb = 8 (sigma = 0.3 bins) sets the figure; every case with nb >= 200 stays below 5e-9.
SHARPEN_SEEN = 1.61e-5
SHARPEN_BAR = 10.0 * SHARPEN_SEEN
# largest relative deviation of the GPU's field from the model's seen over the correction cases below, and ten times it
FIELD_SEEN = 4.9e-14
FIELD_BAR = 10.0 * FIELD_SEEN


def _tile_shapes():
    shapes = []
    for axis in range(3):
        E = E_BIAS[axis]
        for n in (E - 1, E, E + 1, 2 * E + 1):
            s = [3, 5, 6]
            s[axis] = n
            shapes.append(tuple(s))
    return shapes


SHAPES = [(1, 1, 1), (2, 3, 1), (4, 4, 4), (5, 70, 3), (33, 30, 41)] + _tile_shapes()
IDS = ['x'.join(map(str, s)) for s in SHAPES]
SPANS = [(1, 1, 1), (1, 2, 4), (8, 3, 2), (2, 8, 3), (3, 2, 8)]
MASKS = ('full', 'random', 'one', 'half')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mask(kind, shape, seed=0):
    if kind == 'full':
        return np.ones(shape, np.uint8)
    if kind == 'random':
        return (np.random.default_rng(seed).random(shape) < 0.5).astype(np.uint8)
    m = np.zeros(shape, np.uint8)
    if kind == 'one':
        m[tuple(n // 2 for n in shape)] = 1
    else:                                                  # the half of the longest axis: whole spans hold no voxel
        a = int(np.argmax(shape))
        sl = [slice(None)] * 3
        sl[a] = slice(0, max(shape[a] // 2, 1))
        m[tuple(sl)] = 1
    return m


def _residual(shape, seed=1):
    """Both signs, a smooth part and noise."""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    return 0.2 * g[0] - 0.1 * g[1] * g[2] + 0.05 * np.random.default_rng(seed).standard_normal(shape)


def _log_volume(shape, seed=2):
    """Log intensities of three classes under a smooth field with a little noise, and a mask that leaves a corner out."""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    rng = np.random.default_rng(seed)
    classes = np.log(np.array(M.CLASS_VALUES))[rng.integers(0, 3, shape)]
    v = classes + 0.3 * (0.8 * g[0] - 0.5 * g[1] + 0.6 * g[2] * g[2]) + 0.01 * rng.standard_normal(shape)
    m = np.ones(shape, np.uint8)
    m[:max(shape[0] // 3, 1), :max(shape[1] // 3, 1), :max(shape[2] // 3, 1)] = 0
    if not m.any():
        m[...] = 1
    return v, m


# ------------------------------------------------------------------ CPU: the model itself
@pytest.mark.parametrize('shape', [(48, 40, 44), (33, 30, 41)], ids=['48x40x44', '33x30x41'])
def test_model_reduces_every_class_cv_tenfold(shape):
    """What the step is for.  Measured when this was written, both shapes alike: the class CVs fall from 0.140 / 0.103 / 0.061 to
    0.0027 / 0.0014 / 0.0019 (52x, 74x, 33x); the estimated field over the true one has a CV of 0.0028."""
    I, field, labels = M.phantom(shape)
    corrected, estimate, trace = M.correct(I)
    before, after = M.class_cvs(I, labels), M.class_cvs(corrected, labels)
    ratio = (estimate / field)[labels > 0]
    print('{}: CV {} -> {}, field CV {:.4f}, {} iterations'.format(shape, before, after, ratio.std() / ratio.mean(), len(trace)))
    assert all(b >= 10.0 * a for a, b in zip(after, before))
    assert ratio.std() / ratio.mean() < 0.01


def test_model_noise_and_empty_spans():
    """With 3 % multiplicative noise the class CVs end at the noise level; with half of the volume out of the mask, so that
    whole spans of the finest lattice are empty, the field stays finite and moderate everywhere."""
    shape = (33, 30, 41)
    I, field, labels = M.phantom(shape, noise=0.03, seed=4)
    corrected, _, _ = M.correct(I)
    after = M.class_cvs(corrected, labels)
    print('noise 0.03: class CVs', after)
    assert all(0.027 < a < 0.033 for a in after)
    I, field, labels = M.phantom(shape)
    half = np.zeros(shape, np.uint8)
    half[:shape[0] // 2] = 1
    corrected, estimate, _ = M.correct(I, half)
    print('half mask: field {:.3f} .. {:.3f}'.format(estimate.min(), estimate.max()))
    assert np.isfinite(estimate).all() and 0.5 < estimate.min() and estimate.max() < 2.0
    assert all(b >= 10.0 * a for a, b in zip(M.class_cvs(corrected, labels, half), M.class_cvs(I, labels, half)))


def test_axis_tables_are_the_models_and_sum_to_one():
    for n, spans in ((1, 1), (1, 8), (4, 64), (5, 3), (33, 8), (70, 2), (641, 7), (32000, 64)):
        s, w, c2, c3 = B.axisTable(n, spans)
        ms, mw, mc2, mc3 = M.axis_table(n, spans)
        assert np.array_equal(s, ms) and s.min() >= 0 and s.max() <= spans - 1 and (np.diff(s) >= 0).all()
        for a, b in ((w, mw), (c2, mc2), (c3, mc3)):
            assert np.array_equal(_bits(a), _bits(b)), (n, spans)
        assert np.abs(mw.sum(axis=1) - 1.0).max() <= 2.0 * np.finfo(np.float64).eps, (n, spans)
        assert (mw >= 0.0).all()


def _histograms(nb):
    k = np.arange(nb, dtype=np.float64)
    two = np.round(1000.0 * np.exp(-0.5 * ((k - 0.3 * nb) / (0.04 * nb + 0.5)) ** 2) + 600.0 * np.exp(-0.5 * ((k - 0.7 * nb) / (0.06 * nb + 0.5)) ** 2))
    one = np.zeros(nb)
    one[nb // 3] = 12345.0
    return {'two peaks': two, 'one bin': one, 'flat': np.full(nb, 50.0)}


SHARPEN_CASES = [(nb, kind, lim) for nb in (8, 200, 256) for kind in ('two peaks', 'one bin', 'flat') for lim in ((4.0, 5.5), (-0.3, 0.9))]


def test_sharpening_map_is_the_fft_restatement():
    worst = 0.0
    for nb, kind, (umin, umax) in SHARPEN_CASES:
        counts = _histograms(nb)[kind]
        before = counts.copy()
        E, F = B.sharpeningMap(counts, umin, umax), M.sharpen_fft(counts, umin, umax)
        h = (umax - umin) / (nb - 1)
        dev = float(np.abs(E - F).max()) / h
        print('nb {} {} [{}, {}]: max |E - E_fft| / h = {:.3e}'.format(nb, kind, umin, umax, dev))
        worst = max(worst, dev)
        assert np.isfinite(E).all() and np.array_equal(counts, before)
        assert np.array_equal(E, B.sharpeningMap(counts, umin, umax))          # a pure function
    print('worst {:.3e} bin widths'.format(worst))
    assert worst <= SHARPEN_BAR


def test_sharpening_map_sharpens():
    """Two blurred peaks move towards their centres: the map pulls the bins between and beside the peaks onto them."""
    nb, umin, umax = 200, 4.0, 5.5
    E = B.sharpeningMap(_histograms(nb)['two peaks'], umin, umax)
    centre = umin + np.arange(nb) * (umax - umin) / (nb - 1)
    lo, hi = centre[60], centre[140]
    assert abs(E[60] - lo) < 0.01 and abs(E[140] - hi) < 0.01                  # the peaks stay
    assert E[50] > centre[50] and E[70] < centre[70] and E[130] > centre[130] and E[150] < centre[150]
    assert (np.diff(E) > -1e-9).all()


def test_argument_errors_raise():
    """What the host can check is refused before a device is looked for: no GPU needed."""
    I = np.ones((6, 5, 4))
    nan, inf = float('nan'), float('inf')
    bad = [dict(volume=np.ones((6, 5))), dict(volume=np.ones((2, 6, 5, 4))), dict(mask=np.ones((6, 5, 5))), dict(mask=np.ones((6, 5))),
           dict(splineSpans=(1, 1)), dict(splineSpans=(0, 1, 1)), dict(splineSpans=(1, 33, 1)), dict(splineSpans=(1, 1.5, 1)), dict(splineSpans=2),
           dict(levels=0), dict(levels=7), dict(splineSpans=(1, 1, 3), levels=6), dict(splineSpans=(32, 1, 1), levels=3),
           dict(iterations=0), dict(iterations=201), dict(bins=7), dict(bins=257),
           dict(convergenceThreshold=0.0), dict(convergenceThreshold=nan), dict(convergenceThreshold=inf), dict(convergenceThreshold=-1.0),
           dict(fwhm=0.0), dict(fwhm=nan), dict(fwhm=inf), dict(noise=0.0), dict(noise=-0.01), dict(noise=nan), dict(noise=inf)]
    for kw in bad:
        args = dict(volume=I)
        args.update(kw)
        with pytest.raises(ValueError):
            B.biasFieldCorrection(**args)
        if 'volume' not in kw and 'mask' not in kw:
            with pytest.raises(ValueError):
                B.logBiasField(np.zeros((6, 5, 4)), np.ones((6, 5, 4)), **kw)
    with pytest.raises(ValueError):
        B.logBiasField(np.zeros((6, 5)), np.ones((6, 5)))
    with pytest.raises(ValueError):
        B.logBiasField(np.zeros((6, 5, 4)), np.ones((6, 5, 5)))
    for kw in (dict(spans=(0, 1, 1)), dict(spans=(1, 65, 1)), dict(spans=(1, 1)), dict(mask=np.ones((6, 5, 5)))):
        args = dict(residual=np.zeros((6, 5, 4)), mask=np.ones((6, 5, 4)), spans=(1, 1, 1))
        args.update(kw)
        with pytest.raises(ValueError):
            B.bsplineFit(**args)
    for phi, spans, shape in ((np.zeros((4, 4, 4)), (1, 1, 2), (6, 5, 4)), (np.zeros((4, 4, 4)), (1, 1, 1), (6, 5)), (np.zeros((4, 4, 4)), (1, 0, 1), (6, 5, 4))):
        with pytest.raises(ValueError):
            B.bsplineEval(phi, spans, shape)
    for kw in (dict(counts=np.ones(7)), dict(counts=np.ones(257)), dict(counts=np.ones((8, 8))), dict(umax=1.0), dict(umax=nan), dict(umin=-inf),
               dict(fwhm=0.0), dict(noise=nan)):
        args = dict(counts=np.ones(8), umin=1.0, umax=2.0)
        args.update(kw)
        with pytest.raises(ValueError):
            B.sharpeningMap(**args)
    for n, spans in ((0, 1), (32001, 1), (5, 0), (5, 65)):
        with pytest.raises(ValueError):
            B.axisTable(n, spans)
    with pytest.raises(ValueError):
        B.main('.', returnField=True)


def _refusals(dll, vol, f32, mask, out, shape, on_device_too=False):
    """Every refused input of the C entries: (label, return code).  `vol`, `f32`, `mask` and `out` are addresses of a float64
    volume, a float32 volume, a uint8 mask and a float64 output of that shape.  `on_device_too` adds the refusals that a device
    has to find: the empty masks."""
    keep = []

    def ints(*v):
        keep.append(np.array(v, dtype=np.intc))
        return keep[-1].ctypes.data
    nan, inf = float('nan'), float('inf')

    def loop(label, v=vol, m=mask, dims=shape, m0=(1, 1, 1), levels=2, iterations=3, threshold=1e-3, nb=200, fwhm=0.15, noise=0.01, to=out):
        return 'loop ' + label, dll.vmask_bias_log_field(0, v, m, *dims, ints(*m0) if m0 is not None else None, levels, iterations, threshold, nb, fwhm, noise, to, None, None)

    def correct(label, v=vol, dtype=6, m=mask, dims=shape, m0=(1, 1, 1), levels=2, iterations=3, threshold=1e-3, nb=200, fwhm=0.15, noise=0.01, to=out):
        return 'correct ' + label, dll.vmask_bias_correct(0, v, dtype, m, *dims, ints(*m0) if m0 is not None else None, levels, iterations, threshold, nb, fwhm, noise, to, None, None, None)

    def fit(label, r=vol, m=mask, dims=shape, spans=(1, 1, 1), to=out):
        return 'fit ' + label, dll.vmask_bias_fit(0, r, m, *dims, ints(*spans) if spans is not None else None, to)

    def evaluate(label, phi=vol, dims=shape, spans=(1, 1, 1), to=out):
        return 'eval ' + label, dll.vmask_bias_eval(0, phi, ints(*spans) if spans is not None else None, *dims, to)
    res = []
    for f in (loop, correct):
        res += [f('spans 0', m0=(0, 1, 1)), f('spans 33', m0=(1, 1, 33)), f('spans -1', m0=(1, -1, 1)), f('spans 3 x 2^5', m0=(1, 3, 1), levels=6),
                f('spans 32 x 2^2', m0=(32, 1, 1), levels=3), f('levels 0', levels=0), f('levels 7', levels=7),
                f('iterations 0', iterations=0), f('iterations 201', iterations=201), f('bins 7', nb=7), f('bins 257', nb=257),
                f('fwhm 0', fwhm=0.0), f('fwhm nan', fwhm=nan), f('fwhm inf', fwhm=inf), f('noise 0', noise=0.0), f('noise < 0', noise=-1.0),
                f('noise nan', noise=nan), f('threshold 0', threshold=0.0), f('threshold nan', threshold=nan), f('threshold inf', threshold=inf),
                f('null volume', v=None), f('null spans', m0=None), f('null out', to=None),
                f('shape 0', dims=(shape[0], 0, shape[2])), f('shape envelope', dims=(2000, 2000, 600))]
    res += [loop('null mask', m=None), correct('dtype 4', dtype=4), correct('dtype 7', v=f32, dtype=7)]
    res += [fit('spans 0', spans=(1, 0, 1)), fit('spans 65', spans=(65, 1, 1)), fit('null r', r=None), fit('null mask', m=None), fit('null spans', spans=None),
            fit('null phi', to=None), fit('shape 0', dims=(0, shape[1], shape[2])), fit('shape envelope', dims=(2000, 2000, 600)),
            evaluate('spans 0', spans=(1, 1, 0)), evaluate('spans 65', spans=(1, 65, 1)), evaluate('null phi', phi=None), evaluate('null spans', spans=None),
            evaluate('null out', to=None), evaluate('shape 0', dims=(shape[0], shape[1], 0)), evaluate('shape envelope', dims=(2000, 2000, 600))]
    return res


N_REFUSALS = 2 * 25 + 3 + 8 + 7


def test_c_entries_refuse_before_a_device_is_looked_for():
    """Host pointers, no GPU needed: every refusal is VRG_E_ARG and leaves the output alone."""
    dll = B._lib()
    shape = (4, 5, 6)
    I = np.full(shape, 3.0)
    I32 = I.astype(np.float32)
    mask = np.ones(shape, np.uint8)
    out = np.full(shape, -12345.0)
    res = _refusals(dll, I.ctypes.data, I32.ctypes.data, mask.ctypes.data, out.ctypes.data, shape)
    assert len(res) == N_REFUSALS
    for label, rc in res:
        assert rc == -1, label                           # VRG_E_ARG
    assert (out == -12345.0).all() and (I == 3.0).all() and (mask == 1).all()
    E = np.full(8, -12345.0)
    c = np.ones(8)
    for args in ((None, 8, 1.0, 2.0, 0.15, 0.01, E.ctypes.data), (c.ctypes.data, 8, 1.0, 2.0, 0.15, 0.01, None), (c.ctypes.data, 7, 1.0, 2.0, 0.15, 0.01, E.ctypes.data),
                 (c.ctypes.data, 257, 1.0, 2.0, 0.15, 0.01, E.ctypes.data), (c.ctypes.data, 8, 2.0, 2.0, 0.15, 0.01, E.ctypes.data),
                 (c.ctypes.data, 8, 1.0, float('nan'), 0.15, 0.01, E.ctypes.data), (c.ctypes.data, 8, 1.0, 2.0, 0.0, 0.01, E.ctypes.data),
                 (c.ctypes.data, 8, 1.0, 2.0, 0.15, float('inf'), E.ctypes.data)):
        assert dll.vmask_bias_sharpen(*args) == -1, args
    assert (E == -12345.0).all()


# ------------------------------------------------------------------ no GPU needed: the kernels
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vbias_device.hip')


def test_tile_extents_are_the_kernels():
    text = open(SOURCE).read()
    assert int(re.search(r'constexpr int EZ = (\d+);', text).group(1)) == E_BIAS[0]
    assert int(re.search(r'constexpr int BT = (\d+);', text).group(1)) == E_BIAS[1] == E_BIAS[2]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_bias_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vbias_device.hip' in build.SOURCES
    out = tmp_path / 'vbias_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vbias_device.hip'],
                       cwd=os.path.dirname(SOURCE), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1)),
                            int(re.search(r'\.vgpr_count:\s+(\d+)', m.group(2)).group(1)))
    counts = {k: sum(k in name for name in recs) for k in ('k_bias_fit', 'k_bias_expand0', 'k_bias_log', 'k_bias_exp', 'k_bias_minmax', 'k_bias_hist',
                                                           'k_bias_residual', 'k_bias_count')}
    # ("k_bias_exp" is in the names of k_bias_exp (2), k_bias_expand and k_bias_expand0 (2))
    assert counts == dict(k_bias_fit=3, k_bias_expand0=2, k_bias_log=2, k_bias_exp=5, k_bias_minmax=1, k_bias_hist=1, k_bias_residual=1, k_bias_count=1), sorted(recs)
    assert len(recs) == 14, sorted(recs)
    for name, (scratch, vgprs) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        # the first build: k_bias_fit 38 (first pass), 46 and 42; k_bias_expand 20, k_bias_expand0 20 and 24 (fused add); k_bias_log 42 and 38,
        # k_bias_exp 40 and 38, k_bias_minmax 14, k_bias_hist 20, k_bias_residual 18, k_bias_count 8
        assert vgprs <= 64, '%s uses %d VGPRs' % (name, vgprs)


# ------------------------------------------------------------------ GPU: fit and evaluation against the model
@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_fit_and_eval_are_the_model(shape):
    r = _residual(shape)
    rng = np.random.default_rng(7)
    for spans in SPANS:
        for kind in MASKS:
            m = _mask(kind, shape)
            before = r.copy()
            got, ref = B.bsplineFit(r, m, spans), M.fit(r, m, spans)
            label = '{} spans {} mask {}'.format(shape, spans, kind)
            assert got.dtype == np.float64 and got.shape == tuple(k + 3 for k in spans), label
            assert np.array_equal(_bits(got), _bits(ref)), '{}: {} control points differ'.format(label, int((got != ref).sum()))
            assert np.array_equal(r, before), label
            if (kind == 'one' and max(spans) > 1) or (kind == 'half' and shape == (33, 30, 41) and spans == (3, 2, 8)):
                assert (got == 0.0).any(), label             # control points that no mask voxel reaches: D2 == 0
        for phi in (ref, rng.standard_normal(ref.shape)):
            got, want = B.bsplineEval(phi, spans, shape), M.evaluate(phi, spans, shape)
            assert got.dtype == np.float64 and got.shape == tuple(shape)
            assert np.array_equal(_bits(got), _bits(want)), '{} spans {}: {} voxels differ'.format(shape, spans, int((got != want).sum()))


@pytest.mark.gpu
def test_fit_ignores_the_residual_outside_the_mask_and_takes_an_empty_mask():
    shape = (9, 8, 7)
    r = _residual(shape)
    m = _mask('random', shape)
    wild = r.copy()
    wild[m == 0] = np.nan
    assert np.array_equal(_bits(B.bsplineFit(wild, m, (2, 2, 2))), _bits(M.fit(r, m, (2, 2, 2))))
    assert np.array_equal(_bits(B.bsplineFit(r, np.zeros(shape, np.uint8), (2, 1, 3))), _bits(np.zeros((5, 4, 6))))


# ------------------------------------------------------------------ GPU: the loop against the model
def _phantom_log(shape):
    I, _, _ = M.phantom(shape)
    m = (I > 0).astype(np.uint8)
    return np.where(m != 0, np.log(np.where(m != 0, I, 1.0)), 0.0), m


LOOP_CASES = {'33x30x41': lambda: _phantom_log((33, 30, 41)), '5x70x3': lambda: _log_volume((5, 70, 3)), '31x6x257': lambda: _log_volume((31, 6, 257))}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(LOOP_CASES))
def test_log_field_is_the_model(case):
    """Every kernel of the loop at once: b and the trace, iteration counts included, bit for bit.  The model takes its
    sharpening map from the library's host entry, which test_sharpening_map_is_the_fft_restatement pins to np.fft."""
    v, m = LOOP_CASES[case]()
    before = v.copy()
    for m0 in ((1, 1, 1), (2, 1, 3)):
        got, trace = B.logBiasField(v, m, splineSpans=m0, levels=2, iterations=3, convergenceThreshold=1e-6)
        ref, want = M.log_field(v, m, m0=m0, levels=2, iterations=3, threshold=1e-6, sharpen=B.sharpeningMap)
        assert trace.shape == want.shape == (6, 4), (case, m0, trace.shape, want.shape)
        assert np.array_equal(trace, want), (case, m0, trace, want)
        assert np.array_equal(_bits(got), _bits(ref)), '{} {}: {} voxels differ, max {:.3e}'.format(case, m0, int((got != ref).sum()), np.abs(got - ref).max())
        assert np.array_equal(v, before) and np.abs(got).max() > 1e-3


@pytest.mark.gpu
def test_log_field_stops_at_once_and_ends_levels_early():
    shape = (12, 10, 9)
    m = _mask('random', shape)
    b, trace = B.logBiasField(np.full(shape, 4.25), m)
    assert trace.shape == (0, 4) and b.shape == shape and not b.any()             # a uniform volume: umin == umax
    v, m = _log_volume((20, 18, 16))
    got, trace = B.logBiasField(v, m, levels=3, iterations=5, convergenceThreshold=1e3)
    ref, want = M.log_field(v, m, levels=3, iterations=5, threshold=1e3, sharpen=B.sharpeningMap)
    assert np.array_equal(trace[:, 0], [0.0, 1.0, 2.0]) and np.array_equal(trace, want)      # one iteration per level
    assert np.array_equal(_bits(got), _bits(ref))
    # a threshold between the updates of the first level: the level ends in its midst, the count is the model's
    full = M.log_field(v, m, levels=1, iterations=6, threshold=1e-12, sharpen=B.sharpeningMap)[1]
    mid = float(np.sort(full[:, 1])[3])
    got, trace = B.logBiasField(v, m, levels=2, iterations=6, convergenceThreshold=mid)
    ref, want = M.log_field(v, m, levels=2, iterations=6, threshold=mid, sharpen=B.sharpeningMap)
    assert np.array_equal(trace, want) and 2 <= len(trace) < 12 and np.array_equal(_bits(got), _bits(ref))


# ------------------------------------------------------------------ GPU: the correction against the model
def _field_deviation(got, ref):
    return float(np.abs(got / ref - 1.0).max())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(48, 40, 44), (33, 30, 41)], ids=['48x40x44', '33x30x41'])
def test_correction_is_near_the_model_and_reduces_every_class_cv_tenfold(shape):
    """The device's log differs from numpy's in the last bit and may move a voxel across a bin edge: the field agrees to
    FIELD_BAR, ten times the largest deviation seen."""
    I, field, labels = M.phantom(shape)
    before = I.copy()
    got, est = B.biasFieldCorrection(I, returnField=True)
    ref, ref_field, _ = M.correct(I)
    dev = _field_deviation(est, ref_field)
    print('{}: max |field / model - 1| = {:.3e}'.format(shape, dev))
    assert got.dtype == est.dtype == np.float64 and got.shape == est.shape == shape and np.array_equal(I, before)
    assert dev <= FIELD_BAR
    assert np.abs(got - ref).max() <= FIELD_BAR * np.abs(ref).max()
    assert all(b >= 10.0 * a for a, b in zip(M.class_cvs(got, labels), M.class_cvs(I, labels)))
    ratio = (est / field)[labels > 0]
    assert ratio.std() / ratio.mean() < 0.01
    assert np.array_equal(_bits(B.biasFieldCorrection(I)), _bits(got))            # without the field: the same volume


@pytest.mark.gpu
def test_correction_with_noise_a_half_mask_and_other_input_types():
    shape = (33, 30, 41)
    I, _, labels = M.phantom(shape, noise=0.03, seed=4)
    got, est = B.biasFieldCorrection(I, returnField=True)
    ref, ref_field, _ = M.correct(I)
    print('noise: max |field / model - 1| = {:.3e}'.format(_field_deviation(est, ref_field)))
    assert _field_deviation(est, ref_field) <= FIELD_BAR and all(0.027 < a < 0.033 for a in M.class_cvs(got, labels))
    I, _, labels = M.phantom(shape)
    half = np.zeros(shape, np.uint8)
    half[:shape[0] // 2] = 1
    got, est = B.biasFieldCorrection(I, mask=half, returnField=True)
    ref, ref_field, _ = M.correct(I, half)
    print('half mask: max |field / model - 1| = {:.3e}'.format(_field_deviation(est, ref_field)))
    assert np.isfinite(est).all() and _field_deviation(est, ref_field) <= FIELD_BAR
    assert np.array_equal(got[I == 0], np.zeros(int((I == 0).sum())))             # the background stays 0
    for vol in (I.astype(np.float32), np.round(I).astype(np.int16)):
        before = vol.copy()
        got, est = B.biasFieldCorrection(vol, returnField=True, levels=2, iterations=4)
        ref, ref_field, _ = M.correct(vol, levels=2, iterations=4)
        print('{}: max |field / model - 1| = {:.3e}'.format(vol.dtype, _field_deviation(est, ref_field)))
        assert got.dtype == np.float64 and _field_deviation(est, ref_field) <= FIELD_BAR and np.array_equal(vol, before)
        assert np.abs(got - ref).max() <= FIELD_BAR * np.abs(ref).max()


@pytest.mark.gpu
def test_correction_256x256x192():
    shape = (256, 256, 192)
    I, _, labels = M.phantom(shape)
    I = I.astype(np.float32)
    got, est = B.biasFieldCorrection(I, returnField=True, levels=2, iterations=2)
    ref, ref_field, trace = M.correct(I, levels=2, iterations=2)
    dev = _field_deviation(est, ref_field)
    print('256x256x192: max |field / model - 1| = {:.3e}, {} iterations'.format(dev, len(trace)))
    assert dev <= FIELD_BAR and np.abs(got - ref).max() <= FIELD_BAR * np.abs(ref).max()


@pytest.mark.gpu
def test_correction_is_deterministic():
    I, _, _ = M.phantom((33, 30, 41), noise=0.03, seed=5)
    a, b = (B.biasFieldCorrection(I, returnField=True, levels=2, iterations=5) for _ in range(2))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    v, m = _log_volume((20, 18, 16))
    a, b = (B.logBiasField(v, m, levels=2, iterations=3) for _ in range(2))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------ GPU: device pointers, in a process of their own
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import bias as B
import bias_model as M
from test_bias import _refusals, _log_volume, _residual, _mask, N_REFUSALS
dev = torch.device('cuda', 0)
I, _, _ = M.phantom((33, 30, 41))
for dtype in (np.float32, np.float64):
    host = I.astype(dtype)
    t = torch.as_tensor(host, device=dev)
    got, field = B.biasFieldCorrection(t, returnField=True, levels=2, iterations=3)
    assert got.is_cuda and field.is_cuda and got.device == t.device and got.dtype == field.dtype == torch.float64 and tuple(got.shape) == I.shape
    ref, ref_field = B.biasFieldCorrection(host, returnField=True, levels=2, iterations=3)
    assert got.cpu().numpy().tobytes() == ref.tobytes() and field.cpu().numpy().tobytes() == ref_field.tobytes()
    again = B.biasFieldCorrection(t, levels=2, iterations=3)
    assert again.is_cuda and again.cpu().numpy().tobytes() == ref.tobytes()
    half = np.zeros(I.shape, np.uint8); half[:, :15] = 1
    for mask in (half, torch.as_tensor(half, device=dev)):
        got = B.biasFieldCorrection(t, mask=mask, levels=1, iterations=2)
        assert got.cpu().numpy().tobytes() == B.biasFieldCorrection(host, mask=half, levels=1, iterations=2).tobytes()
    assert t.cpu().numpy().tobytes() == host.tobytes()          # the input is unchanged
q = torch.as_tensor(np.round(I).astype(np.int16), device=dev)   # an integer tensor goes in as float64
assert B.biasFieldCorrection(q, levels=1, iterations=2).cpu().numpy().tobytes() == B.biasFieldCorrection(np.round(I), levels=1, iterations=2).tobytes()
v, m = _log_volume((20, 18, 16))
tv, tm = torch.as_tensor(v, device=dev), torch.as_tensor(m, device=dev)
b, trace = B.logBiasField(tv, tm, levels=2, iterations=3)
hb, htrace = B.logBiasField(v, m, levels=2, iterations=3)
assert b.is_cuda and b.cpu().numpy().tobytes() == hb.tobytes() and np.array_equal(trace, htrace) and tv.cpu().numpy().tobytes() == v.tobytes()
r, rm = _residual((20, 18, 16)), _mask('random', (20, 18, 16))
phi = B.bsplineFit(torch.as_tensor(r, device=dev), torch.as_tensor(rm, device=dev), (2, 3, 1))
hphi = B.bsplineFit(r, rm, (2, 3, 1))
assert phi.is_cuda and phi.cpu().numpy().tobytes() == hphi.tobytes()
F = B.bsplineEval(phi, (2, 3, 1), (20, 18, 16))
assert F.is_cuda and F.cpu().numpy().tobytes() == B.bsplineEval(hphi, (2, 3, 1), (20, 18, 16)).tobytes()
print('DEVICE RESIDENT OK')

shape = (4, 5, 6)
a = torch.full(shape, 3.0, dtype=torch.float64, device=dev)
a32 = a.to(torch.float32)
mask = torch.ones(shape, dtype=torch.uint8, device=dev)
out = torch.full(shape, -12345.0, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
dll = B._lib()
res = _refusals(dll, a.data_ptr(), a32.data_ptr(), mask.data_ptr(), out.data_ptr(), shape)
assert len(res) == N_REFUSALS
empty = torch.zeros(shape, dtype=torch.uint8, device=dev)
dark = torch.full(shape, -3.0, dtype=torch.float64, device=dev)
m0 = np.ones(3, np.intc)
res.append(('loop empty mask', dll.vmask_bias_log_field(0, a.data_ptr(), empty.data_ptr(), *shape, m0.ctypes.data, 2, 3, 1e-3, 200, 0.15, 0.01, out.data_ptr(), None, None)))
res.append(('correct empty mask', dll.vmask_bias_correct(0, a.data_ptr(), 6, empty.data_ptr(), *shape, m0.ctypes.data, 2, 3, 1e-3, 200, 0.15, 0.01, out.data_ptr(), None, None, None)))
res.append(('correct nothing positive', dll.vmask_bias_correct(0, dark.data_ptr(), 6, None, *shape, m0.ctypes.data, 2, 3, 1e-3, 200, 0.15, 0.01, out.data_ptr(), None, None, None)))
res.append(('correct mask off the positive voxels', dll.vmask_bias_correct(0, dark.data_ptr(), 6, mask.data_ptr(), *shape, m0.ctypes.data, 2, 3, 1e-3, 200, 0.15, 0.01, out.data_ptr(), None, None, None)))
for label, rc in res:
    assert rc == -1, label
torch.cuda.synchronize()
assert bool((out == -12345.0).all()) and bool((a == 3.0).all()) and bool((mask == 1).all())
print('REFUSALS OK')
"""


@functools.lru_cache(maxsize=None)
def _device_run():
    script = DEVICE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    return out.returncode, out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_bias_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, bit-identical to the host
    call and to a second run; the inputs are unchanged.  Own process: torch is imported before the HIP library there."""
    rc, stdout, tail = _device_run()
    assert 'DEVICE RESIDENT OK' in stdout, tail


@pytest.mark.gpu
def test_bias_refusals_with_device_pointers():
    """Every refused input of the C entries, with device pointers, the empty masks among them: VRG_E_ARG, the sentinel in the
    output untouched."""
    rc, stdout, tail = _device_run()
    assert rc == 0 and 'REFUSALS OK' in stdout, tail


# ------------------------------------------------------------------ GPU: the files
@pytest.mark.gpu
@pytest.mark.parametrize('with_mask', [False, True], ids=['positive', 'maskfile'])
def test_bias_main_feeds_denoise(tmp_path, capsys, with_mask):
    from arterynetwork_amd import nifti, denoise as DN
    shape = (24, 20, 16)
    I, _, _ = M.phantom(shape)
    aff = np.array([[0.5, 0, 0, -10.0], [0, 0.5, 0, 3.0], [0, 0, 0.75, 7.5], [0, 0, 0, 1.0]])
    folder = str(tmp_path)
    nifti.saveVolume(I, aff, os.path.join(folder, 'brainVolume.nii.gz'), astype=np.float32)
    I32 = I.astype(np.float32)
    mask = None
    if with_mask:
        mask = np.zeros(shape, np.uint8)
        mask[:, :12] = 1
        nifti.saveVolume(mask, aff, os.path.join(folder, 'brainVolumeMask.nii.gz'))
    kw = dict(levels=2, iterations=3)
    res = B.main(folder, fieldName='biasField.nii.gz', **kw)
    printed = capsys.readouterr().out
    for name in ('brainVolumeBiasCorrected.nii.gz', 'biasField.nii.gz'):
        assert '{} saved to {}.'.format(name, os.path.join(folder, name)) in printed
    want, want_field = B.biasFieldCorrection(I32, mask=mask, returnField=True, **kw)
    stored, aff2 = nifti.loadVolume(folder, 'brainVolumeBiasCorrected.nii.gz')
    field, aff3 = nifti.loadVolume(folder, 'biasField.nii.gz')
    assert res.dtype == np.float64 and np.array_equal(_bits(res), _bits(want))
    assert stored.dtype == np.float32 and np.array_equal(stored, want.astype(np.float32)) and np.allclose(aff2, aff)
    assert field.dtype == np.float32 and np.array_equal(field, want_field.astype(np.float32)) and np.allclose(aff3, aff)
    os.remove(os.path.join(folder, 'biasField.nii.gz'))
    B.main(folder, outputName='other.nii.gz', **kw)                               # no field unless asked for
    assert os.path.exists(os.path.join(folder, 'other.nii.gz')) and not os.path.exists(os.path.join(folder, 'biasField.nii.gz'))
    # denoise.main reads the corrected file when told to - and brainVolume.nii.gz when not
    den = DN.main(folder, conductance=15.0, iterations=2, volumeName='brainVolumeBiasCorrected.nii.gz')
    assert np.array_equal(_bits(den), _bits(DN.anisotropicDiffusion(stored, 15.0, 2, spacing=(0.5, 0.5, 0.75))))
    plain = DN.main(folder, conductance=15.0, iterations=2)
    assert np.array_equal(_bits(plain), _bits(DN.anisotropicDiffusion(I32, 15.0, 2, spacing=(0.5, 0.5, 0.75)))) and not np.array_equal(plain, den)
    assert np.array_equal(nifti.loadVolume(folder, 'brainVolumeDenoised.nii.gz')[0], plain.astype(np.float32))
