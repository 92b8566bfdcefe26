"""Centreline splines ("f20 centreline splines"): the sequential model of tests/centreline_model.py against
its own long-double run, against scipy's smoothing spline, against answers written out by hand and against the curvature of
digitised arcs and helices, on the CPU; then the GPU (vmask_centrelines / `branchSplines`) against the model bit for bit."""
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import centreline_model as CM
import morphometry_model as MM
import skeleton_model as M
import test_branches as TB
import test_morphometry as TM
from conftest import ROOT
from arterynetwork_amd import phantoms as P
from arterynetwork_amd import skeletonization as S
from arterynetwork_amd.skeletonization import branchMorphometry, branchSplines, deriveMorphometry

H = (0.4, 0.4, 0.7)                                                       # the spacing of the CPU comparisons
HG = (0.1, 0.3, 0.7)                                                      # the spacing of the GPU comparisons
# Measured with these very cases, float64 model against its long-double run (positions / the coordinate span max |y|, second
# derivatives / max |gamma| of the branch): 1.03e-11 and 1.55e-10, the largest at lambda = 2^20 l^3.  The allowance for the positions
# is the issue's: 16 x 5e-11; the one for gamma 16 x the measured figure.
LD_POSITION, LD_SECOND = 16 * 5e-11, 16 * 1.6e-10
# scipy's make_smoothing_spline against the long-double model on the cases of test_model_against_scipy: 3.73e-13 x span, 1.13e-11 x max |gamma|
SCIPY_POSITION, SCIPY_SECOND = 16 * 3.8e-13, 16 * 1.2e-11
# digitally straight branches, any lambda of the range, n up to 400: |g - y| <= 1.02e-15 span, |gamma| <= 7.1e-11 span / U^2 (U the branch's
# length; the largest at lambda_lo, where the spline interpolates the rounding of y), curvature <= 5.8e-5 / U
STRAIGHT_POSITION, STRAIGHT_SECOND, STRAIGHT_CURVATURE = 16 * 1.1e-15, 16 * 7.1e-11, 16 * 5.8e-5
STEPS26 = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)])


def _walk26(n, seed):
    """A random 26-connected walk of n entries (it may cross itself; no two consecutive entries are equal)."""
    return np.cumsum(np.vstack([[0, 0, 0], STEPS26[np.random.default_rng(seed).integers(0, 26, n - 1)]]), axis=0)


def _coords(t, b=0):
    return np.stack(np.unravel_index(t.voxels[t.offsets[b]:t.offsets[b + 1]], t.shape), axis=1)


# ------------------------------------------------------------------ CPU: the model against independent answers
@functools.lru_cache(maxsize=None)
def _pair(n, end_weight, k):
    """The float64 and the long-double fit of one walk at lambda = (2^-20, 1, 2^10, 2^20)[k] l^3: computed once, shared."""
    l2, l, lo, hi = CM.scale(H)
    lam = (2.0 ** -20, 1.0, 2.0 ** 10, 2.0 ** 20)[k] * (l2 * l)
    co = _walk26(n, 100 + n)
    p, q = CM.prepare(co, H, end_weight), CM.prepare(co, H, end_weight, np.longdouble)
    return p, CM.solve(p, lam), q, CM.solve(q, lam), lam


@pytest.mark.parametrize('n', [5, 64, 300, 2000])
def test_model_against_long_double(n):
    worst = [0.0, 0.0]
    for ew in (1.0, 20.0):
        for k in range(4):
            p, (g, gam, F), q, (gl, gaml, Fl), lam = _pair(n, ew, k)
            span, top = float(np.abs(q.y).max()), float(np.abs(gaml).max())
            dg, dgam = float(np.abs(g - gl).max()) / span, float(np.abs(gam - gaml).max()) / top
            print('n {:4d} endWeight {:4.0f} lambda {:.3e}: positions {:.3e} span, second derivatives {:.3e} of the largest'.format(n, ew, lam, dg, dgam))
            worst = [max(worst[0], dg), max(worst[1], dgam)]
            assert dg <= LD_POSITION and dgam <= LD_SECOND
            assert abs(float(F) - float(Fl)) <= 1e-6 * float(Fl) + 1e-20 * span * span
            assert (gam[0] == 0).all() and (gam[-1] == 0).all()
    print('n {}: largest {:.3e} span, {:.3e}'.format(n, *worst))


@pytest.mark.parametrize('n', [5, 64, 300, 2000])
def test_model_against_scipy(n):
    """lambda <= 2^10 l^3 only: scipy's own distance from the long-double solve grows to 1e-4 at 2^40."""
    interpolate = pytest.importorskip('scipy.interpolate')
    for ew in (1.0, 20.0):
        for k in range(3):
            p, (g, gam, F), q, (gl, gaml, Fl), lam = _pair(n, ew, k)
            w = np.ones(n)
            w[0] = w[-1] = ew
            sg, sgam = np.zeros((n, 3)), np.zeros((n, 3))
            for a in range(3):
                s = interpolate.make_smoothing_spline(p.u, p.y[:, a], w=w, lam=lam)
                sg[:, a], sgam[:, a] = s(p.u), s.derivative(2)(p.u)
            span, top = float(np.abs(q.y).max()), float(np.abs(gaml).max())
            print('n {:4d} endWeight {:4.0f} lambda {:.3e}: scipy - long double {:.3e} span, {:.3e}; model - scipy {:.3e} span, {:.3e}'.format(
                n, ew, lam, float(np.abs(sg - gl).max()) / span, float(np.abs(sgam - gaml).max()) / top, np.abs(sg - g).max() / span, np.abs(sgam - gam).max() / top))
            assert np.abs(sg - g).max() <= SCIPY_POSITION * span and np.abs(sgam - gam).max() <= SCIPY_SECOND * top


@pytest.mark.parametrize('step', [(1, 0, 0), (0, 0, 1), (1, 1, 1), (1, -1, 0), (0, 1, -1)])
def test_straight_branches_by_hand(step):
    """Every step the same: the data lie on a line, so g = y, gamma = 0 and the curvature is 0 at any lambda; the search takes
    lambda_hi at its first solve."""
    l2, l, lo, hi = CM.scale(H)
    for n in (3, 4, 5, 50, 400):
        co = np.arange(n)[:, None] * np.array(step)[None, :]
        for lam in (lo, lo * 2 ** 12, l2 * l, hi / 2 ** 10, hi):
            r = CM.fit_branch(co, H, smoothing=lam)
            span, U = np.abs(r['y']).max(), r['u'][-1]
            assert np.abs(r['g'] - r['y']).max() <= STRAIGHT_POSITION * span
            assert np.abs(r['second']).max() <= STRAIGHT_SECOND * span / (U * U)
            assert max(np.abs(r['curvature']).max(), r['maxCurvature'], r['meanCurvature']) <= STRAIGHT_CURVATURE / U
            assert abs(r['splineLength'] - U) <= 1e-12 * U
            want = np.array(step) * np.array(H)
            assert np.abs(r['tangent'] - want / np.linalg.norm(want)).max() <= 1e-9
        r = CM.fit_branch(co, H)
        assert (r['capped'], r['solves'], float(r['lambda'])) == (1, 1, hi)


def _dense(co, h, end_weight, lam):
    """The scaled system with dense matrices and numpy's solver."""
    p = CM.prepare(co, h, end_weight)
    n, m = p.n, p.m
    Q, R = np.zeros((n, m)), np.zeros((m, m))
    for j in range(m):
        Q[j, j], Q[j + 1, j], Q[j + 2, j] = p.r[j], -(p.r[j] + p.r[j + 1]), p.r[j + 1]
        R[j, j] = (p.hh[j] + p.hh[j + 1]) / 3
        if j + 1 < m:
            R[j, j + 1] = R[j + 1, j] = p.hh[j + 1] / 6
    Wi = np.diag(1 / p.w)
    c = np.linalg.solve(R / lam + Q.T @ Wi @ Q, Q.T @ p.y)
    return p.y - Wi @ Q @ c, c / lam


def test_short_branches():
    l2, l, lo, hi = CM.scale(H)
    two = CM.fit_branch([(3, 4, 5), (4, 4, 6)], H)
    assert np.array_equal(two['g'], two['y']) and not two['second'].any() and not two['curvature'].any()
    U = two['u'][-1]
    assert (two['solves'], two['capped'], two['residual']) == (1, 1, 0.0) and two['samples'] == max(3, int(np.ceil(U / (0.5 * l))) + 1) == 5
    assert 0.0 <= two['meanCurvature'] <= two['maxCurvature'] <= STRAIGHT_CURVATURE / U           # (the three-point statistic of samples on a segment)
    assert abs(two['splineLength'] - U) <= 16 * 2.0 ** -53 * U
    far = CM.fit_branch([(3, 4, 5), (4, 4, 6)], H, sample_step=100.0)
    assert far['samples'] == 3
    assert np.array_equal(two['position'][0], np.array([3, 4, 5]) * np.array(H)) and np.array_equal(two['tangent'][0], two['tangent'][1])
    for co in ([(0, 0, 0), (1, 1, 0), (2, 1, 1)], [(0, 0, 0), (1, 0, 0), (1, 1, 1), (2, 2, 1)], [(5, 5, 5), (4, 5, 6), (4, 6, 7), (3, 6, 8), (3, 7, 8)]):
        for ew in (1.0, 20.0):
            for lam in (lo * 2 ** 8, l2 * l, 2.0 ** 10 * l2 * l):
                r = CM.fit_branch(co, H, smoothing=lam, end_weight=ew)
                g, gam = _dense(co, H, ew, lam)
                assert np.abs(r['g'] - g).max() <= 1e-10 * np.abs(r['y']).max()
                assert np.abs(r['second'][1:-1] - gam).max() <= 1e-9 * max(np.abs(gam).max(), 1e-300) and not r['second'][[0, -1]].any()
                assert r['solves'] == 1 and r['capped'] == 0


def test_smallest_lambda_returns_the_data():
    """By the definition itself y - g = lambda W^-1 Q gamma.  On a gentle curve sampled by long steps (a legal table: a pair that is
    no 26-neighbour is an ordinary, longer step) that term is below the long-double allowance at lambda_lo, so the positions return
    the data.  On a voxel staircase it is not: the interpolating spline's gamma changes by about 1 / l from knot to knot, and lambda_lo
    leaves 2.0e-8 to 1.3e-7 of the span (random walks of 5 to 2000 entries, the same in long double) - printed here, not asserted:
    that is what lambda_lo means, not rounding."""
    l2, l, lo, hi = CM.scale(H)
    t = np.linspace(0.0, 1.5, 40)
    co = np.rint(np.stack([2000 * np.cos(t), 2000 * np.sin(t), 300 * t], axis=1)).astype(np.int64)
    for ew in (1.0, 20.0):
        r = CM.fit_branch(co, H, smoothing=lo, end_weight=ew)
        span = np.abs(r['y']).max()
        print('coarse arc, endWeight {}: |g - y| = {:.3e} span'.format(ew, np.abs(r['g'] - r['y']).max() / span))
        assert np.abs(r['g'] - r['y']).max() <= LD_POSITION * span
    for n in (5, 64, 300, 2000):
        r = CM.fit_branch(_walk26(n, 100 + n), H, smoothing=lo)
        print('walk of {} entries: |g - y| = {:.3e} span'.format(n, np.abs(r['g'] - r['y']).max() / np.abs(r['y']).max()))


def test_search_on_a_random_graph():
    t = TM._of_volume(TB._random((24, 24, 24), 0.1, 41))
    l2, l, lo, hi = CM.scale(HG)
    kinds = {0: 0, 1: 0, 2: 0}
    for b in range(len(t.offsets) - 1):
        co = _coords(t, b)
        trace = []
        r = CM.fit_branch(co, HG, trace=trace)
        target = 0.25 * l2 * len(co)
        kinds[r['capped']] += 1
        if r['capped'] == 1:
            assert r['solves'] == 1 and float(r['lambda']) == hi and r['residual'] <= target
            continue
        assert r['solves'] == 25 and len(trace) == 26
        trials, (up, F_up) = sorted(trace[:25], key=lambda x: float(x[0])), trace[25]
        F = [float(x[1]) for x in trials]
        assert all(a <= b * (1 + 1e-9) for a, b in zip(F[:-1], F[1:])), 'F must not decrease with lambda'
        assert lo <= float(r['lambda']) < float(up) <= hi and F_up > target
        assert r['capped'] == 2 or r['residual'] <= target
        assert float(up) / float(r['lambda']) <= (hi / lo) ** (2.0 ** -24) * (1 + 1e-9)       # the bracket after 24 halvings of its logarithm
    print('branches', len(t.offsets) - 1, 'uncapped / capped at lambda_hi / at lambda_lo', kinds)
    assert kinds[0] > 0 and kinds[1] > 0


def _raw_mean_curvature(co, h):
    y = np.asarray(co, np.float64) * np.asarray(h)
    return float(np.mean([CM.triangle(y[k - 1], y[k], y[k + 1]) for k in range(1, len(y) - 1)]))


@pytest.mark.parametrize('kind', ['arc', 'helix'])
@pytest.mark.parametrize('radius', [10, 20, 40])
def test_curvature_of_digitised_curves(kind, radius):
    """Three quarters of a circle and a helix of pitch radius / 3 per radian, digitised (`phantoms.digitise_curve`), the defaults.
    Measured: meanCurvature 3.7 to 6.9 % below the true value, the per-entry mean 4.3 to 10.6 % below (natural ends flatten the
    curve); the raw voxel polyline's three-point curvature 3 to 24 times the true value."""
    pts = P.arc_curve(radius) if kind == 'arc' else P.helix_curve(radius)
    true = 1.0 / radius if kind == 'arc' else radius / (radius ** 2 + (radius / 3.0) ** 2)
    co = P.digitise_curve(pts)
    assert (np.abs(np.diff(co, axis=0)).max(axis=1) == 1).all() and (np.abs(co[2:] - co[:-2]).max(axis=1) == 2).all()
    r = CM.fit_branch(co, (1.0, 1.0, 1.0))
    raw = _raw_mean_curvature(co, (1.0, 1.0, 1.0))
    print('{} of radius {}: n {}, lambda {:.4g}, meanCurvature / true {:.4f}, entries / true {:.4f}, max / true {:.4f}, raw polyline / true {:.2f}'.format(
        kind, radius, len(co), float(r['lambda']), r['meanCurvature'] / true, r['curvature'].mean() / true, r['maxCurvature'] / true, raw / true))
    assert r['capped'] == 0
    assert abs(r['meanCurvature'] - true) <= 0.15 * true
    assert abs(r['curvature'].mean() - true) <= 0.15 * true
    assert raw >= 2 * true
    length = np.linalg.norm(np.diff(pts, axis=0), axis=1).sum()
    assert 0.9 * length <= r['splineLength'] <= length


def _spline_directions(t, spacing, **kw):
    """(B x 2 x 3) local directions from the model's tangents: the tangent at the first entry, minus the tangent at the last."""
    c = CM.centrelines(t.shape, t.offsets, t.voxels, spacing, **kw)
    return np.stack([c['tangent'][t.offsets[:-1]], -c['tangent'][t.offsets[1:] - 1]], axis=1)


def test_spline_directions_on_straight_arms():
    t = TM._of_volume(TM._planar_y())
    raw = TM._model(t, TM._dist_for(t.shape))
    chord = TM._derive(t, raw)
    spline = TM._derive(t, dict(raw, localDirection=_spline_directions(t, (1.0, 1.0, 1.0))))
    assert len(chord['bifurcationNode']) == 1 and np.array_equal(chord['bifurcationBranches'], spline['bifurcationBranches'])
    print('localBifurcationAmplitude: chord', chord['localBifurcationAmplitude'], 'spline', spline['localBifurcationAmplitude'])
    assert abs(chord['localBifurcationAmplitude'][0] - 90.0) <= 1e-12
    # two unit tangents, each off its arm's direction by at most |gamma| U / |f'| <= STRAIGHT_SECOND span / U <= STRAIGHT_SECOND radians
    assert abs(spline['localBifurcationAmplitude'][0] - 90.0) <= 2 * np.degrees(STRAIGHT_SECOND) + 1e-12
    for k in S.MORPHOMETRY_BRANCH:
        assert np.array_equal(chord[k], spline[k], equal_nan=True) or k == 'localBifurcationTorque'


def test_spline_directions_on_the_reference_trees():
    """Nothing asserted: the reference's local direction is a FITPACK spline's derivative, ours a different spline's.  Prints, per
    quantity, the largest distance of the local angles to the recorded reference under both settings (DESIGN.md has the figures)."""
    import test_morphometry_reference as TR
    worst = {}
    for case in TR.CASES:
        fx = TR._fixture(case)
        t = fx.table
        raw = MM.morphometry(t.shape, fx.dist, t.offsets, t.voxels, t.ends, t.node_voxel, (1.0, 1.0, 1.0), fx.roots, TR.LOCAL_STEPS)
        both = {'chord': deriveMorphometry(raw, t.offsets, t.ends, t.kind, (1.0, 1.0, 1.0)),
                'spline': deriveMorphometry(dict(raw, localDirection=_spline_directions(t, (1.0, 1.0, 1.0))), t.offsets, t.ends, t.kind, (1.0, 1.0, 1.0))}
        for mode, d in both.items():
            for key in ('localBifurcationAmplitude', 'localBifurcationTilt'):
                rows = d['bifurcationNode']
                want = fx.z['node_' + key][rows]
                ok = ~np.isnan(want) & ~np.isnan(d[key]) & np.array([v not in fx.deviating_nodes() for v in rows.tolist()], bool)
                if ok.any():
                    e = float(np.abs(d[key][ok] - want[ok]).max())
                    worst[(mode, key)] = max(worst.get((mode, key), 0.0), e)
                    print('{:10s} {:7s} {:28s} largest distance {:8.3f} degrees over {} nodes'.format(case, mode, key, e, int(ok.sum())))
    for k, v in sorted(worst.items()):
        print('largest', k, '{:.3f}'.format(v))


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_centreline_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vcl_device.hip' in build.SOURCES
    out = tmp_path / 'vcl_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vcl_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
        recs[m.group(1)] = (f('private_segment_fixed_size'), f('vgpr_count'))
    for frag in ('k_cl_check', 'k_cl_fit'):
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, (scratch, vgpr) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        assert vgpr <= 128, '%s uses %d VGPRs' % (name, vgpr)


def test_arguments_are_checked_before_the_library_is_asked():
    g = TM._helix(20).graph()
    l2, l, lo, hi = S.splineScale(HG)
    assert (l2, l, lo, hi) == CM.scale(HG)
    for kw in (dict(endWeight=0.0), dict(endWeight=-1.0), dict(endWeight=float('nan')), dict(sampleStep=0.0), dict(sampleStep=-0.5), dict(residualPerPoint=0.0),
               dict(smoothing=float(np.nextafter(lo, 0.0))), dict(smoothing=float(np.nextafter(hi, np.inf))), dict(smoothing=float('inf')), dict(smoothing=0.0),
               dict(spacing=(0.001, float(np.nextafter(1.0, 2.0)), 0.5)), dict(spacing=(0.0, 1.0, 1.0)), dict(spacing=(1.0, float('nan'), 1.0))):
        with pytest.raises(ValueError):
            branchSplines(g, **dict(dict(spacing=HG), **kw))
    with pytest.raises(ValueError):
        branchMorphometry(g, dist=np.ones(g.skeleton.shape), localDirection='tangent')


# ------------------------------------------------------------------ GPU: exactly the model
_KW = {'smoothing': 'smoothing', 'endWeight': 'end_weight', 'residualPerPoint': 'residual_per_point', 'sampleStep': 'sample_step'}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_equal_to_model(got, want):
    for k in S.SPLINE_ENTRY + S.SPLINE_BRANCH:
        a, b = np.asarray(getattr(got, k)), want['lambda' if k == 'smoothing' else k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        same = _bits(a) == _bits(b) if a.dtype == np.float64 else a == b
        assert same.all(), (k, int((~same).sum()), 'of', same.size, 'first at', np.argwhere(~same)[0].tolist(), a[~same][:3], b[~same][:3])


def _check(t, spacing=HG, ldsEntries=0, **kw):
    got = branchSplines(t.graph(), spacing=spacing, ldsEntries=ldsEntries, **kw)
    want = CM.centrelines(t.shape, t.offsets, t.voxels, spacing, **{_KW[k]: v for k, v in kw.items()})
    _assert_equal_to_model(got, want)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize('n', [2, 3, 4, 5, 6, 17, 63, 64, 65, 66, 128, 129, 1000])
def test_single_branches(n):
    """The lengths around the lane stride, the systems of size 0, 1 and 2 and a branch of many trips; a straight line and a helix;
    a fixed lambda and the search; end weights 1 and 20.  The helix of 1000 entries also through the global work space."""
    l2, l, lo, hi = CM.scale(HG)
    line = TM._of_volume(np.ones((1, 1, n), np.uint8))
    assert np.diff(line.offsets).tolist() == [n]
    for ew in (1.0, 20.0):
        _check(line, endWeight=ew, smoothing=8.0 * l2 * l)
        got, want = _check(line, endWeight=ew)
        assert want['capped'].tolist() == [1]
    if n >= 3:
        h = TM._helix(n)
        for ew in (1.0, 20.0):
            _check(h, endWeight=ew, smoothing=8.0 * l2 * l)
            got, want = _check(h, endWeight=ew)
        if n == 1000:
            assert want['capped'].tolist() == [0] and want['solves'].tolist() == [25]
            forced = branchSplines(h.graph(), spacing=HG, ldsEntries=64)
            _assert_equal_to_model(forced, want)
            for k in got.names():
                assert getattr(got, k).tobytes() == getattr(forced, k).tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize('density,seed', [(0.1, 41), (0.3, 42), (0.6, 43)])
def test_many_branches(density, seed):
    """Unthinned random volumes: many branches of 2 to 10 entries share a launch; closed curves, loops on a cluster, jump pairs."""
    t = TM._of_volume(TB._random((24, 24, 24), density, seed))
    n = np.diff(t.offsets)
    info = {}
    got = branchSplines(t.graph(), spacing=HG, info=info)
    want = CM.centrelines(t.shape, t.offsets, t.voxels, HG)
    _assert_equal_to_model(got, want)
    print(density, 'branches', len(n), 'lengths', int(n.min()), int(n.max()), info)
    assert len(n) > 0 and info['solves'] == want['solves'].sum() and info['capped'] == (want['capped'] != 0).sum() and info['kernel_ms'] > 0
    forced = branchSplines(t.graph(), spacing=HG, ldsEntries=4)           # most branches through the global work space
    _assert_equal_to_model(forced, want)


def _call(dll, t, spacing, end_weight, smoothing, rho, step, lds=0):
    B, E = len(t.offsets) - 1, len(t.voxels)
    outs = [np.full(11 * E, -77.0), np.full(5 * B, -77.0), np.full(3 * B, -77, np.int64)]
    h = np.array(spacing, np.float64)
    voxels = np.ascontiguousarray(t.voxels, np.int64)
    rc = dll.vmask_centrelines(0, *t.shape, t.offsets.ctypes.data, B, voxels.ctypes.data, h.ctypes.data, end_weight, smoothing, rho, step, lds,
                               *(a.ctypes.data for a in outs), None)
    return rc, dll.vmask_last_error(), all((a == -77).all() for a in outs)


@pytest.mark.gpu
def test_refusals_and_the_empty_table():
    dll = S._skeleton_lib()
    l2, l, lo, hi = CM.scale(HG)
    good = TM._helix(20)
    ok = (HG, 20.0, 0.0, 0.25 * l2, 0.5 * l)
    rc, msg, untouched = _call(dll, good, *ok)
    assert rc == 0 and not untouched
    repeated = TM._helix(20)
    repeated.voxels = repeated.voxels.copy(); repeated.voxels[7] = repeated.voxels[6]
    outside = TM._helix(20)
    outside.voxels = outside.voxels.copy(); outside.voxels[7] = int(np.prod(outside.shape))
    for t, frag in ((repeated, b'zero step'), (outside, b'out of range')):
        rc, msg, untouched = _call(dll, t, *ok)
        assert rc == -1 and frag in msg and untouched, (rc, msg)
        with pytest.raises(Exception):
            branchSplines(t.graph(), spacing=HG)
    above = float(np.nextafter(1.0, 2.0))
    for args, frag in ((((0.001, above, 0.5),) + ok[1:], b'spacing'), ((HG, 0.0) + ok[2:], b'end_weight'), ((HG, -2.0) + ok[2:], b'end_weight'),
                       ((HG, 20.0, float(np.nextafter(hi, np.inf))) + ok[3:], b'lambda'), ((HG, 20.0, float(np.nextafter(lo, 0.0))) + ok[3:], b'lambda'),
                       ((HG, 20.0, float('nan')) + ok[3:], b'lambda'), ((HG, 20.0, 0.0, 0.0, ok[4]), b'residual_per_point'), ((HG, 20.0, 0.0, ok[3], 0.0), b'sample_step')):
        rc, msg, untouched = _call(dll, good, *args)
        assert rc == -1 and frag in msg and untouched, (args, rc, msg)
    rc, msg, untouched = _call(dll, good, *ok, lds=513)
    assert rc == -1 and untouched
    _check(good, smoothing=lo)                                            # both ends of the range are accepted
    _check(good, smoothing=hi)
    _check(TM._of_volume(TB._star((6, 5, 7))), spacing=(0.001, 1.0, 0.5))  # a ratio of exactly 1000 is accepted
    # two branches that meet at a node: the last entry of one is the first of the next, and that is no zero step
    a, b = [(0, 0, k) for k in range(5)], [(0, 0, 4), (0, 1, 5), (0, 2, 6), (0, 3, 6)]
    v = np.ravel_multi_index(np.array(a + b).T, (2, 5, 8))
    assert v[4] == v[5]
    _check(TM.Tables((2, 5, 8), [0, 5, 9], v, [[0, 1], [1, 2]], [v[0], v[4], v[8]]))
    empty = TM.Tables((4, 5, 6), [0], [], np.zeros((0, 2), np.int64), [])
    got, want = _check(empty)
    assert got.position.shape == (0, 3) and got.u.shape == (0,) and got.meanCurvature.shape == (0,) and got.solves.dtype == np.int64


@pytest.mark.gpu
def test_repeats_are_bit_identical():
    t = TM._of_volume(TB._random((24, 24, 24), 0.3, 42))
    a, b = branchSplines(t.graph(), spacing=HG), branchSplines(t.graph(), spacing=HG)
    assert a.names() == list(S.SPLINE_ENTRY + S.SPLINE_BRANCH)
    for k in a.names():
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    assert a.endWeight == 20.0 and a.fixedSmoothing is None and np.array_equal(a.spacing, HG)


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import skeletonization as S
import test_centrelines as T
v = T.TB._random((24, 24, 24), 0.3, 42)
dev = torch.device('cuda', 0)
gh = S.branchGraph(v)
gd = S.branchGraph(torch.as_tensor(v, device=dev))
h = S.branchSplines(gh, spacing=T.HG)
d = S.branchSplines(gd, spacing=T.HG)
t = T.TM._of_volume(v)
T._assert_equal_to_model(h, T.CM.centrelines(t.shape, t.offsets, t.voxels, T.HG))
for name in h.names():
    a, b = getattr(d, name), getattr(h, name)
    assert a.is_cuda and a.device == dev and tuple(a.shape) == b.shape, name
    assert a.cpu().numpy().tobytes() == b.tobytes(), name
assert d.position.dtype == torch.float64 and d.solves.dtype == torch.int64
dist = T.TM._dist_for(v.shape)
mh = S.branchMorphometry(gh, dist=dist, spacing=T.HG, localDirection='spline')
md = S.branchMorphometry(gd, dist=dist, spacing=T.HG, localDirection='spline', splines=d)
for name in mh.names():
    assert getattr(md, name).cpu().numpy().tobytes() == getattr(mh, name).tobytes(), name
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_splines_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, equal to the host call.
    Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['planar-y', 'star', 'random'])
def test_morphometry_with_spline_directions(case):
    v = {'planar-y': TM._planar_y, 'star': functools.partial(TB._star, (6, 5, 7)), 'random': functools.partial(TB._random, (24, 24, 24), 0.1, 41)}[case]()
    t = TM._of_volume(v)
    dist = TM._dist_for(t.shape)
    got = branchMorphometry(t.graph(), dist=dist, spacing=HG, localDirection='spline')
    chord = branchMorphometry(t.graph(), dist=dist, spacing=HG)
    raw = TM._model(t, dist, HG)
    TM._assert_equal_to_model(chord, raw, t, HG)                          # the default is what it was
    want = deriveMorphometry(dict(raw, localDirection=_spline_directions(t, HG)), t.offsets, t.ends, t.kind, HG)
    assert got.names() == chord.names() and got.localDirection == 'spline' and chord.localDirection == 'chord'
    for k in S.MORPHOMETRY_BRANCH + S.MORPHOMETRY_BIFURCATION:
        a, b = np.asarray(getattr(got, k)), want[k]
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype == np.float64), k
    for k in S.MORPHOMETRY_RAW:
        assert np.asarray(getattr(got, k)).tobytes() == np.asarray(getattr(chord, k)).tobytes(), k
    if case != 'random':
        assert len(got.bifurcationNode) == 1


@pytest.mark.gpu
def test_main_writes_the_files(tmp_path, capsys):
    from arterynetwork_amd import nifti
    m = M.crossing_phantom((48, 48, 32))
    m[10, 33:45, 15:17] = 1
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    plain, curved, alone = tmp_path / 'plain', tmp_path / 'curved', tmp_path / 'alone'
    for d in (plain, curved, alone):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    with pytest.raises(ValueError):
        S.main(str(curved), segments=True, curvature=True)
    before = S.main(str(plain), segments=True, prune=(3, 1.0), morphometry=True)
    capsys.readouterr()
    after = S.main(str(curved), segments=True, prune=(3, 1.0), morphometry=True, curvature=True)
    said = capsys.readouterr().out
    S.main(str(alone), segments=True, prune=(3, 1.0), curvature=True)
    assert sorted(os.listdir(str(curved))) == sorted(os.listdir(str(plain)) + [S.SPLINE_FILE])
    assert '{} saved to {}.'.format(S.SPLINE_FILE, os.path.join(str(curved), S.SPLINE_FILE)) in said
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after))
    for name in os.listdir(str(plain)):
        if name in (S.BRANCH_FILE, S.SEGMENT_INFO_FILE):
            continue
        assert (plain / name).read_bytes() == (curved / name).read_bytes(), name
    graph = S.branchGraph(S.skeletonize(m), minSpurLength=3, radiusFactor=1.0, vesselVolumeMask=m)
    _, stored = nifti.loadVolume(str(curved), 'vesselVolumeMask.nii.gz')
    spacing = np.sqrt((np.asarray(stored, np.float64)[:3, :3] ** 2).sum(axis=0))
    want = branchSplines(graph, spacing=spacing)
    for folder in (curved, alone):
        z = np.load(str(folder / S.SPLINE_FILE))
        assert z['names'].tolist() == want.names() and np.array_equal(z['spacing'], spacing) and float(z['endWeight']) == 20.0 and np.isnan(z['fixedSmoothing'])
        assert float(z['residualPerPoint']) == want.residualPerPoint and float(z['sampleStep']) == want.sampleStep
        for k in want.names():
            assert z[k].dtype == getattr(want, k).dtype and z[k].tobytes() == getattr(want, k).tobytes(), k
    with open(str(plain / S.SEGMENT_INFO_FILE), 'rb') as f:
        old = pickle.load(f)
    with open(str(curved / S.SEGMENT_INFO_FILE), 'rb') as f:
        new = pickle.load(f)
    added = {'maxCurvature', 'meanCurvature', 'splineLength', 'maxCurvatureAveragedInmm', 'meanCurvatureAveragedInmm'}
    assert sorted(old) == sorted(new) and len(new) > 0
    for k, d in new.items():
        assert set(d) == set(old[k]) | added and not added & set(old[k]) and all(d[key] == old[k][key] for key in old[k])
        assert all(type(d[key]) is float for key in added)
        assert d['maxCurvature'] == want.maxCurvature[k] == d['maxCurvatureAveragedInmm'] and d['meanCurvature'] == want.meanCurvature[k] == d['meanCurvatureAveragedInmm']
        assert d['splineLength'] == want.splineLength[k]
