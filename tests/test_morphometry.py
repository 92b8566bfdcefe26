"""Branch morphometry ("f11 branch morphometry"): the sequential model tests/morphometry_model.py is checked
against answers written out by hand and against numpy's own formulas on the CPU, then the GPU (vmask_morphometry /
skeletonization.branchMorphometry) must equal it: every integer array and the bits of every float64 sum (radiusSum, radiusDevSq,
pathLength, pathDistance); the derived floats are compared after the same host formulas (skeletonization.deriveMorphometry)."""
import functools
import math
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import branch_model as BM
import morphometry_model as MM
import skeleton_model as M
import test_branches as TB
from conftest import ROOT
from arterynetwork_amd import skeletonization as S
from arterynetwork_amd.skeletonization import branchMorphometry, deriveMorphometry, pathLengths

U = 2.0 ** -53                                                          # the unit round-off of a double
SUMS = ('radiusSum', 'radiusDevSq', 'pathLength', 'pathDistance')


# ------------------------------------------------------------------ graphs
class Tables:
    """A branch table: what vmask_branches returns (or a hand-made one), as the model and `branchMorphometry` take it."""

    def __init__(self, shape, offsets, voxels, ends, node_voxel, kind=None, degree=None):
        self.shape = tuple(shape)
        self.offsets, self.voxels = np.asarray(offsets, np.int64), np.asarray(voxels, np.int64)
        self.ends, self.node_voxel = np.asarray(ends, np.int64).reshape(-1, 2), np.asarray(node_voxel, np.int64)
        N = len(self.node_voxel)
        self.kind = np.zeros(N, np.int64) if kind is None else np.asarray(kind, np.int64)
        self.degree = np.bincount(self.ends[self.ends >= 0], minlength=N).astype(np.int64) if degree is None else np.asarray(degree, np.int64)

    def graph(self):
        co = lambda v: np.stack(np.unravel_index(v, self.shape), axis=1).astype(np.int64).reshape(len(v), 3)
        sk = np.zeros(self.shape, np.uint8)
        sk.ravel()[self.voxels] = 1
        return S.BranchGraph(sk, co(self.node_voxel), self.kind, np.ones(len(self.kind), np.int64), self.degree, self.ends, self.offsets, co(self.voxels), {})

    def node_at(self, p):
        return int(np.flatnonzero(self.node_voxel == np.ravel_multi_index(p, self.shape))[0])


def _of_volume(volume):
    sk, g = BM.branch_graph(np.asarray(volume), 0, 0.0, None, 64)
    return Tables(np.shape(volume), g.offsets, g.voxels, g.ends, g.nodes[:, 0], g.nodes[:, 1], g.nodes[:, 3])


def _path(shape, points):
    """One branch through `points` between two end points."""
    v = np.ravel_multi_index(np.asarray(points).T, shape)
    return Tables(shape, [0, len(v)], v, [[0, 1]] if v[0] < v[-1] else [[1, 0]], sorted((v[0], v[-1])))


def _walk(start, steps):
    p, out = np.array(start), [tuple(start)]
    for s in steps:
        p = p + s
        out.append(tuple(int(c) for c in p))
    return out


ALL_CLASSES = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
# no voxel twice: three voxels per plane of axis 0 at most, and axis 0 never steps back
HELIX = [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, -1), (0, -1, 0), (1, 1, 1), (1, -1, -1)]


def _helix(n):
    steps = [HELIX[i % 7] for i in range(n - 1)]
    return _path((3 * (n // 7 + 2), 4, 4), _walk((0, 1, 1), steps))


def _double_tee():
    """A line with two perpendicular arms two voxels apart: one cluster of seven junction voxels, represented by the first arm's
    foot; the far half of the line and the second arm end at members that are no neighbours of it - two jump pairs."""
    v = np.zeros((12, 11, 3), np.uint8)
    v[0:12, 5, 1] = 1
    v[5, 6:11, 1] = 1
    v[7, 0:5, 1] = 1
    return v


def _planar_y(arm=7):
    """In the plane of axes 0 and 1: a straight parent along axis 0 up to a junction voxel, two children at +-45 degrees."""
    v = np.zeros((2 * arm + 3, 2 * arm + 3, 3), np.uint8)
    c = arm + 1
    v[0:arm + 1, c, 1] = 1
    for k in range(1, arm + 1):
        v[arm + k, c + k, 1] = v[arm + k, c - k, 1] = 1
    return v


def _tie_ring():
    """The ring of test_branches with a tail at either side: two half rings of equal step counts between the two junctions."""
    v = TB._free_ring().copy()
    v[0:2, 4, 1] = 1
    v[7:9, 4, 1] = 1
    return v


def _long_comb(teeth=40):
    """A backbone along axis 0 with one two-voxel tooth every four voxels: a chain of `teeth` junctions."""
    v = np.zeros((4 * teeth + 5, 9, 9), np.uint8)
    v[:, 4, 4] = 1
    steps = [(0, 1, 1), (0, -1, -1), (0, 1, -1), (0, -1, 1)]
    for k in range(teeth):
        TB._arm(v, (4 + 4 * k, 4, 4), steps[k % 4], 2)
    return v


def _two_components():
    v = np.zeros((14, 14, 30), np.uint8)
    v[:, :, :14] = TB._star((2, 3, 4))
    v[:, :, 16:] = TB._star((3, 3, 5))
    return v


def _dist_for(shape, seed=7):
    """A radius volume that differs from voxel to voxel: 0.5 .. 3.5."""
    return 0.5 + 3.0 * np.random.default_rng(seed).random(shape)


def _model(t, dist, spacing=(1.0, 1.0, 1.0), roots=(), local_steps=5):
    return MM.morphometry(t.shape, dist, t.offsets, t.voxels, t.ends, t.node_voxel, spacing, roots, local_steps)


def _derive(t, raw, spacing=(1.0, 1.0, 1.0)):
    return deriveMorphometry(raw, t.offsets, t.ends, t.kind, spacing)


# ------------------------------------------------------------------ CPU: the model against independent answers
def test_ordered_sum_is_the_stated_order():
    xs = [float(x) for x in np.random.default_rng(1).random(200)]
    lanes = [((xs[j] + xs[j + 64]) + xs[j + 128]) + xs[j + 192] if j < 8 else (xs[j] + xs[j + 64]) + xs[j + 128] for j in range(64)]
    for s in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[j] + lanes[j ^ s] for j in range(64)]
    assert MM.ordered_sum(xs) == lanes[0] and MM.ordered_sum([]) == 0.0 and MM.ordered_sum([1.5]) == 1.5
    # a narrower group gives the same bits: 16 lanes and the steps 8 .. 1 for at most 16 values
    few = xs[:13] + [0.0] * 3
    for s in (8, 4, 2, 1):
        few = [few[j] + few[j ^ s] for j in range(16)]
    assert MM.ordered_sum(xs[:13]) == few[0]


@pytest.mark.parametrize('step', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)])
def test_straight_lines_by_hand(step):
    h = (0.5, 1.0, 2.0)
    t = _path((9, 9, 9), _walk((4 - 2 * step[0], 4 - 2 * step[1], 4 - 2 * step[2]), [step] * 4))
    dist = np.full(t.shape, 1.5)
    raw = _model(t, dist, h)
    c = 4 * abs(step[0]) + 2 * abs(step[1]) + abs(step[2]) - 1
    want = np.zeros(7, np.int64); want[c] = 4
    w = math.sqrt(sum((s * x) ** 2 for s, x in zip(step, h)))            # by hand: 0.5, 1, 2 along the axes, sqrt(5.25) along a space diagonal
    assert w == {0: 2.0, 1: 1.0, 3: 0.5, 6: math.sqrt(5.25)}[c]
    assert raw['stepCounts'].tolist() == [want.tolist()] and raw['jumps'].tolist() == [0] and not raw['jumpOffset'].any()
    assert raw['pathLength'].tolist() == [4 * w] and raw['radiusCount'].tolist() == [3] and raw['radiusSum'].tolist() == [4.5]
    assert raw['radiusDevSq'].tolist() == [0.0] and raw['radiusMin'].tolist() == [1.5] and raw['radiusMax'].tolist() == [1.5]
    assert raw['chord'][0].tolist() == [4 * s for s in step] and raw['endDir'][0, 0].tolist() == [4 * s for s in step]
    assert (raw['endDir'][0, 1] == -raw['endDir'][0, 0]).all()
    assert _model(t, dist, h, local_steps=1)['endDir'][0].tolist() == [list(step), [-s for s in step]]
    d = _derive(t, raw, h)
    assert d['eculideanLength'].tolist() == [4 * w] and d['tortuosity'].tolist() == [1.0] and d['voxelLength'].tolist() == [5]
    assert d['meanRadius'].tolist() == [1.5] and d['sigma'].tolist() == [0.0] and d['aspectRatio'].tolist() == [4 * w / 1.5] and d['type'].tolist() == [0]
    assert np.array_equal(pathLengths(raw['stepCounts'], raw['jumpOffset'], h), raw['pathLength'])


def test_zigzag_uses_every_class():
    h = (0.5, 1.0, 2.0)
    t = _path((6, 6, 6), _walk((0, 0, 0), ALL_CLASSES))
    dist = np.arange(216, dtype=np.float64).reshape(6, 6, 6)
    raw = _model(t, dist, h)
    assert raw['stepCounts'].tolist() == [[1] * 7] and raw['jumps'].tolist() == [0] and raw['chord'].tolist() == [[4, 4, 4]]
    w = [2.0, 1.0, math.sqrt(5.0), 0.5, math.sqrt(4.25), math.sqrt(1.25), math.sqrt(5.25)]
    total = 0.0
    for x in w:
        total = total + x
    assert raw['pathLength'].tolist() == [total]
    inner = [float(dist[p]) for p in _walk((0, 0, 0), ALL_CLASSES)[1:-1]]
    assert raw['radiusCount'].tolist() == [6] and raw['radiusSum'].tolist() == [sum(inner)] and raw['radiusMin'].tolist() == [min(inner)]   # (integers: any order)
    assert raw['endDir'][0].tolist() == [[2, 2, 3], [-4, -3, -3]]         # five steps inwards from either end
    d = _derive(t, raw, h)
    assert d['eculideanLength'].tolist() == [math.sqrt((4.0 + 16.0) + 64.0)] and d['tortuosity'][0] == total / math.sqrt(84.0)
    assert np.array_equal(pathLengths(raw['stepCounts'], raw['jumpOffset'], h), raw['pathLength'])
    two = _path((1, 1, 2), [(0, 0, 0), (0, 0, 1)])                        # n == 2: both entries are the sample
    r2 = _model(two, np.array([[[1.0, 3.0]]]))
    assert r2['radiusCount'].tolist() == [2] and r2['radiusSum'].tolist() == [4.0] and r2['radiusDevSq'].tolist() == [2.0] and r2['endDir'][0].tolist() == [[0, 0, 1], [0, 0, -1]]


def test_tee_and_jumps():
    # the tee of test_branches: its cluster of four voxels is no clique, but the representative (the arm's foot) touches the
    # three others, so the two halves of the line get it attached by a diagonal step - no jump
    t = _of_volume(TB._tee())
    raw = _model(t, np.ones(t.shape))
    assert sorted(np.diff(t.offsets).tolist()) == [5, 6, 6] and raw['jumps'].tolist() == [0, 0, 0]
    assert sorted(raw['pathLength'].tolist()) == [4.0, 4.0 + math.sqrt(2.0), 4.0 + math.sqrt(2.0)]
    v = t.node_at((5, 6, 1))
    assert raw['incidentBranch'][v].tolist() == [0, 1, 2] and sorted(raw['incidentEnd'][v].tolist()) == [0, 0, 1]
    assert (raw['incidentBranch'][[k for k in range(4) if k != v]] == -1).all()
    # two arms two voxels apart: the representative (5, 6, 1) is no neighbour of (7, 4, 1) and (8, 5, 1)
    t = _of_volume(_double_tee())
    h = (0.5, 1.0, 2.0)
    raw = _model(t, np.ones(t.shape), h)
    lin = lambda p: int(np.ravel_multi_index(p, t.shape))
    b_arm = [k for k in range(4) if lin((7, 0, 1)) in t.voxels[t.offsets[k]:t.offsets[k + 1]]][0]
    b_far = [k for k in range(4) if lin((11, 5, 1)) in t.voxels[t.offsets[k]:t.offsets[k + 1]]][0]
    assert raw['jumps'].sum() == 2 and raw['jumps'][b_arm] == 1 and raw['jumps'][b_far] == 1
    assert raw['jumpOffset'][b_arm].tolist() == [[0, 0, 0], [-2, 2, 0]] and raw['jumpOffset'][b_far].tolist() == [[3, -1, 0], [0, 0, 0]]
    assert raw['stepCounts'][b_arm].tolist() == [0, 4, 0, 0, 0, 0, 0] and raw['stepCounts'][b_far].tolist() == [0, 0, 0, 3, 0, 0, 0]
    assert raw['pathLength'][b_arm] == 4.0 + math.sqrt(1.0 + 4.0) and raw['pathLength'][b_far] == 1.5 + math.sqrt(2.25 + 1.0)
    assert raw['radiusCount'][b_arm] == 4 and (raw['incidentBranch'] == -1).all()      # four ends at the one cluster
    assert np.array_equal(pathLengths(raw['stepCounts'], raw['jumpOffset'], h), raw['pathLength'])


def test_model_sums_against_numpy():
    """The model's order against numpy's (pairwise) one.  Any order of adding m non-negative doubles errs by at most
    g(m) S with g(m) = (m - 1) U / (1 - (m - 1) U) and S the exact sum (Higham, Accuracy and Stability, 4.2), so two orders differ
    by at most 2 g S.  Either mean adds one division (relative U): the means differ by at most (2 g + 2 U) (1 + U) S / m <=
    (2 g + 3 U) S / m.  sigma = |x - mean| / sqrt(m) is a 2-norm, so a mean that is off by e moves it by at most e (triangle
    inequality); each term carries the relative errors of the subtraction (U) and, under the root, half those of the square (U / 2),
    of the sum (g / 2), of the division (U / 2), then the root's own U: less than (g / 2 + 4 U) sigma per side.  Both sides:
    2 (e + (g / 2 + 4 U) sigma), e the bound on one mean's own error (g + 2 U) S / m.  The factor 1.01 covers the products of these
    terms."""
    for n in (3, 4, 17, 18, 66, 67, 130, 1000):
        t = _helix(n)
        dist = _dist_for(t.shape, n)
        raw = _model(t, dist)
        d = _derive(t, raw)
        xs = dist.ravel()[t.voxels[1:-1]]
        m = len(xs)
        S_, g = float(xs.sum()), (m - 1) * U / (1 - (m - 1) * U)
        assert raw['radiusCount'][0] == m == n - 2 and raw['radiusMin'][0] == xs.min() and raw['radiusMax'][0] == xs.max()
        assert abs(raw['radiusSum'][0] - S_) <= 1.01 * 2 * g * S_
        assert abs(d['meanRadius'][0] - np.mean(xs)) <= 1.01 * (2 * g + 3 * U) * S_ / m
        sigma = float(np.std(xs))
        assert abs(d['sigma'][0] - sigma) <= 1.01 * 2 * ((g + 2 * U) * S_ / m + (g / 2 + 4 * U) * sigma)
        assert sigma > 0.1 or m < 3


def _angles_by_hand(a, b):
    return math.degrees(math.acos(max(-1.0, min(1.0, float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))))))


def test_bifurcation_of_a_star():
    t = _of_volume(TB._star((6, 5, 7)))
    dist = _dist_for(t.shape)
    raw = _model(t, dist)
    d = _derive(t, raw)
    v = t.node_at((6, 6, 6))
    assert d['bifurcationNode'].tolist() == [v] and raw['incidentBranch'][v].tolist() == [0, 1, 2]
    arm = {}                                                              # branch -> its direction away from the centre
    for b in range(3):
        far = t.voxels[t.offsets[b]] if t.ends[b, 1] == v else t.voxels[t.offsets[b + 1] - 1]
        arm[b] = np.sign(np.array(np.unravel_index(far, t.shape)) - 6).astype(float)
    by_dir = {tuple(x.tolist()): b for b, x in arm.items()}
    pa, c1, c2 = by_dir[(-1, -1, -1)], by_dir[(-1, 1, 1)], by_dir[(1, 1, 1)]          # cosines -1/3, 1/3, -1: the pair of 1/3 are the children
    assert d['bifurcationBranches'][0, 2] == pa and sorted(d['bifurcationBranches'][0, :2].tolist()) == sorted([c1, c2])
    k1, k2 = d['bifurcationBranches'][0, :2]
    assert d['localBifurcationAmplitude'][0] == pytest.approx(math.degrees(math.acos(1 / 3)), rel=1e-12)
    assert d['remoteBifurcationAmplitude'][0] == pytest.approx(math.degrees(math.acos(1 / 3)), rel=1e-12)
    assert d['localBifurcationTilt'][0] == pytest.approx(math.degrees(math.acos(2 / math.sqrt(6))), rel=1e-12)
    assert d['remoteBifurcationTilt'][0] == pytest.approx(_angles_by_hand(arm[k1] / math.sqrt(3) + arm[k2] / math.sqrt(3), -arm[pa]), rel=1e-12)
    n = np.cross(arm[k1], arm[k2])
    assert d['normalVector'][0] == pytest.approx(n / np.linalg.norm(n), rel=1e-12, abs=1e-15)
    r = {b: np.mean(dist.ravel()[t.voxels[t.offsets[b] + 1:t.offsets[b + 1] - 1]]) for b in range(3)}
    assert d['cubicLawResult'][0] == pytest.approx((r[k1] ** 3 + r[k2] ** 3) / r[pa] ** 3, rel=1e-12)
    assert d['squareLawResult'][0] == pytest.approx((r[k1] ** 2 + r[k2] ** 2) / r[pa] ** 2, rel=1e-12)
    assert d['minRadiusRatio'][0] == pytest.approx(min(r[k1], r[k2]) / r[pa], rel=1e-12) and d['maxRadiusRatio'][0] == pytest.approx(max(r[k1], r[k2]) / r[pa], rel=1e-12)
    lengths = {5: 5 * math.sqrt(3), 6: 6 * math.sqrt(3), 7: 7 * math.sqrt(3)}
    n_of = lambda b: int(t.offsets[b + 1] - t.offsets[b]) - 1
    assert d['lengthRatio'][0] == pytest.approx(min(lengths[n_of(k1)], lengths[n_of(k2)]) / lengths[n_of(pa)], rel=1e-12)
    assert d['type'].tolist() == [0, 0, 0] and np.isnan(d['localBifurcationTorque']).all()
    # a root at a child's tip: that child's branch becomes the parent, the two others ascend
    tip = [int(t.ends[k1, e]) for e in (0, 1) if t.ends[k1, e] != v][0]
    d2 = _derive(t, _model(t, dist, roots=[tip]))
    assert d2['bifurcationBranches'][0].tolist() == sorted(b for b in range(3) if b != k1) + [k1]
    # an arm of two entries leaves the table empty
    short = _of_volume(TB._star((1, 5, 7)))
    assert len(_derive(short, _model(short, np.ones(short.shape)))['bifurcationNode']) == 0


@pytest.mark.parametrize('rooted', [False, True])
def test_bifurcation_of_a_planar_y(rooted):
    t = _of_volume(_planar_y())
    assert len(t.offsets) == 4 and len(t.node_voxel) == 4
    roots = [t.node_at((0, 8, 1))] if rooted else []
    d = _derive(t, _model(t, np.ones(t.shape), roots=roots))
    parent = [b for b in range(3) if np.ravel_multi_index((0, 8, 1), t.shape) in t.voxels[t.offsets[b]:t.offsets[b + 1]]][0]
    assert d['bifurcationNode'].tolist() == [t.node_at((7, 8, 1))] and d['bifurcationBranches'][0, 2] == parent
    assert d['localBifurcationAmplitude'][0] == pytest.approx(90.0, rel=1e-12) and d['remoteBifurcationAmplitude'][0] == pytest.approx(90.0, rel=1e-12)
    assert d['localBifurcationTilt'][0] == 0.0 and d['remoteBifurcationTilt'][0] == 0.0
    assert np.abs(d['normalVector'][0]) == pytest.approx([0.0, 0.0, 1.0], rel=1e-12, abs=0.0)
    assert d['cubicLawResult'][0] == 2.0 and d['squareLawResult'][0] == 2.0 and d['minRadiusRatio'][0] == 1.0 and d['lengthRatio'][0] == pytest.approx(math.sqrt(2.0), rel=1e-12)


def test_depth_on_a_comb():
    """The comb of test_branches, rooted at the backbone's first voxel.  Its first junction is represented by the tooth's foot
    (8, 5, 5) (four neighbours), the later ones by the backbone voxel in front of the teeth (17, 4, 4), (27, 4, 4), (37, 4, 4)."""
    t = _of_volume(TB._comb())
    root, far = t.node_at((0, 4, 4)), t.node_at((44, 4, 4))
    raw = _model(t, np.ones(t.shape), roots=[root])
    r3, r2 = math.sqrt(3.0), math.sqrt(2.0)
    assert raw['pathDistance'][root] == 0.0 and raw['parentBranch'][root] == -1 and raw['depthLevel'][root] == 0 and raw['depthVoxel'][root] == 0
    j1, tip1, j2 = t.node_at((8, 5, 5)), t.node_at((8, 6, 6)), t.node_at((17, 4, 4))
    d1 = 7.0 + r3                                                         # seven steps along the backbone, one diagonal step onto the foot
    assert raw['pathDistance'][j1] == d1 and raw['depthLevel'][j1] == 1 and raw['depthVoxel'][j1] == 8
    assert raw['pathDistance'][tip1] == d1 + r2 and raw['depthLevel'][tip1] == 2 and raw['depthVoxel'][tip1] == 9
    assert raw['pathDistance'][j2] == d1 + (8.0 + r3) and raw['depthLevel'][j2] == 2 and raw['depthVoxel'][j2] == 17      # back onto the backbone, eight steps
    for k, x in enumerate((17, 27, 37)):
        assert raw['depthLevel'][t.node_at((x, 4, 4))] == k + 2
    assert raw['pathDistance'][far] == pytest.approx(42.0 + 2 * r3, rel=1e-12) and raw['depthLevel'][far] == 5 and raw['depthVoxel'][far] == 41
    b = int(raw['parentBranch'][tip1])
    assert sorted(t.ends[b].tolist()) == sorted([j1, tip1]) and raw['branchLevel'][b] == 2
    assert (raw['depthLevel'] >= 0).all() and np.isfinite(raw['pathDistance']).all() and raw['branchLevel'].max() == 5


def test_depth_ties_unreached_and_roots():
    t = _of_volume(_tie_ring())
    top, bottom = t.node_at((0, 4, 1)), t.node_at((8, 4, 1))
    raw = _model(t, np.ones(t.shape), roots=[top])
    junctions = [v for v in range(len(t.node_voxel)) if t.kind[v] == 1]
    assert len(junctions) == 2 and len(t.offsets) - 1 == 4
    near, far = sorted(junctions, key=lambda v: raw['pathDistance'][v])
    halves = [b for b in range(4) if sorted(t.ends[b].tolist()) == sorted([near, far])]
    assert len(halves) == 2 and raw['pathLength'][halves[0]] == raw['pathLength'][halves[1]]        # two paths of equal length arrive
    assert raw['parentBranch'][far] == min(halves) and raw['depthLevel'][far] == 2 and raw['depthLevel'][bottom] == 3
    assert raw['pathDistance'][far] == raw['pathDistance'][near] + raw['pathLength'][halves[0]]
    # two components, one root: the other component is all -1 / inf
    t = _of_volume(_two_components())
    root = t.node_at((6, 6, 6))
    raw = _model(t, np.ones(t.shape), roots=[root])
    here = np.array([np.unravel_index(v, t.shape)[2] < 14 for v in t.node_voxel])
    assert here.sum() == 4 and (~here).sum() == 4
    assert np.isfinite(raw['pathDistance'][here]).all() and np.isinf(raw['pathDistance'][~here]).all()
    for k in ('parentBranch', 'depthLevel', 'depthVoxel'):
        assert (raw[k][~here] == -1).all()
    assert (raw['depthLevel'][here] >= 0).all() and sorted(raw['branchLevel'].tolist()) == [-1, -1, -1, 1, 1, 1]
    # a root given as a coordinate must be a representative
    g = t.graph()
    assert S._root_indices([(6, 6, 6), root], g.nodeCoords).tolist() == [root, root]
    with pytest.raises(ValueError):
        branchMorphometry(g, dist=np.ones(t.shape), roots=[(5, 5, 5)])    # a voxel of an arm, no representative
    with pytest.raises(ValueError):
        branchMorphometry(g, dist=np.ones(t.shape), roots=[len(t.node_voxel)])


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_morphometry_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vmor_device.hip' in build.SOURCES
    out = tmp_path / 'vmor_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vmor_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
        recs[m.group(1)] = (f('private_segment_fixed_size'), f('vgpr_count'))
    for frag in ('k_mor_check', 'k_mor_branch', 'k_mor_gather', 'k_mor_incident', 'k_mor_node', 'k_mor_roots', 'k_mor_fill', 'k_mor_relax', 'k_mor_parent',
                 'k_mor_level', 'k_mor_finish'):
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, (scratch, vgpr) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        assert vgpr <= 128, '%s uses %d VGPRs' % (name, vgpr)              # (four waves per SIMD)


# ------------------------------------------------------------------ GPU: exactly the model
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_equal_to_model(got, raw, t, spacing=(1.0, 1.0, 1.0)):
    names = list(S.MORPHOMETRY_RAW) + [k for k in S.MORPHOMETRY_DEPTH if k in raw]
    for k in names:
        a, b = np.asarray(getattr(got, k)), raw[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k
    if 'pathDistance' not in raw:
        assert all(getattr(got, k) is None for k in S.MORPHOMETRY_DEPTH)
    want = _derive(t, raw, spacing)
    for k in S.MORPHOMETRY_BRANCH + S.MORPHOMETRY_BIFURCATION:
        a, b = np.asarray(getattr(got, k)), want[k]
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype == np.float64), k


def _check(t, dist, spacing=(1.0, 1.0, 1.0), roots=(), local_steps=5):
    got = branchMorphometry(t.graph(), dist=dist, spacing=spacing, roots=list(roots) if len(roots) else None, localSteps=local_steps)
    raw = _model(t, dist, spacing, roots, local_steps)
    _assert_equal_to_model(got, raw, t, spacing)
    return got, raw


@pytest.mark.gpu
@pytest.mark.parametrize('n', [2, 3, 4, 17, 18, 19, 63, 64, 65, 66, 128, 129, 1000])
def test_single_branches(n):
    """The lengths around the lane stride (64 sample values are 66 entries), the quarter-wave bound (17 entries), the
    empty-interior rule (2, 3) and a branch of many trips; a straight line in a 1 x 1 x n volume and a helix, dist varying."""
    line = _of_volume(np.ones((1, 1, n), np.uint8))
    assert np.diff(line.offsets).tolist() == [n]
    _check(line, _dist_for(line.shape, n), spacing=(0.1, 0.3, 0.7))
    if n >= 3:
        h = _helix(n)
        got, raw = _check(h, _dist_for(h.shape, n + 1), spacing=(0.1, 0.3, 0.7))
        assert raw['stepCounts'].sum() == n - 1 and raw['radiusDevSq'][0] > 0 or n == 3


@pytest.mark.gpu
@pytest.mark.parametrize('density,seed', [(0.1, 41), (0.3, 42), (0.6, 43)])
def test_many_branches(density, seed):
    """Unthinned random volumes: many branches of 2 to 10 entries share waves; closed curves, loops on a cluster, isolated voxels."""
    v = TB._random((24, 24, 24), density, seed)
    t = _of_volume(v)
    n = np.diff(t.offsets)
    print(density, 'branches', len(n), 'nodes', len(t.node_voxel), 'lengths', int(n.min()), int(n.max()))
    assert len(n) > 0
    roots = [0, len(t.node_voxel) // 2]
    got, raw = _check(t, _dist_for(t.shape, seed), spacing=(0.1, 0.3, 0.7), roots=roots)
    assert got.depthRounds <= max(len(t.node_voxel), 1)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['tee', 'double-tee', 'faces', 'free-ring', 'loop-on-cluster', 'star', 'planar-y'])
def test_shapes(case):
    v = {'tee': TB._tee, 'double-tee': _double_tee, 'faces': TB._faces, 'free-ring': TB._free_ring, 'loop-on-cluster': TB._loop_on_cluster,
         'star': functools.partial(TB._star, (6, 5, 7)), 'planar-y': _planar_y}[case]()
    t = _of_volume(v)
    roots = [0] if len(t.node_voxel) else []
    got, raw = _check(t, _dist_for(t.shape), spacing=(0.5, 1.0, 2.0), roots=roots)
    if case == 'double-tee':
        assert raw['jumps'].sum() == 2
    if case == 'free-ring':
        assert t.ends.tolist() == [[-1, -1]] and np.isinf(got.tortuosity).all() and got.type.tolist() == [-1]
    if case in ('star', 'planar-y'):
        assert len(got.bifurcationNode) == 1


@pytest.mark.gpu
@pytest.mark.parametrize('steps', [1, 5, 1000])
def test_local_steps(steps):
    t = _of_volume(_planar_y())
    got, raw = _check(t, _dist_for(t.shape), local_steps=steps)
    assert np.abs(raw['endDir']).max() == min(steps, 7)
    t = _of_volume(TB._random((24, 24, 24), 0.1, 41))
    _check(t, _dist_for(t.shape), local_steps=steps)


@pytest.mark.gpu
def test_spacing_bounds():
    t = _of_volume(TB._star((6, 5, 7)))
    dist = _dist_for(t.shape)
    _check(t, dist, spacing=(0.001, 1.0, 0.5), roots=[0])                 # a ratio of exactly 1000 is accepted
    above = float(np.nextafter(1.0, 2.0))
    g = t.graph()
    dll = S._skeleton_lib()
    B, N = len(t.offsets) - 1, len(t.node_voxel)
    CANARY = -77
    for h in ((0.001, above, 0.5), (0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, float('inf'), 1.0), (1.0, 1.0, float('nan'))):
        with pytest.raises(Exception):
            branchMorphometry(g, dist=dist, spacing=h)
        h = np.array(h, np.float64)
        bi, bf, rad, inc, ent = (np.full(k, CANARY, dt) for k, dt in ((24 * B, np.int64), (5 * B, np.float64), (N, np.float64), (3 * N, np.int64), (len(t.voxels), np.float64)))
        pd, nd, bl, cnt = np.full(N, CANARY, np.float64), np.full(3 * N, CANARY, np.int64), np.full(B, CANARY, np.int64), np.full(2, CANARY, np.int64)
        roots = np.zeros(1, np.int64)
        rc = dll.vmask_morphometry(0, *t.shape, dist.ctypes.data, t.offsets.ctypes.data, B, t.voxels.ctypes.data, np.ascontiguousarray(t.ends).ctypes.data,
                                   t.node_voxel.ctypes.data, N, h.ctypes.data, roots.ctypes.data, 1, 5, bi.ctypes.data, bf.ctypes.data, rad.ctypes.data,
                                   inc.ctypes.data, ent.ctypes.data, pd.ctypes.data, nd.ctypes.data, bl.ctypes.data, cnt.ctypes.data)
        assert rc == -1 and b'spacing' in dll.vmask_last_error()
        assert all((a == CANARY).all() for a in (bi, bf, rad, inc, ent, pd, nd, bl, cnt))           # the outputs untouched


@pytest.mark.gpu
def test_depth_on_the_gpu():
    t = _of_volume(_long_comb(40))
    N = len(t.node_voxel)
    assert N == 82
    got, raw = _check(t, np.ones(t.shape), roots=[t.node_at((0, 4, 4))])
    print('comb of 40 teeth: depthRounds', got.depthRounds)
    assert 1 <= got.depthRounds <= N and raw['depthLevel'].max() == 41
    got, raw = _check(t, _dist_for(t.shape), spacing=(0.1, 0.3, 0.7), roots=[t.node_at((0, 4, 4)), t.node_at((164, 4, 4))])      # two roots
    assert raw['depthLevel'].max() <= 21 and got.depthRounds <= N
    t = _of_volume(_tie_ring())
    got, raw = _check(t, np.ones(t.shape), roots=[t.node_at((0, 4, 1))])                    # on an end point; the tie
    junctions = sorted((v for v in range(len(t.node_voxel)) if t.kind[v] == 1), key=lambda v: raw['pathDistance'][v])
    halves = [b for b in range(4) if sorted(t.ends[b].tolist()) == sorted(junctions)]
    assert got.parentBranch[junctions[1]] == min(halves) and raw['pathLength'][halves[0]] == raw['pathLength'][halves[1]]
    _check(t, _dist_for(t.shape), roots=[junctions[0]])                                      # on a cluster
    t = _of_volume(_two_components())
    got, raw = _check(t, _dist_for(t.shape), roots=[t.node_at((6, 6, 6))])
    assert np.isinf(got.pathDistance).sum() == 4 and (got.branchLevel == -1).sum() == 3
    # nroots == 0 leaves the depth outputs alone
    got = branchMorphometry(t.graph(), dist=np.ones(t.shape))
    assert got.pathDistance is None and got.depthLevel is None and got.branchLevel is None and got.depthRounds == 0


@pytest.mark.gpu
def test_inputs_infinite_zero_and_empty():
    t = _helix(130)
    dist = _dist_for(t.shape)
    dist.ravel()[t.voxels[5]] = np.inf
    dist.ravel()[t.voxels[6]] = 0.0
    got, raw = _check(t, dist)
    assert np.isinf(got.radiusSum[0]) and np.isnan(got.radiusDevSq[0]) and got.radiusMin[0] == 0.0 and np.isinf(got.radiusMax[0])
    short = _helix(9)                                                     # the same through the quarter-wave path
    dist = _dist_for(short.shape)
    dist.ravel()[short.voxels[3]] = np.inf
    dist.ravel()[short.voxels[4]] = 0.0
    got, raw = _check(short, dist)
    assert np.isnan(got.radiusDevSq[0])
    zero = _helix(40)
    _check(zero, np.zeros(zero.shape))
    empty = Tables((4, 5, 6), [0], [], np.zeros((0, 2), np.int64), [])
    got, raw = _check(empty, np.ones(empty.shape))
    assert got.pathLength.shape == (0,) and got.nodeRadius.shape == (0,) and got.bifurcationNode.shape == (0,) and got.stepCounts.shape == (0, 7)
    # a table that does not fit the volume is refused before anything is written
    bad = _helix(20)
    bad.voxels = bad.voxels.copy(); bad.voxels[7] = int(np.prod(bad.shape))
    dll = S._skeleton_lib()
    B, N = 1, 2
    outs = [np.full(k, -77, dt) for k, dt in ((24, np.int64), (5, np.float64), (2, np.float64), (6, np.int64))]
    rc = dll.vmask_morphometry(0, *bad.shape, np.ones(bad.shape).ctypes.data, bad.offsets.ctypes.data, B, bad.voxels.ctypes.data, np.ascontiguousarray(bad.ends).ctypes.data,
                               bad.node_voxel.ctypes.data, N, None, None, 0, 5, *(a.ctypes.data for a in outs), None, None, None, None, None)
    assert rc == -1 and b'out of range' in dll.vmask_last_error() and all((a == -77).all() for a in outs)


@pytest.mark.gpu
def test_repeats_are_bit_identical():
    t = _of_volume(TB._random((24, 24, 24), 0.3, 42))
    dist = _dist_for(t.shape)
    a = branchMorphometry(t.graph(), dist=dist, spacing=(0.1, 0.3, 0.7), roots=[0, 3])
    b = branchMorphometry(t.graph(), dist=dist, spacing=(0.1, 0.3, 0.7), roots=[0, 3])
    assert a.names() == b.names() and len(a.names()) == len(S.MORPHOMETRY_RAW + S.MORPHOMETRY_DEPTH + S.MORPHOMETRY_BRANCH + S.MORPHOMETRY_BIFURCATION)
    for k in a.names():
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import skeletonization as S
import test_morphometry as T
v = T.TB._random((24, 24, 24), 0.3, 42)
dist = T._dist_for(v.shape)
dev = torch.device('cuda', 0)
gh = S.branchGraph(v)
gd = S.branchGraph(torch.as_tensor(v, device=dev))
h = S.branchMorphometry(gh, dist=dist, spacing=(0.1, 0.3, 0.7), roots=[0, tuple(gh.nodeCoords[3].tolist())])
d = S.branchMorphometry(gd, dist=torch.as_tensor(dist, device=dev), spacing=(0.1, 0.3, 0.7), roots=[0, 3])
m = S.branchMorphometry(gd, dist=dist, spacing=(0.1, 0.3, 0.7), roots=[0, 3])           # (a host dist beside a device graph)
t = T._of_volume(v)
T._assert_equal_to_model(h, T._model(t, dist, (0.1, 0.3, 0.7), [0, 3]), t, (0.1, 0.3, 0.7))
for g in (d, m):
    assert g.names() == h.names()
    for name in h.names():
        a, b = getattr(g, name), getattr(h, name)
        assert a.is_cuda and a.device == dev and tuple(a.shape) == b.shape, name
        assert a.cpu().numpy().tobytes() == b.tobytes(), name
assert d.pathLength.dtype == torch.float64 and d.stepCounts.dtype == torch.int64
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_morphometry_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, equal to the host call.
    Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_main_writes_the_files(tmp_path, capsys):
    from arterynetwork_amd import nifti
    m = M.crossing_phantom((48, 48, 32))
    m[10, 33:45, 15:17] = 1                                               # a flat rod out of the tube: a bifurcation of three branches of three and more entries
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    plain, measured = tmp_path / 'plain', tmp_path / 'measured'
    for d in (plain, measured):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    with pytest.raises(ValueError):
        S.main(str(measured), segments=True, morphometry=True)
    before = S.main(str(plain), segments=True, territories=True, prune=(0, 0.0))
    capsys.readouterr()
    after = S.main(str(measured), segments=True, territories=True, prune=(0, 0.0), morphometry=True, roots=[0])
    said = capsys.readouterr().out
    new = ['branchMorphometry.npz', 'graphRepresentationWithEdgeInfo.graphml', 'nodeInfoDict.pkl', 'segmentInfoDict.pkl']
    assert sorted(os.listdir(str(measured))) == sorted(os.listdir(str(plain)) + new)
    for name in os.listdir(str(plain)):                                   # every other file byte for byte
        if name == S.BRANCH_FILE:                                         # (but for labelRounds, which describes the run and differs between two)
            with np.load(str(plain / name)) as x, np.load(str(measured / name)) as y:
                assert x.files == y.files
                for k in x.files:
                    keep = x['countNames'] != 'labelRounds' if k == 'counts' else slice(None)
                    assert x[k].dtype == y[k].dtype and np.array_equal(x[k][keep], y[k][keep]), (name, k)
            continue
        assert (plain / name).read_bytes() == (measured / name).read_bytes(), name
    for name in new:
        assert '{} saved to {}.'.format(name, os.path.join(str(measured), name)) in said
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after))
    graph = S.branchGraph(S.skeletonize(m))
    _, stored = nifti.loadVolume(str(measured), 'vesselVolumeMask.nii.gz')
    spacing = np.sqrt((np.asarray(stored, np.float64)[:3, :3] ** 2).sum(axis=0))      # (the file keeps the affine in float32)
    assert spacing == pytest.approx([0.4, 0.4, 0.6], rel=1e-6)
    want = branchMorphometry(graph, vesselVolumeMask=m, spacing=spacing, roots=[0])
    z = np.load(str(measured / 'branchMorphometry.npz'))
    assert z['names'].tolist() == want.names() and np.array_equal(z['spacing'], spacing) and z['roots'].tolist() == [0] and int(z['localSteps']) == 5
    for k in want.names():
        assert z[k].dtype == getattr(want, k).dtype and z[k].tobytes() == getattr(want, k).tobytes(), k
    B = len(graph.offsets) - 1
    with open(str(measured / 'segmentInfoDict.pkl'), 'rb') as f:
        seg = pickle.load(f)
    with open(str(measured / 'nodeInfoDict.pkl'), 'rb') as f:
        node = pickle.load(f)
    keep = [k for k in range(B) if graph.branchEnds[k, 0] >= 0 and graph.branchEnds[k, 0] != graph.branchEnds[k, 1]]
    assert sorted(seg) == keep and len(keep) > 0
    for k, d in seg.items():
        assert {'pathLength', 'eculideanLength', 'tortuosity', 'voxelLength', 'meanRadius', 'type', 'aspectRatio'} <= set(d)
        assert ('sigma' in d) == (d['voxelLength'] != 2) and 'segmentLevel' not in d      # (two entries: the reference's rule, no sigma; a level comes from a partition)
        assert all(type(x) in (float, int, str) for x in d.values()) and d['type'] in ('terminating', 'bifurcating')
        assert d['pathLength'] == want.pathLength[k] and d['voxelLength'] == want.voxelLength[k] and d['meanRadius'] == want.meanRadius[k]
    assert sorted(node) == sorted(tuple(c) for c in graph.nodeCoords.tolist())
    for v, c in enumerate(graph.nodeCoords.tolist()):
        d = node[tuple(c)]
        assert type(d['radius']) is float and d['radius'] == want.nodeRadius[v]
        if want.depthLevel[v] >= 0:
            assert (d['depthVoxel'], d['depthLevel'], d['pathDistance']) == (want.depthVoxel[v], want.depthLevel[v], want.pathDistance[v])
    assert len(want.bifurcationNode) > 0
    for row, v in enumerate(want.bifurcationNode.tolist()):
        d = node[tuple(graph.nodeCoords[v].tolist())]
        assert {'localBifurcationAmplitude', 'remoteBifurcationAmplitude', 'cubicLawResult', 'squareLawResult', 'radiusList', 'minRadius', 'minRadiusRatio',
                'maxRadiusRatio', 'lengthRatio', 'normalVector'} <= set(d)
        assert type(d['normalVector']) is list and d['localBifurcationAmplitude'] == want.localBifurcationAmplitude[row]
    try:
        import networkx as nx
    except ImportError:                                                   # (the file must parse with networkx where networkx imports)
        import xml.etree.ElementTree as ET
        root = ET.parse(str(measured / 'graphRepresentationWithEdgeInfo.graphml')).getroot()
        assert len(root.findall('.//{http://graphml.graphdrawing.org/xmlns}node')) == len({tuple(p) for p in graph.coords.tolist()})
        return
    G = nx.read_graphml(str(measured / 'graphRepresentationWithEdgeInfo.graphml'))
    ids = [str(tuple(p)) for p in graph.coords.tolist()]
    assert set(G.nodes) == set(ids) and all(G.nodes[a]['radius'] == r for a, r in zip(ids, want.entryRadius.tolist()))
    for a, b, d in G.edges(data=True):
        k = d['segmentIndex']
        assert d['pathLength'] == want.pathLength[k] and d['voxelLength'] == want.voxelLength[k] and d['meanRadius'] == want.meanRadius[k]
        assert {'eculideanLength', 'tortuosity'} <= set(d) and ('sigma' in d) == (d['voxelLength'] != 2)
    for v in np.flatnonzero(want.depthLevel >= 0).tolist():
        a = str(tuple(graph.nodeCoords[v].tolist()))
        assert G.nodes[a]['depthLevel'] == want.depthLevel[v] and G.nodes[a]['depthVoxel'] == want.depthVoxel[v] and G.nodes[a]['pathDistance'] == want.pathDistance[v]
