"""The envelope pass of the exact distance transform (k_edt_envelope, csrc/vmask_device.hip), path by path: tests/edt_trace.py
restates one wave's bookkeeping and is checked here against a brute-force minimum; directed volumes are CERTIFIED on the CPU
(which counters of the trace each of them makes non-zero, per pass and per arithmetic width) and must then equal scipy's
transform bit for bit on the GPU; the last 32-bit and the first 64-bit extent on every axis with the divisions they hold;
and volumes whose true squared distances reach and pass 2^29, against the closed form."""
import functools
import os
import re

import numpy as np
import pytest

import edt_trace as T
from conftest import ROOT
from oracle import mask_oracle as MO


# ------------------------------------------------------------------ the model against brute force
def test_trace_equals_brute_force_on_random_waves():
    rng = np.random.default_rng(11)
    total = T.new_counts()
    for i in range(150):
        m, lanes = int(rng.integers(1, 120)), int(rng.integers(1, 65))
        inf = (T.INF32, T.INF64)[i % 2]
        G = rng.integers(0, (3, 60, 3000, 10 ** 6)[i % 4], (lanes, m))
        if i % 3 == 0:
            G[rng.random((lanes, m)) < (0.1, 0.6, 0.95)[i % 9 // 3]] = inf       # columns without a zero voxel
        if i % 5 == 0:
            G[:] = G[0]                                                          # a wave of equal lines
        if i % 7 == 0:
            G[:, :m // 2] = inf
        rows, cnt = T.trace_wave(G, inf)
        assert np.array_equal(rows, T.brute_rows(G, inf)), (i, G.tolist())
        T.add_counts(total, cnt)
    assert total['chunk_flush'] == 0 and total['spills'] > 0      # random values never keep a spilled chunk until it is final: hence
    for i in range(60):                                           # nearly constant lines (the distance to a far plane), a level per lane
        m, lanes = int(rng.integers(60, 200)), int(rng.integers(1, 65))
        inf = (T.INF32, T.INF64)[i % 2]
        level = rng.integers(20, 46, (lanes, 1)) if i % 3 else rng.integers(40, 42, (lanes, 1))
        G = level ** 2 + rng.integers(0, 3, (lanes, m))
        for c in rng.integers(0, m, int(rng.integers(0, 3))):
            G[:, c] = rng.integers(0, 2, lanes) * inf              # a cut in some lanes, a column without a zero in the others
        G[:, :int(rng.integers(0, 7))] = inf
        rows, cnt = T.trace_wave(G, inf)
        assert np.array_equal(rows, T.brute_rows(G, inf)), (i, G.tolist())
        T.add_counts(total, cnt)
    assert all(total[k] > 0 for k in T.COUNTERS), total           # every path at least once
    # a line of equal values: every site is pushed, entry i is final (start i, value G) sqrt(G) rows later
    rows, cnt = T.trace_wave(np.full((64, 72), 44 * 44), T.INF32)
    assert (rows == 44 * 44).all() and cnt['depth'] == 57 and cnt['spills'] and cnt['chunk_flush'] and cnt['read_reloads'] and not cnt['reset']
    rows, cnt = T.trace_wave([[7]], T.INF32)                      # a line of one voxel: no batch at all
    assert rows.tolist() == [[7]] and cnt['depth'] == 1


def test_pass_helpers_equal_brute_force():
    """axis0_squared and plane_squared (what pass 1 reads and must write, the latter from the oracle's 2-D transforms) against
    direct minima, with columns and whole planes that hold no zero voxel."""
    rng = np.random.default_rng(12)
    for shape in ((9, 14, 5), (1, 20, 3), (12, 1, 7), (6, 6, 1)):
        mask = (rng.random(shape) < 0.8).astype(np.uint8)
        mask[:, :, 0] = 1                                         # a plane without a zero
        mask[0, 0, shape[2] - 1] = 0
        z = np.argwhere(mask == 0)
        idx = np.indices(shape).reshape(3, -1).T
        for inf in (T.INF32, T.INF64):
            g0 = np.full(len(idx), inf, np.int64)
            pl = np.full(len(idx), inf, np.int64)
            for k, (a, b, c) in enumerate(idx):
                col = z[(z[:, 1] == b) & (z[:, 2] == c)]
                if len(col):
                    g0[k] = ((col[:, 0] - a) ** 2).min()
                pln = z[z[:, 2] == c]
                if len(pln):
                    pl[k] = ((pln[:, 0] - a) ** 2 + (pln[:, 1] - b) ** 2).min()
            assert np.array_equal(T.axis0_squared(mask, inf).ravel(), g0)
            assert np.array_equal(T.plane_squared(mask, inf).ravel(), pl)
        full = ((idx[:, None, :] - z[None, :, :]) ** 2).sum(axis=2).min(axis=1)
        assert np.array_equal(T.volume_squared(mask).ravel(), full)
        for which in (1, 2):
            assert T.trace_pass(mask, which)[1] == 0


# ------------------------------------------------------------------ directed volumes
def _slab(shape, cuts=(), stairs=False, lead=0, swap=False):
    """All ones under a zero plane i0 = 0: along every axis-1 line G = i0^2 is constant, entry i becomes final i0 rows behind the
    scan and the stack holds i0 + AHEAD-odd entries.  cuts: zero planes i1 = c (they pop what is above them: reloads while the
    stack is built, and sites behind them that never win: not pushed).  stairs: also zero where i0 <= i2 // 2, so the lanes of
    a wave differ and some are ready to write a chunk out while others are not.  lead: the first `lead` planes i1 all ones -
    columns without a zero voxel, popped together by the first real site (reset).  swap: axes 1 and 2 exchanged, which moves
    the deep lines into pass 2."""
    m = np.ones(shape, np.uint8)
    m[0] = 0
    if stairs:
        m[np.broadcast_to(np.arange(shape[0])[:, None, None] <= np.arange(shape[2])[None, None, :] // 2, shape)] = 0
    for c in cuts:
        m[:, c, :] = 0
    if lead:
        m[:, :lead, :] = 1
    return np.ascontiguousarray(m.transpose(0, 2, 1)) if swap else m


def _two_zeros(swap=False):
    """40^3 with zeros at (0,0,0) and (39,20,5) only: runs of columns without a zero, a reset and a reload per line"""
    m = np.ones((40, 40, 40), np.uint8)
    m[0, 0, 0] = m[39, 20, 5] = 0
    return np.ascontiguousarray(m.transpose(0, 2, 1)) if swap else m


ALL = frozenset(T.COUNTERS)
# name: (mask, the i0 planes to trace (None: all), {pass: the counters that must be non-zero there}); the totals are in DESIGN.md
CASES = {
    'slab-45x72x3': (functools.partial(_slab, (45, 72, 3)), None,
                     {1: ALL - {'build_reloads', 'flush_blocked', 'reset', 'spill_after_reload', 'not_pushed'}, 2: {'depth'}}),
    'slab-cut-45x130x2': (functools.partial(_slab, (45, 130, 2), (60,)), None, {1: ALL - {'flush_blocked', 'reset'}, 2: {'depth'}}),
    'stairs-45x72x40': (functools.partial(_slab, (45, 72, 40), (), True), None,
                        {1: ALL - {'build_reloads', 'reset', 'spill_after_reload', 'not_pushed'}, 2: {'depth', 'bottom_leaves', 'reset'}}),
    'stairs-cut-45x100x40': (functools.partial(_slab, (45, 100, 40), (60,), True, 5), None, {1: ALL, 2: ALL - {'not_pushed'}}),
    'stairs-cut-45x40x100': (functools.partial(_slab, (45, 100, 40), (60,), True, 5, True), None, {1: {'depth', 'spills', 'read_reloads', 'reset'}, 2: ALL}),
    'two-zeros-40': (_two_zeros, None, {1: {'depth', 'spills', 'build_reloads', 'read_reloads', 'reset', 'not_pushed'}, 2: {'bottom_leaves', 'reset', 'not_pushed'}}),
    'two-zeros-40-swapped': (functools.partial(_two_zeros, True), None, {1: {'depth', 'spills', 'read_reloads', 'reset', 'not_pushed'}, 2: {'bottom_leaves', 'reset', 'not_pushed'}}),
    # 64-bit arithmetic: the long extent on the line axis (the second cut, 40 rows before the end, leaves sites behind it that never win)
    'wide-45x23171x3': (functools.partial(_slab, (45, 23171, 3), (60, 23131), True, 5), (19, 44), {1: ALL}),
    'wide-45x3x23171': (functools.partial(_slab, (45, 23171, 3), (60, 23131), True, 5, True), (21, 44), {2: ALL}),
    'wide-slab-45x3x23171': (functools.partial(_slab, (45, 23171, 3), (), False, 0, True), (44,),
                             {2: ALL - {'build_reloads', 'flush_blocked', 'bottom_leaves', 'reset', 'spill_after_reload', 'not_pushed'}}),
}
NARROW = [n for n in CASES if not n.startswith('wide')]
WIDE = [n for n in CASES if n.startswith('wide')]


@functools.lru_cache(maxsize=None)
def _case_mask(name):
    mask = CASES[name][0]()
    mask.setflags(write=False)
    return mask


@functools.lru_cache(maxsize=None)
def _case_trace(name, which):
    return T.trace_pass(_case_mask(name), which, CASES[name][1])


@pytest.mark.parametrize('name', sorted(CASES))
def test_directed_cases_reach_their_paths(name):
    """Per case and pass: the model's rows are what the pass must write (brute force through the oracle), the counters named in
    CASES are non-zero, and the case is on the side of the arithmetic rule that its name says."""
    mask = _case_mask(name)
    assert T.is_32bit(mask.shape) == (name in NARROW)
    assert mask.size <= (200_000 if name in NARROW else 4_000_000) and not mask.all()
    for which, want in CASES[name][2].items():
        cnt, wrong = _case_trace(name, which)
        print(name, 'pass', which, cnt)
        assert wrong == 0
        assert all(cnt[k] > 0 for k in want), (which, [k for k in want if not cnt[k]])
    if name == 'slab-45x72x3':
        assert _case_trace(name, 1)[0]['depth'] == 57 and _case_trace(name, 2)[0]['depth'] <= 3
    if name == 'stairs-cut-45x100x40':
        assert _case_trace(name, 2)[0]['depth'] == 40


@pytest.mark.parametrize('names', [NARROW, WIDE], ids=['32-bit', '64-bit'])
def test_directed_cases_cover_every_path_in_both_passes(names):
    """Between them the cases of a width make every counter non-zero in pass 1 and again in pass 2."""
    for which in (1, 2):
        total = T.new_counts()
        for name in names:
            if which in CASES[name][2]:
                T.add_counts(total, _case_trace(name, which)[0])
        assert all(total[k] > 0 for k in T.COUNTERS), (which, total)
        assert total['depth'] > 2 * T.RING + T.CHUNK               # deeper than the ring and a whole spilled chunk below it


@pytest.mark.parametrize('mutation', T.MUTATIONS)
def test_mutations_of_the_bookkeeping_fail_the_certified_cases(mutation):
    """A pop that does not bring its chunk back, a chunk write-out that leaves dn_t / dn_v stale, a read-back that runs down to
    row 0 instead of ue: each gives wrong rows on the certified cases, in both passes and at both widths - the cases are
    sensitive to those paths."""
    for name, which in (('stairs-cut-45x100x40', 1), ('stairs-cut-45x40x100', 2), ('wide-45x23171x3', 1), ('wide-45x3x23171', 2)):
        planes = CASES[name][1] and CASES[name][1][:1]
        assert T.trace_pass(_case_mask(name), which, planes, mutation=mutation)[1] > 0, (name, which)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_edt_directed_cases(name):
    from arterynetwork_amd.generateVesselVolume import distance_transform_edt
    mask = _case_mask(name)
    assert np.array_equal(distance_transform_edt(mask), MO.distance_transform_edt(mask))


# ------------------------------------------------------------------ the limits of the two widths
def _kernel_is_32bit(shape):
    """edt_squared's own rule, read from its source: 32-bit arithmetic where n0^2 + n1^2 + n2^2 < EDT_INF"""
    src = open(os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vmask_device.hip')).read()
    inf = re.search(r'constexpr int32_t EDT_INF = 1 << (\d+);', src)
    rule = re.search(r'const bool small = \(int64_t\)d\.n0 \* d\.n0 \+ \(int64_t\)d\.n1 \* d\.n1 \+ \(int64_t\)d\.n2 \* d\.n2 < \(int64_t\)EDT_INF;', src)
    assert inf and rule, 'the rule that chooses the arithmetic has moved'
    assert '<<<egrid(d), EDT_TPB>>>' in src and src.count('if (small) k_edt_envelope<int32_t>') == 2 and src.count('else k_edt_envelope<long long>') == 2
    return sum(int(n) ** 2 for n in shape) < (1 << int(inf.group(1)))


LIMIT_SHAPES = [(23170, 2, 3), (2, 23170, 3), (2, 3, 23170), (23171, 2, 3), (2, 23171, 3), (2, 3, 23171)]


@functools.lru_cache(maxsize=None)
def _limit_mask(shape):
    """Zeros at the same places for 23170 and 23171: about 60 random ones near the two ends, and pairs of equal parity 1000 and 1002 apart on
    neighbouring lines (exact multiples, and remainders of 1 and b - 1 where the neighbour's zero is one voxel away)."""
    axis = int(np.argmax(shape))
    m = np.ones((23170, 2, 3) if shape[axis] == 23170 else (23171, 2, 3), np.uint8)
    rng = np.random.default_rng(77)
    far = rng.integers(0, 6600, 60)                               # (4800 .. 21300 is kept for the pairs)
    m[np.where(far < 4800, far, far + 16500), rng.integers(0, 2, 60), rng.integers(0, 3, 60)] = 0
    for a, b, c in ((5000, 0, 0), (6000, 0, 0), (7002, 1, 0), (12000, 1, 2), (13000, 0, 2), (14002, 0, 1), (23169, 1, 1),
                    (8000, 1, 1), (9000, 1, 1), (16000, 0, 1), (17000, 0, 1), (18000, 0, 0), (19000, 0, 0), (20000, 1, 2), (21000, 1, 2)):
        m[a, b, c] = 0
    m = np.ascontiguousarray(np.moveaxis(m, 0, axis)) if axis else m          # (long, 2, 3) -> (2, long, 3) / (2, 3, long)
    assert m.shape == tuple(shape)
    m.setflags(write=False)
    return m


def test_limit_shapes_select_the_width_they_are_for():
    for shape in LIMIT_SHAPES:
        assert _kernel_is_32bit(shape) == (max(shape) == 23170) == T.is_32bit(shape), shape
        assert T.edt_inf(shape) == (T.INF32 if max(shape) == 23170 else T.INF64)
    assert _kernel_is_32bit((23170, 1, 1)) and not _kernel_is_32bit((23171, 1, 1)) and _kernel_is_32bit((13377, 13377, 13377))
    assert not _kernel_is_32bit((13378, 13378, 13378))
    for name in CASES:
        assert _kernel_is_32bit(_case_mask(name).shape) == (name in NARROW)


def _classes(div):
    q = [(a // b, a % b, b) for a, b in div]
    return {'exact': sum(1000 <= f < 32768 and r == 0 and b > 1000 for f, r, b in q),
            'near': sum(1000 <= f < 32768 and r in (1, 2, b - 1, b - 2) and b > 1000 for f, r, b in q),
            'big': sum(f >= 32768 for f, r, b in q), 'max': max(f for f, r, b in q)}


def test_limit_cases_hold_the_quotients_they_are_for():
    """The divisions of the 32-bit shapes (23170 on each axis), as the trace records them.  Along the long axis (pass 1 for axis
    1, pass 2 for axis 2): exact multiples and near-multiples (remainder 1, 2, b - 1, b - 2) with quotients in the thousands
    and divisors above 1000 - the float quotient may land on either side of the integer -, and quotients of 32768 and more
    from the columns without a zero (the 32-bit floordiv's "do not push" answer).  Across it: only the latter, divisors <= 4."""
    for axis, which in ((1, 1), (2, 2)):
        div = []
        cnt, wrong = T.trace_pass(_limit_mask(LIMIT_SHAPES[axis]), which, divisions=div)
        c = _classes(div)
        print(LIMIT_SHAPES[axis], 'pass', which, len(div), c)
        assert wrong == 0 and c['exact'] >= 5 and c['near'] >= 5 and c['big'] >= 1000 and cnt['not_pushed'] >= 1000
    for axis, which, planes in ((0, 1, range(3000, 7100)), (0, 2, range(3000, 7100)), (1, 2, None), (2, 1, None)):
        div = []
        cnt, wrong = T.trace_pass(_limit_mask(LIMIT_SHAPES[axis]), which, planes, divisions=div)
        c = _classes(div)
        print(LIMIT_SHAPES[axis], 'pass', which, len(div), c)
        assert wrong == 0 and c['big'] >= 100 and c['max'] > 10 ** 6 and all(b <= 4 for _, b in div)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', LIMIT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_edt_at_the_limits_of_the_widths(shape):
    from arterynetwork_amd.generateVesselVolume import distance_transform_edt
    mask = _limit_mask(shape)
    assert np.array_equal(distance_transform_edt(mask), MO.distance_transform_edt(mask))


# ------------------------------------------------------------------ far distances
def _closed_form(shape, zero):
    """The distance to a mask's only zero voxel: the root of an exact integer, correctly rounded"""
    idx = np.indices(shape, dtype=np.int64)
    return np.sqrt(sum((idx[k] - zero[k]) ** 2 for k in range(3)).astype(np.float64))


FAR = [((23172, 1, 1), (0, 0, 0)), ((1, 23172, 1), (0, 0, 0)), ((1, 1, 23172), (0, 0, 0)),
       ((23171, 150, 1), (0, 0, 0)), ((150, 23171, 1), (0, 0, 0)), ((23171, 1, 150), (0, 0, 0)), ((1, 23171, 150), (0, 0, 0)),
       ((150, 1, 23171), (0, 0, 0)), ((1, 150, 23171), (0, 0, 0)),
       ((32000, 1, 2), (0, 0, 0)), ((32000, 1, 2), (31999, 0, 1)),
       ((1, 32000, 2), (0, 31999, 0)), ((2, 1, 32000), (1, 0, 0))]


def test_far_cases_pass_two_to_the_29_and_the_closed_form_is_the_oracle():
    for shape, zero in FAR:
        assert not _kernel_is_32bit(shape)
        far = sum(max(z, n - 1 - z) ** 2 for n, z in zip(shape, zero))
        assert (1 << 29) <= far < (1 << 32), (shape, far)
        if np.prod(shape) <= 100_000:
            mask = np.ones(shape, np.uint8)
            mask[zero] = 0
            ref = _closed_form(shape, zero)
            assert np.array_equal(ref, MO.distance_transform_edt(mask)) and ref.max() == np.sqrt(float(far))
    assert sum(n * n for n in (23170, 149, 0)) == 536_871_101 == (1 << 29) + 189


@pytest.mark.gpu
@pytest.mark.parametrize('shape,zero', FAR, ids=lambda v: 'x'.join(map(str, v)))
def test_edt_far_distances(shape, zero):
    """True squared distances of 2^29 and more (the "no zero voxel" value of the 32-bit width) up to 31999^2 + 1 along a line"""
    from arterynetwork_amd.generateVesselVolume import distance_transform_edt
    mask = np.ones(shape, np.uint8)
    mask[zero] = 0
    got = distance_transform_edt(mask)
    ref = _closed_form(shape, zero)
    bad = np.flatnonzero(got.ravel() != ref.ravel())
    assert not len(bad), (len(bad), bad[:3].tolist(), got.ravel()[bad[:3]].tolist(), ref.ravel()[bad[:3]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(23300, 1, 2), (1, 2, 23300)], ids=lambda s: 'x'.join(map(str, s)))
def test_vessel_mask_with_far_distances(shape):
    """k_threshold reads the same squared distances: with edtMax = 23200 (above sqrt(2^29) = 23170.5, below the farthest voxel's
    23299) the voxels beyond it keep a vesselness between the two thresholds, as in the oracle; distances clamped at 2^29 would
    clear them."""
    from arterynetwork_amd.generateVesselVolume import vesselVolumeMask
    brain = np.ones(shape, np.uint8)
    brain[0, 0, 0] = 0
    ves = np.random.default_rng(5).random(shape)
    ves.flat[:2] = 0.0, 1.0
    ref = MO.vesselVolumeMask(brain, ves, edtMax=23200, minSize=0)
    far = MO.distance_transform_edt(brain) > 23200
    assert far.sum() >= 90 and 10 <= ((ves > 0.7) & (ves <= 0.8) & far).sum() == (ref[far] != 0).sum() - (ves[far] > 0.8).sum()
    assert np.array_equal(vesselVolumeMask(brain, ves, edtMax=23200, minSize=0), ref)


@pytest.mark.gpu
def test_edt_far_distances_with_columns_and_planes_without_a_zero():
    """45 x 3 x 23300, zeros only in the plane i0 = 0 at i2 < 8 and i1 = 1: squared distances past 2^29 reached through columns
    and planes that hold no zero voxel (the wide sentinel must stay above them all), against scipy."""
    from arterynetwork_amd.generateVesselVolume import distance_transform_edt
    mask = np.ones((45, 3, 23300), np.uint8)
    mask[0, 1, :8] = 0
    got = distance_transform_edt(mask)
    far = 44 ** 2 + 1 + 23292 ** 2
    assert far > (1 << 29) + 10 ** 6 and got.max() == np.sqrt(float(far)) and np.array_equal(got, MO.distance_transform_edt(mask))
