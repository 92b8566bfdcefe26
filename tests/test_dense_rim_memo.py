"""Option dense_memo = 2: the 16-bit dense pass takes the outer sum of a 256-voxel group from a table built at init (k_build_rim:
isum, icnt) whenever the group holds no inner voxel and exactly as many outer voxels as it held included voxels at init - the rim
groups of the brain mask (outer and excluded voxels mixed) and, as the case of 256, the full groups of dense_memo = 1.

Why that is right: inclusion is monotone.  A voxel only ever goes 4 -> 3 in the reference, nothing is set to 4 after the start, and
the product never sets the excluded bit after init; so the included set of a group only grows, and a group without inner voxels
whose outer count equals the included count of init has exactly init's included set as its outer set.  The CPU tests check the
monotony on the oracle's labels and restate, in numpy, which groups are memoised and what the pass then requests; the GPU tests
compare the product with that restatement, with the option at 0 and 1, with the oracle and with math.fsum.

Sums: as in tests/test_dense_memo.py - integer data gives exact partial sums (byte-identical traces), other data is held to the
reordering bound 2 n 2^-53 sum|x| of math.fsum."""
import os
import re
import subprocess

import numpy as np
import pytest

import parity
from conftest import ROOT
from test_dense_memo import NX, PX, check_sums, fraction_case, labels_and_tube, sum_bound

SWEEPS = 12


@pytest.fixture(scope='module')
def lib():
    from arterynetwork_amd._capi import product_lib
    return product_lib()


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
def padded(mask):
    """a [x][y][z] mask of the real voxels -> the flat padded volume (two planes / rows of padding, rows of PX voxels), whole units"""
    nx, ny, nz = mask.shape
    px, py = (nx + 2 + 15) // 16 * 16, ny + 4
    n = (nz + 4) * py * px
    out = np.zeros((n + 2048) // 1024 * 1024, dtype=bool)
    out[:n].reshape(nz + 4, py, px)[2:nz + 2, 2:ny + 2, :nx] = np.transpose(mask, (2, 1, 0))
    return out


def flat_index(shape):
    """the padded flat index of every real voxel, as an [x][y][z] array"""
    nx, ny, nz = shape
    px, py = (nx + 2 + 15) // 16 * 16, ny + 4
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij')
    return ((z + 2) * py + (y + 2)) * px + x


def memoised_groups(labels0, labels):
    """which aligned 256-voxel groups of the padded volume take their sum from the table, by the labels at init and now: no inner
    voxel (labels 0, 1), and as many outer voxels (2, 3) as there were included voxels (not 4) at init, not 0.
    Returns (memoised, count at init) per group."""
    cnt0 = padded(labels0 != 4).reshape(-1, 256).sum(axis=1)
    inner = padded(labels <= 1).reshape(-1, 256).any(axis=1)
    nout = padded((labels == 2) | (labels == 3)).reshape(-1, 256).sum(axis=1)
    return ~inner & (nout == cnt0) & (cnt0 > 0), cnt0


def dense_bytes_rim_by_definition(labels0, labels, slab=None):
    """tests/test_dense_memo.py's dense_bytes_memo_by_definition restated for dense_memo = 2: per listed whole unit of the slab
    256 B of class words + 4 B of list entry + 32 B of sums + 8 B of counts (a unit the slab's faces cut: 256 B, always); 128 B for
    every aligned run of 64 voxels that holds an included voxel outside the memoised groups of whole units.
    Returns (bytes, memoised groups of 256 voxels, memoised groups of fewer)."""
    nx, ny, nz = labels.shape
    px, py = (nx + 2 + 15) // 16 * 16, ny + 4
    z0, z1 = slab if slab else (0, nz)
    incl = padded(labels != 4)
    memo, cnt0 = memoised_groups(labels0, labels)
    lo, hi = (2 + z0) * py * px, (2 + z1) * py * px
    f_lo, f_hi = (lo + 1023) >> 10, hi >> 10
    f_hi = max(f_hi, f_lo)
    listed = incl.reshape(-1, 1024).any(axis=1)
    nbytes = full = rim = 0
    fetched = incl.copy()
    fetched[:lo] = False; fetched[hi:] = False
    for u in range(lo >> 10, ((hi - 1) >> 10) + 1):
        whole = f_lo <= u < f_hi
        if whole and not listed[u]:
            continue
        nbytes += 300 if whole else 256
        if whole:
            for g in range(4 * u, 4 * u + 4):
                if memo[g]:
                    if cnt0[g] == 256:
                        full += 1
                    else:
                        rim += 1
                    fetched[256 * g:256 * g + 256] = False
    return nbytes + 128 * int(fetched.reshape(-1, 64).any(axis=1).sum()), full, rim


# ---- the recipe ------------------------------------------------------------------------------------------------------------------
def rim_case():
    """600 x 8 x 6 on labels_and_tube: x >= 300 excluded in the rows y < 4 (every such row ends in a rim group), half of the
    voxels of x = 58..89 excluded at random (rim groups the region reaches: 4 -> 3 inclusions there are what the count has to
    notice), a tube of 3 x 3 rows along x = 40..119 seeded at x = 46..49, and two isolated seeds in the background noise (they flip
    out again: a group that held an inner voxel at init matches its count afterwards).  Integer values 0..3, the tube 4..6."""
    rng = np.random.default_rng(5)
    shape = (NX, 8, 6)
    nx, ny, nz = shape
    vm, _ = labels_and_tube(shape, rng)
    vm[300:, :4, :] = 4
    u = rng.random(shape)
    part = np.zeros(shape, dtype=bool); part[58:90] = True
    vm[part & (u < 0.5)] = 4
    tube = np.zeros(shape, dtype=bool)
    tube[40:120, ny // 2 - 1:ny // 2 + 2, nz // 2 - 1:nz // 2 + 2] = True
    vm[46:50, ny // 2, nz // 2] = 0
    vm[200, 6, 1] = 0; vm[450, 6, 4] = 0
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    data[tube] = rng.integers(4, 7, size=int(tube.sum()))
    return data, vm


_oracle_cache = {}


def oracle_labels(data, vm, sweeps, key):
    """the oracle's labels at init and after every sweep (computed once per case, shared)"""
    if key not in _oracle_cache:
        from oracle import vrg_oracle as O
        o = O.Oracle(data, vm.astype(np.uint8), 2.25, 1)
        o.init()
        labs = [o.labels()]
        for _ in range(sweeps):
            if o.step(sweeps, data.size + 1, -1.0) != 0:
                break
            labs.append(o.labels())
        o.close()
        _oracle_cache[key] = labs
    return _oracle_cache[key]


def test_restatement_on_the_recipe():
    """No GPU needed.  On the oracle's labels of the recipe, sweep by sweep: the included set contains the previous one (monotone);
    the restatement finds memoised rim groups at init, groups lost to 4 -> 3 inclusions later, and groups regained (an inner voxel
    at init, matching again once it has flipped out).  Measured here: 111 memoisable groups at init, 89 of them rim groups (105 and 81
    once the seeds' neighbourhoods have turned); from sweep 7 on 19 and then up to 33 groups stop matching their count because of
    4 -> 3 inclusions; 2 groups that held an inner voxel at init match again from sweep 1 on."""
    data, vm = rim_case()
    labs = oracle_labels(data, vm, SWEEPS, 'rim')
    assert len(labs) == SWEEPS + 1
    for a, b in zip(labs, labs[1:]):
        assert not ((a != 4) & (b == 4)).any()                           # monotone: no included voxel becomes excluded
    assert (labs[0] == 4).sum() > (labs[-1] == 4).sum()                  # ... and some were included on the way
    m0, cnt0 = memoised_groups(labs[0], labs[0])
    lost, regained = [], []
    for k, lab in enumerate(labs):
        m, _ = memoised_groups(labs[0], lab)
        nout = padded((lab == 2) | (lab == 3)).reshape(-1, 256).sum(axis=1)
        lost.append(int(((nout > cnt0) & (cnt0 > 0)).sum()))            # more included voxels than at init: the table's sum is not the group's
        regained.append(int((m & ~m0).sum()))
        print('sweep %2d: memoised %3d (rim %3d), lost to inclusion %2d, regained %d' % (k, m.sum(), (m & (cnt0 < 256)).sum(), lost[-1], regained[-1]))
    assert (m0 & (cnt0 < 256)).sum() > 0 and (m0 & (cnt0 == 256)).sum() > 0
    assert lost[0] == 0 and max(lost) > 0 and max(regained) > 0
    # the recipe's counts, pinned (generator seed 5 as above; the issue's own figures - 105 memoisable groups of which 80 rim, 16 and then up
    # to 33 lost from sweep 7 on, 2 regained - came from a volume it gives no seed for: the shape of the run is the same, the random
    # exclusions of x = 58..89 and the noise differ; its 105 is the count once the seeds' neighbourhoods have turned, as here)
    memo_k = [int(memoised_groups(labs[0], lab)[0].sum()) for lab in labs]
    rim_k = [int((memoised_groups(labs[0], lab)[0] & (cnt0 < 256)).sum()) for lab in labs]
    assert memo_k == [111] + [105] * 6 + [86, 77, 75, 72, 72, 72]
    assert rim_k == [89] + [81] * 6 + [62, 53, 51, 48, 48, 48]
    assert lost == [0] * 7 + [19, 28, 30, 33, 33, 33] and regained == [0] + [2] * 12
    nbytes, full, rim = dense_bytes_rim_by_definition(labs[0], labs[0])
    assert (full, rim) == (int((m0 & (cnt0 == 256)).sum()), int((m0 & (cnt0 < 256)).sum()))   # (the volume's groups lie in whole units)


def test_full_groups_are_those_of_the_memo_definition():
    """No GPU needed.  Without excluded voxels the memoised groups of 256 voxels are the full groups of dense_memo = 1; the groups a
    row's last voxels share with the padding are rim groups."""
    from test_dense_memo import dense_bytes_memo_by_definition
    vm = np.full((NX, 6, 4), 3, dtype=np.int64)
    vm[46:50, 3, 2] = 0
    _, g1 = dense_bytes_memo_by_definition(vm)
    _, full, rim = dense_bytes_rim_by_definition(vm, vm)
    assert full == g1 > 0 and rim > 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def session(lib, data, vmap, memo, H=2.25, slab=None, cb=None):
    from arterynetwork_amd._capi import Session
    s = Session(data.shape, lib=lib)
    s.set_option('storage16', 1); s.set_option('dense_memo', memo)
    if slab:
        s.set_slab(*slab)
    if cb:
        s.set_reduce_callback(cb)
    s.set_volume(data); s.set_labels(vmap.astype(np.uint8)); s.init(H)
    return s


def run_memo(lib, data, vmap, sweeps, memos=(2, 1, 0)):
    """the same run with dense_memo at each of memos -> {memo: (labels, trace, result, stats at the end, stats at init, labels at init)}
    (the labels at init are not the labels as given: init includes the excluded neighbours of the seeds, 4 -> 3, as the reference does)"""
    outs = {}
    for memo in memos:
        s = session(lib, data, vmap, memo)
        st0, lab0 = s.stats(), s.labels()
        r = s.run(sweeps, 10 ** 9, None)
        outs[memo] = (s.labels(), s.trace(), r, s.stats(), st0, lab0)
        s.close()
    return outs


def check_stats(st, labels0, labels, what, slab=None):
    nbytes, full, rim = dense_bytes_rim_by_definition(labels0, labels, slab)
    print('%s: dense_bytes %d (restated %d), full groups %d (%d), rim groups %d (%d)' % (what, st['dense_bytes'], nbytes, st['dense_memo_groups'], full, st['dense_rim_groups'], rim))
    assert (st['dense_bytes'], st['dense_memo_groups'], st['dense_rim_groups']) == (nbytes, full, rim), what
    return full, rim


@pytest.mark.gpu
def test_integer_values_bit_identical_and_oracle(lib):
    """The recipe, integer values: labels and the whole trace - the f64 sums included - are byte-identical with the option at 2, 1
    and 0; stepwise parity with the oracle; dense_bytes and the two group counts equal the restatement at init and at the end, and
    fewer rim groups are memoised at the end than the initial labels give."""
    data, vm = rim_case()
    outs = run_memo(lib, data, vm, SWEEPS)
    assert outs[2][2].sweeps == outs[1][2].sweeps == outs[0][2].sweeps == SWEEPS
    for memo in (1, 0):
        assert np.array_equal(outs[2][0], outs[memo][0]), memo
        assert outs[2][1].tobytes() == outs[memo][1].tobytes(), memo
        assert outs[memo][3]['dense_rim_groups'] == 0
    assert outs[2][3]['dense_rim_bytes'] == 10 * 4 * (((6 + 4) * (8 + 4) * PX + 1023) // 1024) and outs[0][3]['dense_memo_groups'] == 0
    assert np.array_equal(outs[2][0], oracle_labels(data, vm, SWEEPS, 'rim')[-1])
    assert np.array_equal(outs[2][5], oracle_labels(data, vm, SWEEPS, 'rim')[0])
    _, rim0 = check_stats(outs[2][4], outs[2][5], outs[2][5], 'init')
    _, rim1 = check_stats(outs[2][3], outs[2][5], outs[2][0], 'after %d sweeps' % SWEEPS)
    assert 0 < rim1 < rim0
    assert outs[2][3]['dense_kernel'] == outs[1][3]['dense_kernel'] == outs[0][3]['dense_kernel']
    res, k = parity.run_stepwise(lib, data, vm, 2.25, None, SWEEPS, density_mode=1, check_hist=True, options={'storage16': 1, 'dense_memo': 2})
    assert res is not None and k == SWEEPS


def rim_fraction_case(levels, div, seed):
    """the recipe's labels on tests/test_dense_memo.py's non-dyadic values"""
    data, _ = fraction_case(levels, div, seed)
    rng = np.random.default_rng(seed + 100)
    vm, tube = labels_and_tube(data.shape, rng)
    vm[300:, :3, :] = 4
    vm[(rng.random(data.shape) < 0.5) & (np.arange(data.shape[0])[:, None, None] >= 58) & (np.arange(data.shape[0])[:, None, None] < 90)] = 4
    vm[46:50, data.shape[1] // 2, data.shape[2] // 2] = 0
    return data, vm


@pytest.mark.gpu
@pytest.mark.parametrize('levels,div,mode', [(400, 397.0, 3), (6000, 5987.0, 1)])
def test_non_dyadic_values_within_the_reordering_bound(lib, levels, div, mode):
    """Values that are no dyadic fractions (400 levels: kernel mode 3; more than 4096: mode 1): the counts are identical with the
    option at 2 and 0, each sum is within the reordering bound of math.fsum, two runs with the option on are byte-identical."""
    data, vm = rim_fraction_case(levels, div, 7)
    outs = run_memo(lib, data, vm, 8, (2, 0))
    assert ',%d,' % mode in outs[2][3]['dense_kernel'], outs[2][3]['dense_kernel']
    assert outs[2][4]['dense_rim_groups'] > 0 and outs[2][3]['dense_rim_groups'] > 0
    for f in ('nflip', 'nseg', 'n_in', 'n_out', 'ni', 'no'):
        assert np.array_equal(outs[2][1][f], outs[0][1][f]), f
    assert np.array_equal(outs[2][0], outs[0][0])
    for memo in (2, 0):
        lab, tr, r = outs[memo][:3]
        check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'levels %d memo %d' % (levels, memo))
        assert (tr['sum_in'][-1], tr['sum_out'][-1]) == (r.sum_in, r.sum_out)
    check_stats(outs[2][3], outs[2][5], outs[2][0], 'levels %d' % levels)
    again = run_memo(lib, data, vm, 8, (2,))
    assert again[2][1].tobytes() == outs[2][1].tobytes() and np.array_equal(again[2][0], outs[2][0])


def width_case(nx, ny, nz, units=False):
    """Integer values on nx x ny x nz with a seeded tube.  Labels: the odd 256-voxel groups of the padded volume excluded where
    x < nx // 2 (so every row width meets the groups its own way and most groups are rim groups), one group with exactly one
    included voxel and one with all its real voxels but one (255 where rows are wide enough to hold a whole group).  units = True: every even 1024-voxel UNIT excluded instead - a unit of four full groups
    lies beside a unit of four empty ones wherever a row covers both (a wave then counts 4 x 256 outer voxels: what 8-bit fields
    could not hold)."""
    rng = np.random.default_rng(nx)
    shape = (nx, ny, nz)
    idx = flat_index(shape)
    vm = np.full(shape, 3, dtype=np.int64)
    if units:
        vm[((idx >> 10) & 1) == 0] = 4
    else:
        vm[(((idx >> 8) & 1) == 1) & (idx % 3 != 0)] = 4
    groups = idx >> 8
    ids, n = np.unique(groups, return_counts=True)
    lo_u, hi_u = (2 * (ny + 4) * idx_px(nx) + 1023) >> 10, ((nz + 2) * (ny + 4) * idx_px(nx)) >> 10
    inside = (ids >> 2 >= lo_u) & (ids >> 2 < hi_u)              # groups of the whole units
    y, z = ny // 2, nz // 2
    x0 = nx // 3
    inside &= ~np.isin(ids, groups[x0:x0 + 16, y - 1:y + 2, z - 1:z + 2])             # (not the tube's groups)
    ids, n = ids[inside], n[inside]
    order = np.argsort(-n, kind='stable')
    g_most, g_one = ids[order[0]], ids[order[1]]                # (256 real voxels each where a row is at least 511 voxels wide)
    vm[groups == g_most] = 3; vm[idx == idx[groups == g_most][77]] = 4
    vm[groups == g_one] = 4; vm[idx == idx[groups == g_one][130]] = 3
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    tube = np.zeros(shape, dtype=bool)
    tube[x0:x0 + 16, y - 1:y + 2, z - 1:z + 2] = True
    data[tube] = rng.integers(4, 7, size=int(tube.sum()))
    vm[tube] = 3; vm[x0 + 6:x0 + 10, y, z] = 0
    cnt0 = padded(vm != 4).reshape(-1, 256).sum(axis=1)
    assert cnt0[g_one] == 1 and cnt0[g_most] == n[order[0]] - 1 and (cnt0[g_most] == 255 or nx < 511)
    return data, vm


def idx_px(nx):
    return (nx + 2 + 15) // 16 * 16


@pytest.mark.gpu
@pytest.mark.parametrize('nx,ny,nz,units', [(30, 12, 8, False), (254, 5, 4, False), (270, 5, 4, False), (1102, 3, 3, True)])        # (1102 x 3 x 3: the row y = 2, z = 1 covers unit 27 whole)
def test_row_widths(lib, nx, ny, nz, units):
    """Rows of 32 padded voxels (a group spans eight rows), of 256 and of 272, and rows of 1104 with whole units of full groups
    beside empty ones (the field-overflow case of the count); a group with exactly 1 included voxel everywhere, and one with all but
    one of its real voxels - exactly 255 in the wide rows, where a group lies inside a row.
    Integer values: traces byte-identical with the option at 2 and 0, the statistics equal the restatement at init and at the end."""
    data, vm = width_case(nx, ny, nz, units)
    assert idx_px(nx) == {30: 32, 254: 256, 270: 272, 1102: 1104}[nx]
    outs = run_memo(lib, data, vm, 6, (2, 0))
    assert outs[2][2].sweeps == outs[0][2].sweeps > 0
    assert np.array_equal(outs[2][0], outs[0][0]) and outs[2][1].tobytes() == outs[0][1].tobytes()
    full0, rim0 = check_stats(outs[2][4], outs[2][5], outs[2][5], 'init %d' % nx)
    check_stats(outs[2][3], outs[2][5], outs[2][0], 'end %d' % nx)
    assert rim0 > 0
    if units:
        memo, cnt0 = memoised_groups(outs[2][5], outs[2][5])
        m4 = (memo & (cnt0 == 256)).reshape(-1, 4).all(axis=1)
        e4 = (cnt0 == 0).reshape(-1, 4).all(axis=1)
        assert (m4[:-1] & e4[1:]).any() and full0 >= 4                  # a unit of four full groups beside a unit of four empty ones
    lab, tr, r = outs[2][:3]
    check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'width %d' % nx)


@pytest.mark.gpu
def test_tables_follow_labels_and_volume(lib):
    """Re-init on one handle with other labels (set_labels + init): the sums are those of the new exclusion mask; after set_volume
    they are those of the new volume.  The tables are rebuilt at every init."""
    data, vm = rim_fraction_case(400, 397.0, 7)
    rng = np.random.default_rng(8)
    vm2 = vm.copy()
    vm2[300:, :3, :] = 3; vm2[:280, 4:, :] = np.where(rng.random(vm2[:280, 4:, :].shape) < 0.4, 4, vm2[:280, 4:, :])
    vm2[46:50, data.shape[1] // 2, data.shape[2] // 2] = 0
    data2 = (rng.integers(0, 300, size=data.shape) / 293.0 + 1.25).astype(np.float32)
    s = session(lib, data, vm, 2)
    lab0 = s.labels()
    r = s.run(4, 10 ** 9, None)
    check_sums(data, s.labels(), r.n_in, r.n_out, r.sum_in, r.sum_out, 'first labels')
    check_stats(s.stats(), lab0, s.labels(), 'first labels')
    s.set_labels(vm2.astype(np.uint8)); s.init(2.25)
    lab0 = s.labels()                                                  # (init has included the excluded neighbours of the seeds)
    assert not np.array_equal(lab0 != 4, vm2 != 4)
    check_stats(s.stats(), lab0, lab0, 'new labels, init')
    tr0 = s.trace()
    check_sums(data, lab0, int(tr0['n_in'][0]), int(tr0['n_out'][0]), tr0['sum_in'][0], tr0['sum_out'][0], 'new labels, init')
    r = s.run(4, 10 ** 9, None)
    check_sums(data, s.labels(), r.n_in, r.n_out, r.sum_in, r.sum_out, 'new labels')
    assert check_stats(s.stats(), lab0, s.labels(), 'new labels, end')[1] > 0
    s.set_volume(data2); s.set_labels(vm2.astype(np.uint8)); s.init(2.25)
    lab0 = s.labels()
    tr0 = s.trace()
    check_sums(data2, lab0, int(tr0['n_in'][0]), int(tr0['n_out'][0]), tr0['sum_in'][0], tr0['sum_out'][0], 'new volume, init')
    r = s.run(4, 10 ** 9, None)
    check_sums(data2, s.labels(), r.n_in, r.n_out, r.sum_in, r.sum_out, 'new volume')
    assert check_stats(s.stats(), lab0, s.labels(), 'new volume, end')[1] > 0
    s.close()


@pytest.mark.gpu
def test_slabs_add_up(lib):
    """Two Z-slabs whose face cuts a unit, each counted by a handle of its own (as tests/test_dense_memo.py::test_slabs_add_up):
    counts add up exactly and sums within the reordering bound, at init and after every sweep; each slab memoises rim groups."""
    data, vm = rim_fraction_case(400, 397.0, 9)
    nx, ny, nz = data.shape
    zc = 2
    assert ((2 + zc) * (ny + 4) * PX) % 1024 != 0
    sweeps = 5
    seen = {}

    def recorder(key, totals):
        seen[key] = []

        def cb(v):
            seen[key].append(list(v))
            return totals[len(seen[key]) - 1] if totals is not None else list(v)
        return cb
    runs = {}
    for key, slab in (('whole', (0, nz)), ('a', (0, zc)), ('b', (zc, nz))):
        s = session(lib, data, vm, 2, slab=slab, cb=recorder(key, None if key == 'whole' else seen['whole']))
        lab0 = s.labels()
        s.run(sweeps, 10 ** 9, None)
        runs[key] = (s.labels(), s.stats(), lab0)
        s.close()
    assert len(seen['whole']) == len(seen['a']) == len(seen['b']) == sweeps + 1
    assert np.array_equal(runs['a'][0], runs['whole'][0]) and np.array_equal(runs['b'][0], runs['whole'][0])
    for key, slab in (('whole', (0, nz)), ('a', (0, zc)), ('b', (zc, nz))):
        assert check_stats(runs[key][1], runs[key][2], runs[key][0], 'slab ' + key, slab)[1] > 0
    bound = sum_bound(data.astype(np.float64).reshape(-1))               # (of all voxels: no sum of a pass has more addends)
    for k, (w, a, b) in enumerate(zip(seen['whole'], seen['a'], seen['b'])):
        assert a[0] + b[0] == w[0] and a[1] + b[1] == w[1], k
        print('pass %d: sum_in %.3g sum_out %.3g off; bound %.3g' % (k, abs(a[2] + b[2] - w[2]), abs(a[3] + b[3] - w[3]), bound))
        assert abs(a[2] + b[2] - w[2]) <= bound and abs(a[3] + b[3] - w[3]) <= bound, k
    lab = runs['whole'][0]
    check_sums(data, lab, int(seen['whole'][-1][0]), int(seen['whole'][-1][1]), seen['whole'][-1][2], seen['whole'][-1][3], 'whole volume, last pass')


COUNT_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "vrg_rim.h"
// what rim_groups (vrg_device.hip) does with the 64 class words of a unit, the cross-lane steps as what they are - 32-bit additions of the
// packed words over lanes 0..31 and 32..63 - against plain population counts
static int check(const uint32_t* w, const uint32_t* icnt, const char* what) {
    uint32_t a = 0, b = 0, inner = 0, want_n[4], want_m = 0, want_ne = 0, want_total = 0;
    for (int l = 0; l < 64; l++) { (l < 32 ? a : b) += vrg_rim_pack(w[l]); }
    for (int j = 0; j < 4; j++) {
        uint32_t n = 0, in = 0;
        for (int l = 0; l < 64; l++) { const uint32_t wj = (w[l] >> (8 * j)) & 0xffu; n += __builtin_popcount(wj & 0xAAu); in += __builtin_popcount(wj & 0x55u); }
        want_n[j] = n; want_total += n;
        if (in) inner |= 1u << j;
        if (n || in) want_ne |= 1u << j;
        if (!in && n && n == icnt[j]) want_m |= 1u << j;
    }
    uint32_t ne = 0, total = 0;
    const uint32_t m = vrg_rim_decide(a, b, inner, icnt[0] | icnt[1] << 16, icnt[2] | icnt[3] << 16, ne, total);
    if (m != want_m || ne != want_ne || total != want_total) {
        std::printf("FAIL %s: groups %x (want %x) non-empty %x (%x) outer %u (%u) counts %u %u %u %u\n", what, m, want_m, ne, want_ne, total, want_total, want_n[0], want_n[1], want_n[2], want_n[3]);
        return 1;
    }
    return 0;
}
int main() {
    int bad = 0, memoised = 0;
    uint32_t w[64], ic[4];
    // four full groups: 4 x 256 outer voxels (what 8-bit fields could not hold), then each named count in every group position
    for (int l = 0; l < 64; l++) w[l] = 0xAAAAAAAAu;
    ic[0] = ic[1] = ic[2] = ic[3] = 256; bad += check(w, ic, "4 x 256");
    for (int j = 0; j < 4; j++) for (uint32_t n : {0u, 1u, 2u, 127u, 128u, 129u, 255u, 256u}) {
        for (int l = 0; l < 64; l++) w[l] = 0xAAAAAAAAu & ~(0xffu << (8 * j));
        for (uint32_t v = 0; v < n; v++) { const uint32_t pos = (v * 37u) % 256u; w[pos >> 2] |= 2u << (8 * j + 2 * (pos & 3u)); }      // (37 is odd: n distinct voxels)
        for (int k = 0; k < 4; k++) ic[k] = 256; ic[j] = n;
        bad += check(w, ic, "named count");
        ic[j] = n + 1; bad += check(w, ic, "count of init one more");                    // must not be memoised
        if (n) { w[5] |= 1u << (8 * j); bad += check(w, ic, "an inner voxel"); }
    }
    std::srand(7);
    for (int t = 0; t < 20000; t++) {
        const int dens = std::rand() % 4;
        for (int l = 0; l < 64; l++) {
            uint32_t x = 0;
            for (int v = 0; v < 16; v++) { const int r = std::rand() % 64; x |= (dens == 3 || r < 20 * (dens + 1) ? 2u : (r == 63 && t % 7 == 0 ? 1u : 0u)) << (2 * v); }
            w[l] = x;
        }
        for (int j = 0; j < 4; j++) { uint32_t n = 0; for (int l = 0; l < 64; l++) n += __builtin_popcount((w[l] >> (8 * j)) & 0xAAu); ic[j] = n + (std::rand() % 5 == 0); }
        bad += check(w, ic, "random");
    }
    std::printf("%s\n", bad ? "BAD" : "OK");
    return bad != 0;
}
'''


def test_packed_count_equals_popcounts(tmp_path):
    """No GPU needed.  The arithmetic of the pass's count (csrc/vrg_rim.h: the per-lane byte counts, the sum of the two half-waves, the
    comparison with init's counts) compiled for the host and compared with plain population counts: 0, 1, 2, 127..129, 255 and 256 outer
    voxels in each group position beside three full groups, four full groups at once (4 x 256), a count of init that is one off, an
    inner voxel, and 20 000 random units.  The statistics the GPU tests compare come from k_dense_bytes, which counts another way; this
    is what holds the pass's own count to the definition."""
    cxx = os.environ.get('CXX', 'g++')
    src, exe = tmp_path / 'count.cpp', tmp_path / 'count'
    src.write_text(COUNT_PROGRAM)
    p = subprocess.run([cxx, '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-2000:]


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_rim_kernels_resources(tmp_path):
    """No GPU needed (the method of tests/test_dense_memo.py::test_recount_kernels_resources): the instantiations of dense_memo = 2 -
    k_recount_bits<3, NT, MODE 1 and 3, SKIP, MEMO, RIM> - use no scratch and at most 128 VGPRs.  Measured: 73-74 (mode 3) and
    72 (mode 1)."""
    from arterynetwork_amd import build
    out = tmp_path / 'vrg_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vrg_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    found = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):
        k = re.search(r'14k_recount_bitsILi3ELb([01])ELi([13])ELb1ELb1ELb1EE', m.group(1))     # <3, NT, MODE, SKIP, MEMO, RIM = true>
        if k:
            f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
            found[k.groups()] = (f('private_segment_fixed_size'), f('vgpr_count'))
    assert len(found) == 4, sorted(found)
    for key, (scratch, vgpr) in found.items():
        print('k_recount_bits<3,NT=%s,MODE=%s,true,true,true>: %d VGPRs' % (key + (vgpr,)))
        assert scratch == 0 and vgpr <= 128, (key, scratch, vgpr)
