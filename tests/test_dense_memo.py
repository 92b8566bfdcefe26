"""Option dense_memo (1: always; by default only volumes of more than 100 000 units): the 16-bit dense pass takes the intensity sum of a 256-voxel group whose voxels are all outer
from a table built once per volume (k_build_gsum) instead of fetching the group's level indices and looking its values up.

A full group is 256 aligned consecutive included voxels inside one row, so the volumes here have nx = 600 (padded rows of 608
voxels; 608 mod 256 != 0: every row has another alignment), a few rows and planes, and 16-bit storage forced.  Every case runs the
option on (1) against off (0: the kernel of before, bit for bit) and checks that groups really were memoised.

The sums of a memoising pass add the same doubles in another order.  On integer data every partial sum is exact: bit-identical
results.  On other data each sum is compared with math.fsum over the final labels within 2 n 2^-53 sum|x| - the worst case of any
two orders of n double additions (each addition rounds by at most 2^-53 of a partial sum that never exceeds sum|x|).  The values
the 16-bit pass adds are the volume's values as float32, so the volumes are given as float32."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import parity
from conftest import ROOT

NX = 600
PX = (NX + 2 + 15) // 16 * 16


@pytest.fixture(scope='module')
def lib():
    from arterynetwork_amd._capi import product_lib
    return product_lib()


def labels_and_tube(shape, rng):
    """Everything outer except a few excluded voxels near the row ends and a seeded tube across three rows of three planes at
    x = 40..55: the region grows along and around it and soon reaches every row, so the groups that begin at x <= 40 (a row's
    first full group begins at a multiple of 32 by its alignment) turn mixed while the run goes on and the others stay full.
    Returns (valueMap, tube mask)."""
    nx, ny, nz = shape
    vm = np.full(shape, 3, dtype=np.int64)
    u = rng.random(shape)
    ends = np.zeros(shape, dtype=bool)
    ends[:12] = True; ends[-12:] = True
    vm[ends & (u < 0.3)] = 4
    tube = np.zeros(shape, dtype=bool)
    tube[40:56, ny // 2 - 1:ny // 2 + 2, nz // 2 - 1:nz // 2 + 2] = True
    vm[46:50, ny // 2, nz // 2] = 0
    return vm, tube


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


def sum_bound(x):
    return 2.0 * len(x) * 2.0 ** -53 * math.fsum(np.abs(x))


def check_sums(data, lab, n_in, n_out, sum_in, sum_out, what):
    """counts exactly; sums within the reordering bound of math.fsum over the labels (the doubles of the float32 values)"""
    d = data.astype(np.float32).astype(np.float64)
    xin, xout = d[lab <= 1], d[(lab == 2) | (lab == 3)]
    assert (n_in, n_out) == (len(xin), len(xout)), what
    for got, x, name in ((sum_in, xin, 'sum_in'), (sum_out, xout, 'sum_out')):
        ref, bound = math.fsum(x), sum_bound(x)
        print('%s %s: got %.17g fsum %.17g |diff| %.3g bound %.3g' % (what, name, got, ref, abs(got - ref), bound))
        assert abs(got - ref) <= bound, (what, name, got, ref, bound)


def run_pair(lib, data, vmap, sweeps, H=2.25):
    """the same run with dense_memo 1 and 0 -> [(labels, trace, result, stats)] (index = the option's value)"""
    outs = {}
    for memo in (1, 0):
        s = session(lib, data, vmap, memo, H)
        r = s.run(sweeps, 10 ** 9, None)
        outs[memo] = (s.labels(), s.trace(), r, s.stats(), s.nlevels())
        s.close()
    assert outs[1][3]['dense_memo_groups'] > 0 and outs[0][3]['dense_memo_groups'] == 0
    assert outs[1][3]['dense_memo_bytes'] > 0
    assert outs[1][3]['level_index_bytes'] == outs[0][3]['level_index_bytes']
    return outs


def integer_case():
    rng = np.random.default_rng(5)
    shape = (NX, 8, 6)
    vm, tube = labels_and_tube(shape, rng)
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    data[tube] = rng.integers(4, 7, size=int(tube.sum()))
    return data, vm


def dense_bytes_memo_by_definition(labels):
    """tests/test_hostmodel.py's dense_bytes_by_definition restated for a memoising 16-bit pass: per listed whole unit of the
    slab 256 B of class words + 4 B of list entry + 32 B of group sums (a unit the slab's faces cut: 256 B, always); 128 B for
    every aligned run of 64 voxels that holds an included voxel outside the full groups - the aligned groups of 256 voxels, in
    whole units, whose voxels are all outer (labels 2 and 3).  Returns (bytes, full groups)."""
    nx, ny, nz = labels.shape
    px, py = (nx + 2 + 15) // 16 * 16, ny + 4
    n = (nz + 4) * py * px
    incl = np.zeros((n + 2048) // 1024 * 1024, dtype=bool)
    outer = np.zeros_like(incl)
    incl[:n].reshape(nz + 4, py, px)[2:nz + 2, 2:ny + 2, :nx] = np.transpose(labels != 4, (2, 1, 0))
    outer[:n].reshape(nz + 4, py, px)[2:nz + 2, 2:ny + 2, :nx] = np.transpose((labels == 2) | (labels == 3), (2, 1, 0))
    lo, hi = 2 * py * px, (nz + 2) * py * px
    f_lo, f_hi = (lo + 1023) >> 10, hi >> 10
    f_hi = max(f_hi, f_lo)
    listed = incl.reshape(-1, 1024).any(axis=1)
    full = outer.reshape(-1, 256).all(axis=1)
    nbytes = groups = 0
    fetched = incl.copy()
    fetched[:lo] = False; fetched[hi:] = False
    for u in range(lo >> 10, ((hi - 1) >> 10) + 1):
        whole = f_lo <= u < f_hi
        if whole and not listed[u]:
            continue
        nbytes += 292 if whole else 256
        if whole:
            for g in range(4 * u, 4 * u + 4):
                if full[g]:
                    groups += 1
                    fetched[256 * g:256 * g + 256] = False
    return nbytes + 128 * int(fetched.reshape(-1, 64).any(axis=1).sum()), groups


@pytest.mark.gpu
def test_integer_values_bit_identical_and_oracle(lib):
    """Integer values 0..6: labels and the whole trace - the f64 sums included - are byte-identical with the option on and off,
    and the run matches the oracle sweep by sweep.  dense_bytes follows the new definition (on) and the old one (off)."""
    from test_hostmodel import dense_bytes_by_definition
    data, vm = integer_case()
    outs = run_pair(lib, data, vm, 12)
    assert outs[1][2].sweeps == outs[0][2].sweeps > 0
    assert np.array_equal(outs[1][0], outs[0][0])
    assert outs[1][1].tobytes() == outs[0][1].tobytes()
    init_groups = dense_bytes_memo_by_definition(vm)[1]
    nbytes, groups = dense_bytes_memo_by_definition(outs[1][0])
    print('full groups: labels as given %d, after the run %d; dense_bytes %d (memo) %d (off)' % (init_groups, groups, nbytes, outs[0][3]['dense_bytes']))
    assert 0 < groups < init_groups                                  # (groups turned mixed during the run)
    assert outs[1][3]['dense_memo_groups'] == groups and outs[1][3]['dense_bytes'] == nbytes
    assert outs[0][3]['dense_bytes'] == dense_bytes_by_definition(outs[0][0], 64)
    res, k = parity.run_stepwise(lib, data, vm, 2.25, None, 12, density_mode=1, check_hist=True, options={'storage16': 1, 'dense_memo': 1})
    assert res is not None and k == outs[1][2].sweeps


def fraction_case(levels, div, seed):
    rng = np.random.default_rng(seed)
    shape = (NX, 7, 5)
    vm, tube = labels_and_tube(shape, rng)
    data = rng.integers(0, levels, size=shape) / div
    data[tube] += 0.5
    return data.astype(np.float32), vm


@pytest.mark.gpu
@pytest.mark.parametrize('levels,div,mode', [(400, 397.0, 3), (6000, 5987.0, 1)])
def test_non_dyadic_values_within_the_reordering_bound(lib, levels, div, mode):
    """Values that are no dyadic fractions (400 levels: the table of doubles, kernel mode 3; more than 4096 levels: the table of
    floats, mode 1): the counts are identical with the option on and off, each sum is within the reordering bound of math.fsum,
    and two runs with the option on are byte-identical."""
    data, vm = fraction_case(levels, div, 7)
    outs = run_pair(lib, data, vm, 8)
    assert (outs[1][4] > 4096) == (mode == 1) and ',%d,' % mode in outs[1][3]['dense_kernel'], (outs[1][4], outs[1][3]['dense_kernel'])
    for f in ('nflip', 'nseg', 'n_in', 'n_out', 'ni', 'no'):
        assert np.array_equal(outs[1][1][f], outs[0][1][f]), f
    assert np.array_equal(outs[1][0], outs[0][0])
    for memo in (1, 0):
        lab, tr, r = outs[memo][:3]
        check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'levels %d memo %d' % (levels, memo))
        assert (tr['sum_in'][-1], tr['sum_out'][-1]) == (r.sum_in, r.sum_out)
    again = run_pair(lib, data, vm, 8)
    assert again[1][1].tobytes() == outs[1][1].tobytes() and np.array_equal(again[1][0], outs[1][0])


@pytest.mark.gpu
def test_sums_follow_the_volume(lib):
    """The group sums belong to the volume: after set_volume with other values on the same handle they are rebuilt with the
    level indices and the sums are the new volume's; a re-init without set_volume rebuilds nothing and changes nothing."""
    data, vm = fraction_case(400, 397.0, 7)
    rng = np.random.default_rng(8)
    data2 = (rng.integers(0, 300, size=data.shape) / 293.0 + 1.25).astype(np.float32)
    s = session(lib, data, vm, 1)
    s.run(4, 10 ** 9, None)
    builds = s.stats()['level_index_builds']
    s.set_volume(data2); s.set_labels(vm.astype(np.uint8)); s.init(2.25)
    r = s.run(4, 10 ** 9, None)
    st = s.stats()
    assert st['level_index_builds'] == builds + 1 and st['dense_memo_groups'] > 0
    first = (s.labels(), s.trace().tobytes())
    check_sums(data2, first[0], r.n_in, r.n_out, r.sum_in, r.sum_out, 'new volume')
    s.set_labels(vm.astype(np.uint8)); s.init(2.25)
    s.run(4, 10 ** 9, None)
    assert s.stats()['level_index_builds'] == builds + 1
    assert np.array_equal(s.labels(), first[0]) and s.trace().tobytes() == first[1]
    s.close()


@pytest.mark.gpu
def test_slabs_add_up(lib):
    """Two Z-slabs of one volume, each counted by a handle of its own (the reduction callback hands every slab the totals a
    whole-volume handle found, so each runs as a rank of two): the slabs' counts add up to the whole exactly and their sums
    within the reordering bound, at init and after every sweep.  The slab's face is no multiple of 1024 voxels: it cuts a unit
    (which, with two padding rows on either side of a plane, holds no voxel of the volume), and the whole units next to it are
    rows of full groups."""
    data, vm = fraction_case(400, 397.0, 9)
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
        s = session(lib, data, vm, 1, slab=slab, cb=recorder(key, None if key == 'whole' else seen['whole']))
        s.run(sweeps, 10 ** 9, None)
        runs[key] = (s.labels(), s.stats()['dense_memo_groups'])
        s.close()
    assert len(seen['whole']) == len(seen['a']) == len(seen['b']) == sweeps + 1
    assert runs['a'][1] > 0 and runs['b'][1] > 0 and runs['a'][1] + runs['b'][1] == runs['whole'][1]
    assert np.array_equal(runs['a'][0], runs['whole'][0]) and np.array_equal(runs['b'][0], runs['whole'][0])
    d = data.astype(np.float64)
    bound = sum_bound(d.reshape(-1))                                   # (of all voxels: no sum of a pass has more addends)
    for k, (w, a, b) in enumerate(zip(seen['whole'], seen['a'], seen['b'])):
        assert a[0] + b[0] == w[0] and a[1] + b[1] == w[1], k
        print('pass %d: sum_in %.3g sum_out %.3g off; bound %.3g' % (k, abs(a[2] + b[2] - w[2]), abs(a[3] + b[3] - w[3]), bound))
        assert abs(a[2] + b[2] - w[2]) <= bound and abs(a[3] + b[3] - w[3]) <= bound, k
    lab = runs['whole'][0]
    check_sums(data, lab, int(seen['whole'][-1][0]), int(seen['whole'][-1][1]), seen['whole'][-1][2], seen['whole'][-1][3], 'whole volume, last pass')


def test_memo_definition_equals_the_old_one_without_full_groups():
    """No GPU needed: the restated byte count differs from test_hostmodel's only by the 32 B of sums per whole listed unit
    where no group is full - the volumes of test_skip_excluded_is_bit_identical (rows of 256 and 83 voxels) have none."""
    from arterynetwork_amd import phantoms
    from test_hostmodel import dense_bytes_by_definition
    d, v = phantoms.bench_volume((256, 192, 96), seed=4)
    rng = np.random.default_rng(21)
    u = rng.random((83, 61, 47))
    vm = np.full(u.shape, 3, dtype=np.int64); vm[u < 0.03] = 0; vm[u > 0.55] = 4
    for lab in (v, vm):
        nbytes, groups = dense_bytes_memo_by_definition(lab)
        assert groups == 0
        assert (nbytes - dense_bytes_by_definition(lab, 64)) % 32 == 0 and nbytes > dense_bytes_by_definition(lab, 64)
    _, vm1 = integer_case()
    assert dense_bytes_memo_by_definition(vm1)[1] > 0


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_recount_kernels_resources(tmp_path):
    """No GPU needed (the method of tests/test_kernel_resources.py): the 16-bit recount kernels that skip excluded voxels -
    k_recount_bits, MODE 1 and 3, SKIP, with and without the memo - use no scratch and at most 128 VGPRs (four workgroups
    per CU).  Measured: 65 (mode 3) and 62 (mode 1) with the memo, 66 and 61 without."""
    from arterynetwork_amd import build
    out = tmp_path / 'vrg_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vrg_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    found = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):
        k = re.search(r'14k_recount_bitsILi3ELb([01])ELi([13])ELb1ELb([01])E', m.group(1))     # <3, NT, MODE, SKIP = true, MEMO>
        if k:
            f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
            found[k.groups()] = (f('private_segment_fixed_size'), f('vgpr_count'))
    assert len(found) == 8, sorted(found)
    for key, (scratch, vgpr) in found.items():
        print('k_recount_bits<3,NT=%s,MODE=%s,true,MEMO=%s>: %d VGPRs' % (key + (vgpr,)))
        assert scratch == 0 and vgpr <= 128, (key, scratch, vgpr)
