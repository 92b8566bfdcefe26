"""The memoising walk of the 16-bit dense pass (option dense_memo = 2) decides per TRIP of three units whether it takes every sum
from the tables of init (the short way) - one count per unit instead of one per group (csrc/vrg_rim.h, "the unit-level decision").

Why one count is enough: inclusion is monotone (tests/test_dense_rim_memo.py states and checks it on the oracle's labels).  In a unit
without inner voxels the outer voxels are the included ones, group by group a superset of what init included; equal totals then force
equal groups.  The CPU tests run the header's arithmetic in a host program against plain population counts and against the per-group
decision (vrg_rim_decide) on units built by the monotone rule; the resource test reads the kernels' metadata; the GPU tests compare
the product with dense_memo = 0 byte for byte, and with the oracle, where the walk can go wrong: lists that end inside a trip, trips
that leave the short way and come back, two full units in one packed word, values that are no dyadic fractions.  The walk takes the
short way only with whole trips of three matching units (two trips at a time where two make a pair), so every recipe is walked in numpy
on the oracle's labels first (walk_trips) and the tests assert how many of its trips take the short way, alone and in pairs, pass by pass."""
import os
import re
import subprocess

import numpy as np
import pytest

import parity
from conftest import ROOT
from test_dense_rim_memo import (check_stats, flat_index, idx_px, memoised_groups, oracle_labels, padded, rim_fraction_case)
from test_dense_memo import check_sums


@pytest.fixture(scope='module')
def lib():
    from arterynetwork_amd._capi import product_lib
    return product_lib()


# ---- the arithmetic, on the host ------------------------------------------------------------------------------------------------
UNIT_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "vrg_rim.h"
// A trip of the walk (k_recount_bits, RIM): three units of 64 class words, the four counts of init per unit.  What the wave does with
// them, the cross-lane steps as what they are - 32-bit additions of each lane's two words over all 64 lanes -, against the per-group
// decision of vrg_rim_decide ("every group of the trip that holds an included voxel takes its sum from the table").
struct Trip { uint32_t w[3][64]; uint32_t ic[3][4]; };
static bool short_way(const Trip& t) {
    uint32_t t01 = 0, t2i = 0;
    for (uint32_t l = 0; l < 64; l++) {
        const uint32_t q = (l >> 2) < 2 ? (l >> 2) : 2;                 // the slot whose counts lane l fetches: word l & 1 of them
        const uint32_t d = t.ic[q][2 * (l & 1)] | t.ic[q][2 * (l & 1) + 1] << 16;
        const uint32_t share = vrg_unit_share(d);
        t01 += vrg_unit_word01(t.w[0][l], t.w[1][l], share, vrg_unit_role01(l));
        t2i += vrg_unit_word2i(t.w[0][l], t.w[1][l], t.w[2][l], share, vrg_unit_role2i(l));
    }
    return vrg_unit_short(t01, t2i);
}
static bool unit_by_groups(const uint32_t* w, const uint32_t* ic) {    // the walk before: all four groups through vrg_rim_decide
    uint32_t a = 0, b = 0, inner = 0, ne = 0, total = 0;
    for (int l = 0; l < 64; l++) {
        (l < 32 ? a : b) += vrg_rim_pack(w[l]);
        for (int j = 0; j < 4; j++) if ((w[l] >> (8 * j)) & 0x55u) inner |= 1u << j;
    }
    const uint32_t m = vrg_rim_decide(a, b, inner, ic[0] | ic[1] << 16, ic[2] | ic[3] << 16, ne, total);
    return m == ne;
}
static uint32_t popcounts(const uint32_t* w, uint32_t mask) { uint32_t n = 0; for (int l = 0; l < 64; l++) n += __builtin_popcount(w[l] & mask); return n; }
static int bad = 0;
static void expect(const Trip& t, const char* what) {
    bool want = true;
    for (int q = 0; q < 3; q++) {
        const bool g = unit_by_groups(t.w[q], t.ic[q]);
        // ... and both against the definition in plain counts: no inner voxel, and per group as many outer voxels as init counted
        bool def = popcounts(t.w[q], 0x55555555u) == 0;
        for (int j = 0; j < 4; j++) def = def && popcounts(t.w[q], 0xAAu << (8 * j)) == t.ic[q][j];
        if (g != def) { std::printf("FAIL %s: unit %d by groups %d, by definition %d\n", what, q, (int)g, (int)def); bad++; }
        want = want && g;
    }
    const bool got = short_way(t);
    if (got != want) { std::printf("FAIL %s: short way %d, per group %d\n", what, (int)got, (int)want); bad++; }
}
static void clear(Trip& t) { std::memset(&t, 0, sizeof t); }
static void set_outer(Trip& t, int q, uint32_t voxel) { t.w[q][(voxel & 255u) >> 2] |= 2u << (8 * (voxel >> 8) + 2 * (voxel & 3u)); }     // voxel 0..1023 of the unit: group voxel >> 8, lane (voxel & 255) >> 2
static void set_inner(Trip& t, int q, uint32_t voxel) { const uint32_t s = 8 * (voxel >> 8) + 2 * (voxel & 3u); uint32_t& x = t.w[q][(voxel & 255u) >> 2]; x = (x & ~(3u << s)) | 1u << s; }
static void fill(Trip& t, int q, uint32_t n) {                          // n outer voxels, and init's counts to match
    for (int l = 0; l < 64; l++) t.w[q][l] = 0;
    for (uint32_t v = 0; v < n; v++) set_outer(t, q, (v * 613u) % 1024u);               // (613 is odd: n distinct voxels)
    for (int j = 0; j < 4; j++) t.ic[q][j] = popcounts(t.w[q], 0xAAu << (8 * j));
}
int main() {
    Trip t;
    // unit totals 0, 1, 1023 and 1024 in every slot, the other slots empty and full; a count of init one below must not match
    for (int q = 0; q < 3; q++) for (uint32_t n : {0u, 1u, 1023u, 1024u}) for (uint32_t other : {0u, 1024u}) {
        clear(t);
        for (int p = 0; p < 3; p++) fill(t, p, p == q ? n : other);
        expect(t, "unit total");
        if (!short_way(t)) { std::printf("FAIL unit total %u in slot %d beside %u: not the short way\n", n, q, other); bad++; }
        // (one less, not one more: a group never holds fewer included voxels than at init, and the two decisions part on such a state)
        for (int j = 0; j < 4; j++) if (t.ic[q][j]) { t.ic[q][j]--; expect(t, "count of init one less"); if (short_way(t)) { std::printf("FAIL one less accepted\n"); bad++; } t.ic[q][j]++; }
    }
    // two units in one word, 1024 | 1024, 0 | 1024, 1024 | 0: no carry between the fields, and none into the other word
    for (uint32_t n0 : {0u, 1024u}) for (uint32_t n1 : {0u, 1024u}) for (uint32_t n2 : {0u, 1024u}) {
        clear(t); fill(t, 0, n0); fill(t, 1, n1); fill(t, 2, n2);
        expect(t, "packed pair");
        if (!short_way(t)) { std::printf("FAIL packed %u %u %u\n", n0, n1, n2); bad++; }
        if (n0) { t.ic[0][3] = 255; expect(t, "1023 of 1024"); if (short_way(t)) { std::printf("FAIL 1024 against 1023 accepted\n"); bad++; } }
    }
    // one outer voxel in one lane only; one inner voxel in one lane only; the inner voxel outer again
    for (int q = 0; q < 3; q++) for (uint32_t lane : {0u, 15u, 16u, 31u, 32u, 63u}) for (uint32_t j = 0; j < 4; j++) {
        clear(t);
        set_outer(t, q, 256u * j + 4u * lane + (lane & 3u));
        t.ic[q][j] = 1;
        expect(t, "one outer voxel");
        if (!short_way(t)) { std::printf("FAIL one outer voxel, lane %u\n", lane); bad++; }
        t.ic[q][j] = 0; expect(t, "one outer voxel, none at init"); if (short_way(t)) { std::printf("FAIL voxel init did not count accepted\n"); bad++; }
    }
    for (int q = 0; q < 3; q++) for (uint32_t lane : {0u, 31u, 32u, 63u}) {
        clear(t);
        for (int p = 0; p < 3; p++) fill(t, p, 700);
        const uint32_t v = 256u * (lane & 3u) + 4u * lane + 1u;
        const bool was_outer = (t.w[q][lane] >> (8 * (lane & 3u) + 2)) & 2u;
        set_inner(t, q, v);
        expect(t, "one inner voxel");
        if (short_way(t)) { std::printf("FAIL inner voxel in lane %u accepted\n", lane); bad++; }
        t.w[q][lane] &= ~(3u << (8 * (lane & 3u) + 2));
        if (was_outer) set_outer(t, q, v);
        expect(t, "the inner voxel outer again");
        if (!short_way(t)) { std::printf("FAIL inner voxel turned back, lane %u: not the short way\n", lane); bad++; }
    }
    // a voxel included after init into a group that was empty then, the other three groups as at init: the total is one above
    for (int q = 0; q < 3; q++) for (uint32_t j = 0; j < 4; j++) {
        clear(t);
        for (int p = 0; p < 3; p++) fill(t, p, 1024);
        for (int l = 0; l < 64; l++) t.w[q][l] &= ~(0xffu << (8 * j));
        t.ic[q][j] = 0;
        expect(t, "a group empty at init");
        if (!short_way(t)) { std::printf("FAIL empty group\n"); bad++; }
        set_outer(t, q, 256u * j + 77u);
        expect(t, "included after init into an empty group");
        if (short_way(t)) { std::printf("FAIL inclusion into an empty group accepted\n"); bad++; }
    }
    // 20 000 random trips by the monotone rule: init's included set, later inclusions, inner voxels among the included
    std::srand(11);
    int shorts = 0;
    for (int n = 0; n < 20000; n++) {
        clear(t);
        for (int q = 0; q < 3; q++) {
            const int dens = std::rand() % 5, later = std::rand() % 4 == 0, inner = std::rand() % 6 == 0;
            for (uint32_t v = 0; v < 1024; v++) {
                const bool empty_group = dens == 4 && (v >> 8) == (uint32_t)(n & 3);
                const bool at_init = !empty_group && (dens == 3 || std::rand() % 4 <= dens);
                if (at_init) t.ic[q][v >> 8]++;
                if (at_init || (later && std::rand() % 300 == 0)) { if (inner && std::rand() % 500 == 0) set_inner(t, q, v); else set_outer(t, q, v); }
            }
        }
        expect(t, "random");
        shorts += short_way(t);
    }
    std::printf("%d of 20000 random trips take the short way\n", shorts);
    if (shorts < 2000 || shorts > 18000) { std::printf("FAIL the random trips do not exercise both ways\n"); bad++; }
    std::printf("%s\n", bad ? "BAD" : "OK");
    return bad != 0;
}
'''


def test_unit_decision_equals_the_groups_decision(tmp_path):
    """No GPU needed.  csrc/vrg_rim.h's unit-level arithmetic compiled for the host: the packed words of the 64 lanes added with plain
    32-bit additions (what the six DPP steps do) decide a trip's short way exactly as the four groups of each of its units did through
    vrg_rim_decide, and both agree with plain population counts.  Unit totals 0, 1, 1023, 1024 in every slot beside empty and full
    neighbours (no carry between the 16-bit fields), one outer voxel in lane 0, 15, 16, 31, 32 or 63 only, one inner voxel in lane 0,
    31, 32 or 63 only and turned outer again, a voxel included into a group that was empty at init, counts of init one off, and
    20 000 random trips built by the monotone rule, every one of them compared."""
    cxx = os.environ.get('CXX', 'g++')
    src, exe = tmp_path / 'unit.cpp', tmp_path / 'unit'
    src.write_text(UNIT_PROGRAM)
    p = subprocess.run([cxx, '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:]


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_unit_walk_spills_nothing(tmp_path):
    """No GPU needed (the method of tests/test_dense_rim_memo.py::test_rim_kernels_resources): k_recount_bits<3, NT, MODE 1 and 3,
    SKIP, MEMO, RIM> spill no scalar register (73 before the walk fetched its per-unit data with vector loads), use no scratch and at
    most 128 VGPRs.  Measured: 84 VGPRs (mode 3) and 82 (mode 1)."""
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
            found[k.groups()] = (f('sgpr_spill_count'), f('private_segment_fixed_size'), f('vgpr_count'))
    assert len(found) == 4, sorted(found)
    for key, (spills, scratch, vgpr) in sorted(found.items()):
        print('k_recount_bits<3,NT=%s,MODE=%s,true,true,true>: %d SGPR spills, %d B scratch, %d VGPRs' % (key + (spills, scratch, vgpr)))
        assert spills == 0 and scratch == 0 and vgpr <= 128, (key, spills, scratch, vgpr)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def run(lib, data, vmap, sweeps, memo, blocks):
    """one run with dense_memo = memo and the dense grid at `blocks` workgroups (0: the default)
    -> (labels, trace, result, stats at the end, stats at init, labels at init)"""
    from arterynetwork_amd._capi import Session
    s = Session(data.shape, lib=lib)
    s.set_option('storage16', 1); s.set_option('dense_memo', memo)
    if blocks:
        s.set_option('sweep_blocks', blocks)
    s.set_volume(data); s.set_labels(vmap.astype(np.uint8)); s.init(2.25)
    st0, lab0 = s.stats(), s.labels()
    r = s.run(sweeps, 10 ** 9, None)
    out = (s.labels(), s.trace(), r, s.stats(), st0, lab0)
    s.close()
    return out


def compare_with_memo_0_and_oracle(lib, data, vm, sweeps, blocks, what):
    """labels and the whole trace - f64 sums included - byte for byte with dense_memo = 0 on the same grid; stepwise parity with the
    oracle.  Returns the run with the option at 2."""
    a, b = run(lib, data, vm, sweeps, 2, blocks), run(lib, data, vm, sweeps, 0, blocks)
    assert a[2].sweeps == b[2].sweeps > 0, what
    assert np.array_equal(a[0], b[0]), what
    assert a[1].tobytes() == b[1].tobytes(), what
    if blocks:
        assert a[3]['dense_workgroups'] == b[3]['dense_workgroups'] == blocks, what
    options = {'storage16': 1, 'dense_memo': 2}
    if blocks:
        options['sweep_blocks'] = blocks
    res, k = parity.run_stepwise(lib, data, vm.astype(np.uint8), 2.25, None, sweeps, density_mode=1, check_hist=True, options=options)
    assert res is not None and k > 0, what
    return a


def listed_units(lab):
    """the whole units of the volume that hold an included voxel, ascending: what the pass's list holds"""
    nx, ny, nz = lab.shape
    plane = (ny + 4) * idx_px(nx)
    u = np.flatnonzero(padded(lab != 4).reshape(-1, 1024).any(axis=1))
    return u[(u >= (2 * plane + 1023) >> 10) & (u < ((2 + nz) * plane) >> 10)]


def unit_matches(lab0, lab):
    """per unit of the padded volume: every group is memoised by memoised_groups, or empty now and at init - the unit passes the
    walk's test"""
    memo, cnt0 = memoised_groups(lab0, lab)
    inner = padded(lab <= 1).reshape(-1, 256).any(axis=1)
    nout = padded((lab == 2) | (lab == 3)).reshape(-1, 256).sum(axis=1)
    return (memo | ((cnt0 == 0) & (nout == 0) & ~inner)).reshape(-1, 4).all(axis=1)


def walk_trips(lab0, lab, blocks):
    """The walk restated on labels: the list's consecutive triples are the trips (whatever the grid); a trip takes the short way iff
    it is whole and its three units match.  With `blocks` workgroups of four waves, wave w takes the trips at list positions
    3 w + k step, step = 12 blocks, two at a time while both are whole and both pass (the loop of pairs), otherwise one.
    Returns ([(units, short way)], turns of the loop of pairs)."""
    ok, units = unit_matches(lab0, lab), listed_units(lab)
    n, step = len(units), 12 * blocks
    trips = [(units[k:k + 3], bool(k + 3 <= n and ok[units[k:k + 3]].all())) for k in range(0, n, 3)]
    pairs = 0
    for w in range(4 * blocks):
        i = 3 * w
        while i < n:
            both = i + step + 3 <= n and trips[i // 3][1] and trips[(i + step) // 3][1]
            pairs += both
            i += 2 * step if both else step
    return trips, pairs


def short_way_counts(labs, blocks, what):
    """(trips on the short way, turns of the loop of pairs) of the pass at init and behind every sweep, printed"""
    out = []
    for lab in labs:
        trips, pairs = walk_trips(labs[0], lab, blocks)
        out.append((sum(t[1] for t in trips), pairs))
    print('%s, %d workgroups: (short trips, paired turns) per pass %s' % (what, blocks, out))
    return out


def ragged_case(n):
    """Rows of 1104 padded voxels, three rows per plane (tests/test_dense_rim_memo.py's width_case family), everything excluded but
    the voxels of exactly n units: the units around the seeds first, then the others in ascending order.  A third of the voxels of
    every odd group is excluded as well (rim groups).  A seed's neighbours in the rows beside it lie 1104 voxels away, in other units,
    and init includes them: with three rows no list of fewer than three units can hold a seed, so n = 1 has one row and one plane.
    Returns (data, valueMap)."""
    ny, nz = (1, 1) if n == 1 else (3, {3: 1, 4: 1, 12: 3, 13: 3, 36: 9, 37: 9, 61: 15}[n])
    shape = (1102, ny, nz)
    rng = np.random.default_rng(1000 + n)
    idx = flat_index(shape)
    unit = idx >> 10
    plane = (ny + 4) * idx_px(1102)
    ids = np.unique(unit)
    ids = ids[(ids >= (2 * plane + 1023) >> 10) & (ids < ((2 + nz) * plane) >> 10)]
    zc, yc, x0 = nz // 2, ny // 2, 500
    near = np.unique(unit[x0 - 2:x0 + 8, :, max(zc - 1, 0):zc + 2])
    assert len(near) <= n
    keep = (list(near) + [u for u in ids if u not in set(near)])[:n]
    vm = np.full(shape, 4, dtype=np.int64)
    vm[np.isin(unit, keep)] = 3
    vm[(((idx >> 8) & 1) == 1) & (idx % 3 == 0)] = 4
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    tube = np.zeros(shape, dtype=bool)
    tube[x0:x0 + 6, :, zc] = True                        # (one plane: the region stays in the three units of its rows)
    tube &= np.isin(unit, keep)
    data[tube] = rng.integers(4, 7, size=int(tube.sum()))
    vm[tube] = 3
    vm[x0 + 2:x0 + 4, yc, zc] = 0
    return data, vm


RAGGED = [1, 3, 4, 12, 13, 36, 37, 3 * 12 + 1 + 2 * 12]


@pytest.mark.parametrize('n', RAGGED)
def test_ragged_cases_list_n_units(n):
    """No GPU needed: the recipe lists exactly n units at init (restated from the labels as given: init's inclusions stay inside them)."""
    data, vm = ragged_case(n)
    assert len(listed_units(vm)) == n


@pytest.mark.parametrize('n', RAGGED)
def test_ragged_cases_reach_the_short_way(n):
    """No GPU needed.  The walk restated on the oracle's labels: from 12 units on trips take the short way in the pass at init, from
    36 units on in every pass; the loop of pairs turns at init from 36 units on at both grids, in every pass with 8 waves, and with 61
    units in every pass at both grids.  (A list of up to 4 units holds the seeds' units in its only whole trip.)"""
    data, vm = ragged_case(n)
    labs = oracle_labels(data, vm, 6, 'unit-ragged-%d' % n)
    for lab in labs:
        assert len(listed_units(lab)) == n
    c1, c2 = short_way_counts(labs, 1, 'n %d' % n), short_way_counts(labs, 2, 'n %d' % n)
    assert len(labs) >= 3
    if n >= 12:
        assert c1[0][0] > 0
    if n >= 36:
        assert all(c[0] > 0 for c in c1) and c1[0][1] > 0 and all(c[1] > 0 for c in c2)
    if n >= 61:
        assert all(c[1] > 0 for c in c1)


@pytest.mark.gpu
@pytest.mark.parametrize('blocks', [1, 2])
@pytest.mark.parametrize('n', RAGGED)
def test_ragged_lists(lib, n, blocks):
    """Lists of 1, 3, 4, 12, 13, 36, 37 and 61 units walked by 4 and by 8 waves (trips of 3 units, 12 resp. 24 units per round of
    the grid): shorter than one trip, exactly one, one over, whole rounds and rounds with a tail - the entries and tables a wave
    requests up to five trips past the list's end are clamped to its last entry and add nothing.  Integer values: labels and trace
    byte-identical with dense_memo = 0 on the same grid, stepwise parity with the oracle, the statistics equal the restatement."""
    data, vm = ragged_case(n)
    a = compare_with_memo_0_and_oracle(lib, data, vm, 6, blocks, 'n %d, %d workgroups' % (n, blocks))
    assert a[4]['dense_listed_units'] == n and a[3]['dense_listed_units'] == n, (a[4]['dense_listed_units'], a[3]['dense_listed_units'])
    assert len(listed_units(a[5])) == n and len(listed_units(a[0])) == n
    _, rim0 = check_stats(a[4], a[5], a[5], 'init, n %d' % n)
    check_stats(a[3], a[5], a[0], 'end, n %d' % n)
    assert rim0 > 0 and a[3]['dense_rim_groups'] > 0
    lab, tr, r = a[:3]
    check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'n %d' % n)


LEAVE_SWEEPS = 9


def leave_case():
    """254 x 5 x 20 (rows of 256 padded voxels: a group is a row, a unit four rows; 25 400 voxels in 40 listed units, so that the
    units below sit in whole trips beside units nothing happens to, and the loop of pairs turns at 4 and at 8 waves).  A tube of
    3 x 2 rows along all of x in the planes z = 1, 2 holds seeds at x = 0..1, 126..129 and 252..253 - lanes 0, 31 / 32 and 63 of
    their groups (lane = (x mod 256) / 4) -; the row y = 2, z = 3, two voxels from the seeds' row, is excluded whole, so the region's
    growth includes voxels into a group that was empty at init; two isolated seeds lie in the noise of the planes z = 10 and 15 and
    flip out again.  Integer values 0..3, the tube 4..6."""
    rng = np.random.default_rng(11)
    shape = (254, 5, 20)
    vm = np.full(shape, 3, dtype=np.int64)
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    tube = np.zeros(shape, dtype=bool)
    tube[:, 1:4, 1:3] = True
    data[tube] = rng.integers(4, 7, size=int(tube.sum()))
    for x0, x1 in ((0, 2), (126, 130), (252, 254)):
        vm[x0:x1, 2, 1] = 0
    vm[:, 2, 3] = 4
    vm[:, 0, 0] = 4
    vm[60, 2, 10] = 0; vm[200, 2, 15] = 0
    return data, vm


def check_leave_case(labs):
    """Each kind of unit must at some pass sit in a whole trip whose other two units match, so that the trip's way depends on that
    unit alone: a unit that matches at init and stops matching (its trip on the short way at init, off it later through that unit
    alone); a unit that holds an inner voxel in one pass and none later (its trip off the short way through it alone, on it later);
    a unit that never matches; a unit with a 4 -> 3 inclusion into a group that was empty at init, its other three groups as at init."""
    oks = [unit_matches(labs[0], lab) for lab in labs]
    found = {'stops': set(), 'clears': set(), 'never': set(), 'grown': set()}
    alone = {}                                                   # unit -> the passes in which its trip fails through it alone
    short = {}                                                   # unit -> the passes in which its trip takes the short way
    for k, lab in enumerate(labs):
        trips, _ = walk_trips(labs[0], lab, 1)
        for units, way in trips:
            for u in units:
                if way:
                    short.setdefault(int(u), []).append(k)
                elif len(units) == 3 and not oks[k][u] and all(oks[k][v] for v in units if v != u):
                    alone.setdefault(int(u), []).append(k)
    inner = [padded(lab <= 1).reshape(-1, 1024).any(axis=1) for lab in labs]
    cnt0 = padded(labs[0] != 4).reshape(-1, 256).sum(axis=1)
    for u, ks in alone.items():
        if 0 in short.get(u, []) and not any(oks[k][u] for k in range(1, len(labs))):
            found['stops'].add(u)
        if any(inner[k][u] for k in ks) and not inner[-1][u] and len(labs) - 1 in short.get(u, []):
            found['clears'].add(u)
        if not any(o[u] for o in oks):
            found['never'].add(u)
        for k in ks:
            nout = padded((labs[k] == 2) | (labs[k] == 3)).reshape(-1, 256).sum(axis=1)[4 * u:4 * u + 4]
            new = (cnt0[4 * u:4 * u + 4] == 0) & (nout > 0)
            if new.sum() == 1 and (nout[~new] == cnt0[4 * u:4 * u + 4][~new]).all() and not inner[k][u]:
                found['grown'].add(u)
    idx = flat_index(labs[0].shape)
    lanes = sorted(set(((idx[labs[-1] <= 1] & 255) >> 2).tolist()))
    print('units that alone take their trip off the short way:', {k: sorted(v) for k, v in found.items()})
    print('lanes the region\'s voxels fall into:', lanes)
    assert all(found.values()), found
    assert {0, 31, 32, 63} <= set(lanes)
    for blocks in (1, 2):
        counts = short_way_counts(labs, blocks, 'leave')
        assert all(c[0] > 0 and c[1] > 0 for c in counts), counts      # trips on the short way, alone and in pairs, in every pass


def test_leave_case_holds_all_three_kinds_of_units():
    """No GPU needed.  On the oracle's labels of the recipe, through the numpy restatement of the walk (check_leave_case): the three
    kinds of units and the inclusion into an empty group, each deciding its trip alone; the region's voxels in lanes 0, 31, 32 and 63;
    trips on the short way, single and in pairs, in every pass at both grids."""
    data, vm = leave_case()
    labs = oracle_labels(data, vm, LEAVE_SWEEPS, 'unit-leave')
    assert len(labs) == LEAVE_SWEEPS + 1
    check_leave_case(labs)


@pytest.mark.gpu
@pytest.mark.parametrize('blocks', [1, 2])
def test_leaving_and_reentering_the_short_way(lib, blocks):
    """The recipe on the GPU, 9 sweeps, 4 and 8 waves: byte-identical with dense_memo = 0, stepwise parity with the oracle, the labels
    at init and at the end the oracle's (so the run holds the trips the CPU test found), the statistics equal the restatement."""
    data, vm = leave_case()
    a = compare_with_memo_0_and_oracle(lib, data, vm, LEAVE_SWEEPS, blocks, 'leave, %d workgroups' % blocks)
    labs = oracle_labels(data, vm, LEAVE_SWEEPS, 'unit-leave')
    assert a[2].sweeps == LEAVE_SWEEPS
    assert np.array_equal(a[5], labs[0]) and np.array_equal(a[0], labs[-1])
    check_leave_case(labs)
    _, rim0 = check_stats(a[4], a[5], a[5], 'init')
    check_stats(a[3], a[5], a[0], 'end')
    assert rim0 > 0 and a[3]['dense_rim_groups'] > 0
    lab, tr, r = a[:3]
    check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'leave')


def two_full_units_case():
    """2200 x 3 x 3: rows of 2208 padded voxels; the row y = 2, z = 2 begins at voxel 32 * 2208 = 69 * 1024 and covers units 69 and
    70 whole.  Everything is outer but the seeds; one earlier unit is excluded where that is needed to put the two units into slots
    0 and 1 of one trip (list positions 3 m and 3 m + 1: the two fields of one packed word)."""
    rng = np.random.default_rng(22)
    shape = (2200, 3, 3)
    idx = flat_index(shape)
    vm = np.full(shape, 3, dtype=np.int64)
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    tube = np.zeros(shape, dtype=bool)
    tube[40:56, 0:2, 0:2] = True                          # (x < 160: clear of the units excluded below)
    data[tube] = rng.integers(4, 7, size=int(tube.sum()))
    vm[46:50, 0, 0] = 0
    units = listed_units(vm)
    pos = int(np.flatnonzero(units == 69)[0])
    vm[np.isin(idx >> 10, units[pos - pos % 3:pos])] = 4     # (the units just in front of 69: the far end of the row y = 1, z = 2, nowhere near the seeds)
    return data, vm


def test_two_full_units_share_a_trip():
    """No GPU needed: the recipe puts units 69 and 70, 1024 outer voxels each, into list positions 3 m and 3 m + 1."""
    data, vm = two_full_units_case()
    units = listed_units(vm)
    pos = int(np.flatnonzero(units == 69)[0])
    assert pos % 3 == 0 and units[pos + 1] == 70
    assert (padded((vm == 2) | (vm == 3)).reshape(-1, 1024).sum(axis=1)[69:71] == 1024).all()
    labs = oracle_labels(data, vm, 6, 'unit-two-full')
    for lab in labs:                                             # ... and the trip takes the short way in every pass
        trips, _ = walk_trips(labs[0], lab, 1)
        assert [way for units, way in trips if 69 in units] == [True] and [list(units[:2]) for units, way in trips if 69 in units] == [[69, 70]]
    assert all(c[1] > 0 for c in short_way_counts(labs, 1, 'two full units'))


@pytest.mark.gpu
def test_two_full_units_in_one_trip(lib):
    """Totals of 1024 + 1024 in one packed word: units 69 and 70, all outer, in slots 0 and 1 of one trip; 4 waves.  Byte-identical
    with dense_memo = 0, stepwise parity with the oracle, the statistics equal the restatement."""
    data, vm = two_full_units_case()
    a = compare_with_memo_0_and_oracle(lib, data, vm, 6, 1, 'two full units')
    units = listed_units(a[5])
    pos = int(np.flatnonzero(units == 69)[0])
    assert pos % 3 == 0 and units[pos + 1] == 70, (pos, units[pos:pos + 2])
    assert np.array_equal(a[0], oracle_labels(data, vm, 6, 'unit-two-full')[-1])           # (the labels test_two_full_units_share_a_trip walks)
    memo, cnt0 = memoised_groups(a[5], a[0])
    assert (memo & (cnt0 == 256))[4 * 69:4 * 71].all()                 # both units full and memoised, at the end as well
    assert a[4]['dense_listed_units'] == len(units)
    check_stats(a[4], a[5], a[5], 'init')
    check_stats(a[3], a[5], a[0], 'end')


@pytest.mark.gpu
@pytest.mark.parametrize('levels,div,mode', [(400, 397.0, 3), (6000, 5987.0, 1)])
def test_non_dyadic_values_on_four_waves(lib, levels, div, mode):
    """tests/test_dense_rim_memo.py's non-dyadic case at sweep_blocks = 1: the counts identical with dense_memo = 0, each sum within
    the reordering bound of math.fsum, two runs byte-identical."""
    data, vm = rim_fraction_case(levels, div, 7)
    a, b = run(lib, data, vm, 8, 2, 1), run(lib, data, vm, 8, 0, 1)
    assert ',%d,' % mode in a[3]['dense_kernel'], a[3]['dense_kernel']
    assert a[3]['dense_workgroups'] == b[3]['dense_workgroups'] == 1
    assert a[4]['dense_rim_groups'] > 0 and a[3]['dense_rim_groups'] > 0
    for f in ('nflip', 'nseg', 'n_in', 'n_out', 'ni', 'no'):
        assert np.array_equal(a[1][f], b[1][f]), f
    assert np.array_equal(a[0], b[0])
    for memo, o in ((2, a), (0, b)):
        lab, tr, r = o[:3]
        check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'levels %d memo %d' % (levels, memo))
        assert (tr['sum_in'][-1], tr['sum_out'][-1]) == (r.sum_in, r.sum_out)
    check_stats(a[3], a[5], a[0], 'levels %d' % levels)
    again = run(lib, data, vm, 8, 2, 1)
    assert again[1].tobytes() == a[1].tobytes() and np.array_equal(again[0], a[0])


def quiet_fraction_case(levels, div):
    """leave_case's labels on values that are no dyadic fractions, integers below `levels` over div, the tube 3.0 above the noise: the
    region stays in the tube and ten trips stay on the short way through all sweeps"""
    d0, vm = leave_case()
    rng = np.random.default_rng(7)
    data = rng.integers(0, levels, size=d0.shape) / div
    data[d0 >= 4] += 3.0
    return data.astype(np.float32), vm


@pytest.mark.parametrize('levels,div', [(400, 397.0), (6000, 5987.0)])
def test_quiet_fraction_case_stays_on_the_short_way(levels, div):
    """No GPU needed.  The walk restated on the oracle's labels: in the pass at init and behind each of the 8 sweeps at least 8 trips
    take the short way and the loop of pairs turns at least twice with 4 waves (measured: 10 trips; 3 turns at init, then 4)."""
    data, vm = quiet_fraction_case(levels, div)
    labs = oracle_labels(data.astype(np.float64), vm, 8, 'unit-quiet-%d' % levels)
    assert len(labs) == 9
    assert all(c[0] >= 8 and c[1] >= 2 for c in short_way_counts(labs, 1, 'levels %d' % levels))


@pytest.mark.gpu
@pytest.mark.parametrize('levels,div,mode', [(400, 397.0, 3), (6000, 5987.0, 1)])
def test_non_dyadic_values_on_the_short_way(lib, levels, div, mode):
    """Non-dyadic values added on the short way in every pass (the case above; 4 waves): the counts identical with dense_memo = 0,
    each sum within the reordering bound of math.fsum, two runs byte-identical, the labels the oracle's."""
    data, vm = quiet_fraction_case(levels, div)
    a, b = run(lib, data, vm, 8, 2, 1), run(lib, data, vm, 8, 0, 1)
    assert ',%d,' % mode in a[3]['dense_kernel'], a[3]['dense_kernel']
    assert a[3]['dense_workgroups'] == b[3]['dense_workgroups'] == 1
    assert a[2].sweeps == b[2].sweeps == 8
    for f in ('nflip', 'nseg', 'n_in', 'n_out', 'ni', 'no'):
        assert np.array_equal(a[1][f], b[1][f]), f
    assert np.array_equal(a[0], b[0])
    labs = oracle_labels(data.astype(np.float64), vm, 8, 'unit-quiet-%d' % levels)
    assert np.array_equal(a[5], labs[0]) and np.array_equal(a[0], labs[-1])
    for memo, o in ((2, a), (0, b)):
        lab, tr, r = o[:3]
        check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'quiet, levels %d memo %d' % (levels, memo))
        assert (tr['sum_in'][-1], tr['sum_out'][-1]) == (r.sum_in, r.sum_out)
    check_stats(a[3], a[5], a[0], 'quiet, levels %d' % levels)
    again = run(lib, data, vm, 8, 2, 1)
    assert again[1].tobytes() == a[1].tobytes() and np.array_equal(again[0], a[0])
