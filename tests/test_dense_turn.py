"""The short way of the memoising 16-bit dense pass (option dense_memo = 2) by TURNS: one packed word per lane decides a whole turn
of T trips (csrc/vrg_rim.h, "one count per TURN"), and the table sums of the trips that take the short way are added one per lane and
trip (lane 4 q + j: sum j of slot q) instead of lane by lane into one serial accumulator.

The CPU tests run the header's turn arithmetic in a host program against the per-trip test that stays in the header, for 2, 3 and 4
trips per turn, restate the lane-parallel sum in numpy, and read the kernels' resource records.  The GPU tests walk lists that end
at and around a turn of four waves and a recipe whose failing trips fall at every position of a turn, and compare the product with
dense_memo = 0 byte for byte and with the oracle; every recipe is first walked in numpy on the oracle's labels (walk_turns)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_dense_rim_memo import check_stats, flat_index, idx_px, oracle_labels
from test_dense_memo import check_sums, sum_bound
from test_dense_unit_memo import compare_with_memo_0_and_oracle, listed_units, run, unit_matches

CSRC = os.path.join(ROOT, 'arterynetwork_amd', 'csrc')
# the trips of a turn the product is built with (csrc/vrg_device.hip, RIM_TRIPS)
T = int(re.search(r'^#define VRG_RIM_TRIPS (\d+)', open(os.path.join(CSRC, 'vrg_device.hip')).read(), re.M).group(1))


@pytest.fixture(scope='module')
def lib():
    from arterynetwork_amd._capi import product_lib
    return product_lib()


# ---- the arithmetic, on the host ------------------------------------------------------------------------------------------------
TURN_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "vrg_rim.h"
// A turn of the walk's short way: TRIPS trips of three units of 64 class words, the four counts of init per unit.  The wave's
// cross-lane steps are 32-bit additions of the lanes' words over all 64 lanes.
template <int TRIPS> struct Turn { uint32_t w[TRIPS][3][64]; uint32_t ic[TRIPS][3][4]; };
static uint32_t count_word(const uint32_t ic[3][4], uint32_t l) {       // the word of init's counts lane l fetches: word l & 1 of slot min(l / 4, 2)
    const uint32_t q = (l >> 2) < 2 ? (l >> 2) : 2;
    return ic[q][2 * (l & 1)] | ic[q][2 * (l & 1) + 1] << 16;
}
template <int TRIPS> static bool trip_short(const Turn<TRIPS>& t, int k) {           // the per-trip test, as the walk makes it for a trip alone
    uint32_t t01 = 0, t2i = 0;
    for (uint32_t l = 0; l < 64; l++) {
        const uint32_t share = vrg_unit_share(count_word(t.ic[k], l));
        t01 += vrg_unit_word01(t.w[k][0][l], t.w[k][1][l], share, vrg_unit_role01(l));
        t2i += vrg_unit_word2i(t.w[k][0][l], t.w[k][1][l], t.w[k][2][l], share, vrg_unit_role2i(l));
    }
    return vrg_unit_short(t01, t2i);
}
template <int TRIPS> static bool turn_short(const Turn<TRIPS>& t) {
    static_assert(3 * TRIPS <= VRG_TURN_MAX_UNITS, "units per turn");
    uint32_t total = 0;
    for (uint32_t l = 0; l < 64; l++) {
        uint32_t outer = 0, orw = 0, shares = 0;
        for (int k = 0; k < TRIPS; k++) {
            for (int q = 0; q < 3; q++) { outer += vrg_unit_outer(t.w[k][q][l]); orw |= t.w[k][q][l]; }
            shares += vrg_unit_share(count_word(t.ic[k], l));
        }
        total += vrg_turn_word(outer, orw, shares, vrg_turn_mask(l));
    }
    return vrg_turn_short(total);
}
static int bad = 0;
// the turn word passes iff every trip passes; want: 1 / 0 = what the case was built to give, -1 = whatever the trips say
template <int TRIPS> static bool expect(const Turn<TRIPS>& t, const char* what, int want = -1) {
    bool trips = true;
    for (int k = 0; k < TRIPS; k++) trips = trips && trip_short(t, k);
    const bool got = turn_short(t);
    if (got != trips) { std::printf("FAIL %s (%d trips): turn %d, its trips %d\n", what, TRIPS, (int)got, (int)trips); bad++; }
    if (want >= 0 && (int)got != want) { std::printf("FAIL %s (%d trips): turn %d, built to give %d\n", what, TRIPS, (int)got, want); bad++; }
    return got;
}
static uint32_t popcounts(const uint32_t* w, uint32_t mask) { uint32_t n = 0; for (int l = 0; l < 64; l++) n += __builtin_popcount(w[l] & mask); return n; }
static void set_outer(uint32_t* w, uint32_t voxel) { w[(voxel & 255u) >> 2] |= 2u << (8 * (voxel >> 8) + 2 * (voxel & 3u)); }      // voxel 0..1023 of the unit: group voxel >> 8, lane (voxel & 255) >> 2
static void set_inner(uint32_t* w, uint32_t voxel) { const uint32_t s = 8 * (voxel >> 8) + 2 * (voxel & 3u); uint32_t& x = w[(voxel & 255u) >> 2]; x = (x & ~(3u << s)) | 1u << s; }
static bool is_outer(const uint32_t* w, uint32_t voxel) { return (w[(voxel & 255u) >> 2] >> (8 * (voxel >> 8) + 2 * (voxel & 3u))) & 2u; }
static void fill(uint32_t* w, uint32_t* ic, uint32_t n) {                 // n outer voxels, and init's counts to match
    for (int l = 0; l < 64; l++) w[l] = 0;
    for (uint32_t v = 0; v < n; v++) set_outer(w, (v * 613u) % 1024u);               // (613 is odd: n distinct voxels)
    for (int j = 0; j < 4; j++) ic[j] = popcounts(w, 0xAAu << (8 * j));
}
static uint32_t free_voxel(const uint32_t* w, uint32_t lane) {            // a voxel of the lane that is not outer
    for (uint32_t j = 0; j < 4; j++) for (uint32_t b = 0; b < 4; b++) { const uint32_t v = 256u * j + 4u * lane + b; if (!is_outer(w, v)) return v; }
    return 1024u;
}
static uint32_t outer_voxel(const uint32_t* w, uint32_t lane) {
    for (uint32_t j = 0; j < 4; j++) for (uint32_t b = 0; b < 4; b++) { const uint32_t v = 256u * j + 4u * lane + b; if (is_outer(w, v)) return v; }
    return 1024u;
}
template <int TRIPS> static void cases() {
    static Turn<TRIPS> t;
    const int U = 3 * TRIPS;
    auto W = [&](int u) { return t.w[u / 3][u % 3]; };
    auto IC = [&](int u) { return t.ic[u / 3][u % 3]; };
    // every unit full (1024 outer voxels in every slot) or empty, every pattern of the turn's units: no carry between the fields
    for (uint32_t pat = 0; pat < (1u << U); pat++) {
        for (int u = 0; u < U; u++) fill(W(u), IC(u), (pat >> u) & 1u ? 1024u : 0u);
        expect(t, "full and empty units", 1);
    }
    // ... and a full turn against counts of init one below in one unit (1023 of 1024), and one above
    for (int u = 0; u < U; u++) for (int j = 0; j < 4; j++) for (int d : {-1, 1}) {
        for (int v = 0; v < U; v++) fill(W(v), IC(v), v % 2 ? 1024u : 700u);
        IC(u)[j] += d;
        expect(t, "a count of init one off", 0);
    }
    // one surplus voxel, included after init, in the first and in the last unit of the turn
    for (int u : {0, U - 1}) for (uint32_t lane : {0u, 17u, 63u}) {
        for (int v = 0; v < U; v++) fill(W(v), IC(v), 700);
        expect(t, "as at init", 1);
        set_outer(W(u), free_voxel(W(u), lane));
        expect(t, "one surplus voxel", 0);
    }
    // the cancellation: one unit with an included voxel turned inner (one outer voxel fewer than init counted) beside a unit with one
    // newly included voxel - the outer totals of the turn are those of init, the inner field alone says no.  Same trip and other trips.
    for (int a = 0; a < U; a++) for (int b = 0; b < U; b++) if (a != b) {
        for (int v = 0; v < U; v++) fill(W(v), IC(v), 700);
        set_inner(W(a), outer_voxel(W(a), 5));
        set_outer(W(b), free_voxel(W(b), 40));
        uint32_t no = 0, ni = 0;
        for (int v = 0; v < U; v++) { no += popcounts(W(v), 0xAAAAAAAAu); for (int j = 0; j < 4; j++) ni += IC(v)[j]; }
        if (no != ni) { std::printf("FAIL the cancellation case does not cancel\n"); bad++; }
        expect(t, "deficit beside surplus", 0);
    }
    // inner voxels in lane 0 or in lane 63 only, in any unit of the turn (an inner voxel is an included one: init counted it)
    for (int u = 0; u < U; u++) for (uint32_t lane : {0u, 63u}) {
        for (int v = 0; v < U; v++) fill(W(v), IC(v), 1024);
        set_inner(W(u), 256u * (u & 3) + 4u * lane + (lane & 3u));
        expect(t, "an inner voxel in lane 0 or 63", 0);
        for (int v = 0; v < U; v++) fill(W(v), IC(v), 0);                                   // ... in a turn that holds nothing else
        set_inner(W(u), 4u * lane);
        IC(u)[0] = 1;
        expect(t, "an inner voxel alone", 0);
    }
    // random turns by the monotone rule: init's included set, later inclusions, inner voxels among the included
    std::srand(17 + TRIPS);
    int shorts = 0;
    const int N = 24000;
    for (int n = 0; n < N; n++) {
        std::memset(&t, 0, sizeof t);
        const int quiet = std::rand() % 2;                              // (half of the turns: nothing happened since init in most units)
        for (int u = 0; u < U; u++) {
            const int dens = std::rand() % 5, later = std::rand() % (quiet ? 5 * U : 4) == 0, inner = std::rand() % (quiet ? 6 * U : 6) == 0;
            for (uint32_t v = 0; v < 1024; v++) {
                const bool empty_group = dens == 4 && (v >> 8) == (uint32_t)(n & 3);
                const bool at_init = !empty_group && (dens == 3 || std::rand() % 4 <= dens);
                if (at_init) IC(u)[v >> 8]++;
                if (at_init || (later && std::rand() % 300 == 0)) { if (inner && std::rand() % 500 == 0) set_inner(W(u), v); else set_outer(W(u), v); }
            }
        }
        shorts += expect(t, "random");
    }
    std::printf("%d trips per turn: %d of %d random turns take the short way\n", TRIPS, shorts, N);
    if (shorts < N / 10 || shorts > N - N / 10) { std::printf("FAIL the random turns do not exercise both ways\n"); bad++; }
}
int main() {
    cases<2>();
    cases<3>();
    cases<4>();
    std::printf("%s\n", bad ? "BAD" : "OK");
    return bad != 0;
}
'''


def test_turn_word_equals_the_trips_decisions(tmp_path):
    """No GPU needed.  csrc/vrg_rim.h compiled alone for the host: over the 64 lanes' words added with plain 32-bit additions, the turn
    word passes iff every trip of the turn passes the per-trip test (vrg_unit_short), for 2, 3 and 4 trips per turn: every pattern of full
    (1024 outer voxels) and empty units, counts of init one off, one surplus voxel in the first and the last unit, a deficit beside a
    surplus (must fail), an inner voxel in lane 0 or 63 only, and 24 000 random turns built by the monotone rule per width."""
    cxx = os.environ.get('CXX', 'g++')
    src, exe = tmp_path / 'turn.cpp', tmp_path / 'turn'
    src.write_text(TURN_PROGRAM)
    p = subprocess.run([cxx, '-O1', '-std=c++17', '-I', CSRC, '-o', str(exe), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:]


def test_lane_parallel_sum_within_the_reordering_bound():
    """No GPU needed.  One wave's table sums restated in numpy: lane 4 q + j adds sum j of slot q trip by trip, lanes 0..11 join the
    wave's butterfly (wave_sum: xor 32, 16, .., 1), the lanes above add nothing.  Against math.fsum within 2 n 2^-53 sum |x|, on values
    that are no dyadic fractions; a second evaluation is identical."""
    rng = np.random.default_rng(3)
    for trips in (1, 2, 7, 29, 200):
        g = rng.integers(0, 256 * 400, size=(trips, 12)) / 397.0          # (sums of up to 256 values k / 397)

        def wave(g):
            lane = np.zeros(64)
            for k in range(len(g)):
                lane[:12] += g[k]
            o = 32
            while o:
                lane = lane + lane[np.arange(64) ^ o]
                o >>= 1
            return lane[0]
        got, x = wave(g), g.ravel()
        assert abs(got - math.fsum(x)) <= sum_bound(x), (trips, got, math.fsum(x))
        assert wave(g) == got


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_turn_walk_resources(tmp_path):
    """No GPU needed: the four instantiations k_recount_bits<3, NT, MODE 1 and 3, true, true, true> with the window of T trips spill no
    scalar register, use no scratch and at most 128 VGPRs (seven per trip of the window and one for the entry behind it)."""
    from arterynetwork_amd import build
    out = tmp_path / 'vrg_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vrg_device.hip'], cwd=CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    found = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):
        k = re.search(r'14k_recount_bitsILi3ELb([01])ELi([13])ELb1ELb1ELb1EE', m.group(1))
        if k:
            f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
            found[k.groups()] = (f('sgpr_spill_count'), f('private_segment_fixed_size'), f('vgpr_count'))
    assert len(found) == 4, sorted(found)
    for key, (spills, scratch, vgpr) in sorted(found.items()):
        print('%d trips per turn, k_recount_bits<3,NT=%s,MODE=%s,true,true,true>: %d SGPR spills, %d B scratch, %d VGPRs' % ((T,) + key + (spills, scratch, vgpr)))
        assert spills == 0 and scratch == 0 and vgpr <= 128, (key, spills, scratch, vgpr)


# ---- the walk by turns, restated on labels -------------------------------------------------------------------------------------------
def walk_turns(lab0, lab, blocks=1, trips=T):
    """The walk restated on labels.  The list's consecutive triples are the trips; a trip passes iff it is whole and its three units
    match (unit_matches).  Wave w of 4 * blocks starts at list position 3 w and steps by 12 * blocks units per trip; it takes `trips`
    trips in one turn while all of them are whole and pass, otherwise one trip alone.
    Returns {'turns', 'alone_short', 'per_group', 'failed_at': the positions in a whole turn of the first trip that failed it,
    'in_turn': the units that went through a turn}."""
    ok, units = unit_matches(lab0, lab), listed_units(lab)
    n, step = len(units), 12 * blocks
    way = [bool(k + 3 <= n and ok[units[k:k + 3]].all()) for k in range(0, n, 3)]
    out = {'turns': 0, 'alone_short': 0, 'per_group': 0, 'failed_at': set(), 'in_turn': set()}
    for w in range(4 * blocks):
        i = 3 * w
        while i < n:
            if i + (trips - 1) * step + 3 <= n:
                ways = [way[(i + k * step) // 3] for k in range(trips)]
                if all(ways):
                    out['turns'] += 1
                    for k in range(trips):
                        out['in_turn'].update(int(u) for u in units[i + k * step:i + k * step + 3])
                    i += trips * step
                    continue
                out['failed_at'].add(ways.index(False))
            if way[i // 3]:
                out['alone_short'] += 1
            else:
                out['per_group'] += 1
            i += step
    return out


def walks(labs, what):
    out = [walk_turns(labs[0], lab) for lab in labs]
    print('%s, %d trips per turn: (turns, trips alone on the short way, per group, failed at) per pass %s'
          % (what, T, [(o['turns'], o['alone_short'], o['per_group'], sorted(o['failed_at'])) for o in out]))
    return out


def ragged_turn_case(n):
    """tests/test_dense_unit_memo.py's ragged_case for any n >= 12: rows of 1104 padded voxels, three rows per plane, everything
    excluded but the voxels of exactly n units - the units around the seeds first, then the others in ascending order -, a third of the
    voxels of every odd group excluded as well.  Returns (data, valueMap)."""
    ny, nz = 3, n // 4 + 2                                   # (7728 voxels per plane: four units or more with real voxels)
    shape = (1102, ny, nz)
    rng = np.random.default_rng(2000 + n)
    idx = flat_index(shape)
    unit = idx >> 10
    plane = (ny + 4) * idx_px(1102)
    ids = np.unique(unit)
    ids = ids[(ids >= (2 * plane + 1023) >> 10) & (ids < ((2 + nz) * plane) >> 10)]
    assert len(ids) >= n, (len(ids), n)
    zc, yc, x0 = nz // 2, ny // 2, 500
    near = np.unique(unit[x0 - 2:x0 + 8, :, max(zc - 1, 0):zc + 2])
    assert len(near) <= n
    keep = (list(near) + [u for u in ids if u not in set(near)])[:n]
    vm = np.full(shape, 4, dtype=np.int64)
    vm[np.isin(unit, keep)] = 3
    vm[(((idx >> 8) & 1) == 1) & (idx % 3 == 0)] = 4
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    tube = np.zeros(shape, dtype=bool)
    tube[x0:x0 + 6, :, zc] = True                        # (one plane: the region stays in the units of its rows)
    tube &= np.isin(unit, keep)
    data[tube] = rng.integers(4, 7, size=int(tube.sum()))
    vm[tube] = 3
    vm[x0 + 2:x0 + 4, yc, zc] = 0
    return data, vm


# one turn of four waves covers 12 T units: one unit short of it, exactly one turn, one turn plus a partial trip, plus one whole trip
# alone, two turns, two turns and a trip per wave, three turns and a list that ends inside a window already requested
RAGGED = [12 * T - 1, 12 * T, 12 * T + 1, 12 * T + 3, 24 * T, 24 * T + 12, 36 * T + 5]
SWEEPS = 5


@pytest.mark.parametrize('n', RAGGED)
def test_ragged_turn_cases_list_n_units_and_turn(n):
    """No GPU needed: the recipe lists exactly n units in every pass; walked on the oracle's labels, every list turns in the pass at init
    - the list of 12 T - 1 units in fewer than four waves, the last wave's trips going alone -; from 24 T units on in every pass."""
    data, vm = ragged_turn_case(n)
    assert len(listed_units(vm)) == n
    labs = oracle_labels(data, vm, SWEEPS, 'turn-ragged-%d' % n)
    assert len(labs) >= 3
    for lab in labs:
        assert len(listed_units(lab)) == n
    w = walks(labs, 'n %d' % n)
    assert w[0]['turns'] > 0
    if n < 12 * T:                                         # (the last wave's turn is not whole: its trips go alone)
        assert all(o['turns'] < 4 for o in w) and w[0]['alone_short'] >= T - 1
    if n >= 24 * T:
        assert all(o['turns'] > 0 for o in w)


@pytest.mark.gpu
@pytest.mark.parametrize('n', RAGGED)
def test_ragged_turn_lists(lib, n):
    """Lists of 12 T - 1, 12 T, 12 T + 1, 12 T + 3, 24 T, 24 T + 12 and 36 T + 5 units walked by four waves.  Integer values: labels and
    the whole trace byte-identical with dense_memo = 0 on the same grid, stepwise parity with the oracle, the statistics equal the
    restatement, the sums those of the labels."""
    data, vm = ragged_turn_case(n)
    a = compare_with_memo_0_and_oracle(lib, data, vm, SWEEPS, 1, 'n %d' % n)
    assert a[4]['dense_listed_units'] == n and a[3]['dense_listed_units'] == n
    labs = oracle_labels(data, vm, SWEEPS, 'turn-ragged-%d' % n)
    assert np.array_equal(a[5], labs[0]) and np.array_equal(a[0], labs[-1])
    _, rim0 = check_stats(a[4], a[5], a[5], 'init, n %d' % n)
    check_stats(a[3], a[5], a[0], 'end, n %d' % n)
    assert rim0 > 0 and a[3]['dense_rim_groups'] > 0
    lab, tr, r = a[:3]
    check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'n %d' % n)


POSITION_SWEEPS = 8


def position_case():
    """254 x 5 x nz (rows of 256 padded voxels: a group is a row, a unit four rows), every voxel included, 36 T + 12 listed units or
    more.  Wave w's first turn holds the trips at list positions 3 w + 12 k, k < T.  For p < T a tube of one row, 60 voxels long and
    seeded in its middle, lies in the trip at position p of wave p's first turn: the region grows there through all sweeps and fails
    that turn at position p.  In the trips at the same positions of the waves' SECOND turns lie isolated seeds in the noise, which flip
    out again: those turns fail in the first passes and take the short way later.  Integer values 0..3, the tubes 4..6."""
    nz = 18 * T + 10                                            # (two listed units per plane or more)
    shape = (254, 5, nz)
    rng = np.random.default_rng(31)
    vm = np.full(shape, 3, dtype=np.int64)
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    units = listed_units(vm)                                    # (the units that hold a real voxel: the rows of padding fill some)

    def row_of_trip(pos):
        """a real row (y, z) inside the trip at list positions pos .. pos + 2"""
        for u in units[pos:pos + 3]:
            for r in range(4 * u, 4 * u + 4):
                if 2 <= r % 9 <= 6 and 2 <= r // 9 < 2 + nz:
                    return r % 9 - 2, r // 9 - 2
        raise AssertionError(pos)
    tubes = np.zeros(shape, dtype=bool)
    for p in range(T):
        y, z = row_of_trip(3 * (p % 4) + 12 * p)
        tubes[100:160, y, z] = True
        vm[128:130, y, z] = 0
        y, z = row_of_trip(3 * (p % 4) + 12 * p + 12 * T)
        vm[60 + 30 * p, y, z] = 0
    data[tubes] = rng.integers(4, 7, size=int(tubes.sum()))
    return data, vm


def check_position_case(labs):
    """the failing trip falls at each of the T positions of a turn; units whose turn failed in one pass go through a turn in a later
    one; the loop turns in every pass"""
    w = walks(labs, 'positions')
    seen = set().union(*[o['failed_at'] for o in w])
    assert seen >= set(range(T)), seen
    assert all(o['turns'] > 0 for o in w) and all(o['per_group'] > 0 for o in w)
    oks = [unit_matches(labs[0], lab) for lab in labs]
    back = set(u for o in w[1:] for u in o['in_turn'] if not oks[0][u])
    print('units that fail their trip at init and go through a turn in a later pass:', sorted(back))
    assert back


def test_position_case_fails_at_every_position():
    """No GPU needed: the recipe walked on the oracle's labels (check_position_case)."""
    data, vm = position_case()
    assert len(listed_units(vm)) >= 36 * T + 12
    labs = oracle_labels(data, vm, POSITION_SWEEPS, 'turn-positions')
    assert len(labs) == POSITION_SWEEPS + 1
    check_position_case(labs)


@pytest.mark.gpu
def test_failing_trip_at_every_position_of_a_turn(lib):
    """The recipe on the GPU, four waves: byte-identical with dense_memo = 0, stepwise parity with the oracle, the labels at init and
    at the end the oracle's (so the run holds the turns the CPU test found), the statistics equal the restatement."""
    data, vm = position_case()
    a = compare_with_memo_0_and_oracle(lib, data, vm, POSITION_SWEEPS, 1, 'positions')
    labs = oracle_labels(data, vm, POSITION_SWEEPS, 'turn-positions')
    assert a[2].sweeps == POSITION_SWEEPS
    assert np.array_equal(a[5], labs[0]) and np.array_equal(a[0], labs[-1])
    check_position_case(labs)
    check_stats(a[4], a[5], a[5], 'init')
    check_stats(a[3], a[5], a[0], 'end')
    lab, tr, r = a[:3]
    check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'positions')


def fraction_position_case():
    """position_case's labels on values that are no dyadic fractions: integers below 400 over 397.0, the tubes 3.0 above the noise"""
    d0, vm = position_case()
    rng = np.random.default_rng(7)
    data = rng.integers(0, 400, size=d0.shape) / 397.0
    data[d0 >= 4] += 3.0
    return data.astype(np.float32), vm


def test_fraction_position_case_turns():
    """No GPU needed: on the oracle's labels the loop turns in every pass of the non-dyadic case."""
    data, vm = fraction_position_case()
    labs = oracle_labels(data.astype(np.float64), vm, POSITION_SWEEPS, 'turn-fraction')
    assert len(labs) == POSITION_SWEEPS + 1
    assert all(o['turns'] > 0 for o in walks(labs, 'non-dyadic'))


@pytest.mark.gpu
def test_non_dyadic_values_by_turns(lib):
    """Non-dyadic values added lane-parallel in every pass (four waves, the table of doubles): the counts identical with dense_memo = 0,
    each sum within the reordering bound of math.fsum, two runs byte-identical, the labels the oracle's."""
    data, vm = fraction_position_case()
    a, b = run(lib, data, vm, POSITION_SWEEPS, 2, 1), run(lib, data, vm, POSITION_SWEEPS, 0, 1)
    assert ',3,' in a[3]['dense_kernel'], a[3]['dense_kernel']
    assert a[3]['dense_workgroups'] == b[3]['dense_workgroups'] == 1
    assert a[2].sweeps == b[2].sweeps == POSITION_SWEEPS
    for f in ('nflip', 'nseg', 'n_in', 'n_out', 'ni', 'no'):
        assert np.array_equal(a[1][f], b[1][f]), f
    assert np.array_equal(a[0], b[0])
    labs = oracle_labels(data.astype(np.float64), vm, POSITION_SWEEPS, 'turn-fraction')
    assert np.array_equal(a[5], labs[0]) and np.array_equal(a[0], labs[-1])
    for memo, o in ((2, a), (0, b)):
        lab, tr, r = o[:3]
        check_sums(data, lab, r.n_in, r.n_out, r.sum_in, r.sum_out, 'non-dyadic, memo %d' % memo)
        assert (tr['sum_in'][-1], tr['sum_out'][-1]) == (r.sum_in, r.sum_out)
    check_stats(a[3], a[5], a[0], 'non-dyadic')
    again = run(lib, data, vm, POSITION_SWEEPS, 2, 1)
    assert again[1].tobytes() == a[1].tobytes() and np.array_equal(again[0], a[0])
