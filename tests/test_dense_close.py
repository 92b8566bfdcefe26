"""Option dense_close: a gated dense pass leaves its workgroups' slots unsummed and the next kernel on the dense stream closes it - the
gate of the next pass, or k_dense_close where the host looks first (csrc/vrg_device.hip).  The closer adds the slots in the order the
pass's own last workgroup adds them (dense_close = 0: the ticket and the in-kernel close), so everything a run files must be the same
BIT FOR BIT with the option at 1 and at 0, on inexact data too: labels, the order of the segmented list and the whole trace as raw bytes
- sum_in / sum_out as 64-bit words, the NaNs of passes that were left out included.

Every case runs the same plan on two fresh handles that differ in the option only; one case per group is also advanced sweep by sweep
against the oracle (parity.run_stepwise, the suite's tolerances)."""
import numpy as np
import pytest

import parity
from arterynetwork_amd import phantoms
from test_dense_rim_memo import flat_index, idx_px
from test_dense_turn import T, ragged_turn_case
from test_dense_unit_memo import listed_units


@pytest.fixture(scope='module')
def lib():
    from arterynetwork_amd._capi import product_lib
    return product_lib()


# ---- volumes (built once, never changed) ------------------------------------------------------------------------------------------------
_cache = {}


def volume(kind):
    """'noise32': a tube in continuous float32 noise (every value its own level); 'f64': the same tube on values k / 397 + noise that no
    float32 holds (the volume stays float64); 'levels': 16 integer levels (16-bit storage); 'sphere': the salted sphere, which converges
    in a few sweeps.  -> (data, labels as uint8)"""
    if kind not in _cache:
        if kind == 'sphere':
            data, vm = phantoms.sphere_salt()
            data = np.asarray(data, dtype=np.float64)
        else:
            data, vm = phantoms.tube_phantom(shape=(48, 40, 24), radius=3.0, seed=5, seed_planes=3, amp_y=8.0, amp_z=4.0,
                                             levels=16 if kind == 'levels' else None, brain_mask=True)
            if kind == 'noise32':
                data = data.astype(np.float32)
                assert len(np.unique(data)) > 10000
            elif kind == 'f64':
                rng = np.random.default_rng(11)
                data = np.round(data * 40.0) / 397.0 + rng.integers(0, 1000, size=data.shape) / 3970003.0
                assert not np.array_equal(data.astype(np.float32).astype(np.float64), data)
        _cache[kind] = (data, np.asarray(vm).astype(np.uint8))
    return _cache[kind]


def edge_volume(whole_unit):
    """One plane of rows of 64 padded voxels, so that no excluded voxel next to the band lies in another plane's unit.
    60 x 11 x 1: the slab [1920, 2880) holds no whole unit - the list is EMPTY for the whole run, the first and the last wave count the
    two units the slab's faces cut.  60 x 28 x 1: the slab [4096, 6144) is units 4 and 5; everything from y = 12 on is excluded and the
    region stays below y = 9: a list of ONE unit for the whole run.  Integer noise, a blob of higher values around two seeds."""
    shape = (60, 28, 1) if whole_unit else (60, 11, 1)
    assert idx_px(60) == 64
    rng = np.random.default_rng(5 + whole_unit)
    vm = np.full(shape, 3, dtype=np.uint8)
    vm[:, 12:, :] = 4
    data = rng.integers(0, 4, size=shape).astype(np.float64)
    data[20:40, 4:7, 0] = rng.integers(4, 7, size=(20, 3))
    vm[29:31, 5, 0] = 0
    assert len(listed_units(vm)) == (1 if whole_unit else 0)
    return data, vm


# ---- running a plan with the option at 1 and at 0 -----------------------------------------------------------------------------------------
def snapshot(s, r):
    return {'labels': s.labels(), 'seg': s.segmented(), 'trace': s.trace(), 'sweeps': int(r.sweeps), 'stop': int(r.stop_reason),
            'sums': (np.float64(r.sum_in).tobytes(), np.float64(r.sum_out).tobytes()), 'sizes': (int(r.n_in), int(r.n_out))}


def run_plan(lib, data, vm, options, plan, close, prepare=None):
    from arterynetwork_amd._capi import Session
    s = Session(data.shape, lib=lib)
    try:
        for k, v in options.items():
            s.set_option(k, v)
        s.set_option('dense_close', close)
        if prepare:
            prepare(s)
        s.set_volume(data); s.set_labels(vm); s.init(2.25)
        listed0 = s.stats()['dense_listed_units']
        return plan(s), dict(s.stats(), listed_at_init=listed0)
    finally:
        s.close()


def same(a, b, what):
    assert a['sweeps'] == b['sweeps'] and a['stop'] == b['stop'] and a['sizes'] == b['sizes'], what
    assert np.array_equal(a['labels'], b['labels']), what
    assert np.array_equal(a['seg'], b['seg']), what + ': segmented order'
    assert a['trace'].tobytes() == b['trace'].tobytes(), what + ': trace bytes'
    assert a['sums'] == b['sums'], what


def both(lib, data, vm, options, plan, what, prepare=None):
    """the plan on a fresh handle with dense_close = 1 and on one with 0: every snapshot the same; -> (snapshots, stats) of the option at 1"""
    a, sa = run_plan(lib, data, vm, options, plan, 1, prepare)
    b, sb = run_plan(lib, data, vm, options, plan, 0, prepare)
    assert len(a) == len(b) > 0
    for j, (x, y) in enumerate(zip(a, b)):
        same(x, y, '%s, snapshot %d' % (what, j))
    assert sa['dense_kernel'] == sb['dense_kernel'] and sa['dense_workgroups'] == sb['dense_workgroups'], what
    return a, sa


def one_run(n):
    def plan(s):
        return [snapshot(s, s.run(n, 10 ** 9, None))]
    return plan


def has_sums(tr, first=1):
    return not np.isnan(tr['sum_in'][first:]).any() and not np.isnan(tr['sum_out'][first:]).any()


# ---- the slot count at the edges of the closer's loop (TPB = 256 slots per turn) -----------------------------------------------------------
BLOCKS = [1, 5, 255, 256, 257, 300]
SLOT_SWEEPS = 5


@pytest.mark.gpu
@pytest.mark.parametrize('blocks', BLOCKS)
def test_slot_counts_fp32_and_f64(lib, blocks):
    """k_recount_pipe (fp32 storage, continuous noise) and the float64 pass on `blocks` workgroups: one slot, a few, one short of a turn of
    the closer's loop, exactly one, one more, and a second turn well begun."""
    for kind, kernel, storage in (('noise32', 'k_recount_pipe', 'fp32'), ('f64', 'k_recount_bits<2', 'float64')):
        data, vm = volume(kind)
        a, st = both(lib, data, vm, {'sweep_blocks': blocks}, one_run(SLOT_SWEEPS), '%s, %d workgroups' % (kind, blocks))
        assert st['dense_workgroups'] == blocks and st['dense_kernel'].startswith(kernel) and st['dense_storage'].startswith(storage), st
        assert a[0]['sweeps'] == SLOT_SWEEPS and has_sums(a[0]['trace'])


@pytest.mark.gpu
@pytest.mark.parametrize('blocks', BLOCKS)
def test_slot_counts_16_bit(lib, blocks):
    """16-bit storage on `blocks` workgroups: the plain walk (dense_memo = 0) and the rim walk (2) over the ragged list of 12 T + 1 units."""
    data, vm = ragged_turn_case(12 * T + 1)
    vm = vm.astype(np.uint8)
    for memo in (0, 2):
        a, st = both(lib, data, vm, {'storage16': 1, 'dense_memo': memo, 'sweep_blocks': blocks}, one_run(SLOT_SWEEPS), 'memo %d, %d workgroups' % (memo, blocks))
        assert st['dense_workgroups'] == blocks and st['dense_storage'].startswith('u16') and st['dense_listed_units'] == 12 * T + 1, st
        assert a[0]['sweeps'] >= 2 and has_sums(a[0]['trace'])         # (the recipe's region stops growing after a few sweeps)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,options', [('noise32', {'sweep_blocks': 257}), ('f64', {'sweep_blocks': 257}),
                                          ('levels', {'storage16': 1, 'dense_memo': 0, 'sweep_blocks': 257})])
def test_slot_counts_against_the_oracle(lib, kind, options):
    """one case of each storage, 257 workgroups (a turn of the closer's loop and one slot), sweep by sweep against the oracle"""
    data, vm = volume(kind)
    res, k = parity.run_stepwise(lib, data.astype(np.float64), vm, 2.25, None, 6, density_mode=1, options=dict(options, dense_close=1))
    assert res is not None and k == 6, (res, k)


@pytest.mark.gpu
def test_rim_walk_against_the_oracle(lib):
    data, vm = ragged_turn_case(12 * T + 1)
    res, k = parity.run_stepwise(lib, data, vm.astype(np.uint8), 2.25, None, SLOT_SWEEPS, density_mode=1, check_hist=True,
                                 options={'storage16': 1, 'dense_memo': 2, 'sweep_blocks': 257, 'dense_close': 1})
    assert res is not None and k > 0


# ---- who closes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('batch', [1, 2, 64])
@pytest.mark.parametrize('sweeps', [1, 2, 9])
def test_who_closes(lib, sweeps, batch):
    """One sweep: only k_dense_close ever closes; two: a gate and k_dense_close; nine: gates, and k_dense_close at the end of every batch.
    Every sweep's record carries its sums.  A second run on the same handle goes on; set_labels + init + run equals a fresh handle."""
    data, vm = volume('noise32')

    def plan(s):
        out = [snapshot(s, s.run(sweeps, 10 ** 9, None))]
        out.append(snapshot(s, s.run(2 * sweeps, 10 ** 9, None)))
        s.set_labels(vm); s.init(2.25)
        out.append(snapshot(s, s.run(sweeps, 10 ** 9, None)))
        return out
    a, _ = both(lib, data, vm, {'batch': batch}, plan, '%d sweeps, batch %d' % (sweeps, batch))
    assert a[0]['sweeps'] == sweeps and a[1]['sweeps'] == sweeps and len(a[1]['trace']) == 2 * sweeps + 1
    for x in a:
        assert has_sums(x['trace']), x['trace']['sum_in']
    assert a[1]['trace'][:sweeps + 1].tobytes() == a[0]['trace'].tobytes()
    same(a[2], a[0], 'after set_labels + init')


@pytest.mark.gpu
def test_who_closes_against_the_oracle(lib):
    data, vm = volume('noise32')
    res, k = parity.run_batched(lib, data.astype(np.float64), vm, 2.25, None, 9, density_mode=1, options={'batch': 2, 'dense_close': 1})
    assert res is not None and k == 9, (res, k)


# ---- passes left out ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('every', [0, 2, 3])
def test_passes_left_out(lib, every):
    """verify_every: markers and closes interleave - a gate closes the pass before it and then files the marker of its own sweep -, and
    the run's last sweep is counted after all (verify-last).  Sums where a pass ran, NaN where none did."""
    data, vm = volume('noise32')
    a, _ = both(lib, data, vm, {'verify_every': every, 'batch': 4}, one_run(9), 'verify_every %d' % every)
    tr = a[0]['trace']
    assert a[0]['sweeps'] == 9 and len(tr) == 10
    counted = [k for k in range(1, 10) if (every and k % every == 0) or k == 9]
    assert [k for k in range(1, 10) if not np.isnan(tr['sum_in'][k])] == counted, tr['sum_in']


@pytest.mark.gpu
def test_passes_left_out_against_the_oracle(lib):
    data, vm = volume('noise32')
    s_all, _ = run_plan(lib, data, vm, {}, one_run(9), 1)
    s_3, _ = run_plan(lib, data, vm, {'verify_every': 3}, one_run(9), 1)
    assert np.array_equal(s_all[0]['labels'], s_3[0]['labels'])
    for k in (3, 6, 9):                                  # (the passes that ran filed the sums every pass files)
        assert s_3[0]['trace'][k].tobytes() == s_all[0]['trace'][k].tobytes(), k
    res, k = parity.run_batched(lib, data.astype(np.float64), vm, 2.25, None, 9, density_mode=1, options={'dense_close': 1})
    assert res is not None and k == 9


# ---- a run that stops inside a batch ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_run_stops_inside_a_batch(lib):
    """The salted sphere converges in fewer sweeps than the batch of 64 holds: the gates and passes enqueued behind the stop run out on the
    stop word, the last counted sweep has its sums, no error is raised (run would raise)."""
    data, vm = volume('sphere')
    a, _ = both(lib, data, vm, {'batch': 64}, one_run(200), 'sphere, batch 64')
    assert a[0]['stop'] == 1 and 0 < a[0]['sweeps'] < 63, (a[0]['stop'], a[0]['sweeps'])
    assert len(a[0]['trace']) == a[0]['sweeps'] + 1 and has_sums(a[0]['trace'])
    res, k = parity.run_batched(lib, data, vm, 2.25, None, 200, density_mode=1, options={'batch': 64, 'dense_close': 1})
    assert res is None or k == a[0]['sweeps']


# ---- trips handed back --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('options', [{'fused': 0, 'small_flips': 6, 'batch': 8}, {'fused': 0, 'small_flips': 0, 'batch': 8},
                                     {'fused': 0, 'small_flips': 20, 'batch': 5}, {'fused': 0, 'batch': 8}])
def test_trips_handed_back(lib, options):
    """No fused sweeps and a lowered limit of the four-launch chain, as tests/test_gpu_parity.py lowers it: trips come back to the host
    (be_sync with the stop word set, an open pass behind the gates that run out) and host-driven trips take over; the last case runs the
    four-launch trips alone."""
    data, vm = volume('noise32')
    a, st = both(lib, data, vm, options, one_run(12), str(options))
    assert a[0]['sweeps'] == 12 and has_sums(a[0]['trace'])
    assert st['fused_trips'] == 0, st
    if 'small_flips' in options:
        assert st['bail_flips'] + st['host_driven_trips'] > 0, st
    ref, _ = run_plan(lib, data, vm, {}, one_run(12), 1)
    same(a[0], ref[0], 'against the default trips')


# ---- the Z-slab path on one rank: recounts closed by the staged all-reduce -----------------------------------------------------------------
@pytest.mark.gpu
def test_staged_all_reduce_meets_an_open_pass(lib):
    """One rank with a reduce callback (the slab path: the gate's close files the slab sums only, reduce_staged closes the passes eight at
    a time): 17 sweeps, more than two groups - reduce_staged finds the last recount open -, and the flush at the run's end."""
    data, vm = volume('noise32')
    seen = []

    def prepare(s):
        s.set_reduce_callback(lambda v: (seen.append(tuple(v)), list(v))[1])
    a, _ = both(lib, data, vm, {'batch': 6}, one_run(17), 'one-rank slab path', prepare)
    assert a[0]['sweeps'] == 17 and has_sums(a[0]['trace'])
    assert len(seen) == 2 * (1 + 17)                     # (init and every sweep, for each of the two handles)
    assert seen[:18] == seen[18:]
    ref, _ = run_plan(lib, data, vm, {'batch': 6}, one_run(17), 1)
    same(a[0], ref[0], 'against the one-GPU path')


# ---- an empty unit list and a list of one unit ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('whole_unit', [0, 1])
@pytest.mark.parametrize('storage16', [0, 1])
def test_empty_list_and_list_of_one_unit(lib, whole_unit, storage16):
    """the first passes of the run walk an empty list (the last wave counts the one unit the slab's end cuts) or a list of one unit"""
    data, vm = edge_volume(whole_unit)
    options = {'storage16': storage16, 'sweep_blocks': 2}
    a, st = both(lib, data, vm, options, one_run(6), 'edge volume %d' % whole_unit)
    assert st['listed_at_init'] == whole_unit and st['dense_listed_units'] == whole_unit, st
    assert len(listed_units(a[0]['labels'])) == whole_unit
    assert a[0]['sweeps'] > 0 and has_sums(a[0]['trace'])
    assert a[0]['sizes'][0] > 2                          # (the region grew: the passes counted something that changed)
    res, k = parity.run_stepwise(lib, data, vm, 2.25, None, 6, density_mode=1, options=dict(options, dense_close=1))
    assert res is not None and k > 0
