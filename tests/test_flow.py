"""The flow solve on the branch graph ("f13 flow"): the models of tests/flow_model.py are checked on the CPU
against answers by hand and against the reference's own equations (tests/golden/flow/tree.npz), then vmask_flow /
flow.simulateFlow must equal the sequential model bit for bit at k = 1 - pressures, flows and iteration counts - and, at
k = 1.852 and 2, converge at tol = 1e-12 and stay within a measured allowance of the direct-solver model.

THE ALLOWANCE at k != 1, per case: 100 x the difference between the model's variants (a) (spsolve) and (b) (the kernel's
arithmetic) on the CPU - what two correct solvers of the system differ by; the factor is for the device's pow and another stopping
point inside tol.  Only where the two variants agree to the last bit - a difference of exactly 0: one free node, where both
solve a 1 x 1 system - that difference says nothing, and the allowance is what the number format leaves: 64 round-off units of
the largest pressure over the pressure span, 64 round-off units of the largest flow.  No other case is widened by it."""
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import flow_model as FM
from conftest import ROOT
from arterynetwork_amd import flow as F
from arterynetwork_amd import skeletonization as S

U = 2.0 ** -53
T = FM.T
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'flow', 'tree.npz')


# ------------------------------------------------------------------ cases
def _star(arms, seed=5):
    """A free centre (node 1) behind the inlet (node 0) with `arms` terminals."""
    ends = [[0, 1]] + [[1, 2 + i] if i % 3 else [2 + i, 1] for i in range(arms)]
    fixed = np.ones(arms + 2, np.uint8)
    fixed[1] = 0
    return np.array(ends, np.int64), fixed


def _bridge():
    """A Wheatstone bridge, balanced and symmetric: 0 -> 1, 0 -> 2, 1 -> 3, 2 -> 3 and the bridge 1 -> 2; nodes 0 and 3 fixed."""
    ends = np.array([[0, 1], [0, 2], [1, 3], [2, 3], [1, 2]], np.int64)
    return ends, np.array([1, 0, 0, 1], np.uint8), np.array([1.0, 1.0, 3.0, 3.0, 0.7]), np.array([1.0, 0.0, 0.0, 0.25])


@functools.lru_cache(maxsize=None)
def _case(name, n):
    if name == 'comb':
        ends, fixed = FM.comb(n)
    elif name == 'tree':
        ends, fixed = FM.random_tree(n, 100 + n)
    elif name == 'loops':
        ends, fixed = FM.random_tree(n, 202 + n, extra=max(1, n // 8))
    elif name == 'star':
        ends, fixed = _star(n)
    R, P = FM.inputs_for(ends, fixed, 300 + n, level=0.0 if name == 'comb' else 0.7)
    if name == 'comb':                                                     # a wide backbone: the pressure holds along it, no tooth comes close to balance
        R[:n] /= n
    return ends, fixed, R, P


SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
CASES = [('comb', n) for n in SIZES] + [('tree', n) for n in SIZES] + [('loops', 65), ('loops', 2 * T + 1), ('star', 70)]


@functools.lru_cache(maxsize=None)
def _model(name, n, k, tol=1e-12):
    return FM.solve(*_case(name, n), k=k, tol=tol)


@functools.lru_cache(maxsize=None)
def _direct(name, n, k):
    return FM.solve_direct(*_case(name, n), k=k)


def _distance(a, b, P, fixed):
    """|dP| / (pressure span) and |dQ| / max |Q| between two results, and the format's own limits for the two."""
    fx = np.asarray(fixed).astype(bool)
    span = np.ptp(P[fx]) or np.abs(P[fx]).max() or 1.0                   # (fixed pressures all alike: nothing flows, the scales are the values' own)
    ok = ~np.isnan(a.pressure)
    assert np.array_equal(ok, ~np.isnan(b.pressure))
    qmax = np.abs(a.flow).max() or 1.0
    return (np.abs(a.pressure[ok] - b.pressure[ok]).max() / span, np.abs(a.flow - b.flow).max() / qmax,
            64 * U * np.abs(P[fx]).max() / span, 64 * U)


def _allowance(direct, model, P, fixed):
    dP, dQ, fP, fQ = _distance(direct, model, P, fixed)
    return (100 * dP if dP > 0 else fP), (100 * dQ if dQ > 0 else fQ), dP, dQ     # (the format's limit only where the variants agree to the last bit)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------ CPU: the models against answers by hand
def test_block_sum_is_the_stated_order():
    xs = [float(x) for x in np.random.default_rng(1).random(2 * T + 37)]
    lanes = []
    for t in range(T):
        acc = 0.0
        for x in xs[t::T]:
            acc = acc + x
        lanes.append(acc)
    waves = []
    for w in range(T // 64):
        a = lanes[64 * w:64 * w + 64]
        for s in (32, 16, 8, 4, 2, 1):
            a = [a[j] + a[j ^ s] for j in range(64)]
        waves.append(a[0])
    assert FM.block_sum(xs) == ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert FM.block_sum([]) == 0.0 and FM.block_sum([1.5]) == 1.5


@pytest.mark.parametrize('solver', [FM.solve, FM.solve_direct])
@pytest.mark.parametrize('k', [1.0, 1.852, 2.0])
def test_chain_parallel_and_y_by_hand(solver, k):
    # a chain: equal Q, the drops in the ratio of the R's
    ends, R = np.array([[0, 1], [1, 2], [3, 2]], np.int64), np.array([1.0, 2.0, 3.0])
    got = solver(ends, [1, 0, 0, 1], R, [6.0, 0, 0, 0.0], k=k, tol=1e-13)
    assert got.converged
    q = (6.0 / 6.0) ** (1 / k)
    assert got.flow == pytest.approx([q, q, -q], rel=1e-12)              # (the third branch is given from its far end: the sign)
    assert np.diff(got.pressure) == pytest.approx([-1.0, -2.0, -3.0], rel=1e-12)
    # two parallel branches, then one more: Q1 / Q2 = (R2 / R1)^(1/k), Q1 + Q2 = Q3
    ends, R = np.array([[0, 1], [0, 1], [1, 2]], np.int64), np.array([1.0, 4.0, 2.0])
    got = solver(ends, [1, 0, 1], R, [3.0, 0, 1.0], k=k, tol=1e-13)
    assert got.converged and got.flow[0] / got.flow[1] == pytest.approx(4.0 ** (1 / k), rel=1e-12)
    assert got.flow[0] + got.flow[1] == pytest.approx(got.flow[2], rel=1e-12)
    assert R * np.abs(got.flow) ** k == pytest.approx([3.0 - got.pressure[1]] * 2 + [got.pressure[1] - 1.0], rel=1e-11)
    # a symmetric Y: the children carry half each
    ends, R = np.array([[0, 1], [1, 2], [1, 3]], np.int64), np.array([1.0, 2.0, 2.0])
    got = solver(ends, [1, 0, 1, 1], R, [5.0, 0, 1.0, 1.0], k=k, tol=1e-13)
    assert got.converged and got.flow[1] == pytest.approx(got.flow[2], rel=1e-13) and got.flow[0] == pytest.approx(2 * got.flow[1], rel=1e-12)
    h = 2.0 ** k + 2.0                                                     # 4 = q^k (1 + 2 / 2^k) for the parent's flow q
    assert got.flow[0] == pytest.approx((4.0 * 2.0 ** k / h) ** (1 / k), rel=1e-12)


@pytest.mark.parametrize('solver', [FM.solve, FM.solve_direct])
def test_star_against_brentq(solver):
    from scipy.optimize import brentq
    k = 1.852
    ends, R = np.array([[0, 3], [3, 1], [2, 3]], np.int64), np.array([1.3, 0.7, 2.1])
    P = np.array([4.0, 1.0, 2.5, 0.0])
    law = lambda d, r: np.sign(d) * (abs(d) / r) ** (1 / k)
    centre = brentq(lambda x: law(P[0] - x, R[0]) - law(x - P[1], R[1]) + law(P[2] - x, R[2]), 0.0, 4.0, xtol=1e-15, rtol=1e-15)
    got = solver(ends, [1, 1, 1, 0], R, P, k=k, tol=1e-13)
    assert got.converged and got.pressure[3] == pytest.approx(centre, rel=1e-13)
    assert got.flow == pytest.approx([law(P[0] - centre, R[0]), law(centre - P[1], R[1]), law(P[2] - centre, R[2])], rel=1e-12)


@pytest.mark.parametrize('solver', [FM.solve, FM.solve_direct])
@pytest.mark.parametrize('k', [1.0, 1.852])
def test_balanced_bridge_carries_nothing(solver, k):
    ends, fixed, R, P = _bridge()
    got = solver(ends, fixed, R, P, k=k, tol=1e-12)
    assert got.converged and got.flow[4] == 0.0 and got.pressure[1] == got.pressure[2]
    assert got.flow[0] == pytest.approx((0.75 / 4.0) ** (1 / k), rel=1e-12)


def test_unit_exponent_is_the_laplacian():
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    ends, fixed, R, P = _case('loops', 65)
    N, fx = len(fixed), fixed.astype(bool)
    L = sp.lil_matrix((N, N))
    for (u, v), r in zip(ends.tolist(), R.tolist()):
        L[u, u] += 1 / r; L[v, v] += 1 / r; L[u, v] -= 1 / r; L[v, u] -= 1 / r
    L = L.tocsr()
    want = P.copy()
    want[~fx] = spsolve(L[~fx][:, ~fx].tocsc(), -L[~fx][:, fx] @ P[fx])
    for got in (_model('loops', 65, 1.0), _direct('loops', 65, 1.0)):
        assert got.converged and np.abs(got.pressure - want).max() <= 1e-13
    assert _model('loops', 65, 1.0).outer <= 3 and _direct('loops', 65, 1.0).outer == 1


def test_floating_loop_and_closed_branches_in_the_model():
    ends = np.array([[0, 1], [1, 2], [-1, -1], [1, 1], [3, 4], [5, 6]], np.int64)
    fixed = np.array([1, 0, 1, 0, 0, 1, 0], np.uint8)                      # 3 - 4 floats; 5 - 6 hangs on one fixed node
    got = FM.solve(ends, fixed, np.ones(6), [2.0, 0, 0.0, 0, 0, 7.0, 0], k=1.852, tol=1e-12)
    assert got.converged and got.floating == 1 and np.isnan(got.pressure[3:5]).all() and got.pressure[6] == 7.0
    assert got.flow[2:].tolist() == [0.0, 0.0, 0.0, 0.0] and got.flow[0] == got.flow[1] == pytest.approx(1.0)


@pytest.mark.parametrize('k', [1.852, 2.0])
def test_the_two_variants_agree(k):
    worst = [0.0, 0.0]
    for name, n in CASES:
        a, b = _direct(name, n, k), _model(name, n, k)
        assert a.residual <= 1e-12 and b.converged, (name, n, a.residual, b.residual)
        # the case can be solved to 1e-12 in doubles at all: no branch so close to balance that the pressures' round-off decides
        assert FM.balance_limit(a, _case(name, n)[0], _case(name, n)[2], k) <= 0.5e-12, (name, n)
        dP, dQ, _, _ = _distance(a, b, _case(name, n)[3], _case(name, n)[1])
        worst = [max(worst[0], dP), max(worst[1], dQ)]
    print('k', k, 'largest |dP| / span %.2e, |dQ| / max|Q| %.2e between the variants' % tuple(worst))
    assert worst[0] <= 1e-11 and worst[1] <= 1e-11


# ------------------------------------------------------------------ CPU: the reference's own equations, the host formulas
def test_reference_residuals_equal_the_recorded_lists():
    z = np.load(GOLDEN)
    B, free = len(z['ends']), np.flatnonzero(z['fixed'] == 0)
    for probe, want in zip(z['probes'][1:], z['residuals'][1:]):          # the two probes off the solution
        P = z['pressure'].copy()
        P[free] = probe[B:]
        flow_rows, pressure_rows = F.referenceResiduals(z['ends'], z['radius'], z['length'], z['c'], float(z['k']), z['fixed'], P, probe[:B])
        for got, rec in ((flow_rows, want[:len(free)]), (pressure_rows, want[len(free):])):
            assert np.abs(got - rec).max() <= 1e-10 * np.abs(rec).max()
    assert z['residuals'][0].max() < 1e-6 < 1.0 < z['residuals'][1].max()  # the recorded solution satisfies the reference's equations


def test_the_model_satisfies_the_reference_equations():
    z = np.load(GOLDEN)
    k = float(z['k'])
    R = F.branchResistance(z['length'], z['radius'], law='HW', c=z['c'], k=k)
    got = FM.solve(z['ends'], z['fixed'], R, z['pressure'], k=k, tol=1e-12)
    assert got.converged and (got.flow > 0).all()
    flow_rows, pressure_rows = F.referenceResiduals(z['ends'], z['radius'], z['length'], z['c'], k, z['fixed'], got.pressure, got.flow / (np.pi * z['radius'] ** 2))
    assert flow_rows.max() <= 1e-12 * np.abs(got.flow).max() * 2e10
    assert pressure_rows.max() <= 1e-12 * z['pressure'][0] * (1000 / 13560 / 9.8 * 500)


def test_resistance_and_terminal_pressure_formulas():
    L, r = np.array([0.02, 0.05]), np.array([1e-3, 2e-3])
    assert F.branchResistance(L, r, c=120.0) == pytest.approx(10.67 * L / 120.0 ** 1.852 / (2 * r) ** 4.8704, rel=1e-15)
    assert F.branchResistance(L, r, c=[100.0, 140.0], k=2.0)[1] == pytest.approx(10.67 * 0.05 / 140.0 ** 2 / 4e-3 ** 4.8704, rel=1e-15)
    assert F.branchResistance(L, r, law='poiseuille', k=1) == pytest.approx(8 * 3.5e-3 * L / (np.pi * r ** 4), rel=1e-15)
    assert F.terminalPressures([0.0, 0.1], 100.0, -50.0) == pytest.approx([100.0, 96.0])
    for bad in (dict(), dict(law='poiseuille', k=1.852), dict(law='darcy', c=1.0)):
        with pytest.raises(ValueError):
            F.branchResistance(L, r, **bad)


def test_refused_inputs_are_named():
    ends, fixed, R, P = _case('tree', 63)
    N, fx = len(fixed), fixed.astype(bool)
    call = lambda **kw: F.simulateFlow(**{**dict(graph=(ends, N), resistance=R, fixedNodes=fx, fixedPressure=P, k=1.852), **kw})
    bad_R, bad_P, bad_ends = R.copy(), P.copy(), ends.copy()
    bad_R[17], bad_P[np.flatnonzero(fx)[5]], bad_ends[9, 1] = -1.0, np.inf, N
    for kw, said in ((dict(k=0.9), 'k must'), (dict(k=3.5), 'k must'), (dict(tol=0.0), 'tol'), (dict(tol=1.0), 'tol'), (dict(maxIter=0), 'maxIter'),
                     (dict(resistance=bad_R), 'branch 17'), (dict(resistance=np.stack([R, bad_R])), 'branch 17 of scenario 1'),
                     (dict(fixedPressure=bad_P), 'node {}'.format(np.flatnonzero(fx)[5])), (dict(graph=(bad_ends, N)), 'branch 9'),
                     (dict(resistance=R[:-1]), 'resistance'), (dict(fixedNodes=[0, N]), 'fixed node'),
                     (dict(resistance=np.stack([R] * 2), fixedPressure=np.stack([P] * 3)), 'disagree')):
        with pytest.raises(ValueError, match=said):
            call(**kw)


def test_main_flow_argument_check(tmp_path):
    with pytest.raises(ValueError, match='flow needs'):
        S.main(str(tmp_path), segments=True, prune=(0, 0.0), flow=dict(pressureIn=1.0, slope=0.0, c=100.0))
    with pytest.raises(ValueError, match='flow needs'):
        S.main(str(tmp_path), segments=True, prune=(0, 0.0), morphometry=True, flow=dict(pressureIn=1.0, slope=0.0, c=100.0))
    assert os.listdir(str(tmp_path)) == []


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_flow_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vflow_device.hip' in build.SOURCES
    out = tmp_path / 'vflow_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vflow_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1)),
                            int(re.search(r'\.vgpr_count:\s+(\d+)', m.group(2)).group(1)))
    for frag in ('k_flow_check', '6k_flowE'):
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, (scratch, vgprs) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        assert vgprs <= 128, '%s uses %d VGPRs' % (name, vgprs)       # (the first build reports 113 for k_flow: pow is in it)


# ------------------------------------------------------------------ GPU
def _gpu(ends, fixed, R, P, k, tol=1e-12, max_iter=50, info=None):
    return F.simulateFlow((ends, len(fixed)), R, np.asarray(fixed).astype(bool), P, k=k, tol=tol, maxIter=max_iter, info=info)


def _assert_is_model(got, s, model):
    assert _bits(got.pressure[s]) == _bits(model.pressure) and _bits(got.flow[s]) == _bits(model.flow)
    assert (bool(got.converged[s]), int(got.outerIterations[s]), int(got.innerIterations[s])) == (model.converged, model.outer, model.inner)
    assert _bits(got.residual[s]) == _bits(np.float64(model.residual))


def _assert_near_direct(got, direct, model, P, fixed, label):
    """Converged, the contract's residual, and within the measured allowance of the direct-solver model."""
    assert bool(got.converged[0]) and float(got.residual[0]) <= 1e-12, label
    aP, aQ, cP, cQ = _allowance(direct, model, P, fixed)
    one = FM.Result()
    one.pressure, one.flow = got.pressure[0], got.flow[0]
    dP, dQ, _, _ = _distance(direct, one, P, fixed)
    print(label, 'variants differ by %.2e (P) %.2e (Q); the GPU by %.2e (P) %.2e (Q); outer %d inner %d' % (cP, cQ, dP, dQ, got.outerIterations[0], got.innerIterations[0]))
    assert dP <= aP and dQ <= aQ, label
    fx = np.asarray(fixed).astype(bool)
    assert np.array_equal(got.pressure[0][fx & ~np.isnan(got.pressure[0])], P[fx & ~np.isnan(got.pressure[0])])


@pytest.mark.gpu
@pytest.mark.parametrize('name,n', CASES)
def test_unit_exponent_equals_the_model_bit_for_bit(name, n):
    ends, fixed, R, P = _case(name, n)
    got = _gpu(ends, fixed, R, P, 1.0)
    _assert_is_model(got, 0, _model(name, n, 1.0))
    assert got.floating == 0 and got.pressure.shape == (1, len(fixed)) and got.flow.shape == (1, len(ends))


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1.852, 2.0])
@pytest.mark.parametrize('name,n', CASES)
def test_power_law_converges_within_the_allowance(name, n, k):
    ends, fixed, R, P = _case(name, n)
    label = '{} {} k {}'.format(name, n, k)
    _assert_near_direct(_gpu(ends, fixed, R, P, k), _direct(name, n, k), _model(name, n, k), P, fixed, label)


@pytest.mark.gpu
def test_parallel_loop_closed_floating_and_sign():
    """Parallel branches; a loop and a closed curve beside a tree (Q = 0 there, the rest unchanged); a component without a fixed
    node (NaN, counted) and one with a single fixed node (P constant, Q = 0); a branch given from its far end (the sign)."""
    tree, tfixed, tR, tP = _case('tree', 63)
    N0 = len(tfixed)
    plain = _gpu(tree, tfixed, tR, tP, 1.852)
    extra = np.array([[-1, -1], [5, 5], [2, 9], [9, 2], [N0, N0 + 1], [N0 + 1, N0 + 2], [N0 + 4, N0 + 3], [N0 + 5, N0 + 5]], np.int64)
    ends = np.concatenate([tree[:10], extra[:2], tree[10:], extra[2:]])
    at = np.concatenate([np.arange(10), np.arange(12, 12 + len(tree) - 10)])          # where the tree's branches went
    fixed = np.concatenate([tfixed, [0, 0, 0, 1, 0, 0]]).astype(np.uint8)
    R = np.concatenate([tR[:10], [1.0, np.nan], tR[10:], [0.9, 1.1, 1.0, 2.0, 3.0, -1.0]])          # (a loop's R is not looked at)
    P = np.concatenate([tP, [0, 0, 0, 0.6, 0, 0]])
    info = {}
    for k in (1.0, 1.852, 2.0):
        got = _gpu(ends, fixed, R, P, k, info=info)
        model = FM.solve(ends, fixed, R, P, k=k, tol=1e-12)
        assert bool(got.converged[0]) and got.floating == 2 and info == {'floatingComponents': 2, 'floatingNodes': 4}
        assert np.isnan(got.pressure[0, [N0, N0 + 1, N0 + 2, N0 + 5]]).all() and got.pressure[0, N0 + 3] == got.pressure[0, N0 + 4] == 0.6
        closed = [10, 11] + list(range(len(ends) - 4, len(ends)))
        assert (got.flow[0, closed] == 0.0).all() and not np.signbit(got.flow[0, closed]).any()
        pair = got.flow[0, len(ends) - 6:len(ends) - 4]                  # 2 -> 9 and 9 -> 2 in parallel: opposite signs, the law on either
        assert pair[0] * pair[1] < 0 and R[len(ends) - 6] * abs(pair[0]) ** k == pytest.approx(R[len(ends) - 5] * abs(pair[1]) ** k, rel=1e-11)
        if k == 1.0:
            _assert_is_model(got, 0, model)
        else:
            _assert_near_direct(got, FM.solve_direct(ends, fixed, R, P, k=k), model, P, fixed, 'mixed graph k {}'.format(k))
    # without the parallel pair the tree's own solution is untouched by what stands beside it
    keep = np.ones(len(ends), bool)
    keep[len(ends) - 6:len(ends) - 4] = False
    beside = _gpu(ends[keep], fixed, R[keep], P, 1.852)
    assert _bits(beside.pressure[0, :N0]) == _bits(plain.pressure[0]) and _bits(beside.flow[0, at]) == _bits(plain.flow[0])
    # the sign: the same tree with one branch turned round
    turned = tree.copy()
    turned[7] = turned[7, ::-1]
    other = _gpu(turned, tfixed, tR, tP, 1.852)
    assert other.flow[0, 7] == -plain.flow[0, 7] != 0.0
    assert np.abs(other.pressure - plain.pressure).max() <= 1e-12 and np.abs(np.delete(other.flow - plain.flow, 7)).max() <= 1e-12 * np.abs(plain.flow).max()


@pytest.mark.gpu
def test_balanced_bridge_on_the_floor():
    ends, fixed, R, P = _bridge()
    got = _gpu(ends, fixed, R, P, 1.852)
    assert bool(got.converged[0]) and got.flow[0, 4] == 0.0 and got.pressure[0, 1] == got.pressure[0, 2]
    assert got.flow[0, 0] == pytest.approx((0.75 / 4.0) ** (1 / 1.852), rel=1e-12)
    _assert_is_model(_gpu(ends, fixed, R, P, 1.0), 0, FM.solve(ends, fixed, R, P, k=1.0, tol=1e-12))


@functools.lru_cache(maxsize=None)
def _volume_case(density, seed):
    """The unthinned random 24^3 graphs of test_morphometry.py with Hazen-Williams resistances from their own morphometry: a voxel
    of 0.5 mm, c = 120; the end points are fixed, the first one the inlet at 100 mmHg, the others at 0."""
    import test_morphometry as TMo
    t = TMo._of_volume(TMo.TB._random((24, 24, 24), density, seed))
    m = S.branchMorphometry(t.graph(), dist=TMo._dist_for(t.shape))
    # (a two-entry branch takes its meanRadius from its neighbours, as in the reference: 0 where none has one - floored like the length)
    R = F.branchResistance(np.maximum(m.pathLength, 0.5) * 0.5e-3, np.maximum(m.meanRadius, 0.5) * 0.5e-3, c=120.0)
    fixed = (t.degree == 1).astype(np.uint8)
    if not fixed.any():                                                    # (the densest volume is one cluster with two loops)
        fixed[0] = 1
    P = np.zeros(len(fixed))
    P[np.flatnonzero(fixed)[0]] = 13328.0                                  # the other end points drain at pressure 0
    return t.ends, fixed, R, P


@pytest.mark.gpu
@pytest.mark.parametrize('density,seed', [(0.1, 41), (0.3, 42), (0.6, 43)])
def test_graphs_of_random_volumes(density, seed):
    ends, fixed, R, P = _volume_case(density, seed)
    info = {}
    got = _gpu(ends, fixed, R, P, 1.0, info=info)
    model = FM.solve(ends, fixed, R, P, k=1.0, tol=1e-12)
    print(density, 'nodes', len(fixed), 'branches', len(ends), 'fixed', int(fixed.sum()), 'floating', info, 'outer', model.outer, 'inner', model.inner)
    assert len(fixed) <= 2200 and got.floating == model.floating == info['floatingComponents']
    _assert_is_model(got, 0, model)
    for k in (1.852, 2.0):
        label = 'volume {} k {}'.format(density, k)
        _assert_near_direct(_gpu(ends, fixed, R, P, k), FM.solve_direct(ends, fixed, R, P, k=k), FM.solve(ends, fixed, R, P, k=k, tol=1e-12), P, fixed, label)


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1.0, 1.852])
def test_batches_equal_their_single_runs(k):
    ends, fixed, R, P = _case('loops', 65)
    rng = np.random.default_rng(9)
    one = _gpu(ends, fixed, R, P, k)
    Rs, Ps = R * (0.9 + 0.2 * rng.random((3, len(R)))), P * (0.9 + 0.2 * rng.random((3, len(P))))
    fields = ('pressure', 'flow', 'converged', 'outerIterations', 'innerIterations', 'residual')
    same = lambda a, s, b: all(_bits(getattr(a, f)[s]) == _bits(getattr(b, f)[0]) for f in fields)
    for Rin, Pin in ((R, P), (Rs, P), (R, Ps), (Rs, Ps)):
        got = _gpu(ends, fixed, Rin, Pin, k)
        S_ = 3 if (np.ndim(Rin) == 2 or np.ndim(Pin) == 2) else 1
        assert got.pressure.shape == (S_, len(fixed)) and got.converged.all()
        for s in range(S_):
            assert same(got, s, _gpu(ends, fixed, Rin[s] if np.ndim(Rin) == 2 else Rin, Pin[s] if np.ndim(Pin) == 2 else Pin, k)), s
    assert same(_gpu(ends, fixed, np.stack([R] * 3), P, k), 2, one)
    # indices instead of a mask: one pressure per index
    where = np.flatnonzero(fixed)[::-1]
    by_index = F.simulateFlow((ends, len(fixed)), R, where, P[where], k=k, tol=1e-12)
    assert same(by_index, 0, one)


@pytest.mark.gpu
def test_six_hundred_scenarios():
    """More workgroups than compute units: every scenario equals its own single-scenario run bit for bit.  The comb, not the
    random tree: among 600 draws of the tree's resistances one (scenario 141) brings a branch so close to balance that
    flow_model.balance_limit is 1.5e-12 - the round-off of the stored pressures alone is above the tolerance, and the sequential
    model stalls at 1.08e-12 as the kernel does.  On the comb the model's largest residual over the 600 draws is 1.6e-14."""
    ends, fixed, R, P = _case('comb', 63)
    Rs = R * (0.9 + 0.2 * np.random.default_rng(10).random((600, len(R))))
    got = _gpu(ends, fixed, Rs, P, 1.852)
    assert got.converged.all() and got.pressure.shape == (600, len(fixed))
    for s in range(600):
        one = _gpu(ends, fixed, Rs[s], P, 1.852)
        assert _bits(one.pressure[0]) == _bits(got.pressure[s]) and _bits(one.flow[0]) == _bits(got.flow[s]), s
        assert (one.outerIterations[0], one.innerIterations[0], one.residual[0]) == (got.outerIterations[s], got.innerIterations[s], got.residual[s])


@pytest.mark.gpu
def test_one_outer_iteration_is_reported_not_raised():
    """max_iter and k hold for the whole call and the topology is one, so a neighbour that converges in ONE outer step beside a
    scenario that does not can only be one whose linear start is already the answer: on a graph with free nodes that is a
    scenario in which nothing flows (every fixed pressure the same).  Their convergence is trivial, and said to be; what the
    test shows is that the unconverged scenario is reported, holds a finite iterate and leaves them untouched.  A start that is
    exact WITH flow is the graph without free nodes, run last: the law alone, one step."""
    ends, fixed, R, P = _case('tree', 65)
    flat = np.where(fixed, 0.4, 0.0)                                       # every fixed pressure the same: nothing flows, one step
    Ps = np.stack([flat, P, flat])
    got = _gpu(ends, fixed, R, Ps, 1.852, max_iter=1)
    assert got.converged.tolist() == [True, False, True] and got.outerIterations.tolist() == [1, 1, 1]
    assert got.residual[1] > 1e-12 and np.isfinite(got.pressure[1]).all() and np.isfinite(got.flow[1]).all() and np.abs(got.flow[1]).max() > 0
    alone = _gpu(ends, fixed, R, flat, 1.852, max_iter=1)
    for s in (0, 2):
        assert _bits(got.pressure[s]) == _bits(alone.pressure[0]) and (got.flow[s] == 0.0).all() and (got.pressure[s] == 0.4).all()
    full = _gpu(ends, fixed, R, P, 1.852)
    assert bool(full.converged[0]) and full.outerIterations[0] > 1
    every = np.ones(len(fixed), np.uint8)                                  # no free node: the flows are the law's, batch of two
    Pall = np.stack([np.linspace(1.0, 0.0, len(fixed)), np.linspace(0.2, 0.9, len(fixed))])
    got = _gpu(ends, every, R, Pall, 1.852, max_iter=1)
    assert got.converged.tolist() == [True, True] and got.outerIterations.tolist() == [1, 1] and got.innerIterations.tolist() == [0, 0]
    d = Pall[:, ends[:, 0]] - Pall[:, ends[:, 1]]
    assert _bits(got.pressure) == _bits(Pall) and np.abs(got.flow).min() > 0
    assert got.flow == pytest.approx(np.sign(d) * (np.abs(d) / R) ** (1 / 1.852), rel=1e-14)


@pytest.mark.gpu
def test_the_library_refuses_before_it_writes():
    import ctypes as C
    ends, fixed, R, P = _case('tree', 63)
    N, B = len(fixed), len(ends)
    dll = F._lib()
    bad_R, inf_R, bad_P, bad_ends, half = R.copy(), R.copy(), P.copy(), ends.copy(), ends.copy()
    bad_R[3], inf_R[4], bad_P[0], bad_ends[2, 0], half[5] = 0.0, np.inf, np.nan, N, (-1, 3)
    ok = dict(S=1, R=R, rs=0, P=P, ps=0, k=1.852, tol=1e-10, it=50, ends=ends)
    for change in (dict(S=0), dict(k=0.99), dict(k=3.01), dict(k=np.nan), dict(tol=0.0), dict(tol=1.0), dict(it=0), dict(R=bad_R), dict(R=inf_R), dict(P=bad_P),
                   dict(ends=bad_ends), dict(ends=half), dict(rs=B - 1), dict(ps=1)):
        a = {**ok, **change}
        outs = [np.full((1, N), -77.0), np.full((1, B), -77.0), np.full((1, 3), -77, np.int64), np.full(1, -77.0), np.full(2, -77, np.int64)]
        e, r, p = np.ascontiguousarray(a['ends']), np.ascontiguousarray(a['R']), np.ascontiguousarray(a['P'])
        rc = dll.vmask_flow(0, N, B, e.ctypes.data, fixed.ctypes.data, a['S'], r.ctypes.data, a['rs'], p.ctypes.data, a['ps'], float(a['k']), float(a['tol']), a['it'],
                            *[o.ctypes.data for o in outs])
        assert rc == -1 and dll.vmask_last_error() and all((o == -77).all() for o in outs), change
    outs = [np.full((1, N), -77.0), np.full((1, B), -77.0), np.full((1, 3), -77, np.int64), np.full(1, -77.0), np.full(2, -77, np.int64)]
    o = [x.ctypes.data for x in outs]
    common = (0, 1.852, 1e-10, 50)
    for args in ((0, N, B, ends.ctypes.data, fixed.ctypes.data, 2 ** 31, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o),      # too many scenarios
                 (0, -1, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o),           # negative counts
                 (0, N, -1, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o),
                 (0, N, 2 ** 30, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o),
                 (0, N, B, None, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o),                        # null pointers
                 (0, N, B, ends.ctypes.data, None, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o),
                 (0, N, B, ends.ctypes.data, fixed.ctypes.data, 1, None, 0, P.ctypes.data) + common + tuple(o),
                 (0, N, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, None) + common + tuple(o),
                 (0, N, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + (None,) + tuple(o[1:]),
                 (0, N, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + (o[0], None) + tuple(o[2:]),
                 (0, N, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o[:2]) + (None,) + tuple(o[3:]),
                 (0, N, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o[:3]) + (None, o[4]),
                 (99, N, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data) + common + tuple(o)):           # no such device
        rc = dll.vmask_flow(*args)
        assert rc in (-1, -2) and (rc == -2) == (args[0] == 99) and dll.vmask_last_error() and all((x == -77).all() for x in outs), args[:3]
    assert dll.vmask_flow(0, N, B, ends.ctypes.data, fixed.ctypes.data, 1, R.ctypes.data, 0, P.ctypes.data, *common, *o[:4], None) == 0      # counts may be NULL
    assert not any((x == -77).any() for x in outs[:4]) and (outs[4] == -77).all()
    # a pressure that is not finite at a FREE node is not looked at
    loose = P.copy()
    loose[np.flatnonzero(fixed == 0)[0]] = np.nan
    assert _bits(_gpu(ends, fixed, R, loose, 1.0).flow) == _bits(_gpu(ends, fixed, R, P, 1.0).flow)


@pytest.mark.gpu
def test_repeats_are_bit_identical():
    ends, fixed, R, P = _case('loops', 2 * T + 1)
    Rs = R * (0.9 + 0.2 * np.random.default_rng(11).random((5, len(R))))
    a, b = _gpu(ends, fixed, Rs, P, 1.852), _gpu(ends, fixed, Rs, P, 1.852)
    for f in F.FlowResult.names:
        assert _bits(getattr(a, f)) == _bits(getattr(b, f)), f


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import flow as F
import test_flow as T
ends, fixed, R, P = T._case('loops', 65)
dev = torch.device('cuda', 0)
Rs = R * (0.9 + 0.2 * np.random.default_rng(12).random((4, len(R))))
h = T._gpu(ends, fixed, Rs, P, 1.852)
d = F.simulateFlow((torch.as_tensor(ends, device=dev), len(fixed)), torch.as_tensor(Rs, device=dev), fixed.astype(bool), torch.as_tensor(P, device=dev), k=1.852, tol=1e-12)
m = F.simulateFlow((ends, len(fixed)), torch.as_tensor(Rs, device=dev), fixed.astype(bool), P, k=1.852, tol=1e-12)           # (host pressures beside device resistances)
for g in (d, m):
    for name in F.FlowResult.names:
        a, b = getattr(g, name), getattr(h, name)
        assert a.is_cuda and a.device == dev and tuple(a.shape) == b.shape, name
        assert a.cpu().numpy().tobytes() == b.tobytes(), name
    assert g.floating == h.floating == 0
assert d.pressure.dtype == torch.float64 and d.outerIterations.dtype == torch.int64 and d.converged.dtype == torch.bool
bad = torch.as_tensor(Rs, device=dev).clone()
bad[2, 7] = float('nan')
try:
    F.simulateFlow((ends, len(fixed)), bad, fixed.astype(bool), P)
except ValueError as e:
    assert 'branch 7 of scenario 2' in str(e)
else:
    raise AssertionError('a NaN resistance on the device was accepted')
# the library's own check where the tables are device arrays: counted on the device, nothing written
N, B = len(fixed), len(ends)
t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
te, tf, tP = t(ends), t(fixed), t(P)
nan_R, bad_e, inf_P = t(Rs), t(ends), t(P)
nan_R[3, 11], bad_e[4, 1], inf_P[int(np.flatnonzero(fixed)[2])] = float('nan'), N, float('inf')
dll = F._lib()
for e, r, p in ((te, nan_R, tP), (bad_e, t(Rs), tP), (te, t(Rs), inf_P)):
    outs = [torch.full((4, N), -77.0, dtype=torch.float64, device=dev), torch.full((4, B), -77.0, dtype=torch.float64, device=dev),
            torch.full((4, 3), -77, dtype=torch.int64, device=dev), torch.full((4,), -77.0, dtype=torch.float64, device=dev)]
    counts = np.full(2, -77, np.int64)
    torch.cuda.synchronize()
    rc = dll.vmask_flow(0, N, B, e.data_ptr(), tf.data_ptr(), 4, r.data_ptr(), B, p.data_ptr(), 0, 1.852, 1e-10, 50, *[o.data_ptr() for o in outs], counts.ctypes.data)
    assert rc == -1 and b'does not fit' in dll.vmask_last_error(), rc
    assert all(bool((o == -77).all()) for o in outs) and (counts == -77).all()
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_flow_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, equal to the host call.
    Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_reference_residuals_of_the_solution():
    """The contract in the reference's units: its flow rows at the kernel's solution are at most tol max |Q| 2e10, its pressure
    rows - rounding only, the flows come from the pressures - at most 1e-12 of the inlet pressure in those units."""
    z = np.load(GOLDEN)
    k, tol = float(z['k']), 1e-12
    R = F.branchResistance(z['length'], z['radius'], law='HW', c=z['c'], k=k)
    got = _gpu(z['ends'], z['fixed'], R, z['pressure'], k, tol=tol)
    assert bool(got.converged[0]) and (got.flow[0] > 0).all()
    flow_rows, pressure_rows = F.referenceResiduals(z['ends'], z['radius'], z['length'], z['c'], k, z['fixed'], got.pressure[0], got.flow[0] / (np.pi * z['radius'] ** 2))
    unit = 1000 / 13560 / 9.8 * 500
    print('flow rows %.3e (bound %.3e), pressure rows %.3e of the inlet pressure' % (flow_rows.max(), tol * np.abs(got.flow).max() * 2e10, pressure_rows.max() / (z['pressure'][0] * unit)))
    assert flow_rows.max() <= tol * np.abs(got.flow).max() * 2e10
    assert pressure_rows.max() <= 1e-12 * z['pressure'][0] * unit
    B, free = len(z['ends']), np.flatnonzero(z['fixed'] == 0)
    assert np.abs(got.pressure[0][free] - z['probes'][0][B:]).max() <= 1e-10 * z['pressure'][0]


@pytest.mark.gpu
def test_main_writes_the_flow_files(tmp_path, capsys):
    from arterynetwork_amd import nifti
    import skeleton_model as M
    m = M.crossing_phantom((48, 48, 32))
    m[10, 33:45, 15:17] = 1
    aff = np.array([[0.5, 0, 0, -10.0], [0, 0.5, 0, 3.0], [0, 0, 0.5, 7.5], [0, 0, 0, 1.0]])
    plain, solved, skew = tmp_path / 'plain', tmp_path / 'solved', tmp_path / 'skew'
    for d in (plain, solved, skew):
        d.mkdir()
        nifti.saveVolume(m, aff if d is not skew else aff * np.array([1, 1, 1.2, 1.0]), str(d / 'vesselVolumeMask.nii.gz'))
    opts = dict(pressureIn=13328.0, slope=-2000.0, c=120.0, k=1.852)
    before = S.main(str(plain), segments=True, prune=(0, 0.0), morphometry=True, roots=[0])
    capsys.readouterr()
    after = S.main(str(solved), segments=True, prune=(0, 0.0), morphometry=True, roots=[0], flow=opts)
    said = capsys.readouterr().out
    assert sorted(os.listdir(str(solved))) == sorted(os.listdir(str(plain)) + [F.FLOW_FILE])
    assert '{} saved to {}.'.format(F.FLOW_FILE, os.path.join(str(solved), F.FLOW_FILE)) in said
    info_files = (S.SEGMENT_INFO_FILE, S.NODE_INFO_FILE)
    for name in os.listdir(str(plain)):                                   # every other file byte for byte
        if name == S.BRANCH_FILE:                                             # (but for labelRounds, which describes the run and differs between two)
            with np.load(str(plain / name)) as x, np.load(str(solved / name)) as y:
                assert x.files == y.files
                for k in x.files:
                    keep = x['countNames'] != 'labelRounds' if k == 'counts' else slice(None)
                    assert x[k].dtype == y[k].dtype and np.array_equal(x[k][keep], y[k][keep]), (name, k)
        elif name not in info_files:
            assert (plain / name).read_bytes() == (solved / name).read_bytes(), name
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after))
    graph = S.branchGraph(S.skeletonize(m))
    measured = S.branchMorphometry(graph, vesselVolumeMask=m, spacing=(0.5, 0.5, 0.5), roots=[0])
    want, extra = S.flowOnGraph(graph, measured, (0.5, 0.5, 0.5), **opts)
    z = np.load(str(solved / F.FLOW_FILE))
    assert bool(want.converged[0]) and int(z['floating']) == want.floating
    for f in F.FlowResult.names:
        assert _bits(z[f]) == _bits(getattr(want, f)), f
    for f, v in extra.items():
        assert _bits(z[f]) == _bits(v), f
    fixed = extra['fixed']
    assert fixed[0] and fixed.sum() >= 3 and extra['fixedPressure'][0] == 13328.0
    ends_at = np.flatnonzero(fixed)[1:]
    assert extra['fixedPressure'][ends_at] == pytest.approx(13328.0 - 2000.0 * 0.8 * measured.pathDistance[ends_at] * 1e-3, rel=1e-14)
    assert extra['length'] == pytest.approx(measured.pathLength * 1e-3) and extra['radius'] == pytest.approx(measured.meanRadius * 0.5e-3)
    with open(str(solved / S.SEGMENT_INFO_FILE), 'rb') as f:
        seg = pickle.load(f)
    with open(str(plain / S.SEGMENT_INFO_FILE), 'rb') as f:
        seg0 = pickle.load(f)
    with open(str(solved / S.NODE_INFO_FILE), 'rb') as f:
        node = pickle.load(f)
    assert sorted(seg) == sorted(seg0) and len(seg) > 0
    for b, d in seg.items():
        assert d.pop('simulationData') == {'velocity': float(extra['velocity'][b]), 'flow': float(want.flow[0, b])} and d == seg0[b]
    for v, c in enumerate(graph.nodeCoords.tolist()):
        assert node[tuple(c)]['simulationData'] == {'pressure': float(want.pressure[0, v])}
    with pytest.raises(ValueError, match='isotropic'):
        S.main(str(skew), segments=True, prune=(0, 0.0), morphometry=True, roots=[0], flow=opts)
