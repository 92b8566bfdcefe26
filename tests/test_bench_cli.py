"""bench.py plumbing that needs no GPU: `--gpus N` started plainly launches the N ranks itself (a child
torch.distributed.run, before this process touches the GPU); the roofline arithmetic; the traffic stamp."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench


def test_gpus_n_spawns_a_launcher(monkeypatch):
    calls = []
    monkeypatch.setattr(bench.subprocess, 'call', lambda cmd, env=None: calls.append((cmd, env)) or 0)
    monkeypatch.setattr(bench, 'visible_gpus', lambda: 8)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8', '--steps', '7', '--warmup', '3'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and len(calls) == 1
    cmd, env = calls[0]
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1']
    assert cmd[cmd.index('--nproc-per-node') + 1] == '8' and cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-6:] == ['--gpus', '8', '--steps', '7', '--warmup', '3'] and os.path.basename(cmd[-7]) == 'bench.py'
    assert env['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'
    assert '--log-dir' in cmd and cmd[cmd.index('--tee') + 1] == '2'          # every rank's stderr is shown and kept (stdout - the JSON line - passes through untouched)


def test_gpus_n_preflight_and_rank_stderr(monkeypatch, capsys):
    """--gpus N on a node with fewer devices: exit code 2 and a message BEFORE anything is spawned; a launch that fails
    prints the tail of every rank's stderr log."""
    calls = []
    monkeypatch.setattr(bench.subprocess, 'call', lambda cmd, env=None: calls.append(cmd) or 0)
    monkeypatch.setattr(bench, 'visible_gpus', lambda: 1)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and not calls
    assert 'needs 4 visible GPUs, this node shows 1' in capsys.readouterr().err

    def failing(cmd, env=None):
        d = os.path.join(cmd[cmd.index('--log-dir') + 1], 'attempt_0', '1')
        os.makedirs(d)
        open(os.path.join(d, 'stderr.log'), 'w').write('Traceback ...\nVrgError: RCCL all-reduce of the slab statistics failed\n')
        return 1
    monkeypatch.setattr(bench.subprocess, 'call', failing)
    monkeypatch.setattr(bench, 'visible_gpus', lambda: 4)
    with pytest.raises(SystemExit) as e:
        bench.main()
    err = capsys.readouterr().err
    assert e.value.code == 1 and 'the 4-rank launch failed with exit code 1' in err and 'RCCL all-reduce of the slab statistics failed' in err


def test_roofline_is_a_fraction_of_peak():
    r = bench.roofline((880, 880, 640), 640, 0.32, 500, None)
    assert r['bytes_per_launch'] == int(4.25 * 896 * 884 * 640) == 2154414080
    assert 0.8 < r['frac'] < 0.86 and r['frac'] == round(r['achieved'] / 8000.0, 4)
    assert r['algorithmic_equiv_gbs'] > r['achieved']            # 6 B/voxel accounting is kept apart, never as frac
    r16 = bench.roofline((880, 880, 640), 640, 0.24, 500, None, storage16=True)
    assert r16['bytes_per_voxel'] == 2.25 and r16['frac'] < 1
    # bytes counted on the device (excluded runs not fetched) replace the streamed figure in frac, which stays <= 1
    rs = bench.roofline((880, 880, 640), 640, 0.19, 500, None, dense_bytes=1.06e9)
    assert rs['bytes_per_launch'] == 1060000000 and rs['bytes_counted_on_device'] and 0.6 < rs['frac'] < 0.75
    assert rs['streamed_equiv_gbs'] > 8000 > rs['achieved']


def test_traffic_only_for_the_sources_it_was_measured_on():
    t = json.load(open(os.path.join(ROOT, 'profiles', 'traffic.json')))
    entries = t.get('entries', [t])
    assert entries
    for e in entries:                                  # one entry per profiled workload (shape, ranks, storage, slab planes)
        got = bench.load_traffic(tuple(e['shape']), e.get('n_gpus', 1), bool(e.get('storage16')), e.get('planes'))
        assert got == (e['hbm_bytes_per_launch'] if e.get('src_sha') == bench.device_source_sha() else None)
        assert bench.load_traffic(tuple(e['shape']), e.get('n_gpus', 1), not e.get('storage16'), e.get('planes')) is None or len(entries) > 1
        # ... and only for a pass that has to fetch the same bytes (within 2 %): the same shape without its brain mask is another workload
        ref = e.get('design_bytes_per_launch_counted_on_device')
        if ref and e.get('src_sha') == bench.device_source_sha():
            args = (tuple(e['shape']), e.get('n_gpus', 1), bool(e.get('storage16')), e.get('planes'))
            assert bench.load_traffic(*args, design_bytes=ref * 1.01) == e['hbm_bytes_per_launch']
            assert bench.load_traffic(*args, design_bytes=ref * 2.0) is None
    assert bench.load_traffic((1, 2, 3), 1, False) is None


def test_section8d_figure_is_kept_apart_from_frac():
    r = bench.roofline((880, 880, 640), 640, 0.178, 125, None, dense_bytes=1.0616e9, kernel='k_recount_bits<3,true,0,true>')
    assert r['kernel'] == 'k_recount_bits<3,true,0,true>' and 0.7 < r['frac'] < 0.8
    assert r['section8d_frac'] > 1.5 and 'not a fraction' in r['section8d_note']      # 6 B x voxels / time / peak: the driver's own figure


def test_dump_outputs_of_the_timed_steps(tmp_path):
    """--dump-outputs: float32 / float64 .npy files of what the timed sweeps computed (sequential host model as compute); one trace
    row per timed sweep, the label sample agrees with the labels, the same run writes the same files."""
    from arterynetwork_amd._capi import Session, VrgLib
    from test_slabs_gloo import HM, _inputs
    import subprocess
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'tests', 'hostmodel'), '-s', 'libvrg_hostmodel.so'])
    data, vmap = _inputs()
    got = []
    for k in range(2):
        s = Session(data.shape, lib=VrgLib(HM, 'vrgm_'))
        s.set_volume(data); s.set_labels(vmap); s.init(2.25)
        s.run(3, 10 ** 9, None)
        s.run(8, 10 ** 9, None)
        d = tmp_path / str(k)
        bench.dump_outputs(s, str(d), 4)
        lab, seg, tr = s.labels(), s.segmented(), s.trace()
        bands = [s.band(0), s.band(1)]
        s.close()
        files = {p.stem: np.load(str(p)) for p in d.iterdir()}
        assert sorted(files) == ['band_inner', 'band_outer', 'labels_per_plane', 'labels_sample', 'labels_sample_index', 'segmented', 'trace']
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= bench.DUMP_MAX_BYTES
        assert np.array_equal(files['labels_sample'], lab.reshape(-1)[files['labels_sample_index'].astype(np.int64)])
        assert files['labels_per_plane'].shape == (data.shape[2], 5)
        assert np.array_equal(files['labels_per_plane'], np.stack([(lab == k).sum(axis=(0, 1)) for k in range(5)], axis=1))
        assert np.array_equal(files['segmented'], seg.astype(np.float32))
        assert files['trace'].shape == (5, len(tr.dtype.names))                     # the sweeps 4..8 of the second call
        for j, f in enumerate(tr.dtype.names):
            assert np.array_equal(files['trace'][:, j], tr[f][4:].astype(np.float64), equal_nan=True), f
        for (co, ip, op), name in zip(bands, ('band_inner', 'band_outer')):
            assert len(co) and np.array_equal(files[name], np.concatenate([co, ip[:, None], op[:, None]], axis=1))
        got.append(files)
    assert got[0].keys() == got[1].keys() and all(np.array_equal(got[0][n], got[1][n]) for n in got[0])


def test_dump_outputs_samples_long_lists(tmp_path, monkeypatch):
    """Lists longer than their caps are written as seeded samples of rows, in order, with the rows' positions beside them."""
    from arterynetwork_amd._capi import Session, VrgLib
    from test_slabs_gloo import HM, _inputs
    data, vmap = _inputs()
    monkeypatch.setattr(bench, 'DUMP_SEG_ROWS', 100)
    monkeypatch.setattr(bench, 'DUMP_BAND_ROWS', 50)
    s = Session(data.shape, lib=VrgLib(HM, 'vrgm_'))
    s.set_volume(data); s.set_labels(vmap); s.init(2.25)
    s.run(8, 10 ** 9, None)
    bench.dump_outputs(s, str(tmp_path), 1)
    seg, bands = s.segmented(), [s.band(0), s.band(1)]
    s.close()
    f = {p.stem: np.load(str(p)) for p in tmp_path.iterdir()}
    rows = f['segmented_index'].astype(np.int64)
    assert len(seg) > 100 and len(rows) == 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(f['segmented'], seg[rows].astype(np.float32))
    for (co, ip, op), name in zip(bands, ('band_inner', 'band_outer')):
        full = np.concatenate([co, ip[:, None], op[:, None]], axis=1)
        if len(full) > 50:
            rows = f[name + '_index'].astype(np.int64)
            assert len(rows) == 50 and np.all(np.diff(rows) > 0) and np.array_equal(f[name], full[rows])
        else:
            assert np.array_equal(f[name], full)
