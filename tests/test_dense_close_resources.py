"""The two kernels that close a dense pass left open (option dense_close: k_gate in front of the next pass, k_dense_close where the host
looks first) use no scratch memory.  No GPU needed: hipcc cross-compiles the device code of vrg_device.hip and vrg_chain.hip to gfx950
assembly, as tests/test_kernel_resources.py does, and the kernels' resource records are read from it - records only, no instruction."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from arterynetwork_amd import build

CSRC = os.path.join(ROOT, 'arterynetwork_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_closing_kernels_use_no_scratch(tmp_path):
    recs = {}
    for src in ('vrg_device.hip', 'vrg_chain.hip'):
        out = tmp_path / (os.path.splitext(src)[0] + '.s')
        p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), src], cwd=CSRC, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):          # one metadata record per kernel
            f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
            recs[m.group(1)] = (f('private_segment_fixed_size'), f('vgpr_count'))
    found = {frag: [(n, r) for n, r in recs.items() if frag in n] for frag in ('13k_dense_closeE', '6k_gateE')}
    for frag, hits in found.items():
        assert len(hits) == 1, (frag, hits)
        name, (scratch, vgpr) = hits[0]
        print('%s: %d B scratch, %d VGPRs' % (name, scratch, vgpr))
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
    assert found['6k_gateE'][0][1][1] <= 64                  # (the gate's budget of tests/test_kernel_resources.py)
    assert any('6k_bandILi' in n for n in recs)              # (the chain's records were read too)
