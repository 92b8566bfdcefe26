#!/bin/bash
# Diagnostic build of the product sources with in-kernel time stamps (-DVRG_STAMPS) for tools/chain_stamps.py:
#   arterynetwork_amd/csrc/libvrg_hip_stamps.so   (never loaded by the package; VRG_HIP_LIB selects it)
cd "$(dirname "$0")/.." && python3 -m arterynetwork_amd.build --define VRG_STAMPS --out libvrg_hip_stamps.so
