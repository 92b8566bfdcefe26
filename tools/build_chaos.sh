#!/bin/bash
# Diagnostic build of the product sources with random delays at every kernel entry and hand-off (-DVRG_CHAOS) for the interleaving campaign of tools/gpu.sh <tag> chaos:
#   arterynetwork_amd/csrc/libvrg_hip_chaos.so   (never loaded by the package; VRG_HIP_LIB selects it)
cd "$(dirname "$0")/.." && python3 -m arterynetwork_amd.build --define VRG_CHAOS --out libvrg_hip_chaos.so
