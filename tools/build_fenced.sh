#!/bin/bash
# The FENCED TWIN of the product sources (-DVRG_FENCES: every poll and ticket an acquire, every announcing store and ticket a release, a release fence where the
# product only drains - vrg_items.h "backend shims") for the A/B of tools/gpu.sh <tag> fenced:
#   arterynetwork_amd/csrc/libvrg_hip_fenced.so   (never loaded by the package; VRG_HIP_LIB selects it)
cd "$(dirname "$0")/.." && python3 -m arterynetwork_amd.build --define VRG_FENCES --out libvrg_hip_fenced.so
