"""arterynetwork_amd - MI355X-native variational region growing (the hot path of zjx1805/ArteryNetwork).

Only what that path needs: csrc/ (HIP kernels + C-ABI, include/vrg.h), the ctypes binding, the Python
mirror of the reference function, synthetic phantoms, and the Z-slab multi-GPU driver.
"""
from .variationalRegionGrowing import variationalRegionGrowing  # noqa: F401
from .vesselness import vesselnessFilter, sigmasFromDiameters  # noqa: F401
from .denoise import anisotropicDiffusion, medianFilter  # noqa: F401
from .bias import biasFieldCorrection, logBiasField  # noqa: F401
from .registration import register, resample  # noqa: F401
from .brain import brainExtraction  # noqa: F401
from .skeletonization import branchTerritories, territoryVolumes, geodesicTerritories  # noqa: F401
from .skeletonization import branchMorphometry, BranchMorphometry, deriveMorphometry, pathLengths, writeMorphometry  # noqa: F401
from .skeletonization import partitionCompartments, Compartments, compartmentTerritories, compartmentSummary, writeCompartments  # noqa: F401
from .geodesic import geodesicDistance  # noqa: F401
from .reconnect import bridgeCandidates, selectBridges, applyBridges, vesselCost, tipRegions, Bridges  # noqa: F401  (reconnect.reconnect keeps the module's name free)
from .flow import simulateFlow, FlowResult, branchResistance, terminalPressures, referenceResiduals  # noqa: F401

__all__ = ['variationalRegionGrowing', 'vesselnessFilter', 'sigmasFromDiameters', 'anisotropicDiffusion', 'medianFilter', 'biasFieldCorrection', 'logBiasField', 'register', 'resample', 'brainExtraction',
           'branchTerritories', 'territoryVolumes',
           'geodesicTerritories', 'geodesicDistance', 'branchMorphometry', 'BranchMorphometry', 'deriveMorphometry', 'pathLengths', 'writeMorphometry',
           'partitionCompartments', 'Compartments', 'compartmentTerritories', 'compartmentSummary', 'writeCompartments',
           'bridgeCandidates', 'selectBridges', 'applyBridges', 'vesselCost', 'tipRegions', 'Bridges',
           'simulateFlow', 'FlowResult', 'branchResistance', 'terminalPressures', 'referenceResiduals']
