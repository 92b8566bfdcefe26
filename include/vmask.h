/*
 * vmask.h - C-ABI (in libvrg_hip.so) of the voxel passes on either side of the VRG stage
 * (SURVEY.md section 8 rows f2-f4): what Code/generateVesselVolume.py and its consumers do with
 * scipy / scikit-image on the CPU, as HIP kernels on MI355X.
 *
 *   vmask_edt          scipy.ndimage.distance_transform_edt(mask)       generateVesselVolume.py:183,
 *                                                                       manualCorrectionGUI.py:248 (vessel radii)
 *   vmask_label        skimage.measure.label(volume, return_num=True, connectivity=maxHop) + np.bincount
 *                                                                       generateVesselVolume.py:107-136 (labelVolume),
 *                                                                       skeletonization.py:108
 *   vmask_vessel_mask  the threshold / component-size pipeline of       generateVesselVolume.py:187-199
 *   vmask_skeleton     the curve skeleton that skeletonization.py:148-162 gets from an external tool and saves as
 *                      skeleton.nii.gz (:783-790); here: subfield-sequential thinning, DESIGN.md section 9
 *   vmask_segments     the branches that skeletonization.py keeps as segmentList.npz / graphRepresentation.graphml
 *                      (:745-794): the 26-adjacency graph of the skeleton voxels traced into segments that end at voxels
 *                      of degree != 2 and run through voxels of degree 2 (the contract of validateSegment :649-680 and
 *                      getSegmentListDetail :565-601), in one canonical orientation and order; DESIGN.md section 9.
 *                      Claimed: exact equality with the sequential model tests/segment_model.py.  Not claimed: agreement
 *                      with the external tool's segments, junction clusters merged into single nodes.
 *
 * All arrays are dense C-order [n0][n1][n2] (the caller's own axis order; numbering of components
 * follows that raster order exactly as skimage / scipy do).  Pointers may be host or device pointers.
 * Return 0 on success, negative VRG_E_* codes of vrg.h otherwise.
 */
#ifndef VMASK_H
#define VMASK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[v] = Euclidean distance (unit sampling) from v to the nearest voxel with mask == 0; 0 where mask == 0.
 * mask: uint8.  out: float64, like scipy returns. */
int vmask_edt(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, double* out);

/* Connected components of volume != 0 with skimage's `connectivity` 1 (6), 2 (18) or 3 (26 neighbours).
 * labels: int32, 0 = background, components 1..n numbered in raster order of their first voxel.
 * sizes (optional, capacity cap): voxel count of component k at sizes[k-1]; *n receives the component count. */
int vmask_label(int device, const uint8_t* volume, int64_t n0, int64_t n1, int64_t n2, int connectivity,
                int32_t* labels, int64_t* sizes, int64_t cap, int64_t* n);

/* generateVesselVolume.py:187-199 in one call:
 *   lo = min(vesselness), hi = max(vesselness)
 *   v2 = vesselness;  v2[(edt(brainMask) <= edt_max) & (v2 <= lo + frac1*(hi-lo))] = 0      (:187-189)
 *   v2[v2 <= lo + frac2*(hi-lo)] = 0                                                          (:190-191)
 *   v2 = (v2 != 0);  drop 26-connected components with size <= min_size                       (:194-199)
 * vesselness: float32 or float64 (dtype VRG_F32 / VRG_F64).  out: uint8 0/1.  *kept receives the voxel count. */
int vmask_vessel_mask(int device, const uint8_t* brainMask, const void* vesselness, int dtype,
                      int64_t n0, int64_t n1, int64_t n2, double edt_max, double frac1, double frac2,
                      int64_t min_size, uint8_t* out, int64_t* kept);

/* Curve skeleton of volume != 0 by subfield-sequential thinning.  out: uint8 0/1.
 * *kept = voxels left, *cycles = cycles run (either may be NULL). */
int vmask_skeleton(int device, const uint8_t* volume, int64_t n0, int64_t n1, int64_t n2,
                   uint8_t* out, int64_t* kept, int64_t* cycles);

/* The segments of the 26-adjacency graph of skeleton != 0 (any volume, not only a thinned one; outside is background).
 * deg(v) = object voxels among v's 26 neighbours; node: deg != 2, path voxel: deg == 2.  Segments: every pair of adjacent
 * nodes [a, b]; every maximal run of path voxels with the nodes at its ends [a, p1 .. pk, b] (a == b allowed); every
 * component of path voxels only, closed through its voxel m of smallest index [m, .., m].  Canonical form: idx(first) <
 * idx(last), or idx(second) < idx(second-to-last) when first == last; segments ascending by (idx(first), idx(second)).
 * counts[0] segments, [1] total voxel entries (= offsets[nseg]), [2] nodes (deg != 2, isolated included),
 * [3] isolated voxels, [4] pointer-jumping rounds run.
 * offsets == NULL && voxels == NULL: counts only.  Otherwise offsets has cap_seg + 1 and voxels cap_vox int64 slots;
 * too small a capacity: VRG_E_ARG with the needed sizes in counts, nothing written.
 * voxels: C-order linear indices; segment k = voxels[offsets[k] .. offsets[k+1]) in the canonical form and order. */
int vmask_segments(int device, const uint8_t* skeleton, int64_t n0, int64_t n1, int64_t n2,
                   int64_t* counts, int64_t* offsets, int64_t cap_seg, int64_t* voxels, int64_t cap_vox);

const char* vmask_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
