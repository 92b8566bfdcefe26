/*
 * vmask.h - C-ABI (in libvrg_hip.so) of the voxel passes on either side of the VRG stage
 * (DESIGN.md section 9 rows f5-f14): what Code/generateVesselVolume.py and its consumers do with
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
 *                      with the external tool's segments.  Junction clusters are not merged here: vmask_branches does that.
 *   vmask_vesselness   the multiscale Hessian vesselness filter whose output the pipeline reads as vesselnessFiltered.nii.gz
 *                      (generateVesselVolume.py:170) and the reference's README.md:61-67 leaves to an external GUI tool:
 *                      Frangi's measure by the definition below.  Claimed: agreement to 1e-9 with
 *                      the float64 scipy / numpy model tests/vesselness_model.py outside the measure's one discontinuity.
 *                      Not claimed: agreement with the external tool's output (its discretisation differs).
 *   vmask_territories  what carries the branches back to the voxels: the reference can give a branch's volume only as a cylinder
 *                      (fluidSimulation.py:814-842) and keeps a hand-maintained indexVolume of centre voxels
 *                      (manualCorrectionGUIDetail.py); here every voxel of the mask gets the label of the segment that owns its
 *                      nearest skeleton voxel and every segment its voxel count: an exact Euclidean feature transform, DESIGN.md
 *                      section 9, f8.  Claimed: exact equality - labels, nearest, sizes - with the brute-force model
 *                      tests/territory_model.py, the tie rule below included; bit-identical repeats.  Not claimed: geodesic
 *                      (inside-the-mask) nearness - where two vessels touch, a voxel can go to the neighbour's centre line -,
 *                      anisotropic spacing, any per-branch quantity other than the voxel count (vmask_geodesic supplies the
 *                      first two).
 *   vmask_geodesic     path length from chosen voxels through the vessels for every voxel of the mask - the "depth" of
 *                      partitionCompartmentGUI.py and the "path length" of fluidSimulation.py's terminating-pressure relation,
 *                      which the reference computes on the centre-line graph only - and the territories by nearness inside the
 *                      mask, in the volume's spacing: shortest paths in the 26-adjacency graph of the mask's voxels by a
 *                      block-based label-correcting iteration, DESIGN.md section 9, f9.  Claimed: exact equality - the bits of
 *                      dist, labels, sizes - with the Dijkstra model tests/geodesic_model.py; bit-identical repeats.  Not
 *                      claimed: sub-voxel (eikonal) distances, connectivities other than 26, seeds outside the mask, agreement
 *                      with the reference's graph-level depth.
 *   vmask_branches     the "simple branches" that the reference's processSegments / validateSegment expect of segmentList and
 *                      that it reaches by hand in a GUI: the segments of vmask_segments with every cluster of junction voxels
 *                      merged into one node, and short spurs pruned by a stated rule; DESIGN.md section 9, f10.  Claimed: exact
 *                      equality - skeleton, tables, counts - with the sequential model tests/branch_model.py; bit-identical
 *                      repeats.  Not claimed: pass-through clusters dissolved, agreement with the external tool's segments,
 *                      spur lengths in physical units, any per-branch quantity (vmask_morphometry supplies those).
 *   vmask_morphometry  what the reference's calculateBranchInfo (manualCorrectionGUI.py:215-385) and calculateProperty
 *                      (graphRelated.py:35-400) compute with networkx and Python loops over every voxel of every segment: per
 *                      branch the step counts that give its path length, the chord, the sums of the radius sample and the end
 *                      directions; per node the radius and the three incident branches; from roots the path distance, the
 *                      parent branch and the depth of every node; DESIGN.md section 9, f11.  Claimed: exact equality - every
 *                      integer, the bits of every float64 sum - with the sequential model tests/morphometry_model.py;
 *                      bit-identical repeats.  Not claimed: the reference's spline-based local directions and curvature,
 *                      anything derived from these outputs (the Python layer's host formulas).
 *   vmask_compartments the reference's compartment partition (myFunctions.randomWalkBFS, partitionCompartmentGUIDetail.py:316-343):
 *                      the branch graph walked from every compartment's initial voxels without stepping onto one of its boundary
 *                      voxels - per entry, node and branch the owning compartment, the depth and the level; DESIGN.md section 9,
 *                      f12.  Claimed: exact equality - every output is an integer - with the sequential model
 *                      tests/compartment_model.py; bit-identical repeats.  Not claimed: the reference's list order, its
 *                      order-dependent depthLevel and segmentIndexList in loops, voxels of a cluster other than the
 *                      representative, per-compartment flow quantities.
 *   vmask_flow         the network solve of the reference's fluidSimulation.py (computeNetworkDetail's equations, :4636-4728) as a
 *                      signed solve: the pressures at the free nodes and the flow in every branch for S scenarios of one graph in
 *                      one launch; DESIGN.md section 9, f13.  Claimed: at k == 1 bit equality with tests/flow_model.py, iteration
 *                      counts included; at k != 1 the stated residual and a measured distance to a direct solver; bit-identical
 *                      repeats.  Not claimed: the reference's optimiser and weights, its distributeFlow mode, pulsatile flow.
 *   vmask_diffuse      the "MR image denoising" step that the reference's README (Pre-processing) leaves to an external GUI tool, in
 *                      front of vmask_vesselness: explicit Perona-Malik diffusion over the 6 neighbours in float64 by the
 *                      definition below; DESIGN.md section 9, f14.  Claimed: with the rational conductance bit equality with
 *                      the numpy restatement tests/denoise_model.py, with the exponential one agreement to 1e-9 of the input's
 *                      span (the device's exp); bit-identical repeats.  Not claimed: agreement with the external tool's
 *                      filters (their discretisation differs and they rescale K every step), an automatic K.
 *   vmask_median       the median over a window of at most 3 x 3 x 3 voxels, scipy.ndimage.median_filter(mode='nearest'); it
 *                      keeps the value set of integer data.  Claimed: equality with scipy as numbers.  Not claimed: wider
 *                      windows.
 *   vmask_bias_*       the "MR image bias field correction" step that the reference's README (Pre-processing) leaves to an external
 *                      tool, in front of vmask_diffuse: an N4-style estimate by the definition below - log domain, histogram
 *                      sharpening by Wiener deconvolution, an incremental cubic B-spline fit of the residual over a lattice
 *                      that doubles per level; DESIGN.md section 9, f15.  Claimed: bit equality of the fit, the evaluation and
 *                      the whole loop (field, trace and iteration counts) with the numpy restatement tests/bias_model.py, the
 *                      model taking its sharpening map from vmask_bias_sharpen; that map within a measured rounding distance of
 *                      an np.fft restatement; the corrected volume and the field within a measured distance of the model (the
 *                      device's log and exp); bit-identical repeats.  Not claimed: agreement with ITK / Slicer (their
 *                      linear-weight histogram, shrink factor, lattice refinement and convergence measure all differ).
 *   vmask_reg_*        the "register multiple sets of images" step that the reference's README (Usage, step 1) leaves to FSL flirt:
 *                      what a rigid / affine registration evaluates on the device - the joint histogram of the fixed volume's bins
 *                      and the moving volume sampled through an affine voxel map, the block-mean pyramid, the resampled volume -
 *                      and the host-only cost of a histogram, by the definition below; DESIGN.md section 9, f16.  Claimed: equality of
 *                      the integer counts, and bit equality of the extrema, bin images, pyramids and resampled volumes, with the
 *                      numpy restatement tests/registration_model.py; the corratio cost bit-equal to its restatement, mi and nmi
 *                      within a measured distance (the host's log); bit-identical repeats.  Not claimed: agreement with flirt
 *                      (its smoothing, partial-volume weights, optimiser and matrix convention all differ).
 *   vmask_warp_*       the nonlinear part of the same step, which the README leaves to FSL fnirt: a displacement field on the fixed
 *                      grid refined by demons forces (sum of squared differences after a linear intensity scaling) that a
 *                      multilevel cubic B-spline fit smooths, the fit and the evaluation those of vmask_bias_*, the sample that of
 *                      vmask_reg_*; DESIGN.md section 9, f18.  Claimed: bit equality of the force pass, the three-numerator fit,
 *                      the upsampled and the final warp, the trace and the resampled volumes with the numpy restatement
 *                      tests/warp_model.py; a measured recovery of a known deformation; bit-identical repeats.  Not claimed:
 *                      agreement with fnirt, cross-modality costs, a diffeomorphic or invertible warp.
 *   vmask_bridge       the "Reconnect" operation of the reference's manual-correction GUI (manualCorrectionGUIDetail.py:739-951, Usage
 *                      step 5), which joins two branches across a gap along a spline that the user anchors by four clicks; here,
 *                      with no GUI: for every two components of the vessel mask the cheapest path between them through a cost
 *                      volume (derived from vesselness), within a bound on the cost; DESIGN.md section 9, f19.  Claimed: exact
 *                      equality - the bits of dist, root, pred, costs, every integer - with the Jacobi model
 *                      tests/bridge_model.py, which a heap Dijkstra beside it confirms; bit-identical repeats.  Not claimed: the
 *                      reference's spline geometry, its Grow and Cut, sub-voxel paths, bridges inside one component; which
 *                      bridges to take is the Python layer's decision (reconnect.selectBridges).
 *   vmask_tubes        the way back from the graph to the voxels: the reference's manual-correction step edits centre lines only
 *                      ("the ability to directly modify the 3D segmentation volume might be added in the future") and gives a
 *                      branch's volume only as a cylinder (getVolumePerPartition, fluidSimulation.py:814-842); vmask_territories
 *                      and vmask_geodesic label the voxels of a given mask.  Here the branch table itself - sub-voxel centre points
 *                      and radii - is rasterised: every voxel gets the branch whose swept ball it lies deepest in, every branch its
 *                      voxel count and how many of them a given mask has; DESIGN.md section 9, f21.  Claimed: exact equality - the
 *                      bits of label, field, nearest, every count - with the brute-force model tests/tube_model.py, the tie rule
 *                      included; bit-identical repeats.  Not claimed: anti-aliased (partial-volume) voxels, any treatment of
 *                      junctions beyond the union of the tubes, the reference's cylinder volumes, any smoothing of the radii.
 *
 * All arrays are dense C-order [n0][n1][n2] (the caller's own axis order; numbering of components
 * follows that raster order exactly as skimage / scipy do).  Pointers may be host or device pointers.
 * Return 0 on success, negative VRG_E_* codes of vrg.h otherwise.  A device allocation that fails is VRG_E_MEM in every call,
 * vmask_edt, vmask_label, vmask_vessel_mask and vmask_skeleton included (they used to report some of theirs as VRG_E_INTERNAL),
 * with a text that begins "out of device memory"; whatever the call allocated is freed on every return.
 */
#ifndef VMASK_H
#define VMASK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[v] = Euclidean distance (unit sampling) from v to the nearest voxel with mask == 0; 0 where mask == 0.
 * mask: uint8.  out: float64, like scipy returns: the correctly rounded root of the exact integer squared distance, for every
 * shape that is accepted (extents <= 32000, fewer than 2^31 voxels), distances of sqrt(2^29) and more included.
 * Inside, "no zero voxel on this line" is a sentinel above every real squared distance of the arithmetic width in use: 2^29
 * where n0^2 + n1^2 + n2^2 < 2^29 (32-bit arithmetic), 2^32 - 1 otherwise (64-bit arithmetic on unsigned 32-bit values; a real
 * squared distance is at most 3 * 31999^2 < 2^32).  A mask without any zero voxel has no distance transform: out is then the
 * root of the sentinel everywhere, which is unspecified (scipy's answer for it is arbitrary too). */
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

/* Frangi vesselness (Frangi et al. 1998) of a 3-D volume I, the maximum over nsig scales; float64 from the taps to the
 * measure (float32 is an input type only).  Input voxels are assumed finite.
 *
 * Taps: for a physical scale sigma and axis a with spacing h_a (spacing == NULL: 1 1 1): s = sigma / h_a, r = int(4 s + 0.5);
 * on x = -r .. r: phi = exp(-x^2 / 2 s^2) / sum, phi' = -x / s^2 phi, phi'' = (x^2 / s^4 - 1 / s^2) phi.  The operation is
 * convolution (not correlation) with indices clamped at the volume's faces - scipy.ndimage.gaussian_filter(I, s per axis,
 * order, mode='nearest', truncate=4.0) in float64.  A radius larger than an extent is legal.
 * Hessian: H_ab = sigma^2 (d_a d_b G_sigma * I) / (h_a h_b).
 * Measure: the eigenvalues of H ordered |l1| <= |l2| <= |l3|; V_sigma = 0 unless l2 < 0 and l3 < 0 (bright == 0: l2 > 0 and
 * l3 > 0), otherwise (1 - exp(-RA^2 / 2 alpha^2)) exp(-RB^2 / 2 beta^2) (1 - exp(-S^2 / 2 gamma^2)) with RA = |l2| / |l3|,
 * RB = |l1| / sqrt(|l2 l3|), S^2 = l1^2 + l2^2 + l3^2.
 * gamma > 0 is used for every scale; gamma <= 0 is automatic: per scale half the largest Frobenius norm of H_sigma over the
 * volume (over the voxels with mask != 0 when a mask is given); a scale whose gamma is 0 contributes 0.
 * out: float64, max over the scales of V_sigma, 0 where mask == 0.  scale (optional, uint8): index of the first scale that
 * attains the maximum, 0 where out is 0.  gammas_used (optional, nsig, host): the gamma of every scale.
 * volume: VRG_F32 or VRG_F64.  VRG_E_ARG: nsig outside 1..32; a sigma or spacing not finite and positive; a radius r < 1 or
 * r > 64 on any axis; alpha or beta not finite and positive; a shape outside the envelope of the other passes.
 * VRG_E_MEM: the input, the output and nine float64 volumes do not fit the device (volumes are not processed in slabs);
 * everything allocated is freed. */
int vmask_vesselness(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const uint8_t* mask,
                     const double* sigmas, int nsig, const double* spacing, double alpha, double beta, double gamma, int bright,
                     double* out, uint8_t* scale, double* gammas_used);

/* Branch territories.  mask, skeleton: uint8 volumes; offsets[nseg + 1] and voxels[offsets[nseg]]: what vmask_segments returned
 * for that skeleton (C-order linear indices; idx below is that index).
 * Sites: all voxels with skeleton != 0; they need not lie in the mask.
 * Site label L(s) = 1 + the smallest k such that s occurs in segment k (a node shared by several segments belongs to the one of
 * smallest index); 0 for a skeleton voxel that occurs in no segment (the isolated voxels, which vmask_segments only counts).
 * Nearest site N(v) of a voxel with mask != 0: the site of smallest squared Euclidean distance (unit sampling, integers); AMONG
 * EQUIDISTANT SITES THE ONE OF SMALLEST idx WINS; with no site at all N(v) = -1.
 * labels (int32): L(N(v)) inside the mask; 0 outside the mask and where N(v) = -1.  Label 0 inside the mask therefore means:
 * no site, or the nearest site belongs to no segment.
 * nearest (int64, may be NULL): idx(N(v)); -1 outside the mask or where there is no site.
 * sizes (int64, nseg + 1): sizes[l] = number of mask voxels with label l (sizes[0]: the in-mask voxels left unassigned); the sum
 * equals the mask's voxel count.  The output is a pure function of the inputs; repeated runs are bit-identical.
 * nseg == 0 is legal (offsets and voxels may then be NULL): every label is 0.
 * VRG_E_ARG: an entry of voxels that is not a skeleton voxel or lies outside the volume, offsets that do not start at 0 or
 * descend (counted on the device; nothing is written); a shape outside the envelope of the other passes.
 * VRG_E_MEM: the volume does not fit the device - 20 bytes per voxel of work space beside the two inputs and the outputs (up to
 * 34 in all with host arrays and nearest); everything allocated is freed. */
int vmask_territories(int device, const uint8_t* mask, const uint8_t* skeleton, int64_t n0, int64_t n1, int64_t n2,
                      const int64_t* offsets, int64_t nseg, const int64_t* voxels,
                      int32_t* labels, int64_t* nearest /* may be NULL */, int64_t* sizes /* nseg + 1 */);

/* Geodesic distance and territories inside the mask.  mask: uint8 volume; idx = C-order linear index.
 * Graph: the vertices are the voxels with mask != 0, the edges join 26-neighbours that are both in the mask, an edge with the
 * offset delta weighs w(delta) = sqrt((delta0 h0)^2 + (delta1 h1)^2 + (delta2 h2)^2) for spacing = (h0, h1, h2) (NULL: 1 1 1):
 * a table of 26 values computed once on the host in float64, the squares summed in the order of the axes.
 * Seeds: seeds[nseed] (int64 idx values, every one a voxel of the mask) and seed_labels[nseed] (int32, 1 .. max_label; NULL: all
 * 1).  Several entries may name one voxel: THE SMALLEST LABEL HOLDS.  nseed == 0 is legal (seeds may then be NULL).
 * dist (float64, may be NULL): D(s) = 0 at the seeds; elsewhere in the mask D(v) = min over in-mask neighbours u of
 * fl(D(u) + w(u - v)), fl the IEEE double addition - the least fixed point, which is what Dijkstra's algorithm computes with the
 * same addition (fl(a + w) is monotone in a).  +inf at a mask voxel that no seed reaches, -1 outside the mask.
 * labels (int32, may be NULL): Lab(seed) = its label; for every other voxel with finite D, Lab(v) = min{ Lab(u) : u an in-mask
 * neighbour with fl(D(u) + w(u - v)) == D(v) } (well founded: w > 0, so D(u) < D(v)).  WHERE PATHS OF EQUAL LENGTH ARRIVE FROM
 * SEEDS OF DIFFERENT LABELS THE SMALLEST LABEL WINS - not the smallest idx, unlike vmask_territories.  0 outside the mask and
 * where D = +inf.
 * sizes (int64, max_label + 1, may be NULL): sizes[l] = number of mask voxels with label l, sizes[0] the unreached ones; the sum
 * equals the mask's voxel count.
 * counts (int64, 5, may be NULL): [0] mask voxels, [1] reached voxels (finite D), [2] occupied 8x8x8 bricks, [3] distance
 * rounds, [4] label rounds (0 when neither labels nor sizes is asked for).
 * dist, labels, sizes and counts[0..2] are a pure function of the inputs, bit-identical between runs; the round counts describe
 * the run, not the result.
 * VRG_E_ARG: a seed outside the volume or on a voxel with mask == 0, a label < 1 or > max_label (counted on the device before
 * anything is written); a spacing that is not finite and positive, or with max / min > 1000 (the bound keeps fl(D + w) > D for
 * every D inside the shape envelope); a shape outside the envelope of the other passes.  Nothing is written then.
 * VRG_E_MEM: the mask, 4 bytes per brick of the volume and 6160 bytes per occupied brick (4112 without labels) do not fit the
 * device, or the dense outputs where they are host arrays (12 bytes per voxel); everything allocated is freed. */
int vmask_geodesic(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2,
                   const int64_t* seeds, const int32_t* seed_labels /* may be NULL */, int64_t nseed,
                   const double* spacing /* may be NULL */,
                   double* dist /* may be NULL */, int32_t* labels /* may be NULL */,
                   int64_t* sizes /* may be NULL */, int64_t max_label, int64_t* counts /* may be NULL */);

/* The branch graph.  S = the voxels != 0 of volume (any volume; outside is background); deg, node, path voxel, idx and the
 * segments of S exactly as vmask_segments defines them.
 * Junction voxel: deg >= 3.  Cluster: a 26-connected component of junction voxels; its representative is the member of largest
 * deg, among those the one of smallest idx.
 * Nodes: the clusters and the end points (deg == 1; its own representative), numbered ascending by idx(representative).
 * Branches: every segment of S other than the two-voxel segments whose two voxels lie in one cluster, in the segments' order.
 * A branch's voxels are the segment's, with the node's representative put in front / behind where the end voxel is not the
 * representative itself (consecutive entries are 26-adjacent except possibly the first and the last pair inside a cluster that
 * is no clique); its ends are the two node ids, -1 -1 for a closed curve that touches no node; its length L = the segment's
 * voxel count - 1.  Isolated voxels are only counted.  A cluster with exactly two branch ends stays a node (counted as
 * pass_through).
 * Spur: a branch with an end point at one end and a cluster C at the other, and
 *     L <= min_len || (dist && (double)L <= radius_factor * dist[idx(rep(C))])      (one IEEE multiply, one compare).
 * A pruning round selects per cluster at most one spur - smallest L, then smallest branch index -, clears every voxel of the
 * selected segments but the one that belongs to C, thins the volume again (vmask_skeleton, end points kept) and rebuilds the
 * graph.  Pruning stops at the first round that selects nothing, or after max_rounds rounds.  With min_len == 0 and no dist
 * nothing is pruned and the thinning never runs.
 * skeleton (uint8, may be NULL): the volume after pruning, 0/1.  dist (float64 volume, may be NULL): typically vmask_edt(mask).
 * counts (12): [0] nodes, [1] clusters, [2] end points, [3] pass_through clusters, [4] branches, [5] voxel entries
 * (= offsets[branches]), [6] isolated voxels, [7] intra-cluster segments dropped, [8] pruning rounds that removed something,
 * [9] spurs removed, [10] voxels removed by the spur deletions (the thinning's deletions not included), [11] cluster-labelling
 * rounds of the last graph build (describes the run, not the result).
 * nodes (cap_node x 4: idx(representative), kind 0 end point / 1 cluster, member count, branch ends incident - a loop counts
 * twice), branch_ends (cap_branch x 2), offsets (cap_branch + 1), voxels (cap_vox): all four NULL = counts (and skeleton) only;
 * too small a capacity: VRG_E_ARG with the needed sizes in counts, nothing else written.
 * Everything but counts[11] is a pure function of the inputs, bit-identical between runs.
 * VRG_E_ARG: min_len, max_rounds or radius_factor negative, radius_factor not finite; a shape outside the envelope of the
 * other passes.  VRG_E_MEM: device memory does not fit - the volume, dist where it is a host array, up to 80 bytes per object
 * voxel, 44 per segment, 8 per segment entry, and what vmask_segments and vmask_skeleton take while they run; everything
 * allocated is freed. */
int vmask_branches(int device, const uint8_t* volume, int64_t n0, int64_t n1, int64_t n2,
                   int64_t min_len, double radius_factor, const double* dist /* may be NULL */, int64_t max_rounds,
                   uint8_t* skeleton /* may be NULL */, int64_t* counts,
                   int64_t* nodes, int64_t cap_node, int64_t* branch_ends, int64_t* offsets, int64_t cap_branch,
                   int64_t* voxels, int64_t cap_vox);

/* Branch morphometry.  The shape of the volume; dist (float64 volume, non-negative, typically vmask_edt(mask)); the branch table
 * that vmask_branches returned for a volume of that shape: offsets[nbranch + 1], voxels[offsets[nbranch]] (C-order linear
 * indices), branch_ends[2 nbranch] (node ids, -1 -1 for a closed curve), node_voxel[nnode] (idx of the representatives).
 * spacing (h0, h1, h2; NULL: 1 1 1; host or device), roots[nroots] (node ids, nroots >= 0), local_steps >= 1.
 * Branch b has n = offsets[b + 1] - offsets[b] >= 2 entries e_0 .. e_(n-1); a pair is two consecutive entries, its offset
 * d = e_(i+1) - e_i in voxel coordinates.
 * branch_int (nbranch x 24, int64):
 *   [0..6]   stepCounts: the pairs with (|d0|, |d1|, |d2|) in {0,1}^3 \ 0, at the class index 4 |d0| + 2 |d1| + |d2| - 1
 *   [7]      jumps: every other pair (not 26-adjacent - the first or last pair inside a cluster that is no clique - or twice the
 *            same voxel)
 *   [8..13]  jumpOffset [2][3]: front = d of the pair (e_0, e_1) where it is a jump, back = d of the pair (e_(n-2), e_(n-1))
 *            where it is a jump and n > 2; 0 0 0 otherwise.  A jump elsewhere is counted in [7] only.
 *   [14]     radiusCount m: the radius sample is dist at the interior entries e_1 .. e_(n-2) for n >= 3 (m = n - 2), at both
 *            entries for n == 2 (m = 2)
 *   [15..20] endDir [2][3]: with k = min(local_steps, n - 1): e_k - e_0, then e_(n-1-k) - e_(n-1)
 *   [21..23] chord: e_(n-1) - e_0
 * branch_f64 (nbranch x 5, float64): [0] radiusSum, [1] radiusDevSq = sum of (r - mean)^2 with mean = fl(radiusSum / m),
 *   [2] radiusMin, [3] radiusMax, [4] pathLength.
 * THE ORDER OF THE TWO SUMS, for the values x_0 .. x_(m-1) in the sample's order (every operation one IEEE double operation,
 * nothing contracted into an FMA, no floating-point atomics):
 *   1. for j in [0, 64): a_j = ((x_j + x_(j+64)) + x_(j+128)) + ..; 0.0 where there is no x_j
 *   2. for s = 32, 16, 8, 4, 2, 1: a_j <- a_j + a_(j xor s), all j at once
 *   3. the sum is a_0.
 * radiusDevSq sums fl(fl(x_i - mean) * fl(x_i - mean)) in the same order; a NaN result (an infinite radius) is stored as the
 * quiet NaN 0x7ff8000000000000.  (A branch of at most 17 entries is summed by 16 lanes: steps 32 and 16 would add 0.0.)
 * pathLength = ((..(0 + stepCounts[0] w_0) + ..) + stepCounts[6] w_6) + |front| + |back| on the host: w_c = sqrt((g0^2 + g1^2) +
 * g2^2) with g_a = h_a where bit a of the class is set (d0 the bit of weight 4) and 0 elsewhere; a jump's length is the same
 * expression of g_a = jumpOffset_a h_a.
 * node_radius (nnode): dist[node_voxel].  incident (nnode x 3, int64): where exactly three branch ends meet at the node and
 * they belong to three distinct branches: 2 branch + end (end 0: the branch starts here, 1: it ends here), ascending; -1 -1 -1
 * otherwise.  entry_radius (offsets[nbranch], may be NULL): dist at every entry.
 * With nroots > 0 (otherwise these three are not touched and may be NULL), w_b = pathLength[b]:
 *   path_distance (nnode, float64): D(root) = 0; elsewhere D(v) = min over the branches b between u and v, u != v, of
 *     fl(D(u) + w_b) - the least fixed point, which Dijkstra's algorithm computes with the same addition; +inf where no root is
 *     reached.  Closed curves and loops on one node relax nothing.  Computed in rounds of one thread per branch with 64-bit
 *     atomicMin on the bit patterns (non-negative doubles order as their bits) until a round lowers nothing; more than
 *     max(nnode, 1) rounds: VRG_E_INTERNAL.
 *   node_depth (nnode x 3, int64): [0] parentBranch = the smallest b with fl(D(u) + w_b) == D(v) and D(u) < D(v), -1 at roots
 *     and unreached nodes; [1] depthLevel = depthLevel(u) + 1 and [2] depthVoxel = depthVoxel(u) + (n_b - 1) along
 *     parentBranch, 0 at the roots, -1 at unreached nodes.
 *   branch_level (nbranch): the larger depthLevel of the branch's ends, -1 where either is unreached or the branch has none.
 * counts (2, may be NULL): [0] depthRounds (distance rounds run), [1] level rounds run - they describe the run, not the result.
 * Everything else is a pure function of the inputs, bit-identical between runs.
 * VRG_E_ARG, before anything is written: a spacing that is not finite and positive or with max / min > 1000 (as
 * vmask_geodesic); local_steps < 1; a negative count; offsets that do not start at 0 or leave a branch fewer than two entries,
 * a voxel outside the volume, an end or root that is no node id (counted on the device); a shape outside the envelope of the
 * other passes.  VRG_E_MEM: dist and the tables where they are host arrays, 232 bytes per branch and 28 per node do not fit
 * the device; everything allocated is freed. */
int vmask_morphometry(int device, int64_t n0, int64_t n1, int64_t n2, const double* dist,
                      const int64_t* offsets, int64_t nbranch, const int64_t* voxels, const int64_t* branch_ends,
                      const int64_t* node_voxel, int64_t nnode, const double* spacing /* may be NULL */,
                      const int64_t* roots, int64_t nroots, int64_t local_steps,
                      int64_t* branch_int, double* branch_f64, double* node_radius, int64_t* incident,
                      double* entry_radius /* may be NULL */,
                      double* path_distance, int64_t* node_depth, int64_t* branch_level, int64_t* counts /* may be NULL */);

/* The compartment partition: a bounded traversal of the branch graph.  The branch table is what vmask_branches returned for a
 * volume of the given shape (offsets[nbranch + 1], voxels[E], E = offsets[nbranch], branch_ends[2 nbranch], node_voxel[nnode]);
 * branch b has n_b >= 2 entries.
 * Vertices: the nnode nodes; every interior entry (b, i), 0 < i < n_b - 1; one private vertex per closed branch (ends -1 -1),
 * whose first and last entry are the same voxel.  Entry (b, 0) IS the node branch_ends[b][0], entry (b, n_b - 1) IS the node
 * branch_ends[b][1].  Edges: consecutive entries of a branch (a jump pair inside a cluster is one edge like any other).  The
 * voxel of a node is its representative; the other members of a junction cluster are no vertices.
 * Compartment c = 1 .. ncomp (1 <= ncomp <= 255) has two lists of C-order linear indices, the initial voxels
 * init_vox[init_off[c - 1] .. init_off[c]) and the boundary voxels bound_vox[bound_off[c - 1] .. bound_off[c]); duplicates are
 * allowed, an empty initial list reaches nothing.  A vertex is blocked in c when its voxel is a boundary voxel of c, initial
 * when it is an initial voxel of c.
 *   d_c(x)  the fewest edges from an initial vertex to x over paths with no blocked vertex; x is reached by c when there is one
 *           (the reference's depthVoxel; the reached set is its visitedVoxels as a set)
 *   l_c(x)  0 at the initial vertices; elsewhere the minimum over the unblocked neighbours y with d_c(y) = d_c(x) - 1 of
 *           l_c(y) + [x is a node] - end points count as nodes, a closed branch's private vertex does not.  On a tree this is
 *           the reference's depthLevel; in a loop the reference's value depends on list order, this one is the stated minimum.
 * Owner of a vertex: the c with the smallest (d_c(x), c) among those that reach it, 0 where none does.  Branch b belongs to c
 * when every one of its entries is owned by c (the reference's segmentIndexList on trees; a branch cut by a boundary voxel
 * belongs to nobody); its level is the minimum level of its entries (segmentLevel).  ncomp = 1 is the reference's independent
 * traversal of that compartment.
 * entry_comp / entry_depth / entry_level (E each), node_comp / node_depth / node_level (nnode each): the owner, and the depth
 * and level in the owner; -1 -1 without an owner.  branch_comp / branch_level (nbranch each): -1 where branch_comp is 0.
 * comp_counts ((ncomp + 1) x 3): row c: [0] vertices owned by c, [1] vertices reached by c, [2] branches with branch_comp == c;
 * row 0: [0] vertices owned by none, [1] vertices reached by two or more compartments, [2] all remaining branches.
 * counts (2, may be NULL): the depth rounds and the level rounds run - they describe the run, not the result.  Everything else
 * is a pure function of the inputs, bit-identical between runs.
 * Per (compartment, branch) pair one thread: a pass over the branch finds whether it has a blocked entry and the hops from
 * its initial entries to either end; the nodes' depths settle in label-correcting rounds with 64-bit integer atomicMin until
 * a round lowers nothing, then the levels over the tight predecessors in the same way (more than max(nnode, 1) + 1 rounds:
 * VRG_E_INTERNAL); a walk per pair fills the entries between the ends and the initial entries; the compartments are merged by
 * the key (depth, c).  No floating point.
 * VRG_E_ARG, before anything is written: ncomp outside [1, 255]; a list offset table that does not ascend from 0 (looked at on
 * the host: it says how much is read); and, counted on the device: a listed index outside the volume, a listed voxel that is
 * the voxel of no vertex, a voxel in both lists of one compartment, the table errors that vmask_morphometry refuses,
 * voxels[offsets[b]] != node_voxel[branch_ends[b][0]] and likewise at the last entry, a closed branch whose first and last
 * entry differ; a shape outside the envelope of the other passes.
 * VRG_E_MEM: the tables and outputs where they are host arrays, 17 bytes per (compartment, branch), 17 per (compartment, node)
 * and one per entry do not fit the device; everything allocated is freed. */
int vmask_compartments(int device, int64_t n0, int64_t n1, int64_t n2,
                       const int64_t* offsets, int64_t nbranch, const int64_t* voxels, const int64_t* branch_ends,
                       const int64_t* node_voxel, int64_t nnode,
                       int64_t ncomp, const int64_t* init_off, const int64_t* init_vox, const int64_t* bound_off, const int64_t* bound_vox,
                       uint8_t* entry_comp, int64_t* entry_depth, int64_t* entry_level,      /* E each */
                       uint8_t* node_comp, int64_t* node_depth, int64_t* node_level,         /* nnode each */
                       uint8_t* branch_comp, int64_t* branch_level,                          /* nbranch each */
                       int64_t* comp_counts /* (ncomp + 1) x 3 */, int64_t* counts /* 2, may be NULL */);

/* Centreline splines: one natural cubic smoothing spline (Reinsch) per branch, the three coordinates sharing one matrix.  The
 * shape of the volume and the branch table of vmask_branches: offsets[nbranch + 1], voxels[E], E = offsets[nbranch] (C-order
 * linear indices); spacing (h0, h1, h2; NULL: 1 1 1; host or device).  Every operation below is one IEEE double operation in the
 * order written, nothing contracted into an FMA, no floating-point atomics, division and square root correctly rounded.
 * |x| = sqrt((x0^2 + x1^2) + x2^2).  Branch b has n >= 2 entries e_0 .. e_(n-1) (voxel coordinates):
 *   y_i = (e_i - e_0) h per axis (the integer difference, then one product);  u_0 = 0, u_(i+1) = u_i + |y_(i+1) - y_i|;
 *   hh_i = u_(i+1) - u_i, r_i = 1 / hh_i;  w_0 = w_(n-1) = end_weight, w_i = 1 elsewhere, v_i = 1 / w_i.
 * The curve f minimises sum_i w_i |y_i - f(u_i)|^2 + lambda int |f''|^2 du over the natural cubic splines with knots u_i.  With
 * mu = 1 / lambda, m = n - 2, Q (n x m: column j = (r_j, -(r_j + r_(j+1)), r_(j+1)) in rows j, j + 1, j + 2) and R (m x m:
 * R_jj = (hh_j + hh_(j+1)) / 3, R_(j,j+1) = hh_(j+1) / 6) it solves the scaled system (mu R + Q' W^-1 Q) c = Q' y; g = y - W^-1 Q c are the
 * fitted positions, gamma = mu c (0 at both ends) the second derivatives at the knots.  For j in [0, m), s_j = r_j + r_(j+1):
 *   a0_j = ((r_j r_j) v_j + (s_j s_j) v_(j+1)) + (r_(j+1) r_(j+1)) v_(j+2)
 *   a1_j = -((s_j r_(j+1)) v_(j+1) + (r_(j+1) s_(j+1)) v_(j+2)) for j < m - 1;  a2_j = (r_(j+1) r_(j+2)) v_(j+2) for j < m - 2
 *   R0_j = (hh_j + hh_(j+1)) / 3, R1_j = hh_(j+1) / 6;  b_j = (y_(j+2) - y_(j+1)) r_(j+1) - (y_(j+1) - y_j) r_j per axis (this is Q' y)
 *   d0 = mu R0 + a0, d1 = mu R1 + a1, d2 = a2, factored L D L' by the forward recurrence, with L2_i = 0 for i < 2, L1_0 = 0, and 1
 *   for a D, 0 for a z' or c outside [0, m):
 *     L2_i = d2_(i-2) / D_(i-2);  L1_i = (d1_(i-1) - (L2_i D_(i-2)) L1_(i-1)) / D_(i-1);  D_i = (d0_i - (L1_i L1_i) D_(i-1)) - (L2_i L2_i) D_(i-2)
 *     z'_i = (b_i - L1_i z'_(i-1)) - L2_i z'_(i-2);  z_i = z'_i / D_i;  then downwards c_i = (z_i - L1_(i+1) c_(i+1)) - L2_(i+2) c_(i+2)
 *   q_i = r_(i-1) (c_(i-2) - c_(i-1)) + r_i (c_i - c_(i-1)) per axis, an r or c outside its range being 0 (this is (Q c)_i);
 *   e_i = v_i q_i, g_i = y_i - e_i, gamma_i = mu c_(i-1) for 0 < i < n - 1.
 *   The residual F(lambda) = the ORDERED SUM that vmask_morphometry states, of x_i = w_i ((e_i0^2 + e_i1^2) + e_i2^2), i = 0 .. n - 1.
 * n = 2 has no unknown: g = y, gamma = 0, F = 0.  n = 3 and 4 go through the same formulas (m = 1, 2).  A closed curve (first
 * entry = last entry) is fitted as an open curve with natural ends; no periodic spline.
 * LAMBDA.  l2 = ((h0^2 + h1^2) + h2^2) / 3, l = sqrt(l2), lambda_lo = 2^-24 (l2 l), lambda_hi = 2^24 (l2 l), on the host.
 *   smoothing > 0: lambda = smoothing (inside [lambda_lo, lambda_hi]); solves = 1, capped = 0.
 *   smoothing <= 0: the target is S = residual_per_point n.  F(lambda_hi) <= S, or n = 2: lambda = lambda_hi, solves = 1, capped = 1.
 *   Otherwise lo = lambda_lo, hi = lambda_hi and 24 times: mid = sqrt(lo hi); F(mid) > S ? hi = mid : lo = mid.  lambda = lo, solves =
 *   25 (the trial values; the fit at lambda is one more solve); capped = 2 when no trial moved lo and F(lambda_lo) > S, else 0.
 * entry_f64 (E x 11): [0] u_i; [1..3] position (e_0 h) + g_i; [4..6] the second derivative gamma_i; [7..9] the unit tangent d_i / |d_i|
 *   of the first derivative d_i = (g_(i+1) - g_i) / hh_i - (hh_i (2 gamma_i + gamma_(i+1))) / 6 on the right of knot i < n - 1, and at the last
 *   entry, with k = n - 2, (g_(k+1) - g_k) / hh_k + (hh_k (gamma_k + 2 gamma_(k+1))) / 6; [10] the curvature |d x gamma| / ((|d| |d|) |d|), the cross
 *   product being (d1 s2 - d2 s1, d2 s0 - d0 s2, d0 s1 - d1 s0).  A NaN is stored as 0x7ff8000000000000.
 * branch_f64 (nbranch x 5): [0] lambda, [1] the residual F(lambda), [2] splineLength, [3] maxCurvature, [4] meanCurvature.
 * branch_int (nbranch x 3): [0] solves, [1] capped, [2] samples.
 * THE SAMPLES.  U = u_(n-1); M = max(3, ceil(U / sample_step) + 1) samples at u_k = (k U) / (M - 1) for k < M - 1 and u_(M-1) = U.
 *   THE CUBIC at a parameter x: i = the last knot of 0 .. n - 2 with u_i <= x, t = x - u_i,
 *     P = g_i + t (d_i + t (0.5 gamma_i + t ((gamma_(i+1) - gamma_i) / (6 hh_i))))   per axis (centred on e_0 h, which no difference needs).
 *   chord_k = |P_(k+1) - P_k|, k in [0, M - 1): splineLength = their ordered sum.  Triangle k in [0, M - 2) of P_k, P_(k+1), P_(k+2): the sides
 *   |P_k - P_(k+1)|, |P_k - P_(k+2)|, |P_(k+1) - P_(k+2)| sorted a >= b >= c, t = (((a + (b + c)) (c - (a - b))) (c + (a - b))) (a + (b - c)),
 *   kappa_k = (t > 0 ? sqrt(t) : 0) / ((a b) c) - the 4 S / (a b c) of the reference's curvature_by_triangle, S = 0 where t < 0.  maxCurvature = the
 *   maximum (fmax from 0), meanCurvature = the ordered sum of kappa_0 .. kappa_(M-3), divided by M - 2.
 * lds_entries: the longest branch whose work arrays (15 doubles per entry) are kept in LDS, 0 = 256, at most 512; a longer
 * branch runs the same code over a global work space.  Every output is a pure function of the other inputs, bit-identical
 * between runs and whatever lds_entries is.  kernel_ms (host, may be NULL): the time of the kernels by hipEvents - it
 * describes the run, not the result.
 * VRG_E_ARG, before anything is written: the spacing rules of vmask_morphometry; end_weight not finite and positive; a NaN
 * smoothing or one > 0 outside [lambda_lo, lambda_hi]; in search mode a residual_per_point not finite and positive; sample_step
 * not finite or below 2^-10 l; lds_entries outside [0, 512]; offsets that do not start at 0 or leave a branch fewer than two
 * entries, a voxel outside the volume, two consecutive entries of a branch on the same voxel - a zero step - (counted on the
 * device); a shape outside the envelope of the other passes.  nbranch = 0 succeeds and writes nothing.
 * VRG_E_MEM: the tables and outputs where they are host arrays, and - only when a branch is longer than lds_entries - 120 bytes
 * per entry do not fit the device; everything allocated is freed. */
int vmask_centrelines(int device, int64_t n0, int64_t n1, int64_t n2,
                      const int64_t* offsets, int64_t nbranch, const int64_t* voxels,
                      const double* spacing /* may be NULL */, double end_weight,
                      double smoothing /* > 0: fixed lambda; <= 0: search */, double residual_per_point, double sample_step,
                      int64_t lds_entries /* 0: default */,
                      double* entry_f64 /* E x 11 */, double* branch_f64 /* nbranch x 5 */, int64_t* branch_int /* nbranch x 3 */,
                      double* kernel_ms /* may be NULL */);

/* The tube model: a branch table with centre points and radii rasterised to a volume of n0 x n1 x n2 voxels (fewer than 2^31).
 * INPUTS.  spacing h (h0, h1, h2; NULL: 1 1 1; the rules of vmask_centrelines: finite, positive, max / min <= 1000).  The branch
 * table offsets[nbranch + 1]: it starts at 0 and every branch has at least two entries (so it does not decrease); E = offsets[nbranch]
 * < 2^31.  P (E x 3 float64): the centre points in the units of the spacing - voxel (i0, i1, i2) sits at (i0 h0, i1 h1, i2 h2).
 * r (E float64): the radii in the same units.  keep (nbranch uint8, may be NULL): a branch with 0 contributes nothing.
 * branch_label (nbranch int32, > 0; NULL: b + 1).  mask (uint8 volume, may be NULL).
 * PRIMITIVES.  Primitive e joins the consecutive entries e and e + 1 of one branch (A = P[e], B = P[e + 1], rA = r[e], rB = r[e + 1]):
 * the segment A B swept by a ball whose radius runs linearly from rA to rB.  At voxel i, in float64, every operation rounded on
 * its own (nothing contracted into an FMA), the sums in the order written, per axis a:
 *   x_a = fl(i_a h_a)
 *   d_a = B_a - A_a                 dd = (d0 d0 + d1 d1) + d2 d2
 *   w_a = x_a - A_a                 wd = (w0 d0 + w1 d1) + w2 d2
 *   t   = 0 if dd == 0 else min(max(wd / dd, 0), 1), taken as: t = wd / dd; t = t if t > 0 else 0; t = 1 if t > 1 else t (a NaN gives 0)
 *   c_a = A_a + t d_a               q_a = x_a - c_a
 *   qq  = (q0 q0 + q1 q1) + q2 q2
 *   rho = rA + t (rB - rA)          f = qq - rho rho
 * wd / dd is the correctly rounded division, never a reciprocal.  The voxel is INSIDE primitive e iff f <= 0.  f is the power
 * distance to the swept ball at the foot point: where two vessels overlap, a voxel goes to the one it lies deeper in, as in a
 * power diagram.
 * PER VOXEL.  Over the primitives of kept branches with f <= 0 the lexicographically least pair (f, e) wins:
 *   label (int32): the label of e's branch, 0 when there is none;  field (float64, may be NULL): that f, +inf when there is none;
 *   nearest (int64, may be NULL): that e, -1 when there is none.
 * PER CALL.  sizes[nbranch] (int64): the voxels whose winner belongs to branch b;  overlap[nbranch]: those of them with mask != 0
 * (all 0 without a mask);  missed (1): the voxels with mask != 0 and label 0;  counts (4, may be NULL): the primitives of kept
 * branches, the occupied bricks, the (brick, primitive) pairs, the longest brick list.  Every count comes from integer atomics and
 * every other output is a minimum over a set: repeats are bit-identical.
 * THE RUN (it describes the run, no output bit depends on it).  The volume is cut into the 8 x 8 x 8 bricks of the floods.  Per
 * primitive an index box: per axis from floor(min(A_a - rA, B_a - rB) / h_a) - 1 to ceil(max(A_a + rA, B_a + rB) / h_a) + 1, clipped
 * to the volume.  c_a - rho and c_a + rho are linear in t, so in exact arithmetic every voxel with f <= 0 lies in the box without
 * the extra voxel; the rounding of x, c and rho moves a bound by less than 2^-30 of the largest spacing - the inputs are at most
 * 2^20 of it - which is less than 2^-20 voxels at the spacing ratio allowed, and the box is one whole voxel wider.  The bricks
 * that a box meets are counted, scanned and filled into per-brick lists (order free: the winner rule does not see it); one workgroup
 * of 512 threads per occupied brick evaluates its list, a wave skipping a primitive whose box misses its slice; the bricks with an
 * empty list are filled with 0, +inf, -1.  A call in which no brick is occupied (nbranch = 0, every branch dropped, everything
 * outside the volume) launches no empty grid and returns zeros, +inf and -1.
 * step_ms (6, host, may be NULL): the time by hipEvents of the table check, the count pass, the scan, the list fill, the evaluation
 * and the fill of the empty bricks.
 * VRG_E_ARG, before anything is written: a spacing outside the rules; offsets that do not start at 0 or leave a branch fewer than
 * two entries, E >= 2^31; a coordinate or radius that is not finite; a negative radius; |P_a| or r above 2^20 max(h); a label <= 0
 * (all counted on the device, over every branch whether kept or not); more than 2^31 - 1 (brick, primitive) pairs, with a text
 * that says so; a shape outside the envelope of the other passes; a NULL label or missed.  nbranch = 0 is no error.
 * VRG_E_MEM: the tables and outputs where they are host arrays, 4 bytes per entry, 8 per brick and 4 per pair do not fit the
 * device; everything allocated is freed. */
int vmask_tubes(int device, int64_t n0, int64_t n1, int64_t n2, const double* spacing /* may be NULL */,
                const int64_t* offsets, int64_t nbranch, const double* positions /* E x 3 */, const double* radius /* E */,
                const uint8_t* keep /* nbranch, may be NULL */, const int32_t* branch_label /* nbranch, may be NULL */,
                const uint8_t* mask /* may be NULL */,
                int32_t* label, double* field /* may be NULL */, int64_t* nearest /* may be NULL */,
                int64_t* sizes /* nbranch */, int64_t* overlap /* nbranch */, int64_t* missed /* 1 */,
                int64_t* counts /* 4, may be NULL */, double* step_ms /* 6, host, may be NULL */);

/* The flow solve on the branch graph: S >= 1 scenarios of one topology in one launch.  The graph is vmask_branches': nnode nodes,
 * nbranch branches with branch_ends[2 nbranch].  A branch with ends -1 -1 (a closed curve) or with both ends on one node (a
 * loop) carries no flow: Q = 0, it takes no part.  Parallel branches are ordinary.
 * fixed[nnode] (0 / non-zero, the same for all scenarios); resistance: nbranch values used by every scenario (r_stride 0) or
 * S x nbranch (r_stride nbranch), R > 0 and finite; fixed_pressure: nnode values (p_stride 0) or S x nnode (p_stride nnode), read at
 * the fixed nodes only; one exponent k, 1 <= k <= 3.
 * THE LAW, with Q_b the flow from branch_ends[b][0] = u to branch_ends[b][1] = v and D = P_u - P_v:
 *   D = R_b |Q_b|^(k-1) Q_b,  that is  Q_b = sign(D) (|D| / R_b)^(1/k) = copysign(pow(fl(|D| / R_b), fl(1 / k)), D);  for k == 1: fl(D / R_b).
 * THE UNKNOWN: P at the free nodes such that at every free node i the signed sum of the incident flows (s_ib = +1 where i is the
 * branch's first end, -1 where it is the second) is 0 - unique in every component that holds a fixed node.  A component without
 * a fixed node is floating: P = NaN (0x7ff8000000000000) at its nodes, Q = 0 in its branches; counts = {floating components,
 * floating nodes} (may be NULL; an unfixed node without a participating branch is such a component).
 * node_pressure (S x nnode), branch_flow (S x nbranch): branch_flow is computed from the returned node_pressure by the law, so every
 * branch satisfies it by construction.  status (S x 3, int64): [0] converged: max over the free nodes |sum_b s_ib Q_b| <= tol
 * max_b |Q_b|; [1] the outer iterations run; [2] the inner iterations summed.  residual (S): the final max |sum| / max |Q| (0 where
 * both are 0).  A scenario that does not converge within max_iter outer iterations holds its last iterate and says so in status;
 * it neither fails the call nor touches another scenario.
 * THE ITERATION (one workgroup of T = 256 threads per scenario; these choices describe the run, the contract is the residual):
 *   start   P = its pressure at a fixed node, at a free node the pressure of its anchor - the smallest fixed node of its component.
 *   outer   step n = 0, 1, ..: with c = fl(1 - fl(1 / k)),
 *             g_b = fl(1 / R_b) when k == 1 or n == 0 (the linear start), otherwise 1 / ((k R_b) pow(a, k - 1)) with
 *                   a = max(|Qi_b|, floor), floor = (0.01 tol) max_b |Qi_b| (1 / R_b where a is 0);
 *             at every free node i over its incidence list:  diag_i = sum g_b,  r_i = rhs_i - sum g_b (P_i - P_other),
 *                   rhs_i = 0 when k == 1 or n == 0, otherwise 0 - c sum s_ib Qi_b;
 *             conjugate gradients from the current P with z = r / diag:  p = z, rz = sum r z, then while rz > 1e-16 rz_0 and fewer
 *                   than 2 F + 64 inner iterations (F free nodes):  Ap_i = sum g_b (p_i - p_other) (p = 0 at fixed nodes),
 *                   pAp = sum p Ap (stop unless > 0), alpha = rz / pAp, P += alpha p, r -= alpha Ap, z = r / diag, rz' = sum r z,
 *                   beta = rz' / rz, p = z + beta p;
 *             Q_b by the law from P (branch_flow); for k != 1 the iteration's own flows Qi_b = Q_b at n == 0, else c Qi_b + g_b D_b;
 *             the residual above; converged ends the scenario.
 *           Below the floor the law is replaced by a linear one, which moves a flow by at most the floor: 0.01 tol max |Q|.
 * THE ORDER OF THE SUMS (every operation one IEEE double operation, nothing contracted into an FMA, no floating-point atomics):
 *   a sum over a node's incidence list: added to 0.0 in the list's order - the node's participating branches in ascending branch
 *     index - each term formed as fl(g_b fl(x_i - x_other)), fl(+-Q_b);
 *   a sum over the free nodes j = 0 .. F - 1 (ascending node id): thread t adds its terms j = t, t + T, .. to 0.0 in sequence; every
 *     wave of 64 threads then runs a_l <- a_l + a_(l xor s) for s = 32, 16, 8, 4, 2, 1; the four wave sums are added as
 *     ((w0 + w1) + w2) + w3.  The maxima are order-free.
 * Repeats are bit-identical, and a scenario's results do not depend on the other scenarios of the call.  For k == 1 no pow runs
 * and every output is a pure function of the inputs in IEEE arithmetic (tests/flow_model.py restates it); for k != 1 the results
 * depend on the device's pow.
 * VRG_E_ARG, before anything is written: nscen < 1; k outside [1, 3]; tol not in (0, 1); max_iter < 1; a stride that is neither 0
 * nor the row length; a negative count, nbranch >= 2^30; and, counted on the device: an end that is no node id or -1 -1, an R of a
 * participating branch that is not finite and > 0, a fixed pressure that is not finite.  VRG_E_MEM: the tables where they are host
 * arrays, the outputs likewise, 13 bytes per node and 9 per branch for the topology and, per scenario, 32 bytes per node and 16
 * per branch of work space do not fit the device; everything allocated is freed. */
int vmask_flow(int device, int64_t nnode, int64_t nbranch, const int64_t* branch_ends, const uint8_t* fixed,
               int64_t nscen, const double* resistance, int64_t r_stride, const double* fixed_pressure, int64_t p_stride,
               double k, double tol, int64_t max_iter,
               double* node_pressure, double* branch_flow, int64_t* status, double* residual, int64_t* counts /* 2, may be NULL */);

/* Perona-Malik diffusion of a 3-D volume I (VRG_F32 or VRG_F64, assumed finite; float32 is an input type only): `iterations`
 * explicit steps over the 6 neighbours, float64 throughout.
 * The host forms, in double, ih_a = 1.0 / h_a per axis (spacing == NULL: 1 1 1) and iK = 1.0 / K.  u^0 = (double) I.
 * One step at voxel p: acc = 0.0; the neighbours q in the order axis 0 -, axis 0 +, axis 1 -, axis 1 +, axis 2 -, axis 2 +, the
 * neighbour's index clamped at the faces (a missing neighbour is p itself: d = 0); per neighbour on axis a
 *     d = u[q] - u[p];  g = d * ih_a;  t = g * iK;
 *     c = 1.0 / (1.0 + t * t)      function 0, "rational"
 *     c = exp(-(t * t))            function 1, "exponential"
 *     acc = acc + (c * g) * ih_a;
 * then u'[p] = u[p] + dt * acc.  EVERY OPERATION IS ONE IEEE DOUBLE OPERATION IN EXACTLY THIS ASSOCIATION, nothing contracted
 * into an FMA.  out (float64) is u after `iterations` steps; it must not overlap the input, which is never written.
 * Stability: B = 1.0 / (2.0 * ((ih_0 * ih_0 + ih_1 * ih_1) + ih_2 * ih_2)), 1/6 at unit spacing.  time_step <= 0 is automatic:
 * dt = 0.5 * B.  For dt <= B a step is a convex combination of the voxel and its neighbours: nothing leaves the input's range
 * and a constant volume is a fixed point to the last bit.
 * With function 0 the result is a pure function of the inputs in IEEE arithmetic (tests/denoise_model.py restates it); with
 * function 1 it depends on the device's exp.  Repeats are bit-identical.
 * One launch per step, ping-pong between out and one float64 work volume - the only allocation of a call with device pointers.
 * VRG_E_ARG, before anything is written: iterations outside 1..1000; K not finite and positive; a spacing not finite and
 * positive; time_step not finite or above B; function not 0 or 1; a dtype other than the two; a null pointer; a shape outside
 * the envelope of the other passes.  VRG_E_MEM: the input, the output and one float64 volume do not fit the device (volumes are
 * not processed in slabs); everything allocated is freed. */
int vmask_diffuse(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const double* spacing /* may be NULL */,
                  double K, int iterations, double time_step, int function, double* out);

/* Median over the window of (2 r0 + 1) x (2 r1 + 1) x (2 r2 + 1) voxels around every voxel, every radius 0 or 1, the window's
 * indices clamped at the faces: scipy.ndimage.median_filter(I, size=(2 r0 + 1, 2 r1 + 1, 2 r2 + 1), mode='nearest').  A window
 * has 1, 3, 9 or 27 values, so the median is one of the input's values: exact in either type, and the output's value set is a
 * subset of the input's.  volume: VRG_F32 or VRG_F64, assumed finite; out: the same type, not overlapping the input, which is
 * never written.  Radii (1, 1, 0) give the in-plane 3 x 3 median of a thick-slice volume; (0, 0, 0) is a copy.  Equal as
 * numbers: where -0.0 and +0.0 meet in a window either may come back.
 * VRG_E_ARG, before anything is written: a radius outside {0, 1}; a dtype other than the two; a null pointer; a shape outside
 * the envelope of the other passes.  VRG_E_MEM: the input and the output do not fit the device; everything allocated is freed. */
int vmask_median(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, int r0, int r1, int r2, void* out);

/* N4-style bias-field correction, by a definition of our own.  All arithmetic is float64, EVERY OPERATION ONE IEEE DOUBLE OPERATION
 * IN THE WRITTEN ASSOCIATION, nothing contracted into an FMA; no float atomics (integer atomics count the histogram).
 *
 * Axis tables (host, double).  An axis of extent n with M spans has K = M + 3 control points.  For voxel index i:
 *     u = ((i + 0.5) * M) / n;  s = min(floor(u), M - 1);  t = u - s;  o = 1.0 - t;
 *     w0 = ((o*o)*o)/6.0;  w1 = ((((3.0*t - 6.0)*t)*t) + 4.0)/6.0;  w2 = (((((-3.0*t + 3.0)*t + 3.0)*t)) + 1.0)/6.0;  w3 = ((t*t)*t)/6.0;
 *     S = ((w0*w0 + w1*w1) + w2*w2) + w3*w3;  c2_j = w_j*w_j;  c3_j = ((w_j*w_j)*w_j)/S.
 * vmask_bias_axis_table writes them: s[n] and w, c2, c3 as [n][4].  Host code only.  VRG_E_ARG: n outside 1..32000, spans outside
 * 1..64, a null pointer. */
int vmask_bias_axis_table(int n, int spans, int32_t* s, double* w, double* c2, double* c3);

/* The fit: the multilevel-B-spline approximation of Lee, Wolberg and Shin of the residual r (float64) over the voxels with
 * mask != 0 (uint8), on a voxel grid, where it factorises into three contractions, each summed in ascending voxel index from +0.0:
 *     N0[k0,y,z] = sum_x c3_0[x][k0 - s0[x]] * r[x,y,z],   D0[k0,y,z] = sum_x c2_0[x][k0 - s0[x]]
 *                  over the x with s0[x] <= k0 <= s0[x] + 3 and mask[x,y,z] != 0 (what r holds elsewhere does not matter);
 *     N1[k0,k1,z] = sum_y c3_1[y][k1 - s1[y]] * N0[k0,y,z], D1[k0,k1,z] = sum_y c2_1[y][k1 - s1[y]] * D0[k0,y,z]
 *                  over the y with s1[y] <= k1 <= s1[y] + 3;  axis 2 likewise, giving N2 and D2 over (k0, k1, k2);
 *     phi = N2 / D2 where D2 > 0, else 0.0.
 * spans: the three M_a, each 1..64.  phi: float64 [M_0 + 3][M_1 + 3][M_2 + 3].  An empty mask gives phi = 0.
 * VRG_E_ARG, before anything is written: spans outside 1..64, a null pointer, a shape outside the envelope of the other passes.
 * VRG_E_MEM: r and the mask where they are host arrays and 2 (M_0 + 3) n1 n2 doubles do not fit the device; everything is freed. */
int vmask_bias_fit(int device, const double* r, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, const int* spans, double* phi);

/* The evaluation of a lattice phi [K0][K1][K2] on the voxel grid: three expansions, each a four-term sum over j = 0..3 ascending
 * from +0.0:
 *     E2[k0,k1,z] = sum_j w2[z][j] * phi[k0,k1,s2[z] + j];  E1[k0,y,z] = sum_j w1[y][j] * E2[k0,s1[y] + j,z];
 *     F[x,y,z] = sum_j w0[x][j] * E1[s0[x] + j,y,z].
 * out: float64 [n0][n1][n2].  Errors as vmask_bias_fit. */
int vmask_bias_eval(int device, const double* phi, const int* spans, int64_t n0, int64_t n1, int64_t n2, double* out);

/* The sharpening map.  Host code only: it touches no device.  counts: nb bin counts (float64), bin centres umin + k h,
 * h = (umax - umin) / (nb - 1).  The counts are zero-padded to P = 512 at offset (P - nb) / 2; G is a Gaussian of
 * sigma = fwhm / (2 sqrt(2 ln 2)) / h bins on the circular index min(k, P - k), normalised to sum 1.  With G^ and V^ the DFTs:
 *     U = max(Re IDFT(conj(G^) / (|G^|^2 + noise) . V^), 0);  num = Re IDFT(G^ . DFT(centre . U));  den = Re IDFT(G^ . DFT(U));
 *     E[k] = num / den where den > 1e-12 max(den), else the bin centre - cut back to the nb bins.
 * The transforms are direct O(P^2) sums in double: E is a pure function of the inputs on one machine, and equals an FFT
 * restatement up to rounding.  VRG_E_ARG: nb outside 8..256; fwhm or noise not finite and positive; umin, umax not finite or
 * umax <= umin; a null pointer. */
int vmask_bias_sharpen(const double* counts, int nb, double umin, double umax, double fwhm, double noise, double* E /* nb */);

/* The loop.  v: float64 log intensities (finite over the mask); mask: uint8; m0: the spans of the first level.  b = 0.  Per level
 * L = 0 .. levels - 1 the spans are M_a = m0_a 2^L; per iteration, at most `iterations` per level:
 *   1. u = v - b over the mask; umin, umax its exact extrema.  umin == umax ends the whole run.
 *   2. h = (umax - umin) / (nb - 1); counts (64-bit integers) at idx = clamp(floor((u - umin) / h + 0.5), 0, nb - 1); E from
 *      vmask_bias_sharpen.
 *   3. p = (u - umin) / h; i0 = clamp(floor(p), 0, nb - 2); f = p - i0; r = u - (E[i0] + f * (E[i0 + 1] - E[i0])) over the mask.
 *   4. phi = fit(r, mask); b <- b + eval(phi) over the whole volume.
 *   5. phi goes to the host; max |phi| < threshold ends the level.
 * b: float64 [n0][n1][n2].  trace (may be NULL): one record of four doubles per iteration - level, max |phi|, umin, umax -, room
 * for levels * iterations records; ntrace (may be NULL): their number.  Both are host pointers.
 * VRG_E_ARG, before anything is written: m0 outside 1..32 or m0 2^(levels - 1) > 64; levels outside 1..6; iterations outside
 * 1..200; nb outside 8..256; fwhm, noise or threshold not finite and positive; a null pointer; a shape outside the envelope of
 * the other passes; an empty mask.  VRG_E_MEM: v, the mask and b where they are host arrays, one float64 work volume and the
 * fit's 2 (M_0 + 3) n1 n2 doubles do not fit the device (volumes are not processed in slabs); everything allocated is freed. */
int vmask_bias_log_field(int device, const double* v, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, const int* m0, int levels,
                         int iterations, double threshold, int nb, double fwhm, double noise, double* b,
                         double* trace /* may be NULL */, int64_t* ntrace /* may be NULL */);

/* The correction of a volume I (VRG_F32 or VRG_F64).  mask (uint8) may be NULL: I > 0; a mask voxel with I <= 0 is taken out of the
 * mask.  v = log((double) I) on the device over the mask; the loop; field = exp(b) and corrected = (double) I / field over the
 * whole volume, both float64; field may be NULL.  The result depends on the device's log and exp.  Errors as
 * vmask_bias_log_field, and a dtype other than the two. */
int vmask_bias_correct(int device, const void* volume, int dtype, const uint8_t* mask /* may be NULL */, int64_t n0, int64_t n1, int64_t n2,
                       const int* m0, int levels, int iterations, double threshold, int nb, double fwhm, double noise,
                       double* corrected, double* field /* may be NULL */, double* trace /* may be NULL */, int64_t* ntrace /* may be NULL */);

/* Rigid / affine registration of a moving volume to a fixed one, by a definition of our own: what one cost evaluation needs on the
 * device - the moving volume sampled at every voxel of the fixed grid through an affine voxel map and scattered into a joint
 * histogram -, the pyramid and the resampled result.  The search is host code (registration.py).  All arithmetic is float64, EVERY
 * OPERATION ONE IEEE DOUBLE OPERATION IN THE WRITTEN ASSOCIATION, nothing contracted into an FMA; the only atomics are integer ones.
 * Volumes are C-contiguous, indexed (i0, i1, i2); n are the fixed extents, m the moving ones.
 *
 * Voxel map.  T: 12 doubles on the host, the first three rows of the 4 x 4 matrix that takes a fixed voxel index to a moving one.
 * With W (4 x 4) taking the moving image's world coordinates to the fixed image's and the NIfTI voxel -> world affines of the two,
 * the caller forms T = inv(movingAffine) . inv(W) . fixedAffine; the entries below are functions of T.
 *
 * Sample at fixed voxel (i, j, k).  Per axis a:  p_a = ((T[a][0]*i + T[a][1]*j) + T[a][2]*k) + T[a][3]  (never accumulated along a
 * row).  The voxel is INSIDE iff 0 <= p_a <= m_a - 1 on all three axes (false for a NaN; p = -0.0 is inside).  f_a = floor(p_a),
 * t_a = p_a - f_a, the upper neighbour's index is min(f_a + 1, m_a - 1).  Each moving value is converted to double when read
 * (dtype VRG_F32 or VRG_F64); interpolation runs along axis 2, then axis 1, then axis 0, each step lo + t * (hi - lo):
 *     x[a][b] = v[a][b][0] + t_2 * (v[a][b][1] - v[a][b][0]);  y[a] = x[a][0] + t_1 * (x[a][1] - x[a][0]);  value = y[0] + t_0 * (y[1] - y[0]).
 * A sample that is not finite counts as outside - so does every sample that touches a moving value that is not finite, also with
 * weight 0 (0 * inf is a NaN): such a value takes the up to 8 fixed voxels around it out.
 * Nearest (order 0): q_a = floor(p_a + 0.5); inside iff 0 <= q_a <= m_a - 1; the value at q is copied in its own type.
 *
 * Quantisation.  b(v) = clamp(floor((v - lo) * s), 0, B - 1), clamped as a double and then converted (a NaN lands in bin 0);
 * 8 <= B <= 128; the caller forms s = B / (hi - lo) in double, s = 0 when hi == lo. */

/* lohi[0], lohi[1] (host): the exact minimum and maximum, as doubles, of the finite voxels of a VRG_F32 or VRG_F64 volume - of
 * those with mask != 0 where mask (uint8) is not NULL; +inf, -inf when there is none.  Per-workgroup pairs are reduced on the host:
 * the result does not depend on any order (where -0.0 and +0.0 are both extreme, either may come back).
 * VRG_E_ARG: a dtype other than the two; a null pointer; a shape outside the envelope of the other passes. */
int vmask_reg_minmax(int device, const void* volume, int dtype, const uint8_t* mask /* may be NULL */, int64_t n0, int64_t n1, int64_t n2,
                     double* lohi /* 2, host */);

/* bins[v] = b((double) volume[v]) with (lo, s); 255 where mask[v] == 0 (mask not NULL) or the value is not finite.  *inside (host,
 * may be NULL) receives the number of voxels that are not 255.  VRG_E_ARG, before anything is written: B outside 8..128; lo or s not
 * finite, s < 0; a dtype other than VRG_F32 / VRG_F64; a null pointer; a shape outside the envelope. */
int vmask_reg_quantise(int device, const void* volume, int dtype, const uint8_t* mask /* may be NULL */, int64_t n0, int64_t n1, int64_t n2,
                       int B, double lo, double s, uint8_t* bins, int64_t* inside /* may be NULL */);

/* The joint histogram: H[bf * B + bm] = the number of fixed voxels v with bf = fixedBins[v] < B (255 marks a voxel that does not
 * take part; any other value >= B is treated alike) whose sample is inside, bm = b(sample) with (mlo, ms).  H: B * B unsigned
 * 64-bit counts, overwritten.  Counts are integers: they do not depend on the order of the additions, and repeats are identical.
 * VRG_E_ARG, before anything is written: B outside 8..128; a T, mlo or ms that is not finite; a dtype other than VRG_F32 / VRG_F64;
 * a null pointer; a fixed or moving shape outside the envelope of the other passes.  VRG_E_MEM: the bin image and the moving
 * volume, where they are host arrays, do not fit the device (volumes are not processed in slabs); everything allocated is freed. */
int vmask_reg_joint_hist(int device, const uint8_t* fixedBins, int64_t n0, int64_t n1, int64_t n2, const void* moving, int dtype,
                         int64_t m0, int64_t m1, int64_t m2, const double* T /* 12, host */, int B, double mlo, double ms, uint64_t* H /* B * B */);

/* The cost of a joint histogram.  Host code only: it touches no device.  N = sum H; *cost = +inf when N == 0 or
 * (double) N < minOverlap * (double) nmask (nmask: the fixed voxels that take part).  Sums run in row-major order.
 *   kind 0, corratio (one minus the correlation ratio of the moving bin given the fixed bin, as flirt's default): with y = bm, per
 *     row r the 64-bit integers n_r = sum H, S_r = sum y H, Q_r = sum y^2 H, and n, S, Q their totals;
 *         within = sum over the rows with n_r > 0, ascending from +0.0, of ((double) Q_r - ((double) S_r * (double) S_r) / (double) n_r);
 *         total  = (double) Q - ((double) S * (double) S) / (double) n;      cost = within / total,  0 when total <= 0.
 *     A diagonal histogram costs exactly 0.
 *   kind 1, mi: -((H_F + H_M) - H_FM);   kind 2, nmi: -((H_F + H_M) / H_FM), 0 when H_FM is 0.
 *     An entropy is -(sum over the non-zero counts c, ascending from +0.0, of p * log(p)), p = (double) c / (double) N, with the
 *     host's log; H_F over the row sums, H_M over the column sums, H_FM over the cells.
 * VRG_E_ARG: B outside 8..128; kind outside 0..2; minOverlap outside [0, 1] (a NaN included); nmask < 0; a null pointer. */
int vmask_reg_cost(const uint64_t* H, int B, int kind, double minOverlap, int64_t nmask, double* cost);

/* One level of the pyramid.  The output extent is ceil(n / 2) per axis.  A VRG_F32 or VRG_F64 volume gives float64:
 *     out[i0][i1][i2] = 0.125 * sum over d0, d1, d2 in {0, 1} (d2 fastest, ascending from +0.0) of (double) in[min(2 i_a + d_a, n_a - 1)];
 * a VRG_U8 mask gives uint8: 1 iff any voxel of that block is non-zero.  The voxel -> world affine of the output is
 * A . [[2,0,0,.5],[0,2,0,.5],[0,0,2,.5],[0,0,0,1]].  VRG_E_ARG: another dtype; a null pointer; a shape outside the envelope. */
int vmask_reg_shrink(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, void* out);

/* The moving volume on the fixed grid.  order 1: out is float64, the sample above (dtype VRG_F32 or VRG_F64); order 0: out has the
 * moving volume's type (VRG_U8, VRG_I16, VRG_I32, VRG_F32, VRG_F64), the nearest voxel.  fill is written where the voxel is
 * outside; with order 0 it must be a value of that type.  VRG_E_ARG, before anything is written: order not 0 or 1; a dtype that
 * the order does not take; a fill that an integer type does not hold; a T that is not finite; a null pointer; a shape outside the
 * envelope.  VRG_E_MEM: the moving volume and the output, where they are host arrays, do not fit the device. */
int vmask_reg_resample(int device, const void* moving, int dtype, int64_t m0, int64_t m1, int64_t m2, const double* T /* 12, host */, int order,
                       double fill, void* out, int64_t n0, int64_t n1, int64_t n2);

/* A device array that outlives a call: registration.register keeps the volumes, the pyramid and the bin images of host arrays on
 * the device through it, so that they cross once and not with every evaluation.  *held receives `bytes` bytes of device memory,
 * filled from `host` where that is not NULL; vmask_reg_release frees them (NULL is allowed).  VRG_E_ARG: bytes < 1, held NULL;
 * VRG_E_NOGPU; VRG_E_MEM.  vmask_reg_fetch copies the first `bytes` bytes of a held array to the host (VRG_E_ARG: a null pointer,
 * bytes < 1): how the warp of registration.registerNonlinear comes back. */
int vmask_reg_hold(int device, const void* host /* may be NULL */, int64_t bytes, void** held);
int vmask_reg_fetch(const void* held, void* host, int64_t bytes);
void vmask_reg_release(void* held);

/* Nonlinear registration by a B-spline demons warp, by a definition of our own (no parity with FSL fnirt is claimed).  All arithmetic
 * is float64, EVERY OPERATION ONE IEEE DOUBLE OPERATION IN THE WRITTEN ASSOCIATION, nothing contracted into an FMA; no float atomics.
 * Volumes are C-contiguous (i0, i1, i2); n are the fixed extents, m the moving ones, V = n0 n1 n2.
 *
 * Warp.  u: float64 [3][n0][n1][n2] on the fixed grid, component c the displacement along axis c in fixed-voxel units.  T: 12 doubles
 * on the host, the fixed voxel -> moving voxel map of vmask_reg_*.  At fixed voxel v = (i0, i1, i2):
 *     q_c = (double) v_c + u_c[v];      p_a = ((T[a][0]*q_0 + T[a][1]*q_1) + T[a][2]*q_2) + T[a][3].
 * The inside test (0 <= p_a <= m_a - 1; false for a NaN), f_a = floor(p_a), t_a = p_a - f_a, the upper neighbour min(f_a + 1, m_a - 1)
 * and the interpolation along axis 2, then 1, then 0, each step lo + t * (hi - lo), are those of vmask_reg_joint_hist:
 *     x[a][b] = v[a][b][0] + t_2 * (v[a][b][1] - v[a][b][0]);  y[a] = x[a][0] + t_1 * (x[a][1] - x[a][0]);  m = y[0] + t_0 * (y[1] - y[0]).
 * A sample that is not finite counts as outside.  With u = 0, q_c = (double) v_c and every sample is that of vmask_reg_*.
 *
 * Force pass.  A voxel TAKES PART iff mask[v] != 0 (mask uint8, may be NULL: every voxel), (double) F[v] is finite and its sample m is
 * inside.  For such a voxel, with the caller's flo, fs, mlo, ms (fs = 1 / (fhi - flo), 0 when fhi == flo; ms likewise) and maxStep:
 *     r = (F - flo) * fs - (m - mlo) * ms;
 *     g0 = y[1] - y[0];   e[a] = x[a][1] - x[a][0],  g1 = e[0] + t_0 * (e[1] - e[0]);
 *     d[a][b] = v[a][b][1] - v[a][b][0],  h[a] = d[a][0] + t_1 * (d[a][1] - d[a][0]),  g2 = h[0] + t_0 * (h[1] - h[0]);
 *     G_c = ((g0*T[0][c] + g1*T[1][c]) + g2*T[2][c]) * ms;
 *     a2 = 1.0 / ((4.0*maxStep)*maxStep);    den = ((G_0*G_0 + G_1*G_1) + G_2*G_2) + (r*r)*a2;
 *     delta_c = (r*G_c) / den  where den > 0 and den is finite, else 0.0 (the voxel still takes part).
 * |delta| <= maxStep (Thirion's bound: |r||G| <= (|G|^2 + r^2 a2) maxStep).  A voxel that takes no part has delta = 0 and part = 0.
 *     S = sum over i2 ( sum over i1 ( sum over i0 of r*r ) ) over the voxels that take part, every sum ascending from +0.0 (the last,
 *     n2-long one on the host); count: their number, a 64-bit integer; the cost of u is S / (double) count.
 * delta: float64 [3][n0][n1][n2]; part: uint8 [n0][n1][n2], 0 / 1; S, count: host pointers.
 * VRG_E_ARG, before a device is looked for and before anything is written: a null pointer (mask excepted); a dtype of either volume
 * other than VRG_F32 / VRG_F64; a T, flo, fs, mlo or ms that is not finite; maxStep not finite and positive (or so small that a2 is not
 * finite); a fixed or moving shape
 * outside the envelope of the other passes.  VRG_E_MEM: the arrays that are host arrays do not fit the device; everything is freed. */
int vmask_warp_force(int device, const void* fixed, int fdtype, const uint8_t* mask /* may be NULL */, int64_t n0, int64_t n1, int64_t n2,
                     const double* u, const void* moving, int mdtype, int64_t m0, int64_t m1, int64_t m2, const double* T /* 12, host */,
                     double flo, double fs, double mlo, double ms, double maxStep, double* delta, uint8_t* part, double* S /* host */,
                     int64_t* count /* host */);

/* The fit of the three force components over the voxels with part != 0: phi[c] = vmask_bias_fit(delta[c], part, spans) for c = 0, 1, 2,
 * bit for bit - the denominators do not depend on c and are computed once.  phi: float64 [3][M_0 + 3][M_1 + 3][M_2 + 3].
 * VRG_E_ARG: spans outside 1..64, a null pointer, a shape outside the envelope.  VRG_E_MEM: delta and part where they are host arrays
 * and 4 (M_0 + 3) n1 n2 doubles do not fit the device. */
int vmask_warp_fit(int device, const double* delta, const uint8_t* part, int64_t n0, int64_t n1, int64_t n2, const int* spans, double* phi);

/* The warp of the next finer level of the pyramid of vmask_reg_shrink (coarse extents c, usually ceil(n / 2)):
 *     fine[comp][i] = 2.0 * trilinear(coarse[comp]) at x_a = clamp(((double) i_a - 0.5) * 0.5, 0, c_a - 1),
 * f_a = floor(x_a), t_a = x_a - f_a, upper neighbour min(f_a + 1, c_a - 1), interpolation along axis 2, 1, 0 in the form above.
 * coarse: float64 [3][c0][c1][c2]; fine: float64 [3][n0][n1][n2].  VRG_E_ARG: a null pointer, a shape outside the envelope. */
int vmask_warp_upsample(int device, const double* coarse, int64_t c0, int64_t c1, int64_t c2, double* fine, int64_t n0, int64_t n1, int64_t n2);

/* The moving volume on the fixed grid through T and the warp u (float64 [3][n0][n1][n2]): vmask_reg_resample with p of the warp above.
 * order 1: float64 samples (dtype VRG_F32 or VRG_F64); order 0: the voxel at floor(p_a + 0.5) in the moving volume's own type
 * (VRG_U8, VRG_I16, VRG_I32, VRG_F32, VRG_F64).  fill where the voxel is outside.  u = 0 gives the bytes of vmask_reg_resample.
 * Errors as vmask_reg_resample, and a null u. */
int vmask_warp_resample(int device, const void* moving, int dtype, int64_t m0, int64_t m1, int64_t m2, const double* T /* 12, host */,
                        const double* u, int order, double fill, void* out, int64_t n0, int64_t n1, int64_t n2);

/* The loop of one level.  u (float64 [3][n0][n1][n2]) is the start and receives the result.  Per iteration, at most `iterations`:
 *   1. the force pass at u: delta, part, S, count.  count == 0 at the first iteration refuses the call (VRG_E_ARG, u unchanged).
 *   2. dphi = vmask_warp_fit(delta, part, spans);  u_c <- u_c + vmask_bias_eval(dphi_c) over the whole grid.
 *   3. dphi goes to the host; top = max |dphi| over the three lattices (a NaN is skipped); top < threshold ends the level.
 * trace (host, may be NULL): one record of three doubles per iteration - S / (double) count (the cost BEFORE the step), (double)
 * count, top -, room for `iterations` records; ntrace (host, may be NULL): their number.  The pyramid, T and the scales of every
 * level and the warp between levels are the caller's (registration.registerNonlinearWith).
 * VRG_E_ARG, before a device is looked for: as vmask_warp_force, and spans outside 1..64, iterations outside 1..200, a threshold that
 * is not finite and positive.  VRG_E_MEM: the arrays that are host arrays, three float64 force volumes, the participation bytes and
 * 4 (M_0 + 3) n1 n2 doubles of the fit do not fit the device (volumes are not processed in slabs); everything allocated is freed. */
int vmask_warp_field(int device, const void* fixed, int fdtype, const uint8_t* mask /* may be NULL */, int64_t n0, int64_t n1, int64_t n2,
                     const void* moving, int mdtype, int64_t m0, int64_t m1, int64_t m2, const double* T /* 12, host */, double flo, double fs,
                     double mlo, double ms, const int* spans, int iterations, double maxStep, double threshold, double* u,
                     double* trace /* may be NULL */, int64_t* ntrace /* may be NULL */);

/* Skull stripping: the brain mask of a head volume, by a definition of our own (the reference leaves the step to an atlas-based GUI
 * plugin; no parity with it is claimed).  Atlas-free, after the Brain Surface Extractor recipe: Marr-Hildreth edges, erosion, the
 * main component, dilation, closing, hole filling.  Only a brain that is BRIGHTER than what surrounds it is supported.
 * All floating-point work is float64, EVERY OPERATION ONE IEEE DOUBLE OPERATION IN THE WRITTEN ASSOCIATION, nothing contracted into
 * an FMA; integer work is exact; the only atomics are integer ones.  Volumes are C-contiguous (i0, i1, i2), VRG_F32 or VRG_F64 (a
 * float32 value is converted to double when read); a voxel that is not finite is refused (VRG_E_ARG).  Masks are uint8, non-zero =
 * set; outputs hold 0 and 1.  Every array may be a host or a device pointer.  An optional Perona-Malik diffusion (vmask_diffuse)
 * in front, and the floor and the contrast below, are the caller's (brain.py):
 *
 * Floor and contrast (host, from the 256 counts c of vmask_brain_histogram, in float64).  w = (hi - lo) / 256, N = sum c,
 * W0[t] = sum_{k<=t} c_k, W1 = N - W0, m[t] = sum_{k<=t} k c_k, M = m[255].  t* = the first maximum over t = 0..254 of
 * ((m W1 - (M - m) W0)^2) / (W0 W1), 0 where a class is empty (Otsu).  floor = lo + (t* + 1) w;
 * contrast = (mu1 - mu0) w with mu0 = m[t*] / W0[t*], mu1 = (M - m[t*]) / W1[t*] (0 where a class is empty).
 *
 * Packed bit volumes (internal): 64 voxels of a row along axis 2 per 64-bit word, voxel i2 at bit i2 % 64 of word i2 / 64, rows
 * padded to whole words, padding bits 0. */

/* lo = min, hi = max of the volume (exact), counts[b] = the number of voxels with
 *     b = min(255, floor((v - lo) * s)),  s = 256.0 / (hi - lo)   (s formed once on the host; v - lo, the product, floor: one operation each).
 * lo, hi: one double each; counts: 256 unsigned 64-bit integers.  Counted with 32-bit atomics on LDS counters per workgroup, added
 * to the 64-bit counts once per workgroup: integers, so no order matters and repeats are identical.
 * VRG_E_ARG, before anything is written: a dtype other than the two; a null pointer; a shape outside the envelope of the other
 * passes; and, found on the device: a voxel that is not finite, hi == lo. */
int vmask_brain_histogram(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, double* lo, double* hi, uint64_t* counts /* 256 */);

/* The scale-normalised Laplacian of Gaussian  E = sum_a (sigma^2 / h_a^2) d_a^2 (G_sigma * J),  spacing h (NULL: 1 1 1), sigma in
 * the units of the spacing.  Taps per axis (host, double), s = sigma / h_a, r = (int)(4.0 * s + 0.5), which must lie in 1..64:
 *     e[x] = exp(-0.5 * x * x / (s * s)) for x = -r..r;  S = their sum, ascending from 0.0;  phi[x] = e[x] / S;
 *     phi2[x] = (x * x / (s * s * s * s) - 1.0 / (s * s)) * phi[x].
 * A pass along an axis with taps w:  out[i] = sum over k = -r..r ascending, from +0.0, of w[k] * in[clamp(i - k, 0, n - 1)], one
 * multiplication and one addition per tap.  Axis 2: A0 = phi * J, A2 = phi2 * J.  Axis 1: B00 = phi * A0, B20 = phi2 * A0,
 * B02 = phi * A2.  Axis 0: T0 = phi2 * B00, T1 = phi * B20, T2 = phi * B02.  With c_a = (sigma * sigma) / (h_a * h_a):
 *     E = (c_0 * T0 + c_1 * T1) + c_2 * T2.
 * out: float64.  The result depends on the host's exp only through the taps (tests/brain_model.py restates everything else one
 * numpy operation per operation).  Five float64 volumes of work space at the peak.
 * VRG_E_ARG, before anything is written: a sigma or spacing that is not finite and positive or gives a radius outside 1..64; a
 * dtype other than the two; a null pointer; a shape outside the envelope; a voxel that is not finite. */
int vmask_brain_log(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const double* spacing /* may be NULL */,
                    double sigma, double* out);

/* `steps` steps of erosion (op 0) or dilation (op 1) by the 6-neighbour cross: scipy.ndimage.binary_erosion / binary_dilation with
 * generate_binary_structure(3, 1), iterations=steps, border_value=border.  Voxels outside the volume count as `border` for an
 * erosion (0 or 1) and as 0 for a dilation (border must be 0).  steps == 0 copies.  One launch per step on the packed volume.
 * VRG_E_ARG, before anything is written: op not 0 or 1; steps outside 0..100000; border not 0 or 1, or 1 with a dilation; a null
 * pointer; a shape outside the envelope. */
int vmask_binary_morph(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, int op /* 0 erode, 1 dilate */, int steps,
                       int border /* 0 | 1, erosion only */, uint8_t* out);

/* The largest connected component of the mask (connectivity 1, 2, 3 as vmask_label: 6, 18, 26 neighbours); among equals the one
 * whose first voxel in raster order comes first (the smallest label of scipy.ndimage.label).  seed >= 0 (a raster index): the
 * component that holds that voxel instead; VRG_E_ARG when the voxel is not set.  *size (may be NULL): its number of voxels.  An
 * empty mask gives zeros and size 0.  Sizes are counted wave-aggregated (one atomic for the lanes of a wave that share a component).
 * VRG_E_ARG, before anything is written: connectivity outside 1..3; a seed outside -1 .. n0 n1 n2 - 1; a null pointer; a shape
 * outside the envelope. */
int vmask_largest_component(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, int connectivity, int64_t seed /* or -1 */,
                            uint8_t* out, int64_t* size /* may be NULL */);

/* scipy.ndimage.binary_fill_holes(mask): every 6-connected component of the complement that has no voxel on a face of the volume
 * is added (a cavity that reaches the outside only across a diagonal is filled).
 * VRG_E_ARG: a null pointer; a shape outside the envelope. */
int vmask_fill_holes(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, uint8_t* out);

/* Steps 3-7 of the extraction on a volume J, packed from the candidate to the final unpack:
 *   candidate     C = ((double) J > floor) & (E <= threshold), E as vmask_brain_log, written as bits by the last edge pass (E itself
 *                 is never stored); threshold = edge * contrast.  The edge response of a bright body is positive in the dark gap
 *                 just outside it: a positive threshold removes that rim and keeps flat interiors, where E is next to 0 and never above it
 *                 (the truncated taps of phi'' sum to about -7e-5 at s = 1: E = -2.2e-4 of a flat intensity).
 *   eroded        `erosion` steps of the cross, the outside counting as 0;
 *   main          its largest 6-connected component (ties: the first in raster order), or the one that holds voxel `seed` (>= 0;
 *                 VRG_E_ARG when that voxel is not in the eroded set); then `erosion` steps of dilation;
 *   closed        `closing` steps of dilation, then `closing` steps of erosion with the outside counting as 1 (a brain that
 *                 touches a face of a cropped scan is not eaten there);
 *   final         the holes filled.
 * out: uint8.  stages (may be NULL): 5 volumes of n0 n1 n2 bytes - candidate, eroded, main (before its dilation), closed, final.
 * info (may be NULL): 16 int64 - [0..4] the set voxels of the five stages, [5] the peak of the call's own device allocations in
 * bytes, [6] the number of components of the eroded set, [7] the size of the kept one, [8..13] the microseconds between HIP events
 * around the edge passes, the erosion, the main component (unpack, labelling, sizes, selection), the dilation and the closing, the
 * hole filling and the final unpack - the copies of `stages` included where asked for -, [14] those of the size pass alone, [15] 0.
 * The edge passes' float64 volumes are freed before anything is labelled.
 * VRG_E_ARG, before anything is written: sigma / spacing as vmask_brain_log; a threshold that is a NaN; a floor that is not
 * finite; erosion or closing outside 0..1000; a seed outside -1 .. n0 n1 n2 - 1; a dtype other than the two; a null volume or out;
 * a shape outside the envelope; a voxel that is not finite.  VRG_E_MEM: the work space does not fit the device. */
int vmask_brain_extract(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const double* spacing /* may be NULL */,
                        double sigma, double threshold, double floor, int erosion, int closing, int64_t seed /* or -1 */, uint8_t* out,
                        uint8_t* stages /* may be NULL */, int64_t* info /* 16, may be NULL */);

/* Minimal-cost bridges between the components of a mask.  idx = C-order linear index.
 * mask (uint8): the vessel mask; its 26-connected components are numbered 1..n as vmask_label numbers them.
 * domain (uint8, may be NULL: the whole volume): where a path may run; effective domain = domain != 0 or mask != 0.
 * cost (VRG_F32 or VRG_F64, used as float64): c(v) > 0, read inside the effective domain only.
 * tips (uint8, may be NULL: all 1): the mask voxels that count as vessel ends.   spacing = (h0, h1, h2), NULL: 1 1 1.
 * Weights: the 26 offsets have codes k = 0..25, the lexicographic order of (d0, d1, d2) in -1..1 with the centre left out (the
 * opposite of k is 25 - k).  hw[k] = 0.5 sqrt((d0 h0)^2 + (d1 h1)^2 + (d2 h2)^2): computed once on the host in float64, the squares
 * summed in the order of the axes, the halving exact.  w(u, v) = fl(fl(c(u) + c(v)) hw[k]) for v = u + offset k: symmetric.  No
 * operation below is fused: every sum is fl(D + w) with w already rounded.
 * Flood: R = 0.5 max_cost.  Every mask voxel is a source: D = 0, Root = its own idx.  A domain voxel outside the mask has
 * D(v) = min over its domain neighbours u of fl(D(u) + w(u, v)) if that is <= R, else +inf - the least fixed point, what Dijkstra
 * computes with the same additions.  No path passes through a mask voxel: it is a source itself.
 * Root(v) = the smallest Root(u) among the tight predecessors u, fl(D(u) + w(u, v)) == D(v).  Pred(v) = the code k of the tight
 * predecessor u = v + offset k with Root(u) == Root(v) of smallest k.  Both are unique fixed points (w > 0, so D(u) < D(v));
 * following Pred from v ends at the mask voxel Root(v).
 * Contact: an ordered pair (u, v = u + offset k) of voxels with finite D such that a = comp(Root(u)) < b = comp(Root(v)) and at
 * least tip_rule (0, 1 or 2) of Root(u), Root(v) have tips != 0.  Its cost K = fl(fl(D(u) + D(v)) + w(u, v)).
 * Bridge of a pair (a, b): its contact of smallest (K, idx(u), k), kept iff K <= max_cost.  Its path: the Pred chain of u
 * reversed, then the Pred chain of v - mask voxel of a .. u, v .. mask voxel of b, both mask voxels included, consecutive entries
 * 26-adjacent.
 * Outputs, the bridges ascending by (a, b): pairs (cap_pair x 6 int64: a, b, idx(u), idx(v), Root(u), Root(v)), costs (cap_pair
 * float64: K), offsets (cap_pair + 1) and voxels (cap_vox): path i = voxels[offsets[i] .. offsets[i + 1]).  All four NULL: counts
 * only.  Otherwise all four are given; too small a capacity: VRG_E_ARG with the needed sizes in counts, nothing else written.
 * Dense outputs, each may be NULL: dist (float64: 0 in the mask, -1 outside the domain, +inf unreached), root (int32: -1 where
 * there is none), pred (uint8: the code k, 255 where there is none), comp (int32: the component labels, 0 outside the mask).
 * counts (int64, 10, may be NULL): [0] components, [1] domain voxels, [2] reached voxels outside the mask, [3] qualifying
 * contacts, [4] pairs with a contact, [5] bridges kept, [6] path entries (= offsets[counts[5]]), [7] 8x8x8 bricks with storage,
 * [8] flood rounds, [9] root rounds.  [7..9] describe the run, not the result; everything else is a pure function of the
 * inputs and bit-identical between runs.
 * VRG_E_ARG, counted on the device before anything is written: a cost inside the effective domain that is not finite or not > 0;
 * max_cost not finite or not > 0; R / w_min > 2^40 with w_min = fl(fl(2 c_min) min hw), c_min the smallest cost in the domain
 * (the bound keeps fl(D + w) > D); a spacing that is not finite and positive, or with max / min > 1000; tip_rule outside 0..2; a
 * dtype other than the two; a shape outside the envelope of the other passes.
 * VRG_E_MEM: storage goes to the bricks that hold a domain voxel and lie within ceil((floor(1.001 R / w_min) + 1) / 8) bricks of
 * one that holds a mask voxel.  12 bytes per brick of the volume, 12812 bytes per brick with storage, what the labelling takes
 * (8 bytes per voxel and 12 per 64 voxels), 24 bytes per entry of the pair table (the next power of two above twice min(contacts,
 * n (n - 1) / 2)) and 24 per pair, the inputs and the dense outputs where they are host arrays; everything allocated is freed. */
int vmask_bridge(int device, const uint8_t* mask, const uint8_t* domain /* may be NULL */, const void* cost, int dtype,
                 const uint8_t* tips /* may be NULL */, int64_t n0, int64_t n1, int64_t n2, const double* spacing /* may be NULL */,
                 double max_cost, int tip_rule, int64_t* counts /* 10, may be NULL */,
                 int64_t* pairs, double* costs, int64_t cap_pair, int64_t* offsets, int64_t* voxels, int64_t cap_vox,
                 double* dist /* may be NULL */, int32_t* root /* may be NULL */, uint8_t* pred /* may be NULL */, int32_t* comp /* may be NULL */);

const char* vmask_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
