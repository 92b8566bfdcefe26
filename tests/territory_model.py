"""The sequential yardstick of the territory map ("f8 territories"): brute force in numpy.

Sites: the voxels with skeleton != 0, sorted by raster index.  A site's label: 1 + the smallest index of a segment that
holds it, 0 for a site in no segment.  A mask voxel's nearest site: the smallest squared Euclidean distance over ALL sites,
``argmin`` over the sorted sites returning the first, hence the smallest raster index, of equidistant ones."""
import numpy as np

BLOCK = 4_000_000                                       # entries of one distance block


def site_labels(shape, offsets, voxels):
    """int32 volume: 1 + the first segment that holds the voxel, 0 elsewhere (a plain loop over the segments)."""
    L = np.zeros(int(np.prod(shape)), np.int32)
    offsets, voxels = [int(x) for x in offsets], [int(x) for x in voxels]
    for k in range(len(offsets) - 1):
        for v in voxels[offsets[k]:offsets[k + 1]]:
            if L[v] == 0:
                L[v] = k + 1
    return L.reshape(shape)


def nearest_sites(mask, skeleton):
    """(nearest, dist2), both int64 volumes: the raster index of every mask voxel's nearest site and the squared distance to
    it; -1 outside the mask and where there is no site."""
    mask, skeleton = np.asarray(mask) != 0, np.asarray(skeleton) != 0
    shape = mask.shape
    nearest = np.full(mask.size, -1, np.int64)
    dist2 = np.full(mask.size, -1, np.int64)
    sites = np.flatnonzero(skeleton.ravel())             # ascending raster index
    vox = np.flatnonzero(mask.ravel())
    if len(sites) and len(vox):
        s = [c.astype(np.int64) for c in np.unravel_index(sites, shape)]
        step = max(1, BLOCK // len(sites))
        for a in range(0, len(vox), step):
            p = np.unravel_index(vox[a:a + step], shape)
            d = np.zeros((len(p[0]), len(sites)), np.int64)
            for axis in range(3):
                d += (p[axis].astype(np.int64)[:, None] - s[axis][None, :]) ** 2
            j = d.argmin(axis=1)                         # the first of equal minima: the smallest raster index
            nearest[vox[a:a + step]] = sites[j]
            dist2[vox[a:a + step]] = d[np.arange(len(j)), j]
    return nearest.reshape(shape), dist2.reshape(shape)


def territories(mask, skeleton, offsets, voxels):
    """(labels int32, nearest int64, sizes int64[segments + 1]) by the definition of include/vmask.h."""
    mask = np.asarray(mask) != 0
    nseg = len(offsets) - 1
    L = site_labels(mask.shape, offsets, voxels)
    nearest, _ = nearest_sites(mask, skeleton)
    labels = np.zeros(mask.shape, np.int32)
    got = nearest >= 0
    labels[got] = L.ravel()[nearest[got]]
    sizes = np.bincount(labels[mask].ravel(), minlength=nseg + 1).astype(np.int64)
    return labels, nearest, sizes
