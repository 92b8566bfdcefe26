"""Sequential model of the curve skeleton (subfield-sequential thinning with border marking):
the yardstick of tests/test_skeleton.py.  Plain numpy / scipy; component counts by scipy.ndimage.label inside each
3x3x3 neighbourhood.

Definitions, for an object voxel P with neighbourhood N26*(P) (P removed); everything outside the volume is background:
  border     one of P's 6 face neighbours is background
  end point  exactly one object voxel in N26*(P)
  simple     the object voxels of N26*(P) form exactly one 26-connected component, and the background voxels of N18*(P)
             that are 6-connected within N18*(P) to a background face neighbour of P form exactly one 6-connected component
  subfield   (i0 & 1) * 4 + (i1 & 1) * 2 + (i2 & 1)

    repeat
        mark every voxel that is object and border now
        for s = 0 .. 7: delete every voxel that is marked, still object, in subfield s, not an end point and simple,
                        all judged on the image as it is at the start of step s
    until a whole cycle deleted nothing
"""
import numpy as np
from scipy import ndimage

S26 = np.ones((3, 3, 3), bool)
S6 = ndimage.generate_binary_structure(3, 1)
N18 = ndimage.generate_binary_structure(3, 2).copy()
N18[1, 1, 1] = False
FACES = S6.copy()
FACES[1, 1, 1] = False


def is_simple(block):
    """block: the 3x3x3 neighbourhood of an object voxel (bool; the centre's own value is ignored)."""
    obj = block.copy()
    obj[1, 1, 1] = False
    if ndimage.label(obj, structure=S26)[1] != 1:
        return False
    lab, _ = ndimage.label(~obj & N18, structure=S6)
    return len(set(lab[FACES]) - {0}) == 1


def is_end_point(block):
    return int(block.sum()) - int(block[1, 1, 1]) == 1


def border_mask(img):
    """img: bool volume padded with one layer of background.  True where an object voxel has a background face neighbour."""
    inner = img[1:-1, 1:-1, 1:-1]
    allobj = (img[:-2, 1:-1, 1:-1] & img[2:, 1:-1, 1:-1] & img[1:-1, :-2, 1:-1] & img[1:-1, 2:, 1:-1]
              & img[1:-1, 1:-1, :-2] & img[1:-1, 1:-1, 2:])
    return inner & ~allobj


def subfields(shape):
    i0, i1, i2 = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij', sparse=True)
    return (i0 & 1) * 4 + (i1 & 1) * 2 + (i2 & 1)


def thin(volume):
    """-> (skeleton uint8 0/1, cycles run).  The last cycle, which deletes nothing, counts."""
    volume = np.asarray(volume)
    assert volume.ndim == 3
    img = np.zeros(tuple(n + 2 for n in volume.shape), bool)
    img[1:-1, 1:-1, 1:-1] = volume != 0
    sub = subfields(volume.shape)
    cycles = 0
    while True:
        cycles += 1
        deleted = 0
        marked = border_mask(img)
        for s in range(8):
            cand = np.argwhere(marked & img[1:-1, 1:-1, 1:-1] & (sub == s))
            doomed = []
            for i0, i1, i2 in cand:                       # judged on the image at the start of step s
                block = img[i0:i0 + 3, i1:i1 + 3, i2:i2 + 3]
                if not is_end_point(block) and is_simple(block):
                    doomed.append((i0, i1, i2))
            for i0, i1, i2 in doomed:                     # one after the other: each still simple at its moment
                assert is_simple(img[i0:i0 + 3, i1:i1 + 3, i2:i2 + 3]), 'deleted a voxel that is not simple'
                img[i0 + 1, i1 + 1, i2 + 1] = False
            deleted += len(doomed)
        if not deleted:
            break
    return img[1:-1, 1:-1, 1:-1].astype(np.uint8), cycles


def deletable_left(skeleton):
    """Voxels of `skeleton` that are border, simple and not an end point (a finished skeleton has none)."""
    img = np.zeros(tuple(n + 2 for n in skeleton.shape), bool)
    img[1:-1, 1:-1, 1:-1] = np.asarray(skeleton) != 0
    out = []
    for i0, i1, i2 in np.argwhere(border_mask(img)):
        block = img[i0:i0 + 3, i1:i1 + 3, i2:i2 + 3]
        if not is_end_point(block) and is_simple(block):
            out.append((int(i0), int(i1), int(i2)))
    return out


def topology(volume):
    """(26-components of the object, 6-components of the background of the volume padded with background)."""
    obj = np.pad(np.asarray(volume) != 0, 1)
    return ndimage.label(obj, structure=S26)[1], ndimage.label(~obj, structure=S6)[1]


def crossing_phantom(shape=(48, 40, 32)):
    """A sinusoidal tube crossing a straight tube, plus a separate ring."""
    x, y, z = np.meshgrid(*[np.arange(n, dtype=float) for n in shape], indexing='ij')
    c = [(n - 1) / 2.0 for n in shape]
    tube = ((y - c[1] - 0.2 * shape[1] * np.sin(2 * np.pi * x / shape[0])) ** 2 + (z - c[2]) ** 2) <= 6.0
    tube2 = ((x - 0.3 * shape[0]) ** 2 + (z - c[2]) ** 2) <= 4.0
    return (tube | tube2 | ring_phantom(shape, centre=(0.75 * shape[0], 0.5 * shape[1], 0.2 * shape[2]))).astype(np.uint8)


def ring_phantom(shape=(24, 24, 12), centre=None, radius=5.0, thickness=1.6):
    """A torus in the plane of axes 0 and 1."""
    x, y, z = np.meshgrid(*[np.arange(n, dtype=float) for n in shape], indexing='ij')
    c = centre if centre is not None else [(n - 1) / 2.0 for n in shape]
    rho = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2)
    return ((rho - radius) ** 2 + (z - c[2]) ** 2 <= thickness ** 2).astype(np.uint8)
