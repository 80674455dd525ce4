"""Statement of the objects of a volume (include/gnr.h, gnr_volume_objects_fwd and gnr_grasp_objects_fwd) -- TEST INFRASTRUCTURE ONLY, the
arbiter of csrc/gnr_objects.hip and of k_grasp_objects in csrc/gnr_hand.hip.  The labelling is scipy.ndimage.label with
generate_binary_structure(3, 1 | 2 | 3): it numbers the components in raster order of their first voxel, which is the header's "1 + the
number of components whose smallest linear index is smaller".  The statistics are numpy integers.  Which object a grasp closes on is
built on hand_reference's opening, pose and position (one correctly rounded float64 operation per line there); the votes are integers.
Everything is compared with np.array_equal."""
import math

import numpy as np
from scipy import ndimage

import hand_reference as href

f32, f64 = np.float32, np.float64
FREE = f32(1.0)
ORDER = {6: 1, 18: 2, 26: 3}


def solid(vol, level=0.0, lower=None, z_min=0):
    """[R,R,R] bool: lower < (double)v < level and k >= z_min; a NaN is not solid."""
    v = np.asarray(vol, f32).astype(f64)
    with np.errstate(invalid='ignore'):
        s = (v < f64(level)) & ((-np.inf if lower is None else f64(lower)) < v)
    s[:, :, :int(z_min)] = False
    return s


def label(vol, level=0.0, lower=None, z_min=0, connectivity=6):
    """One scene -> (labels [R,R,R] int32, count)."""
    lab, count = ndimage.label(solid(vol, level, lower, z_min), structure=ndimage.generate_binary_structure(3, ORDER[connectivity]))
    return lab.astype(np.int32), int(count)


def statistics(labels, count, max_objects):
    """-> voxels [max_objects] int32, bbox [max_objects,6] int32 (lo i, j, k, hi i, j, k inclusive; (R,R,R,-1,-1,-1) where there is no
    object), sums [max_objects,3] int64, for the labels 1 .. min(count, max_objects)."""
    R, m = labels.shape[0], min(count, max_objects)
    voxels, sums = np.zeros(max_objects, np.int32), np.zeros((max_objects, 3), np.int64)
    bbox = np.tile(np.int32([R, R, R, -1, -1, -1]), (max_objects, 1))
    if m:
        flat = labels.ravel()
        at = np.flatnonzero(flat)
        at = at[np.argsort(flat[at], kind='stable')]
        lab = flat[at]
        start = np.searchsorted(lab, np.arange(1, count + 1))                  # every label 1 .. count has a voxel
        ijk = np.stack(np.unravel_index(at, labels.shape), 1).astype(np.int64)
        voxels[:m] = np.diff(np.append(start, len(lab)))[:m]
        bbox[:m, :3] = np.minimum.reduceat(ijk, start, axis=0)[:m]
        bbox[:m, 3:] = np.maximum.reduceat(ijk, start, axis=0)[:m]
        sums[:m] = np.add.reduceat(ijk, start, axis=0)[:m]
    return voxels, bbox, sums


def cleaned(vol, labels, count, min_voxels, free=FREE):
    """vol with every component of fewer than min_voxels voxels set to `free`."""
    size = np.bincount(labels.ravel(), minlength=count + 1)
    small = (size < int(min_voxels))
    small[0] = False
    return np.where(small[labels], f32(free), np.asarray(vol, f32))


def objects(vol, level=0.0, lower=None, z_min=0, connectivity=6, max_objects=1024, min_voxels=1):
    """vol [B,R,R,R] -> dict of labels [B,R,R,R] int32, count [B] int32, voxels [B,max] int32, bbox [B,max,6] int32, sums [B,max,3] int64,
    cleaned [B,R,R,R] float32."""
    out = {k: [] for k in ('labels', 'count', 'voxels', 'bbox', 'sums', 'cleaned')}
    for v in np.asarray(vol, f32):
        lab, count = label(v, level, lower, z_min, connectivity)
        vox, bbox, sums = statistics(lab, count, max_objects)
        for k, a in zip(out, (lab, np.int32(count), vox, bbox, sums, cleaned(v, lab, count, min_voxels))):
            out[k].append(a)
    return {k: np.stack(a) for k, a in out.items()}


def closing_lattice(w, scale, height=0.004, depth=0.05, spacing=0.5):
    """The samples of the closing region between the pads of a hand opened to w metres: hand_reference.lattice's rule on the one box
    (lo, extent) = x (-0.5 h, h), y (-hw, w), z (0, d), m = 0 -> local [N,3] float64 metres."""
    h, d, w = f64(height), f64(depth), f64(w)
    cell = f64(spacing) * f64(scale)
    lo, ext = (-0.5 * h, -(0.5 * w), f64(0.0)), (h, w, d)
    n = [max(2.0, math.ceil(e / cell) + 1.0) for e in ext]
    step = [f64(e) / f64(k - 1.0) for e, k in zip(ext, n)]
    ix, iy, iz = (a.ravel() for a in np.meshgrid(*(np.arange(int(k)) for k in n), indexing='ij'))
    return np.stack([lo[0] + ix.astype(f64) * step[0], lo[1] + iy.astype(f64) * step[1], lo[2] + iz.astype(f64) * step[2]], 1)


def grasp_object(labels, pos, quat, width, scale, opening=None, height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, spacing=0.5,
                 approach=0.05):
    """One grasp on labels [R,R,R] int32 -> (object, votes, distinct, inside)."""
    R = labels.shape[0]
    w = href.opening_of(width, R, scale, opening)
    p = href.positions(pos, quat, closing_lattice(w, scale, height, depth, spacing), scale)
    with np.errstate(invalid='ignore'):
        ok = np.all((0.0 <= p) & (p <= f64(R - 1)), axis=1)
    v = np.floor(p[ok] + 0.5).astype(np.int64)
    L = labels[v[:, 0], v[:, 1], v[:, 2]]
    L = L[L > 0]
    if not len(L):
        return 0, 0, 0, int(ok.sum())
    c = np.bincount(L)
    best = int(np.argmax(c))                                                   # the first that attains the maximum: the smallest label
    return best, int(c[best]), int(np.count_nonzero(c)), int(ok.sum())


def grasp_objects(labels, pos, quat, width, count, scale, top_k=None, out=None, **hand):
    """One scene: rows r < min(count, top_k or max_n, max_n); the other rows of `out` = (object, votes, distinct, inside) [max_n] int32
    each are left untouched (zeros without `out`)."""
    pos = np.asarray(pos, f64)
    max_n = len(pos)
    n = max(0, min(int(count), int(top_k or max_n), max_n))
    out = tuple(np.zeros(max_n, np.int32) for _ in range(4)) if out is None else out
    for r in range(n):
        for dst, src in zip(out, grasp_object(labels, pos[r], quat[r], width[r], scale, **hand)):
            dst[r] = src
    return out
