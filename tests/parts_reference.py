"""Statement of the parts of a volume (include/gnr.h, gnr_volume_parts_fwd) -- TEST INFRASTRUCTURE ONLY, the arbiter of
csrc/gnr_parts.hip.  A watershed of the solid voxels (height > 0) by steepest ascent on an integer height field, neighbouring basins
merged where the pass between them is no neck; ndimage.label's numbering of the parts; objects_reference's statistics rows plus the
peak of every part.  Everything is an integer beyond the one float64 multiply and compare of the neck test; everything is compared
with np.array_equal.
The ascent, the basins and the passes are numpy over shifted views; two things are stated in another form than the header's words and
give the same result: the walk along `up` is pointer jumping (basin <- basin[basin] to a fixed point ends where the walk ends), and of
all the voxel pairs between two basins only the highest pass is tested (both tests of a pair are monotone in its pass, the peaks are the
basins' own).  The closure is a sequential union-find over the joined basin pairs.  tests/test_volume_parts.py holds the literal
restatement, voxel by voxel, and compares."""
import numpy as np

import distance_reference as dref
import objects_reference as oref

f64 = np.float64
ORDER = oref.ORDER


def offsets(connectivity, forward=False):
    """The index differences (di, dj, dk) of a voxel's neighbours; forward: the half with a negative linear offset (every pair once)."""
    r = (-1, 0, 1)
    out = [(a, b, c) for a in r for b in r for c in r if 0 < (a != 0) + (b != 0) + (c != 0) <= ORDER[connectivity]]
    return [d for d in out if d < (0, 0, 0)] if forward else out


def _views(R, d):
    """The slices of the voxels v and of their neighbours v + d, where both lie inside the lattice."""
    return (tuple(slice(max(0, -x), R - max(0, x)) for x in d), tuple(slice(max(0, x), R - max(0, -x)) for x in d))


def ascent(height, connectivity=26):
    """height [R,R,R] int32 -> up [R^3] int64: per solid voxel the voxel of the largest height among itself and its solid neighbours, of
    several the smallest linear index; -1 where not solid."""
    h = np.asarray(height, np.int32)
    R = h.shape[0]
    n = R ** 3
    idx = np.arange(n, dtype=np.int64).reshape(R, R, R)
    key = np.where(h > 0, h.astype(np.int64) * n + (n - 1 - idx), -1)         # orders by (height, -index); -1: not solid
    best = key.copy()
    for d in offsets(connectivity):
        v, w = _views(R, d)
        np.maximum(best[v], key[w], out=best[v])
    return np.where(h > 0, n - 1 - best % n, -1).ravel()


def basins_of(up):
    """up [n] -> basin [n]: the summit (up[v] == v) the links from v end at; -1 where not solid."""
    basin, solid = up.copy(), up >= 0
    while True:
        nxt = basin.copy()
        nxt[solid] = basin[basin[solid]]
        if np.array_equal(nxt, basin):
            return basin
        basin = nxt


def passes(height, basin, connectivity=26):
    """-> (a, b, top) [m]: the pairs of different basins a < b that hold neighbouring voxels u, w, and the largest min(height[u],
    height[w]) over those voxel pairs."""
    h = np.asarray(height, np.int32)
    R = h.shape[0]
    bas = basin.reshape(R, R, R)
    rows = []
    for d in offsets(connectivity, forward=True):
        v, w = _views(R, d)
        a, b = bas[v], bas[w]
        m = (a >= 0) & (b >= 0) & (a != b)
        rows.append(np.stack([np.minimum(a[m], b[m]), np.maximum(a[m], b[m]), np.minimum(h[v][m], h[w][m]).astype(np.int64)], 1))
    rows = np.concatenate(rows)
    if not len(rows):
        return (np.zeros(0, np.int64),) * 3
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    last = np.append((rows[1:, 0] != rows[:-1, 0]) | (rows[1:, 1] != rows[:-1, 1]), True)   # the largest pass of a pair comes last
    return rows[last, 0], rows[last, 1], rows[last, 2]


def structure(height, connectivity=26):
    """What does not depend on neck and min_peak: (height, basin [n], the summits in ascending order, passes())."""
    h = np.asarray(height, np.int32)
    basin = basins_of(ascent(h, connectivity))
    return h, basin, np.flatnonzero(basin == np.arange(basin.size)), passes(h, basin, connectivity)


def joined(h, a, b, top, neck=0.8, min_peak=0):
    """Which basin pairs are joined: min(peak_a, peak_b) <= min_peak, or (double)pass >= (neck * neck) * (double)min(peak_a, peak_b)."""
    flat = h.ravel()
    low = np.minimum(flat[a], flat[b]).astype(np.int64)
    return (low <= int(min_peak)) | (top.astype(f64) >= (f64(neck) * f64(neck)) * low.astype(f64))


def closure(summits, a, b):
    """The transitive closure of the joins (a[i], b[i]) by a sequential union-find -> per summit the smallest summit of its set."""
    pos = {int(s): i for i, s in enumerate(summits)}
    parent = list(range(len(summits)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(pos[x]), find(pos[y])
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return summits[[find(i) for i in range(len(summits))]] if len(summits) else summits


def merge(st, neck=0.8, min_peak=0):
    """structure() -> (labels [R,R,R] int32, count, basins): a part's label is 1 + the rank of its smallest voxel among the parts."""
    h, basin, summits, (a, b, top) = st
    j = joined(h, a, b, top, neck, min_peak)
    root = closure(summits, a[j], b[j])
    labels = np.zeros(basin.size, np.int32)
    vox = np.flatnonzero(basin >= 0)                                           # ascending: a part's first voxel is its smallest
    if len(vox):
        part = root[np.searchsorted(summits, basin[vox])]
        ids, first, inv = np.unique(part, return_index=True, return_inverse=True)
        rank = np.empty(len(ids), np.int64)
        rank[np.argsort(first)] = np.arange(len(ids))
        labels[vox] = (rank[inv] + 1).astype(np.int32)
    return labels.reshape(h.shape), int(labels.max(initial=0)), len(summits)


def label(height, connectivity=26, neck=0.8, min_peak=0):
    """One scene [R,R,R] int32 -> (labels [R,R,R] int32, count, basins)."""
    return merge(structure(height, connectivity), neck, min_peak)


def peaks(height, labels, count, max_parts):
    """-> peak [max_parts] int32 (the largest height in the part; 0: no such part), peak_voxel [max_parts] int32 (the smallest index in
    the part that has it; -1), for the labels 1 .. min(count, max_parts)."""
    h, lab = np.asarray(height, np.int32).ravel(), labels.ravel()
    n, m = h.size, min(count, max_parts)
    peak, peak_voxel = np.zeros(max_parts, np.int32), np.full(max_parts, -1, np.int32)
    at = np.flatnonzero((lab > 0) & (lab <= m))
    if len(at):
        best = np.full(m, -1, np.int64)
        np.maximum.at(best, lab[at] - 1, h[at].astype(np.int64) * n + (n - 1 - at))
        peak[:m], peak_voxel[:m] = best // n, n - 1 - best % n
    return peak, peak_voxel


KEYS = ('labels', 'count', 'basins', 'voxels', 'bbox', 'sums', 'peak', 'peak_voxel')


def parts(height, connectivity=26, max_parts=1024, neck=0.8, min_peak=0, structures=None):
    """height [B,R,R,R] int32 -> dict of labels [B,R,R,R] int32, count [B] int32, basins [B] int32, voxels [B,max] int32, bbox [B,max,6]
    int32, sums [B,max,3] int64, peak [B,max] int32, peak_voxel [B,max] int32.  structures: structure() of every scene under this
    connectivity, when the caller keeps them."""
    out = {k: [] for k in KEYS}
    for b, h in enumerate(np.asarray(height, np.int32)):
        lab, count, basins = merge(structures[b] if structures is not None else structure(h, connectivity), neck, min_peak)
        vox, bbox, sums = oref.statistics(lab, count, max_parts)
        for k, a in zip(out, (lab, np.int32(count), np.int32(basins), vox, bbox, sums, *peaks(h, lab, count, max_parts))):
            out[k].append(a)
    return {k: np.stack(a) for k, a in out.items()}


def d2_free(vol, level=0.0, lower=None, z_min=0):
    """vol [B,R,R,R] float32 -> [B,R,R,R] int32: gnr_volume_distance_fwd's d2_free, > 0 exactly at the solid voxels (distance_reference.edt)."""
    return np.stack([dref.edt(~dref.solid(v, level, lower, z_min))[0] for v in np.asarray(vol, np.float32)])
