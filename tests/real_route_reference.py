"""numpy statement of the reference's real-robot route -- TEST INFRASTRUCTURE ONLY (imported by tests/, never by the product).

Four functions of the reference, restated (the scipy.ndimage filters they call are the ones oracle/grasp_post_oracle.py restates,
pinned there against scipy itself):
  * process   src/nr/utils/grasp_utils.py:40-68   three thresholds: outside tsdf > 0.1 (:59), inside -1 < tsdf < -0.1 (:60), two masked
                                                  dilations (:61-63), widths kept in 0..12 (:66)
  * select    grasp_utils.py:78-94                threshold 0.90, maximum_filter(size=4), np.argwhere order
  * rank      grasp_utils.py:105 (sim_grasp)      np.argsort(scores)[::-1][:top_k]; stated here as descending score with ties by
                                                  ascending row (= ascending linear voxel index), which numpy does not promise: the
                                                  tests that compare with numpy assert that the scores in play are distinct
  * surface   src/nr/utils/draw_utils.py:355-377  voxels with rg[0] < vol < rg[1] in np.nonzero order, points = index * scale in float64
                                                  (open3d's scale about the origin), one colour or the value map of :364-370 in float32
Pinned by tests/golden/golden_real_route.npz, which the reference's own functions wrote (tools/make_real_route_goldens.py)."""
import numpy as np

from oracle import grasp_post_oracle as P

PROCESS_DEFAULTS = dict(sigma=1.0, min_width=0, max_width=12, outside=0.1, high=-0.1, low=-1)      # grasp_utils.py:45-47,59-60


def process(tsdf, qual, rot, width, sigma=1.0, min_width=0, max_width=12, outside=0.1, high=-0.1, low=-1):
    """[R,R,R] float32 volumes -> the processed quality volume (grasp_utils.py:53-66)."""
    f = np.float32
    q = P.gaussian_filter_nearest(qual, sigma)
    out = tsdf > f(outside)
    inside = (f(low) < tsdf) & (tsdf < f(high))
    valid = P.masked_dilation(out, ~inside, 2)
    q[~valid] = 0.0
    q[(width < f(min_width)) | (width > f(max_width))] = 0.0
    return q


def select(qual, rot, width, threshold=0.90, size=4):
    """-> index [N,3] (argwhere order), score [N], quat [N,4] as stored, width [N]   (grasp_utils.py:78-94)."""
    q = qual.copy()
    q[q < np.float32(threshold)] = 0.0
    q = np.where(q == P.maximum_filter_reflect(q, size), q, np.float32(0.0))
    idx = np.argwhere(q != 0)
    i, j, k = idx[:, 0], idx[:, 1], idx[:, 2]
    return idx, q[i, j, k], rot[:, i, j, k].T, width[i, j, k]


def rank(score, top_k=None):
    """Rows of a select() result, best score first, equal scores in ascending row order; the first top_k of them."""
    order = np.lexsort((np.arange(len(score)), -np.asarray(score, np.float64)))
    return order if top_k is None else order[:top_k]


def surface(vol, rg=(-0.2, 0.2), bound=(-1, 1), color=(0, 0, 1), scale=0.3 / 40):
    """vol [R,R,R] float32 -> index [N,3] int64, points [N,3] float64, colors [N,3] float32."""
    f = np.float32
    idx = np.transpose(((vol > f(rg[0])) & (vol < f(rg[1]))).nonzero())
    points = idx.astype(np.float64) * scale
    if color is None:
        v = vol[idx[:, 0], idx[:, 1], idx[:, 2]].astype(f)
        a, b = f(bound[0]), f(bound[1])
        m = (a + b) / f(2)
        r = np.where(v <= m, v - a, -v + b)
        g = np.where(v <= m, f(0), f(1) - r)
        bl = np.where(v <= m, f(1) - r, f(0))
        colors = np.stack([r, g, bl], -1).astype(f)
    else:
        colors = np.asarray([color], f).repeat(len(idx), 0)
    return idx, points, colors
