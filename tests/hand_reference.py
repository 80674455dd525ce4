"""Float64 statement (plain numpy) of the gripper clearance of a grasp against a scalar volume -- TEST INFRASTRUCTURE ONLY, the arbiter
of csrc/gnr_hand.hip (include/gnr.h, gnr_hand_clearance_fwd, has the same words).
The hand is four boxes in the grasp frame (z the approach, y the closing direction, x the thickness): two fingers, the palm and the
tail of draw_utils.draw_gripper_o3d.  Every box carries a lattice of samples at most `spacing` voxels apart; along z the lattice
continues backwards over `approach` metres: the places the box's samples pass through while the hand comes in from the pre-grasp
pose.  The clearance is the smallest trilinear value of the volume over the samples inside the lattice -- at the grasp (i_z >= 0) and
on the approach (all samples).  Vectorised over the samples of a grasp; every line below is ONE correctly rounded IEEE float64
operation per sample in the order written (numpy never contracts a multiply and an add), so the device's rows are compared with
np.array_equal on the bits."""
import math

import numpy as np

from raycast_reference import trilinear

f32, f64 = np.float32, np.float64
DEFAULTS = dict(height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, opening=None, spacing=0.5, approach=0.05)
FREE = 1.0                                                                     # the volume's upper clip: what a hand outside the box reports
BOXES = ('left finger', 'right finger', 'palm', 'tail')


def opening_of(width, R, scale, opening=None):
    """The hand's opening in metres: `opening` for every grasp, or the row's own width (voxels, float32); clamped to [0, R] voxels with
    fmin(fmax(.)) -- fmax drops a NaN."""
    wv = f64(opening) / f64(scale) if opening is not None else f64(f32(width))
    with np.errstate(invalid='ignore'):
        wv = np.fmin(np.fmax(wv, 0.0), f64(R))
    return wv * f64(scale)


def boxes_of(w, height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05):
    """(lo [3], extent [3]) of the four boxes of a hand opened to w metres, in BOXES order."""
    h, f, t, d, w = f64(height), f64(finger_width), f64(tail_length), f64(depth), f64(w)
    hw = 0.5 * w
    return [((-0.5 * h, -hw - f, -f), (h, f, d + f)), ((-0.5 * h, hw, -f), (h, f, d + f)),
            ((-0.5 * h, -hw, -f), (h, w, f)), ((-0.5 * h, -0.5 * f, -t - f), (h, f, t))]


def lattice(w, scale, height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, spacing=0.5, approach=0.05):
    """The sample lattices of the four boxes: per box (lo [3], step [3], n [3] ints, m) with n_a = max(2, ceil(e_a / cell) + 1),
    step_a = e_a / (n_a - 1), cell = spacing * scale, and m = ceil(approach / step_z) further z layers behind the box (0 without an
    approach)."""
    cell = f64(spacing) * f64(scale)
    out = []
    for lo, ext in boxes_of(w, height, finger_width, tail_length, depth):
        n = [max(2.0, math.ceil(e / cell) + 1.0) for e in ext]
        step = [f64(e) / f64(k - 1.0) for e, k in zip(ext, n)]
        m = math.ceil(f64(approach) / step[2]) if approach > 0 else 0
        out.append((lo, step, [int(k) for k in n], int(m)))
    return out


def totals(w, scale, **hand):
    """(samples at the grasp, samples on the approach) of a hand opened to w metres: a function of the parameters and the width alone."""
    lat = lattice(w, scale, **hand)
    return sum(n[0] * n[1] * n[2] for _, _, n, _ in lat), sum(n[0] * n[1] * (n[2] + m) for _, _, n, m in lat)


def samples(w, scale, **hand):
    """Every sample in ordinal order (box, then i_x, then i_y, then i_z ascending from -m): local [N,3] float64 metres, box [N] and
    i_z [N] ints."""
    loc, box, izs = [], [], []
    for k, (lo, step, n, m) in enumerate(lattice(w, scale, **hand)):
        ix, iy, iz = (a.ravel() for a in np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(-m, n[2]), indexing='ij'))
        loc.append(np.stack([lo[0] + ix.astype(f64) * step[0], lo[1] + iy.astype(f64) * step[1], lo[2] + iz.astype(f64) * step[2]], 1))
        box.append(np.full(len(ix), k))
        izs.append(iz)
    return np.concatenate(loc), np.concatenate(box), np.concatenate(izs)


def matrix(quat):
    """The rotation of a float32 quaternion (x, y, z, w): float64, divided by max(|q|, 1e-12), tsdf.rotation_matrix's formula."""
    x, y, z, w = (f64(c) for c in np.asarray(quat, f32))
    with np.errstate(invalid='ignore', over='ignore'):
        n = np.fmax(np.sqrt(((x * x + y * y) + z * z) + w * w), 1e-12)
        x, y, z, w = x / n, y / n, z / n, w / n
        return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                         [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                         [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])


def positions(pos, quat, local, scale):
    """Lattice positions [N,3] of the local samples of a grasp at pos (lattice units): p_a = pos_a + ((M[a][0] l_x + M[a][1] l_y) +
    M[a][2] l_z) / scale."""
    M, g, scale = matrix(quat), np.asarray(pos, f64), f64(scale)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([g[a] + ((M[a, 0] * local[:, 0] + M[a, 1] * local[:, 1]) + M[a, 2] * local[:, 2]) / scale for a in range(3)], 1)


def clearance(vol, pos, quat, width, scale, opening=None, details=None, **hand):
    """The statement for one grasp: vol [R,R,R] float32, pos [3] float64 (lattice units), quat [4] float32, width float32 (voxels).
    -> (clearance [2] float32, worst [2] int32, inside [2] int32): column 0 at the grasp, column 1 on the approach.
    details: a dict that receives `p` [N,3] (every sample's lattice position), `value` [N] (NaN where skipped), `at_grasp` [N] bool."""
    vol = np.ascontiguousarray(vol, f32)
    R = vol.shape[0]
    assert vol.shape == (R, R, R) and R >= 2
    v64, top = vol.astype(f64), f64(R - 1)
    w = opening_of(width, R, scale, opening)
    local, _, iz = samples(w, scale, **hand)
    p = positions(pos, quat, local, scale)
    with np.errstate(invalid='ignore'):
        ok = np.all((0.0 <= p) & (p <= top), axis=1)
    j = np.flatnonzero(ok)
    val = trilinear(v64, p[j, 0], p[j, 1], p[j, 2])
    out = (np.full(2, FREE, f32), np.full(2, -1, np.int32), np.zeros(2, np.int32))
    for c, sel in enumerate((iz[j] >= 0, np.ones(len(j), bool))):
        out[2][c] = np.count_nonzero(sel)
        if out[2][c]:
            k = np.flatnonzero(sel)[np.argmin(val[sel])]                       # the first that attains the minimum
            out[1][c] = j[k]
            out[0][c] = f32(np.fmin(val[k], FREE))
    if details is not None:
        value = np.full(len(p), np.nan)
        value[j] = val
        details.update(p=p, value=value, at_grasp=iz >= 0)
    return out


def clearance_rows(vol, pos, quat, width, count, scale, top_k=None, out=None, **hand):
    """One scene: rows r < min(count, top_k or max_n, max_n) of pos [max_n,3], quat [max_n,4], width [max_n]; the other rows of `out` =
    (clearance [max_n,2] float32, worst [max_n,2] int32, inside [max_n,2] int32) are left untouched (zeros without `out`)."""
    pos = np.asarray(pos, f64)
    max_n = len(pos)
    n = max(0, min(int(count), int(top_k or max_n), max_n))
    out = (np.zeros((max_n, 2), f32), np.zeros((max_n, 2), np.int32), np.zeros((max_n, 2), np.int32)) if out is None else out
    for r in range(n):
        for dst, src in zip(out, clearance(vol, pos[r], quat[r], width[r], scale, **hand)):
            dst[r] = src
    return out
