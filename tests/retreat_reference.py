"""Statement (plain numpy) of the retreat of a grasp's held part through a label volume -- TEST INFRASTRUCTURE ONLY, the arbiter of
csrc/gnr_retreat.hip (include/gnr.h, gnr_grasp_retreat_fwd, has the same words).
The voxels that carry the held label inside the label's box move K steps along the retreat -- back along the hand's own z, or along
world +z (lattice axis 2) for a side grasp -- by integer offsets rint(u * (k * sl)); a step counts the moving voxels that land on a
label that is neither 0 nor their own; a position outside the lattice hits nothing.  The float64 lines are ONE correctly rounded IEEE
operation each in the order written (numpy never contracts a multiply and an add); everything else is integers; the device's rows are
compared with np.array_equal on the bits.  Vectorised over the moving voxels and the steps; tests/test_grasp_retreat.py holds the
literal restatement, voxel by voxel, and compares."""
import math

import numpy as np

from hand_reference import matrix

f32, f64 = np.float32, np.float64
DEFAULTS = dict(retreat=0.1, step=0.5, side_cos=0.5, tolerance=0)
MAX_STEPS = 1024
KEYS = ('blocked_step', 'blocker', 'overlap', 'moved', 'side', 'travel')
TYPES = (np.int32,) * 5 + (f32,)


def steps(retreat, step, scale):
    """(T, K, sl): T = retreat / scale voxels in K = max(1, ceil(T / step)) steps of sl = T / K."""
    T = f64(retreat) / f64(scale)
    K = int(max(1.0, math.ceil(T / f64(step))))
    assert K <= MAX_STEPS
    return T, K, T / f64(K)


def direction(quat, side_cos=0.5):
    """(u [3] float64, side): u_a = -M[a][2] of hand_reference.matrix; side = -M[2][2] < side_cos, and then u = (0, 0, 1).  u is None
    when a component is not a number."""
    M = matrix(quat)
    u = np.array([-M[0, 2], -M[1, 2], -M[2, 2]])
    if np.isnan(u).any():
        return None, 0
    side = int(u[2] < f64(side_cos))
    return (np.array([0.0, 0.0, 1.0]) if side else u), side


def offsets(u, K, sl, R):
    """[K,3] int64: o_a = rint(u_a * (k * sl)) for k = 1 .. K; an offset of R and more moves every voxel out, so it is held at +-R."""
    k = np.arange(1, K + 1).astype(f64)
    with np.errstate(over='ignore'):
        d = np.rint(u[None, :] * (k * f64(sl))[:, None])
    return np.clip(d, -f64(R), f64(R)).astype(np.int64)


def moving(labels, bbox, held):
    """[m,3] int64: the voxels of the held label's box, clamped to the lattice, that carry the label, in ascending linear index."""
    R, L = labels.shape[0], int(held)
    if L < 1 or L > len(bbox):
        return np.zeros((0, 3), np.int64)
    lo = np.maximum(np.asarray(bbox[L - 1][:3], np.int64), 0)
    hi = np.minimum(np.asarray(bbox[L - 1][3:], np.int64), R - 1)
    if (lo > hi).any():
        return np.zeros((0, 3), np.int64)
    sub = labels[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    return np.argwhere(sub == np.int32(L)).astype(np.int64) + lo                # (argwhere: C order, ascending linear index)


def retreat(labels, bbox, held, quat, scale, retreat=0.1, step=0.5, side_cos=0.5, tolerance=0, details=None):
    """The statement for one grasp: labels [R,R,R] int32, bbox [max_parts,6] int32, held int32, quat [4] float32.
    -> (blocked_step, blocker, overlap, moved, side int32, travel float32).  details: a dict that receives `hits` [K] and `offsets`
    [K,3]."""
    labels = np.asarray(labels, np.int32)
    R = labels.shape[0]
    assert labels.shape == (R, R, R) and R >= 2
    T, K, sl = steps(retreat, step, scale)
    free = f32(T * f64(scale))
    u, side = direction(quat, side_cos)
    if u is None:
        return np.int32(0), np.int32(0), np.int32(0), np.int32(0), np.int32(0), free
    L = np.int32(held)
    v = moving(labels, np.asarray(bbox, np.int32).reshape(-1, 6), L)
    o = offsets(u, K, sl, R)
    t = v[None, :, :] + o[:, None, :]                                          # [K,m,3]
    inside = np.all((t >= 0) & (t <= R - 1), axis=2)
    tc = np.clip(t, 0, R - 1)
    at = labels[tc[..., 0], tc[..., 1], tc[..., 2]]
    hit = inside & (at != 0) & (at != L)
    hits = hit.sum(axis=1)
    if details is not None:
        details.update(hits=hits, offsets=o)
    over = np.flatnonzero(hits > int(tolerance))
    blocked = int(over[0]) + 1 if len(over) else 0
    blocker = int(at[blocked - 1, np.flatnonzero(hit[blocked - 1])[0]]) if blocked else 0      # (v ascends in linear index)
    travel = f32((f64(blocked - 1) * sl) * f64(scale)) if blocked else free
    return np.int32(blocked), np.int32(blocker), np.int32(hits.max()), np.int32(len(v)), np.int32(side), travel


def retreat_rows(labels, bbox, held, quat, count, scale, top_k=None, out=None, **params):
    """One scene: rows r < min(count, top_k or max_n, max_n) of held [max_n], quat [max_n,4]; the other rows of `out` = (blocked_step,
    blocker, overlap, moved, side [max_n] int32 each, travel [max_n] float32) are left untouched (zeros without `out`)."""
    held = np.asarray(held, np.int32)
    max_n = len(held)
    n = max(0, min(int(count), int(top_k or max_n), max_n))
    out = tuple(np.zeros(max_n, t) for t in TYPES) if out is None else out
    for r in range(n):
        for dst, src in zip(out, retreat(labels, bbox, held[r], quat[r], scale, **params)):
            dst[r] = src
    return out
