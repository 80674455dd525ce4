"""Float64 statement (plain numpy) of the finger closure of a grasp against a scalar volume -- TEST INFRASTRUCTURE ONLY, the arbiter of
k_finger_closure in csrc/gnr_hand.hip (include/gnr.h, gnr_finger_closure_fwd, has the same words).
The frame, the opening and the pose are hand_reference's (x the thickness, y the closing direction, z the approach).  Each finger's inner
face carries a lattice of pad rays over x in [-h/2, h/2] and z in [0, depth]; finger 0 starts at y = -hw and moves towards +y, finger 1
at +hw towards -y, both to the centre plane at the latest.  A ray marches f(t) = value - level over the travel t in steps of at most
`spacing` voxels, brackets the first change from f >= 0 to f < 0 and refines it as the ray cast does (raycast_reference.py:112-118:
halvings, then one secant step).  A finger stops at the smallest t* of its rays; there the gradient of the trilinear interpolant gives
the cosine between the surface and the closing direction.  Vectorised over the rays of a grasp; every line below is ONE correctly
rounded IEEE float64 operation per ray in the order written (numpy never contracts a multiply and an add), so the device's rows are
compared with np.array_equal on the bits."""
import math

import numpy as np

from hand_reference import FREE, matrix, opening_of, positions
from raycast_reference import trilinear

f32, f64 = np.float32, np.float64
DEFAULTS = dict(height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, opening=None, spacing=0.5, approach=0.05, level=0.0,
                bisections=4)


def pads(scale, height=0.004, depth=0.05, spacing=0.5):
    """The pad rays of one finger in ordinal order i_x * n_z + i_z: (l_x [n], l_z [n], n_x, n_z) with n = max(2, ceil(extent / cell) + 1),
    step = extent / (n - 1), l_x = -0.5 h + i_x step_x, l_z = i_z step_z."""
    cell, h, d = f64(spacing) * f64(scale), f64(height), f64(depth)
    nx, nz = max(2.0, math.ceil(h / cell) + 1.0), max(2.0, math.ceil(d / cell) + 1.0)
    sx, sz = h / f64(nx - 1.0), d / f64(nz - 1.0)
    ix, iz = (a.ravel().astype(f64) for a in np.meshgrid(np.arange(int(nx)), np.arange(int(nz)), indexing='ij'))
    return -0.5 * h + ix * sx, iz * sz, int(nx), int(nz)


def steps(hw, scale, spacing=0.5):
    """(n_y, ds): the march intervals of a finger that travels hw metres at most, n_y = max(1, ceil(hw / cell)), ds = hw / n_y."""
    ny = max(1.0, math.ceil(f64(hw) / (f64(spacing) * f64(scale))))
    return int(ny), f64(hw) / f64(ny)


def reads(w, scale, bisections=4, **hand):
    """The most volume reads of a grasp opened to w metres: 2 n_x n_z (n_y + 1 + bisections + 2), a function of the parameters alone."""
    _, _, nx, nz = pads(scale, hand.get('height', 0.004), hand.get('depth', 0.05), hand.get('spacing', 0.5))
    ny, _ = steps(0.5 * f64(w), scale, hand.get('spacing', 0.5))
    return 2.0 * nx * nz * (ny + 1.0 + bisections + 2.0)


def gradient(v, p):
    """The gradient [3] (lattice units) of the trilinear interpolant of v [R,R,R] float64 at p [3]: trilinear's base corners and t's."""
    R = v.shape[0]
    with np.errstate(invalid='ignore'):
        b = [np.fmin(np.fmax(np.floor(c), 0.0), f64(R - 2)) for c in p]
        tx, ty, tz = (c - k for c, k in zip(p, b))
    ix, iy, iz = (int(k) for k in b)
    c = lambda dx, dy, dz: v[ix + dx, iy + dy, iz + dz]
    with np.errstate(invalid='ignore'):
        c00 = c(0, 0, 0) + tz * (c(0, 0, 1) - c(0, 0, 0))
        c01 = c(0, 1, 0) + tz * (c(0, 1, 1) - c(0, 1, 0))
        c10 = c(1, 0, 0) + tz * (c(1, 0, 1) - c(1, 0, 0))
        c11 = c(1, 1, 0) + tz * (c(1, 1, 1) - c(1, 1, 0))
        c0 = c00 + ty * (c01 - c00)
        c1 = c10 + ty * (c11 - c10)
        gx = c1 - c0
        e0, e1 = c01 - c00, c11 - c10
        gy = e0 + tx * (e1 - e0)
        d00, d01, d10, d11 = c(0, 0, 1) - c(0, 0, 0), c(0, 1, 1) - c(0, 1, 0), c(1, 0, 1) - c(1, 0, 0), c(1, 1, 1) - c(1, 1, 0)
        d0 = d00 + ty * (d01 - d00)
        d1 = d10 + ty * (d11 - d10)
        gz = d0 + tx * (d1 - d0)
    return np.array([gx, gy, gz])


def closure(vol, pos, quat, width, scale, opening=None, level=0.0, bisections=4, height=0.004, depth=0.05, spacing=0.5, details=None,
            finger_width=0.004, tail_length=0.04, approach=0.05):
    """The statement for one grasp: vol [R,R,R] float32, pos [3] float64 (lattice units), quat [4] float32, width float32 (voxels);
    finger_width, tail_length and approach belong to the hand's parameters and are not used.
    -> (travel [2] float32, cosine [2] float32, contact [2] int32, closed float32).
    details: a dict that receives `t` [2 n] (every ray's t*, NaN without a contact; finger 0's rays first) and `point` [2,3] (the contact
    points in lattice units, NaN without)."""
    vol = np.ascontiguousarray(vol, f32)
    R = vol.shape[0]
    assert vol.shape == (R, R, R) and R >= 2
    v64, top, level = vol.astype(f64), f64(R - 1), f64(level)
    w = opening_of(width, R, scale, opening)
    hw = 0.5 * w
    lx, lz, nx, nz = pads(scale, height, depth, spacing)
    n = nx * nz
    lx, lz, sign = np.tile(lx, 2), np.tile(lz, 2), np.repeat([-1.0, 1.0], n)     # finger 0: l_y = -u, finger 1: l_y = u
    ny, ds = steps(hw, scale, spacing)

    def at(t, k):
        u = hw - t
        return positions(pos, quat, np.stack([lx[k], sign[k] * u, lz[k]], 1), scale)

    def f(t, k):
        p = at(t, k)
        with np.errstate(invalid='ignore'):
            ok = np.flatnonzero(np.all((0.0 <= p) & (p <= top), axis=1))
        value = np.full(len(p), FREE)
        value[ok] = trilinear(v64, p[ok, 0], p[ok, 1], p[ok, 2])
        return value - level

    every = np.arange(2 * n)
    tp = np.full(2 * n, np.fmin(0.0 * ds, hw))
    fp = f(tp, every)
    start = fp < 0.0                                                             # the pad starts inside: t* = 0
    hit = np.zeros(2 * n, bool)
    A, B, fA, fB = (np.zeros(2 * n) for _ in range(4))
    for k in range(1, ny + 1):
        live = np.flatnonzero(~start & ~hit)
        if not len(live):
            break
        tk = np.fmin(f64(k) * ds, hw)
        fk = f(np.full(len(live), tk), live)
        now = (fp[live] >= 0.0) & (fk < 0.0)                                     # outside -> inside
        j = live[now]
        A[j], B[j], fA[j], fB[j] = tp[j], tk, fp[j], fk[now]
        hit[j] = True
        tp[live], fp[live] = tk, fk
    j = np.flatnonzero(hit)
    A, B, fA, fB = A[j], B[j], fA[j], fB[j]
    for _ in range(int(bisections)):
        m = 0.5 * (A + B)
        fm = f(m, j)
        inside = fm < 0.0
        A, fA = np.where(inside, A, m), np.where(inside, fA, fm)
        B, fB = np.where(inside, m, B), np.where(inside, fm, fB)
    t = np.full(2 * n, np.nan)
    t[j] = A + (B - A) * (fA / (fA - fB))
    t[start] = 0.0
    travel, cosine, contact = np.zeros(2, f64), np.zeros(2, f64), np.full(2, -1, np.int32)
    point = np.full((2, 3), np.nan)
    a = matrix(quat)[:, 1]
    for c in range(2):
        mine = t[c * n:(c + 1) * n]
        has = ~np.isnan(mine)
        travel[c] = hw
        if not has.any():
            continue
        o = int(np.argmin(np.where(has, mine, np.inf)))                          # the first that attains the minimum
        travel[c], contact[c] = mine[o], o
        point[c] = at(mine[o:o + 1], np.array([c * n + o]))[0]
        g = gradient(v64, point[c])
        with np.errstate(invalid='ignore'):
            dot = (g[0] * a[0] + g[1] * a[1]) + g[2] * a[2]
            norm = np.fmax(np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]), 1e-12)
            cosine[c] = dot / norm if c else -dot / norm
    closed = (hw - travel[0]) + (hw - travel[1])
    if details is not None:
        details.update(t=t, point=point)
    return travel.astype(f32), cosine.astype(f32), contact, f32(closed)


def closure_rows(vol, pos, quat, width, count, scale, top_k=None, out=None, **kw):
    """One scene: rows r < min(count, top_k or max_n, max_n) of pos [max_n,3], quat [max_n,4], width [max_n]; the other rows of `out` =
    (travel [max_n,2] float32, cosine [max_n,2] float32, contact [max_n,2] int32, closed [max_n] float32) are left untouched (zeros
    without `out`)."""
    pos = np.asarray(pos, f64)
    max_n = len(pos)
    n = max(0, min(int(count), int(top_k or max_n), max_n))
    out = (np.zeros((max_n, 2), f32), np.zeros((max_n, 2), f32), np.zeros((max_n, 2), np.int32), np.zeros(max_n, f32)) if out is None else out
    for r in range(n):
        for dst, src in zip(out, closure(vol, pos[r], quat[r], width[r], scale, **kw)):
            dst[r] = src
    return out
