"""Float64 statement (plain numpy) of the ray cast of a scalar volume into depth (and gradient) images -- TEST INFRASTRUCTURE ONLY,
the arbiter of csrc/gnr_raycast.hip (include/gnr.h, gnr_volume_raycast_fwd, has the same words).
One ray through every integer pixel centre; the parameter s of a ray is camera-z depth in metres (tsdf_reference.render_depth's
convention).  Vectorised over the pixels of a view; every line below is ONE correctly rounded IEEE float64 operation per pixel in
the order written (numpy never contracts a multiply and an add), so the device's images are compared with np.array_equal on the
bits.  No result rests on inf / NaN arithmetic: a direction component that is zero is decided on its own, before any division."""
import math

import numpy as np

f32, f64 = np.float32, np.float64


def max_samples(R, step):
    """The most march intervals of a ray: the box's diagonal in voxels over the step, plus one for the roundings (the device's loop
    bound; it never binds on a well-formed camera)."""
    return int(math.ceil(math.sqrt(3.0) * (R - 1) / float(step))) + 1


def trilinear(v, px, py, pz):
    """v [R,R,R] or [R,R,R,C] float64 at the index positions p: base b = clamp(floor(p), 0, R-2), t = p - b, lerp along z, then y,
    then x, each a + t * (b - a)."""
    R = v.shape[0]
    b = [np.clip(np.floor(p), 0.0, float(R - 2)) for p in (px, py, pz)]
    tx, ty, tz = px - b[0], py - b[1], pz - b[2]
    ix, iy, iz = (c.astype(np.int64) for c in b)
    if v.ndim == 4:
        tx, ty, tz = tx[..., None], ty[..., None], tz[..., None]
    c = lambda dx, dy, dz: v[ix + dx, iy + dy, iz + dz]
    c00 = c(0, 0, 0) + tz * (c(0, 0, 1) - c(0, 0, 0))
    c01 = c(0, 1, 0) + tz * (c(0, 1, 1) - c(0, 1, 0))
    c10 = c(1, 0, 0) + tz * (c(1, 0, 1) - c(1, 0, 0))
    c11 = c(1, 1, 0) + tz * (c(1, 1, 1) - c(1, 1, 0))
    c0 = c00 + ty * (c01 - c00)
    c1 = c10 + ty * (c11 - c10)
    return c0 + tx * (c1 - c0)


def raycast(vol, poses, Ks, h, w, origin, scale, iso=0.0, step=0.5, bisections=4, near=0.0, far=np.inf, gradient=None, details=None):
    """vol [R,R,R] float32; poses [V,3,4] world->camera, Ks [V,3,3] (float32: they convert to float64 exactly); origin [3], scale, step,
    near, far float64; lattice point i sits at world origin + i * scale.
    -> depth [V,h,w] float32 (0: no surface), and (depth, gradient [V,h,w,3] float32) when a gradient volume [R,R,R,3] is given.
    details: a dict that receives `crosses` [V,h,w] bool (the ray crosses the box: s0 < s1) and `s` [V,h,w] float64 (s* before the
    rounding to float32, 0 on a miss)."""
    vol = np.ascontiguousarray(vol, f32)
    R = vol.shape[0]
    assert vol.shape == (R, R, R) and R >= 2
    v64 = vol.astype(f64)
    iso64 = f64(f32(iso))
    g64 = None
    if gradient is not None:
        g64 = np.ascontiguousarray(gradient, f32).astype(f64)
        assert g64.shape == (R, R, R, 3)
    poses, Ks = np.asarray(poses, f32).astype(f64), np.asarray(Ks, f32).astype(f64)
    V = poses.shape[0]
    o = np.asarray(origin, f64)
    scale, step, near, far = f64(scale), f64(step), f64(near), f64(far)
    top, nmax = f64(R - 1), max_samples(R, step)
    depth = np.zeros((V, h, w), f32)
    gout = np.zeros((V, h, w, 3), f32)
    crosses, sstar = np.zeros((V, h, w), bool), np.zeros((V, h, w))
    vs, us = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing='ij')
    vs, us = vs.ravel(), us.ravel()
    for view in range(V):
        Rm, t, K = poses[view, :, :3], poses[view, :, 3], Ks[view]
        dcx = (us - K[0, 2]) / K[0, 0]
        dcy = (vs - K[1, 2]) / K[1, 1]
        e, d = [], []
        for a in range(3):
            eye = -((Rm[0, a] * t[0] + Rm[1, a] * t[1]) + Rm[2, a] * t[2])
            dw = (Rm[0, a] * dcx + Rm[1, a] * dcy) + Rm[2, a]                    # the camera ray's z is 1: R[2,a] * 1 is R[2,a]
            e.append((eye - o[a]) / scale)
            d.append(dw / scale)
        s0, s1 = np.full(h * w, near), np.full(h * w, far)
        ok = np.ones(h * w, bool)
        for a in range(3):                                                       # the slabs, x then y then z
            zero = d[a] == 0.0
            dd = np.where(zero, 1.0, d[a])
            ta, tb = (0.0 - e[a]) / dd, (top - e[a]) / dd
            s0 = np.where(zero, s0, np.maximum(s0, np.minimum(ta, tb)))          # (max and min are exact: their order is free)
            s1 = np.where(zero, s1, np.minimum(s1, np.maximum(ta, tb)))
            ok &= ~zero | ((0.0 <= e[a]) & (e[a] <= top))
        ok &= (s0 < s1) & np.isfinite(s1)
        idx = np.flatnonzero(ok)
        crosses[view].ravel()[idx] = True
        if not len(idx):
            continue
        dx, dy, dz, s0, s1 = d[0][idx], d[1][idx], d[2][idx], s0[idx], s1[idx]
        ds = step / np.sqrt((dx * dx + dy * dy) + dz * dz)
        n = np.minimum(np.ceil((s1 - s0) / ds), float(nmax))
        f = lambda s, k: trilinear(v64, e[0] + s * dx[k], e[1] + s * dy[k], e[2] + s * dz[k]) - iso64
        every = np.arange(len(idx))
        sp = np.minimum(s0 + 0.0 * ds, s1)
        fp = f(sp, every)
        hit = np.zeros(len(idx), bool)
        A, B, fA, fB = (np.zeros(len(idx)) for _ in range(4))
        k = 1
        while True:
            live = np.flatnonzero(~hit & (n >= k))
            if not len(live):
                break
            sk = np.minimum(s0[live] + float(k) * ds[live], s1[live])
            fk = f(sk, live)
            now = (fp[live] >= 0.0) & (fk < 0.0)                                 # outside -> inside
            j = live[now]
            A[j], B[j], fA[j], fB[j] = sp[live][now], sk[now], fp[live][now], fk[now]
            hit[j] = True
            sp[live], fp[live] = sk, fk
            k += 1
        j = np.flatnonzero(hit)
        A, B, fA, fB = A[j], B[j], fA[j], fB[j]
        for _ in range(int(bisections)):
            m = 0.5 * (A + B)
            fm = f(m, j)
            inside = fm < 0.0
            A, fA = np.where(inside, A, m), np.where(inside, fA, fm)
            B, fB = np.where(inside, m, B), np.where(inside, fm, fB)
        s = A + (B - A) * (fA / (fA - fB))
        depth[view].ravel()[idx[j]] = s.astype(f32)
        sstar[view].ravel()[idx[j]] = s
        if g64 is not None:
            gout[view].reshape(-1, 3)[idx[j]] = trilinear(g64, e[0] + s * dx[j], e[1] + s * dy[j], e[2] + s * dz[j]).astype(f32)
    if details is not None:
        details['crosses'], details['s'] = crosses, sstar
    return (depth, gout) if gradient is not None else depth
