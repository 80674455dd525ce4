"""Float64 statement (plain numpy) of the view colours of surface points -- TEST INFRASTRUCTURE ONLY, the arbiter of
csrc/gnr_surface_color.hip (include/gnr.h, gnr_surface_color_points_fwd / gnr_surface_color_pixels_fwd, has the same words).
A point of the volume's surface takes the colour of the source images it is seen in: per view, in view order, it must project into
the image, face the camera by the volume's own normal, and reach the camera without a sample below the level on the way; the colour
is the mean of the views' bilinear taps weighted by the cosines.  Vectorised over the points; every line below is ONE correctly
rounded IEEE float64 operation per point in the order written (numpy never contracts a multiply and an add), so the device's results
are compared with np.array_equal on the bits."""
import numpy as np

from raycast_reference import max_samples, trilinear

f32, f64 = np.float32, np.float64
DEFAULTS = dict(iso=0.0, step=0.5, bias=1.5, cos_min=0.0, fill=(0.0, 0.0, 0.0))


def camera(pose, K):
    """(R [3,3], t [3], eye [3], fx, fy, cx, cy) of one float32 camera, in float64: eye_a = -((R[0][a] t[0] + R[1][a] t[1]) + R[2][a] t[2])."""
    pose, K = np.asarray(pose, f32).astype(f64), np.asarray(K, f32).astype(f64)
    Rm, t = pose[:3, :3], pose[:3, 3]
    eye = np.array([-((Rm[0, a] * t[0] + Rm[1, a] * t[1]) + Rm[2, a] * t[2]) for a in range(3)])
    return Rm, t, eye, K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def bilinear(img, u, v):
    """img [H,W] float64 at (u, v): base clamp(floor(.), 0, size-2) per axis, lerp along x in both rows, then along y."""
    H, W = img.shape
    bx, by = np.clip(np.floor(u), 0.0, float(W - 2)), np.clip(np.floor(v), 0.0, float(H - 2))
    tx, ty = u - bx, v - by
    ix, iy = bx.astype(np.int64), by.astype(np.int64)
    r0 = img[iy, ix] + tx * (img[iy, ix + 1] - img[iy, ix])
    r1 = img[iy + 1, ix] + tx * (img[iy + 1, ix + 1] - img[iy + 1, ix])
    return r0 + ty * (r1 - r0)


def color_world(vol, x, images, poses, Ks, origin, scale, iso=0.0, step=0.5, bias=1.5, cos_min=0.0, fill=(0.0, 0.0, 0.0), details=None):
    """The statement for N world points x [N,3] float64 of one scene: vol [R,R,R] float32, images [V,3,H,W] float32, poses [V,3,4],
    Ks [V,3,3] float32; lattice point i sits at world origin + i * scale.
    -> colors [N,3] float32, weight [N] float32, views [N] int32.
    details: a dict that receives `p` [N,3], `g` [N,3] (the volume's gradient at p), and per view [V,N] `inside` (the point projects
    into the image), `cos`, `occluded` (the march of a facing candidate met a sample below the level) and `used`."""
    vol = np.ascontiguousarray(vol, f32)
    R = vol.shape[0]
    assert vol.shape == (R, R, R) and R >= 2
    v64, iso64 = vol.astype(f64), f64(f32(iso))
    images = np.asarray(images, f32).astype(f64)
    V, _, H, W = images.shape
    assert 1 <= V <= 32 and H >= 2 and W >= 2
    o, scale, step, bias, cos_min = np.asarray(origin, f64), f64(scale), f64(step), f64(bias), f64(cos_min)
    fill64 = np.asarray(fill, f32).astype(f64)
    top, nmax = f64(R - 1), max_samples(R, step)
    x = np.asarray(x, f64).reshape(-1, 3)
    N = len(x)
    with np.errstate(all='ignore'):
        p = [(x[:, a] - o[a]) / scale for a in range(3)]
        half = lambda a, s: [p[j] + s if j == a else p[j] for j in range(3)]
        g = [trilinear(v64, *half(a, 0.5)) - trilinear(v64, *half(a, -0.5)) for a in range(3)]
        n2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        live = ~(n2 == 0.0)
        norm = np.sqrt(n2)
        acc, wsum, mask = np.zeros((3, N)), np.zeros(N), np.zeros(N, np.uint32)
        D = {k: np.zeros((V, N), t) for k, t in (('inside', bool), ('cos', f64), ('occluded', bool), ('used', bool))}
        for view in range(V):
            Rm, t, eye, fx, fy, cx, cy = camera(poses[view], Ks[view])
            pc = [((Rm[a, 0] * x[:, 0] + Rm[a, 1] * x[:, 1]) + Rm[a, 2] * x[:, 2]) + t[a] for a in range(3)]
            ok = live & (pc[2] > 0.0)
            u, w = pc[0] * fx / pc[2] + cx, pc[1] * fy / pc[2] + cy
            ok &= (0.0 <= u) & (u <= float(W - 1)) & (0.0 <= w) & (w <= float(H - 1))
            D['inside'][view] = ok
            q = [(eye[a] - o[a]) / scale - p[a] for a in range(3)]
            L = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
            ok &= ~(L == 0.0)
            d = [q[a] / L for a in range(3)]
            c = ((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]) / norm
            D['cos'][view] = c
            ok &= c > cos_min
            # the occlusion march of the candidates, towards the eye
            cand = ok.copy()
            march = ok.copy()
            for k in range(nmax):
                j = np.flatnonzero(march)
                if not len(j):
                    break
                sk = bias + float(k) * step
                go = sk < L[j]
                march[j[~go]] = False
                j = j[go]
                s = [p[a][j] + sk * d[a][j] for a in range(3)]
                box = (0.0 <= s[0]) & (s[0] <= top) & (0.0 <= s[1]) & (s[1] <= top) & (0.0 <= s[2]) & (s[2] <= top)
                march[j[~box]] = False
                j, s = j[box], [c_[box] for c_ in s]
                below = trilinear(v64, *s) - iso64 < 0.0
                march[j[below]] = False
                ok[j[below]] = False
            D['occluded'][view] = cand & ~ok
            D['used'][view] = ok
            j = np.flatnonzero(ok)
            for ch in range(3):
                acc[ch, j] = acc[ch, j] + c[j] * bilinear(images[view, ch], u[j], w[j])
            wsum[j] = wsum[j] + c[j]
            mask[j] |= np.uint32(1 << view)
        some = wsum > 0.0
        colors = np.where(some[None], acc / np.where(some, wsum, 1.0)[None], fill64[:, None]).T.astype(f32)
    if details is not None:
        details.update(D, p=np.stack(p, 1), g=np.stack(g, 1))
    return np.ascontiguousarray(colors), wsum.astype(f32), mask.view(np.int32).copy()


def color_points(vol, points, count, images, poses, Ks, origin, scale, point_offset=(0.0, 0.0, 0.0), out=None, **kw):
    """Points mode, one scene: rows r < min(count, max_n) of points [max_n,3] float64 at world point_offset + points[r]; the other rows
    of `out` = (colors [max_n,3], weight [max_n], views [max_n]) are left untouched (zeros without `out`)."""
    points = np.asarray(points, f64)
    n = max(0, min(int(count), len(points)))
    off = np.asarray(point_offset, f64)
    x = np.stack([off[a] + points[:n, a] for a in range(3)], 1)
    got = color_world(vol, x, images, poses, Ks, origin, scale, **kw)
    out = (np.zeros((len(points), 3), f32), np.zeros(len(points), f32), np.zeros(len(points), np.int32)) if out is None else out
    for dst, src in zip(out, got):
        dst[:n] = src
    return out


def color_pixels(vol, depth, cam_poses, cam_Ks, images, poses, Ks, origin, scale, fill=(0.0, 0.0, 0.0), **kw):
    """Pixels mode, one scene: depth [Vc,h,w] float32 of the ray cast from cam_poses [Vc,3,4] / cam_Ks [Vc,3,3]; s <= 0 gives fill, weight
    0, views 0, otherwise the point eye' + s * dw' of the target camera's ray through the pixel.
    -> colors [Vc,h,w,3] float32, weight [Vc,h,w] float32, views [Vc,h,w] int32."""
    depth = np.asarray(depth, f32)
    Vc, h, w = depth.shape
    colors = np.empty((Vc, h, w, 3), f32)
    colors[:] = np.asarray(fill, f32)
    weight, views = np.zeros((Vc, h, w), f32), np.zeros((Vc, h, w), np.int32)
    vs, us = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing='ij')
    for c in range(Vc):
        Rm, t, eye, fx, fy, cx, cy = camera(cam_poses[c], cam_Ks[c])
        s = depth[c].astype(f64)
        hit = ~(s <= 0.0)
        dcx, dcy = (us[hit] - cx) / fx, (vs[hit] - cy) / fy
        x = np.stack([eye[a] + s[hit] * ((Rm[0, a] * dcx + Rm[1, a] * dcy) + Rm[2, a]) for a in range(3)], 1)
        colors[c][hit], weight[c][hit], views[c][hit] = color_world(vol, x, images, poses, Ks, origin, scale, fill=fill, **kw)
    return colors, weight, views
