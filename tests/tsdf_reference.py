"""Float64 statement (plain numpy) of the depth route's TSDF fusion -- TEST INFRASTRUCTURE ONLY, the arbiter of csrc/gnr_tsdf.hip --
and an analytic ray-caster for its test depth images.

The statement is Open3D's UniformTSDFVolume::Integrate + extract_voxel_point_cloud as src/gd/perception.py:66-128 drives them
(no colour), spelled out in include/gnr.h.  It follows the kernel's operation order exactly: every line below is ONE correctly
rounded IEEE operation per array element (numpy never contracts a multiply and an add), float64 up to t = min(1, sdf / trunc),
which is rounded once to float32; the running average and the grid are float32.  The kernel's results are therefore these bits.
Besides the state it returns, per voxel, the smallest distance of any decision it took to its flip (`margin`): a scene whose
margins are far above the rounding of a float64 operation is one on which the comparison cannot hinge on a rounding."""
import functools

import numpy as np

from graspnerf_amd.synth import CONFIGS, ring_cameras

f32 = np.float32


def integrate(tsdf, weight, depth, poses, Ks, origin, voxel_size, sdf_trunc, depth_scale=1.0, depth_trunc=2.0, margin=None):
    """One scene.  tsdf, weight [R,R,R] float32 (not modified); depth [V,h,w] float32 or uint16; poses [V,3,4], Ks [V,3,3], origin [3]
    float32 (they convert to float64 exactly); the four scalars are float64.
    -> (tsdf, weight, margin): the state after the V views in order and the running minimum of the decision margins [R,R,R] float64."""
    tv, wv = np.array(tsdf, f32), np.array(weight, f32)
    R = tv.shape[0]
    assert tv.shape == wv.shape == (R, R, R) and depth.dtype in (np.float32, np.uint16)
    V, h, w = depth.shape
    o = np.asarray(origin, f32).astype(np.float64)
    voxel_size, sdf_trunc, depth_scale, depth_trunc = float(voxel_size), float(sdf_trunc), float(depth_scale), float(depth_trunc)
    idx = np.arange(R, dtype=np.float64) + 0.5
    px = (o[0] + idx * voxel_size)[:, None, None]                                   # step 1
    py = (o[1] + idx * voxel_size)[None, :, None]
    pz = (o[2] + idx * voxel_size)[None, None, :]
    wmax, hmax = float(w) - 1e-4, float(h) - 1e-4
    mg = np.full((R, R, R), np.inf) if margin is None else np.array(margin, np.float64)
    for view in range(V):
        P = np.asarray(poses[view], f32).astype(np.float64)
        K = np.asarray(Ks[view], f32).astype(np.float64)
        with np.errstate(all='ignore'):
            cz = ((P[2, 0] * px + P[2, 1] * py) + P[2, 2] * pz) + P[2, 3]           # step 2
            front = ~(cz <= 0.0)
            cx = ((P[0, 0] * px + P[0, 1] * py) + P[0, 2] * pz) + P[0, 3]
            cy = ((P[1, 0] * px + P[1, 1] * py) + P[1, 2] * pz) + P[1, 3]
            fx, fy, ppx, ppy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
            uf = ((cx * fx) / cz + ppx) + 0.5                                       # step 3
            vf = ((cy * fy) / cz + ppy) + 0.5
            inside = front & (uf >= 1e-4) & (uf < wmax) & (vf >= 1e-4) & (vf < hmax)
            u = np.where(inside, np.trunc(uf), 0.0).astype(np.int64)
            v = np.where(inside, np.trunc(vf), 0.0).astype(np.int64)
            d_raw = depth[view][v, u].astype(np.float64) / depth_scale              # step 4
            d = np.where(d_raw >= depth_trunc, 0.0, d_raw)
            seen = inside & ~(d <= 0.0)
            a, c = (u.astype(np.float64) - ppx) / fx, (v.astype(np.float64) - ppy) / fy
            m = np.sqrt((a * a + c * c) + 1.0)                                      # step 5
            sdf = (d - cz) * m
            upd = seen & (sdf > -sdf_trunc)
            tn = np.minimum(1.0, sdf / sdf_trunc).astype(f32)                       # step 6: rounded once
            new = (tv * wv + tn) / (wv + f32(1.0))
            assert new.dtype == np.float32
            tv = np.where(upd, new, tv)
            wv = np.where(upd, wv + f32(1.0), wv)
            mg = np.minimum(mg, np.abs(cz))
            bounds = np.minimum(np.minimum(np.abs(uf - 1e-4), np.abs(uf - wmax)), np.minimum(np.abs(vf - 1e-4), np.abs(vf - hmax)))
            mg = np.where(front, np.minimum(mg, bounds), mg)
            pixel = np.minimum(np.minimum(np.abs(uf - np.rint(uf)), np.abs(vf - np.rint(vf))), np.abs(d_raw - depth_trunc))
            mg = np.where(inside, np.minimum(mg, pixel), mg)
            mg = np.where(seen, np.minimum(mg, np.abs(sdf + sdf_trunc)), mg)
    return tv, wv, mg


def grid(tsdf, weight):
    """get_grid: (tsdf + 1) * 0.5 where weight != 0 and -0.98 <= tsdf < 0.98, else 0 (float32)."""
    keep = (weight != f32(0.0)) & (tsdf < f32(0.98)) & (tsdf >= f32(-0.98))
    return np.where(keep, (tsdf + f32(1.0)) * f32(0.5), f32(0.0)).astype(f32)


def sdf_label(g):
    """get_sdf (dataset/database.py:207-209): grid * 2 - 1 (float32); unobserved or saturated voxels become -1."""
    return (g * f32(2.0) - f32(1.0)).astype(f32)


def fuse(sc, **kw):
    """A scene of make_scene (or one with the same keys) from zeros -> dict(tsdf, weight, margin, grid, sdf_label)."""
    R = sc['R']
    z = np.zeros((R, R, R), f32)
    tv, wv, mg = integrate(z, z, sc['depth'], sc['poses'], sc['Ks'], sc['origin'], sc['voxel_size'], sc['sdf_trunc'],
                           sc.get('depth_scale', 1.0), sc.get('depth_trunc', 2.0), **kw)
    g = grid(tv, wv)
    return {'tsdf': tv, 'weight': wv, 'margin': mg, 'grid': g, 'sdf_label': sdf_label(g)}


# ---- the analytic test scene: a table plane and two spheres ------------------------------------------------------------------------
PLANE_Z = 0.06
SPHERES = (((0.03, -0.02, 0.10), 0.04), ((-0.06, 0.05, 0.09), 0.03))
SPHERES_MOVED = (((-0.02, 0.04, 0.11), 0.04), ((0.07, -0.05, 0.09), 0.03))
ORIGIN, SIZE = (-0.15, -0.15, -0.05), 0.3


def render_depth(poses, K, h, w, spheres=SPHERES, plane_z=PLANE_Z, hole=True):
    """Camera-z depth [V,h,w] float32 of the plane z = plane_z and the spheres seen through the integer pixel centres of pinhole
    cameras (poses [V,3,4] world->camera, OpenCV axes): the nearest hit wins, a ray that hits nothing reads 0.
    hole: view 0 reads 0 in rows h//3:h//2, columns w//4:w//2 (missing depth)."""
    K = np.asarray(K, np.float64)
    vs, us = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    dc = np.stack([(us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1], np.ones_like(us)], -1)      # camera-frame ray, z = 1: s is depth
    out = np.zeros((len(poses), h, w), f32)
    for i, pose in enumerate(np.asarray(poses, np.float64)):
        Rm, t = pose[:, :3], pose[:, 3]
        eye = -Rm.T @ t
        dw = dc @ Rm                                                                              # Rm^T dc per pixel
        with np.errstate(all='ignore'):
            s = (plane_z - eye[2]) / dw[..., 2]
            best = np.where(s > 0, s, np.inf)
            for centre, radius in spheres:
                oc = eye - np.asarray(centre, np.float64)
                qa, qb, qc = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - radius * radius
                disc = qb * qb - 4.0 * qa * qc
                s = (-qb - np.sqrt(disc)) / (2.0 * qa)
                best = np.minimum(best, np.where((disc >= 0) & (s > 0), s, np.inf))
        out[i] = np.where(np.isfinite(best), best, 0.0).astype(f32)
    if hole:
        out[0, h // 3:h // 2, w // 4:w // 2] = 0.0
    return out


def make_scene(V, h, w, K, R, trunc_voxels, spheres=SPHERES, origin=ORIGIN, size=SIZE):
    """-> dict: depth [V,h,w], poses [V,3,4], Ks [V,3,3], origin [3] (float32), R, size, voxel_size, sdf_trunc (float64)."""
    poses = ring_cameras(V)
    K = np.asarray(K, f32).reshape(-1, 3)
    K = np.concatenate([K, np.asarray([[0, 0, 1]], f32)], 0) if K.shape[0] == 2 else K
    voxel = size / R
    return {'depth': render_depth(poses, K, h, w, spheres), 'poses': poses, 'Ks': np.repeat(K[None], V, 0).copy(),
            'origin': np.asarray(origin, f32), 'R': R, 'size': size, 'voxel_size': voxel, 'sdf_trunc': trunc_voxels * voxel}


SCENES = {'tiny': dict(V=2, h=24, w=32, K=[[25, 0, 15.5], [0, 25, 11.5]], R=8, trunc_voxels=2),
          'small': dict(V=3, h=96, w=128, K=CONFIGS['cfg1']['K'], R=16, trunc_voxels=4),
          'eight': dict(V=8, h=48, w=64, K=[[50, 0, 31.3], [0, 50, 23.7]], R=12, trunc_voxels=3)}


@functools.lru_cache(maxsize=None)
def scene(name, R=None, V=None, moved=False):
    """A named scene, optionally at another resolution / view count or with the spheres moved: made once, shared, never written to."""
    kw = dict(SCENES[name])
    if R is not None:
        kw['R'] = R
    if V is not None:
        kw['V'] = V
    return make_scene(spheres=SPHERES_MOVED if moved else SPHERES, **kw)


@functools.lru_cache(maxsize=None)
def statement(name, R=None, V=None, moved=False):
    """fuse() of scene(...): computed once, shared, never written to."""
    return fuse(scene(name, R, V, moved))
