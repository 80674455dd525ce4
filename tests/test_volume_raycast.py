"""Depth and gradient images of a scalar volume from any camera (csrc/gnr_raycast.hip, raycast.VolumeRaycaster, TSDFVolume.render_depth,
plan_real(volume_depth=True), Validator(volume_depth=True)).  tests/raycast_reference.py is the statement in numpy float64; the device's
images are compared with it by np.array_equal on the bits.  Without a GPU: the statement against analytic geometry (a sphere, the
round trip depth -> fused grid -> depth, exact cases), the refusals made before the device is touched, and the keyword checks."""
import ctypes as C
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib
from graspnerf_amd.raycast import VolumeRaycaster
from graspnerf_amd.synth import CONFIGS, ring_cameras
import mesh_reference as mref
import raycast_reference as ref
import tsdf_reference as tref
from test_surface_mesh import TORUS, same

f32, f64 = np.float32, np.float64
K_CFG1 = np.asarray(CONFIGS['cfg1']['K'], f32).reshape(3, 3)
H1, W1 = 96, 128


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """World->camera [3,4] float32 (OpenCV axes: z forward) of a camera at `eye` that looks at `target`."""
    eye, f = np.asarray(eye, f64), np.asarray(target, f64) - np.asarray(eye, f64)
    f = f / np.linalg.norm(f)
    x = np.cross(np.asarray(up, f64), f)
    x = x / np.linalg.norm(x)
    Rm = np.stack([x, np.cross(f, x), f])
    return np.concatenate([Rm, (-Rm @ eye)[:, None]], 1).astype(f32)


def straight_down(eye):
    """The axis-aligned camera R = diag(1,-1,-1) above `eye`: every ray has d_x = 0 or d_y = 0 on the principal column / row."""
    Rm = np.diag([1.0, -1.0, -1.0])
    return np.concatenate([Rm, (-Rm @ np.asarray(eye, f64))[:, None]], 1).astype(f32)


def path_scale(K, h, w):
    """|dc| per pixel: a depth difference times this is a distance along the ray."""
    K = np.asarray(K, f64)
    vs, us = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing='ij')
    return np.sqrt(((us - K[0, 2]) / K[0, 0]) ** 2 + ((vs - K[1, 2]) / K[1, 1]) ** 2 + 1.0)


# ---- 1. the statement against an analytic sphere (no GPU) ----------------------------------------------------------------------
# measured with this statement, view 0 (step 0.5, 4 bisections), in voxels along the ray; the bounds are 1.5 x these, rounded up
#   R = 16 (radius 2.1 voxels): max 0.4738, mean 0.1395 over 208 pixels;   R = 40: max 0.2388, mean 0.05617 over 222 pixels
SPHERE_BOUNDS = {16: (0.72, 0.21), 40: (0.36, 0.085)}


@pytest.mark.parametrize('R', [16, 40])
def test_statement_on_an_analytic_sphere(R):
    voxel = tref.SIZE / R
    c = (np.arange(R, dtype=f64) + 0.5) * voxel
    centre, radius = tref.SPHERES[0]
    X, Y, Z = np.meshgrid(c + tref.ORIGIN[0], c + tref.ORIGIN[1], c + tref.ORIGIN[2], indexing='ij')
    sdf = (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius).astype(f32)      # exact metric SDF at the centres
    poses = ring_cameras(3)[:, :3, :]
    got = ref.raycast(sdf, poses, np.repeat(K_CFG1[None], 3, 0), H1, W1, origin=np.asarray(tref.ORIGIN, f64) + 0.5 * voxel, scale=voxel)
    want = tref.render_depth(poses, K_CFG1, H1, W1, spheres=(tref.SPHERES[0],), plane_z=-10, hole=False)
    sphere = (want > 0) & (want < 5.0)                                            # (the plane at z = -10 lies 10 m behind everything)
    assert got.dtype == f32 and got.shape == (3, H1, W1)
    m = path_scale(K_CFG1, H1, W1)
    for v in range(3):
        both = (got[v] > 0) & sphere[v]
        err = np.abs(got[v].astype(f64) - want[v]) * m / voxel
        s = sphere[v]
        rim = s & ~(np.roll(s, 1, 0) & np.roll(s, -1, 0) & np.roll(s, 1, 1) & np.roll(s, -1, 1))      # the silhouette's own pixels
        print(f'R = {R}, view {v}: {(got[v] > 0).sum()} and {s.sum()} pixels hit ({rim.sum()} on the silhouette), '
              f'max {err[both].max():.4f} mean {err[both].mean():.4f} voxel over {both.sum()} pixels')
        assert abs(int((got[v] > 0).sum()) - int(s.sum())) <= rim.sum() and both.sum() >= 150
        assert not (got[v] > 0)[~s & ~rim & ~np.roll(rim, 1, 0) & ~np.roll(rim, -1, 0) & ~np.roll(rim, 1, 1) & ~np.roll(rim, -1, 1)].any()
    both = (got[0] > 0) & sphere[0]
    err = (np.abs(got[0].astype(f64) - want[0]) * m / voxel)[both]
    assert both.sum() == {16: 208, 40: 222}[R]
    assert err.max() <= SPHERE_BOUNDS[R][0] and err.mean() <= SPHERE_BOUNDS[R][1]


# ---- 2. the round trip depth -> fused grid -> depth (no GPU) ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused40():
    """tsdf_reference.scene('small', R=40) fused by the TSDF statement, as the volume the ray cast reads (unobserved: 1, outside), its
    lattice and the statement's images of it from the scene's own three cameras: computed once, shared, never written to."""
    sc, st = tref.scene('small', R=40), tref.statement('small', R=40)
    vol = np.where(st['weight'] > 0, st['tsdf'], f32(1.0)).astype(f32)
    voxel = sc['voxel_size']
    frame = dict(origin=sc['origin'].astype(f64) + 0.5 * voxel, scale=voxel)
    details = {}
    depth = ref.raycast(vol, sc['poses'][:, :3, :], sc['Ks'], H1, W1, details=details, **frame)
    return sc, vol, frame, depth, details


def test_round_trip_through_the_fused_grid():
    """View 1, measured with this statement: median 0.0802, 90th percentile 0.2824 voxel over 2 025 pixels (the maximum, 14 voxels, sits on
    the silhouette where one image sees the sphere and the other the table: not asserted).  The bounds are 1.5 x, rounded up.
    Of the pixels with a depth whose ray crosses the box only 34.2 % are hit -- the table is an infinite plane and most of those rays
    leave the box through a side before they reach it -- so the 95 % condition does not hold as worded; it is lowered to the statement's
    figure minus two points (32 %), and 95 % is asked of the pixels whose own surface point lies inside the lattice (measured: 99.7 %)."""
    sc, vol, frame, depth, details = fused40()
    v = 1
    true = sc['depth'][v]
    both = (depth[v] > 0) & (true > 0)
    err = (np.abs(depth[v].astype(f64) - true) * path_scale(sc['Ks'][v], H1, W1) / frame['scale'])[both]
    med, p90 = float(np.median(err)), float(np.percentile(err, 90))
    crossing = (true > 0) & details['crosses'][v]
    frac = float((depth[v] > 0)[crossing].mean())
    P = sc['poses'][v].astype(f64)
    K = sc['Ks'][v].astype(f64)
    vs, us = np.meshgrid(np.arange(H1, dtype=f64), np.arange(W1, dtype=f64), indexing='ij')
    dw = np.stack([(us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1], np.ones_like(us)], -1) @ P[:, :3]
    pt = ((-P[:, :3].T @ P[:, 3]) + true.astype(f64)[..., None] * dw - frame['origin']) / frame['scale']
    inside = (true > 0) & ((pt >= 0) & (pt <= 39)).all(-1)
    frac_inside = float((depth[v] > 0)[inside].mean())
    print(f'round trip, view {v}: median {med:.4f}, 90th percentile {p90:.4f}, max {err.max():.1f} voxel over {both.sum()} pixels; '
          f'{100 * frac:.1f} % of {crossing.sum()} crossing pixels hit, {100 * frac_inside:.1f} % of {inside.sum()} with the surface in the lattice')
    assert both.sum() >= 2000
    assert med <= 0.13 and p90 <= 0.43
    assert frac >= 0.32 and frac_inside >= 0.95


# ---- 3. exact cases (no GPU) -------------------------------------------------------------------------------------------------------
def _plane(R=8, level=3.25):
    return (np.indices((R, R, R))[2] - level).astype(f32)


DOWN = dict(pose=straight_down((0.03, 0.04, 0.5)), K=np.array([[100, 0, 4], [0, 100, 3], [0, 0, 1]], f32), hw=(7, 9), scale=0.01)


def _down(vol, **kw):
    d = {}
    out = ref.raycast(vol, DOWN['pose'][None], DOWN['K'][None], *DOWN['hw'], origin=(0.0, 0.0, 0.0), scale=DOWN['scale'], details=d, **kw)
    return out, d


def test_exact_cases():
    # a plane seen straight down: trilinear is exact on a linear field; the centre pixel's ray has d_x = d_y = 0
    depth, d = _down(_plane())
    want = 0.5 - 3.25 * 0.01
    assert d['crosses'].all() and (depth > 0).all()
    assert np.abs(d['s'] / want - 1.0).max() <= 1e-12 and same(depth, np.full_like(depth, f32(want)))
    assert d['s'][0, 3, 4] != 0 and DOWN['K'][0, 2] == 4 and DOWN['K'][1, 2] == 3
    # bisections = 0: the secant step alone is exact on a linear field
    depth0, d0 = _down(_plane(), bisections=0)
    assert np.abs(d0['s'] / want - 1.0).max() <= 1e-12
    # with a gradient volume: the interpolated rows, rounded once
    g = np.zeros((8, 8, 8, 3), f32)
    g[..., 0], g[..., 2] = np.indices((8, 8, 8))[0], 1.0
    dg, gg = ref.raycast(_plane(), DOWN['pose'][None], DOWN['K'][None], *DOWN['hw'], origin=(0.0, 0.0, 0.0), scale=0.01, gradient=g)
    assert same(dg, depth) and gg.dtype == f32 and np.array_equal(gg[..., 2], np.ones_like(gg[..., 2])) and np.array_equal(gg[..., 1], 0 * gg[..., 1])
    assert abs(gg[0, 3, 4, 0] - 3.0) <= 1e-6                                     # the eye sits above lattice x = 3
    # R = 2: one cell, the surface at z = 0.25
    v2 = (np.indices((2, 2, 2))[2] - 0.25).astype(f32)
    K2 = np.array([[1000, 0, 4], [0, 1000, 3], [0, 0, 1]], f32)
    d = {}
    depth2 = ref.raycast(v2, straight_down((0.005, 0.005, 0.5))[None], K2[None], 7, 9, origin=(0.0, 0.0, 0.0), scale=0.01, details=d)
    assert (depth2 > 0).all() and np.abs(d['s'] / (0.5 - 0.0025) - 1.0).max() <= 1e-12
    # a ray that starts inside (the camera below the plane's level, looking down): inside all the way, no hit
    inside_pose = straight_down((0.03, 0.04, 0.02))
    dep = ref.raycast(_plane(), inside_pose[None], DOWN['K'][None], 7, 9, origin=(0.0, 0.0, 0.0), scale=0.01)
    assert not dep.any()
    # ... and one that starts inside, leaves and enters again: the hit is the second surface, not the start
    slab = np.abs(np.indices((8, 8, 8))[2] - 5.0).astype(f32) - 1.0                # inside for 4 < z < 6
    two = np.minimum(slab, np.abs(np.indices((8, 8, 8))[2] - 1.5).astype(f32) - 1.0)      # and for 0.5 < z < 2.5
    d = {}
    dep = ref.raycast(two, straight_down((0.03, 0.04, 0.055))[None], DOWN['K'][None], 7, 9, origin=(0.0, 0.0, 0.0), scale=0.01, details=d)
    assert (dep > 0).all() and np.abs(d['s'] / (float(f32(0.055)) - 0.025) - 1.0).max() <= 1e-12       # (the pose is float32)
    # iso equal to a corner value: that corner is outside (vol < iso is false), as in the mesh
    lv = np.indices((8, 8, 8))[2].astype(f32)                                    # values 0..7 along z; iso = 3 is the value of the lattice plane z = 3
    depi, d = _down(lv, iso=3.0, step=1.0, bisections=0)
    assert (depi > 0).all() and np.abs(d['s'] / (0.5 - 0.03) - 1.0).max() <= 1e-12
    assert not _down(np.full((8, 8, 8), 3.0, f32), iso=3.0)[0].any()             # every value equal to iso: all outside
    # near / far that cut the surface off
    assert not _down(_plane(), far=0.46)[0].any() and not _down(_plane(), near=0.47)[0].any()
    cut, d = _down(_plane(), near=0.44, far=0.48)                                # between them: other samples, the same surface
    assert (cut > 0).all() and np.abs(d['s'] / want - 1.0).max() <= 1e-12
    # all outside and all inside
    assert not _down(np.ones((8, 8, 8), f32))[0].any() and not _down(-np.ones((8, 8, 8), f32))[0].any()
    # a camera that looks away from the box
    away = look_at((0.03, 0.04, 0.5), (0.03, 0.04, 1.0), up=(0, 1, 0))
    d = {}
    assert not ref.raycast(_plane(), away[None], DOWN['K'][None], 7, 9, origin=(0.0, 0.0, 0.0), scale=0.01, details=d).any() and not d['crosses'].any()
    assert ref.max_samples(40, 0.5) == math.ceil(math.sqrt(3.0) * 39 / 0.5) + 1


# ---- 4. the C ABI's refusals, before the device (no GPU) ---------------------------------------------------------------------------
def _params(**kw):
    p = _lib.GnrRaycastParams(B=1, V=1, h=8, w=8, R=8, bisections=4, iso=0.0, scale=1.0, step=0.5, near_s=0.0, far_s=float('inf'))
    for k, v in kw.items():
        if k == 'origin':
            p.origin[:] = v
        else:
            setattr(p, k, v)
    return p


def test_refusals_before_the_device():
    """Fake pointers: every call is one that validation refuses, each with its code and a text that names the limit."""
    L = _lib.lib()
    one = C.c_void_p(16)

    def call(p=None, vol=one, grad=None, poses=one, Ks=one, depth=one, gradient=None, **kw):
        p = _params(**kw) if p is None else p
        return L.gnr_volume_raycast_fwd(C.byref(p) if p is not False else None, vol, grad, poses, Ks, depth, gradient, None)

    text = lambda: L.gnr_last_error().decode()
    for name in ('vol', 'poses', 'Ks', 'depth'):
        assert call(**{name: None}) == _lib.GNR_ERR_ARG, name
        assert text() == 'gnr_volume_raycast_fwd: null pointer', name
    assert call(p=False) == _lib.GNR_ERR_ARG and text() == 'gnr_volume_raycast_fwd: null pointer'
    for kw in (dict(grad=one), dict(gradient=one)):
        assert call(**kw) == _lib.GNR_ERR_ARG and 'both given or both NULL' in text(), kw
    for B in (0, -1, 65536):
        assert call(B=B) == _lib.GNR_ERR_SHAPE and 'B must be in 1..65535' in text(), B
    for V in (0, -3):
        assert call(V=V) == _lib.GNR_ERR_SHAPE and 'V must be >= 1' in text(), V
    for kw in (dict(h=0), dict(w=0), dict(h=-1)):
        assert call(**kw) == _lib.GNR_ERR_SHAPE and 'h and w must be >= 1' in text(), kw
    for R in (1, 0, 257):
        assert call(R=R) == _lib.GNR_ERR_SHAPE and 'R must be in 2..256' in text(), R
    for n in (-1, 33):
        assert call(bisections=n) == _lib.GNR_ERR_ARG and 'bisections must be in 0..32' in text(), n
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf')), dict(step=0.0), dict(step=-0.5),
               dict(step=float('nan')), dict(step=float('inf'))):
        assert call(**kw) == _lib.GNR_ERR_ARG and 'scale and step must be finite and > 0' in text(), kw
    for kw in (dict(iso=float('nan')), dict(iso=float('inf')), dict(origin=[0.0, float('nan'), 0.0]), dict(origin=[float('-inf'), 0.0, 0.0]),
               dict(origin=[0.0, 0.0, float('nan')])):
        assert call(**kw) == _lib.GNR_ERR_ARG and 'iso and origin must be finite' in text(), kw
    for kw in (dict(near_s=-1e-9), dict(near_s=float('nan')), dict(near_s=1.0, far_s=1.0), dict(near_s=1.0, far_s=0.5), dict(far_s=float('nan'))):
        assert call(**kw) == _lib.GNR_ERR_ARG and 'near_s must be >= 0 and far_s > near_s' in text(), kw
    # the march's loop bound: ceil(sqrt(3) (R-1) / step) + 1 samples at most
    assert call(R=256, step=1e-3) == _lib.GNR_ERR_ARG and 'GNR_RAYCAST_MAX_SAMPLES' in text() and str(_lib.GNR_RAYCAST_MAX_SAMPLES) in text()
    assert ref.max_samples(256, 1e-2) <= _lib.GNR_RAYCAST_MAX_SAMPLES < ref.max_samples(256, 1e-3)
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1) == _lib.GNR_ERR_SHAPE and '2^28 tiles' in text()


def test_raycaster_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        VolumeRaycaster()


# ---- 5. keyword checks (no GPU) ------------------------------------------------------------------------------------------------------
def test_keyword_checks(monkeypatch):
    from graspnerf_amd import planner, trainer as trainer_mod, validation
    from graspnerf_amd.planner_session import PlannerSession
    from test_validation import StubNet, stub_losses, stub_scene
    with pytest.raises(TypeError, match='unknown volume_depth parameters'):
        planner.plan_real(None, [np.zeros((8, 8, 3), np.uint8)] * 4, [np.eye(4)] * 4, np.eye(3), volume_depth={'bogus': 1})
    with pytest.raises(TypeError, match='unknown volume_depth parameters'):
        planner.real_session(None, 4, (8, 8), (32, 32), volume_depth={'bogus': 1})
    assert planner._depth_params(False) is None and planner._depth_params(None) is None
    assert planner._depth_params(True) == dict(extrinsics=None, intrinsic=None, hw=None, iso=0.0, step=0.5, bisections=4)
    p = planner._depth_params(dict(extrinsics=[np.eye(4)] * 2, intrinsic=np.eye(3), hw=[5, 7], iso=0.25))
    assert p['extrinsics'].shape == (2, 3, 4) and p['extrinsics'].dtype == f32 and p['hw'] == (5, 7) and p['iso'] == 0.25
    assert planner.same_params(p, dict(p, origin=(0, 0, 0))) and not planner.same_params(p, planner._depth_params(True))
    assert not planner.same_params(p, None) and planner.same_params(None, None)
    assert inspect.signature(PlannerSession.__init__).parameters['volume_depth'].default is None
    # Validator(volume_depth=False): the keys of today
    monkeypatch.setattr(trainer_mod, 'train_losses', stub_losses)
    scenes = [stub_scene(0)]
    today = validation.Validator()(StubNet(), scenes)
    off = validation.Validator(volume_depth=False)(StubNet(), scenes)
    assert set(off[0]) == {'loss_vgn', 'other', 'psnr_nr', 'psnr_nr_fine', 'ssim_nr', 'ssim_nr_fine', 'depth_mae'}
    assert off == today
    with pytest.raises(KeyError, match='volume_depth=True needs'):
        validation.Validator(volume_depth=True)(StubNet(), [dict(scenes[0], ref_imgs_info={})])


# ---- GPU: the bits of the statement ------------------------------------------------------------------------------------------------
FRAME = dict(origin=(0.125, -0.3, 0.0517), scale=0.3 / 40)


def _world(idx):
    return np.asarray(FRAME['origin'], f64) + np.asarray(idx, f64) * FRAME['scale']


def _scenes(R):
    """Two scenes of three views each at resolution R: a sphere seen from outside, straight down (the axis-aligned camera) and from
    inside the object;  a torus (R = 16) or a plane that leaves the grid, from outside, from a camera that looks away (its box is
    entirely off-image) and from a third side.  Different intrinsics per view."""
    mid = (R - 1) / 2.0
    vols = np.stack([mref.sphere(R, (mid + 0.3, mid - 0.4, mid + 0.05), 0.3 * R),
                     mref.torus(*TORUS) if R == 16 else mref.plane(R, offset=0.8 * R)])
    c = _world((mid, mid, mid))
    far = 2.0 * R * FRAME['scale']
    x0, y0 = _world((mid, mid, 0))[:2]
    poses = np.stack([np.stack([look_at(c + far * np.array([0.6, -0.5, 0.62]), c), straight_down((x0, y0, c[2] + far)),
                                look_at(_world((mid + 0.3, mid - 0.4, mid + 0.05)), c + np.array([0.3, 0.2, 0.1]))]),
                      np.stack([look_at(c + far * np.array([-0.4, 0.7, 0.59]), c), look_at(c + far * np.array([0.0, 0.0, 1.0]), c + far * np.array([0.3, 0.1, 2.0])),
                                look_at(c + far * np.array([0.1, -0.2, -0.97]), c, up=(0, 1, 0))])])
    Ks = lambda h, w: np.stack([np.stack([np.array([[f * w, 0, cx], [0, f * w, cy], [0, 0, 1]], f32)
                                          for f, cx, cy in ((0.9, 0.5 * w - 0.5, 0.5 * h - 0.5), (1.1, float(w // 2), float(h // 2)), (0.6, 0.47 * w, 0.52 * h))])] * 2)
    return vols.astype(f32), poses.astype(f32), Ks


def _raw(vol, grad, poses, Ks, h, w, sentinel=0x5a, **kw):
    """The C call on buffers filled with a sentinel byte, with one more image row behind [B,V,h,w] that the call is not told about
    -> (depth [B,V,h,w], gradient or None, the rows behind them)."""
    L = _lib.lib()
    B, R, V = vol.shape[0], vol.shape[-1], poses.shape[1]
    d = torch.device('cuda:0')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    v, P, K = up(vol), up(poses), up(Ks)
    g = None if grad is None else up(grad)
    n = B * V * h * w
    fill = lambda m: torch.full((m * 4,), sentinel, dtype=torch.uint8, device=d).view(torch.float32)
    depth = fill(n + w)
    gout = None if grad is None else fill(3 * (n + w))
    p = _params(B=B, V=V, h=h, w=w, R=R, bisections=kw.get('bisections', 4), iso=kw.get('iso', 0.0), scale=FRAME['scale'], step=kw.get('step', 0.5),
                origin=list(FRAME['origin']))
    rc = L.gnr_volume_raycast_fwd(C.byref(p), v.data_ptr(), None if g is None else g.data_ptr(), P.data_ptr(), K.data_ptr(), depth.data_ptr(),
                                  None if g is None else gout.data_ptr(), C.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    _lib.check(rc, 'gnr_volume_raycast_fwd')
    torch.cuda.synchronize()
    depth = depth.cpu().numpy()
    gout = None if gout is None else gout.cpu().numpy()
    tail = [depth[n:]] + ([] if gout is None else [gout[3 * n:]])
    return depth[:n].reshape(B, V, h, w), None if gout is None else gout[:3 * n].reshape(B, V, h, w, 3), tail


@pytest.mark.gpu
@pytest.mark.parametrize('hw', [(24, 32), (37, 53)])
@pytest.mark.parametrize('R', [6, 8, 16])
def test_smallest_shapes_equal_the_statement(R, hw):
    """37 x 53 is no multiple of the 8 x 8 tile: the padding lanes write nothing (the row behind the images keeps its sentinel)."""
    h, w = hw
    vol, poses, Ks = _scenes(R)
    Ks = Ks(h, w)
    grad = np.random.default_rng(R).standard_normal((2, R, R, R, 3)).astype(f32)
    hits = 0
    for kw in (dict(bisections=4, step=0.5, iso=0.0), dict(bisections=0, step=1.0, iso=0.3), dict(bisections=4, step=1.0, iso=0.0),
               dict(bisections=0, step=0.5, iso=0.3)):
        want = [ref.raycast(vol[b], poses[b], Ks[b], h, w, gradient=grad[b], **FRAME, **kw) for b in range(2)]
        for with_grad in (True, False):
            depth, gout, tail = _raw(vol, grad if with_grad else None, poses, Ks, h, w, **kw)
            for t in tail:
                assert (t.view(np.uint8) == 0x5a).all(), 'written beyond [B,V,h,w]'
            for b in range(2):
                assert same(depth[b], want[b][0]), (kw, with_grad, b, 'depth', int((depth[b] != want[b][0]).sum()))
                if with_grad:
                    assert same(gout[b], want[b][1]), (kw, with_grad, b, 'gradient')
        hits += sum(int((wb[0] > 0).sum()) for wb in want)
        assert (want[0][0][0] > 0).sum() > 20 and (want[0][0][1] > 0).sum() > 20     # the sphere from outside and straight down
        assert not want[1][0][1].any(), 'the camera that looks away sees something'
        assert (want[1][0][0] > 0).sum() > 20
    print(f'R = {R}, {h} x {w}: {hits} hits in all')
    # the raycaster: one scene's cameras for both, kept buffers
    rc = VolumeRaycaster()
    a = rc(vol, poses[0], Ks[0], hw, gradient=grad, **FRAME)
    ptr = a['depth'].data_ptr()
    got = a['depth'].cpu().numpy()
    for b in range(2):
        assert same(got[b], ref.raycast(vol[b], poses[0], Ks[0], h, w, **FRAME)), b
    assert rc(vol, poses[1], Ks[1], hw, gradient=grad, **FRAME)['depth'].data_ptr() == ptr
    assert 'gradient' not in rc(vol[0], poses[0], Ks[0], hw, **FRAME)


@pytest.mark.gpu
def test_fused_tsdf_direct_and_in_a_replayed_graph():
    """One 40^3 volume, V = 6, 96 x 128: the fused TSDF of the round trip from its own three cameras and three more."""
    sc, vol, frame, depth3, _ = fused40()
    c = np.asarray(tref.ORIGIN, f64) + 0.5 * tref.SIZE
    more = np.stack([look_at(c + np.array([0.35, 0.1, 0.3]), c), look_at(c + np.array([-0.2, -0.3, 0.35]), c), straight_down((c[0], c[1], 0.6))])
    poses = np.concatenate([sc['poses'][:, :3, :], more]).astype(f32)
    Ks = np.repeat(K_CFG1[None], 6, 0)
    want = np.concatenate([depth3, ref.raycast(vol, more, Ks[3:], H1, W1, **frame)])
    assert all((want[v] > 0).sum() > 1000 and (want[v] == 0).sum() > 1000 for v in range(6))
    rc = VolumeRaycaster()
    d = rc.device
    static = torch.from_numpy(vol.copy()).to(d)
    P, K = torch.from_numpy(poses).to(d), torch.from_numpy(Ks).to(d)
    out = rc(static, P, K, (H1, W1), **frame)['depth']
    out.view(torch.uint8).fill_(0x71)
    got = rc(static, P, K, (H1, W1), **frame)['depth']
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert same(got[0].cpu().numpy(), want), 'direct'                             # misses read 0, not the 0x71 fill
    s = torch.cuda.Stream(d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        rc(static, P, K, (H1, W1), **frame)
    torch.cuda.current_stream(d).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = rc(static, P, K, (H1, W1), **frame)['depth']
    assert cap.data_ptr() == out.data_ptr()
    for i in range(2):
        out.view(torch.uint8).fill_(0x71)
        g.replay()
        torch.cuda.synchronize()
        assert same(cap[0].cpu().numpy(), want), f'replay {i}'


@pytest.mark.gpu
def test_tsdf_volume_render_depth_equals_the_statement():
    from graspnerf_amd.tsdf import TSDFVolume
    sc, st = tref.scene('tiny'), tref.statement('tiny')
    vol = TSDFVolume(sc['size'], sc['R'], origin=sc['origin'], sdf_trunc=sc['sdf_trunc'])
    vol.integrate(sc['depth'], sc['Ks'], sc['poses'])
    assert same(vol.tsdf[0].cpu().numpy(), st['tsdf'])
    h, w = sc['depth'].shape[-2:]
    got = vol.render_depth(sc['Ks'], sc['poses'], (h, w))
    assert tuple(got.shape) == (1, 2, h, w) and got.is_cuda
    grid = np.where(st['weight'] > 0, st['tsdf'], f32(1.0)).astype(f32)
    voxel = sc['size'] / sc['R']
    want = ref.raycast(grid, sc['poses'][:, :3, :], sc['Ks'], h, w, origin=sc['origin'].astype(f64) + 0.5 * voxel, scale=voxel)
    assert (want > 0).sum() > 50
    assert same(got[0].cpu().numpy(), want)
    one = vol.render_depth(sc['Ks'][0], sc['poses'][:1], (h, w))                  # one intrinsic matrix, one camera
    assert same(one[0].cpu().numpy(), want[:1])
    # two scenes with an origin each: every scene's lattice is its own
    moved = (sc['origin'] + f32([0.01, -0.02, 0.005])).astype(f32)
    two = TSDFVolume(sc['size'], sc['R'], B=2, origin=np.stack([sc['origin'], moved]), sdf_trunc=sc['sdf_trunc'])
    two.integrate(np.stack([sc['depth']] * 2), sc['Ks'], sc['poses'])
    st2 = tref.fuse(dict(sc, origin=moved))
    grid2 = np.where(st2['weight'] > 0, st2['tsdf'], f32(1.0)).astype(f32)
    want2 = ref.raycast(grid2, sc['poses'][:, :3, :], sc['Ks'], h, w, origin=moved.astype(f64) + 0.5 * voxel, scale=voxel)
    got2 = two.render_depth(sc['Ks'], sc['poses'], (h, w)).cpu().numpy()
    assert same(got2[0], want) and same(got2[1], want2) and not same(want, want2)


@pytest.mark.gpu
def test_plan_real_with_the_volume_depth_eager_and_session():
    """The synthetic checkpoint's volume need not cross zero: the level of the compared images is the eager volume's own median, and
    volume_depth=True (iso = 0) is compared with the statement whatever it holds."""
    from graspnerf_amd import planner
    from test_planner_session import CFG, _state_dict
    from test_planner_session_real import V, HW, TOP_K, _frames
    net = planner.load_model(dict(CFG), {'network_state_dict': _state_dict(width_bias=5.0)})
    K = np.float32([[0.7 * HW[1], 0, 0.5 * HW[1]], [0, 0.7 * HW[1], 0.5 * HW[0]], [0, 0, 1]])
    ext = ring_cameras(V)
    cam = dict(extrinsics=list(ext), intrinsic=K)
    A, B = _frames(1), _frames(2)
    vol = planner.plan_real(net, A, **cam)[2]
    rg = (float(np.percentile(vol, 40)), float(np.percentile(vol, 60)))
    iso = float(f32(np.median(vol)))
    kw = dict(order='score', top_k=TOP_K, surface_rg=rg, normals=True)
    vd = dict(iso=iso)
    plain = planner.plan_real(net, A, **cam, **kw)
    assert 'volume_depth' not in plain[3]
    eager = planner.plan_real(net, A, **cam, **kw, volume_depth=vd)
    sess = planner.real_session(net, V, HW, HW[::-1], order='score', top_k=TOP_K, surface_rg=rg, normals=True, volume_depth=vd)
    got = planner.plan_real(net, A, **cam, **kw, volume_depth=vd, session=sess)
    other = planner.plan_real(net, B, **cam, **kw, volume_depth=vd, session=sess)
    again = planner.plan_real(net, A, **cam, **kw, volume_depth=vd, session=sess)
    assert sess.captures == 1
    frame = dict(origin=planner.real_volume_origin(), scale=planner.REAL_VOXEL_SIZE)
    poses, Ks = np.asarray(ext, f32)[:, :3, :], np.repeat(K[None], V, 0)
    for what, res in (('eager', eager), ('session', got), ('session, second replay', again)):
        for k in ('index', 'pos', 'quat', 'width', 'score'):
            assert same(res[0][k], plain[0][k]), (what, k)                         # grasps, scores and cloud do not depend on the switch
        assert same(res[1], plain[1]) and same(res[2], plain[2]), what
        for k in ('index', 'points', 'colors', 'gradient', 'normals'):
            assert same(res[3][k], plain[3][k]), (what, 'cloud', k)
        img = res[3]['volume_depth']
        want = ref.raycast(res[2], poses, Ks, *HW, iso=iso, **frame)
        print(what, [(int((want[v] > 0).sum())) for v in range(V)], 'pixels hit per view')
        assert img.dtype == f32 and img.shape == (V, *HW) and same(img, want), what
        assert (want > 0).sum() > 100, 'the cameras do not see the level set'
        nrm = res[3]['volume_depth_normals']
        assert nrm.shape == (V, *HW, 3) and same(nrm, eager[3]['volume_depth_normals']), what
        ln = np.linalg.norm(nrm, axis=-1)
        assert np.abs(ln[img > 0] - 1).max() <= 1e-12 and not ln[img == 0].any()
    assert same(other[3]['volume_depth'], ref.raycast(other[2], poses, Ks, *HW, iso=iso, **frame)) and not same(other[2], got[2])
    # volume_depth=True: iso = 0, the plan's cameras;  other cameras, another size and step through the dict
    assert same(planner.plan_real(net, A, **cam, **kw, volume_depth=True)[3]['volume_depth'], ref.raycast(plain[2], poses, Ks, *HW, **frame))
    c = np.asarray(planner.REAL_BBOX3D, f64).mean(0)
    K2 = K.copy()
    K2[:2] *= f32(0.5)
    mine = dict(extrinsics=[look_at(c + np.array([0.3, 0.2, 0.4]), c), straight_down((c[0], c[1], 0.7))], intrinsic=K2, hw=(37, 53), iso=iso,
                step=1.0, bisections=2)
    wm = ref.raycast(plain[2], np.stack(mine['extrinsics']), np.repeat(K2[None], 2, 0), 37, 53, iso=iso, step=1.0, bisections=2, **frame)
    em = planner.plan_real(net, A, **cam, order='score', top_k=TOP_K, surface_rg=rg, volume_depth=mine)
    assert same(em[3]['volume_depth'], wm) and 'volume_depth_normals' not in em[3] and (wm > 0).sum() > 100
    sm = planner.real_session(net, V, HW, HW[::-1], order='score', top_k=TOP_K, surface_rg=rg, volume_depth=mine)
    assert same(planner.plan_real(net, A, **cam, order='score', top_k=TOP_K, surface_rg=rg, volume_depth=mine, session=sm)[3]['volume_depth'], wm)
    # a session refuses a plan that asks for another volume_depth than its own
    with pytest.raises(ValueError, match='real_session'):
        planner.plan_real(net, A, **cam, **kw, session=sess, volume_depth=True)
    with pytest.raises(ValueError, match='real_session'):
        planner.plan_real(net, A, **cam, **kw, session=sess)


@pytest.mark.gpu
def test_validator_volume_depth_mae(monkeypatch):
    """A stub network on the device that returns a sphere's SDF as its volume, scored against the analytic depth of the same sphere from
    the scene's cameras: volume_depth_mae is the numpy expression over the statement's image; every other key keeps its bits."""
    from graspnerf_amd import trainer as trainer_mod, validation
    from test_validation import StubNet, stub_losses, stub_scene
    monkeypatch.setattr(trainer_mod, 'train_losses', stub_losses)
    R = 16
    voxel = tref.SIZE / R
    c = (np.arange(R, dtype=f64) + 0.5) * voxel
    centre, radius = tref.SPHERES[0]
    X, Y, Z = np.meshgrid(c + tref.ORIGIN[0], c + tref.ORIGIN[1], c + tref.ORIGIN[2], indexing='ij')
    sdf = (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius).astype(f32)
    poses = ring_cameras(3)[:, :3, :].astype(f32)
    Ks = np.repeat(K_CFG1[None], 3, 0)
    true = tref.render_depth(poses, K_CFG1, H1, W1, spheres=tref.SPHERES, plane_z=tref.PLANE_Z, hole=True)      # the table, both spheres, a hole
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sc = stub_scene(0)
    box = np.asarray([tref.ORIGIN, np.asarray(tref.ORIGIN) + tref.SIZE], f32)
    scene = {'target': sc['target'].cuda(), 'stub': dict({k: v.cuda() for k, v in sc['stub'].items()}, volume=up(sdf)[None, None]),
             'que_imgs_info': {k: v.cuda() for k, v in sc['que_imgs_info'].items()},
             'ref_imgs_info': {'poses': up(poses), 'Ks': up(Ks), 'bbox3d': up(box), 'true_depth': up(true)[:, None]}}
    net = StubNet().cuda()
    off = validation.Validator()(net, [scene])
    on = validation.Validator(volume_depth=True)(net, [scene])
    assert set(on[0]) == set(off[0]) | {'volume_depth_mae'} and on[1] == off[1]
    for k in off[0]:
        assert same(np.float64(on[0][k]), np.float64(off[0][k])), k
    b64 = box.astype(f64)
    scale = float(b64[1, 0] - b64[0, 0]) / R
    img = ref.raycast(sdf, poses, Ks, H1, W1, origin=b64[0] + 0.5 * scale, scale=scale)
    both = (img > 0) & (true > 0)
    want = np.abs(img.astype(f64) - true.astype(f64))[both].mean()
    print(f'volume_depth_mae {on[0]["volume_depth_mae"]:.6e}, numpy over the statement {want:.6e}, {both.sum()} pixels')
    assert both.sum() > 400 and abs(on[0]['volume_depth_mae'] - want) <= 1e-6 * want
    # no pixel where both have a depth: NaN
    empty = dict(scene, ref_imgs_info=dict(scene['ref_imgs_info'], true_depth=torch.zeros(3, 1, H1, W1, device='cuda')))
    assert math.isnan(validation.Validator(volume_depth=True)(net, [empty])[0]['volume_depth_mae'])
