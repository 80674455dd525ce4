"""View colours of surface points (csrc/gnr_surface_color.hip, surface_color.SurfaceColorizer, plan_real(view_colors=True)).
tests/surface_color_reference.py is the statement in numpy float64; the device's colours, weights and masks are compared with it by
np.array_equal on the bits.  Without a GPU: the statement against an analytic colour field painted on two spheres, the coverage
condition, occlusion by the volume, exact cases, the refusals made before the device is touched, and the keyword checks."""
import ctypes as C
import functools
import inspect
import types

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib
from graspnerf_amd.synth import CONFIGS, ring_cameras
import mesh_reference as mref
import raycast_reference as rref
import surface_color_reference as ref
import tsdf_reference as tref
from test_surface_mesh import same
from test_volume_raycast import FRAME, _scenes, _world, look_at

f32, f64 = np.float32, np.float64
K_CFG1 = np.asarray(CONFIGS['cfg1']['K'], f32).reshape(3, 3)
H1, W1 = 96, 128                                                               # cfg1's image size
R_FIELD, TRUNC = 40, 4                                                         # the analytic scene: 40^3, a TSDF truncated at 4 voxels


# ---- 1. the statement against an analytic colour field (no GPU) ---------------------------------------------------------------------
def field(X):
    """A smooth colour of the world point X [..,3] in [0.1, 0.9]^3 (wavelengths of 0.2 m and more: a pixel of cfg1's cameras at 0.5 m
    covers about 4 mm)."""
    X = np.asarray(X, f64)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    return np.stack([0.5 + 0.4 * np.sin(25.0 * x + 8.0 * y + 0.3), 0.5 + 0.4 * np.sin(-9.0 * x + 22.0 * y + 12.0 * z + 1.1),
                     0.5 + 0.4 * np.cos(14.0 * x - 6.0 * y + 20.0 * z)], -1)


def paint(poses):
    """Images [V,3,H1,W1] float32 of the table and the two spheres of tsdf_reference: every pixel holds `field` at its ray's hit point
    (tsdf_reference.render_depth gives the depth)."""
    depth = tref.render_depth(poses, K_CFG1, H1, W1, hole=False).astype(f64)
    vs, us = np.meshgrid(np.arange(H1, dtype=f64), np.arange(W1, dtype=f64), indexing='ij')
    dc = np.stack([(us - K_CFG1[0, 2]) / K_CFG1[0, 0], (vs - K_CFG1[1, 2]) / K_CFG1[1, 1], np.ones_like(us)], -1)
    out = []
    for i, P in enumerate(np.asarray(poses, f64)):
        Rm, t = P[:, :3], P[:, 3]
        X = -Rm.T @ t + depth[i][..., None] * (dc @ Rm)
        out.append(np.where(depth[i][..., None] > 0, field(X), 0.0).transpose(2, 0, 1))
    return np.stack(out).astype(f32)


def occluded_camera():
    """A camera on the line through both sphere centres, 0.4 m beyond the large one: the small sphere is entirely behind the large."""
    (c0, _), (c1, _) = tref.SPHERES
    c0, c1 = np.asarray(c0, f64), np.asarray(c1, f64)
    along = (c0 - c1) / np.linalg.norm(c0 - c1)
    return look_at(c0 + 0.4 * along, c0)


@functools.lru_cache(maxsize=None)
def spheres40():
    """The two spheres of tsdf_reference.SPHERES at R = 40 as a TSDF truncated at 4 voxels, the cloud |tsdf| < 0.2, the three ring
    cameras and the camera behind the large sphere with their painted images, and the statement's colours from the three and from all
    four: computed once, shared, never written to."""
    R, voxel = R_FIELD, tref.SIZE / R_FIELD
    c = (np.arange(R, dtype=f64) + 0.5) * voxel
    XYZ = np.stack(np.meshgrid(c + tref.ORIGIN[0], c + tref.ORIGIN[1], c + tref.ORIGIN[2], indexing='ij'), -1)
    centres, radii = np.array([s[0] for s in tref.SPHERES], f64), np.array([s[1] for s in tref.SPHERES], f64)
    sdf = (np.linalg.norm(XYZ[..., None, :] - centres, axis=-1) - radii).min(-1)
    vol = np.clip(sdf / (TRUNC * voxel), -1.0, 1.0).astype(f32)
    x = XYZ[tuple(np.argwhere(np.abs(vol) < 0.2).T)]
    poses = np.concatenate([ring_cameras(3)[:, :3, :], occluded_camera()[None]]).astype(f32)
    Ks = np.repeat(K_CFG1[None], 4, 0)
    images = paint(poses)
    frame = dict(origin=np.asarray(tref.ORIGIN, f64) + 0.5 * voxel, scale=voxel)
    d3, d4 = {}, {}
    three = ref.color_world(vol, x, images[:3], poses[:3], Ks[:3], details=d3, **frame)
    four = ref.color_world(vol, x, images, poses, Ks, details=d4, **frame)
    dist = np.linalg.norm(x[:, None] - centres, axis=-1) - radii
    which = np.argmin(np.abs(dist), 1)
    out = x - centres[which]
    nearest = centres[which] + radii[which, None] * out / np.linalg.norm(out, axis=1, keepdims=True)
    return dict(vol=vol, x=x, which=which, nearest=nearest, three=three, d3=d3, four=four, d4=d4)


# measured with this statement (R = 40, ring_cameras(3), cfg1's K at 96 x 128, bias 1.5, step 0.5), the largest channel difference over the
# 784 coloured points of 920: max 0.4647, mean 0.0455 (the largest sit on points a camera sees at a grazing angle next to the
# silhouette, where the bilinear tap mixes the table's colour in);  over the 560 strongly faced points: max 0.3054, mean 0.0358.
# The bounds are 1.5 x these, rounded up.
FIELD_BOUNDS = (0.70, 0.069)


def test_statement_on_an_analytic_colour_field():
    s = spheres40()
    colors, weight, mask = s['three']
    some = weight > 0
    err = np.abs(colors.astype(f64) - field(s['nearest'])).max(1)
    strong = (s['d3']['inside'] & (s['d3']['cos'] > 0.5)).any(0)
    print(f'R = {R_FIELD}: {len(err)} cloud points, {some.sum()} coloured: max {err[some].max():.4f} mean {err[some].mean():.4f};  '
          f'{strong.sum()} strongly faced: max {err[strong & some].max():.4f} mean {err[strong & some].mean():.4f}')
    assert colors.dtype == f32 and weight.dtype == f32 and mask.dtype == np.int32
    assert len(err) == 920 and some.sum() == 784
    assert err[some].max() <= FIELD_BOUNDS[0] and err[some].mean() <= FIELD_BOUNDS[1]
    assert np.array_equal(mask != 0, some) and not colors[~some].any()          # no view: fill = 0, weight 0, mask 0


def test_coverage_of_the_strongly_faced_points():
    """A point is strongly faced when for at least one view it projects inside the image and the volume's normal makes cos > 0.5 with
    the direction to that camera.  Measured with this statement: 100 % of them are coloured (asserted: >= 98 %)."""
    s = spheres40()
    strong = (s['d3']['inside'] & (s['d3']['cos'] > 0.5)).any(0)
    frac = float((s['three'][1] > 0)[strong].mean())
    print(f'{strong.sum()} of {len(strong)} cloud points are strongly faced by one of 3 ring cameras, {100 * frac:.2f} % of them are coloured')
    assert strong.sum() >= 500 and frac >= 0.98


def test_occlusion_by_the_volume():
    s = spheres40()
    colors, weight, mask = s['four']
    small = s['which'] == 1
    bit = (mask >> 3) & 1
    assert small.sum() > 200 and not bit[small].any(), 'a point of the small sphere is coloured from the camera behind the large one'
    assert s['d4']['occluded'][3][small].sum() > 50                             # ... because the march met the large sphere, not for want of candidates
    assert bit[~small].sum() > 100                                              # the large sphere's near side is seen by that camera
    faced = (s['d4']['inside'][:3] & (s['d4']['cos'][:3] > 0.5)).any(0)
    assert (small & faced).sum() > 100 and (weight[small & faced] > 0).all()    # what a ring camera faces still has a colour
    for a, b in zip(s['three'], s['four']):                                     # the fourth view changes nothing on the small sphere
        assert same(a[small], b[small])


# ---- 2. exact cases (no GPU) ------------------------------------------------------------------------------------------------------------
EXACT = dict(origin=(-0.25, -0.25, 0.5), scale=0.125)                           # the world point (0.125, 0, 1) is the lattice point (3, 2, 4)


def _facing_plane(R=8, level=4.0):
    """level - z: outside (positive) towards z = 0, where the identity camera sits; the gradient points at it."""
    return (level - np.indices((R, R, R))[2]).astype(f32)


def test_exact_cases():
    eye3 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32)           # the camera at the world's origin, looking along +z
    K = np.array([[256, 0, 0], [0, 256, 1], [0, 0, 1]], f32)
    W, H = 33, 5
    rng = np.random.default_rng(5)
    images = rng.random((2, 3, H, W)).astype(f32)
    vol = _facing_plane()
    x = np.array([[0.125, 0.0, 1.0], [np.nextafter(0.125, 1.0), 0.0, 1.0], [0.0625, 0.0, 1.0]])
    poses, Ks = np.stack([eye3, eye3]), np.stack([K, K])
    # u == W - 1 contributes, the next representable value above it does not
    d = {}
    colors, weight, mask = ref.color_world(vol, x, images, poses, Ks, details=d, **EXACT)
    assert mask.tolist() == [3, 0, 3] and weight[1] == 0 and weight[0] > 0 and not colors[1].any()
    assert np.array_equal(d['p'][0], [3.0, 2.0, 4.0]) and np.array_equal(d['g'][0], [0.0, 0.0, -1.0])
    # ... and the tap at u = W - 1, v = 1 is the last texel of row 1, the mean of the two views' in view order
    c0 = d['cos'][0, 0]
    want = [f32((c0 * f64(images[0, ch, 1, W - 1]) + c0 * f64(images[1, ch, 1, W - 1])) / (c0 + c0)) for ch in range(3)]
    assert same(colors[0], np.array(want, f32))
    # a constant image gives exactly that constant wherever a view contributes
    const = np.empty((2, 3, H, W), f32)
    const[:] = np.array([0.3, 0.55, 0.7], f32)[None, :, None, None]
    pts = np.stack([rng.uniform(-0.12, 0.12, 50), rng.uniform(-0.004, 0.012, 50), rng.uniform(0.9, 1.0, 50)], 1)
    poses2 = np.stack([eye3, look_at((0.05, 0.0, 0.0), (0.0, 0.0, 1.0), up=(0, 1, 0))])
    colors, weight, mask = ref.color_world(vol, pts, const, poses2, Ks, **EXACT)
    assert (weight > 0).sum() >= 20 and same(colors[weight > 0], np.repeat(const[0, :, 0, 0][None], (weight > 0).sum(), 0))
    # all views behind the point: fill, weight 0, mask 0
    fill = (0.25, 0.5, 0.75)
    colors, weight, mask = ref.color_world(vol, np.array([[0.0, 0.0, -1.0], [0.1, 0.0, -0.5]]), images, poses, Ks, fill=fill, **EXACT)
    assert same(colors, np.repeat(np.array(fill, f32)[None], 2, 0)) and not weight.any() and not mask.any()
    # a volume without a gradient (n2 == 0) and a point at the eye (L == 0): no view
    flat = ref.color_world(np.ones((8, 8, 8), f32), x, images, poses, Ks, **EXACT)
    assert not flat[1].any() and not flat[2].any()
    at_eye = ref.color_world(vol, np.zeros((1, 3)), images, poses, Ks, **EXACT)
    assert not at_eye[1].any() and not at_eye[2].any()
    # the level decides: with iso above the values on the way, the march is below the level at its first sample
    assert not ref.color_world(vol, x, images, poses, Ks, iso=100.0, **EXACT)[1].any()
    # cos_min: the cosine of point 0 is 8 / sqrt(65)
    assert abs(c0 - 8.0 / np.sqrt(65.0)) <= 1e-15
    assert ref.color_world(vol, x, images, poses, Ks, cos_min=c0, **EXACT)[2][0] == 0                 # c > cos_min is strict
    assert ref.color_world(vol, x, images, poses, Ks, cos_min=np.nextafter(c0, 0.0), **EXACT)[2][0] == 3
    # points mode leaves rows beyond the count untouched; pixels mode gives fill where the depth is 0
    out = (np.full((3, 3), 7, f32), np.full(3, 7, f32), np.full(3, 7, np.int32))
    ref.color_points(vol, x, 1, images, poses, Ks, out=out, **EXACT)
    assert out[2].tolist() == [3, 7, 7] and (out[0][1:] == 7).all() and (out[1][1:] == 7).all()
    depth = np.zeros((1, 4, 6), f32)
    depth[0, 1, 2] = 1.0
    Kc = np.array([[8, 0, 1], [0, 8, 1], [0, 0, 1]], f32)                         # pixel (2, 1) of the target camera looks at (0.125, 0, 1)
    pc, pw, pm = ref.color_pixels(vol, depth, eye3[None], Kc[None], images, poses, Ks, fill=fill, **EXACT)
    assert pm[0, 1, 2] == 3 and pm.sum() == 3 and same(pc[0, 0, 0], np.array(fill, f32))
    assert same(pc[0, 1, 2], ref.color_world(vol, x[:1], images, poses, Ks, fill=fill, **EXACT)[0][0])


# ---- 3. the C ABI's refusals, before the device (no GPU) --------------------------------------------------------------------------------
def _params(**kw):
    p = _lib.GnrSurfaceColorParams(B=1, V=3, H=8, W=8, R=8, iso=0.0, scale=1.0, step=0.5, bias=1.5, cos_min=0.0)
    for k, v in kw.items():
        if k in ('origin', 'point_offset', 'fill'):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    return p


def test_refusals_before_the_device():
    """Fake pointers: every call is one that validation refuses, each with its code and a text that names the entry point and the limit."""
    L = _lib.lib()
    one = C.c_void_p(16)
    text = lambda: L.gnr_last_error().decode()

    def points(p=None, max_n=4, stride=1, **kw):
        ptr = {k: kw.pop(k, one) for k in ('vol', 'points', 'count', 'images', 'poses', 'Ks', 'colors', 'weight', 'views')}
        p = _params(**kw) if p is None else p
        return L.gnr_surface_color_points_fwd(C.byref(p) if p is not False else None, ptr['vol'], ptr['points'], ptr['count'], stride, max_n,
                                              ptr['images'], ptr['poses'], ptr['Ks'], ptr['colors'], ptr['weight'], ptr['views'], None)

    def pixels(p=None, Vc=2, hc=4, wc=4, **kw):
        ptr = {k: kw.pop(k, one) for k in ('vol', 'depth', 'cam_poses', 'cam_Ks', 'images', 'poses', 'Ks', 'colors', 'weight', 'views')}
        p = _params(**kw) if p is None else p
        return L.gnr_surface_color_pixels_fwd(C.byref(p) if p is not False else None, ptr['vol'], ptr['depth'], ptr['cam_poses'], ptr['cam_Ks'],
                                              Vc, hc, wc, ptr['images'], ptr['poses'], ptr['Ks'], ptr['colors'], ptr['weight'], ptr['views'], None)

    for call, fn, names in ((points, 'gnr_surface_color_points_fwd', ('vol', 'points', 'count', 'images', 'poses', 'Ks', 'colors', 'weight', 'views')),
                            (pixels, 'gnr_surface_color_pixels_fwd', ('vol', 'depth', 'cam_poses', 'cam_Ks', 'images', 'poses', 'Ks', 'colors',
                                                                      'weight', 'views'))):
        for name in names:
            assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', (fn, name)
        assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
        for B in (0, -1, 65536):
            assert call(B=B) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', B
        for V in (0, -2, 33):
            assert call(V=V) == _lib.GNR_ERR_SHAPE and 'V must be in 1..32' in text() and fn in text(), V
        for kw in (dict(H=1), dict(W=1), dict(H=0), dict(W=-4)):
            assert call(**kw) == _lib.GNR_ERR_SHAPE and 'H and W must be >= 2' in text(), kw
        for R in (1, 0, 257):
            assert call(R=R) == _lib.GNR_ERR_SHAPE and 'R must be in 2..256' in text(), R
        for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf')), dict(step=0.0), dict(step=-0.5),
                   dict(step=float('nan')), dict(step=float('inf'))):
            assert call(**kw) == _lib.GNR_ERR_ARG and 'scale and step must be finite and > 0' in text(), kw
        for bias in (-1e-9, float('nan'), float('inf')):
            assert call(bias=bias) == _lib.GNR_ERR_ARG and 'bias must be finite and >= 0' in text(), bias
        nan, inf = float('nan'), float('inf')
        for kw in (dict(iso=nan), dict(iso=inf), dict(origin=[0.0, nan, 0.0]), dict(origin=[-inf, 0.0, 0.0]), dict(point_offset=[0.0, 0.0, nan]),
                   dict(point_offset=[inf, 0.0, 0.0]), dict(cos_min=nan), dict(cos_min=-inf), dict(fill=[0.0, nan, 0.0]), dict(fill=[0.0, 0.0, inf])):
            assert call(**kw) == _lib.GNR_ERR_ARG and 'iso, origin, point_offset, cos_min and fill must be finite' in text(), kw
        # the march's loop bound is the ray cast's: ceil(sqrt(3) (R-1) / step) + 1 samples at most
        assert call(R=256, step=1e-3) == _lib.GNR_ERR_ARG and 'GNR_RAYCAST_MAX_SAMPLES' in text() and str(_lib.GNR_RAYCAST_MAX_SAMPLES) in text()
    assert rref.max_samples(256, 1e-2) <= _lib.GNR_RAYCAST_MAX_SAMPLES < rref.max_samples(256, 1e-3)
    for n in (0, -1):
        assert points(max_n=n) == _lib.GNR_ERR_SHAPE and 'max_n must be >= 1' in text(), n
    assert points(stride=0) == _lib.GNR_ERR_ARG and 'count_stride must be >= 1' in text()
    assert pixels(Vc=0) == _lib.GNR_ERR_SHAPE and 'Vc must be >= 1' in text()
    for kw in (dict(hc=0), dict(wc=0), dict(hc=-1)):
        assert pixels(**kw) == _lib.GNR_ERR_SHAPE and 'hc and wc must be >= 1' in text(), kw
    assert pixels(hc=2 ** 31 - 1, wc=2 ** 31 - 1) == _lib.GNR_ERR_SHAPE and '2^28 tiles' in text()


def test_colorizer_needs_a_gpu(monkeypatch):
    from graspnerf_amd.surface_color import SurfaceColorizer
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        SurfaceColorizer()


# ---- 4. keyword checks (no GPU) -----------------------------------------------------------------------------------------------------------
def test_keyword_checks():
    from graspnerf_amd import planner, surface_color
    from graspnerf_amd.grasp_post import GRASP_UTILS_PROCESS
    from graspnerf_amd.planner_session import PlannerSession
    frames, cams = [np.zeros((8, 8, 3), np.uint8)] * 4, [np.eye(4)] * 4
    with pytest.raises(TypeError, match='unknown view_colors parameters'):
        planner.plan_real(None, frames, cams, np.eye(3), view_colors={'bogus': 1})
    with pytest.raises(TypeError, match='unknown view_colors parameters'):
        planner.real_session(None, 4, (8, 8), (32, 32), view_colors={'iso': 0.0})
    assert surface_color.color_params(False) is None and surface_color.color_params(None) is None
    assert surface_color.color_params(True) == dict(step=0.5, bias=1.5, cos_min=0.0, fill=(0.0, 0.0, 0.0))
    p = surface_color.color_params(dict(step=1, fill=[0.25, 0.5, 0.75]))
    assert p == dict(step=1.0, bias=1.5, cos_min=0.0, fill=(0.25, 0.5, 0.75)) and isinstance(p['step'], float)
    with pytest.raises(ValueError, match='three numbers'):
        surface_color.color_params(dict(fill=(0, 0)))
    assert planner.same_params(p, dict(p, origin=(0, 0, 0))) and not planner.same_params(p, surface_color.color_params(True))
    assert not planner.same_params(p, None) and planner.same_params(None, None)
    assert surface_color.cloud_level((-0.2, 0.2)) == 0.0 and surface_color.cloud_level((0.25, 0.5)) == 0.375
    for fn, default in ((planner.plan_real, False), (planner.real_session, False), (PlannerSession.__init__, None)):
        assert inspect.signature(fn).parameters['view_colors'].default is default, fn
    # a session built without the switch and asked for it, and the other way round: the session-mismatch error, which names the switch
    net = object()
    built = lambda vc: types.SimpleNamespace(net=net, selector_params=dict(GRASP_UTILS_PROCESS, order='index', top_k=None), surface_params=dict(rg=(-0.2, 0.2)),
                                             voxel_size=planner.REAL_VOXEL_SIZE, surface_normals=False, mesh_params=None, volume_depth_params=None,
                                             view_color_params=surface_color.color_params(vc, origin=(0.0, 0.0, 0.0)), hand_params=None,
                                             closure_params=None)
    for have, ask in ((False, True), (True, False), (True, dict(bias=2.0))):
        with pytest.raises(ValueError, match=r'the session was built for another .*volume_depth or view_colors \(build it with planner.real_session\)'):
            planner.plan_real(net, frames, cams, np.eye(3), session=built(have), view_colors=ask)


# ---- GPU: the bits of the statement -------------------------------------------------------------------------------------------------------
SRC_HW = (24, 32)                                                              # the source images of the GPU tests
DEFAULT_SET = dict(iso=0.0, step=0.5, bias=1.5, cos_min=0.0, fill=(0.0, 0.0, 0.0))
OTHER_SET = dict(iso=0.3, step=1.0, bias=0.0, cos_min=0.3, fill=(0.25, 0.5, 0.75))
SENTINEL = 0x5a


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _sentinel(rows, width, dtype):
    """[rows + 1, width] of `dtype` on the device, every byte the sentinel: one spare row behind what the call is told about."""
    return torch.full(((rows + 1) * width * 4,), SENTINEL, dtype=torch.uint8, device='cuda:0').view(dtype)


def _kept(t):
    return bool((t.view(np.uint8) == SENTINEL).all())


def _fill_params(B, V, H, W, R, kw, origin, scale, point_offset=(0.0, 0.0, 0.0)):
    return _params(B=B, V=V, H=H, W=W, R=R, iso=kw['iso'], scale=scale, step=kw['step'], bias=kw['bias'], cos_min=kw['cos_min'],
                   fill=list(kw['fill']), origin=list(origin), point_offset=list(point_offset))


def _raw_points(vol, points, count, images, poses, Ks, kw, point_offset=(0.0, 0.0, 0.0)):
    """The C call on outputs filled with a sentinel byte, with one more row behind [B,max_n] that the call is not told about
    -> (colors [B,max_n,3], weight [B,max_n], views [B,max_n]) as numpy, and whether the spare rows kept the sentinel."""
    L = _lib.lib()
    B, R, V = vol.shape[0], vol.shape[-1], poses.shape[1]
    n = points.shape[1]
    count = np.ascontiguousarray(count, np.int32)
    dev = [_up(a) for a in (vol, np.asarray(points, f64), count, images, poses, Ks)]
    colors, weight, views = _sentinel(B * n, 3, torch.float32), _sentinel(B * n, 1, torch.float32), _sentinel(B * n, 1, torch.int32)
    p = _fill_params(B, V, *images.shape[-2:], R, kw, FRAME['origin'], FRAME['scale'], point_offset)
    rc = L.gnr_surface_color_points_fwd(C.byref(p), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), count.size // B, n, dev[3].data_ptr(),
                                        dev[4].data_ptr(), dev[5].data_ptr(), colors.data_ptr(), weight.data_ptr(), views.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'gnr_surface_color_points_fwd')
    torch.cuda.synchronize()
    colors, weight, views = (t.cpu().numpy() for t in (colors, weight, views))
    spare = _kept(colors[3 * B * n:]) and _kept(weight[B * n:]) and _kept(views[B * n:])
    return (colors[:3 * B * n].reshape(B, n, 3), weight[:B * n].reshape(B, n), views[:B * n].reshape(B, n)), spare


def _want_points(vol, points, count, images, poses, Ks, kw, point_offset=(0.0, 0.0, 0.0)):
    """The statement on the same sentinel-filled outputs, scene by scene."""
    B, n = points.shape[:2]
    out = []
    for b in range(B):
        o = tuple(np.full(4 * n * w, SENTINEL, np.uint8).view(t).reshape(shape) for w, t, shape in ((3, f32, (n, 3)), (1, f32, (n,)), (1, np.int32, (n,))))
        out.append(ref.color_points(vol[b], points[b], np.asarray(count).reshape(B, -1)[b, 0], images[b], poses[b], Ks[b], point_offset=point_offset,
                                    **FRAME, **kw, out=o))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _sources(R, seed=0):
    """_scenes(R) of the ray cast's tests -- two volumes (a sphere; a torus at R = 16, else a plane) with three cameras each (scene 0: from
    outside, straight down with a d_a == 0 axis, from inside the object;  scene 1: from outside, one that looks away, from below), another
    intrinsic matrix per view -- and random source images 24 x 32 per scene and view."""
    vol, poses, Ks = _scenes(R)
    images = np.random.default_rng(100 + R + seed).random((2, 3, 3, *SRC_HW)).astype(f32)
    return vol, poses, Ks(*SRC_HW), images


def _check_points(what, vol, points, count, images, poses, Ks, kw, point_offset=(0.0, 0.0, 0.0)):
    got, spare = _raw_points(vol, points, count, images, poses, Ks, kw, point_offset)
    want = _want_points(vol, points, count, images, poses, Ks, kw, point_offset)
    assert spare, (what, 'written beyond [B,max_n]')
    for name, g, w in zip(('colors', 'weight', 'views'), got, want):
        assert same(g, w), (what, kw['step'], name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('R', [6, 16])
def test_points_mode_equals_the_statement(R):
    """B = 2, V = 3, 24 x 32 sources.  The cloud's lattice points, the mesh's off-lattice vertices (count stride 2) and hand-made rows;
    max_n lies between the two scenes' counts, so one scene is cut at max_n and the other leaves rows untouched."""
    from graspnerf_amd.grasp_post import MeshExtractor, SurfaceExtractor
    vol, poses, Ks, images = _sources(R)
    eye = ref.camera(poses[0, 0], Ks[0, 0])[2]
    hand = np.stack([_world((0, 0, 0)), _world((R - 1, R - 1, R - 1)), _world((R + 2.5, -3.0, 0.5 * R)), eye, _world((0.5 * R, 0.4 * R, 0.9 * R))])
    for kw in (DEFAULT_SET, OTHER_SET):
        used = 0
        cloud = SurfaceExtractor()(vol, rg=(kw['iso'] - 0.7, kw['iso'] + 0.7), scale=FRAME['scale'])      # around the level that occludes
        mesh = MeshExtractor()(vol, iso=kw['iso'], scale=FRAME['scale'])
        for what, pts, cnt in (('cloud', cloud['points'], cloud['count']), ('mesh', mesh['vertices'], mesh['count'])):
            pts, cnt = pts.cpu().numpy(), cnt.cpu().numpy()
            n = np.sort(cnt.reshape(2, -1)[:, 0])
            assert n[0] >= 8 and n[1] - n[0] >= 2, (what, n)
            max_n = int(n.sum() // 2)                                             # between the two counts
            want = _check_points(what, vol, np.ascontiguousarray(pts[:, :max_n]), cnt, images, poses, Ks, kw, point_offset=FRAME['origin'])
            live = np.arange(max_n)[None] < np.minimum(cnt.reshape(2, -1)[:, :1], max_n)
            used += int((want[1][live] > 0).sum())
            # (bias = 0 puts the first sample on the point itself: a vertex, which lies on the level, is then occluded or not by a rounding)
            assert (want[1][live] > 0).sum() >= (8 if kw['bias'] > 0 or what == 'cloud' else 0), (what, 'no view sees these points')
        want = _check_points('hand-made rows', vol, np.stack([hand, hand]), np.array([5, 4], np.int32), images, poses, Ks, kw)
        assert want[1][0, 3] == 0 or not (want[2][0, 3] & 1), 'the point at the eye of view 0 is coloured from view 0'
        print(f'R = {R}, step {kw["step"]}: {used} cloud and mesh points coloured')


@pytest.mark.gpu
@pytest.mark.parametrize('V', [1, 32])
def test_mask_limits(V):
    """V = 1, and V = 32 with 4 x 4 images at R = 6: the mask's top bit."""
    R = 6
    mid = (R - 1) / 2.0
    vol = mref.sphere(R, (mid, mid, mid), 0.3 * R)[None].astype(f32)
    c = _world((mid, mid, mid))
    far = 2.0 * R * FRAME['scale']
    ring = [np.array([np.cos(a), np.sin(a), 0.8]) for a in 2 * np.pi * np.arange(V) / V]
    poses = np.stack([look_at(c + far * d / np.linalg.norm(d), c) for d in ring])[None].astype(f32)
    Ks = np.repeat(np.array([[4.0, 0, 1.5], [0, 4.0, 1.5], [0, 0, 1]], f32)[None], V, 0)[None]
    images = np.random.default_rng(V).random((1, V, 3, 4, 4)).astype(f32)
    g = np.indices((R, R, R)).reshape(3, -1).T
    pts = _world(g[np.abs(vol[0].ravel()) < 0.7])[None]
    want = _check_points(f'V = {V}', vol, pts, np.array([pts.shape[1]], np.int32), images, poses, Ks, DEFAULT_SET)
    seen = np.bitwise_or.reduce(want[2][0].view(np.uint32))
    assert seen == (1 << V) - 1, f'views seen: {seen:#x}'
    if V == 32:
        assert (want[2] < 0).any()                                                # bit 31 is the int32's sign


def _raw_pixels(vol, depth, cam_poses, cam_Ks, images, poses, Ks, kw):
    L = _lib.lib()
    B, R, V = vol.shape[0], vol.shape[-1], poses.shape[1]
    Vc, h, w = depth.shape[1:]
    dev = [_up(a) for a in (vol, depth, cam_poses, cam_Ks, images, poses, Ks)]
    n = B * Vc * h
    colors, weight, views = _sentinel(n, 3 * w, torch.float32), _sentinel(n, w, torch.float32), _sentinel(n, w, torch.int32)
    p = _fill_params(B, V, *images.shape[-2:], R, kw, FRAME['origin'], FRAME['scale'])
    rc = L.gnr_surface_color_pixels_fwd(C.byref(p), *(t.data_ptr() for t in dev[:4]), Vc, h, w, *(t.data_ptr() for t in dev[4:]), colors.data_ptr(),
                                        weight.data_ptr(), views.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'gnr_surface_color_pixels_fwd')
    torch.cuda.synchronize()
    colors, weight, views = (t.cpu().numpy() for t in (colors, weight, views))
    spare = _kept(colors[3 * n * w:]) and _kept(weight[n * w:]) and _kept(views[n * w:])
    return (colors[:3 * n * w].reshape(B, Vc, h, w, 3), weight[:n * w].reshape(B, Vc, h, w), views[:n * w].reshape(B, Vc, h, w)), spare


@pytest.mark.gpu
@pytest.mark.parametrize('hw', [(24, 32), (37, 53)])
@pytest.mark.parametrize('R', [8, 16])
def test_pixels_mode_equals_the_statement(R, hw):
    """Depth from VolumeRaycaster from Vc = 2 novel cameras (37 x 53 is no multiple of the 8 x 8 tile: the row behind the images keeps its
    sentinel), V = 3 sources; a miss gives fill."""
    from graspnerf_amd.raycast import VolumeRaycaster
    vol, poses, Ks, images = _sources(R)
    h, w = hw
    mid = (R - 1) / 2.0
    c = _world((mid, mid, mid))
    far = 2.0 * R * FRAME['scale']
    cam_poses = np.stack([np.stack([look_at(c + far * np.array([0.5, -0.6, 0.62]), c), look_at(c + far * np.array([-0.3, 0.2, 0.93]), c, up=(0, 1, 0))])] * 2)
    cam_Ks = np.stack([np.stack([np.array([[f * w, 0, cx], [0, f * w, cy], [0, 0, 1]], f32)
                                 for f, cx, cy in ((1.0, 0.5 * w - 0.5, 0.5 * h - 0.5), (0.8, 0.45 * w, 0.55 * h))])] * 2)
    for kw in (DEFAULT_SET, OTHER_SET):
        depth = VolumeRaycaster()(vol, cam_poses, cam_Ks, hw, iso=kw['iso'], **FRAME)['depth'].cpu().numpy()
        got, spare = _raw_pixels(vol, depth, cam_poses, cam_Ks, images, poses, Ks, kw)
        assert spare, 'written beyond [B,Vc,h,w]'
        for b in range(2):
            want = ref.color_pixels(vol[b], depth[b], cam_poses[b], cam_Ks[b], images[b], poses[b], Ks[b], **FRAME, **kw)
            for name, g_, w_ in zip(('colors', 'weight', 'views'), got, want):
                assert same(g_[b], w_), (kw['step'], b, name, int((g_[b].view(np.uint32) != w_.view(np.uint32)).sum()))
            miss = depth[b] == 0
            assert miss.sum() > 20 and (depth[b] > 0).sum() > 20, b
            assert same(want[0][miss], np.repeat(np.array(kw['fill'], f32)[None], miss.sum(), 0)) and not want[1][miss].any() and not want[2][miss].any()
            assert (want[1] > 0).sum() > 20, (b, 'no pixel is coloured')


@pytest.mark.gpu
def test_reproducible_and_batch_equals_single_scenes():
    """The same call twice gives the same bits (and writes the same kept buffers); a B = 2 call equals the two B = 1 calls."""
    from graspnerf_amd.grasp_post import MeshExtractor
    from graspnerf_amd.raycast import VolumeRaycaster
    from graspnerf_amd.surface_color import SurfaceColorizer
    R = 16
    vol, poses, Ks, images = _sources(R)
    mesh = MeshExtractor()(vol, scale=FRAME['scale'])
    paint = SurfaceColorizer()
    kw = dict(FRAME, point_offset=FRAME['origin'])
    host = lambda res: {k: v.cpu().numpy() for k, v in res.items()}
    first = paint.points(vol, mesh['vertices'], mesh['count'], images, poses, Ks, **kw)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    a = host(first)
    second = paint.points(vol, mesh['vertices'], mesh['count'], images, poses, Ks, **kw)
    assert {k: v.data_ptr() for k, v in second.items()} == ptrs
    b = host(second)
    n = mesh['count'][:, 0].tolist()
    assert set(a) == {'view_colors', 'view_weight', 'view_mask'} and all(same(a[k], b[k]) for k in a)
    for s in range(2):
        one = host(SurfaceColorizer().points(vol[s], mesh['vertices'][s:s + 1], mesh['count'][s:s + 1].contiguous(), images[s], poses[s], Ks[s], **kw))
        want = ref.color_points(vol[s], mesh['vertices'][s].cpu().numpy(), n[s], images[s], poses[s], Ks[s], point_offset=FRAME['origin'], **FRAME)
        for k, w_ in zip(('view_colors', 'view_weight', 'view_mask'), want):
            assert same(one[k][0, :n[s]], a[k][s, :n[s]]) and same(one[k][0, :n[s]], w_[:n[s]]), (s, k)
    depth = VolumeRaycaster()(vol, poses, Ks, (21, 30), **FRAME)['depth']
    pa = host(paint.pixels(vol, depth, poses, Ks, images, poses, Ks, **FRAME))
    pb = host(paint.pixels(vol, depth, poses, Ks, images, poses, Ks, **FRAME))
    assert set(pa) == {'color', 'color_weight', 'color_mask'} and all(same(pa[k], pb[k]) for k in pa) and (pa['color_weight'] > 0).sum() > 50
    for s in range(2):
        one = host(SurfaceColorizer().pixels(vol[s], depth[s], poses[s], Ks[s], images[s], poses[s], Ks[s], **FRAME))
        assert all(same(one[k][0], pa[k][s]) for k in pa), s


@pytest.mark.gpu
def test_plan_real_with_view_colors_eager_and_session():
    """The small net of tests/test_planner_session_real.py.  The synthetic checkpoint's volume need not cross zero: the cloud's range, the
    mesh's and the ray cast's level are taken from the eager volume itself."""
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
    kw = dict(order='score', top_k=TOP_K, surface_rg=rg, mesh=dict(iso=iso), volume_depth=dict(iso=iso))
    off = planner.plan_real(net, A, **cam, **kw)
    eager = planner.plan_real(net, A, **cam, **kw, view_colors=True)
    sess = planner.real_session(net, V, HW, HW[::-1], **{**kw, 'view_colors': True})
    got = planner.plan_real(net, A, **cam, **kw, view_colors=True, session=sess)
    other = planner.plan_real(net, B, **cam, **kw, view_colors=True, session=sess)
    again = planner.plan_real(net, A, **cam, **kw, view_colors=True, session=sess)
    assert sess.captures == 1
    # switch off: exactly today's keys, on both routes (a session's cloud also says its `count`)
    off_s = planner.plan_real(net, A, **cam, **kw, session=planner.real_session(net, V, HW, HW[::-1], **kw))
    assert set(off[3]) == {'index', 'points', 'colors', 'mesh', 'volume_depth'} and set(off[3]['mesh']) == {'vertices', 'faces'}
    assert set(off_s[3]) == set(off[3]) | {'count'} and set(off_s[3]['mesh']) == set(off[3]['mesh'])
    new_cloud, new_mesh, new_img = {'view_colors', 'view_weight', 'view_mask'}, {'view_colors', 'view_weight', 'view_mask'}, {'volume_color', 'volume_color_weight'}
    frame = dict(origin=planner.real_volume_origin(), scale=planner.REAL_VOXEL_SIZE)
    poses, Ks = np.asarray(ext, f32)[:, :3, :], np.repeat(K[None], V, 0)
    imgs = (A.astype(f32) / 255).transpose(0, 3, 1, 2)
    for what, res in (('eager', eager), ('session', got), ('session, second replay', again)):
        cloud = res[3]
        today = off if what == 'eager' else off_s
        assert set(cloud) == set(today[3]) | new_cloud | new_img and set(cloud['mesh']) == set(today[3]['mesh']) | new_mesh, what
        # every other key equals the switch-off run bit for bit
        for k in ('index', 'pos', 'quat', 'width', 'score'):
            assert same(res[0][k], off[0][k]), (what, k)
        assert same(res[1], off[1]) and same(res[2], off[2]), what
        for k in ('index', 'points', 'colors', 'volume_depth'):
            assert same(cloud[k], off[3][k]), (what, k)
        for k in ('vertices', 'faces'):
            assert same(cloud['mesh'][k], off[3]['mesh'][k]), (what, 'mesh', k)
        # the new keys: the same bits on both routes, and the statement's
        for k in new_cloud | new_img:
            assert same(cloud[k], eager[3][k]), (what, k)
        for k in new_mesh:
            assert same(cloud['mesh'][k], eager[3]['mesh'][k]), (what, 'mesh', k)
        n, nv = len(cloud['points']), len(cloud['mesh']['vertices'])
        assert cloud['view_colors'].shape == (n, 3) and cloud['view_colors'].dtype == f32 and cloud['view_weight'].shape == (n,) \
            and cloud['view_mask'].shape == (n,) and cloud['view_mask'].dtype == np.int32 and cloud['mesh']['view_colors'].shape == (nv, 3)
        assert cloud['volume_color'].shape == (V, *HW, 3) and cloud['volume_color_weight'].shape == (V, *HW)
    cloud = eager[3]
    from graspnerf_amd.surface_color import cloud_level
    want = ref.color_points(eager[2], cloud['points'], len(cloud['points']), imgs, poses, Ks, point_offset=frame['origin'], iso=cloud_level(rg), **frame)
    for k, w_ in zip(('view_colors', 'view_weight', 'view_mask'), want):
        assert same(cloud[k], w_), ('cloud', k)
    mesh = cloud['mesh']
    wantm = ref.color_points(eager[2], mesh['vertices'], len(mesh['vertices']), imgs, poses, Ks, point_offset=frame['origin'], iso=iso, **frame)
    for k, w_ in zip(('view_colors', 'view_weight', 'view_mask'), wantm):
        assert same(mesh[k], w_), ('mesh', k)
    wantp = ref.color_pixels(eager[2], cloud['volume_depth'], poses, Ks, imgs, poses, Ks, iso=iso, **frame)
    assert same(cloud['volume_color'], wantp[0]) and same(cloud['volume_color_weight'], wantp[1])
    print(f'{(want[1] > 0).sum()} of {len(want[1])} cloud points, {(wantm[1] > 0).sum()} of {len(wantm[1])} vertices, {(wantp[1] > 0).sum()} pixels coloured')
    assert (wantm[1] > 0).sum() > 100 and (wantp[1] > 0).sum() > 100, 'the plan\'s cameras see nothing of the level set'
    # a second plan with other frames changes the colours
    assert not same(other[3]['volume_color'], got[3]['volume_color'])
    assert len(other[3]['view_colors']) != len(got[3]['view_colors']) or not same(other[3]['view_colors'], got[3]['view_colors'])
    # a session refuses a plan that asks for another colouring than its own
    with pytest.raises(ValueError, match='view_colors'):
        planner.plan_real(net, A, **cam, **kw, session=sess)
    with pytest.raises(ValueError, match='view_colors'):
        planner.plan_real(net, A, **cam, **kw, session=sess, view_colors=dict(bias=2.0))
