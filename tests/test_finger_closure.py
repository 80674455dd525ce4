"""Finger closure of the ranked grasps against the volume (k_finger_closure in csrc/gnr_hand.hip, hand.FingerClosure,
PlannerSession(finger_closure=...), plan_real(closure=True)).  tests/closure_reference.py is the statement in numpy float64; the device's
rows are compared with it by np.array_equal on the bits.  Without a GPU: the statement on a sphere (square and oblique contacts), in
empty space and inside a solid, under a halved spacing, the refusals made before the device is touched, and the keyword checks."""
import ctypes as C
import functools
import inspect
import types

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, grasp_post, hand
import closure_reference as cref
import hand_reference as href
from test_hand_clearance import ORIGIN, R40, VOXEL, sphere_volume
from test_surface_mesh import same

f32, f64 = np.float32, np.float64
DOWN = f32([1.0, 0.0, 0.0, 0.0])                                               # top-down: the approach is world -z, the closing direction world -y
RADIUS = 4.0                                                                   # voxels
CENTRE = np.array([19.7, 19.4, 20.1])                                          # lattice units, off the lattice's symmetries
# a hand whose pads are half a radius long: moved back by one radius, the pad row nearest the sphere's equator is half a radius below it
SHORT = dict(depth=0.5 * RADIUS * VOXEL)
KEYS = ('closed_width', 'finger_travel', 'contact_cos', 'finger_contact', 'grip_cos', 'held')


@functools.lru_cache(maxsize=None)
def sphere():
    """The truncated sphere of radius 4 voxels about CENTRE at R = 40: never written to."""
    vol = sphere_volume(ORIGIN + CENTRE * VOXEL, RADIUS * VOXEL)
    vol.setflags(write=False)
    return vol


def sphere_grasps():
    """(pos, analytic width in voxels, analytic cosine) of the two sphere grasps: at the centre, and one radius back along the approach
    (the approach of DOWN is world -z, so back is +z): there the pads' first row, the nearest to the equator, sits half a radius from it;
    the contact circle has radius sqrt(R^2 - (R/2)^2) and its normals make the cosine sqrt(1 - 1/4) with the closing direction."""
    back = CENTRE + [0.0, 0.0, RADIUS]
    d = RADIUS - SHORT['depth'] / VOXEL
    return ((CENTRE, 2.0 * RADIUS, 1.0), (back, 2.0 * np.sqrt(RADIUS ** 2 - d ** 2), np.sqrt(1.0 - (d / RADIUS) ** 2)))


def columns(out, **kw):
    """One statement result as the plan's columns (closure_from_rows on rows of one)."""
    rows = dict(zip(hand.CLOSURE_ROWS, (np.asarray(a)[None] for a in out)))
    return {k: v[0] for k, v in hand.closure_from_rows(rows, **kw).items()}


# ---- 1. the statement on analytic scenes (no GPU) ------------------------------------------------------------------------------------------
def test_sphere_square_and_oblique():
    """The hand opened to 12 voxels about a sphere of radius 4.  Width: within half a voxel (the volume's own resolution) of the chord.
    Observed once (spacing 0.5): at the centre a width of 7.951 voxels against 8 and cosines 0.99369 and 0.99365 against 1, so asserted
    within 2 * 0.00635; one radius back 6.873 voxels against 6.928 and cosines 0.82455 and 0.84065 against 0.86603 -- the gradient of the
    trilinear interpolant of a sphere four voxels in radius is piecewise, and coarse -- so asserted within 2 * 0.0415."""
    (centre, w0, c0), (back, w1, c1) = sphere_grasps()
    square = columns(cref.closure(sphere(), centre, DOWN, f32(12.0), VOXEL, **SHORT), friction=0.3)
    oblique = columns(cref.closure(sphere(), back, DOWN, f32(12.0), VOXEL, **SHORT), friction=0.3)
    print('square:', square, '\noblique:', oblique, '\nanalytic:', (w0, c0), (w1, c1))
    assert (square['finger_contact'] >= 0).all() and (oblique['finger_contact'] >= 0).all()
    assert abs(float(square['closed_width']) / VOXEL - w0) < 0.5 and abs(float(oblique['closed_width']) / VOXEL - w1) < 0.5
    assert np.abs(square['contact_cos'].astype(f64) - c0).max() < 2 * 0.00635
    assert np.abs(oblique['contact_cos'].astype(f64) - c1).max() < 2 * 0.0415
    assert oblique['grip_cos'] < square['grip_cos'] - 0.1
    assert square['grip_cos'] == square['contact_cos'].min() and oblique['grip_cos'] == oblique['contact_cos'].min()
    # a friction coefficient of 0.3 is a cone of 16.7 degrees: cos 0.958
    assert square['force_closure'] and not oblique['force_closure'] and square['held'] and oblique['held']
    assert 'force_closure' not in columns(cref.closure(sphere(), centre, DOWN, f32(12.0), VOXEL, **SHORT))
    # each finger travelled from 6 voxels to the chord's half
    assert np.abs(square['finger_travel'].astype(f64) / VOXEL - (6.0 - 0.5 * w0)).max() < 0.25
    assert abs(float(square['closed_width']) - (12.0 * VOXEL - float(square['finger_travel'].astype(f64).sum()))) < 1e-8


def test_empty_space_and_a_hand_that_starts_inside():
    empty = np.ones((R40,) * 3, f32)
    travel, cosine, contact, closed = cref.closure(empty, CENTRE, DOWN, f32(8.0), VOXEL)
    hw = 0.5 * href.opening_of(f32(8.0), R40, VOXEL)
    assert same(travel, f32([hw, hw])) and list(contact) == [-1, -1] and same(cosine, f32([0.0, 0.0])) and closed == 0.0
    assert not columns((travel, cosine, contact, closed))['held']
    # wholly outside the lattice: the same
    out = cref.closure(sphere(), np.array([-30.0, 5.0, 5.0]), DOWN, f32(8.0), VOXEL)
    assert same(out[0], f32([hw, hw])) and list(out[2]) == [-1, -1] and out[3] == 0.0
    # a solid: every pad starts inside, the first ray wins, the hand stays as wide as it was
    solid = np.full((R40,) * 3, -0.5, f32)
    travel, cosine, contact, closed = cref.closure(solid, CENTRE, DOWN, f32(8.0), VOXEL)
    assert same(travel, f32([0.0, 0.0])) and list(contact) == [0, 0] and same(closed, f32(href.opening_of(f32(8.0), R40, VOXEL)))
    # fingers that start inside the sphere: contact, no travel
    travel, _, contact, closed = cref.closure(sphere(), CENTRE, DOWN, f32(6.0), VOXEL, **SHORT)
    assert same(travel, f32([0.0, 0.0])) and (contact != -1).all() and same(closed, f32(href.opening_of(f32(6.0), R40, VOXEL)))
    # an opening of zero, a NaN and a negative width: every sample coincides, nothing is divided by zero
    for w in (f32(0.0), f32(np.nan), f32(-2.0)):
        out = cref.closure(sphere(), CENTRE + [0.0, 9.0, 0.0], DOWN, w, VOXEL)
        assert same(out[0], f32([0.0, 0.0])) and list(out[2]) == [-1, -1] and out[3] == 0.0
        out = cref.closure(sphere(), CENTRE, DOWN, w, VOXEL)
        assert same(out[0], f32([0.0, 0.0])) and list(out[2]) == [0, 0] and out[3] == 0.0
    # one finger only: held needs both
    one = columns(cref.closure(sphere(), CENTRE + [0.0, 5.5, 0.0], DOWN, f32(12.0), VOXEL, **SHORT))
    assert sorted(one['finger_contact'] >= 0) == [False, True] and not one['held'] and one['grip_cos'] == 0.0
    # check_success's threshold: the closed hand must stay wider than a tenth of max_opening
    rows = dict(travel=np.zeros((3, 2), f32), cosine=np.ones((3, 2), f32), contact=np.zeros((3, 2), np.int32), closed=f32([0.008, 0.0081, 0.05]))
    assert list(hand.closure_from_rows(rows)['held']) == [False, True, True]
    assert list(hand.closure_from_rows(rows, max_opening=0.6)['held']) == [False, False, False]
    none = hand.closure_from_rows({k: v[:0] for k, v in rows.items()}, friction=0.5)
    assert all(len(v) == 0 for v in none.values()) and none['grip_cos'].dtype == f32 and set(none) == set(KEYS) | {'force_closure'}


def test_halving_the_spacing():
    """Halving `spacing` moves the closed width of the sphere grasps by less than the coarser cell."""
    for pos, _, _ in sphere_grasps():
        for s in (1.0, 0.5):
            coarse = cref.closure(sphere(), pos, DOWN, f32(12.0), VOXEL, spacing=s, **SHORT)[3]
            fine = cref.closure(sphere(), pos, DOWN, f32(12.0), VOXEL, spacing=0.5 * s, **SHORT)[3]
            print(pos, s, coarse / VOXEL, fine / VOXEL)
            assert abs(float(fine) - float(coarse)) < s * VOXEL


def test_read_counts():
    assert cref.pads(VOXEL)[2:] == (3, 15) and cref.steps(0.035, VOXEL)[0] == 10 and cref.steps(0.0, VOXEL) == (1, 0.0)
    assert cref.reads(0.07, VOXEL) == 2 * 45 * (10 + 1 + 4 + 2)
    assert cref.DEFAULTS == hand.CLOSURE_DEFAULTS


# ---- 2. the C ABI's refusals, before the device (no GPU) --------------------------------------------------------------------------------------
def test_refusals_before_the_device():
    """Fake pointers: every call is one that validation refuses, with the clearance's codes and texts under this entry point's name."""
    L = _lib.lib()
    one = C.c_void_p(16)
    fn = 'gnr_finger_closure_fwd'
    text = lambda: L.gnr_last_error().decode()
    names = ('vol', 'pos', 'quat', 'width', 'count', 'travel', 'cosine', 'contact', 'closed')

    def call(p=None, level=0.0, bisections=4, stride=1, B=1, R=40, max_n=4, top_k=0, **kw):
        ptr = {k: kw.pop(k, one) for k in names}
        p = _lib.GnrHandParams(**{**hand.checked_hand(), 'scale': VOXEL, **kw}) if p is None else p
        return L.gnr_finger_closure_fwd(C.byref(p) if p is not False else None, level, bisections, ptr['vol'], ptr['pos'], ptr['quat'], ptr['width'],
                                        ptr['count'], stride, B, R, max_n, top_k, ptr['travel'], ptr['cosine'], ptr['contact'], ptr['closed'], None)

    for name in names:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for B in (0, -1, 65536):
        assert call(B=B) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', B
    for R in (1, 0, 257):
        assert call(R=R) == _lib.GNR_ERR_SHAPE and 'R must be in 2..256' in text(), R
    for n in (0, -1):
        assert call(max_n=n) == _lib.GNR_ERR_SHAPE and 'max_n must be >= 1' in text(), n
    assert call(stride=0) == _lib.GNR_ERR_ARG and 'count_stride must be >= 1' in text()
    assert call(top_k=-1) == _lib.GNR_ERR_ARG and 'top_k must be >= 0' in text()
    nan, inf = float('nan'), float('inf')
    for key in ('height', 'finger_width', 'tail_length', 'depth', 'spacing', 'scale'):
        for bad in (0.0, -1.0, nan, inf):
            assert call(**{key: bad}) == _lib.GNR_ERR_ARG and 'must be finite and > 0' in text() and fn in text(), (key, bad)
    for bad in (-1e-9, nan, inf):
        assert call(approach=bad) == _lib.GNR_ERR_ARG and 'approach must be finite and >= 0' in text(), bad
    for bad in (nan, inf, -inf):
        assert call(opening=bad) == _lib.GNR_ERR_ARG and 'opening must be finite' in text(), bad
        assert call(level=bad) == _lib.GNR_ERR_ARG and text() == fn + ': level must be finite', bad
    for bad in (-1, 17):
        assert call(bisections=bad) == _lib.GNR_ERR_ARG and text() == fn + ': bisections must be in 0..16', bad
    # the cap on a grasp's volume reads, counted for the widest opening (R voxels)
    for kw in (dict(spacing=1e-3), dict(R=256, spacing=0.004), dict(height=1.0, depth=1.0)):
        assert call(**kw) == _lib.GNR_ERR_ARG and 'GNR_HAND_MAX_SAMPLES' in text() and str(_lib.GNR_HAND_MAX_SAMPLES) in text(), kw
    assert cref.reads(256 * VOXEL, VOXEL, 16) <= _lib.GNR_HAND_MAX_SAMPLES < cref.reads(256 * VOXEL, VOXEL, spacing=0.004)


def test_finger_closure_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        hand.FingerClosure()


# ---- 3. keyword checks (no GPU) -------------------------------------------------------------------------------------------------------------------
def test_keyword_checks():
    from graspnerf_amd import planner
    from graspnerf_amd.grasp_post import GRASP_UTILS_PROCESS
    from graspnerf_amd.planner_session import PlannerSession
    frames, cams = [np.zeros((8, 8, 3), np.uint8)] * 4, [np.eye(4)] * 4
    with pytest.raises(TypeError, match='unknown closure parameters'):
        planner.plan_real(None, frames, cams, np.eye(3), closure={'bogus': 1})
    with pytest.raises(TypeError, match='unknown closure parameters'):
        planner.real_session(None, 4, (8, 8), (32, 32), closure={'iso': 0.0})
    with pytest.raises(ValueError, match='depth must be finite and > 0'):
        planner.plan_real(None, frames, cams, np.eye(3), closure=dict(depth=0.0))
    with pytest.raises(ValueError, match='level must be finite'):
        planner.real_session(None, 4, (8, 8), (32, 32), closure=dict(level=float('nan')))
    for bad in (-1, 17, 2.5):
        with pytest.raises(ValueError, match='bisections must be an integer in 0..16'):
            hand.closure_params(dict(bisections=bad))
    with pytest.raises(ValueError, match='max_opening must be finite and > 0'):
        hand.closure_params(dict(max_opening=0.0))
    with pytest.raises(ValueError, match='friction must be None or finite and >= 0'):
        hand.closure_params(dict(friction=-0.1))
    with pytest.raises(ValueError, match='opening must be None'):
        hand.closure_params(dict(opening=float('nan')))
    assert hand.closure_params(False) is None and hand.closure_params(None) is None
    want = dict(height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, opening=None, spacing=0.5, approach=0.05, level=0.0, bisections=4,
                max_opening=0.08, friction=None)
    assert hand.closure_params(True) == want and hand.closure_params({}) == want
    sig = inspect.signature(hand.FingerClosure.__call__).parameters
    assert {k: p.default for k, p in sig.items() if k in hand.CLOSURE_DEFAULTS} == hand.CLOSURE_DEFAULTS and sig['top_k'].default is None
    assert {k: p.default for k, p in inspect.signature(hand.closure_from_rows).parameters.items() if k != 'rows'} == hand.CLOSURE_PLAN_DEFAULTS
    p = hand.closure_params(dict(opening=hand.EXECUTE_GRASP_OPENING, spacing=1, bisections=2, friction=1, filter=True), filter=False)
    assert p == dict(want, opening=0.08, spacing=1.0, bisections=2, friction=1.0, filter=True) and isinstance(p['spacing'], float)
    assert grasp_post.same_params(p, {k: v for k, v in p.items() if k != 'filter'}) and not grasp_post.same_params(p, hand.closure_params(True))
    assert not grasp_post.same_params(p, None) and grasp_post.same_params(None, None)
    assert set(grasp_post.picked(p, hand.CLOSURE_DEFAULTS)) == set(hand.CLOSURE_DEFAULTS) and set(grasp_post.picked(p, hand.CLOSURE_PLAN_DEFAULTS)) == {'max_opening', 'friction'}
    for fn, name, default in ((planner.plan_real, 'closure', False), (planner.real_session, 'closure', False),
                              (PlannerSession.__init__, 'finger_closure', None)):
        assert inspect.signature(fn).parameters[name].default is default, fn
    # a session built without the switch and asked for it, and the other way round
    net = object()
    built = lambda fc: types.SimpleNamespace(net=net, selector_params=dict(GRASP_UTILS_PROCESS, order='index', top_k=None), surface_params=dict(rg=(-0.2, 0.2)),
                                             voxel_size=planner.REAL_VOXEL_SIZE, surface_normals=False, mesh_params=None, volume_depth_params=None,
                                             view_color_params=None, hand_params=None, closure_params=hand.closure_params(fc))
    for have, ask in ((False, True), (True, False), (True, dict(level=0.1)), (dict(friction=0.5), True)):
        with pytest.raises(ValueError, match=r'the session was built for another closure \(build it with planner.real_session'):
            planner.plan_real(net, frames, cams, np.eye(3), session=built(have), closure=ask)


def test_hand_mesh_with_stopped_fingers():
    """hand_mesh(travel=...) draws each finger where it stopped; without it the vertices are today's."""
    g = dict(pos=np.array([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1]]), quat=np.array([[0.0, 0.0, 0.0, 1.0], [0.3, -0.5, 0.2, 0.7]]), width=np.array([0.05, 0.07]),
             score=np.array([0.75, 0.25]))
    open_ = grasp_post.hand_mesh(g)
    assert same(grasp_post.hand_mesh(g, travel=None)['vertices'], open_['vertices'])
    travel = np.array([[0.01, 0.015], [0.0, 0.02]])
    shut = grasp_post.hand_mesh(g, travel=travel)
    assert same(shut['faces'], open_['faces']) and same(shut['colors'], open_['colors'])
    from graspnerf_amd.tsdf import rotation_matrix
    for k in range(2):
        q = g['quat'][k] / np.linalg.norm(g['quat'][k])
        local = lambda m: (m['vertices'][32 * k:32 * k + 32] - g['pos'][k]) @ rotation_matrix(q)
        moved = local(shut) - local(open_)
        want = np.zeros((32, 3))
        want[:8, 1], want[8:16, 1] = travel[k, 0], -travel[k, 1]               # the left finger towards +y, the right one towards -y
        np.testing.assert_allclose(moved, want, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='travel'):
        grasp_post.hand_mesh(g, travel=travel[:1])


# ---- GPU: the bits of the statement ----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5a
TYPES = ((2, torch.float32, f32), (2, torch.float32, f32), (2, torch.int32, np.int32), (1, torch.float32, f32))


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _raw(vol, pos, quat, width, count, scale, top_k=None, level=0.0, bisections=4, **kw):
    """The C call on outputs filled with a sentinel byte, with one more row behind [B,max_n] that the call is not told about
    -> (travel, cosine, contact [B,max_n,2], closed [B,max_n]) as numpy, and whether the spare rows kept the sentinel."""
    L = _lib.lib()
    B, R, n = vol.shape[0], vol.shape[-1], pos.shape[1]
    count = np.ascontiguousarray(count, np.int32)
    dev = [_up(a) for a in (np.asarray(vol, f32), np.asarray(pos, f64), np.asarray(quat, f32), np.asarray(width, f32), count)]
    outs = [torch.full(((B * n + 1) * c * 4,), SENTINEL, dtype=torch.uint8, device='cuda:0').view(t) for c, t, _ in TYPES]
    p = _lib.GnrHandParams(scale=float(scale), **hand.checked_hand(**kw))
    rc = L.gnr_finger_closure_fwd(C.byref(p), float(level), int(bisections), *(t.data_ptr() for t in dev), count.size // B, B, R, n, int(top_k or 0),
                                  *(t.data_ptr() for t in outs), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'gnr_finger_closure_fwd')
    torch.cuda.synchronize()
    outs = [t.cpu().numpy() for t in outs]
    spare = all(bool((t[c * B * n:].view(np.uint8) == SENTINEL).all()) for t, (c, _, _) in zip(outs, TYPES))
    return tuple(t[:c * B * n].reshape((B, n, 2) if c == 2 else (B, n)) for t, (c, _, _) in zip(outs, TYPES)), spare


def _want(vol, pos, quat, width, count, scale, top_k=None, **kw):
    """The statement on the same sentinel-filled outputs, scene by scene."""
    B, n = pos.shape[:2]
    out = []
    for b in range(B):
        o = tuple(np.full(4 * c * n, SENTINEL, np.uint8).view(t).reshape((n, 2) if c == 2 else (n,)) for c, _, t in TYPES)
        out.append(cref.closure_rows(vol[b], pos[b], quat[b], width[b], np.asarray(count).reshape(B, -1)[b, 0], scale, top_k=top_k, out=o, **kw))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def _check(what, vol, pos, quat, width, count, scale, top_k=None, **kw):
    got, spare = _raw(vol, pos, quat, width, count, scale, top_k, **kw)
    want = _want(vol, pos, quat, width, count, scale, top_k, **kw)
    assert spare, (what, 'written beyond [B,max_n]')
    for name, g, w in zip(hand.CLOSURE_ROWS, got, want):
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert same(g, w), (what, name, len(bad), bad[:3], [g[tuple(i)] for i in bad[:3]], [w[tuple(i)] for i in bad[:3]])
    return want


@pytest.mark.gpu
def test_small_volume_and_contents_that_are_no_numbers():
    """R = 3, B = 2: poses inside, partly and wholly outside the lattice, widths 0, negative, NaN and above R, quaternions that are zero or
    NaN, positions that are NaN or huge; counts 0, negative and above max_n, a top_k; the rows beyond keep their sentinel."""
    R, scale = 3, 0.02                                                         # pads of 2.5 voxels in a lattice of 2
    rng = np.random.default_rng(5)
    vol = rng.uniform(-1, 1, (2, R, R, R)).astype(f32)
    vol[1] = np.clip(vol[1] + 0.6, -1, 1)                                      # mostly free: fingers travel before they stop
    pos = np.array([[1.0, 1.0, 1.0], [0.7, 1.2, 0.4], [1.0, 1.0, -1.0], [1.0, 3.5, 1.0], [9.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0],
                    [1.0, 1.0, 1.0], [1.0, 1.0, 0.5], [np.nan, 1.0, 1.0], [1e300, -1e300, 1.0], [1.0, 1.0, 1.0]])
    quat = f32([[0, 0, 0, 1], [0.3, -0.5, 0.2, 0.7], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0], [np.nan, 0, 0, 1], [0.1, 0.9, 0, 0.2],
                [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0.5, 0.5, 0.5, -0.5]])
    width = f32([2.0, 1.5, 2.0, 4.0, 2.0, 2.0, 2.0, 0.0, -4.0, 2.0, 2.0, np.nan])
    n = len(pos)
    pos, quat, width = (np.stack([a, np.roll(a, 5, 0)]) for a in (pos, quat, width))
    width[1, :3] = (1e30, 3.5, 1.0)
    want = _check('R = 3', vol, pos, quat, width, [n, n], scale)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[3]).all()
    assert list(want[2][0, 4]) == [-1, -1] and want[3][0, 4] == 0.0, 'a hand wholly outside touches nothing'
    assert (want[2][:, :, 0] >= 0).sum() > 4 and (want[2][:, :, 0] < 0).sum() > 4 and (want[0] > 0).sum() > 4
    for count, top_k, rows in (([0, n + 7], None, (0, n)), ([-3, 5], 2, (0, 2)), ([3, 1], 2, (2, 1)), ([n, n], n + 9, (n, n))):
        want = _check((count, top_k), vol, pos, quat, width, count, scale, top_k=top_k)
        for b in range(2):
            assert (want[0][b, rows[b]:].view(np.uint8) == SENTINEL).all() and (want[3][b, rows[b]:].view(np.uint8) == SENTINEL).all(), (count, top_k, b)
            assert not (want[3][b, :rows[b]].view(np.uint32) == 0x5a5a5a5a).any(), (count, top_k, b)
    _check('stride 2', vol, pos, quat, width, [[2, 99], [3, 99]], scale)
    _check('one opening, a real hand, another level', vol, pos, quat, width, [n, n], scale, opening=0.05, height=0.02, finger_width=0.01, spacing=0.7,
           level=0.25, bisections=2)
    _check('R = 2', vol[:, :2, :2, :2].copy(), pos * 0.5, quat, width, [n, n], 0.05)


LANES = (('24 pairs: 40 idle lanes', dict(height=0.008, depth=0.045), 24), ('64 pairs: one each', dict(height=0.008, depth=0.145), 64),
         ('66 pairs: two lanes do a second round', dict(height=0.015, depth=0.095), 66))


@pytest.mark.gpu
def test_lanes_and_ordinals():
    """R = 12: fewer (finger, ray) pairs than lanes, exactly 64, and the first count above 64 (the count is even: 66); a slab across the
    closing direction, where every ray of a finger has the same t* and ordinal 0 must win; bisections 0 and 16."""
    R, scale = 12, 0.01
    rng = np.random.default_rng(17)
    x = np.arange(R, dtype=f64)
    X = np.stack(np.meshgrid(x, x, x, indexing='ij'), -1)
    blob = np.clip((np.linalg.norm(X - [5.3, 5.8, 6.1], axis=-1) - 2.6) / 2.0, -1, 1).astype(f32)
    pos = rng.uniform(3.0, 8.0, (1, 6, 3))
    quat = rng.normal(size=(1, 6, 4)).astype(f32)
    width = rng.uniform(5.0, 11.0, (1, 6)).astype(f32)
    for what, kw, pairs in LANES:
        _, _, nx, nz = cref.pads(scale, kw['height'], kw['depth'], 1.0)
        assert 2 * nx * nz == pairs, what
        want = _check(what, blob[None], pos, quat, width, [6], scale, spacing=1.0, **kw)
        assert (want[2] >= 0).any(), what
    # the slab 4 <= y <= 7 seen by a hand whose closing direction is the lattice's y: p_y is l_y to the bit in every ray
    slab = np.broadcast_to(np.clip((np.abs(x - 5.5) - 1.5) / 2.0, -1, 1).astype(f32)[None, :, None], (R, R, R)).copy()
    for what, kw, _ in LANES:
        want = _check(('slab', what), slab[None], np.array([[[5.5, 5.5, 3.0]]]), f32([[[0, 0, 0, 1]]]), f32([[8.0]]), [1], scale, spacing=1.0, **kw)
        assert list(want[2][0, 0]) == [0, 0] and abs(float(want[3][0, 0]) / scale - 3.0) < 1e-6, what
        d = {}
        cref.closure(slab, np.array([5.5, 5.5, 3.0]), f32([0, 0, 0, 1]), f32(8.0), scale, spacing=1.0, details=d, **kw)
        inside = d['t'][~np.isnan(d['t'])]
        assert len(inside) > 8 and (inside == inside[0]).all(), 'the rays inside the lattice do not tie'
    for bis in (0, 16):
        _check(('bisections', bis), blob[None], pos, quat, width, [6], scale, bisections=bis)


@functools.lru_cache(maxsize=None)
def blobs():
    """A seeded volume of smooth blobs at R = 40: a sum of Gaussians against a threshold, clipped like a TSDF."""
    rng = np.random.default_rng(23)
    x = np.arange(R40, dtype=f64)
    X = np.stack(np.meshgrid(x, x, x, indexing='ij'), -1)
    field = sum(np.exp(-((X - c) ** 2).sum(-1) / (2.0 * s * s)) for c, s in zip(rng.uniform(4, 35, (24, 3)), rng.uniform(3.0, 6.0, 24)))
    vol = np.clip(0.6 - field, -1, 1).astype(f32)
    vol.setflags(write=False)
    return vol


@pytest.mark.gpu
def test_random_grasps_equal_the_statement():
    """B = 2 (the sphere, the blobs), 100 and 73 of 100 seeded grasps each: positions partly outside the box, unnormalised quaternions,
    per-row widths and one opening; and hand.FingerClosure on the same rows gives the same bits into buffers it keeps."""
    vol = np.stack([sphere(), blobs()])
    rng = np.random.default_rng(41)
    pos = rng.uniform(-3.0, R40 + 2.0, (2, 100, 3))
    pos[0, :60] = CENTRE + rng.normal(size=(60, 3)) * 3.0                       # most of the sphere's grasps near the sphere
    pos[1, :60] = rng.uniform(6.0, 33.0, (60, 3))                               # most of the blobs' grasps among the blobs
    quat = (rng.normal(size=(2, 100, 4)) * rng.uniform(0.1, 10.0, (2, 100, 1))).astype(f32)
    width = rng.uniform(1.33, 14.0, (2, 100)).astype(f32)
    count = [100, 73]
    want = _check('own widths', vol, pos, quat, width, count, VOXEL)
    for b, n in enumerate(count):
        hit = (want[2][b, :n] >= 0)
        print('scene', b, 'fingers with a contact:', hit.sum(), 'of', 2 * n, ' moved before it:', (hit & (want[0][b, :n] > 0)).sum())
        assert hit.sum() > 20 and (~hit).sum() > 20 and (hit & (want[0][b, :n] > 0)).sum() > 10
    _check('one opening', vol, pos, quat, width, count, VOXEL, opening=0.06, spacing=0.8, height=0.02, level=0.1)
    op = hand.FingerClosure()
    n_dev = torch.tensor(count, dtype=torch.int32, device='cuda:0')
    a = op(vol, pos, quat, width, n_dev, scale=VOXEL)
    ptrs = {k: v.data_ptr() for k, v in a.items()}
    host = {k: v.cpu().numpy() for k, v in a.items()}
    assert tuple(host) == hand.CLOSURE_ROWS
    for b, n in enumerate(count):
        assert all(same(host[k][b, :n], w[b, :n]) for k, w in zip(hand.CLOSURE_ROWS, want))
    b_ = op(vol, pos, quat, width, n_dev, scale=VOXEL, top_k=300)
    assert {k: v.data_ptr() for k, v in b_.items()} == ptrs and all(same(b_[k].cpu().numpy(), host[k]) for k in host)
    with pytest.raises(ValueError, match='pos must be'):
        op(vol, pos[:, :, :2], quat, width, n_dev, scale=VOXEL)
    with pytest.raises(ValueError, match='count must be'):
        op(vol, pos, quat, width, count, scale=VOXEL)
    with pytest.raises(ValueError, match='bisections must be'):
        op(vol, pos, quat, width, n_dev, scale=VOXEL, bisections=17)
    with pytest.raises(_lib.GnrError, match='GNR_HAND_MAX_SAMPLES'):
        op(vol, pos, quat, width, n_dev, scale=VOXEL, spacing=1e-3)


def _eager(vol, sel, n, level, **kw):
    """hand.FingerClosure on the volume and the (host) selection a plan returned -> the plan's columns in the selection's order."""
    up = {k: _up(sel[k].numpy() if torch.is_tensor(sel[k]) else sel[k]) for k in ('count', 'index', 'quat', 'width')}
    res = hand.FingerClosure().of_selection(_up(vol), dict(up, top_k=sel.get('top_k')), scale=0.3 / 40, level=level)
    return hand.closure_from_rows({k: v.cpu().numpy() for k, v in hand.closure_rows(res, 0, n).items()}, **kw)


@pytest.mark.gpu
def test_session_records_the_closure():
    """PlannerSession(finger_closure=...) at cfg1's size: every plan's columns equal the eager FingerClosure on the volume and the
    selection that plan returned (and the statement on its first rows); a replay of the first plan returns the first plan's bits; the
    columns go through the seeded permutation of the other columns; beside the clearance both sets of columns arrive.  The synthetic
    checkpoint's volume need not cross zero: the level is the median of a first plan's volume."""
    from graspnerf_amd import planner
    from graspnerf_amd.planner_session import PlannerSession
    from test_planner_session import CFG, IMG_WH, MAX_GRASPS, PARAMS, SEED, SRC_HW, V, _scene, _state_dict
    net = planner.load_model(dict(CFG), {'network_state_dict': _state_dict(width_bias=5.0)})
    plain = PlannerSession(net, V, SRC_HW, IMG_WH, max_grasps=MAX_GRASPS, **PARAMS)
    A, B = _scene(1), _scene(2, radius=0.55, theta=np.pi / 3.4)
    plan = lambda ses, sc, seed: ses.plan(sc['frames'], sc['poses'], sc['Ks'], sc['depth_range'], sc['bbox3d'], seed=seed, return_volumes=True)[0]
    p0 = plan(plain, A, None)
    level = float(np.median(p0['volumes'][0]))
    s = PlannerSession(net, V, SRC_HW, IMG_WH, max_grasps=MAX_GRASPS, finger_closure=dict(level=level, friction=0.5), **PARAMS)
    assert s._d_out.numel() == plain._d_out.numel() and [p.out for p in s.products] == ['closure'] and plain.products == []
    keys = KEYS + ('force_closure',)
    first = None
    for what, sc in (('A', A), ('B', B), ('A again', A)):
        g = plan(s, sc, None)
        n = len(g['score'])
        assert 1 <= n < MAX_GRASPS and all(len(g[k]) == n for k in keys)
        want = _eager(g['volumes'][0], s.selection, n, level, friction=0.5)
        for k in keys:
            assert same(g[k], want[k]), (what, k)
        assert g['closed_width'].dtype == f32 and g['finger_contact'].shape == (n, 2) and g['held'].dtype == bool
        print(what, n, 'grasps,', int(g['held'].sum()), 'held,', int((g['finger_contact'] >= 0).sum()), 'finger contacts')
        vol = g['volumes'][0].reshape(40, 40, 40)
        for r in range(min(n, 8)):
            t, c, o, w = cref.closure(vol, g['index'][r].astype(f64), s.selection['quat'][0, r].numpy(), s.selection['width'][0, r].numpy(), 0.3 / 40,
                                      level=level)
            assert same(g['finger_travel'][r], t) and same(g['contact_cos'][r], c) and same(g['finger_contact'][r], o) and same(g['closed_width'][r], w), \
                (what, r)
        if first is None:
            first = g
            for k in ('index', 'pos', 'quat', 'width', 'score'):
                assert same(g[k], p0[k]), ('the other columns do not depend on the product', k)
            assert set(g) == set(p0) | set(keys)
        elif what == 'A again':
            assert all(same(g[k], first[k]) for k in keys + ('index', 'score'))
    assert s.captures == 1
    seeded = plan(s, A, SEED)
    np.random.seed(SEED)
    perm = np.random.permutation(len(first['score']))
    for k in keys + ('index', 'score'):
        assert same(seeded[k], first[k][perm]), k
    # beside the clearance: both products, the clearance first, each with its own columns
    both = PlannerSession(net, V, SRC_HW, IMG_WH, max_grasps=MAX_GRASPS, hand_clearance={}, finger_closure=dict(level=level, friction=0.5), **PARAMS)
    assert [p.out for p in both.products] == ['hand', 'closure']
    g = plan(both, A, SEED)
    assert all(same(g[k], seeded[k]) for k in keys + ('index', 'score')) and len(g['collision_free']) == len(g['score'])


@pytest.mark.gpu
def test_plan_real_with_closure_eager_and_session():
    """plan_real(closure=...) with and without session= agree bit for bit, every other key is what it is without the option -- also through
    a session -- and filter=True returns exactly the held rows in their order; with the clearance's filter too, the rows that pass both."""
    from graspnerf_amd import planner
    from test_planner_session import CFG, _state_dict
    from test_planner_session_real import HW, TOP_K, V, _frames
    from graspnerf_amd.synth import ring_cameras
    net = planner.load_model(dict(CFG), {'network_state_dict': _state_dict(width_bias=5.0)})
    K = np.float32([[0.7 * HW[1], 0, 0.5 * HW[1]], [0, 0.7 * HW[1], 0.5 * HW[0]], [0, 0, 1]])
    cam = dict(extrinsics=list(ring_cameras(V)), intrinsic=K)
    A = _frames(1)
    kw = dict(order='score', top_k=TOP_K)
    off = planner.plan_real(net, A, **cam, **kw)
    on = planner.plan_real(net, A, **cam, **kw, closure=True)
    assert set(on[0]) == set(off[0]) | set(KEYS) and set(on[3]) == set(off[3])
    for k in off[0]:
        assert same(on[0][k], off[0][k]), k
    assert same(on[1], off[1]) and same(on[2], off[2]) and all(same(on[3][k], off[3][k]) for k in off[3])
    # without the switch a session returns what plan_real() returns, and no new key
    plain = planner.real_session(net, V, HW, HW[::-1], **kw)
    off_s = planner.plan_real(net, A, **cam, **kw, session=plain)
    assert set(off_s[0]) == set(off[0]) and all(same(off_s[0][k], off[0][k]) for k in off[0]) and same(off_s[1], off[1]) and same(off_s[2], off[2])
    n = len(on[0]['score'])
    assert n == TOP_K
    ask = dict(level=float(np.median(on[2])), opening=hand.EXECUTE_GRASP_OPENING, friction=0.5)
    eager = planner.plan_real(net, A, **cam, **kw, closure=ask)
    sess = planner.real_session(net, V, HW, HW[::-1], **kw, closure=ask)
    got = planner.plan_real(net, A, **cam, **kw, closure=ask, session=sess)
    assert set(eager[0]) == set(off[0]) | set(KEYS) | {'force_closure'}
    for k in eager[0]:
        assert same(got[0][k], eager[0][k]), k
    held = eager[0]['held']
    print(f'{held.sum()} of {n} grasps are held at the level {ask["level"]:.4f}; closed widths', eager[0]['closed_width'])
    assert np.array_equal(held, (eager[0]['finger_contact'] >= 0).all(1) & (eager[0]['closed_width'] > f32(0.008)))
    for route in (dict(), dict(session=sess)):
        kept = planner.plan_real(net, A, **cam, **kw, closure=dict(ask, filter=True), **route)
        assert kept[0]['held'].all() and len(kept[1]) == held.sum()
        for k in eager[0]:
            assert same(kept[0][k], eager[0][k][held]), (sorted(route), k)
        assert same(kept[1], eager[1][held])
    # both filters: a row must pass both
    clear = dict(level=float(np.median(planner.plan_real(net, A, **cam, **kw, clearance=True)[0]['approach_clearance'])))
    both = planner.plan_real(net, A, **cam, **kw, closure=ask, clearance=clear)
    mask = both[0]['held'] & both[0]['collision_free']
    kept = planner.plan_real(net, A, **cam, **kw, closure=dict(ask, filter=True), clearance=dict(clear, filter=True))
    print(f'{both[0]["collision_free"].sum()} collision free, {mask.sum()} both')
    assert all(same(kept[0][k], both[0][k][mask]) for k in both[0]) and same(both[0]['held'], held)
    # order='permuted': the new columns go through the permutation of the other columns
    a = planner.plan_real(net, A, **cam, seed=5, closure=True)
    b = planner.plan_real(net, A, **cam, seed=5)
    assert same(a[0]['index'], b[0]['index']) and len(a[0]['closed_width']) == len(b[0]['score'])
    with pytest.raises(ValueError, match='another closure'):
        planner.plan_real(net, A, **cam, **kw, session=sess)
    with pytest.raises(ValueError, match='another closure'):
        planner.plan_real(net, A, **cam, **kw, session=sess, closure=True)
