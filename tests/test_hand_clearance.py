"""Gripper clearance of the ranked grasps against the volume (csrc/gnr_hand.hip, hand.HandClearance, PlannerSession(hand_clearance=...),
plan_real(clearance=True)) and the gripper mesh (grasp_post.hand_mesh).  tests/hand_reference.py is the statement in numpy float64; the
device's rows are compared with it by np.array_equal on the bits.  Without a GPU: the statement on analytic scenes (a hand that fits,
one that does not, an obstacle that only the approach meets), its invariants, the sample counts, the mesh, the refusals made before the
device is touched, and the keyword checks."""
import ctypes as C
import functools
import inspect
import types

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, grasp_post, hand
from graspnerf_amd.tsdf import rotation_matrix
import hand_reference as ref
import tsdf_reference as tref
from test_surface_color import spheres40
from test_surface_mesh import same

f32, f64 = np.float32, np.float64
R40 = 40
VOXEL = tref.SIZE / R40
ORIGIN = np.asarray(tref.ORIGIN, f64) + 0.5 * VOXEL                             # world position of voxel (0,0,0)'s value (spheres40's lattice)
DOWN = f32([1.0, 0.0, 0.0, 0.0])                                               # top-down: the fingers point along world -z
F = ref.DEFAULTS['finger_width']


def lattice_pos(world):
    return (np.asarray(world, f64) - ORIGIN) / VOXEL


def sphere_volume(centre, radius, trunc=4):
    """A TSDF [40,40,40] of one sphere on spheres40's lattice, truncated at `trunc` voxels."""
    x = np.arange(R40, dtype=f64) * VOXEL
    X = np.stack(np.meshgrid(x + ORIGIN[0], x + ORIGIN[1], x + ORIGIN[2], indexing='ij'), -1)
    return np.clip((np.linalg.norm(X - np.asarray(centre, f64), axis=-1) - radius) / (trunc * VOXEL), -1.0, 1.0).astype(f32)


@functools.lru_cache(maxsize=None)
def analytic():
    """The five analytic grasps of the module: (vol, pos, quat, width in voxels) each, never written to."""
    vol = spheres40()['vol']
    small = np.asarray(tref.SPHERES[1][0], f64)
    above = lattice_pos(small + [0.0, 0.0, 0.045])
    g = np.array([0.0, 0.0, 0.08])
    M = ref.matrix(DOWN)
    behind = lambda back: sphere_volume(g + M @ np.array([0.0, 0.07 / 2 + F / 2, -back]), 0.015)
    return (('fits', vol, above, DOWN, f32(0.07 / VOXEL)), ('fingers in the sphere', vol, above, DOWN, f32(0.05 / VOXEL)),
            ('obstacle 5 cm behind the finger', behind(0.05), lattice_pos(g), DOWN, f32(0.07 / VOXEL)),
            ('obstacle 10 cm behind the finger', behind(0.10), lattice_pos(g), DOWN, f32(0.07 / VOXEL)),
            ('top of the box', vol, lattice_pos([0.0, 0.0, 0.24]), DOWN, f32(0.07 / VOXEL)))


# ---- 1. the statement on analytic scenes (no GPU) ------------------------------------------------------------------------------------------
def test_sample_counts_of_the_default_hand():
    assert ref.totals(0.07, VOXEL) == (576, 2454)
    assert ref.totals(0.07, VOXEL, approach=0.0) == (576, 576)
    local, box, iz = ref.samples(0.07, VOXEL)
    assert len(local) == 2454 and (iz >= 0).sum() == 576 and list(np.bincount(box)) == [270, 270, 1680, 234]
    # the samples at the grasp span exactly the four boxes of the hand model (hand_boxes: what hand_mesh draws)
    for k, (lo, hi) in enumerate(grasp_post.hand_boxes(0.07)):
        at = local[(box == k) & (iz >= 0)]
        np.testing.assert_allclose(at.min(0), lo, rtol=0, atol=1e-15)
        np.testing.assert_allclose(at.max(0), hi, rtol=0, atol=1e-15)
    # the approach continues every box's z lattice backwards over at least 5 cm, by less than one more step
    for k, (lo, step, n, m) in enumerate(ref.lattice(0.07, VOXEL)):
        back = lo[2] - local[box == k][:, 2].min()
        assert 0.05 <= back + 1e-15 and back < 0.05 + step[2]
        assert all(s <= 0.5 * VOXEL * (1 + 1e-12) for s in step), 'samples more than `spacing` voxels apart'


def test_a_hand_that_fits_and_one_that_does_not():
    (_, vol, pos, q, w_fit), (_, _, _, _, w_tight) = analytic()[:2]
    c, worst, inside = ref.clearance(vol, pos, q, w_fit, VOXEL)
    print('width 0.07:', c, worst, inside)
    assert 0.1 < c[0] < 0.25 and c[1] == c[0] and worst[0] == worst[1]         # a 5 mm gap of a TSDF truncated at 30 mm: about 1/6
    assert list(inside) == [576, 2454]
    c, worst, inside = ref.clearance(vol, pos, q, w_tight, VOXEL)
    print('width 0.05:', c, worst, inside)
    assert c[0] < 0.0 and c[1] <= c[0]
    _, box, _ = ref.samples(ref.opening_of(w_tight, R40, VOXEL), VOXEL)
    assert box[worst[0]] in (0, 1), 'the worst sample of a hand too narrow for the sphere is on a finger'


def test_the_sweep_is_there_and_ends():
    (_, vol5, pos, q, w), (_, vol10, _, _, _) = analytic()[2:4]
    c5 = ref.clearance(vol5, pos, q, w, VOXEL)[0]
    c10 = ref.clearance(vol10, pos, q, w, VOXEL)[0]
    print('obstacle 5 cm behind:', c5, ' 10 cm behind:', c10)
    assert c5[0] > 0.0 and c5[1] < 0.0, 'the obstacle is clear of the hand at the grasp and in the way of its approach'
    assert c10[0] > 0.0 and c10[1] > 0.0, 'an obstacle beyond the pre-grasp pose is in nobody\'s way'
    # without an approach nothing is swept
    c0 = ref.clearance(vol5, pos, q, w, VOXEL, approach=0.0)[0]
    assert c0[0] == c5[0] and c0[1] == c0[0]


def test_part_of_the_hand_outside_the_volume():
    _, vol, pos, q, w = analytic()[4]
    c, worst, inside = ref.clearance(vol, pos, q, w, VOXEL)
    assert list(inside) == [477, 537]                                          # 11 of the tail's 12 layers and most of the sweep are above the box


def _random_grasps(n, seed, lo=-4.0, hi=R40 + 3.0):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(lo, hi, (n, 3))
    quat = rng.normal(size=(n, 4)).astype(f32)
    width = rng.uniform(1.33, 9.33, n).astype(f32)
    return pos, quat, width


def test_invariants_over_random_poses():
    vol = spheres40()['vol']
    const = np.full((R40,) * 3, 0.25, f32)
    pos, quat, width = _random_grasps(40, 7)
    partly = 0
    for r in range(len(pos)):
        c, worst, inside = ref.clearance(vol, pos[r], quat[r], width[r], VOXEL)
        at, swept = ref.totals(ref.opening_of(width[r], R40, VOXEL), VOXEL)
        assert c[1] <= c[0] and inside[0] <= inside[1] and inside[0] <= at and inside[1] <= swept
        assert (worst[0] == -1) == (inside[0] == 0) and (worst[1] == -1) == (inside[1] == 0)
        partly += 0 < inside[1] < swept
        c0, w0, i0 = ref.clearance(vol, pos[r], quat[r], width[r], VOXEL, approach=0.0)
        assert c0[0] == c0[1] and w0[0] == w0[1] and i0[0] == i0[1] and same(c0[0], c[0]) and i0[0] == inside[0]
    assert partly > 5, 'no pose has part of its hand outside the volume'
    # a constant volume: the first sample wins (a grasp whose hand is wholly inside; the first sample at the grasp is the m-th)
    centre = np.full(3, 0.5 * (R40 - 1))
    for q in (DOWN, f32([0, 0, 0, 1]), f32([0.3, -0.5, 0.2, 0.7])):
        c, worst, inside = ref.clearance(const, centre, q, f32(6.0), VOXEL)
        m = ref.lattice(6.0 * VOXEL, VOXEL)[0][3]
        assert same(c, f32([0.25, 0.25])) and list(worst) == [m, 0] and list(inside) == list(ref.totals(6.0 * VOXEL, VOXEL))
        c, worst, _ = ref.clearance(const, centre, q, f32(6.0), VOXEL, approach=0.0)
        assert list(worst) == [0, 0]
    # a hand wholly outside
    for p in ([-30.0, 5.0, 5.0], [20.0, 20.0, 80.0]):
        c, worst, inside = ref.clearance(vol, np.array(p), DOWN, f32(6.0), VOXEL)
        assert same(c, f32([1.0, 1.0])) and list(worst) == [-1, -1] and list(inside) == [0, 0]
    # contents that are no numbers: finite, in-statement results
    for q, w in ((f32([np.nan, 0, 0, 1]), f32(5.0)), (f32([0, 0, 0, 0]), f32(5.0))):
        c, worst, inside = ref.clearance(vol, centre, q, w, VOXEL)
        assert np.isfinite(c).all()
    assert ref.opening_of(f32(np.nan), R40, VOXEL) == 0.0 and ref.opening_of(f32(1e30), R40, VOXEL) == R40 * VOXEL
    assert ref.opening_of(f32(-3.0), R40, VOXEL) == 0.0 and ref.opening_of(f32(5.0), R40, VOXEL, opening=0.08) == (0.08 / VOXEL) * VOXEL


def test_halving_the_spacing():
    """Every sample of the coarse lattice at the grasp has a sample of the fine lattice within half a fine step per axis of its box (both
    lattices span the same boxes), so within sqrt(3)/2 fine steps; a trilinear field changes by at most D per voxel along each axis (D:
    the largest difference between neighbouring voxels), so by at most sqrt(3) D per voxel of path.  A fine step is at most half the
    coarse spacing s: the fine minimum is at most 0.75 D s above the coarse one -- within the D s bound, for hands wholly inside the
    volume.  On the approach the coarse lattice may reach up to one coarse step further back than the fine one: the nearest fine sample
    is then within sqrt(s^2 + 2 (s/4)^2) voxels, and the bound is sqrt(3) sqrt(1.125) D s."""
    vol = spheres40()['vol']
    D = max(float(np.abs(np.diff(vol.astype(f64), axis=a)).max()) for a in range(3))
    pos, quat, width = _random_grasps(12, 11, lo=15.0, hi=24.0)                 # the hand and its sweep (within 14.4 voxels of the grasp) stay inside
    for s in (1.0, 0.5):
        for r in range(len(pos)):
            coarse, _, ci = ref.clearance(vol, pos[r], quat[r], width[r], VOXEL, spacing=s)
            fine, _, fi = ref.clearance(vol, pos[r], quat[r], width[r], VOXEL, spacing=0.5 * s)
            w = ref.opening_of(width[r], R40, VOXEL)
            assert list(ci) == list(ref.totals(w, VOXEL, spacing=s)) and list(fi) == list(ref.totals(w, VOXEL, spacing=0.5 * s)), 'not wholly inside'
            assert float(fine[0]) - float(coarse[0]) <= D * s, (s, r, fine, coarse)
            assert float(fine[1]) - float(coarse[1]) <= np.sqrt(3.0) * np.sqrt(1.125) * D * s, (s, r, fine, coarse)


# ---- 2. the gripper mesh (no GPU) --------------------------------------------------------------------------------------------------------------
def test_hand_mesh():
    rng = np.random.default_rng(3)
    n = 5
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    g = dict(pos=rng.uniform(0.05, 0.25, (n, 3)), quat=quat, width=rng.uniform(0.01, 0.07, n), score=rng.uniform(0, 1, n).astype(f32))
    m = grasp_post.hand_mesh(g)
    assert m['vertices'].shape == (32 * n, 3) and m['faces'].shape == (48 * n, 3) and m['colors'].shape == (32 * n, 3)
    assert m['faces'].dtype == np.int64 and m['vertices'].dtype == f64
    for k in range(n):
        f = m['faces'][48 * k:48 * k + 48]
        assert f.min() >= 32 * k and f.max() < 32 * k + 32, 'a face index outside its own grasp\'s rows'
        np.testing.assert_array_equal(m['colors'][32 * k:32 * k + 32], np.repeat([[f64(g['score'][k]), 0.0, 1.0 - f64(g['score'][k])]], 32, 0))
        # draw_gripper_o3d's corner arithmetic (its X is this z, its Z this -x; create_mesh_box spans [0, d] per axis before the shifts)
        w, h, fw, t, d = g['width'][k], 0.004, 0.004, 0.04, 0.05
        Rm = rotation_matrix(quat[k])
        spans = (((-fw, d), (-w / 2 - fw, -w / 2)), ((-fw, d), (w / 2, w / 2 + fw)), ((-fw, 0.0), (-w / 2, w / 2)), ((-t - fw, -fw), (-fw / 2, fw / 2)))
        for b, (zs, ys) in enumerate(spans):
            want = np.array([[x, y, z] for x in (-h / 2, h / 2) for y in ys for z in zs]) @ Rm.T + g['pos'][k]
            np.testing.assert_allclose(m['vertices'][32 * k + 8 * b:32 * k + 8 * b + 8], want, rtol=0, atol=1e-15)
        # every box is a closed surface wound outwards: each edge once in each direction, a positive volume
        for b in range(4):
            fb = f[12 * b:12 * b + 12]
            edges = {(int(a_), int(b_)) for tri in fb for a_, b_ in zip(tri, np.roll(tri, -1))}
            assert len(edges) == 36 and all((b_, a_) in edges for a_, b_ in edges)
            v = m['vertices']
            vol6 = sum(np.dot(v[i], np.cross(v[j], v[l])) for i, j, l in fb)
            ext = np.ptp((v[32 * k + 8 * b:32 * k + 8 * b + 8] - g['pos'][k]) @ Rm, axis=0)
            np.testing.assert_allclose(vol6 / 6.0, np.prod(ext), rtol=1e-6)
        # the mesh's bounding box in the grasp frame is that of the statement's samples at the grasp: one model, two uses (the samples'
        # far ends are lo + (n - 1) * (e / (n - 1)): equal to the corners to the last bits of 0.1 m)
        local, _, iz = ref.samples(w, VOXEL)
        mine = (m['vertices'][32 * k:32 * k + 32] - g['pos'][k]) @ Rm
        np.testing.assert_allclose(mine.min(0), local[iz >= 0].min(0), rtol=0, atol=1e-15)
        np.testing.assert_allclose(mine.max(0), local[iz >= 0].max(0), rtol=0, atol=1e-15)
    # one opening for every hand, other dimensions, explicit scores, and the keyword check
    m2 = grasp_post.hand_mesh(g, scores=np.ones(n), opening=0.08, height=0.02, finger_width=0.01)
    assert np.array_equal(m2['colors'], np.repeat([[1.0, 0.0, 0.0]], 32 * n, 0))
    ys = ((m2['vertices'][:32] - g['pos'][0]) @ rotation_matrix(quat[0]))[:, 1]
    np.testing.assert_allclose([ys.min(), ys.max()], [-0.05, 0.05], rtol=0, atol=1e-15)
    with pytest.raises(TypeError, match='unknown hand parameters'):
        grasp_post.hand_mesh(g, spacing=1.0)
    empty = grasp_post.hand_mesh(dict(pos=np.zeros((0, 3)), quat=np.zeros((0, 4)), width=np.zeros(0), score=np.zeros(0)))
    assert empty['vertices'].shape == (0, 3) and empty['faces'].shape == (0, 3)


def test_hand_mesh_writes_a_ply(tmp_path):
    g = dict(pos=np.array([[0.1, 0.1, 0.1]]), quat=np.array([[0.0, 0.0, 0.0, 1.0]]), width=np.array([0.05]), score=np.array([0.75]))
    m = grasp_post.hand_mesh(g)
    path = tmp_path / 'hand.ply'
    grasp_post.write_ply(path, m['vertices'], m['colors'], faces=m['faces'])
    text = path.read_text().splitlines()
    assert 'element vertex 32' in text and 'element face 48' in text and text[-1].startswith('3 ')


# ---- 3. the C ABI's refusals, before the device (no GPU) --------------------------------------------------------------------------------------
def _params(scale=VOXEL, **kw):
    return _lib.GnrHandParams(**{**hand.checked_hand(), 'scale': scale, **kw})


def test_refusals_before_the_device():
    """Fake pointers: every call is one that validation refuses, each with its code and a text that names the entry point and the limit."""
    L = _lib.lib()
    one = C.c_void_p(16)
    fn = 'gnr_hand_clearance_fwd'
    text = lambda: L.gnr_last_error().decode()
    names = ('vol', 'pos', 'quat', 'width', 'count', 'clearance', 'worst', 'inside')

    def call(p=None, stride=1, B=1, R=40, max_n=4, top_k=0, **kw):
        ptr = {k: kw.pop(k, one) for k in names}
        p = _params(**kw) if p is None else p
        return L.gnr_hand_clearance_fwd(C.byref(p) if p is not False else None, ptr['vol'], ptr['pos'], ptr['quat'], ptr['width'], ptr['count'], stride,
                                        B, R, max_n, top_k, ptr['clearance'], ptr['worst'], ptr['inside'], None)

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
    # the cap on a grasp's samples, counted for the widest opening (R voxels)
    for kw in (dict(spacing=1e-3), dict(approach=1e4), dict(R=256, spacing=0.01)):
        assert call(**kw) == _lib.GNR_ERR_ARG and 'GNR_HAND_MAX_SAMPLES' in text() and str(_lib.GNR_HAND_MAX_SAMPLES) in text(), kw
    assert ref.totals(256 * VOXEL, VOXEL)[1] <= _lib.GNR_HAND_MAX_SAMPLES < ref.totals(256 * VOXEL, VOXEL, spacing=0.01)[1]


def test_hand_clearance_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        hand.HandClearance()


# ---- 4. keyword checks (no GPU) -------------------------------------------------------------------------------------------------------------------
def test_keyword_checks():
    from graspnerf_amd import planner
    from graspnerf_amd.grasp_post import GRASP_UTILS_PROCESS
    from graspnerf_amd.planner_session import PlannerSession
    frames, cams = [np.zeros((8, 8, 3), np.uint8)] * 4, [np.eye(4)] * 4
    with pytest.raises(TypeError, match='unknown clearance parameters'):
        planner.plan_real(None, frames, cams, np.eye(3), clearance={'bogus': 1})
    with pytest.raises(TypeError, match='unknown clearance parameters'):
        planner.real_session(None, 4, (8, 8), (32, 32), clearance={'iso': 0.0})
    with pytest.raises(ValueError, match='finger_width must be finite and > 0'):
        planner.plan_real(None, frames, cams, np.eye(3), clearance=dict(finger_width=0.0))
    with pytest.raises(ValueError, match='approach must be finite and >= 0'):
        planner.real_session(None, 4, (8, 8), (32, 32), clearance=dict(approach=-0.01))
    with pytest.raises(ValueError, match='opening must be None'):
        hand.hand_params(dict(opening=float('nan')))
    for k in ('height', 'tail_length', 'depth', 'spacing'):
        with pytest.raises(ValueError, match=k + ' must be finite and > 0'):
            hand.hand_params({k: float('inf')})
    assert hand.hand_params(False) is None and hand.hand_params(None) is None
    want = dict(height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, opening=None, spacing=0.5, approach=0.05, level=0.0)
    assert hand.hand_params(True) == want and hand.hand_params({}) == want
    assert hand.HAND_DEFAULTS == {k: v for k, v in want.items() if k != 'level'} == ref.DEFAULTS
    assert {k: p.default for k, p in inspect.signature(hand.HandClearance.__call__).parameters.items() if k in hand.HAND_DEFAULTS} == hand.HAND_DEFAULTS
    assert inspect.signature(hand.HandClearance.__call__).parameters['top_k'].default is None
    p = hand.hand_params(dict(opening=hand.EXECUTE_GRASP_OPENING, spacing=1, filter=True), filter=False)
    assert p == dict(want, opening=0.08, spacing=1.0, filter=True) and isinstance(p['spacing'], float)
    assert grasp_post.same_params(p, {k: v for k, v in p.items() if k != 'filter'}) and not grasp_post.same_params(p, hand.hand_params(True))
    assert not grasp_post.same_params(p, None) and grasp_post.same_params(None, None)
    assert hand.checked_hand()['opening'] == -1.0 and hand.checked_hand(opening=0.0)['opening'] == 0.0
    for fn, name, default in ((planner.plan_real, 'clearance', False), (planner.real_session, 'clearance', False),
                              (PlannerSession.__init__, 'hand_clearance', None)):
        assert inspect.signature(fn).parameters[name].default is default, fn
    # a session built without the switch and asked for it, and the other way round
    net = object()
    built = lambda hc: types.SimpleNamespace(net=net, selector_params=dict(GRASP_UTILS_PROCESS, order='index', top_k=None), surface_params=dict(rg=(-0.2, 0.2)),
                                             voxel_size=planner.REAL_VOXEL_SIZE, surface_normals=False, mesh_params=None, volume_depth_params=None,
                                             view_color_params=None, hand_params=hand.hand_params(hc), closure_params=None)
    for have, ask in ((False, True), (True, False), (True, dict(approach=0.0)), (dict(level=0.5), True)):
        with pytest.raises(ValueError, match=r'the session was built for another clearance \(build it with planner.real_session'):
            planner.plan_real(net, frames, cams, np.eye(3), session=built(have), clearance=ask)


# ---- GPU: the bits of the statement ----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5a


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _sentinel(rows, width, dtype):
    """[rows + 1, width] of `dtype` on the device, every byte the sentinel: one spare row behind what the call is told about."""
    return torch.full(((rows + 1) * width * 4,), SENTINEL, dtype=torch.uint8, device='cuda:0').view(dtype)


def _raw(vol, pos, quat, width, count, scale, top_k=None, **kw):
    """The C call on outputs filled with a sentinel byte, with one more row behind [B,max_n] that the call is not told about
    -> (clearance, worst, inside) [B,max_n,2] as numpy, and whether the spare rows kept the sentinel."""
    L = _lib.lib()
    B, R, n = vol.shape[0], vol.shape[-1], pos.shape[1]
    count = np.ascontiguousarray(count, np.int32)
    dev = [_up(a) for a in (np.asarray(vol, f32), np.asarray(pos, f64), np.asarray(quat, f32), np.asarray(width, f32), count)]
    outs = [_sentinel(B * n, 2, t) for t in (torch.float32, torch.int32, torch.int32)]
    p = _lib.GnrHandParams(scale=float(scale), **hand.checked_hand(**kw))
    rc = L.gnr_hand_clearance_fwd(C.byref(p), *(t.data_ptr() for t in dev), count.size // B, B, R, n, int(top_k or 0), *(t.data_ptr() for t in outs),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'gnr_hand_clearance_fwd')
    torch.cuda.synchronize()
    outs = [t.cpu().numpy() for t in outs]
    spare = all(bool((t[2 * B * n:].view(np.uint8) == SENTINEL).all()) for t in outs)
    return tuple(t[:2 * B * n].reshape(B, n, 2) for t in outs), spare


def _want(vol, pos, quat, width, count, scale, top_k=None, **kw):
    """The statement on the same sentinel-filled outputs, scene by scene."""
    B, n = pos.shape[:2]
    out = []
    for b in range(B):
        o = tuple(np.full(8 * n, SENTINEL, np.uint8).view(t).reshape(n, 2) for t in (f32, np.int32, np.int32))
        out.append(ref.clearance_rows(vol[b], pos[b], quat[b], width[b], np.asarray(count).reshape(B, -1)[b, 0], scale, top_k=top_k, out=o, **kw))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _check(what, vol, pos, quat, width, count, scale, top_k=None, **kw):
    got, spare = _raw(vol, pos, quat, width, count, scale, top_k, **kw)
    want = _want(vol, pos, quat, width, count, scale, top_k, **kw)
    assert spare, (what, 'written beyond [B,max_n]')
    for name, g, w in zip(('clearance', 'worst', 'inside'), got, want):
        assert same(g, w), (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()), g[(g != w).any(-1)][:3], w[(g != w).any(-1)][:3])
    return want


@pytest.mark.gpu
def test_small_volume_and_contents_that_are_no_numbers():
    """R = 8, B = 1: an axis-aligned grasp, a general rotation, a clamped width, and rows whose width is NaN or 1e30, whose quaternion is
    zero or NaN, whose position is NaN or huge."""
    R, scale = 8, 0.02                                                         # a hand of 0.1 m in a lattice of 0.14 m
    vol = np.random.default_rng(5).uniform(-1, 1, (1, R, R, R)).astype(f32)
    pos = np.array([[[3.5, 3.5, 3.5], [3.2, 4.1, 2.7], [3.0, 3.0, 3.0], [3.0, 3.0, 3.0], [3.5, 3.5, 3.5], [3.5, 3.5, 3.5], [3.5, 3.5, 3.5],
                     [np.nan, 3.0, 3.0], [1e300, -1e300, 3.0]]])
    quat = f32([[[0, 0, 0, 1], [0.3, -0.5, 0.2, 0.7], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [np.nan, 0, 0, 1], [0, 0, 0, 1],
                 [0, 0, 0, 1]]])
    width = f32([[2.0, 1.5, -4.0, np.nan, 1e30, 2.0, 2.0, 2.0, 2.0]])
    want = _check('R = 8', vol, pos, quat, width, [9], scale)
    assert np.isfinite(want[0]).all() and (want[2][0, :5, 0] > 0).all()
    assert list(want[2][0, 3]) == list(want[2][0, 2]), 'a NaN width is an opening of 0, like a negative one'
    assert want[2][0, 4, 1] <= ref.totals(R * scale, scale)[1]
    _check('R = 8, one opening, a real hand', vol, pos, quat, width, [9], scale, opening=0.05, height=0.02, finger_width=0.01, spacing=0.7, approach=0.03)
    _check('R = 2', vol[:, :2, :2, :2].copy(), pos * 0.1, quat, width, [9], 0.1)


@pytest.mark.gpu
def test_the_analytic_grasps():
    """R = 40, B = 5 (one volume per grasp), the five analytic grasps of the module in one call."""
    cases = analytic()
    vol = np.stack([c[1] for c in cases])
    pos, quat, width = (np.stack([c[i] for c in cases])[:, None] for i in (2, 3, 4))
    want = _check('analytic', vol, pos, quat, width, [1] * 5, VOXEL)
    c, inside = want[0][:, 0], want[2][:, 0]
    assert 0.1 < c[0, 0] < 0.25 and c[0, 1] == c[0, 0] and c[1, 0] < 0 and c[2, 0] > 0 > c[2, 1] and c[3, 0] > 0 and c[3, 1] > 0
    assert list(inside[4]) == [477, 537]


@pytest.mark.gpu
def test_counts_rows_and_top_k():
    """B = 2, max_n = 4: rows beyond min(count, top_k, max_n) keep the sentinel, a scene without grasps writes nothing."""
    vol = np.stack([spheres40()['vol'], sphere_volume([0.0, 0.0, 0.1], 0.05)])
    pos, quat, width = _random_grasps(8, 21, lo=5.0, hi=34.0)
    pos, quat, width = pos.reshape(2, 4, 3), quat.reshape(2, 4, 4), width.reshape(2, 4)
    for count, top_k, rows in (([0, 7], None, (0, 4)), ([0, 7], 2, (0, 2)), ([3, 1], 2, (2, 1)), ([-5, 2], None, (0, 2)), ([4, 4], 9, (4, 4))):
        want = _check((count, top_k), vol, pos, quat, width, count, VOXEL, top_k=top_k)
        for b in range(2):
            assert (want[2][b, :rows[b], 1] > 0).all() and (want[0][b, rows[b]:].view(np.uint8) == SENTINEL).all(), (count, top_k, b)
    # a count with a stride of 2 (a [B,2] tensor): the first column counts
    _check('stride 2', vol, pos, quat, width, [[2, 99], [3, 99]], VOXEL)


@pytest.mark.gpu
def test_sample_counts_and_idle_lanes():
    """Sample counts that are no multiples of 64, and a grasp with fewer than 64 samples: lanes without a sample take part in the
    reduction with an empty pair."""
    vol = spheres40()['vol'][None]
    pos, quat, width = _random_grasps(6, 31, lo=10.0, hi=29.0)
    pos, quat, width = pos[None], quat[None], width[None]
    for kw in (dict(spacing=4.0, approach=0.0), dict(spacing=4.0), dict(spacing=1.3, approach=0.02), dict(spacing=0.5, approach=0.013)):
        at, swept = ref.totals(ref.opening_of(width[0, 0], R40, VOXEL), VOXEL, **kw)
        print(kw, at, swept)
        assert swept % 64 != 0
        _check(kw, vol, pos, quat, width, [6], VOXEL, **kw)
    assert ref.totals(9.33 * VOXEL, VOXEL, spacing=4.0, approach=0.0)[1] < 64


@pytest.mark.gpu
def test_ties_take_the_lower_ordinal():
    """A volume with slabs of one value: many samples attain the minimum exactly, on several lanes; and a volume of -0.0 and 0.0."""
    slabs = np.ones((R40,) * 3, f32)
    slabs[:, 8:14, :] = 0.25
    slabs[:, 26:32, :] = 0.25                                                  # both fingers of a wide hand along y reach a slab
    zeros = np.zeros((R40,) * 3, f32)
    zeros[:20] = -0.0
    vol = np.stack([slabs, zeros, zeros])
    centre = np.full(3, 19.5)
    pos = np.stack([centre, centre + [6.0, 0.0, 0.0], centre - [6.0, 0.0, 0.0]])[:, None]
    quat = f32([[DOWN], [[0, 0, 0, 1]], [[0.3, -0.5, 0.2, 0.7]]])
    width = f32([[9.33 + 6.0], [5.0], [5.0]])
    want = _check('ties', vol, pos, quat, width, [1, 1, 1], VOXEL)
    d = {}
    c, worst, inside = ref.clearance(slabs, pos[0, 0], quat[0, 0], width[0, 0], VOXEL, details=d)
    tied = np.flatnonzero(d['value'] == 0.25)
    assert c[1] == f32(0.25) and len(tied) > 64 and worst[1] == tied[0] and worst[0] == tied[d['at_grasp'][tied]][0]
    # -0.0 and 0.0 tie: the first sample inside wins and its own bits are the clearance
    for b in (1, 2):
        d = {}
        ref.clearance(zeros, pos[b, 0], quat[b, 0], width[b, 0], VOXEL, details=d)
        first = np.flatnonzero(~np.isnan(d['value']))[0]
        assert want[1][b, 0, 1] == first and same(want[0][b, 0, 1], f32(d['value'][first]))
    signs = {bool(np.signbit(want[0][b, 0, 1])) for b in (1, 2)}
    print('signs of the zero clearances:', signs)


@pytest.mark.gpu
def test_random_grasps_equal_the_statement():
    """256 seeded grasps at R = 40, positions partly outside the box, widths over the selector's range; and hand.HandClearance on the
    same rows gives the same bits into buffers it keeps."""
    vol = spheres40()['vol'][None]
    pos, quat, width = _random_grasps(256, 41)
    want = _check('random', vol, pos[None], quat[None], width[None], [256], VOXEL)
    inside = want[2][0]
    assert (inside[:, 1] == 0).sum() > 0 and (inside[:, 1] > 2000).sum() > 20 and ((0 < inside[:, 1]) & (inside[:, 1] < 2000)).sum() > 20
    op = hand.HandClearance()
    count = torch.tensor([256], dtype=torch.int32, device='cuda:0')
    a = op(vol, pos[None], quat[None], width[None], count, scale=VOXEL)
    ptrs = {k: v.data_ptr() for k, v in a.items()}
    host = {k: v.cpu().numpy() for k, v in a.items()}
    for k, w in zip(('clearance', 'worst', 'inside'), want):
        assert same(host[k], w), k
    b = op(vol[0], pos, quat, width, count, scale=VOXEL, top_k=300)
    assert {k: v.data_ptr() for k, v in b.items()} == ptrs and all(same(b[k].cpu().numpy(), host[k]) for k in host)
    with pytest.raises(ValueError, match='pos must be'):
        op(vol, pos[None, :, :2], quat[None], width[None], count, scale=VOXEL)
    with pytest.raises(ValueError, match='count must be'):
        op(vol, pos[None], quat[None], width[None], [256], scale=VOXEL)
    with pytest.raises(_lib.GnrError, match='GNR_HAND_MAX_SAMPLES'):
        op(vol, pos[None], quat[None], width[None], count, scale=VOXEL, spacing=1e-3)


def _eager_hand(vol, sel, n, **kw):
    """hand.HandClearance on the volume and the (host) selection a plan returned -> the plan's columns in the selection's order."""
    up = {k: _up(sel[k].numpy() if torch.is_tensor(sel[k]) else sel[k]) for k in ('count', 'index', 'quat', 'width')}
    res = hand.HandClearance().of_selection(_up(vol), dict(up, top_k=sel.get('top_k')), scale=0.3 / 40, **kw)
    return hand.hand_from_rows({k: v.cpu().numpy() for k, v in hand.hand_rows(res, 0, n).items()})


@pytest.mark.gpu
def test_session_records_the_hand():
    """PlannerSession(hand_clearance={}) at cfg1's size: every plan's columns equal the eager HandClearance on the volume and the selection
    that plan returned (and the statement on its first rows); a replay of the first plan returns the first plan's bits; the columns go
    through the seeded permutation of the other columns."""
    from graspnerf_amd import planner
    from graspnerf_amd.planner_session import PlannerSession
    from test_planner_session import CFG, IMG_WH, MAX_GRASPS, PARAMS, SEED, SRC_HW, V, _scene, _state_dict
    net = planner.load_model(dict(CFG), {'network_state_dict': _state_dict(width_bias=5.0)})
    plain = PlannerSession(net, V, SRC_HW, IMG_WH, max_grasps=MAX_GRASPS, **PARAMS)
    s = PlannerSession(net, V, SRC_HW, IMG_WH, max_grasps=MAX_GRASPS, hand_clearance={}, **PARAMS)
    assert s._d_out.numel() == plain._d_out.numel() and [p.out for p in s.products] == ['hand'] and plain.products == []
    A, B = _scene(1), _scene(2, radius=0.55, theta=np.pi / 3.4)
    plan = lambda ses, sc, seed: ses.plan(sc['frames'], sc['poses'], sc['Ks'], sc['depth_range'], sc['bbox3d'], seed=seed, return_volumes=True)[0]
    keys = ('clearance', 'approach_clearance', 'hand_inside', 'hand_worst', 'collision_free')
    first = None
    for what, sc in (('A', A), ('B', B), ('A again', A)):
        g = plan(s, sc, None)
        n = len(g['score'])
        assert 1 <= n < MAX_GRASPS and all(len(g[k]) == n for k in keys)
        want = _eager_hand(g['volumes'][0], s.selection, n)
        for k in keys:
            assert same(g[k], want[k]), (what, k)
        assert g['clearance'].dtype == f32 and g['hand_inside'].shape == (n, 2) and g['collision_free'].dtype == bool
        assert np.array_equal(g['collision_free'], g['approach_clearance'] > 0)
        vol = g['volumes'][0].reshape(40, 40, 40)
        for r in range(min(n, 8)):
            c, worst, inside = ref.clearance(vol, g['index'][r].astype(f64), s.selection['quat'][0, r].numpy(), s.selection['width'][0, r].numpy(), 0.3 / 40)
            assert same(g['clearance'][r], c[0]) and same(g['approach_clearance'][r], c[1]) and same(g['hand_worst'][r], worst) \
                and same(g['hand_inside'][r], inside), (what, r)
        if first is None:
            first = g
            p0 = plan(plain, sc, None)
            for k in ('index', 'pos', 'quat', 'width', 'score'):
                assert same(g[k], p0[k]), ('the other columns do not depend on the product', k)
            assert set(g) == set(p0) | set(keys)
        elif what == 'A again':
            assert all(same(g[k], first[k]) for k in keys + ('index', 'score'))
        else:
            assert len(g['score']) != len(first['score']) or not same(g['clearance'], first['clearance'])
    assert s.captures == 1
    seeded = plan(s, A, SEED)
    np.random.seed(SEED)
    perm = np.random.permutation(len(first['score']))
    for k in keys + ('index', 'score'):
        assert same(seeded[k], first[k][perm]), k


@pytest.mark.gpu
def test_plan_real_with_clearance_eager_and_session():
    """plan_real(clearance=...) with and without session= agree bit for bit, every other key is what it is without the option, and
    filter=True returns exactly the collision_free rows in their order.  The synthetic checkpoint's volume need not cross zero: the
    level is the median of the plan's own approach clearances."""
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
    on = planner.plan_real(net, A, **cam, **kw, clearance=True)
    keys = {'clearance', 'approach_clearance', 'hand_inside', 'hand_worst', 'collision_free'}
    assert set(on[0]) == set(off[0]) | keys and set(on[3]) == set(off[3])
    for k in off[0]:
        assert same(on[0][k], off[0][k]), k
    assert same(on[1], off[1]) and same(on[2], off[2]) and all(same(on[3][k], off[3][k]) for k in off[3])
    n = len(on[0]['score'])
    assert n == TOP_K
    level = float(np.median(on[0]['approach_clearance']))
    ask = dict(level=level, opening=hand.EXECUTE_GRASP_OPENING)
    eager = planner.plan_real(net, A, **cam, **kw, clearance=ask)
    sess = planner.real_session(net, V, HW, HW[::-1], **kw, clearance=ask)
    got = planner.plan_real(net, A, **cam, **kw, clearance=ask, session=sess)
    for k in eager[0]:
        assert same(got[0][k], eager[0][k]), k
    free = eager[0]['collision_free']
    print(f'{free.sum()} of {n} grasps are collision free above the level {level:.4f}')
    assert np.array_equal(free, eager[0]['approach_clearance'] > f32(level))
    for route in (dict(), dict(session=sess)):
        kept = planner.plan_real(net, A, **cam, **kw, clearance=dict(ask, filter=True), **route)
        assert kept[0]['collision_free'].all() and len(kept[1]) == free.sum()
        for k in eager[0]:
            assert same(kept[0][k], eager[0][k][free]), (sorted(route), k)
        assert same(kept[1], eager[1][free])
    # order='permuted': the new columns go through the permutation of the other columns
    a = planner.plan_real(net, A, **cam, seed=5, clearance=True)
    b = planner.plan_real(net, A, **cam, seed=5)
    assert same(a[0]['index'], b[0]['index']) and len(a[0]['clearance']) == len(b[0]['score'])
    with pytest.raises(ValueError, match='another clearance'):
        planner.plan_real(net, A, **cam, **kw, session=sess)
    with pytest.raises(ValueError, match='another clearance'):
        planner.plan_real(net, A, **cam, **kw, session=sess, clearance=True)
