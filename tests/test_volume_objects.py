"""Objects of the volume (csrc/gnr_objects.hip, objects.VolumeObjects; k_grasp_objects in csrc/gnr_hand.hip, objects.GraspObjects).
tests/objects_reference.py is the statement (scipy.ndimage.label, numpy integers, hand_reference's poses); every comparison is
np.array_equal.  Without a GPU: the statement on a slab with two truncated spheres standing on it, corner- and edge-only contact, the
parameter checks, the host functions.  On the GPU: shapes chosen to break a parallel union-find rather than to resemble the workload."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, hand, objects
import objects_reference as oref
from test_hand_clearance import DOWN, ORIGIN, R40, VOXEL, sphere_volume

f32, f64 = np.float32, np.float64
CENTRE_A, RADIUS_A, CENTRE_B, RADIUS_B = (12, 12, 9), 6.3, (12, 30, 8), 5.3     # lattice units (no voxel lies on either sphere); both reach below k = 3
SLAB_TOP, FLOATER = 3, (35, 5, 30)                                             # the slab is solid for k <= 3
REAL_HAND = dict(height=0.02, finger_width=0.01, opening=0.08)                 # a 2 cm x 1 cm hand opened to 0.08 m
KEYS = ('labels', 'count', 'voxels', 'bbox', 'sums', 'cleaned')


@functools.lru_cache(maxsize=None)
def table_scene():
    """[40,40,40] float32, never written to: a slab, two spheres that stand on it (their lowest part is inside the slab) and a floater
    of one voxel."""
    world = lambda c: ORIGIN + np.asarray(c, f64) * VOXEL
    k = np.arange(R40, dtype=f64)
    slab = np.broadcast_to(np.clip((k - (SLAB_TOP + 0.5)) / 4.0, -1.0, 1.0).astype(f32), (R40,) * 3)
    vol = np.minimum(np.minimum(sphere_volume(world(CENTRE_A), RADIUS_A * VOXEL), sphere_volume(world(CENTRE_B), RADIUS_B * VOXEL)), slab).copy()
    vol[FLOATER] = -0.5
    vol.setflags(write=False)
    return vol


def ball(centre, radius):
    i = np.arange(R40, dtype=f64)
    I, J, K = np.meshgrid(i, i, i, indexing='ij')
    return (I - centre[0]) ** 2 + (J - centre[1]) ** 2 + (K - centre[2]) ** 2 < radius ** 2


# the three grasps of the module: (pos in lattice units, quat, width in voxels): across sphere A, across both spheres, in empty space
GRASPS = ((f64([12, 12, 16]), DOWN, f32(14.0)), (f64([12, 21, 14]), DOWN, f32(30.0)), (f64([30, 10, 30]), DOWN, f32(8.0)))


# ---- 1. the statement (no GPU) --------------------------------------------------------------------------------------------------------
def test_the_table_must_be_cut_for_objects_to_separate():
    vol = table_scene()
    lab, count = oref.label(vol)
    assert count == 2 and lab[0, 0, 0] == 1 and lab[CENTRE_A] == 1 and lab[CENTRE_B] == 1 and lab[FLOATER] == 2
    lab, count = oref.label(vol, z_min=SLAB_TOP + 1)
    assert count == 3 and (lab[CENTRE_A], lab[CENTRE_B], lab[FLOATER]) == (1, 2, 3) and not lab[:, :, :SLAB_TOP + 1].any()
    voxels, bbox, sums = oref.statistics(lab, count, 8)
    above = np.arange(R40)[None, None, :] > SLAB_TOP
    for row, (c, r) in enumerate(((CENTRE_A, RADIUS_A), (CENTRE_B, RADIUS_B))):
        mask = ball(c, r) & above
        assert voxels[row] == mask.sum() == (lab == row + 1).sum()
        at = np.argwhere(mask)
        assert list(bbox[row]) == list(at.min(0)) + list(at.max(0)) and list(sums[row]) == list(at.sum(0))
    assert voxels[2] == 1 and list(bbox[2]) == list(FLOATER) * 2 and list(sums[2]) == list(FLOATER)
    assert not voxels[3:].any() and (bbox[3:] == [R40] * 3 + [-1] * 3).all() and not sums[3:].any()
    # the floater is listed, and gone from `cleaned` at min_voxels = 2; nothing else moves
    c1, c2 = oref.cleaned(vol, lab, count, 1), oref.cleaned(vol, lab, count, 2)
    assert np.array_equal(c1, vol) and c2[FLOATER] == 1.0 and np.array_equal(np.argwhere(c2 != vol), [list(FLOATER)])
    assert oref.label(c2, z_min=SLAB_TOP + 1)[1] == 2
    # the host function on these rows: centres within half a voxel of the spheres' (the cut takes a cap of one voxel off each)
    rows = dict(count=np.int32([count]), voxels=voxels[:count], bbox=bbox[:count], sums=sums[:count], status=np.int32([0]))
    o = objects.objects_from_rows(rows, VOXEL, ORIGIN, min_voxels=2)
    assert o['count'] == 3 and list(o['kept']) == [True, True, False] and o['voxels'].dtype == np.int32 and o['centroid'].dtype == f64
    for row, c in enumerate((CENTRE_A, CENTRE_B)):
        assert np.abs((o['centroid'][row] - ORIGIN) / VOXEL - c).max() < 0.5, (row, o['centroid'][row])
    assert np.array_equal(o['centroid'], ORIGIN + (sums[:3].astype(f64) / voxels[:3, None].astype(f64)) * f64(VOXEL))
    assert np.array_equal(o['extent'], (bbox[:3, 3:] - bbox[:3, :3] + 1).astype(f64) * f64(VOXEL))
    assert np.array_equal(o['top'], ORIGIN[2] + bbox[:3, 5].astype(f64) * f64(VOXEL)) and np.array_equal(o['bbox_hi'], bbox[:3, 3:])
    assert o['top'][0] > o['top'][1] and np.array_equal(o['bbox_lo'][2], FLOATER)


def test_which_object_a_grasp_closes_on():
    lab, _ = oref.label(table_scene(), z_min=SLAB_TOP + 1)
    one, both, none = (oref.grasp_object(lab, *g, VOXEL) for g in GRASPS)
    print(one, both, none)
    assert one[0] == 1 and one[2] == 1 and one[1] > 50 and one[3] > one[1]
    assert both[2] == 2 and both[0] == 1 and both[1] > 50                    # sphere A is the larger one
    assert none[:3] == (0, 0, 0) and none[3] > 0
    # the same hand over sphere B alone
    assert oref.grasp_object(lab, f64([12, 30, 15]), DOWN, f32(14.0), VOXEL)[::2] == (2, 1)
    # a hand outside the lattice takes no sample; ties go to the smaller label
    assert oref.grasp_object(lab, f64([-30, 5, 5]), DOWN, f32(8.0), VOXEL) == (0, 0, 0, 0)
    halves = np.ones((8, 8, 8), np.int32)
    halves[:, 4:, :] = 2
    got = oref.grasp_object(halves, f64([3.5, 3.5, 3.5]), f32([0, 0, 0, 1]), f32(3.5), 0.5, depth=1.0)    # 8 samples along y, 4 on each side
    assert got[0] == 1 and got[2] == 2 and 2 * got[1] == got[3], got
    rows = oref.grasp_objects(lab, np.stack([g[0] for g in GRASPS]), np.stack([g[1] for g in GRASPS]), f32([g[2] for g in GRASPS]), 2, VOXEL)
    assert list(rows[0]) == [1, 1, 0] and list(rows[2]) == [1, 2, 0] and rows[3][2] == 0


def test_corner_and_edge_contact():
    corner, edge = np.ones((4, 4, 4), f32), np.ones((4, 4, 4), f32)
    corner[1, 1, 1] = corner[2, 2, 2] = edge[1, 1, 1] = edge[1, 2, 2] = -1.0
    assert [oref.label(corner, connectivity=c)[1] for c in (6, 18, 26)] == [2, 2, 1]
    assert [oref.label(edge, connectivity=c)[1] for c in (6, 18, 26)] == [2, 1, 1]


def test_object_params():
    assert objects.object_params(False) is None and objects.object_params(None) is None
    want = dict(level=0.0, lower=None, z_min=0, connectivity=6, max_objects=1024, min_voxels=1, cleaned=False)
    assert objects.object_params(True) == want == objects.object_params({}) == objects.OBJECT_DEFAULTS
    p = objects.object_params(dict(z_min=4, connectivity=26, lower=-1, filter=True), filter=False)
    assert p == dict(want, z_min=4, connectivity=26, lower=-1.0, filter=True) and isinstance(p['lower'], float)
    with pytest.raises(TypeError, match='unknown objects parameters'):
        objects.object_params(dict(iso=0.0))
    for bad, text in ((dict(level=math.nan), 'level must be finite'), (dict(level=math.inf), 'level must be finite'),
                      (dict(lower=math.nan), 'lower must be None'), (dict(z_min=-1), 'z_min must be an integer >= 0'),
                      (dict(z_min=1.5), 'z_min must be an integer'), (dict(connectivity=8), 'connectivity must be 6, 18 or 26'),
                      (dict(max_objects=0), 'max_objects must be an integer >= 1'), (dict(min_voxels=2.5), 'min_voxels must be an integer'),
                      (dict(cleaned=1), 'cleaned must be True or False')):
        with pytest.raises(ValueError, match=text):
            objects.object_params(bad)
    import inspect
    assert {k: v.default for k, v in inspect.signature(objects.VolumeObjects.__call__).parameters.items() if k in want} == want


def test_host_functions():
    rows = dict(count=np.int32([5]), voxels=np.int32([3, 2, 1]), bbox=np.zeros((3, 6), np.int32), sums=np.zeros((3, 3), np.int64))
    with pytest.raises(_lib.GnrError, match='5 objects but the buffers hold 3: raise max_objects'):
        objects.objects_from_rows(rows, VOXEL)
    with pytest.raises(_lib.GnrError, match='bound of one of its loops'):
        objects.objects_from_rows(dict(rows, count=np.int32([3]), status=np.int32([_lib.GNR_OBJECTS_STATUS_BOUND])), VOXEL)
    o = objects.objects_from_rows(dict(rows, count=np.int32([2])), 0.5, (1.0, 2.0, 3.0))
    assert o['count'] == 2 and list(o['voxels']) == [3, 2] and np.array_equal(o['centroid'], [[1.0, 2.0, 3.0]] * 2) and list(o['kept']) == [True, True]
    assert objects.best_per_object(np.int32([2, 2, 0, 1, 2, 3, 1])) == {2: 0, 1: 3, 3: 5}
    assert objects.best_per_object(np.zeros(0, np.int32)) == {} and objects.best_per_object([0, 0]) == {}
    cols = objects.grasp_objects_from_rows(dict(object=np.int32([1]), votes=np.int32([7]), distinct=np.int32([2]), inside=np.int32([9])))
    assert {k: int(v[0]) for k, v in cols.items()} == dict(object=1, object_votes=7, objects_in_hand=2, object_samples=9)
    with pytest.raises(TypeError, match='unknown objects parameters'):
        objects.objects_of_plan(table_scene(), dict(index=np.zeros((0, 3)), quat=np.zeros((0, 4)), width=np.zeros(0)), iso=0.0)


def test_volume_objects_need_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for op in (objects.VolumeObjects, objects.GraspObjects):
        with pytest.raises(_lib.GnrError, match='no CPU fallback'):
            op()


# ---- 2. the refusals of the two entry points --------------------------------------------------------------------------------------------
OBJ_NAMES = ('vol', 'labels', 'count', 'voxels', 'bbox', 'sums', 'workspace')
ROW_NAMES = ('labels', 'pos', 'quat', 'width', 'count', 'object', 'votes', 'distinct', 'inside')


def _params(**kw):
    return _lib.GnrObjectsParams(**{**dict(level=0.0, lower=-math.inf, z_min=0, connectivity=6, max_objects=4, min_voxels=1, free_value=1.0), **kw})


def _refusals(ptr_objects, ptr_rows, cleaned, ws_bytes, B=1, R=8, max_n=4):
    """Every refusal of the two entry points, each with its code and its text, on the pointers given (fake ones, or buffers whose
    bytes the caller checks afterwards)."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_volume_objects_fwd'
    need = L.gnr_volume_objects_workspace_bytes(B, R)
    assert need >= 2 * 4 * B * R ** 3 and ws_bytes >= need
    assert L.gnr_volume_objects_workspace_bytes(0, R) == 0 and L.gnr_volume_objects_workspace_bytes(B, 1) == 0 and L.gnr_volume_objects_workspace_bytes(B, 257) == 0

    def call(p=None, B=B, R=R, ws=ws_bytes, **kw):
        ptr = {k: kw.pop(k, ptr_objects[k]) for k in OBJ_NAMES}
        p = _params(**kw) if p is None else p
        return L.gnr_volume_objects_fwd(C.byref(p) if p is not False else None, ptr['vol'], B, R, ptr['labels'], ptr['count'], ptr['voxels'], ptr['bbox'],
                                        ptr['sums'], cleaned, ptr['workspace'], ws, None)

    for name in OBJ_NAMES:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for r in (1, 0, 257):
        assert call(R=r) == _lib.GNR_ERR_SHAPE and text() == fn + ': R must be in 2..256', r
    for c in (0, 4, 8, 27, -6):
        assert call(connectivity=c) == _lib.GNR_ERR_ARG and 'connectivity must be 6, 18 or 26' in text(), c
    for m in (0, -1):
        assert call(max_objects=m) == _lib.GNR_ERR_SHAPE and 'max_objects must be >= 1' in text(), m
    for z in (-1, R + 1):
        assert call(z_min=z) == _lib.GNR_ERR_ARG and 'z_min must be in 0..R' in text(), z
    for bad in (math.nan, math.inf, -math.inf):
        assert call(level=bad) == _lib.GNR_ERR_ARG and 'level must be finite' in text(), bad
        assert call(free_value=bad) == _lib.GNR_ERR_ARG and 'free_value must be finite' in text(), bad
    assert call(lower=math.nan) == _lib.GNR_ERR_ARG and 'lower must not be a NaN' in text()
    for ws in (0, need - 1):
        assert call(ws=ws) == _lib.GNR_ERR_WORKSPACE and text() == fn + ': workspace too small', ws
    fn = 'gnr_grasp_objects_fwd'

    def rows(p=None, stride=1, B=B, R=R, max_n=max_n, top_k=0, **kw):
        ptr = {k: kw.pop(k, ptr_rows[k]) for k in ROW_NAMES}
        p = _lib.GnrHandParams(**{**hand.checked_hand(), 'scale': 0.02, **kw}) if p is None else p
        return L.gnr_grasp_objects_fwd(C.byref(p) if p is not False else None, ptr['labels'], ptr['pos'], ptr['quat'], ptr['width'], ptr['count'], stride,
                                       B, R, max_n, top_k, ptr['object'], ptr['votes'], ptr['distinct'], ptr['inside'], None)

    for name in ROW_NAMES:
        assert rows(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    assert rows(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, 65536):
        assert rows(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for r in (1, 257):
        assert rows(R=r) == _lib.GNR_ERR_SHAPE and 'R must be in 2..256' in text(), r
    assert rows(max_n=0) == _lib.GNR_ERR_SHAPE and 'max_n must be >= 1' in text()
    assert rows(stride=0) == _lib.GNR_ERR_ARG and 'count_stride must be >= 1' in text()
    assert rows(top_k=-1) == _lib.GNR_ERR_ARG and 'top_k must be >= 0' in text()
    for key in ('height', 'finger_width', 'tail_length', 'depth', 'spacing', 'scale'):
        for bad in (0.0, -1.0, math.nan, math.inf):
            assert rows(**{key: bad}) == _lib.GNR_ERR_ARG and 'must be finite and > 0' in text() and fn in text(), (key, bad)
    assert rows(approach=-1e-9) == _lib.GNR_ERR_ARG and 'approach must be finite and >= 0' in text()
    assert rows(opening=math.nan) == _lib.GNR_ERR_ARG and 'opening must be finite' in text()
    assert rows(spacing=1e-3) == _lib.GNR_ERR_ARG and 'GNR_HAND_MAX_SAMPLES' in text() and str(_lib.GNR_HAND_MAX_SAMPLES) in text()


def test_refusals_before_the_device():
    one = C.c_void_p(16)
    _refusals({k: one for k in OBJ_NAMES}, {k: one for k in ROW_NAMES}, one, 1 << 30)


# ---- GPU: the bits of the statement ---------------------------------------------------------------------------------------------------
SENTINEL = 0x5a


@functools.lru_cache(maxsize=None)
def _ops():
    return objects.VolumeObjects(), objects.GraspObjects()


def _host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if torch.is_tensor(v)}


def _check(what, vol, **params):
    """VolumeObjects on vol [B,R,R,R] with cleaned=True against the statement; -> the statement."""
    want = oref.objects(vol, **params)
    got = _host(_ops()[0](vol, cleaned=True, **params))
    assert got['status'][0] == 0, what
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=(k == 'cleaned')), \
            (what, k, int((got[k] != want[k]).sum()), got['count'], want['count'])
    return want


def _random(R, density, seed):
    return np.where(np.random.default_rng(seed).random((R, R, R)) < density, -1.0, 1.0).astype(f32)


@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 3, 5, 8, 33, 40, 64])
def test_random_solids(R):
    """Densities 0.2 / 0.5 / 0.8 as the three scenes of one call (in three orders), each connectivity; every statistics row at the
    small sizes, the first 4 096 at the large ones."""
    scenes = [_random(R, d, 100 * R + n) for n, d in enumerate((0.2, 0.5, 0.8))]
    for shift, conn in enumerate((6, 18, 26)):
        vol = np.stack(scenes[shift:] + scenes[:shift])
        want = _check((R, conn), vol, connectivity=conn, max_objects=4096, min_voxels=3)
        if R == 64:
            assert want['count'].max() > 4096 or conn != 6, 'no scene with more objects than rows'


@pytest.mark.gpu
def test_rows_and_scenes_do_not_wrap():
    """Solid pairs (i, j, R-1) / (i, j+1, 0) and (i, R-1, R-1) / (i+1, 0, 0) are next to each other in memory and no neighbours; nor are
    the last voxel of a scene and the first of the next."""
    for R in (2, 5, 9):
        a, b = np.ones((R, R, R), f32), np.ones((R, R, R), f32)
        i2 = min(2, R - 2)
        a[0, 0, R - 1] = a[0, 1, 0] = a[i2, R - 1, R - 1] = a[i2 + 1, 0, 0] = a[R - 1, R - 1, R - 1] = -1.0
        b[0, 0, 0] = b[i2, 0, R - 1] = b[i2, 1, 0] = -1.0
        for conn in (6, 18, 26):
            want = _check(('wrap', R, conn), np.stack([a, b]), connectivity=conn)
            if R > 2:                                                          # (at R = 2 every voxel is a 26-neighbour of every other)
                assert list(want['count']) == [5, 3] and (want['voxels'][:, :3] == 1).all(), (R, conn, want['count'])


def serpentine(R):
    """One 6-connected path (R odd): rows along k at even (i, j), joined by single voxels at alternating ends; k runs backwards in every
    other row and j in every other plane, so the linear index is not monotone along the path.  -> (vol, the path's voxels in order)."""
    path, k_dir, j_dir = [], 1, 1
    for i in range(0, R, 2):
        js = list(range(0, R, 2))[::j_dir]
        for n, j in enumerate(js):
            ks = list(range(R))[::k_dir]
            path += [(i, j, k) for k in ks]
            k_dir = -k_dir
            if n < len(js) - 1:
                path.append((i, j + j_dir, ks[-1]))
        j_dir = -j_dir
        if i + 2 < R:
            path.append((i + 1, js[-1], ks[-1]))
    vol = np.ones((R, R, R), f32)
    vol[tuple(np.array(path).T)] = -1.0
    return vol, path


def u_shapes(R):
    """U-shapes whose two arms meet only at their highest index: arms along i joined at the largest i, arms along k joined at the
    largest k, of several lengths; -> (vol, their number)."""
    vol, n = np.ones((R, R, R), f32), 0
    for j0 in range(0, R - 2, 4):                                              # arms along i at (.., j0, k0) and (.., j0 + 2, k0)
        m = 1 + (j0 * 7) % (R - 1)
        vol[0:m + 1, j0, 0] = vol[0:m + 1, j0 + 2, 0] = vol[m, j0 + 1, 0] = -1.0
        n += 1
    for i0 in range(0, R, 2):                                                  # arms along k in the planes i0, away from the first family (k >= 2)
        for j0 in range(0, R - 2, 4):
            m = 3 + (i0 * 5 + j0) % (R - 3)
            vol[i0, j0, 2:m + 1] = vol[i0, j0 + 2, 2:m + 1] = vol[i0, j0 + 1, m] = -1.0
            n += 1
    return vol, n


def comb(R, plate):
    """Teeth along k at even (i, j), k < R-1; the base plate is the layer k = R-1: the teeth's highest indices."""
    vol = np.ones((R, R, R), f32)
    vol[0::2, 0::2, :R - 1] = -1.0
    if plate:
        vol[:, :, R - 1] = -1.0
    return vol


@pytest.mark.gpu
@pytest.mark.parametrize('R', [9, 33])
def test_shapes_that_break_a_parallel_union(R):
    vol, path = serpentine(R)
    assert len(path) == len(set(path)) >= R ** 3 / 4 and all(sum(abs(a - b) for a, b in zip(p, q)) == 1 for p, q in zip(path, path[1:]))
    lin = [(i * R + j) * R + k for i, j, k in path]
    assert sum(a > b for a, b in zip(lin, lin[1:])) > len(lin) // 4, 'the linear index is monotone along the path'
    us, n_us = u_shapes(R)
    teeth = ((R + 1) // 2) ** 2
    want = _check(('serpentine, u-shapes, comb', R), np.stack([vol, us, comb(R, True), comb(R, False)]))
    assert list(want['count']) == [1, n_us, 1, teeth] and want['voxels'][0, 0] == len(path)
    # the path alone, under every connectivity (its rows are two apart: no diagonal joins anything new)
    for conn in (18, 26):
        assert _check(('serpentine', R, conn), vol[None], connectivity=conn)['count'][0] == 1
    # the 3-D checkerboard: under 6 every solid voxel is an object -- more than the rows --, under 26 they are one
    i = np.arange(R)
    board = np.where((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0, -1.0, 1.0).astype(f32)
    most = 64
    want = _check(('checkerboard', R, 6), np.stack([board, -board]), connectivity=6, max_objects=most, min_voxels=2)
    assert list(want['count']) == [(R ** 3 + 1) // 2, R ** 3 // 2] and want['labels'].max() == (R ** 3 + 1) // 2
    assert (want['voxels'] == 1).all() and (want['cleaned'] == 1.0).all(), '`cleaned` is right beyond max_objects'
    want = _check(('checkerboard', R, 26), np.stack([board, -board]), connectivity=26, max_objects=most, min_voxels=2)
    assert list(want['count']) == [1, 1] and np.array_equal(want['cleaned'], np.stack([board, -board]))
    # all solid, all free, NaNs (not solid)
    holes = _random(R, 0.6, R)
    holes[np.random.default_rng(R).random((R, R, R)) < 0.1] = np.nan
    want = _check(('solid, free, NaN', R), np.stack([np.full((R, R, R), -1.0, f32), np.ones((R, R, R), f32), holes]), max_objects=8192)
    assert want['count'][0] == 1 and want['voxels'][0, 0] == R ** 3 and want['count'][1] == 0 and not want['labels'][1].any()
    assert list(want['bbox'][0, 0]) == [0, 0, 0, R - 1, R - 1, R - 1] and list(want['sums'][0, 0]) == [R * R * R * (R - 1) // 2] * 3
    assert not want['labels'][2][np.isnan(holes)].any() and np.isnan(want['cleaned'][2]).sum() == np.isnan(holes).sum()


@pytest.mark.gpu
def test_parameters_on_and_off():
    """z_min, lower and min_voxels each on and off, on values spread over (-1, 1); cleaned=False returns no copy and the same rest."""
    R = 33
    vol = np.random.default_rng(4).uniform(-1, 1, (2, R, R, R)).astype(f32)
    vol[1] = np.where(vol[1] < 0.3, vol[1], 1.0)
    base = None
    for kw in (dict(), dict(z_min=5), dict(lower=-0.5), dict(min_voxels=4), dict(z_min=R), dict(level=0.25, lower=-1.0, z_min=2, min_voxels=2, connectivity=18)):
        want = _check(kw, vol, max_objects=8192, **kw)
        base = want if base is None else base
        if kw in (dict(z_min=5), dict(lower=-0.5)):
            assert not np.array_equal(want['labels'], base['labels'])
        if kw == dict(min_voxels=4):
            assert np.array_equal(want['labels'], base['labels']) and (want['cleaned'] != base['cleaned']).any() and np.array_equal(base['cleaned'], vol)
        if kw == dict(z_min=R):
            assert not want['count'].any()
    op = _ops()[0]
    res = op(vol, max_objects=8192, cleaned=False)
    assert 'cleaned' not in res
    got = _host(res)
    assert all(np.array_equal(got[k], base[k]) for k in KEYS[:-1])
    ptrs = {k: v.data_ptr() for k, v in res.items() if torch.is_tensor(v)}
    again = op(torch.from_numpy(vol).to('cuda:0'), max_objects=8192)
    assert {k: v.data_ptr() for k, v in again.items() if torch.is_tensor(v)} == ptrs, 'the buffers of a shape are kept'
    with pytest.raises(ValueError, match='z_min must be in 0..R'):
        op(vol, z_min=R + 1)
    with pytest.raises(ValueError, match='vol must be'):
        op(vol[:, :, :, :5])


def _raw_objects(vol, ws, cleaned=True, **params):
    """The C call on sentinel-filled outputs and the workspace given -> dict of numpy arrays."""
    L = _lib.lib()
    B, R = vol.shape[0], vol.shape[-1]
    p = _params(**params)
    M = p.max_objects
    fill = lambda n, dtype: torch.full((n * (8 if dtype == torch.int64 else 4),), SENTINEL, dtype=torch.uint8, device='cuda:0').view(dtype)
    out = dict(labels=fill(B * R ** 3, torch.int32), count=fill(B, torch.int32), voxels=fill(B * M, torch.int32), bbox=fill(B * M * 6, torch.int32),
               sums=fill(B * M * 3, torch.int64), cleaned=fill(B * R ** 3, torch.float32))
    dev = torch.from_numpy(vol).to('cuda:0')
    rc = L.gnr_volume_objects_fwd(C.byref(p), dev.data_ptr(), B, R, *(out[k].data_ptr() for k in KEYS[:-1]), out['cleaned'].data_ptr() if cleaned else None,
                                  ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'gnr_volume_objects_fwd')
    torch.cuda.synchronize()
    shapes = dict(labels=(B, R, R, R), count=(B,), voxels=(B, M), bbox=(B, M, 6), sums=(B, M, 3), cleaned=(B, R, R, R))
    return {k: v.cpu().numpy().reshape(shapes[k]) for k, v in out.items()}


@pytest.mark.gpu
def test_nothing_is_kept_in_the_workspace():
    """Repeated calls on one workspace filled with 0x00 / 0xff / 0x71 before each: the same bits, the statement's; without `cleaned`
    that buffer keeps its bytes."""
    R = 9
    vol = np.stack([_random(R, 0.5, 1), serpentine(R)[0], _random(R, 0.3, 2)])
    want = oref.objects(vol, connectivity=18, max_objects=16, min_voxels=2)
    need = _lib.lib().gnr_volume_objects_workspace_bytes(3, R)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    for byte in (0x00, 0xff, 0x71, 0x71):
        ws.fill_(byte)
        got = _raw_objects(vol, ws, connectivity=18, max_objects=16, min_voxels=2)
        assert all(np.array_equal(got[k], want[k]) for k in KEYS), byte
        assert ws[:4].view(torch.int32).item() == 0
    got = _raw_objects(vol, ws, cleaned=False, connectivity=18, max_objects=16, min_voxels=2)
    assert all(np.array_equal(got[k], want[k]) for k in KEYS[:-1]) and (got['cleaned'].view(np.uint8) == SENTINEL).all()


def _grasp_rows(lab, pos, quat, width, count, scale, top_k=None, **kw):
    """GraspObjects on one scene's rows against the statement, on buffers pre-filled with a sentinel."""
    op = _ops()[1]
    n = len(pos)
    count_t = torch.tensor([count], dtype=torch.int32, device='cuda:0')
    args = (torch.from_numpy(lab[None]).to('cuda:0'), pos[None], quat[None], width[None], count_t)
    for t in op(*args, scale=scale, top_k=top_k, **kw).values():
        t.fill_(0x5a5a5a5a)
    got = _host(op(*args, scale=scale, top_k=top_k, **kw))
    want = oref.grasp_objects(lab, pos, quat, width, count, scale, top_k=top_k, out=tuple(np.full(n, 0x5a5a5a5a, np.int32) for _ in range(4)), **kw)
    for k, w in zip(objects.GRASP_OBJECT_ROWS, want):
        assert got[k].dtype == np.int32 and np.array_equal(got[k][0], w), (k, got[k][0][:8], w[:8])
    return want


@pytest.mark.gpu
def test_grasp_objects_equal_the_statement():
    """The three grasps of the module on the slab-and-spheres scene, and 64 seeded poses at R = 40 with the viewer's hand and with a
    2 cm x 1 cm hand opened to 0.08 m; rows beyond min(count, top_k) keep what they held."""
    want = _check('table', np.array(table_scene())[None], z_min=SLAB_TOP + 1)                  # (a writable copy: torch wants one)
    lab = want['labels'][0]
    pos, quat, width = np.stack([g[0] for g in GRASPS]), np.stack([g[1] for g in GRASPS]), f32([g[2] for g in GRASPS])
    rows = _grasp_rows(lab, pos, quat, width, 3, VOXEL)
    assert list(rows[0]) == [1, 1, 0] and list(rows[2]) == [1, 2, 0]
    rng = np.random.default_rng(17)
    # 16 top-down hands between the two spheres, 40 poses anywhere in the lattice, 8 outside it
    pos = np.concatenate([rng.uniform([10, 17, 12], [14, 25, 16], (16, 3)), rng.uniform(2.0, 38.0, (40, 3)), rng.uniform(-30.0, -10.0, (8, 3))])
    pos[:, 2] = np.minimum(pos[:, 2], 24.0)
    quat, width = rng.normal(size=(64, 4)).astype(f32), rng.uniform(1.33, 30.0, 64).astype(f32)
    quat[:16], width[:16] = DOWN, rng.uniform(24.0, 32.0, 16).astype(f32)
    for kw in (dict(), REAL_HAND):
        rows = _grasp_rows(lab, pos, quat, width, 64, VOXEL, **kw)
        assert (rows[0] > 0).sum() > 8 and (rows[2] >= 2).sum() > 0 and (rows[3] == 0).sum() > 0, [list(r[:16]) for r in rows]
    _grasp_rows(lab, pos, quat, width, 40, VOXEL, top_k=9)
    _grasp_rows(lab, pos, quat, width, 0, VOXEL)
    # a label volume where the votes are spread over many labels: every voxel its own object
    own = np.arange(1, 9 ** 3 + 1, dtype=np.int32).reshape(9, 9, 9)
    rng = np.random.default_rng(18)
    rows = _grasp_rows(own, rng.uniform(2.0, 6.0, (6, 3)), rng.normal(size=(6, 4)).astype(f32), rng.uniform(1.0, 6.0, 6).astype(f32), 6, 0.02, depth=0.06)
    assert (rows[2] > 5).all()


@pytest.mark.gpu
def test_objects_of_plan():
    vol = np.array(table_scene())
    g = dict(index=np.stack([p for p, _, _ in GRASPS]).astype(np.int64), quat=np.stack([q for _, q, _ in GRASPS]).astype(f64),
             width=f32([w for _, _, w in GRASPS]) * f32(VOXEL))
    g['pos'] = g['index'].astype(f64) * VOXEL
    obj, cols = objects.objects_of_plan(vol, g, voxel_size=VOXEL, origin=ORIGIN, z_min=SLAB_TOP + 1, min_voxels=2, cleaned=True)
    want = oref.objects(vol[None], z_min=SLAB_TOP + 1, min_voxels=2)
    assert obj['count'] == 3 and np.array_equal(obj['labels'], want['labels'][0]) and np.array_equal(obj['cleaned'], want['cleaned'][0])
    assert np.array_equal(obj['voxels'], want['voxels'][0, :3]) and list(obj['kept']) == [True, True, False]
    assert list(cols['object']) == [1, 1, 0] and list(cols['objects_in_hand']) == [1, 2, 0] and objects.best_per_object(cols['object']) == {1: 0}
    w_vox = (g['width'] / f32(VOXEL)).astype(f32)
    for r in range(3):
        assert tuple(int(cols[k][r]) for k in ('object', 'object_votes', 'objects_in_hand', 'object_samples')) == \
            oref.grasp_object(want['labels'][0], g['index'][r].astype(f64), g['quat'][r].astype(f32), w_vox[r], VOXEL)
    none, cols0 = objects.objects_of_plan(vol[None], dict(index=np.zeros((0, 3), np.int64), quat=np.zeros((0, 4)), width=np.zeros(0, f32)), voxel_size=VOXEL)
    assert none['count'] == 2 and all(len(v) == 0 for v in cols0.values())
    with pytest.raises(_lib.GnrError, match='raise max_objects'):
        objects.objects_of_plan(vol, g, voxel_size=VOXEL, z_min=SLAB_TOP + 1, max_objects=2)


@pytest.mark.gpu
def test_one_captured_graph_of_both_operators():
    """Both operators captured once on one stream, replayed on changed input: the bits of the eager calls (and the statement's)."""
    R, n = 17, 12
    rng = np.random.default_rng(23)
    scenes = [np.stack([_random(R, d, s), _random(R, 0.9 - d, s + 1)]) for s, d in ((1, 0.3), (5, 0.6), (9, 0.45))]
    pos, quat, width = rng.uniform(1.0, R - 2.0, (2, n, 3)), rng.normal(size=(2, n, 4)).astype(f32), rng.uniform(1.0, 9.0, (2, n)).astype(f32)
    dev = 'cuda:0'
    vol = torch.from_numpy(scenes[0]).to(dev)
    P, Q, W = (torch.from_numpy(a).to(dev) for a in (pos, quat, width))
    count = torch.tensor([n, n - 5], dtype=torch.int32, device=dev)
    vo, go = objects.VolumeObjects(), objects.GraspObjects()
    kw = dict(connectivity=26, max_objects=512, min_voxels=2, cleaned=True)

    def run(a, b):
        r = a(vol, **kw)
        return r, b(r['labels'], P, Q, W, count, scale=0.02, depth=0.08)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(vo, go)                                                            # sizes the workspace and the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, rows = run(vo, go)
    eager_vo, eager_go = objects.VolumeObjects(), objects.GraspObjects()
    for s in (scenes[1], scenes[2], scenes[1]):
        vol.copy_(torch.from_numpy(s).to(dev))
        torch.cuda.synchronize()
        graph.replay()
        got, got_rows = _host(res), _host(rows)
        e_res, e_rows = run(eager_vo, eager_go)
        e_res, e_rows = _host(e_res), _host(e_rows)
        want = oref.objects(s, **{k: v for k, v in kw.items() if k != 'cleaned'})
        assert got['status'][0] == 0
        for k in KEYS:
            assert np.array_equal(got[k], e_res[k]) and np.array_equal(got[k], want[k]), k
        for b in range(2):
            ref_rows = oref.grasp_objects(want['labels'][b], pos[b], quat[b], width[b], (n, n - 5)[b], 0.02, depth=0.08)
            for k, w in zip(objects.GRASP_OBJECT_ROWS, ref_rows):
                assert np.array_equal(got_rows[k][b], e_rows[k][b]) and np.array_equal(got_rows[k][b], w), (k, b)


@pytest.mark.gpu
def test_a_refused_call_writes_nothing():
    B, R, M, n = 1, 8, 4, 4
    fill = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    sizes = dict(vol=4 * R ** 3, labels=4 * R ** 3, count=4, voxels=4 * M, bbox=24 * M, sums=24 * M, workspace=_lib.lib().gnr_volume_objects_workspace_bytes(B, R))
    bufs = {k: fill(v) for k, v in sizes.items()}
    rsizes = dict(labels=4 * R ** 3, pos=24 * n, quat=16 * n, width=4 * n, count=4, object=4 * n, votes=4 * n, distinct=4 * n, inside=4 * n)
    rbufs = {k: fill(v) for k, v in rsizes.items()}
    cleaned = fill(4 * R ** 3)
    _refusals({k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}, {k: C.c_void_p(v.data_ptr()) for k, v in rbufs.items()},
              C.c_void_p(cleaned.data_ptr()), sizes['workspace'], B=B, R=R, max_n=n)
    torch.cuda.synchronize()
    for k, v in (*bufs.items(), *rbufs.items(), ('cleaned', cleaned)):
        assert bool((v == SENTINEL).all()), k
