"""Distance field of the volume (csrc/gnr_distance.hip, distance.VolumeDistance, distance.distance_of_plan).
tests/distance_reference.py is the statement (scipy's feature transform summed as integers, exhaustive search for the nearest site of
the smallest index, the float64 esdf); every comparison of integers and of esdf is np.array_equal.  Without a GPU: the statement against
its own exhaustive search, the three line passes and their tie rule in numpy, the parameter checks, every refusal of the entry point.
On the GPU: shapes chosen to break a separable transform -- ties, line ends, scene ends, sentinels -- rather than to resemble the
workload."""
import ctypes as C
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, distance, hand, objects
import distance_reference as dref
import hand_reference as href
import objects_reference as oref

f32, f64 = np.float32, np.float64
OUTPUTS = ('d2_solid', 'nearest_solid', 'd2_free', 'nearest_free', 'esdf', 'nearest_label')
VOXEL = 0.3 / 40
DOWN = f32([1.0, 0.0, 0.0, 0.0])                                               # top-down: the fingers point along world -z


def random_volume(R, density, seed):
    return np.where(np.random.default_rng(seed).random((R, R, R)) < density, -1.0, 1.0).astype(f32)


def three_passes(sites):
    """The method of csrc/gnr_distance.hip in numpy: line passes along k, j, i, each min over x' of g[x'] + (x - x')^2 with the smaller
    x' winning a tie (argmin's first), carrying the site.  -> (d2, nearest) with the statement's sentinels."""
    R, inf = sites.shape[0], 1 << 29
    val = np.where(sites, 0, inf).astype(np.int64)
    site = np.where(sites, np.arange(R ** 3).reshape(sites.shape), -1)
    x = np.arange(R)
    for axis in (2, 1, 0):
        v, s = np.moveaxis(val, axis, -1), np.moveaxis(site, axis, -1)
        cand = v[..., None, :] + (x[:, None] - x[None, :]) ** 2                 # [.., x, x']
        arg = cand.argmin(-1)
        val = np.moveaxis(np.take_along_axis(cand, arg[..., None], -1)[..., 0], -1, axis)
        site = np.moveaxis(np.take_along_axis(s, arg, -1), -1, axis)
    return np.where(val >= inf, 3 * R * R, val).astype(np.int32), site.astype(np.int32)


# ---- 1. the statement (no GPU) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [2, 3, 5, 8, 11])
def test_the_reference_equals_its_exhaustive_search(R):
    for n, density in enumerate((0.0, 0.01, 0.1, 0.5, 0.9, 1.0)):
        vol = random_volume(R, density, 10 * R + n)
        s = dref.solid(vol)
        assert s.sum() == (vol < 0).sum() and (density not in (0.0, 1.0) or s.all() == (density == 1.0))
        for sites in (s, ~s):
            d2, some = dref.edt(sites)
            want_d2, want = dref.exhaustive(sites)
            assert d2.dtype == np.int32 and np.array_equal(d2, want_d2), (R, density)
            assert not dref.invalid_nearest(sites, d2, some).any() and not dref.invalid_nearest(sites, d2, want).any(), (R, density)
            assert (want <= some).all(), 'the exhaustive nearest site is the smallest index'
            if not sites.any():
                assert (d2 == 3 * R * R).all() and (want == -1).all()
            else:
                assert d2.max() <= 3 * (R - 1) ** 2 and (d2[sites] == 0).all() and (d2[~sites] > 0).all()
            got_d2, got = three_passes(sites)
            assert np.array_equal(got_d2, want_d2) and np.array_equal(got, want), ('three passes k, j, i with the smaller x\' on a tie', R, density)


def test_esdf_and_nearest_label_of_the_statement():
    vol = np.ones((1, 5, 5, 5), f32)
    vol[0, 2, 2, 2] = -1.0
    want = dref.distance(vol, scale=0.01)
    e = want['esdf'][0]
    assert e.dtype == f32 and e[2, 2, 2] == f32(-0.005) and e[2, 2, 3] == f32(0.005) and e[2, 2, 4] == f32(0.015)
    assert e[0, 0, 0] == f32((math.sqrt(12.0) - 0.5) * 0.01)
    assert dref.distance(vol, scale=1.0, surface_offset=0.0)['esdf'][0, 2, 2, 2] == -1.0
    labels = np.zeros((5, 5, 5), np.int32)
    labels[2, 2, 2] = 7
    assert (dref.nearest_label(labels, want['nearest_solid'][0]) == 7).all()
    assert not dref.nearest_label(labels, np.full((5, 5, 5), -1, np.int32)).any()
    nan = vol.copy()
    nan[0, 0, 0, 0] = np.nan
    assert not dref.solid(nan[0])[0, 0, 0] and not dref.solid(vol[0], z_min=3).any() and not dref.solid(vol[0], lower=-1.0).any()


def test_distance_params():
    assert distance.distance_params(False) is None and distance.distance_params(None) is None
    want = dict(level=0.0, lower=None, z_min=0, surface_offset=0.5, signed=True)
    assert distance.distance_params(True) == want == distance.distance_params({}) == distance.DISTANCE_DEFAULTS
    p = distance.distance_params(dict(z_min=4, lower=-1, surface_offset=0, margin=0.01), margin=0.0)
    assert p == dict(want, z_min=4, lower=-1.0, surface_offset=0.0, margin=0.01) and isinstance(p['lower'], float) and isinstance(p['surface_offset'], float)
    with pytest.raises(TypeError, match='unknown distance parameters'):
        distance.distance_params(dict(iso=0.0))
    for bad, text in ((dict(level=math.nan), 'level must be finite'), (dict(level=math.inf), 'level must be finite'),
                      (dict(lower=math.nan), 'lower must be None'), (dict(z_min=-1), 'z_min must be an integer >= 0'),
                      (dict(z_min=1.5), 'z_min must be an integer'), (dict(surface_offset=-0.1), 'surface_offset must be finite and >= 0'),
                      (dict(surface_offset=math.inf), 'surface_offset must be finite and >= 0'), (dict(signed=1), 'signed must be True or False')):
        with pytest.raises(ValueError, match=text):
            distance.distance_params(bad)
    assert distance.checked_distance(**want) == want
    for bad in (0.0, -1.0, math.nan, math.inf, True):
        with pytest.raises(ValueError, match='scale must be finite and > 0'):
            distance.checked_scale(bad)
    params = inspect.signature(distance.VolumeDistance.__call__).parameters
    assert {k: v.default for k, v in params.items() if k in want} == want and params['scale'].default is inspect.Parameter.empty
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in (*want, 'scale', 'labels'))


def test_host_functions():
    R = 4
    nearest = np.full((2, R, R, R), -1, np.int32)
    nearest[0] = (1 * R + 2) * R + 3
    vec = distance.nearest_vector(nearest, R, 0.5)
    assert vec.shape == (2, R, R, R, 3) and vec.dtype == f64 and np.isnan(vec[1]).all()
    assert np.array_equal(vec[0, 0, 0, 0], [0.5, 1.0, 1.5]) and np.array_equal(vec[0, 1, 2, 3], [0.0, 0.0, 0.0]) and np.array_equal(vec[0, 3, 3, 3], [-1.0, -0.5, 0.0])
    with pytest.raises(ValueError, match='nearest must be'):
        distance.nearest_vector(nearest[:, :, :, :2], R, 0.5)
    want = dref.distance(random_volume(R, 0.3, 1)[None], scale=0.5)
    rows = {k: want[k][0] for k in OUTPUTS[:5]}
    field = distance.distance_from_rows(rows, 0.5)
    assert field['has_solid'] and field['has_free'] and field['scale'] == 0.5 and all(np.array_equal(field[k], rows[k]) for k in rows)
    assert np.array_equal(field['distance_m'], np.sqrt(rows['d2_solid'].astype(f64)) * 0.5) and field['esdf'] is not rows['esdf']
    empty = dref.distance(np.ones((1, R, R, R), f32), scale=0.5)
    field = distance.distance_from_rows({k: empty[k][0] for k in OUTPUTS[:5]}, 0.5)
    assert not field['has_solid'] and field['has_free'] and np.isinf(field['distance_m']).all()
    g = dict(index=np.zeros((0, 3)), quat=np.zeros((0, 4)), width=np.zeros(0))
    with pytest.raises(TypeError, match='unknown distance parameters'):
        distance.distance_of_plan(np.ones((R, R, R), f32), g, iso=0.0)
    with pytest.raises(ValueError, match='signed must be True'):
        distance.distance_of_plan(np.ones((R, R, R), f32), g, signed=False)
    with pytest.raises(ValueError, match='margin must be finite'):
        distance.distance_of_plan(np.ones((R, R, R), f32), g, margin=math.nan)


def test_volume_distance_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        distance.VolumeDistance()


# ---- 2. the refusals of the entry point -----------------------------------------------------------------------------------------------
PTR_NAMES = ('vol', 'labels', 'd2_solid', 'nearest_solid', 'd2_free', 'nearest_free', 'esdf', 'nearest_label', 'workspace')
REQUIRED = ('vol', 'd2_solid', 'nearest_solid', 'workspace')


def _params(**kw):
    return _lib.GnrDistanceParams(**{**dict(level=0.0, lower=-math.inf, scale=0.0075, surface_offset=0.5, z_min=0), **kw})


def _refusals(ptr, ws_bytes, B=1, R=8):
    """Every refusal of gnr_volume_distance_fwd, each with its code and its text, on the pointers given (fake ones, or buffers whose
    bytes the caller checks afterwards)."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_volume_distance_fwd'
    need = L.gnr_volume_distance_workspace_bytes(B, R)
    assert need >= 6 * 4 * B * R ** 3 and ws_bytes >= need
    assert L.gnr_volume_distance_workspace_bytes(0, R) == 0 and L.gnr_volume_distance_workspace_bytes(B, 1) == 0
    assert L.gnr_volume_distance_workspace_bytes(B, 257) == 0 and L.gnr_volume_distance_workspace_bytes(65536, R) == 0

    def call(B=B, R=R, ws=ws_bytes, p=None, **kw):
        p = _params(**{k: v for k, v in kw.items() if k not in PTR_NAMES}) if p is None else p
        a = {**ptr, **{k: v for k, v in kw.items() if k in PTR_NAMES}}
        return L.gnr_volume_distance_fwd(C.byref(p) if p is not False else None, a['vol'], a['labels'], B, R, a['d2_solid'], a['nearest_solid'],
                                         a['d2_free'], a['nearest_free'], a['esdf'], a['nearest_label'], a['workspace'], ws, None)

    for name in REQUIRED:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_ARG and text() == fn + ': B must be in 1..65535', b
    for r in (1, 0, 257):
        assert call(R=r) == _lib.GNR_ERR_ARG and text() == fn + ': R must be in 2..256', r
    for z in (-1, R + 1):
        assert call(z_min=z) == _lib.GNR_ERR_ARG and text() == fn + ': z_min must be in 0..R', z
    for bad in (math.nan, math.inf, -math.inf):
        assert call(level=bad) == _lib.GNR_ERR_ARG and text() == fn + ': level must be finite', bad
    assert call(lower=math.nan) == _lib.GNR_ERR_ARG and 'lower must not be a NaN' in text()
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert call(scale=bad) == _lib.GNR_ERR_ARG and text() == fn + ': scale must be finite and > 0', bad
    for bad in (-1e-9, math.nan, math.inf):
        assert call(surface_offset=bad) == _lib.GNR_ERR_ARG and text() == fn + ': surface_offset must be finite and >= 0', bad
    assert call(labels=None) == _lib.GNR_ERR_ARG and text() == fn + ': nearest_label needs labels'
    for name in ('d2_free', 'nearest_free'):
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': d2_free and nearest_free go together', name
    for ws in (0, need - 1):
        assert call(ws=ws) == _lib.GNR_ERR_WORKSPACE and text() == fn + ': workspace too small', ws


def test_refusals_before_the_device():
    one = C.c_void_p(16)
    _refusals({k: one for k in PTR_NAMES}, 1 << 30)


# ---- GPU: the bits of the statement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op():
    return distance.VolumeDistance()


def _host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(what, name, got, want):
    """np.array_equal, naming the output, the scene and the voxel that differs first."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(a) for a in np.argwhere(got != want)[0])
        pytest.fail(f'{what}: {name} differs at {int((got != want).sum())} voxels, first in scene {at[0]} at voxel {at[1:]}: {got[at]!r}, not {want[at]!r}')


def check(what, vol, scale=1.0, labels=None, op=None, **params):
    """VolumeDistance (signed) on vol [B,R,R,R] against the statement: d2 and esdf bit for bit, the nearest sites valid everywhere and,
    for R <= 12, the smallest index; nearest_label from the nearest sites found.  -> (the device's arrays, the statement)."""
    vol = np.asarray(vol, f32)
    want = dref.distance(vol, scale=scale, **params)
    got = _host((op or _op())(vol, scale=scale, labels=labels, **params))
    assert sorted(got) == sorted(OUTPUTS[:5] + (OUTPUTS[5:] if labels is not None else ()))
    for k in ('d2_solid', 'd2_free', 'esdf'):
        same(what, k, got[k], want[k])
    for kind, sites in (('solid', want['solid']), ('free', ~want['solid'])):
        bad = np.stack([dref.invalid_nearest(s, d, n) for s, d, n in zip(sites, got['d2_' + kind], got['nearest_' + kind])])
        same(what, f'nearest_{kind} (in range, a {kind} voxel of its scene, at distance d2)', bad, np.zeros_like(bad))
        if 'nearest_' + kind in want:
            same(what, 'nearest_' + kind, got['nearest_' + kind], want['nearest_' + kind])
    if labels is not None:
        same(what, 'nearest_label', got['nearest_label'], np.stack([dref.nearest_label(l, n) for l, n in zip(np.asarray(labels), got['nearest_solid'])]))
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 3, 5, 8, 33, 40, 64, 65, 130])
def test_random_solids(R):
    """Three scenes of densities 0.002 / 0.1 / 0.9 in one call; 65 and 130 are the first line lengths past one and two wavefronts."""
    vol = np.stack([random_volume(R, d, 100 * R + n) for n, d in enumerate((0.002, 0.1, 0.9))])
    got, want = check(('random', R), vol)
    assert R < 8 or (want['solid'].reshape(3, -1).any(1).all() and not want['solid'].reshape(3, -1).all(1).any())
    unsigned = _host(_op()(vol, scale=1.0, signed=False))
    assert sorted(unsigned) == ['d2_solid', 'nearest_solid'] and all(np.array_equal(unsigned[k], got[k]) for k in unsigned)


@pytest.mark.gpu
def test_ties_go_to_the_smaller_index():
    R, c = 9, 4
    scenes, names = [], []

    def add(name, voxels):
        v = np.ones((R, R, R), f32)
        v[tuple(np.array(voxels).T)] = -1.0
        scenes.append(v)
        names.append(name)

    for axis in range(3):                                                      # two voxels mirrored about the centre along an axis
        a, b = [c, c, c], [c, c, c]
        a[axis], b[axis] = 1, 7
        add(f'mirror along axis {axis}', [a, b])
    for a, b in (((1, 1, c), (7, 7, c)), ((1, 7, c), (7, 1, c)), ((1, c, 1), (7, c, 7)), ((1, c, 7), (7, c, 1)), ((c, 1, 1), (c, 7, 7)), ((c, 1, 7), (c, 7, 1))):
        add(f'face diagonal {a} {b}', [a, b])
    for a, b in (((1, 1, 1), (7, 7, 7)), ((1, 7, 1), (7, 1, 7)), ((7, 1, 1), (1, 7, 7)), ((1, 1, 7), (7, 7, 1))):
        add(f'body diagonal {a} {b}', [a, b])
    for axis in range(3):                                                      # a full plane: every voxel off it is nearest to one voxel of it;
        v = np.ones((R, R, R), f32)                                            # two planes: the voxels between them tie
        v[(slice(None),) * axis + (2,)] = v[(slice(None),) * axis + (6,)] = -1.0
        scenes.append(v)
        names.append(f'planes across axis {axis}')
    i = np.arange(R)
    board = np.where((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0, -1.0, 1.0).astype(f32)
    scenes += [board, -board]
    names += ['checkerboard', 'checkerboard, inverted']
    got, want = check('ties', np.stack(scenes))
    for b, name in enumerate(names[:13]):                                      # the voxels of the mirror plane through the centre are nearest to both:
        two = np.flatnonzero(want['solid'][b].ravel())                         # the smaller index must win
        centre = got['nearest_solid'][b, c, c, c]
        assert centre == two.min() and (got['nearest_solid'][b] == two.max()).any(), name
    assert names[13] == 'planes across axis 0' and got['nearest_solid'][13, 4, 0, 0] == (2 * R + 0) * R + 0, 'between two planes: the plane of the smaller index'


@pytest.mark.gpu
def test_lines_planes_and_scenes_do_not_wrap():
    """One solid voxel at the last voxel of scene 0 and one at the first of scene 1; one at k = R-1 of a single row: the distances of the
    row, the plane and the scene behind it in memory must not see it."""
    R = 5
    vol = np.ones((4, R, R, R), f32)
    vol[0, R - 1, R - 1, R - 1] = vol[1, 0, 0, 0] = vol[2, 1, 2, R - 1] = vol[3, 2, R - 1, R - 1] = -1.0
    got, _ = check('wrap', vol)
    assert got['d2_solid'][0, 0, 0, 0] == 3 * (R - 1) ** 2 == got['d2_solid'][1, R - 1, R - 1, R - 1]
    assert got['d2_solid'][2, 1, 3, 0] == 1 + (R - 1) ** 2 and got['d2_solid'][3, 3, 0, 0] == 1 + 2 * (R - 1) ** 2
    assert (got['nearest_solid'][0] == R ** 3 - 1).all() and (got['nearest_solid'][1] == 0).all()


@pytest.mark.gpu
def test_sentinels_of_empty_and_full_scenes():
    R = 6
    vol = np.stack([np.ones((R, R, R), f32), np.full((R, R, R), -1.0, f32), random_volume(R, 0.3, 5)])
    got, _ = check('sentinels', vol)
    assert (got['d2_solid'][0] == 3 * R * R).all() and (got['nearest_solid'][0] == -1).all() and not got['d2_free'][0].any()
    assert (got['d2_free'][1] == 3 * R * R).all() and (got['nearest_free'][1] == -1).all() and not got['d2_solid'][1].any()
    assert np.array_equal(got['nearest_free'][0].ravel(), np.arange(R ** 3)) and np.array_equal(got['nearest_solid'][1].ravel(), np.arange(R ** 3))
    big = f32((math.sqrt(3.0 * R * R) - 0.5) * 1.0)
    assert (got['esdf'][0] == big).all() and (got['esdf'][1] == -big).all()
    labels = np.arange(1, 3 * R ** 3 + 1, dtype=np.int32).reshape(3, R, R, R)
    got, _ = check('sentinels with labels', vol, labels=labels)
    assert not got['nearest_label'][0].any() and np.array_equal(got['nearest_label'][1], labels[1])


@pytest.mark.gpu
def test_the_solid_rule():
    """NaNs, a lower bound, z_min in {0, 3, R}, values equal to the level and to the lower bound (neither is solid)."""
    R = 8
    rng = np.random.default_rng(8)
    vol = rng.uniform(-1, 1, (2, R, R, R)).astype(f32)
    vol[rng.random(vol.shape) < 0.1] = np.nan
    vol[rng.random(vol.shape) < 0.1] = 0.25                                    # == level below
    vol[rng.random(vol.shape) < 0.1] = -0.5                                    # == lower below
    seen = set()
    for z_min in (0, 3, R):
        for kw in (dict(), dict(level=0.25, lower=-0.5)):
            got, want = check(('solid rule', z_min, kw), vol, z_min=z_min, **kw)
            s = want['solid']
            assert not s[np.isnan(vol)].any() and not s[:, :, :, :z_min].any() and (z_min < R or not s.any())
            if kw:
                assert (vol == f32(0.25)).sum() > 50 and (vol == f32(-0.5)).sum() > 50 and not s[vol == f32(0.25)].any() and not s[vol == f32(-0.5)].any()
            seen.add(int(s.sum()))
    assert len(seen) == 5, 'every parameter moves the mask (z_min = R leaves none under both rules)'
    with pytest.raises(ValueError, match='z_min must be in 0..R'):
        _op()(vol, scale=1.0, z_min=R + 1)
    with pytest.raises(ValueError, match='labels must be'):
        _op()(vol, scale=1.0, labels=np.zeros((1, R, R, R), np.int32))


@pytest.mark.gpu
def test_esdf_bits():
    R = 11
    vol = np.stack([random_volume(R, d, 40 + n) for n, d in enumerate((0.03, 0.5))])
    for offset in (0.0, 0.5):
        for scale in (0.0075, 1.0):
            got, want = check(('esdf', offset, scale), vol, scale=scale, surface_offset=offset)
            e, s = got['esdf'], want['solid']
            if offset:
                assert (e[s] < 0).all() and (e[~s] > 0).all() and not (e == 0).any()
                assert (e[s] <= f32(-0.5 * scale)).all() and (e[~s] >= f32(0.5 * scale)).all()
            else:
                assert (e[s] <= f32(-scale)).all() and (e[~s] >= f32(scale)).all()
            # antisymmetry: the inverted mask gives the negated field
            inv, _ = check(('esdf, inverted', offset, scale), -vol, scale=scale, surface_offset=offset)
            assert np.array_equal(inv['esdf'], -e) and np.array_equal(inv['d2_solid'], got['d2_free']) and np.array_equal(inv['nearest_free'], got['nearest_solid'])


def slab_scene(R, seed):
    """[R,R,R]: a slab solid for k < 3 and blobs above it, some standing on it."""
    rng = np.random.default_rng(seed)
    vol = np.ones((R, R, R), f32)
    vol[:, :, :3] = -1.0
    for _ in range(5):
        p, e = rng.integers(0, R - 3, 3), rng.integers(1, 4, 3)
        p[2] = max(p[2], 3 + rng.integers(0, 3))
        vol[p[0]:p[0] + e[0], p[1]:p[1] + e[1], p[2]:p[2] + e[2]] = -1.0
    return vol


@pytest.mark.gpu
def test_nearest_label():
    """The labels cut the slab (z_min = 3), the distance does not: slab voxels are nearest sites that carry label 0."""
    R = 12
    vol = np.stack([slab_scene(R, 3), slab_scene(R, 4)])
    labels = np.stack([oref.label(v, z_min=3)[0] for v in vol])
    assert labels.max() >= 2 and not labels[:, :, :, :3].any()
    got, _ = check('nearest label', vol, labels=labels)
    nl = got['nearest_label']
    assert (nl == 0).any() and (nl > 0).any() and np.array_equal(nl[labels > 0], labels[labels > 0]) and not nl[:, :, :, :3].any()
    dev = objects.VolumeObjects()(vol, z_min=3)['labels']
    again = _host(_op()(vol, scale=1.0, labels=dev))
    assert np.array_equal(dev.cpu().numpy(), labels) and all(np.array_equal(again[k], got[k]) for k in OUTPUTS)


@pytest.mark.gpu
def test_the_largest_volume():
    """R = 256, the bound of R and of the line staging: five solid voxels, one at a corner, two tied for a whole plane of voxels; against
    the direct minimum over the five."""
    R = 256
    sites = [(0, 0, 0), (255, 255, 255), (100, 60, 31), (100, 60, 201), (17, 250, 128)]     # the plane k = 116 ties the middle two
    vol = torch.ones(1, R, R, R, dtype=torch.float32, device='cuda:0')
    for s in sites:
        vol[(0, *s)] = -1.0
    res = _op()(vol, scale=VOXEL)
    torch.cuda.synchronize()
    i = np.arange(R, dtype=np.int32)
    want_d2, want_n = np.full((R, R, R), np.iinfo(np.int32).max, np.int32), np.full((R, R, R), -1, np.int32)
    for s in sorted(sites):                                                    # ascending linear index, strictly smaller replaces
        d = ((i - s[0]) ** 2)[:, None, None] + ((i - s[1]) ** 2)[None, :, None] + ((i - s[2]) ** 2)[None, None, :]
        closer = d < want_d2
        want_d2[closer], want_n[closer] = d[closer], (s[0] * R + s[1]) * R + s[2]
    same('R = 256', 'd2_solid', res['d2_solid'].cpu().numpy(), want_d2[None])
    same('R = 256', 'nearest_solid', res['nearest_solid'].cpu().numpy(), want_n[None])
    assert (want_n[:, :, 116] == (100 * R + 60) * R + 31).sum() > 1000, 'no plane of ties'
    is_solid = want_d2 == 0
    d2_free, own = is_solid.astype(np.int32), np.arange(R ** 3, dtype=np.int32).reshape(R, R, R)
    same('R = 256', 'd2_free', res['d2_free'].cpu().numpy(), d2_free[None])
    got_nf = res['nearest_free'].cpu().numpy()[0]
    assert np.array_equal(got_nf[~is_solid], own[~is_solid])
    for s in sites:                                                            # the free neighbour of the smallest index: -i, then -j, then -k
        nb = next((s[0] - (a == 0), s[1] - (a == 1), s[2] - (a == 2)) for a in range(3) if s[a] > 0) if any(s) else (0, 0, 1)
        assert got_nf[s] == (nb[0] * R + nb[1]) * R + nb[2], s
    same('R = 256', 'esdf', res['esdf'].cpu().numpy(), dref.esdf(is_solid, want_d2, d2_free, VOXEL)[None])


@pytest.mark.gpu
def test_nothing_is_kept_between_calls():
    """One object on (B=3, R=8), (B=1, R=33), (B=3, R=8), its workspace and every output filled with 0x7f bytes before each call: the
    bits of fresh calls; and two runs of one call are equal."""
    op = distance.VolumeDistance()
    vols = [np.stack([random_volume(8, d, n) for n, d in enumerate((0.05, 0.4, 0.8))]), random_volume(33, 0.01, 7)[None],
            np.stack([random_volume(8, d, 10 + n) for n, d in enumerate((0.6, 0.02, 0.3))])]
    labels = [np.random.default_rng(n).integers(0, 9, v.shape).astype(np.int32) for n, v in enumerate(vols)]
    op(vols[1], scale=VOXEL, labels=labels[1])                                # sizes the workspace
    for v, l in zip(vols, labels):
        op._ws.fill_(0x7f)
        for shape_out in op._out.values():
            for t in shape_out.values():
                t.view(torch.uint8).fill_(0x7f)
        got, _ = check(('stale', v.shape), v, scale=VOXEL, labels=l, op=op)
        fresh = _host(distance.VolumeDistance()(v, scale=VOXEL, labels=l))
        twice = _host(op(v, scale=VOXEL, labels=l))
        for k in OUTPUTS:
            same(('stale, against a fresh object', v.shape), k, got[k], fresh[k])
            same(('stale, the same call twice', v.shape), k, twice[k], got[k])
    ptrs = {k: t.data_ptr() for k, t in op(vols[0], scale=VOXEL, labels=labels[0]).items()}
    assert {k: t.data_ptr() for k, t in op(vols[2], scale=VOXEL, labels=labels[2]).items()} == ptrs, 'the buffers of a shape are kept'


# ---- the hand's margin in the field ---------------------------------------------------------------------------------------------------
BALL, RADIUS, TRUNCATION = (20, 20, 14), 5.0, 0.75                             # voxels; the raw volume is clipped 0.75 voxels off a surface
# (index, width in voxels): the hand 1.7 and 4.7 voxels beside the ball, above it, its fingers in it, its tail out of the lattice, all of it out
GRASPS = (((27, 20, 16), 8.0), ((30, 20, 16), 8.0), ((20, 20, 28), 8.0), ((20, 20, 22), 8.0), ((20, 20, 37), 8.0), ((-30, 5, 5), 8.0))


@functools.lru_cache(maxsize=None)
def ball_scene():
    """[40,40,40] float32: a ball of radius 5 voxels over a slab that is solid for k <= 3, as a field clipped 0.75 voxels off the surfaces."""
    i = np.arange(40, dtype=f64)
    I, J, K = np.meshgrid(i, i, i, indexing='ij')
    d = np.minimum(np.sqrt((I - BALL[0]) ** 2 + (J - BALL[1]) ** 2 + (K - BALL[2]) ** 2) - RADIUS, K - 3.5)
    vol = np.clip(d / TRUNCATION, -1.0, 1.0).astype(f32)
    vol.setflags(write=False)
    return vol


@pytest.mark.gpu
def test_hand_clearance_on_the_field_reads_metres():
    vol = np.array(ball_scene())
    n = len(GRASPS)
    pos, quat, width = f64([g[0] for g in GRASPS]), np.tile(DOWN, (n, 1)), f32([g[1] for g in GRASPS])
    got, want = check('ball over a slab', vol[None], scale=VOXEL)
    count = torch.tensor([n], dtype=torch.int32, device='cuda:0')
    hc = hand.HandClearance()
    rows = _host(hc(torch.from_numpy(got['esdf']).to('cuda:0'), pos[None], quat[None], width[None], count, scale=VOXEL))
    ref_rows = dict(zip(hand.HAND_ROW_TYPES, href.clearance_rows(want['esdf'][0], pos, quat, width, n, VOXEL)))
    for k in hand.HAND_ROW_TYPES:
        same('HandClearance on esdf', k, rows[k], ref_rows[k][None])
    raw = _host(hc(vol[None], pos[None], quat[None], width[None], count, scale=VOXEL))['clearance'][0]
    c = ref_rows['clearance']
    print('clearance_m', c[:, 0], 'raw', raw[:, 0])
    near, far, above, touching, tail_out, outside = range(n)
    assert raw[near, 0] == raw[far, 0] == 1.0, 'beyond the truncation the raw volume cannot tell 1.7 voxels from 4.7'
    # the hand's nearest samples are 0.27 voxels off its index towards the ball, whose last solid voxel along that line is (24, 20, 14)
    assert 0 < c[near, 0] < c[far, 0] < 1.0 and abs(c[near, 0] / VOXEL - (27 - 24.77)) < 0.3 and abs(c[far, 0] / VOXEL - (30 - 24.77)) < 0.3
    assert c[above, 0] > 0 and c[touching, 0] < 0 and raw[touching, 0] < 0
    assert 0 < ref_rows['inside'][tail_out, 0] < ref_rows['inside'][above, 0] and ref_rows['inside'][outside, 1] == 0 and c[outside, 1] == 1.0
    # distance_of_plan: the same columns from what a plan returns, and the object every grasp's voxel is nearest to
    g = dict(index=np.int64([g[0] for g in GRASPS[:5]]), quat=np.tile(DOWN, (5, 1)).astype(f64), width=width[:5] * f32(VOXEL))
    labels = oref.label(vol, z_min=4)[0]
    assert labels.max() == 1 and labels[BALL] == 1
    field, cols = distance.distance_of_plan(vol, g, voxel_size=VOXEL, objects=dict(labels=labels), margin=0.02)
    for k in OUTPUTS[:5]:
        same('distance_of_plan', k, field[k][None], got[k])
    assert np.array_equal(cols['clearance_m'], c[:5, 0]) and np.array_equal(cols['approach_clearance_m'], c[:5, 1]) and cols['clearance_m'].dtype == f32
    assert np.array_equal(cols['collision_free_m'], c[:5, 1] > f32(0.02)) and list(cols['collision_free_m'][:4]) == [False, True, True, False]
    assert np.array_equal(cols['hand_inside'], ref_rows['inside'][:5]) and np.array_equal(cols['hand_worst'], ref_rows['worst'][:5])
    at = g['index']
    assert np.array_equal(cols['nearest_object'], dref.nearest_label(labels, got['nearest_solid'][0])[at[:, 0], at[:, 1], at[:, 2]])
    assert list(cols['nearest_object']) == [1, 1, 1, 1, 1] and field['nearest_label'][20, 20, 5] == 0
    none, cols0 = distance.distance_of_plan(vol[None], dict(index=np.zeros((0, 3), np.int64), quat=np.zeros((0, 4)), width=np.zeros(0, f32)), voxel_size=VOXEL)
    assert np.array_equal(none['esdf'], got['esdf'][0]) and all(len(v) == 0 for v in cols0.values()) and 'nearest_object' not in cols0


@pytest.mark.gpu
def test_one_captured_graph_with_the_hand_behind_it():
    """VolumeDistance (signed, with labels) and HandClearance on its esdf captured once on one stream, replayed on changed input: the
    bits of the eager calls and of the statement."""
    R, n, dev = 17, 6, 'cuda:0'
    rng = np.random.default_rng(31)
    scenes = [np.stack([random_volume(R, d, s), random_volume(R, 0.5 - d, s + 1)]) for s, d in ((1, 0.05), (5, 0.3), (9, 0.45))]
    scene_labels = [rng.integers(0, 5, s.shape).astype(np.int32) for s in scenes]
    pos, quat, width = rng.uniform(1.0, R - 2.0, (2, n, 3)), rng.normal(size=(2, n, 4)).astype(f32), rng.uniform(1.0, 6.0, (2, n)).astype(f32)
    vol, labels = torch.from_numpy(scenes[0]).to(dev), torch.from_numpy(scene_labels[0]).to(dev)
    P, Q, W = (torch.from_numpy(a).to(dev) for a in (pos, quat, width))
    count = torch.tensor([n, n - 2], dtype=torch.int32, device=dev)

    def run(a, b):
        r = a(vol, scale=0.02, labels=labels, z_min=1)
        return r, b(r['esdf'], P, Q, W, count, scale=0.02, depth=0.08)

    vd, hc = distance.VolumeDistance(), hand.HandClearance()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(vd, hc)                                                            # sizes the workspace and the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, rows = run(vd, hc)
    eager = distance.VolumeDistance(), hand.HandClearance()
    for s, l in ((scenes[1], scene_labels[1]), (scenes[2], scene_labels[2])):
        vol.copy_(torch.from_numpy(s).to(dev))
        labels.copy_(torch.from_numpy(l).to(dev))
        torch.cuda.synchronize()
        graph.replay()
        got, got_rows = _host(res), _host(rows)
        e_res, e_rows = run(*eager)
        e_res, e_rows = _host(e_res), _host(e_rows)
        want = dref.distance(s, scale=0.02, z_min=1)
        for k in OUTPUTS:
            same('replay against the eager call', k, got[k], e_res[k])
        for k in ('d2_solid', 'd2_free', 'esdf'):
            same('replay against the statement', k, got[k], want[k])
        for b in range(2):
            ref_rows = href.clearance_rows(want['esdf'][b], pos[b], quat[b], width[b], (n, n - 2)[b], 0.02, depth=0.08)
            for k, w in zip(hand.HAND_ROW_TYPES, ref_rows):
                assert np.array_equal(got_rows[k][b], e_rows[k][b]) and np.array_equal(got_rows[k][b][:(n, n - 2)[b]], w[:(n, n - 2)[b]]), (k, b)


@pytest.mark.gpu
def test_a_refused_call_writes_nothing():
    B, R, fill_byte = 1, 8, 0x5a
    fill = lambda nbytes: torch.full((nbytes,), fill_byte, dtype=torch.uint8, device='cuda:0')
    sizes = {k: 4 * B * R ** 3 for k in PTR_NAMES}
    sizes['workspace'] = _lib.lib().gnr_volume_distance_workspace_bytes(B, R)
    bufs = {k: fill(v) for k, v in sizes.items()}
    _refusals({k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}, sizes['workspace'], B=B, R=R)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == fill_byte).all()), k
