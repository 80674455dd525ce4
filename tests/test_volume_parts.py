"""Parts of the volume (csrc/gnr_parts.hip, parts.VolumeParts, parts.parts_of_plan).  tests/parts_reference.py is the statement (numpy
integers, one float64 multiply and compare); every comparison is np.array_equal, dtypes included.  Without a GPU: the statement
against a literal restatement voxel by voxel, its two consequences (neck = 0 is the connected components, a plateau is one part), the
synthetic shapes the default neck was chosen on, the parameter checks, every refusal of the entry point.  On the GPU: shapes chosen to
break a parallel watershed -- ties, long walks, long chains of joins, lattice ends -- rather than to resemble the workload, then the
distance field of touching shapes, a plan's route and a captured graph."""
import ctypes as C
import functools
import inspect
import itertools
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, distance, objects, parts
import objects_reference as oref
import parts_reference as pref

f32, f64 = np.float32, np.float64
CONNECTIVITIES, NECKS, MIN_PEAKS = (6, 18, 26), (0.0, 0.5, 0.8, 1.0), (0, 2)
VOXEL = 0.3 / 40
DOWN = f32([1.0, 0.0, 0.0, 0.0])                                               # top-down: the fingers point along world -z, the hand closes along y
SENTINEL = 0x5a


def same(what, got, want, keys=pref.KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, k, int((g != w).sum()), np.asarray(got['count']), np.asarray(want['count']))


def random_fields(R, seed):
    """[3,R,R,R] int32: heights uniform in 0..3 (ties everywhere, a quarter not solid), in 0..1000, and in {0, 7}."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 4, (R, R, R)), rng.integers(0, 1001, (R, R, R)), 7 * rng.integers(0, 2, (R, R, R))]).astype(np.int32)


def mask_volume(mask):
    return np.where(mask, -1.0, 1.0).astype(f32)


# ---- 1. the statement (no GPU) --------------------------------------------------------------------------------------------------------
def restatement(height, connectivity, max_parts, neck, min_peak):
    """include/gnr.h's words one voxel at a time, in plain Python: one scene [R,R,R] -> parts_reference.parts' dict of that scene."""
    R = height.shape[0]
    n = R ** 3
    h = [int(x) for x in height.ravel()]
    order = {6: 1, 18: 2, 26: 3}[connectivity]

    def neighbours(v):
        i, j, k = v // (R * R), (v // R) % R, v % R
        for di, dj, dk in itertools.product((-1, 0, 1), repeat=3):
            if 0 < (di != 0) + (dj != 0) + (dk != 0) <= order and 0 <= i + di < R and 0 <= j + dj < R and 0 <= k + dk < R:
                w = ((i + di) * R + j + dj) * R + k + dk
                if h[w] > 0:
                    yield w

    solid = [v for v in range(n) if h[v] > 0]
    up = {}
    for v in solid:
        best = v
        for w in neighbours(v):
            if h[w] > h[best] or (h[w] == h[best] and w < best):
                best = w
        up[v] = best
    basin = {}
    for v in solid:
        x, links = v, 0
        while up[x] != x:
            x, links = up[x], links + 1
            assert links < n
        basin[v] = x
    summits = sorted(set(basin.values()))
    parent = {s: s for s in summits}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    nn = f64(neck) * f64(neck)
    for u in solid:
        for w in neighbours(u):
            a, b = basin[u], basin[w]
            if a != b:
                low = min(h[a], h[b])
                if low <= min_peak or f64(min(h[u], h[w])) >= nn * f64(low):
                    ra, rb = find(a), find(b)
                    parent[max(ra, rb)] = min(ra, rb)
    members = {}
    for v in solid:                                                            # ascending: a part's first voxel is its smallest
        members.setdefault(find(basin[v]), []).append(v)
    ordered = sorted(members.values(), key=lambda m: m[0])
    out = dict(labels=np.zeros(n, np.int32), count=np.int32(len(ordered)), basins=np.int32(len(summits)), voxels=np.zeros(max_parts, np.int32),
               bbox=np.tile(np.int32([R, R, R, -1, -1, -1]), (max_parts, 1)), sums=np.zeros((max_parts, 3), np.int64),
               peak=np.zeros(max_parts, np.int32), peak_voxel=np.full(max_parts, -1, np.int32))
    for row, m in enumerate(ordered):
        out['labels'][m] = row + 1
        if row < max_parts:
            ijk = np.array([(v // (R * R), (v // R) % R, v % R) for v in m])
            top = max(h[v] for v in m)
            out['voxels'][row], out['bbox'][row], out['sums'][row] = len(m), list(ijk.min(0)) + list(ijk.max(0)), ijk.sum(0)
            out['peak'][row], out['peak_voxel'][row] = top, min(v for v in m if h[v] == top)
    out['labels'] = out['labels'].reshape(R, R, R)
    return out


@pytest.mark.parametrize('R', [2, 3, 5])
def test_the_reference_equals_its_literal_restatement(R):
    fields = random_fields(R, R)
    for conn in CONNECTIVITIES:
        for neck, min_peak in itertools.product(NECKS, MIN_PEAKS):
            M = 5 if R == 5 else 200                                           # (at R = 5 some scenes have more parts than rows)
            want = pref.parts(fields, conn, M, neck, min_peak)
            for b, h in enumerate(fields):
                same((R, conn, neck, min_peak, b), restatement(h, conn, M, neck, min_peak), {k: v[b] for k, v in want.items()})
    assert pref.parts(fields, 6, 5, 1.0, 0)['count'].max() > 5 or R < 5


@pytest.mark.parametrize('conn', CONNECTIVITIES)
def test_without_a_neck_the_parts_are_the_connected_components(conn):
    for R in (3, 8, 13):
        for b, h in enumerate(random_fields(R, 10 + R)):
            lab, count, basins = pref.label(h, conn, neck=0.0)
            want, n = oref.label(mask_volume(h > 0), connectivity=conn)
            assert lab.dtype == np.int32 and np.array_equal(lab, want) and count == n and basins >= count, (R, b)


@pytest.mark.parametrize('neck', [0.5, 1.0])
def test_one_plateau_is_one_part(neck):
    R = 9
    flat = np.full((R, R, R), 4, np.int32)
    for conn in CONNECTIVITIES:
        lab, count, basins = pref.label(flat, conn, neck)
        assert count == 1 and basins == 1 and (lab == 1).all()
        # the components of a {0, 7} field are plateaus: many summits by index, all of one component merge
        h = random_fields(R, 3)[2]
        lab, count, basins = pref.label(h, conn, neck)
        want, n = oref.label(mask_volume(h > 0), connectivity=conn)
        assert np.array_equal(lab, want) and count == n and basins > count


def lattice(R):
    i = np.arange(R, dtype=f64)
    return np.meshgrid(i, i, i, indexing='ij')


def ball(R, centre, radius):
    """The voxels at most `radius` from the centre: two balls of radius r whose centres are 2 r apart along an axis share a voxel."""
    I, J, K = lattice(R)
    return (I - centre[0]) ** 2 + (J - centre[1]) ** 2 + (K - centre[2]) ** 2 <= radius ** 2


def box(R, lo, hi):
    I, J, K = lattice(R)
    return (I >= lo[0]) & (I <= hi[0]) & (J >= lo[1]) & (J <= hi[1]) & (K >= lo[2]) & (K <= hi[2])


def spheres(R, gap, s=1.0):
    """Two balls of radius 7 s with centres gap * s apart along j, the first on a voxel."""
    c, j0 = R // 2, round(14 * s)
    return ball(R, (c, j0, c), 7 * s) | ball(R, (c, j0 + gap * s, c), 7 * s)


def sphere_on_box(R, s=1.0):
    """A box of half-width 8 s that is solid for 3 s <= k <= 10 s, and a ball of radius 6 s resting on it."""
    c, top = R // 2, int(10 * s)
    return box(R, (c - 8 * s, c - 8 * s, int(3 * s)), (c + 8 * s, c + 8 * s, top)) | ball(R, (c, c, top + 6 * s), 6 * s)


def parts_count(mask, neck):
    return pref.label(pref.d2_free(mask_volume(mask)[None])[0], 26, neck, 0)[1]


def test_the_shapes_the_default_neck_was_chosen_on():
    """40^3, connectivity 26, heights from the exact distance transform: what the default neck = 0.8 separates and what it keeps whole."""
    R = 40
    overlapping, touching, resting = spheres(R, 11), spheres(R, 14), sphere_on_box(R)
    assert [parts_count(overlapping, n) for n in (0.7, 0.8)] == [1, 2]
    assert [parts_count(touching, n) for n in (0.5, 0.6, 0.7, 0.8, 0.9)] == [2] * 5
    assert [parts_count(resting, n) for n in (0.7, 0.8)] == [1, 2]
    I, J, K = lattice(R)
    singles = dict(sphere=ball(R, (20, 20, 20), 7), box=box(R, (12, 14, 3), (28, 26, 12)), cylinder=((J - 20) ** 2 + (K - 10) ** 2 < 36) & (abs(I - 20) <= 12),
                   ell=box(R, (8, 8, 3), (30, 16, 11)) | box(R, (8, 8, 3), (16, 30, 11)))
    for name, mask in singles.items():
        assert [parts_count(mask, n) for n in (0.5, 0.8, 0.9)] == [1, 1, 1], name
    three = ball(R, (13, 14, 12), 7) | ball(R, (27, 14, 12), 7) | ball(R, (20, 26, 12), 7)
    assert oref.label(mask_volume(three), connectivity=26)[1] == 1 and parts_count(three, parts.PART_DEFAULTS['neck']) == 3
    # two boxes face to face without a gap are one box
    assert parts_count(box(R, (10, 10, 3), (19, 20, 12)) | box(R, (20, 10, 3), (29, 20, 12)), 0.8) == 1
    # the statistics of the two touching spheres: sizes, peaks and radii of the two parts
    h = pref.d2_free(mask_volume(touching)[None])
    want = pref.parts(h, max_parts=4)
    assert list(want['count']) == [2] and abs(int(want['voxels'][0, 0]) - int(want['voxels'][0, 1])) == 1 and want['voxels'][0, :2].sum() == touching.sum()    # (the voxel they share is one part's)
    assert list(want['peak'][0]) == [50, 50, 0, 0] and list(want['peak_voxel'][0, :2]) == [(20 * R + 14) * R + 20, (20 * R + 28) * R + 20]
    rows = {k: v[0] for k, v in want.items()}
    got = parts.parts_from_rows(dict(rows, count=want['count'], basins=want['basins'], status=np.int32([0])), VOXEL)
    assert got['count'] == 2 and np.array_equal(got['radius'], np.sqrt(f64([50, 50])) * f64(VOXEL)) and got['radius'].dtype == f64
    assert got['basins'] == int(want['basins'][0]) and np.array_equal(got['peak_voxel'], want['peak_voxel'][0, :2]) and list(got['kept']) == [True, True]
    assert np.abs(got['centroid'] / VOXEL - [[20, 14, 20], [20, 28, 20]]).max() < 0.5


def test_part_params_and_host_functions():
    assert parts.part_params(False) is None and parts.part_params(None) is None
    want = dict(connectivity=26, max_parts=1024, neck=0.8, min_peak=0)
    assert parts.part_params(True) == want == parts.part_params({}) == parts.PART_DEFAULTS == parts.checked_parts()
    p = parts.part_params(dict(neck=1, connectivity=6, filter=True), filter=False)
    assert p == dict(want, neck=1.0, connectivity=6, filter=True) and isinstance(p['neck'], float)
    with pytest.raises(TypeError, match='unknown parts parameters'):
        parts.part_params(dict(iso=0.0))
    for bad, text in ((dict(connectivity=8), 'parts connectivity must be 6, 18 or 26, got 8'), (dict(connectivity=True), 'parts connectivity must be 6, 18 or 26'),
                      (dict(max_parts=0), 'parts max_parts must be an integer >= 1, got 0'), (dict(max_parts=2.5), 'parts max_parts must be an integer >= 1'),
                      (dict(neck=1.5), 'parts neck must be finite and in 0..1'), (dict(neck=math.nan), 'parts neck must be finite and in 0..1'),
                      (dict(neck=-0.1), 'parts neck must be finite and in 0..1'), (dict(min_peak=-1), 'parts min_peak must be an integer >= 0, got -1'),
                      (dict(min_peak=0.5), 'parts min_peak must be an integer >= 0')):
        with pytest.raises(ValueError, match=text):
            parts.part_params(bad)
    params = inspect.signature(parts.VolumeParts.__call__).parameters
    assert {k: v.default for k, v in params.items() if k in want} == want and all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
    rows = dict(count=np.int32([5]), basins=np.int32([9]), voxels=np.int32([3, 2, 1]), bbox=np.zeros((3, 6), np.int32), sums=np.zeros((3, 3), np.int64),
                peak=np.int32([4, 9, 1]), peak_voxel=np.int32([0, 5, 7]))
    with pytest.raises(_lib.GnrError, match='5 parts but the buffers hold 3: raise max_parts'):
        parts.parts_from_rows(rows, VOXEL)
    with pytest.raises(_lib.GnrError, match='GNR_PARTS_STATUS_BOUND'):
        parts.parts_from_rows(dict(rows, count=np.int32([3]), status=np.int32([_lib.GNR_PARTS_STATUS_BOUND])), VOXEL)
    o = parts.parts_from_rows(dict(rows, count=np.int32([2])), 0.5, (1.0, 2.0, 3.0))
    assert o['count'] == 2 and o['basins'] == 9 and list(o['peak']) == [4, 9] and list(o['radius']) == [1.0, 1.5] and list(o['peak_voxel']) == [0, 5]
    assert np.array_equal(o['centroid'], [[1.0, 2.0, 3.0]] * 2)
    cols = parts.grasp_parts_from_rows(dict(object=np.int32([1]), votes=np.int32([7]), distinct=np.int32([2]), inside=np.int32([9])))
    assert {k: int(v[0]) for k, v in cols.items()} == dict(part=1, part_votes=7, parts_in_hand=2, part_samples=9)
    g = dict(index=np.zeros((0, 3)), quat=np.zeros((0, 4)), width=np.zeros(0))
    with pytest.raises(TypeError, match='unknown parts parameters'):
        parts.parts_of_plan(np.ones((4, 4, 4), f32), g, iso=0.0)
    with pytest.raises(ValueError, match='parts neck must be finite and in 0..1'):
        parts.parts_of_plan(np.ones((4, 4, 4), f32), g, neck=2.0)
    with pytest.raises(ValueError, match='parts z_min must be an integer >= 0'):
        parts.parts_of_plan(np.ones((4, 4, 4), f32), g, z_min=-1)


def test_volume_parts_need_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        parts.VolumeParts()


# ---- 2. the refusals of the entry point -----------------------------------------------------------------------------------------------
PTR_NAMES = ('height', 'labels', 'count', 'basins', 'voxels', 'bbox', 'sums', 'peak', 'peak_voxel', 'workspace')


def _params(**kw):
    return _lib.GnrPartsParams(**{**dict(neck=0.8, connectivity=26, max_parts=4, min_peak=0), **kw})


def _refusals(ptr, ws_bytes, B=1, R=8):
    """Every refusal of gnr_volume_parts_fwd, each with its code and its text, on the pointers given (fake ones, or buffers whose bytes
    the caller checks afterwards)."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_volume_parts_fwd'
    need = L.gnr_volume_parts_workspace_bytes(B, R)
    assert need >= 5 * 4 * B * R ** 3 and ws_bytes >= need

    def call(p=None, B=B, R=R, ws=ws_bytes, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in PTR_NAMES}
        p = _params(**kw) if p is None else p
        return L.gnr_volume_parts_fwd(C.byref(p) if p is not False else None, a['height'], B, R, *(a[k] for k in PTR_NAMES[1:-1]), a['workspace'], ws, None)

    for name in PTR_NAMES:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for r in (1, 0, 257):
        assert call(R=r) == _lib.GNR_ERR_SHAPE and text() == fn + ': R must be in 2..256', r
    for c in (0, 4, 8, 27, -6):
        assert call(connectivity=c) == _lib.GNR_ERR_ARG and text() == fn + ': connectivity must be 6, 18 or 26', c
    for m in (0, -1):
        assert call(max_parts=m) == _lib.GNR_ERR_SHAPE and text() == fn + ': max_parts must be >= 1', m
    assert call(min_peak=-1) == _lib.GNR_ERR_ARG and text() == fn + ': min_peak must be >= 0'
    for bad in (1.5, math.nan, -0.1, math.inf, -math.inf, math.nextafter(1.0, 2.0)):
        assert call(neck=bad) == _lib.GNR_ERR_ARG and text() == fn + ': neck must be finite and in 0..1', bad
    for ws in (0, need - 1):
        assert call(ws=ws) == _lib.GNR_ERR_WORKSPACE and text() == fn + ': workspace too small', ws


def test_refusals_before_the_device():
    one = C.c_void_p(16)
    _refusals({k: one for k in PTR_NAMES}, 1 << 30)


def test_workspace_byte_counts():
    L = _lib.lib()
    fn = L.gnr_volume_parts_workspace_bytes
    assert [fn(B, R) for B, R in ((0, 8), (65536, 8), (1, 1), (1, 257))] == [0, 0, 0, 0]
    assert fn(65535, 2) > 0 and fn(1, 256) > 0
    # the status word keeps the first 256 bytes to itself; five int volumes, one of 64-bit keys and the chunk counts lie behind it
    assert fn(1, 8) == 256 + 5 * 2048 + 4096 + 256 and fn(3, 8) == 256 + 3 * (5 * 2048 + 4096) + 256
    # the objects' workspace is what it was
    assert L.gnr_volume_objects_workspace_bytes(1, 8) == 256 + 2 * 2048 + 256 and L.gnr_volume_objects_workspace_bytes(1, 40) == 512512


# ---- GPU: the bits of the statement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op():
    return parts.VolumeParts()


def _host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if torch.is_tensor(v)}


def check(what, height, structures=None, op=None, **params):
    """VolumeParts on height [B,R,R,R] against the statement, status word 0; -> the statement."""
    height = np.asarray(height, np.int32)
    want = pref.parts(height, structures=structures, **{**parts.PART_DEFAULTS, **params})
    got = _host((op or _op())(height, **params))
    assert got['status'].dtype == np.int32 and got['status'][0] == 0, what
    same(what, got, want)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('conn', CONNECTIVITIES)
@pytest.mark.parametrize('R', [2, 3, 5, 8, 33])
def test_random_fields(R, conn):
    """Three scenes per call, every neck and min_peak; at R = 33 fewer rows than parts."""
    fields = random_fields(R, 100 + R)
    M = 64 if R == 33 else 600
    structures = [pref.structure(h, conn) for h in fields]
    most = 0
    for neck, min_peak in itertools.product(NECKS, MIN_PEAKS):
        want = check((R, conn, neck, min_peak), fields, structures, connectivity=conn, max_parts=M, neck=neck, min_peak=min_peak)
        most = max(most, int(want['count'].max()))
    assert R < 33 or most > M, 'no scene with more parts than rows'


def wrap_fields(R):
    """test_volume_objects.py's solid pairs as heights: (i, j, R-1) / (i, j+1, 0) and (i, R-1, R-1) / (i+1, 0, 0) are next to each other
    in memory and no neighbours; nor are the last voxel of a scene and the first of the next."""
    a, b = np.zeros((R, R, R), np.int32), np.zeros((R, R, R), np.int32)
    i2 = min(2, R - 2)
    a[0, 0, R - 1], a[0, 1, 0], a[i2, R - 1, R - 1], a[i2 + 1, 0, 0], a[R - 1, R - 1, R - 1] = 5, 9, 5, 5, 2
    b[0, 0, 0], b[i2, 0, R - 1], b[i2, 1, 0] = 9, 3, 3
    return np.stack([a, b])


@pytest.mark.gpu
def test_rows_and_scenes_do_not_wrap():
    for R in (2, 5, 9):
        for conn in CONNECTIVITIES:
            for neck in (0.0, 0.8):
                want = check(('wrap', R, conn, neck), wrap_fields(R), connectivity=conn, neck=neck)
                if R > 2:                                                      # (at R = 2 every voxel is a 26-neighbour of every other)
                    assert list(want['count']) == [5, 3] == list(want['basins']) and (want['voxels'][:, :3] == 1).all(), (R, conn, want['count'])


def serpentine(R):
    """test_volume_objects.py's path: one 6-connected path (R odd), rows along k at even (i, j), joined by single voxels at alternating
    ends; the linear index is not monotone along it.  -> the path's voxels in order."""
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
    return path


@pytest.mark.gpu
def test_long_walks_and_long_chains():
    R = 9
    path = serpentine(R)
    n = len(path)
    assert n == len(set(path)) >= R ** 3 / 4 and all(sum(abs(a - b) for a, b in zip(p, q)) == 1 for p, q in zip(path, path[1:]))
    at = tuple(np.array(path).T)
    up, down, flat = (np.zeros((R, R, R), np.int32) for _ in range(3))
    up[at], down[at], flat[at] = 1 + np.arange(n), n - np.arange(n), 1
    for conn in CONNECTIVITIES:                                                # (the rows are two apart: no diagonal joins anything new)
        for neck in (0.5, 1.0):
            want = check(('serpentine', conn, neck), np.stack([up, down, flat]), connectivity=conn, neck=neck)
            assert list(want['count']) == [1, 1, 1] and list(want['basins'][:2]) == [1, 1] and want['basins'][2] > 10, want['basins']
            assert list(want['voxels'][:, 0]) == [n] * 3 and list(want['peak'][:, 0]) == [n, n, 1]
            assert list(want['peak_voxel'][:, 0]) == [(path[-1][0] * R + path[-1][1]) * R + path[-1][2], 0, 0]
    # the 3-D checkerboard: under 6 every solid voxel is a part -- more than the rows --, under 26 with neck = 1 one plateau
    i = np.arange(R)
    board = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0).astype(np.int32) * 3
    want = check(('checkerboard', 6), np.stack([board, 3 - board]), connectivity=6, max_parts=64)
    assert list(want['count']) == [(R ** 3 + 1) // 2, R ** 3 // 2] == list(want['basins']) and want['labels'].max() == (R ** 3 + 1) // 2
    assert (want['voxels'] == 1).all() and (want['peak'] == 3).all()
    want = check(('checkerboard', 26), np.stack([board, 3 - board]), connectivity=26, max_parts=64, neck=1.0)
    assert list(want['count']) == [1, 1] and (want['basins'] > 1).all()
    # all solid and all free
    want = check('solid, free', np.stack([np.full((R, R, R), 7, np.int32), np.zeros((R, R, R), np.int32), np.full((R, R, R), -7, np.int32)]), max_parts=8)
    assert list(want['count']) == [1, 0, 0] and list(want['basins']) == [1, 0, 0] and want['voxels'][0, 0] == R ** 3 and not want['labels'][1:].any()
    assert list(want['bbox'][0, 0]) == [0, 0, 0, R - 1, R - 1, R - 1] and list(want['peak_voxel'][:, 0]) == [0, -1, -1]


@pytest.mark.gpu
def test_the_distance_field_of_touching_shapes():
    """R = 24, the shapes of the 40^3 table scaled by 0.6: VolumeDistance's d2_free is the statement's, VolumeParts on it splits where the
    statement splits -- the counts are the statement's own, at neck 0.7 and 0.8, with and without a table cut."""
    R, s = 24, 0.6
    vol = np.stack([mask_volume(spheres(R, 11, s)), mask_volume(sphere_on_box(R, s)), mask_volume(spheres(R, 14, s))])
    vd = distance.VolumeDistance()
    counts = {}
    for z_min in (0, 4):
        field = vd(vol, scale=VOXEL, z_min=z_min)
        torch.cuda.synchronize()
        height = pref.d2_free(vol, z_min=z_min)
        assert np.array_equal(field['d2_free'].cpu().numpy(), height) and height.dtype == np.int32
        assert np.array_equal(height > 0, (vol < 0) & (np.arange(R) >= z_min))
        for neck in (0.7, 0.8):
            want = pref.parts(height, neck=neck)
            got = _host(_op()(field['d2_free'], neck=neck))
            assert got['status'][0] == 0
            same((z_min, neck), got, want)
            counts[z_min, neck] = list(want['count'])
    print(counts)
    assert all(a <= b for z in (0, 4) for a, b in zip(counts[z, 0.7], counts[z, 0.8])), 'a larger neck joins less'
    assert counts[0, 0.8][0] == 2 and counts[0, 0.8][2] == 2 and max(counts[0, 0.7]) <= 2, counts


@functools.lru_cache(maxsize=None)
def touching_scene():
    """[40,40,40] float32, never written to: two balls of radius 7 that touch, centres 14 apart along j."""
    vol = mask_volume(ball(40, (20, 13, 12), 7) | ball(40, (20, 27, 12), 7))
    vol.setflags(write=False)
    return vol


# (index, width in voxels): across the first ball, across the contact of the two, in empty space
GRASPS = (((20, 13, 17), 14.0), ((20, 20, 16), 30.0), ((32, 6, 32), 8.0))


@pytest.mark.gpu
def test_parts_of_plan():
    vol = np.array(touching_scene())
    g = dict(index=np.int64([p for p, _ in GRASPS]), quat=np.tile(DOWN, (len(GRASPS), 1)).astype(f64), width=f32([w for _, w in GRASPS]) * f32(VOXEL))
    g['pos'] = g['index'].astype(f64) * VOXEL
    got, cols = parts.parts_of_plan(vol, g, voxel_size=VOXEL, max_parts=16)
    height = pref.d2_free(vol[None])
    want = pref.parts(height, max_parts=16)
    assert list(want['count']) == [2] and got['count'] == 2 and np.array_equal(got['labels'], want['labels'][0]) and got['labels'].dtype == np.int32
    for k in ('voxels', 'peak', 'peak_voxel'):
        assert np.array_equal(got[k], want[k][0, :2]) and got[k].dtype == np.int32, k
    assert np.array_equal(got['bbox_lo'], want['bbox'][0, :2, :3]) and np.array_equal(got['bbox_hi'], want['bbox'][0, :2, 3:]) and got['basins'] == want['basins'][0]
    assert np.array_equal(got['radius'], np.sqrt(want['peak'][0, :2].astype(f64)) * f64(VOXEL))
    w_vox = (g['width'] / f32(VOXEL)).astype(f32)
    for r in range(len(GRASPS)):
        assert tuple(int(cols[k][r]) for k in ('part', 'part_votes', 'parts_in_hand', 'part_samples')) == \
            oref.grasp_object(want['labels'][0], g['index'][r].astype(f64), g['quat'][r].astype(f32), w_vox[r], VOXEL), r
    _, ocols = objects.objects_of_plan(vol, g, voxel_size=VOXEL)
    print(cols, ocols)
    assert list(cols['parts_in_hand']) == [1, 2, 0] and list(ocols['objects_in_hand']) == [1, 1, 0], 'the grasp across the contact pinches two parts of one object'
    assert list(cols['part'])[::2] == [1, 0] and cols['part'][1] in (1, 2) and objects.best_per_object(cols['part']) == {1: 0}
    assert all(v.dtype == np.int32 for v in cols.values())
    none, cols0 = parts.parts_of_plan(vol[None], dict(index=np.zeros((0, 3), np.int64), quat=np.zeros((0, 4)), width=np.zeros(0, f32)), voxel_size=VOXEL, neck=0.0)
    assert none['count'] == 1 and all(len(v) == 0 for v in cols0.values())
    with pytest.raises(_lib.GnrError, match='raise max_parts'):
        parts.parts_of_plan(vol, g, voxel_size=VOXEL, max_parts=1)
    with pytest.raises(ValueError, match='z_min must be in 0..R'):
        parts.parts_of_plan(vol, g, voxel_size=VOXEL, z_min=41)


@pytest.mark.gpu
def test_nothing_is_kept_in_the_workspace():
    """One object on (B=3, R=9), (B=1, R=33), (B=3, R=9), its workspace and every output filled with 0x5a bytes before each call: the
    statement's bits, and those of a fresh object."""
    op = parts.VolumeParts()
    fields = [random_fields(9, 1), random_fields(33, 2)[:1], random_fields(9, 3)]
    kw = dict(connectivity=18, max_parts=32, neck=0.5, min_peak=1)
    op(fields[1], **kw)                                                        # sizes the workspace
    for h in (*fields, fields[0]):
        op._ws.fill_(SENTINEL)
        for shape_out in op._out.values():
            for t in shape_out.values():
                t.view(torch.uint8).fill_(SENTINEL)
        want = check(('stale', h.shape), h, op=op, **kw)
        same(('stale, against a fresh object', h.shape), _host(parts.VolumeParts()(h, **kw)), want)
    ptrs = {k: t.data_ptr() for k, t in op(fields[0], **kw).items() if torch.is_tensor(t)}
    assert {k: t.data_ptr() for k, t in op(fields[2], **kw).items() if torch.is_tensor(t)} == ptrs, 'the buffers of a shape are kept'
    with pytest.raises(ValueError, match='height must be'):
        op(fields[0][:, :, :, :5])


@pytest.mark.gpu
def test_one_captured_graph_from_the_volume_to_the_grasps():
    """VolumeDistance, VolumeParts on its d2_free and GraspObjects on the parts' labels captured once on one stream, replayed after the
    input volume changed: the bits of the eager calls and of the statement."""
    R, n, dev = 17, 10, 'cuda:0'
    rng = np.random.default_rng(29)

    def blobs(seed):
        """Two scenes of a few overlapping balls each."""
        r = np.random.default_rng(seed)
        return np.stack([mask_volume(functools.reduce(np.logical_or, [ball(R, r.uniform(3, R - 4, 3), r.uniform(2.0, 4.5)) for _ in range(5)])) for _ in range(2)])

    scenes = [blobs(s) for s in (1, 2, 3)]
    pos, quat, width = rng.uniform(1.0, R - 2.0, (2, n, 3)), rng.normal(size=(2, n, 4)).astype(f32), rng.uniform(1.0, 9.0, (2, n)).astype(f32)
    vol = torch.from_numpy(scenes[0]).to(dev)
    P, Q, W = (torch.from_numpy(a).to(dev) for a in (pos, quat, width))
    counts = (n, n - 3)
    count = torch.tensor(counts, dtype=torch.int32, device=dev)
    kw = dict(connectivity=26, max_parts=64, neck=0.8)

    def run(a, b, c):
        field = a(vol, scale=0.02, z_min=1)
        res = b(field['d2_free'], **kw)
        return field, res, c(res['labels'], P, Q, W, count, scale=0.02, depth=0.08)

    ops = distance.VolumeDistance(), parts.VolumeParts(), objects.GraspObjects()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*ops)                                                              # sizes the workspaces and the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        field, res, rows = run(*ops)
    eager = distance.VolumeDistance(), parts.VolumeParts(), objects.GraspObjects()
    split = 0
    for s in (scenes[1], scenes[2], scenes[1]):
        vol.copy_(torch.from_numpy(s).to(dev))
        torch.cuda.synchronize()
        graph.replay()
        got, got_rows, got_h = _host(res), _host(rows), _host(field)['d2_free']
        _, e_res, e_rows = run(*eager)
        e_res, e_rows = _host(e_res), _host(e_rows)
        height = pref.d2_free(s, z_min=1)
        want = pref.parts(height, **kw)
        assert got['status'][0] == 0 and np.array_equal(got_h, height)
        same('replay against the eager call', got, e_res)
        same('replay against the statement', got, want)
        split += int((want['count'] > [oref.label(v, z_min=1, connectivity=26)[1] for v in s]).sum())
        for b in range(2):
            ref_rows = oref.grasp_objects(want['labels'][b], pos[b], quat[b], width[b], counts[b], 0.02, depth=0.08)
            for k, w in zip(objects.GRASP_OBJECT_ROWS, ref_rows):
                assert np.array_equal(got_rows[k][b], e_rows[k][b]) and np.array_equal(got_rows[k][b][:counts[b]], w[:counts[b]]), (k, b)
    assert split > 0, 'no scene in which the parts are more than the components'


@pytest.mark.gpu
def test_a_refused_call_writes_nothing():
    B, R, M = 1, 8, 4
    fill = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    sizes = dict(height=4 * R ** 3, labels=4 * R ** 3, count=4, basins=4, voxels=4 * M, bbox=24 * M, sums=24 * M, peak=4 * M, peak_voxel=4 * M,
                 workspace=_lib.lib().gnr_volume_parts_workspace_bytes(B, R))
    bufs = {k: fill(v) for k, v in sizes.items()}
    _refusals({k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}, sizes['workspace'], B=B, R=R)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == SENTINEL).all()), k
