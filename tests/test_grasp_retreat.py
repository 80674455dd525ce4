"""Retreat of the ranked grasps (csrc/gnr_retreat.hip, retreat.GraspRetreat, retreat.retreat_of_plan).  tests/retreat_reference.py is the
statement (numpy integers, a handful of float64 operations); every comparison is np.array_equal, dtypes included (the float32 travel
by its bits).  Without a GPU: the statement against a literal restatement voxel by voxel, the synthetic piles, the ties of rint, the
host functions, the parameter checks, every refusal of the entry point.  On the GPU: shapes chosen to break the kernel -- unconnected
random labels, lattice ends next to filled scenes, boxes that lie, counts across all wavefronts -- rather than to resemble the
workload, then a plan's route and a captured graph from the volume to the retreat."""
import ctypes as C
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, distance, objects, parts, retreat
import hand_reference as href
import objects_reference as oref
import parts_reference as pref
import retreat_reference as rref

f32, f64 = np.float32, np.float64
VOXEL = 0.3 / 40
DOWN = f32([1.0, 0.0, 0.0, 0.0])                                               # top-down: the hand's z is world -z, it retreats along +z
SENTINEL = 0x5a
SENTINEL_WORD = 0x5a5a5a5a
# quaternions whose retreat u = -M[:, 2] is an axis of the lattice (half turns about a diagonal: no component needs a rounded sine)
ALONG = {(-1, 0, 0): f32([1, 0, 1, 0]), (1, 0, 0): f32([-1, 0, 1, 0]), (0, -1, 0): f32([0, 1, 1, 0]), (0, 1, 0): f32([0, -1, 1, 0]),
         (0, 0, -1): f32([0, 0, 0, 1]), (0, 0, 1): DOWN}
NEVER_SIDE = -2.0                                                              # a side_cos below every -a_z: the hand always moves along its own z


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == f32 else a


def same(what, got, want):
    for k, g, w in zip(rref.KEYS, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, k, g, w)


def sentinels(n):
    """The six columns of n rows nobody wrote."""
    return tuple(np.full(n, SENTINEL_WORD, np.int32).view(t) for t in rref.TYPES)


def random_scene(R, seed, max_parts=4):
    """labels [R,R,R] int32 uniform in 0..4, unconnected on purpose, and the statistics rows' boxes of the labels 1..4."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 5, (R, R, R)).astype(np.int32)
    lab.ravel()[rng.permutation(R ** 3)[:4]] = (1, 2, 3, 4)                    # (the statistics take every label 1..4 to have a voxel)
    return lab, oref.statistics(lab, 4, max_parts)[1]


def random_rows(n, seed):
    """held [n] int32 in -1..6 and quat [n,4] float32: random ones, the zero quaternion, one with a NaN, straight down, one with an inf."""
    rng = np.random.default_rng(seed)
    held = rng.integers(-1, 7, n).astype(np.int32)
    quat = rng.normal(size=(n, 4)).astype(f32)
    quat[1], quat[2], quat[3], quat[4] = 0.0, (0.3, np.nan, 0.1, 0.5), DOWN, (0.0, 0.0, 0.0, np.inf)
    held[:5] = (1, 2, 3, 4, 1)
    return held, quat


PARAMS = (dict(scale=0.02), dict(scale=VOXEL, tolerance=5), dict(scale=0.05, step=0.37, side_cos=NEVER_SIDE), dict(scale=0.03, retreat=0.01, step=0.5, side_cos=0.9),
          dict(scale=1.0, retreat=3.0, step=1.0, tolerance=1))


# ---- 1. the statement (no GPU) --------------------------------------------------------------------------------------------------------
def restatement(labels, bbox, held, quat, scale, retreat=0.1, step=0.5, side_cos=0.5, tolerance=0):
    """include/gnr.h's words one voxel and one step at a time, in plain Python."""
    R = labels.shape[0]
    T = f64(retreat) / f64(scale)
    K = int(max(1.0, math.ceil(T / f64(step))))
    sl = T / f64(K)
    M = href.matrix(quat)
    u = [-M[a, 2] for a in range(3)]
    if any(math.isnan(x) for x in u):
        return np.int32(0), np.int32(0), np.int32(0), np.int32(0), np.int32(0), f32(T * f64(scale))
    side = 1 if u[2] < f64(side_cos) else 0
    if side:
        u = [f64(0.0), f64(0.0), f64(1.0)]
    L, vox = int(held), []
    if 1 <= L <= len(bbox):
        lo = [max(int(bbox[L - 1][a]), 0) for a in range(3)]
        hi = [min(int(bbox[L - 1][3 + a]), R - 1) for a in range(3)]
        vox = [(i, j, k) for i in range(lo[0], hi[0] + 1) for j in range(lo[1], hi[1] + 1) for k in range(lo[2], hi[2] + 1) if labels[i, j, k] == L]
    overlap, blocked, blocker = 0, 0, 0
    for k in range(1, K + 1):
        o = [int(np.rint(u[a] * (f64(k) * sl))) for a in range(3)]             # (a Python int: no width)
        hits, first = 0, 0
        for v in vox:                                                          # ascending linear index
            t = [v[a] + o[a] for a in range(3)]
            if all(0 <= x <= R - 1 for x in t):
                x = int(labels[t[0], t[1], t[2]])
                if x != 0 and x != L:
                    hits, first = hits + 1, first if hits else x
        overlap = max(overlap, hits)
        if not blocked and hits > tolerance:
            blocked, blocker = k, first
    travel = f32((f64(blocked - 1) * sl) * f64(scale)) if blocked else f32(T * f64(scale))
    return np.int32(blocked), np.int32(blocker), np.int32(overlap), np.int32(len(vox)), np.int32(side), travel


@pytest.mark.parametrize('R', [2, 3, 5])
def test_the_reference_equals_its_literal_restatement(R):
    blocked = 0
    for seed in range(3):
        lab, bbox = random_scene(R, 10 * R + seed)
        held, quat = random_rows(12, R + seed)
        for p in PARAMS:
            for r in range(len(held)):
                want = restatement(lab, bbox, held[r], quat[r], **p)
                same((R, seed, p, r), rref.retreat(lab, bbox, held[r], quat[r], **p), want)
                blocked += int(want[0] > 0)
    assert blocked > 10, 'hardly a row is blocked'
    # a box that lies -- wider than the part, beyond the lattice, empty -- and the rows of a scene
    lab, bbox = random_scene(R, 77)
    wide = bbox.copy()
    wide[0], wide[1], wide[2] = (-5, -5, -5, R + 5, R + 5, R + 5), (0, 0, 0, R - 1, R - 1, R - 1), (R, R, R, -1, -1, -1)
    for L in (1, 2, 3):
        got = rref.retreat(lab, wide, L, DOWN, 0.02)
        same(('wide', L), got, restatement(lab, wide, L, DOWN, 0.02))
        same(('a wider box gives the part\'s own result, an empty one what no label gives', L), got, rref.retreat(lab, bbox, L if L < 3 else 9, DOWN, 0.02))
    assert rref.retreat(lab, wide, 3, DOWN, 0.02)[3] == 0 and rref.retreat(lab, bbox, 3, DOWN, 0.02)[3] > 0
    held, quat = random_rows(8, 5)
    rows = rref.retreat_rows(lab, bbox, held, quat, 6, 0.02, top_k=5, out=sentinels(8))
    for r in range(8):
        same(('rows', r), [c[r] for c in rows], rref.retreat(lab, bbox, held[r], quat[r], 0.02) if r < 5 else [c[0] for c in sentinels(1)])
    assert all(c.dtype == t for c, t in zip(rref.retreat_rows(lab, bbox, held, quat, 8, 0.02), rref.TYPES))


def lattice(R):
    i = np.arange(R, dtype=f64)
    return np.meshgrid(i, i, i, indexing='ij')


def ball(R, centre, radius):
    I, J, K = lattice(R)
    return (I - centre[0]) ** 2 + (J - centre[1]) ** 2 + (K - centre[2]) ** 2 <= radius ** 2


def box(R, lo, hi):
    I, J, K = lattice(R)
    return (I >= lo[0]) & (I <= hi[0]) & (J >= lo[1]) & (J <= hi[1]) & (K >= lo[2]) & (K <= hi[2])


def mask_volume(mask):
    return np.where(mask, -1.0, 1.0).astype(f32)


def tilted(degrees):
    """Straight down, then turned about the world's x by `degrees`: the retreat leans towards +j (positive) or -j."""
    a = (math.pi - math.radians(degrees)) / 2
    return f32([math.sin(a), 0.0, 0.0, math.cos(a)])


@functools.lru_cache(maxsize=None)
def scenes():
    """The 40^3 synthetic piles, never written to: name -> (vol [40,40,40] float32, labels, bbox [8,6], voxels [8], count) with the
    labels of parts_reference, 26-connected, neck 0.8.  sphere_on_box is test_volume_parts.py's; the pile is three touching balls of
    radius 7 on the floor and a fourth of radius 6 resting in their hollow; side_by_side two touching balls of radius 7 along j."""
    R, c, top = 40, 20, 10
    low = ((13, 14, 7), (27, 14, 7), (20, 26, 7))
    masks = dict(sphere_on_box=box(R, (c - 8, c - 8, 3), (c + 8, c + 8, top)) | ball(R, (c, c, top + 6), 6),
                 pile=functools.reduce(np.logical_or, [ball(R, p, 7) for p in low]) | ball(R, (20, 18, 17), 6),
                 side_by_side=ball(R, (20, 13, 12), 7) | ball(R, (20, 27, 12), 7))
    out = {}
    for name, m in masks.items():
        vol = mask_volume(m)
        w = pref.parts(pref.d2_free(vol[None]), max_parts=8)
        out[name] = tuple(a for a in (vol, w['labels'][0], w['bbox'][0], w['voxels'][0])) + (int(w['count'][0]),)
        for a in out[name][:4]:
            a.setflags(write=False)
    return out


def test_the_synthetic_piles():
    """What the statement says of the piles at 40^3 (0.0075 m voxels: T = 13.33 voxels in K = 27 steps)."""
    T, K, sl = rref.steps(0.1, 0.5, VOXEL)
    assert K == 27 and T == f64(0.1) / f64(VOXEL) and sl == T / 27.0
    free = lambda got: (int(got[0]), int(got[1]), int(got[2])) == (0, 0, 0) and got[5] == f32(T * f64(VOXEL))
    _, lab, bbox, voxels, n = scenes()['sphere_on_box']
    assert n == 2 and list(voxels[:2]) == [2349, 887]                          # the box, the ball
    for q in (DOWN, tilted(20), tilted(-35), ALONG[1, 0, 0], ALONG[0, 0, -1], f32([0.3, -0.2, 0.1, 0.9])):
        got = rref.retreat(lab, bbox, 2, q, VOXEL)
        assert free(got) and got[3] == 887, ('the ball retreats free from every pose', q, got)
    d = {}
    got = rref.retreat(lab, bbox, 1, DOWN, VOXEL, details=d)
    assert tuple(int(x) for x in got[:5]) == (2, 2, 817, 2349, 0) and got[5] == f32((f64(1) * sl) * f64(VOXEL)), got
    assert list(d['hits'][:4]) == [0, 37, 37, 106] and list(d['offsets'][:4, 2]) == [0, 1, 1, 2] and not d['offsets'][:, :2].any()
    # the pile: the three lower balls are blocked by the top one at the first step that moves a voxel, the top one is free
    _, lab, bbox, voxels, n = scenes()['pile']
    assert n == 4
    top = int(lab[20, 18, 20])
    assert voxels[top - 1] == 924 and free(rref.retreat(lab, bbox, top, DOWN, VOXEL))
    for L in sorted(set(range(1, 5)) - {top}):
        got = rref.retreat(lab, bbox, L, DOWN, VOXEL)
        assert (int(got[0]), int(got[1])) == (2, top) and 200 < got[2] < 230 and got[3] == voxels[L - 1], (L, got)
    # two balls side by side: either lifts free; leaning 20 degrees towards the neighbour it is blocked at step 3, leaning away free
    _, lab, bbox, voxels, n = scenes()['side_by_side']
    assert n == 2 and lab[20, 13, 12] == 1 and lab[20, 27, 12] == 2
    for L, towards in ((1, 20), (2, -20)):
        assert free(rref.retreat(lab, bbox, L, DOWN, VOXEL)) and free(rref.retreat(lab, bbox, L, tilted(-towards), VOXEL))
        got = rref.retreat(lab, bbox, L, tilted(towards), VOXEL)
        assert tuple(int(x) for x in got[:5]) == (3, 3 - L, 18, int(voxels[L - 1]), 0) and got[5] == f32((f64(2) * sl) * f64(VOXEL)), got
        assert rref.retreat(lab, bbox, L, tilted(towards), VOXEL, tolerance=18)[0] == 0
    # a side grasp lifts along world +z whatever its own z: the hand's z horizontal, towards the neighbour
    got = rref.retreat(lab, bbox, 1, ALONG[0, 1, 0], VOXEL)
    assert free(got) and got[4] == 1
    got = rref.retreat(lab, bbox, 1, ALONG[0, 1, 0], VOXEL, side_cos=NEVER_SIDE)
    assert got[4] == 0 and got[0] == 2 and got[1] == 2 and got[5] == f32((f64(1) * sl) * f64(VOXEL))      # (step 1 is rint(0.49) = 0 voxels)


def tie_scene():
    """R = 8: part 1 is the voxel (3, 3, 1), part 2 the voxel (3, 3, 3), part 3 the voxel (3, 3, 2) -- with scale = 1, retreat = 4 and
    step = 0.5 the offsets of the 8 steps along +z are rint(0.5 k): 0, 1, 2, 2, 2, 3, 4, 4."""
    lab = np.zeros((8, 8, 8), np.int32)
    lab[3, 3, 1], lab[3, 3, 3], lab[3, 3, 2] = 1, 2, 3
    return lab, oref.statistics(lab, 3, 4)[1]


def test_ties_round_to_even():
    T, K, sl = rref.steps(4.0, 0.5, 1.0)
    assert (T, K, sl) == (4.0, 8, 0.5)
    assert list(rref.offsets(np.array([0.0, 0.0, 1.0]), K, sl, 8)[:, 2]) == [0, 1, 2, 2, 2, 3, 4, 4]
    assert list(rref.offsets(np.array([0.0, 0.0, -1.0]), K, sl, 8)[:, 2]) == [0, -1, -2, -2, -2, -3, -4, -4]
    lab, bbox = tie_scene()
    kw = dict(scale=1.0, retreat=4.0, step=0.5)
    d = {}
    got = rref.retreat(lab, bbox, 1, DOWN, details=d, **kw)                    # 0.5 -> 0: step 1 stays; step 2 moves one voxel onto part 3
    assert list(d['hits']) == [0, 1, 1, 1, 1, 0, 0, 0] and tuple(int(x) for x in got[:5]) == (2, 3, 1, 1, 0) and got[5] == f32(0.5)
    same('tie', got, restatement(lab, bbox, 1, DOWN, **kw))
    lab[3, 3, 2] = 0                                                           # without part 3: 1.5 -> 2 lands on part 2 at step 3, not at step 2
    d = {}
    got = rref.retreat(lab, bbox, 1, DOWN, details=d, **kw)
    assert list(d['hits']) == [0, 0, 1, 1, 1, 0, 0, 0] and tuple(int(x) for x in got[:5]) == (3, 2, 1, 1, 0) and got[5] == f32(1.0)
    same('tie', got, restatement(lab, bbox, 1, DOWN, **kw))
    # an offset of R and more is out whatever its size: one step of 10^12 voxels
    far = dict(scale=1.0, retreat=1e12, step=1e12)
    got = rref.retreat(lab, bbox, 1, DOWN, **far)
    assert tuple(int(x) for x in got[:5]) == (0, 0, 0, 1, 0) and got[5] == f32(1e12)
    same('far', got, restatement(lab, bbox, 1, DOWN, **far))


def test_best_free_per_part():
    cols = dict(part=np.int32([2, 2, 0, 1, 3, 1, 2]), retreat_free=np.array([False, True, True, False, False, True, True]))
    assert retreat.best_free_per_part(cols) == {2: 1, 1: 5}
    assert objects.best_per_object(cols['part']) == {1: 3, 2: 0, 3: 4}
    assert retreat.best_free_per_part(dict(object=cols['part'], retreat_free=np.zeros(7, bool))) == {}
    assert retreat.best_free_per_part(dict(part=np.zeros(0, np.int32), retreat_free=np.zeros(0, bool))) == {}
    rows = dict(blocked_step=np.int32([0, 3]), blocker=np.int32([0, 2]), overlap=np.int32([1, 18]), moved=np.int32([7, 9]), side=np.int32([1, 0]),
                travel=f32([0.1, 0.0074]))
    cols = retreat.retreat_from_rows(rows)
    assert list(cols) == ['retreat_free', 'retreat_travel', 'retreat_blocker', 'retreat_overlap', 'lifted_voxels', 'side_grasp']
    assert list(cols['retreat_free']) == [True, False] and cols['retreat_free'].dtype == bool and list(cols['side_grasp']) == [True, False]
    assert cols['retreat_travel'].dtype == f32 and np.array_equal(cols['retreat_travel'], rows['travel']) and cols['retreat_travel'] is not rows['travel']
    assert [cols[k].dtype for k in ('retreat_blocker', 'retreat_overlap', 'lifted_voxels')] == [np.int32] * 3
    assert list(cols['retreat_blocker']) == [0, 2] and list(cols['retreat_overlap']) == [1, 18] and list(cols['lifted_voxels']) == [7, 9]


def test_retreat_params():
    assert retreat.retreat_params(False) is None and retreat.retreat_params(None) is None
    want = dict(retreat=0.1, step=0.5, side_cos=0.5, tolerance=0)
    assert retreat.retreat_params(True) == want == retreat.retreat_params({}) == retreat.RETREAT_DEFAULTS == retreat.checked_retreat() == rref.DEFAULTS
    p = retreat.retreat_params(dict(retreat=1, tolerance=3, filter=True), filter=False)
    assert p == dict(want, retreat=1.0, tolerance=3, filter=True) and isinstance(p['retreat'], float) and isinstance(p['tolerance'], int)
    with pytest.raises(TypeError, match='unknown retreat parameters'):
        retreat.retreat_params(dict(neck=0.8))
    for bad, text in ((dict(retreat=0), 'retreat retreat must be finite and > 0, got 0'), (dict(retreat=math.inf), 'retreat retreat must be finite and > 0'),
                      (dict(retreat=True), 'retreat retreat must be finite and > 0'), (dict(step=-0.5), 'retreat step must be finite and > 0, got -0.5'),
                      (dict(step=math.nan), 'retreat step must be finite and > 0'), (dict(side_cos=math.nan), 'retreat side_cos must be finite'),
                      (dict(side_cos=math.inf), 'retreat side_cos must be finite'), (dict(tolerance=-1), 'retreat tolerance must be an integer >= 0, got -1'),
                      (dict(tolerance=0.5), 'retreat tolerance must be an integer >= 0')):
        with pytest.raises(ValueError, match=text):
            retreat.retreat_params(bad)
    params = inspect.signature(retreat.GraspRetreat.__call__).parameters
    assert {k: v.default for k, v in params.items() if k in want} == want and all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in (*want, 'scale', 'top_k'))
    assert retreat.retreat_steps(0.1, 0.5, VOXEL) == rref.steps(0.1, 0.5, VOXEL) and retreat.retreat_steps(1e-3, 0.5, 1.0)[1] == 1
    assert retreat.retreat_steps(512.0, 0.5, 1.0)[1] == _lib.GNR_RETREAT_MAX_STEPS == rref.MAX_STEPS
    for r, s, v in ((512.1, 0.5, 1.0), (1e308, 0.5, 1e-308), (0.1, 1e-300, 1.0)):
        with pytest.raises(ValueError, match='takes more than 1024 steps'):
            retreat.retreat_steps(r, s, v)
    g = dict(index=np.zeros((0, 3)), quat=np.zeros((0, 4)), width=np.zeros(0))
    with pytest.raises(TypeError, match='unknown retreat parameters'):
        retreat.retreat_of_plan(np.ones((4, 4, 4), f32), g, iso=0.0)
    with pytest.raises(ValueError, match='retreat tolerance must be an integer >= 0'):
        retreat.retreat_of_plan(np.ones((4, 4, 4), f32), g, tolerance=-2)
    with pytest.raises(ValueError, match='parts neck must be finite and in 0..1'):
        retreat.retreat_of_plan(np.ones((4, 4, 4), f32), g, neck=2.0)
    with pytest.raises(ValueError, match='retreat z_min must be an integer >= 0'):
        retreat.retreat_of_plan(np.ones((4, 4, 4), f32), g, z_min=-1)
    with pytest.raises(ValueError, match='takes more than 1024 steps'):
        retreat.retreat_of_plan(np.ones((4, 4, 4), f32), g, retreat=10.0)


def test_grasp_retreat_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        retreat.GraspRetreat()


# ---- 2. the refusals of the entry point -----------------------------------------------------------------------------------------------
PTR_NAMES = ('labels', 'bbox', 'held', 'quat', 'count', 'blocked_step', 'blocker', 'overlap', 'moved', 'side', 'travel')


def _params(**kw):
    return _lib.GnrRetreatParams(**{**dict(retreat=0.1, step=0.5, side_cos=0.5, scale=VOXEL, tolerance=0, max_parts=4), **kw})


def _refusals(ptr, B=1, R=8, max_n=4):
    """Every refusal of gnr_grasp_retreat_fwd, each with its code and its text, on the pointers given (fake ones, or buffers whose bytes
    the caller checks afterwards)."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_grasp_retreat_fwd'

    def call(p=None, B=B, R=R, max_n=max_n, count_stride=1, top_k=0, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in PTR_NAMES}
        p = _params(**kw) if p is None else p
        return L.gnr_grasp_retreat_fwd(C.byref(p) if p is not False else None, *(a[k] for k in PTR_NAMES[:5]), count_stride, B, R, max_n, top_k,
                                       *(a[k] for k in PTR_NAMES[5:]), None)

    for name in PTR_NAMES:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for r in (1, 0, 257):
        assert call(R=r) == _lib.GNR_ERR_SHAPE and text() == fn + ': R must be in 2..256', r
    for n in (0, -3):
        assert call(max_n=n) == _lib.GNR_ERR_SHAPE and text() == fn + ': max_n must be >= 1', n
    for s in (0, -1):
        assert call(count_stride=s) == _lib.GNR_ERR_ARG and text() == fn + ': count_stride must be >= 1', s
    assert call(top_k=-1) == _lib.GNR_ERR_ARG and text() == fn + ': top_k must be >= 0 (0: every row)'
    for key in ('retreat', 'step', 'scale'):
        for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
            assert call(**{key: bad}) == _lib.GNR_ERR_ARG and text() == fn + ': retreat, step and scale must be finite and > 0', (key, bad)
    for bad in (math.nan, math.inf, -math.inf):
        assert call(side_cos=bad) == _lib.GNR_ERR_ARG and text() == fn + ': side_cos must be finite', bad
    assert call(tolerance=-1) == _lib.GNR_ERR_ARG and text() == fn + ': tolerance must be >= 0'
    for m in (0, -1):
        assert call(max_parts=m) == _lib.GNR_ERR_SHAPE and text() == fn + ': max_parts must be >= 1', m
    cap = fn + ': step too small or retreat too long, a grasp would take more than GNR_RETREAT_MAX_STEPS (1024) steps'
    for kw in (dict(retreat=512.1, step=0.5, scale=1.0), dict(retreat=1e308, scale=1e-308), dict(step=1e-300), dict(retreat=1.0, scale=1e-3, step=0.97)):
        assert call(**kw) == _lib.GNR_ERR_ARG and text() == cap, kw


def test_refusals_before_the_device():
    one = C.c_void_p(16)
    _refusals({k: one for k in PTR_NAMES})


def test_a_refused_call_writes_nothing_without_a_device():
    """The same refusals on host buffers of 0x5a bytes: a refused call has launched nothing and the host side writes nothing."""
    bufs = {k: np.full(4096, SENTINEL, np.uint8) for k in PTR_NAMES}
    _refusals({k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()})
    for k, v in bufs.items():
        assert (v == SENTINEL).all(), k


# ---- GPU: the bits of the statement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op():
    return retreat.GraspRetreat()


def check(what, labels, bbox, held, quat, counts, top_k=None, stride=1, op=None, **params):
    """GraspRetreat on B scenes, its output tensors filled with 0x5a bytes before the call, against the statement: the rows the call owes
    and the sentinel in every other.  -> the statement's rows, per scene."""
    op = op or _op()
    labels, bbox, held, quat = np.asarray(labels, np.int32), np.asarray(bbox, np.int32), np.asarray(held, np.int32), np.asarray(quat, f32)
    B, n = held.shape
    cnt = np.full((B, stride), 999, np.int32)
    cnt[:, 0] = counts
    count = torch.from_numpy(cnt if stride > 1 else cnt[:, 0].copy()).to('cuda:0')
    for t in op(labels, bbox, held, quat, count, top_k=top_k, **params).values():          # (the tensors of this shape)
        t.view(torch.uint8).fill_(SENTINEL)
    res = op(labels, bbox, held, quat, count, top_k=top_k, **params)
    torch.cuda.synchronize()
    got = [res[k].cpu().numpy() for k in rref.KEYS]
    want = [rref.retreat_rows(labels[b], bbox[b], held[b], quat[b], counts[b], top_k=top_k, out=sentinels(n), **params) for b in range(B)]
    for b in range(B):
        same((what, b), [g[b] for g in got], want[b])
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 3, 5, 8, 13])
def test_random_labels(R):
    """Three scenes per call, rows beyond the count and beyond top_k hold the sentinel; count_stride 2."""
    n = 12
    scenes_ = [random_scene(R, 100 * R + b) for b in range(3)]
    labels, bbox = np.stack([s[0] for s in scenes_]), np.stack([s[1] for s in scenes_])
    rows = [random_rows(n, 7 * R + b) for b in range(3)]
    held, quat = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    blocked = 0
    for p in PARAMS:
        for top_k, stride, counts in ((None, 1, (n, 9, 0)), (7, 2, (n + 5, 3, -2))):
            want = check((R, p, top_k), labels, bbox, held, quat, counts, top_k, stride, **p)
            blocked += sum(int((w[0][:max(0, min(c, top_k or n, n))] > 0).sum()) for w, c in zip(want, counts))
    assert blocked > 20 or R == 2, 'hardly a row is blocked'


@pytest.mark.gpu
def test_ties_round_to_even_on_the_device():
    lab, bbox = tie_scene()
    kw = dict(scale=1.0, retreat=4.0, step=0.5)
    bare = lab.copy()
    bare[3, 3, 2] = 0
    held = np.int32([[1, 2, 3, 1]] * 2)
    quat = np.stack([np.stack([DOWN, DOWN, ALONG[0, 0, -1], ALONG[0, 0, -1]])] * 2)
    want = check('tie', np.stack([lab, bare]), np.stack([bbox, bbox]), held, quat, (4, 4), side_cos=NEVER_SIDE, **kw)
    assert [int(want[0][k][0]) for k in range(3)] == [2, 3, 1] and [int(want[1][k][0]) for k in range(3)] == [3, 2, 1]
    assert want[0][0][2] == 2 and want[0][1][2] == 1                           # part 3 moving down: 0.5 -> -0, 1.5 -> -2, onto nothing; then part 1 at -1


def face_scene(R):
    """Every voxel carries a label: six parts, one per face of the lattice (1, 2: the planes i = 0 and i = R-1; 3, 4: j, without those;
    5, 6: k), and 7 inside.  Carried outwards a face part meets nothing; any wrap into a neighbouring row, plane or scene is a hit."""
    lab = np.full((R, R, R), 7, np.int32)
    lab[:, :, 0], lab[:, :, R - 1] = 5, 6
    lab[:, 0, :], lab[:, R - 1, :] = 3, 4
    lab[0], lab[R - 1] = 1, 2
    bbox = np.tile(np.int32([R, R, R, -1, -1, -1]), (8, 1))                    # (at R = 2 the labels 3..7 have no voxel)
    for L in range(1, 8):
        at = np.argwhere(lab == L)
        if len(at):
            bbox[L - 1] = (*at.min(0), *at.max(0))
    return lab, bbox


@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 6, 9])
def test_parts_carried_out_of_the_lattice_meet_nothing(R):
    lab, bbox = face_scene(R)
    full = np.full((R, R, R), 9, np.int32)
    labels = np.stack([full, lab, full])
    boxes = np.stack([np.tile(np.int32([R, R, R, -1, -1, -1]), (8, 1)), bbox, np.tile(np.int32([0, 0, 0, R - 1, R - 1, R - 1]), (8, 1))])
    outwards = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    held = np.int32([[1, 2, 3, 4, 5, 6] * 2] * 3)
    quat = np.stack([np.stack([ALONG[d] for d in outwards] + [ALONG[tuple(-x for x in d)] for d in outwards])] * 3)
    for p in (dict(scale=VOXEL), dict(scale=1.0, retreat=float(R), step=1.0), dict(scale=1.0, retreat=1e9, step=1e9), dict(scale=0.05, step=0.3)):
        want = check(('faces', R, p), labels, boxes, held, quat, (12, 12, 12), side_cos=NEVER_SIDE, **p)
        blocked, blocker, overlap, moved = (want[1][k] for k in range(4))
        assert not blocked[:6].any() and not blocker[:6].any() and not overlap[:6].any() and (moved[:6 if R > 2 else 2] > 0).all(), (R, p, blocked, overlap)
        if R > 2 and p['scale'] != 1.0:
            assert (blocked[6:] > 0).all() and (overlap[6:] >= moved[6:] // 2).all(), 'carried inwards every face part is blocked'
        assert not want[0][3].any() and (want[2][3][:6] == 0).all()            # scene 0's boxes are empty; scene 2 has no label below 9


@pytest.mark.gpu
def test_boxes_that_lie_and_labels_that_hold_nothing():
    R = 9
    lab, bbox = random_scene(R, 3, max_parts=6)                                # rows 4 and 5: no such part
    wide = bbox.copy()
    wide[0], wide[1], wide[2] = (-5, -7, -2 ** 31, R + 5, 2 ** 31 - 1, R), (0, 0, 0, R - 1, R - 1, R - 1), (-1, 0, 0, R, R - 1, R - 1)
    held, quat = random_rows(16, 11)
    held[:] = [1, 2, 3, 4, 1, 2, 3, 4, 0, -1, -2 ** 31, 7, 2 ** 31 - 1, 5, 6, 3]
    for p in PARAMS[:3]:
        want = check(('honest', p), np.stack([lab, lab]), np.stack([bbox, wide]), np.stack([held, held]), np.stack([quat, quat]), (16, 16), **p)
        same(('a wider box gives the part\'s own result', p), want[1], want[0])
        assert not want[0][3][8:15].any() and (want[0][3][[0, 1, 3, 5, 6, 7, 15]] > 0).all() and not want[0][3][[2, 4]].any(), want[0][3]      # (rows 2 and 4: no direction)
        assert all(not want[0][k][8:15].any() for k in (0, 1, 2))
    # a label above the rows of bbox holds nothing even where the volume has it; a box that misses part of the part moves the rest
    small = bbox[:2].copy()
    small[1] = tuple(np.argwhere(lab == 2)[5]) * 2
    want = check('rows', lab[None], small[None], np.int32([[1, 2, 3, 4]]), np.stack([DOWN] * 4)[None], (4,), scale=0.02)
    assert list(want[0][3][1:]) == [1, 0, 0] and want[0][3][0] == (lab == 1).sum()


@pytest.mark.gpu
def test_counts_across_every_wavefront():
    """R = 16 split into two solid labels: 2 048 moving voxels, hundreds of hits per step in every wavefront of the block; a part of
    one voxel; K = 1."""
    R = 16
    lab = np.ones((R, R, R), np.int32)
    lab[:, :, R // 2:] = 2
    lab[5, 6, 3] = 3                                                           # one voxel inside part 1
    bbox = oref.statistics(lab, 3, 4)[1]
    held = np.int32([[1, 2, 3, 1, 2, 3, 1, 2]])
    quat = np.stack([DOWN, DOWN, DOWN, ALONG[0, 0, -1], ALONG[0, 0, -1], ALONG[1, 0, 0], tilted(30), f32([0.2, 0.5, -0.4, 0.1])])[None]
    for p in (dict(scale=0.0125), dict(scale=0.0125, tolerance=300), dict(scale=0.0125, tolerance=2047), dict(scale=1.0, retreat=0.3, step=0.5),
              dict(scale=1.0, retreat=0.7, step=1.0), dict(scale=0.01, step=0.01)):
        want = check(('split', p), lab[None], bbox[None], held, quat, (8,), side_cos=NEVER_SIDE, **p)
        assert want[0][3][0] == 2047 and want[0][3][1] == 2048 and want[0][3][2] == 1
    want = check('split', lab[None], bbox[None], held, quat, (8,), side_cos=NEVER_SIDE, scale=0.0125)
    assert want[0][2][0] == 2047 and want[0][0][0] == 2 and want[0][1][0] == 2, 'part 1 moves up into part 2: all of it at the deepest step'
    assert want[0][0][1] == 0 and want[0][0][2] == 2 and want[0][1][2] == 1 and want[0][2][2] == 1
    assert rref.steps(0.3, 0.5, 1.0)[1] == 1 and rref.steps(0.7, 1.0, 1.0)[1] == 1 and rref.steps(0.1, 0.01, 0.01)[1] == 1000


def plan_of(name):
    """Grasps on a synthetic pile: at every part's box centre, straight down and leaning both ways, and one in empty space."""
    vol, lab, bbox, voxels, n = scenes()[name]
    centres = [(bbox[L, :3] + bbox[L, 3:]) // 2 for L in range(n)]
    index, quat = [], []
    for c in centres:
        for q in (DOWN, tilted(20), tilted(-20), ALONG[0, 1, 0]):
            index.append(c)
            quat.append(q)
    index.append((36, 36, 36))
    quat.append(DOWN)
    return dict(index=np.int64(index), quat=np.stack(quat).astype(f64), width=np.full(len(index), 10.0, f32) * f32(VOXEL))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['sphere_on_box', 'pile', 'side_by_side'])
def test_retreat_of_plan(name):
    vol, lab, bbox, voxels, n = scenes()[name]
    g = plan_of(name)
    got, cols = retreat.retreat_of_plan(np.array(vol), g, voxel_size=VOXEL, max_parts=8)
    assert got['count'] == n and np.array_equal(got['labels'], lab) and np.array_equal(got['voxels'], voxels[:n])
    rows = len(g['index'])
    w_vox = (g['width'] / f32(VOXEL)).astype(f32)
    held = np.int32([oref.grasp_object(lab, g['index'][r].astype(f64), g['quat'][r].astype(f32), w_vox[r], VOXEL)[0] for r in range(rows)])
    assert np.array_equal(cols['part'], held) and held[-1] == 0 and (held[:-1] > 0).sum() >= n
    want = retreat.retreat_from_rows(dict(zip(rref.KEYS, rref.retreat_rows(lab, bbox, held, g['quat'].astype(f32), rows, VOXEL))))
    for k, w in want.items():
        assert cols[k].dtype == w.dtype and np.array_equal(bits(cols[k]), bits(w)), (k, cols[k], w)
    assert not cols['lifted_voxels'][-1] and cols['retreat_free'][-1] and cols['side_grasp'][3::4].all() and not cols['side_grasp'][0::4].any()
    best = retreat.best_free_per_part(cols)
    print(name, held, cols['retreat_free'], best)
    if name == 'sphere_on_box':
        assert set(best) == {2} and not cols['retreat_free'][held == 1].any(), 'only the ball comes out'
    if name == 'pile':
        top = int(lab[20, 18, 20])
        assert set(best) == {top} and (cols['retreat_blocker'][(held > 0) & (held != top)] == top).all(), 'only the top ball comes out'
    if name == 'side_by_side':
        assert set(best) == {1, 2}
    with pytest.raises(_lib.GnrError, match='raise max_parts'):
        retreat.retreat_of_plan(np.array(vol), g, voxel_size=VOXEL, max_parts=1)


@pytest.mark.gpu
def test_one_captured_graph_from_the_volume_to_the_retreat():
    """VolumeDistance, VolumeParts, GraspObjects and GraspRetreat captured once on one stream, replayed after the input volume changed:
    the bits of the statement at every replay."""
    R, n, dev, scale = 17, 10, 'cuda:0', 0.02
    rng = np.random.default_rng(31)

    def blobs(seed):
        """Two scenes of a few overlapping balls each."""
        r = np.random.default_rng(seed)
        return np.stack([mask_volume(functools.reduce(np.logical_or, [ball(R, r.uniform(3, R - 4, 3), r.uniform(2.0, 4.5)) for _ in range(5)])) for _ in range(2)])

    volumes = [blobs(s) for s in (1, 2, 3)]
    pos, width = rng.uniform(3.0, R - 4.0, (2, n, 3)), rng.uniform(2.0, 9.0, (2, n)).astype(f32)
    quat = rng.normal(size=(2, n, 4)).astype(f32)
    quat[:, :4] = DOWN
    vol = torch.from_numpy(volumes[0]).to(dev)
    P, Q, W = (torch.from_numpy(a).to(dev) for a in (pos, quat, width))
    counts = (n, n - 3)
    count = torch.tensor(counts, dtype=torch.int32, device=dev)
    kw = dict(connectivity=26, max_parts=64, neck=0.8)

    def run(a, b, c, d):
        field = a(vol, scale=scale, z_min=1)
        res = b(field['d2_free'], **kw)
        gres = c(res['labels'], P, Q, W, count, scale=scale, depth=0.08)
        return res, gres, d.of_parts(res, gres, dict(quat=Q, count=count), scale=scale, tolerance=1)

    ops = distance.VolumeDistance(), parts.VolumeParts(), objects.GraspObjects(), retreat.GraspRetreat()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*ops)                                                              # sizes the workspaces and the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, gres, rres = run(*ops)
    held_any = blocked = 0
    for s in (volumes[1], volumes[2]):
        vol.copy_(torch.from_numpy(s).to(dev))
        for t in rres.values():
            t.view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = pref.parts(pref.d2_free(s, z_min=1), **kw)
        assert np.array_equal(res['labels'].cpu().numpy(), want['labels']) and np.array_equal(res['bbox'].cpu().numpy(), want['bbox'])
        for b in range(2):
            held = oref.grasp_objects(want['labels'][b], pos[b], quat[b], width[b], counts[b], scale, depth=0.08)[0]
            assert np.array_equal(gres['object'][b, :counts[b]].cpu().numpy(), held[:counts[b]])
            rows = rref.retreat_rows(want['labels'][b], want['bbox'][b], held, quat[b], counts[b], scale, out=sentinels(n), tolerance=1)
            same(('replay', b), [rres[k][b].cpu().numpy() for k in rref.KEYS], rows)
            held_any += int((held[:counts[b]] > 0).sum())
            blocked += int((rows[0][:counts[b]] > 0).sum())
    print(held_any, blocked)
    assert held_any > 4, 'hardly a grasp holds a part'


@pytest.mark.gpu
def test_a_refused_call_writes_nothing():
    B, R, n, M = 1, 8, 4, 4
    fill = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    sizes = dict(labels=4 * R ** 3, bbox=24 * M, held=4 * n, quat=16 * n, count=4, blocked_step=4 * n, blocker=4 * n, overlap=4 * n, moved=4 * n,
                 side=4 * n, travel=4 * n)
    bufs = {k: fill(v) for k, v in sizes.items()}
    _refusals({k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}, B=B, R=R, max_n=n)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == SENTINEL).all()), k
