"""Support of the parts (csrc/gnr_support.hip, support.PartContacts, support.PartSupport, support.support_of_plan).
tests/support_reference.py is the statement (numpy integers, one float64 multiply and compare); every comparison is np.array_equal,
dtypes and shapes included.  Without a GPU: the statement against a literal restatement one voxel and one neighbour at a time and the
graph rules against plain Python sets, the synthetic piles, a column, a cycle, a floating part, the lean on its boundary, the host
functions, the parameter checks, every refusal of the two entry points.  On the GPU: shapes chosen to break the kernels -- unconnected
random labels next to other scenes, 256 labels in one wavefront, two solid halves, a chain of 256 parts written straight into the
table, tables full of cycles -- rather than to resemble the workload, then a plan's route and one captured graph from the volume to
the grasps' support columns."""
import ctypes as C
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, distance, objects, parts, retreat, support
import objects_reference as oref
import parts_reference as pref
import retreat_reference as rref
import support_reference as sref
import test_grasp_retreat as tgr

f32, f64, i32 = np.float32, np.float64, np.int32
VOXEL = tgr.VOXEL
SENTINEL = 0x5a
KEYS = (*sref.COLUMNS, 'rests_on')


def same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, got, want)


def random_labels(R, seed, lo=-1, hi=6):
    """labels [R,R,R] int32 uniform in lo..hi, unconnected on purpose: contacts everywhere."""
    return np.random.default_rng(seed).integers(lo, hi + 1, (R, R, R)).astype(i32)


# ---- 1. the statement (no GPU) --------------------------------------------------------------------------------------------------------
def contacts_restatement(lab, P, connectivity, z_min):
    """include/gnr.h's words one voxel and one neighbour at a time, in plain Python."""
    R = lab.shape[0]
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    touch, over = [[0] * P for _ in range(P)], [[0] * P for _ in range(P)]
    floor, dropped = [0] * P, 0
    for i in range(R):
        for j in range(R):
            for k in range(R):
                a = int(lab[i, j, k])
                if 1 <= a <= P and k == z_min:
                    floor[a - 1] += 1
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        for dk in (-1, 0, 1):
                            if not 1 <= (di != 0) + (dj != 0) + (dk != 0) <= most:
                                continue
                            wi, wj, wk = i + di, j + dj, k + dk
                            if not (0 <= wi < R and 0 <= wj < R and 0 <= wk < R):
                                continue
                            b = int(lab[wi, wj, wk])
                            if a < 1 or b < 1 or a == b:
                                continue
                            if a <= P and b <= P:
                                touch[a - 1][b - 1] += 1
                                if wk > k:
                                    over[a - 1][b - 1] += 1
                            else:
                                dropped += 1
    return np.stack([i32(touch), i32(over)], -1).reshape(P, P, 2), i32(floor).reshape(P), i32(dropped)


@pytest.mark.parametrize('R', [2, 3, 5])
def test_the_contacts_equal_their_literal_restatement(R):
    seen = dropped = 0
    for seed in range(2):
        lab = random_labels(R, 10 * R + seed)
        for connectivity in (6, 18, 26):
            for z_min in (0, 1, R):
                got = sref.contacts(lab, 4, connectivity, z_min)
                want = contacts_restatement(lab, 4, connectivity, z_min)
                for k, g, w in zip(('pairs', 'floor', 'dropped'), got, want):
                    same((R, seed, connectivity, z_min, k), g, w)
                assert np.array_equal(got[0][..., 0], got[0][..., 0].T), 'touch is symmetric by construction'
                assert not got[1].any() if z_min == R else True
                seen, dropped = seen + int(got[0][..., 0].sum()), dropped + int(got[2])
    assert seen > 50 and dropped > 10
    few = sref.contacts(random_labels(R, 5), 4, 6)[0][..., 0].sum()
    assert few < sref.contacts(random_labels(R, 5), 4, 18)[0][..., 0].sum() < sref.contacts(random_labels(R, 5), 4, 26)[0][..., 0].sum()


def graph_restatement(pairs, floor, count, lean=0.25, min_contact=1, min_floor=1):
    """The graph rules over plain Python sets, round by round as the header words them."""
    P = len(floor)
    n = min(max(int(count), 0), P)

    def rests(c, a):
        N, D = int(pairs[a, c, 0]), int(pairs[a, c, 1]) - int(pairs[c, a, 1])
        return a != c and N >= min_contact and D > 0 and float(D) >= float(lean) * float(N)

    part = range(n)
    footings = {a: {c for c in part if rests(a, c)} for a in part}
    riders = {a: {c for c in part if rests(c, a)} for a in part}
    on_floor = {a: int(floor[a]) >= min_floor for a in part}
    out = {k: [0] * P for k in sref.COLUMNS}
    out['layer'] = [-1] * P
    for a in part:
        out['below'][a], out['above'][a] = len(footings[a]), len(riders[a])
        reach, edge = set(), {a}
        while edge:
            edge = {c for x in edge for c in riders[x]} - reach
            reach |= edge
        out['carried'][a] = len(reach - {a})
        F = {a}
        for _ in range(n):
            more = {c for c in part if c not in F and not on_floor[c] and footings[c] and footings[c] <= F}
            if not more:
                break
            F |= more
        out['orphans'][a] = len(F) - 1
    layer = {a: 0 for a in part if not riders[a]}
    for _ in range(n):
        ready = {a: 1 + max(layer[c] for c in riders[a]) for a in part if a not in layer and all(c in layer for c in riders[a])}
        layer.update(ready)
    grounded = {a for a in part if on_floor[a]}
    for _ in range(n):
        grounded |= {a for a in part if footings[a] & grounded}
    for a in part:
        out['layer'][a], out['grounded'][a] = layer.get(a, -1), int(a in grounded)
    rel = np.zeros((P, P), np.uint8)
    for a in part:
        for c in footings[a]:
            rel[a, c] = 1
    return {**{k: i32(v) for k, v in out.items()}, 'rests_on': rel}


def random_table(P, seed, dense=0.3, cyclic=False):
    """pairs [P,P,2], floor [P]: a random table, not one a label volume gives unless asked -- touch is symmetric only by construction."""
    rng = np.random.default_rng(seed)
    touch = rng.integers(1, 7, (P, P)) * (rng.random((P, P)) < (max(dense, 0.8) if cyclic else dense))
    touch = np.maximum(touch, touch.T) if seed % 2 else touch
    over = rng.integers(0, 7, (P, P))
    if not cyclic:
        over = np.triu(over)                                                   # only the larger label ever lies on the smaller: no cycle
    over = np.minimum(over, touch)
    pairs = np.stack([touch, over], -1).astype(i32)
    pairs[np.arange(P), np.arange(P)] = (3, 2)                                 # the diagonal is never read as a contact
    return pairs, (rng.integers(0, 3, P) * (rng.random(P) < 0.4)).astype(i32)


PARAMS = (dict(), dict(lean=0.0), dict(lean=1.0, min_floor=2), dict(lean=0.5, min_contact=3))


@pytest.mark.parametrize('P', [1, 2, 5, 17])
def test_the_graph_equals_its_literal_restatement(P):
    edges = cycles = 0
    for seed in range(6):
        pairs, floor = random_table(P, 100 * P + seed, dense=0.5 if P < 17 else 0.15, cyclic=seed >= 4)
        for count in (P, P - 1, 0, P + 3, -2):
            for p in PARAMS:
                got, want = sref.support(pairs, floor, count, **p), graph_restatement(pairs, floor, count, **p)
                for k in KEYS:
                    same((P, seed, count, p, k), got[k], want[k])
                edges, cycles = edges + int(got['rests_on'].sum()), cycles + int((got['layer'][:max(0, min(count, P))] < 0).sum())
                n = max(0, min(count, P))
                assert not got['rests_on'][n:].any() and not got['rests_on'][:, n:].any() and (got['layer'][n:] == -1).all()
                assert not (got['rests_on'] & got['rests_on'].T).any(), 'never both ways'
    assert P < 5 or (edges > 20 and cycles > 0)


def lattice_of(R, voxels):
    lab = np.zeros((R, R, R), i32)
    for at, L in voxels.items():
        lab[at] = L
    return lab


@functools.lru_cache(maxsize=None)
def piles():
    """test_grasp_retreat.py's 40^3 piles and `leaning`, a ball of radius 7 at (20, 23, 19) on a ball of radius 7 at (20, 13, 9):
    name -> (vol, labels, bbox, voxels, count, z_min), the labels parts_reference's, 26-connected, neck 0.8."""
    out = {k: v + (z,) for (k, v), z in zip(tgr.scenes().items(), (3, 0, 5))}
    assert list(out) == ['sphere_on_box', 'pile', 'side_by_side']
    vol = tgr.mask_volume(tgr.ball(40, (20, 13, 9), 7) | tgr.ball(40, (20, 23, 19), 7))
    w = pref.parts(pref.d2_free(vol[None]), max_parts=8)
    out['leaning'] = (vol, w['labels'][0], w['bbox'][0], w['voxels'][0], int(w['count'][0]), 2)
    for a in out['leaning'][:4]:
        a.setflags(write=False)
    return out


def pile_support(name, P=8, connectivity=26, **params):
    _, lab, _, _, n, z_min = piles()[name]
    return sref.support_of_labels(lab, n, P, connectivity, z_min, **params)


def host_support(s, n, **params):
    """support.support_from_rows on the statement's arrays of one scene."""
    rows = {k: s[k][:n] for k in (*sref.COLUMNS, 'floor')}
    rows.update(pairs=s['pairs'][:n, :n], rests_on=s['rests_on'][:n, :n], dropped=i32([s['dropped']]), count=i32([n]))
    return support.support_from_rows(rows, **params)


def test_the_synthetic_piles():
    """What the statement says of the piles at 40^3: (touch, over[a,b], over[b,a]) per pair of labels, and the graph."""
    table = lambda s, a, b: (int(s['pairs'][a - 1, b - 1, 0]), int(s['pairs'][a - 1, b - 1, 1]), int(s['pairs'][b - 1, a - 1, 1]))
    col = lambda s, k, n: [int(x) for x in s[k][:n]]
    s = pile_support('sphere_on_box')
    assert table(s, 1, 2) == (333, 333, 0) and s['dropped'] == 0 and col(s, 'floor', 2) == [289, 0]
    assert s['rests_on'][1, 0] == 1 and s['rests_on'].sum() == 1, 'the ball rests on the box'
    assert col(s, 'orphans', 2) == [1, 0] and col(s, 'carried', 2) == [1, 0] and col(s, 'layer', 2) == [1, 0]
    assert col(s, 'below', 2) == [0, 1] and col(s, 'above', 2) == [1, 0] and col(s, 'grounded', 2) == [1, 1]
    assert (s['layer'][2:] == -1).all() and not any(s[k][2:].any() for k in sref.COLUMNS if k != 'layer')
    # the pile: the top ball rests on all three; they touch each other sideways
    s = pile_support('pile')
    lab = piles()['pile'][1]
    top = int(lab[20, 18, 20])
    assert top == 3 and table(s, 1, 3) == (117, 99, 0) and table(s, 2, 3) == (129, 107, 0) and table(s, 4, 3) == (122, 103, 0)
    assert table(s, 1, 2) == (116, 38, 38) and table(s, 2, 4) == (116, 38, 38) and table(s, 1, 4) == (9, 3, 3)
    assert col(s, 'floor', 4) == [1, 1, 0, 1] and col(s, 'below', 4) == [0, 0, 3, 0] and col(s, 'above', 4) == [1, 1, 0, 1]
    assert col(s, 'orphans', 4) == [0, 0, 0, 0] and col(s, 'layer', 4) == [1, 1, 0, 1] and col(s, 'grounded', 4) == [1, 1, 1, 1]
    assert col(s, 'carried', 4) == [1, 1, 0, 1]
    assert support.take_order(host_support(s, 4))[0] == top
    # side by side: a contact and no relation
    s = pile_support('side_by_side')
    assert table(s, 1, 2) == (9, 3, 3) and not s['rests_on'].any() and col(s, 'floor', 2) == [1, 1]
    assert col(s, 'layer', 2) == [0, 0] and col(s, 'grounded', 2) == [1, 1] and not s['orphans'].any() and not s['carried'].any()
    # leaning: the balls meet over an edge of the lattice only
    s = pile_support('leaning')
    assert piles()['leaning'][4] == 2 and table(s, 1, 2) == (52, 52, 0) and s['rests_on'][1, 0] == 1 and col(s, 'floor', 2) == [1, 0]
    assert col(s, 'orphans', 2) == [1, 0] and col(s, 'carried', 2) == [1, 0] and col(s, 'layer', 2) == [1, 0] and col(s, 'grounded', 2) == [1, 1]
    s = pile_support('leaning', connectivity=6)
    assert not s['pairs'].any() and not s['rests_on'].any() and col(s, 'grounded', 2) == [1, 0], 'no contact at all under connectivity 6'
    # the default lean lies between every side contact and every resting contact of these piles
    for name in piles():
        s = pile_support(name)
        touch, over = s['pairs'][..., 0].astype(f64), s['pairs'][..., 1].astype(f64)
        share = np.abs(over - over.T)[touch > 0] / touch[touch > 0]
        assert ((share == 0.0) | (share > 0.8)).all() and sref.DEFAULTS['lean'] == 0.25, (name, share)


def test_a_column_of_one_voxel_parts():
    R = 32
    lab = lattice_of(R, {(5, 6, k): k + 1 for k in range(R)})
    s = sref.support_of_labels(lab, R, R)
    down = np.arange(R - 1, -1, -1, dtype=i32)
    for k in ('layer', 'carried', 'orphans'):
        same(k, s[k], down)
    same('below', s['below'], i32([0] + [1] * (R - 1)))
    same('above', s['above'], i32([1] * (R - 1) + [0]))
    assert s['grounded'].all() and s['floor'][0] == 1 and s['floor'].sum() == 1 and s['dropped'] == 0
    assert support.take_order(host_support(s, R)) == list(range(R, 0, -1))
    # half the rows: the labels beyond them are dropped, both ways
    half = sref.support_of_labels(lab, R, R // 2)
    assert half['dropped'] == 2 * (R // 2) and (half['layer'] == down[R // 2:]).all()
    with pytest.raises(_lib.GnrError, match='raise max_parts'):
        host_support(half, R // 2)


def cycle_scene():
    """R = 8: three upright stacks of two voxels far from each other -- 1 over 2, 2 over 3, 3 over 1 --, each label one voxel in two
    stacks; label 4 rests on label 1's upper voxel; label 5 floats."""
    return lattice_of(8, {(1, 1, 1): 2, (1, 1, 2): 1, (1, 1, 3): 4, (4, 4, 1): 3, (4, 4, 2): 2, (6, 1, 4): 1, (6, 1, 5): 3, (6, 6, 6): 5})


def test_a_cycle_and_a_floating_part():
    s = sref.support_of_labels(cycle_scene(), 5, 5, z_min=1)
    rel = np.zeros((5, 5), np.uint8)
    rel[0, 1] = rel[1, 2] = rel[2, 0] = rel[3, 0] = 1
    same('relation', s['rests_on'], rel)
    same('layer', s['layer'], i32([-1, -1, -1, 0, 0]))
    same('carried', s['carried'], i32([3, 3, 3, 0, 0]))
    same('floor', s['floor'], i32([0, 1, 1, 0, 0]))
    same('grounded', s['grounded'], i32([1, 1, 1, 1, 0]))
    same('orphans', s['orphans'], i32([1, 2, 0, 0, 0]))                        # 1 takes 4 along; 2 takes 1, which takes 4; 3 carries 2, which stands on the floor
    h = host_support(s, 5)
    assert support.take_order(h) == [4, 5] and h['grounded'].dtype == bool and not h['grounded'][4] and h['on_floor'].tolist() == [False, True, True, False, False]


def test_the_lean_on_its_boundary():
    """D == lean * N holds; the next double above the ratio does not."""
    pairs = np.zeros((2, 2, 2), i32)
    pairs[0, 1], pairs[1, 0] = (4, 2), (4, 1)                                  # N = 4, D = 1
    floor = i32([1, 0])
    assert sref.support(pairs, floor, 2, lean=0.25)['rests_on'][1, 0] == 1
    assert not sref.support(pairs, floor, 2, lean=np.nextafter(0.25, 1.0))['rests_on'].any()
    assert sref.support(pairs, floor, 2, lean=np.nextafter(0.25, 0.0))['rests_on'][1, 0] == 1
    pairs[1, 0, 1] = 2                                                         # D = 0: never, not even at lean 0
    assert not sref.support(pairs, floor, 2, lean=0.0)['rests_on'].any()
    pairs[0, 1], pairs[1, 0] = (3, 3), (3, 2)                                  # N = 3, D = 1: 1 >= (1/3) * 3 in doubles
    assert sref.support(pairs, floor, 2, lean=1.0 / 3.0)['rests_on'][1, 0] == (1.0 >= (1.0 / 3.0) * 3.0)
    assert not sref.support(pairs, floor, 2, min_contact=4)['rests_on'].any()


def test_host_functions():
    s = pile_support('pile')
    h = host_support(s, 4)
    assert list(h) == ['rests_on', 'touch', 'floor', 'on_floor', 'below', 'above', 'carried', 'orphans', 'layer', 'grounded']
    assert h['rests_on'].dtype == bool and h['rests_on'].shape == (4, 4) and h['touch'].dtype == i32 and h['on_floor'].tolist() == [True, True, False, True]
    assert all(h[k].dtype == i32 and h[k].shape == (4,) for k in ('floor', 'below', 'above', 'carried', 'orphans', 'layer'))
    assert support.take_order(h) == [3, 1, 2, 4] and support.take_order(dict(layer=i32([2, -1, 0, 0, 1]))) == [3, 4, 5, 1]
    # without the device's relation the host applies the rule to the table: the same
    rows = {k: s[k][:4] for k in (*sref.COLUMNS, 'floor')}
    rows.update(pairs=s['pairs'][:4, :4], dropped=i32([0]), count=i32([4]))
    same('host relation', support.support_from_rows(rows)['rests_on'], h['rests_on'])
    assert not support.support_from_rows(rows, lean=0.9)['rests_on'].any()
    with pytest.raises(_lib.GnrError, match='5 parts but the support tables hold 4: raise max_parts'):
        support.support_from_rows(dict(rows, count=i32([5])))
    with pytest.raises(_lib.GnrError, match='more than 256 parts'):
        support.support_from_rows(dict(rows, count=i32([300])), max_parts=256)
    with pytest.raises(_lib.GnrError, match='6 contacts of labels beyond the 4 rows of the support tables were dropped: raise max_parts'):
        support.support_from_rows(dict(rows, dropped=i32([6])))
    # the grasps' columns: numpy, and torch (a gather) with a batch axis
    part = i32([3, 1, 0, 4, 9, -2, 2])
    cols = support.grasp_support_columns(part, h)
    assert list(cols) == ['part_above', 'part_carried', 'part_orphans', 'part_layer', 'part_grounded']
    same('above', cols['part_above'], i32([0, 1, 0, 1, 0, 0, 1]))
    same('carried', cols['part_carried'], i32([0, 1, 0, 1, 0, 0, 1]))
    same('orphans', cols['part_orphans'], i32([0] * 7))
    same('layer', cols['part_layer'], i32([0, 1, -1, 1, -1, -1, 1]))
    same('grounded', cols['part_grounded'], np.array([True, True, False, True, False, False, True]))
    dev = {k: torch.from_numpy(np.stack([s[k], s[k][::-1].copy()])) for k in sref.COLUMNS}
    tcols = support.grasp_support_columns(torch.from_numpy(np.stack([part, part])), dev)
    for k, v in cols.items():
        same(('torch', k), tcols[k][0].numpy(), v)
    assert tcols['part_layer'][1].tolist() == [-1, -1, -1, -1, -1, -1, -1] and tcols['part_above'].dtype == torch.int32      # (rows 8..5 reversed: empty)
    none = support.grasp_support_columns(np.zeros(0, i32), h)
    assert all(len(v) == 0 for v in none.values()) and none['part_grounded'].dtype == bool
    # the best grasp of every part that comes out and carries nothing
    columns = dict(part=i32([1, 3, 3, 0, 2, 1]), retreat_free=np.array([True, False, True, True, True, True]), part_carried=i32([1, 0, 0, 0, 0, 0]))
    assert retreat.best_free_per_part(columns) == {1: 0, 3: 2, 2: 4} and support.best_clear_per_part(columns) == {3: 2, 2: 4, 1: 5}
    assert support.best_clear_per_part(dict(object=columns['part'], retreat_free=columns['retreat_free'], part_carried=i32([1] * 6))) == {}


def test_support_params():
    want = dict(lean=0.25, min_contact=1, min_floor=1)
    assert support.support_params(False) is None and support.support_params(None) is None
    assert support.support_params(True) == want == support.support_params({}) == support.SUPPORT_DEFAULTS == support.checked_support() == sref.DEFAULTS
    p = support.support_params(dict(lean=1, min_floor=3, filter=True), filter=False)
    assert p == dict(want, lean=1.0, min_floor=3, filter=True) and isinstance(p['lean'], float) and isinstance(p['min_floor'], int)
    with pytest.raises(TypeError, match='unknown support parameters'):
        support.support_params(dict(neck=0.8))
    for bad, text in ((dict(lean=-0.1), 'support lean must be finite and in 0..1'), (dict(lean=1.5), 'support lean must be finite and in 0..1'),
                      (dict(lean=math.nan), 'support lean must be finite and in 0..1'), (dict(lean=True), 'support lean must be finite and in 0..1'),
                      (dict(min_contact=0), 'support min_contact must be an integer >= 1, got 0'), (dict(min_contact=1.5), 'support min_contact must be an integer >= 1'),
                      (dict(min_floor=0), 'support min_floor must be an integer >= 1, got 0'), (dict(min_floor=True), 'support min_floor must be an integer >= 1')):
        with pytest.raises(ValueError, match=text):
            support.support_params(bad)
    for cls, keys in ((support.PartSupport, (*want, 'relation')), (support.PartContacts, ('max_parts', 'connectivity', 'z_min'))):
        params = inspect.signature(cls.__call__).parameters
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keys)
    assert {k: v.default for k, v in inspect.signature(support.PartSupport.__call__).parameters.items() if k in want} == want
    assert support.MAX_PARTS == _lib.GNR_SUPPORT_MAX_PARTS == sref.MAX_PARTS == 256
    for bad in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match='support max_parts must be an integer in 1..256'):
            support.checked_rows(bad)
    g = dict(index=np.zeros((0, 3)), quat=np.zeros((0, 4)), width=np.zeros(0))
    with pytest.raises(TypeError, match='unknown support parameters'):
        support.support_of_plan(np.ones((4, 4, 4), f32), g, iso=0.0)
    with pytest.raises(ValueError, match='support lean must be finite and in 0..1'):
        support.support_of_plan(np.ones((4, 4, 4), f32), g, lean=2.0)
    with pytest.raises(ValueError, match='retreat tolerance must be an integer >= 0'):
        support.support_of_plan(np.ones((4, 4, 4), f32), g, tolerance=-2)
    with pytest.raises(ValueError, match='support z_min must be an integer >= 0'):
        support.support_of_plan(np.ones((4, 4, 4), f32), g, z_min=-1)


def test_part_support_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for cls in (support.PartContacts, support.PartSupport):
        with pytest.raises(_lib.GnrError, match='no CPU fallback'):
            cls()


# ---- 2. the refusals of the two entry points ------------------------------------------------------------------------------------------
CONTACT_PTRS = ('labels', 'pairs', 'floor', 'dropped')
SUPPORT_PTRS = ('pairs', 'floor', 'count', 'below', 'above', 'carried', 'orphans', 'layer', 'grounded')
ROWS_TEXT = ': max_parts must be in 1..GNR_SUPPORT_MAX_PARTS (256)'


def _contact_refusals(ptr, B=1, R=8, P=4):
    """Every refusal of gnr_part_contacts_fwd, each with its code and its text, and their order, on the pointers given (fake ones, or
    buffers whose bytes the caller checks afterwards)."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_part_contacts_fwd'

    def call(p=None, B=B, R=R, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in CONTACT_PTRS}
        p = _lib.GnrContactsParams(**{**dict(connectivity=26, max_parts=P, z_min=0), **kw}) if p is None else p
        return L.gnr_part_contacts_fwd(C.byref(p) if p is not False else None, a['labels'], B, R, a['pairs'], a['floor'], a['dropped'], None)

    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for r in (1, 0, 257):
        assert call(R=r) == _lib.GNR_ERR_SHAPE and text() == fn + ': R must be in 2..256', r
    for m in (0, -1, 257):
        assert call(max_parts=m) == _lib.GNR_ERR_SHAPE and text() == fn + ROWS_TEXT, m
    for c in (0, 7, 27, -6):
        assert call(connectivity=c) == _lib.GNR_ERR_ARG and text() == fn + ': connectivity must be 6, 18 or 26', c
    for z in (-1, R + 1):
        assert call(z_min=z) == _lib.GNR_ERR_ARG and text() == fn + ': z_min must be in 0..R', z
    for name in CONTACT_PTRS:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    # the order: of two faults the one the header names first is reported
    faults = (dict(B=0), dict(R=1), dict(max_parts=257), dict(connectivity=5), dict(z_min=-1), dict(labels=None))
    texts = (': B must be in 1..65535', ': R must be in 2..256', ROWS_TEXT, ': connectivity must be 6, 18 or 26', ': z_min must be in 0..R', ': null pointer')
    for i in range(len(faults)):
        for j in range(i + 1, len(faults)):
            assert call(**faults[i], **faults[j]) != _lib.GNR_OK and text() == fn + texts[i], (i, j)


def _support_refusals(ptr, B=1, P=4):
    """Every refusal of gnr_part_support_fwd; rests_on may be null."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_part_support_fwd'

    def call(p=None, B=B, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in SUPPORT_PTRS}
        rel = kw.pop('rests_on', ptr.get('rests_on'))
        p = _lib.GnrSupportParams(**{**dict(lean=0.25, max_parts=P, min_contact=1, min_floor=1), **kw}) if p is None else p
        return L.gnr_part_support_fwd(C.byref(p) if p is not False else None, a['pairs'], a['floor'], a['count'], B, *(a[k] for k in SUPPORT_PTRS[3:]), rel, None)

    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for m in (0, -1, 257):
        assert call(max_parts=m) == _lib.GNR_ERR_SHAPE and text() == fn + ROWS_TEXT, m
    for m in (0, -3):
        assert call(min_contact=m) == _lib.GNR_ERR_ARG and text() == fn + ': min_contact must be >= 1', m
        assert call(min_floor=m) == _lib.GNR_ERR_ARG and text() == fn + ': min_floor must be >= 1', m
    for bad in (-0.01, 1.01, math.nan, math.inf, -math.inf):
        assert call(lean=bad) == _lib.GNR_ERR_ARG and text() == fn + ': lean must be finite and in 0..1', bad
    for name in SUPPORT_PTRS:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    faults = (dict(B=0), dict(max_parts=0), dict(min_contact=0), dict(min_floor=0), dict(lean=2.0), dict(count=None))
    texts = (': B must be in 1..65535', ROWS_TEXT, ': min_contact must be >= 1', ': min_floor must be >= 1', ': lean must be finite and in 0..1', ': null pointer')
    for i in range(len(faults)):
        for j in range(i + 1, len(faults)):
            assert call(**faults[i], **faults[j]) != _lib.GNR_OK and text() == fn + texts[i], (i, j)


def test_refusals_before_the_device():
    one = C.c_void_p(16)
    _contact_refusals({k: one for k in CONTACT_PTRS})
    _support_refusals({k: one for k in (*SUPPORT_PTRS, 'rests_on')})
    _support_refusals({k: one for k in SUPPORT_PTRS})


def test_a_refused_call_writes_nothing_without_a_device():
    """The same refusals on host buffers of 0x5a bytes: a refused call has launched nothing and the host side writes nothing."""
    bufs = {k: np.full(4096, SENTINEL, np.uint8) for k in (*CONTACT_PTRS, *SUPPORT_PTRS, 'rests_on')}
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    _contact_refusals(ptr)
    _support_refusals(ptr)
    for k, v in bufs.items():
        assert (v == SENTINEL).all(), k


# ---- GPU: the bits of the statement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ops():
    return support.PartContacts(), support.PartSupport()


def check_contacts(what, labels, P, connectivity=26, z_min=0):
    """PartContacts on B scenes, its output tensors filled with 0x5a bytes before the call, against the statement: every element is
    written.  -> the statement's (pairs, floor, dropped), per scene."""
    op = _ops()[0]
    labels = np.asarray(labels, i32)
    kw = dict(max_parts=P, connectivity=connectivity, z_min=z_min)
    for k in ('pairs', 'floor', 'dropped'):
        op(labels, **kw)[k].view(torch.uint8).fill_(SENTINEL)                  # (the tensors of this shape)
    res = op(labels, **kw)
    torch.cuda.synchronize()
    want = [sref.contacts(lab, P, connectivity, z_min) for lab in labels]
    for k, at in (('pairs', 0), ('floor', 1), ('dropped', 2)):
        same((what, k), res[k].cpu().numpy(), np.stack([w[at] for w in want]))
    return want


def check_support(what, pairs, floor, counts, **params):
    """PartSupport on B tables, sentinels first, against the statement, the relation included and the rows beyond the parts."""
    op = _ops()[1]
    con = dict(pairs=torch.from_numpy(np.ascontiguousarray(pairs, i32)).to('cuda:0'), floor=torch.from_numpy(np.ascontiguousarray(floor, i32)).to('cuda:0'))
    count = torch.tensor(list(counts), dtype=torch.int32, device='cuda:0')
    for k in KEYS:
        op(con, count, relation=True, **params)[k].view(torch.uint8).fill_(SENTINEL)
    res = op(con, count, relation=True, **params)
    torch.cuda.synchronize()
    want = [sref.support(pairs[b], floor[b], counts[b], **params) for b in range(len(counts))]
    for k in KEYS:
        same((what, k), res[k].cpu().numpy(), np.stack([w[k] for w in want]))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 3, 5, 8, 13])
def test_random_labels(R):
    """Three scenes per call with other labels in each, so any wrap into a neighbouring row, plane or scene shows; labels beyond the
    rows; then the graph of those tables."""
    labels = np.stack([random_labels(R, 100 * R), random_labels(R, 100 * R + 1, 3, 6), random_labels(R, 100 * R + 2, -1, 2)])
    dropped = 0
    for connectivity in (6, 18, 26):
        for z_min in (0, R // 2, R):
            want = check_contacts((R, connectivity, z_min), labels, 4, connectivity, z_min)
            dropped += int(want[0][2]) + int(want[1][2])
            assert want[2][2] == 0
            pairs, floor = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
            check_support((R, connectivity, z_min), pairs, floor, (4, 6, 2))
    assert dropped > 0


@pytest.mark.gpu
def test_many_keys_in_a_wavefront():
    """R = 16, labels uniform in 1..256 at 256 rows: up to 64 distinct keys per wavefront and direction."""
    labels = np.stack([random_labels(16, s, 1, 256) for s in (1, 2)])
    for connectivity in (6, 26):
        want = check_contacts(('keys', connectivity), labels, 256, connectivity, 3)
        assert want[0][2] == 0 and want[0][0][..., 0].sum() > 16 ** 3 * (3 if connectivity == 6 else 13)
    want = check_contacts('keys', labels, 100, 18, 15)
    assert want[0][2] > 0


@pytest.mark.gpu
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_two_solid_halves(axis):
    """R = 16 split into two solid labels by a plane: hundreds of equal keys in every wavefront; two single voxels in opposite corners
    touch nothing."""
    R = 16
    lab = np.ones((R, R, R), i32)
    np.moveaxis(lab, axis, 0)[R // 2:] = 2
    far = lattice_of(R, {(0, 0, 0): 1, (R - 1, R - 1, R - 1): 2})
    for connectivity, per_voxel in ((6, 1), (18, 5), (26, 9)):
        want = check_contacts(('halves', axis, connectivity), np.stack([lab, far, lab[::-1].copy()]), 2, connectivity, 0)
        pairs = want[0][0]
        assert pairs[0, 1, 0] == pairs[1, 0, 0] and R * R <= pairs[0, 1, 0] <= R * R * per_voxel
        if axis == 2:
            assert (pairs[0, 1, 1], pairs[1, 0, 1]) == (pairs[0, 1, 0], 0), 'label 2 lies on label 1 at every contact'
        else:
            assert pairs[0, 1, 1] == pairs[1, 0, 1] and (pairs[0, 1, 1] > 0) == (connectivity != 6), 'side by side: as many up as down'
        assert not want[1][0].any() and want[1][1].tolist() == [1, 0], 'opposite corners: no contact; one voxel on the floor'
        check_support(('halves', axis), np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), (2, 2, 2))


def chain_table(order):
    """P = len(order) parts in one chain written straight into the table: order[i + 1] rests on order[i]; order[0] stands on the floor."""
    P = len(order)
    pairs, floor = np.zeros((P, P, 2), i32), np.zeros(P, i32)
    for lo, hi in zip(order[:-1], order[1:]):
        pairs[lo, hi], pairs[hi, lo] = (1, 1), (1, 0)
    floor[order[0]] = 1
    return pairs, floor


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 2, 5, 64, 256])
def test_the_graph_alone(P):
    """gnr_part_support_fwd on tables no label volume gave: random ones with and without cycles, counts beyond the rows and below
    zero, and at 256 rows a chain through every part -- ascending, descending and shuffled, so every closure runs its full length."""
    for seed in (0, 1):
        tabs = [random_table(P, 10 * P + 3 * seed + b, dense=min(0.5, 6.0 / P), cyclic=b == 2) for b in range(3)]
        pairs, floor = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
        cycles = 0
        for p in PARAMS[:2] if P > 5 else PARAMS:
            want = check_support((P, seed, p), pairs, floor, (P, P + 7, P - 1), **p)
            check_support((P, seed, p, 'few'), pairs, floor, (0, -3, (P + 1) // 2), **p)
            cycles += int((want[2]['layer'][:P - 1] < 0).sum())
        assert P < 64 or cycles > 0, 'the third table has a cycle'
    if P >= 64:
        full = np.stack([np.full((P, P), 5), np.random.default_rng(P).integers(0, 6, (P, P))], -1).astype(i32)      # a tournament: cycles everywhere
        want = check_support((P, 'cycles'), np.stack([full] * 3), np.ones((3, P), i32), (P, P, 3))
        assert (want[0]['layer'] < 0).sum() > P // 2
        orders = [list(range(P)), list(range(P - 1, -1, -1)), np.random.default_rng(7).permutation(P).tolist()]
        tabs = [chain_table(o) for o in orders]
        want = check_support((P, 'chain'), np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), (P, P, P))
        for o, w in zip(orders, want):
            assert w['layer'][o].tolist() == list(range(P - 1, -1, -1)) == w['carried'][o].tolist() == w['orphans'][o].tolist() and w['grounded'].all()


@pytest.mark.gpu
def test_the_column_and_the_cycle_on_the_device():
    R = 32
    lab = lattice_of(R, {(5, 6, k): k + 1 for k in range(R)})
    big = np.zeros((R, R, R), i32)
    big[:8, :8, :8] = cycle_scene()
    want = check_contacts('column', np.stack([lab, big]), R, 26, 0)
    check_support('column', np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), (R, 5))
    want = check_contacts('cycle', cycle_scene()[None], 5, 26, 1)
    w = check_support('cycle', want[0][0][None], want[0][1][None], (5,))[0]
    assert w['layer'].tolist() == [-1, -1, -1, 0, 0] and w['grounded'].tolist() == [1, 1, 1, 1, 0]


def plan_of(name):
    """tgr.plan_of's grasps on any of the piles: at every part's box centre, straight down, leaning both ways and from the side, and
    one in empty space."""
    vol, lab, bbox, voxels, n, z_min = piles()[name]
    index, quat = [], []
    for L in range(n):
        for q in (tgr.DOWN, tgr.tilted(20), tgr.tilted(-20), tgr.ALONG[0, 1, 0]):
            index.append((bbox[L, :3] + bbox[L, 3:]) // 2)
            quat.append(q)
    index.append((36, 36, 36))
    quat.append(tgr.DOWN)
    return dict(index=np.int64(index), quat=np.stack(quat).astype(f64), width=np.full(len(index), 10.0, f32) * f32(VOXEL))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['sphere_on_box', 'pile', 'side_by_side', 'leaning'])
def test_support_of_plan(name):
    vol, lab, bbox, voxels, n, z_min = piles()[name]
    g = plan_of(name)
    got, cols = support.support_of_plan(np.array(vol), g, voxel_size=VOXEL, max_parts=8, z_min=z_min)
    assert got['count'] == n and np.array_equal(got['labels'], lab) and np.array_equal(got['voxels'], voxels[:n])
    s = sref.support_of_labels(lab, n, 8, 26, z_min)
    want = host_support(s, n)
    for k, w in want.items():
        same((name, k), got[k], w)
    w_vox = (g['width'] / f32(VOXEL)).astype(f32)
    held = i32([oref.grasp_object(lab, g['index'][r].astype(f64), g['quat'][r].astype(f32), w_vox[r], VOXEL)[0] for r in range(len(w_vox))])
    assert np.array_equal(cols['part'], held) and held[-1] == 0
    for k, w in support.grasp_support_columns(held, want).items():
        same((name, k), cols[k], w)
    rows = retreat.retreat_from_rows(dict(zip(rref.KEYS, rref.retreat_rows(lab, bbox, held, g['quat'].astype(f32), len(held), VOXEL))))
    for k, w in rows.items():
        same((name, k), tgr.bits(cols[k]), tgr.bits(w))
    clear, order = support.best_clear_per_part(cols), support.take_order(got)
    print(name, held, cols['part_carried'], clear, order)
    if name == 'sphere_on_box':
        assert order == [2, 1] and set(clear) == {2}
    if name == 'pile':
        assert order[0] == 3 and set(clear) == {3} and (cols['part_carried'][(held > 0) & (held != 3)] == 1).all()
    if name == 'side_by_side':
        assert order == [1, 2] and set(clear) == {1, 2}
    if name == 'leaning':
        assert order == [2, 1] and 1 not in clear and (cols['part_orphans'][held == 1] == 1).all()
    with pytest.raises(_lib.GnrError, match='raise max_parts'):
        support.support_of_plan(np.array(vol), g, voxel_size=VOXEL, max_parts=1, z_min=z_min)


@pytest.mark.gpu
def test_one_captured_graph_from_the_volume_to_the_support_columns():
    """VolumeDistance, VolumeParts, GraspObjects, GraspRetreat, PartContacts, PartSupport and the gather of the grasps' columns captured
    once on one stream, replayed after the input volume changed, and replayed twice on the same input: the bits of the statement at
    every replay."""
    R, n, dev, scale, M = 17, 10, 'cuda:0', 0.02, 64
    rng = np.random.default_rng(31)

    def blobs(seed):
        r = np.random.default_rng(seed)
        return np.stack([tgr.mask_volume(functools.reduce(np.logical_or, [tgr.ball(R, r.uniform(3, R - 4, 3), r.uniform(2.0, 4.5)) for _ in range(5)])) for _ in range(2)])

    volumes = [blobs(s) for s in (1, 2, 3)]
    pos, width = rng.uniform(3.0, R - 4.0, (2, n, 3)), rng.uniform(2.0, 9.0, (2, n)).astype(f32)
    quat = rng.normal(size=(2, n, 4)).astype(f32)
    quat[:, :4] = tgr.DOWN
    vol = torch.from_numpy(volumes[0]).to(dev)
    Pos, Q, W = (torch.from_numpy(a).to(dev) for a in (pos, quat, width))
    counts = (n, n - 3)
    count = torch.tensor(counts, dtype=torch.int32, device=dev)
    kw = dict(connectivity=26, max_parts=M, neck=0.8)

    def run(a, b, c, d, e):
        field = a(vol, scale=scale, z_min=1)
        res = b(field['d2_free'], **kw)
        gres = c(res['labels'], Pos, Q, W, count, scale=scale, depth=0.08)
        rres = d.of_parts(res, gres, dict(quat=Q, count=count), scale=scale, tolerance=1)
        sres = e.of_parts(res, connectivity=26, z_min=1, relation=True)
        return res, gres, rres, sres, support.grasp_support_columns(gres['object'], sres)

    ops = distance.VolumeDistance(), parts.VolumeParts(), objects.GraspObjects(), retreat.GraspRetreat(), support.PartSupport()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*ops)                                                              # sizes the workspaces and the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, gres, rres, sres, gcols = run(*ops)
    edges, first = 0, None
    for s in (volumes[1], volumes[2], volumes[2]):
        vol.copy_(torch.from_numpy(s).to(dev))
        for t in (*(sres[k] for k in (*KEYS, 'pairs', 'floor', 'dropped')), *gcols.values()):
            t.view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = pref.parts(pref.d2_free(s, z_min=1), **kw)
        assert np.array_equal(res['labels'].cpu().numpy(), want['labels'])
        bits = {}
        for b in range(2):
            w = sref.support_of_labels(want['labels'][b], want['count'][b], M, 26, 1)
            for k in (*KEYS, 'pairs', 'floor', 'dropped'):
                same(('replay', b, k), sres[k][b].cpu().numpy(), w[k])
            held = oref.grasp_objects(want['labels'][b], pos[b], quat[b], width[b], counts[b], scale, depth=0.08)[0]
            assert np.array_equal(gres['object'][b, :counts[b]].cpu().numpy(), held[:counts[b]])
            cols = support.grasp_support_columns(gres['object'][b].cpu().numpy(), {k: w[k] for k in sref.COLUMNS})
            for k, v in cols.items():
                same(('replay', b, k), gcols[k][b].cpu().numpy(), v)
                bits[b, k] = gcols[k][b].cpu().numpy()
            edges += int(w['rests_on'].sum())
        if s is volumes[2]:
            if first is None:
                first = bits
            else:
                assert all(np.array_equal(first[k], bits[k]) for k in bits), 'the same graph on the same input: the same bits'
    print(edges)
    assert edges > 2, 'hardly a part rests on another'


@pytest.mark.gpu
def test_a_refused_call_writes_nothing():
    B, R, P = 1, 8, 4
    fill = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    sizes = dict(labels=4 * R ** 3, pairs=8 * P * P, floor=4 * P, dropped=4, count=4, rests_on=P * P, **{k: 4 * P for k in sref.COLUMNS})
    bufs = {k: fill(v) for k, v in sizes.items()}
    ptr = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    _contact_refusals(ptr, B=B, R=R, P=P)
    _support_refusals(ptr, B=B, P=P)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == SENTINEL).all()), k
