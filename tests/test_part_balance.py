"""Balance of the parts (csrc/gnr_balance.hip, balance.PartFeet, balance.PartBalance, balance.balance_of_plan).
tests/balance_reference.py is the statement (numpy integers, one float64 multiply and one divide per direction of a margin); every
comparison is np.array_equal, dtypes and shapes included, the margin by its bits.  Without a GPU: the statement against a literal
restatement one voxel and one neighbour at a time, the balance rule against plain Python integers and fractions, what the statement says
of the synthetic piles, a bridge and an overhang, the host functions, the parameter checks, every refusal of the two entry points.  On
the GPU: shapes chosen to break the kernels -- unconnected random labels next to other scenes under relations of random bytes, 256
labels cycling through one small scene, two solid halves, one solid 128^3 whose sums of squares pass 2^32, tables written by hand --
rather than to resemble the workload, then a plan's route and one captured graph from the volume to the grasps' balance columns."""
import ctypes as C
import fractions
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, balance, distance, objects, parts, support
import balance_reference as bref
import parts_reference as pref
import support_reference as sref
import test_grasp_retreat as tgr
import test_part_support as tps

f32, f64, i32, i64, u8 = np.float32, np.float64, np.int32, np.int64, np.uint8
VOXEL = tgr.VOXEL
SENTINEL = 0x5a
TABLES = ('moments', 'slots', 'feet', 'reach', 'crowded')
COLUMNS = (*bref.COLUMNS, 'tips')
NONE = np.iinfo(i32).min


def same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == f64:
        got, want = got.view(i64), want.view(i64)                              # by bits
    assert np.array_equal(got, want), (what, got, want)


def random_relation(P, seed, dense=0.3, nine=None):
    """rests_on [P,P] uint8: random bytes, not only 0 / 1, the diagonal set too (it is never read as a footing);  nine: a row that
    rests on nine others."""
    rng = np.random.default_rng(seed)
    rel = (rng.integers(1, 256, (P, P)) * (rng.random((P, P)) < dense)).astype(u8)
    rel[np.arange(P), np.arange(P)] = 7
    if nine is not None:
        rel[nine] = 0
        rel[nine, [a for a in range(P) if a != nine][:9]] = rng.integers(1, 256, 9)
    return rel


# ---- 1. the statement (no GPU) --------------------------------------------------------------------------------------------------------
def slots_restatement(rel, count):
    """include/gnr.h's words one footing at a time."""
    P = len(rel)
    n = min(max(int(count), 0), P)
    slots, crowded = [[0] * P for _ in range(P)], [0] * P
    for c in range(1, n + 1):
        footings = [a for a in range(1, n + 1) if rel[c - 1][a - 1] != 0 and a != c]
        for rank, a in enumerate(footings, 1):
            slots[c - 1][a - 1] = rank if rank < 7 else 7
        crowded[c - 1] = int(len(footings) > 7)
    return u8(slots).reshape(P, P), i32(crowded).reshape(P)


def feet_restatement(lab, slots, connectivity, z_min):
    """... one voxel and one neighbour at a time, in plain Python."""
    R, P = lab.shape[0], len(slots)
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    moments = [[0] * 10 for _ in range(P)]
    feet = [[0] * 8 for _ in range(P)]
    reach = [[[None] * 16 for _ in range(8)] for _ in range(P)]
    for i in range(R):
        for j in range(R):
            for k in range(R):
                c = int(lab[i, j, k])
                if not 1 <= c <= P:
                    continue
                for col, v in enumerate((1, i, j, k, i * i, j * j, k * k, i * j, i * k, j * k)):
                    moments[c - 1][col] += v
                mine = {0} if k == z_min else set()
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        for dk in (-1, 0, 1):
                            if not 1 <= (di != 0) + (dj != 0) + (dk != 0) <= most:
                                continue
                            wi, wj, wk = i + di, j + dj, k + dk
                            if not (0 <= wi < R and 0 <= wj < R and 0 <= wk < R) or not wk < k:
                                continue
                            a = int(lab[wi, wj, wk])
                            if 1 <= a <= P and a != c and slots[c - 1][a - 1] >= 1:
                                mine.add(int(slots[c - 1][a - 1]))
                for s in mine:
                    feet[c - 1][s] += 1
                    for q, (dx, dy) in enumerate(bref.DIRS):
                        p = int(dx) * i + int(dy) * j
                        reach[c - 1][s][q] = p if reach[c - 1][s][q] is None else max(reach[c - 1][s][q], p)
    reach = [[[NONE if v is None else v for v in row] for row in part] for part in reach]
    return i64(moments).reshape(P, 10), i32(feet).reshape(P, 8), i32(reach).reshape(P, 8, 16)


def test_the_directions():
    assert bref.DIRS[:8].tolist() == [[1, 0], [2, 1], [1, 1], [1, 2], [0, 1], [-1, 2], [-1, 1], [-2, 1]] and np.array_equal(bref.DIRS[8:], -bref.DIRS[:8])
    assert bref.LENGTH[:8].tolist() == [1.0, math.sqrt(5), math.sqrt(2), math.sqrt(5), 1.0, math.sqrt(5), math.sqrt(2), math.sqrt(5)]
    assert (math.sqrt(2), math.sqrt(5)) == (1.4142135623730951, 2.23606797749979) and bref.WIDTH[:8].tolist() == [1, 3, 2, 3, 1, 3, 2, 3]
    assert (bref.MAX_PARTS, bref.SLOTS, bref.DIRECTIONS) == (_lib.GNR_BALANCE_MAX_PARTS, _lib.GNR_BALANCE_SLOTS, _lib.GNR_BALANCE_DIRECTIONS) == (256, 8, 16)


@pytest.mark.parametrize('R', [2, 3, 5])
def test_the_feet_equal_their_literal_restatement(R):
    P = 11
    seen = shared = 0
    for seed in range(2):
        lab = tps.random_labels(R, 10 * R + seed, -1, P + 1)
        rel = random_relation(P, 20 * R + seed, nine=3 * seed)
        for count in (P, P - 2, 0, P + 3, -1):
            got, want = bref.slots(rel, count), slots_restatement(rel.tolist(), count)
            same((R, seed, count, 'slots'), got[0], want[0])
            same((R, seed, count, 'crowded'), got[1], want[1])
            for connectivity in (6, 18, 26):
                for z_min in (0, 1, R):
                    g = bref.feet(lab, got[0], connectivity, z_min)
                    w = feet_restatement(lab, want[0].tolist(), connectivity, z_min)
                    for k, a, b in zip(('moments', 'feet', 'reach'), g, w):
                        same((R, seed, count, connectivity, z_min, k), a, b)
                    assert not g[1][:, 0].any() if z_min == R else True
                    assert ((g[1] == 0) == (g[2] == NONE).all(2)).all() and ((g[1] == 0) == (g[2] == NONE).any(2)).all()
                    seen, shared = seen + int(g[1][:, 1:].sum()), shared + int(g[1][:, 7].sum())
            n, nine = max(0, min(count, P)), 3 * seed
            held = sum(a < n for a in [a for a in range(P) if a != nine][:9]) if nine < n else 0
            assert got[1][nine] == (held >= 8) and got[0][nine].max() == min(held, 7), 'the row with nine footings'
    assert seen > 20 and (R < 3 or shared > 0)


def rule_restatement(m, Si, Sj, feet, reach, chosen, min_floor=1):
    """The balance rule in Python integers; the margin in Python floats (IEEE doubles: the same two operations), and exactly, as a
    fraction over the direction's length squared, to bound the rounding."""
    use = [s for s in range(8) if chosen[s] and int(feet[s]) >= (min_floor if s == 0 else 1)]
    if m < 1 or not use:
        return False, -math.inf, None
    ok, least, exact = True, math.inf, math.inf
    for q, (dx, dy) in enumerate(bref.DIRS.tolist()):
        r = max(int(reach[s][q]) for s in use)
        num = m * (2 * r + abs(dx) + abs(dy)) - 2 * (dx * Si + dy * Sj)
        # the centre's coordinate along d, exactly, against the support function of the feet's unit squares
        inside = fractions.Fraction(dx * Si + dy * Sj, m) <= r + fractions.Fraction(abs(dx) + abs(dy), 2)
        assert inside == (num >= 0)
        ok = ok and num >= 0
        least = min(least, float(num) / (float(2 * m) * math.sqrt(dx * dx + dy * dy)))
        exact = min(exact, float(fractions.Fraction(num, 2 * m)) / math.sqrt(dx * dx + dy * dy))
    return ok, least, exact


def random_tables(P, seed, R=40):
    """moments, feet, reach of P parts that no label volume gave: centres anywhere in the lattice, feet anywhere."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 500, P) * (rng.random(P) < 0.9)
    moments = np.zeros((P, 10), i64)
    moments[:, 0], moments[:, 1], moments[:, 2] = m, m * rng.integers(0, R, P) + rng.integers(0, 2, P) * (m > 0), m * rng.integers(0, R, P)
    feet = (rng.integers(1, 9, (P, 8)) * (rng.random((P, 8)) < 0.4)).astype(i32)
    reach = np.full((P, 8, 16), NONE, i32)
    for c in range(P):
        for s in range(8):
            if feet[c, s]:
                pts = rng.integers(0, R, (int(feet[c, s]), 2))
                reach[c, s] = (pts @ bref.DIRS.T).max(0)
    return moments, feet, reach


def test_the_balance_rule_in_integers_and_fractions():
    tipped = steady = 0
    for seed in range(8):
        moments, feet, reach = random_tables(12, seed)
        for min_floor in (1, 3):
            ok = bref.usable(feet, min_floor)
            for c in range(12):
                for leave in (None, 0, 1, 5, 7):
                    chosen = [s != leave for s in range(8)]
                    got = bref.balance_of(moments[c, 0], moments[c, 1], moments[c, 2], reach[c], ok[c] & np.array(chosen))
                    want = rule_restatement(int(moments[c, 0]), int(moments[c, 1]), int(moments[c, 2]), feet[c], reach[c], chosen, min_floor)
                    assert got[0] == want[0] and isinstance(got[1], f64) and f64(want[1]).view(i64) == got[1].view(i64), (seed, c, leave, got, want)
                    assert got[0] == (got[1] >= 0), 'balanced: the margin is not negative'
                    if want[2] is not None:
                        assert abs(want[1] - want[2]) <= 4 * np.finfo(f64).eps * abs(want[2])
                    tipped, steady = tipped + (not got[0]), steady + got[0]
    assert tipped > 100 and steady > 100
    # one voxel on one floor voxel: half a voxel on every side, exactly
    one = np.full((8, 16), NONE, i32)
    one[0] = bref.DIRS @ (3, 4)
    for q in range(16):
        assert bref.balance_of(1, 3, 4, one, np.arange(8) == 0) == (True, 0.5)
    assert bref.balance_of(0, 0, 0, one, np.arange(8) == 0) == (False, -np.inf) and bref.balance_of(1, 3, 4, one, np.zeros(8, bool)) == (False, -np.inf)
    assert bref.balance_of(2, 7, 8, one, np.arange(8) == 0) == (True, 0.0), 'the centre on the edge of the foot: balanced, margin 0'
    assert bref.balance_of(2, 8, 8, one, np.arange(8) == 0) == (False, -0.5)


def graph_restatement(tables, rel, count, min_floor=1):
    """The per-part rules over plain Python sets."""
    moments, slots, feet, reach = (tables[k] for k in ('moments', 'slots', 'feet', 'reach'))
    P = len(feet)
    n = min(max(int(count), 0), P)
    rests = lambda c, a: c != a and rel[c][a] != 0
    rule = lambda c, chosen: rule_restatement(int(moments[c, 0]), int(moments[c, 1]), int(moments[c, 2]), feet[c], reach[c], chosen, min_floor)
    out = dict(balanced=[0] * P, margin=[-math.inf] * P, unsettles=[0] * P, falls=[0] * P, tips=[[0] * P for _ in range(P)])
    riders = {a: {c for c in range(n) if rests(c, a)} for a in range(n)}
    for c in range(n):
        ok, margin, _ = rule(c, [True] * 8)
        out['balanced'][c], out['margin'][c] = int(ok), margin
    for a in range(n):
        first = {c for c in riders[a] if not rule(c, [s != (int(slots[c][a]) & 7) for s in range(8)])[0]}
        gone, edge = set(first), set(first)
        while edge:
            edge = {x for c in edge for x in riders[c]} - gone
            gone |= edge
        for c in first:
            out['tips'][c][a] = 1
        out['unsettles'][a], out['falls'][a] = len(first), len(gone - {a})
    return dict(balanced=i32(out['balanced']).reshape(P), margin=f64(out['margin']).reshape(P), unsettles=i32(out['unsettles']).reshape(P),
                falls=i32(out['falls']).reshape(P), tips=u8(out['tips']).reshape(P, P))


@pytest.mark.parametrize('P', [1, 2, 5, 12])
def test_the_graph_equals_its_literal_restatement(P):
    tips = falls = 0
    for seed in range(4):
        moments, feet, reach = random_tables(P, 100 * P + seed)
        rel = random_relation(P, 50 * P + seed, dense=0.4, nine=1 if P >= 12 and seed % 2 else None)
        for count in (P, P - 1, 0, P + 3):
            slots = bref.slots(rel, count)[0]
            tables = dict(moments=moments, slots=slots, feet=feet, reach=reach)
            for min_floor in (1, 4):
                got = bref.balance(moments, feet, reach, slots, rel, count, min_floor)
                want = graph_restatement(tables, rel.tolist(), count, min_floor)
                for k in COLUMNS:
                    same((P, seed, count, min_floor, k), got[k], want[k])
                n = max(0, min(count, P))
                assert not got['tips'][n:].any() and not got['tips'][:, n:].any() and (got['margin'][n:] == -np.inf).all() and not got['balanced'][n:].any()
                assert (got['falls'] >= got['unsettles']).all()
                tips, falls = tips + int(got['tips'].sum()), falls + int((got['falls'] - got['unsettles']).sum())
    assert P < 5 or (tips > 20 and falls > 0)


def pile_balance(name, P=8, connectivity=26, **params):
    """The support's statement and the balance's on one of test_part_support.py's piles."""
    _, lab, _, _, n, z_min = tps.piles()[name]
    s = sref.support_of_labels(lab, n, P, connectivity, z_min, **params)
    return s, bref.balance_of_labels(lab, s['rests_on'], n, connectivity, z_min, params.get('min_floor', 1)), n


def boxes(R, *corners):
    """labels [R,R,R]: box L + 1 = corners[L] = (lo, hi), inclusive as tgr.box."""
    lab = np.zeros((R, R, R), i32)
    for L, (lo, hi) in enumerate(corners, 1):
        lab[tgr.box(R, lo, hi)] = L
    return lab


BRIDGE = (((8, 16, 2), (12, 24, 10)), ((28, 16, 2), (32, 24, 10)), ((6, 16, 11), (34, 24, 13)), ((16, 18, 14), (22, 22, 18)))


def labels_balance(lab, n, P=8, connectivity=26, z_min=0):
    s = sref.support_of_labels(lab, n, P, connectivity, z_min)
    return s, bref.balance_of_labels(lab, s['rests_on'], n, connectivity, z_min)


def test_the_synthetic_shapes():
    """What the statement says of the piles at 40^3, of a bridge and of an overhang: the exact doubles."""
    col = lambda b, k, n: b[k][:n].tolist()
    hexes = lambda b, n: [float(x).hex() for x in b['margin'][:n]]
    s, b, n = pile_balance('sphere_on_box')
    assert col(b, 'balanced', n) == [1, 1] and col(b, 'margin', n) == [8.5, 4.5] and b['feet'][0, 0] == 289 and b['feet'][1, 1] == 69
    assert col(b, 'unsettles', n) == col(b, 'falls', n) == col(s, 'orphans', n) == [1, 0] and b['feet'].sum() == 289 + 69
    assert (b['margin'][n:] == -np.inf).all() and not b['balanced'][n:].any() and b['tips'][1, 0] == 1 and b['tips'].sum() == 1
    s, b, n = pile_balance('leaning')
    assert col(b, 'balanced', n) == [1, 0] and col(b, 'margin', n) == [0.5, -2.5] and b['feet'][1].tolist() == [0, 20, 0, 0, 0, 0, 0, 0]
    assert col(b, 'unsettles', n) == col(b, 'falls', n) == [1, 0]
    s, b, n = pile_balance('side_by_side')
    assert col(b, 'balanced', n) == [1, 1] and hexes(b, n) == ['0x1.0000000000000p-1', '0x1.faf1eb0ecdcfap-2'] and abs(b['margin'][1] - 0.495) < 1e-3
    assert not b['unsettles'].any() and not b['falls'].any() and b['feet'][:2].tolist() == [[1] + [0] * 7] * 2
    s, b, n = pile_balance('pile')
    assert n == 4 and col(b, 'balanced', n) == [1, 1, 1, 1]
    assert hexes(b, n) == ['0x1.e9b536a6d4daap-2', '0x1.e6be269b83284p-2', '0x1.1fee44b5bfb91p+2', '0x1.ea3e5e4712216p-2']
    assert [round(x, 2) for x in col(b, 'margin', n)] == [0.48, 0.48, 4.5, 0.48] and b['feet'][2].tolist() == [0, 31, 30, 31, 0, 0, 0, 0]
    assert b['feet'][[0, 1, 3]].tolist() == [[1] + [0] * 7] * 3, 'each low ball on one floor voxel'
    assert not b['unsettles'].any() and not b['falls'].any() and not b['crowded'].any(), 'the contact patches are fat enough to hold the top ball on two'
    # the bridge: two pillars, a plank across them, a small box on the plank
    lab = boxes(40, *BRIDGE)
    for connectivity, plank in ((6, 45), (18, 63), (26, 63)):
        s, b = labels_balance(lab, 4, 8, connectivity, 2)
        assert col(b, 'margin', 4) == [2.5, 2.5, 4.5, 2.5] and col(b, 'balanced', 4) == [1, 1, 1, 1]
        assert col(b, 'unsettles', 4) == [1, 1, 1, 0] and col(b, 'falls', 4) == [2, 2, 1, 0] and col(s, 'orphans', 4) == [0, 0, 1, 0]
        assert b['feet'][2].tolist() == [0, plank, plank, 0, 0, 0, 0, 0] and b['slots'][2, :2].tolist() == [1, 2]
    # the overhang: under connectivity 26 the upper box keeps a foot one diagonal beyond its footing
    for lo, margin in ((8, 3.5), (10, 1.5), (11, 0.5), (12, -0.5)):
        s, b = labels_balance(boxes(40, ((5, 15, 0), (15, 25, 9)), ((lo, 15, 10), (lo + 10, 25, 14))), 2)
        assert col(b, 'margin', 2) == [5.5, margin] and col(b, 'balanced', 2) == [1, int(lo < 12)], lo
    s, b = labels_balance(boxes(40, ((5, 15, 0), (15, 25, 9)), ((12, 15, 10), (22, 25, 14))), 2, connectivity=6)
    assert col(b, 'margin', 2) == [5.5, -1.5], 'connectivity 6: the strict footprint'


def host_rows(b, n):
    """balance.balance_rows' fields from the statement's arrays of one scene."""
    rows = {k: b[k][:n] for k in (*bref.COLUMNS, 'moments', 'feet', 'reach', 'crowded')}
    rows.update(slots=b['slots'][:n, :n], tips=b['tips'][:n, :n])
    return rows


def test_host_functions():
    scale, origin = 0.0075, (0.1, -0.2, 0.05)
    # a 4 x 8 x 16 box reads its edge lengths along the lattice's axes
    lab = boxes(24, ((3, 5, 0), (6, 12, 15)))
    s, b = labels_balance(lab, 1, 2)
    h = balance.balance_from_rows(host_rows(b, 1), scale, origin)
    assert list(h) == ['balanced', 'margin', 'unsettles', 'falls', 'moments', 'feet', 'reach', 'crowded', 'slots', 'tips', 'margin_m', 'centre',
                       'covariance', 'axes', 'extent']
    assert np.allclose(h['extent'][0], np.array([16.0, 8.0, 4.0]) * scale, rtol=1e-9, atol=0) and h['extent'].shape == (1, 3)
    same('axes', np.abs(h['axes'][0]).round(12), np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], f64))
    assert (h['axes'][0].sum(1) > 0).all() and h['margin_m'][0] == h['margin'][0] * scale == 2.0 * scale and h['balanced'].dtype == bool
    assert np.allclose(h['covariance'][0], np.diag([16.0, 64.0, 256.0]) / 12 * scale ** 2, rtol=1e-12, atol=1e-18)
    # a diagonal bar: its long axis is the diagonal, sign fixed
    bar = np.zeros((24, 24, 24), i32)
    for t in range(20):
        bar[t + 1, t + 2, 5] = 1
    h = balance.balance_from_rows(host_rows(labels_balance(bar, 1, 2, z_min=5)[1], 1), 1.0)
    assert np.allclose(h['axes'][0, 0], [math.sqrt(0.5), math.sqrt(0.5), 0.0]) and h['extent'][0, 0] > 20 and np.allclose(h['extent'][0, 1:], 1.0)
    # the centre is the parts' own
    vol, lab, _, _, n, z_min = tps.piles()['pile']
    w = pref.parts(pref.d2_free(vol[None]), max_parts=8)
    p = parts.parts_from_rows({k: (v[0, :n] if np.ndim(v) > 1 else v[:1]) for k, v in w.items() if k != 'labels'}, scale, origin)
    s, b, n = pile_balance('pile')
    h = balance.balance_from_rows(host_rows(b, n), scale, origin)
    same('centre', h['centre'], p['centroid'])
    assert h['tips'].dtype == bool and h['slots'].dtype == u8 and h['crowded'].dtype == bool and h['moments'].dtype == i64 and h['covariance'].shape == (4, 3, 3)
    assert np.allclose(h['extent'][2], math.sqrt(12 / 5) * 6 * scale, rtol=0.03), 'a ball of radius 6 has the variance r^2 / 5 along every axis'
    none = balance.balance_from_rows(host_rows(b, 0), scale)
    assert none['axes'].shape == (0, 3, 3) and none['centre'].shape == (0, 3)
    # the grasps' columns: numpy, and torch (a gather) with a batch axis
    s, b, n = pile_balance('leaning')
    h = balance.balance_from_rows(host_rows(b, n), scale)
    part = i32([2, 1, 0, 3, 9, -2, 1])
    cols = balance.grasp_balance_columns(part, h)
    assert list(cols) == ['part_margin', 'part_balanced', 'part_unsettles', 'part_falls']
    same('margin', cols['part_margin'], f64([-2.5, 0.5, -np.inf, -np.inf, -np.inf, -np.inf, 0.5]))
    same('balanced', cols['part_balanced'], np.array([False, True, False, False, False, False, True]))
    same('unsettles', cols['part_unsettles'], i32([0, 1, 0, 0, 0, 0, 1]))
    same('falls', cols['part_falls'], i32([0, 1, 0, 0, 0, 0, 1]))
    dev = {k: torch.from_numpy(np.stack([b[k], b[k][::-1].copy()])) for k in bref.COLUMNS}
    tcols = balance.grasp_balance_columns(torch.from_numpy(np.stack([part, part])), dev)
    for k, v in cols.items():
        same(('torch', k), tcols[k][0].numpy(), v)
    assert tcols['part_margin'][1].tolist() == [-np.inf] * 7 and tcols['part_falls'].dtype == torch.int32 and tcols['part_margin'].dtype == torch.float64
    none = balance.grasp_balance_columns(np.zeros(0, i32), h)
    assert all(len(v) == 0 for v in none.values()) and none['part_balanced'].dtype == bool and none['part_margin'].dtype == f64
    # the best grasp of every part that comes out, carries nothing and lets nothing fall
    columns = dict(part=i32([1, 3, 3, 0, 2, 1]), retreat_free=np.array([True, False, True, True, True, True]), part_carried=i32([0, 0, 0, 0, 0, 0]),
                   part_falls=i32([1, 0, 0, 0, 2, 0]))
    assert support.best_clear_per_part(columns) == {1: 0, 3: 2, 2: 4} and balance.best_steady_per_part(columns) == {3: 2, 1: 5}
    assert balance.best_steady_per_part(dict(columns, part_carried=i32([1] * 6))) == {}


def test_balance_params():
    want = dict(min_floor=1)
    assert balance.balance_params(False) is None and balance.balance_params(None) is None
    assert balance.balance_params(True) == want == balance.balance_params({}) == balance.BALANCE_DEFAULTS == balance.checked_balance()
    assert balance.balance_params(dict(min_floor=3, filter=True), filter=False) == dict(min_floor=3, filter=True)
    with pytest.raises(TypeError, match='unknown balance parameters'):
        balance.balance_params(dict(lean=0.5))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='balance min_floor must be an integer >= 1, got'):
            balance.balance_params(dict(min_floor=bad))
    assert balance.checked_feet(8) == dict(max_parts=8, connectivity=26, z_min=0) and balance.checked_feet(256, 6, 40, 40)['z_min'] == 40
    for bad in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match='balance max_parts must be an integer in 1..256'):
            balance.checked_feet(bad)
    for bad in (0, 7, True, 27):
        with pytest.raises(ValueError, match='balance connectivity must be 6, 18 or 26'):
            balance.checked_feet(8, bad)
    for bad in (-1, 0.5, True):
        with pytest.raises(ValueError, match='balance z_min must be an integer >= 0'):
            balance.checked_feet(8, 26, bad)
    with pytest.raises(ValueError, match='balance z_min must be in 0..R = 40, got 41'):
        balance.checked_feet(8, 26, 41, 40)
    for cls, keys in ((balance.PartFeet, ('connectivity', 'z_min')), (balance.PartBalance, ('min_floor', 'tips'))):
        params = inspect.signature(cls.__call__).parameters
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keys)
    assert balance.MAX_PARTS == _lib.GNR_BALANCE_MAX_PARTS == support.MAX_PARTS == 256
    g = dict(index=np.zeros((0, 3)), quat=np.zeros((0, 4)), width=np.zeros(0))
    with pytest.raises(TypeError, match='unknown balance parameters'):
        balance.balance_of_plan(np.ones((4, 4, 4), f32), g, iso=0.0)
    with pytest.raises(ValueError, match='support min_floor must be an integer >= 1'):
        balance.balance_of_plan(np.ones((4, 4, 4), f32), g, min_floor=0)
    with pytest.raises(ValueError, match='balance z_min must be an integer >= 0'):
        balance.balance_of_plan(np.ones((4, 4, 4), f32), g, z_min=-1)


def test_part_balance_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for cls in (balance.PartFeet, balance.PartBalance):
        with pytest.raises(_lib.GnrError, match='no CPU fallback'):
            cls()


# ---- 2. the refusals of the two entry points ------------------------------------------------------------------------------------------
FEET_PTRS = ('labels', 'rests_on', 'count', 'moments', 'slots', 'feet', 'reach', 'crowded')
BALANCE_PTRS = ('moments', 'feet', 'reach', 'slots', 'rests_on', 'count', 'balanced', 'margin', 'unsettles', 'falls')
ROWS_TEXT = ': max_parts must be in 1..GNR_BALANCE_MAX_PARTS (256)'


def _feet_refusals(ptr, B=1, R=8, P=4):
    """Every refusal of gnr_part_feet_fwd, each with its code and its text, and their order, on the pointers given (fake ones, or
    buffers whose bytes the caller checks afterwards)."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_part_feet_fwd'

    def call(p=None, B=B, R=R, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in FEET_PTRS}
        p = _lib.GnrFeetParams(**{**dict(connectivity=26, max_parts=P, z_min=0), **kw}) if p is None else p
        return L.gnr_part_feet_fwd(C.byref(p) if p is not False else None, a['labels'], a['rests_on'], a['count'], B, R, *(a[k] for k in FEET_PTRS[3:]), None)

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
    for name in FEET_PTRS:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    # the order: of two faults the one the header names first is reported
    faults = (dict(B=0), dict(R=1), dict(max_parts=257), dict(connectivity=5), dict(z_min=-1), dict(labels=None))
    texts = (': B must be in 1..65535', ': R must be in 2..256', ROWS_TEXT, ': connectivity must be 6, 18 or 26', ': z_min must be in 0..R', ': null pointer')
    for i in range(len(faults)):
        for j in range(i + 1, len(faults)):
            assert call(**faults[i], **faults[j]) != _lib.GNR_OK and text() == fn + texts[i], (i, j)


def _balance_refusals(ptr, B=1, P=4):
    """Every refusal of gnr_part_balance_fwd; tips may be null."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_part_balance_fwd'

    def call(p=None, B=B, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in BALANCE_PTRS}
        tips = kw.pop('tips', ptr.get('tips'))
        p = _lib.GnrBalanceParams(**{**dict(max_parts=P, min_floor=1), **kw}) if p is None else p
        return L.gnr_part_balance_fwd(C.byref(p) if p is not False else None, *(a[k] for k in BALANCE_PTRS[:6]), B, *(a[k] for k in BALANCE_PTRS[6:]), tips, None)

    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for m in (0, -1, 257):
        assert call(max_parts=m) == _lib.GNR_ERR_SHAPE and text() == fn + ROWS_TEXT, m
    for m in (0, -3):
        assert call(min_floor=m) == _lib.GNR_ERR_ARG and text() == fn + ': min_floor must be >= 1', m
    for name in BALANCE_PTRS:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    faults = (dict(B=0), dict(max_parts=0), dict(min_floor=0), dict(count=None))
    texts = (': B must be in 1..65535', ROWS_TEXT, ': min_floor must be >= 1', ': null pointer')
    for i in range(len(faults)):
        for j in range(i + 1, len(faults)):
            assert call(**faults[i], **faults[j]) != _lib.GNR_OK and text() == fn + texts[i], (i, j)


def test_refusals_before_the_device():
    one = C.c_void_p(16)
    _feet_refusals({k: one for k in FEET_PTRS})
    _balance_refusals({k: one for k in (*BALANCE_PTRS, 'tips')})
    _balance_refusals({k: one for k in BALANCE_PTRS})


def test_a_refused_call_writes_nothing_without_a_device():
    """The same refusals on host buffers of 0x5a bytes: a refused call has launched nothing and the host side writes nothing."""
    bufs = {k: np.full(4096, SENTINEL, u8) for k in (*FEET_PTRS, *BALANCE_PTRS, 'tips')}
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    _feet_refusals(ptr)
    _balance_refusals(ptr)
    for k, v in bufs.items():
        assert (v == SENTINEL).all(), k


# ---- GPU: the bits of the statement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ops():
    return balance.PartFeet(), balance.PartBalance()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to('cuda:0')


def check_feet(what, labels, rests_on, counts, connectivity=26, z_min=0):
    """PartFeet on B scenes, its output tensors filled with 0x5a bytes before the call, against the statement: every element is
    written.  -> the device's result and the statement's (slots, crowded, moments, feet, reach) dicts, per scene."""
    op = _ops()[0]
    labels = _dev(labels, i32)
    rel, count = _dev(rests_on, u8), torch.tensor(list(counts), dtype=torch.int32, device='cuda:0')
    kw = dict(connectivity=connectivity, z_min=z_min)
    for k in TABLES:
        op(labels, rel, count, **kw)[k].view(torch.uint8).fill_(SENTINEL)      # (the tensors of this shape)
    res = op(labels, rel, count, **kw)
    torch.cuda.synchronize()
    want = []
    for b in range(len(counts)):
        slots, crowded = bref.slots(rests_on[b], counts[b])
        want.append(dict(zip(TABLES, (None, slots, None, None, crowded)), **dict(zip(('moments', 'feet', 'reach'), bref.feet(labels[b].cpu().numpy(), slots, connectivity, z_min)))))
    for k in TABLES:
        same((what, k), res[k].cpu().numpy(), np.stack([w[k] for w in want]))
    return res, want


def check_balance(what, tables, rests_on, counts, min_floor=1):
    """PartBalance on B hand-written or statement-made tables (dict of [B,..] arrays), sentinels first, against the statement, tips
    included and the rows beyond the parts."""
    op = _ops()[1]
    feet = {k: _dev(tables[k], t) for k, t in (('moments', i64), ('feet', i32), ('reach', i32), ('slots', u8))}
    feet.update(rests_on=_dev(rests_on, u8), count=torch.tensor(list(counts), dtype=torch.int32, device='cuda:0'))
    for k in COLUMNS:
        op(feet, min_floor=min_floor, tips=True)[k].view(torch.uint8).fill_(SENTINEL)
    res = op(feet, min_floor=min_floor, tips=True)
    torch.cuda.synchronize()
    want = [bref.balance(tables['moments'][b], tables['feet'][b], tables['reach'][b], tables['slots'][b], rests_on[b], counts[b], min_floor) for b in range(len(counts))]
    for k in COLUMNS:
        same((what, k), res[k].cpu().numpy(), np.stack([w[k] for w in want]))
    return want


def check_both(what, labels, rests_on, counts, connectivity=26, z_min=0, min_floor=1):
    """The feet, then the balance of the statement's tables (which the device's equal)."""
    _, want = check_feet(what, labels, rests_on, counts, connectivity, z_min)
    tables = {k: np.stack([w[k] for w in want]) for k in ('moments', 'slots', 'feet', 'reach')}
    return want, check_balance(what, tables, rests_on, counts, min_floor)


@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 3, 5, 8, 17])
def test_random_labels(R):
    """Three scenes per call with other labels, relations and counts in each, so any wrap into a neighbouring row, plane or scene
    shows; labels from -1 to beyond the rows; relations of random bytes, one row with nine footings."""
    P = 12
    labels = np.stack([tps.random_labels(R, 100 * R, -1, P + 2), tps.random_labels(R, 100 * R + 1, 3, P + 1), tps.random_labels(R, 100 * R + 2, -1, 4)])
    rel = np.stack([random_relation(P, 7 * R, 0.3, nine=2), random_relation(P, 7 * R + 1, 0.6), random_relation(P, 7 * R + 2, 0.2, nine=0)])
    feet = tips = 0
    for connectivity in (6, 18, 26):
        for z_min, counts in ((0, (P, 0, P + 5)), (1, (P - 3, -2, P)), (R, (P, P, 3))):
            want, bal = check_both((R, connectivity, z_min), labels, rel, counts, connectivity, z_min, min_floor=1 + (z_min == 1))
            feet, tips = feet + sum(int(w['feet'][:, 1:].sum()) for w in want), tips + sum(int(w['tips'].sum()) for w in bal)
    assert feet > 0 and (R < 3 or tips > 0)


@pytest.mark.gpu
def test_many_keys_in_a_wavefront():
    """R = 8, the labels 1..256 cycling through the scene at 256 rows: 64 distinct labels in every wavefront; a relation with a
    crowded row, and a second scene of random labels."""
    R, P = 8, 256
    cyc = (np.arange(R ** 3, dtype=i32) % P + 1).reshape(R, R, R)
    labels = np.stack([cyc, tps.random_labels(R, 3, 1, P)])
    rel = np.stack([random_relation(P, 11, 0.02, nine=40), random_relation(P, 12, 0.05, nine=255)])
    for connectivity in (6, 26):
        want, bal = check_both(('keys', connectivity), labels, rel, (P, P - 1), connectivity, 3)
        assert want[0]['crowded'][40] == 1 and want[0]['crowded'].sum() >= 1 and want[0]['feet'][:, 0].sum() == R * R and (want[0]['moments'][:, 0] == 2).all()
    assert want[0]['feet'][:, 1:].sum() > 50


@pytest.mark.gpu
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_two_solid_halves(axis):
    """R = 16 split into two solid labels by a plane: one key takes every lane.  Split along k with the top resting on the bottom,
    every voxel of a plane is a foot."""
    R = 16
    lab = np.ones((R, R, R), i32)
    np.moveaxis(lab, axis, 0)[R // 2:] = 2
    rel = np.zeros((3, 2, 2), u8)
    rel[:, 1, 0] = (1, 200, 0)                                                 # 2 rests on 1, in two of the scenes
    for connectivity in (6, 18, 26):
        want, bal = check_both(('halves', axis, connectivity), np.stack([lab, lab[::-1].copy(), lab]), rel, (2, 2, 2), connectivity, 0)
        w = want[0]
        assert w['moments'][:, 0].tolist() == [R ** 3 // 2] * 2 and w['feet'][0].tolist() == [R * R // (1 if axis == 2 else 2)] + [0] * 7
        if axis == 2:
            assert w['feet'][1].tolist() == [0, R * R] + [0] * 6, 'every voxel of the plane k = 8 is a foot'
            assert w['reach'][1, 1].tolist() == [15, 45, 30, 45, 15, 30, 15, 15, 0, 0, 0, 0, 0, 15, 15, 30]
            assert bal[0]['margin'].tolist() == [8.0, 8.0] and bal[0]['falls'].tolist() == [1, 0]
        else:
            assert (w['feet'][1, 1] > 0) == (connectivity != 6), 'side by side: a diagonal neighbour lies lower'
        assert not want[2]['feet'][:, 1:].any(), 'no relation, no feet but the floor\'s'


@pytest.mark.gpu
def test_a_solid_lattice_of_128():
    """One scene at R = 128 filled with label 1: the smallest solid whose sum of i^2 (1.13e10) wraps 32 bits.  Against the closed
    forms, not a numpy pass."""
    R = 128
    op = _ops()[0]
    labels = torch.ones(1, R, R, R, dtype=torch.int32, device='cuda:0')
    rel, count = torch.zeros(1, 1, 1, dtype=torch.uint8, device='cuda:0'), torch.ones(1, dtype=torch.int32, device='cuda:0')
    for k in TABLES:
        op(labels, rel, count, z_min=0)[k].view(torch.uint8).fill_(SENTINEL)
    res = op(labels, rel, count, z_min=0)
    torch.cuda.synchronize()
    s1, s2 = R * (R - 1) // 2, (R - 1) * R * (2 * R - 1) // 6
    assert s2 * R * R > 2 ** 32
    same('moments', res['moments'].cpu().numpy(), i64([R ** 3, s1 * R * R, s1 * R * R, s1 * R * R, s2 * R * R, s2 * R * R, s2 * R * R, s1 * s1 * R, s1 * s1 * R, s1 * s1 * R]).reshape(1, 1, 10))
    feet, reach = np.zeros((1, 1, 8), i32), np.full((1, 1, 8, 16), NONE, i32)
    feet[0, 0, 0], reach[0, 0, 0] = R * R, np.maximum(bref.DIRS, 0).sum(1) * (R - 1)
    same('feet', res['feet'].cpu().numpy(), feet)
    same('reach', res['reach'].cpu().numpy(), reach)
    bal = _ops()[1](res)
    torch.cuda.synchronize()
    assert bal['margin'].tolist() == [[64.0]] and bal['balanced'].tolist() == [[1]]


def chain(order, R=40):
    """P = len(order) parts in one chain written straight into the tables: order[i + 1] rests on order[i] and stands on it squarely;
    order[0] stands on the floor."""
    P = len(order)
    moments, feet, reach, rel = np.zeros((P, 10), i64), np.zeros((P, 8), i32), np.full((P, 8, 16), NONE, i32), np.zeros((P, P), u8)
    moments[:, :3] = (4, 4 * 10, 4 * 10)
    for lo, hi in zip(order[:-1], order[1:]):
        rel[hi, lo] = 1
        feet[hi, 1], reach[hi, 1] = 1, bref.DIRS @ (10, 10)
    feet[order[0], 0], reach[order[0], 0] = 1, bref.DIRS @ (10, 10)
    return dict(moments=moments, feet=feet, reach=reach), rel


def stacked(tables, rels, counts):
    slots = [bref.slots(r, c)[0] for r, c in zip(rels, counts)]
    return dict({k: np.stack([t[k] for t in tables]) for k in ('moments', 'feet', 'reach')}, slots=np.stack(slots)), np.stack(rels)


@pytest.mark.gpu
def test_the_balance_alone():
    """gnr_part_balance_fwd on tables no label volume gave."""
    # random tables and relations at several row counts, counts beyond the rows and below zero
    for P in (1, 5, 64, 256):
        tabs = [random_tables(P, 10 * P + b) for b in range(3)]
        rels = [random_relation(P, 20 * P + b, min(0.4, 5.0 / P), nine=(b if P >= 64 else None)) for b in range(3)]
        for counts in ((P, P + 7, P - 1), (0, -3, (P + 1) // 2)):
            tables, rel = stacked([dict(zip(('moments', 'feet', 'reach'), t)) for t in tabs], rels, counts)
            for min_floor in (1, 3):
                check_balance((P, counts, min_floor), tables, rel, counts, min_floor)
    # a chain through all 256 parts -- ascending, descending, shuffled: taking any part but the top one drops everything above it
    P = 256
    orders = [list(range(P)), list(range(P - 1, -1, -1)), np.random.default_rng(7).permutation(P).tolist()]
    made = [chain(o) for o in orders]
    tables, rel = stacked([m[0] for m in made], [m[1] for m in made], (P,) * 3)
    for o, w in zip(orders, check_balance('chain', tables, rel, (P,) * 3)):
        assert w['falls'][o].tolist() == list(range(P - 1, -1, -1)) and w['unsettles'][o].tolist() == [1] * (P - 1) + [0] and w['balanced'].all()
    # a cycle in the relation: 0 on 1 on 2 on 0, each on one slot only, and 3 on 0: everything falls, whichever is taken; never itself
    t, _ = chain([0, 1, 2, 3])
    t['feet'][0], t['reach'][0] = t['feet'][1], t['reach'][1]
    cyc = np.zeros((4, 4), u8)
    cyc[0, 1] = cyc[1, 2] = cyc[2, 0] = cyc[3, 0] = 9
    tables, rel = stacked([t], [cyc], (4,))
    w = check_balance('cycle', tables, rel, (4,))[0]
    assert w['falls'].tolist() == [3, 3, 3, 0] and w['unsettles'].tolist() == [2, 1, 1, 0]
    # nine footings: part 0 rests on 1..9, its centre over the feet of slot 3 and of the shared slot 7 only; a part without feet; a
    # part without mass
    P = 12
    moments, feet, reach, rel = np.zeros((P, 10), i64), np.zeros((P, 8), i32), np.full((P, 8, 16), NONE, i32), np.zeros((P, P), u8)
    moments[:, :3] = (2, 2 * 20, 2 * 20)
    rel[0, 1:10] = 1
    feet[1:, 0], reach[1:, 0] = 1, bref.DIRS @ (20, 20)
    feet[0, 1:], reach[0, 1:] = 1, bref.DIRS @ (3, 3)                          # seven slots off to one side ..
    reach[0, 3] = reach[0, 7] = bref.DIRS @ (20, 20)                           # .. but slot 3 (footing 3) and slot 7 (footings 7, 8, 9)
    feet[10] = 0                                                               # 11: no feet
    moments[11, 0] = 0                                                         # 12: no mass
    tables, rels = stacked([dict(moments=moments, feet=feet, reach=reach)], [rel], (P,))
    w = check_balance('nine', tables, rels, (P,))[0]
    assert tables['slots'][0, 0, :10].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7, 7] and w['balanced'].tolist() == [1] * 10 + [0, 0]
    assert w['margin'][10] == w['margin'][11] == -np.inf and not w['tips'].any(), 'either of the two good slots holds it'
    tables['reach'][0, 0, 7] = bref.DIRS @ (3, 3)                              # now slot 3 alone holds it
    w = check_balance('nine', tables, rels, (P,))[0]
    assert w['tips'][0].tolist() == [0, 0, 0, 1] + [0] * 8 and w['falls'].tolist() == [0, 0, 0, 1] + [0] * 8
    tables['reach'][0, 0, 7], tables['reach'][0, 0, 3] = bref.DIRS @ (20, 20), bref.DIRS @ (3, 3)     # now the shared slot alone
    w = check_balance('nine', tables, rels, (P,))[0]
    assert w['tips'][0].tolist() == [0] * 7 + [1, 1, 1, 0, 0] and w['unsettles'].tolist() == [0] * 7 + [1, 1, 1, 0, 0], 'the whole slot goes'
    # the extremes of R = 256: m = 2^24, coordinates 255 -- m * H is 2^24 * 1533, past 32 bits, the levers 2^33
    moments, feet, reach = np.zeros((2, 10), i64), np.zeros((2, 8), i32), np.full((2, 8, 16), NONE, i32)
    moments[:, 0] = 2 ** 24
    moments[0, 1:3], moments[1, 1:3] = (2 ** 24 * 255, 2 ** 24 * 255), (2 ** 24 * 255 - 1, 1)
    feet[:, 0], reach[:, 0] = 1, bref.DIRS @ (255, 255)
    feet[1, 2], reach[1, 2] = 3, bref.DIRS @ (0, 0)
    tables, rels = stacked([dict(moments=moments, feet=feet, reach=reach)], [np.zeros((2, 2), u8)], (2,))
    w = check_balance('extremes', tables, rels, (2,))[0]
    assert w['margin'][0] == 0.5 and w['balanced'].tolist() == [1, 0] and w['margin'][1] < -100


@pytest.mark.gpu
def test_falls_is_never_less_than_orphans():
    """On relations that came from PartSupport: the piles, the bridge, random blobs."""
    R = 40
    blobs = lambda seed: functools.reduce(np.logical_or, [tgr.ball(R, np.random.default_rng(seed + i).uniform(6, R - 7, 3), np.random.default_rng(seed + i).uniform(3.0, 7.0)) for i in range(7)])
    vols = [np.asarray(tps.piles()[k][0]) for k in ('sphere_on_box', 'pile', 'leaning')] + [tgr.mask_volume(blobs(s)) for s in (1, 20)]
    vol = torch.from_numpy(np.stack(vols)).to('cuda:0')
    field = distance.VolumeDistance()(vol, scale=VOXEL, z_min=2)
    res = parts.VolumeParts()(field['d2_free'], connectivity=26, max_parts=16, neck=0.8)
    sres = support.PartSupport().of_parts(res, connectivity=26, z_min=2, relation=True)
    bres = _ops()[1].of_support(res, sres, connectivity=26, z_min=2, tips=True)
    torch.cuda.synchronize()
    falls, orphans, edges = bres['falls'].cpu().numpy(), sres['orphans'].cpu().numpy(), int(sres['rests_on'].sum().item())
    assert (falls >= orphans).all() and edges > 5 and falls.sum() > 0, (falls, orphans)
    for b in range(len(vols)):
        w = bref.balance_of_labels(res['labels'][b].cpu().numpy(), sres['rests_on'][b].cpu().numpy(), int(res['count'][b].item()), 26, 2)
        for k in (*COLUMNS, *TABLES):
            same(('blobs', b, k), bres[k][b].cpu().numpy(), w[k])
    with pytest.raises(ValueError, match='build the PartSupport result with relation=True'):
        _ops()[1].of_support(res, {k: v for k, v in sres.items() if k != 'rests_on'})
    # the bridge: orphans sees nothing when a pillar is taken
    lab = torch.from_numpy(boxes(40, *BRIDGE)[None]).to('cuda:0')
    pres = dict(labels=lab, count=torch.tensor([4], dtype=torch.int32, device='cuda:0'), max_parts=8)
    sres = support.PartSupport().of_parts(pres, connectivity=26, z_min=2, relation=True)
    bres = _ops()[1].of_support(pres, sres, connectivity=26, z_min=2)
    assert bres['falls'][0, :4].tolist() == [2, 2, 1, 0] and sres['orphans'][0, :4].tolist() == [0, 0, 1, 0] and bres['margin'][0, :4].tolist() == [2.5, 2.5, 4.5, 2.5]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['sphere_on_box', 'pile', 'side_by_side', 'leaning'])
def test_balance_of_plan(name):
    vol, lab, bbox, voxels, n, z_min = tps.piles()[name]
    g = tps.plan_of(name)
    got, cols = balance.balance_of_plan(np.array(vol), g, voxel_size=VOXEL, max_parts=8, z_min=z_min)
    assert got['count'] == n and np.array_equal(got['labels'], lab)
    s, b, _ = pile_balance(name)
    want = balance.balance_from_rows(host_rows(b, n), VOXEL)
    want['axis_extent'] = want.pop('extent')
    for k, w in want.items():
        same((name, k), got[k], w)
    same((name, 'centre'), got['centre'], got['centroid'])
    for k, w in tps.host_support(s, n).items():
        same((name, k), got[k], w)
    assert got['extent'].shape == (n, 3) and np.array_equal(got['extent'], (got['bbox_hi'] - got['bbox_lo'] + 1) * f64(VOXEL)), 'the parts\' own extent stays'
    held = cols['part']
    for k, w in balance.grasp_balance_columns(held, want).items():
        same((name, k), cols[k], w)
    steady, clear = balance.best_steady_per_part(cols), support.best_clear_per_part(cols)
    print(name, held, cols['part_falls'], cols['part_margin'], steady, clear)
    assert set(steady) <= set(clear) and (cols['part_falls'] >= cols['part_orphans']).all()
    if name == 'leaning':
        assert not got['balanced'][1] and got['margin'][1] == -2.5 and 1 not in steady and (cols['part_falls'][held == 1] == 1).all()
    if name == 'pile':
        assert set(steady) == {3} and got['balanced'].all()


@pytest.mark.gpu
def test_one_captured_graph_from_the_volume_to_the_balance_columns():
    """VolumeDistance, VolumeParts, GraspObjects, PartContacts, PartSupport, PartFeet, PartBalance and the gather of the grasps' columns
    captured once on one stream, replayed on a second volume and twice on a third: the bits of the statement at every replay."""
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
        sres = d.of_parts(res, connectivity=26, z_min=1, relation=True)
        bres = e.of_support(res, sres, connectivity=26, z_min=1, tips=True)
        return res, gres, sres, bres, balance.grasp_balance_columns(gres['object'], bres)

    ops = distance.VolumeDistance(), parts.VolumeParts(), objects.GraspObjects(), support.PartSupport(), balance.PartBalance()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*ops)                                                              # sizes the workspaces and the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, gres, sres, bres, gcols = run(*ops)
    feet, first = 0, None
    for s in (volumes[1], volumes[2], volumes[2]):
        vol.copy_(torch.from_numpy(s).to(dev))
        for t in (*(bres[k] for k in (*COLUMNS, *TABLES)), *gcols.values()):
            t.view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = pref.parts(pref.d2_free(s, z_min=1), **kw)
        assert np.array_equal(res['labels'].cpu().numpy(), want['labels'])
        bits = {}
        for b in range(2):
            sw = sref.support_of_labels(want['labels'][b], want['count'][b], M, 26, 1)
            w = bref.balance_of_labels(want['labels'][b], sw['rests_on'], want['count'][b], 26, 1)
            for k in (*COLUMNS, *TABLES):
                same(('replay', b, k), bres[k][b].cpu().numpy(), w[k])
            cols = balance.grasp_balance_columns(gres['object'][b].cpu().numpy(), {k: w[k] for k in bref.COLUMNS})
            for k, v in cols.items():
                same(('replay', b, k), gcols[k][b].cpu().numpy(), v)
                bits[b, k] = gcols[k][b].cpu().numpy()
            feet += int(w['feet'][:, 1:].sum())
            assert (w['falls'] >= sw['orphans']).all()
        if s is volumes[2]:
            if first is None:
                first = bits
            else:
                assert all(np.array_equal(first[k], bits[k]) for k in bits), 'the same graph on the same input: the same bits'
    print(feet)
    assert feet > 10, 'hardly a part stands on another'


@pytest.mark.gpu
def test_a_refused_call_writes_nothing():
    B, R, P = 1, 8, 4
    fill = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    sizes = dict(labels=4 * R ** 3, rests_on=P * P, count=4, moments=80 * P, slots=P * P, feet=32 * P, reach=512 * P, crowded=4 * P, balanced=4 * P,
                 margin=8 * P, unsettles=4 * P, falls=4 * P, tips=P * P)
    bufs = {k: fill(v) for k, v in sizes.items()}
    ptr = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    _feet_refusals(ptr, B=B, R=R, P=P)
    _balance_refusals(ptr, B=B, P=P)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == SENTINEL).all()), k
