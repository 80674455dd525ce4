"""Statement (plain numpy) of the support of the parts of a label volume -- TEST INFRASTRUCTURE ONLY, the arbiter of
csrc/gnr_support.hip (include/gnr.h, gnr_part_contacts_fwd and gnr_part_support_fwd, has the same words).
contacts(): every ordered pair of neighbouring voxels with two different labels >= 1 counts once in touch[a,b], and once in over[a,b]
when b's voxel is the higher one along axis 2; labels beyond the rows count in `dropped`; floor[a] counts a's voxels in the plane
k == z_min.  support(): c rests on a when the net of over is positive and at least `lean` times the touch count -- the one float64
multiply and compare --, and from that relation the footings, what a part carries, what loses every footing when it is taken, the
layers of an order of removal, and what is grounded.  Everything is compared with np.array_equal.
Vectorised over shifted views and boolean matrices; tests/test_part_support.py holds the literal restatement, one voxel and one
neighbour at a time, and compares."""
import numpy as np

from parts_reference import _views, offsets

f64 = np.float64
DEFAULTS = dict(lean=0.25, min_contact=1, min_floor=1)
MAX_PARTS = 256
COLUMNS = ('below', 'above', 'carried', 'orphans', 'layer', 'grounded')


def contacts(labels, max_parts, connectivity=26, z_min=0):
    """One scene: labels [R,R,R] int32 -> (pairs [P,P,2] int32: touch and over, floor [P] int32, dropped int32)."""
    lab = np.asarray(labels, np.int32)
    R, P = lab.shape[0], int(max_parts)
    assert lab.shape == (R, R, R) and R >= 2 and 1 <= P <= MAX_PARTS and 0 <= z_min <= R
    pairs, dropped = np.zeros((P, P, 2), np.int64), 0
    for d in offsets(connectivity):                                            # w = u + d: every ordered pair of neighbours once
        u, w = _views(R, d)
        a, b = lab[u].astype(np.int64), lab[w].astype(np.int64)
        m = (a >= 1) & (b >= 1) & (a != b)
        rows = m & (a <= P) & (b <= P)
        np.add.at(pairs[:, :, 0], (a[rows] - 1, b[rows] - 1), 1)
        if d[2] > 0:                                                           # k_w > k_u
            np.add.at(pairs[:, :, 1], (a[rows] - 1, b[rows] - 1), 1)
        dropped += int((m & ~rows).sum())
    floor = np.zeros(P, np.int64)
    if z_min < R:
        plane = lab[:, :, z_min].astype(np.int64)
        plane = plane[(plane >= 1) & (plane <= P)]
        np.add.at(floor, plane - 1, 1)
    return pairs.astype(np.int32), floor.astype(np.int32), np.int32(dropped)


def relation(pairs, n, lean=0.25, min_contact=1):
    """rests [n,n] bool: rests[c,a] = c rests on a (0-based rows), over the parts 1..n of one scene's table."""
    touch, over = np.asarray(pairs)[:n, :n, 0].astype(np.int64), np.asarray(pairs)[:n, :n, 1].astype(np.int64)
    D = over - over.T                                                          # [a,c]
    holds = (touch >= int(min_contact)) & (D > 0) & (D.astype(f64) >= f64(lean) * touch.astype(f64)) & ~np.eye(n, dtype=bool)
    return holds.T


def support(pairs, floor, count, lean=0.25, min_contact=1, min_floor=1):
    """One scene: pairs [P,P,2] int32, floor [P] int32, count -> dict of below, above, carried, orphans, layer, grounded [P] int32 and
    rests_on [P,P] uint8 ([c-1,a-1]); rows beyond n = min(max(count, 0), P) hold the empty values."""
    pairs, floor = np.asarray(pairs, np.int32), np.asarray(floor, np.int32)
    P = len(floor)
    assert pairs.shape == (P, P, 2)
    n = min(max(int(count), 0), P)
    rests = relation(pairs, n, lean, min_contact)
    on_floor = floor[:n] >= int(min_floor)
    below, above = rests.sum(1), rests.sum(0)
    # carried: the parts reachable along "rests on a" -- reach[a,c]: c reached from a
    step = rests.T.astype(f64)                                                 # (products of 0 / 1 counts up to 256: exact in float64)
    reach = rests.T.copy()
    for _ in range(n):
        more = reach | ((reach.astype(f64) @ step) > 0)
        if np.array_equal(more, reach):
            break
        reach = more
    carried = (reach & ~np.eye(n, dtype=bool)).sum(1)
    # orphans: F[a] starts as {a}; a round adds every c outside F, not on the floor, with a footing and every footing in F[a]
    F = np.eye(n, dtype=bool)
    may = ~on_floor & (below >= 1)
    for _ in range(n):
        outside = ((~F).astype(f64) @ step) > 0                                # [a,c]: c has a footing outside F[a]
        more = F | (may[None, :] & ~outside)
        if np.array_equal(more, F):
            break
        F = more
    orphans = F.sum(1) - 1
    # layer: 0 with nothing above; 1 + the largest layer above once every part above has one
    layer = np.where(above == 0, 0, -1).astype(np.int64)
    for _ in range(n):
        done = layer >= 0
        ready = ~done & ~(rests & ~done[:, None]).any(0)
        if not ready.any():
            break
        top = np.where(rests, layer[:, None], -1).max(0, initial=-1)
        layer = np.where(ready, top + 1, layer)
    grounded = on_floor.copy()
    for _ in range(n):
        more = grounded | (rests & grounded[None, :]).any(1)
        if np.array_equal(more, grounded):
            break
        grounded = more
    out = {k: np.zeros(P, np.int32) for k in COLUMNS}
    out['layer'][:] = -1
    for k, v in zip(COLUMNS, (below, above, carried, orphans, layer, grounded)):
        out[k][:n] = v
    out['rests_on'] = np.zeros((P, P), np.uint8)
    out['rests_on'][:n, :n] = rests
    return out


def support_of_labels(labels, count, max_parts, connectivity=26, z_min=0, **params):
    """contacts() then support() of one scene -> support()'s dict with `pairs`, `floor`, `dropped` added."""
    pairs, floor, dropped = contacts(labels, max_parts, connectivity, z_min)
    return dict(support(pairs, floor, count, **params), pairs=pairs, floor=floor, dropped=dropped)
