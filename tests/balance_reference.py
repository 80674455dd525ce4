"""Statement (plain numpy) of the balance of the parts of a label volume -- TEST INFRASTRUCTURE ONLY, the arbiter of
csrc/gnr_balance.hip (include/gnr.h, gnr_part_feet_fwd and gnr_part_balance_fwd, has the same words).
slots(): the footings of a part take the foot slots 1, 2, .. in ascending label order, from the seventh on they share slot 7; slot 0 is
the floor plane.  feet(): a voxel of part c is a foot in slot 0 when it lies in the plane k == z_min, and in slot s >= 1 when a neighbour
one plane lower carries a footing of c whose slot is s; per part and slot the number of feet and their reach along 16 directions of
the (i, j) plane, and per part the ten integer moments up to the second order.  balance(): a mass is balanced over a set of slots when
its centre lies inside the hull of the feet's unit squares along all 16 directions -- integers, and one float64 multiply and one divide
per direction for the margin --, per part over all its usable slots, and per part what tips, and what falls with it, when it is taken.
Everything is compared with np.array_equal, the margin by its bits.
Vectorised over shifted views; tests/test_part_balance.py holds the literal restatement, one voxel and one neighbour at a time, and
compares."""
import numpy as np

from parts_reference import _views, offsets

f64 = np.float64
MAX_PARTS, SLOTS, DIRECTIONS = 256, 8, 16
_HALF = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1))
DIRS = np.array(_HALF + tuple((-x, -y) for x, y in _HALF), np.int64)          # [16,2]: dx, dy
LENGTH = np.sqrt((DIRS.astype(f64) ** 2).sum(1))                              # 1, sqrt 5, sqrt 2, ..: the nearest doubles
WIDTH = np.abs(DIRS).sum(1)                                                    # |dx| + |dy|: a unit square's own width along d, doubled
NONE = np.iinfo(np.int32).min
MOMENTS = ('n', 'i', 'j', 'k', 'ii', 'jj', 'kk', 'ij', 'ik', 'jk')
COLUMNS = ('balanced', 'margin', 'unsettles', 'falls')


def slots(rests_on, count):
    """One scene: rests_on [P,P] (any bytes: != 0 holds), count -> (slots [P,P] uint8, crowded [P] int32)."""
    rel = np.asarray(rests_on)
    P = rel.shape[0]
    n = min(max(int(count), 0), P)
    foot = np.zeros((P, P), bool)
    foot[:n, :n] = (rel[:n, :n] != 0) & ~np.eye(n, dtype=bool)
    rank = np.cumsum(foot, 1)                                                  # 1, 2, .. in ascending label order
    return np.where(foot, np.minimum(rank, SLOTS - 1), 0).astype(np.uint8), (foot.sum(1) >= SLOTS).astype(np.int32)     # crowded: slot 7 holds two or more


def feet(labels, slot_rows, connectivity=26, z_min=0):
    """One scene: labels [R,R,R] int32, slots [P,P] -> (moments [P,10] int64, feet [P,8] int32, reach [P,8,16] int32)."""
    lab = np.asarray(labels, np.int32).astype(np.int64)
    slot_rows = np.asarray(slot_rows)
    R, P = lab.shape[0], slot_rows.shape[0]
    assert lab.shape == (R, R, R) and R >= 2 and 1 <= P <= MAX_PARTS and 0 <= z_min <= R
    part = (lab >= 1) & (lab <= P)
    mask = np.zeros((R, R, R), np.int64)                                       # bit s: a foot in slot s
    if z_min < R:
        mask[:, :, z_min] |= part[:, :, z_min]
    for d in offsets(connectivity):
        if d[2] != -1:                                                         # k_w < k_u: the neighbours one plane lower
            continue
        u, w = _views(R, d)
        c, a = lab[u], lab[w]
        ok = part[u] & part[w] & (a != c)
        s = np.where(ok, slot_rows[np.where(ok, c, 1) - 1, np.where(ok, a, 1) - 1], 0).astype(np.int64)
        mask[u] |= np.where(s > 0, 1 << s, 0)
    i, j, k = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing='ij')
    moments = np.zeros((P, 10), np.int64)
    row = lab[part] - 1
    for col, v in enumerate((np.ones_like(i), i, j, k, i * i, j * j, k * k, i * j, i * k, j * k)):
        np.add.at(moments[:, col], row, v[part])
    count, reach = np.zeros((P, SLOTS), np.int64), np.full((P, SLOTS, DIRECTIONS), NONE, np.int64)
    for s in range(SLOTS):
        sel = part & ((mask >> s) & 1 > 0)
        row = lab[sel] - 1
        np.add.at(count[:, s], row, 1)
        for q, (dx, dy) in enumerate(DIRS):
            np.maximum.at(reach[:, s, q], row, dx * i[sel] + dy * j[sel])
    return moments, count.astype(np.int32), reach.astype(np.int32)


def usable(feet_row, min_floor=1):
    """feet [..,8] -> [..,8] bool: the slots that have feet; slot 0 wants min_floor of them."""
    out = np.asarray(feet_row) >= 1
    out[..., 0] = np.asarray(feet_row)[..., 0] >= int(min_floor)
    return out


def balance_of(m, Si, Sj, reach_row, chosen):
    """The balance of the mass (m voxels, sums Si, Sj) over the slots `chosen` [8] bool (usable ones) of one part's reach [8,16]
    -> (balanced, margin float64)."""
    m = int(m)
    if m < 1 or not np.any(chosen):
        return False, f64(-np.inf)
    r = np.asarray(reach_row, np.int64)[np.asarray(chosen, bool)].max(0)
    num = np.int64(m) * (2 * r + WIDTH) - 2 * (DIRS[:, 0] * np.int64(Si) + DIRS[:, 1] * np.int64(Sj))
    return bool((num >= 0).all()), (num.astype(f64) / (f64(2 * m) * LENGTH)).min()


def balance(moments, feet_rows, reach, slot_rows, rests_on, count, min_floor=1):
    """One scene -> dict of balanced [P] int32, margin [P] float64, unsettles, falls [P] int32, tips [P,P] uint8 ([c-1,a-1]: c tips
    when a is taken); rows beyond n = min(max(count, 0), P) hold 0 and -inf."""
    moments, feet_rows, reach = np.asarray(moments, np.int64), np.asarray(feet_rows, np.int32), np.asarray(reach, np.int32)
    slot_rows, rel = np.asarray(slot_rows), np.asarray(rests_on)
    P = len(feet_rows)
    n = min(max(int(count), 0), P)
    out = dict(balanced=np.zeros(P, np.int32), margin=np.full(P, -np.inf, f64), unsettles=np.zeros(P, np.int32), falls=np.zeros(P, np.int32),
               tips=np.zeros((P, P), np.uint8))
    rests = np.zeros((P, P), bool)
    rests[:n, :n] = (rel[:n, :n] != 0) & ~np.eye(n, dtype=bool)
    ok = usable(feet_rows, min_floor)
    without = np.zeros((P, SLOTS), bool)                                       # [c,s]: c is not balanced once slot s is gone
    for c in range(n):
        m, Si, Sj = moments[c, 0], moments[c, 1], moments[c, 2]
        out['balanced'][c], out['margin'][c] = balance_of(m, Si, Sj, reach[c], ok[c])
        for s in range(SLOTS):
            without[c, s] = not balance_of(m, Si, Sj, reach[c], ok[c] & (np.arange(SLOTS) != s))[0]
    tips = rests & without[np.arange(P)[:, None], slot_rows.astype(np.int64) & (SLOTS - 1)]
    # carried: reach_[a,c]: c reached from a along "rests on" (support_reference's closure)
    step = rests.T.astype(f64)
    closure = rests.T.copy()
    for _ in range(n):
        more = closure | ((closure.astype(f64) @ step) > 0)
        if np.array_equal(more, closure):
            break
        closure = more
    for a in range(n):
        first = tips[:, a]
        gone = first | closure[first].any(0)
        gone[a] = False
        out['unsettles'][a], out['falls'][a] = first.sum(), gone.sum()
    out['tips'] = tips.astype(np.uint8)
    return out


def balance_of_labels(labels, rests_on, count, connectivity=26, z_min=0, min_floor=1):
    """slots(), feet() then balance() of one scene -> balance()'s dict with `moments`, `slots`, `feet`, `reach`, `crowded` added."""
    slot_rows, crowded = slots(rests_on, count)
    moments, feet_rows, reach = feet(labels, slot_rows, connectivity, z_min)
    return dict(balance(moments, feet_rows, reach, slot_rows, rests_on, count, min_floor), moments=moments, slots=slot_rows, feet=feet_rows,
                reach=reach, crowded=crowded)
