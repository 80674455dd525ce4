"""Statement (plain numpy) of the parts across two plans -- TEST INFRASTRUCTURE ONLY, the arbiter of csrc/gnr_track.hip (include/gnr.h,
gnr_part_overlap_fwd and gnr_part_track_fwd, has the same words).
overlap(): table[i,j] counts the voxels with index(before) = i and index(after) = j (index(l) = l in 1..P, 0 below 1), (0,0) left out,
and `beyond` those where either label lies above P.  track(): per old part its heir (where most of its voxels are now), per new part
its source (what it is mostly made of), each kept only at `share` of the part's size; the two agreeing is "the same part", which
STAYED at `stay` of the union and MOVED below it; the rest is GONE, MERGED, NEW, FRAGMENT.  The only floating point is the float64
multiply and compare of those two thresholds.  Everything is compared with np.array_equal.
Vectorised (bincount, argmax over the table); tests/test_part_track.py holds the literal restatement, one voxel and one table row at a
time, and compares."""
import numpy as np

f64, i32, i64 = np.float64, np.int32, np.int64
DEFAULTS = dict(share=0.5, stay=0.6)
MAX_PARTS = 256
STAYED, MOVED, GONE, MERGED = 0, 1, 2, 3
SAME, NEW, FRAGMENT = 0, 1, 2
OLD_COLUMNS = ('heir', 'shared', 'size_before', 'vacated', 'pieces', 'fate')
NEW_COLUMNS = ('source', 'size_after', 'fresh', 'absorbed', 'origin')
COLUMNS = (*OLD_COLUMNS, *NEW_COLUMNS)
SUMMARY = ('nb', 'na', 'stayed', 'moved', 'gone', 'merged', 'new', 'fragments')


def overlap(before, after, max_parts):
    """One scene: two label volumes [R,R,R] int32 -> (table [P+1,P+1] int32, beyond int32)."""
    a, c = np.asarray(before, i32).astype(i64).reshape(-1), np.asarray(after, i32).astype(i64).reshape(-1)
    P = int(max_parts)
    assert a.shape == c.shape and 1 <= P <= MAX_PARTS
    out = (a > P) | (c > P)
    i, j = np.maximum(a, 0)[~out], np.maximum(c, 0)[~out]
    table = np.bincount(i * (P + 1) + j, minlength=(P + 1) ** 2).reshape(P + 1, P + 1)
    table[0, 0] = 0
    return table.astype(i32), i32(out.sum())


def _first_largest(block, axis):
    """(the largest entry along `axis`, the smallest index that has it); an empty axis gives (0, -1)."""
    if block.shape[axis] == 0:
        n = block.shape[1 - axis]
        return np.zeros(n, i64), np.full(n, -1, i64)
    at = block.argmax(axis)                                                    # (the first occurrence: the smallest index)
    return np.take_along_axis(block, np.expand_dims(at, axis), axis).squeeze(axis), at


def track(table, count_before, count_after, share=0.5, stay=0.6):
    """One scene: table [P+1,P+1] int32 and the two counts -> dict of COLUMNS [P] int32 and `summary` [8] int32; rows beyond the parts
    hold 0, and -1 in fate / origin."""
    T = np.asarray(table, i32)
    P = T.shape[0] - 1
    assert T.shape == (P + 1, P + 1) and 1 <= P <= MAX_PARTS
    nb, na = min(max(int(count_before), 0), P), min(max(int(count_after), 0), P)
    T = T[:nb + 1, :na + 1].astype(i64)
    wrap = lambda s: s.astype(i32).astype(i64)                                 # (int32 sums, as the device adds)
    size_b, size_a = wrap(T[1:].sum(1)), wrap(T[:, 1:].sum(0))                 # [nb], [na]
    core = T[1:, 1:]
    t_row, at_row = _first_largest(core, 1)                                    # per old part
    t_col, at_col = _first_largest(core, 0)                                    # per new part
    share, stay = f64(share), f64(stay)
    heir = np.where((t_row >= 1) & (t_row.astype(f64) >= share * size_b.astype(f64)), at_row + 1, 0)
    source = np.where((t_col >= 1) & (t_col.astype(f64) >= share * size_a.astype(f64)), at_col + 1, 0)
    back = np.where(heir > 0, np.append(source, 0)[heir - 1], -1)              # source[heir[a]]
    same = (heir > 0) & (back == np.arange(1, nb + 1))
    union = size_b + np.where(heir > 0, np.append(size_a, 0)[heir - 1], 0) - t_row
    fate = np.where(heir == 0, GONE, np.where(~same, MERGED, np.where(t_row.astype(f64) >= stay * union.astype(f64), STAYED, MOVED)))
    forth = np.where(source > 0, np.append(heir, 0)[source - 1], -1)           # heir[source[b]]
    origin = np.where(source == 0, NEW, np.where(forth == np.arange(1, na + 1), SAME, FRAGMENT))
    out = {k: np.zeros(P, i32) for k in COLUMNS}
    out['fate'][:], out['origin'][:] = -1, -1
    old = dict(heir=heir, shared=t_row, size_before=size_b, vacated=T[1:, 0], pieces=np.bincount(source, minlength=nb + 1)[1:], fate=fate)
    new = dict(source=source, size_after=size_a, fresh=T[0, 1:], absorbed=np.bincount(heir, minlength=na + 1)[1:], origin=origin)
    for k, v in old.items():
        out[k][:nb] = v
    for k, v in new.items():
        out[k][:na] = v
    out['summary'] = i32([nb, na, (fate == STAYED).sum(), (fate == MOVED).sum(), (fate == GONE).sum(), (fate == MERGED).sum(),
                          (origin == NEW).sum(), (origin == FRAGMENT).sum()])
    return out


def track_of_labels(before, after, count_before, count_after, max_parts, **params):
    """overlap() then track() of one scene -> track()'s dict with `table` and `beyond` added."""
    table, beyond = overlap(before, after, max_parts)
    return dict(track(table, count_before, count_after, **params), table=table, beyond=beyond)
