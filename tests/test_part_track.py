"""Parts across two plans (csrc/gnr_track.hip, track.PartOverlap, track.PartTrack, track.track_of_plans).
tests/track_reference.py is the statement (numpy integers, float64 multiplies and compares for the two thresholds); every comparison
is np.array_equal, dtypes and shapes included.  Without a GPU: the statement against a literal restatement one voxel and one table row
at a time, the synthetic pile and its three second plans, the balls behind the defaults, the host functions, the parameter checks,
every refusal of the two entry points.  On the GPU: shapes chosen to break the kernels -- random labels beyond the rows next to other
scenes, a partial last wavefront, 257 columns, counts of every kind, exact ties, the thresholds on their boundary, stale state --
then the piles through the operators, the aliasing refusal, one captured graph and track_of_plans."""
import ctypes as C
import functools
import inspect
import math
import re

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, distance, parts, support, track
import parts_reference as pref
import support_reference as sref
import test_grasp_retreat as tgr
import track_reference as tref

f32, f64, i32 = np.float32, np.float64, np.int32
VOXEL = tgr.VOXEL
SENTINEL = 0x5a
KEYS = (*tref.COLUMNS, 'summary')
S, M, G, X = tref.STAYED, tref.MOVED, tref.GONE, tref.MERGED


def same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, got, want)


def random_pair(R, seed, lo, hi):
    """Two label volumes [R,R,R] int32 uniform in lo..hi, unrelated on purpose: every cell of the table gets something."""
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, (R, R, R)).astype(i32), rng.integers(lo, hi + 1, (R, R, R)).astype(i32)


# ---- 1. the statement (no GPU) --------------------------------------------------------------------------------------------------------
def overlap_restatement(before, after, P):
    """include/gnr.h's words one voxel at a time, in plain Python."""
    R = before.shape[0]
    table, beyond = [[0] * (P + 1) for _ in range(P + 1)], 0
    for i in range(R):
        for j in range(R):
            for k in range(R):
                a, c = int(before[i, j, k]), int(after[i, j, k])
                if a > P or c > P:
                    beyond += 1
                    continue
                a, c = max(a, 0), max(c, 0)
                if (a, c) != (0, 0):
                    table[a][c] += 1
    return i32(table).reshape(P + 1, P + 1), i32(beyond)


def track_restatement(table, count_before, count_after, share=0.5, stay=0.6):
    """The fates one table row at a time, as the header words them."""
    P = len(table) - 1
    nb, na = min(max(int(count_before), 0), P), min(max(int(count_after), 0), P)
    T = [[int(v) for v in row] for row in table]
    size_b = {a: sum(T[a][j] for j in range(na + 1)) for a in range(1, nb + 1)}
    size_a = {b: sum(T[i][b] for i in range(nb + 1)) for b in range(1, na + 1)}
    heir, source, shared = {}, {}, {}
    for a in range(1, nb + 1):
        best, t = 0, None
        for b in range(1, na + 1):
            if t is None or T[a][b] > t:
                best, t = b, T[a][b]
        shared[a] = 0 if t is None else t
        heir[a] = best if t is not None and t >= 1 and float(t) >= float(share) * float(size_b[a]) else 0
    for b in range(1, na + 1):
        best, t = 0, None
        for a in range(1, nb + 1):
            if t is None or T[a][b] > t:
                best, t = a, T[a][b]
        source[b] = best if t is not None and t >= 1 and float(t) >= float(share) * float(size_a[b]) else 0
    out = {k: [0] * P for k in tref.COLUMNS}
    out['fate'], out['origin'] = [-1] * P, [-1] * P
    for a in range(1, nb + 1):
        b = heir[a]
        if b == 0:
            fate = G
        elif source[b] != a:
            fate = X
        else:
            t = T[a][b]
            fate = S if float(t) >= float(stay) * float(size_b[a] + size_a[b] - t) else M
        row = dict(heir=b, shared=shared[a], size_before=size_b[a], vacated=T[a][0], pieces=sum(1 for c in source.values() if c == a), fate=fate)
        for k, v in row.items():
            out[k][a - 1] = v
    for b in range(1, na + 1):
        a = source[b]
        origin = tref.NEW if a == 0 else tref.SAME if heir[a] == b else tref.FRAGMENT
        row = dict(source=a, size_after=size_a[b], fresh=T[0][b], absorbed=sum(1 for c in heir.values() if c == b), origin=origin)
        for k, v in row.items():
            out[k][b - 1] = v
    count = lambda k, v: sum(1 for x in out[k] if x == v)
    out = {k: i32(v) for k, v in out.items()}
    out['summary'] = i32([nb, na, count('fate', S), count('fate', M), count('fate', G), count('fate', X), count('origin', tref.NEW),
                          count('origin', tref.FRAGMENT)])
    return out


def blocky_pair(R, seed, P):
    """Two label volumes of a few slabs each, so that heirs and sources exist, with a little noise and labels beyond P."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        lab = np.zeros((R, R, R), i32)
        cuts = np.sort(rng.integers(0, R + 1, 3))
        for n, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            lab[lo:hi, :, rng.integers(0, 2):] = rng.integers(1, P + 1)
        noise = rng.random((R, R, R)) < 0.1
        lab[noise] = rng.integers(-1, P + 2, int(noise.sum()))
        out.append(lab)
    return out


@pytest.mark.parametrize('R', [5, 8])
def test_the_statement_equals_its_literal_restatement(R):
    kinds, beyond = set(), 0
    for seed in range(6):
        P = (4, 3, 6)[seed % 3]
        before, after = random_pair(R, 10 * R + seed, -1, P + 2) if seed < 2 else blocky_pair(R, 10 * R + seed, P)
        got, want = tref.overlap(before, after, P), overlap_restatement(before, after, P)
        same((R, seed, 'table'), got[0], want[0])
        same((R, seed, 'beyond'), got[1], want[1])
        assert got[0][0, 0] == 0 and got[0].sum() + got[1] + ((before < 1) & (after < 1)).sum() == R ** 3
        beyond += int(got[1])
        for nb, na in ((P, P), (P - 1, P + 3), (0, P), (P, 0), (-2, 2), (2, 1)):
            for p in (dict(), dict(share=0.0, stay=0.0), dict(share=0.3, stay=1.0), dict(share=1.0)):
                g, w = tref.track(got[0], nb, na, **p), track_restatement(got[0], nb, na, **p)
                for k in KEYS:
                    same((R, seed, nb, na, p, k), g[k], w[k])
                kinds |= {('fate', int(v)) for v in g['fate']} | {('origin', int(v)) for v in g['origin']}
                n = max(0, min(nb, P))
                assert (g['fate'][n:] == -1).all() and not any(g[k][n:].any() for k in tref.OLD_COLUMNS if k != 'fate')
    assert beyond > 0 and kinds >= {('fate', v) for v in (-1, S, M, G, X)} | {('origin', v) for v in (-1, 0, 1, 2)}, kinds


BOX, TOP, SIDE = ((11, 11, 3), (27, 27, 10)), (19, 19, 16), (19, 34, 8)


@functools.lru_cache(maxsize=None)
def pile_masks():
    """The pile at 40^3: a box, a ball of radius 5 on it, a ball of radius 5 beside it; the side ball shifted by one voxel; the box
    with a slab of one voxel taken out of it (9 and 7 voxels wide).  Never written to."""
    R = 40
    out = dict(box=tgr.box(R, *BOX), top=tgr.ball(R, TOP, 5), side=tgr.ball(R, SIDE, 5), shifted=tgr.ball(R, (SIDE[0] + 1, *SIDE[1:]), 5))
    out['half_lo'] = out['box'] & (tgr.lattice(R)[0] <= 19)
    out['half_hi'] = out['box'] & (tgr.lattice(R)[0] >= 21)
    assert not (out['box'] & out['top']).any() and not (out['box'] & out['side']).any() and not (out['box'] & out['shifted']).any()
    for m in out.values():
        m.setflags(write=False)
    return out


def painted(**labels):
    """A label volume with the named masks of pile_masks() painted in the order given."""
    lab = np.zeros((40, 40, 40), i32)
    for name, L in labels.items():
        lab[pile_masks()[name]] = L
    return lab


def test_the_pile_and_its_second_plans():
    col = lambda s, k, n: [int(v) for v in s[k][:n]]
    before = painted(box=1, top=2, side=3)
    # the top ball taken, the side ball shifted by a voxel, and the numbering turned round
    s = tref.track_of_labels(before, painted(shifted=1, box=2), 3, 2, 8)
    assert col(s, 'heir', 3) == [2, 0, 1] and col(s, 'fate', 3) == [S, G, S] and col(s, 'origin', 2) == [tref.SAME, tref.SAME]
    assert col(s, 'source', 2) == [3, 1] and col(s, 'pieces', 3) == [1, 0, 1] and col(s, 'absorbed', 2) == [1, 1] and s['beyond'] == 0
    assert s['summary'].tolist() == [3, 2, 2, 0, 1, 0, 0, 0] and col(s, 'vacated', 3)[1] == col(s, 'size_before', 3)[1] == int(pile_masks()['top'].sum())
    assert (s['fate'][3:] == -1).all() and (s['origin'][2:] == -1).all() and not s['heir'][3:].any()
    # the same with the top ball's voxels given the box's label
    s = tref.track_of_labels(before, painted(shifted=1, box=2, top=2), 3, 2, 8)
    assert col(s, 'heir', 3) == [2, 2, 1] and col(s, 'fate', 3) == [S, X, S] and col(s, 'absorbed', 2) == [1, 2] and col(s, 'source', 2) == [3, 1]
    assert s['summary'].tolist() == [3, 2, 2, 0, 0, 1, 0, 0]
    # the box cut in two labels in the second plan: 9 of its 17 planes keep to the larger piece
    s = tref.track_of_labels(before, painted(box=1, half_hi=4, top=2, side=3), 3, 4, 8)
    assert col(s, 'fate', 3) == [M, S, S] and col(s, 'pieces', 3) == [2, 1, 1] and col(s, 'heir', 3) == [1, 2, 3]
    assert col(s, 'origin', 4) == [tref.SAME, tref.SAME, tref.SAME, tref.FRAGMENT] and s['summary'].tolist() == [3, 4, 2, 1, 0, 0, 0, 1]
    h = host_track(s, 3, 4)
    assert track.take_verdict(h, 2) == dict(removed=False, fate='STAYED', disturbed=[1], appeared=[], remaining=4)


BALLS = {(3, 1): (0.764, 0.618), (3, 2): (0.561, 0.390), (5, 1): (0.843, 0.728), (5, 2): (0.709, 0.549), (5, 3): (0.575, 0.403),
         (5, 4): (0.441, None), (8, 1): (None, 0.829), (8, 2): (None, 0.688), (8, 3): (None, 0.567)}


def test_what_the_defaults_mean_on_balls():
    """The table of track.py's docstring: a ball of the radius, shifted along one axis, against itself."""
    assert track.TRACK_DEFAULTS == tref.DEFAULTS == dict(share=0.5, stay=0.6)
    for (r, shift), (share, iou) in BALLS.items():
        a, b = tgr.ball(32, (12, 16, 16), r), tgr.ball(32, (12 + shift, 16, 16), r)
        s = tref.track_of_labels(a.astype(i32), b.astype(i32), 1, 1, 1)
        t, size = int(s['shared'][0]), int(s['size_before'][0])
        assert size == a.sum() == s['size_after'][0] and t == (a & b).sum()
        if share is not None:
            assert round(t / size, 3) == share, (r, shift, t / size)
        if iou is not None:
            assert round(t / (2 * size - t), 3) == iou, (r, shift, t / (2 * size - t))
        want = G if t / size < 0.5 else S if t / (2 * size - t) >= 0.6 else M
        assert s['fate'][0] == want and (s['origin'][0] == tref.NEW) == (want == G), (r, shift)
    assert [int(tref.track_of_labels(tgr.ball(32, (12, 16, 16), 5).astype(i32), tgr.ball(32, (12 + d, 16, 16), 5).astype(i32), 1, 1, 1)['fate'][0])
            for d in range(6)] == [S, S, M, M, G, G]


def test_the_thresholds_on_their_boundary():
    """t == share * size holds; the next double above does not.  A part of 8 voxels sharing 4, and the same one voxel short."""
    T = i32([[0, 0, 0], [4, 4, 0], [0, 0, 5]])                                  # part 1: 8 voxels, 4 of them now in new part 1
    assert tref.track(T, 2, 2, share=0.5)['heir'].tolist() == [1, 2] and tref.track(T, 2, 2, share=0.5)['fate'].tolist() == [M, S]
    assert tref.track(T, 2, 2, share=np.nextafter(0.5, 1.0))['heir'].tolist() == [0, 2]
    T[1] = (5, 3, 0)
    g = tref.track(T, 2, 2, share=0.5)
    assert g['heir'].tolist() == [0, 2] and g['source'].tolist() == [1, 2] and g['fate'].tolist() == [G, S] and g['origin'].tolist() == [tref.FRAGMENT, tref.SAME]
    T = i32([[0, 2, 0], [0, 3, 0], [0, 0, 1]])                                  # t = 3 over a union of 5: exactly 0.6 in doubles
    assert tref.track(T, 2, 2, stay=0.6)['fate'][0] == (S if 3.0 >= 0.6 * 5.0 else M) == S
    assert tref.track(T, 2, 2, stay=np.nextafter(0.6, 1.0))['fate'][0] == M
    T = i32([[0, 0, 0], [0, 0, 0], [0, 0, 0]])                                  # a count of zero is never an heir, not even at share 0
    assert tref.track(T, 2, 2, share=0.0)['heir'].tolist() == [0, 0] and tref.track(T, 2, 2, share=0.0)['origin'].tolist() == [tref.NEW] * 2


def host_track(s, nb, na, **params):
    """track.track_from_rows on the statement's arrays of one scene."""
    rows = {k: s[k][:nb] for k in tref.OLD_COLUMNS}
    rows.update({k: s[k][:na] for k in tref.NEW_COLUMNS})
    rows.update(table=s['table'][:nb + 1, :na + 1], summary=s['summary'], beyond=i32([s['beyond']]), count_before=i32([nb]), count_after=i32([na]))
    return track.track_from_rows(rows, **params)


def test_host_functions():
    before = painted(box=1, top=2, side=3)
    s = tref.track_of_labels(before, painted(shifted=1, box=2), 3, 2, 8)
    h = host_track(s, 3, 2)
    assert list(h) == [*tref.COLUMNS, 'fate_name', 'origin_name', 'table', 'summary', 'nb', 'na', 'share', 'stay']
    assert all(h[k].dtype == i32 and h[k].shape == (3,) for k in tref.OLD_COLUMNS) and all(h[k].shape == (2,) for k in tref.NEW_COLUMNS)
    assert h['fate_name'] == ['STAYED', 'GONE', 'STAYED'] and h['origin_name'] == ['SAME', 'SAME'] and h['table'].shape == (4, 3)
    assert h['summary'] == dict(nb=3, na=2, stayed=2, moved=0, gone=1, merged=0, new=0, fragments=0) and (h['nb'], h['na']) == (3, 2)
    assert track.take_verdict(h, 2) == dict(removed=True, fate='GONE', disturbed=[], appeared=[], remaining=2)
    assert track.take_verdict(h, 1) == dict(removed=False, fate='STAYED', disturbed=[2], appeared=[], remaining=2)
    # the side ball rolled away: GONE and a NEW part
    far = tref.track_of_labels(before, np.where(tgr.ball(40, (30, 34, 8), 5), 1, painted(box=2)).astype(i32), 3, 2, 8)
    v = track.take_verdict(host_track(far, 3, 2), 2)
    assert v == dict(removed=True, fate='GONE', disturbed=[3], appeared=[1], remaining=2)
    # with the support of the first plan: the top ball rests on the box, so taking the box predicts it orphaned and carried
    sup = sref.support_of_labels(before, 3, 8, 26, 3)
    rows = {k: sup[k][:3] for k in (*sref.COLUMNS, 'floor')}
    rows.update(pairs=sup['pairs'][:3, :3], rests_on=sup['rests_on'][:3, :3], dropped=i32([0]), count=i32([3]))
    hs = support.support_from_rows(rows)
    assert hs['rests_on'][1, 0] and hs['orphans'].tolist() == [1, 0, 0]
    v = track.take_verdict(h, 1, support=hs)
    assert v['predicted'] == dict(orphans=[2], carried=[2]) and v['not_stayed'] == dict(orphans=[2], carried=[2])
    v = track.take_verdict(h, 2, support=hs)
    assert v['predicted'] == dict(orphans=[], carried=[]) and v['not_stayed'] == dict(orphans=[], carried=[]) and v['removed']
    for bad in (0, 4, 1.5, True):
        with pytest.raises(ValueError, match='part must be a label of the first plan, 1..3'):
            track.take_verdict(h, bad)
    with pytest.raises(ValueError, match='support must be the first plan\'s'):
        track.take_verdict(h, 1, support=dict(rests_on=np.zeros((2, 2), bool), on_floor=np.zeros(2, bool)))
    # the two refusals of track_from_rows
    rows = {k: s[k][:3] for k in tref.OLD_COLUMNS}
    rows.update({k: s[k][:2] for k in tref.NEW_COLUMNS})
    rows.update(table=s['table'][:4, :3], summary=s['summary'], beyond=i32([0]), count_before=i32([3]), count_after=i32([2]))
    with pytest.raises(_lib.GnrError, match='5 parts before but the track tables hold 3: raise max_parts'):
        track.track_from_rows(dict(rows, count_before=i32([5])))
    with pytest.raises(_lib.GnrError, match='4 parts after but the track tables hold 2: raise max_parts'):
        track.track_from_rows(dict(rows, count_after=i32([4])))
    with pytest.raises(_lib.GnrError, match='more than 256 parts'):
        track.track_from_rows(dict(rows, count_after=i32([300])), max_parts=256)
    with pytest.raises(_lib.GnrError, match='7 voxels carry labels beyond the rows of the overlap table: raise max_parts'):
        track.track_from_rows(dict(rows, beyond=i32([7])))


def test_track_params():
    want = dict(share=0.5, stay=0.6)
    assert track.track_params(False) is None and track.track_params(None) is None
    assert track.track_params(True) == want == track.track_params({}) == track.TRACK_DEFAULTS == track.checked_track() == tref.DEFAULTS
    p = track.track_params(dict(share=1, taken=2), taken=None)
    assert p == dict(want, share=1.0, taken=2) and isinstance(p['share'], float)
    with pytest.raises(TypeError, match='unknown track parameters'):
        track.track_params(dict(lean=0.25))
    for k in ('share', 'stay'):
        for bad in (-0.1, 1.5, math.nan, math.inf, True):
            with pytest.raises(ValueError, match=f'track {k} must be finite and in 0..1'):
                track.track_params({k: bad})
    params = inspect.signature(track.PartTrack.__call__).parameters
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want) and {k: params[k].default for k in want} == want
    assert inspect.signature(track.PartOverlap.__call__).parameters['max_parts'].kind is inspect.Parameter.KEYWORD_ONLY
    assert track.MAX_PARTS == _lib.GNR_TRACK_MAX_PARTS == tref.MAX_PARTS == 256
    assert (track.STAYED, track.MOVED, track.GONE, track.MERGED, track.SAME, track.NEW, track.FRAGMENT) == (S, M, G, X, tref.SAME, tref.NEW, tref.FRAGMENT)
    assert track.TRACK_COLUMNS == tref.COLUMNS and track.SUMMARY_FIELDS == tref.SUMMARY
    for bad in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match='track max_parts must be an integer in 1..256'):
            track.checked_rows(bad)
    vol = np.ones((4, 4, 4), f32)
    with pytest.raises(TypeError, match='unknown track parameters'):
        track.track_of_plans(vol, vol, lean=0.25)
    with pytest.raises(ValueError, match='track stay must be finite and in 0..1'):
        track.track_of_plans(vol, vol, stay=2.0)
    with pytest.raises(ValueError, match='track z_min must be an integer >= 0'):
        track.track_of_plans(vol, vol, z_min=-1)
    with pytest.raises(ValueError, match='parts neck must be finite and in 0..1'):
        track.track_of_plans(vol, vol, neck=3.0)


def test_part_track_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for cls in (track.PartOverlap, track.PartTrack):
        with pytest.raises(_lib.GnrError, match='no CPU fallback'):
            cls()


# ---- 2. the refusals of the two entry points ------------------------------------------------------------------------------------------
OVERLAP_PTRS = ('before', 'after', 'table', 'beyond')
TRACK_PTRS = ('table', 'count_before', 'count_after', *tref.COLUMNS, 'summary')
ROWS_TEXT = ': max_parts must be in 1..GNR_TRACK_MAX_PARTS (256)'


def _overlap_refusals(ptr, B=1, R=8, P=4):
    """Every refusal of gnr_part_overlap_fwd, each with its code and its text, and their order, on the pointers given (fake ones, or
    buffers whose bytes the caller checks afterwards)."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_part_overlap_fwd'

    def call(p=None, B=B, R=R, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in OVERLAP_PTRS}
        p = _lib.GnrOverlapParams(**{**dict(max_parts=P), **kw}) if p is None else p
        return L.gnr_part_overlap_fwd(C.byref(p) if p is not False else None, a['before'], a['after'], B, R, a['table'], a['beyond'], None)

    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for r in (1, 0, 257):
        assert call(R=r) == _lib.GNR_ERR_SHAPE and text() == fn + ': R must be in 2..256', r
    for m in (0, -1, 257):
        assert call(max_parts=m) == _lib.GNR_ERR_SHAPE and text() == fn + ROWS_TEXT, m
    for name in OVERLAP_PTRS:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    faults = (dict(B=0), dict(R=1), dict(max_parts=257), dict(after=None))
    texts = (': B must be in 1..65535', ': R must be in 2..256', ROWS_TEXT, ': null pointer')
    for i in range(len(faults)):
        for j in range(i + 1, len(faults)):
            assert call(**faults[i], **faults[j]) != _lib.GNR_OK and text() == fn + texts[i], (i, j)


def _track_refusals(ptr, B=1, P=4):
    """Every refusal of gnr_part_track_fwd."""
    L = _lib.lib()
    text = lambda: L.gnr_last_error().decode()
    fn = 'gnr_part_track_fwd'

    def call(p=None, B=B, **kw):
        a = {k: kw.pop(k, ptr[k]) for k in TRACK_PTRS}
        p = _lib.GnrTrackParams(**{**dict(share=0.5, stay=0.6, max_parts=P), **kw}) if p is None else p
        return L.gnr_part_track_fwd(C.byref(p) if p is not False else None, *(a[k] for k in TRACK_PTRS[:3]), B, *(a[k] for k in TRACK_PTRS[3:]), None)

    assert call(p=False) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer'
    for b in (0, -1, 65536):
        assert call(B=b) == _lib.GNR_ERR_SHAPE and text() == fn + ': B must be in 1..65535', b
    for m in (0, -1, 257):
        assert call(max_parts=m) == _lib.GNR_ERR_SHAPE and text() == fn + ROWS_TEXT, m
    for bad in (-0.01, 1.01, math.nan, math.inf, -math.inf):
        assert call(share=bad) == _lib.GNR_ERR_ARG and text() == fn + ': share must be finite and in 0..1', bad
        assert call(stay=bad) == _lib.GNR_ERR_ARG and text() == fn + ': stay must be finite and in 0..1', bad
    for name in TRACK_PTRS:
        assert call(**{name: None}) == _lib.GNR_ERR_ARG and text() == fn + ': null pointer', name
    faults = (dict(B=0), dict(max_parts=0), dict(share=2.0), dict(stay=-1.0), dict(summary=None))
    texts = (': B must be in 1..65535', ROWS_TEXT, ': share must be finite and in 0..1', ': stay must be finite and in 0..1', ': null pointer')
    for i in range(len(faults)):
        for j in range(i + 1, len(faults)):
            assert call(**faults[i], **faults[j]) != _lib.GNR_OK and text() == fn + texts[i], (i, j)


def test_refusals_before_the_device():
    one = C.c_void_p(16)
    _overlap_refusals({k: one for k in OVERLAP_PTRS})
    _track_refusals({k: one for k in TRACK_PTRS})


def test_a_refused_call_writes_nothing_without_a_device():
    """The same refusals on host buffers of 0x5a bytes: a refused call has launched nothing and the host side writes nothing."""
    bufs = {k: np.full(4096, SENTINEL, np.uint8) for k in (*OVERLAP_PTRS, *TRACK_PTRS)}
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    _overlap_refusals(ptr)
    _track_refusals(ptr)
    for k, v in bufs.items():
        assert (v == SENTINEL).all(), k


# ---- GPU: the bits of the statement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ops():
    return track.PartOverlap(), track.PartTrack()


def check_overlap(what, before, after, P):
    """PartOverlap on B scenes, its output tensors filled with 0x5a bytes before the call, against the statement: every element is
    written.  -> the device result and the statement's (table, beyond) per scene."""
    op = _ops()[0]
    before, after = np.asarray(before, i32), np.asarray(after, i32)
    for k in ('table', 'beyond'):
        op(before, after, max_parts=P)[k].view(torch.uint8).fill_(SENTINEL)    # (the tensors of this shape)
    res = op(before, after, max_parts=P)
    torch.cuda.synchronize()
    want = [tref.overlap(a, c, P) for a, c in zip(before, after)]
    same((what, 'table'), res['table'].cpu().numpy(), np.stack([w[0] for w in want]))
    same((what, 'beyond'), res['beyond'].cpu().numpy(), np.stack([w[1] for w in want]))
    return res, want


def check_track(what, table, counts_before, counts_after, **params):
    """PartTrack on B tables (a device result of PartOverlap, or numpy tables), sentinels first, against the statement."""
    op = _ops()[1]
    if not isinstance(table, dict):
        table = dict(table=torch.from_numpy(np.ascontiguousarray(table, i32)).to('cuda:0'))
    cb, ca = (torch.tensor(list(c), dtype=torch.int32, device='cuda:0') for c in (counts_before, counts_after))
    for k in KEYS:
        op(table, cb, ca, **params)[k].view(torch.uint8).fill_(SENTINEL)
    res = op(table, cb, ca, **params)
    torch.cuda.synchronize()
    T = table['table'].cpu().numpy()
    want = [tref.track(T[b], counts_before[b], counts_after[b], **params) for b in range(len(T))]
    for k in KEYS:
        same((what, k), res[k].cpu().numpy(), np.stack([w[k] for w in want]))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('B,R', [(1, 2), (1, 5), (3, 8), (2, 16)])
def test_random_labels(B, R):
    """Labels in -1..P+3, other ones in every scene: labels beyond the rows, the partial last wavefront (R = 5: 125 voxels), threads
    past R^3; then the fates of those tables under counts within, at and beyond the rows."""
    for P in (1, 7):
        pairs = [random_pair(R, 100 * R + 10 * P + b, -1, P + 3) for b in range(B)]
        res, want = check_overlap((B, R, P), [p[0] for p in pairs], [p[1] for p in pairs], P)
        assert sum(int(w[1]) for w in want) > 0
        for p in (dict(), dict(share=0.0, stay=0.1)):
            check_track((B, R, P, p), res, [P, P + 2, 1][:B], [P, 0, P - 1][:B], **p)


@pytest.mark.gpu
def test_every_row_of_the_widest_table():
    """P = 256 at R = 16: up to 64 distinct keys in a wavefront, all 257 columns (the fifth load of lane 0), every thread a part; blocky
    volumes of 256 slabs so that heirs and sources exist, and a permutation of them."""
    R, P = 16, 256
    rng = np.random.default_rng(5)
    slabs = (np.arange(R ** 3, dtype=i32).reshape(R, R, R) // 16 + 1)          # 256 parts of 16 voxels
    moved = np.roll(slabs.reshape(-1), 5).reshape(R, R, R)                      # every part keeps 11 of its 16 voxels
    perm = np.concatenate([[0], rng.permutation(P) + 1]).astype(i32)
    noisy = np.where(rng.random((R, R, R)) < 0.2, rng.integers(-1, P + 2, (R, R, R)), moved).astype(i32)
    uniform = random_pair(R, 9, 1, P)
    res, want = check_overlap('widest', [slabs, slabs, uniform[0]], [perm[moved], noisy, uniform[1]], P)
    assert want[0][1] == 0 and want[1][1] > 0
    w = check_track('widest', res, (P, P, P), (P, P, P))
    assert (w[0]['heir'] == perm[1:]).all() and (w[0]['shared'] == 11).all() and (w[0]['fate'] == M).all() and w[0]['summary'][3] == P
    check_track('widest', res, (P + 9, 100, -1), (7, P, P), share=0.25, stay=0.3)


@pytest.mark.gpu
def test_counts_of_every_kind():
    """Counts negative, zero, beyond the rows and different per scene, on one table."""
    P = 7
    pairs = [blocky_pair(8, 40 + b, P) for b in range(6)]
    res, _ = check_overlap('counts', [p[0] for p in pairs], [p[1] for p in pairs], P)
    check_track('counts', res, (-3, 0, P + 5, 2, P, 0), (P, 4, -1, P + 1, 0, 0))
    check_track('counts', res, (P, P, P, P, P, 1), (P, P, P, P, P, 1), share=0.2)


@pytest.mark.gpu
def test_all_free_volumes():
    zero = np.zeros((2, 8, 8, 8), i32)
    res, _ = check_overlap('free', zero, zero - 1, 7)
    assert not res['table'].any().item() and not res['beyond'].any().item()
    w = check_track('free', res, (0, 0), (0, 0))
    assert all(not w[b]['summary'].any() for b in range(2))
    w = check_track('free', res, (3, 7), (2, 9))
    assert w[0]['summary'].tolist() == [3, 2, 0, 0, 3, 0, 2, 0] and w[1]['summary'].tolist() == [7, 7, 0, 0, 7, 0, 7, 0]


@pytest.mark.gpu
def test_identical_volumes_under_a_permutation_of_the_labels():
    P = 12
    lab = np.stack([np.abs(blocky_pair(12, 70 + b, P)[0]) % (P + 1) for b in range(2)]).astype(i32)
    lab[:, 0, 0, :P] = np.arange(1, P + 1)                                      # every label is there
    perm = np.concatenate([[0], np.random.default_rng(3).permutation(P) + 1]).astype(i32)
    res, _ = check_overlap('perm', lab, perm[lab], P)
    w = check_track('perm', res, (P, P), (P, P))
    for b in range(2):
        assert (w[b]['heir'] == perm[1:]).all() and (w[b]['fate'] == S).all() and (w[b]['origin'] == tref.SAME).all()
        assert (w[b]['source'][perm[1:] - 1] == np.arange(1, P + 1)).all() and w[b]['summary'].tolist() == [P, P, P, 0, 0, 0, 0, 0]


@pytest.mark.gpu
def test_exact_ties_go_to_the_smaller_label():
    """Built voxel by voxel: old part 1 has two voxels in each of the new parts 5, 3 and 6 (heir 3); new part 2 has one voxel of each of
    the old parts 7, 4 and 2 (source 2).  The voxels lie in several wavefronts and in any order."""
    R, P = 8, 7
    before, after = np.zeros((R, R, R), i32), np.zeros((R, R, R), i32)
    for n, (at, b) in enumerate(zip([(0, 0, 0), (7, 7, 7), (3, 3, 3), (0, 0, 1), (4, 0, 0), (7, 0, 2)], (5, 3, 6, 6, 5, 3))):
        before[at], after[at] = 1, b
    for at, a in zip([(6, 6, 6), (1, 1, 1), (2, 5, 0)], (7, 4, 2)):
        before[at], after[at] = a, 2
    res, _ = check_overlap('ties', before[None], after[None], P)
    w = check_track('ties', res, (P,), (P,), share=0.2)[0]
    assert w['heir'][0] == 3 and w['shared'][0] == 2 and w['source'][1] == 2 and w['size_after'][1] == 3
    w = check_track('ties', res, (P,), (P,), share=0.34)[0]
    assert w['heir'][0] == 0 and w['shared'][0] == 2 and w['source'][1] == 0


@pytest.mark.gpu
def test_the_thresholds_on_their_boundary_on_the_device():
    """A part of 8 voxels sharing 4 at share = 0.5, the same one voxel short, 3 over a union of 5 at stay = 0.6, and the next doubles."""
    def volumes(shared):
        before, after = np.zeros((4, 4, 4), i32), np.zeros((4, 4, 4), i32)
        before.reshape(-1)[:8] = 1
        after.reshape(-1)[:shared] = 1
        before.reshape(-1)[40:45], after.reshape(-1)[40:45] = 2, 2
        return before, after
    (b4, a4), (b3, a3) = volumes(4), volumes(3)
    before, after = np.zeros((4, 4, 4), i32), np.zeros((4, 4, 4), i32)
    before.reshape(-1)[:3], after.reshape(-1)[:5] = 1, 1
    res, _ = check_overlap('edge', [b4, b3, before], [a4, a3, after], 2)
    for share, stay in ((0.5, 0.6), (float(np.nextafter(0.5, 1.0)), float(np.nextafter(0.6, 1.0))), (float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.6, 0.0)))):
        w = check_track(('edge', share, stay), res, (2, 2, 1), (2, 2, 1), share=share, stay=stay)
        assert w[0]['heir'][0] == (1 if share <= 0.5 else 0) and w[1]['heir'][0] == 0 and w[2]['fate'][0] == (S if stay <= 0.6 else M)


@pytest.mark.gpu
def test_a_second_call_leaves_nothing_of_the_first():
    """The same operator objects and the same shape, other volumes, no sentinels in between: the fill, and the rows beyond nb / na."""
    P = 7
    over, trk = track.PartOverlap(), track.PartTrack()
    first, second = blocky_pair(8, 1, P), [np.where(v > 2, 0, v).astype(i32) for v in blocky_pair(8, 2, P)]
    for (a, c), (nb, na) in ((first, (P, P)), (second, (2, 1))):
        res = trk(over(a, c, max_parts=P), torch.tensor([nb], dtype=torch.int32, device='cuda:0'), torch.tensor([na], dtype=torch.int32, device='cuda:0'))
        torch.cuda.synchronize()
        w = tref.track_of_labels(a, c, nb, na, P)
        for k in (*KEYS, 'table', 'beyond'):
            same(('stale', nb, k), res[k][0].cpu().numpy(), w[k])
    assert tref.overlap(*first, P)[0][3:].any() and not w['table'][3:].any() and (w['fate'][2:] == -1).all()


def pile_volumes(which):
    """(vol_before, vol_after, the neck of the second split, {name: a voxel inside the thing} before and after)."""
    m = pile_masks()
    before = m['box'] | m['top'] | m['side']
    at = dict(box=(12, 12, 6), top=TOP, side=SIDE, shifted=(SIDE[0] + 1, *SIDE[1:]), half_lo=(12, 12, 6), half_hi=(26, 12, 6))
    if which == 'taken':
        return before, m['box'] | m['shifted'], 0.8, at, ('box', 'top', 'side'), ('box', 'shifted')
    if which == 'merged':                                                      # neck 0: the ball and the box are one component
        return before, m['box'] | m['top'] | m['shifted'], 0.0, at, ('box', 'top', 'side'), ('box', 'shifted')
    return before, m['half_lo'] | m['half_hi'] | m['top'] | m['side'], 0.8, at, ('box', 'top', 'side'), ('half_lo', 'half_hi', 'top', 'side')


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['taken', 'merged', 'cut'])
def test_the_piles_through_the_operators(which):
    """VolumeDistance and VolumeParts on each of the two volumes (two operator objects), then of_parts: the statement's bits on the
    device's own labels, and the fates by the thing, whatever number the split gave it."""
    mb, ma, neck, at, old, new = pile_volumes(which)
    vd, trk = distance.VolumeDistance(), track.PartTrack()
    rb = parts.VolumeParts()(vd(tgr.mask_volume(mb), scale=VOXEL, z_min=3)['d2_free'].clone(), max_parts=8)
    ra = parts.VolumeParts()(vd(tgr.mask_volume(ma), scale=VOXEL, z_min=3)['d2_free'], max_parts=8, neck=neck)
    res = trk.of_parts(rb, ra)
    torch.cuda.synchronize()
    lb, la = rb['labels'][0].cpu().numpy(), ra['labels'][0].cpu().numpy()
    nb, na = int(rb['count'][0].item()), int(ra['count'][0].item())
    assert (nb, na) == (len(old), len(new)) and res['max_parts'] == 8
    w = tref.track_of_labels(lb, la, nb, na, 8)
    for k in (*KEYS, 'table', 'beyond'):
        same((which, k), res[k][0].cpu().numpy(), w[k])
    h = track.track_from_rows({k: v.cpu().numpy() for k, v in track.track_rows(res, 0, nb, na).items()}, max_parts=8)
    L = {k: int(lb[at[k]]) for k in old}
    N = {k: int(la[at[k]]) for k in new}
    fate = {k: h['fate_name'][L[k] - 1] for k in old}
    if which == 'taken':
        assert fate == dict(box='STAYED', top='GONE', side='STAYED') and h['heir'][L['side'] - 1] == N['shifted'] and h['origin_name'] == ['SAME', 'SAME']
        assert track.take_verdict(h, L['top']) == dict(removed=True, fate='GONE', disturbed=[], appeared=[], remaining=2)
    if which == 'merged':
        assert fate == dict(box='STAYED', top='MERGED', side='STAYED') and h['heir'][L['top'] - 1] == N['box'] and h['absorbed'][N['box'] - 1] == 2
    if which == 'cut':
        assert fate == dict(box='MOVED', top='STAYED', side='STAYED') and h['pieces'][L['box'] - 1] == 2
        assert h['origin_name'][N['half_hi'] - 1] == 'FRAGMENT' and h['summary']['fragments'] == 1 and h['heir'][L['box'] - 1] == N['half_lo']


@pytest.mark.gpu
def test_two_results_of_one_operator_are_refused():
    vp, trk = parts.VolumeParts(), track.PartTrack()
    h = torch.from_numpy(np.stack([pref.d2_free(tgr.mask_volume(tgr.ball(12, (5, 5, 5), 3))[None])[0]] * 2)).to('cuda:0')
    first = vp(h[:1], max_parts=4)
    second = vp(h[1:], max_parts=4)
    with pytest.raises(ValueError, match='share the storage of `labels`'):
        trk.of_parts(first, second)
    kept = dict(first, labels=first['labels'].clone(), count=first['count'].clone())
    res = trk.of_parts(kept, second, share=0.4)
    assert res['summary'][0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and res['share'] == 0.4 and res['max_parts'] == 4


@pytest.mark.gpu
def test_mis_shaped_arguments_are_refused_and_write_nothing():
    """Every ValueError of the two wrappers and of track_of_plans that stands between a mis-shaped argument and a kernel that indexes
    by B, R and P, each with its text; the operators' output tensors of that shape hold afterwards what the last good call wrote."""
    P, R, dev = 4, 8, 'cuda:0'
    over, trk = track.PartOverlap(), track.PartTrack()
    pair = np.stack(blocky_pair(R, 3, P))
    res = over(pair, pair[::-1].copy(), max_parts=P)
    cb, ca = torch.tensor([P, 2], dtype=torch.int32, device=dev), torch.tensor([3, P], dtype=torch.int32, device=dev)
    out = trk(res, cb, ca)
    torch.cuda.synchronize()
    kept = {k: out[k].clone() for k in (*KEYS, 'table', 'beyond')}
    refused = lambda text: pytest.raises(ValueError, match=re.escape(text))
    # PartOverlap: the two volumes differ in B, in R
    for after in (pair[:1], np.zeros((2, R - 1, R - 1, R - 1), i32), np.zeros((3, R, R, R), i32), np.zeros((R + 1,) * 3, i32)):
        with refused(f'before and after must have the same shape, got (2, 8, 8, 8) and {after.shape}'):
            over(pair, after, max_parts=P)
    with refused('labels must be [B,R,R,R], got (2, 8, 8, 7)'):
        over(pair, pair[..., :7], max_parts=P)
    # PartTrack: the table is not a contiguous square int32 device tensor [B,P+1,P+1]
    table = res['table']
    tables = (table.float(), table.long(), table.transpose(1, 2), table[:, :, :P].contiguous(), table[:, :P].contiguous(), table[0], table.cpu(),
              table.cpu().numpy(), table[:, :1, :1].contiguous())
    for bad in tables:
        with refused('overlap must hold PartOverlap\'s contiguous int32 device tensor `table` [B,P+1,P+1]'):
            trk(dict(res, table=bad), cb, ca)
    with refused('track max_parts must be an integer in 1..256, got 257'):
        trk(dict(table=torch.zeros(2, 258, 258, dtype=torch.int32, device=dev)), cb, ca)
    # PartTrack: a count of the wrong length, dtype, device, layout
    counts = (cb[:1], torch.cat([cb, cb]), cb.long(), cb.float(), cb.cpu(), cb.cpu().numpy(), torch.stack([cb, cb], 1)[:, 0], cb[None], [P, 2])
    for bad in counts:
        with refused('count_before must be a contiguous int32 device tensor [2]'):
            trk(res, bad, ca)
        with refused('count_after must be a contiguous int32 device tensor [2]'):
            trk(res, cb, bad)
    # track_of_plans: one scene each
    two = np.stack([tgr.mask_volume(tgr.ball(R, (4, 4, 4), 2))] * 2)
    for before, after in ((two, two[:1]), (two[:1], two), (two, two)):
        with refused('track_of_plans takes the volumes of one scene, got 2'):
            track.track_of_plans(before, after, voxel_size=VOXEL)
    torch.cuda.synchronize()
    again = trk._out[(2, P)]
    assert again['heir'] is out['heir'] and over._out[(2, P)]['table'] is table
    for k, v in kept.items():
        same(('after the refusals', k), out[k].cpu().numpy(), v.cpu().numpy())


@pytest.mark.gpu
def test_one_captured_graph_from_two_volumes_to_the_summary():
    """VolumeDistance and VolumeParts on each volume, PartOverlap and PartTrack captured once on one stream, replayed after both input
    volumes changed, and twice on the same input: the bits of the statement at every replay."""
    R, dev, scale, M_ = 17, 'cuda:0', 0.02, 32

    def blobs(seed):
        r = np.random.default_rng(seed)
        return np.stack([tgr.mask_volume(functools.reduce(np.logical_or, [tgr.ball(R, r.uniform(3, R - 4, 3), r.uniform(2.0, 4.5)) for _ in range(5)])) for _ in range(2)])

    def nudged(vol, seed):
        """The same blobs, rolled by a voxel in one scene and with one corner cleared in the other."""
        out = vol.copy()
        out[0] = np.roll(out[0], 1, axis=seed % 3)
        out[1, :R // 2, :R // 2] = 1.0
        return out

    firsts = [blobs(s) for s in (1, 2, 3)]
    seconds = [nudged(v, s) for s, v in enumerate(firsts)]
    va, vb = torch.from_numpy(firsts[0]).to(dev), torch.from_numpy(seconds[0]).to(dev)
    kw = dict(connectivity=26, max_parts=M_, neck=0.8)

    def run(d1, d2, p1, p2, t):
        ra = p1(d1(va, scale=scale, z_min=1)['d2_free'], **kw)
        rb = p2(d2(vb, scale=scale, z_min=1)['d2_free'], **kw)
        return ra, rb, t.of_parts(ra, rb)

    ops = distance.VolumeDistance(), distance.VolumeDistance(), parts.VolumeParts(), parts.VolumeParts(), track.PartTrack()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*ops)                                                              # sizes the workspaces and the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ra, rb, res = run(*ops)
    first, kept = None, 0
    for n in (1, 2, 2):
        va.copy_(torch.from_numpy(firsts[n]).to(dev))
        vb.copy_(torch.from_numpy(seconds[n]).to(dev))
        for k in (*KEYS, 'table', 'beyond'):
            res[k].view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        wa, wb = (pref.parts(pref.d2_free(v, z_min=1), **kw) for v in (firsts[n], seconds[n]))
        assert np.array_equal(ra['labels'].cpu().numpy(), wa['labels']) and np.array_equal(rb['labels'].cpu().numpy(), wb['labels'])
        bits = {}
        for b in range(2):
            w = tref.track_of_labels(wa['labels'][b], wb['labels'][b], wa['count'][b], wb['count'][b], M_)
            for k in (*KEYS, 'table', 'beyond'):
                same(('replay', n, b, k), res[k][b].cpu().numpy(), w[k])
                bits[b, k] = res[k][b].cpu().numpy()
            kept += int(w['summary'][2] + w['summary'][3])
        if n == 2:
            if first is None:
                first = bits
            else:
                assert all(np.array_equal(first[k], bits[k]) for k in bits), 'the same graph on the same input: the same bits'
    assert kept > 2, 'hardly a part was followed'


@pytest.mark.gpu
def test_track_of_plans():
    mb, ma, _, at, old, new = pile_volumes('taken')
    vb, va = tgr.mask_volume(mb), tgr.mask_volume(ma)
    pb, pa, h = track.track_of_plans(vb, va, voxel_size=VOXEL, max_parts=8, z_min=3)
    wb, wa = (pref.parts(pref.d2_free(v[None], z_min=3), max_parts=8) for v in (vb, va))
    assert np.array_equal(pb['labels'], wb['labels'][0]) and np.array_equal(pa['labels'], wa['labels'][0]) and (pb['count'], pa['count']) == (3, 2)
    w = host_track(tref.track_of_labels(wb['labels'][0], wa['labels'][0], 3, 2, 8), 3, 2)
    assert list(h) == list(w)
    for k in w:
        if isinstance(w[k], np.ndarray):
            same(('plans', k), h[k], w[k])
        else:
            assert h[k] == w[k], k
    top = int(pb['labels'][TOP])
    out = track.track_of_plans(vb, va, taken=top, voxel_size=VOXEL, max_parts=8, z_min=3, stay=0.5)
    assert len(out) == 4 and out[3] == dict(removed=True, fate='GONE', disturbed=[], appeared=[], remaining=2) and out[2]['stay'] == 0.5
    with pytest.raises(_lib.GnrError, match='raise max_parts'):
        track.track_of_plans(vb, va, voxel_size=VOXEL, max_parts=2, z_min=3)
    with pytest.raises(ValueError, match='the two volumes must share a lattice'):
        track.track_of_plans(vb, va[:20, :20, :20], voxel_size=VOXEL, z_min=3)


@pytest.mark.gpu
def test_a_refused_call_writes_nothing():
    B, R, P = 1, 8, 4
    fill = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    sizes = dict(before=4 * R ** 3, after=4 * R ** 3, table=4 * (P + 1) ** 2, beyond=4, count_before=4, count_after=4, summary=32, **{k: 4 * P for k in tref.COLUMNS})
    bufs = {k: fill(v) for k, v in sizes.items()}
    ptr = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    _overlap_refusals(ptr, B=B, R=R, P=P)
    _track_refusals(ptr, B=B, P=P)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == SENTINEL).all()), k
