"""Parts across two plans, on the device (csrc/gnr_track.hip, gnr_part_overlap_fwd and gnr_part_track_fwd): which part of plan t is
which part of plan t+1, and what became of every part.  parts.VolumeParts numbers each volume on its own, in voxel order, so taking
one ball renumbers every part behind it; support.PartSupport predicts what loses its footing, and nothing so far says what did
happen.  The reference reads that off its simulator (check_success, remove_body, remove_and_wait; clutter_removal.py:92-150); on the
real-robot route (planner.plan_real, PlannerSession) the next plan's volume is the only witness of a take.
PartOverlap counts, per pair (old label, new label), the voxels that carry both (`table`, row 0 "was free", column 0 "is free now").
PartTrack derives per old part its `heir` (where most of its voxels are now), per new part its `source` (what it is mostly made of),
each kept only at `share` of the part's size; where the two agree it is the same part, which STAYED when the shared voxels are at
least `stay` of the union and MOVED below that; otherwise an old part is GONE or MERGED into another and a new part is NEW or a
FRAGMENT.  include/gnr.h states the rule; the results are the bits of tests/track_reference.py.
What a caller must know.  The match is by overlap alone: a part that rolls away by more than about its own radius shares too few
voxels with itself, reads GONE next to a NEW part, and is not followed; nothing is matched by shape and nothing turns.  share = 0.5 and
stay = 0.6 are policy, not measurement.  What they mean on synthetic balls, computed with the statement on the CPU (share: the shared
voxels over the ball's; IoU: over the union):
    radius 3 voxels:  shift 1: share 0.764, IoU 0.618;  shift 2: 0.561, 0.390
    radius 5 voxels:  shift 1: 0.843, 0.728;  shift 2: 0.709, 0.549;  shift 3: 0.575, 0.403;  shift 4: share 0.441
    radius 8 voxels:  shift 1: IoU 0.829;  shift 2: 0.688;  shift 3: 0.567
so a part shifted by about one voxel reads STAYED, one shifted by up to about 0.6 of its radius MOVED, and one shifted further GONE
plus a NEW part.  Neither threshold has been run on a network's volumes, whose surface noise between two plans nobody has measured,
which is why both stay keywords, and the integer columns `shared`, `size_before` / `size_after`, `vacated` and `fresh` let a caller
apply their own.  The table is dense: at most 256 parts per scene, and `beyond` says when labels went beyond the rows.
No row of planner.PRODUCTS: like parts, retreat and support this is an operator for after the plan -- track_of_plans runs it on the
volumes of two plans."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .distance import VolumeDistance, checked_scale
from .grasp_post import SOLID_DEFAULTS, DeviceOp, _host, checked_params, checked_solid, labels_batch, picked, split_params, volume_batch
from .objects import PLAN_VOXEL_SIZE
from .parts import PART_DEFAULTS, VolumeParts, part_params, parts_from_rows, parts_rows

TRACK_DEFAULTS = dict(share=0.5, stay=0.6)
OLD_COLUMNS = ('heir', 'shared', 'size_before', 'vacated', 'pieces', 'fate')           # per old part: [B,P] int32
NEW_COLUMNS = ('source', 'size_after', 'fresh', 'absorbed', 'origin')                 # per new part: [B,P] int32
TRACK_COLUMNS = (*OLD_COLUMNS, *NEW_COLUMNS)
SUMMARY_FIELDS = ('nb', 'na', 'stayed', 'moved', 'gone', 'merged', 'new', 'fragments')
FATES = ('STAYED', 'MOVED', 'GONE', 'MERGED')
ORIGINS = ('SAME', 'NEW', 'FRAGMENT')
STAYED, MOVED, GONE, MERGED = range(4)
SAME, NEW, FRAGMENT = range(3)
MAX_PARTS = _lib.GNR_TRACK_MAX_PARTS


def checked_track(share=0.5, stay=0.6):
    """The track's parameters, checked before anything touches the device (the library refuses the same)."""
    for k, v, what in (('share', share, 'the part of a part\'s voxels its heir or source must hold'),
                       ('stay', stay, 'the shared voxels over the union at which the same part has stayed')):
        if isinstance(v, bool) or not (math.isfinite(v) and 0 <= v <= 1):
            raise ValueError(f'track {k} must be finite and in 0..1 ({what}), got {v!r}')
    return dict(share=float(share), stay=float(stay))


def track_params(track, **more):
    """A `track` argument -> None (False / None: not asked for), or the track's parameters (True / {}: share 0.5, stay 0.6).  Unknown
    keys are a TypeError, and every value is checked here, before the device.  more: further keys the caller takes, with their
    defaults."""
    out = checked_params('track', track, {**TRACK_DEFAULTS, **more})
    if out is not None:
        out.update(checked_track(**picked(out, TRACK_DEFAULTS)))
    return out


def checked_rows(max_parts):
    """The parts the table has rows for: an integer in 1..256."""
    if isinstance(max_parts, bool) or int(max_parts) != max_parts or not 1 <= max_parts <= MAX_PARTS:
        raise ValueError(f'track max_parts must be an integer in 1..{MAX_PARTS}, got {max_parts!r}')
    return int(max_parts)


class PartOverlap(DeviceOp):
    """The overlap table of B pairs of label volumes.  The output tensors are kept per (B, max_parts) and written again by the next call
    of that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'part overlap')
        self._out = {}

    def __call__(self, before, after, *, max_parts):
        """before, after [B,R,R,R] int32 (VolumeParts' or VolumeObjects' `labels` of two plans, or any; or one [R,R,R] each), the
        same shape, 2 <= R <= 256: a label < 1 is no part;  max_parts: P, 1..256.
        -> {'table': [B,P+1,P+1] int32 ([..,i,j]: the voxels with old label i and new label j, 0: free; [..,0,0] is 0), 'beyond': [B]
        int32 (the voxels with a label above P)}, with `max_parts` as given.  The tensors are this object's: the next call with the
        same shape writes them again."""
        d = self.device
        P = checked_rows(max_parts)
        before, B, R = labels_batch(before, d)
        after, B2, R2 = labels_batch(after, d)
        if (B, R) != (B2, R2):
            raise ValueError(f'before and after must have the same shape, got {tuple(before.shape)} and {tuple(after.shape)}')
        out = self._out.get((B, P))
        if out is None:
            out = self._out[(B, P)] = {'table': torch.zeros(B, P + 1, P + 1, dtype=torch.int32, device=d), 'beyond': torch.zeros(B, dtype=torch.int32, device=d)}
        p = _lib.GnrOverlapParams(max_parts=P)
        rc = self.L.gnr_part_overlap_fwd(C.byref(p), before.data_ptr(), after.data_ptr(), B, R, out['table'].data_ptr(), out['beyond'].data_ptr(),
                                         self._stream())
        _lib.check(rc, 'gnr_part_overlap_fwd')
        return dict(out, max_parts=P)


class PartTrack(DeviceOp):
    """The fates of the parts of B overlap tables.  The output tensors are kept per (B, max_parts) and written again by the next call of
    that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'part track')
        self._out = {}
        self._overlap = None

    def __call__(self, overlap, count_before, count_after, *, share=0.5, stay=0.6):
        """overlap: a PartOverlap result (`table` [B,P+1,P+1] int32 device tensor);  count_before, count_after [B] int32 device tensors:
        the parts of each scene in the two plans (VolumeParts' `count`; the parts are the labels 1..min(max(count, 0), P));  share in
        [0, 1]: an heir / a source holds at least this share of the part's voxels;  stay in [0, 1]: the same part has stayed when
        the shared voxels are at least this share of the union.
        -> {'heir', 'shared', 'size_before', 'vacated', 'pieces', 'fate' (per old part), 'source', 'size_after', 'fresh', 'absorbed',
        'origin' (per new part): [B,P] int32 (rows beyond the parts: 0, fate and origin -1), 'summary': [B,8] int32 (SUMMARY_FIELDS)},
        and the overlap's `table`, `beyond`, `max_parts` as they came, the two counts, and the two parameters.  The tensors are this
        object's: the next call with the same shape writes them again."""
        d = self.device
        q = checked_track(share, stay)
        table = overlap['table']
        ok = lambda t, dim: torch.is_tensor(t) and t.dtype == torch.int32 and t.device.type == d.type and t.dim() == dim and t.is_contiguous()
        if not ok(table, 3) or table.shape[1] != table.shape[2] or table.shape[1] < 2:
            raise ValueError('overlap must hold PartOverlap\'s contiguous int32 device tensor `table` [B,P+1,P+1]')
        B, P = table.shape[0], table.shape[1] - 1
        checked_rows(P)
        for name, count in (('count_before', count_before), ('count_after', count_after)):
            if not ok(count, 1) or count.shape[0] != B:
                raise ValueError(f'{name} must be a contiguous int32 device tensor [{B}]')
        out = self._out.get((B, P))
        if out is None:
            out = self._out[(B, P)] = {**{k: torch.zeros(B, P, dtype=torch.int32, device=d) for k in TRACK_COLUMNS},
                                       'summary': torch.zeros(B, 8, dtype=torch.int32, device=d)}
        p = _lib.GnrTrackParams(max_parts=P, **q)
        rc = self.L.gnr_part_track_fwd(C.byref(p), table.data_ptr(), count_before.data_ptr(), count_after.data_ptr(), B,
                                       *(out[k].data_ptr() for k in TRACK_COLUMNS), out['summary'].data_ptr(), self._stream())
        _lib.check(rc, 'gnr_part_track_fwd')
        res = dict(out)
        res.update({k: overlap[k] for k in ('table', 'beyond') if k in overlap}, max_parts=P, count_before=count_before, count_after=count_after, **q)
        return res

    def of_parts(self, res_before, res_after, **kw):
        """... of two VolumeParts / VolumeObjects results as they are: PartOverlap on their labels with min(their max_parts, 256) rows
        (this object keeps the operator), then the fates with their counts.  A VolumeParts object writes its own output tensors again
        on the next call of the same shape: the two results must come from two operator objects, or the first one's `labels` and
        `count` must be cloned -- two results that share the storage of `labels` are refused."""
        la, lb = res_before['labels'], res_after['labels']
        if torch.is_tensor(la) and torch.is_tensor(lb) and la.untyped_storage().data_ptr() == lb.untyped_storage().data_ptr():
            raise ValueError('the two results share the storage of `labels`: an operator object writes its outputs again on the next call of '
                             'the same shape -- run the two plans through two VolumeParts objects, or clone the first one\'s `labels` and `count`')
        if self._overlap is None:
            self._overlap = PartOverlap(self.device)
        rows = lambda r: int(r['max_parts'] if 'max_parts' in r else r['max_objects'])
        P = min(rows(res_before), rows(res_after), MAX_PARTS)
        return self(self._overlap(la, lb, max_parts=P), res_before['count'], res_after['count'], **kw)


def track_rows(res, b, nb, na):
    """The device rows of scene b of a PartTrack result, given the scene's two counts: the first min(nb, max_parts) rows of every
    column of the old parts, the first min(na, max_parts) of the new parts', that corner of the table, the summary, `beyond` and the
    counts."""
    P = res['heir'].shape[1]
    mb, ma = max(0, min(int(nb), P)), max(0, min(int(na), P))
    out = {k: res[k][b, :mb] for k in OLD_COLUMNS}
    out.update({k: res[k][b, :ma] for k in NEW_COLUMNS})
    out.update(table=res['table'][b, :mb + 1, :ma + 1], summary=res['summary'][b], beyond=res['beyond'][b:b + 1],
               count_before=res['count_before'][b:b + 1], count_after=res['count_after'][b:b + 1])
    return out


def track_from_rows(rows, share=0.5, stay=0.6, max_parts=None):
    """track_rows on the host (numpy) -> every column as an int32 array ([nb] for the old parts, [na] for the new), `fate_name` and
    `origin_name` (lists of FATES / ORIGINS names), `table` [nb+1,na+1] int32, `summary` (a dict over SUMMARY_FIELDS), `nb`, `na`, and
    the two parameters.  max_parts: the rows the table had (for the text of the error).
    Raises when labels went beyond the rows of the table, or when a plan has more parts than rows."""
    q = checked_track(share, stay)
    one = lambda k: int(np.asarray(rows[k]).reshape(-1)[0])
    held_b, held_a = len(np.asarray(rows['heir'])), len(np.asarray(rows['source']))
    full = max_parts is not None and int(max_parts) >= MAX_PARTS
    how = f'more than {MAX_PARTS} parts: the overlap table is dense and does not answer a heap' if full else 'raise max_parts'
    for what, count, held in (('before', one('count_before'), held_b), ('after', one('count_after'), held_a)):
        if count > held:
            raise _lib.GnrError(f'{count} parts {what} but the track tables hold {held}: {how}')
    if one('beyond') > 0:
        raise _lib.GnrError(f'{one("beyond")} voxels carry labels beyond the rows of the overlap table: {how}')
    out = {k: np.array(np.asarray(rows[k], np.int32).reshape(-1)) for k in TRACK_COLUMNS}
    out['fate_name'] = [FATES[f] for f in out['fate']]
    out['origin_name'] = [ORIGINS[o] for o in out['origin']]
    out['table'] = np.array(np.asarray(rows['table'], np.int32).reshape(held_b + 1, held_a + 1))
    out['summary'] = dict(zip(SUMMARY_FIELDS, (int(v) for v in np.asarray(rows['summary']).reshape(-1))))
    out.update(nb=held_b, na=held_a, **q)
    return out


def take_verdict(track, part, support=None):
    """What the second plan says of taking `part` (a label of the first plan): track_from_rows' dict -> {'removed': the part is GONE,
    'fate': its fate's name, 'disturbed': the labels of the other old parts that have not STAYED, 'appeared': the labels of the NEW parts
    of the second plan, 'remaining': the parts of the second plan}.  support: support.support_from_rows' dict of the first plan; then
    also 'predicted': {'orphans', 'carried': the labels the support graph says lose every footing with `part` / rest on it,
    transitively} and 'not_stayed': {'orphans', 'carried': those of them that have not STAYED} -- the prediction next to the
    observation."""
    nb = len(track['fate'])
    if isinstance(part, bool) or int(part) != part or not 1 <= part <= nb:
        raise ValueError(f'part must be a label of the first plan, 1..{nb}, got {part!r}')
    part = int(part)
    fate = np.asarray(track['fate'])
    out = dict(removed=bool(fate[part - 1] == GONE), fate=FATES[int(fate[part - 1])],
               disturbed=[int(a) + 1 for a in np.flatnonzero(fate != STAYED) if a + 1 != part],
               appeared=[int(b) + 1 for b in np.flatnonzero(np.asarray(track['origin']) == NEW)], remaining=int(track['na']))
    if support is not None:
        rests = np.asarray(support['rests_on'], bool)
        if rests.shape != (nb, nb):
            raise ValueError(f'support must be the first plan\'s: its rests_on is {rests.shape}, the track has {nb} old parts')
        on_floor = np.asarray(support['on_floor'], bool)
        carried, edge = set(), {part - 1}
        while edge:                                                            # everything that rests on it, transitively
            edge = {int(c) for a in edge for c in np.flatnonzero(rests[:, a])} - carried - {part - 1}
            carried |= edge
        gone = {part - 1}
        for _ in range(nb):                                                    # include/gnr.h's rounds of `orphans`
            more = {c for c in range(nb) if c not in gone and not on_floor[c] and rests[c].any() and set(np.flatnonzero(rests[c])) <= gone}
            if not more:
                break
            gone |= more
        pred = dict(orphans=sorted(c + 1 for c in gone - {part - 1}), carried=sorted(c + 1 for c in carried))
        out['predicted'] = pred
        out['not_stayed'] = {k: [a for a in v if fate[a - 1] != STAYED] for k, v in pred.items()}
    return out


def track_of_plans(tsdf_before, tsdf_after, *, taken=None, voxel_size=PLAN_VOXEL_SIZE, origin=(0.0, 0.0, 0.0), device='cuda:0', **params):
    """The parts of two consecutive plans and what became of them: tsdf_before, tsdf_after as plan_real / plan / plan_depth return
    their volume (one scene each, the same lattice).  params: the solid rule's keys (SOLID_DEFAULTS -- z_min must cut the table slab),
    PART_DEFAULTS' and TRACK_DEFAULTS'.  VolumeDistance then VolumeParts on each volume, with two operator objects (their outputs live
    side by side), PartOverlap on the two label volumes, PartTrack on its table.
    -> (parts_before, parts_after, track): parts.parts_from_rows' dicts with `labels` [R,R,R] int32, and track_from_rows' dict;
    with taken (a label of the first plan, the part the hand closed on): (parts_before, parts_after, track, take_verdict(track, taken))."""
    params = split_params('track', params, SOLID_DEFAULTS, PART_DEFAULTS, TRACK_DEFAULTS)
    solid = checked_solid('track', **picked(params, SOLID_DEFAULTS))
    q = part_params(picked(params, PART_DEFAULTS))
    tp = track_params(picked(params, TRACK_DEFAULTS))
    scale = checked_scale(voxel_size)
    d = torch.device(device)
    results, shapes = [], []
    for vol in (tsdf_before, tsdf_after):
        vol, B, R = volume_batch(vol, d)
        if B != 1:
            raise ValueError(f'track_of_plans takes the volumes of one scene, got {B}')
        shapes.append(R)
        results.append(VolumeParts(d)(VolumeDistance(d)(vol, scale=scale, **solid)['d2_free'], **q))
    if shapes[0] != shapes[1]:
        raise ValueError(f'the two volumes must share a lattice, got R = {shapes[0]} and {shapes[1]}')
    tres = PartTrack(d).of_parts(*results, **tp)
    found = [int(r['count'][0].item()) for r in results]
    parts = []
    for r, n in zip(results, found):
        parts.append(parts_from_rows(_host(parts_rows(r, 0, n)), scale, origin))
        parts[-1]['labels'] = r['labels'][0].cpu().numpy()
    track = track_from_rows(_host(track_rows(tres, 0, *found)), max_parts=tres['max_parts'], **tp)
    return (*parts, track) if taken is None else (*parts, track, take_verdict(track, taken))
