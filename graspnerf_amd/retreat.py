"""Retreat of the ranked grasps, on the device (csrc/gnr_retreat.hip, gnr_grasp_retreat_fwd): whether the part a grasp holds comes out
of the pile.  ClutterRemovalSim.execute_grasp (gd/simulation.py:369-422) has four steps; hand.HandClearance answers the way in,
hand.FingerClosure the closing of the fingers and check_success, objects.GraspObjects what the hand closes on, and this module the
last: after `gripper.move(0.0)` the simulator moves the hand 0.1 m back along its own z, or, when the approach is more than 60 degrees
off straight down, lifts it 0.1 m along world +z (:378-386, 406), and only then asks check_success.  In a pile that is where a grasp
fails: the hand fits and the fingers hold, but the held object lies under another one.
Per grasp the voxels of the held part (parts.VolumeParts' or objects.VolumeObjects' label, GraspObjects' `object`) move along the
retreat by integer offsets, at most `step` voxels between tested positions; a step is blocked when more than `tolerance` of them land
inside another part.  include/gnr.h states the rule; the results are the bits of tests/retreat_reference.py.
What a caller must know.  The part moves as a rigid set of voxels without rotation; a position outside the lattice is free (the
workspace ends there); parts that would be pushed aside count as blocking; the closed hand's own sweep on a side grasp's lift is not
tested (for a top grasp the way out is the way in, HandClearance's approach_clearance); what rests on the held part and what loses
its footing once it is gone is support.PartSupport's answer, how the pile then moves is nobody's.  Labels of touching parts meet without a gap, and a split is never perfectly along the contact: a few voxels
of overlap on the first steps are the split's own noise, which is what `tolerance` is for.
No row of planner_session.PRODUCTS yet: retreat_of_plan runs the operators on what plan_real / plan / plan_depth return."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .distance import VolumeDistance, checked_scale
from .grasp_post import SOLID_DEFAULTS, DeviceOp, _host, checked_params, checked_solid, labels_batch, picked, split_params, volume_batch
from .hand import HAND_DEFAULTS, checked_hand, plan_rows
from .objects import PLAN_VOXEL_SIZE, GraspObjects, grasp_objects_rows
from .parts import PART_DEFAULTS, VolumeParts, grasp_parts_from_rows, part_params, parts_from_rows, parts_rows

RETREAT_DEFAULTS = dict(retreat=0.1, step=0.5, side_cos=0.5, tolerance=0)      # execute_grasp's 0.1 m; cos(pi / 3) (simulation.py:378)
RETREAT_ROW_TYPES = dict(blocked_step=((), torch.int32), blocker=((), torch.int32), overlap=((), torch.int32), moved=((), torch.int32),
                         side=((), torch.int32), travel=((), torch.float32))                               # per grasp: shape, dtype
RETREAT_ROWS = tuple(RETREAT_ROW_TYPES)


def checked_retreat(retreat=0.1, step=0.5, side_cos=0.5, tolerance=0):
    """The retreat's parameters, checked before anything touches the device (the library refuses the same; the number of steps needs
    the scale: retreat_steps)."""
    for k, v in (('retreat', retreat), ('step', step)):
        if isinstance(v, bool) or not (math.isfinite(v) and v > 0):
            raise ValueError(f'retreat {k} must be finite and > 0, got {v!r}')
    if isinstance(side_cos, bool) or not math.isfinite(side_cos):
        raise ValueError(f'retreat side_cos must be finite, got {side_cos!r}')
    if isinstance(tolerance, bool) or int(tolerance) != tolerance or tolerance < 0:
        raise ValueError(f'retreat tolerance must be an integer >= 0, got {tolerance!r}')
    return dict(retreat=float(retreat), step=float(step), side_cos=float(side_cos), tolerance=int(tolerance))


def retreat_params(retreat, **more):
    """A `retreat` argument -> None (False / None: not asked for), or the retreat's parameters (True / {}: 0.1 m in steps of half a
    voxel at most, a lift along world +z beyond 60 degrees off straight down, no voxel of overlap tolerated).  Unknown keys are a
    TypeError, and every value is checked here, before the device.  more: further keys the caller takes, with their defaults."""
    out = checked_params('retreat', retreat, {**RETREAT_DEFAULTS, **more})
    if out is not None:
        out.update(checked_retreat(**picked(out, RETREAT_DEFAULTS)))
    return out


def retreat_steps(retreat, step, scale):
    """(T, K, sl) of the statement: the retreat in voxels, the number of tested positions and the voxels between two of them.  Raises
    when K exceeds the library's cap."""
    T = float(retreat) / float(scale)
    ratio = T / float(step)
    K = max(1.0, float(math.ceil(ratio))) if math.isfinite(ratio) else math.inf
    if not K <= _lib.GNR_RETREAT_MAX_STEPS:
        raise ValueError(f'retreat {retreat!r} m in steps of {step!r} voxels of {scale!r} m takes more than {_lib.GNR_RETREAT_MAX_STEPS} steps')
    return T, int(K), T / K


class GraspRetreat(DeviceOp):
    """The retreat of the held part at rows of grasps of B label volumes.  The output tensors are kept per (B, max_n) and written
    again by the next call of that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'grasp retreat')
        self._out = {}

    def __call__(self, labels, bbox, held, quat, count, *, scale, top_k=None, retreat=0.1, step=0.5, side_cos=0.5, tolerance=0):
        """labels [B,R,R,R] int32 (VolumeParts' or VolumeObjects' `labels`; or one [R,R,R]), 2 <= R <= 256;  bbox [B,max_parts,6] int32
        (their `bbox`: lo i, j, k, hi i, j, k inclusive);  held [B,max_n] int32: the label each grasp holds (GraspObjects' `object`;
        below 1 or above max_parts: nothing);  quat [B,max_n,4] float32 (x, y, z, w; as the selection stores it);  count [B] or [B,k]
        int32 device tensor, its first column the rows of each scene;  scale: metres per voxel;  top_k: at most that many rows per
        scene;  retreat: metres the hand moves away;  step: voxels between tested positions at most;  side_cos: a grasp whose approach
        has -a_z below it lifts along world +z (lattice axis 2) instead of moving back along its own z;  tolerance: a step is blocked
        when more than this many moving voxels are inside other parts.
        -> {'blocked_step': [B,max_n] int32 (the first blocked step, 1 .. K; 0: the part comes out), 'blocker': [B,max_n] int32 (the
        label in the way there, 0: none), 'overlap': [B,max_n] int32 (the most voxels inside other parts at any step), 'moved':
        [B,max_n] int32 (the voxels of the held part), 'side': [B,max_n] int32 (1: lifted along world +z), 'travel': [B,max_n] float32
        (metres moved before the first blocked step; `retreat` when free)}; rows beyond min(count, top_k, max_n) keep what they held.
        The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        q = checked_retreat(retreat, step, side_cos, tolerance)
        scale = checked_scale(scale)
        retreat_steps(q['retreat'], q['step'], scale)
        labels, B, R = labels_batch(labels, d)
        bbox = torch.as_tensor(bbox, dtype=torch.int32, device=d).contiguous()
        held = torch.as_tensor(held, dtype=torch.int32, device=d).contiguous()
        quat = torch.as_tensor(quat, dtype=torch.float32, device=d).contiguous()
        if bbox.dim() == 2:
            bbox = bbox[None]
        if held.dim() == 1:
            held, quat = held[None], quat[None]
        if bbox.dim() != 3 or bbox.shape[0] != B or bbox.shape[1] < 1 or bbox.shape[2] != 6:
            raise ValueError(f'bbox must be [{B},max_parts,6], got {tuple(bbox.shape)}')
        n = held.shape[-1]
        if tuple(held.shape) != (B, n) or n < 1 or tuple(quat.shape) != (B, n, 4):
            raise ValueError(f'held must be [{B},max_n] and quat [{B},max_n,4], got {tuple(held.shape)} and {tuple(quat.shape)}')
        if not torch.is_tensor(count) or count.dtype != torch.int32 or count.device != labels.device or count.shape[0] != B or \
                not count.is_contiguous():
            raise ValueError(f'count must be a contiguous int32 device tensor [{B}] or [{B},k]')
        if top_k is not None and int(top_k) < 1:
            raise ValueError(f'top_k must be None or positive, got {top_k!r}')
        out = self._out.get((B, n))
        if out is None:
            out = self._out[(B, n)] = tuple(torch.zeros(B, n, *tail, dtype=dtype, device=d) for tail, dtype in RETREAT_ROW_TYPES.values())
        p = _lib.GnrRetreatParams(scale=scale, max_parts=bbox.shape[1], **q)
        rc = self.L.gnr_grasp_retreat_fwd(C.byref(p), labels.data_ptr(), bbox.data_ptr(), held.data_ptr(), quat.data_ptr(), count.data_ptr(),
                                          count.numel() // B, B, R, n, int(top_k or 0), *(t.data_ptr() for t in out), self._stream())
        _lib.check(rc, 'gnr_grasp_retreat_fwd')
        return dict(zip(RETREAT_ROWS, out))

    def of_parts(self, res, gres, sel_or_rows, *, scale, **kw):
        """... of a VolumeParts / VolumeObjects result and a GraspObjects result on its labels, as they are, at the rows of a
        GraspSelector result (any route's, with its top_k) or of hand.plan_rows' tuple (pos, quat, width, count, n)."""
        if isinstance(sel_or_rows, dict):
            quat, count, top_k = sel_or_rows['quat'], sel_or_rows['count'], sel_or_rows.get('top_k')
        else:
            (_, quat, _, count, _), top_k = sel_or_rows, None
        return self(res['labels'], res['bbox'], gres['object'], quat, count, scale=scale, top_k=kw.pop('top_k', top_k), **kw)


def retreat_rows(res, b, n):
    """The device rows of scene b of a GraspRetreat result, given the number of grasps n the selection stored."""
    return {k: res[k][b, :n] for k in RETREAT_ROWS}


def retreat_from_rows(rows):
    """retreat_rows on the host (numpy) -> the columns a plan adds to its grasps: `retreat_free` [n] bool (no step is blocked),
    `retreat_travel` [n] float32 (metres the part moves before the first blocked step), `retreat_blocker` [n] int32 (the label in the
    way, 0: none), `retreat_overlap` [n] int32 (the most voxels inside other parts at any step), `lifted_voxels` [n] int32 (the voxels
    of the held part; 0: the hand holds nothing the labels know), `side_grasp` [n] bool (lifted along world +z)."""
    return {'retreat_free': np.asarray(rows['blocked_step']) == 0, 'retreat_travel': np.array(rows['travel']),
            'retreat_blocker': np.array(rows['blocker']), 'retreat_overlap': np.array(rows['overlap']),
            'lifted_voxels': np.array(rows['moved']), 'side_grasp': np.asarray(rows['side']) != 0}


def best_free_per_part(columns):
    """The columns of ranked grasps (`part` or `object`, and `retreat_free`) -> {label: the index of its first row that retreats
    free}: which grasp of which part to take now (objects.best_per_object, restricted to the rows with retreat_free); label 0, a hand
    that closes on nothing, is left out, and so is a part none of whose grasps comes out."""
    col = np.asarray(columns['part'] if 'part' in columns else columns['object']).reshape(-1)
    free = np.asarray(columns['retreat_free'], bool).reshape(-1)
    out = {}
    for i in np.flatnonzero(free & (col > 0)):
        out.setdefault(int(col[i]), int(i))
    return out


def retreat_of_plan(tsdf_vol, grasps, *, voxel_size=PLAN_VOXEL_SIZE, origin=(0.0, 0.0, 0.0), device='cuda:0', **params):
    """The retreat of a plan: tsdf_vol and the grasps dict as plan_real / plan / plan_depth return them (one scene;
    parts.parts_of_plan's conventions).  params: the solid rule's keys (SOLID_DEFAULTS -- z_min must cut the table slab, or the table
    is a part that blocks nothing and is never lifted), PART_DEFAULTS', the hand's (HAND_DEFAULTS) and RETREAT_DEFAULTS'.
    VolumeDistance on the volume, VolumeParts on its d2_free, GraspObjects on the parts' labels, GraspRetreat on the part each grasp
    closes on.
    -> (parts, columns): parts_from_rows' dict with `labels` [R,R,R] int32, and grasp_parts_from_rows' columns plus
    retreat_from_rows', in the order of the grasps; best_free_per_part(columns) is the best-ranked grasp of every part that comes
    out."""
    params = split_params('retreat', params, SOLID_DEFAULTS, PART_DEFAULTS, HAND_DEFAULTS, RETREAT_DEFAULTS)
    solid = checked_solid('retreat', **picked(params, SOLID_DEFAULTS))
    q = part_params(picked(params, PART_DEFAULTS))
    hand = picked(params, HAND_DEFAULTS)
    checked_hand(**hand)
    rt = retreat_params(picked(params, RETREAT_DEFAULTS))
    scale = checked_scale(voxel_size)
    retreat_steps(rt['retreat'], rt['step'], scale)
    d = torch.device(device)
    vol, B, R = volume_batch(tsdf_vol, d)
    if B != 1:
        raise ValueError(f'retreat_of_plan takes the volume of one scene, got {B}')
    field = VolumeDistance(d)(vol, scale=scale, **solid)
    res = VolumeParts(d)(field['d2_free'], **q)
    rows = plan_rows(grasps, voxel_size, d)
    pos, qt, wd, count, n = rows
    gres = GraspObjects(d)(res['labels'], pos, qt, wd, count, scale=scale, **hand)
    rres = GraspRetreat(d).of_parts(res, gres, rows, scale=scale, **rt)
    parts = parts_from_rows(_host(parts_rows(res, 0, int(res['count'][0].item()))), scale, origin)
    parts['labels'] = res['labels'][0].cpu().numpy()
    columns = grasp_parts_from_rows(_host(grasp_objects_rows(gres, 0, n)))
    columns.update(retreat_from_rows(_host(retreat_rows(rres, 0, n))))
    return parts, columns
