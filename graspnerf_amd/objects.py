"""Objects of the plan's volume, on the device (csrc/gnr_objects.hip, gnr_volume_objects_fwd): connected-component labelling of the
solid voxels with ndimage.label's numbering, per component its size, box and centre, and a copy of the volume with the small
components -- a NeRF volume's floaters -- set to free, which every other operator (HandClearance, FingerClosure, MeshExtractor,
SurfaceExtractor, VolumeRaycaster) takes as it is.  The reference asks its simulator (`while sim.num_objects > 0`,
src/gd/experiments/clutter_removal.py:92; `object_count` per round); on a real robot the only geometry is the volume.
GraspObjects (gnr_grasp_objects_fwd, csrc/gnr_hand.hip's third kernel) says which object each ranked grasp would close on, and whether
it pinches two at once.  include/gnr.h states both; the results are the bits of tests/objects_reference.py (scipy.ndimage.label).
Two things a caller must know.  Objects that stand on the table are one component with the table and with each other through it:
`z_min` must cut the table slab (voxels with k < z_min are not solid) for them to separate.  And objects that touch each other are
one component, whatever the connectivity: the labelling knows solid voxels and nothing of shapes (parts.VolumeParts splits such a
component at its necks, with this module's numbering and rows).
No row of planner.PRODUCTS yet: objects_of_plan runs both operators on what plan_real / plan / plan_depth return."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .grasp_post import (SOLID_DEFAULTS, DeviceOp, _host, checked_params, checked_solid, labels_batch, picked, solid_fields, split_params,
                         volume_batch)
from .hand import HAND_DEFAULTS, _GraspRows, checked_hand, plan_rows

OBJECT_DEFAULTS = dict(SOLID_DEFAULTS, connectivity=6, max_objects=1024, min_voxels=1, cleaned=False)
FREE_VALUE = 1.0                                                               # the volume's upper clip: what `cleaned` holds where a component went
OBJECT_ROW_TYPES = dict(voxels=((), torch.int32), bbox=((6,), torch.int32), sums=((3,), torch.int64))      # per statistics row: shape, dtype
GRASP_OBJECT_ROW_TYPES = dict(object=((), torch.int32), votes=((), torch.int32), distinct=((), torch.int32), inside=((), torch.int32))
GRASP_OBJECT_ROWS = tuple(GRASP_OBJECT_ROW_TYPES)
# planner.REAL_VOXEL_SIZE (grasp_utils.py:146), a second literal: planner imports planner_session, whose product table is to import
# this module for the objects' rows, so importing planner here would close a cycle
PLAN_VOXEL_SIZE = 0.3 / 40


def checked_objects(level=0.0, lower=None, z_min=0, connectivity=6, max_objects=1024, min_voxels=1, cleaned=False):
    """The labelling's parameters, checked before anything touches the device (the library refuses the same; z_min <= R is the
    library's, which knows R)."""
    solid = checked_solid('objects', level, lower, z_min)
    if isinstance(max_objects, bool) or int(max_objects) != max_objects or max_objects < 1:
        raise ValueError(f'objects max_objects must be an integer >= 1, got {max_objects!r}')
    if isinstance(min_voxels, bool) or int(min_voxels) != min_voxels:
        raise ValueError(f'objects min_voxels must be an integer, got {min_voxels!r}')
    if connectivity not in (6, 18, 26) or isinstance(connectivity, bool):
        raise ValueError(f'objects connectivity must be 6, 18 or 26, got {connectivity!r}')
    if not isinstance(cleaned, bool):
        raise ValueError(f'objects cleaned must be True or False, got {cleaned!r}')
    return dict(solid, connectivity=int(connectivity), max_objects=int(max_objects), min_voxels=int(min_voxels), cleaned=cleaned)


def object_params(objects, **more):
    """An `objects` argument -> None (False / None: not asked for), or the labelling's parameters (True / {}: solid below 0, no lower
    bound, no table cut, 6-connected, 1 024 statistics rows, nothing removed, no cleaned copy).  Unknown keys are a TypeError, and every
    value is checked here, before the device.  more: further keys the caller takes, with their defaults."""
    out = checked_params('objects', objects, {**OBJECT_DEFAULTS, **more})
    if out is not None:
        out.update(checked_objects(**picked(out, OBJECT_DEFAULTS)))
    return out


class VolumeObjects(DeviceOp):
    """The connected components of the solid voxels of B volumes.  The output tensors are kept per shape and written again by the next
    call of that shape, and the workspace only grows, so the addresses are stable for a captured graph once a warm-up call has run."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'volume objects')
        self._out = {}

    def __call__(self, vol, level=0.0, lower=None, z_min=0, connectivity=6, max_objects=1024, min_voxels=1, cleaned=False):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]), 2 <= R <= 256;  solid: lower < v < level and k >= z_min (lower None: no lower
        bound; a NaN is not solid);  connectivity 6, 18 or 26;  max_objects: rows of the statistics;  min_voxels, cleaned: with
        cleaned=True also a copy of the volume with every component of fewer than min_voxels voxels set to FREE_VALUE.
        -> {'labels': [B,R,R,R] int32 (0: not solid; else ndimage.label's number), 'count': [B] int32 (the true number of components,
        also beyond max_objects), 'voxels': [B,max_objects] int32, 'bbox': [B,max_objects,6] int32 (lo i, j, k, hi i, j, k, inclusive;
        (R,R,R,-1,-1,-1): no such object), 'sums': [B,max_objects,3] int64 (of i, j, k), 'status': [1] int32 (0, or
        _lib.GNR_OBJECTS_STATUS_BOUND: a loop ran into its bound and the results are not to be used), 'cleaned': [B,R,R,R] float32 when
        asked for}, with `max_objects` and `min_voxels` as given.  The tensors are this object's: the next call with the same shape
        writes them again."""
        d = self.device
        q = checked_objects(level, lower, z_min, connectivity, max_objects, min_voxels, cleaned)
        vol, B, R = volume_batch(vol, d)
        solid = solid_fields('objects', q, R, z_min)
        M = q['max_objects']
        out = self._out.get((B, R, M))
        if out is None:
            out = self._out[(B, R, M)] = {'labels': torch.zeros(B, R, R, R, dtype=torch.int32, device=d), 'count': torch.zeros(B, dtype=torch.int32, device=d),
                                          **{k: torch.zeros(B, M, *tail, dtype=dtype, device=d) for k, (tail, dtype) in OBJECT_ROW_TYPES.items()}}
        if q['cleaned'] and 'cleaned' not in out:
            out['cleaned'] = torch.zeros(B, R, R, R, dtype=torch.float32, device=d)
        p = _lib.GnrObjectsParams(**solid, connectivity=q['connectivity'], max_objects=M, min_voxels=q['min_voxels'], free_value=FREE_VALUE)
        ws, ws_bytes = self._workspace(self.L.gnr_volume_objects_workspace_bytes(B, R))
        rc = self.L.gnr_volume_objects_fwd(C.byref(p), vol.data_ptr(), B, R, out['labels'].data_ptr(), out['count'].data_ptr(),
                                           out['voxels'].data_ptr(), out['bbox'].data_ptr(), out['sums'].data_ptr(),
                                           out['cleaned'].data_ptr() if q['cleaned'] else None, ws, ws_bytes, self._stream())
        _lib.check(rc, 'gnr_volume_objects_fwd')
        res = {k: v for k, v in out.items() if k != 'cleaned' or q['cleaned']}
        res.update(status=self._ws[:4].view(torch.int32), max_objects=M, min_voxels=q['min_voxels'])
        return res


class GraspObjects(_GraspRows):
    """Which object each of the rows of grasps of B label volumes would close on (csrc/gnr_hand.hip, gnr_grasp_objects_fwd)."""
    NOUN, ROW_TYPES = 'grasp objects', GRASP_OBJECT_ROW_TYPES
    _batch = staticmethod(labels_batch)

    def __call__(self, labels, pos, quat, width, count, *, scale, top_k=None, height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05,
                 opening=None, spacing=0.5, approach=0.05):
        """labels [B,R,R,R] int32 (VolumeObjects' `labels`);  pos, quat, width, count, scale, top_k and the hand's keywords:
        HandClearance.__call__'s (finger_width, tail_length and approach are checked and not used).  The samples of the closing region
        between the pads -- x over the hand's height, y over its opening, z over its depth, at most `spacing` voxels apart -- vote for
        the label at their nearest voxel.
        -> {'object': [B,max_n] int32 (the label with the most votes, of several the smallest; 0: the hand closes on nothing), 'votes':
        [B,max_n] int32 (that label's), 'distinct': [B,max_n] int32 (the different labels voted for: 2 and more, the grasp pinches
        several objects), 'inside': [B,max_n] int32 (the samples inside the volume)}; rows beyond min(count, top_k, max_n) keep what
        they held.  The tensors are this object's."""
        p, labels, pos, quat, width, B, R, n, out = self._checked(labels, pos, quat, width, count, scale, top_k, height, finger_width, tail_length,
                                                                  depth, opening, spacing, approach)
        rc = self.L.gnr_grasp_objects_fwd(C.byref(p), labels.data_ptr(), pos.data_ptr(), quat.data_ptr(), width.data_ptr(), count.data_ptr(),
                                          count.numel() // B, B, R, n, int(top_k or 0), *(t.data_ptr() for t in out), self._stream())
        _lib.check(rc, 'gnr_grasp_objects_fwd')
        return dict(zip(GRASP_OBJECT_ROWS, out))


def objects_rows(res, b, n):
    """The device rows of scene b of a VolumeObjects result, given its count n: the first min(n, max_objects) statistics rows, the count
    and the status word."""
    m = min(int(n), res['voxels'].shape[1])
    return {'count': res['count'][b:b + 1], 'status': res['status'], **{k: res[k][b, :m] for k in OBJECT_ROW_TYPES}}


def objects_from_rows(rows, scale, origin=(0.0, 0.0, 0.0), min_voxels=1):
    """objects_rows on the host (numpy) -> `count` (int), `voxels` [n] int32, `bbox_lo` / `bbox_hi` [n,3] int32 (inclusive voxel
    indices), `centroid` [n,3] float64 metres = origin + (sums / voxels) * scale -- the division first, in float64 (both integers are
    exact there), then the product, then the sum --, `extent` [n,3] float64 metres = (bbox_hi - bbox_lo + 1) * scale, `top` [n] float64 =
    origin_z + bbox_hi_k * scale (the highest voxel's value sits there), `kept` [n] bool = voxels >= min_voxels (what `cleaned` keeps).
    Raises when the scene has more objects than statistics rows, or when the labelling reported that a loop ran into its bound."""
    count, voxels = int(np.asarray(rows['count']).reshape(-1)[0]), np.asarray(rows['voxels'])
    if 'status' in rows and int(np.asarray(rows['status']).reshape(-1)[0]) != 0:
        raise _lib.GnrError('the labelling ran into the bound of one of its loops (GNR_OBJECTS_STATUS_BOUND): its results are not to be used')
    if count > len(voxels):
        raise _lib.GnrError(f'{count} objects but the buffers hold {len(voxels)}: raise max_objects')
    voxels = voxels[:count]                                                    # (rows behind the count are empty)
    bbox, sums = np.asarray(rows['bbox']).reshape(-1, 6)[:count], np.asarray(rows['sums']).reshape(-1, 3)[:count]
    origin, scale = np.asarray(origin, np.float64), np.float64(scale)
    lo, hi = bbox[:, :3].copy(), bbox[:, 3:].copy()
    return {'count': count, 'voxels': voxels.copy(), 'bbox_lo': lo, 'bbox_hi': hi,
            'centroid': origin + (sums.astype(np.float64) / voxels.astype(np.float64)[:, None]) * scale,
            'extent': (hi - lo + 1).astype(np.float64) * scale, 'top': origin[2] + hi[:, 2].astype(np.float64) * scale,
            'kept': voxels >= int(min_voxels)}


def grasp_objects_rows(res, b, n):
    """The device rows of scene b of a GraspObjects result, given the number of grasps n the selection stored."""
    return {k: res[k][b, :n] for k in GRASP_OBJECT_ROWS}


def grasp_objects_from_rows(rows):
    """grasp_objects_rows on the host (numpy) -> the columns of the grasps: `object` [n] int32 (the label the hand closes on, 0: none),
    `object_votes` [n] int32, `objects_in_hand` [n] int32 (2 and more: the grasp pinches several), `object_samples` [n] int32."""
    return {'object': np.array(rows['object']), 'object_votes': np.array(rows['votes']), 'objects_in_hand': np.array(rows['distinct']),
            'object_samples': np.array(rows['inside'])}


def best_per_object(object_column):
    """The `object` column of ranked grasps -> {label: the index of its first row}: per object with a grasp, its best-ranked one (the
    rows are in the order of the ranking); label 0, a hand that closes on nothing, is left out."""
    col = np.asarray(object_column).reshape(-1)
    labels, first = np.unique(col, return_index=True)
    return {int(l): int(i) for l, i in zip(labels, first) if l > 0}


def objects_of_plan(tsdf_vol, grasps, *, voxel_size=PLAN_VOXEL_SIZE, origin=(0.0, 0.0, 0.0), device='cuda:0', **params):
    """The objects of a plan: tsdf_vol and the grasps dict as plan_real / plan / plan_depth return them (one scene; grasps_from_selection's
    conventions: `index` the voxel of each grasp, `quat` (x, y, z, w), `width` in metres -- back to voxels by / voxel_size in float32,
    the selection's own format; `pos` = index * voxel_size is not read).  params: OBJECT_DEFAULTS' keys and the hand's (HAND_DEFAULTS);
    origin: the metres of voxel (0,0,0)'s value in the frame the caller wants the centres in (the grasps' own: 0).
    -> (objects, columns): objects_from_rows' dict with `labels` [R,R,R] int32 (and `cleaned` [R,R,R] float32 when asked for), and
    grasp_objects_from_rows' columns, in the order of the grasps."""
    params = split_params('objects', params, OBJECT_DEFAULTS, HAND_DEFAULTS)
    q = object_params(picked(params, OBJECT_DEFAULTS))
    hand = picked(params, HAND_DEFAULTS)
    checked_hand(**hand)
    d = torch.device(device)
    vol, B, R = volume_batch(tsdf_vol, d)
    if B != 1:
        raise ValueError(f'objects_of_plan takes the volume of one scene, got {B}')
    res = VolumeObjects(d)(vol, **q)
    pos, qt, wd, count, n = plan_rows(grasps, voxel_size, d)
    gres = GraspObjects(d)(res['labels'], pos, qt, wd, count, scale=float(voxel_size), **hand)
    objects = objects_from_rows(_host(objects_rows(res, 0, int(res['count'][0].item()))), float(voxel_size), origin, q['min_voxels'])
    objects['labels'] = res['labels'][0].cpu().numpy()
    if q['cleaned']:
        objects['cleaned'] = res['cleaned'][0].cpu().numpy()
    return objects, grasp_objects_from_rows(_host(grasp_objects_rows(gres, 0, n)))
