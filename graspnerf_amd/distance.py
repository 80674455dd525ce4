"""Distance field of the plan's volume, on the device (csrc/gnr_distance.hip, gnr_volume_distance_fwd): the exact Euclidean distance
transform of the solid mask -- per voxel the squared distance to the nearest solid voxel and that voxel, the same to the nearest free
voxel, and `esdf`, the signed metric field made of the two.  The network's volume is a truncated SDF clipped to +-1: metric within a few
voxels of a surface, 1.0 everywhere beyond, so HandClearance on it says whether the hand touches and not by how much it misses.  On
`esdf` the same operator answers in metres, and a motion planner behind this library has its cost field (CHOMP, TrajOpt, voxblox's
ESDF) without the read-back that scipy.ndimage.distance_transform_edt would need.  include/gnr.h states the arithmetic; the results are
the bits of tests/distance_reference.py.  No reference counterpart (the reference asks pybullet).
`solid` is VolumeObjects' rule (lower < v < level and k >= z_min), ties go to the smallest linear index, a scene without a solid (free)
voxel reads 3 R^2 / -1.  Given VolumeObjects' labels, `nearest_label` says which object every voxel is nearest to.
One limit: HandClearance clips at its `free` value 1.0, so margins read from `esdf` are at most 1 m (the largest distance inside the
0.3 m workspace is 0.52 m).
No row of planner.PRODUCTS yet: distance_of_plan runs the operators on what plan_real / plan / plan_depth return."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .grasp_post import (SOLID_DEFAULTS, DeviceOp, _host, checked_params, checked_solid, labels_batch, picked, solid_fields, split_params,
                         volume_batch)
from .hand import HAND_DEFAULTS, HandClearance, checked_hand, hand_from_rows, hand_rows, plan_rows
from .objects import PLAN_VOXEL_SIZE

DISTANCE_DEFAULTS = dict(SOLID_DEFAULTS, surface_offset=0.5, signed=True)
DISTANCE_ROW_TYPES = dict(d2_solid=torch.int32, nearest_solid=torch.int32, d2_free=torch.int32, nearest_free=torch.int32, esdf=torch.float32,
                          nearest_label=torch.int32)
UNSIGNED_ROWS, SIGNED_ROWS = ('d2_solid', 'nearest_solid'), ('d2_free', 'nearest_free', 'esdf')
PLAN_DEFAULTS = dict(margin=0.0)                                               # what a plan adds: collision_free_m = approach_clearance_m > margin


def checked_distance(level=0.0, lower=None, z_min=0, surface_offset=0.5, signed=True):
    """The transform's parameters, checked before anything touches the device (the library refuses the same; z_min <= R is the
    library's, which knows R)."""
    solid = checked_solid('distance', level, lower, z_min)
    if not (math.isfinite(surface_offset) and surface_offset >= 0):
        raise ValueError(f'distance surface_offset must be finite and >= 0 voxels, got {surface_offset!r}')
    if not isinstance(signed, bool):
        raise ValueError(f'distance signed must be True or False, got {signed!r}')
    return dict(solid, surface_offset=float(surface_offset), signed=signed)


def distance_params(distance, **more):
    """A `distance` argument -> None (False / None: not asked for), or the transform's parameters (True / {}: solid below 0, no lower
    bound, no table cut, the surface half a voxel off the solid voxels, the signed field too).  Unknown keys are a TypeError, and every
    value is checked here, before the device.  more: further keys the caller takes, with their defaults."""
    out = checked_params('distance', distance, {**DISTANCE_DEFAULTS, **more})
    if out is not None:
        out.update(checked_distance(**picked(out, DISTANCE_DEFAULTS)))
    return out


def checked_scale(scale):
    if isinstance(scale, bool) or not (math.isfinite(scale) and scale > 0):
        raise ValueError(f'distance scale must be finite and > 0 metres per voxel, got {scale!r}')
    return float(scale)


class VolumeDistance(DeviceOp):
    """The distance field of B volumes.  The output tensors are kept per (B, R) and written again by the next call of that shape, and
    the workspace only grows, so the addresses are stable for a captured graph once a warm-up call has run."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'volume distance')
        self._out = {}

    def __call__(self, vol, *, scale, labels=None, level=0.0, lower=None, z_min=0, surface_offset=0.5, signed=True):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]), 2 <= R <= 256;  scale: metres per voxel;  labels: None, or VolumeObjects'
        `labels` of the same shape;  solid: lower < v < level and k >= z_min (lower None: no lower bound; a NaN is not solid), every
        other voxel is free;  surface_offset: voxels taken off every distance (0.5: the surface lies halfway between a solid voxel and
        its free neighbour);  signed: also the transform to the free voxels and the signed field.
        -> {'d2_solid': [B,R,R,R] int32 (the squared distance in voxels to the nearest solid voxel of the same scene, 0 at a solid one;
        3 R^2: the scene has none), 'nearest_solid': [B,R,R,R] int32 (that voxel as i R^2 + j R + k, of several the smallest; -1: none);
        with signed 'd2_free' and 'nearest_free' (the same to the free voxels) and 'esdf': [B,R,R,R] float32 (metres:
        (sqrt(d2_solid) - surface_offset) * scale at a free voxel, -(sqrt(d2_free) - surface_offset) * scale at a solid one);  with
        labels 'nearest_label': [B,R,R,R] int32 (the label at nearest_solid; 0: none, or that voxel carries no label)}.
        The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        q = checked_distance(level, lower, z_min, surface_offset, signed)
        scale = checked_scale(scale)
        vol, B, R = volume_batch(vol, d)
        solid = solid_fields('distance', q, R, z_min)
        if labels is not None:
            labels, Bl, Rl = labels_batch(labels, d)
            if (Bl, Rl) != (B, R):
                raise ValueError(f'labels must be [{B},{R},{R},{R}] like vol, got {tuple(labels.shape)}')
        names = UNSIGNED_ROWS + (SIGNED_ROWS if q['signed'] else ()) + (('nearest_label',) if labels is not None else ())
        out = self._out.setdefault((B, R), {})
        for k in names:
            if k not in out:
                out[k] = torch.zeros(B, R, R, R, dtype=DISTANCE_ROW_TYPES[k], device=d)
        p = _lib.GnrDistanceParams(**solid, scale=scale, surface_offset=q['surface_offset'])
        ws, ws_bytes = self._workspace(self.L.gnr_volume_distance_workspace_bytes(B, R))
        ptr = lambda k: out[k].data_ptr() if k in names else None
        rc = self.L.gnr_volume_distance_fwd(C.byref(p), vol.data_ptr(), None if labels is None else labels.data_ptr(), B, R,
                                            *(ptr(k) for k in DISTANCE_ROW_TYPES), ws, ws_bytes, self._stream())
        _lib.check(rc, 'gnr_volume_distance_fwd')
        return {k: out[k] for k in names}


def distance_rows(res, b):
    """The device tensors of scene b of a VolumeDistance result."""
    return {k: v[b] for k, v in res.items()}


def distance_from_rows(rows, scale):
    """distance_rows on the host (numpy) -> the field of one scene: the arrays [R,R,R] under their names, `scale` (metres per voxel),
    `has_solid` / `has_free` (False: the scene has no such voxel, d2 reads 3 R^2 and nearest -1 everywhere), and `distance_m` [R,R,R]
    float64 = sqrt(d2_solid) * scale, the unsigned distance to the nearest solid voxel's centre (inf without one)."""
    out = {k: np.array(v) for k, v in rows.items()}
    out['scale'] = checked_scale(scale)
    out['has_solid'] = bool(out['nearest_solid'].flat[0] >= 0)
    if 'nearest_free' in out:
        out['has_free'] = bool(out['nearest_free'].flat[0] >= 0)
    out['distance_m'] = np.sqrt(out['d2_solid'].astype(np.float64)) * np.float64(scale) if out['has_solid'] else \
        np.full(out['d2_solid'].shape, np.inf)
    return out


def nearest_vector(nearest, R, scale):
    """nearest [...,R,R,R] int32 (`nearest_solid` or `nearest_free`, on the host) -> [...,R,R,R,3] float64 metres from each voxel to its
    nearest site, (i' - i, j' - j, k' - k) * scale; NaN where there is none (-1).  The direction a planner pushes along (away from
    nearest_solid: its negative)."""
    nearest = np.asarray(nearest)
    if nearest.ndim < 3 or tuple(nearest.shape[-3:]) != (R, R, R):
        raise ValueError(f'nearest must be [...,{R},{R},{R}], got {tuple(nearest.shape)}')
    site = np.stack(np.unravel_index(np.maximum(nearest, 0), (R, R, R)), -1)
    own = np.stack(np.meshgrid(*(np.arange(R),) * 3, indexing='ij'), -1)
    vec = (site - own).astype(np.float64) * np.float64(scale)
    vec[nearest < 0] = np.nan
    return vec


def _labels_of(objects):
    """An objects_of_plan result (the pair, or its first dict) or a labels array -> the labels array."""
    if isinstance(objects, tuple):
        objects = objects[0]
    return objects['labels'] if isinstance(objects, dict) else objects


def distance_of_plan(tsdf_vol, grasps, *, voxel_size=PLAN_VOXEL_SIZE, objects=None, device='cuda:0', **params):
    """The distance field of a plan and the hand's margin in it: tsdf_vol and the grasps dict as plan_real / plan / plan_depth return
    them (one scene; objects.objects_of_plan's conventions: `index` the voxel of each grasp, `quat` (x, y, z, w), `width` in metres).
    objects: None, or what objects_of_plan returned (or a labels array [R,R,R]): then also the object every voxel is nearest to.
    params: DISTANCE_DEFAULTS' keys (signed must stay True: the hand reads `esdf`), the hand's (HAND_DEFAULTS) and margin (metres).
    -> (field, columns): distance_from_rows' dict, and per grasp, in the order of the grasps, `clearance_m` [n] float32 (the smallest
    value of esdf under the hand at the grasp: by how many metres the hand misses the nearest solid voxel's half-voxel shell;
    negative: how deep it is in), `approach_clearance_m` [n] float32 (the same over the approach), `collision_free_m` [n] bool =
    approach_clearance_m > margin, hand_from_rows' `hand_inside` and `hand_worst`, and with objects `nearest_object` [n] int32
    (nearest_label at the grasp's own voxel).  HandClearance clips at 1.0: a margin reads at most 1 m."""
    params = split_params('distance', params, DISTANCE_DEFAULTS, HAND_DEFAULTS, PLAN_DEFAULTS)
    q = distance_params(picked(params, DISTANCE_DEFAULTS))
    if not q['signed']:
        raise ValueError('distance_of_plan reads the hand\'s margin from esdf: signed must be True')
    hand = picked(params, HAND_DEFAULTS)
    checked_hand(**hand)
    margin = float(params['margin'])
    if not math.isfinite(margin):
        raise ValueError(f'distance margin must be finite metres, got {margin!r}')
    scale = checked_scale(voxel_size)
    d = torch.device(device)
    vol, B, R = volume_batch(tsdf_vol, d)
    if B != 1:
        raise ValueError(f'distance_of_plan takes the volume of one scene, got {B}')
    labels = None if objects is None else torch.as_tensor(np.asarray(_labels_of(objects)), dtype=torch.int32).reshape(1, R, R, R)
    res = VolumeDistance(d)(vol, scale=scale, labels=labels, **q)
    pos, qt, wd, count, n = plan_rows(grasps, voxel_size, d)
    hres = HandClearance(d)(res['esdf'], pos, qt, wd, count, scale=scale, **hand)
    field = distance_from_rows(_host(distance_rows(res, 0)), scale)
    cols = hand_from_rows(_host(hand_rows(hres, 0, n)), margin)
    columns = {'clearance_m': cols['clearance'], 'approach_clearance_m': cols['approach_clearance'], 'collision_free_m': cols['collision_free'],
               'hand_inside': cols['hand_inside'], 'hand_worst': cols['hand_worst']}
    if labels is not None:
        at = np.asarray(grasps['index']).reshape(n, 3).astype(np.int64)
        columns['nearest_object'] = field['nearest_label'][at[:, 0], at[:, 1], at[:, 2]].astype(np.int32)
    return field, columns
