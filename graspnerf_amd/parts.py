"""Parts of touching objects, on the device (csrc/gnr_parts.hip, gnr_volume_parts_fwd): the solid voxels split at their necks.
objects.VolumeObjects knows solid voxels and nothing of shapes, so the objects of a pile are one component; the reference's scenes are
piles and packed clutter (render_pile_STD_rand.py, sim_grasp.py).  distance.VolumeDistance's `d2_free` is, per solid voxel, the
squared radius of the largest ball around it that stays inside the solid: two convex things that touch are two hills joined over a
low pass.  VolumeParts is a watershed of the solid voxels by steepest ascent on such an integer height field; neighbouring basins are
merged where the pass between them is no neck: pass >= neck^2 * the smaller of the two peaks (`neck` a ratio of radii).  Numbering,
statistics rows and calling conventions are VolumeObjects', so GraspObjects and best_per_object take the labels as they are.
include/gnr.h states the rule; the results are the bits of tests/parts_reference.py.
What a caller must know.  Two boxes face to face without a gap are one box to any rule that sees the solid voxels alone, and stay one;
a single object whose waist is narrower than `neck` times its smaller bulge is cut in two.  The default neck = 0.8 separates the
synthetic touching shapes of tests/test_volume_parts.py (two overlapping spheres, a sphere resting on a box, three touching spheres)
and keeps single spheres, boxes, a lying cylinder and an L-shape whole; it has not been run on a network's volume, whose rough
surfaces may need `min_peak` (basins that low join whatever they adjoin) -- which is why both stay keywords.
No row of planner.PRODUCTS yet: parts_of_plan runs the operators on what plan_real / plan / plan_depth return."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .distance import VolumeDistance, checked_scale
from .grasp_post import SOLID_DEFAULTS, DeviceOp, _host, checked_params, checked_solid, height_batch, picked, split_params, volume_batch
from .hand import HAND_DEFAULTS, checked_hand, plan_rows
from .objects import OBJECT_ROW_TYPES, PLAN_VOXEL_SIZE, GraspObjects, grasp_objects_rows, objects_from_rows

PART_DEFAULTS = dict(connectivity=26, max_parts=1024, neck=0.8, min_peak=0)
PART_ROW_TYPES = dict(OBJECT_ROW_TYPES, peak=((), torch.int32), peak_voxel=((), torch.int32))      # per statistics row: shape, dtype


def checked_parts(connectivity=26, max_parts=1024, neck=0.8, min_peak=0):
    """The split's parameters, checked before anything touches the device (the library refuses the same)."""
    if connectivity not in (6, 18, 26) or isinstance(connectivity, bool):
        raise ValueError(f'parts connectivity must be 6, 18 or 26, got {connectivity!r}')
    if isinstance(max_parts, bool) or int(max_parts) != max_parts or max_parts < 1:
        raise ValueError(f'parts max_parts must be an integer >= 1, got {max_parts!r}')
    if isinstance(neck, bool) or not (math.isfinite(neck) and 0 <= neck <= 1):
        raise ValueError(f'parts neck must be finite and in 0..1 (a ratio of radii; above 1 the summits of one plateau would not merge), got {neck!r}')
    if isinstance(min_peak, bool) or int(min_peak) != min_peak or min_peak < 0:
        raise ValueError(f'parts min_peak must be an integer >= 0, got {min_peak!r}')
    return dict(connectivity=int(connectivity), max_parts=int(max_parts), neck=float(neck), min_peak=int(min_peak))


def part_params(parts, **more):
    """A `parts` argument -> None (False / None: not asked for), or the split's parameters (True / {}: 26-connected, 1 024 statistics
    rows, neck 0.8, no minimum peak).  Unknown keys are a TypeError, and every value is checked here, before the device.  more: further
    keys the caller takes, with their defaults."""
    out = checked_params('parts', parts, {**PART_DEFAULTS, **more})
    if out is not None:
        out.update(checked_parts(**picked(out, PART_DEFAULTS)))
    return out


class VolumeParts(DeviceOp):
    """The parts of the solid voxels of B height fields.  The output tensors are kept per (B, R, max_parts) and written again by the
    next call of that shape, and the workspace only grows, so the addresses are stable for a captured graph once a warm-up call has
    run."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'volume parts')
        self._out = {}

    def __call__(self, height, *, connectivity=26, max_parts=1024, neck=0.8, min_peak=0):
        """height [B,R,R,R] int32 (or one [R,R,R]), 2 <= R <= 256: VolumeDistance's `d2_free`, or any integer field -- solid: height > 0;
        connectivity 6, 18 or 26;  max_parts: rows of the statistics;  neck in [0, 1]: two adjoining basins are joined when the pass
        between them is at least neck^2 times the smaller of their peaks (0: always, the parts are VolumeObjects' components);
        min_peak: a basin whose peak is at most this joins every basin it adjoins.
        -> {'labels': [B,R,R,R] int32 (0: not solid; else the part's number, ndimage.label's order), 'count': [B] int32 (the true number
        of parts, also beyond max_parts), 'basins': [B] int32 (the summits of the ascent, before any merge), 'voxels': [B,max_parts]
        int32, 'bbox': [B,max_parts,6] int32 and 'sums': [B,max_parts,3] int64 (VolumeObjects' rows), 'peak': [B,max_parts] int32 (the
        largest height in the part; 0: no such part), 'peak_voxel': [B,max_parts] int32 (the smallest voxel i R^2 + j R + k of the part
        that has it; -1), 'status': [1] int32 (0, or _lib.GNR_PARTS_STATUS_BOUND: a loop ran into its bound and the results are not to
        be used)}, with `max_parts` as given.  The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        q = checked_parts(connectivity, max_parts, neck, min_peak)
        height, B, R = height_batch(height, d)
        M = q['max_parts']
        out = self._out.get((B, R, M))
        if out is None:
            out = self._out[(B, R, M)] = {'labels': torch.zeros(B, R, R, R, dtype=torch.int32, device=d), 'count': torch.zeros(B, dtype=torch.int32, device=d),
                                          'basins': torch.zeros(B, dtype=torch.int32, device=d),
                                          **{k: torch.zeros(B, M, *tail, dtype=dtype, device=d) for k, (tail, dtype) in PART_ROW_TYPES.items()}}
        p = _lib.GnrPartsParams(neck=q['neck'], connectivity=q['connectivity'], max_parts=M, min_peak=q['min_peak'])
        ws, ws_bytes = self._workspace(self.L.gnr_volume_parts_workspace_bytes(B, R))
        rc = self.L.gnr_volume_parts_fwd(C.byref(p), height.data_ptr(), B, R, out['labels'].data_ptr(), out['count'].data_ptr(),
                                         out['basins'].data_ptr(), *(out[k].data_ptr() for k in PART_ROW_TYPES), ws, ws_bytes, self._stream())
        _lib.check(rc, 'gnr_volume_parts_fwd')
        return dict(out, status=self._ws[:4].view(torch.int32), max_parts=M)


def parts_rows(res, b, n):
    """The device rows of scene b of a VolumeParts result, given its count n: the first min(n, max_parts) statistics rows, the count,
    the basin count and the status word."""
    m = min(int(n), res['voxels'].shape[1])
    return {'count': res['count'][b:b + 1], 'basins': res['basins'][b:b + 1], 'status': res['status'], **{k: res[k][b, :m] for k in PART_ROW_TYPES}}


def parts_from_rows(rows, scale, origin=(0.0, 0.0, 0.0)):
    """parts_rows on the host (numpy) -> objects.objects_from_rows' fields (`count`, `voxels`, `bbox_lo`, `bbox_hi`, `centroid`,
    `extent`, `top`, `kept`) and `peak` [n] int32, `peak_voxel` [n] int32, `radius` [n] float64 metres = sqrt(peak) * scale (with heights
    from d2_free: the distance from the part's deepest voxel to the nearest free voxel's centre), `basins` (int).
    Raises when the scene has more parts than statistics rows, or when the split reported that a loop ran into its bound."""
    count, held = int(np.asarray(rows['count']).reshape(-1)[0]), len(np.asarray(rows['voxels']))
    if 'status' in rows and int(np.asarray(rows['status']).reshape(-1)[0]) != 0:
        raise _lib.GnrError('the split ran into the bound of one of its loops (GNR_PARTS_STATUS_BOUND): its results are not to be used')
    if count > held:
        raise _lib.GnrError(f'{count} parts but the buffers hold {held}: raise max_parts')
    out = objects_from_rows({k: rows[k] for k in ('count', *OBJECT_ROW_TYPES)}, scale, origin)
    peak = np.array(np.asarray(rows['peak']).reshape(-1)[:count])
    out.update(peak=peak, peak_voxel=np.array(np.asarray(rows['peak_voxel']).reshape(-1)[:count]),
               radius=np.sqrt(peak.astype(np.float64)) * np.float64(scale), basins=int(np.asarray(rows['basins']).reshape(-1)[0]))
    return out


def grasp_parts_from_rows(rows):
    """objects.grasp_objects_rows of a GraspObjects call on the parts' labels, on the host (numpy) -> the columns of the grasps: `part`
    [n] int32 (the label the hand closes on, 0: none), `part_votes` [n] int32, `parts_in_hand` [n] int32 (2 and more: the grasp pinches
    several), `part_samples` [n] int32."""
    return {'part': np.array(rows['object']), 'part_votes': np.array(rows['votes']), 'parts_in_hand': np.array(rows['distinct']),
            'part_samples': np.array(rows['inside'])}


def parts_of_plan(tsdf_vol, grasps, *, voxel_size=PLAN_VOXEL_SIZE, origin=(0.0, 0.0, 0.0), device='cuda:0', **params):
    """The parts of a plan: tsdf_vol and the grasps dict as plan_real / plan / plan_depth return them (one scene;
    objects.objects_of_plan's conventions).  params: the solid rule's keys (SOLID_DEFAULTS: level, lower, z_min -- z_min must cut the
    table slab, or the table is the largest hill), PART_DEFAULTS' and the hand's (HAND_DEFAULTS).  VolumeDistance on the volume,
    VolumeParts on its d2_free, GraspObjects on the parts' labels.
    -> (parts, columns): parts_from_rows' dict with `labels` [R,R,R] int32, and grasp_parts_from_rows' columns, in the order of the
    grasps; objects.best_per_object(columns['part']) is the best-ranked grasp of every part."""
    params = split_params('parts', params, SOLID_DEFAULTS, PART_DEFAULTS, HAND_DEFAULTS)
    solid = checked_solid('parts', **picked(params, SOLID_DEFAULTS))
    q = part_params(picked(params, PART_DEFAULTS))
    hand = picked(params, HAND_DEFAULTS)
    checked_hand(**hand)
    scale = checked_scale(voxel_size)
    d = torch.device(device)
    vol, B, R = volume_batch(tsdf_vol, d)
    if B != 1:
        raise ValueError(f'parts_of_plan takes the volume of one scene, got {B}')
    field = VolumeDistance(d)(vol, scale=scale, **solid)
    res = VolumeParts(d)(field['d2_free'], **q)
    pos, qt, wd, count, n = plan_rows(grasps, voxel_size, d)
    gres = GraspObjects(d)(res['labels'], pos, qt, wd, count, scale=scale, **hand)
    parts = parts_from_rows(_host(parts_rows(res, 0, int(res['count'][0].item()))), scale, origin)
    parts['labels'] = res['labels'][0].cpu().numpy()
    return parts, grasp_parts_from_rows(_host(grasp_objects_rows(gres, 0, n)))
