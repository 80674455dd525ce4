"""Gripper clearance of the ranked grasps against the volume, on the device (csrc/gnr_hand.hip, gnr_hand_clearance_fwd): whether the
hand fits where the network wants to put it.  The reference answers this with physics -- ClutterRemovalSim.execute_grasp
(gd/simulation.py:369-402) fails a grasp on contact at the pre-grasp pose 5 cm back along the grasp's z and again on the straight way
in; on a real robot the only geometry the planner has is the volume it has just predicted.  Per grasp: the smallest value of the
volume over samples of the hand's four boxes (grasp_post.HAND_GEOMETRY, draw_gripper_o3d's) at the grasp, and over everything they
pass through on the approach.  include/gnr.h states the arithmetic; the results are the bits of the float64 statement
tests/hand_reference.py.  No reference counterpart.
FingerClosure (gnr_finger_closure_fwd, the same file's second kernel) is the step after it: execute_grasp closes the fingers and
check_success (gd/simulation.py:404,465-469) asks whether they hold something.  Per grasp: where pad rays on each finger's inner face
first meet the surface on their way to the centre plane, the width of the closed hand, and the cosine between the surface and the
closing direction at the two contacts; the bits of tests/closure_reference.py."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .grasp_post import HAND_GEOMETRY, DeviceOp, checked_params, picked, volume_batch

HAND_DEFAULTS = dict(HAND_GEOMETRY, opening=None, spacing=0.5, approach=0.05)
PLAN_DEFAULTS = dict(level=0.0)                              # what a plan adds: collision_free = approach_clearance > level
EXECUTE_GRASP_OPENING = 0.08                                 # execute_grasp opens the hand to max_opening_width (simulation.py:372)
HAND_ROW_TYPES = dict(clearance=((2,), torch.float32), worst=((2,), torch.int32), inside=((2,), torch.int32))      # per grasp: shape, dtype
CLOSURE_ROW_TYPES = dict(travel=((2,), torch.float32), cosine=((2,), torch.float32), contact=((2,), torch.int32), closed=((), torch.float32))
CLOSURE_ROWS = tuple(CLOSURE_ROW_TYPES)
CLOSURE_DEFAULTS = dict(HAND_DEFAULTS, level=0.0, bisections=4)                # FingerClosure.__call__'s keywords
CLOSURE_PLAN_DEFAULTS = dict(max_opening=0.08, friction=None)                  # what a plan adds: closure_from_rows's keywords
CHECK_SUCCESS_FRACTION = 0.1                                                   # check_success: width > 0.1 * max_opening_width (simulation.py:468)


def _hand_params(what, given, defaults):
    """checked_params, with the hand's own keys as floats and checked (checked_hand)."""
    out = checked_params(what, given, defaults)
    if out is not None:
        for k in ('height', 'finger_width', 'tail_length', 'depth', 'spacing', 'approach'):
            out[k] = float(out[k])
        out['opening'] = None if out['opening'] is None else float(out['opening'])
        checked_hand(**picked(out, HAND_DEFAULTS))
    return out


def hand_params(clearance, **more):
    """A plan's `clearance` / a session's `hand_clearance` argument -> None, or the hand's parameters (True / {}: the viewer's hand of
    draw_gripper_o3d opened to each grasp's own predicted width, samples half a voxel apart, a 5 cm approach, collision_free =
    approach_clearance > 0).  more: further keys the caller takes, with their defaults (plan_real's `filter`)."""
    out = _hand_params('clearance', clearance, {**HAND_DEFAULTS, **PLAN_DEFAULTS, **more})
    if out is not None:
        out['level'] = float(out['level'])
    return out


def checked_hand(height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, opening=None, spacing=0.5, approach=0.05):
    """The hand's parameters, checked before anything touches the device (the library refuses the same): every dimension and the
    spacing finite and positive, the approach finite and not negative, an opening a finite number of metres that is not negative
    (None: each grasp's own width)."""
    for k, v in (('height', height), ('finger_width', finger_width), ('tail_length', tail_length), ('depth', depth), ('spacing', spacing)):
        if not (math.isfinite(v) and v > 0):
            raise ValueError(f'hand {k} must be finite and > 0, got {v!r}')
    if not (math.isfinite(approach) and approach >= 0):
        raise ValueError(f'hand approach must be finite and >= 0, got {approach!r}')
    if opening is not None and not (math.isfinite(opening) and opening >= 0):
        raise ValueError(f'hand opening must be None (each grasp\'s own width) or finite and >= 0 metres, got {opening!r}')
    return dict(height=float(height), finger_width=float(finger_width), tail_length=float(tail_length), depth=float(depth),
                opening=-1.0 if opening is None else float(opening), spacing=float(spacing), approach=float(approach))


def selection_pos(sel):
    """The grasp positions of a GraspSelector result in lattice units: its voxel indices as float64 [B,max,3] (a device tensor)."""
    return sel['index'].double()


def plan_rows(grasps, voxel_size, device):
    """The grasps dict of a plan (one scene; grasps_from_selection's conventions: `index` the voxel of each grasp, `quat` (x, y, z, w),
    `width` in metres) -> (pos [1,rows,3] float64, quat [1,rows,4] float32, width [1,rows] float32 in voxels, count [1] int32 on the
    device, n): the rows the checks of grasps take.  The width goes back to voxels by / voxel_size in float32, the selection's own
    format; rows = max(n, 1): the library takes no empty buffer, so no grasp is one row that the count leaves out."""
    index, quat, width = np.asarray(grasps['index']), np.asarray(grasps['quat']), np.asarray(grasps['width'])
    n = len(index)
    rows = max(n, 1)
    pos, qt, wd = np.zeros((1, rows, 3), np.float64), np.zeros((1, rows, 4), np.float32), np.zeros((1, rows), np.float32)
    pos[0, :n], qt[0, :n], wd[0, :n] = index.reshape(n, 3), quat.reshape(n, 4), (width.reshape(n) / np.float32(voxel_size)).astype(np.float32)
    return pos, qt, wd, torch.tensor([n], dtype=torch.int32, device=device), n


def checked_rows(pos, quat, width, count, top_k, B, d):
    """The rows of grasps of B scenes on device d, as the kernels read them -> (pos [B,n,3] float64, quat [B,n,4] float32, width [B,n]
    float32, n); count and top_k are checked."""
    pos = torch.as_tensor(pos, dtype=torch.float64, device=d).contiguous()
    quat = torch.as_tensor(quat, dtype=torch.float32, device=d).contiguous()
    width = torch.as_tensor(width, dtype=torch.float32, device=d).contiguous()
    if pos.dim() == 2:
        pos, quat, width = pos[None], quat[None], width[None]
    if pos.dim() != 3 or pos.shape[0] != B or pos.shape[2] != 3:
        raise ValueError(f'pos must be [{B},max_n,3], got {tuple(pos.shape)}')
    n = pos.shape[1]
    if tuple(quat.shape) != (B, n, 4) or tuple(width.shape) != (B, n):
        raise ValueError(f'quat must be [{B},{n},4] and width [{B},{n}], got {tuple(quat.shape)} and {tuple(width.shape)}')
    if not torch.is_tensor(count) or count.dtype != torch.int32 or count.device != pos.device or count.shape[0] != B or \
            not count.is_contiguous():
        raise ValueError(f'count must be a contiguous int32 device tensor [{B}] or [{B},k]')
    if top_k is not None and int(top_k) < 1:
        raise ValueError(f'top_k must be None or positive, got {top_k!r}')
    return pos, quat, width, n


class _GraspRows(DeviceOp):
    """What the two checks of rows of grasps share.  The output buffers (ROW_TYPES) are kept per shape and written again by the next
    call of that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, self.NOUN)
        self._out = {}

    _batch = staticmethod(volume_batch)                      # what the rows are checked against (objects.GraspObjects: a label volume)

    def _checked(self, vol, pos, quat, width, count, scale, top_k, *hand):
        """The arguments both kernels take (hand: checked_hand's, in its order), checked -> (GnrHandParams, vol, pos, quat, width, B, R, n,
        this shape's output tensors)."""
        d = self.device
        hand = checked_hand(*hand)
        vol, B, R = self._batch(vol, d)
        pos, quat, width, n = checked_rows(pos, quat, width, count, top_k, B, d)
        out = self._out.get((B, n))
        if out is None:
            out = self._out[(B, n)] = tuple(torch.zeros(B, n, *tail, dtype=dtype, device=d) for tail, dtype in self.ROW_TYPES.values())
        return _lib.GnrHandParams(scale=float(scale), **hand), vol, pos, quat, width, B, R, n, out

    def of_selection(self, vol, sel, *, scale, **kw):
        """... of the rows of a GraspSelector result (any route's: plan, plan_real, plan_depth), with its top_k."""
        return self(vol, selection_pos(sel), sel['quat'], sel['width'], sel['count'], scale=scale, top_k=sel.get('top_k'), **kw)


class HandClearance(_GraspRows):
    """The clearance of the hand at rows of grasps of B volumes."""
    NOUN, ROW_TYPES = 'hand clearance', HAND_ROW_TYPES

    def __call__(self, vol, pos, quat, width, count, *, scale, top_k=None, height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05,
                 opening=None, spacing=0.5, approach=0.05):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]), 2 <= R <= 256;  pos [B,max_n,3] float64 in lattice units (voxel (i,j,k)'s value
        sits at (i,j,k): selection_pos(sel), or metres / scale);  quat [B,max_n,4] float32 (x, y, z, w; as the selection stores it, it is
        normalised in float64);  width [B,max_n] float32 in voxels;  count [B] or [B,k] int32 device tensor, its first column the rows of
        each scene;  scale: metres per voxel;  top_k: at most that many rows per scene;  opening: None for each grasp's own width, or one
        opening in metres for every grasp (EXECUTE_GRASP_OPENING: what execute_grasp opens the hand to);  height, finger_width,
        tail_length, depth: the hand in metres (the defaults are the viewer's; a real hand is thicker, e.g. height=0.02,
        finger_width=0.01);  spacing: voxels between samples at most;  approach: metres the hand comes in along its z (0: none).
        -> {'clearance': [B,max_n,2] float32 (the smallest value of the volume under the hand at the grasp, and on its approach; 1.0:
        nothing of the hand is inside the volume), 'worst': [B,max_n,2] int32 (the ordinal of the sample that attains it, -1: none),
        'inside': [B,max_n,2] int32 (the samples inside the volume)}; rows beyond min(count, top_k, max_n) keep what they held.
        The tensors are this object's: the next call with the same shape writes them again."""
        p, vol, pos, quat, width, B, R, n, out = self._checked(vol, pos, quat, width, count, scale, top_k, height, finger_width, tail_length, depth,
                                                               opening, spacing, approach)
        rc = self.L.gnr_hand_clearance_fwd(C.byref(p), vol.data_ptr(), pos.data_ptr(), quat.data_ptr(), width.data_ptr(), count.data_ptr(),
                                           count.numel() // B, B, R, n, int(top_k or 0), *(t.data_ptr() for t in out), self._stream())
        _lib.check(rc, 'gnr_hand_clearance_fwd')
        return dict(zip(HAND_ROW_TYPES, out))


class FingerClosure(_GraspRows):
    """Where the two fingers stop when the hand closes on the volume, at rows of grasps of B volumes (csrc/gnr_hand.hip,
    gnr_finger_closure_fwd): the third step of execute_grasp -- `gripper.move(0.0)` and check_success (gd/simulation.py:404,465-469) --
    answered from the volume.  include/gnr.h states the arithmetic; the results are the bits of tests/closure_reference.py.  The depth
    route has no switch for it and calls of_selection by hand with level=0.5 on (tsdf + 1) / 2 where weight > 0 and 1 elsewhere
    (get_grid() itself is 0 in unseen and far free space, which would read as solid)."""
    NOUN, ROW_TYPES = 'finger closure', CLOSURE_ROW_TYPES

    def __call__(self, vol, pos, quat, width, count, *, scale, top_k=None, level=0.0, bisections=4, height=0.004, finger_width=0.004,
                 tail_length=0.04, depth=0.05, opening=None, spacing=0.5, approach=0.05):
        """vol, pos, quat, width, count, scale, top_k and the hand's keywords: HandClearance.__call__'s (tail_length and approach are checked
        and not used);  level: the value of the volume at the surface (0 for the network's tsdf; 0.5 for the depth route's fused volume,
        tsdf.py);  bisections: halvings of a ray's bracket before its secant step, 0..16.
        Each finger's inner face carries pad rays at most `spacing` voxels apart; finger 0 closes from y = -opening / 2 towards +y,
        finger 1 from +opening / 2 towards -y, both to the centre plane at the latest, and stops where its first ray meets a value below
        the level.
        -> {'travel': [B,max_n,2] float32 (metres each finger moved; opening / 2: it met nothing), 'cosine': [B,max_n,2] float32 (between
        the surface's normal at the contact and the closing direction; 1: squarely, 0: no contact), 'contact': [B,max_n,2] int32 (the
        ordinal of the ray that stopped the finger, -1: none), 'closed': [B,max_n] float32 (the width of the closed hand in metres)};
        rows beyond min(count, top_k, max_n) keep what they held.  The tensors are this object's."""
        level, bisections = checked_closure(level, bisections)
        p, vol, pos, quat, width, B, R, n, out = self._checked(vol, pos, quat, width, count, scale, top_k, height, finger_width, tail_length, depth,
                                                               opening, spacing, approach)
        rc = self.L.gnr_finger_closure_fwd(C.byref(p), level, bisections, vol.data_ptr(), pos.data_ptr(), quat.data_ptr(), width.data_ptr(),
                                           count.data_ptr(), count.numel() // B, B, R, n, int(top_k or 0), *(t.data_ptr() for t in out),
                                           self._stream())
        _lib.check(rc, 'gnr_finger_closure_fwd')
        return dict(zip(CLOSURE_ROWS, out))


def checked_closure(level=0.0, bisections=4):
    """The closure's own parameters, checked before anything touches the device (the library refuses the same)."""
    if not math.isfinite(level):
        raise ValueError(f'closure level must be finite, got {level!r}')
    if int(bisections) != bisections or not 0 <= bisections <= 16:
        raise ValueError(f'closure bisections must be an integer in 0..16, got {bisections!r}')
    return float(level), int(bisections)


def closure_params(closure, **more):
    """A plan's `closure` / a session's `finger_closure` argument -> None, or the closure's parameters (True / {}: the viewer's hand
    opened to each grasp's own predicted width, pad rays half a voxel apart, the surface at 0, held = both fingers touch and the closed
    hand is wider than 0.1 * 0.08 m, no friction coefficient).  more: further keys the caller takes, with their defaults (plan_real's
    `filter`)."""
    out = _hand_params('closure', closure, {**CLOSURE_DEFAULTS, **CLOSURE_PLAN_DEFAULTS, **more})
    if out is not None:
        out['max_opening'] = float(out['max_opening'])
        out['friction'] = None if out['friction'] is None else float(out['friction'])
        out['level'], out['bisections'] = checked_closure(out['level'], out['bisections'])
        checked_held(out['max_opening'], out['friction'])
    return out


def checked_held(max_opening=0.08, friction=None):
    if not (math.isfinite(max_opening) and max_opening > 0):
        raise ValueError(f'closure max_opening must be finite and > 0 metres, got {max_opening!r}')
    if friction is not None and not (math.isfinite(friction) and friction >= 0):
        raise ValueError(f'closure friction must be None or finite and >= 0, got {friction!r}')


def closure_rows(res, b, n):
    """The device rows of scene b of a FingerClosure result, given the number of grasps n the selection stored."""
    return {k: res[k][b, :n] for k in CLOSURE_ROWS}


def closure_from_rows(rows, max_opening=0.08, friction=None):
    """closure_rows on the host (numpy) -> the columns a plan adds to its grasps: `closed_width` [n] float32 (metres: what a robot
    compares with its gripper's read-back), `finger_travel` [n,2] and `contact_cos` [n,2] float32, `finger_contact` [n,2] int32,
    `grip_cos` [n] float32 (the smaller of the two cosines), `held` [n] bool = both fingers have a contact and closed_width >
    0.1 * max_opening (check_success, gd/simulation.py:465-469,478);  with friction=mu also `force_closure` [n] bool = grip_cos >=
    1 / sqrt(1 + mu^2): both contact normals lie within the friction cone about the closing direction (no default: the reference
    sets none)."""
    checked_held(max_opening, friction)
    cos, contact, closed = np.asarray(rows['cosine']), np.asarray(rows['contact']), np.asarray(rows['closed'])
    out = {'closed_width': closed.copy(), 'finger_travel': np.array(rows['travel']), 'contact_cos': cos.copy(), 'finger_contact': contact.copy(),
           'grip_cos': cos.min(axis=1) if len(cos) else np.zeros(0, np.float32)}
    out['held'] = (contact >= 0).all(axis=1) & (closed > np.float32(CHECK_SUCCESS_FRACTION * max_opening))
    if friction is not None:
        out['force_closure'] = out['grip_cos'] >= np.float32(1.0 / math.sqrt(1.0 + friction * friction))
    return out


def hand_rows(res, b, n):
    """The device rows of scene b of a HandClearance result, given the number of grasps n the selection stored."""
    return {k: res[k][b, :n] for k in HAND_ROW_TYPES}


def hand_from_rows(rows, level=0.0):
    """hand_rows on the host (numpy) -> the columns a plan adds to its grasps: `clearance` [n] and `approach_clearance` [n] float32 (the
    volume's units), `hand_inside` [n,2] and `hand_worst` [n,2] int32 (at the grasp, on the approach), `collision_free` [n] bool =
    approach_clearance > level."""
    c = np.asarray(rows['clearance'])
    return {'clearance': c[:, 0].copy(), 'approach_clearance': c[:, 1].copy(), 'hand_inside': np.array(rows['inside']),
            'hand_worst': np.array(rows['worst']), 'collision_free': c[:, 1] > np.float32(level)}
