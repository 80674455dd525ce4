"""Gripper clearance of the ranked grasps against the volume, on the device (csrc/gnr_hand.hip, gnr_hand_clearance_fwd): whether the
hand fits where the network wants to put it.  The reference answers this with physics -- ClutterRemovalSim.execute_grasp
(gd/simulation.py:369-402) fails a grasp on contact at the pre-grasp pose 5 cm back along the grasp's z and again on the straight way
in; on a real robot the only geometry the planner has is the volume it has just predicted.  Per grasp: the smallest value of the
volume over samples of the hand's four boxes (grasp_post.HAND_GEOMETRY, draw_gripper_o3d's) at the grasp, and over everything they
pass through on the approach.  include/gnr.h states the arithmetic; the results are the bits of the float64 statement
tests/hand_reference.py.  No reference counterpart."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .grasp_post import HAND_GEOMETRY, DeviceOp, checked_params, volume_batch

HAND_DEFAULTS = dict(HAND_GEOMETRY, opening=None, spacing=0.5, approach=0.05)
PLAN_DEFAULTS = dict(level=0.0)                              # what a plan adds: collision_free = approach_clearance > level
EXECUTE_GRASP_OPENING = 0.08                                 # execute_grasp opens the hand to max_opening_width (simulation.py:372)


def hand_params(clearance, **more):
    """A plan's `clearance` / a session's `hand_clearance` argument -> None, or the hand's parameters (True / {}: the viewer's hand of
    draw_gripper_o3d opened to each grasp's own predicted width, samples half a voxel apart, a 5 cm approach, collision_free =
    approach_clearance > 0).  more: further keys the caller takes, with their defaults (plan_real's `filter`)."""
    out = checked_params('clearance', clearance, {**HAND_DEFAULTS, **PLAN_DEFAULTS, **more})
    if out is None:
        return None
    for k in ('height', 'finger_width', 'tail_length', 'depth', 'spacing', 'approach', 'level'):
        out[k] = float(out[k])
    out['opening'] = None if out['opening'] is None else float(out['opening'])
    checked_hand(**{k: out[k] for k in HAND_DEFAULTS})
    return out


def same_hand_params(a, b):
    """Whether two hand_params results ask for the same check (either may hold further keys, plan_real's `filter`)."""
    if a is None or b is None:
        return a is None and b is None
    return all(a[k] == b.get(k) for k in (*HAND_DEFAULTS, *PLAN_DEFAULTS))


def device_params(hp):
    """hand_params -> the keyword arguments of HandClearance.__call__ it sets."""
    return {k: hp[k] for k in HAND_DEFAULTS}


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


class HandClearance(DeviceOp):
    """The clearance of the hand at rows of grasps of B volumes.  The output buffers are kept per shape and written again by the next
    call of that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'hand clearance')
        self._out = {}

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
        d = self.device
        hand = checked_hand(height, finger_width, tail_length, depth, opening, spacing, approach)
        vol, B, R = volume_batch(vol, d)
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
        out = self._out.get((B, n))
        if out is None:
            out = self._out[(B, n)] = (torch.zeros(B, n, 2, dtype=torch.float32, device=d), torch.zeros(B, n, 2, dtype=torch.int32, device=d),
                                       torch.zeros(B, n, 2, dtype=torch.int32, device=d))
        p = _lib.GnrHandParams(scale=float(scale), **hand)
        rc = self.L.gnr_hand_clearance_fwd(C.byref(p), vol.data_ptr(), pos.data_ptr(), quat.data_ptr(), width.data_ptr(), count.data_ptr(),
                                           count.numel() // B, B, R, n, int(top_k or 0), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                           self._stream())
        _lib.check(rc, 'gnr_hand_clearance_fwd')
        return dict(zip(('clearance', 'worst', 'inside'), out))

    def of_selection(self, vol, sel, *, scale, **hand):
        """... of the rows of a GraspSelector result (any route's: plan, plan_real, plan_depth), with its top_k."""
        return self(vol, selection_pos(sel), sel['quat'], sel['width'], sel['count'], scale=scale, top_k=sel.get('top_k'), **hand)


def hand_rows(res, b, n):
    """The device rows of scene b of a HandClearance result, given the number of grasps n the selection stored."""
    return {k: res[k][b, :n] for k in ('clearance', 'worst', 'inside')}


def hand_from_rows(rows, level=0.0):
    """hand_rows on the host (numpy) -> the columns a plan adds to its grasps: `clearance` [n] and `approach_clearance` [n] float32 (the
    volume's units), `hand_inside` [n,2] and `hand_worst` [n,2] int32 (at the grasp, on the approach), `collision_free` [n] bool =
    approach_clearance > level."""
    c = np.asarray(rows['clearance'])
    return {'clearance': c[:, 0].copy(), 'approach_clearance': c[:, 1].copy(), 'hand_inside': np.array(rows['inside']),
            'hand_worst': np.array(rows['worst']), 'collision_free': c[:, 1] > np.float32(level)}
