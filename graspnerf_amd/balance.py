"""Balance of the parts, on the device (csrc/gnr_balance.hip, gnr_part_feet_fwd and gnr_part_balance_fwd): on which of its voxels a part
stands, whether its centre of mass lies over them, and what tips over when a part is taken.  support.PartSupport's `orphans` counts
the parts that lose every footing; a plank across two pillars keeps one when a pillar is taken, and falls all the same.
PartFeet gives every footing of a part one of eight foot slots (slot 0 is the floor plane; from the seventh footing on they share slot
7 and the part is `crowded`), and counts per part and slot the foot voxels (`feet`) and their `reach` along 16 directions of the
(i, j) plane, and per part the ten integer `moments` up to the second order.  PartBalance says a part is `balanced` when its centre of
mass lies inside the hull of its feet's unit squares along all 16 directions, by `margin` voxels, and per part `a` which parts tip
when it is taken (`tips`: those that rest on it and are not balanced on their other slots; `unsettles`: how many) and `falls`: they
and everything they carry.  falls >= orphans, part by part.  include/gnr.h states the rule; the results are the bits of
tests/balance_reference.py.
What a caller must know.  It is the statics of each part's own mass: what a part carries does not shift its balance point, and
nothing slides or rotates.  A part on a single floor voxel reads a margin of 0.5 -- voxelised balls do that.  Under connectivity 18 or
26 a foot voxel may overhang its footing by one diagonal; connectivity 6 gives the strict footprint.  There is no threshold of its
own: integer geometry plus the support's min_floor.  It has not been run on a network's volume.
No row of planner.PRODUCTS, no plan_real keyword and no session keyword yet: balance_of_plan runs the operators on what plan_real /
plan / plan_depth return."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .grasp_post import DeviceOp, _host, checked_params, labels_batch, picked
from .objects import PLAN_VOXEL_SIZE
from .support import _plan_support, best_clear_per_part

BALANCE_DEFAULTS = dict(min_floor=1)                                           # the support's
FEET_TABLES = dict(moments=((10,), torch.int64), feet=((_lib.GNR_BALANCE_SLOTS,), torch.int32),
                   reach=((_lib.GNR_BALANCE_SLOTS, _lib.GNR_BALANCE_DIRECTIONS), torch.int32), crowded=((), torch.int32))      # per part: [B,P,..]
BALANCE_COLUMNS = ('balanced', 'margin', 'unsettles', 'falls')                 # per part: [B,P] int32, margin float64
GRASP_BALANCE_COLUMNS = dict(part_margin='margin', part_balanced='balanced', part_unsettles='unsettles', part_falls='falls')
MAX_PARTS = _lib.GNR_BALANCE_MAX_PARTS


def checked_balance(min_floor=1):
    """The balance's parameter, checked before anything touches the device (the library refuses the same)."""
    if isinstance(min_floor, bool) or int(min_floor) != min_floor or min_floor < 1:
        raise ValueError(f'balance min_floor must be an integer >= 1, got {min_floor!r}')
    return dict(min_floor=int(min_floor))


def balance_params(balance, **more):
    """A `balance` argument -> None (False / None: not asked for), or the balance's parameters (True / {}: one voxel in the floor
    plane stands on the table).  Unknown keys are a TypeError, and every value is checked here, before the device.  more: further keys
    the caller takes, with their defaults."""
    out = checked_params('balance', balance, {**BALANCE_DEFAULTS, **more})
    if out is not None:
        out.update(checked_balance(**picked(out, BALANCE_DEFAULTS)))
    return out


def checked_feet(max_parts, connectivity=26, z_min=0, R=None):
    """The feet's parameters: the rows of the tables, an integer in 1..256; the parts' connectivity; the floor plane, in 0..R once R
    is known."""
    if isinstance(max_parts, bool) or int(max_parts) != max_parts or not 1 <= max_parts <= MAX_PARTS:
        raise ValueError(f'balance max_parts must be an integer in 1..{MAX_PARTS}, got {max_parts!r}')
    if connectivity not in (6, 18, 26) or isinstance(connectivity, bool):
        raise ValueError(f'balance connectivity must be 6, 18 or 26, got {connectivity!r}')
    if isinstance(z_min, bool) or int(z_min) != z_min or z_min < 0:
        raise ValueError(f'balance z_min must be an integer >= 0, got {z_min!r}')
    if R is not None and z_min > R:
        raise ValueError(f'balance z_min must be in 0..R = {R}, got {z_min!r}')
    return dict(max_parts=int(max_parts), connectivity=int(connectivity), z_min=int(z_min))


def _is(t, dtype, device, dim):
    return torch.is_tensor(t) and t.dtype == dtype and t.device.type == device.type and t.dim() == dim and t.is_contiguous()


def _checked_relation(rests_on, count, d):
    """rests_on [B,P,P] uint8 and count [B] int32, contiguous device tensors -> (B, P)."""
    if not _is(rests_on, torch.uint8, d, 3) or rests_on.shape[1] != rests_on.shape[2]:
        raise ValueError('rests_on must be a contiguous uint8 device tensor [B,P,P] (PartSupport\'s, with relation=True)')
    B, P = rests_on.shape[:2]
    checked_feet(P)
    if not _is(count, torch.int32, d, 1) or count.shape[0] != B:
        raise ValueError(f'count must be a contiguous int32 device tensor [{B}]')
    return B, P


class PartFeet(DeviceOp):
    """The foot tables of B label volumes under B relations.  The output tensors are kept per (B, max_parts) and written again by the
    next call of that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'part feet')
        self._out = {}

    def __call__(self, labels, rests_on, count, *, connectivity=26, z_min=0):
        """labels [B,R,R,R] int32 (VolumeParts' `labels`, or any; or one [R,R,R]), 2 <= R <= 256;  rests_on [B,P,P] uint8 device
        tensor ([..,c-1,a-1] != 0: c rests on a; PartSupport's with relation=True, or any bytes), P in 1..256;  count [B] int32 device
        tensor: the parts of each scene;  connectivity 6, 18 or 26: the parts' own;  z_min: the floor plane (the solid rule's; R: none).
        -> {'moments': [B,P,10] int64 (n, sums of i, j, k, i^2, j^2, k^2, ij, ik, jk per label), 'slots': [B,P,P] uint8 (the foot slot of
        footing a of part c, 0: none), 'feet': [B,P,8] int32, 'reach': [B,P,8,16] int32 (INT32_MIN: no feet), 'crowded': [B,P] int32},
        and `rests_on`, `count`, `max_parts`, `connectivity`, `z_min` as they came.  The tensors are this object's: the next call with
        the same shape writes them again."""
        d = self.device
        B, P = _checked_relation(rests_on, count, d)
        q = checked_feet(P, connectivity, z_min)
        labels, Bl, R = labels_batch(labels, d)
        if Bl != B:
            raise ValueError(f'labels hold {Bl} scene(s), rests_on {B}')
        checked_feet(P, connectivity, z_min, R)
        out = self._out.get((B, P))
        if out is None:
            out = self._out[(B, P)] = {k: torch.zeros(B, P, *shape, dtype=t, device=d) for k, (shape, t) in FEET_TABLES.items()}
            out['slots'] = torch.zeros(B, P, P, dtype=torch.uint8, device=d)
        p = _lib.GnrFeetParams(**q)
        rc = self.L.gnr_part_feet_fwd(C.byref(p), labels.data_ptr(), rests_on.data_ptr(), count.data_ptr(), B, R, out['moments'].data_ptr(),
                                      out['slots'].data_ptr(), out['feet'].data_ptr(), out['reach'].data_ptr(), out['crowded'].data_ptr(), self._stream())
        _lib.check(rc, 'gnr_part_feet_fwd')
        return dict(out, rests_on=rests_on, count=count, **q)


class PartBalance(DeviceOp):
    """The balance of B foot tables.  The output tensors are kept per (B, max_parts) and written again by the next call of that
    shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'part balance')
        self._out = {}
        self._feet = None

    def __call__(self, feet, *, min_floor=1, tips=False):
        """feet: a PartFeet result (`moments`, `slots`, `feet`, `reach`, and the `rests_on` and `count` it was built from), or a dict of
        such contiguous device tensors written by hand;  min_floor: slot 0 is usable with at least this many voxels in the floor plane
        (the support's);  tips: also the table itself.
        -> {'balanced': [B,P] int32, 'margin': [B,P] float64 (voxels; -inf: nothing to stand on), 'unsettles', 'falls': [B,P] int32
        (rows beyond the parts: 0 and -inf), 'tips': [B,P,P] uint8 with tips=True ([..,c-1,a-1]: c tips when a is taken)}, and the feet's
        entries as they came, and min_floor.  The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        q = checked_balance(min_floor)
        B, P = _checked_relation(feet['rests_on'], feet['count'], d)
        for k, (shape, t) in FEET_TABLES.items():
            if k != 'crowded' and (not _is(feet[k], t, d, 2 + len(shape)) or tuple(feet[k].shape) != (B, P, *shape)):
                raise ValueError(f'{k} must be a contiguous {t} device tensor {[B, P, *shape]}')
        if not _is(feet['slots'], torch.uint8, d, 3) or tuple(feet['slots'].shape) != (B, P, P):
            raise ValueError(f'slots must be a contiguous uint8 device tensor {[B, P, P]}')
        out = self._out.get((B, P))
        if out is None:
            out = self._out[(B, P)] = {k: torch.zeros(B, P, dtype=torch.float64 if k == 'margin' else torch.int32, device=d) for k in BALANCE_COLUMNS}
        if tips and 'tips' not in out:
            out['tips'] = torch.zeros(B, P, P, dtype=torch.uint8, device=d)
        p = _lib.GnrBalanceParams(max_parts=P, **q)
        rc = self.L.gnr_part_balance_fwd(C.byref(p), *(feet[k].data_ptr() for k in ('moments', 'feet', 'reach', 'slots', 'rests_on', 'count')), B,
                                         *(out[k].data_ptr() for k in BALANCE_COLUMNS), out['tips'].data_ptr() if tips else None, self._stream())
        _lib.check(rc, 'gnr_part_balance_fwd')
        res = dict(feet)
        res.update({k: v for k, v in out.items() if tips or k != 'tips'}, max_parts=P, **q)
        return res

    def of_support(self, parts_res, support_res, *, connectivity=26, z_min=0, tips=False):
        """... of a VolumeParts result and the PartSupport result of its labels, built with relation=True: PartFeet on the labels under
        the support's relation and count (this object keeps the operator), then the balance with the support's min_floor.
        connectivity: the parts' own;  z_min: the solid rule's -- both as the support was given them."""
        if 'rests_on' not in support_res:
            raise ValueError('the balance needs the support\'s relation: build the PartSupport result with relation=True')
        if self._feet is None:
            self._feet = PartFeet(self.device)
        feet = self._feet(parts_res['labels'], support_res['rests_on'], support_res['count'], connectivity=connectivity, z_min=z_min)
        return self(feet, min_floor=support_res['min_floor'], tips=tips)


def balance_rows(res, b, n):
    """The device rows of scene b of a PartBalance result, given the scene's count n: the first min(n, max_parts) rows of every column
    and table."""
    m = max(0, min(int(n), res['feet'].shape[1]))
    out = {k: res[k][b, :m] for k in (*BALANCE_COLUMNS, *FEET_TABLES)}
    out.update({k: res[k][b, :m, :m] for k in ('slots', 'tips') if k in res})
    return out


def balance_from_rows(rows, scale, origin=(0.0, 0.0, 0.0)):
    """balance_rows on the host (numpy) -> the device's columns: `balanced` [n] bool, `margin` [n] float64 (voxels), `unsettles`, `falls`
    [n] int32, `moments` [n,10] int64, `feet` [n,8] int32, `reach` [n,8,16] int32, `crowded` [n] bool, `slots` [n,n] uint8, `tips` [n,n]
    bool when the rows hold it;  and four conveniences of the host, float64: `margin_m` = margin * scale;  `centre` [n,3] metres =
    origin + (sums / voxels) * scale (objects_from_rows' `centroid`, the same operations);  `covariance` [n,3,3] m^2: the second moments
    about the centre -- the integers exactly, then one division --, with the 1/12 of a voxel's own extent on the diagonal;  `axes`
    [n,3,3] (row r of a part: its r-th principal axis, its largest-magnitude component positive) and `extent` [n,3] = sqrt(12 *
    eigenvalue) metres, in descending order, from numpy.linalg.eigh: a box reads its edge lengths.  A part without voxels reads nan."""
    scale, origin = np.float64(scale), np.asarray(origin, np.float64)
    mom = np.asarray(rows['moments'], np.int64).reshape(-1, 10)
    n = len(mom)
    out = dict(balanced=np.asarray(rows['balanced']).reshape(-1) != 0, margin=np.array(np.asarray(rows['margin'], np.float64).reshape(-1)))
    out.update({k: np.array(np.asarray(rows[k], np.int32).reshape(-1)) for k in ('unsettles', 'falls')})
    out.update(moments=np.array(mom), feet=np.array(np.asarray(rows['feet'], np.int32).reshape(n, _lib.GNR_BALANCE_SLOTS)),
               reach=np.array(np.asarray(rows['reach'], np.int32).reshape(n, _lib.GNR_BALANCE_SLOTS, _lib.GNR_BALANCE_DIRECTIONS)),
               crowded=np.asarray(rows['crowded']).reshape(-1) != 0)
    if 'slots' in rows:
        out['slots'] = np.array(np.asarray(rows['slots'], np.uint8).reshape(n, n))
    if 'tips' in rows:
        out['tips'] = np.asarray(rows['tips']).reshape(n, n) != 0
    out['margin_m'] = out['margin'] * scale
    voxels = mom[:, 0].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        out['centre'] = origin + (mom[:, 1:4].astype(np.float64) / voxels[:, None]) * scale
        m = mom.astype(object)                                                 # (n * sum ij reaches 2^64: Python integers)
        second = {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}
        cov = np.zeros((n, 3, 3), np.float64)
        for (x, y), col in second.items():
            num = m[:, 0] * m[:, col] - m[:, 1 + x] * m[:, 1 + y]
            cov[:, x, y] = cov[:, y, x] = num.astype(np.float64) / (voxels * voxels)
    cov[:, np.arange(3), np.arange(3)] += 1.0 / 12.0
    cov *= scale * scale
    axes, extent = np.full((n, 3, 3), np.nan), np.full((n, 3), np.nan)
    some = mom[:, 0] > 0
    if some.any():
        w, v = np.linalg.eigh(cov[some])                                       # ascending; the columns of v
        ax = np.swapaxes(v, 1, 2)[:, ::-1]
        lead = np.take_along_axis(ax, np.abs(ax).argmax(2)[..., None], 2)
        axes[some], extent[some] = ax * np.where(lead < 0, -1.0, 1.0), np.sqrt(12.0 * np.maximum(w[:, ::-1], 0.0))
    out.update(covariance=cov, axes=axes, extent=extent)
    return out


def grasp_balance_columns(part_column, balance):
    """The `part` column of ranked grasps (the label each hand holds) and the per-part columns of a balance (PartBalance's device
    tensors [B,P] with a part column [B,n], or balance_from_rows' arrays [n_parts] with a part column [n]) -> per grasp, for the part
    it holds: `part_margin` float64 (-inf for a hand that holds nothing the rows know), `part_balanced` bool (False), `part_unsettles`,
    `part_falls` int32 (0).  On device tensors it is a torch.gather: it can be captured."""
    if torch.is_tensor(part_column):
        rows = balance['margin'].shape[-1]
        known = (part_column >= 1) & (part_column <= rows)
        at = (part_column.clamp(1, max(rows, 1)) - 1).long()
        out = {}
        for k, src in GRASP_BALANCE_COLUMNS.items():
            src = balance[src]
            dtype, empty = (torch.float64, -np.inf) if k == 'part_margin' else (torch.int32, 0)
            out[k] = torch.where(known, torch.gather(src.to(dtype), -1, at), torch.full_like(part_column, empty, dtype=dtype))
        out['part_balanced'] = out['part_balanced'] != 0
        return out
    col = np.asarray(part_column).reshape(-1).astype(np.int64)
    rows = len(np.asarray(balance['margin']))
    known = (col >= 1) & (col <= rows)
    at = np.clip(col, 1, max(rows, 1)) - 1
    out = {}
    for k, src in GRASP_BALANCE_COLUMNS.items():
        dtype, empty = (np.float64, -np.inf) if k == 'part_margin' else (np.int32, 0)
        src = np.asarray(balance[src]).astype(dtype)
        out[k] = np.where(known, src[at] if rows else empty, empty).astype(dtype)
    out['part_balanced'] = out['part_balanced'] != 0
    return out


def best_steady_per_part(columns):
    """The columns of ranked grasps (`part` or `object`, `retreat_free`, `part_carried`, `part_falls`) -> {label: the index of its first
    row that retreats free, carries nothing and lets nothing fall}: support.best_clear_per_part restricted to the rows with
    part_falls == 0."""
    steady = np.asarray(columns['retreat_free'], bool).reshape(-1) & (np.asarray(columns['part_falls']).reshape(-1) == 0)
    return best_clear_per_part({**columns, 'retreat_free': steady})


def balance_of_plan(tsdf_vol, grasps, *, voxel_size=PLAN_VOXEL_SIZE, origin=(0.0, 0.0, 0.0), device='cuda:0', **params):
    """The balance of a plan: tsdf_vol and the grasps dict as plan_real / plan / plan_depth return them (one scene;
    support.support_of_plan's conventions, chain and params -- min_floor is the support's), then PartFeet on the parts' labels under the
    support's relation, the parts' connectivity and the solid rule's z_min, and PartBalance on its tables.
    -> (parts, columns): support_of_plan's, with balance_from_rows' fields added to the parts -- its `extent` as `axis_extent`: the
    parts' own `extent` is their box's -- and grasp_balance_columns' to the columns; best_steady_per_part(columns) is the best-ranked
    grasp of every part that comes out, carries nothing and lets nothing fall."""
    parts, columns, res, sres, q, scale = _plan_support('balance', tsdf_vol, grasps, voxel_size, origin, device, params)
    bres = PartBalance(torch.device(device)).of_support(res, sres, connectivity=q['connectivity'], z_min=q['z_min'], tips=True)
    bal = balance_from_rows(_host(balance_rows(bres, 0, parts['count'])), scale, origin)
    bal['axis_extent'] = bal.pop('extent')
    parts.update(bal)
    columns.update(grasp_balance_columns(columns['part'], bal))
    return parts, columns
