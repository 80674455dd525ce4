"""Support of the parts, on the device (csrc/gnr_support.hip, gnr_part_contacts_fwd and gnr_part_support_fwd): where two parts of a
label volume touch, which of the two lies on the other there, and the graph that follows.  retreat.GraspRetreat moves one part along
one line; it cannot say that a ball pulled out sideways would have been carrying something, that a part which retreats free is the
only footing of its neighbour, or in which order a pile comes apart without anything falling.  The reference leaves all of that to
physics (remove_and_wait, gd/simulation.py; `while sim.num_objects > 0`, clutter_removal.py:92).
PartContacts counts, per ordered pair of labels, the neighbouring voxel pairs (`touch`) and those where the second label's voxel is the
higher one (`over`), and per label its voxels in the plane z_min (`floor`).  PartSupport says c rests on a when over[a,c] - over[c,a] is
positive and at least `lean` times touch[a,c], and derives per part: `below` (its footings), `above`, `carried` (everything that rests
on it, transitively), `orphans` (the parts that lose every footing when it is taken), `layer` (0: nothing rests on it; ascending
(layer, label) is an order of removal in which nothing taken carries anything) and `grounded`.  include/gnr.h states the rule; the
results are the bits of tests/support_reference.py.
What a caller must know.  Nothing here is dynamics: nothing slides, tips or settles, there are no contact points or normals in metres
and no centre of mass over a footing.  The default lean = 0.25 lies between the 0.0 of every side contact and the 0.83 .. 1.0 of every
resting contact of the synthetic piles of tests/test_part_support.py (a sphere on a box, a ball in the hollow of three, two balls side
by side, one ball leaning on another); it has not been run on a network's volume, which is why every threshold stays a keyword.  The
table is dense: at most 256 parts per scene, and `dropped` says when labels went beyond the rows.
No row of planner.PRODUCTS yet: support_of_plan runs the operators on what plan_real / plan / plan_depth return."""
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
from .retreat import RETREAT_DEFAULTS, GraspRetreat, best_free_per_part, retreat_from_rows, retreat_params, retreat_rows, retreat_steps

SUPPORT_DEFAULTS = dict(lean=0.25, min_contact=1, min_floor=1)
SUPPORT_COLUMNS = ('below', 'above', 'carried', 'orphans', 'layer', 'grounded')                    # per part: [B,P] int32
GRASP_SUPPORT_COLUMNS = dict(part_above='above', part_carried='carried', part_orphans='orphans', part_layer='layer', part_grounded='grounded')
MAX_PARTS = _lib.GNR_SUPPORT_MAX_PARTS


def checked_support(lean=0.25, min_contact=1, min_floor=1):
    """The support's parameters, checked before anything touches the device (the library refuses the same)."""
    if isinstance(lean, bool) or not (math.isfinite(lean) and 0 <= lean <= 1):
        raise ValueError(f'support lean must be finite and in 0..1 (the share of a contact that lies over the other part), got {lean!r}')
    for k, v in (('min_contact', min_contact), ('min_floor', min_floor)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError(f'support {k} must be an integer >= 1, got {v!r}')
    return dict(lean=float(lean), min_contact=int(min_contact), min_floor=int(min_floor))


def support_params(support, **more):
    """A `support` argument -> None (False / None: not asked for), or the support's parameters (True / {}: lean 0.25, one touching
    voxel pair is a contact, one voxel in the floor plane stands on the table).  Unknown keys are a TypeError, and every value is
    checked here, before the device.  more: further keys the caller takes, with their defaults."""
    out = checked_params('support', support, {**SUPPORT_DEFAULTS, **more})
    if out is not None:
        out.update(checked_support(**picked(out, SUPPORT_DEFAULTS)))
    return out


def checked_rows(max_parts):
    """The rows of the tables: an integer in 1..256."""
    if isinstance(max_parts, bool) or int(max_parts) != max_parts or not 1 <= max_parts <= MAX_PARTS:
        raise ValueError(f'support max_parts must be an integer in 1..{MAX_PARTS}, got {max_parts!r}')
    return int(max_parts)


class PartContacts(DeviceOp):
    """The contact tables of B label volumes.  The output tensors are kept per (B, max_parts) and written again by the next call of
    that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'part contacts')
        self._out = {}

    def __call__(self, labels, *, max_parts, connectivity=26, z_min=0):
        """labels [B,R,R,R] int32 (VolumeParts' or VolumeObjects' `labels`, or any; or one [R,R,R]), 2 <= R <= 256: a label < 1 is no
        part;  max_parts: P, the rows of the tables, 1..256;  connectivity 6, 18 or 26: the parts' own;  z_min: the plane whose voxels
        stand on the table (the solid rule's z_min; R: none).
        -> {'pairs': [B,P,P,2] int32 ([..,a-1,b-1,0]: the ordered pairs of neighbouring voxels with labels a, b; [..,1]: those where
        b's voxel is the higher one), 'floor': [B,P] int32 (the voxels of the label in the plane z_min), 'dropped': [B] int32 (the
        ordered pairs with a label beyond P)}, with `max_parts` as given.  The tensors are this object's: the next call with the same
        shape writes them again."""
        d = self.device
        P = checked_rows(max_parts)
        if connectivity not in (6, 18, 26) or isinstance(connectivity, bool):
            raise ValueError(f'support connectivity must be 6, 18 or 26, got {connectivity!r}')
        if isinstance(z_min, bool) or int(z_min) != z_min or z_min < 0:
            raise ValueError(f'support z_min must be an integer >= 0, got {z_min!r}')
        labels, B, R = labels_batch(labels, d)
        if z_min > R:
            raise ValueError(f'support z_min must be in 0..R = {R}, got {z_min!r}')
        out = self._out.get((B, P))
        if out is None:
            out = self._out[(B, P)] = {'pairs': torch.zeros(B, P, P, 2, dtype=torch.int32, device=d), 'floor': torch.zeros(B, P, dtype=torch.int32, device=d),
                                       'dropped': torch.zeros(B, dtype=torch.int32, device=d)}
        p = _lib.GnrContactsParams(connectivity=int(connectivity), max_parts=P, z_min=int(z_min))
        rc = self.L.gnr_part_contacts_fwd(C.byref(p), labels.data_ptr(), B, R, out['pairs'].data_ptr(), out['floor'].data_ptr(),
                                          out['dropped'].data_ptr(), self._stream())
        _lib.check(rc, 'gnr_part_contacts_fwd')
        return dict(out, max_parts=P)


class PartSupport(DeviceOp):
    """The support graph of B contact tables.  The output tensors are kept per (B, max_parts) and written again by the next call of
    that shape, so their addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'part support')
        self._out = {}
        self._contacts = None

    def __call__(self, contacts, count, *, lean=0.25, min_contact=1, min_floor=1, relation=False):
        """contacts: a PartContacts result (`pairs` [B,P,P,2], `floor` [B,P] int32 device tensors);  count [B] int32 device tensor: the
        parts of each scene (VolumeParts' `count`; the parts are the labels 1..min(max(count, 0), P));  lean in [0, 1]: c rests on a
        when over[a,c] - over[c,a] > 0 and >= lean * touch[a,c];  min_contact: fewer touching voxel pairs are no contact;  min_floor: a
        part with at least this many voxels in the floor plane stands on the table;  relation: also the relation itself.
        -> {'below', 'above', 'carried', 'orphans', 'layer', 'grounded': [B,P] int32 (rows beyond the parts: 0, layer -1), 'rests_on':
        [B,P,P] uint8 with relation=True ([..,c-1,a-1]: c rests on a)}, and the contacts' `pairs`, `floor`, `dropped`, `max_parts` as they
        came, `count`, and the three parameters.  The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        q = checked_support(lean, min_contact, min_floor)
        pairs, floor = contacts['pairs'], contacts['floor']
        ok = lambda t, dim: torch.is_tensor(t) and t.dtype == torch.int32 and t.device.type == d.type and t.dim() == dim and t.is_contiguous()
        if not ok(pairs, 4) or not ok(floor, 2):
            raise ValueError('contacts must hold PartContacts\' contiguous int32 device tensors `pairs` [B,P,P,2] and `floor` [B,P]')
        B, P = floor.shape
        checked_rows(P)
        if tuple(pairs.shape) != (B, P, P, 2):
            raise ValueError(f'pairs must be [{B},{P},{P},2], got {tuple(pairs.shape)}')
        if not ok(count, 1) or count.shape[0] != B:
            raise ValueError(f'count must be a contiguous int32 device tensor [{B}]')
        out = self._out.get((B, P))
        if out is None:
            out = self._out[(B, P)] = {k: torch.zeros(B, P, dtype=torch.int32, device=d) for k in SUPPORT_COLUMNS}
        if relation and 'rests_on' not in out:
            out['rests_on'] = torch.zeros(B, P, P, dtype=torch.uint8, device=d)
        p = _lib.GnrSupportParams(max_parts=P, **q)
        rc = self.L.gnr_part_support_fwd(C.byref(p), pairs.data_ptr(), floor.data_ptr(), count.data_ptr(), B, *(out[k].data_ptr() for k in SUPPORT_COLUMNS),
                                         out['rests_on'].data_ptr() if relation else None, self._stream())
        _lib.check(rc, 'gnr_part_support_fwd')
        res = {k: v for k, v in out.items() if relation or k != 'rests_on'}
        res.update({k: contacts[k] for k in ('pairs', 'floor', 'dropped') if k in contacts}, max_parts=P, count=count, **q)
        return res

    def of_parts(self, res, *, connectivity=26, z_min=0, **kw):
        """... of a VolumeParts / VolumeObjects result as it is: PartContacts on its labels with min(its max_parts, 256) rows (this
        object keeps the operator), then the graph with its count.  connectivity: the parts' own;  z_min: the solid rule's."""
        if self._contacts is None:
            self._contacts = PartContacts(self.device)
        rows = min(int(res['max_parts'] if 'max_parts' in res else res['max_objects']), MAX_PARTS)
        return self(self._contacts(res['labels'], max_parts=rows, connectivity=connectivity, z_min=z_min), res['count'], **kw)


def support_rows(res, b, n):
    """The device rows of scene b of a PartSupport result, given the scene's count n: the first min(n, max_parts) rows of every column,
    that corner of the tables, `dropped` and the count."""
    m = max(0, min(int(n), res['floor'].shape[1]))
    out = {k: res[k][b, :m] for k in (*SUPPORT_COLUMNS, 'floor')}
    out.update(pairs=res['pairs'][b, :m, :m], dropped=res['dropped'][b:b + 1], count=res['count'][b:b + 1])
    if 'rests_on' in res:
        out['rests_on'] = res['rests_on'][b, :m, :m]
    return out


def support_from_rows(rows, lean=0.25, min_contact=1, min_floor=1, max_parts=None):
    """support_rows on the host (numpy) -> `rests_on` [n,n] bool ([c-1,a-1]: c rests on a; the device's when the rows hold it, else
    the rule on the host), `touch` [n,n] int32 (for inspection), `floor` [n] int32, `on_floor` [n] bool, `below`, `above`, `carried`,
    `orphans`, `layer` [n] int32 and `grounded` [n] bool.  max_parts: the rows the tables had (for the text of the error).
    Raises when labels went beyond the rows of the tables, or when the scene has more parts than rows."""
    q = checked_support(lean, min_contact, min_floor)
    count, held = int(np.asarray(rows['count']).reshape(-1)[0]), len(np.asarray(rows['floor']))
    dropped = int(np.asarray(rows['dropped']).reshape(-1)[0])
    full = max_parts is not None and int(max_parts) >= MAX_PARTS or held >= MAX_PARTS
    how = f'more than {MAX_PARTS} parts: the support table is dense and does not answer a heap' if full else 'raise max_parts'
    if count > held:
        raise _lib.GnrError(f'{count} parts but the support tables hold {held}: {how}')
    if dropped > 0:
        raise _lib.GnrError(f'{dropped} contacts of labels beyond the {held} rows of the support tables were dropped: {how}')
    pairs = np.asarray(rows['pairs'], np.int32).reshape(held, held, 2)
    touch, over = pairs[..., 0], pairs[..., 1].astype(np.int64)
    if 'rests_on' in rows:
        rests = np.asarray(rows['rests_on']).reshape(held, held) != 0
    else:
        D = over - over.T
        rests = ((touch >= q['min_contact']) & (D > 0) & (D.astype(np.float64) >= np.float64(q['lean']) * touch.astype(np.float64))
                 & ~np.eye(held, dtype=bool)).T
    floor = np.array(np.asarray(rows['floor'], np.int32).reshape(-1))
    out = dict(rests_on=rests, touch=np.array(touch), floor=floor, on_floor=floor >= q['min_floor'])
    out.update({k: np.array(np.asarray(rows[k], np.int32).reshape(-1)) for k in SUPPORT_COLUMNS})
    out['grounded'] = out['grounded'] != 0
    return out


def grasp_support_columns(part_column, support):
    """The `part` column of ranked grasps (the label each hand holds) and the per-part columns of a support (PartSupport's device
    tensors [B,P] with a part column [B,n], or support_from_rows' arrays [n_parts] with a part column [n]) -> per grasp, for the
    part it holds: `part_above`, `part_carried`, `part_orphans` int32 (0 for a hand that holds nothing the rows know), `part_layer`
    int32 (-1), `part_grounded` bool (False).  On device tensors it is a torch.gather: it can be captured."""
    empty = dict(part_above=0, part_carried=0, part_orphans=0, part_layer=-1, part_grounded=0)
    if torch.is_tensor(part_column):
        rows = support['above'].shape[-1]
        known = (part_column >= 1) & (part_column <= rows)
        at = (part_column.clamp(1, max(rows, 1)) - 1).long()
        out = {k: torch.where(known, torch.gather(support[src], -1, at).to(torch.int32), torch.full_like(part_column, empty[k], dtype=torch.int32))
               for k, src in GRASP_SUPPORT_COLUMNS.items()}
        out['part_grounded'] = out['part_grounded'] != 0
        return out
    col = np.asarray(part_column).reshape(-1).astype(np.int64)
    rows = len(np.asarray(support['above']))
    known = (col >= 1) & (col <= rows)
    at = np.clip(col, 1, max(rows, 1)) - 1
    out = {}
    for k, src in GRASP_SUPPORT_COLUMNS.items():
        src = np.asarray(support[src]).astype(np.int32)
        out[k] = np.where(known, src[at] if rows else 0, empty[k]).astype(np.int32)
    out['part_grounded'] = out['part_grounded'] != 0
    return out


def take_order(support):
    """support_from_rows' dict (or any with `layer` [n]) -> the labels sorted by (layer, label), those of layer -1 (a cycle above
    them) left out: an order in which nothing taken has anything resting on it."""
    layer = np.asarray(support['layer']).reshape(-1)
    return [int(i) + 1 for i in sorted(np.flatnonzero(layer >= 0), key=lambda i: (int(layer[i]), int(i)))]


def best_clear_per_part(columns):
    """The columns of ranked grasps (`part` or `object`, `retreat_free`, `part_carried`) -> {label: the index of its first row that
    retreats free and carries nothing}: retreat.best_free_per_part restricted to the rows with part_carried == 0."""
    clear = np.asarray(columns['retreat_free'], bool).reshape(-1) & (np.asarray(columns['part_carried']).reshape(-1) == 0)
    return best_free_per_part({**{k: columns[k] for k in ('part', 'object') if k in columns}, 'retreat_free': clear})


def _plan_support(what, tsdf_vol, grasps, voxel_size, origin, device, params, *more):
    """support_of_plan's chain for operator `what` (the noun of its errors), which takes the keys of the defaults dicts `more` on top.
    -> (parts, columns, the VolumeParts result, the PartSupport result, every parameter, the checked scale)."""
    params = split_params(what, params, SOLID_DEFAULTS, PART_DEFAULTS, HAND_DEFAULTS, RETREAT_DEFAULTS, SUPPORT_DEFAULTS, *more)
    solid = checked_solid(what, **picked(params, SOLID_DEFAULTS))
    q = part_params(picked(params, PART_DEFAULTS))
    hand = picked(params, HAND_DEFAULTS)
    checked_hand(**hand)
    rt = retreat_params(picked(params, RETREAT_DEFAULTS))
    sp = support_params(picked(params, SUPPORT_DEFAULTS))
    scale = checked_scale(voxel_size)
    retreat_steps(rt['retreat'], rt['step'], scale)
    d = torch.device(device)
    vol, B, R = volume_batch(tsdf_vol, d)
    if B != 1:
        raise ValueError(f'{what}_of_plan takes the volume of one scene, got {B}')
    field = VolumeDistance(d)(vol, scale=scale, **solid)
    res = VolumeParts(d)(field['d2_free'], **q)
    rows = plan_rows(grasps, voxel_size, d)
    pos, qt, wd, count, n = rows
    gres = GraspObjects(d)(res['labels'], pos, qt, wd, count, scale=scale, **hand)
    rres = GraspRetreat(d).of_parts(res, gres, rows, scale=scale, **rt)
    sres = PartSupport(d).of_parts(res, connectivity=q['connectivity'], z_min=solid['z_min'], relation=True, **sp)
    found = int(res['count'][0].item())
    parts = parts_from_rows(_host(parts_rows(res, 0, found)), scale, origin)
    parts['labels'] = res['labels'][0].cpu().numpy()
    parts.update(support_from_rows(_host(support_rows(sres, 0, found)), max_parts=sres['max_parts'], **sp))
    columns = grasp_parts_from_rows(_host(grasp_objects_rows(gres, 0, n)))
    columns.update(retreat_from_rows(_host(retreat_rows(rres, 0, n))))
    columns.update(grasp_support_columns(columns['part'], parts))
    return parts, columns, res, sres, {**params, **solid, **q}, scale


def support_of_plan(tsdf_vol, grasps, *, voxel_size=PLAN_VOXEL_SIZE, origin=(0.0, 0.0, 0.0), device='cuda:0', **params):
    """The support of a plan: tsdf_vol and the grasps dict as plan_real / plan / plan_depth return them (one scene;
    retreat.retreat_of_plan's conventions and chain).  params: the solid rule's keys (SOLID_DEFAULTS -- z_min must cut the table slab:
    it is the floor plane), PART_DEFAULTS', the hand's (HAND_DEFAULTS), RETREAT_DEFAULTS' and SUPPORT_DEFAULTS'.  VolumeDistance on the
    volume, VolumeParts on its d2_free, GraspObjects on the parts' labels, GraspRetreat on the part each grasp closes on, PartContacts
    on the labels under the parts' connectivity and the solid rule's z_min, PartSupport on its tables.
    -> (parts, columns): retreat_of_plan's, with support_from_rows' fields added to the parts and grasp_support_columns' to the
    columns; take_order(parts) is an order of removal, best_clear_per_part(columns) the best-ranked grasp of every part that comes out
    and carries nothing."""
    return _plan_support('support', tsdf_vol, grasps, voxel_size, origin, device, params)[:2]
