"""The planner's operating point -- one scene per call (ref: src/nr/main.py:188-209) -- as ONE captured hipGraph from raw
uint8 frames to the selected grasps: device ingest (csrc/gnr_ingest.hip) -> image_encoder / init_net / vis_encoder ->
gnr_prepare -> sample_volume -> HIP grasp head -> process + select (csrc/gnr_post.hip).  The graph holds what the planner
consumes and nothing else: no depth-mean head (renderer.py:732 runs it on every eval forward, the planner drops it), no
render pass, no valid-ratio read-back.  A plan is two pinned host->device copies, one graph replay and one read-back.

Limits: one scene per plan, a fixed view count, frame size and selector parameters per session (forward_scenes is the batched
route); the model's parameters may change between plans (the graph is captured again when they did)."""
import contextlib
import time
import types
import typing

import numpy as np
import torch

from . import _lib
from .grasp_post import SELECTOR_DEFAULTS, SURFACE_DEFAULTS, VIEW_KEYS, GraspSelector, MeshExtractor, SurfaceExtractor, checked_params, \
    grasps_from_selection, mesh_bounds, mesh_from_rows, mesh_params, mesh_rows, picked, surface_from_rows, surface_params, surface_rows
from .hand import CLOSURE_DEFAULTS, CLOSURE_PLAN_DEFAULTS, CLOSURE_ROW_TYPES, HAND_DEFAULTS, HAND_ROW_TYPES, PLAN_DEFAULTS, FingerClosure, \
    HandClearance, closure_from_rows, closure_params, closure_rows, hand_from_rows, hand_params, hand_rows
from .ingest import DeviceIngest
from .raycast import COLOR_KEYS, VolumeRaycaster, depth_params, images_from_rows, raycast_rows, volume_origin
from .surface_color import COLOR_DEFAULTS, SurfaceColorizer, cloud_level, color_params

_SEG = 64                                                    # floats: every camera block starts on a 256-byte boundary
PLAN_BBOX3D = ((-0.15, -0.15, -0.0503), (0.15, 0.15, 0.2497))       # the planner's workspace box (main.py:91): plan()'s default
PLAN_ORIGIN = tuple(volume_origin(PLAN_BBOX3D[0], 0.3 / 40))        # ... and the lattice origin of its volume: the products' default


@contextlib.contextmanager
def deterministic_convolutions(on=True):
    """MIOpen's deterministic solvers for the convolutions that pick their solver inside the block (its default solvers for some of the
    strided layers sum in arrival order); on=False leaves the switch as it is."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = was or on
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


# ---- the optional products of the volume ---------------------------------------------------------------------------------------------
# A product is one further output of a plan, on both routes: a PlannerSession records it into its graph, the eager planner.plan_real runs
# it after its forward.  It states (1) its normalised parameters, its device wrappers and the number of count words it appends to a
# session's packed selection, (2) record(): its device step (it gets the volume, its gradient, the cameras, the float frames and the
# selection), (3) rows(): which device rows of that result belong to one plan (by its own count words, or by the number of stored
# grasps), and shapes(): the most such rows, (4) result(): the plan's numpy dict from those rows on the host -- through the *_rows /
# *_from_rows pair beside its wrapper (grasp_post.py, raycast.py, hand.py).  How the rows reach the host is the route's: a session
# copies them into pinned twins of shapes() and waits once, the eager route reads each product's rows before the next one records.
# The table PRODUCTS below lists them with their keywords; nothing else names a product (a product with `columns` adds columns to the
# grasps, the others join the cloud's dict, under `key` if they have one).
# The view colours (`colors`: a _Colors, or None) are no product of their own: each product colours its own rows in its record(), right
# after the step that makes them, and reads the colours back with them.
class _Pinned:
    """Pinned host twins of the rows a product reads back: name=(shape, dtype)."""

    def __init__(self, **rows):
        self.buf = {k: torch.zeros(*shape, dtype=dtype, pin_memory=True) for k, (shape, dtype) in rows.items()}

    def fetch(self, rows):
        """Device rows -> the heads of their twins, not waited for."""
        self.rows = {k: self.buf[k][:len(v)] for k, v in rows.items()}
        for k, v in rows.items():
            self.rows[k].copy_(v, non_blocking=True)

    def host(self, *kept):
        """The fetched rows as numpy.  kept: the rows the builder hands on as they are -- copied, the next plan rewrites the buffers."""
        return {k: v.numpy().copy() if k in kept else v.numpy() for k, v in self.rows.items()}


def _gradient_rows(normals, *shape):
    return {'gradient': (shape, torch.float32)} if normals else {}


def _view_rows(colors, *shape):
    if colors is None:
        return {}
    return dict(zip(VIEW_KEYS, ((shape + (3,), torch.float32), (shape, torch.float32), (shape, torch.int32))))


class _Colors:
    """What a product needs to colour its rows from the plan's views (surface_color.SurfaceColorizer): the march's parameters, the
    volume's lattice (origin, voxel size) and a colouriser of its own, whose kept buffers are the product's."""

    def __init__(self, params, env):
        self.origin, self.op = params['origin'], SurfaceColorizer(env.dev)
        self.kw = dict(picked(params, COLOR_DEFAULTS), origin=params['origin'], scale=env.voxel_size)

    def points(self, vol, res, key, images, cams, iso):
        """An extractor's result, completed with the view colours of its rows `key` (in the frame with origin 0)."""
        res.update(self.op.points(vol, res[key], res['count'], images, cams['poses'], cams['Ks'], point_offset=self.origin, iso=iso, **self.kw))
        return res


class _Product:
    """params: the product's normalised parameters;  env: what the route knows (dev, R, max_grasps, n_views, hw = the frames' (H, W),
    voxel_size, normals, cloud_scale, lean: a session's, which leaves on the device what the host knows);  paint(): a _Colors of the
    product's own, or None.  words: its count words;  columns: it adds columns to the grasps;  key: where it goes in the cloud's dict
    (None: its keys join the dict's);  kept: the host rows result() hands on as they are;  wrapper: of its device step, self.op;
    painted: it colours its rows, with self.colors."""
    words, columns, key, kept, painted = 0, False, None, (), True

    def __init__(self, params, env, paint):
        self.params, self.env, self.op, self.colors = params, env, self.wrapper(env.dev), paint() if self.painted else None


class _Cloud(_Product):
    """The surface cloud: one count word.  A session reads back the index rows (the colours in value-map mode, the gradient rows with
    normals); the float64 points stay on the device and are recomputed on the host as index * scale, a fixed colour is known on the
    host, and its cloud says its row count."""
    out, attr, words, kept, wrapper = 'surface', 'cloud', 1, ('gradient', *VIEW_KEYS), SurfaceExtractor

    def shapes(self):
        n = self.env.R ** 3 if self.params['max_points'] is None else int(self.params['max_points'])
        return dict(index=((n, 3), torch.int32), colors=((n, 3), torch.float32), **_gradient_rows(self.env.normals, n, 3),
                    **_view_rows(self.colors, n))

    def record(self, vol, grad, cams, images, sel):
        res = self.op(vol, **self.params, gradient=grad)
        if self.colors is not None:                          # occluded below the middle of the cloud's range (0 for the real route's)
            self.colors.points(vol, res, 'points', images, cams, cloud_level(self.params['rg']))
        return res

    def rows(self, res, counts, n_sel):
        rows = surface_rows(res, 0, *counts)
        if self.env.lean:
            del rows['points']
            if self.params['color'] is not None:
                del rows['colors']
        return rows

    def result(self, rows):
        if 'points' in rows:
            return surface_from_rows(rows)
        n = len(rows['index'])
        rows['points'] = rows['index'].astype(np.float64) * float(self.params['scale'])
        if 'colors' not in rows:
            rows['colors'] = np.array([self.params['color']], np.float64).repeat(n, axis=0)
        return {'count': n, **surface_from_rows(rows)}


class _Mesh(_Product):
    """The triangle mesh of the iso-surface, in the cloud's frame (origin 0, the cloud's scale): two count words, vertices and
    triangles; the stored vertex, face (and gradient) rows are read back."""
    out, attr, words, key, kept, wrapper = 'mesh', 'mesh', 2, 'mesh', ('vertices', 'gradient', *VIEW_KEYS), MeshExtractor
    result = staticmethod(mesh_from_rows)

    def shapes(self):
        nv, nf = (b if m is None else int(m) for b, m in zip(mesh_bounds(self.env.R), (self.params['max_vertices'], self.params['max_faces'])))
        return dict(vertices=((nv, 3), torch.float64), faces=((nf, 3), torch.int32), **_gradient_rows(self.env.normals, nv, 3),
                    **_view_rows(self.colors, nv))

    def record(self, vol, grad, cams, images, sel):
        res = self.op(vol, **self.params, scale=self.env.cloud_scale, gradient=grad)
        if self.colors is not None:                          # (the count's stride is 2: vertices, triangles)
            self.colors.points(vol, res, 'vertices', images, cams, self.params['iso'])
        return res

    def rows(self, res, counts, n_sel):
        return mesh_rows(res, 0, *counts)


class _DepthImages(_Product):
    """The ray cast of the volume: no count word, the whole images are read back.  Without cameras of its own it takes the plan's (a
    session's device block, which every plan uploads anyway); other cameras are the product's, uploaded once."""
    out, attr, kept, wrapper = 'volume_depth', 'volume_images', ('depth', *COLOR_KEYS), VolumeRaycaster
    result = staticmethod(images_from_rows)

    def __init__(self, params, env, paint):
        super().__init__(params, env, paint)
        self.hw = env.hw if params['hw'] is None else params['hw']
        self.nv = env.n_views if params['extrinsics'] is None else len(params['extrinsics'])
        up = lambda a: None if a is None else torch.from_numpy(a).to(env.dev)
        self.poses = up(params['extrinsics'])
        self.Ks = up(None if params['intrinsic'] is None else np.repeat(params['intrinsic'][None], self.nv, 0))

    def shapes(self):
        shape = (self.nv, *self.hw)
        color_rows = {} if self.colors is None else dict(zip(COLOR_KEYS, (((*shape, 3), torch.float32), (shape, torch.float32))))
        return dict(depth=(shape, torch.float32), **_gradient_rows(self.env.normals, *shape, 3), **color_rows)

    def record(self, vol, grad, cams, images, sel):
        p = self.params
        poses = cams['poses'] if self.poses is None else self.poses
        Ks = cams['Ks'] if self.Ks is None else self.Ks
        if Ks.shape[0] != poses.shape[0]:                    # the plan's own intrinsics (one per view, all equal on this route) for other cameras
            Ks = Ks[:1].expand(poses.shape[0], 3, 3)
        res = self.op(vol, poses, Ks, self.hw, origin=p['origin'], scale=self.env.voxel_size, iso=p['iso'], step=p['step'],
                        bisections=p['bisections'], gradient=grad)
        if self.colors is not None:                          # the ray cast's own lattice and level; the sources are the plan's views
            res.update(self.colors.op.pixels(vol, res['depth'], poses, Ks, images, cams['poses'], cams['Ks'],
                                             **dict(self.colors.kw, origin=p['origin']), iso=p['iso']))
        return res

    def rows(self, res, counts, n_sel):
        return raycast_rows(res, 0)


class _Hand(_Product):
    """The gripper clearance of the selected grasps (hand.HandClearance): no count word -- its rows are the selection's, sized by the
    selection's count.  It reads the selection, so it comes right after it; positions are voxel indices, the lattice is the volume's."""
    out, attr, columns, painted = 'hand', 'hand', True, False      # columns: one row per stored grasp, merged into the plan's grasps
    wrapper, row_types, rows_of, from_rows = HandClearance, HAND_ROW_TYPES, staticmethod(hand_rows), staticmethod(hand_from_rows)
    device_keys, host_keys = HAND_DEFAULTS, PLAN_DEFAULTS    # the keywords of the wrapper's call and of from_rows among the parameters

    def shapes(self):
        return {k: ((self.env.max_grasps, *tail), dtype) for k, (tail, dtype) in self.row_types.items()}

    def record(self, vol, grad, cams, images, sel):
        return self.op.of_selection(vol, sel, scale=self.env.voxel_size, **picked(self.params, self.device_keys))

    def rows(self, res, counts, n_sel):
        return self.rows_of(res, 0, n_sel)

    def result(self, rows):
        return self.from_rows(rows, **picked(self.params, self.host_keys))


class _Closure(_Hand):
    """The finger closure of the selected grasps (hand.FingerClosure): the same shape of product as _Hand."""
    out, attr = 'closure', 'closure'
    wrapper, row_types, rows_of, from_rows = FingerClosure, CLOSURE_ROW_TYPES, staticmethod(closure_rows), staticmethod(closure_from_rows)
    device_keys, host_keys = CLOSURE_DEFAULTS, CLOSURE_PLAN_DEFAULTS


class Product(typing.NamedTuple):
    """One row of PRODUCTS.  plan_kw: the keyword of planner.plan_real / real_session (None: every plan has it);  session_kw:
    PlannerSession's;  attr: the session attribute with its normalised parameters;  params: argument -> those (None: not asked for);
    noun: what planner.plan_real(session=...) says the session was built for another of (None: its general list names it);  cls: its
    class above (None: it is part of the others);  keep: the bool column of the grasps its plan_real parameter filter=True keeps the
    rows of;  origin: its parameters take the lattice origin of the volume (PLAN_ORIGIN unless given)."""
    plan_kw: typing.Optional[str]
    session_kw: str
    attr: str
    params: typing.Callable
    noun: typing.Optional[str]
    cls: typing.Optional[type]
    keep: typing.Optional[str] = None
    origin: bool = False


PRODUCTS = (                                                 # in the order of a session's count words and copies
    Product('clearance', 'hand_clearance', 'hand_params', hand_params, 'clearance', _Hand, keep='collision_free'),
    Product('closure', 'finger_closure', 'closure_params', closure_params, 'closure', _Closure, keep='held'),
    Product(None, 'surface', 'surface_params', surface_params, None, _Cloud),
    Product('mesh', 'surface_mesh', 'mesh_params', mesh_params, None, _Mesh),
    Product('volume_depth', 'volume_depth', 'volume_depth_params', depth_params, None, _DepthImages, origin=True),
    Product('view_colors', 'view_colors', 'view_color_params', color_params, None, None, origin=True),
)


def product_params(given):
    """PlannerSession's product keywords (absent: not asked for) -> {Product.attr: normalised parameters, or None}."""
    return {t.attr: t.params(given.get(t.session_kw), **({'origin': PLAN_ORIGIN} if t.origin else {})) for t in PRODUCTS}


def build_products(params, **env):
    """product_params -> the list of the products asked for, in the table's order.  env: _Product's, but for cloud_scale."""
    env = types.SimpleNamespace(**env, cloud_scale=(params['surface_params'] or SURFACE_DEFAULTS)['scale'])
    cp = params['view_color_params']
    paint = (lambda: None) if cp is None else (lambda: _Colors(cp, env))
    return [t.cls(params[t.attr], env, paint) for t in PRODUCTS if t.cls is not None and params[t.attr] is not None]


class PlannerSession:
    """PlannerSession(net, n_views, src_hw, img_wh, max_grasps=2048, **selector_params)

    net: GraspNeRF on a ROCm GPU (planner.load_model);  src_hw = (h, w) of the uint8 frames;  img_wh = (W, H) of the network
    input (multiples of 32, main.py:226);  selector_params: keyword arguments of GraspSelector.__call__ (the reference planner
    passes tsdf_thres_high=0.0, tsdf_thres_low=-0.85, main.py:93-94,199);  channels: 3, or 4 for RGBA frames (alpha ignored);
    deterministic: the convolutions of the 2D backbones are recorded with MIOpen's deterministic solvers, so the same frames and
    cameras give the same bits on every replay (its default solvers for some of the strided layers sum in arrival order: an
    eager forward differs from itself by ~1e-5); False records whatever MIOpen picks.
    The real-robot route (planner.plan_real): the selector parameters tsdf_thres_outside / order / top_k, and surface = dict(rg=...,
    bound=..., color=..., max_points=...) (keyword arguments of SurfaceExtractor.__call__; {} for its defaults) adds the surface
    point cloud of the volume to the graph; self.cloud then holds the last plan's cloud (index, points, colors as numpy).  The
    read-back of the cloud is sized by its row count: the counts come with the selection, then ONE copy of the stored index rows
    (and of the colours in value-map mode; a fixed colour is known on the host); the float64 points stay on the device (the graph's
    output `surface`) and are recomputed on the host as index * scale, which is the same float64 product.
    surface_normals=True (needs `surface`): the SDF gradient volume (NeuralRayRenderer.sample_volume_gradient) and the gather of its
    rows at the cloud's voxels are captured in the graph too; the gradient rows are read back in the same sized step as the index
    rows, and self.cloud gains `gradient` [N,3] float32 and `normals` [N,3] float64 (g / |g| on the host).
    surface_mesh = dict(iso=..., max_vertices=..., max_faces=...) ({} for iso = 0 and the exact upper bounds): the triangle mesh of
    the iso-surface of the volume (grasp_post.MeshExtractor) is captured in the graph too, in the cloud's frame (origin 0, the cloud's
    scale); its two counts come with the selection, the stored vertex and face rows in the same sized step as the cloud's rows, and
    self.mesh holds the last plan's mesh (vertices float64, faces int64; with surface_normals=True also `gradient` and `normals` at the
    vertices).
    volume_depth = dict(extrinsics=..., intrinsic=..., hw=..., origin=..., iso=..., step=..., bisections=...) ({} for the defaults): the
    ray cast of the volume (raycast.VolumeRaycaster) is recorded in the graph after sample_volume.  extrinsics [V',3,4] / intrinsic [3,3] /
    hw: the cameras and the image size; None: the plan's own V cameras -- the kernel reads them from the session's device block, which
    every plan uploads anyway -- at the network's image size.  origin: the world position of voxel (0,0,0)'s centre (the default is that
    of plan()'s default box; the spacing is voxel_size).  The images are read back in the cloud's sized step, and self.volume_images
    holds the last plan's: `volume_depth` [V,h,w] float32 (metres, 0: no surface), with surface_normals=True also `volume_depth_normals`
    [V,h,w,3] float64.
    view_colors = dict(step=..., bias=..., cos_min=..., fill=..., origin=...) ({} for the defaults; needs at least one of the products
    above): the colouring of every product's rows from the plan's own frames (surface_color.SurfaceColorizer: the ingested float images
    self.images, the plan's poses and Ks) is recorded in the graph, each right after the product whose rows it reads.  self.cloud and
    self.mesh gain `view_colors` [N,3] float32, `view_weight` [N] float32 and `view_mask` [N] int32 (bit v: view v contributed),
    self.volume_images gains `volume_color` [V',h,w,3] and `volume_color_weight` [V',h,w] float32; they are read back in the same sized
    step as the rows they colour.  origin: the world position of voxel (0,0,0)'s centre and of the cloud's and the mesh's origin (the
    default is that of plan()'s default box).  Occluders are the voxels below the product's own level: the middle of the cloud's range,
    the mesh's iso, the ray cast's iso.
    hand_clearance = dict(height=..., finger_width=..., tail_length=..., depth=..., opening=..., spacing=..., approach=..., level=...) ({}
    for the defaults): the gripper clearance of the stored grasps against the volume (hand.HandClearance: positions are the voxel indices,
    the lattice is the volume's own) is recorded right after the selection.  Its rows are read back sized by the selection's count, and
    plan()'s grasps gain `clearance` and `approach_clearance` [n] float32 (the smallest value of the volume under the hand at the grasp
    and on its approach), `hand_inside` and `hand_worst` [n,2] int32 and `collision_free` [n] bool = approach_clearance > level, through
    the same permutation as the other columns; self.hand holds them in the selection's order.
    finger_closure = dict(level=..., bisections=..., max_opening=..., friction=..., and hand_clearance's hand keys) ({} for the defaults):
    where the fingers stop when the hand closes on the volume (hand.FingerClosure) is recorded right after the selection (and the
    clearance).  plan()'s grasps gain `closed_width` [n], `finger_travel` and `contact_cos` [n,2] float32, `finger_contact` [n,2] int32,
    `grip_cos` [n] float32 and `held` [n] bool (hand.closure_from_rows; with a friction coefficient also `force_closure`), through the
    same permutation; self.closure holds them in the selection's order.
    A session built without any of these records the graph it always recorded."""

    def __init__(self, net, n_views, src_hw, img_wh, max_grasps=2048, voxel_size=0.3 / 40, channels=3, warmup=3, deterministic=True,
                 surface=None, surface_normals=False, surface_mesh=None, volume_depth=None, view_colors=None, hand_clearance=None,
                 finger_closure=None, **selector_params):
        given = dict(locals())                               # (the products' keywords, by name: PRODUCTS' session_kw)
        cfg = net.nr_net.cfg
        if surface_normals and surface is None:
            raise ValueError('surface_normals=True needs the surface cloud: pass surface=dict(...) ({} for its defaults)')
        if cfg.get('warn_low_valid_ratio', False):
            raise ValueError("graph capture cannot read the valid ratio back on every call: unset cfg['warn_low_valid_ratio']")
        if not cfg.get('sample_volume', False):
            raise ValueError("the planner needs cfg['sample_volume'] = True")
        self.selector_params = checked_params('selector', selector_params, SELECTOR_DEFAULTS)
        self.surface_normals = bool(surface_normals)
        params = product_params(given)
        vars(self).update(params)                            # self.surface_params, .mesh_params, ...: Product.attr
        if self.view_color_params is not None and self.surface_params is None and self.mesh_params is None and self.volume_depth_params is None:
            raise ValueError('view_colors needs a product to colour: pass surface=, surface_mesh= or volume_depth=')
        dev = next(net.parameters()).device
        if dev.type != 'cuda':
            raise _lib.GnrError('PlannerSession needs the model on a ROCm GPU; there is no CPU fallback')
        W, H = int(img_wh[0]), int(img_wh[1])
        if H % 32 or W % 32 or channels not in (3, 4):
            raise ValueError('img_wh must be multiples of 32 (main.py:226) and channels 3 or 4')
        self.net, self.device = net, dev
        self.n_views, self.src_hw, self.img_wh, self.channels = int(n_views), (int(src_hw[0]), int(src_hw[1])), (W, H), int(channels)
        self.max_grasps, self.voxel_size, self.warmup = int(max_grasps), float(voxel_size), int(warmup)
        self.deterministic = bool(deterministic)
        self.ingest = DeviceIngest(dev)
        self.selector = GraspSelector(dev, max_grasps=self.max_grasps)
        V, M = self.n_views, self.max_grasps
        # static inputs of the graph and their pinned staging twins: the frames, and one float block for the cameras
        self._d_frames = torch.zeros(V, *self.src_hw, self.channels, dtype=torch.uint8, device=dev)
        self._h_frames = torch.zeros(V, *self.src_hw, self.channels, dtype=torch.uint8, pin_memory=True)
        sizes = (('poses', (V, 3, 4)), ('Ks', (V, 3, 3)), ('depth_range', (V, 2)), ('bbox3d', (2, 3)))
        offs, n = {}, 0
        for k, shp in sizes:
            offs[k] = (n, shp)
            n += -(-int(np.prod(shp)) // _SEG) * _SEG
        self._h_cam = torch.zeros(n, dtype=torch.float32, pin_memory=True)
        self._d_cam = torch.zeros(n, dtype=torch.float32, device=dev)
        view = lambda buf: {k: buf[o:o + int(np.prod(shp))].view(shp) for k, (o, shp) in offs.items()}
        self._h = {k: v.numpy() for k, v in view(self._h_cam).items()}
        self._h_frames_np = self._h_frames.numpy()
        self._d = view(self._d_cam)
        self.images = torch.zeros(V, 3, H, W, dtype=torch.float32, device=dev)       # the ingested frames of the last plan
        # the selection, packed for one read-back: count | index [M,3] | score [M] | quat [M,4] | width [M], 4-byte words
        # (+ the cloud's row count, when the session extracts one; + the mesh's vertex and triangle counts, likewise)
        self.products = build_products(params, dev=dev, R=int(cfg['volume_resolution']), max_grasps=M, n_views=V, hw=(H, W),
                                       voxel_size=self.voxel_size, normals=self.surface_normals, lean=True)
        words = 1 + 9 * M
        for p in self.products:                              # in the order of their count words and of their copies
            p.at, words, p.pinned = words, words + p.words, _Pinned(**p.shapes())
        self._d_out = torch.zeros(words, dtype=torch.int32, device=dev)
        self._h_out = torch.zeros(words, dtype=torch.int32, pin_memory=True)
        self.selection = None
        vars(self).update({t.cls.attr: None for t in PRODUCTS if t.cls is not None})      # self.cloud, .mesh, ...: the last plan's
        self.captures = 0
        self._set_example_cameras()
        self._capture()

    # ---- capture -----------------------------------------------------------------------------------------------
    def _set_example_cameras(self):
        """Well-formed cameras for the warm-up runs (a zero intrinsic matrix would divide by zero in the projections)."""
        from .synth import ring_cameras
        W, H = self.img_wh
        self._h['poses'][:] = ring_cameras(self.n_views).astype(np.float32)[:, :3, :]
        self._h['Ks'][:] = np.float32([[0.7 * W, 0, 0.5 * W], [0, 0.7 * W, 0.5 * H], [0, 0, 1]])
        self._h['depth_range'][:] = np.float32([0.2, 0.8])
        self._h['bbox3d'][:] = np.float32(PLAN_BBOX3D)
        self._d_cam.copy_(self._h_cam)

    def _forward(self):
        nr = self.net.nr_net
        imgs = self.ingest(self._d_frames, self.img_wh, out=self.images)
        ref = {'imgs': imgs, **self._d}
        ref['img_feats'] = nr.image_encoder(imgs)
        ref['ray_feats'] = nr.vis_encoder(nr.init_net(ref, None, False), ref['img_feats'])
        prep = nr._prepare(ref, 0, volume_gradient=True) if self.surface_normals else nr._prepare(ref, 0)
        vol = nr.sample_volume(ref, _prep=prep)
        q, r, w = self.net.grasp_head(vol)
        sel = self.selector(vol, q, r, w, **self.selector_params)
        M, o = self.max_grasps, self._d_out
        o[0:1].copy_(sel['count'])
        o[1:1 + 3 * M].copy_(sel['index'].reshape(-1))
        for k, a, b in (('score', 1 + 3 * M, 1 + 4 * M), ('quat', 1 + 4 * M, 1 + 8 * M), ('width', 1 + 8 * M, 1 + 9 * M)):
            o[a:b].copy_(sel[k].reshape(-1).view(torch.int32))
        out = {'volume': vol, 'qual': q, 'rot': r, 'width': w, 'sel_qual': sel['qual']}
        grad = nr.sample_volume_gradient(ref, _prep=prep) if self.surface_normals else None
        for p in self.products:
            out[p.out] = p.record(vol, grad, self._d, imgs, sel)
            if p.words:
                o[p.at:p.at + p.words].copy_(out[p.out]['count'].reshape(-1))
        return out

    def _state(self):
        """What the captured graph depends on besides its static inputs: the parameter versions and addresses (the packed
        copies of the hot path and of the grasp head are re-uploaded when they move -- outside a capture) and the addresses
        of the workspaces those two keep (another caller's larger shape re-allocates them)."""
        nr, head = self.net.nr_net, self.net._head
        hot = nr._hot
        ptr = lambda t: None if t is None else t.data_ptr()
        return (tuple((p._version, p.data_ptr()) for p in self._params), hot, head,
                None if hot is None else (ptr(hot._ws), ptr(hot.wc), hot.options), None if head is None else (ptr(head._ws), ptr(head.w)))

    def _capture(self):
        self._params = list(self.net.parameters())
        self.graph = self._out = None                        # the previous capture's pool goes back first
        with deterministic_convolutions(self.deterministic):  # read when a convolution picks its solver: warm-up and capture
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s), torch.no_grad():
                for _ in range(max(self.warmup, 1)):         # builds HotPath / GraspHead / the workspaces, re-packs moved weights
                    self._forward()
            torch.cuda.current_stream(self.device).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(g):
                out = self._forward()
        self.graph, self._out, self._captured = g, out, self._state()
        self.captures += 1

    # ---- one plan ----------------------------------------------------------------------------------------------
    def _stage_frames(self, frames):
        if torch.is_tensor(frames) and frames.is_cuda:       # frames that are on the device already: no staging
            if frames.dtype != torch.uint8 or tuple(frames.shape) != tuple(self._d_frames.shape):
                raise ValueError(f'frames must be uint8 {tuple(self._d_frames.shape)}, got {frames.dtype} {tuple(frames.shape)}')
            self._d_frames.copy_(frames, non_blocking=True)
            return
        if isinstance(frames, (list, tuple)):
            if len(frames) != self.n_views:
                raise ValueError(f'this session takes {self.n_views} frames, got {len(frames)}')
            frames = [np.asarray(f) for f in frames]
        else:
            frames = np.asarray(frames)
            frames = frames[None] if frames.ndim == 3 else frames
        want = self._h_frames_np.shape
        for f in frames:
            if f.dtype != np.uint8 or f.shape != want[1:]:
                raise ValueError(f'this session takes {want[0]} uint8 frames {want[1:]}, got {f.dtype} {f.shape}')
        if len(frames) != want[0]:
            raise ValueError(f'this session takes {want[0]} frames, got {len(frames)}')
        for dst, f in zip(self._h_frames_np, frames):
            np.copyto(dst, f)
        self._d_frames.copy_(self._h_frames, non_blocking=True)

    def _read_rows(self, h, st):
        """The stored rows of the cloud and of the mesh, sized by the counts that came with the selection: one copy of the cloud's index
        (and of its colours in value-map mode, of its gradient rows with normals), one each of the mesh's vertex, face (and gradient)
        rows, the volume's depth images when the session casts them, then one wait."""
        n_sel = min(int(h[0]), self.selector_params['top_k'] or self.max_grasps, self.max_grasps)
        for p in self.products:
            p.pinned.fetch(p.rows(self._out[p.out], h[p.at:p.at + p.words].tolist(), max(n_sel, 0)))
        st.synchronize()
        for p in self.products:
            setattr(self, p.attr, p.result(p.pinned.host(*p.kept)))

    def plan(self, frames_u8, extrinsics, intrinsics, depth_range=(0.2, 0.8), bbox3d=PLAN_BBOX3D, seed=None, return_volumes=False):
        """planner.plan() from raw frames: frames_u8 [V,h,w,c] uint8 (array, list of arrays, or a device tensor);
        extrinsics [V,3|4,4] world->camera; intrinsics [V,3,3] of the RESIZED images; depth_range [2] or [V,2].
        -> (grasps dict: pos, quat, width, score, index (+ volumes); seconds from before the first copy to after the read-back)."""
        if self._state() != self._captured:
            self._capture()
        V = self.n_views
        ext, K = np.asarray(extrinsics, np.float32), np.asarray(intrinsics, np.float32)
        if ext.shape[0] != V or K.shape != (V, 3, 3):
            raise ValueError(f'this session takes {V} views, got extrinsics {ext.shape} and intrinsics {K.shape}')
        st = torch.cuda.current_stream(self.device)
        t0 = time.time()
        self._stage_frames(frames_u8)
        self._h['poses'][:] = ext[:, :3, :]
        self._h['Ks'][:] = K
        self._h['depth_range'][:] = np.asarray(depth_range, np.float32)      # [2] broadcasts over the views
        self._h['bbox3d'][:] = np.asarray(bbox3d, np.float32)
        self._d_cam.copy_(self._h_cam, non_blocking=True)
        self.graph.replay()
        self._h_out.copy_(self._d_out, non_blocking=True)
        st.synchronize()
        dt = time.time() - t0
        M, h = self.max_grasps, self._h_out.clone()          # the staging buffer is rewritten by the next plan
        f = lambda a, b, *shp: h[a:b].view(torch.float32).view(1, M, *shp)
        self.selection = {'count': h[0:1], 'index': h[1:1 + 3 * M].view(1, M, 3), 'score': f(1 + 3 * M, 1 + 4 * M),
                          'quat': f(1 + 4 * M, 1 + 8 * M, 4), 'width': f(1 + 8 * M, 1 + 9 * M),
                          'order': self.selector_params['order'], 'top_k': self.selector_params['top_k']}
        if self.products:
            self._read_rows(h, st)
            dt = time.time() - t0
        grasps = grasps_from_selection(self.selection, 0, self.voxel_size, seed)
        columns = [getattr(self, p.attr) for p in self.products if p.columns]
        if columns:                                          # the hand's columns, through the permutation of the other columns
            n, p = len(grasps['score']), None
            if seed is not None and n > 0:
                np.random.seed(seed)
                p = np.random.permutation(n)
            for cols in columns:
                grasps.update(cols if p is None else {k: v[p] for k, v in cols.items()})
        if return_volumes:
            grasps['volumes'] = tuple(self._out[k].cpu().numpy() for k in ('volume', 'qual', 'rot', 'width', 'sel_qual'))
        return grasps, dt
