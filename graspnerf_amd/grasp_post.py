"""Device-side grasp post-processing: the reference planner's `process` + `select` (ref: src/nr/main.py:23-84) as HIP
kernels (csrc/gnr_post.hip) instead of scipy.ndimage on the host, plus the host-side tail of `GraspNeRFPlanner.__call__`
(main.py:197-209: seeded permutation, voxel -> metric coordinates).  The real-robot route of src/nr/utils/grasp_utils.py and
draw_utils.py is here too: `process` with its three thresholds (GRASP_UTILS_PROCESS), `sim_grasp`'s ranking by score
(order='score', top_k), and the surface point cloud of `extract_surface_points_from_volume` (SurfaceExtractor, write_ply).  The
triangle mesh of the volume's iso-surface (MeshExtractor, csrc/gnr_mesh.hip) has no counterpart in the reference."""
import ctypes as C
import inspect
import math

import numpy as np
import torch

from . import _lib


class DeviceOp:
    """What every wrapper of a libgnr.so entry point keeps: the library, its device, the current stream's pointer and a byte workspace
    that only grows -- a request it already covers never reallocates, so its address is stable for a captured graph once a warm-up call
    has sized it.  noun: what the wrapper does, for the error of a box without a GPU."""

    def __init__(self, device, noun):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.GnrError(f'the HIP {noun} needs a ROCm GPU; there is no CPU fallback')
        self.device = torch.device(device)
        self._ws = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, need):
        """-> (address, bytes) of a workspace of at least `need` bytes."""
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws.data_ptr(), self._ws.numel()


def _lattice_batch(x, device, dtype, noun):
    x = torch.as_tensor(x, dtype=dtype, device=device).contiguous()
    R = x.shape[-1]
    if x.dim() < 3 or tuple(x.shape[-3:]) != (R, R, R) or x.numel() % R ** 3:
        raise ValueError(f'{noun} must be [B,R,R,R], got {tuple(x.shape)}')
    return x, x.numel() // R ** 3, R


def volume_batch(vol, device):
    """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]) -> (contiguous float32 device tensor, B, R)."""
    return _lattice_batch(vol, device, torch.float32, 'vol')


def labels_batch(labels, device):
    """labels [B,R,R,R] (or one [R,R,R]) -> (contiguous int32 device tensor, B, R): objects.VolumeObjects' `labels`."""
    return _lattice_batch(labels, device, torch.int32, 'labels')


def height_batch(height, device):
    """height [B,R,R,R] (or one [R,R,R]) -> (contiguous int32 device tensor, B, R): parts.VolumeParts' input, distance.VolumeDistance's
    `d2_free`."""
    return _lattice_batch(height, device, torch.int32, 'height')


def gradient_batch(gradient, B, R, device):
    """The gradient volume [B,R,R,R,3] of B volumes as a contiguous float32 device tensor; None stays None."""
    if gradient is None:
        return None
    g = torch.as_tensor(gradient, dtype=torch.float32, device=device).contiguous()
    if tuple(g.shape) != (B, R, R, R, 3):
        raise ValueError(f'gradient must be [{B},{R},{R},{R},3], got {tuple(g.shape)}')
    return g


def expand_cameras(a, b, B, V):
    """Two stacks of per-view camera matrices ([..,3,4] poses and [..,3,3] intrinsics, in the caller's order) -> each [B,V,..]: one
    scene's, or one view's, serve all."""
    try:
        return a.expand(B, V, *a.shape[-2:]), b.expand(B, V, *b.shape[-2:])
    except RuntimeError:
        raise ValueError(f'cameras {tuple(a.shape)} / {tuple(b.shape)} do not fit {B} scene(s) of {V} view(s)') from None


def checked_params(what, given, defaults):
    """The parameters of one optional output: None / False -> None (not asked for), True -> the defaults, a dict -> the defaults with
    its entries; a key the defaults do not have is a TypeError that names `what`."""
    if given is None or given is False:
        return None
    given = {} if given is True else dict(given)
    unknown = sorted(set(given) - set(defaults))
    if unknown:
        raise TypeError(f'unknown {what} parameters {unknown}; it takes {sorted(defaults)}')
    return {**defaults, **given}


def same_params(asked, have):
    """Whether a session that holds the parameters `have` serves a plan that asks for `asked` (checked_params results, or what became of
    them): None equals only None; otherwise every key the asker set, `filter` aside (a plan's own business), has an equal value in
    `have`, arrays and sequences compared by value.  `have` may hold further keys (a session's `origin`)."""
    if asked is None or have is None:
        return asked is None and have is None
    plain = (type(None), bool, int, float, str)              # (every plan asks: numpy is for the few values that need it)
    same = lambda x, y: x == y if isinstance(x, plain) and isinstance(y, plain) else np.array_equal(x, y)
    return all(k in have and same(v, have[k]) for k, v in asked.items() if k != 'filter')


def picked(params, defaults):
    """The entries of `params` under the keys of one defaults dict: the keywords of the one call those are the defaults of."""
    return {k: params[k] for k in defaults}


def split_params(what, params, *defaults):
    """The keywords of a call that serves several operators -> every key of the defaults dicts with its value (picked() then takes
    each operator's share); a key none of them has is checked_params' TypeError."""
    return checked_params(what, dict(params), {k: v for d in defaults for k, v in d.items()})


SOLID_DEFAULTS = dict(level=0.0, lower=None, z_min=0)      # the solid rule of the volume operators: lower < v < level and k >= z_min


def checked_solid(what, level, lower, z_min):
    """The solid rule's parameters of operator `what`, checked before anything touches the device (the library refuses the same)
    -> them as float, None or float, int."""
    if not math.isfinite(level):
        raise ValueError(f'{what} level must be finite, got {level!r}')
    if lower is not None and math.isnan(lower):
        raise ValueError(f'{what} lower must be None (no lower bound) or a number, got {lower!r}')
    if isinstance(z_min, bool) or int(z_min) != z_min or z_min < 0:
        raise ValueError(f'{what} z_min must be an integer >= 0, got {z_min!r}')
    return dict(level=float(level), lower=None if lower is None else float(lower), z_min=int(z_min))


def solid_fields(what, q, R, z_min):
    """checked_solid's dict, now that R is known -> the level, lower and z_min fields of the library's parameter struct (z_min: as the
    caller wrote it, for the text)."""
    if q['z_min'] > R:
        raise ValueError(f'{what} z_min must be in 0..R = {R}, got {z_min!r}')
    return dict(level=q['level'], lower=-math.inf if q['lower'] is None else q['lower'], z_min=q['z_min'])


def _call_defaults(cls, *skip):
    return {k: p.default for k, p in inspect.signature(cls.__call__).parameters.items() if p.default is not inspect.Parameter.empty and k not in skip}


VIEW_KEYS = ('view_colors', 'view_weight', 'view_mask')     # what surface_color.SurfaceColorizer.points adds to an extractor's result


def _host(rows):
    return {k: v.cpu().numpy() for k, v in rows.items()}


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage._filters._gaussian_kernel1d (order 0): fp64, radius int(truncate*sigma + .5); centre first."""
    r = int(truncate * float(sigma) + 0.5)
    if r > _lib.GNR_GAUSS_MAX_RADIUS:
        raise ValueError(f'gaussian radius {r} > {_lib.GNR_GAUSS_MAX_RADIUS}')
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w = w / w.sum()
    return r, w[r:]


# the defaults and thresholds of grasp_utils.process (grasp_utils.py:40-68): outside tsdf > 0.1, inside -1 < tsdf < -0.1, widths 0..12
GRASP_UTILS_PROCESS = dict(gaussian_filter_sigma=1.0, min_width=0, max_width=12, tsdf_thres_outside=0.1, tsdf_thres_high=-0.1,
                           tsdf_thres_low=-1)
_ORDERS = {'index': _lib.GNR_SELECT_ORDER_INDEX, 'score': _lib.GNR_SELECT_ORDER_SCORE}


class GraspSelector(DeviceOp):
    """process() + select() for B scenes at once.  Defaults are the reference functions' defaults; the planner passes
    tsdf_thres_high=0, tsdf_thres_low=-0.85 (main.py:93-94,199)."""

    def __init__(self, device='cuda:0', max_grasps=2048):
        super().__init__(device, 'grasp post-processing')
        self.max_grasps = int(max_grasps)

    def __call__(self, tsdf, qual, rot, width, gaussian_filter_sigma=1.0, min_width=1.33, max_width=9.33,
                 tsdf_thres_high=0.5, tsdf_thres_low=1e-3, threshold=0.90, max_filter_size=4, tsdf_thres_outside=None, order='index',
                 top_k=None):
        """tsdf, qual, width [B,1,R,R,R] (or [B,R,R,R]); rot [B,4,R,R,R]  ->  dict of device tensors:
        qual [B,R,R,R] processed quality; count [B]; index [B,max,3] int32; score [B,max]; quat [B,max,4]; width [B,max]
        (entries beyond count[b] are undefined).
        tsdf_thres_outside: the outside threshold when it is not tsdf_thres_high (grasp_utils.py:59-60);  order: 'index' (np.argwhere
        order) or 'score' (descending score over ALL survivors, ties by ascending voxel index; R <= 64);  top_k: store the first
        top_k rows only (count still reports every survivor).  The result carries `order` and `top_k` for grasps_from_selection."""
        if order not in _ORDERS:
            raise ValueError(f"order must be 'index' or 'score', got {order!r}")
        if top_k is not None and int(top_k) < 1:
            raise ValueError(f'top_k must be None or positive, got {top_k!r}')
        d = self.device
        f = lambda a: torch.as_tensor(a, dtype=torch.float32, device=d).contiguous()
        tsdf, qual, rot, width = f(tsdf), f(qual), f(rot), f(width)
        B, R = rot.shape[0], rot.shape[-1]
        assert rot.shape == (B, 4, R, R, R) and tsdf.numel() == qual.numel() == width.numel() == B * R ** 3
        p = _lib.GnrSelectParams()
        p.gauss_radius, w = gaussian_weights(gaussian_filter_sigma)
        for k, v in enumerate(w):
            p.gauss_w[k] = float(v)
        p.tsdf_thres_high, p.tsdf_thres_low = float(tsdf_thres_high), float(tsdf_thres_low)
        p.min_width, p.max_width, p.threshold = float(min_width), float(max_width), float(threshold)
        p.dilate_iterations, p.max_filter_size = 2, int(max_filter_size)
        v2 = tsdf_thres_outside is not None or order != 'index' or top_k is not None
        if v2:
            p2 = _lib.GnrSelectParamsV2()
            p2.select = p
            p2.tsdf_thres_outside = float(tsdf_thres_high if tsdf_thres_outside is None else tsdf_thres_outside)
            p2.order, p2.top_k = _ORDERS[order], int(top_k or 0)
        need = self.L.gnr_grasp_select_v2_workspace_bytes(B, R, _ORDERS[order]) if v2 else self.L.gnr_grasp_select_workspace_bytes(B, R)
        M = self.max_grasps
        out = {'qual': torch.empty(B, R, R, R, device=d), 'count': torch.empty(B, dtype=torch.int32, device=d),
               'index': torch.empty(B, M, 3, dtype=torch.int32, device=d), 'score': torch.empty(B, M, device=d),
               'quat': torch.empty(B, M, 4, device=d), 'width': torch.empty(B, M, device=d)}
        fn, name = (self.L.gnr_grasp_select_v2_fwd, 'gnr_grasp_select_v2_fwd') if v2 else (self.L.gnr_grasp_select_fwd, 'gnr_grasp_select_fwd')
        rc = fn(tsdf.data_ptr(), qual.data_ptr(), rot.data_ptr(), width.data_ptr(), B, R, C.byref(p2 if v2 else p),
                out['qual'].data_ptr(), out['count'].data_ptr(), out['index'].data_ptr(), out['score'].data_ptr(),
                out['quat'].data_ptr(), out['width'].data_ptr(), M, *self._workspace(need), self._stream())
        _lib.check(rc, name)
        out['order'], out['top_k'] = order, None if top_k is None else int(top_k)
        return out


class SurfaceExtractor(DeviceOp):
    """extract_surface_points_from_volume (draw_utils.py:355-377) for B volumes at once, on the device."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'surface extraction')

    def __call__(self, vol, rg=(-0.2, 0.2), bound=(-1, 1), color=(0, 0, 1), scale=0.3 / 40, max_points=None, gradient=None):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R])  ->  dict of device tensors: count [B] voxels with rg[0] < vol < rg[1];
        index [B,max,3] int32 in np.nonzero order; points [B,max,3] float64 = index * scale; colors [B,max,3] float32 (`color`, or
        the value map over `bound` when color is None); entries beyond count[b] are undefined.  max_points=None: R^3, nothing is
        truncated.  The result carries `scale` and `value_map` for surface_from_extraction.
        gradient [B,R,R,R,3] (HotPath.sample_volume_gradient): adds `gradient` [B,max,3] float32, its rows at the cloud's voxels
        gathered on the device (gnr_surface_gradient_fwd); rows beyond count[b] are zero."""
        d = self.device
        vol, B, R = volume_batch(vol, d)
        M = R ** 3 if max_points is None else int(max_points)
        p = _lib.GnrSurfaceParams()
        p.lo, p.hi, p.scale = float(rg[0]), float(rg[1]), float(scale)
        p.color_mode = _lib.GNR_SURFACE_COLOR_VALUE if color is None else _lib.GNR_SURFACE_COLOR_FIXED
        p.color[:] = [float(c) for c in (color or (0, 0, 0))]
        p.bound_a, p.bound_b = float(bound[0]), float(bound[1])
        out = {'count': torch.empty(B, dtype=torch.int32, device=d), 'index': torch.empty(B, M, 3, dtype=torch.int32, device=d),
               'points': torch.empty(B, M, 3, dtype=torch.float64, device=d), 'colors': torch.empty(B, M, 3, device=d)}
        rc = self.L.gnr_surface_points_fwd(vol.data_ptr(), B, R, C.byref(p), out['count'].data_ptr(), out['index'].data_ptr(),
                                           out['points'].data_ptr(), out['colors'].data_ptr(), M,
                                           *self._workspace(self.L.gnr_surface_points_workspace_bytes(B, R)), self._stream())
        _lib.check(rc, 'gnr_surface_points_fwd')
        g = gradient_batch(gradient, B, R, d)
        if g is not None:
            out['gradient'] = torch.zeros(B, M, 3, dtype=torch.float32, device=d)
            rc = self.L.gnr_surface_gradient_fwd(g.data_ptr(), out['index'].data_ptr(), out['count'].data_ptr(), B, R, M,
                                                 out['gradient'].data_ptr(), self._stream())
            _lib.check(rc, 'gnr_surface_gradient_fwd')
        out['scale'], out['value_map'] = float(scale), color is None
        return out


SELECTOR_DEFAULTS = _call_defaults(GraspSelector)
SURFACE_DEFAULTS = _call_defaults(SurfaceExtractor, 'gradient')      # (the gradient volume is the caller's, not a parameter)


def surface_rows(res, b, n):
    """The device rows of scene b of a SurfaceExtractor result, given its count n.  Raises when the buffers held fewer rows than the
    scene has voxels in range."""
    if n > res['index'].shape[1]:
        raise _lib.GnrError(f'{n} surface voxels but the buffers hold {res["index"].shape[1]}: raise max_points')
    return {k: res[k][b, :n] for k in ('index', 'points', 'colors', 'gradient', *VIEW_KEYS) if k in res}


def surface_from_rows(rows):
    """surface_rows on the host (numpy) -> the cloud: `index` [N,3] int64, `points` [N,3] float64 (metres), `colors` [N,3] float64 (what
    open3d's Vector3dVector holds); with `gradient` [N,3] float32 (the device's rows) also `normals` [N,3] float64 = g / |g| computed
    here on the host (the convention of `points` = index * scale); a zero row stays zero.  The view colours of a result that
    SurfaceColorizer.points completed (VIEW_KEYS: `view_colors` [N,3] float32, `view_weight` [N] float32, `view_mask` [N] int32) pass
    as they are."""
    out = {'index': rows['index'].astype(np.int64), 'points': rows['points'], 'colors': rows['colors'].astype(np.float64)}
    if 'gradient' in rows:
        out['gradient'] = rows['gradient']
        out['normals'] = unit_normals(out['gradient'])
    out.update({k: rows[k] for k in VIEW_KEYS if k in rows})
    return out


def surface_from_extraction(res, b=0):
    """Scene b of a SurfaceExtractor result -> numpy dict (surface_from_rows), every row read back."""
    return surface_from_rows(_host(surface_rows(res, b, int(res['count'][b].item()))))


def unit_normals(gradient):
    """[N,3] gradient rows -> float64 g / |g|; a zero row stays zero."""
    g = np.asarray(gradient, np.float64).reshape(-1, 3)
    n = np.linalg.norm(g, axis=1, keepdims=True)
    return np.divide(g, n, out=np.zeros_like(g), where=n > 0)


def mesh_bounds(R):
    """The most vertices and triangles the surface mesh of an [R,R,R] volume can have: one vertex per cell, two triangles per interior
    edge.  (At least one row each: R = 2 has no interior edge and a buffer of no rows is refused.)"""
    return (R - 1) ** 3, max(1, 6 * (R - 1) * (R - 2) ** 2)


class MeshExtractor(DeviceOp):
    """The indexed triangle mesh of the iso-surface vol = iso of B volumes at once, on the device (gnr_surface_mesh_fwd: naive surface
    nets; include/gnr.h has the statement).  No reference counterpart."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'surface mesh')

    def __call__(self, vol, iso=0.0, scale=0.3 / 40, origin=(0.0, 0.0, 0.0), max_vertices=None, max_faces=None, gradient=None):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]), 2 <= R <= 256  ->  dict of device tensors: count [B,2] int32 (vertices,
        triangles: the true totals); vertices [B,max_vertices,3] float64 = origin + (voxel-index position) * scale, one per
        sign-changing cell in ascending cell index; faces [B,max_faces,3] int32, rows of `vertices`, normals towards increasing vol.
        Rows beyond count[b] are undefined.  max_vertices / max_faces = None: the exact upper bounds (mesh_bounds), nothing is
        truncated.  gradient [B,R,R,R,3] (HotPath.sample_volume_gradient): adds `gradient` [B,max_vertices,3] float32, the volume's
        rows interpolated to the vertices like the positions (not normalised)."""
        d = self.device
        vol, B, R = volume_batch(vol, d)
        bv, bf = mesh_bounds(R)
        MV, MF = bv if max_vertices is None else int(max_vertices), bf if max_faces is None else int(max_faces)
        p = _lib.GnrMeshParams()
        p.iso, p.scale = float(iso), float(scale)
        p.origin[:] = [float(c) for c in origin]
        out = {'count': torch.empty(B, 2, dtype=torch.int32, device=d), 'vertices': torch.empty(B, max(MV, 0), 3, dtype=torch.float64, device=d),
               'faces': torch.empty(B, max(MF, 0), 3, dtype=torch.int32, device=d)}
        g = gradient_batch(gradient, B, R, d)
        if g is not None:
            out['gradient'] = torch.empty(B, max(MV, 0), 3, dtype=torch.float32, device=d)
        rc = self.L.gnr_surface_mesh_fwd(vol.data_ptr(), None if g is None else g.data_ptr(), B, R, C.byref(p), out['count'].data_ptr(),
                                         out['vertices'].data_ptr(), out['faces'].data_ptr(),
                                         None if g is None else out['gradient'].data_ptr(), MV, MF,
                                         *self._workspace(self.L.gnr_surface_mesh_workspace_bytes(B, R)), self._stream())
        _lib.check(rc, 'gnr_surface_mesh_fwd')
        return out


MESH_DEFAULTS = dict(iso=0.0, max_vertices=None, max_faces=None)     # what a plan sets of MeshExtractor.__call__: the frame is the cloud's


def surface_params(surface):
    """A session's `surface` argument -> None, or the keyword arguments of SurfaceExtractor.__call__ ({}: its defaults)."""
    return checked_params('surface', surface, SURFACE_DEFAULTS)


def mesh_params(mesh):
    """A plan's `mesh` / a session's `surface_mesh` argument -> None, or the mesh's parameters (True / {}: iso = 0, the exact upper
    bounds)."""
    return checked_params('mesh', mesh, MESH_DEFAULTS)


def mesh_rows(res, b, nv, nf):
    """The device rows of scene b of a MeshExtractor result, given its vertex and triangle counts.  Raises when a buffer held fewer
    rows than the scene has vertices or triangles."""
    if nv > res['vertices'].shape[1]:
        raise _lib.GnrError(f'{nv} mesh vertices but the buffers hold {res["vertices"].shape[1]}: raise max_vertices')
    if nf > res['faces'].shape[1]:
        raise _lib.GnrError(f'{nf} mesh triangles but the buffers hold {res["faces"].shape[1]}: raise max_faces')
    return {k: res[k][b, :nf if k == 'faces' else nv] for k in ('vertices', 'faces', 'gradient', *VIEW_KEYS) if k in res}


def mesh_from_rows(rows):
    """mesh_rows on the host (numpy) -> the mesh: `vertices` [N,3] float64, `faces` [F,3] int64; with `gradient` [N,3] float32 (the
    device's rows) also `normals` [N,3] float64 = g / |g| (unit_normals, as for the cloud); the view colours at the vertices
    (VIEW_KEYS) pass as they are."""
    out = {'vertices': rows['vertices'], 'faces': rows['faces'].astype(np.int64)}
    if 'gradient' in rows:
        out['gradient'] = rows['gradient']
        out['normals'] = unit_normals(out['gradient'])
    out.update({k: rows[k] for k in VIEW_KEYS if k in rows})
    return out


def mesh_from_extraction(res, b=0):
    """Scene b of a MeshExtractor result -> numpy dict (mesh_from_rows), every row read back."""
    return mesh_from_rows(_host(mesh_rows(res, b, *(int(c) for c in res['count'][b].tolist()))))


def write_ply(path, points, colors, normals=None, faces=None):
    """A point cloud as an ASCII PLY 1.0 file (draw_utils.py:382 writes open3d's): x y z as float64, colours in [0, 1] as uchar;
    normals [N,3]: nx ny nz as float64 between them (open3d's property order).  faces [F,3]: the points are a mesh's vertices and
    the file gains `element face F` with `property list uchar int vertex_indices` and a row "3 i j k" per triangle.  Without
    normals and faces the file is what it was before.  The view colours of a plan go in as they are: colors=cloud['view_colors'],
    or a mesh's vertices with colors=mesh['view_colors']."""
    points, colors = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(colors, np.float64).reshape(-1, 3)
    if len(points) != len(colors):
        raise ValueError(f'{len(points)} points but {len(colors)} colours')
    if normals is not None:
        normals = np.asarray(normals, np.float64).reshape(-1, 3)
        if len(normals) != len(points):
            raise ValueError(f'{len(points)} points but {len(normals)} normals')
    if faces is not None:
        faces = np.asarray(faces, np.int64).reshape(-1, 3)
        if len(faces) and (faces.min() < 0 or faces.max() >= len(points)):
            raise ValueError(f'faces name vertices outside 0..{len(points) - 1}')
    rgb = np.clip(np.floor(colors * 255.0 + 0.5), 0, 255).astype(np.uint8)
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\ncomment graspnerf_amd surface cloud\n'
                f'element vertex {len(points)}\nproperty double x\nproperty double y\nproperty double z\n'
                + ('property double nx\nproperty double ny\nproperty double nz\n' if normals is not None else '') +
                'property uchar red\nproperty uchar green\nproperty uchar blue\n'
                + (f'element face {len(faces)}\nproperty list uchar int vertex_indices\n' if faces is not None else '') +
                'end_header\n')
        if normals is None:
            for (x, y, z), (r, g, b) in zip(points.tolist(), rgb.tolist()):
                f.write(f'{x!r} {y!r} {z!r} {r} {g} {b}\n')
        else:
            for (x, y, z), (nx, ny, nz), (r, g, b) in zip(points.tolist(), normals.tolist(), rgb.tolist()):
                f.write(f'{x!r} {y!r} {z!r} {nx!r} {ny!r} {nz!r} {r} {g} {b}\n')
        if faces is not None:
            for i, j, k in faces.tolist():
                f.write(f'3 {i} {j} {k}\n')


# the hand of draw_utils.draw_gripper_o3d (draw_utils.py:429-432), metres: four boxes in the grasp frame of gd/vis.py's draw_grasp -- z the
# approach (the fingers point along +z), y the closing direction, x the hand's thickness
HAND_GEOMETRY = dict(height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05)


def hand_boxes(width, height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05):
    """(lo [3], hi [3]) of the left finger, the right finger, the palm and the tail of a hand opened to `width` metres, in the grasp
    frame: the boxes hand.HandClearance samples (include/gnr.h, gnr_hand_clearance_fwd) and hand_mesh draws."""
    h, f, t, d, w = float(height), float(finger_width), float(tail_length), float(depth), float(width)
    return (((-h / 2, -w / 2 - f, -f), (h / 2, -w / 2, d)), ((-h / 2, w / 2, -f), (h / 2, w / 2 + f, d)),
            ((-h / 2, -w / 2, -f), (h / 2, w / 2, 0.0)), ((-h / 2, -f / 2, -t - f), (h / 2, f / 2, -f)))


def _box_faces():
    """The 12 triangles of a box whose corner 4 i + 2 j + k sits at (x_i, y_j, z_k), 0 the low and 1 the high end: two per side, wound
    counter-clockwise seen from outside."""
    out = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3                      # u x v = +a
        for side in (0, 1):
            quad = []
            for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):  # counter-clockwise about +a
                bits = [0, 0, 0]
                bits[a], bits[u], bits[v] = side, cu, cv
                quad.append(4 * bits[0] + 2 * bits[1] + bits[2])
            quad = quad if side else quad[::-1]
            out += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.array(out, np.int64)


BOX_FACES = _box_faces()


def hand_mesh(grasps, scores=None, opening=None, travel=None, **hand):
    """The gripper mesh of visualize_grasping_3d / draw_gripper_o3d (database.py:260-276, draw_utils.py:408-480) for a list of grasps, on
    the host: grasps = a plan's dict (`pos` [n,3] metres in the cloud's frame, `quat` [n,4] (x, y, z, w), `width` [n] metres);  scores
    [n]: the colour, (score, 0, 1 - score) per vertex as in draw_gripper_o3d (None: the grasps' own `score`);  opening: one opening in
    metres for every hand (None: each grasp's width);  travel [n,2]: metres each finger has moved towards the centre plane -- a plan's
    `finger_travel` (plan_real(closure=True)) draws the fingers where they stopped (None: the open hand);  hand: HAND_GEOMETRY's keys.
    -> {'vertices': [32 n,3] float64, 'faces': [48 n,3] int64, 'colors': [32 n,3] float64}: per grasp the 8 corners of the left finger,
    the right finger, the palm and the tail (hand_boxes; corner 4 i + 2 j + k of a box at (x_i, y_j, z_k)), 12 outward triangles each.
    write_ply(path, m['vertices'], m['colors'], faces=m['faces']) writes it."""
    from .tsdf import rotation_matrix
    geometry = checked_params('hand', hand, HAND_GEOMETRY)
    pos = np.asarray(grasps['pos'], np.float64).reshape(-1, 3)
    quat = np.asarray(grasps['quat'], np.float64).reshape(-1, 4)
    width = np.asarray(grasps['width'], np.float64).reshape(-1)
    n = len(pos)
    if len(quat) != n or len(width) != n:
        raise ValueError(f'{n} positions but {len(quat)} quaternions and {len(width)} widths')
    scores = np.asarray(grasps['score'] if scores is None else scores, np.float64).reshape(-1)
    if len(scores) != n:
        raise ValueError(f'{n} grasps but {len(scores)} scores')
    if travel is not None:
        travel = np.asarray(travel, np.float64)
        if travel.shape != (n, 2):
            raise ValueError(f'travel must be [{n},2], got {travel.shape}')
    corner = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    vertices, faces = np.zeros((n, 32, 3)), np.zeros((n, 48, 3), np.int64)
    for g in range(n):
        M = rotation_matrix(quat[g] / max(np.linalg.norm(quat[g]), 1e-12))
        for b, (lo, hi) in enumerate(hand_boxes(width[g] if opening is None else opening, **geometry)):
            local = np.where(corner == 1, np.array(hi), np.array(lo))
            if travel is not None and b < 2:                 # the left finger closes towards +y, the right one towards -y
                local = local + [0.0, travel[g, 0] if b == 0 else -travel[g, 1], 0.0]
            vertices[g, 8 * b:8 * b + 8] = pos[g] + local @ M.T
            faces[g, 12 * b:12 * b + 12] = BOX_FACES + (32 * g + 8 * b)
    colors = np.repeat(np.stack([scores, np.zeros(n), 1.0 - scores], 1), 32, axis=0)
    return {'vertices': vertices.reshape(-1, 3), 'faces': faces.reshape(-1, 3), 'colors': colors}


def grasps_from_selection(sel, b=0, voxel_size=0.3 / 40, seed=None):
    """Scene b of a GraspSelector result -> numpy dict in the reference's conventions (main.py:79-84,201-209):
    `pos` = voxel index * voxel_size (metres, bbox-local), `quat` normalised (x,y,z,w; scipy Rotation.from_quat),
    `width` in metres, `score`, `index`; permuted with np.random.seed(seed) like the planner when seed is given.
    A result made with top_k holds min(count, top_k) rows by request (ranked: sim_grasp's list, grasp_utils.py:105)."""
    n = int(sel['count'][b].item())
    if sel.get('top_k') is not None:
        n = min(n, sel['top_k'])
    if n > sel['index'].shape[1]:
        # the reference's select() returns EVERY non-maximum-suppression survivor (main.py:70-84); a truncated list (in
        # index order, before the seeded permutation) would silently be a different result
        raise _lib.GnrError(f'{n} grasps selected but the buffers hold {sel["index"].shape[1]}: raise GraspSelector(max_grasps=...)')
    idx = sel['index'][b, :n].cpu().numpy().astype(np.int64)
    quat = sel['quat'][b, :n].cpu().numpy().astype(np.float64)
    quat = quat / np.linalg.norm(quat, axis=1, keepdims=True) if n else quat
    score = sel['score'][b, :n].cpu().numpy()
    width = sel['width'][b, :n].cpu().numpy()
    if seed is not None and n > 0:
        np.random.seed(seed)
        p = np.random.permutation(n)
        idx, quat, score, width = idx[p], quat[p], score[p], width[p]
    return {'index': idx, 'pos': idx.astype(np.float64) * voxel_size, 'quat': quat, 'width': width * voxel_size, 'score': score}
