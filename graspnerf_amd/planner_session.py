"""The planner's operating point -- one scene per call (ref: src/nr/main.py:188-209) -- as ONE captured hipGraph from raw
uint8 frames to the selected grasps: device ingest (csrc/gnr_ingest.hip) -> image_encoder / init_net / vis_encoder ->
gnr_prepare -> sample_volume -> HIP grasp head -> process + select (csrc/gnr_post.hip).  The graph holds what the planner
consumes and nothing else: no depth-mean head (renderer.py:732 runs it on every eval forward, the planner drops it), no
render pass, no valid-ratio read-back.  A plan is two pinned host->device copies, one graph replay and one read-back.

Limits: one scene per plan, a fixed view count, frame size and selector parameters per session (forward_scenes is the batched
route); the model's parameters may change between plans (the graph is captured again when they did)."""
import inspect
import time

import numpy as np
import torch

from . import _lib
from .grasp_post import GraspSelector, MeshExtractor, SurfaceExtractor, grasps_from_selection, mesh_bounds, unit_normals
from .ingest import DeviceIngest
from .raycast import RAYCAST_DEFAULTS, VolumeRaycaster

_SELECTOR_DEFAULTS = {k: p.default for k, p in inspect.signature(GraspSelector.__call__).parameters.items()
                      if p.default is not inspect.Parameter.empty}
_SURFACE_DEFAULTS = {k: p.default for k, p in inspect.signature(SurfaceExtractor.__call__).parameters.items()
                     if p.default is not inspect.Parameter.empty and k != 'gradient'}      # (the gradient volume is the session's: surface_normals)
_MESH_DEFAULTS = dict(iso=0.0, max_vertices=None, max_faces=None)
_DEPTH_DEFAULTS = dict(extrinsics=None, intrinsic=None, hw=None, origin=(-0.15 + 0.5 * 0.3 / 40, -0.15 + 0.5 * 0.3 / 40, -0.0503 + 0.5 * 0.3 / 40),
                       **RAYCAST_DEFAULTS)
_SEG = 64                                                    # floats: every camera block starts on a 256-byte boundary


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
    A session built without any of these records the graph it always recorded."""

    def __init__(self, net, n_views, src_hw, img_wh, max_grasps=2048, voxel_size=0.3 / 40, channels=3, warmup=3, deterministic=True,
                 surface=None, surface_normals=False, surface_mesh=None, volume_depth=None, **selector_params):
        cfg = net.nr_net.cfg
        if surface_normals and surface is None:
            raise ValueError('surface_normals=True needs the surface cloud: pass surface=dict(...) ({} for its defaults)')
        if cfg.get('warn_low_valid_ratio', False):
            raise ValueError("graph capture cannot read the valid ratio back on every call: unset cfg['warn_low_valid_ratio']")
        if not cfg.get('sample_volume', False):
            raise ValueError("the planner needs cfg['sample_volume'] = True")
        unknown = sorted(set(selector_params) - set(_SELECTOR_DEFAULTS))
        if unknown:
            raise TypeError(f'unknown selector parameters {unknown}; GraspSelector takes {sorted(_SELECTOR_DEFAULTS)}')
        if surface is not None:
            unknown = sorted(set(surface) - set(_SURFACE_DEFAULTS))
            if unknown:
                raise TypeError(f'unknown surface parameters {unknown}; SurfaceExtractor takes {sorted(_SURFACE_DEFAULTS)}')
        if surface_mesh is not None:
            unknown = sorted(set(surface_mesh) - set(_MESH_DEFAULTS))
            if unknown:
                raise TypeError(f'unknown surface_mesh parameters {unknown}; it takes {sorted(_MESH_DEFAULTS)}')
        if volume_depth is not None:
            unknown = sorted(set(volume_depth) - set(_DEPTH_DEFAULTS))
            if unknown:
                raise TypeError(f'unknown volume_depth parameters {unknown}; it takes {sorted(_DEPTH_DEFAULTS)}')
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
        self.selector_params = {**_SELECTOR_DEFAULTS, **selector_params}
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
        self.surface_params = None if surface is None else {**_SURFACE_DEFAULTS, **surface}
        self.surface_normals = bool(surface_normals)
        self.mesh_params = None if surface_mesh is None else {**_MESH_DEFAULTS, **surface_mesh}
        words = 1 + 9 * M + (0 if surface is None else 1) + (0 if surface_mesh is None else 2)
        self._d_out = torch.zeros(words, dtype=torch.int32, device=dev)
        self._h_out = torch.zeros(words, dtype=torch.int32, pin_memory=True)
        self.selection = self.cloud = self.mesh = None
        if surface is not None:
            R = int(cfg['volume_resolution'])
            self.surface = SurfaceExtractor(dev)
            self._surface_rows = R ** 3 if self.surface_params['max_points'] is None else int(self.surface_params['max_points'])
            self._h_surf_index = torch.zeros(self._surface_rows, 3, dtype=torch.int32, pin_memory=True)
            self._h_surf_colors = torch.zeros(self._surface_rows, 3, dtype=torch.float32, pin_memory=True)
            if self.surface_normals:
                self._h_surf_grad = torch.zeros(self._surface_rows, 3, dtype=torch.float32, pin_memory=True)
        if surface_mesh is not None:
            bv, bf = mesh_bounds(int(cfg['volume_resolution']))
            mp = self.mesh_params
            self.mesher = MeshExtractor(dev)
            self._mesh_rows = (bv if mp['max_vertices'] is None else int(mp['max_vertices']), bf if mp['max_faces'] is None else int(mp['max_faces']))
            self._h_mesh_vertices = torch.zeros(self._mesh_rows[0], 3, dtype=torch.float64, pin_memory=True)
            self._h_mesh_faces = torch.zeros(self._mesh_rows[1], 3, dtype=torch.int32, pin_memory=True)
            if self.surface_normals:
                self._h_mesh_grad = torch.zeros(self._mesh_rows[0], 3, dtype=torch.float32, pin_memory=True)
        self.volume_depth_params = None if volume_depth is None else {**_DEPTH_DEFAULTS, **volume_depth}
        self.volume_images = None
        if volume_depth is not None:
            vd = self.volume_depth_params
            self.raycaster = VolumeRaycaster(dev)
            dh, dw = (H, W) if vd['hw'] is None else (int(vd['hw'][0]), int(vd['hw'][1]))
            nv = V if vd['extrinsics'] is None else len(vd['extrinsics'])
            self._depth_hw = (dh, dw)
            # other cameras than the plan's own are the session's: uploaded once
            self._depth_poses = None if vd['extrinsics'] is None else \
                torch.from_numpy(np.ascontiguousarray(np.asarray(vd['extrinsics'], np.float32)[:, :3, :])).to(dev)
            self._depth_Ks = None if vd['intrinsic'] is None else \
                torch.from_numpy(np.repeat(np.asarray(vd['intrinsic'], np.float32).reshape(1, 3, 3), nv, 0)).to(dev)
            self._h_depth = torch.zeros(nv, dh, dw, dtype=torch.float32, pin_memory=True)
            if self.surface_normals:
                self._h_depth_grad = torch.zeros(nv, dh, dw, 3, dtype=torch.float32, pin_memory=True)
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
        self._h['bbox3d'][:] = np.float32([[-0.15, -0.15, -0.0503], [0.15, 0.15, 0.2497]])
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
        if self.surface_params is not None:
            out['surface'] = self.surface(vol, **self.surface_params, **({'gradient': grad} if self.surface_normals else {}))
            o[1 + 9 * M:2 + 9 * M].copy_(out['surface']['count'])
        if self.mesh_params is not None:
            at = 1 + 9 * M + (0 if self.surface_params is None else 1)
            out['mesh'] = self.mesher(vol, **self.mesh_params, scale=(self.surface_params or _SURFACE_DEFAULTS)['scale'],
                                      **({'gradient': grad} if self.surface_normals else {}))
            o[at:at + 2].copy_(out['mesh']['count'].reshape(-1))
        if self.volume_depth_params is not None:
            vd = self.volume_depth_params
            poses = self._d['poses'] if self._depth_poses is None else self._depth_poses
            Ks = self._d['Ks'] if self._depth_Ks is None else self._depth_Ks
            if Ks.shape[0] != poses.shape[0]:                # the plan's own intrinsics (one per view, all equal on this route) for other cameras
                Ks = Ks[:1].expand(poses.shape[0], 3, 3)
            out['volume_depth'] = self.raycaster(vol, poses, Ks, self._depth_hw, origin=vd['origin'], scale=self.voxel_size, iso=vd['iso'],
                                                 step=vd['step'], bisections=vd['bisections'],
                                                 **({'gradient': grad} if self.surface_normals else {}))
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
        was = torch.backends.cudnn.deterministic             # read when a convolution picks its solver: warm-up and capture
        torch.backends.cudnn.deterministic = was or self.deterministic
        try:
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s), torch.no_grad():
                for _ in range(max(self.warmup, 1)):         # builds HotPath / GraspHead / the workspaces, re-packs moved weights
                    self._forward()
            torch.cuda.current_stream(self.device).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(g):
                out = self._forward()
        finally:
            torch.backends.cudnn.deterministic = was
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
        at = 1 + 9 * self.max_grasps
        count = nv = nf = None
        if self.surface_params is not None:
            count, at = int(h[at]), at + 1
            if count > self._surface_rows:
                raise _lib.GnrError(f'{count} surface voxels but the buffers hold {self._surface_rows}: raise surface max_points')
            sp, surf = self.surface_params, self._out['surface']
            self._h_surf_index[:count].copy_(surf['index'][0, :count], non_blocking=True)
            if sp['color'] is None:
                self._h_surf_colors[:count].copy_(surf['colors'][0, :count], non_blocking=True)
            if self.surface_normals:
                self._h_surf_grad[:count].copy_(surf['gradient'][0, :count], non_blocking=True)
        if self.mesh_params is not None:
            nv, nf = int(h[at]), int(h[at + 1])
            if nv > self._mesh_rows[0] or nf > self._mesh_rows[1]:
                raise _lib.GnrError(f'{nv} mesh vertices and {nf} triangles but the buffers hold {self._mesh_rows[0]} and '
                                    f'{self._mesh_rows[1]}: raise surface_mesh max_vertices / max_faces')
            mesh = self._out['mesh']
            self._h_mesh_vertices[:nv].copy_(mesh['vertices'][0, :nv], non_blocking=True)
            self._h_mesh_faces[:nf].copy_(mesh['faces'][0, :nf], non_blocking=True)
            if self.surface_normals:
                self._h_mesh_grad[:nv].copy_(mesh['gradient'][0, :nv], non_blocking=True)
        if self.volume_depth_params is not None:
            self._h_depth.copy_(self._out['volume_depth']['depth'][0], non_blocking=True)
            if self.surface_normals:
                self._h_depth_grad.copy_(self._out['volume_depth']['gradient'][0], non_blocking=True)
        st.synchronize()
        if self.volume_depth_params is not None:
            self.volume_images = {'volume_depth': self._h_depth.numpy().copy()}
            if self.surface_normals:
                g = self._h_depth_grad.numpy()
                self.volume_images['volume_depth_normals'] = unit_normals(g).reshape(g.shape)
        if count is not None:
            index = self._h_surf_index[:count].numpy().astype(np.int64)
            colors = self._h_surf_colors[:count].numpy().astype(np.float64) if sp['color'] is None else \
                np.array([sp['color']], np.float64).repeat(count, axis=0)
            self.cloud = {'count': count, 'index': index, 'points': index.astype(np.float64) * float(sp['scale']), 'colors': colors}
            if self.surface_normals:
                self.cloud['gradient'] = self._h_surf_grad[:count].numpy().copy()
                self.cloud['normals'] = unit_normals(self.cloud['gradient'])
        if nv is not None:
            self.mesh = {'vertices': self._h_mesh_vertices[:nv].numpy().copy(), 'faces': self._h_mesh_faces[:nf].numpy().astype(np.int64)}
            if self.surface_normals:
                self.mesh['gradient'] = self._h_mesh_grad[:nv].numpy().copy()
                self.mesh['normals'] = unit_normals(self.mesh['gradient'])

    def plan(self, frames_u8, extrinsics, intrinsics, depth_range=(0.2, 0.8), bbox3d=((-0.15, -0.15, -0.0503), (0.15, 0.15, 0.2497)),
             seed=None, return_volumes=False):
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
        if self.surface_params is not None or self.mesh_params is not None or self.volume_depth_params is not None:
            self._read_rows(h, st)
            dt = time.time() - t0
        grasps = grasps_from_selection(self.selection, 0, self.voxel_size, seed)
        if return_volumes:
            grasps['volumes'] = tuple(self._out[k].cpu().numpy() for k in ('volume', 'qual', 'rot', 'width', 'sel_qual'))
        return grasps, dt
