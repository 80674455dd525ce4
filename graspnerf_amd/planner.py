"""Inference wrapper with the call shape of the reference planner's `core()` (ref: src/nr/main.py:211-253):
numpy images / extrinsics / intrinsics in, (volume, qual, rot, width, seconds) out, and of its `__call__`
(main.py:185-209) from arrays: `plan()` adds the grasp post-processing (`process`, `select`, main.py:23-84) on the
device (graspnerf_amd/grasp_post.py).  Loads reference checkpoints (`network_state_dict`, main.py:153-155) unchanged.
`GraspNeRFPlanner` below is the file-I/O half of the reference class (main.py:87-209: rendered PNGs, camera poses, intrinsics,
fixed depth range -> core -> process/select), with PIL / numpy only.  The simulator / Blender loop that produces those files
is outside the volumetric path and not rebuilt."""
import os
import time

import numpy as np
import torch

from .renderer import GraspNeRF
from .grasp_post import GRASP_UTILS_PROCESS, GraspSelector, grasps_from_selection, same_params
from .ingest import axis_tables
from .planner_session import PLAN_BBOX3D, PRODUCTS, PlannerSession, build_products, deterministic_convolutions, product_params
from .raycast import depth_params as _depth_params, volume_origin            # (_depth_params: the name the tests and tools know)
from .tsdf import create_tsdf, rotation_matrix


def load_model(cfg, checkpoint=None, device='cuda:0', depth_coords_rng='device'):
    """cfg: the reference's yaml as a dict.  checkpoint: path to `model_best.pth` or a state dict."""
    cfg = {**cfg, 'render_rgb': False, 'depth_coords_rng': depth_coords_rng}     # main.py:150: no rendering when grasping
    net = GraspNeRF(cfg)
    if checkpoint is not None:
        sd = torch.load(checkpoint, map_location='cpu') if isinstance(checkpoint, (str, bytes)) else checkpoint
        net.load_state_dict(sd.get('network_state_dict', sd), strict=True)
    return net.to(device).eval()


def full_frame_coords(h, w):
    """Pixel coordinates (x, y) of every pixel of an h x w query frame, row-major, float32 [1,h*w,2] (build_render_imgs_info,
    utils/imgs_info.py:126-135): the query view of the planner's forward and of a validation scene."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return np.stack([xs, ys], -1).reshape(1, -1, 2).astype(np.float32)


def _scene(dev, images, extrinsics, intrinsics, depth_range, bbox3d, que_id=None, coords=None):
    """One scene from arrays, on the device: `ref_imgs_info` alone (que_id None), or the forward's `data` with the query view que_id at
    the pixel coordinates `coords` [1,N,2]."""
    V = len(images)
    t = lambda a: torch.as_tensor(np.array(a, np.float32), device=dev)
    ext, K = np.asarray(extrinsics, np.float32)[:, :3, :], np.asarray(intrinsics, np.float32)
    dr = np.broadcast_to(np.asarray(depth_range, np.float32), (V, 2)) if np.ndim(depth_range) == 1 else np.asarray(depth_range, np.float32)
    ref = {'imgs': t(images), 'poses': t(ext), 'Ks': t(K), 'depth_range': t(dr), 'bbox3d': t(bbox3d)}
    if que_id is None:
        return ref
    que = {'poses': t(ext[que_id])[None], 'Ks': t(K[que_id])[None], 'coords': coords, 'depth_range': t(dr[que_id])[None]}
    return {'step': 0, 'eval': True, 'full_vol': True, 'ref_imgs_info': ref, 'que_imgs_info': que, 'src_imgs_info': dict(ref)}


def core(net, images, extrinsics, intrinsics, depth_range=(0.2, 0.8),
         bbox3d=((-0.15, -0.15, -0.05), (0.15, 0.15, 0.25)), que_id=0):
    """images [V,3,H,W] in [0,1]; extrinsics [V,3|4,4] world->camera; intrinsics [V,3,3]; H, W multiples of 32.
    -> volume [1,1,R,R,R], qual [1,1,40^3], rot [1,4,40^3], width [1,1,40^3] (numpy) and the forward seconds."""
    h, w = images.shape[2:]
    assert h % 32 == 0 and w % 32 == 0                                          # main.py:226
    dev = next(net.parameters()).device
    data = _scene(dev, images, extrinsics, intrinsics, depth_range, bbox3d, que_id, torch.as_tensor(full_frame_coords(h, w), device=dev))
    with torch.no_grad():
        torch.cuda.synchronize(dev)
        t0 = time.time()
        out = net(data)
        torch.cuda.synchronize(dev)                                             # the reference times without a sync (main.py:244-247)
        dt = time.time() - t0
    q, r, wd = out['vgn_pred']
    return out['volume'].cpu().numpy(), q.cpu().numpy(), r.cpu().numpy(), wd.cpu().numpy(), dt


def plan(net, images, extrinsics, intrinsics, depth_range=(0.2, 0.8), bbox3d=PLAN_BBOX3D,
         seed=None, selector=None, tsdf_thres_high=0.0, tsdf_thres_low=-0.85, voxel_size=0.3 / 40, return_volumes=False,
         session=None, tsdf_thres_outside=None, order='index', top_k=None, que_id=0):
    """`GraspNeRFPlanner.__call__` from arrays (main.py:185-209): forward, process + select on the device, seeded
    permutation, voxel -> metric.  -> (grasps dict of numpy arrays: pos, quat, width, score, index; forward seconds).
    session: a PlannerSession of this net -- `images` are then the raw uint8 frames [V,h,w,c] and the whole plan is one replay
    of the session's captured graph (the thresholds and the voxel size are the session's: they must agree with the arguments).
    tsdf_thres_outside, order, top_k: GraspSelector's (the outside threshold of grasp_utils.process, ranking by score, a prefix);
    que_id: the view the one-pixel query render of the eager forward is taken from (the volume does not depend on it)."""
    if session is not None:
        sp = session.selector_params
        if session.net is not net or selector is not None or \
                (sp['tsdf_thres_high'], sp['tsdf_thres_low'], session.voxel_size, sp['tsdf_thres_outside'], sp['order'], sp['top_k']) != \
                (tsdf_thres_high, tsdf_thres_low, voxel_size, tsdf_thres_outside, order, top_k):
            raise ValueError('plan(session=...): the session was built for another net, thresholds or voxel size '
                             '(its GraspSelector is its own: pass no selector)')
        return session.plan(images, extrinsics, intrinsics, depth_range, bbox3d, seed=seed, return_volumes=return_volumes)
    dev = next(net.parameters()).device
    data = _scene(dev, images, extrinsics, intrinsics, depth_range, bbox3d, que_id, torch.zeros(1, 1, 2, device=dev))
    selector = selector or GraspSelector(dev)
    with torch.no_grad():
        torch.cuda.synchronize(dev)
        t0 = time.time()
        out = net(data)
        q, r, wd = out['vgn_pred']
        new = {k: v for k, v in (('tsdf_thres_outside', tsdf_thres_outside), ('top_k', top_k)) if v is not None}
        if order != 'index':                                                      # (a caller's own selector sees today's call otherwise)
            new['order'] = order
        sel = selector(out['volume'], q, r, wd, tsdf_thres_high=tsdf_thres_high, tsdf_thres_low=tsdf_thres_low, **new)
        torch.cuda.synchronize(dev)
        dt = time.time() - t0
    grasps = grasps_from_selection(sel, 0, voxel_size, seed)
    if return_volumes:
        grasps['volumes'] = tuple(x.cpu().numpy() for x in (out['volume'], q, r, wd, sel['qual']))
    return grasps, dt


# ---- the real-robot route (ref: src/nr/utils/grasp_utils.py:119-151) ------------------------------------------------------
REAL_BBOX3D = ((-0.15, -0.15, 0.0), (0.15, 0.15, 0.3))                                                    # grasp_utils.py:123
REAL_DEPTH_RANGE, REAL_QUE_ID, REAL_VOXEL_SIZE = (0.2, 0.8), 3, 0.3 / 40                                  # grasp_utils.py:122,137,146


def real_volume_origin():
    """World position of voxel (0,0,0)'s centre of run_real's volume: the lattice origin of its ray cast."""
    return volume_origin(REAL_BBOX3D[0], REAL_VOXEL_SIZE)


def _asked(given):
    """plan_real's product arguments {Product.plan_kw: argument} -> {Product.attr: normalised parameters, or None} (with `filter`, where
    the product adds columns to the grasps)."""
    return {t.attr: t.params(given[t.plan_kw], **({'filter': False} if t.keep else {})) for t in PRODUCTS if t.plan_kw is not None}


def _session_keywords(asked, surface_rg, normals):
    """_asked -> PlannerSession's keywords for the real route's products: the cloud over surface_rg, `filter` stripped (a plan's own
    business), the real route's lattice origin where a product takes one."""
    kw = dict(surface=dict(rg=tuple(surface_rg)), surface_normals=bool(normals))
    for t in PRODUCTS:
        if asked.get(t.attr) is not None:
            kw[t.session_kw] = {k: v for k, v in asked[t.attr].items() if k != 'filter'}
            if t.origin:
                kw[t.session_kw]['origin'] = tuple(real_volume_origin())
    return kw


def real_session(net, n_views, src_hw, img_wh, order='permuted', top_k=None, surface_rg=(-0.2, 0.2), max_grasps=2048, normals=False, mesh=False,
                 volume_depth=False, view_colors=False, clearance=False, closure=False, **kw):
    """The PlannerSession plan_real(session=...) takes: grasp_utils.process's thresholds, the ranking and the surface cloud, and for
    each of normals, mesh, volume_depth, view_colors, clearance and closure (plan_real's, to be given here as there) that product in
    the graph."""
    kw.update(_session_keywords(_asked(locals()), surface_rg, normals))
    return PlannerSession(net, n_views, src_hw, img_wh, max_grasps=max_grasps, voxel_size=REAL_VOXEL_SIZE,
                          order='score' if order == 'score' else 'index', top_k=top_k, **GRASP_UTILS_PROCESS, **kw)


def plan_real(net, images, extrinsics, intrinsic, *, seed=None, order='permuted', top_k=None, surface_rg=(-0.2, 0.2), session=None,
              normals=False, mesh=False, volume_depth=False, view_colors=False, clearance=False, closure=False):
    """`run_real` (grasp_utils.py:119-151) without its file output: one plan from camera frames.
    images: V >= 4 uint8 frames [h,w,3] (list or array); extrinsics: V world->camera [3|4,4]; intrinsic [3,3], the same for every view.
    run_real's workspace box, depth range (0.2, 0.8) and query view 3; grasp_utils.process's thresholds (GRASP_UTILS_PROCESS),
    select's defaults.  order='permuted': every survivor, permuted (np.random.seed(seed) first when a seed is given; run_real draws
    from the global state);  order='score': ranked by descending score, best first -- with top_k=10 sim_grasp's list
    (grasp_utils.py:105).  session: a real_session of this net for these frames -- the whole plan is then one replay of its graph.
    -> (grasps dict: pos (metres), quat, width, score, index;  scores;  tsdf_vol [R,R,R];
        cloud dict: points [N,3] float64, colors [N,3], index [N,3] of the voxels with surface_rg[0] < tsdf < surface_rg[1];  seconds).
    normals=True: the cloud also carries `gradient` [N,3] float32 -- the rows of the SDF gradient volume at its voxels
    (NeuralRayRenderer.sample_volume_gradient: the reference's summed VJP, world frame) -- and `normals` [N,3] float64 = g / |g|;
    a session must have been built with real_session(normals=True).  The grasps do not depend on the switch.
    mesh=True: the cloud dict gains `mesh` = {vertices [N,3] float64, faces [F,3] int64}: the triangle mesh of the surface tsdf = 0
    (gnr_surface_mesh_fwd, naive surface nets; no counterpart in run_real) in the cloud's own frame -- origin 0, REAL_VOXEL_SIZE per
    voxel, so it overlays `points` -- with triangle normals towards increasing tsdf; with normals=True also `gradient` [N,3] float32 and
    `normals` [N,3] float64 at the vertices.  mesh=dict(iso=..., max_vertices=..., max_faces=...) sets another level or smaller
    buffers; a session must have been built with the same real_session(mesh=...).  Grasps and cloud do not depend on it.
    volume_depth=True: the cloud dict gains `volume_depth` [V,h,w] float32 -- the camera-z depth in metres (0: no surface) of the surface
    tsdf = 0 of the volume seen from the plan's own V cameras at the network's image size (raycast.py over gnr_volume_raycast_fwd; world frame, voxel
    centres at REAL_BBOX3D[0] + (i + 0.5) * REAL_VOXEL_SIZE; `intrinsic` is that of the frames the network sees); with normals=True also
    `volume_depth_normals` [V,h,w,3] float64, unit vectors, zero on a miss.  volume_depth=dict(extrinsics=..., intrinsic=..., hw=...,
    iso=..., step=..., bisections=...) chooses other cameras, another image size or level; a session must have been built with the same
    real_session(volume_depth=...).  Grasps, cloud and mesh do not depend on it.
    view_colors=True: colours from the plan's own frames (surface_color.py over gnr_surface_color_*_fwd; the float frames the network sees, the plan's
    cameras).  The cloud dict gains `view_colors` [N,3] float32 -- per point the mean of the bilinear taps of the views that see it,
    weighted by the cosine between the volume's normal there and the direction to each camera; a view sees a point that projects into
    its image, faces it, and whose way to the camera crosses no voxel below the surface level -- `view_weight` [N] float32 (the sum of
    those cosines; 0: no view, the colour is `fill`) and `view_mask` [N] int32 (bit v: view v contributed); `mesh` (with mesh on) gains
    the same three at its vertices, and with volume_depth on the dict gains `volume_color` [V',h,w,3] and `volume_color_weight` [V',h,w]
    float32 beside `volume_depth`: from other cameras an image-based rendering of the scene.  view_colors=dict(step=..., bias=...,
    cos_min=..., fill=...): the occlusion march's step and its start off the point in voxels (0.5, 1.5), the least cosine (0) and the
    colour without a view (black); a session must have been built with the same real_session(view_colors=...).  `colors` and every
    other key do not depend on it; grasp_post.write_ply takes colors=cloud['view_colors'].
    clearance=True: whether the hand fits where each grasp puts it, answered from the volume (hand.py over gnr_hand_clearance_fwd; execute_grasp,
    gd/simulation.py:369-402, answers it with physics).  The grasps dict gains `clearance` and `approach_clearance` [n] float32 -- the
    smallest tsdf value under the four boxes of draw_gripper_o3d's hand at the grasp, and over everything they pass through on the
    5 cm approach along the grasp's z; 1.0: nothing of the hand is inside the volume -- `hand_inside` and `hand_worst` [n,2] int32 (the
    samples the volume could vouch for and the ordinal of the worst, at the grasp and on the approach) and `collision_free` [n] bool =
    approach_clearance > level.  clearance=dict(height=..., finger_width=..., tail_length=..., depth=..., opening=..., spacing=...,
    approach=..., level=..., filter=...): a real hand's dimensions in metres (the defaults are the viewer's), one opening for every grasp
    (None: each grasp's own width; hand.EXECUTE_GRASP_OPENING is execute_grasp's 0.08), the samples' spacing in voxels, the approach in
    metres, the level (0) -- and filter=True keeps only the collision_free rows of every column, in their order.  A session must have
    been built with the same real_session(clearance=...) (`filter` aside).  No other key depends on it; grasp_post.hand_mesh draws the
    same boxes.
    closure=True: what happens when the hand then closes, answered from the volume (gnr_finger_closure_fwd; execute_grasp closes the fingers
    and check_success asks whether they touch something and the hand stays wider than a tenth of its opening, gd/simulation.py:404,
    465-469).  The grasps dict gains `closed_width` [n] float32 -- the width in metres at which the fingers stop on the surface tsdf =
    level, the number a robot compares with its gripper's read-back; 0: nothing between the fingers -- `finger_travel` [n,2] float32
    (metres each finger moved), `finger_contact` [n,2] int32 (the pad ray that stopped it, -1: none), `contact_cos` [n,2] and `grip_cos`
    [n] float32 (the cosine between the surface normal at each contact and the closing direction, and the smaller of the two; 1: the
    surfaces face each other squarely) and `held` [n] bool = both fingers touch and closed_width > 0.1 * max_opening.
    closure=dict(level=..., bisections=..., max_opening=..., friction=..., filter=..., and clearance's hand keys): the surface level
    (0), the refinement of a contact (4 halvings), check_success's opening (0.08), a friction coefficient mu -- the dict then gains
    `force_closure` [n] bool = grip_cos >= 1 / sqrt(1 + mu^2); no default, the reference sets none -- and filter=True keeps only the
    `held` rows (with clearance=dict(filter=True) too, the rows that pass both).  A session must have been built with the same
    real_session(closure=...) (`filter` aside).  No other key depends on it.  The depth route (plan_depth) has no such switch: on its selection
    call of_selection(vol, sel, scale=size / resolution, level=0.5) of hand.py's closure wrapper by hand, with a volume on the grid's scale
    (tsdf + 1) / 2, whose surface is at 0.5 -- but not get_grid() itself, which is 0 in unseen and far free space and would read as
    solid there: take (tsdf + 1) / 2 where weight > 0 and 1 elsewhere, as tsdf.render_depth does for its ray cast."""
    if order not in ('permuted', 'score'):
        raise ValueError(f"order must be 'permuted' or 'score', got {order!r}")
    asked = _asked(locals())
    ext = np.stack([np.asarray(e, np.float32) for e in extrinsics], 0)                                    # grasp_utils.py:120-122
    V = ext.shape[0]
    if V <= REAL_QUE_ID:
        raise ValueError(f'run_real renders its query from view {REAL_QUE_ID} (grasp_utils.py:137): it needs at least '
                         f'{REAL_QUE_ID + 1} views, got {V}')
    if len(images) != V:
        raise ValueError(f'{len(images)} images but {V} extrinsics')
    Ks = np.repeat(np.asarray(intrinsic, np.float32)[None], V, 0)
    sel_order = 'score' if order == 'score' else 'index'
    if session is not None:
        want = dict(GRASP_UTILS_PROCESS, order=sel_order, top_k=top_k)
        general = 'net, order, top_k, surface range, normals, mesh, volume_depth or view_colors'
        other = [t.noun or general for t in PRODUCTS              # (of the cloud, a plan sets the range alone)
                 if not same_params(asked.get(t.attr, dict(rg=tuple(surface_rg))), getattr(session, t.attr))]
        if session.net is not net or any(session.selector_params[k] != v for k, v in want.items()) or session.voxel_size != REAL_VOXEL_SIZE \
                or bool(normals) != session.surface_normals:
            other.insert(0, general)
        if other:
            raise ValueError(f'plan_real(session=...): the session was built for another {other[0]} (build it with planner.real_session)')
        g, dt = session.plan(images, ext, Ks, REAL_DEPTH_RANGE, REAL_BBOX3D, seed=None, return_volumes=True)
        tsdf_vol = g.pop('volumes')[0]
        results = [(p, getattr(session, p.attr)) for p in session.products]       # (their columns are in g already: the same again)
    else:
        dev = next(net.parameters()).device
        frames = np.stack([np.asarray(f) for f in images], 0)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
            raise ValueError(f'images must be uint8 [V,h,w,3] frames, got {frames.dtype} {frames.shape}')
        imgs = (frames.astype(np.float32) / 255).transpose([0, 3, 1, 2])                                  # color_map_forward, grasp_utils.py:134
        selector = GraspSelector(dev)
        kept = {}                                                 # the device volume and selection of the plan, for the products

        def call(vol, q, r, w, **kw):
            kept['vol'], kept['sel'] = vol, selector(vol, q, r, w, **{**kw, **GRASP_UTILS_PROCESS})
            return kept['sel']
        with deterministic_convolutions():                        # the solvers a PlannerSession records: the same frames, the same bits
            g, dt = plan(net, imgs, ext, Ks, REAL_DEPTH_RANGE, REAL_BBOX3D, seed=None, selector=call, voxel_size=REAL_VOXEL_SIZE,
                         tsdf_thres_high=GRASP_UTILS_PROCESS['tsdf_thres_high'], tsdf_thres_low=GRASP_UTILS_PROCESS['tsdf_thres_low'],
                         order=sel_order, top_k=top_k, return_volumes=True, que_id=REAL_QUE_ID)
        tsdf_vol = g.pop('volumes')[0]
        # the products a real_session would record, on the plan's volume, the frames the network saw and the plan's cameras;  the
        # gradient from the volume's cameras again: the forward keeps no feature maps
        products = build_products(product_params(_session_keywords(asked, surface_rg, normals)), dev=dev, R=tsdf_vol.shape[-1],
                                  max_grasps=selector.max_grasps, n_views=V, hw=frames.shape[1:3], voxel_size=REAL_VOXEL_SIZE,
                                  normals=bool(normals), lean=False)
        grad = _volume_gradient(net, imgs, ext, Ks, dev) if normals else None
        cams = {'poses': torch.as_tensor(ext[:, :3, :], device=dev), 'Ks': torch.as_tensor(Ks, device=dev)}
        seen, results = torch.as_tensor(imgs, device=dev), []
        for p in products:                                        # each one's rows are on the host before the next one records
            res = p.record(kept['vol'], grad, cams, seen, kept['sel'])
            counts = res['count'].reshape(-1).tolist() if p.words else []
            results.append((p, p.result({k: v.cpu().numpy() for k, v in p.rows(res, counts, len(g['score'])).items()})))
    cloud = {}
    for p, out in results:
        (g if p.columns else cloud).update(out if p.key is None else {p.key: out})
    tsdf_vol = np.asarray(tsdf_vol).reshape(tsdf_vol.shape[-3:])
    n = len(g['score'])
    if order == 'permuted' and n > 0:                                                                     # grasp_utils.py:144-147
        if seed is not None:
            np.random.seed(seed)
        p = np.random.permutation(n)
        g = {k: v[p] for k, v in g.items()}
    keep = [g[t.keep] for t in PRODUCTS if t.keep and asked[t.attr] is not None and asked[t.attr]['filter']]
    if keep:
        g = {k: v[np.logical_and.reduce(keep)] for k, v in g.items()}
    return g, g['score'], tsdf_vol, cloud, dt


def _volume_gradient(net, imgs, ext, Ks, dev):
    """The SDF gradient volume [1,R,R,R,3] of run_real's scene from the resized float images (the backbones run again: the eager
    forward of plan() hands back its outputs, not its feature maps; a session computes both in one graph)."""
    nr = net.nr_net
    ref = _scene(dev, imgs, ext, Ks, REAL_DEPTH_RANGE, REAL_BBOX3D)
    with deterministic_convolutions(), torch.no_grad():
        ref['img_feats'] = nr.image_encoder(ref['imgs'])
        ref['ray_feats'] = nr.vis_encoder(nr.init_net(ref, dict(ref), False), ref['img_feats'])
        return nr.sample_volume_gradient(ref)


# ---- the depth route (ref: src/gd/detection.py:13-40, the VGN baseline) ------------------------------------------------------
def plan_depth(head, depth_imgs, intrinsic, extrinsics, size=0.3, resolution=40, seed=None):
    """`VGN.__call__` (detection.py:13-40) from the depth images of `acquire_tsdf` (gd/simulation.py:341-367): TSDF fusion
    (tsdf.create_tsdf) -> grid -> grasp head -> process + select with detection.py's defaults (GraspSelector's own) -> seeded
    permutation, voxel -> metric, all on the device.  head: a grasp_head.GraspHead;  depth_imgs [V,h,w] float32 metres (or uint16);
    intrinsic: 3x3 or an object with fx, fy, cx, cy;  extrinsics: V world->camera transforms, 7-lists [qx,qy,qz,qw,tx,ty,tz] or
    matrices;  resolution: 40, the head's output grid (detection.py:44).
    -> (grasps dict: pos (metres), quat, width, score, index;  scores;  seconds)."""
    dev = head.device
    with torch.no_grad():
        torch.cuda.synchronize(dev)
        t0 = time.time()
        grid = create_tsdf(size, resolution, depth_imgs, intrinsic, extrinsics, device=dev).get_grid()
        q, r, wd = head(grid)
        sel = GraspSelector(dev)(grid, q, r, wd)
        torch.cuda.synchronize(dev)
        dt = time.time() - t0
    grasps = grasps_from_selection(sel, 0, size / resolution, seed)
    return grasps, grasps['score'], dt


# ---- the planner's file I/O (ref: src/nr/main.py:87-209) -----------------------------------------------
BLENDER2OPENCV = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], np.float64)      # main.py:104
SRC_WH = {'vgn_syn': (640, 360)}                                                                          # main.py:100-102


def resize_bilinear_u8(img, wh):
    """cv2.resize(img, wh) for uint8 HxWxC images with its default INTER_LINEAR (main.py:171): half-pixel centres, border
    replication, OpenCV's fixed-point arithmetic (11-bit coefficients, (.. + 2) >> 2 rounding in the vertical pass), no
    anti-aliasing -- PIL's BILINEAR filters when downscaling and gives different pixels.  (cv2 is not in this image: written
    from OpenCV's resize.cpp, checked against float bilinear to 1 LSB in tests/test_planner_io.py.)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    sh, sw = img.shape[:2]
    dw, dh = int(wh[0]), int(wh[1])
    if (dw, dh) == (sw, sh):
        return img.copy()

    x0, x1, a0, a1 = axis_tables(dw, sw)
    y0, y1, b0, b1 = axis_tables(dh, sh)
    src = img.astype(np.int64)
    rows = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]                       # horizontal pass: int, scale 2^11
    s0, s1 = rows[y0], rows[y1]
    out = (((b0[:, None, None] * (s0 >> 4)) >> 16) + ((b1[:, None, None] * (s1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def read_rgb_png(path):
    """skimage.io.imread(path)[:, :, :3] (main.py:169-170) through PIL."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGBA' if im.mode in ('RGBA', 'LA', 'P') else 'RGB'))[:, :, :3].copy()


class _Rotation:
    """The two accessors of scipy's Rotation the reference's callers use on a grasp pose (clutter_removal.py:198-199,
    simulation.execute_grasp): as_quat() (x, y, z, w) and as_matrix()."""

    def __init__(self, quat):
        q = np.asarray(quat, np.float64)
        self._q = q / max(np.linalg.norm(q), 1e-12)

    def as_quat(self):
        return self._q.copy()

    def as_matrix(self):
        return rotation_matrix(self._q)


class _Pose:
    def __init__(self, quat, translation):
        self.rotation, self.translation = _Rotation(quat), np.asarray(translation, np.float64)


class Grasp:
    """gd.grasp.Grasp(Transform(Rotation, t), width) as the planner's callers read it (main.py:79-84, 205;
    clutter_removal.py:198-199): `.pose.rotation.as_quat()` / `.as_matrix()`, `.pose.translation`, `.width` -- plus the flat
    `.quat` (x, y, z, w) and `.translation` this package uses itself."""

    def __init__(self, quat, translation, width):
        self.quat, self.translation, self.width = np.asarray(quat, np.float64), np.asarray(translation, np.float64), float(width)
        self.pose = _Pose(self.quat, self.translation)

    def __repr__(self):
        return f'Grasp(t={self.translation.round(4).tolist()}, q={self.quat.round(4).tolist()}, w={self.width:.4f})'


class GraspNeRFPlanner:
    """Mirror of the reference planner (main.py:87-209) on files: `rgb/%04d.png` renderings and `camera_pose.npy`.

    cfg: the reference's yaml as a dict;  checkpoint: `model_best.pth` path or state dict ({'network_state_dict': ...});
    renderer_root_dir: holds camera_pose.npy (main.py:174);  rgb_dir: the directory of the rendered `%04d.png` images
    (main.py:168);  database_name: as in the reference's args, e.g. 'vgn_syn/test/packed/packed_170-220/032cd891d9be4a16be5ea4be9f7eca2b/w_0.8'
    (the trailing `<background>_<size>` sets the down-sampling, main.py:96-103);  graphed: plan through a PlannerSession --
    the decoded PNGs go to the device as uint8 and the resize, the forward and the selection replay as one captured graph
    (built at the first call from its frame size and view count, rebuilt when either changes)."""

    def __init__(self, cfg, checkpoint, renderer_root_dir, rgb_dir, database_name='vgn_syn/test/x/x/x/w_0.8', seed=0, device='cuda:0',
                 graphed=False):
        tp, _split, _stype, _ssplit, _sid, background_size = database_name.split('/')                 # main.py:96
        self.tp, self.down_sample = tp, float(background_size.split('_')[1])
        self.img_wh = (np.array(SRC_WH[tp]) * self.down_sample).astype(int)                            # main.py:103
        K = np.array([[892.62, 0.0, 639.5], [0.0, 892.62, 359.5], [0.0, 0.0, 1.0]])                    # main.py:105-111
        K[:2] = K[:2] * self.down_sample
        if tp == 'vgn_syn':
            K[:2] /= 2
        self.K = K
        self.voxel_size, self.bbox3d = 0.3 / 40, [[-0.15, -0.15, -0.0503], [0.15, 0.15, 0.2497]]       # main.py:90-91
        self.tsdf_thres_high, self.tsdf_thres_low = 0.0, -0.85                                         # main.py:92-93
        self.renderer_root_dir, self.rgb_dir, self.seed = renderer_root_dir, rgb_dir, seed
        ckpt = torch.load(checkpoint, map_location='cpu') if isinstance(checkpoint, (str, bytes)) else checkpoint   # read once
        self.net = load_model(cfg, ckpt, device)                                                       # main.py:150-157
        self.step = int(ckpt.get('step', 0)) if isinstance(ckpt, dict) else 0                          # main.py:155
        self.selector = GraspSelector(next(self.net.parameters()).device)
        self.graphed, self.session = bool(graphed), None

    def get_image(self, img_id, round_idx=0):                                                          # main.py:167-172
        img = read_rgb_png(os.path.join(self.rgb_dir, '%04d.png' % img_id))
        if getattr(self, 'graphed', False):
            return img                                                                                 # the session resizes on the device
        return resize_bilinear_u8(img, self.img_wh).astype(np.float32)

    def get_pose(self, img_id):                                                                        # main.py:174-177
        # read on every call like the reference: the simulator rewrites camera_pose.npy between rounds
        ori = np.load(os.path.join(self.renderer_root_dir, 'camera_pose.npy'))[img_id]
        return np.linalg.inv(ori @ BLENDER2OPENCV)[:3, :].astype(np.float32)

    def get_K(self, img_id):
        return self.K.astype(np.float32).copy()

    def get_depth_range(self, img_id, round_idx=0, fixed=True):                                        # main.py:182-187
        if not fixed:
            raise NotImplementedError('depth-map based ranges need the simulator\'s depth renderings (main.py:185-187)')
        return np.array([0.2, 0.8])

    def _session_for(self, frames):
        key = (len(frames), frames[0].shape[:2])
        if self.session is None or (self.session.n_views, self.session.src_hw) != key:
            self.session = PlannerSession(self.net, key[0], key[1], self.img_wh, max_grasps=self.selector.max_grasps,
                                          voxel_size=self.voxel_size, tsdf_thres_high=self.tsdf_thres_high,
                                          tsdf_thres_low=self.tsdf_thres_low)
        return self.session

    def __call__(self, test_view_id, round_idx=0, n_grasp=0, gt_tsdf=None):                            # main.py:189-209
        images = [self.get_image(i, round_idx) for i in test_view_id]
        session = self._session_for(images) if self.graphed else None
        if session is None:
            images = (np.stack(images, 0).astype(np.float32) / 255).transpose([0, 3, 1, 2])            # color_map_forward
        extrinsics = np.stack([self.get_pose(i) for i in test_view_id], 0)
        intrinsics = np.stack([self.get_K(i) for i in test_view_id], 0)
        depth_range = np.asarray([self.get_depth_range(i, round_idx, fixed=True) for i in test_view_id], dtype=np.float32)
        g, toc = plan(self.net, images, extrinsics, intrinsics, depth_range, self.bbox3d, seed=self.seed + round_idx + n_grasp,
                      selector=None if session else self.selector, tsdf_thres_high=self.tsdf_thres_high,
                      tsdf_thres_low=self.tsdf_thres_low, voxel_size=self.voxel_size, session=session)
        grasps = [Grasp(q, t, w) for q, t, w in zip(g['quat'], g['pos'], g['width'])]
        return grasps, g['score'], toc
