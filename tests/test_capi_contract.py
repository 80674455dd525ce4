"""What the host layer between include/gnr.h and the kernels (csrc/gnr_capi.inc) promises its callers besides values: every entry
point that takes a GnrScene refuses a bad call with the documented status code and text BEFORE anything touches the device, and every
kernel launch is bracketed under a fixed timing label (bench.py, tools/ab_*.py and the profiles key on them)."""
import ctypes as C

import numpy as np
import pytest

from graspnerf_amd import _lib

P = 4096                                            # any non-null address: validation happens first
BIG = 1 << 40
ARG, SHAPE, WORKSPACE = -1, -2, -4


def _scene(**kw):
    f = dict(B=1, V=2, H=8, W=8, fh=2, fw=2, imgs=P, img_feats=P, ray_feats=P, poses=P, Ks=P, depth_range=P, use_vis=0, options=0)
    f.update(kw)
    return _lib.GnrScene(**f)


def _rays(**kw):
    f = dict(rn=4, dn=4, fdn=4, ray_mask_view_num=2, ray_mask_point_num=8, coords=P, que_pose=P, que_K=P, que_depth_range=P,
             que_imgs=None, fine_u=None, ray_batch_num=0, fine_depth_use_all=0)
    f.update(kw)
    return _lib.GnrRays(**f)


def _out(**kw):
    f = {k: P for k in _lib.RENDER_OUT_FIELDS}
    f.update(kw)
    return _lib.GnrRenderOut(**f)


class Entry:
    """One entry point with a complete set of acceptable arguments (keyword order = argument order); a call overrides some of them."""

    def __init__(self, name, **defaults):
        self.name, self.fn, self.defaults = name, getattr(_lib.lib(), name), defaults

    def __call__(self, **kw):
        assert set(kw) <= set(self.defaults), kw
        args = dict(self.defaults, **kw)
        return self.fn(*[C.byref(v) if isinstance(v, C.Structure) else v for v in args.values()])


def test_scene_entry_points_refuse_before_touching_the_device():
    """Null pointers, unknown option bits, view counts and sample counts outside the supported range and workspaces one byte short are
    refused with GNR_ERR_ARG / GNR_ERR_SHAPE / GNR_ERR_WORKSPACE and the text below, in the order of the entry point's checks, before
    the first launch.  EVERY call here is one that validation refuses (the pointers are fake: a call that passed would launch on a
    machine with a GPU; without one it would come back as GNR_ERR_HIP and fail the assertion).  Runs without a GPU."""
    L = _lib.lib()
    s = _scene()
    R, rn, dn = 4, 4, 4
    ws0 = L.gnr_workspace_bytes(C.byref(s), 0, 0, 0)                 # the regions gnr_prepare fills
    ws_vol = L.gnr_workspace_bytes(C.byref(s), R, 0, 0)
    ws_ray = L.gnr_workspace_bytes(C.byref(s), 0, rn, dn)
    tws_vol = L.gnr_sample_volume_train_workspace_bytes(C.byref(s), R)
    tws_ray = L.gnr_render_chain_train_workspace_bytes(C.byref(s), rn, dn)
    dm_scratch = L.gnr_depth_mean_bwd_workspace_bytes(C.byref(s))
    assert 0 < ws0 < ws_vol and ws0 < ws_ray and tws_vol > 0 and tws_ray > 0 and dm_scratch > 0
    flags = C.c_uint(0)

    def refused(code, text, entry, **kw):
        rc = entry(**kw)
        msg = L.gnr_last_error().decode()
        assert (rc, msg) == (code, text), (entry.name, kw, rc, msg)

    prepare = Entry('gnr_prepare', s=s, ws=P, ws_bytes=ws0, stream=None)
    volume = Entry('gnr_sample_volume_fwd', s=s, bbox_min=P, R=R, wc=P, sdf_out=P, vmask_out=None, ws=P, ws_bytes=ws_vol, stream=None)
    volume_train = Entry('gnr_sample_volume_fwd_train', s=s, bbox_min=P, R=R, wc=P, sdf_out=P, ws=P, ws_bytes=ws_vol, tws=P,
                         tws_bytes=tws_vol, stream=None)
    volume_bwd = Entry('gnr_sample_volume_bwd', s=s, R=R, wc=P, wb=P, canonical_dev=P, dvol=P, d_canonical=P, d_ray_feats=P,
                       d_img_feats=P, ws=P, ws_bytes=ws_vol, tws=P, tws_bytes=tws_vol, stages=0x1f, stream=None)
    by_depth = Entry('gnr_render_by_depth_fwd', s=s, q=_rays(), depth=P, dn=dn, wl=P, out=_out(), ws=P, ws_bytes=ws_ray, stream=None)
    render = Entry('gnr_render_rays_fwd', s=s, q=_rays(), wc=P, wf=P, coarse=_out(), fine=_out(), fine_depth_in=None,
                   fine_inds_out=None, ws=P, ws_bytes=ws_ray, stream=None)
    chain_train = Entry('gnr_render_chain_fwd_train', s=s, q=_rays(), depth=P, dn=dn, wl=P, stats_out=P, colors_out=P, depth_out=None,
                        pts_out=P, qdir_out=P, ws=P, ws_bytes=ws_ray, tws=P, tws_bytes=tws_ray, stream=None)
    chain_bwd = Entry('gnr_render_chain_bwd', s=s, rn=rn, dn=dn, wl=P, wb=P, dstats=P, dcolors=P, d_canonical=P, d_ray_feats=P,
                      d_img_feats=P, ws=P, ws_bytes=ws0, tws=P, tws_bytes=tws_ray, stream=None)
    tail_train = Entry('gnr_render_tail_fwd_train', s=s, q=_rays(), depth=P, dn=dn, wl=P, out=_out(), fine_depth_out=None, ws=P,
                       ws_bytes=ws_ray, tws=P, tws_bytes=tws_ray, stream=None)
    mean = Entry('gnr_depth_mean_fwd', s=s, coords=P, pn=5, level_weights=P, mean_out=P, ws=P, ws_bytes=ws0, stream=None)
    mean_bwd = Entry('gnr_depth_mean_bwd', s=s, coords=P, pn=5, level_weights=P, level_weights_bwd=P, dmean=P, d_canonical=P,
                     d_ray_feats=P, ws=P, ws_bytes=ws0, scratch=P, scratch_bytes=dm_scratch, stream=None)
    status = Entry('gnr_range_status', s=s, ws=P, ws_bytes=ws0, flags_out=C.byref(flags), stream=None)

    # ---- the scene: the same checks, first, in every entry point -------------------------------------------------------
    for e in (prepare, volume, volume_train, volume_bwd, by_depth, render, chain_train, chain_bwd, tail_train, mean, mean_bwd, status):
        refused(ARG, 'GnrScene: null pointer', e, s=None)
        refused(ARG, 'GnrScene: null pointer', e, s=_scene(Ks=None))
        refused(ARG, 'GnrScene.options: unknown bits (GNR_OPT_*)', e, s=_scene(options=0x1000))
        refused(SHAPE, 'GnrScene: V must be in 2..8', e, s=_scene(V=1))
        refused(SHAPE, 'GnrScene: V must be in 2..8', e, s=_scene(V=9))
    # ---- the rays, behind the scene and in front of the entry point's own arguments ------------------------------------
    for e in (by_depth, render, chain_train, tail_train):
        refused(ARG, 'GnrRays: null pointer', e, q=None)
        refused(ARG, 'GnrRays: null pointer', e, q=_rays(que_K=None), ws=None)
        refused(SHAPE, 'GnrRays: rn must be positive', e, q=_rays(rn=0))
    for e in (render, chain_train, tail_train):                     # (gnr_render_by_depth_fwd takes its sample count as an argument)
        for bad in (dict(dn=2), dict(dn=65), dict(fdn=0), dict(fdn=65)):
            refused(SHAPE, 'GnrRays: dn/fdn must be in 3..64', e, q=_rays(**bad))
    refused(SHAPE, 'GnrRays: rn must be positive', by_depth, q=_rays(rn=0, dn=2, fdn=65), dn=2)

    # ---- per entry point: null pointer, sizes, workspaces, in the order of its checks ----------------------------------
    refused(ARG, 'workspace is null', prepare, ws=None)
    refused(WORKSPACE, 'workspace too small', prepare, ws_bytes=ws0 - 1)

    refused(ARG, 'gnr_range_status: null pointer', status, ws=None)
    refused(ARG, 'gnr_range_status: null pointer', status, flags_out=None, ws_bytes=0)
    refused(WORKSPACE, 'workspace too small', status, ws_bytes=ws0 - 1)

    for k in ('bbox_min', 'wc', 'sdf_out', 'ws'):
        refused(ARG, 'gnr_sample_volume_fwd: null pointer', volume, **{k: None})
    refused(ARG, 'gnr_sample_volume_fwd: null pointer', volume, wc=None, R=1)
    refused(SHAPE, 'volume_res must be in 2..64', volume, R=1)
    refused(SHAPE, 'volume_res must be in 2..64', volume, R=65, ws_bytes=BIG)
    refused(SHAPE, 'volume_res must be in 2..64', volume, R=1, ws_bytes=0)
    refused(WORKSPACE, 'workspace too small', volume, ws_bytes=ws_vol - 1)
    refused(WORKSPACE, 'workspace too small', volume, ws_bytes=ws0)            # (gnr_prepare's share alone is not enough)

    for k in ('bbox_min', 'wc', 'sdf_out', 'ws', 'tws'):
        refused(ARG, 'gnr_sample_volume_fwd_train: null pointer', volume_train, **{k: None})
    refused(SHAPE, 'volume_res must be in 2..64', volume_train, R=1)
    refused(SHAPE, 'volume_res must be in 2..64', volume_train, R=65, ws_bytes=BIG, tws_bytes=BIG)
    refused(WORKSPACE, 'training workspace too small', volume_train, tws_bytes=tws_vol - 1)
    refused(WORKSPACE, 'training workspace too small', volume_train, tws_bytes=tws_vol - 1, ws_bytes=0)    # the training workspace first
    refused(WORKSPACE, 'workspace too small', volume_train, ws_bytes=ws_vol - 1)

    for k in ('wc', 'wb', 'canonical_dev', 'dvol', 'd_canonical', 'ws', 'tws'):
        refused(ARG, 'gnr_sample_volume_bwd: null pointer', volume_bwd, **{k: None})
    refused(ARG, 'gnr_sample_volume_bwd: null pointer', volume_bwd, dvol=None, R=65)
    refused(SHAPE, 'volume_res must be in 2..64', volume_bwd, R=1)
    refused(SHAPE, 'volume_res must be in 2..64', volume_bwd, R=65, ws_bytes=BIG, tws_bytes=BIG)
    refused(WORKSPACE, 'training workspace too small', volume_bwd, tws_bytes=tws_vol - 1)
    refused(WORKSPACE, 'training workspace too small', volume_bwd, tws_bytes=tws_vol - 1, ws_bytes=0)
    refused(WORKSPACE, 'workspace too small', volume_bwd, ws_bytes=ws_vol - 1)
    refused(WORKSPACE, 'workspace too small', volume_bwd, ws_bytes=ws_vol - 1, stages=0)

    for k in ('depth', 'wl', 'ws'):
        refused(ARG, 'gnr_render_by_depth_fwd: null pointer', by_depth, **{k: None})
    refused(SHAPE, 'dn must be in 3..128', by_depth, dn=2)
    refused(SHAPE, 'dn must be in 3..128', by_depth, dn=129, ws_bytes=BIG)
    refused(WORKSPACE, 'workspace too small', by_depth, ws_bytes=ws_ray - 1)
    refused(WORKSPACE, 'workspace too small', by_depth, ws_bytes=ws_ray - 1, out=None)
    refused(ARG, 'GnrRenderOut.colors_nr is required', by_depth, out=None)
    refused(ARG, 'GnrRenderOut.colors_nr is required', by_depth, out=_out(colors_nr=None))

    for k in ('wc', 'coarse', 'ws', 'wf'):
        refused(ARG, 'gnr_render_rays_fwd: null pointer', render, **{k: None})
    refused(ARG, 'gnr_render_rays_fwd: fine depths / indices without a fine pass', render, fine=None, wf=None, fine_depth_in=P)
    refused(ARG, 'gnr_render_rays_fwd: fine depths / indices without a fine pass', render, fine=None, fine_inds_out=P, ws_bytes=0)
    refused(WORKSPACE, 'workspace too small', render, ws_bytes=ws_ray - 1)
    refused(WORKSPACE, 'workspace too small', render, ws_bytes=ws_ray - 1, fine=None, wf=None)
    refused(WORKSPACE, 'workspace too small', render, q=_rays(fine_depth_use_all=1), ws_bytes=ws_ray)      # dn + fdn samples per ray
    refused(ARG, 'GnrRays: fine_depth_use_all must be 0 or 1', render, q=_rays(fine_depth_use_all=2))
    refused(SHAPE, 'GnrRays: ray_batch_num must be >= 0', render, q=_rays(ray_batch_num=-1))
    refused(ARG, 'GnrRenderOut.colors_nr is required', render, coarse=_out(colors_nr=None))
    refused(ARG, 'GnrRenderOut.colors_nr is required', render, coarse=_out(colors_nr=None), fine=None, wf=None)

    for k in ('wl', 'stats_out', 'colors_out', 'ws', 'tws'):
        refused(ARG, 'gnr_render_chain_fwd_train: null pointer', chain_train, **{k: None})
    refused(SHAPE, 'gnr_render_chain_fwd_train: the coarse pass (depth == NULL) samples rays->dn depths', chain_train, depth=None, dn=5)
    refused(SHAPE, 'dn must be in 3..64 (3..128 with caller-given depths)', chain_train, dn=2)
    refused(SHAPE, 'dn must be in 3..64 (3..128 with caller-given depths)', chain_train, dn=129, ws_bytes=BIG, tws_bytes=BIG)
    refused(WORKSPACE, 'training workspace too small', chain_train, tws_bytes=tws_ray - 1)
    refused(WORKSPACE, 'training workspace too small', chain_train, tws_bytes=tws_ray - 1, ws_bytes=0, depth=None)
    refused(WORKSPACE, 'workspace too small', chain_train, ws_bytes=ws_ray - 1)
    refused(WORKSPACE, 'workspace too small', chain_train, ws_bytes=ws_ray - 1, depth=None)

    for k in ('wl', 'wb', 'dstats', 'dcolors', 'd_canonical', 'ws', 'tws'):
        refused(ARG, 'gnr_render_chain_bwd: null pointer', chain_bwd, **{k: None})
    refused(WORKSPACE, 'training workspace too small', chain_bwd, tws_bytes=tws_ray - 1)
    refused(WORKSPACE, 'training workspace too small', chain_bwd, tws_bytes=tws_ray - 1, ws_bytes=0)
    refused(WORKSPACE, 'workspace too small', chain_bwd, ws_bytes=ws0 - 1)

    for k in ('depth', 'wl', 'out', 'ws', 'tws'):
        refused(ARG, 'gnr_render_tail_fwd_train: null pointer', tail_train, **{k: None})
    refused(ARG, 'gnr_render_tail_fwd_train: null pointer', tail_train, out=_out(colors_nr=None))
    refused(SHAPE, 'dn must be in 3..128', tail_train, dn=2)
    refused(SHAPE, 'dn must be in 3..128', tail_train, dn=129, ws_bytes=BIG, tws_bytes=BIG)
    refused(SHAPE, 'the inverse-CDF resampler (fine_depth_out) takes at most 64 samples per ray', tail_train, dn=65, fine_depth_out=P,
            ws_bytes=BIG, tws_bytes=BIG)
    refused(WORKSPACE, 'training workspace too small', tail_train, tws_bytes=tws_ray - 1)
    refused(WORKSPACE, 'training workspace too small', tail_train, tws_bytes=tws_ray - 1, ws_bytes=0)
    refused(WORKSPACE, 'workspace too small', tail_train, ws_bytes=ws_ray - 1)

    for k in ('coords', 'level_weights', 'mean_out', 'ws'):
        refused(ARG, 'gnr_depth_mean_fwd: null pointer', mean, **{k: None})
    refused(SHAPE, 'pn must be positive', mean, pn=0)
    refused(WORKSPACE, 'workspace too small', mean, ws_bytes=ws0 - 1)

    for k in ('coords', 'level_weights', 'level_weights_bwd', 'dmean', 'd_canonical', 'ws'):
        refused(ARG, 'gnr_depth_mean_bwd: null pointer', mean_bwd, **{k: None})
    refused(SHAPE, 'pn must be positive', mean_bwd, pn=0)
    refused(WORKSPACE, 'workspace too small', mean_bwd, ws_bytes=ws0 - 1)
    refused(WORKSPACE, 'workspace too small', mean_bwd, ws_bytes=ws0 - 1, scratch=None)
    refused(WORKSPACE, 'gnr_depth_mean_bwd: scratch too small', mean_bwd, scratch=None)
    refused(WORKSPACE, 'gnr_depth_mean_bwd: scratch too small', mean_bwd, scratch_bytes=dm_scratch - 1)
    refused(WORKSPACE, 'gnr_depth_mean_bwd: scratch too small', mean_bwd, scratch_bytes=dm_scratch - 1, d_ray_feats=None)


# What the library built from the commit before the host layer's launches went through one helper reports for the run below.
LABELS = [
    'k_view_setup@gnr_prepare', 'k_repack_feats@gnr_prepare',
    'k_chain.volume', 'k_chain.volume.fp32_twin', 'k_ray.volume',
    'k_points_rays@render_pass', 'k_chain.render', 'k_chain.render.fp32_twin', 'k_ray.render', 'k_ray.render.fp32_twin',
    'k_gerr_reduce@render_pass', 'k_pixel_gt@render_pass',
    'k_points_volume@gnr_sample_volume_fwd_train', 'k_chain.volume.train',
    'k_ray_bwd@gnr_sample_volume_bwd', 'k_grad_reduce@tail', 'k_tail_finish', 'k_tail_unfold@gnr_sample_volume_bwd',
    'k_geo_bwd@launch_geo_bwd', 'k_view2_bwd@gnr_sample_volume_bwd', 'k_view2_bwd.fp32_twin@gnr_sample_volume_bwd',
    'k_hoist_bwd@launch_hoist_bwd', 'k_view1_bwd@gnr_sample_volume_bwd', 'k_scatter_place@gnr_sample_volume_bwd',
    'k_scatter_gather@gnr_sample_volume_bwd', 'k_view1_bwd.fp32_twin@gnr_sample_volume_bwd',
    'k_unpack_feat_grad@gnr_sample_volume_bwd', 'k_grad_reduce@gnr_sample_volume_bwd',
    'k_coarse_depth@gnr_render_chain_fwd_train', 'k_points_rays@gnr_render_chain_fwd_train', 'k_desc_unpack@gnr_render_chain_fwd_train',
    'k_chain.render.train', 'k_stats_unpack@gnr_render_chain_fwd_train',
    'k_gerr_reduce@gnr_render_tail_fwd_train', 'k_pixel_gt@gnr_render_tail_fwd_train',
    'k_red2_bwd@launch_red2_bwd', 'k_view2_bwd@gnr_render_chain_bwd', 'k_view2_bwd.fp32_twin@gnr_render_chain_bwd',
    'k_view1_bwd@gnr_render_chain_bwd', 'k_scatter_place@gnr_render_chain_bwd', 'k_scatter_gather@gnr_render_chain_bwd',
    'k_view1_bwd.fp32_twin@gnr_render_chain_bwd', 'k_unpack_feat_grad@gnr_render_chain_bwd', 'k_grad_reduce@gnr_render_chain_bwd',
    'k_depth_mean@gnr_depth_mean_fwd', 'k_depth_mean_bwd@gnr_depth_mean_bwd', 'k_grad_reduce@gnr_depth_mean_bwd',
    'k_unpack_feat_grad@gnr_depth_mean_bwd',
]


@pytest.mark.gpu
def test_timing_labels_of_a_tiny_forward_and_backward(weights_np):
    """One scene of 2 views 32 x 32 (feature maps 8 x 8), a 4^3 volume, 4 rays x 4 samples -- the smallest shapes every entry point
    accepts -- through the inference forwards, the training forwards and their backwards under gnr_timing_begin(): the SET of labels
    the launches report equals LABELS.  Nothing about the set depends on the sizes except the binned scatter's choice between
    k_scatter_place (the pixel counters of a view fit the LDS: 8 x 8 pixels here) and k_scatter_scan + k_scatter_fill."""
    import torch
    from graspnerf_amd import weights
    from graspnerf_amd.hotpath import HotPath, batch_scenes
    from graspnerf_amd.synth import make_scene
    hp = HotPath(weights.pack_state_dict(weights_np, 'coarse'), weights.pack_state_dict(weights_np, 'fine'))
    hp.set_bwd_weights(weights.pack_bwd(weights.canonical_blob(weights_np, 'coarse')), weights.pack_bwd(weights.canonical_blob(weights_np, 'fine')))
    canon = torch.from_numpy(weights.canonical_blob(weights_np, 'coarse')).cuda()
    res, rn, dn = 4, 4, 4
    bref, bque = batch_scenes([make_scene(0, dict(V=2, H=32, W=32, rn=rn, K=[[30.0, 0, 15.5], [0, 30.0, 15.5], [0, 0, 1]]))])
    cfg = {'depth_sample_num': dn, 'fine_depth_sample_num': dn, 'ray_mask_view_num': 2, 'ray_mask_point_num': 8}
    rng = np.random.default_rng(0)
    t = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    bq = {k: torch.from_numpy(v).cuda() for k, v in bque.items()}
    _lib.timing_begin()
    try:
        hp.sample_volume(bref, res)
        hp.render(bref, bque, cfg)
        hp.sample_volume_train(bref, res)
        hp.sample_volume_bwd(t(1, 1, res, res, res), canon)
        prep = hp.prepare(bref, 1, rn, dn)
        stats, colors, geo, ctx = hp.render_chain_train(bq, None, 'coarse', cfg, prep)
        hp.render_tail_train(ctx, bq, geo['depth'], colors)
        hp.render_chain_bwd(ctx, t(1, rn * dn, 65), t(1, rn * dn, 3))
        coords = torch.from_numpy(rng.uniform(0, 31, (1, 5, 2)).astype(np.float32)).cuda()
        hp.depth_mean(bref, coords)
        hp.depth_mean_bwd(bref, coords, t(1, 2, 5, 2))
        torch.cuda.synchronize()
    finally:
        got = _lib.timing_end()
    print('timing labels:', sorted(got))
    assert len(set(LABELS)) == len(LABELS)
    assert set(got) == set(LABELS), (sorted(set(got) - set(LABELS)), sorted(set(LABELS) - set(got)))
