"""What the host layer between include/gnr.h and the kernels (csrc/gnr_capi.inc, csrc/gnr_host.h) promises its callers besides values:
every entry point refuses a bad call with the documented status code and text BEFORE anything touches the device, the text is ONE
string per thread whichever source file the entry point lives in, and every kernel launch is bracketed under a fixed timing label
(bench.py, tools/ab_*.py and the profiles key on them)."""
import ctypes as C
import threading

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


# ---- one error text for every source file of the library -------------------------------------------------------------------------
def _unit_refusals():
    """(unit's reader, call, status, text): refusals of the entry points that live outside gnr_capi.inc, the calls of test_grasp_head,
    test_backbone_ops, test_ingest and test_frame_metrics.  The texts are what the library built from the commit before the units shared
    one error text left in the unit's OWN reader (gnr_metrics.hip already wrote gnr_last_error's)."""
    L = _lib.lib()
    one, big = C.c_void_p(16), C.c_size_t(1 << 40)        # never dereferenced: the argument checks come first
    head = lambda B, R, vol=one, ws=one, ws_bytes=big: lambda: L.gnr_grasp_head_fwd(B, R, vol, one, one, one, one, ws, ws_bytes, None)
    conv = lambda x=one, K=3, mode=0, ws_bytes=big: lambda: L.gnr_conv3d_same(x, one, one, one, 1, 16, 16, 4, 4, 4, K, mode, one, ws_bytes, None)
    sel_p = _lib.GnrSelectParams(gauss_radius=4, dilate_iterations=2, max_filter_size=4)
    sel = lambda tsdf=one, R=8, p=sel_p, ws_bytes=big: lambda: L.gnr_grasp_select_fwd(tsdf, one, one, one, 1, R, C.byref(p), one, one, one, one, one, one,
                                                                                  8, one, ws_bytes, None)
    norm = lambda x=one, planes=4, act=0: lambda: L.gnr_instnorm_act(x, None, one, one, one, one, one, planes, 2, 16, 1e-5, act, None)
    ok = dict(frames=P, n=1, sh=4, sw=5, ch=3, rp=15, fp=60, tab=P, out=P, dh=3, dw=4, stream=None)
    ingest = lambda **kw: lambda: L.gnr_ingest_u8(*dict(ok, **kw).values())
    ptrs = (C.c_void_p * 2)(P, P)
    need = L.gnr_frame_metrics_workspace_bytes(2, 33, 64, 2, 0, 0, 1)
    base = dict(gt=P, preds=ptrs, n_pred=2, depth_pr=P, depth_gt=P, B=2, h=33, w=64, hm=0, wm=0, ssim=1, out=P, ws=P, ws_bytes=need, stream=None)
    fm = lambda **kw: lambda: L.gnr_frame_metrics(*dict(base, **kw).values())
    return [
        ('gnr_head_last_error', head(1, 7), SHAPE, 'gnr_grasp_head_fwd: bad B/R'),
        ('gnr_head_last_error', head(0, 40), SHAPE, 'gnr_grasp_head_fwd: bad B/R'),
        ('gnr_head_last_error', head(1, 40, vol=None), ARG, 'gnr_grasp_head_fwd: null pointer'),
        ('gnr_head_last_error', head(1, 40, ws=None), ARG, 'gnr_grasp_head_fwd: null pointer'),
        ('gnr_head_last_error', head(3, 41, ws_bytes=C.c_size_t(L.gnr_grasp_head_workspace_bytes(3, 41) - 1)), WORKSPACE, 'workspace too small'),
        ('gnr_head_last_error', conv(x=None), ARG, 'gnr_conv3d_same: null pointer'),
        ('gnr_head_last_error', conv(K=4), SHAPE, 'gnr_conv3d_same: bad shape / mode (K must be 3 or 5)'),
        ('gnr_head_last_error', conv(mode=2), SHAPE, 'gnr_conv3d_same: bad shape / mode (K must be 3 or 5)'),
        ('gnr_head_last_error', conv(ws_bytes=C.c_size_t(L.gnr_conv3d_same_workspace_bytes(16, 16, 3) - 1)), WORKSPACE, 'gnr_conv3d_same: workspace too small'),
        ('gnr_post_last_error', sel(tsdf=None), ARG, 'gnr_grasp_select_fwd: null pointer'),
        ('gnr_post_last_error', sel(R=1), SHAPE, 'gnr_grasp_select_fwd: bad B / R / max_n'),
        ('gnr_post_last_error', sel(p=_lib.GnrSelectParams(gauss_radius=17, max_filter_size=4)), ARG, 'gnr_grasp_select_fwd: bad filter parameters'),
        ('gnr_post_last_error', sel(ws_bytes=C.c_size_t(L.gnr_grasp_select_workspace_bytes(1, 8) - 1)), WORKSPACE, 'workspace too small'),
        ('gnr_img_last_error', norm(x=None), ARG, 'gnr_instnorm_act: null pointer'),
        ('gnr_img_last_error', norm(planes=5), SHAPE, 'gnr_instnorm_act: planes must be a multiple of C > 0, HW > 0, act in {0,1,2}'),
        ('gnr_img_last_error', norm(act=3), SHAPE, 'gnr_instnorm_act: planes must be a multiple of C > 0, HW > 0, act in {0,1,2}'),
        ('gnr_img_last_error', lambda: L.gnr_reflect_pad2d(one, one, 2, 4, 4, 4, None), SHAPE, 'gnr_reflect_pad2d: null pointer or pad outside [0, min(H, W))'),
        ('gnr_img_last_error', lambda: L.gnr_reflect_pad2d_bwd(one, None, 2, 4, 4, 1, None), ARG, 'gnr_reflect_pad2d_bwd: null pointer or pad outside [0, min(H, W))'),
        ('gnr_img_last_error', lambda: L.gnr_upsample2x_bilinear(one, one, 2, 0, 4, None), SHAPE, 'gnr_upsample2x_bilinear: H, W > 0'),
        ('gnr_ingest_last_error', ingest(frames=None), ARG, 'gnr_ingest_u8: null pointer'),
        ('gnr_ingest_last_error', ingest(ch=5, rp=64), ARG, 'gnr_ingest_u8: channels must be 3 or 4'),
        ('gnr_ingest_last_error', ingest(sh=16385, rp=1 << 20), SHAPE, 'gnr_ingest_u8: n >= 1 and every dimension in 1..16384'),
        ('gnr_ingest_last_error', ingest(rp=14), ARG, 'gnr_ingest_u8: row_pitch < src_w * channels'),
        ('gnr_ingest_last_error', ingest(n=2, fp=59), ARG, 'gnr_ingest_u8: frame_pitch shorter than one frame'),
        ('gnr_ingest_last_error', lambda: L.gnr_ingest_tables_host(4, 5, 3, 4, None), ARG, 'gnr_ingest_tables_host: null pointer'),
        ('gnr_ingest_last_error', lambda: L.gnr_ingest_tables_host(4, 16385, 3, 4, P), SHAPE, 'gnr_ingest_tables_host: every dimension must be in 1..16384'),
        ('gnr_last_error', fm(gt=None), ARG, 'gnr_frame_metrics: null pointer'),
        ('gnr_last_error', fm(preds=(C.c_void_p * 2)(P, None)), ARG, 'gnr_frame_metrics: null prediction pointer'),
        ('gnr_last_error', fm(n_pred=5), ARG, 'gnr_frame_metrics: n_pred must be in 1..4'),
        ('gnr_last_error', fm(hm=17), SHAPE, 'gnr_frame_metrics: the crop margins leave no pixel'),
        ('gnr_last_error', fm(h=10), SHAPE, 'gnr_frame_metrics: SSIM needs a cropped frame of at least 11 x 11 pixels (the 11 x 11 window)'),
        ('gnr_last_error', fm(ws_bytes=need - 1), WORKSPACE, 'gnr_frame_metrics: workspace smaller than gnr_frame_metrics_workspace_bytes()'),
    ]


def test_every_unit_refuses_with_its_text_in_the_one_error_string():
    """Head, gnr_conv3d_same, post, img, ingest and metrics: every refusal keeps its status and its text byte for byte, and the text is
    the library's ONE error string -- gnr_last_error() and the unit's own reader (an alias now) return the same bytes.  Every call is one
    that validation refuses (fake pointers); runs without a GPU."""
    L = _lib.lib()
    rows = _unit_refusals()
    assert all(sum(r[0] == unit for r in rows) >= 2 for unit in {r[0] for r in rows}) and len({r[0] for r in rows}) == 5
    for reader, call, code, text in rows:
        rc = call()
        unit_text, one_text = getattr(L, reader)(), L.gnr_last_error()
        assert (rc, unit_text.decode()) == (code, text), (reader, text, rc, unit_text)
        assert one_text == unit_text, (reader, one_text, unit_text)
    for reader in ('gnr_head_last_error', 'gnr_post_last_error', 'gnr_img_last_error', 'gnr_ingest_last_error'):      # all five, after one failure
        assert getattr(L, reader)() == L.gnr_last_error() == rows[-1][3].encode()


def test_the_error_text_belongs_to_the_calling_thread():
    """Thread A is refused by the head while thread B is refused by the ingest, 100 times each: each thread reads back only its own
    text (the string is thread_local), through gnr_last_error and through either alias."""
    L = _lib.lib()
    one, big = C.c_void_p(16), C.c_size_t(1 << 40)
    calls = {'gnr_grasp_head_fwd: bad B/R': lambda: L.gnr_grasp_head_fwd(1, 7, one, one, one, one, one, one, big, None),
             'gnr_ingest_u8: row_pitch < src_w * channels': lambda: L.gnr_ingest_u8(P, 1, 4, 5, 3, 14, 60, P, P, 3, 4, None)}
    start, seen = threading.Barrier(len(calls)), {}

    def run(text, call):
        start.wait()
        got = set()
        for _ in range(100):
            rc = call()
            got.add((rc, L.gnr_last_error(), L.gnr_head_last_error(), L.gnr_ingest_last_error()))
        seen[text] = got
    threads = [threading.Thread(target=run, args=item) for item in calls.items()]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert seen == {'gnr_grasp_head_fwd: bad B/R': {(SHAPE,) + (b'gnr_grasp_head_fwd: bad B/R',) * 3},
                    'gnr_ingest_u8: row_pitch < src_w * channels': {(ARG,) + (b'gnr_ingest_u8: row_pitch < src_w * channels',) * 3}}


# ---- the operator entry points: every refusal with its code, its exact text and its place in the order of the checks -------------
class Op(Entry):
    """An Entry whose parameter struct `p` is written as a dict of fields, so that the faults of two rows merge field by field."""

    def __init__(self, name, struct=None, fields=None, **defaults):
        super().__init__(name, **defaults)
        self.struct, self.fields = struct, fields or {}

    def __call__(self, **kw):
        if self.struct is not None and kw.get('p', {}) is not None:
            kw = dict(kw, p=self.struct(**{**self.fields, **kw.get('p', {})}))
        return super().__call__(**kw)


def _merged(first, then):
    """The overrides of two rows in one call, or None when both set the same argument (or the same field of `p`)."""
    pa, pb = first.get('p', {}), then.get('p', {})
    if (set(first) & set(then)) - {'p'} or pa is None or pb is None or set(pa) & set(pb):
        return None
    out = {**then, **first}
    if 'p' in out:
        out['p'] = {**pb, **pa}
    return out


NAN, INF = float('nan'), float('inf')
HAND = dict(height=0.004, finger_width=0.004, tail_length=0.04, depth=0.05, opening=-1.0, spacing=0.5, approach=0.05, scale=0.0075)
HUGE = 1 << 40                                       # planes / bytes no launch takes


def _hand_rows(t):
    """The refusals gnr_hand.hip's three entry points share, in their order."""
    return [(ARG, t + 'null pointer', dict(pos=None)), (ARG, t + 'null pointer', dict(p=None)),
            (SHAPE, t + 'B must be in 1..65535', dict(B=0)), (SHAPE, t + 'B must be in 1..65535', dict(B=65536)),
            (SHAPE, t + 'R must be in 2..256', dict(R=1)), (SHAPE, t + 'R must be in 2..256', dict(R=257)),
            (SHAPE, t + 'max_n must be >= 1', dict(max_n=0)), (ARG, t + 'count_stride must be >= 1', dict(count_stride=0)),
            (ARG, t + 'top_k must be >= 0 (0: every row)', dict(top_k=-1)),
            (ARG, t + 'height, finger_width, tail_length, depth, spacing and scale must be finite and > 0', dict(p=dict(depth=0.0))),
            (ARG, t + 'height, finger_width, tail_length, depth, spacing and scale must be finite and > 0', dict(p=dict(scale=INF))),
            (ARG, t + 'approach must be finite and >= 0', dict(p=dict(approach=-1.0))),
            (ARG, t + "opening must be finite (negative: each grasp's own width)", dict(p=dict(opening=NAN)))]


def _operator_refusals():
    """[(Op, [(status, text, overrides)])]: per entry point of the operator files its refusals IN THE ORDER OF ITS CHECKS, as the library
    built from the commit before they went through gnr::Refuse, the shared limits and gnr::Carve reports them."""
    L = _lib.lib()
    out = []

    mesh = Op('gnr_surface_mesh_fwd', _lib.GnrMeshParams, dict(iso=0.0, scale=1.0), vol=P, grad=None, B=1, R=8, p={}, count=P, vertices=P,
              faces=P, gradient=None, max_v=8, max_f=8, ws=P, ws_bytes=BIG, stream=None)
    t = mesh.name + ': '
    out.append((mesh, [
        (ARG, t + 'null pointer', dict(vol=None)), (ARG, t + 'null pointer', dict(p=None)),
        (ARG, t + 'grad and gradient must be both given or both NULL', dict(grad=P)),
        (SHAPE, t + 'B must be in 1..65535', dict(B=0)), (SHAPE, t + 'B must be in 1..65535', dict(B=65536)),
        (SHAPE, t + 'R must be in 2..256', dict(R=1)), (SHAPE, t + 'R must be in 2..256', dict(R=257)),
        (SHAPE, t + 'max_v must be >= 1', dict(max_v=0)), (SHAPE, t + 'max_f must be >= 1', dict(max_f=0)),
        (ARG, t + 'iso, scale and origin must be finite', dict(p=dict(iso=NAN))),
        (ARG, t + 'iso, scale and origin must be finite', dict(p=dict(origin=(0.0, INF, 0.0)))),
        (WORKSPACE, t + 'workspace smaller than gnr_surface_mesh_workspace_bytes(B, R)', dict(ws_bytes=L.gnr_surface_mesh_workspace_bytes(1, 8) - 1))]))

    ray = Op('gnr_volume_raycast_fwd', _lib.GnrRaycastParams, dict(B=1, V=1, h=8, w=8, R=8, bisections=4, iso=0.0, scale=1.0, step=0.5, near_s=0.0,
                                                                  far_s=4.0), p={}, vol=P, grad=None, poses=P, Ks=P, depth=P, gradient=None, stream=None)
    t = ray.name + ': '
    out.append((ray, [
        (ARG, t + 'null pointer', dict(depth=None)), (ARG, t + 'null pointer', dict(p=None)),
        (ARG, t + 'grad and gradient must be both given or both NULL', dict(gradient=P)),
        (SHAPE, t + 'B must be in 1..65535', dict(p=dict(B=65536))), (SHAPE, t + 'V must be >= 1', dict(p=dict(V=0))),
        (SHAPE, t + 'h and w must be >= 1', dict(p=dict(h=0))), (SHAPE, t + 'R must be in 2..256', dict(p=dict(R=1))),
        (SHAPE, t + 'R must be in 2..256', dict(p=dict(R=257))), (ARG, t + 'bisections must be in 0..32', dict(p=dict(bisections=33))),
        (ARG, t + 'scale and step must be finite and > 0', dict(p=dict(scale=0.0))),
        (ARG, t + 'iso and origin must be finite', dict(p=dict(iso=INF))),
        (ARG, t + 'near_s must be >= 0 and far_s > near_s', dict(p=dict(far_s=0.0))),
        (ARG, t + 'step too small, a ray would take more than GNR_RAYCAST_MAX_SAMPLES (65536) samples', dict(p=dict(step=1e-6))),
        (SHAPE, t + 'h and w must give at most 2^28 tiles of 8 x 8 pixels', dict(p=dict(w=200000, h=200000)))]))

    reset = Op('gnr_tsdf_reset', B=1, R=8, tsdf=P, weight=P, stream=None)
    grid = Op('gnr_tsdf_grid', B=1, R=8, tsdf=P, weight=P, mode=0, out=P, stream=None)
    for op, last in ((reset, []), (grid, [(ARG, 'gnr_tsdf_grid: mode must be GNR_TSDF_GRID or GNR_TSDF_SDF_LABEL', dict(mode=2))])):
        t = op.name + ': '
        out.append((op, [(ARG, t + 'null pointer', dict(weight=None)), (SHAPE, t + 'B must be in 1..65535', dict(B=0)),
                         (SHAPE, t + 'B must be in 1..65535', dict(B=65536)), (SHAPE, t + 'R must be in 2..256', dict(R=1)),
                         (SHAPE, t + 'R must be in 2..256', dict(R=257))] + last))
    fuse = Op('gnr_tsdf_integrate', _lib.GnrTsdfParams, dict(B=1, V=1, h=8, w=8, R=8, depth_dtype=0, voxel_size=0.01, sdf_trunc=0.04, depth_scale=1.0,
                                                            depth_trunc=2.0), p={}, depth=P, poses=P, Ks=P, origin=P, tsdf=P, weight=P, stream=None)
    t = fuse.name + ': '
    out.append((fuse, [
        (ARG, t + 'null pointer', dict(origin=None)), (ARG, t + 'null pointer', dict(p=None)),
        (SHAPE, t + 'B must be in 1..65535', dict(p=dict(B=0))), (SHAPE, t + 'R must be in 2..256', dict(p=dict(R=257))),
        (SHAPE, t + 'V must be >= 1', dict(p=dict(V=0))), (SHAPE, t + 'h and w must be >= 1', dict(p=dict(w=0))),
        (ARG, t + 'depth_dtype must be GNR_DEPTH_F32 or GNR_DEPTH_U16', dict(p=dict(depth_dtype=2))),
        (ARG, t + 'voxel_size, sdf_trunc, depth_scale and depth_trunc must be > 0', dict(p=dict(sdf_trunc=NAN)))]))

    sel_fields = dict(gauss_radius=4, dilate_iterations=2, max_filter_size=4)
    sel_args = dict(tsdf=P, qual=P, rot=P, width=P, B=1, R=8, p={}, qual_out=P, count=P, index=P, score=P, quat=P, width_out=P, max_n=8, ws=P, ws_bytes=BIG,
                    stream=None)
    sel = Op('gnr_grasp_select_fwd', _lib.GnrSelectParams, sel_fields, **sel_args)
    sel2 = Op('gnr_grasp_select_v2_fwd', lambda order=0, top_k=0, **kw: _lib.GnrSelectParamsV2(select=_lib.GnrSelectParams(**kw), order=order, top_k=top_k),
              sel_fields, **sel_args)
    for op in (sel, sel2):
        t = op.name + ': '
        out.append((op, [
            (ARG, t + 'null pointer', dict(width_out=None)), (ARG, t + 'null pointer', dict(p=None)),
            (SHAPE, t + 'bad B / R / max_n', dict(B=0)), (SHAPE, t + 'bad B / R / max_n', dict(R=1)), (SHAPE, t + 'bad B / R / max_n', dict(R=257)),
            (SHAPE, t + 'bad B / R / max_n', dict(max_n=0)), (ARG, t + 'bad filter parameters', dict(p=dict(gauss_radius=17))),
            (ARG, t + 'bad filter parameters', dict(p=dict(max_filter_size=17)))] + ([] if op is sel else [
                (ARG, t + 'order must be GNR_SELECT_ORDER_INDEX or GNR_SELECT_ORDER_SCORE', dict(p=dict(order=2))),
                (ARG, t + 'top_k must be >= 0 (0: as many as max_n)', dict(p=dict(top_k=-1))),
                (SHAPE, t + 'GNR_SELECT_ORDER_SCORE takes R <= 64 (2^18 voxels per scene to rank)', dict(p=dict(order=1), R=65)),
                (WORKSPACE, 'workspace too small', dict(p=dict(order=1), ws_bytes=L.gnr_grasp_select_v2_workspace_bytes(1, 8, 1) - 1))]) + [
            (WORKSPACE, 'workspace too small', dict(ws_bytes=L.gnr_grasp_select_workspace_bytes(1, 8) - 1))]))

    cloud = Op('gnr_surface_points_fwd', _lib.GnrSurfaceParams, dict(lo=-0.1, hi=0.1, color_mode=0, scale=1.0), vol=P, B=1, R=8, p={}, count=P, index=P,
               points=P, colors=P, max_n=8, ws=P, ws_bytes=BIG, stream=None)
    t = cloud.name + ': '
    out.append((cloud, [
        (ARG, t + 'null pointer', dict(colors=None)), (ARG, t + 'null pointer', dict(p=None)),
        (SHAPE, t + 'bad B / R / max_n (R <= 256)', dict(B=0)), (SHAPE, t + 'bad B / R / max_n (R <= 256)', dict(B=65536)),
        (SHAPE, t + 'bad B / R / max_n (R <= 256)', dict(R=0)), (SHAPE, t + 'bad B / R / max_n (R <= 256)', dict(R=257)),
        (SHAPE, t + 'bad B / R / max_n (R <= 256)', dict(max_n=0)),
        (ARG, t + 'color_mode must be GNR_SURFACE_COLOR_FIXED or GNR_SURFACE_COLOR_VALUE', dict(p=dict(color_mode=2))),
        (WORKSPACE, 'workspace too small', dict(ws_bytes=L.gnr_surface_points_workspace_bytes(1, 8) - 1))]))
    normals = Op('gnr_surface_gradient_fwd', grad=P, index=P, count=P, B=1, R=8, max_points=8, out=P, stream=None)
    t = normals.name + ': bad B / R / max_points (1 <= R <= 256, max_points >= 0)'
    out.append((normals, [(ARG, normals.name + ': null pointer', dict(count=None))] +
                [(SHAPE, t, kw) for kw in (dict(B=0), dict(B=65536), dict(R=0), dict(R=257), dict(max_points=-1))]))

    t = 'gnr_ingest_u8: '
    out.append((Op('gnr_ingest_u8', frames=P, n=1, sh=4, sw=5, ch=3, rp=15, fp=60, tab=P, out=P, dh=3, dw=4, stream=None), [
        (ARG, t + 'null pointer', dict(tab=None)), (ARG, t + 'channels must be 3 or 4', dict(ch=2)),
        (SHAPE, t + 'n >= 1 and every dimension in 1..16384', dict(n=0)), (SHAPE, t + 'n >= 1 and every dimension in 1..16384', dict(dw=16385)),
        (ARG, t + 'row_pitch < src_w * channels', dict(rp=14)), (ARG, t + 'frame_pitch shorter than one frame', dict(n=2, fp=59)),
        (SHAPE, t + 'too many output pixels for one launch', dict(n=64, fp=60, dh=16384, dw=16384))]))
    t = 'gnr_ingest_tables_host: '
    out.append((Op('gnr_ingest_tables_host', sh=4, sw=5, dh=3, dw=4, tables=P), [
        (ARG, t + 'null pointer', dict(tables=None)), (SHAPE, t + 'every dimension must be in 1..16384', dict(sw=0)),
        (SHAPE, t + 'every dimension must be in 1..16384', dict(dh=16385))]))

    t = 'gnr_instnorm_act_bwd: '
    out.append((Op('gnr_instnorm_act_bwd', dy=P, out=None, x=P, mean=P, rstd=P, weight=P, dx=P, dres=None, s1=P, s2=P, dweight=P, dbias=P, planes=4, C=2,
                   HW=16, act=0, stream=None), [
        (ARG, t + 'null pointer', dict(s2=None)), (ARG, t + 'null pointer', dict(act=1)),                   # (an activation needs `out`)
        (SHAPE, t + 'planes must be a multiple of C > 0, HW > 0, act in {0,1,2}', dict(planes=5)),
        (SHAPE, t + 'planes must be a multiple of C > 0, HW > 0, act in {0,1,2}', dict(HW=0)),
        (SHAPE, t + 'planes must be a multiple of C > 0, HW > 0, act in {0,1,2}', dict(planes=HUGE))]))
    for name in ('gnr_reflect_pad2d', 'gnr_reflect_pad2d_bwd'):
        t = name + ': null pointer or pad outside [0, min(H, W))'
        out.append((Op(name, a=P, b=P, planes=2, H=4, W=4, pad=1, stream=None), [
            (ARG, t, dict(b=None)), (SHAPE, t, dict(planes=-1)), (SHAPE, t, dict(pad=4)), (SHAPE, name + ': too many pixels for one launch', dict(planes=HUGE))]))
    t = 'gnr_upsample2x_bilinear: '
    out.append((Op('gnr_upsample2x_bilinear', x=P, y=P, planes=2, H=4, W=4, stream=None), [
        (ARG, t + 'null pointer', dict(y=None)), (SHAPE, t + 'H, W > 0', dict(H=0)), (SHAPE, t + 'H, W > 0', dict(planes=-1)),
        (SHAPE, t + 'too large for one launch', dict(planes=HUGE)), (SHAPE, t + 'too large for one launch', dict(planes=HUGE, W=5))]))

    out.append((Op('gnr_pack_grasp_head', c=None, p=None), [(ARG, 'gnr_pack_grasp_head: null pointer', {})]))
    out.append((Op('gnr_conv3d_bwd_weight', x=P, dy=P, dw=P, B=1, Cin=16, Cout=16, D=4, H=4, W=4, K=3, stream=None),
                [(ARG, 'gnr_conv3d_bwd_weight: null pointer, a size below 1 or an even K', kw) for kw in (dict(dw=None), dict(Cin=0), dict(K=4), dict(K=0))]))
    out.append((Op('gnr_conv3d_tap_mask', pattern=P, mask=P, Cin=16, Cout=16, K=3, stream=None),
                [(ARG, 'gnr_conv3d_tap_mask: null pointer, a size below 1 or K not 3 or 5', kw) for kw in (dict(mask=None), dict(Cout=0), dict(K=7))]))
    for name in ('gnr_pack_weights_device', 'gnr_pack_weights_bwd_device', 'gnr_pack_vis_decoder_device', 'gnr_pack_vis_decoder_bwd_device'):
        out.append((Op(name, src=P, dst=P, stream=None), [(ARG, name + ': null pointer', dict(src=None)), (ARG, name + ': null pointer', dict(dst=None))]))

    color_fields = dict(B=1, V=2, H=8, W=8, R=8, iso=0.0, scale=1.0, step=0.5, bias=0.0, cos_min=0.0)
    points = Op('gnr_surface_color_points_fwd', _lib.GnrSurfaceColorParams, color_fields, p={}, vol=P, points=P, count=P, count_stride=1, max_n=8,
                images=P, poses=P, Ks=P, colors=P, weight=P, views=P, stream=None)
    pixels = Op('gnr_surface_color_pixels_fwd', _lib.GnrSurfaceColorParams, color_fields, p={}, vol=P, depth=P, cam_poses=P, cam_Ks=P, Vc=1, hc=8, wc=8,
                images=P, poses=P, Ks=P, colors=P, weight=P, views=P, stream=None)
    for op in (points, pixels):
        t = op.name + ': '
        out.append((op, [
            (ARG, t + 'null pointer', dict(views=None)), (ARG, t + 'null pointer', dict(p=None)),
            (SHAPE, t + 'B must be in 1..65535', dict(p=dict(B=0))), (SHAPE, t + 'B must be in 1..65535', dict(p=dict(B=65536))),
            (SHAPE, t + 'V must be in 1..32 (one bit of the view mask each)', dict(p=dict(V=33))), (SHAPE, t + 'H and W must be >= 2', dict(p=dict(W=1))),
            (SHAPE, t + 'R must be in 2..256', dict(p=dict(R=1))), (SHAPE, t + 'R must be in 2..256', dict(p=dict(R=257))),
            (ARG, t + 'scale and step must be finite and > 0', dict(p=dict(step=-1.0))), (ARG, t + 'bias must be finite and >= 0', dict(p=dict(bias=-1.0))),
            (ARG, t + 'iso, origin, point_offset, cos_min and fill must be finite', dict(p=dict(fill=(0.0, NAN, 0.0)))),
            (ARG, t + 'step too small, a march would take more than GNR_RAYCAST_MAX_SAMPLES (65536) samples', dict(p=dict(step=1e-6)))] + (
                [(SHAPE, t + 'max_n must be >= 1', dict(max_n=0)), (ARG, t + 'count_stride must be >= 1', dict(count_stride=0))] if op is points else
                [(SHAPE, t + 'Vc must be >= 1', dict(Vc=0)), (SHAPE, t + 'hc and wc must be >= 1', dict(hc=0)),
                 (SHAPE, t + 'hc and wc must give at most 2^28 tiles of 8 x 8 pixels', dict(hc=200000, wc=200000))])))

    ptrs = (C.c_void_p * 2)(P, P)
    need = L.gnr_frame_metrics_workspace_bytes(2, 33, 64, 2, 0, 0, 1)
    t = 'gnr_frame_metrics: '
    out.append((Op('gnr_frame_metrics', gt=P, preds=ptrs, n_pred=2, depth_pr=P, depth_gt=P, B=2, h=33, w=64, hm=0, wm=0, ssim=1, out=P, ws=P, ws_bytes=need,
                   stream=None), [
        (ARG, t + 'null pointer', dict(depth_gt=None)), (ARG, t + 'n_pred must be in 1..4', dict(n_pred=0)),
        (SHAPE, t + 'B in 1..65535, h, w >= 1, h * w below 2^31', dict(B=0)), (SHAPE, t + 'B in 1..65535, h, w >= 1, h * w below 2^31', dict(B=65536)),
        (SHAPE, t + 'B in 1..65535, h, w >= 1, h * w below 2^31', dict(h=1 << 16, w=1 << 15)),
        (SHAPE, t + 'the crop margins leave no pixel', dict(wm=32)),
        (SHAPE, t + 'SSIM needs a cropped frame of at least 11 x 11 pixels (the 11 x 11 window)', dict(hm=12)),
        (ARG, t + 'null prediction pointer', dict(preds=(C.c_void_p * 2)(P, None))),
        (WORKSPACE, t + 'workspace smaller than gnr_frame_metrics_workspace_bytes()', dict(ws_bytes=need - 1))]))

    rows = dict(vol=P, pos=P, quat=P, width=P, count=P, count_stride=1, B=1, R=8, max_n=4, top_k=0)
    small = dict(p=dict(spacing=1e-6))
    clear = Op('gnr_hand_clearance_fwd', _lib.GnrHandParams, HAND, p={}, **rows, clearance=P, worst=P, inside=P, stream=None)
    close = Op('gnr_finger_closure_fwd', _lib.GnrHandParams, HAND, p={}, level=0.0, bisections=4, **rows, travel=P, cosine=P, contact=P, closed=P, stream=None)
    which = Op('gnr_grasp_objects_fwd', _lib.GnrHandParams, HAND, p={}, **rows, object=P, votes=P, distinct=P, inside=P, stream=None)
    t = clear.name + ': '
    out.append((clear, _hand_rows(t) + [
        (ARG, t + 'spacing too small or approach too long, a grasp would take more than GNR_HAND_MAX_SAMPLES (4194304) samples', small)]))
    t = close.name + ': '
    out.append((close, _hand_rows(t) + [
        (ARG, t + 'level must be finite', dict(level=NAN)), (ARG, t + 'bisections must be in 0..16', dict(bisections=17)),
        (ARG, t + 'spacing too small, a grasp would take more than GNR_HAND_MAX_SAMPLES (4194304) volume reads', small)]))
    t = which.name + ': '
    out.append((which, _hand_rows(t) + [
        (ARG, t + 'spacing too small, a grasp would take more than GNR_HAND_MAX_SAMPLES (4194304) samples', small)]))

    solid = lambda t: [(ARG, t + 'z_min must be in 0..R', dict(p=dict(z_min=-1))), (ARG, t + 'z_min must be in 0..R', dict(p=dict(z_min=9))),
                       (ARG, t + 'level must be finite', dict(p=dict(level=INF))), (ARG, t + 'lower must not be a NaN (-inf: none)', dict(p=dict(lower=NAN)))]
    objects = Op('gnr_volume_objects_fwd', _lib.GnrObjectsParams, dict(level=0.0, lower=-INF, z_min=0, connectivity=6, max_objects=8, min_voxels=1,
                                                                      free_value=1.0), p={}, vol=P, B=1, R=8, labels=P, count=P, voxels=P, bbox=P,
                 sums=P, cleaned=None, ws=P, ws_bytes=BIG, stream=None)
    t = objects.name + ': '
    out.append((objects, [
        (ARG, t + 'null pointer', dict(sums=None)), (ARG, t + 'null pointer', dict(p=None)),
        (SHAPE, t + 'B must be in 1..65535', dict(B=0)), (SHAPE, t + 'B must be in 1..65535', dict(B=65536)),
        (SHAPE, t + 'R must be in 2..256', dict(R=1)), (SHAPE, t + 'R must be in 2..256', dict(R=257)),
        (ARG, t + 'connectivity must be 6, 18 or 26', dict(p=dict(connectivity=8))), (SHAPE, t + 'max_objects must be >= 1', dict(p=dict(max_objects=0)))] +
        solid(t) + [(ARG, t + 'free_value must be finite', dict(p=dict(free_value=NAN))),
                    (WORKSPACE, t + 'workspace too small', dict(ws_bytes=L.gnr_volume_objects_workspace_bytes(1, 8) - 1))]))
    distance = Op('gnr_volume_distance_fwd', _lib.GnrDistanceParams, dict(level=0.0, lower=-INF, scale=0.0075, surface_offset=0.5, z_min=0), p={}, vol=P,
                  labels=None, B=1, R=8, d2_solid=P, nearest_solid=P, d2_free=None, nearest_free=None, esdf=None, nearest_label=None, ws=P, ws_bytes=BIG,
                  stream=None)
    t = distance.name + ': '
    out.append((distance, [
        (ARG, t + 'null pointer', dict(nearest_solid=None)), (ARG, t + 'null pointer', dict(p=None)),
        (ARG, t + 'B must be in 1..65535', dict(B=0)), (ARG, t + 'B must be in 1..65535', dict(B=65536)),       # GNR_ERR_ARG, not the siblings' GNR_ERR_SHAPE
        (ARG, t + 'R must be in 2..256', dict(R=1)), (ARG, t + 'R must be in 2..256', dict(R=257))] + solid(t) + [
        (ARG, t + 'scale must be finite and > 0', dict(p=dict(scale=0.0))), (ARG, t + 'surface_offset must be finite and >= 0', dict(p=dict(surface_offset=-0.5))),
        (ARG, t + 'nearest_label needs labels', dict(nearest_label=P)), (ARG, t + 'd2_free and nearest_free go together', dict(d2_free=P)),
        (WORKSPACE, t + 'workspace too small', dict(ws_bytes=L.gnr_volume_distance_workspace_bytes(1, 8) - 1))]))
    return out


def test_operator_entry_points_refuse_in_order():
    """Mesh, ray cast, TSDF, select, surface cloud and normals, ingest, img, the head's small entry points, pack_dev, surface colours,
    frame metrics, the hand's three, objects and distance: every refusal alone gives its status and its exact text, and together with
    the fault of the row behind it (where the two do not set the same argument) it still gives its own -- the order of the checks.
    Every call is one that validation refuses (fake pointers); runs without a GPU."""
    L = _lib.lib()
    singles = pairs = 0
    for op, rows in _operator_refusals():
        for i, (code, text, kw) in enumerate(rows):
            assert (op(**kw), L.gnr_last_error().decode()) == (code, text), (op.name, kw)
            singles += 1
            for _, _, later in rows[i + 1:]:
                both = _merged(kw, later)
                if both is not None:
                    assert (op(**both), L.gnr_last_error().decode()) == (code, text), (op.name, both)
                    pairs += 1
    assert (singles, pairs) == (237, 969)                     # (no row and no pair dropped out on the way)


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


# What the library built from the commit before every source file launched through csrc/gnr_host.h reports for the run below: the grasp
# head's forward is ONE bracket around all of its kernels, the head's training convolutions and the frame metrics label each launch,
# and the post-processing, the image ops, the ingest and the device packer report nothing.
UNIT_LABELS = [
    'grasp_head_fwd(all kernels)@gnr_grasp_head_fwd',
    'k_pack_conv3d_frag@gnr_conv3d_same', 'k_conv3d_s1.fwd@gnr_conv3d_same',
    'k_conv3d_wgrad_s1@gnr_conv3d_same_bwd_weight', 'k_conv3d_wgrad_reduce@gnr_conv3d_same_bwd_weight',
    'k_conv3d_bwd_weight@gnr_conv3d_bwd_weight',
    'k_frame_pixels@gnr_frame_metrics', 'k_frame_ssim@gnr_frame_metrics', 'k_frame_finish@gnr_frame_metrics',
]


@pytest.mark.gpu
def test_timing_labels_of_the_units_outside_the_scene_entry_points():
    """One smallest accepted call of every unit that is not gnr_capi.inc -- head forward (B = 1, R = 8), gnr_conv3d_same forward and both
    weight gradients (16 -> 16, k3, 4^3), select (R = 8), the three image ops on an 8 x 8 plane, ingest (8 x 8 -> 4 x 4), the device
    packers, the frame metrics (16 x 16, one prediction) -- under gnr_timing_begin(): the SET of labels equals UNIT_LABELS."""
    import torch
    from graspnerf_amd import backbone, metrics
    from graspnerf_amd.grasp_post import GraspSelector
    from graspnerf_amd.ingest import DeviceIngest
    L = _lib.lib()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    t = lambda *shape: torch.rand(*shape, generator=g).to(dev)
    z = lambda n: torch.zeros(n, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    B, R, n40 = 1, 8, 40 ** 3
    vol, packed, qual, rot, width = t(B, 1, R, R, R), z(L.gnr_head_packed_floats()), z(B * n40), z(B * 4 * n40), z(B * n40)
    head_ws = torch.empty(L.gnr_grasp_head_workspace_bytes(B, R), dtype=torch.uint8, device=dev)
    x, w, dy, dw = t(1, 16, 4, 4, 4), t(16, 16, 3, 3, 3).requires_grad_(), t(1, 16, 4, 4, 4), z(16 * 16 * 27)
    plane, nw, nb = t(1, 1, 8, 8), torch.ones(1, device=dev), z(1)
    canon, packed_fwd, packed_bwd = z(L.gnr_canonical_weights_floats()), z(L.gnr_packed_weights_floats()), z(L.gnr_packed_bwd_floats())
    frames = (t(1, 8, 8, 3) * 255).to(torch.uint8)
    ingest, select = DeviceIngest(dev), GraspSelector(dev, max_grasps=8)
    ingest.tables((8, 8), (4, 4))                                      # (the upload of the tables is not a launch of the library)
    gt, pred, depth = t(1, 256, 3), t(1, 256, 3), t(1, 256)
    _lib.timing_begin()
    try:
        _lib.check(L.gnr_grasp_head_fwd(B, R, vol.data_ptr(), packed.data_ptr(), qual.data_ptr(), rot.data_ptr(), width.data_ptr(),
                                        head_ws.data_ptr(), head_ws.numel(), stream), 'gnr_grasp_head_fwd')
        backbone._Conv3dSame.apply(x, w, None).backward(dy)             # forward + gnr_conv3d_same_bwd_weight (x takes no gradient)
        _lib.check(L.gnr_conv3d_bwd_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 1, 16, 16, 4, 4, 4, 3, stream), 'gnr_conv3d_bwd_weight')
        select(t(B, 1, R, R, R), t(B, 1, R, R, R), t(B, 4, R, R, R), t(B, 1, R, R, R))
        backbone._InstNormActFn.apply(plane, nw, nb, 1e-5, 1, None)
        backbone._ReflectPadFn.apply(plane, 1)
        backbone._Upsample2xFn.apply(plane)
        ingest(frames, (4, 4))
        _lib.check(L.gnr_pack_weights_device(canon.data_ptr(), packed_fwd.data_ptr(), stream), 'gnr_pack_weights_device')
        _lib.check(L.gnr_pack_weights_bwd_device(canon.data_ptr(), packed_bwd.data_ptr(), stream), 'gnr_pack_weights_bwd_device')
        metrics.frame_metrics_device(gt, [pred], depth, depth.clone(), 16, 16, ssim=True)
        torch.cuda.synchronize()
    finally:
        got = _lib.timing_end()
    print('timing labels:', sorted(got))
    assert len(set(UNIT_LABELS)) == len(UNIT_LABELS)
    assert set(got) == set(UNIT_LABELS), (sorted(set(got) - set(UNIT_LABELS)), sorted(set(UNIT_LABELS) - set(got)))
