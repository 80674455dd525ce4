"""The SDF gradient volume (include/gnr.h gnr_sample_volume_grad_fwd, HotPath.sample_volume_gradient): what the reference's network
returns next to the SDF on every sample_volume call (ibrnet.py:485-513) and its volume path drops (aggregate_net.py:133-134).

What the GPU tests compare against is pinned on the CPU first: the reference's own second return value (tests/golden/
golden_volume_gradient_cfg1.npz, tools/make_volume_gradient_golden.py) equals the oracle's composition of volume_query_points ->
project_points -> gather_views -> decode_hit_vis -> aggregate(want_grad=True) -> flip, whose sdf is bitwise O.sample_volume.

Tolerances are the project's (tests/test_gpu_parity.py): the gradient |a-b| <= 2e-4 + 1e-3 |b| (the bound on the render passes'
sdf_gradient: the same kernel arithmetic), sdf and the eikonal term ATOL = 2e-5, RTOL = 1e-3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, weights
from graspnerf_amd.synth import make_scene, CONFIGS
from oracle import graspnerf_oracle as O
from conftest import PARITY_LOG

RTOL, ATOL, ATOL_G = 1e-3, 2e-5, 2e-4
SHIFT = np.asarray([0.45, 0.0, 0.0], np.float32)


def close(a, b, what, rtol=RTOL, atol=ATOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64).reshape(a.shape)
    assert np.isfinite(a).all(), f'{what}: not finite'
    err = np.abs(a - b)
    PARITY_LOG.append({'what': what, 'max_abs': float(err.max()), 'max_over_tol': float((err / (atol + rtol * np.abs(b))).max()),
                       'atol': atol, 'rtol': rtol, 'n': int(a.size)})
    print(f'{what}: max abs {err.max():.3e}, max err/tol {(err / (atol + rtol * np.abs(b))).max():.3f}')
    assert (err - (atol + rtol * np.abs(b))).max() <= 0, f'{what}: max abs diff {err.max():.3e} exceeds tolerance (atol {atol}, rtol {rtol})'


# ---- the oracle's composition (computed once per case, shared, never modified) --------------------------------------------------
_ORACLE = {}


def oracle_gradient(tag, W, ref, res):
    """-> dict(sdf [R,R,R], grad [R,R,R,3] float32 numpy, nviews [R,R,R] int) in the volume's voxel order."""
    key = (tag, res, ref['poses'].shape[0], float(ref['bbox3d'][0, 0]), float(ref['ray_feats'].reshape(-1)[0]))
    if key not in _ORACLE:
        inp = O.to_torch(ref)
        with torch.no_grad():
            h, w = inp['imgs'].shape[-2:]
            pts = O.volume_query_points(res, inp['bbox3d'][0]).reshape(-1, 3)
            uv, z, mask, dirv = O.project_points(pts, inp['poses'], inp['Ks'], h, w)
            f_ray, rgb, f_img = O.gather_views(inp, uv, mask)
            hit, vis = O.decode_hit_vis(W, 'dist_decoder.', f_ray, z, mask, inp['depth_range'], 0.005, 0.005)
            qdir = torch.tensor([0., 0., 1.], dtype=torch.float32).expand(pts.shape[0], 3)
        o = O.aggregate(W, 'agg_net.', f_ray, rgb, f_img, hit, vis, mask, dirv, qdir, pts, res * res, res, want_grad=True, want_rgb=False)
        flip = lambda t, *tail: torch.flip(t.reshape(res, res, res, *tail), (2,)).numpy()       # renderer.py:197-198
        out = {'sdf': flip(o['sdf']), 'grad': flip(o['grad'], 3), 'nviews': flip(mask.sum(0).to(torch.int32))}
        for v in out.values():
            v.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _torch_w(wnp):
    return {k: torch.from_numpy(v) for k, v in wnp.items()}


def _shifted(ref):
    return dict(ref, bbox3d=(ref['bbox3d'] + SHIFT).astype(np.float32))


# =================================================================================================================================
# CPU
# =================================================================================================================================
def test_reference_golden_equals_the_oracle_composition(weights_np, golden):
    """Both are torch fp32 on the CPU: 1e-5 + 1e-4 |b|; and the composition's sdf is bitwise O.sample_volume."""
    G = golden('volume_gradient_cfg1')
    ref, _ = make_scene(0, 'cfg1')
    W = _torch_w(weights_np)
    o = oracle_gradient('seed0', W, ref, 16)
    assert G['gradient'].shape == (16, 16, 16, 3) and G['gradient'].dtype == np.float32
    err = np.abs(G['gradient'].astype(np.float64) - o['grad'])
    assert (err - (1e-5 + 1e-4 * np.abs(o['grad']))).max() <= 0, err.max()
    assert np.array_equal(o['sdf'], O.sample_volume(W, O.to_torch(ref), 16).numpy()[0, 0])


def _fake_scene(B=1, V=3, options=0):
    p = 4096                                           # never dereferenced: every refusal below happens on the host
    return _lib.GnrScene(B, V, 96, 128, 24, 32, p, p, p, p, p, p, 0, options)


def _last_error():
    return _lib.lib().gnr_last_error().decode()


def test_refusals_before_the_device():
    L = _lib.lib()
    s = _fake_scene()
    need = L.gnr_sample_volume_grad_workspace_bytes(C.byref(s), 16)
    assert need > L.gnr_workspace_bytes(C.byref(s), 16, 0, 0) and need > L.gnr_workspace_bytes(C.byref(s), 1, 256, 16)
    p = C.c_void_p(4096)
    call = lambda scene, bbox, R, w, g, ws, nbytes: L.gnr_sample_volume_grad_fwd(scene, bbox, R, w, g, None, None, ws, nbytes, None)
    assert call(None, p, 16, p, p, p, need) == _lib.GNR_ERR_ARG
    for args in [(None, 16, p, p, p), (p, 16, None, p, p), (p, 16, p, None, p), (p, 16, p, p, None)]:
        assert call(C.byref(s), args[0], args[1], args[2], args[3], args[4], need) == _lib.GNR_ERR_ARG
        assert 'null pointer' in _last_error()
    for R in (2, 65, 0, -1):
        assert call(C.byref(s), p, R, p, p, p, 1 << 40) == _lib.GNR_ERR_SHAPE
        assert '3..64' in _last_error()
    bad = _fake_scene(options=0x1000)
    assert call(C.byref(bad), p, 16, p, p, p, need) == _lib.GNR_ERR_ARG and 'unknown bits' in _last_error()
    assert call(C.byref(s), p, 16, p, p, p, need - 1) == _lib.GNR_ERR_WORKSPACE and 'workspace too small' in _last_error()
    for R in (3, 64):
        assert L.gnr_sample_volume_grad_workspace_bytes(C.byref(s), R) > 0
    assert L.gnr_sample_volume_grad_workspace_bytes(C.byref(s), 65) == 0 and L.gnr_sample_volume_grad_workspace_bytes(None, 16) == 0
    # the gather
    g = lambda grad, index, count, B, R, n, out: L.gnr_surface_gradient_fwd(grad, index, count, B, R, n, out, None)
    for args in [(None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)]:
        assert g(args[0], args[1], args[2], 1, 9, 8, args[3]) == _lib.GNR_ERR_ARG and 'null pointer' in _last_error()
    assert g(p, p, p, 1, 0, 8, p) == _lib.GNR_ERR_SHAPE
    assert g(p, p, p, 1, 9, -1, p) == _lib.GNR_ERR_SHAPE and 'max_points' in _last_error()
    assert g(p, p, p, 0, 9, 8, p) == _lib.GNR_ERR_SHAPE


# =================================================================================================================================
# GPU
# =================================================================================================================================
gpu = pytest.mark.gpu
_HOT = {}


def _hp(tag, wnp):
    from graspnerf_amd.hotpath import HotPath
    if tag not in _HOT:
        _HOT[tag] = HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))
    return _HOT[tag]


def _batch(refs):
    return {k: np.stack([r[k] for r in refs]) for k in refs[0]}


def _grad(hp, refs, res, **kw):
    out = hp.sample_volume_gradient(_batch(refs), res, **kw)
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.cpu().numpy()


@gpu
def test_cfg1_against_the_reference_golden_and_the_oracle(weights_np, weights_trained_np, golden):
    ref, _ = make_scene(0, 'cfg1')
    G = golden('volume_gradient_cfg1')
    for tag, wnp in (('seed0', weights_np), ('trained', weights_trained_np)):
        hp = _hp(tag, wnp)
        o = oracle_gradient(tag, _torch_w(wnp), ref, 16)
        grad, sdf, err = _grad(hp, [ref], 16, want_sdf=True, want_error=True)
        assert grad.shape == (1, 16, 16, 16, 3) and sdf.shape == (1, 16, 16, 16) and err.shape == (1,)
        if tag == 'seed0':
            close(_np(grad)[0], G['gradient'], 'volume gradient vs reference golden', atol=ATOL_G)
        close(_np(grad)[0], o['grad'], f'volume gradient vs oracle ({tag})', atol=ATOL_G)
        close(_np(sdf)[0], o['sdf'], f'volume gradient pass sdf vs oracle ({tag})')
        gn = np.linalg.norm(o['grad'].astype(np.float64), axis=-1)
        close(_np(err), [np.mean((gn - 1.0) ** 2)], f'volume gradient error vs oracle ({tag})')
        vol = _np(hp.sample_volume(_batch([ref]), 16))[0, 0]
        close(_np(sdf)[0], vol, f'volume gradient pass sdf vs sample_volume ({tag})')
        print(f'sdf_out bitwise equal to sample_volume ({tag}):', bool(np.array_equal(_np(sdf)[0], vol)),
              'max abs', float(np.abs(_np(sdf)[0] - vol).max()))
        assert hp.range_status() == 0


# R = 3: 27 points, one partial 16-point tile; 5: 125 points; 9; 17: a column longer than one 16-sample MFMA column group of the VJP tail
@gpu
@pytest.mark.parametrize('res,V,use_vis', [(3, 3, False), (5, 3, False), (9, 3, False), (17, 3, False), (5, 2, False), (9, 8, False), (5, 3, True)])
def test_awkward_sizes_against_the_oracle(res, V, use_vis, weights_np, golden):
    wnp, tag = weights_np, 'seed0'
    if use_vis:
        Gv = golden('cfg1_use_vis')
        wnp, tag = {**weights_np, **{k[len('weights.'):]: v for k, v in Gv.items() if k.startswith('weights.')}}, 'seed0_vis'
    ref, _ = make_scene(0, dict(CONFIGS['cfg1'], V=V))
    hp = _hp(tag, wnp)
    assert hp.use_vis == use_vis
    o = oracle_gradient(tag, _torch_w(wnp), ref, res)
    grad, sdf, err = _grad(hp, [ref], res, want_sdf=True, want_error=True)
    what = f'R={res} V={V}' + (' use_vis' if use_vis else '')
    close(_np(grad)[0], o['grad'], f'volume gradient vs oracle {what}', atol=ATOL_G)
    close(_np(sdf)[0], o['sdf'], f'volume gradient pass sdf vs oracle {what}')
    gn = np.linalg.norm(o['grad'].astype(np.float64), axis=-1)
    close(_np(err), [np.mean((gn - 1.0) ** 2)], f'volume gradient error vs oracle {what}')


@gpu
@pytest.mark.parametrize('res,classes', [(8, (16, 288, 198, 10)), (9, (30, 400, 282, 17))])
def test_voxels_outside_the_cameras(res, classes, weights_trained_np):
    """bbox3d shifted by (+0.45, 0, 0): voxels seen by 0 / 1 / 2 / 3 views.  The SDF of a voxel no view sees is filled with 1, its
    gradient is NOT zero (about 1.0 - 1.5: through the keys and values the other rows of its column attend to)."""
    ref = _shifted(make_scene(0, 'cfg1')[0])
    o = oracle_gradient('trained', _torch_w(weights_trained_np), ref, res)
    counts = tuple(int((o['nviews'] == k).sum()) for k in range(4))
    assert counts == classes and min(counts) > 0, counts
    unseen = o['nviews'] == 0
    # (a kernel that zeroes them misses the bound by more than a hundred times)
    assert (o['sdf'][unseen] == 1.0).all() and np.linalg.norm(o['grad'][unseen], axis=-1).min() > 100 * ATOL_G
    grad, sdf = _grad(_hp('trained', weights_trained_np), [ref], res, want_sdf=True)
    close(_np(grad)[0], o['grad'], f'volume gradient vs oracle, shifted box R={res}', atol=ATOL_G)
    close(_np(grad)[0][unseen], o['grad'][unseen], f'volume gradient vs oracle, voxels no view sees R={res}', atol=ATOL_G)
    close(_np(sdf)[0], o['sdf'], f'volume gradient pass sdf vs oracle, shifted box R={res}')


@gpu
def test_batch_and_repeatability(weights_trained_np):
    hp = _hp('trained', weights_trained_np)
    refs = [make_scene(0, 'cfg1')[0], make_scene(1, 'cfg1')[0], _shifted(make_scene(0, 'cfg1')[0])]
    res = 9
    g3, s3, e3 = (_np(t) for t in _grad(hp, refs, res, want_sdf=True, want_error=True))
    for b, ref in enumerate(refs):
        g1, s1, e1 = (_np(t) for t in _grad(hp, [ref], res, want_sdf=True, want_error=True))
        assert np.array_equal(g3[b], g1[0]) and np.array_equal(s3[b], s1[0]) and np.array_equal(e3[b], e1[0]), f'scene {b} of the batch'
    again = [_np(t) for t in _grad(hp, refs, res, want_sdf=True, want_error=True)]
    assert np.array_equal(again[0], g3) and np.array_equal(again[1], s3) and np.array_equal(again[2], e3)
    for pattern in (0x7fc00000, 0x7149f2ca):                                   # NaN, 1e30 in every CU's LDS
        bref = _batch(refs)
        prep = hp.prepare(bref, res, grad_res=res)
        _lib.check(_lib.lib().gnr_debug_fill_lds(pattern, torch.cuda.current_stream().cuda_stream), 'gnr_debug_fill_lds')
        g, s, e = hp.sample_volume_gradient(bref, res, want_sdf=True, want_error=True, prepared=prep)
        assert np.array_equal(_np(g), g3) and np.array_equal(_np(s), s3) and np.array_equal(_np(e), e3), hex(pattern)
    # either order next to sample_volume on one prepared scene: both keep the bits they have alone
    bref = _batch(refs)
    vol = _np(hp.sample_volume(bref, res))
    prep = hp.prepare(bref, res, grad_res=res)
    ga = _np(hp.sample_volume_gradient(bref, res, prepared=prep))
    va = _np(hp.sample_volume(bref, res, prepared=prep))
    gb = _np(hp.sample_volume_gradient(bref, res, prepared=prep))
    prep = hp.prepare(bref, res, grad_res=res)
    vb = _np(hp.sample_volume(bref, res, prepared=prep))
    gc = _np(hp.sample_volume_gradient(bref, res, prepared=prep))
    assert np.array_equal(ga, g3) and np.array_equal(gb, g3) and np.array_equal(gc, g3)
    assert np.array_equal(va, vol) and np.array_equal(vb, vol)


@gpu
def test_range_guard_of_the_gradient_pass(weights_np):
    """Feature maps x3000 (tests/test_range_guard.py): the pass's own status slot is set, the gradient is finite and bitwise that of
    the fp32-MFMA chain forced to run alone; an in-range scene leaves the slot clear."""
    hp = _hp('seed0_guard', weights_np)
    ref, _ = make_scene(0, 'cfg1')
    big = dict(ref, ray_feats=ref['ray_feats'] * np.float32(3000.0), img_feats=ref['img_feats'] * np.float32(3000.0))

    def run(r):
        bref = _batch([r])
        prep = hp.prepare(bref, 16, grad_res=16)
        g, s, e = hp.sample_volume_gradient(bref, 16, want_sdf=True, want_error=True, prepared=prep)
        words = _np(hp.status_words(prep))
        return _np(g), _np(s), _np(e), words

    g, s, e, words = run(ref)
    assert words[_lib.STATUS_SLOT_VOLUME_GRAD] == 0 and words[_lib.STATUS_SLOT_VOLUME_GRAD_RAY] == 0 and not words.any()
    g, s, e, words = run(big)
    assert words[_lib.STATUS_SLOT_VOLUME_GRAD] & 2, words[:9]
    assert words[1] == 0 and words[2] == 0 and words[3] == 0, 'the other launch slots are not this pass\'s'
    assert np.isfinite(g).all() and np.isfinite(s).all() and np.isfinite(e).all()
    prev = hp.force_fp32_chain(True)
    try:
        g32, s32, e32, _ = run(big)
    finally:
        hp.force_fp32_chain(prev)
    assert np.array_equal(g, g32) and np.array_equal(s, s32) and np.array_equal(e, e32)


@gpu
def test_gather_rows_of_a_surface_cloud():
    from graspnerf_amd.grasp_post import SurfaceExtractor
    rng = np.random.default_rng(11)
    R, B = 9, 2
    grad = torch.from_numpy(rng.standard_normal((B, R, R, R, 3)).astype(np.float32)).cuda()
    vol = rng.uniform(-1, 1, (B, 1, R, R, R)).astype(np.float32)
    vol[1] = 0.9                                                              # a scene with no voxel in (-0.2, 0.2)
    vol = torch.from_numpy(vol).cuda()
    for max_points in (R ** 3, 40):
        out = SurfaceExtractor()(vol, max_points=max_points, gradient=grad)
        torch.cuda.synchronize()
        count, index, rows = _np(out['count']), _np(out['index']), _np(out['gradient'])
        assert rows.shape == (B, max_points, 3) and rows.dtype == np.float32
        assert count[1] == 0 and (count[0] > 40 if max_points == 40 else 40 < count[0] <= max_points)
        n = min(int(count[0]), max_points)
        i, j, k = index[0, :n].T
        assert np.array_equal(rows[0, :n], _np(grad)[0][i, j, k])
        assert not rows[1].any() and not rows[0, n:].any()


@gpu
def test_registered_operator_equals_the_ctypes_route(weights_np):
    from graspnerf_amd import torch_ops
    if not os.path.exists(torch_ops.LIB_PATH):
        pytest.skip('libgnr_torch.so was not built')
    ops = torch_ops.load()
    hp = _hp('seed0', weights_np)
    ref, _ = make_scene(0, 'cfg1')
    bref = _batch([ref])
    want = _np(hp.sample_volume_gradient(bref, 9))
    t = {k: torch.from_numpy(bref[k]).cuda() for k in ('imgs', 'img_feats', 'ray_feats', 'poses', 'Ks', 'depth_range')}
    bbox_min = torch.from_numpy(bref['bbox3d'][:, 0].copy()).cuda()
    args = (t['imgs'], t['img_feats'], t['ray_feats'], t['poses'], t['Ks'], t['depth_range'], bbox_min, hp.wc, 9)
    got = ops.sample_volume_gradient(*args)
    torch.cuda.synchronize()
    assert got.shape == (1, 9, 9, 9, 3) and np.array_equal(_np(got), want)
    with pytest.raises(RuntimeError):
        ops.sample_volume_gradient(*args[:7], hp.wc[:-1].contiguous(), 9)
