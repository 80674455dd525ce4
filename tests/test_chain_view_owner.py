"""One owner per (point, view) in the inference chain kernels (csrc/gnr_kernels.hip ViewRec).

Lane group v & 3 of a point projects view v and computes its taps, in rounds of four views (0..3, then 4..V-1 in the same
registers), every lane fetches the finished records, and a record waits in the state queue's row of its view until that view's
turn.  What can go wrong is ownership: the wrong lane group, the wrong round, a record fetched after the next round overwrote the
owner's registers, the wrong queue row at a view's turn, a mask bit of another view in the skip ballot.  So: tiny scenes with
V = 2, 4 (one round), 5, 6 (a partial round B), 8 (a full one), 125 volume points (seven full tiles and one of 13) and 3 x 7 ray
samples (one full tile and one of 5), and a last camera placed so that it sees NO point of one tile and exactly ONE point of
another -- in the volume and on the rays (checked on the CPU, on the oracle alone, before anything runs on the GPU)."""
import functools

import numpy as np
import pytest
import torch

from graspnerf_amd import weights
from graspnerf_amd.synth import ring_cameras
from oracle import graspnerf_oracle as O
from test_gpu_parity import close, ATOL, ATOL_A, ATOLS

VIEWS = [2, 4, 5, 6, 8]
H, W, RES, RN, DN = 32, 48, 5, 3, 7
MARGIN_PX = 1e-3          # no point of the scenes is closer than this to an image border: the masks are the same in any fp32 arithmetic


def _look_at(eye, tgt):
    eye, tgt = np.asarray(eye, np.float64), np.asarray(tgt, np.float64)
    zf = (tgt - eye) / np.linalg.norm(tgt - eye)
    xr = np.cross(zf, np.array([0.0, 0.0, 1.0]))
    xr /= np.linalg.norm(xr)
    R = np.stack([xr, np.cross(zf, xr), zf], 0)
    return np.concatenate([R, (-R @ eye)[:, None]], 1).astype(np.float32)


def make_tiny_scene(V, seed=0):
    """V - 1 cameras of the usual ring and a last one with a narrow field of view that looks past the workspace box; three query rays from
    a camera that is none of the reference views.  The seed only changes images and feature maps."""
    rng = np.random.default_rng(7000 + 10 * V + seed)
    poses = ring_cameras(V)
    poses[V - 1] = _look_at((0.45, 0.1, 0.4), (0.15, 0.2, 0.1))
    Ks = np.repeat(np.asarray([[[36.0, 0, 23.5], [0, 36.0, 15.5], [0, 0, 1]]], np.float32), V, 0).copy()
    Ks[V - 1, 0, 0] = Ks[V - 1, 1, 1] = 60.0
    ref = dict(imgs=rng.random((V, 3, H, W)).astype(np.float32),
               img_feats=(0.5 * rng.standard_normal((V, 32, H // 4, W // 4))).astype(np.float32),
               ray_feats=(0.5 * rng.standard_normal((V, 32, H // 4, W // 4))).astype(np.float32),
               poses=poses, Ks=Ks, depth_range=np.repeat(np.asarray([[0.2, 0.8]], np.float32), V, 0).copy(),
               bbox3d=np.asarray([[-0.15, -0.15, -0.05], [0.15, 0.15, 0.25]], np.float32))
    que = dict(coords=np.asarray([[10.0, 8.0], [24.0, 16.0], [40.0, 25.0]], np.float32), pose=ring_cameras(3)[1].copy(), K=Ks[0].copy(),
               depth_range=np.asarray([0.2, 0.8], np.float32), imgs=ref['imgs'][:1].copy())
    return ref, que


def _in_tiles(mask):
    """[V, P] bool in the kernel's point order -> [V, tiles]: points of the 16-point tile inside the view."""
    V, P = mask.shape
    m = np.concatenate([mask, np.zeros((V, (-P) % 16), bool)], 1)
    return m.reshape(V, -1, 16).sum(-1)


def _kernel_order(a):
    """[..., R*R*R] of the oracle's volume points (a column from the bottom up) -> the kernel's order (from the top down)."""
    return np.ascontiguousarray(a.reshape(a.shape[:-1] + (RES * RES, RES))[..., ::-1]).reshape(a.shape)


@functools.lru_cache(maxsize=None)
def _weights():
    import os
    from conftest import GOLDEN
    wnp = dict(np.load(os.path.join(GOLDEN, 'weights_seed0.npz')))
    return wnp, {k: torch.from_numpy(v) for k, v in wnp.items()}


@functools.lru_cache(maxsize=None)
def oracle_case(V):
    """Everything the tests compare against, computed once per view count: the scene, the oracle's volume and coarse pass on given
    depths, and its in-image masks [V, points] in the kernel's point order."""
    ref, que = make_tiny_scene(V)
    Wt = _weights()[1]
    dv, dr = {}, {}
    vol = O.sample_volume(Wt, O.to_torch(ref), RES, debug=dv).numpy()
    depth = O.sample_depth(torch.from_numpy(que['depth_range']), RN, DN)
    out = O.render_by_depth(Wt, O.to_torch(ref), O.to_torch(que), depth, 'dist_decoder.', 'agg_net.', O.DEFAULT_RENDER_CFG, debug=dr)
    pts, _ = O.ray_points(torch.from_numpy(que['coords']), torch.from_numpy(que['pose']), torch.from_numpy(que['K']), depth)
    uv_r, z_r, _, _ = O.project_points(pts.reshape(-1, 3), torch.from_numpy(ref['poses']), torch.from_numpy(ref['Ks']), H, W)

    def margin(uv, z):
        uv, z = uv.numpy(), z.numpy()
        return float(np.minimum.reduce([np.abs(uv[..., 0] + 0.5), np.abs(uv[..., 0] - (W - 0.5)), np.abs(uv[..., 1] + 0.5),
                                        np.abs(uv[..., 1] - (H - 0.5)), 1e3 * np.abs(np.abs(z) - 1e-4)]).min())
    return dict(ref=ref, que=que, vol=vol, depth=depth, out={k: v.numpy() for k, v in out.items()},
                vol_mask=_kernel_order(dv['mask'].numpy().reshape(V, -1)), ray_mask=dr['mask'].numpy().reshape(V, -1),
                margin=min(margin(dv['uv'], dv['z']), margin(uv_r, z_r)))


@pytest.mark.parametrize('V', VIEWS)
def test_the_oracle_alone_gives_both_mask_situations(V):
    """CPU: the last view sees nothing of one tile and exactly one point of another, among the volume tiles and among the ray tiles; the
    other views see (nearly) everything, so the tile is not skipped as a whole; no point sits within float noise of a border."""
    c = oracle_case(V)
    for name, mask, tiles in (('volume', c['vol_mask'], 8), ('rays', c['ray_mask'], 2)):
        n = _in_tiles(mask)
        assert n.shape == (V, tiles)
        assert (n[V - 1] == 0).any(), f'{name}: no tile entirely outside the last view: {n[V - 1]}'
        assert (n[V - 1] == 1).any(), f'{name}: no tile with exactly one point inside the last view: {n[V - 1]}'
        assert (n[0] >= 5).all(), f'{name}: view 0 should see every tile: {n[0]}'
    assert c['margin'] > MARGIN_PX, c['margin']


# ------------------------------------------------------------------------------------------------------------------ GPU
def _hp():
    from graspnerf_amd.hotpath import HotPath
    wnp = _weights()[0]
    return HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))


def _bits(mask):
    """[V, P] bool -> [P] uint8, bit v = view v."""
    return sum((mask[v].astype(np.uint8) << v) for v in range(mask.shape[0])).astype(np.uint8)


def _assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs'


@pytest.mark.gpu
@pytest.mark.parametrize('V', VIEWS)
def test_outputs_and_masks_match_the_oracle(V):
    from graspnerf_amd.hotpath import batch_scenes
    c = oracle_case(V)
    hp = _hp()
    bref, bque = batch_scenes([(c['ref'], c['que'])])
    prep = hp.prepare(bref, RES, RN, DN)
    vol, vm = hp.sample_volume(bref, RES, want_mask=True, prepared=prep)
    close(vol.cpu().numpy()[0], c['vol'][0], f'V={V} volume vs oracle')
    assert np.array_equal(vm.cpu().numpy().reshape(-1), _bits(c['vol_mask'])), f'V={V}: want_mask bits differ from the oracle'
    o = hp.render_by_depth(bref, bque, c['depth'][None], 'coarse', debug=True, prepared=prep)
    for k in ('sdf_values', 'alpha_values', 'hit_prob_nr', 'render_depth', 'colors_nr', 'pixel_colors_nr'):
        close(o[k].cpu().numpy(), c['out'][k], f'V={V} {k}', atol=ATOLS.get(k, ATOL_A))
    assert np.array_equal(o['ray_mask'].cpu().numpy(), c['out']['ray_mask'])
    assert np.array_equal(o['view_mask'].cpu().numpy().reshape(-1), _bits(c['ray_mask'])), f'V={V}: view_mask differs from the oracle'
    assert hp.range_status(prep) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('V', VIEWS)
def test_scene_0_alone_equals_scene_0_in_a_batch_of_three(V):
    """125 points are 8 tiles, 21 samples are 2: in the batch the tiles of scene 0 meet other wavefronts and other neighbours."""
    from graspnerf_amd.hotpath import batch_scenes
    c = oracle_case(V)
    hp = _hp()
    scenes = [(c['ref'], c['que'])] + [make_tiny_scene(V, s) for s in (1, 2)]
    depth = c['depth'][None]
    outs = []
    for group in (scenes[:1], scenes):
        bref, bque = batch_scenes(group)
        vol, vm = hp.sample_volume(bref, RES, want_mask=True)
        o = hp.render_by_depth(bref, bque, depth.repeat(len(group), 1, 1), 'coarse', debug=True)
        outs.append(dict({k: v[:1] for k, v in o.items()}, volume=vol[:1], volume_mask=vm[:1]))
    _assert_same(outs[0], outs[1], f'V={V} scene 0')


@pytest.mark.gpu
@pytest.mark.parametrize('V', VIEWS)
def test_a_random_sample_permutation_gives_the_same_bits(V):
    """The same points in other tiles and other lanes: another point of the tile inside the last view, another tile skipped."""
    from graspnerf_amd.hotpath import batch_scenes
    c = oracle_case(V)
    hp = _hp()
    bref, bque = batch_scenes([(c['ref'], c['que']), make_tiny_scene(V, 1)])
    depth = c['depth'][None].repeat(2, 1, 1)
    hp.set_option('sample_order_natural', True)
    want = hp.render_by_depth(bref, bque, depth, 'coarse', debug=True)
    g = torch.Generator().manual_seed(100 + V)
    perm = torch.stack([torch.randperm(RN * DN, generator=g) for _ in range(2)]).to(torch.int32)
    got = hp.debug_render_by_depth_perm(bref, bque, depth, perm, 'coarse', debug=True)
    _assert_same(got, want, f'V={V} random permutation')


@pytest.mark.gpu
@pytest.mark.parametrize('V', VIEWS)
def test_the_forced_fp32_chain_is_the_range_guard_fallback(V):
    """Feature maps x3000 (tests/test_range_guard.py) trip the watch of the pair launches; what comes out is the fp32 twin's, bit for bit."""
    from graspnerf_amd.hotpath import batch_scenes
    c = oracle_case(V)
    ref = dict(c['ref'], ray_feats=c['ref']['ray_feats'] * np.float32(3000), img_feats=c['ref']['img_feats'] * np.float32(3000))
    bref, bque = batch_scenes([(ref, c['que'])])
    depth = c['depth'][None]

    def run(hp):
        prep = hp.prepare(bref, RES, RN, DN)
        vol = hp.sample_volume(bref, RES, prepared=prep)
        o = hp.render_by_depth(bref, bque, depth, 'coarse', debug=True, prepared=prep)
        return dict(o, volume=vol), hp.range_status(prep)
    hp = _hp()
    guarded, flags = run(hp)
    assert flags & 2, f'V={V}: the x3000 scene should leave the fp16-pair range (flags {flags})'
    prev = hp.force_fp32_chain(True)
    try:
        forced, _ = run(hp)
    finally:
        hp.force_fp32_chain(prev)
    _assert_same(guarded, forced, f'V={V} range-guard fallback vs forced fp32 chain')
