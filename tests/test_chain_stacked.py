"""The K-stacked pair layers of k_chain's pair instantiations, through the inference launches (csrc/gnr_kernels.hip mm16s:
ray_dir_fc.2, rgb_fc.2 and the two extra k-steps of rgb_fc.0 on the f16 matrix cores; ST section of the blob, tests/test_pack_stacked.py) on the smallest shapes that
reach every path: 6-view scenes with 8 x 16 feature maps, an 8^3 volume (32 tiles) and 16 rays x (8 + 8) samples, one scene and a
batch of three different ones, with and without the fourth decoder branch (use_vis: instantiations of their own), 2 and 8 views
(other per-layer fences), and a pass whose last tile is partial.  pytest -m gpu.

(a) the product launch against the same call on the fp32-input MFMA alone (GNR_OPT_FP32_CHAIN), (b) against the fp32 CPU oracle --
both within the tolerances of tests/test_gpu_parity.py --, (c) the range guard end to end: an ELU output of ray_dir_fc.0 /
rgb_fc.0 beyond 65 520 is an operand of a stacked layer, the watch word must say so and every output must be the fp32 twin's.
(The training forward runs the same layers: tests/test_torch_ops.py holds its volume to the inference launch's bits, the gradient
tests of tests/test_train_step.py / test_bwd_twins.py / test_bwd_arbiter.py run behind it.)"""
import numpy as np
import pytest
import torch

from graspnerf_amd import weights
from graspnerf_amd.synth import make_scene
from oracle import graspnerf_oracle as O
from test_gpu_parity import ATOL, ATOL_A, ATOLS, close

pytestmark = pytest.mark.gpu

RES, RN, DN = 8, 16, 8
CFG = {'depth_sample_num': DN, 'fine_depth_sample_num': DN}
ORACLE_KEYS = ('sdf_values', 'alpha_values', 'hit_prob_nr', 'render_depth', 'colors_nr')


def _cfg(V, rn=RN):
    return dict(V=V, H=32, W=64, res=RES, rn=rn, K=[[50.0, 0, 31.5], [0, 50.0, 15.5], [0, 0, 1]])


@pytest.fixture(scope='module')
def sds(weights_np, golden):
    G = golden('cfg1_use_vis')
    return {False: weights_np, True: {**weights_np, **{k[len('weights.'):]: v for k, v in G.items() if k.startswith('weights.')}}}


@pytest.fixture(scope='module')
def hots(sds):
    from graspnerf_amd.hotpath import HotPath
    return {uv: HotPath(weights.pack_state_dict(sd, 'coarse'), weights.pack_state_dict(sd, 'fine')) for uv, sd in sds.items()}


def _forward(hp, bref, bque, cfg=CFG, res=RES, fine_depth_in=None):
    """-> ({name: numpy array} of every output of the volume launch and the two render passes, range word)."""
    rn = bque['coords'].shape[1]
    prep = hp.prepare(bref, res, rn, max(cfg['depth_sample_num'], cfg['fine_depth_sample_num']))
    out = {'volume': hp.sample_volume(bref, res, prepared=prep)}
    co, fi = hp.render(bref, bque, cfg, fine_depth_in=fine_depth_in, prepared=prep)
    flags = hp.range_status(prep)
    out.update({'coarse ' + k: v for k, v in co.items()})
    out.update({'fine ' + k: v for k, v in fi.items()})
    return {k: v.cpu().numpy() for k, v in out.items()}, flags


def _forced_fp32(hp, bref, bque, cfg=CFG, res=RES, fine_depth_in=None):
    prev = hp.force_fp32_chain(True)
    try:
        return _forward(hp, bref, bque, cfg, res, fine_depth_in)[0]
    finally:
        hp.force_fp32_chain(prev)


def _atol(name):
    return ATOL if name == 'volume' else ATOLS.get(name.split(' ', 1)[1], ATOL_A)


def _check_pair_vs_fp32_vs_oracle(hp, sd, scenes, tag, cfg=CFG, res=RES):
    from graspnerf_amd.hotpath import batch_scenes
    bref, bque = batch_scenes(scenes)
    out, flags = _forward(hp, bref, bque, cfg, res)
    assert flags == 0, f'{tag}: the pair kernels should have served these scenes (range word {flags})'
    # (the fine pass of both on the same sample positions: the pair launch's resampled depths)
    f32 = _forced_fp32(hp, bref, bque, cfg, res, fine_depth_in=out['fine depth'])
    for k, v in out.items():
        if v.dtype == np.float32:
            close(v, f32[k], f'{tag} pair vs fp32 chain: {k}', atol=_atol(k))
        else:
            assert np.array_equal(v, f32[k]), (tag, k)
    W = {k: torch.from_numpy(v) for k, v in sd.items()}
    for i, (ref, que) in enumerate(scenes):
        close(out['volume'][i], O.sample_volume(W, O.to_torch(ref), res).numpy()[0], f'{tag} scene {i} volume vs oracle')
        o = O.render(W, O.to_torch(ref), O.to_torch(que), cfg, fine_depth_override=torch.from_numpy(out['fine depth'][i]))
        for k in ORACLE_KEYS:
            close(out['coarse ' + k][i], o[k].numpy(), f'{tag} scene {i} coarse {k} vs oracle', atol=ATOLS.get(k, ATOL_A))
            close(out['fine ' + k][i], o[k + '_fine'].numpy(), f'{tag} scene {i} fine {k} vs oracle', atol=ATOLS.get(k, ATOL_A))
    return out


@pytest.mark.parametrize('use_vis', [False, True], ids=['plain', 'use_vis'])
@pytest.mark.parametrize('seeds', [(41,), (42, 43, 44)], ids=['B1', 'B3'])
def test_six_views(seeds, use_vis, hots, sds):
    scenes = [make_scene(s, _cfg(6)) for s in seeds]
    out = _check_pair_vs_fp32_vs_oracle(hots[use_vis], sds[use_vis], scenes, f'V=6 B={len(seeds)} use_vis={use_vis}')
    if len(seeds) > 1:                      # a batch whose scenes differ: every scene is bitwise its own launch
        from graspnerf_amd.hotpath import batch_scenes
        assert np.abs(out['volume'][0] - out['volume'][1]).max() > 1e-3
        for i, sc in enumerate(scenes):
            one, _ = _forward(hots[use_vis], *batch_scenes([sc]))
            for k in ('volume', 'coarse sdf_values', 'coarse colors_nr', 'coarse hit_prob_nr'):
                assert np.array_equal(one[k][0], out[k][i]), (i, k)


@pytest.mark.parametrize('V', [2, 8])
def test_other_view_counts(V, hots, sds):
    _check_pair_vs_fp32_vs_oracle(hots[False], sds[False], [make_scene(50 + V, _cfg(V))], f'V={V}')


@pytest.mark.parametrize('use_vis', [False, True], ids=['plain', 'use_vis'])
def test_partial_last_tile_in_a_batch_of_different_scenes(use_vis, hots, sds):
    """5 rays x 7 samples = 35 points per scene: two full tiles and one of three points, in both render passes."""
    cfg = {'depth_sample_num': 7, 'fine_depth_sample_num': 7}
    scenes = [make_scene(s, _cfg(6, rn=5)) for s in (61, 62, 63)]
    _check_pair_vs_fp32_vs_oracle(hots[use_vis], sds[use_vis], scenes, f'P=35 use_vis={use_vis}', cfg=cfg)


@pytest.mark.parametrize('layer', ['ray_dir_fc.0', 'rgb_fc.0'])
def test_range_guard_of_the_stacked_layers(layer, weights_np):
    """A bias of 1e5 drives the layer's ELU outputs -- the B operands of the stacked layer behind it (ray_dir_fc.2: both kinds of
    launch; rgb_fc.2: the render passes) -- past the fp16 range: bit 1 of the range word, and every output of the launches that
    run the layer bitwise the forced fp32-MFMA launch, as tests/test_range_guard.py requires of the other pair layers.
    An end-to-end guard: only the rgb_fc.0 case depends on the stacked layer's OWN watch (rgb_fc.2's outputs feed no further pair
    layer); behind ray_dir_fc.2 the garbage would also reach base_fc.0's watched operands."""
    from graspnerf_amd.hotpath import HotPath, batch_scenes
    w = dict(weights_np)
    for lvl in ('agg_net.', 'fine_agg_net.'):
        k = lvl + 'agg_impl.' + layer + '.bias'
        w[k] = np.full_like(w[k], 1e5)
    hp = HotPath(weights.pack_state_dict(w, 'coarse'), weights.pack_state_dict(w, 'fine'))
    bref, bque = batch_scenes([make_scene(71, _cfg(6))])
    out, flags = _forward(hp, bref, bque)
    assert flags & 2 == 2, (layer, flags)
    assert flags & 5 == 0, (layer, flags)
    f32 = _forced_fp32(hp, bref, bque)
    for k, v in out.items():
        assert np.isfinite(v.astype(np.float64)).all(), (layer, k)
        if k == 'volume' and layer == 'rgb_fc.0':
            # the volume launch has no colour head: nothing of it left the range, its watch word (one per launch) stays clear and
            # it remains the pair kernel's
            close(v, f32[k], 'rgb_fc.0 bias 1e5: volume, pair vs fp32 chain')
            assert not np.array_equal(v, f32[k])
        else:
            assert np.array_equal(v, f32[k]), f'{layer}: {k} differs from the forced fp32-MFMA launch'
