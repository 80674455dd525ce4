"""Range guard of the fp16-pair form and an fp64 arbiter for its accuracy claim (pytest -m gpu, through the C ABI).

The reference computes in fp32 everywhere (ibrnet.py:474-482; SURVEY.md 5: no mixed precision).  k_chain multiplies on the f16
matrix cores with every fp32 operand carried as an fp16 pair, whose high half cannot hold a magnitude of 65 520 or more
(DESIGN.md 4.1b).  include/gnr.h `gnr_range_status`: every chain launch watches its operands and is followed by its fp32-MFMA
twin, which recomputes the launch when the watch tripped.

* in range: the watch word stays 0 and the fp32 twin leaves the outputs alone;
* out of range (feature maps x3000: cross-view variances ~1e7; a feature of 1e5; weights that drive an ELU output past 65 504):
  the word is set, every output is finite and equals -- bitwise -- what the fp32-MFMA kernel produces when it is forced to run
  alone (`GNR_OPT_FP32_CHAIN`), and sits within the usual tolerance of the fp32 oracle on the same inputs;
* fp64 arbiter: on feature maps x1, x30 and x1e-3 and on decoder / geometry weights x3 the distance of the HIP path from the
  float64 evaluation of the oracle is compared with the distance of the fp32 oracle (the reference's arithmetic on the CPU)
  from it, over all 16^3 voxels (quantiles: single voxels can sit on a bilinear-tap edge where fp32 and fp64 pick
  different taps)."""
import numpy as np
import pytest
import torch

from graspnerf_amd import weights
from graspnerf_amd.synth import make_scene
from oracle import graspnerf_oracle as O
from conftest import PARITY_LOG

pytestmark = pytest.mark.gpu


def _hp(wnp):
    from graspnerf_amd.hotpath import HotPath
    return HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))


def _scaled(ref, f):
    return dict(ref, ray_feats=ref['ray_feats'] * np.float32(f), img_feats=ref['img_feats'] * np.float32(f))


def _run(hp, ref, que, cfg):
    from graspnerf_amd.hotpath import batch_scenes
    bref, bque = batch_scenes([(ref, que)])
    prep = hp.prepare(bref, 16, que['coords'].shape[0], 16)
    vol = hp.sample_volume(bref, 16, prepared=prep)
    co, fi = hp.render(bref, bque, cfg, prepared=prep)
    flags = hp.range_status(prep)
    return vol.cpu().numpy(), {k: v.cpu().numpy() for k, v in co.items()}, {k: v.cpu().numpy() for k, v in fi.items()}, flags


CFG = {'depth_sample_num': 16, 'fine_depth_sample_num': 16}


def _quantiles(e):
    e = np.sort(np.abs(e).reshape(-1))
    return {'median': float(e[len(e) // 2]), 'p99': float(e[int(0.99 * (len(e) - 1))]), 'max': float(e[-1]), 'rms': float(np.sqrt(np.mean(e ** 2)))}


def test_in_range_scene_does_not_trip_the_watch(weights_np):
    hp = _hp(weights_np)
    ref, que = make_scene(0, 'cfg1')
    vol, co, fi, flags = _run(hp, ref, que, CFG)
    assert flags == 0
    # x30 feature maps (activations in the hundreds, variances ~1e3) are still inside the pair form's range
    _, _, _, flags30 = _run(hp, _scaled(ref, 30.0), que, CFG)
    assert flags30 == 0


def _check_fallback(hp, wnp, ref, que, want_bits, tag):
    vol, co, fi, flags = _run(hp, ref, que, CFG)
    assert flags & want_bits == want_bits, (tag, flags)
    for name, arr in [('volume', vol)] + [('coarse ' + k, v) for k, v in co.items()] + [('fine ' + k, v) for k, v in fi.items()]:
        assert np.isfinite(arr.astype(np.float64)).all(), f'{tag}: {name} is not finite'
    # the values ARE the fp32-MFMA kernel's: force it and compare bitwise
    prev = hp.force_fp32_chain(True)
    try:
        vol32, co32, fi32, _ = _run(hp, ref, que, CFG)
    finally:
        hp.force_fp32_chain(prev)
    assert np.array_equal(vol, vol32), f'{tag}: volume differs from the forced fp32-MFMA launch'
    for k in co:
        assert np.array_equal(co[k], co32[k]), (tag, 'coarse', k)
        assert np.array_equal(fi[k], fi32[k]), (tag, 'fine', k)
    # and they are as good an fp32 evaluation as the oracle's: distance from the float64 arbiter, fp32 oracle next to it (such
    # inputs make the network thousands of times steeper, so two fp32 evaluations differ by far more than at unit scale)
    Wt = {k: torch.from_numpy(v) for k, v in wnp.items()}
    vol_o = O.sample_volume(Wt, O.to_torch(ref), 16).numpy().astype(np.float64)
    with O.fp64_mode():
        vol64 = O.sample_volume({k: v.double() for k, v in Wt.items()}, O.to_torch64(ref), 16).numpy()
    qh, qo = _quantiles(vol.astype(np.float64) - vol64), _quantiles(vol_o - vol64)
    PARITY_LOG.append({'what': f'range guard {tag}: volume vs fp64', 'hip_fallback_vs_fp64': qh, 'fp32_oracle_vs_fp64': qo,
                       'max_abs_err': qh['max'], 'max_over_tol': qh['rms'] / (3 * qo['rms'] + 1e-6)})
    assert qh['rms'] <= 3.0 * qo['rms'] + 1e-6, (tag, qh, qo)
    assert qh['p99'] <= 3.0 * qo['p99'] + 1e-5, (tag, qh, qo)
    return flags


def test_feature_maps_x3000_fall_back_to_fp32(weights_np):
    """|feature| ~ 7e3 (inside +-6e4), cross-view variances ~ 5e7: the hoisted base_fc.0 operands leave the fp16 range."""
    hp = _hp(weights_np)
    ref, que = make_scene(0, 'cfg1')
    flags = _check_fallback(hp, weights_np, _scaled(ref, 3000.0), que, 2, 'features x3000')
    assert flags & 1 == 0


def test_one_huge_or_nonfinite_feature_is_caught_in_prepare(weights_np):
    hp = _hp(weights_np)
    ref, que = make_scene(0, 'cfg1')
    big = dict(ref, ray_feats=ref['ray_feats'].copy())
    big['ray_feats'][1, 7, 10, 13] = 1e5
    _check_fallback(hp, weights_np, big, que, 1, 'one feature = 1e5')
    from graspnerf_amd.hotpath import batch_scenes
    bad = dict(ref, img_feats=ref['img_feats'].copy())
    bad['img_feats'][0, 3, 5, 5] = np.inf
    bref, _ = batch_scenes([(bad, que)])
    prep = hp.prepare(bref, 16)
    assert hp.range_status(prep) & 1


def test_weights_that_drive_an_activation_past_the_fp16_range(weights_np):
    """base_fc.0 x 3e4: its ELU outputs (the operands of base_fc.2) reach ~1e5 with feature maps of unit scale."""
    w = dict(weights_np)
    for lvl in ('agg_net.', 'fine_agg_net.'):
        for s in ('weight', 'bias'):
            k = lvl + 'agg_impl.base_fc.0.' + s
            w[k] = (w[k] * np.float32(3e4)).astype(np.float32)
    hp = _hp(w)
    ref, que = make_scene(0, 'cfg1')
    _check_fallback(hp, w, ref, que, 2, 'base_fc.0 x3e4')


def test_a_weight_without_an_fp16_pair_runs_on_the_fp32_twin(weights_np):
    """mean_decoder.0 (a layer whose operands are the bounded feature maps, i.e. not watched inside the kernel) with one weight of
    1e5: the packer marks the blob (bit 2) and the launches are the fp32 twin's."""
    w = dict(weights_np)
    for lvl in ('dist_decoder.', 'fine_dist_decoder.'):
        k = lvl + 'mean_decoder.0.weight'
        w[k] = w[k].copy()
        w[k][3, 5] = 1e5
    hp = _hp(w)
    ref, que = make_scene(0, 'cfg1')
    _check_fallback(hp, w, ref, que, 4, 'mean_decoder.0 weight = 1e5')


@pytest.mark.parametrize('rn', [64, 50])
def test_stale_lds_does_not_reach_the_outputs(rn, weights_np):
    """LDS is not cleared between kernels.  64 rays of 16 samples are 14 rays per k_ray workgroup: the last workgroup holds eight
    rays and six ray slots whose lanes shadow the last ray on LDS nobody wrote.  Those lanes take part in the barriers -- and, since
    round 6, would take part in the workgroup's vote for the plain-chain column pass (csrc/gnr_kernels.hip: `exact`): they must not,
    or the last rays' SDF gradients depend on what earlier kernels left behind (found as a one-ulp difference between a launch and
    its repeat that only showed after the x3000 scene had run; a build with docs/experiments/shadow_vote_bug.patch applied fails here).  The whole forward
    after gnr_debug_fill_lds(0), after a NaN pattern and after 1e30: the same bits, SDF gradient included."""
    from graspnerf_amd import _lib
    from graspnerf_amd.hotpath import batch_scenes
    ref, que = make_scene(0, 'cfg1')
    que = dict(que, coords=que['coords'][:rn])
    hp = _hp(weights_np)
    bref, bque = batch_scenes([(ref, que)])

    def run(pattern):
        prep = hp.prepare(bref, 16, rn, 16)
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().gnr_debug_fill_lds(pattern, s), 'gnr_debug_fill_lds')
        vol = hp.sample_volume(bref, 16, prepared=prep)
        _lib.check(_lib.lib().gnr_debug_fill_lds(pattern, s), 'gnr_debug_fill_lds')
        co, fi = hp.render(bref, bque, CFG, debug=True, prepared=prep)[:2]
        assert hp.range_status(prep) == 0
        return {**{'coarse ' + k: v.cpu().numpy() for k, v in co.items()}, **{'fine ' + k: v.cpu().numpy() for k, v in fi.items()}, 'volume': vol.cpu().numpy()}
    zero = run(0)
    assert 'coarse sdf_gradient' in zero and np.isfinite(zero['coarse sdf_gradient']).all()
    for pattern in (0x7fc00000, 0x7149f2ca):          # NaN, 1e30
        got = run(pattern)
        for k in zero:
            assert np.array_equal(zero[k], got[k], equal_nan=True), (hex(pattern), k)


@pytest.mark.parametrize('key,ij', [('agg_impl.geometry_fc.2.weight', (3, 5)), ('agg_impl.ray_attention.w_ks.weight', (2, 9)),
                                    ('agg_impl.geometry_fc.0.weight', (7, 70))])
def test_a_k_ray_weight_without_an_fp16_pair_runs_on_the_fp32_twin(key, ij, weights_np):
    """The dense tail of k_ray<true>'s in-forward VJP multiplies on the f16 matrix cores ([Wq;Wk;Wv]^T, geometry_fc.2^T, geometry_fc.0^T:
    csrc/gnr_kernels.hip).  A weight of 1e5 has no fp16 pair: the packer stores inf for it, the tail's outputs turn non-finite, the
    launch's watch word (bit 1 of gnr_range_status) makes the fp32 instantiation behind the launch recompute it -- the SDF gradient is the
    fp32 one (oracle autograd to 1e-3), everything is finite."""
    from graspnerf_amd.hotpath import batch_scenes
    w = dict(weights_np)
    w['agg_net.' + key] = w['agg_net.' + key].copy()
    w['agg_net.' + key][ij] = 1e5
    hp = _hp(w)
    ref, que = make_scene(0, 'cfg1')
    bref, bque = batch_scenes([(ref, que)])
    dn = 16
    depth = O.sample_depth(torch.from_numpy(que['depth_range']), que['coords'].shape[0], dn)
    prep = hp.prepare(bref, 1, que['coords'].shape[0], dn)
    o = hp.render_by_depth(bref, bque, depth[None], 'coarse', debug=True, prepared=prep)
    flags = hp.range_status(prep)
    assert flags & 2, flags
    dbg = {}
    Wt = {k: torch.from_numpy(v) for k, v in w.items()}
    O.render_by_depth(Wt, O.to_torch(ref), O.to_torch(que), depth, 'dist_decoder.', 'agg_net.', O.DEFAULT_RENDER_CFG, debug=dbg)
    got, want = o['sdf_gradient'].cpu().numpy()[0].astype(np.float64), dbg['grad'].numpy().astype(np.float64)
    assert np.isfinite(got).all() and all(np.isfinite(v.float().cpu().numpy()).all() for v in o.values())
    assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())
    # and an in-range scene on the same workspace afterwards: a new prepare clears the watch
    hp2 = _hp(weights_np)
    prep2 = hp2.prepare(bref, 1, que['coords'].shape[0], dn)
    hp2.render_by_depth(bref, bque, depth[None], 'coarse', debug=True, prepared=prep2)
    assert hp2.range_status(prep2) == 0


@pytest.mark.parametrize('regime', ['x1', 'features x30', 'features x1e-3', 'decoder+geometry weights x3'])
def test_fp64_arbiter(regime, weights_np):
    """|HIP - fp64| against |fp32 oracle - fp64| on the volume (16^3) and the coarse sdf / alpha of 64 rays.  The HIP path uses
    hardware exp / log / rcp approximations where torch calls libm, so it is not expected to be CLOSER to fp64 than torch's
    fp32; the requirement is the same distance: rms within 1.5x and 99th percentile within 2x of the fp32 oracle's (measured rms
    ratios 0.8 - 1.15 over the four regimes, e.g. x1 volume 2.6e-7 against 2.8e-7, features x30 1.6e-5 against 1.8e-5:
    profiles/r03_*_parity_errors.json), and the pair form no further away than the forced fp32-MFMA kernel by more than 1.5x."""
    w = dict(weights_np)
    ref, que = make_scene(0, 'cfg1')
    if regime == 'features x30':
        ref = _scaled(ref, 30.0)
    elif regime == 'features x1e-3':
        ref = _scaled(ref, 1e-3)
    elif regime.startswith('decoder'):
        for k in list(w):
            if ('mean_decoder' in k or 'var_decoder' in k or 'geometry_fc' in k) and k.endswith('weight'):
                w[k] = (w[k] * np.float32(3.0)).astype(np.float32)
    hp = _hp(w)
    vol, co, fi, flags = _run(hp, ref, que, CFG)
    assert flags == 0
    prev = hp.force_fp32_chain(True)
    try:
        vol_m, co_m, _, _ = _run(hp, ref, que, CFG)
    finally:
        hp.force_fp32_chain(prev)
    Wt = {k: torch.from_numpy(v) for k, v in w.items()}
    vol32 = O.sample_volume(Wt, O.to_torch(ref), 16).numpy().astype(np.float64)
    r32 = O.render(Wt, O.to_torch(ref), O.to_torch(que), CFG)
    with O.fp64_mode():
        W64 = {k: v.double() for k, v in Wt.items()}
        vol64 = O.sample_volume(W64, O.to_torch64(ref), 16).numpy()
        r64 = O.render(W64, O.to_torch64(ref), O.to_torch64(que), CFG)
    for name, hip, hip32, o32, o64 in [('volume', vol, vol_m, vol32, vol64)] + \
            [('coarse ' + k, co[k], co_m[k], r32[k].numpy().astype(np.float64), r64[k].numpy()) for k in ('sdf_values', 'alpha_values')]:
        qh, qm, qo = _quantiles(hip.astype(np.float64) - o64), _quantiles(hip32.astype(np.float64) - o64), _quantiles(o32 - o64)
        PARITY_LOG.append({'what': f'fp64 arbiter {regime}: {name}', 'hip_pairs_vs_fp64': qh, 'hip_fp32mfma_vs_fp64': qm, 'fp32_oracle_vs_fp64': qo,
                           'max_abs_err': qh['max'], 'max_over_tol': qh['rms'] / (1.5 * qo['rms'] + 1e-12)})
        assert qh['rms'] <= 1.5 * qo['rms'] + 1e-7, (regime, name, qh, qo)
        assert qh['p99'] <= 2.0 * qo['p99'] + 2e-7, (regime, name, qh, qo)
        assert qh['rms'] <= 1.5 * qm['rms'] + 1e-7, (regime, name, 'pair form vs fp32-MFMA kernel', qh, qm)


CFG_FULL = {'depth_sample_num': 40, 'fine_depth_sample_num': 40}


@pytest.mark.parametrize('case', ['cfg2 scene alone', 'scenes 0 and 17 of the B=32 bench batch'])
def test_fp64_arbiter_benched_shape(case, weights_np):
    _arbiter_benched_shape(case, weights_np)


def test_fp64_arbiter_on_weights_an_optimiser_has_moved(weights_trained_np, weights_np):
    """The same arbiter, same bounds, on hot-path weights after 1 000 Adam steps of this repository's trainer (tools/train_probe.py: HIP path in
    both directions, the reference's losses, synthetic scenes; lr 1e-3: the tensors moved by a median of 17 % and up to 170 % from the trainer's initialisation -- recorded in
    profiles/r06_g_train_probe.json, where no sampled step's forward or backward tripped the range guard).  Not a trained GraspNeRF -- there is
    none in this environment -- but weights whose dynamic ranges an optimiser chose, not a seeded generator: the pair form's distance from
    float64 stays within the fp32 oracle's, and no launch falls back to its fp32 twin."""
    assert set(weights_trained_np) == set(weights_np) and all(np.isfinite(v).all() for v in weights_trained_np.values())
    _arbiter_benched_shape('cfg2 scene alone', weights_trained_np, tag=' [optimiser-moved weights]')


def _arbiter_benched_shape(case, weights_np, tag=''):
    """The same arbiter at the shape bench.py times (BASELINE configs[1] / configs[2]): 6 views of 288x512, 40^3 voxels, 512 rays x
    (40 coarse + 40 fine) samples -- where the unscaled-residual floor of the inner layers (gnr_kernels.hip "unscaled activation pairs") meets
    6-view statistics.  |HIP pair form - fp64| against |fp32 oracle - fp64| over every voxel and every coarse / fine sample (the fine
    pass of both oracles runs on the HIP path's resampled depths: the resampler is compared elsewhere, this test is about arithmetic).
    Requirement as at 16^3: rms within 1.5x and 99th percentile within 2x of the fp32 oracle's distance."""
    from graspnerf_amd.hotpath import batch_scenes
    hp = _hp(weights_np)
    if case.startswith('cfg2'):
        ids, pick = [0], [0]
    else:
        ids, pick = list(range(32)), [0, 17]
    scenes = [make_scene(i, 'cfg2') for i in ids]
    bref, bque = batch_scenes(scenes)
    prep = hp.prepare(bref, 40, 512, 40)
    vol = hp.sample_volume(bref, 40, prepared=prep).cpu().numpy()
    co, fi = hp.render(bref, bque, CFG_FULL, prepared=prep)
    assert hp.range_status(prep) == 0
    prev = hp.force_fp32_chain(True)
    try:
        prep_m = hp.prepare(bref, 40, 512, 40)
        vol_m = hp.sample_volume(bref, 40, prepared=prep_m).cpu().numpy()
    finally:
        hp.force_fp32_chain(prev)
    co = {k: v.cpu().numpy() for k, v in co.items()}
    fi = {k: v.cpu().numpy() for k, v in fi.items()}
    Wt = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    W64 = {k: v.double() for k, v in Wt.items()}
    for s in pick:
        ref, que = scenes[s]
        fd = torch.from_numpy(fi['depth'][s])
        vol32 = O.sample_volume(Wt, O.to_torch(ref), 40).numpy().astype(np.float64)
        r32 = O.render(Wt, O.to_torch(ref), O.to_torch(que), CFG_FULL, fine_depth_override=fd)
        with O.fp64_mode():
            vol64 = O.sample_volume(W64, O.to_torch64(ref), 40).numpy()
            r64 = O.render(W64, O.to_torch64(ref), O.to_torch64(que), CFG_FULL, fine_depth_override=fd.double())
        rows = [('volume', vol[s], vol32[0], vol64[0])]
        for k in ('sdf_values', 'alpha_values'):
            rows.append(('coarse ' + k, co[k][s], r32[k].numpy().astype(np.float64), r64[k].numpy()))
            rows.append(('fine ' + k, fi[k][s], r32[k + '_fine'].numpy().astype(np.float64), r64[k + '_fine'].numpy()))
        for name, hip, o32, o64 in rows:
            qh, qo = _quantiles(hip.astype(np.float64).reshape(o64.shape) - o64), _quantiles(o32.reshape(o64.shape) - o64)
            PARITY_LOG.append({'what': f'fp64 arbiter, benched shape ({case}, scene {ids[s]}){tag}: {name}', 'hip_pairs_vs_fp64': qh,
                               'fp32_oracle_vs_fp64': qo, 'rms_ratio': qh['rms'] / (qo['rms'] + 1e-30), 'p99_ratio': qh['p99'] / (qo['p99'] + 1e-30),
                               'max_abs_err': qh['max'], 'max_over_tol': qh['rms'] / (1.5 * qo['rms'] + 1e-12)})
            assert qh['rms'] <= 1.5 * qo['rms'] + 1e-7, (case, s, name, qh, qo)
            assert qh['p99'] <= 2.0 * qo['p99'] + 2e-7, (case, s, name, qh, qo)
        qm = _quantiles(vol_m[s].astype(np.float64).reshape(vol64[0].shape) - vol64[0])
        qh = _quantiles(vol[s].astype(np.float64).reshape(vol64[0].shape) - vol64[0])
        assert qh['rms'] <= 1.5 * qm['rms'] + 1e-7, (case, s, 'pair form vs fp32-MFMA kernel', qh, qm)
