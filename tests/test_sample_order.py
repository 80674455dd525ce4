"""Sample order of the inference render passes (include/gnr.h "sample order", csrc/gnr_sample_order.h).

The chain kernel skips a view for a 16-sample tile only when all 16 samples lie outside it, so a render pass groups a scene's samples
by their view-mask byte before its chain launch.  A point's outputs do not depend on its tile, hence the contract:

* CPU: the order rule (host twin `gnr_sample_order_host`) is a bijection with the stated structure, and on the cfg2 scenes it
  reaches the share of skippable (tile, view) pairs that plain grouping by mask reaches (tools/maskstat.py);
* GPU: the device sort equals the host twin; every output of render() / render_by_depth() is torch.equal between the default order
  and GNR_OPT_SAMPLE_ORDER_NATURAL, also for a caller-given RANDOM permutation (a wrong key or order cannot change a result), and a
  range-flagged ordered launch is bitwise the forced fp32 launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, weights
from graspnerf_amd.synth import CONFIGS, make_scene
from conftest import GOLDEN

STRIPES, TILE = 8, 16


def host_order(keys):
    keys = np.ascontiguousarray(keys, np.uint8)
    perm = np.full(len(keys), -1, np.int32)
    _lib.check(_lib.lib().gnr_sample_order_host(keys.ctypes.data_as(C.c_void_p), len(keys), perm.ctypes.data_as(C.c_void_p)), 'gnr_sample_order_host')
    return perm


def stripe_ranges(P):
    """[(first tile, end tile)] of the 8 stripes of a scene with P samples (csrc/gnr_sample_order.h stripe_tiles)."""
    tps = (P + TILE - 1) // TILE
    out, t = [], 0
    for s in range(STRIPES):
        n = max((tps - s + STRIPES - 1) // STRIPES, 0)
        out.append((t, t + n))
        t += n
    assert t == tps
    return out


def _key_arrays(P, rng):
    few = rng.choice(256, 5, replace=False).astype(np.uint8)
    return {'single key': np.full(P, 0x2d, np.uint8),
            'all 256 keys': rng.integers(0, 256, P).astype(np.uint8),
            'five keys': few[rng.integers(0, 5, P)],
            '6-view masks in runs': np.repeat(rng.integers(0, 64, (P + 6) // 7).astype(np.uint8), 7)[:P]}


# P < 16, P not a multiple of 16, fewer tiles than stripes, one tile more / less than a multiple of 8 tiles, the benched 20 480
SIZES = [1, 5, 15, 16, 17, 100, 127, 128, 129, 143, 1000, 2049, 20480, 20481]


@pytest.mark.parametrize('P', SIZES)
def test_host_order_is_a_bijection_with_the_stated_structure(P):
    rng = np.random.default_rng(P)
    pop = np.array([bin(k).count('1') for k in range(256)])
    for name, keys in _key_arrays(P, rng).items():
        perm = host_order(keys)
        assert np.array_equal(np.sort(perm), np.arange(P)), (name, 'not a bijection')
        assert np.array_equal(host_order(keys), perm), (name, 'not repeatable')
        ks = keys[perm]                                             # key of every slot
        tiles_with = np.zeros((STRIPES, 256), np.int64)             # per stripe and key: tiles that hold it, samples
        samples = np.zeros((STRIPES, 256), np.int64)
        for s, (t0, t1) in enumerate(stripe_ranges(P)):
            k = ks[t0 * TILE:min(t1 * TILE, P)]
            if len(k) == 0:
                continue
            # popcount never rises along a stripe, equal keys are one run
            assert (np.diff(pop[k]) <= 0).all(), (name, s, 'popcount rises along the stripe')
            starts = np.flatnonzero(np.diff(k.astype(np.int32)) != 0) + 1
            run_keys = k[np.concatenate([[0], starts])]
            assert len(np.unique(run_keys)) == len(run_keys), (name, s, 'a key appears in two runs of a stripe')
            samples[s] = np.bincount(k, minlength=256)
            for t in range(t0, t1):
                tiles_with[s, np.unique(ks[t * TILE:min((t + 1) * TILE, P)])] += 1
        # The sorted 16-sample groups are dealt round-robin: a key's run covers consecutive groups, so two stripes hold it in numbers of
        # tiles that differ by at most one; its first and last group may be partial, so in samples by less than two groups.
        assert (tiles_with.max(0) - tiles_with.min(0) <= 1).all(), (name, 'stripes differ by more than one group')
        assert (samples.max(0) - samples.min(0) < 2 * TILE).all(), name


def test_within_a_key_the_order_is_the_sample_order():
    """Stable: the samples of one key keep their order along the sorted sequence (the device sort reproduces it: wavefront segments in order,
    lanes in order).  Checked on one stripe-free case: fewer tiles than stripes, every tile its own stripe."""
    keys = np.array([3, 1, 3, 7, 1, 3, 7, 7, 1, 1, 3, 3, 7, 1, 3, 3, 3, 1], np.uint8)
    perm = host_order(keys)
    seq = perm.tolist()                                             # 2 tiles = stripes 0 and 1 in order = the sorted sequence itself
    for k in (1, 3, 7):
        idx = [i for i in seq if keys[i] == k]
        assert idx == sorted(idx)
    assert keys[perm].tolist() == sorted(keys.tolist(), key=lambda k: (-bin(k).count('1'), -k))


# DESIGN 4.1 / tools/maskstat.py: share of skippable (tile, view) pairs when the samples of scenes 0, 1, 7, 19, 31 of cfg2 are grouped by mask
TABLE_GROUPED = {'coarse': 17.3, 'fine': 26.6}


def test_cfg2_scenes_reach_the_grouped_share_of_skipped_tiles():
    """Keys from the oracle's projection (coarse: its disparity-uniform depths; fine: its resampled depths, recorded by
    tools/maskstat.py --write-golden), order from the host twin: within 0.5 points of the table's grouped column."""
    from tools import maskstat
    fd = np.load(os.path.join(GOLDEN, 'maskstat_cfg2_fine_depth.npz'))
    share = {'coarse': [], 'fine': []}
    masked = {'coarse': [], 'fine': []}
    for sid in maskstat.SCENES:
        for name, keys in zip(('coarse', 'fine'), maskstat.pass_keys(sid, fd[f'scene{sid}'])):
            share[name].append(maskstat.skipped_share(keys, 6, host_order(keys)))
            masked[name].append(maskstat.masked_share(keys, 6))
    for name, want in TABLE_GROUPED.items():
        got = 100 * float(np.mean(share[name]))
        print(f'{name}: skipped (tile, view) pairs under the order {got:.2f} % (table {want} %, masked pairs {100 * float(np.mean(masked[name])):.2f} %)')
        assert want - 0.5 <= got <= 100 * float(np.mean(masked[name])), (name, got)


# ---------------------------------------------------------------------------------------------------------------- GPU
CFG = {'depth_sample_num': 40, 'fine_depth_sample_num': 40}


def _hp(wnp):
    from graspnerf_amd.hotpath import HotPath
    return HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))


@pytest.fixture(scope='module')
def bench_batch():
    """The 32 cfg2 scenes of the benched batch; B = 4 is its first four."""
    from graspnerf_amd.hotpath import batch_scenes
    bref, bque = batch_scenes([make_scene(i, 'cfg2') for i in range(32)])

    def take(B):
        return {k: v[:B] for k, v in bref.items()}, {k: v[:B] for k, v in bque.items()}
    return take


def _assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs'


@pytest.mark.gpu
@pytest.mark.parametrize('P', [5, 16, 143, 2049, 20480, 20481])
def test_device_sort_equals_the_host_twin(P, weights_np):
    hp = _hp(weights_np)
    rng = np.random.default_rng(100 + P)
    arrays = list(_key_arrays(P, rng).values())
    perm = hp.debug_sample_order(torch.from_numpy(np.stack(arrays))).cpu().numpy()
    for keys, row in zip(arrays, perm):
        assert np.array_equal(row, host_order(keys))


def _clear_order_state(hp, prep, rn, dn_max, P):
    """Zero the keys and the permutation of a prepared workspace, so that what _assert_pass_ordered reads was written by the pass under test."""
    keys, perm = hp.sample_order_state(rn, dn_max, P, prep)
    keys.zero_()
    perm.zero_()


def _assert_pass_ordered(hp, prep, rn, dn_max, P, tag):
    """The last pass on `prep` did order its samples: its permutation is the host twin's on its own keys (a pass in the natural order leaves
    the cleared state: zeros, no permutation).  -> keys"""
    keys, perm = hp.sample_order_state(rn, dn_max, P, prep)
    keys, perm = keys.cpu().numpy(), perm.cpu().numpy()
    for b in range(len(keys)):
        assert np.array_equal(perm[b], host_order(keys[b])), f'{tag}: scene {b} was not ordered by the pass'
    return keys


# 16 scenes x 1280 tiles is the smallest power of two above the 8 tiles per wavefront slot from which a pass orders its samples (include/gnr.h)
ORDERED_FROM = 16


@pytest.mark.gpu
@pytest.mark.parametrize('B', [4, 16, 32])
@pytest.mark.parametrize('mode', ['default', 'fp32_chain', 'ray_order_morton'])
def test_render_outputs_do_not_depend_on_the_sample_order(B, mode, weights_np, bench_batch):
    """Every coarse and fine output of render() with the debug extras (sdf_gradient, view_mask, fine_inds).  B = 16, 32: the passes order
    their samples, and the test says so; B = 4 launches too few tiles, its passes keep the natural order under either setting."""
    hp = _hp(weights_np)
    if mode != 'default':
        hp.set_option(mode, True)
    bref, bque = bench_batch(B)
    rn, dn = bque['coords'].shape[1], CFG['fine_depth_sample_num']
    prep = hp.prepare(bref, 1, rn, dn)
    _clear_order_state(hp, prep, rn, dn, rn * dn)
    co, fi, inds = hp.render(bref, bque, CFG, debug=True, prepared=prep)
    if B >= ORDERED_FROM:
        # the last (fine) pass: its keys are the kernel's own masks, its permutation the host twin's
        keys = _assert_pass_ordered(hp, prep, rn, dn, rn * dn, f'B={B} {mode}')
        if mode != 'ray_order_morton':                              # (Morton: the keys are in the rays' internal order, view_mask in the caller's)
            assert np.array_equal(keys, fi['view_mask'].reshape(B, -1).cpu().numpy())
    hp.set_option('sample_order_natural', True)
    co_n, fi_n, inds_n = hp.render(bref, bque, CFG, debug=True, prepared=prep)
    _assert_same(co, co_n, f'B={B} {mode} coarse')
    _assert_same(fi, fi_n, f'B={B} {mode} fine')
    assert torch.equal(inds, inds_n)
    assert hp.range_status(prep) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('level', ['coarse', 'fine'])
def test_render_by_depth_does_not_depend_on_the_sample_order(level, weights_np, bench_batch):
    """gnr_render_by_depth_fwd on given depths at B = 32: the pass orders its samples (asserted), every output equals the natural order's."""
    hp = _hp(weights_np)
    B = 32
    bref, bque = bench_batch(B)
    co, fi = hp.render(bref, bque, CFG)
    depth = (co if level == 'coarse' else fi)['depth'].clone()
    rn, dn = depth.shape[1:]
    prep = hp.prepare(bref, 1, rn, dn)
    _clear_order_state(hp, prep, rn, dn, rn * dn)
    a = hp.render_by_depth(bref, bque, depth, level, debug=True, prepared=prep)
    keys = _assert_pass_ordered(hp, prep, rn, dn, rn * dn, f'render_by_depth {level}')
    assert np.array_equal(keys, a['view_mask'].reshape(B, -1).cpu().numpy())
    hp.set_option('sample_order_natural', True)
    b = hp.render_by_depth(bref, bque, depth, level, debug=True, prepared=prep)
    _assert_same(a, b, f'render_by_depth {level}')


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['cfg1 37 rays x 19 (703 points)', 'cfg1 5 rays x 3 (15 points)', 'cfg2 B=4'])
@pytest.mark.parametrize('mode', ['default', 'fp32_chain', 'ray_order_morton'])
def test_a_random_permutation_gives_the_same_bits(case, mode, weights_np, bench_batch):
    """The invariant itself: a caller-given random permutation of every scene's samples, the identity, and the device sort of RANDOM keys
    (wrong keys) all give the natural order's outputs."""
    from graspnerf_amd.hotpath import batch_scenes
    hp = _hp(weights_np)
    if mode != 'default':
        hp.set_option(mode, True)
    if case.startswith('cfg2'):
        bref, bque = bench_batch(4)
        dn = 40
    else:
        rn, dn = (37, 19) if '37' in case else (5, 3)
        bref, bque = batch_scenes([make_scene(i, dict(CONFIGS['cfg1'], rn=rn)) for i in range(2)])
    B, rn = bque['coords'].shape[:2]
    P = rn * dn
    g = torch.Generator().manual_seed(P)
    depth = torch.sort(0.25 + 0.5 * torch.rand(B, rn, dn, generator=g), -1)[0]
    hp.set_option('sample_order_natural', True)
    want = hp.render_by_depth(bref, bque, depth, 'coarse', debug=True)
    perms = {'random': torch.stack([torch.randperm(P, generator=g) for _ in range(B)]).to(torch.int32),
             'identity': torch.arange(P, dtype=torch.int32).repeat(B, 1),
             'sort of random keys': hp.debug_sample_order(torch.randint(0, 256, (B, P), generator=g).to(torch.uint8))}
    for name, perm in perms.items():
        got = hp.debug_render_by_depth_perm(bref, bque, depth, perm, 'coarse', debug=True)
        _assert_same(got, want, f'{case} {mode} {name}')


@pytest.mark.gpu
def test_a_range_flagged_ordered_launch_is_the_forced_fp32_launch(weights_np, bench_batch):
    """Feature maps x3000 (tests/test_range_guard.py): the ordered pair launches trip their watch, the fp32 twin recomputes them in the same
    order -> bitwise the forced fp32 launch in the natural order."""
    hp = _hp(weights_np)
    bref, bque = bench_batch(32)                                    # (a launch size whose passes order their samples)
    bref = dict(bref, ray_feats=bref['ray_feats'] * np.float32(3000), img_feats=bref['img_feats'] * np.float32(3000))
    rn, dn = bque['coords'].shape[1], CFG['fine_depth_sample_num']
    prep = hp.prepare(bref, 1, rn, dn)
    _clear_order_state(hp, prep, rn, dn, rn * dn)
    co, fi = hp.render(bref, bque, CFG, prepared=prep)
    assert hp.range_status(prep) & 2
    _assert_pass_ordered(hp, prep, rn, dn, rn * dn, 'flagged')
    hp.set_option('fp32_chain', True)
    hp.set_option('sample_order_natural', True)
    co32, fi32 = hp.render(bref, bque, CFG)
    _assert_same(co, co32, 'flagged coarse')
    _assert_same(fi, fi32, 'flagged fine')
