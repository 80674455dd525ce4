"""The real-robot route (reference: src/nr/utils/grasp_utils.py:40-151, draw_utils.py:355-377): grasp_utils.process with its three
thresholds, select, sim_grasp's ranking by score and the surface point cloud.  The numpy statement (tests/real_route_reference.py)
against the golden the reference's own functions wrote (tools/make_real_route_goldens.py), and the HIP kernels (csrc/gnr_post.hip:
gnr_grasp_select_v2_fwd, gnr_surface_points_fwd) against both.  Everything here is integer, comparison or fp64-ordered arithmetic
(DESIGN.md 4.7): every comparison is bitwise."""
import os

import numpy as np
import pytest

import real_route_reference as RR
from graspnerf_amd.synth import synth_head_outputs
from oracle import grasp_post_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS, R40, TOP_K = (0, 1, 2), 40, 10
SURVIVORS = {0: 27, 1: 39, 2: 35}                       # measured with the reference's functions on synth_head_outputs(seed)
SURFACE = {0: 21036, 1: 21220, 2: 23357}


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_real_route.npz')))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- CPU: the numpy statement against the reference's own results ------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
def test_statement_equals_reference_functions(seed, G):
    tsdf, qual, rot, width = synth_head_outputs(seed)
    q = RR.process(tsdf[0, 0], qual[0, 0], rot[0], width[0, 0])
    assert same(q, G[f's{seed}.qual'])
    idx, score, quat, w = RR.select(q, rot[0], width[0, 0])
    n = len(idx)
    assert n == SURVIVORS[seed] and 0 < n < R40 ** 3
    assert np.array_equal(idx, G[f's{seed}.index']) and same(score, G[f's{seed}.score']) and same(w, G[f's{seed}.width'])
    qn = quat.astype(np.float64) / np.linalg.norm(quat.astype(np.float64), axis=1, keepdims=True)     # scipy's Rotation normalises
    assert np.abs(qn - G[f's{seed}.quat']).max() < 1e-6
    # the ranking: numpy leaves the order of tied scores open, so the k + 1 largest must be pairwise distinct
    top = np.sort(score)[::-1][:TOP_K + 1]
    assert len(top) == TOP_K + 1 and len(np.unique(top)) == TOP_K + 1
    assert int(G['top_k']) == TOP_K and np.array_equal(RR.rank(score, TOP_K), G[f's{seed}.rank'])
    for color, key in (((0, 0, 1), None), (None, f's{seed}.surface_colors_value')):
        sidx, pts, col = RR.surface(tsdf[0, 0], tuple(G['surface_rg']), color=color)
        assert len(sidx) == SURFACE[seed] and 0 < len(sidx) < R40 ** 3
        assert np.array_equal(sidx, G[f's{seed}.surface_index']) and same(pts, G[f's{seed}.surface_points'])
        if key is None:
            assert np.array_equal(col.astype(np.float64), np.repeat(G[f's{seed}.surface_color_fixed'][None], len(sidx), 0))
        else:
            assert same(col, G[key])


@pytest.mark.parametrize('seed', SEEDS)
def test_statement_with_two_thresholds_is_the_planner_oracle(seed):
    """outside == high: grasp_utils.process is main.py's process (oracle/grasp_post_oracle.py)."""
    tsdf, qual, rot, width = synth_head_outputs(seed)
    for hi, lo in ((0.0, -0.85), (0.5, 1e-3)):
        a = RR.process(tsdf[0, 0], qual[0, 0], rot[0], width[0, 0], min_width=1.33, max_width=9.33, outside=hi, high=hi, low=lo)
        b = P.process(tsdf[0, 0], qual[0, 0], rot[0], width[0, 0], thres_high=hi, thres_low=lo)
        assert same(a, b) and (a != 0).any()
        for x, y in zip(RR.select(a, rot[0], width[0, 0]), P.select(b, rot[0], width[0, 0])):
            assert same(x, y)


def test_rank_orders_ties_by_row_and_negative_scores():
    s = np.float32([0.5, -1.0, 2.0, 0.5, -0.25, 2.0, 0.0])
    assert RR.rank(s).tolist() == [2, 5, 0, 3, 6, 4, 1] and RR.rank(s, 3).tolist() == [2, 5, 0]


def test_write_ply_round_trip(tmp_path):
    from graspnerf_amd.grasp_post import write_ply
    pts = np.array([[0.0, 0.0075, 0.015], [0.2925, 0.1, 1.0 / 3.0]])
    path = os.path.join(str(tmp_path), 'surface.ply')
    write_ply(path, pts, [[0, 0, 1], [0.25, 0.5, 1.0]])
    lines = open(path).read().splitlines()
    end = lines.index('end_header')
    assert lines[0] == 'ply' and lines[1] == 'format ascii 1.0' and 'element vertex 2' in lines[:end] and len(lines) == end + 3
    rows = [l.split() for l in lines[end + 1:]]
    assert np.array_equal(np.array([[float(x) for x in r[:3]] for r in rows]), pts)          # repr round-trips float64
    assert [[int(x) for x in r[3:]] for r in rows] == [[0, 0, 255], [64, 128, 255]]
    with pytest.raises(ValueError):
        write_ply(path, pts, [[0, 0, 1]])


def test_refusals_before_the_device():
    """Score order at R = 65 is refused with a text that names the limit; the v2 call's other refusals.  Fake pointers: every call is
    one that validation refuses.  Runs without a GPU."""
    import ctypes as C
    from graspnerf_amd import _lib
    L = _lib.lib()
    one, big = C.c_void_p(16), C.c_size_t(1 << 40)
    p = _lib.GnrSelectParamsV2(order=_lib.GNR_SELECT_ORDER_SCORE)
    p.select.gauss_radius, p.select.dilate_iterations, p.select.max_filter_size = 4, 2, 4
    call = lambda R, p=p, tsdf=one, ws=big: L.gnr_grasp_select_v2_fwd(tsdf, one, one, one, 1, R, C.byref(p), one, one, one, one, one, one, 8,
                                                                      one, ws, None)
    assert call(65) == _lib.GNR_ERR_SHAPE
    text = L.gnr_last_error().decode()
    assert 'R <= 64' in text and 'GNR_SELECT_ORDER_SCORE' in text, text
    assert call(64, tsdf=None) == _lib.GNR_ERR_ARG and L.gnr_last_error() == b'gnr_grasp_select_v2_fwd: null pointer'
    assert call(64, ws=C.c_size_t(L.gnr_grasp_select_v2_workspace_bytes(1, 64, 1) - 1)) == _lib.GNR_ERR_WORKSPACE
    assert L.gnr_grasp_select_v2_workspace_bytes(1, 64, 1) > L.gnr_grasp_select_v2_workspace_bytes(1, 64, 0) == L.gnr_grasp_select_workspace_bytes(1, 64)
    bad = _lib.GnrSelectParamsV2(order=2)
    bad.select.gauss_radius, bad.select.dilate_iterations, bad.select.max_filter_size = 4, 2, 4
    assert call(8, p=bad) == _lib.GNR_ERR_ARG and b'order' in L.gnr_last_error()
    neg = _lib.GnrSelectParamsV2(top_k=-1)
    neg.select.gauss_radius, neg.select.dilate_iterations, neg.select.max_filter_size = 4, 2, 4
    assert call(8, p=neg) == _lib.GNR_ERR_ARG and b'top_k' in L.gnr_last_error()
    sp = _lib.GnrSurfaceParams(lo=-0.2, hi=0.2, scale=1.0)
    surf = lambda R=8, vol=one, p=sp, ws=big: L.gnr_surface_points_fwd(vol, 1, R, C.byref(p), one, one, one, one, 8, one, ws, None)
    assert surf(vol=None) == _lib.GNR_ERR_ARG and L.gnr_last_error() == b'gnr_surface_points_fwd: null pointer'
    assert surf(R=257) == _lib.GNR_ERR_SHAPE and b'R <= 256' in L.gnr_last_error()
    assert surf(p=_lib.GnrSurfaceParams(color_mode=2)) == _lib.GNR_ERR_ARG
    assert surf(ws=C.c_size_t(L.gnr_surface_points_workspace_bytes(1, 8) - 1)) == _lib.GNR_ERR_WORKSPACE


# ---- GPU: bit-exact against the goldens ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scenes():
    import torch
    vols = [synth_head_outputs(s) for s in SEEDS]
    return [torch.from_numpy(np.concatenate([v[i] for v in vols])).cuda() for i in range(4)]


@pytest.mark.gpu
def test_hip_real_route_is_bit_exact_with_the_reference(G, scenes):
    """Three scenes in one batch: the processed volume, the selection in index order and in score order, the top-10 list; the
    surface cloud's index, points and colours in both colour modes."""
    import torch
    from graspnerf_amd.grasp_post import GRASP_UTILS_PROCESS, GraspSelector, SurfaceExtractor, grasps_from_selection, surface_from_extraction
    sel = GraspSelector()
    by_index = sel(*scenes, **GRASP_UTILS_PROCESS)
    by_score = sel(*scenes, **GRASP_UTILS_PROCESS, order='score')
    top = sel(*scenes, **GRASP_UTILS_PROCESS, order='score', top_k=TOP_K)
    torch.cuda.synchronize()
    for s in SEEDS:
        g = {k: G[f's{s}.{k}'] for k in ('qual', 'index', 'score', 'quat', 'width', 'rank')}
        full = RR.rank(g['score'])
        assert np.array_equal(full[:TOP_K], g['rank'])                               # (distinct: pinned by the CPU test)
        for out, rows in ((by_index, np.arange(len(g['score']))), (by_score, full), (top, g['rank'].astype(np.int64))):
            assert same(out['qual'][s].cpu().numpy(), g['qual']), f'scene {s} processed quality'
            assert int(out['count'][s]) == len(g['score']) == SURVIVORS[s]
            got = grasps_from_selection(out, s, voxel_size=1.0)
            assert len(got['index']) == len(rows)
            assert np.array_equal(got['index'], g['index'][rows].astype(np.int64)) and same(got['score'], g['score'][rows])
            assert same(got['width'], g['width'][rows]) and np.abs(got['quat'] - g['quat'][rows]).max() < 1e-6
    ex = SurfaceExtractor()
    rg = tuple(G['surface_rg'])
    fixed, value = ex(scenes[0], rg=rg), ex(scenes[0], rg=rg, color=None)
    torch.cuda.synchronize()
    for s in SEEDS:
        for res, want in ((fixed, np.repeat(G[f's{s}.surface_color_fixed'][None], SURFACE[s], 0)),
                          (value, G[f's{s}.surface_colors_value'].astype(np.float64))):
            c = surface_from_extraction(res, s)
            assert int(res['count'][s]) == SURFACE[s]
            assert np.array_equal(c['index'], G[f's{s}.surface_index'].astype(np.int64))
            assert same(c['points'], G[f's{s}.surface_points']) and same(c['colors'], want)


# ---- GPU: the smallest shapes that can still go wrong, against the numpy statement -----------------------------------------------
def _volumes(rng, B, R):
    tsdf = (rng.random((B, 1, R, R, R)) * 2.4 - 1.2).astype(np.float32)              # some beyond -1: outside the `inside` interval
    qual = rng.random((B, 1, R, R, R)).astype(np.float32) ** 0.05                    # mostly > 0.9 after smoothing
    rot = rng.standard_normal((B, 4, R, R, R)).astype(np.float32)
    width = (rng.random((B, 1, R, R, R)) * 14 - 1).astype(np.float32)                # some outside 0..12
    return tsdf, qual, rot, width


@pytest.mark.gpu
@pytest.mark.parametrize('R', [8, 11])
def test_hip_three_thresholds_small_volumes(R):
    """R = 8: every voxel is within the Gaussian's, the dilation's and the NMS's borders.  R = 11: 1 331 voxels, one full 1 024-voxel
    chunk of the compaction plus a partial one.  Two scenes, both orders, max_n below the count: the stored prefix and the true count."""
    import torch
    from graspnerf_amd.grasp_post import GRASP_UTILS_PROCESS, GraspSelector
    tsdf, qual, rot, width = _volumes(np.random.default_rng(20 + R), 2, R)
    M = 8
    sel = GraspSelector(max_grasps=M)
    outs = {o: sel(tsdf, qual, rot, width, **GRASP_UTILS_PROCESS, max_filter_size=3, order=o) for o in ('index', 'score')}
    torch.cuda.synchronize()
    for b in range(2):
        q = RR.process(tsdf[b, 0], qual[b, 0], rot[b], width[b, 0])
        assert 0 < (q != 0).sum() < q.size
        idx, score, quat, w = RR.select(q, rot[b], width[b, 0], size=3)
        assert len(idx) > M
        for o, rows in (('index', np.arange(M)), ('score', RR.rank(score, M))):
            out = outs[o]
            assert same(out['qual'][b].cpu().numpy(), q)
            assert int(out['count'][b]) == len(idx)
            assert np.array_equal(out['index'][b].cpu().numpy(), idx[rows]), o
            assert same(out['score'][b].cpu().numpy(), score[rows]) and same(out['quat'][b].cpu().numpy(), quat[rows])
            assert same(out['width'][b].cpu().numpy(), w[rows])


def _open_selector_kw(threshold):
    """Nothing masked, no smoothing to speak of, a 1-voxel maximum filter: every voxel at or above the threshold survives."""
    return dict(gaussian_filter_sigma=0.1, tsdf_thres_outside=-1e6, tsdf_thres_high=-1e6, tsdf_thres_low=-2e6, min_width=-1e6,
                max_width=1e6, threshold=threshold, max_filter_size=1)


@pytest.mark.gpu
def test_hip_ranking_is_over_all_survivors():
    """R = 11, most voxels survive.  Scene 0: distinct scores, some negative, the best at the LAST voxel, max_n = 16: a ranking over
    the first max_n survivors in index order cannot find it.  Scene 1: a constant plateau -- order by ascending index.  Scene 2: nothing
    survives."""
    import torch
    from graspnerf_amd.grasp_post import GraspSelector, grasps_from_selection
    R, M = 11, 16
    n = R ** 3
    rng = np.random.default_rng(5)
    vals = (rng.permutation(n).astype(np.float32) - 300.0) / 64.0                    # distinct, exact in float32, 300 of them negative
    vals[np.argmax(vals)], vals[-1] = vals[-1], vals.max()
    qual = np.stack([vals.reshape(R, R, R), np.full((R, R, R), 0.75, np.float32), np.full((R, R, R), -9.0, np.float32)])[:, None]
    tsdf, rot, width = np.zeros((3, 1, R, R, R), np.float32), rng.standard_normal((3, 4, R, R, R)).astype(np.float32), \
        rng.random((3, 1, R, R, R)).astype(np.float32)
    kw = _open_selector_kw(threshold=-4.0)
    sel = GraspSelector(max_grasps=M)
    out = sel(tsdf, qual, rot, width, **kw, order='score')
    top3 = sel(tsdf, qual, rot, width, **kw, order='score', top_k=3)
    first3 = sel(tsdf, qual, rot, width, **kw, top_k=3)
    torch.cuda.synchronize()
    want_counts = []
    for b in range(3):
        q = RR.process(tsdf[b, 0], qual[b, 0], rot[b], width[b, 0], sigma=0.1, min_width=-1e6, max_width=1e6, outside=-1e6, high=-1e6, low=-2e6)
        assert same(q, qual[b, 0])                                                   # sigma 0.1: radius 0, the volume itself
        idx, score, quat, w = RR.select(q, rot[b], width[b, 0], threshold=-4.0, size=1)
        want_counts.append(len(idx))
        rows = RR.rank(score, M)
        k = min(M, len(idx))
        for o, r in ((out, rows), (top3, rows[:3]), (first3, np.arange(min(3, len(idx))))):
            assert int(o['count'][b]) == len(idx)
            for key, ref in (('index', idx), ('score', score), ('quat', quat), ('width', w)):
                assert same(o[key][b, :len(r)].cpu().numpy(), ref[r].astype(o[key].cpu().numpy().dtype)), (b, key)
        if b == 0:
            assert out['index'][0, 0].tolist() == [R - 1] * 3 and float(out['score'][0, 0]) == vals.max() and k == M
            assert (score < 0).sum() > 100 and len(np.unique(score)) == len(score)
        if b == 1:
            assert np.array_equal(out['index'][1].cpu().numpy(), np.argwhere(np.ones((R, R, R)))[:M])
    assert want_counts[0] > n // 2 and want_counts[1] == n and want_counts[2] == 0
    # a top-k result is a prefix by request: no truncation error; without top_k a truncated list is still reported
    assert len(grasps_from_selection(top3, 0)['index']) == 3 and len(grasps_from_selection(top3, 2)['index']) == 0
    from graspnerf_amd import _lib
    with pytest.raises(_lib.GnrError):
        grasps_from_selection(out, 0)


@pytest.mark.gpu
def test_hip_v2_with_todays_arguments_is_todays_call(scenes):
    """gnr_grasp_select_v2_fwd with outside == high, index order and top_k = 0 against gnr_grasp_select_fwd: every output, every bit
    (entries beyond the count are undefined in both: the buffers start from the same fill)."""
    import ctypes as C
    import torch
    from graspnerf_amd import _lib
    from graspnerf_amd.grasp_post import gaussian_weights
    L = _lib.lib()
    B, R, M = 3, R40, 64
    p = _lib.GnrSelectParams()
    p.gauss_radius, w = gaussian_weights(1.0)
    for k, v in enumerate(w):
        p.gauss_w[k] = float(v)
    p.tsdf_thres_high, p.tsdf_thres_low, p.min_width, p.max_width, p.threshold = 0.0, -0.85, 1.33, 9.33, 0.9
    p.dilate_iterations, p.max_filter_size = 2, 4
    p2 = _lib.GnrSelectParamsV2(select=p, tsdf_thres_outside=0.0, order=_lib.GNR_SELECT_ORDER_INDEX, top_k=0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(L.gnr_grasp_select_v2_workspace_bytes(B, R, 0), dtype=torch.uint8, device='cuda')

    def run(fn, par):
        o = [torch.full(s, 7, dtype=d, device='cuda') for s, d in (((B, R, R, R), torch.float32), ((B,), torch.int32), ((B, M, 3), torch.int32),
                                                                 ((B, M), torch.float32), ((B, M, 4), torch.float32), ((B, M), torch.float32))]
        _lib.check(fn(*[t.data_ptr() for t in scenes], B, R, C.byref(par), *[t.data_ptr() for t in o], M, ws.data_ptr(), ws.numel(), stream), 'select')
        torch.cuda.synchronize()
        return o
    old, new = run(L.gnr_grasp_select_fwd, p), run(L.gnr_grasp_select_v2_fwd, p2)
    assert all(0 < int(c) <= M for c in old[1])
    for a, b in zip(old, new):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_hip_surface_ragged_batch():
    """R = 11 (a full chunk and a partial one), B = 3: an empty scene, an all-surface scene and a mixed one, both colour modes; then
    max_points below the count: the stored prefix is correct and the count is true, and surface_from_extraction reports it."""
    import torch
    from graspnerf_amd import _lib
    from graspnerf_amd.grasp_post import SurfaceExtractor, surface_from_extraction
    R = 11
    rng = np.random.default_rng(9)
    vol = np.stack([np.full((R, R, R), 0.5, np.float32), np.zeros((R, R, R), np.float32),
                    (rng.random((R, R, R)) * 2 - 1).astype(np.float32)])
    vol[1].reshape(-1)[::2] = -0.125                                                  # both sides of the value map's middle
    vol[2, 0, 0, 0], vol[2, 0, 0, 1] = -0.2, 0.2                                      # the bounds themselves are outside
    ex = SurfaceExtractor()
    for color, bound, scale in (((0.25, 0.5, 1), (-1, 1), 0.3 / 40), (None, (-1, 1), 0.3 / 40), (None, (-0.5, 0.25), 0.013)):
        full = ex(vol, rg=(-0.2, 0.2), bound=bound, color=color, scale=scale)
        cut = ex(vol, rg=(-0.2, 0.2), bound=bound, color=color, scale=scale, max_points=100)
        torch.cuda.synchronize()
        counts = []
        for b in range(3):
            idx, pts, col = RR.surface(vol[b], (-0.2, 0.2), bound=bound, color=color, scale=scale)
            counts.append(len(idx))
            c = surface_from_extraction(full, b)
            assert int(full['count'][b]) == int(cut['count'][b]) == len(idx)
            assert np.array_equal(c['index'], idx) and same(c['points'], pts) and same(c['colors'], col.astype(np.float64))
            k = min(100, len(idx))
            assert np.array_equal(cut['index'][b, :k].cpu().numpy(), idx[:k]) and same(cut['points'][b, :k].cpu().numpy(), pts[:k])
            assert same(cut['colors'][b, :k].cpu().numpy(), col[:k])
            if len(idx) > 100:
                with pytest.raises(_lib.GnrError, match='max_points'):
                    surface_from_extraction(cut, b)
        assert counts[0] == 0 and counts[1] == R ** 3 and 100 < counts[2] < R ** 3 - 2


@pytest.mark.gpu
def test_hip_surface_more_chunks_than_one_scan_pass():
    """R = 104: 1 099 chunks of 1 024 voxels per scene, so the scan of the chunk counts takes a second pass of its 1 024 threads with a
    carried base.  Two scenes (the second scene's chunk offsets start from zero again), a narrow range, max_points below R^3."""
    import torch
    from graspnerf_amd.grasp_post import SurfaceExtractor
    R, M = 104, 120000
    vol = (np.random.default_rng(3).random((2, R, R, R)) * 2 - 1).astype(np.float32)
    res = SurfaceExtractor()(vol, rg=(-0.05, 0.05), color=None, max_points=M)
    torch.cuda.synchronize()
    for b in range(2):
        idx, pts, col = RR.surface(vol[b], (-0.05, 0.05), color=None)
        n = int(res['count'][b])
        assert n == len(idx) and R ** 3 // 40 < n < M
        assert np.array_equal(res['index'][b, :n].cpu().numpy(), idx) and same(res['points'][b, :n].cpu().numpy(), pts)
        assert same(res['colors'][b, :n].cpu().numpy(), col)
        assert idx[-1, 0] == R - 1                                                    # rows from the chunks of the second pass
