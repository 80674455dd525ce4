"""The real-robot route through a PlannerSession (graspnerf_amd/planner.py: plan_real, real_session): the ranked grasps and the
surface cloud come out of the session's captured graph, bitwise equal to the eager plan_real on the same frames.  4 views (run_real
renders its query from view 3), 96x128 uint8 frames at the network's size, 40^3.

Both routes run the 2D backbones with MIOpen's deterministic solvers (PlannerSession(deterministic=True) records them, plan_real
switches them on for its forward), so the volumes agree bit for bit and with them everything downstream: comparisons, integer
arithmetic and one float64 product per coordinate (csrc/gnr_post.hip)."""
import numpy as np
import pytest
import torch

from graspnerf_amd import planner
from graspnerf_amd.synth import ring_cameras
from test_planner_session import CFG, PARAMS, _state_dict

pytestmark = pytest.mark.gpu

V, HW, MAX_GRASPS, TOP_K, SEED = 4, (96, 128), 2048, 10, 3
R = 40


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def _frames(seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (V, HW[0] // 8, HW[1] // 8, 3)).repeat(8, 1).repeat(8, 2)
    return np.clip(base + rng.integers(-40, 41, (V, *HW, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope='module')
def ctx():
    net = planner.load_model(dict(CFG), {'network_state_dict': _state_dict(width_bias=5.0)})       # widths inside process()'s 0..12
    K = np.float32([[0.7 * HW[1], 0, 0.5 * HW[1]], [0, 0.7 * HW[1], 0.5 * HW[0]], [0, 0, 1]])
    cam = dict(extrinsics=list(ring_cameras(V)), intrinsic=K)
    A, B = _frames(1), _frames(2)
    # the synthetic checkpoint's volume has no zero crossing (tests/test_planner_session.py:40): the cloud's range is taken from
    # the eager volume itself, so that some voxels and not all of them are in it
    vol = planner.plan_real(net, A, **cam)[2]
    rg = (float(np.percentile(vol, 40)), float(np.percentile(vol, 60)))
    print(f'eager volume: min {vol.min():.4f} max {vol.max():.4f}, surface range {rg}')
    return dict(net=net, cam=cam, A=A, B=B, rg=rg, iso=float(np.float32(np.median(vol))))


def _equal_plans(got, want, what):
    g, scores, vol, cloud, dt = got
    e, escores, evol, ecloud, _ = want
    assert 0 < dt < 60
    assert same(vol, evol), f'{what}: the volumes differ by {np.abs(vol - evol).max():.3e}'
    for k in ('index', 'pos', 'quat', 'width', 'score'):
        assert same(g[k], e[k]), (what, k)
    assert same(scores, escores)
    for k in ('index', 'points', 'colors'):
        assert same(cloud[k], ecloud[k]), (what, 'cloud', k)
    return len(scores), len(cloud['index'])


def test_session_equals_eager_plan_real(ctx):
    net, cam, A, B, rg = (ctx[k] for k in ('net', 'cam', 'A', 'B', 'rg'))
    ranked = planner.real_session(net, V, HW, HW[::-1], order='score', top_k=TOP_K, surface_rg=rg, max_grasps=MAX_GRASPS)
    assert ranked.captures == 1
    eA = planner.plan_real(net, A, **cam, order='score', top_k=TOP_K, surface_rg=rg)
    eB = planner.plan_real(net, B, **cam, order='score', top_k=TOP_K, surface_rg=rg)
    n_all = len(planner.plan_real(net, A, **cam, order='score', surface_rg=rg)[1])
    print(f'eager plan_real: {n_all} survivors, top scores {eA[1][:3]}, cloud {len(eA[3]["index"])} of {R ** 3}')
    assert n_all > TOP_K, 'fewer survivors than top_k: the prefix shows nothing'
    sA = planner.plan_real(net, A, **cam, order='score', top_k=TOP_K, surface_rg=rg, session=ranked)
    n, c = _equal_plans(sA, eA, 'ranked A')
    assert n == TOP_K and 0 < c < R ** 3 and int(ranked.selection['count'][0]) == n_all
    assert np.all(np.diff(sA[1].astype(np.float64)) <= 0)                                 # best first
    assert np.array_equal(ranked.images.cpu().numpy().view(np.uint32),
                          (A.astype(np.float32) / 255).transpose(0, 3, 1, 2).copy().view(np.uint32))
    # the float64 points the graph wrote on the device are the ones the host recomputed
    dev_pts = ranked._out['surface']['points'][0, :c].cpu().numpy()
    assert same(dev_pts, sA[3]['points'])
    _equal_plans(planner.plan_real(net, B, **cam, order='score', top_k=TOP_K, surface_rg=rg, session=ranked), eB, 'ranked B')
    _equal_plans(planner.plan_real(net, A, **cam, order='score', top_k=TOP_K, surface_rg=rg, session=ranked), eA, 'ranked A, second replay')
    assert ranked.captures == 1
    with pytest.raises(ValueError, match='real_session'):
        planner.plan_real(net, A, **cam, order='score', top_k=TOP_K + 1, surface_rg=rg, session=ranked)
    with pytest.raises(ValueError, match='at least 4 views'):
        planner.plan_real(net, A[:3], cam['extrinsics'][:3], cam['intrinsic'])


def test_permuted_session_and_value_map_colours(ctx):
    """order='permuted' (run_real's own list): every survivor, seeded permutation.  Then a session whose cloud carries the value map:
    the sized copy of the colours against the eager extraction on the same volume."""
    from graspnerf_amd.grasp_post import GRASP_UTILS_PROCESS, SurfaceExtractor, surface_from_extraction
    from graspnerf_amd.planner_session import PlannerSession
    net, cam, A, rg = (ctx[k] for k in ('net', 'cam', 'A', 'rg'))
    e = planner.plan_real(net, A, **cam, seed=SEED, surface_rg=rg)
    s = planner.real_session(net, V, HW, HW[::-1], surface_rg=rg)
    n, c = _equal_plans(planner.plan_real(net, A, **cam, seed=SEED, surface_rg=rg, session=s), e, 'permuted')
    assert n > 1 and 0 < c < R ** 3
    ranked = planner.plan_real(net, A, **cam, order='score', surface_rg=rg)
    assert sorted(e[1].tolist()) == sorted(ranked[1].tolist()) and not np.array_equal(e[1], ranked[1])
    col = PlannerSession(net, V, HW, HW[::-1], voxel_size=planner.REAL_VOXEL_SIZE, surface=dict(rg=rg, color=None, bound=(-2, 2)),
                         **GRASP_UTILS_PROCESS)
    g, _ = col.plan(A, np.stack(cam['extrinsics']), np.repeat(cam['intrinsic'][None], V, 0), planner.REAL_DEPTH_RANGE,
                    planner.REAL_BBOX3D, return_volumes=True)
    assert same(g['volumes'][0].reshape(R, R, R), e[2])
    want = surface_from_extraction(SurfaceExtractor()(torch.from_numpy(e[2]).cuda(), rg=rg, color=None, bound=(-2, 2)), 0)
    assert col.cloud['count'] == c and len(np.unique(want['colors'])) > 100
    for k in ('index', 'points', 'colors'):
        assert same(col.cloud[k], want[k]), k


def test_every_product_in_one_graph(ctx):
    """Cloud with normals, mesh and depth images in ONE session: the count words of the cloud (1) and of the mesh (2) follow the
    selection in that order, and the sized copies follow in the same order.  Every output of the first and third plan is bitwise the
    eager plan_real's with the same three switches; the plan between them is another scene's."""
    net, cam, A, B, rg, iso = (ctx[k] for k in ('net', 'cam', 'A', 'B', 'rg', 'iso'))
    kw = dict(order='score', top_k=TOP_K, surface_rg=rg, normals=True, mesh=dict(iso=iso), volume_depth=dict(iso=iso))
    sess = planner.real_session(net, V, HW, HW[::-1], max_grasps=MAX_GRASPS, **kw)
    assert sess.captures == 1 and sess._d_out.numel() == 1 + 9 * MAX_GRASPS + 1 + 2
    eA, eB = planner.plan_real(net, A, **cam, **kw), planner.plan_real(net, B, **cam, **kw)
    m, img = eA[3]['mesh'], eA[3]['volume_depth']
    assert len(m['vertices']) > 100 and len(m['faces']) > 100 and (img > 0).sum() > 100, 'the level set is too small to show anything'
    plans = [planner.plan_real(net, f, **cam, **kw, session=sess) for f in (A, B, A)]
    assert sess.captures == 1
    for what, got, want in (('A', plans[0], eA), ('B', plans[1], eB), ('A, second replay', plans[2], eA)):
        _equal_plans(got, want, what)
        assert sorted(got[3]) == sorted([*want[3], 'count']), what                        # (a session's cloud also says its row count)
        for k in ('gradient', 'normals', 'volume_depth', 'volume_depth_normals'):
            assert same(got[3][k], want[3][k]), (what, k)
        assert sorted(got[3]['mesh']) == sorted(want[3]['mesh']) == ['faces', 'gradient', 'normals', 'vertices'], what
        for k in want[3]['mesh']:
            assert same(got[3]['mesh'][k], want[3]['mesh'][k]), (what, 'mesh', k)
    assert not same(eA[2], eB[2]) and not same(eA[3]['volume_depth'], eB[3]['volume_depth'])


def test_all_six_switches_in_one_graph(ctx):
    """Every product of the table at once -- clearance, closure, cloud with normals, mesh, depth images, each of the last three coloured
    from the views -- in ONE session against the eager plan_real with the same keywords: the first and third plan are bitwise the eager
    plan of A, the one between them that of B.  No count word but the cloud's and the mesh's two; the products in the table's order."""
    net, cam, A, B, rg, iso = (ctx[k] for k in ('net', 'cam', 'A', 'B', 'rg', 'iso'))
    kw = dict(order='score', top_k=TOP_K, surface_rg=rg, normals=True, mesh=dict(iso=iso), volume_depth=dict(iso=iso), view_colors=True,
              clearance=dict(level=iso), closure=dict(level=iso, friction=0.5))
    sess = planner.real_session(net, V, HW, HW[::-1], max_grasps=MAX_GRASPS, **kw)
    assert sess.captures == 1 and sess._d_out.numel() == 1 + 9 * MAX_GRASPS + 1 + 2
    assert [p.out for p in sess.products] == ['hand', 'closure', 'surface', 'mesh', 'volume_depth']
    eA, eB = planner.plan_real(net, A, **cam, **kw), planner.plan_real(net, B, **cam, **kw)
    g, cloud = eA[0], eA[3]
    assert len(cloud['index']) > 100 and len(cloud['mesh']['faces']) > 100 and (cloud['volume_depth'] > 0).sum() > 100, \
        'the level set is too small to show anything'
    assert (g['finger_contact'] >= 0).any(), 'no finger touches anything: the closure columns show nothing'
    print(f'{len(cloud["index"])} cloud rows, {len(cloud["mesh"]["faces"])} faces, {(cloud["volume_depth"] > 0).sum()} pixels hit, '
          f'{(g["finger_contact"] >= 0).sum()} finger contacts; coloured: {(cloud["view_weight"] > 0).sum()} rows, '
          f'{(cloud["mesh"]["view_weight"] > 0).sum()} vertices, {(cloud["volume_color_weight"] > 0).sum()} pixels')
    hand_keys = {'clearance', 'approach_clearance', 'hand_inside', 'hand_worst', 'collision_free'}
    closure_keys = {'closed_width', 'finger_travel', 'finger_contact', 'contact_cos', 'grip_cos', 'held', 'force_closure'}
    assert set(g) == {'index', 'pos', 'quat', 'width', 'score'} | hand_keys | closure_keys
    view_keys = ['view_colors', 'view_mask', 'view_weight']
    images = ['volume_color', 'volume_color_weight', 'volume_depth', 'volume_depth_normals']
    assert sorted(cloud) == sorted(['index', 'points', 'colors', 'gradient', 'normals', 'mesh', *view_keys, *images])
    assert sorted(cloud['mesh']) == sorted(['vertices', 'faces', 'gradient', 'normals', *view_keys])
    plans = [planner.plan_real(net, f, **cam, **kw, session=sess) for f in (A, B, A)]
    assert sess.captures == 1
    for what, got, want in (('A', plans[0], eA), ('B', plans[1], eB), ('A, second replay', plans[2], eA)):
        _equal_plans(got, want, what)
        assert sorted(got[0]) == sorted(want[0]), what
        for k in want[0]:
            assert same(got[0][k], want[0][k]), (what, 'grasps', k)
        assert sorted(got[3]) == sorted([*want[3], 'count']), what                        # (a session's cloud also says its row count)
        for k in set(want[3]) - {'mesh'}:
            assert same(got[3][k], want[3][k]), (what, 'cloud', k)
        assert sorted(got[3]['mesh']) == sorted(want[3]['mesh']), what
        for k in want[3]['mesh']:
            assert same(got[3]['mesh'][k], want[3]['mesh'][k]), (what, 'mesh', k)
    assert not same(eA[2], eB[2]) and not same(eA[3]['volume_color'], eB[3]['volume_color'])


def test_session_without_the_new_arguments_is_todays_session(ctx):
    """No surface, no ranking: the packed read-back has today's size, the graph's outputs today's names, and the plan the bits of the
    original select call on the session's own volumes."""
    from graspnerf_amd.grasp_post import GraspSelector, grasps_from_selection
    from graspnerf_amd.planner_session import PlannerSession
    net, cam, A = ctx['net'], ctx['cam'], ctx['A']
    s = PlannerSession(net, V, HW, HW[::-1], max_grasps=MAX_GRASPS, **PARAMS)           # (tests/test_planner_session.py:40-44)
    assert s._d_out.numel() == 1 + 9 * MAX_GRASPS and sorted(s._out) == ['qual', 'rot', 'sel_qual', 'volume', 'width']
    assert s.surface_params is None and s.cloud is None
    args = (A, np.stack(cam['extrinsics']), np.repeat(cam['intrinsic'][None], V, 0), planner.REAL_DEPTH_RANGE, planner.REAL_BBOX3D)
    g, _ = s.plan(*args, seed=SEED, return_volumes=True)
    vol, q, r, w, qp = (torch.from_numpy(x).cuda() for x in g['volumes'])
    own = GraspSelector(max_grasps=MAX_GRASPS)(vol, q, r, w, **PARAMS)
    torch.cuda.synchronize()
    assert 1 <= int(own['count'][0]) < MAX_GRASPS and same(qp.cpu().numpy(), own['qual'].cpu().numpy())
    want = grasps_from_selection(own, 0, 0.3 / 40, SEED)
    for k in ('index', 'pos', 'quat', 'width', 'score'):
        assert same(g[k], want[k]), k
    assert s.cloud is None
