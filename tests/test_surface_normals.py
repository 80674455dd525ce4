"""Normals for the surface cloud of the real-robot route: the rows of the SDF gradient volume (tests/test_volume_gradient.py) at the
cloud's voxels, gathered on the device (SurfaceExtractor(gradient=...), gnr_surface_gradient_fwd), unit normals in float64 on the host
(surface_from_extraction), `property double nx/ny/nz` in write_ply, and plan_real / real_session(normals=True): the gradient pass and
the gather inside the session's captured graph, bitwise equal to the eager route."""
import os

import numpy as np
import pytest
import torch

from graspnerf_amd import planner
from graspnerf_amd.grasp_post import surface_from_extraction, unit_normals, write_ply
from graspnerf_amd.synth import ring_cameras
from test_planner_session import CFG, _state_dict
from test_planner_session_real import V, HW, TOP_K, R, _frames, same

PLY_TODAY = ('ply\nformat ascii 1.0\ncomment graspnerf_amd surface cloud\nelement vertex 2\nproperty double x\nproperty double y\n'
             'property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n'
             '0.0 0.0075 0.015 0 0 255\n0.2925 0.1 0.3333333333333333 64 128 255\n')


def test_write_ply_with_and_without_normals(tmp_path):
    pts = np.array([[0.0, 0.0075, 0.015], [0.2925, 0.1, 1.0 / 3.0]])
    col = [[0, 0, 1], [0.25, 0.5, 1.0]]
    path = os.path.join(str(tmp_path), 'surface.ply')
    write_ply(path, pts, col)
    assert open(path, 'rb').read() == PLY_TODAY.encode()                       # without normals: byte for byte the format before them
    nrm = unit_normals(np.array([[1.0, 2.0, -2.0], [0.1, -0.7, 1e-3]]))
    write_ply(path, pts, col, normals=nrm)
    lines = open(path).read().splitlines()
    end = lines.index('end_header')
    assert lines[:end] == ['ply', 'format ascii 1.0', 'comment graspnerf_amd surface cloud', 'element vertex 2', 'property double x',
                           'property double y', 'property double z', 'property double nx', 'property double ny', 'property double nz',
                           'property uchar red', 'property uchar green', 'property uchar blue'] and len(lines) == end + 3
    rows = [l.split() for l in lines[end + 1:]]
    assert np.array_equal(np.array([[float(x) for x in r[:3]] for r in rows]), pts)       # repr round-trips float64
    assert np.array_equal(np.array([[float(x) for x in r[3:6]] for r in rows]), nrm)
    assert [[int(x) for x in r[6:]] for r in rows] == [[0, 0, 255], [64, 128, 255]]
    with pytest.raises(ValueError):
        write_ply(path, pts, col, normals=nrm[:1])


def test_surface_from_extraction_adds_unit_normals():
    rng = np.random.default_rng(5)
    M, n = 12, 9
    g = rng.standard_normal((1, M, 3)).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 3, (1, M, 1)).astype(np.float32)
    g[0, 4] = 0.0
    index = rng.integers(0, 40, (1, M, 3)).astype(np.int32)
    res = {'count': torch.tensor([n], dtype=torch.int32), 'index': torch.from_numpy(index),
           'points': torch.from_numpy(index.astype(np.float64) * (0.3 / 40)), 'colors': torch.zeros(1, M, 3), 'gradient': torch.from_numpy(g),
           'scale': 0.3 / 40, 'value_map': False}
    out = surface_from_extraction(res, 0)
    assert out['gradient'].dtype == np.float32 and np.array_equal(out['gradient'], g[0, :n])
    nrm = out['normals']
    assert nrm.dtype == np.float64 and nrm.shape == (n, 3)
    length = np.linalg.norm(nrm, axis=1)
    keep = np.arange(n) != 4
    assert np.abs(length[keep] - 1.0).max() <= 1e-12
    assert not nrm[4].any()                                                    # a zero gradient row gives a zero normal
    assert np.array_equal(nrm[keep], g[0, :n][keep].astype(np.float64) / np.linalg.norm(g[0, :n][keep].astype(np.float64), axis=1, keepdims=True))
    plain = surface_from_extraction({k: v for k, v in res.items() if k != 'gradient'}, 0)
    assert sorted(plain) == ['colors', 'index', 'points']


def test_mirror_accepts_the_switch_and_the_session_needs_a_cloud():
    from graspnerf_amd.renderer import GraspNeRF
    from graspnerf_amd.planner_session import PlannerSession
    net = GraspNeRF(dict(CFG, volume_gradient=True))
    assert net.nr_net.cfg['volume_gradient'] is True
    assert GraspNeRF(dict(CFG)).nr_net.cfg.get('volume_gradient', False) is False
    with pytest.raises(ValueError, match='surface'):
        PlannerSession(net, V, HW, HW[::-1], surface_normals=True)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    net = planner.load_model(dict(CFG), {'network_state_dict': _state_dict(width_bias=5.0)})
    K = np.float32([[0.7 * HW[1], 0, 0.5 * HW[1]], [0, 0.7 * HW[1], 0.5 * HW[0]], [0, 0, 1]])
    cam = dict(extrinsics=list(ring_cameras(V)), intrinsic=K)
    A = _frames(1)
    vol = planner.plan_real(net, A, **cam)[2]
    rg = (float(np.percentile(vol, 40)), float(np.percentile(vol, 60)))        # (tests/test_planner_session_real.py: no zero crossing)
    return dict(net=net, cam=cam, A=A, rg=rg)


@pytest.mark.gpu
def test_plan_real_with_normals_eager_and_session(ctx):
    net, cam, A, rg = (ctx[k] for k in ('net', 'cam', 'A', 'rg'))
    kw = dict(order='score', top_k=TOP_K, surface_rg=rg)
    plain = planner.plan_real(net, A, **cam, **kw)
    off = planner.plan_real(net, A, **cam, **kw, normals=False)
    eager = planner.plan_real(net, A, **cam, **kw, normals=True)
    sess = planner.real_session(net, V, HW, HW[::-1], order='score', top_k=TOP_K, surface_rg=rg, normals=True)
    assert sess.captures == 1
    got = planner.plan_real(net, A, **cam, **kw, session=sess, normals=True)
    again = planner.plan_real(net, A, **cam, **kw, session=sess, normals=True)
    for what, res in (('normals=False', off), ('eager', eager), ('session', got), ('session, second replay', again)):
        for k in ('index', 'pos', 'quat', 'width', 'score'):
            assert same(res[0][k], plain[0][k]), (what, k)                     # the grasps do not depend on the switch
        assert same(res[2], plain[2]), what
        for k in ('index', 'points', 'colors'):
            assert same(res[3][k], plain[3][k]), (what, 'cloud', k)
    assert sorted(off[3]) == sorted(plain[3]) and 'normals' not in off[3] and 'gradient' not in off[3]
    n = len(eager[3]['index'])
    assert 0 < n < R ** 3 and eager[3]['gradient'].shape == (n, 3) and eager[3]['gradient'].dtype == np.float32
    for what, res in (('session', got), ('session, second replay', again)):
        assert same(res[3]['gradient'], eager[3]['gradient']), what
        assert same(res[3]['normals'], eager[3]['normals']), what
    nrm = eager[3]['normals']
    assert nrm.dtype == np.float64 and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-12
    # the rows are the gradient volume's at the cloud's voxels
    grad = sess._out['surface']['gradient'][0, :n].cpu().numpy()
    assert same(grad, eager[3]['gradient'])
    assert sess.captures == 1
    # a session without the argument returns what it returns today, and refuses a plan that asks for normals
    today = planner.real_session(net, V, HW, HW[::-1], order='score', top_k=TOP_K, surface_rg=rg)
    assert not today.surface_normals and sorted(today._out['surface']) == sorted(k for k in sess._out['surface'] if k != 'gradient')
    t = planner.plan_real(net, A, **cam, **kw, session=today)
    assert sorted(t[3]) == ['colors', 'count', 'index', 'points']                  # (a session's cloud also says its row count)
    with pytest.raises(ValueError, match='real_session'):
        planner.plan_real(net, A, **cam, **kw, session=today, normals=True)


@pytest.mark.gpu
def test_eval_forward_adds_the_gradient_volume_only_when_asked(ctx):
    net, cam, A = ctx['net'], ctx['cam'], ctx['A']
    nr = net.nr_net
    dev = next(net.parameters()).device
    t = lambda a: torch.as_tensor(np.array(a, np.float32), device=dev)
    imgs = (A.astype(np.float32) / 255).transpose(0, 3, 1, 2)
    ext = np.stack(cam['extrinsics'])[:, :3, :]
    ref = {'imgs': t(imgs), 'poses': t(ext), 'Ks': t(np.repeat(cam['intrinsic'][None], V, 0)),
           'depth_range': t(np.tile(np.float32([0.2, 0.8]), (V, 1))), 'bbox3d': t(planner.REAL_BBOX3D)}
    que = {'poses': ref['poses'][3:4], 'Ks': ref['Ks'][3:4], 'coords': torch.zeros(1, 1, 2, device=dev), 'depth_range': ref['depth_range'][3:4]}
    data = {'step': 0, 'eval': True, 'full_vol': True, 'ref_imgs_info': ref, 'que_imgs_info': que, 'src_imgs_info': dict(ref)}
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            off = nr(data)
            nr.cfg['volume_gradient'] = True
            try:
                on = nr(data)
                train = nr({k: v for k, v in data.items() if k != 'eval'})
            finally:
                nr.cfg['volume_gradient'] = False
    finally:
        torch.backends.cudnn.deterministic = was
    assert 'volume_gradient' not in off and 'volume_gradient' not in train and 'volume_gradient_error' not in train
    assert on['volume_gradient'].shape == (1, R, R, R, 3) and on['volume_gradient_error'].shape == (1,)
    assert same(on['volume'].cpu().numpy(), off['volume'].cpu().numpy())      # `volume` never comes from the gradient pass
    g = on['volume_gradient'].cpu().numpy().astype(np.float64)
    want = np.mean((np.linalg.norm(g, axis=-1) - 1.0) ** 2)
    assert abs(float(on['volume_gradient_error'][0]) - want) <= 2e-5 + 1e-3 * want
