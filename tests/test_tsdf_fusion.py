"""Depth route: TSDF fusion of posed depth images on the device (csrc/gnr_tsdf.hip, graspnerf_amd/tsdf.py) against the float64
statement of tests/tsdf_reference.py -- bit for bit: the statement and the kernel take the same single IEEE operations in the same
order, and the test scenes keep every decision of the arithmetic (in front of the camera, inside the image, which pixel, depth
truncation, the truncation band) far from its flip.  An analytic column guards against the statement and the kernel sharing one
misreading.  Then the callers: planner.plan_depth (the VGN baseline) and Trainer(sdf_gt_from_depth=True)."""
import ctypes as C

import numpy as np
import pytest

import tsdf_reference as T
from graspnerf_amd import _lib
from graspnerf_amd.synth import CONFIGS, synth_state_dict

ARG, SHAPE = -1, -2
P = 4096                                            # any non-null address: validation happens first
NAMES = ('tiny', 'small', 'eight')
KEYS = ('tsdf', 'weight', 'grid', 'sdf_label')


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    diff = _bits(got) != _bits(want)
    print(f'{what}: {int(diff.sum())} of {diff.size} values differ' +
          (f', worst |d| = {np.abs(got.astype(np.float64) - want)[diff].max():.3e}' if diff.any() else ''))
    assert not diff.any(), what


# ---- without a GPU: the statement itself, the scenes, the refusals ---------------------------------------------------------------------
def test_statement_matches_the_analytic_column():
    """A camera at z = 0.6 looking straight down at a constant depth image of 0.53: the surface is the plane z = 0.07, and along the
    voxel column (8, 8) the statement must give t = min(1, (z_c - 0.07) * m / trunc) with m the ray-length multiplier of the pixel the
    voxel falls on, written here from the geometry alone; the two lowest voxels lie more than the truncation behind the surface."""
    R, voxel = 16, 0.3 / 16
    pose = np.asarray([[[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0.6]]], np.float32)
    K = np.asarray(CONFIGS['cfg1']['K'], np.float32)
    depth = np.full((1, 96, 128), 0.53, np.float32)
    z0 = np.zeros((R, R, R), np.float32)
    tv, wv, _ = T.integrate(z0, z0, depth, pose, K[None], np.asarray(T.ORIGIN, np.float32), voxel, 4 * voxel)
    x = np.float64(np.float32(-0.15)) + 8.5 * voxel
    zc = np.float64(np.float32(-0.05)) + (np.arange(R) + 0.5) * voxel
    cam_z = np.float64(np.float32(0.6)) - zc
    u, v = np.floor(x * 100.0 / cam_z + 63.5 + 0.5), np.floor(-x * 100.0 / cam_z + 47.5 + 0.5)
    m = np.sqrt(((u - 63.5) / 100.0) ** 2 + ((v - 47.5) / 100.0) ** 2 + 1.0)
    want = np.minimum(1.0, (zc - (0.6 - 0.53)) * m / (4 * voxel))
    assert wv[8, 8].tolist() == [0.0, 0.0] + [1.0] * (R - 2)
    assert (want[:2] <= -1.0).all() and (tv[8, 8, :2] == 0).all()
    err = np.abs(tv[8, 8, 2:].astype(np.float64) - want[2:]).max()
    print('analytic column: max |statement - closed form| =', err)
    assert err <= 1e-6
    assert (tv[8, 8, 2:] < 1).sum() >= 3 and tv[8, 8, -1] == 1.0                  # the band and the saturated free space above it


@pytest.mark.parametrize('name', NAMES)
def test_scenes_exercise_every_branch_away_from_every_flip(name):
    """A condition of the INPUTS, not a tolerance: no decision of the statement is closer than 1e-9 to its flip (a float64 operation
    rounds at 1e-16 relative), every weight 0..V occurs, the grid has zero, interior and saturated voxels, some tsdf is negative."""
    sc, st = T.scene(name), T.statement(name)
    V = sc['depth'].shape[0]
    hist = np.bincount(st['weight'].astype(np.int64).ravel(), minlength=V + 1)
    print(name, 'weights', hist.tolist(), 'margin', st['margin'].min(), 'hole', float((sc['depth'] == 0).mean()),
          'beyond depth_trunc', float((sc['depth'] >= 2).mean()), 'grid != 0', float((st['grid'] != 0).mean()))
    assert st['margin'].min() >= 1e-9
    assert len(hist) == V + 1 and (hist > 0).all()
    assert (st['grid'] == 0).any() and ((st['grid'] > 0) & (st['grid'] < 0.99)).any()
    assert ((st['weight'] != 0) & (st['tsdf'] >= np.float32(0.98))).any()           # observed but saturated
    assert (st['tsdf'] < 0).any()
    assert (sc['depth'][0] == 0).any() and (sc['depth'] >= 2).any()                 # the hole and pixels beyond depth_trunc
    assert np.array_equal(st['sdf_label'] == -1, st['grid'] == 0)


@pytest.mark.parametrize('name', NAMES)
def test_statement_view_by_view_equals_all_at_once(name):
    sc, st = T.scene(name), T.statement(name)
    R = sc['R']
    tv = wv = np.zeros((R, R, R), np.float32)
    mg = None
    for i in range(sc['depth'].shape[0]):
        tv, wv, mg = T.integrate(tv, wv, sc['depth'][i:i + 1], sc['poses'][i:i + 1], sc['Ks'][i:i + 1], sc['origin'], sc['voxel_size'],
                                 sc['sdf_trunc'], margin=mg)
    _same_bits(tv, st['tsdf'], name + ' tsdf'), _same_bits(wv, st['weight'], name + ' weight')
    assert np.array_equal(mg, st['margin'])


def _millimetres(sc):
    """The scene's depth as uint16 millimetres, and its float32 twin holding the same integers (both fused with depth_scale = 1000)."""
    mm = np.clip(np.rint(sc['depth'].astype(np.float64) * 1000.0), 0, 65535).astype(np.uint16)
    return mm, mm.astype(np.float32)


def test_statement_uint16_equals_its_float32_twin():
    sc = T.scene('small')
    mm, twin = _millimetres(sc)
    a, b = T.fuse(dict(sc, depth=mm, depth_scale=1000.0)), T.fuse(dict(sc, depth=twin, depth_scale=1000.0))
    for k in KEYS:
        _same_bits(a[k], b[k], 'uint16 / float32 twin ' + k)
    assert np.array_equal(a['margin'], b['margin']) and a['weight'].max() == 3 and (mm >= 2000).any()


class Entry:
    """One entry point with a complete set of acceptable arguments (keyword order = argument order); a call overrides some of them."""

    def __init__(self, name, **defaults):
        self.name, self.fn, self.defaults = name, getattr(_lib.lib(), name), defaults

    def __call__(self, **kw):
        assert set(kw) <= set(self.defaults), kw
        args = dict(self.defaults, **kw)
        return self.fn(*[C.byref(v) if isinstance(v, C.Structure) else v for v in args.values()])


def _params(**kw):
    f = dict(B=1, V=2, h=24, w=32, R=8, depth_dtype=_lib.GNR_DEPTH_F32, voxel_size=0.0375, sdf_trunc=0.075, depth_scale=1.0, depth_trunc=2.0)
    f.update(kw)
    return _lib.GnrTsdfParams(**f)


def test_entry_points_refuse_before_touching_the_device():
    """Null pointers, every limit, an unknown depth_dtype / mode: GNR_ERR_ARG / GNR_ERR_SHAPE with the entry point's own text, in the
    order of its checks, before the first launch.  EVERY call here is one that validation refuses (the pointers are fake: a call that
    passed would launch on a machine with a GPU and come back as GNR_ERR_HIP without one).  Runs without a GPU."""
    L = _lib.lib()

    def refused(code, text, entry, **kw):
        rc = entry(**kw)
        msg = L.gnr_last_error().decode()
        assert (rc, msg) == (code, text), (entry.name, kw, rc, msg)

    reset = Entry('gnr_tsdf_reset', B=1, R=8, tsdf=P, weight=P, stream=None)
    fuse = Entry('gnr_tsdf_integrate', p=_params(), depth=P, poses=P, Ks=P, origin=P, tsdf=P, weight=P, stream=None)
    grid = Entry('gnr_tsdf_grid', B=1, R=8, tsdf=P, weight=P, mode=_lib.GNR_TSDF_GRID, out=P, stream=None)

    for k in ('tsdf', 'weight'):
        refused(ARG, 'gnr_tsdf_reset: null pointer', reset, **{k: None})
    refused(ARG, 'gnr_tsdf_reset: null pointer', reset, tsdf=None, R=1)
    for B in (0, -1, 65536):
        refused(SHAPE, 'gnr_tsdf_reset: B must be in 1..65535', reset, B=B)
    for R in (1, 0, 257):
        refused(SHAPE, 'gnr_tsdf_reset: R must be in 2..256', reset, R=R)

    for k in ('p', 'depth', 'poses', 'Ks', 'origin', 'tsdf', 'weight'):
        refused(ARG, 'gnr_tsdf_integrate: null pointer', fuse, **{k: None})
    refused(ARG, 'gnr_tsdf_integrate: null pointer', fuse, depth=None, p=_params(R=1))
    for B in (0, 65536):
        refused(SHAPE, 'gnr_tsdf_integrate: B must be in 1..65535', fuse, p=_params(B=B))
    for R in (1, 257):
        refused(SHAPE, 'gnr_tsdf_integrate: R must be in 2..256', fuse, p=_params(R=R))
    refused(SHAPE, 'gnr_tsdf_integrate: R must be in 2..256', fuse, p=_params(R=1, V=0))
    for V in (0, -3):
        refused(SHAPE, 'gnr_tsdf_integrate: V must be >= 1', fuse, p=_params(V=V))
    for bad in (dict(h=0), dict(w=0), dict(h=-1, w=-1)):
        refused(SHAPE, 'gnr_tsdf_integrate: h and w must be >= 1', fuse, p=_params(**bad))
    for code in (2, -1):
        refused(ARG, 'gnr_tsdf_integrate: depth_dtype must be GNR_DEPTH_F32 or GNR_DEPTH_U16', fuse, p=_params(depth_dtype=code))
    for k in ('voxel_size', 'sdf_trunc', 'depth_scale', 'depth_trunc'):
        for bad in (0.0, -1.0, float('nan')):
            refused(ARG, 'gnr_tsdf_integrate: voxel_size, sdf_trunc, depth_scale and depth_trunc must be > 0', fuse, p=_params(**{k: bad}))

    for k in ('tsdf', 'weight', 'out'):
        refused(ARG, 'gnr_tsdf_grid: null pointer', grid, **{k: None})
    for B in (0, 65536):
        refused(SHAPE, 'gnr_tsdf_grid: B must be in 1..65535', grid, B=B)
    for R in (1, 257):
        refused(SHAPE, 'gnr_tsdf_grid: R must be in 2..256', grid, R=R)
    for mode in (2, -1):
        refused(ARG, 'gnr_tsdf_grid: mode must be GNR_TSDF_GRID or GNR_TSDF_SDF_LABEL', grid, mode=mode)
    refused(SHAPE, 'gnr_tsdf_grid: R must be in 2..256', grid, R=1, mode=2)


def test_python_layer_has_no_cpu_fallback(monkeypatch):
    import torch
    from graspnerf_amd.tsdf import TSDFVolume
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError):
        TSDFVolume(0.3, 40)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------
def _volume(sc, B=1, origin=None, **kw):
    from graspnerf_amd.tsdf import TSDFVolume
    return TSDFVolume(sc['size'], sc['R'], B=B, origin=sc['origin'] if origin is None else origin, sdf_trunc=sc['sdf_trunc'], **kw)


def _read(vol):
    import torch
    torch.cuda.synchronize()
    out = {'tsdf': vol.tsdf, 'weight': vol.weight, 'grid': vol.get_grid()[:, 0], 'sdf_label': vol.sdf_label()}
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, st, what, b=0):
    for k in KEYS:
        _same_bits(got[k][b], st[k], f'{what} {k}')


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_device_equals_the_statement_bitwise(name):
    """tsdf, weight, grid and sdf_label of one V-view call; V single-view calls give the same bits; a reset restores zeros and a second
    fusion after it gives the same bits again."""
    sc, st = T.scene(name), T.statement(name)
    vol = _volume(sc)
    assert vol.voxel_size == sc['voxel_size'] and vol.get_grid().shape == (1, 1, sc['R'], sc['R'], sc['R'])
    vol.integrate(sc['depth'], sc['Ks'][0], sc['poses'])
    _check(_read(vol), st, name)
    vol.reset()
    zero = _read(vol)
    assert not zero['tsdf'].any() and not zero['weight'].any() and not zero['grid'].any() and (zero['sdf_label'] == -1).all()
    for i in range(sc['depth'].shape[0]):
        vol.integrate(sc['depth'][i], sc['Ks'][i], sc['poses'][i])
    _check(_read(vol), st, name + ' view by view after a reset')


def _three_scenes():
    """B = 3 over the frames of `small`: per-scene origins a third of a voxel apart, and scene 1's view 1 turned half round about its
    own y axis at its place -- the whole workspace is behind it (pc.z <= 0 at every voxel)."""
    sc = T.scene('small')
    origins = np.stack([(sc['origin'].astype(np.float64) + b * sc['voxel_size'] / 3).astype(np.float32) for b in range(3)])
    poses = np.repeat(sc['poses'][None], 3, 0).copy()
    poses[1, 1] = np.diag([-1.0, 1.0, -1.0]).astype(np.float32) @ poses[1, 1]
    scenes = [dict(sc, origin=origins[b], poses=poses[b]) for b in range(3)]
    return sc, origins, poses, scenes


@pytest.mark.gpu
def test_three_scenes_in_one_call():
    sc, origins, poses, scenes = _three_scenes()
    sts = [T.fuse(s) for s in scenes]
    assert all(s['margin'].min() >= 1e-9 for s in sts)
    assert sts[1]['weight'].max() == 2 and sts[0]['weight'].max() == 3               # the view that looks away adds nothing
    vol = _volume(sc, B=3, origin=origins)
    vol.integrate(np.repeat(sc['depth'][None], 3, 0), sc['Ks'][0], poses)
    got = _read(vol)
    for b in range(3):
        _check(got, sts[b], f'B = 3, scene {b}', b)
        one = _volume(sc, origin=origins[b])
        one.integrate(sc['depth'], sc['Ks'], poses[b])
        alone = _read(one)
        for k in KEYS:
            _same_bits(got[k][b], alone[k][0], f'scene {b} of B = 3 against its own B = 1 call, {k}')


@pytest.mark.gpu
def test_uint16_depth_equals_its_float32_twin():
    sc = T.scene('small')
    mm, twin = _millimetres(sc)
    st = T.fuse(dict(sc, depth=mm, depth_scale=1000.0))
    got = []
    for depth in (mm, twin):
        vol = _volume(sc, depth_scale=1000.0)
        vol.integrate(depth, sc['Ks'], sc['poses'])
        got.append(_read(vol))
        _check(got[-1], st, f'depth {depth.dtype}')
    for k in KEYS:
        _same_bits(got[0][k], got[1][k], 'uint16 against float32 ' + k)


@pytest.mark.gpu
def test_resolution_120():
    """The 120^3 volume of acquire_tsdf (gd/simulation.py:341-367) on the frames of `small`: voxel indices beyond 64, 6 750 workgroups."""
    sc, st = T.scene('small', R=120), T.statement('small', R=120)
    assert st['margin'].min() >= 1e-9 and st['weight'].max() == 3
    vol = _volume(sc)
    vol.integrate(sc['depth'], sc['Ks'], sc['poses'])
    _check(_read(vol), st, 'R = 120')


@pytest.mark.gpu
def test_reset_integrate_grid_replay_in_a_captured_graph():
    """reset + integrate + grid recorded once on a side stream; replayed with the frames of `small` and then with the same cameras'
    frames of the moved spheres copied into the static input: each replay gives the bits of the eager call and of the statement."""
    import torch
    sc, moved = T.scene('small'), T.scene('small', moved=True)
    st = {'small': T.statement('small'), 'moved': T.statement('small', moved=True)}
    assert st['moved']['margin'].min() >= 1e-9 and not np.array_equal(st['small']['tsdf'], st['moved']['tsdf'])
    dev = torch.device('cuda:0')
    frames = {'small': torch.from_numpy(sc['depth']).to(dev), 'moved': torch.from_numpy(moved['depth']).to(dev)}
    K, E = torch.from_numpy(sc['Ks']).to(dev), torch.from_numpy(sc['poses']).to(dev)
    eager = {}
    for k, f in frames.items():
        vol = _volume(sc)
        vol.integrate(f, K, E)
        eager[k] = _read(vol)
    static = torch.zeros_like(frames['small'])
    vol = _volume(sc)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                       # warm-up on the capture stream (a fusion of zeros: nothing is observed)
        vol.reset(), vol.integrate(static, K, E), vol.get_grid()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        vol.reset()
        vol.integrate(static, K, E)
        grid, label = vol.get_grid(), vol.sdf_label()
    for k in ('small', 'moved', 'small'):
        static.copy_(frames[k])
        graph.replay()
        torch.cuda.synchronize()
        got = {'tsdf': vol.tsdf.cpu().numpy(), 'weight': vol.weight.cpu().numpy(), 'grid': grid[:, 0].cpu().numpy(), 'sdf_label': label.cpu().numpy()}
        _check(got, st[k], f'replay {k} against the statement')
        for key in KEYS:
            _same_bits(got[key], eager[k][key], f'replay {k} against the eager call, {key}')


def _head_state_dict():
    """Seed-0 synthetic parameters of the grasp head (synth_state_dict); the quality bias raised so that qualities pass 0.9 and the
    width bias so that widths fall inside detection.py's 1.33..9.33 voxels (as tests/test_planner_session.py does)."""
    from graspnerf_amd.backbone import ConvNet
    syn = synth_state_dict({k: tuple(v.shape) for k, v in ConvNet().state_dict().items()}, seed=0)
    syn['conv_qual.bias'] = syn['conv_qual.bias'] + np.float32(2.5)
    syn['conv_width.bias'] = syn['conv_width.bias'] + np.float32(5.0)
    return syn


def _task_frame_scene():
    """`small` at R = 40 with six views, its cameras re-expressed in the volume's own frame (origin at zero, perception.py's
    convention: extrinsics are T_eye_task), and the statement of exactly these float32 poses."""
    sc = T.scene('small', R=40, V=6)
    poses = sc['poses'].astype(np.float64)
    poses[:, :, 3] += poses[:, :, :3] @ sc['origin'].astype(np.float64)
    sc = dict(sc, origin=np.zeros(3, np.float32), poses=poses.astype(np.float32))
    return sc, T.fuse(sc)


@pytest.mark.gpu
def test_plan_depth_is_the_vgn_route():
    """planner.plan_depth on six 96 x 128 frames at R = 40 (cameras in the volume's frame): the selection is grasp_post_oracle's process + select (detection.py's
    defaults) on the device head's volumes and the STATEMENT's grid -- indices exact, scores bitwise -- under the seed's permutation,
    positions = index * size / R."""
    import types
    import torch
    from graspnerf_amd import planner
    from graspnerf_amd.grasp_head import GraspHead
    from graspnerf_amd.tsdf import TSDFVolume
    from oracle import grasp_post_oracle as PO
    sc, st = _task_frame_scene()
    assert st['margin'].min() >= 1e-9 and (st['grid'] != 0).any()
    head = GraspHead(_head_state_dict())
    K = sc['Ks'][0]
    intrinsic = types.SimpleNamespace(width=128, height=96, fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]), cy=float(K[1, 2]))
    grasps, scores, dt = planner.plan_depth(head, sc['depth'], intrinsic, sc['poses'], size=sc['size'], resolution=40, seed=3)
    q, r, w = (x.cpu().numpy() for x in head(torch.from_numpy(st['grid'][None, None]).cuda()))
    qual = PO.process(st['grid'], q[0, 0], r[0], w[0, 0])
    idx, score, quat, width = PO.select(qual, r[0], w[0, 0])
    n = len(idx)
    print('plan_depth:', n, 'grasps,', round(dt * 1e3, 2), 'ms')
    assert n > 0 and len(grasps['index']) == n and dt > 0
    np.random.seed(3)
    p = np.random.permutation(n)
    assert np.array_equal(grasps['index'], idx[p])
    _same_bits(grasps['score'], score[p], 'scores')
    assert scores is grasps['score'] or np.array_equal(scores, grasps['score'])
    assert np.array_equal(grasps['pos'], idx[p].astype(np.float64) * (sc['size'] / 40))
    _same_bits(grasps['width'], (width[p] * (sc['size'] / 40)).astype(np.float32), 'widths')
    lists = [np.r_[_quat(e[:, :3]), e[:, 3]] for e in sc['poses'].astype(np.float64)]    # the reference's Transform.to_list()
    K7, E7 = TSDFVolume(sc['size'], 40)._cameras(intrinsic, lists, 6)
    assert np.array_equal(K7.cpu().numpy()[0], sc['Ks']) and np.abs(E7.cpu().numpy()[0] - sc['poses']).max() < 1e-6


def _quat(Rm):
    """(x, y, z, w) of a rotation matrix (trace > -1 branch suffices for the ring cameras' test poses or falls back on the largest axis)."""
    t = np.trace(Rm)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        return np.array([(Rm[2, 1] - Rm[1, 2]) / s, (Rm[0, 2] - Rm[2, 0]) / s, (Rm[1, 0] - Rm[0, 1]) / s, 0.25 * s])
    i = int(np.argmax(np.diag(Rm)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(1.0 + Rm[i, i] - Rm[j, j] - Rm[k, k]) * 2
    q = np.zeros(4)
    q[i], q[j], q[k], q[3] = 0.25 * s, (Rm[j, i] + Rm[i, j]) / s, (Rm[k, i] + Rm[i, k]) / s, (Rm[k, j] - Rm[j, k]) / s
    return q


@pytest.mark.gpu
def test_trainer_labels_a_scene_from_its_depth():
    """One Trainer.step on a scene without sdf_gt: with sdf_gt_from_depth=True its loss_sdf and sdf_mae are those of the same step fed
    the statement's label of the scene's true_depth (bitwise); with the switch off the missing key raises as it always did."""
    import torch
    from graspnerf_amd.trainer import Trainer
    from test_train_step import build, scene_data
    data = scene_data('cuda')
    ref = data['ref_imgs_info']
    R, voxel = 16, 0.3 / 16
    z0 = np.zeros((R, R, R), np.float32)
    tv, wv, mg = T.integrate(z0, z0, ref['true_depth'][:, 0].cpu().numpy(), ref['poses'].cpu().numpy(), ref['Ks'].cpu().numpy(),
                             ref['bbox3d'][0].cpu().numpy(), voxel, 4 * voxel)
    label = T.sdf_label(T.grid(tv, wv))
    assert mg.min() >= 1e-9 and (label != -1).any() and (label == -1).any()
    bare = dict(data, ref_imgs_info={k: v for k, v in ref.items() if k != 'sdf_gt'}, src_imgs_info={k: v for k, v in ref.items() if k != 'sdf_gt'})
    fed = dict(bare, ref_imgs_info=dict(bare['ref_imgs_info'], sdf_gt=torch.from_numpy(label).cuda()))
    recorded = {}

    class Replay(torch.nn.Module):
        """A 2D feature extractor held fixed: MIOpen's convolutions are not bit-reproducible from call to call (tests/test_determinism.py),
        and the comparison is about the label."""

        def __init__(self, name):
            super().__init__()
            self.name = name

        def forward(self, *a, **k):
            return recorded[self.name].clone().requires_grad_(True)

    def net():
        n = build('cuda')
        nr = n.nr_net
        if not recorded:
            with torch.no_grad():
                recorded['img'] = nr.image_encoder(ref['imgs'])
                recorded['ray'] = nr.vis_encoder(nr.init_net({'imgs': ref['imgs']}, None, True), recorded['img'])
        nr.image_encoder, nr.init_net, nr.vis_encoder = Replay('img'), Replay('ray'), Replay('ray')
        return n
    logs = {}
    for name, scene, switch in (('from depth', bare, True), ('fed', fed, False)):
        tr = Trainer(net(), {'lr_init': 1e-3}, sdf_gt_from_depth=switch)
        torch.manual_seed(1)
        logs[name] = tr.step([scene])
    print({k: {t: v[t] for t in ('loss_sdf', 'sdf_mae')} for k, v in logs.items()})
    for term in ('loss_sdf', 'sdf_mae'):
        assert np.isfinite(logs['fed'][term]) and logs['from depth'][term] == logs['fed'][term], term
    assert 'sdf_gt' not in bare['ref_imgs_info']                                     # the caller's scene is not written to
    with pytest.raises(KeyError):
        Trainer(net(), {'lr_init': 1e-3}).step([bare])
