"""The layer the volume operators share around their kernels: the byte counts of their workspaces (csrc/gnr_host.h's Carve; Python
callers allocate by them), and the Python vocabulary of the solid rule and of a plan's grasp rows (grasp_post.checked_solid,
hand.plan_rows).  Everything here runs without a GPU."""
import math

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, distance, grasp_post, hand, objects

# *_workspace_bytes(B, R) of the library built from the commit before the workspaces were carved by gnr::Carve, at (3, 8) and (1, 40)
WORKSPACE_BYTES = {
    'gnr_surface_mesh_workspace_bytes': (4864, 237824),
    'gnr_grasp_select_workspace_bytes': (16896, 704000),
    'gnr_surface_points_workspace_bytes': (256, 256),
    'gnr_volume_objects_workspace_bytes': (12800, 512512),
    'gnr_volume_distance_workspace_bytes': (36864, 1536000),
}


def test_workspace_byte_counts_are_what_callers_allocate_by():
    L = _lib.lib()
    for name, want in WORKSPACE_BYTES.items():
        fn = getattr(L, name)
        assert (fn(3, 8), fn(1, 40)) == want, name
    v2 = L.gnr_grasp_select_v2_workspace_bytes
    assert (v2(3, 8, _lib.GNR_SELECT_ORDER_INDEX), v2(1, 40, _lib.GNR_SELECT_ORDER_INDEX)) == (16896, 704000)
    assert (v2(3, 8, _lib.GNR_SELECT_ORDER_SCORE), v2(1, 40, _lib.GNR_SELECT_ORDER_SCORE)) == (41472, 1728000)
    fm = L.gnr_frame_metrics_workspace_bytes                  # (B, h, w, n_pred, h_margin, w_margin, ssim)
    assert (fm(3, 33, 64, 2, 0, 0, 1), fm(3, 33, 64, 2, 0, 0, 0), fm(3, 240, 320, 4, 8, 8, 1)) == (1536, 768, 43008)
    assert (fm(1, 33, 64, 2, 0, 0, 1), fm(1, 33, 64, 2, 0, 0, 0), fm(1, 240, 320, 4, 8, 8, 1)) == (1024, 768, 14848)
    # outside the limits: 0 where the operator has a batch or a lattice limit, the select's and the cloud's sizes as they always were
    for name in ('gnr_surface_mesh_workspace_bytes', 'gnr_volume_objects_workspace_bytes', 'gnr_volume_distance_workspace_bytes'):
        fn = getattr(L, name)
        assert [fn(B, R) for B, R in ((0, 8), (65536, 8), (1, 1), (1, 257))] == [0, 0, 0, 0], name
        assert fn(65535, 2) > 0 and fn(1, 256) > 0, name
    for fn in (L.gnr_grasp_select_workspace_bytes, L.gnr_surface_points_workspace_bytes):
        assert fn(0, 8) == 0 and fn(1, 0) == 0 and fn(65536, 8) > 0 and fn(1, 1) == 256 * (5 if fn is L.gnr_grasp_select_workspace_bytes else 1)
    # the objects' status word keeps the first 256 bytes to itself: two int volumes and the chunk counts lie behind it
    assert L.gnr_volume_objects_workspace_bytes(1, 8) == 256 + 2 * 2048 + 256


@pytest.mark.parametrize('what', ['objects', 'distance'])
def test_checked_solid_raises_each_text_for_both_nouns(what):
    ok = dict(level=0.0, lower=None, z_min=0)
    assert grasp_post.SOLID_DEFAULTS == ok and grasp_post.checked_solid(what, **ok) == ok
    assert grasp_post.checked_solid(what, 1, -1, 3.0) == dict(level=1.0, lower=-1.0, z_min=3)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError) as e:
            grasp_post.checked_solid(what, bad, None, 0)
        assert str(e.value) == f'{what} level must be finite, got {bad!r}'
    with pytest.raises(ValueError) as e:
        grasp_post.checked_solid(what, 0.0, math.nan, 0)
    assert str(e.value) == f'{what} lower must be None (no lower bound) or a number, got nan'
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError) as e:
            grasp_post.checked_solid(what, 0.0, None, bad)
        assert str(e.value) == f'{what} z_min must be an integer >= 0, got {bad!r}'
    q = grasp_post.checked_solid(what, 0.0, None, 9)
    with pytest.raises(ValueError) as e:
        grasp_post.solid_fields(what, q, 8, 9.0)
    assert str(e.value) == f'{what} z_min must be in 0..R = 8, got 9.0'
    assert grasp_post.solid_fields(what, q, 9, 9) == dict(level=0.0, lower=-math.inf, z_min=9)
    assert grasp_post.solid_fields(what, grasp_post.checked_solid(what, 0.5, -1, 0), 8, 0) == dict(level=0.5, lower=-1.0, z_min=0)
    # the operators' own checks are built on it
    checked = dict(objects=objects.checked_objects, distance=distance.checked_distance)[what]
    defaults = dict(objects=objects.OBJECT_DEFAULTS, distance=distance.DISTANCE_DEFAULTS)[what]
    assert checked() == defaults and list(defaults)[:3] == list(ok)
    with pytest.raises(ValueError, match=f'^{what} z_min must be an integer >= 0, got -1$'):
        checked(z_min=-1)


def test_split_params_merges_the_defaults_and_names_unknown_keys():
    a, b = dict(x=1, y=2), dict(z=3)
    assert grasp_post.split_params('objects', dict(y=5), a, b) == dict(x=1, y=5, z=3)
    assert grasp_post.split_params('objects', {}, a, b) == dict(x=1, y=2, z=3)
    with pytest.raises(TypeError) as e:
        grasp_post.split_params('distance', dict(w=0, y=1, v=2), a, b)
    assert str(e.value) == "unknown distance parameters ['v', 'w']; it takes ['x', 'y', 'z']"


@pytest.mark.parametrize('n', [0, 3])
def test_plan_rows_builds_the_rows_the_plan_adapters_built(n):
    """The expected arrays are objects_of_plan's own construction before it called plan_rows."""
    rng = np.random.default_rng(n)
    voxel_size = 0.3 / 40
    grasps = {'index': rng.integers(0, 40, (n, 3)).astype(np.int32), 'quat': rng.standard_normal((n, 4)).astype(np.float32),
              'width': rng.uniform(0.01, 0.08, n).astype(np.float32), 'pos': rng.standard_normal((n, 3))}
    index, quat, width = np.asarray(grasps['index']), np.asarray(grasps['quat']), np.asarray(grasps['width'])
    rows = max(n, 1)
    pos, qt, wd = np.zeros((1, rows, 3), np.float64), np.zeros((1, rows, 4), np.float32), np.zeros((1, rows), np.float32)
    pos[0, :n], qt[0, :n], wd[0, :n] = index.reshape(n, 3), quat.reshape(n, 4), (width.reshape(n) / np.float32(voxel_size)).astype(np.float32)
    got = hand.plan_rows(grasps, voxel_size, torch.device('cpu'))
    assert len(got) == 5 and got[4] == n
    for g, w in zip(got[:3], (pos, qt, wd)):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    count = got[3]
    assert torch.is_tensor(count) and count.dtype == torch.int32 and tuple(count.shape) == (1,) and count.tolist() == [n]
    assert got[0].shape == (1, rows, 3) and got[1].shape == (1, rows, 4) and got[2].shape == (1, rows)
