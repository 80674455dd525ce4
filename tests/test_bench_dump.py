"""bench.py --dump-outputs: the arrays the last timed step computed, as DIR/<name>.npy in float32, at most 64 MB in all (a larger
batch keeps a fixed seeded sample of its scenes), and --steps < 1 refused.  The GPU test runs the benchmark and checks scene 0 of
the dump against the reference golden the parity gate pins."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _outputs(B, rn=7, dn=5):
    """Stand-ins of (volume, coarse dict, fine dict) whose every entry of scene i holds the value i."""
    s = torch.arange(B, dtype=torch.float32)

    def level():
        return {'sdf_values': s[:, None, None].expand(B, rn, dn).contiguous(), 'render_depth': s[:, None].expand(B, rn).contiguous(),
                'ray_mask': (s[:, None].expand(B, rn) % 2).to(torch.bool)}
    return s[:, None, None, None, None].expand(B, 1, 4, 4, 4).contiguous(), level(), level()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_output_of_every_scene_in_float32(tmp_path):
    _bench().dump_outputs(str(tmp_path), _outputs(6), 10)
    got = _load(tmp_path)
    assert sorted(got) == ['coarse_ray_mask', 'coarse_render_depth', 'coarse_sdf_values', 'fine_ray_mask', 'fine_render_depth',
                           'fine_sdf_values', 'scene_index', 'volume']
    assert got['volume'].shape == (6, 1, 4, 4, 4) and got['coarse_sdf_values'].shape == (6, 7, 5)
    assert all(v.dtype == (np.float64 if k == 'scene_index' else np.float32) for k, v in got.items())
    assert np.array_equal(got['scene_index'], np.arange(10, 16))
    assert np.array_equal(got['fine_ray_mask'], np.arange(6)[:, None].repeat(7, 1) % 2)


def test_dump_of_a_large_batch_is_a_fixed_sample_of_whole_scenes_within_the_budget(tmp_path, monkeypatch):
    m = _bench()
    monkeypatch.setattr(m, 'DUMP_MAX_BYTES', 4000)
    for d in ('a', 'b'):
        m.dump_outputs(str(tmp_path / d), _outputs(40), 0)
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sum(v.nbytes for v in a.values()) <= 4000
    rows = a['scene_index'].astype(int)
    assert 1 <= len(rows) < 40 and np.all(np.diff(rows) > 0)
    for k, v in a.items():
        assert np.array_equal(v, b[k]), k                                        # the same sample every run
        if k not in ('scene_index', 'coarse_ray_mask', 'fine_ray_mask'):
            assert np.array_equal(v.reshape(len(rows), -1)[:, 0], rows), k     # the same scenes in every array


@pytest.mark.parametrize('args', [['--steps', '0'], ['--dump-outputs', 'x', '--stub-step-ms', '1']])
def test_bench_refuses_arguments_it_cannot_honour(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and 'error' in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_outputs_of_its_last_timed_step(tmp_path, golden):
    from test_gpu_parity import close, ATOL_A, ATOLS
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--batch', '2', '--steps', '3', '--warmup', '1', '--no-train',
                        '--no-backbones', '--no-f32-build', '--no-live-pmc', '--no-cpu-baseline', '--dump-outputs', str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert line['steps'] == 3
    got = _load(tmp_path)
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert np.array_equal(got['scene_index'], [0, 1]) and got['volume'].shape == (2, 1, 40, 40, 40)
    assert all(v.dtype == np.float32 for k, v in got.items() if k != 'scene_index')
    G = golden('cfg2')
    close(got['volume'][0], G['volume'][0], 'bench dump scene 0 volume vs reference golden')
    for k in ('sdf_values', 'alpha_values', 'colors_nr', 'hit_prob_nr', 'pixel_colors_nr', 'pixel_colors_gt', 'render_depth', 'sdf_gradient_error'):
        close(got['coarse_' + k][0], G['render.' + k][0], f'bench dump scene 0 coarse {k}', atol=ATOLS.get(k, ATOL_A))
    assert np.array_equal(got['coarse_ray_mask'][0], G['render.ray_mask'][0])
    assert np.isfinite(got['fine_sdf_values']).all()
