"""Cost of the surface mesh (gnr_surface_mesh_fwd, grasp_post.MeshExtractor) of SDF volumes: 40^3 for B = 1 and B = 32 and 120^3 for
B = 1, with and without the gradient volume: p10 / p50 / p90 of single calls between HIP events, next to the host route to the same
mesh -- the volume read back and the numpy float64 statement (tests/mesh_reference.py) on this box's CPU.  The volumes are a sphere and
a torus joined, scaled like a predicted SDF (values in [-1, 1], a few per cent of the cells on the surface).
Then the real-robot plan (planner.plan_real through planner.real_session; tools/time_planner.py --real, leg (b)) with and without the
mesh in the session's graph, host clock around the whole call, alternating: with the mesh of iso = 0 (mesh=True) and with the level at the
synthetic checkpoint's median, where the surface is larger.
Usage: python tools/time_mesh.py [--calls 100] [--out profiles/surface_mesh.json] [--session-out profiles/planner_session_mesh.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import mesh_reference as M                                                   # noqa: E402
from graspnerf_amd.grasp_post import MeshExtractor                           # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402


def scene(R, shift):
    """A sphere and a torus, side by side, as a clipped signed distance in voxel units / 8."""
    s = R / 40.0
    a = M.sphere(R, (12.3 * s + shift, 13.6 * s, 14.45 * s), 8.2 * s)
    b = M.torus(R, (26.3 * s, 25.6 * s - shift, 24.45 * s), 8.5 * s, 3.0 * s)
    return np.clip(np.minimum(a, b) / 8.0, -1.0, 1.0).astype(np.float32)


def kernels(a):
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls', 'calls': a.calls,
           'volumes': 'a sphere and a torus, clipped signed distance (tools/time_mesh.py), iso = 0', 'device': torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    for R, B in ((40, 1), (40, 32), (120, 1)):
        vol = torch.from_numpy(np.stack([scene(R, 0.37 * b) for b in range(B)])).to(dev)
        grad = torch.from_numpy(rng.standard_normal((B, R, R, R, 3)).astype(np.float32)).to(dev)
        ex = MeshExtractor(dev)
        out = ex(vol, gradient=grad)
        count = out['count'].cpu().numpy()
        rec = {'vertices_scene0': int(count[0, 0]), 'triangles_scene0': int(count[0, 1]), 'active_cells_share': round(float(count[0, 0]) / (R - 1) ** 3, 4),
               'mesh_ms': pct(event_ms(lambda: ex(vol), a.calls)), 'mesh_with_gradient_ms': pct(event_ms(lambda: ex(vol, gradient=grad), a.calls))}
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = vol[0].cpu().numpy()
            want = M.surface_mesh(host, scale=0.3 / 40)                          # MeshExtractor's default frame
            times.append((time.perf_counter() - t0) * 1e3)
        rec['host_route_one_scene_ms'] = {'median_of_3': round(float(np.median(times)), 3), 'what': 'volume read back + numpy float64 statement, no gradient'}
        rec['equals_host_route'] = bool(np.array_equal(out['vertices'][0, :count[0, 0]].cpu().numpy(), want['vertices'])
                                        and np.array_equal(out['faces'][0, :count[0, 1]].cpu().numpy(), want['faces']))
        res[f'R={R},B={B}'] = rec
    return res


def session(a):
    import time_planner as TP
    res, last, iso = TP.session_legs(a.calls, lambda iso: {'b_with_mesh_iso0': dict(mesh=True), 'c_with_mesh_at_the_median': dict(mesh=dict(iso=iso))})
    m = last['c_with_mesh_at_the_median'][3]['mesh']
    res['mesh_at_the_median'] = {'iso': iso, 'vertices': int(len(m['vertices'])), 'triangles': int(len(m['faces']))}
    res['mesh_iso0_vertices'] = int(len(last['b_with_mesh_iso0'][3]['mesh']['vertices']))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'surface_mesh.json'))
    ap.add_argument('--session-out', default=os.path.join(ROOT, 'profiles', 'planner_session_mesh.json'))
    ap.add_argument('--skip-session', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_mesh.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    jobs = [(a.out, kernels)] + ([] if a.skip_session else [(a.session_out, session)])
    for path, job in jobs:
        res = job(a)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))


if __name__ == '__main__':
    main()
