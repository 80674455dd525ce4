"""Cost of the view colours of surface points (gnr_surface_color_points_fwd / gnr_surface_color_pixels_fwd, surface_color.SurfaceColorizer)
at the real-robot route's shape -- a 40^3 volume, 6 source frames of 288 x 512: the points kernel on the surface cloud and on the mesh's
vertices, the pixels kernel on the 6 ray-cast depth frames of the plan's own cameras; p10 / p50 / p90 of single calls between HIP events,
next to the host route to the same bits -- the numpy float64 statement (tests/surface_color_reference.py) on this box's CPU, on the same
inputs.  The volume is tools/time_mesh.py's (a sphere and a torus, a clipped signed distance) on the real-robot route's lattice; the
cameras ring the workspace at the planner's distance; the frames are random.
Then the real-robot plan (planner.plan_real through planner.real_session) with the mesh and the ray cast in the session's graph, without
and with view_colors, host clock around the whole call, alternating, with the level at the synthetic checkpoint's median.
Usage: python tools/time_surface_color.py [--calls 100] [--out profiles/surface_color.json]"""
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
import surface_color_reference as SC                                         # noqa: E402
from graspnerf_amd import planner                                            # noqa: E402
from graspnerf_amd.grasp_post import MeshExtractor, SurfaceExtractor         # noqa: E402
from graspnerf_amd.raycast import VolumeRaycaster                            # noqa: E402
from graspnerf_amd.surface_color import SurfaceColorizer                     # noqa: E402
from graspnerf_amd.synth import ring_cameras                                 # noqa: E402
from time_mesh import scene                                                  # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402

HW = (288, 512)
K = np.float32([[357.048, 0, 255.8], [0, 357.048, 143.8], [0, 0, 1]])
R, V = 40, 6


def kernels(a):
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls', 'calls': a.calls, 'source_frames': [V, 3, *HW],
           'volume': 'a sphere and a torus, clipped signed distance (tools/time_mesh.py), 40^3, iso = 0, step 0.5, bias 1.5, cos_min 0',
           'device': torch.cuda.get_device_name(0)}
    scale = 0.3 / R
    origin = np.asarray(planner.REAL_BBOX3D[0], np.float64) + 0.5 * scale
    frame = dict(origin=origin, scale=scale)
    host_vol = scene(R, 0.0)
    vol = torch.from_numpy(host_vol[None]).to(dev)
    images = np.random.default_rng(0).random((V, 3, *HW)).astype(np.float32)
    poses, Ks = np.asarray(ring_cameras(V), np.float32)[:, :3, :], np.repeat(K[None], V, 0)
    I, P, Kd = (torch.from_numpy(x).to(dev) for x in (images, poses, Ks))
    paint = SurfaceColorizer(dev)
    same = lambda got, want: bool(all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want)))
    cloud = SurfaceExtractor(dev)(vol, scale=scale)
    mesh = MeshExtractor(dev)(vol, scale=scale)
    for name, pts, cnt in (('points_cloud', cloud['points'], cloud['count']), ('points_mesh_vertices', mesh['vertices'], mesh['count'])):
        call = lambda: paint.points(vol, pts, cnt, I, P, Kd, point_offset=origin, **frame)
        n = int(cnt.reshape(1, -1)[0, 0])
        got = [call()[k][0, :n].cpu().numpy() for k in ('view_colors', 'view_weight', 'view_mask')]
        rec = {'rows': n, 'buffer_rows': int(pts.shape[1]), 'coloured_share': round(float((got[1] > 0).mean()), 4), 'device_ms': pct(event_ms(call, a.calls))}
        host_pts = pts[0].cpu().numpy()
        t0 = time.perf_counter()
        want = SC.color_points(host_vol, host_pts[:n], n, images, poses, Ks, point_offset=origin, **frame)
        rec['host_statement_ms'] = {'once': round((time.perf_counter() - t0) * 1e3, 1), 'what': 'numpy float64 statement on the same rows'}
        rec['equals_host_statement'] = same(got, want)
        res[name] = rec
    depth = VolumeRaycaster(dev)(vol, P, Kd, HW, **frame)['depth']
    call = lambda: paint.pixels(vol, depth, P, Kd, I, P, Kd, **frame)
    got = [call()[k][0].cpu().numpy() for k in ('color', 'color_weight', 'color_mask')]
    host_depth = depth[0].cpu().numpy()
    rec = {'pixels': int(host_depth.size), 'hit_share': round(float((host_depth > 0).mean()), 4), 'coloured_share': round(float((got[1] > 0).mean()), 4),
           'device_ms': pct(event_ms(call, a.calls))}
    t0 = time.perf_counter()
    want = SC.color_pixels(host_vol, host_depth, poses, Ks, images, poses, Ks, **frame)
    rec['host_statement_ms'] = {'once': round((time.perf_counter() - t0) * 1e3, 1), 'what': 'numpy float64 statement on the same depth frames'}
    rec['equals_host_statement'] = same(got, want)
    res['pixels_six_depth_frames'] = rec
    return res


def session(a):
    import time_planner as TP
    both = lambda iso: dict(mesh=dict(iso=iso), volume_depth=dict(iso=iso))
    res, last, _ = TP.session_legs(a.calls, lambda iso: {'b_with_mesh_and_volume_depth_at_the_median': both(iso),
                                                         'c_the_same_with_view_colors': dict(both(iso), view_colors=True)})
    res['c_minus_b_p50'] = res['c_the_same_with_view_colors']['p50'] - res['b_with_mesh_and_volume_depth_at_the_median']['p50']
    c = last['c_the_same_with_view_colors'][3]
    res['coloured'] = {'cloud_points': [int((c['view_weight'] > 0).sum()), len(c['view_weight'])],
                       'mesh_vertices': [int((c['mesh']['view_weight'] > 0).sum()), len(c['mesh']['view_weight'])],
                       'pixels': [int((c['volume_color_weight'] > 0).sum()), int(c['volume_color_weight'].size)]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'surface_color.json'))
    ap.add_argument('--skip-session', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_surface_color.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    res = kernels(a)
    if not a.skip_session:
        res['planner_session'] = session(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
