"""Cost of the depth route's TSDF fusion (gnr_tsdf_integrate) at the planner's frames -- 6 views of 288x512 -- into 40^3 for B = 1 and
B = 32 and into 120^3 for B = 1 (the two volumes of gd/simulation.py:341-367): p10 / p50 / p90 of single calls between HIP events, the
state traffic that time stands for (tsdf and weight read and written once per call) in GB/s, reset + integrate + grid together, and
the numpy float64 statement (tests/tsdf_reference.py) of one scene on the same box's CPU.  The frames are the analytic test scene's.
Usage: python tools/time_tsdf.py [--calls 100] [--out profiles/tsdf_fusion.json]"""
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
import tsdf_reference as T                                                   # noqa: E402
from graspnerf_amd.synth import CONFIGS                                      # noqa: E402
from graspnerf_amd.tsdf import TSDFVolume                                    # noqa: E402

V, H, W = 6, 288, 512


def event_ms(f, calls):
    """Milliseconds of `calls` single calls of f, each between its own pair of HIP events (after three warm-up calls)."""
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return np.asarray([a.elapsed_time(b) for a, b in pairs])


def pct(ms):
    return {k: round(float(np.percentile(ms, q)), 5) for k, q in (('p10', 10), ('p50', 50), ('p90', 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsdf_fusion.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_tsdf.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    dev = torch.device('cuda:0')
    sc = T.make_scene(V, H, W, CONFIGS['cfg2']['K'], 40, 4)
    res = {'shape': {'views': V, 'image': [H, W], 'depth': 'float32, analytic plane + two spheres (tests/tsdf_reference.py)'},
           'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls', 'calls': a.calls,
           'state_traffic': 'tsdf and weight [B,R,R,R] float32, each read and written once per integrate call: 16 * B * R^3 bytes',
           'device': torch.cuda.get_device_name(0)}
    for R, B in ((40, 1), (40, 32), (120, 1)):
        vol = TSDFVolume(sc['size'], R, B=B, origin=sc['origin'])
        depth = torch.from_numpy(sc['depth']).to(dev)[None].expand(B, V, H, W).contiguous()
        K, E = (torch.from_numpy(sc[k]).to(dev)[None].expand(B, *sc[k].shape).contiguous() for k in ('Ks', 'poses'))

        def all_three():
            vol.reset()
            vol.integrate(depth, K, E)
            vol.get_grid()
        fuse = pct(event_ms(lambda: vol.integrate(depth, K, E), a.calls))
        rec = {'integrate_ms': fuse, 'state_gb_per_s_at_p50': round(16.0 * B * R ** 3 / (fuse['p50'] * 1e-3) / 1e9, 2),
               'reset_integrate_grid_ms': pct(event_ms(all_three, a.calls))}
        res[f'R={R},B={B}'] = rec
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        T.fuse(sc)
        times.append((time.perf_counter() - t0) * 1e3)
    res['host_statement_one_scene_R40_ms'] = {'median_of_5': round(float(np.median(times)), 3), 'what': 'numpy float64, one process thread'}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
