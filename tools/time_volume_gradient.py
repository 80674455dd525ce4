"""Cost of the SDF gradient volume (gnr_sample_volume_grad_fwd) at the planner's shape -- R = 40, 6 views of 288x512 -- for B = 1 and
B = 32, between the library's own event brackets (gnr_timing_begin / gnr_timing_end: HIP events around every launch, on its stream),
next to gnr_sample_volume_fwd and to a coarse gnr_render_by_depth_fwd of 1 600 rays x 40 samples (the same point count through the same
kernels) in the same run.  Writes the `cost` record of profiles/volume_gradient.json (the other records of that file are kept).
Usage: python tools/time_volume_gradient.py [--iters 20] [--out profiles/volume_gradient.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graspnerf_amd import _lib, weights                                      # noqa: E402
from graspnerf_amd.hotpath import HotPath, batch_scenes                      # noqa: E402
from graspnerf_amd.synth import make_scene                                   # noqa: E402

R, RN, DN = 40, 1600, 40


def bracket(f, iters):
    """-> {label: ms per call} and their sum, over `iters` calls of f between the library's brackets (after two warm-up calls)."""
    f(), f()
    torch.cuda.synchronize()
    _lib.timing_begin()
    for _ in range(iters):
        f()
    torch.cuda.synchronize()
    t = {k: round(ms / iters, 5) for k, (n, ms) in sorted(_lib.timing_end().items())}
    return {'kernels_ms': t, 'total_ms': round(sum(t.values()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_gradient.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_volume_gradient.py measures on a ROCm GPU; there is nothing to time without one')
    wnp = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'weights_seed0.npz')))
    hp = HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))
    rng = np.random.default_rng(0)
    res = {'shape': {'volume_resolution': R, 'views': 6, 'image': [288, 512], 'render': f'{RN} rays x {DN} samples, coarse level, by depth'},
           'unit': 'ms per call, sum of the HIP-event brackets of the call\'s launches', 'iters': a.iters, 'device': torch.cuda.get_device_name(0)}
    for B in (1, 32):
        scenes = [make_scene(i % 4, 'cfg2', with_query_image=False) for i in range(B)]
        bref, bque = batch_scenes(scenes)
        bref = {k: torch.from_numpy(v).cuda() for k, v in bref.items()}
        coords = np.stack([rng.uniform(0, 511, (B, RN)), rng.uniform(0, 287, (B, RN))], -1).astype(np.float32)
        bque = dict(bque, coords=coords)
        near, far = 0.2, 0.8
        depth = np.broadcast_to(1.0 / np.linspace(1.0 / near, 1.0 / far, DN, dtype=np.float64), (B, RN, DN)).astype(np.float32)
        depth = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
        prep = hp.prepare(bref, R, RN, DN, grad_res=R)
        rec = {'sample_volume_gradient': bracket(lambda: hp.sample_volume_gradient(bref, R, want_error=True, prepared=prep), a.iters),
               'sample_volume': bracket(lambda: hp.sample_volume(bref, R, prepared=prep), a.iters),
               'render_by_depth_coarse': bracket(lambda: hp.render_by_depth(bref, bque, depth, 'coarse', prepared=prep), a.iters)}
        rec['gradient_over_render'] = round(rec['sample_volume_gradient']['total_ms'] / rec['render_by_depth_coarse']['total_ms'], 4)
        rec['gradient_over_volume'] = round(rec['sample_volume_gradient']['total_ms'] / rec['sample_volume']['total_ms'], 4)
        rec['range_status'] = hp.range_status(prep)
        res[f'B={B}'] = rec
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out['cost'] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
