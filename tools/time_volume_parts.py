"""Cost of the parts of the volume (gnr_volume_parts_fwd, parts.VolumeParts) at three shapes -- B = 1 at 40^3, B = 32 at 40^3, B = 1 at
128^3 -- on a cluttered scene (a slab, a heap of six balls that touch or overlap their neighbours, eight floaters): p10 / p50 / p90 of
single calls between HIP events, of VolumeParts alone on a d2_free computed before, of the chain VolumeDistance then VolumeParts, and,
for scale, of VolumeObjects on the same volumes in the same run.  In a pass of its own, every launch of the call bracketed by events
(gnr_timing_begin): where the time is.  Next to it the host route to the same bits on this box's CPU, once per shape by the host clock:
the read-back of the volume, scipy's distance transform and the numpy statement of the parts (tests/parts_reference.py); and whether
the device's bits equal them.
Usage: python tools/time_volume_parts.py [--calls 100] [--out profiles/volume_parts.json]"""
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
import parts_reference as PR                                                 # noqa: E402
from graspnerf_amd import _lib                                               # noqa: E402
from graspnerf_amd.distance import VolumeDistance                            # noqa: E402
from graspnerf_amd.objects import VolumeObjects                              # noqa: E402
from graspnerf_amd.parts import PART_DEFAULTS, VolumeParts                   # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402

SHAPES = (('B1_R40', 1, 40), ('B32_R40', 32, 40), ('B1_R128', 1, 128))
MAX_ROWS = 1024


def heap(R, seed):
    """[R,R,R] float32: a slab (solid below a tenth of the height), a heap of six balls on it -- a ring of five, each touching or
    overlapping the next, and one on top --, eight floaters of one to eight voxels; values clipped to [-1, 1] like a tsdf.
    -> (vol, the first layer above the slab)."""
    rng = np.random.default_rng(seed)
    i = np.arange(R, dtype=np.float64)
    I, J, K = np.meshgrid(i, i, i, indexing='ij')
    top = R // 10
    d = K - (top - 0.5)
    r = R * 0.11
    ring = r / np.sin(np.pi / 5) * rng.uniform(0.88, 1.0)                      # neighbours 1.76 r to 2 r apart
    phase = rng.uniform(0, 2 * np.pi)
    centres = [(R / 2 + ring * np.cos(phase + q * 2 * np.pi / 5), R / 2 + ring * np.sin(phase + q * 2 * np.pi / 5), top + 0.9 * r) for q in range(5)]
    centres.append((R / 2, R / 2, top + 0.9 * r + 1.2 * r))
    for c in centres:
        d = np.minimum(d, np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2) - r * rng.uniform(0.95, 1.05))
    vol = np.clip(d / 4.0, -1.0, 1.0).astype(np.float32)
    for _ in range(8):
        p = rng.integers(1, R - 3, 3)
        p[2] = max(p[2], int(R * 0.7))
        e = rng.integers(1, 3, 3)
        vol[p[0]:p[0] + e[0], p[1]:p[1] + e[1], p[2]:p[2] + e[2]] = -0.5
    return vol, top


def measure(B, R, calls, dev):
    scale = 0.3 / R                                                            # the same 0.3 m box at every R
    scenes = [heap(R, 10 * B + b) for b in range(B)]
    host_vol, z_min = np.stack([s[0] for s in scenes]), scenes[0][1]
    params = dict(PART_DEFAULTS, max_parts=MAX_ROWS)
    vol = torch.from_numpy(host_vol).to(dev)
    vd, vp, vo = VolumeDistance(dev), VolumeParts(dev), VolumeObjects(dev)
    height = vd(vol, scale=scale, z_min=z_min)['d2_free']
    alone = lambda: vp(height, **params)
    chain = lambda: vp(vd(vol, scale=scale, z_min=z_min)['d2_free'], **params)
    distance = lambda: vd(vol, scale=scale, z_min=z_min)
    components = lambda: vo(vol, z_min=z_min, connectivity=26, max_objects=MAX_ROWS)
    rec = {'B': B, 'R': R, 'z_min': z_min, 'parameters': params,
           'device_ms': {'volume_parts': pct(event_ms(alone, calls)), 'volume_distance': pct(event_ms(distance, calls)),
                         'volume_distance_then_parts': pct(event_ms(chain, calls)), 'volume_objects': pct(event_ms(components, calls))}}
    # every launch of the call between its own events, in a pass of its own (the brackets cost a few microseconds each)
    _lib.timing_begin('@gnr_volume_parts_fwd')
    for _ in range(calls):
        alone()
    rec['launch_ms_mean'] = {k.split('@')[0]: round(ms / n, 5) for k, (n, ms) in sorted(_lib.timing_end().items())}
    got = {k: v.cpu().numpy() for k, v in alone().items() if torch.is_tensor(v)}
    got_objects = int(components()['count'].max().item())
    rec['parts_per_scene'] = [int(got['count'].min()), int(got['count'].max())]
    rec['basins_per_scene'] = [int(got['basins'].min()), int(got['basins'].max())]
    rec['components_per_scene_max'] = got_objects
    rec['status_word'] = int(got['status'][0])
    # the host route to the same bits, once each by the host clock
    t0 = time.perf_counter()
    back = vol.cpu().numpy()
    t1 = time.perf_counter()
    host_height = PR.d2_free(back, z_min=z_min)
    t2 = time.perf_counter()
    want = PR.parts(host_height, **params)
    t3 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    rec['host_ms'] = {'read_back': ms(t0, t1), 'distance_transform_edt': ms(t1, t2), 'numpy_parts': ms(t2, t3), 'total': ms(t0, t3),
                      'what': 'once each, host clock, this box\'s CPU'}
    rec['equals_host_route'] = bool(np.array_equal(height.cpu().numpy(), host_height) and all(np.array_equal(got[k], want[k]) for k in PR.KEYS))
    rec['parts_p50_over_objects_p50'] = round(rec['device_ms']['volume_parts']['p50'] / rec['device_ms']['volume_objects']['p50'], 3)
    rec['device_chain_p50_over_host_total'] = round(rec['device_ms']['volume_distance_then_parts']['p50'] / rec['host_ms']['total'], 5)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_parts.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_volume_parts.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls (three warm-up calls); launch_ms_mean: mean per launch, bracketed pass',
           'calls': a.calls,
           'volume': 'a slab, a heap of six balls that touch or overlap, eight floaters (tools/time_volume_parts.py); solid: v < 0, z_min cuts the slab',
           'device': torch.cuda.get_device_name(0), 'cpus_of_the_host_route': len(os.sched_getaffinity(0))}
    for name, B, R in SHAPES:
        res[name] = measure(B, R, a.calls, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
