"""Cost of the objects of the volume (gnr_volume_objects_fwd, objects.VolumeObjects) and of which object each grasp closes on
(gnr_grasp_objects_fwd, objects.GraspObjects) at three shapes -- B = 1 at 40^3 with the 2 048-row buffer of a default session, B = 32 at
40^3, B = 1 at 128^3 -- on a slab with objects standing on it and a few floaters: p10 / p50 / p90 of single calls between HIP events.
Next to it the host route to the same bits on this box's CPU: the read-back of the volume, scipy.ndimage.label, the numpy statistics
and `cleaned` (tests/objects_reference.py), and the float64 statement of the grasps' votes on the same rows, each once by the host
clock; and whether the device's bits equal them.
Usage: python tools/time_volume_objects.py [--calls 100] [--out profiles/volume_objects.json]"""
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
import objects_reference as OR                                               # noqa: E402
from graspnerf_amd.objects import GRASP_OBJECT_ROWS, GraspObjects, VolumeObjects   # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402

KEYS = ('labels', 'count', 'voxels', 'bbox', 'sums', 'cleaned')
SHAPES = (('B1_R40_rows2048', 1, 40, 2048), ('B32_R40_rows256', 32, 40, 256), ('B1_R128_rows2048', 1, 128, 2048))


def table(R, seed):
    """[R,R,R] float32: a slab (solid below a tenth of the height), four balls standing on it, eight floaters of one to eight voxels;
    values clipped to [-1, 1] like a tsdf.  -> (vol, the first layer above the slab)."""
    rng = np.random.default_rng(seed)
    i = np.arange(R, dtype=np.float64)
    I, J, K = np.meshgrid(i, i, i, indexing='ij')
    top = R // 10
    d = K - (top - 0.5)
    for q in range(4):
        r = R * rng.uniform(0.08, 0.14)
        c = (R * (0.25 + 0.5 * (q // 2)) + rng.uniform(-2, 2), R * (0.25 + 0.5 * (q % 2)) + rng.uniform(-2, 2), top + 0.8 * r)
        d = np.minimum(d, np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2) - r)
    vol = np.clip(d / 4.0, -1.0, 1.0).astype(np.float32)
    for _ in range(8):
        p = rng.integers(1, R - 3, 3)
        p[2] = max(p[2], R // 2)
        e = rng.integers(1, 3, 3)
        vol[p[0]:p[0] + e[0], p[1]:p[1] + e[1], p[2]:p[2] + e[2]] = -0.5
    return vol, top


def measure(name, B, R, rows, calls, dev):
    scale = 0.3 / R                                                            # the same 0.3 m box at every R
    scenes = [table(R, 10 * B + b) for b in range(B)]
    host_vol, z_min = np.stack([s[0] for s in scenes]), scenes[0][1]
    params = dict(z_min=z_min, connectivity=6, max_objects=1024, min_voxels=9)
    rng = np.random.default_rng(B + R)
    pos = rng.uniform(0.0, R - 1.0, (B, rows, 3))
    quat = rng.normal(size=(B, rows, 4)).astype(np.float32)
    width = (rng.uniform(1.33, 9.33, (B, rows)) * R / 40).astype(np.float32)
    vol = torch.from_numpy(host_vol).to(dev)
    P, Q, W = (torch.from_numpy(x).to(dev) for x in (pos, quat, width))
    count = torch.full((B,), rows, dtype=torch.int32, device=dev)
    vo, go = VolumeObjects(dev), GraspObjects(dev)
    objects = lambda: vo(vol, cleaned=True, **params)
    res = objects()
    grasps = lambda: go(res['labels'], P, Q, W, count, scale=scale)
    both = lambda: (objects(), grasps())
    rec = {'B': B, 'R': R, 'grasp_rows_per_scene': rows, 'parameters': params,
           'device_ms': {'volume_objects': pct(event_ms(objects, calls)), 'grasp_objects': pct(event_ms(grasps, calls)), 'both': pct(event_ms(both, calls))}}
    got = {k: v.cpu().numpy() for k, v in objects().items() if torch.is_tensor(v)}
    got_rows = {k: v.cpu().numpy() for k, v in grasps().items()}
    rec['objects_per_scene'] = [int(got['count'].min()), int(got['count'].max())]
    rec['status_word'] = int(got['status'][0])
    # the host route to the same bits, once each by the host clock
    t0 = time.perf_counter()
    back = vol.cpu().numpy()
    t1 = time.perf_counter()
    labelled = [OR.label(v, z_min=z_min) for v in back]
    t2 = time.perf_counter()
    stats = [OR.statistics(lab, n, params['max_objects']) + (OR.cleaned(v, lab, n, params['min_voxels']),) for v, (lab, n) in zip(back, labelled)]
    t3 = time.perf_counter()
    want_rows = [OR.grasp_objects(lab, pos[b], quat[b], width[b], rows, scale) for b, (lab, _) in enumerate(labelled)]
    t4 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    rec['host_ms'] = {'read_back': ms(t0, t1), 'ndimage_label': ms(t1, t2), 'numpy_statistics_and_cleaned': ms(t2, t3),
                      'volume_objects_total': ms(t0, t3), 'grasp_objects_statement': ms(t3, t4), 'what': 'once each, host clock, this box\'s CPU'}
    want = {'labels': np.stack([l for l, _ in labelled]), 'count': np.int32([n for _, n in labelled]),
            **{k: np.stack([s[i] for s in stats]) for i, k in enumerate(('voxels', 'bbox', 'sums', 'cleaned'))}}
    rec['equals_host_route'] = bool(all(np.array_equal(got[k], want[k]) for k in KEYS) and
                                    all(np.array_equal(got_rows[k][b], want_rows[b][i]) for b in range(B) for i, k in enumerate(GRASP_OBJECT_ROWS)))
    rec['device_p50_over_host_volume_objects'] = round(rec['device_ms']['volume_objects']['p50'] / rec['host_ms']['volume_objects_total'], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_objects.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_volume_objects.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls (three warm-up calls)', 'calls': a.calls,
           'volume': 'a slab, four balls standing on it, eight floaters; z_min cuts the slab (tools/time_volume_objects.py)',
           'device': torch.cuda.get_device_name(0), 'cpus_of_the_host_route': len(os.sched_getaffinity(0))}
    for name, B, R, rows in SHAPES:
        res[name] = measure(name, B, R, rows, a.calls, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
