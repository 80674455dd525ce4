"""Cost of the distance field of the volume (gnr_volume_distance_fwd, distance.VolumeDistance) at three shapes -- B = 1 at 40^3, B = 32
at 40^3, B = 1 at 128^3 -- on tools/time_volume_objects.py's scene (a slab, four balls standing on it, eight floaters): p10 / p50 / p90
of single calls between HIP events, unsigned (the transform to the solid voxels alone), signed (both transforms and esdf), and signed
with HandClearance on esdf behind it on 2 048 rows.  Next to it the host route to the same integers on this box's CPU, once per shape by
the host clock: the read-back of the volume, scipy.ndimage.distance_transform_edt(return_indices=True) twice per scene and the float64
formula of esdf (tests/distance_reference.py); and whether the device's d2 and esdf equal them and its nearest sites are valid.
Usage: python tools/time_volume_distance.py [--calls 100] [--out profiles/volume_distance.json]"""
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
import distance_reference as DR                                              # noqa: E402
from graspnerf_amd.distance import VolumeDistance                            # noqa: E402
from graspnerf_amd.hand import HandClearance                                 # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402
from time_volume_objects import table                                        # noqa: E402

SHAPES = (('B1_R40', 1, 40), ('B32_R40', 32, 40), ('B1_R128', 1, 128))
HAND_ROWS = 2048                                                               # per call, spread over the scenes


def measure(B, R, calls, dev):
    scale = 0.3 / R                                                            # the same 0.3 m box at every R
    host_vol = np.stack([table(R, 10 * B + b)[0] for b in range(B)])
    rows = HAND_ROWS // B
    rng = np.random.default_rng(B + R)
    pos = rng.uniform(0.0, R - 1.0, (B, rows, 3))
    quat = rng.normal(size=(B, rows, 4)).astype(np.float32)
    width = (rng.uniform(1.33, 9.33, (B, rows)) * R / 40).astype(np.float32)
    vol = torch.from_numpy(host_vol).to(dev)
    P, Q, W = (torch.from_numpy(x).to(dev) for x in (pos, quat, width))
    count = torch.full((B,), rows, dtype=torch.int32, device=dev)
    vd, hc = VolumeDistance(dev), HandClearance(dev)
    unsigned = lambda: vd(vol, scale=scale, signed=False)
    signed = lambda: vd(vol, scale=scale)
    with_hand = lambda: hc(signed()['esdf'], P, Q, W, count, scale=scale)
    rec = {'B': B, 'R': R, 'hand_rows_per_scene': rows,
           'device_ms': {'unsigned': pct(event_ms(unsigned, calls)), 'signed': pct(event_ms(signed, calls)),
                         'signed_with_hand_clearance': pct(event_ms(with_hand, calls))}}
    got = {k: v.cpu().numpy() for k, v in signed().items()}
    # the host route to the same integers, once by the host clock
    t0 = time.perf_counter()
    back = vol.cpu().numpy()
    t1 = time.perf_counter()
    masks = [DR.solid(v) for v in back]
    both = [(DR.edt(s), DR.edt(~s)) for s in masks]
    t2 = time.perf_counter()
    field = [DR.esdf(s, ds, df, scale) for s, ((ds, _), (df, _)) in zip(masks, both)]
    t3 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    rec['host_ms'] = {'read_back': ms(t0, t1), 'distance_transform_edt_twice': ms(t1, t2), 'esdf_formula': ms(t2, t3), 'total': ms(t0, t3),
                      'what': 'once each, host clock, this box\'s CPU'}
    same = all(np.array_equal(got['d2_solid'][b], ds) and np.array_equal(got['d2_free'][b], df) and np.array_equal(got['esdf'][b], field[b])
               for b, ((ds, _), (df, _)) in enumerate(both))
    valid = not any(DR.invalid_nearest(s, got['d2_solid'][b], got['nearest_solid'][b]).any() or
                    DR.invalid_nearest(~s, got['d2_free'][b], got['nearest_free'][b]).any() for b, s in enumerate(masks))
    rec['equals_host_route'] = bool(same and valid)
    rec['largest_distance_m'] = round(float(np.sqrt(got['d2_solid'].max()) * scale), 4)
    rec['device_signed_p50_over_host_total'] = round(rec['device_ms']['signed']['p50'] / rec['host_ms']['total'], 5)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_distance.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_volume_distance.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls (three warm-up calls)', 'calls': a.calls,
           'volume': 'a slab, four balls standing on it, eight floaters (tools/time_volume_objects.py); solid: v < 0, no z_min',
           'device': torch.cuda.get_device_name(0), 'cpus_of_the_host_route': len(os.sched_getaffinity(0))}
    for name, B, R in SHAPES:
        res[name] = measure(B, R, a.calls, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
