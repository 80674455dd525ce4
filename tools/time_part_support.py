"""Cost of the support of the parts (gnr_part_contacts_fwd, gnr_part_support_fwd; support.PartContacts, support.PartSupport) at three
shapes -- B = 1 at 40^3, B = 32 at 40^3, B = 1 at 128^3 -- on the pile of tools/time_grasp_retreat.py scaled to the lattice (three
touching balls on the floor, a fourth resting in their hollow), with the 256 rows PartSupport.of_parts takes from the parts' default
max_parts: p10 / p50 / p90 of single calls between HIP events of the two calls and of both; the mean of every launch of the two
calls, and of VolumeParts' launches on the same volume for comparison (k_contacts reads what k_up reads), from the library's own
timing brackets.  Next to it the host route to the same bits on this box's CPU by the host clock: the read-back of the labels and the
numpy statement (tests/support_reference.py) of scene 0, once, and whether the device's bits equal it on everything compared.
Usage: python tools/time_part_support.py [--calls 100] [--out profiles/part_support.json]"""
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
import support_reference as SR                                               # noqa: E402
from graspnerf_amd import _lib                                               # noqa: E402
from graspnerf_amd.distance import VolumeDistance                            # noqa: E402
from graspnerf_amd.parts import PART_DEFAULTS, VolumeParts                   # noqa: E402
from graspnerf_amd.support import SUPPORT_COLUMNS, SUPPORT_DEFAULTS, PartContacts, PartSupport  # noqa: E402
from time_grasp_retreat import pile                                          # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402

SHAPES = (('B1_R40', 1, 40), ('B32_R40', 32, 40), ('B1_R128', 1, 128))
ROWS = 256


def launches(f, calls, only):
    """{label: mean ms per launch} of the library's launches whose label contains `only`, over `calls` calls of f."""
    f()
    torch.cuda.synchronize()
    _lib.timing_begin(only)
    for _ in range(calls):
        f()
    return {k: round(ms / max(cnt, 1), 5) for k, (cnt, ms) in _lib.timing_end().items()}


def measure(B, R, calls, dev):
    scale = 0.3 / R
    vol = torch.from_numpy(np.stack([pile(R, b) for b in range(B)])).to(dev)
    vd, vp, pc, ps = VolumeDistance(dev), VolumeParts(dev), PartContacts(dev), PartSupport(dev)
    height = vd(vol, scale=scale)['d2_free']
    res = vp(height, **PART_DEFAULTS)
    con = pc(res['labels'], max_parts=ROWS, connectivity=PART_DEFAULTS['connectivity'], z_min=0)
    contacts = lambda: pc(res['labels'], max_parts=ROWS, connectivity=PART_DEFAULTS['connectivity'], z_min=0)
    graph = lambda: ps(con, res['count'], relation=True, **SUPPORT_DEFAULTS)
    both = lambda: ps(contacts(), res['count'], relation=True, **SUPPORT_DEFAULTS)
    rec = {'B': B, 'R': R, 'rows': ROWS, 'parameters': dict(SUPPORT_DEFAULTS, connectivity=PART_DEFAULTS['connectivity'], z_min=0),
           'parts_per_scene': [int(res['count'].min().item()), int(res['count'].max().item())],
           'device_ms': {'part_contacts': pct(event_ms(contacts, calls)), 'part_support': pct(event_ms(graph, calls)),
                         'contacts_and_support': pct(event_ms(both, calls)),
                         'volume_parts': pct(event_ms(lambda: vp(height, **PART_DEFAULTS), calls))},
           'launch_ms_mean': {**launches(both, calls, 'gnr_part_'), **launches(lambda: vp(height, **PART_DEFAULTS), calls, 'gnr_volume_parts_fwd')}}
    got = both()
    torch.cuda.synchronize()
    # the host route to the same bits: scene 0, once, by the host clock
    t0 = time.perf_counter()
    lab, n = res['labels'][0].cpu().numpy(), int(res['count'][0].item())
    t1 = time.perf_counter()
    pairs, floor, dropped = SR.contacts(lab, ROWS, PART_DEFAULTS['connectivity'], 0)
    t2 = time.perf_counter()
    want = SR.support(pairs, floor, n, **SUPPORT_DEFAULTS)
    t3 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    rec['host_ms'] = {'read_back': ms(t0, t1), 'numpy_contacts': ms(t1, t2), 'numpy_support': ms(t2, t3),
                      'what': 'once, host clock, this box\'s CPU; scene 0'}
    want.update(pairs=pairs, floor=floor, dropped=dropped)
    rec['equals_host_route'] = bool(all(np.array_equal(got[k][0].cpu().numpy(), want[k]) for k in (*SUPPORT_COLUMNS, 'rests_on', 'pairs', 'floor', 'dropped')))
    rec['scene_0'] = {'rests_on_pairs': int(want['rests_on'].sum()), 'layer': want['layer'][:n].tolist(), 'touching_pairs': int((pairs[..., 0] > 0).sum()) // 2}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'part_support.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_part_support.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls (three warm-up calls); launch_ms_mean: mean ms per launch '
                   'from the library\'s timing brackets', 'calls': a.calls,
           'scene': 'three touching balls on the floor and a fourth in their hollow, scaled to the lattice (tools/time_grasp_retreat.py)',
           'device': torch.cuda.get_device_name(0), 'cpus_of_the_host_route': len(os.sched_getaffinity(0))}
    for name, B, R in SHAPES:
        res[name] = measure(B, R, a.calls, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
