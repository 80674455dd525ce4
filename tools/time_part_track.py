"""Cost of the parts across two plans (gnr_part_overlap_fwd, gnr_part_track_fwd; track.PartOverlap, track.PartTrack) at three shapes --
B = 1 at 40^3, B = 32 at 40^3, B = 1 at 128^3 -- on the labels of two plans of the pile of tools/time_grasp_retreat.py scaled to the
lattice: three touching balls on the floor and a fourth in their hollow, then the same with the fourth taken and the first shifted by
a voxel; the 256 rows PartTrack.of_parts takes from the parts' default max_parts.  p10 / p50 / p90 of single calls between HIP events
of the two calls and of both; the mean of every launch of the two calls, and of PartContacts' launches at connectivity 26 on the first
plan's labels in the same run as the yardstick (k_overlap reads two volumes and no neighbours; k_contacts one volume and 13
neighbours), from the library's own timing brackets.  Next to it the host route to the same bits on this box's CPU by the host clock:
the read-back of the two label volumes and the numpy statement (tests/track_reference.py) of scene 0, once, and whether the device's
bits equal it on everything compared.
Usage: python tools/time_part_track.py [--calls 100] [--out profiles/part_track.json]"""
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
import track_reference as TR                                                 # noqa: E402
from graspnerf_amd.distance import VolumeDistance                            # noqa: E402
from graspnerf_amd.parts import PART_DEFAULTS, VolumeParts                   # noqa: E402
from graspnerf_amd.support import PartContacts                               # noqa: E402
from graspnerf_amd.track import TRACK_COLUMNS, TRACK_DEFAULTS, PartOverlap, PartTrack  # noqa: E402
from time_grasp_retreat import CENTRES                                       # noqa: E402
from time_part_support import launches                                       # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402

SHAPES = (('B1_R40', 1, 40), ('B32_R40', 32, 40), ('B1_R128', 1, 128))
ROWS = 256


def plans(R, seed):
    """Two [R,R,R] float32 volumes (-1 inside a ball, 1 elsewhere): the pile at R / 40 of its size, moved by up to a voxel per scene;
    then the same with the fourth ball taken and the first shifted by one voxel along i."""
    rng = np.random.default_rng(seed)
    s = R / 40.0
    i = np.arange(R, dtype=np.float64)
    I, J, K = np.meshgrid(i, i, i, indexing='ij')
    shift = rng.uniform(-1.0, 1.0, 2) if seed else np.zeros(2)
    ball = lambda ci, cj, ck, r, di=0.0: (I - (ci * s + shift[0] + di)) ** 2 + (J - (cj * s + shift[1])) ** 2 + (K - ck * s) ** 2 <= (r * s) ** 2
    first = np.logical_or.reduce([ball(*c) for c in CENTRES])
    second = np.logical_or.reduce([ball(*c, di=1.0 if n == 0 else 0.0) for n, c in enumerate(CENTRES[:3])])
    return tuple(np.where(m, -1.0, 1.0).astype(np.float32) for m in (first, second))


def measure(B, R, calls, dev):
    scale = 0.3 / R
    pairs = [plans(R, b) for b in range(B)]
    vd = VolumeDistance(dev)
    results = []
    for k in (0, 1):                                                          # two VolumeParts objects: their outputs live side by side
        vol = torch.from_numpy(np.stack([p[k] for p in pairs])).to(dev)
        results.append(VolumeParts(dev)(vd(vol, scale=scale)['d2_free'], **PART_DEFAULTS))
    rb, ra = results
    po, pt, pc = PartOverlap(dev), PartTrack(dev), PartContacts(dev)
    overlap = lambda: po(rb['labels'], ra['labels'], max_parts=ROWS)
    table = overlap()
    fates = lambda: pt(table, rb['count'], ra['count'], **TRACK_DEFAULTS)
    both = lambda: pt(overlap(), rb['count'], ra['count'], **TRACK_DEFAULTS)
    contacts = lambda: pc(rb['labels'], max_parts=ROWS, connectivity=26, z_min=0)
    rec = {'B': B, 'R': R, 'rows': ROWS, 'parameters': dict(TRACK_DEFAULTS),
           'parts_per_scene': {'before': [int(rb['count'].min().item()), int(rb['count'].max().item())],
                               'after': [int(ra['count'].min().item()), int(ra['count'].max().item())]},
           'device_ms': {'part_overlap': pct(event_ms(overlap, calls)), 'part_track': pct(event_ms(fates, calls)),
                         'overlap_and_track': pct(event_ms(both, calls)), 'part_contacts_26': pct(event_ms(contacts, calls))},
           'launch_ms_mean': {**launches(both, calls, 'gnr_part_'), **launches(contacts, calls, 'gnr_part_contacts_fwd')}}
    got = both()
    torch.cuda.synchronize()
    # the host route to the same bits: scene 0, once, by the host clock
    t0 = time.perf_counter()
    lb, la = rb['labels'][0].cpu().numpy(), ra['labels'][0].cpu().numpy()
    nb, na = int(rb['count'][0].item()), int(ra['count'][0].item())
    t1 = time.perf_counter()
    tab, beyond = TR.overlap(lb, la, ROWS)
    t2 = time.perf_counter()
    want = TR.track(tab, nb, na, **TRACK_DEFAULTS)
    t3 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    rec['host_ms'] = {'read_back': ms(t0, t1), 'numpy_overlap': ms(t1, t2), 'numpy_track': ms(t2, t3), 'what': 'once, host clock, this box\'s CPU; scene 0'}
    want.update(table=tab, beyond=beyond)
    rec['equals_host_route'] = bool(all(np.array_equal(got[k][0].cpu().numpy(), want[k]) for k in (*TRACK_COLUMNS, 'summary', 'table', 'beyond')))
    rec['scene_0'] = {'summary': dict(zip(TR.SUMMARY, want['summary'].tolist())), 'heir': want['heir'][:nb].tolist(), 'fate': want['fate'][:nb].tolist(),
                      'shared': want['shared'][:nb].tolist(), 'size_before': want['size_before'][:nb].tolist()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'part_track.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_part_track.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls (three warm-up calls); launch_ms_mean: mean ms per launch '
                   'from the library\'s timing brackets', 'calls': a.calls,
           'scene': 'two plans of the pile of tools/time_grasp_retreat.py scaled to the lattice: four balls, then the fourth taken and the first shifted by a voxel',
           'device': torch.cuda.get_device_name(0), 'cpus_of_the_host_route': len(os.sched_getaffinity(0))}
    for name, B, R in SHAPES:
        res[name] = measure(B, R, a.calls, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
