"""Cost of the balance of the parts (gnr_part_feet_fwd, gnr_part_balance_fwd; balance.PartFeet, balance.PartBalance) at three shapes
-- B = 1 at 40^3, B = 32 at 40^3, B = 1 at 128^3 -- on the pile of tools/time_grasp_retreat.py scaled to the lattice (three touching
balls on the floor, a fourth resting in their hollow), with the 256 rows PartSupport.of_parts takes from the parts' default max_parts:
p10 / p50 / p90 of single calls between HIP events of the two calls, of both, and of the chain from the volume (VolumeDistance,
VolumeParts, PartContacts, PartSupport with the relation, PartFeet, PartBalance); PartContacts alone in the same run for comparison
(k_feet reads what k_contacts reads); the mean of every launch of the four calls from the library's own timing brackets.  Next to it
the host route to the same bits on this box's CPU by the host clock: the read-back of the labels and the relation and the numpy
statement (tests/balance_reference.py) of scene 0, once, and whether the device's bits equal it on everything compared.
Usage: python tools/time_part_balance.py [--calls 100] [--out profiles/part_balance.json]"""
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
import balance_reference as BR                                               # noqa: E402
from graspnerf_amd.balance import BALANCE_COLUMNS, FEET_TABLES, PartBalance, PartFeet  # noqa: E402
from graspnerf_amd.distance import VolumeDistance                            # noqa: E402
from graspnerf_amd.parts import PART_DEFAULTS, VolumeParts                   # noqa: E402
from graspnerf_amd.support import SUPPORT_DEFAULTS, PartContacts, PartSupport  # noqa: E402
from time_grasp_retreat import pile                                          # noqa: E402
from time_part_support import launches                                       # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402

SHAPES = (('B1_R40', 1, 40), ('B32_R40', 32, 40), ('B1_R128', 1, 128))
ROWS = 256


def measure(B, R, calls, dev):
    scale = 0.3 / R
    conn = PART_DEFAULTS['connectivity']
    vol = torch.from_numpy(np.stack([pile(R, b) for b in range(B)])).to(dev)
    vd, vp, pc, ps, pf, pb = VolumeDistance(dev), VolumeParts(dev), PartContacts(dev), PartSupport(dev), PartFeet(dev), PartBalance(dev)
    res = vp(vd(vol, scale=scale)['d2_free'], **PART_DEFAULTS)
    contacts = lambda: pc(res['labels'], max_parts=ROWS, connectivity=conn, z_min=0)
    sres = ps(contacts(), res['count'], relation=True, **SUPPORT_DEFAULTS)
    feet = lambda: pf(res['labels'], sres['rests_on'], sres['count'], connectivity=conn, z_min=0)
    fres = feet()
    bal = lambda: pb(fres, min_floor=SUPPORT_DEFAULTS['min_floor'], tips=True)
    both = lambda: pb(feet(), min_floor=SUPPORT_DEFAULTS['min_floor'], tips=True)

    def chain():
        r = vp(vd(vol, scale=scale)['d2_free'], **PART_DEFAULTS)
        s = ps(pc(r['labels'], max_parts=ROWS, connectivity=conn, z_min=0), r['count'], relation=True, **SUPPORT_DEFAULTS)
        return pb(pf(r['labels'], s['rests_on'], s['count'], connectivity=conn, z_min=0), min_floor=SUPPORT_DEFAULTS['min_floor'], tips=True)

    rec = {'B': B, 'R': R, 'rows': ROWS, 'parameters': dict(min_floor=SUPPORT_DEFAULTS['min_floor'], connectivity=conn, z_min=0),
           'parts_per_scene': [int(res['count'].min().item()), int(res['count'].max().item())],
           'device_ms': {'part_feet': pct(event_ms(feet, calls)), 'part_balance': pct(event_ms(bal, calls)), 'feet_and_balance': pct(event_ms(both, calls)),
                         'part_contacts': pct(event_ms(contacts, calls)), 'chain_from_the_volume': pct(event_ms(chain, calls))},
           'launch_ms_mean': launches(lambda: (contacts(), both()), calls, 'gnr_part_')}
    got = both()
    torch.cuda.synchronize()
    # the host route to the same bits: scene 0, once, by the host clock
    t0 = time.perf_counter()
    lab, rel, n = res['labels'][0].cpu().numpy(), sres['rests_on'][0].cpu().numpy(), int(res['count'][0].item())
    t1 = time.perf_counter()
    slots, crowded = BR.slots(rel, n)
    moments, feet_rows, reach = BR.feet(lab, slots, conn, 0)
    t2 = time.perf_counter()
    want = BR.balance(moments, feet_rows, reach, slots, rel, n, SUPPORT_DEFAULTS['min_floor'])
    t3 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    rec['host_ms'] = {'read_back': ms(t0, t1), 'numpy_feet': ms(t1, t2), 'numpy_balance': ms(t2, t3), 'what': 'once, host clock, this box\'s CPU; scene 0'}
    want.update(moments=moments, slots=slots, feet=feet_rows, reach=reach, crowded=crowded)
    same = lambda k: np.array_equal(got[k][0].cpu().numpy().view(np.int64) if k == 'margin' else got[k][0].cpu().numpy(), want[k].view(np.int64) if k == 'margin' else want[k])
    rec['equals_host_route'] = bool(all(same(k) for k in (*BALANCE_COLUMNS, 'tips', 'slots', *FEET_TABLES)))
    rec['scene_0'] = {'margin': [round(float(x), 4) for x in want['margin'][:n]], 'balanced': want['balanced'][:n].tolist(), 'falls': want['falls'][:n].tolist(),
                      'unsettles': want['unsettles'][:n].tolist(), 'feet': want['feet'][:n].tolist()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'part_balance.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_part_balance.py measures on a ROCm GPU; there is nothing to time without one')
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
