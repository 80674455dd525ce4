"""Cost of the retreat of the ranked grasps (gnr_grasp_retreat_fwd, retreat.GraspRetreat) at three shapes -- B = 1 at 40^3, B = 32 at
40^3, B = 1 at 128^3, 2 048 rows of grasps per scene -- on the pile of tests/test_grasp_retreat.py scaled to the lattice (three touching
balls on the floor, a fourth resting in their hollow; the same 0.3 m box at every R): p10 / p50 / p90 of single calls between HIP
events, of GraspRetreat alone on labels and held parts computed before, and of the chain from the volume (VolumeDistance, VolumeParts,
GraspObjects, GraspRetreat).  Next to it the host route to the same bits on this box's CPU by the host clock: the read-back of labels,
boxes, held parts and quaternions, and the numpy statement (tests/retreat_reference.py) over the first `host_rows` rows of scene 0 --
all 2 048 at 40^3, fewer where a row moves tens of thousands of voxels --, and whether the device's bits equal them.
Usage: python tools/time_grasp_retreat.py [--calls 100] [--out profiles/grasp_retreat.json]"""
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
import retreat_reference as RR                                               # noqa: E402
from graspnerf_amd.distance import VolumeDistance                            # noqa: E402
from graspnerf_amd.objects import GraspObjects                               # noqa: E402
from graspnerf_amd.parts import PART_DEFAULTS, VolumeParts                   # noqa: E402
from graspnerf_amd.retreat import RETREAT_DEFAULTS, RETREAT_ROWS, GraspRetreat  # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402

SHAPES = (('B1_R40', 1, 40, 2048), ('B32_R40', 32, 40, 64), ('B1_R128', 1, 128, 16))       # name, B, R, rows of the host route
ROWS, MAX_PARTS = 2048, 64
CENTRES = ((13.0, 14.0, 7.0, 7.0), (27.0, 14.0, 7.0, 7.0), (20.0, 26.0, 7.0, 7.0), (20.0, 18.0, 17.0, 6.0))     # i, j, k, radius at 40^3


def pile(R, seed):
    """[R,R,R] float32: the pile at R / 40 of its size, moved by up to a voxel per scene; -1 inside a ball, 1 elsewhere."""
    rng = np.random.default_rng(seed)
    s = R / 40.0
    i = np.arange(R, dtype=np.float64)
    I, J, K = np.meshgrid(i, i, i, indexing='ij')
    shift = rng.uniform(-1.0, 1.0, 2) if seed else np.zeros(2)
    solid = np.zeros((R, R, R), bool)
    for ci, cj, ck, r in CENTRES:
        solid |= (I - (ci * s + shift[0])) ** 2 + (J - (cj * s + shift[1])) ** 2 + (K - ck * s) ** 2 <= (r * s) ** 2
    return np.where(solid, -1.0, 1.0).astype(np.float32)


def grasps(R, seed):
    """ROWS grasps of one scene: positions within a ball's radius of a ball's centre, the hand's z within 40 degrees of straight down
    for three quarters of them and anywhere for the rest (side grasps among them), widths of 6 to 12 voxels at 40^3."""
    rng = np.random.default_rng(1000 + seed)
    s = R / 40.0
    c = np.asarray(CENTRES)[rng.integers(0, 4, ROWS)]
    pos = (c[:, :3] + rng.uniform(-0.6, 0.6, (ROWS, 3)) * c[:, 3:]) * s
    tilt = np.where(rng.random(ROWS) < 0.75, rng.uniform(0, np.radians(40), ROWS), rng.uniform(0, np.pi, ROWS))
    turn = rng.uniform(0, 2 * np.pi, ROWS)
    a = (np.pi - tilt) / 2                                                     # straight down is the half turn about x
    axis = np.stack([np.cos(turn), np.sin(turn), np.zeros(ROWS)], 1)
    quat = np.concatenate([axis * np.sin(a)[:, None], np.cos(a)[:, None]], 1).astype(np.float32)
    return pos, quat, (rng.uniform(6.0, 12.0, ROWS) * s).astype(np.float32)


def measure(B, R, host_rows, calls, dev):
    scale = 0.3 / R
    vol = torch.from_numpy(np.stack([pile(R, b) for b in range(B)])).to(dev)
    rows = [grasps(R, b) for b in range(B)]
    pos, quat, width = (torch.from_numpy(np.stack([r[k] for r in rows])).to(dev) for k in range(3))
    count = torch.full((B,), ROWS, dtype=torch.int32, device=dev)
    vd, vp, go, gr = VolumeDistance(dev), VolumeParts(dev), GraspObjects(dev), GraspRetreat(dev)
    part_kw = dict(PART_DEFAULTS, max_parts=MAX_PARTS)

    def chain():
        res = vp(vd(vol, scale=scale)['d2_free'], **part_kw)
        gres = go(res['labels'], pos, quat, width, count, scale=scale)
        return res, gres, gr(res['labels'], res['bbox'], gres['object'], quat, count, scale=scale)

    res, gres, rres = chain()
    alone = lambda: gr(res['labels'], res['bbox'], gres['object'], quat, count, scale=scale)
    T, K, sl = RR.steps(scale=scale, **{k: RETREAT_DEFAULTS[k] for k in ('retreat', 'step')})
    rec = {'B': B, 'R': R, 'rows_per_scene': ROWS, 'scale': scale, 'steps': K, 'parameters': RETREAT_DEFAULTS,
           'device_ms': {'grasp_retreat': pct(event_ms(alone, calls)), 'volume_to_retreat': pct(event_ms(chain, calls)),
                         'grasp_objects': pct(event_ms(lambda: go(res['labels'], pos, quat, width, count, scale=scale), calls))}}
    got = {k: v.cpu().numpy() for k, v in alone().items()}
    held = gres['object'].cpu().numpy()
    rec['parts_per_scene'] = [int(res['count'].min().item()), int(res['count'].max().item())]
    rec['rows'] = {'holding_a_part': int((held > 0).sum()), 'free': int(((got['blocked_step'] == 0) & (held > 0)).sum()),
                   'blocked': int((got['blocked_step'] > 0).sum()), 'side': int(got['side'].sum()),
                   'moving_voxels_mean': round(float(got['moved'][held > 0].mean()), 1) if (held > 0).any() else 0.0}
    # the host route to the same bits: scene 0's first host_rows rows, once, by the host clock
    t0 = time.perf_counter()
    lab, bbox, h0, q0 = res['labels'][0].cpu().numpy(), res['bbox'][0].cpu().numpy(), gres['object'][0].cpu().numpy(), quat[0].cpu().numpy()
    t1 = time.perf_counter()
    want = RR.retreat_rows(lab, bbox, h0[:host_rows], q0[:host_rows], host_rows, scale)
    t2 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    rec['host_ms'] = {'rows': host_rows, 'read_back': ms(t0, t1), 'numpy_retreat': ms(t1, t2), 'numpy_retreat_per_row': round((t2 - t1) * 1e3 / host_rows, 4),
                      'what': 'once, host clock, this box\'s CPU; scene 0\'s first `rows` rows'}
    rec['equals_host_route'] = bool(all(np.array_equal(got[k][0, :host_rows].view(np.int32), w.view(np.int32)) for k, w in zip(RETREAT_ROWS, want)))
    rec['device_p50_per_row_us'] = round(rec['device_ms']['grasp_retreat']['p50'] * 1e3 / (B * ROWS), 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grasp_retreat.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_grasp_retreat.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    dev = torch.device('cuda:0')
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls (three warm-up calls)', 'calls': a.calls,
           'scene': 'three touching balls on the floor and a fourth in their hollow, scaled to the lattice (tools/time_grasp_retreat.py); '
                    '2 048 grasps per scene around the balls, three quarters within 40 degrees of straight down',
           'device': torch.cuda.get_device_name(0), 'cpus_of_the_host_route': len(os.sched_getaffinity(0))}
    for name, B, R, host_rows in SHAPES:
        res[name] = measure(B, R, host_rows, a.calls, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
