"""Wall time of one plan at the reference planner's operating point (src/nr/main.py:188-209: 6 views, 640x360 renderings
-> 512x288, 40^3, one scene per call), synthetic weights, from the SAME uint8 frames on two routes:
  (a) today's route: host resize_bilinear_u8 per view + / 255 + transpose, then planner.plan() (eager forward + selection);
      the host image preparation is timed on its own and the two are summed per call;
  (b) PlannerSession.plan(): pinned upload of the uint8 frames, one captured-graph replay, one read-back.
Both are timed with a host clock around the whole call (each ends in a device synchronisation), alternating a, b, a, b ...
after a warm-up, and reported as p50 / p99 with (a)'s spread.  Writes profiles/planner_session.json.
Usage: python tools/time_planner.py [--calls 60] [--warmup 5] [--out profiles/planner_session.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graspnerf_amd import planner                                            # noqa: E402
from graspnerf_amd.grasp_post import GraspSelector                           # noqa: E402
from graspnerf_amd.planner_session import PlannerSession                     # noqa: E402
from graspnerf_amd.renderer import GraspNeRF                                 # noqa: E402
from graspnerf_amd.synth import ring_cameras, synth_state_dict               # noqa: E402

CFG = yaml.safe_load("""
init_net_type: cost_volume
agg_net_type: neus
use_hierarchical_sampling: true
use_depth_loss: true
dist_decoder_cfg: {use_vis: false}
fine_dist_decoder_cfg: {use_vis: false}
ray_batch_num: 4096
sample_volume: true
render_rgb: false
volume_type: [sdf]
volume_resolution: 40
depth_sample_num: 40
fine_depth_sample_num: 40
agg_net_cfg: {sample_num: 40, init_s: 0.3, fix_s: 0}
fine_agg_net_cfg: {sample_num: 40, init_s: 0.3, fix_s: 0}
""")
V, SRC_HW, IMG_WH = 6, (360, 640), (512, 288)
THRES = dict(tsdf_thres_high=0.0, tsdf_thres_low=-0.85)                      # main.py:93-94


def pct(x, p):
    return float(np.percentile(np.asarray(x) * 1e3, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'planner_session.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_planner.py measures on a ROCm GPU; there is nothing to time without one')
    shapes = {k: tuple(v.shape) for k, v in GraspNeRF(dict(CFG)).state_dict().items()}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_state_dict(shapes).items()}
    sd['vgn_net.conv_qual.bias'] = sd['vgn_net.conv_qual.bias'] + 2.5
    net = planner.load_model(dict(CFG), sd)
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (V, *SRC_HW, 3), dtype=np.uint8)
    poses = ring_cameras(V)
    K = np.repeat(np.float32([[357.048, 0, 255.8], [0, 357.048, 143.8], [0, 0, 1]])[None], V, 0)    # main.py:105-112 at 0.8 / 2
    dr = np.tile(np.float32([0.2, 0.8]), (V, 1))
    bbox = [[-0.15, -0.15, -0.0503], [0.15, 0.15, 0.2497]]
    selector = GraspSelector(next(net.parameters()).device)
    session = PlannerSession(net, V, SRC_HW, IMG_WH, **THRES)

    def route_a():
        t0 = time.perf_counter()
        images = np.stack([planner.resize_bilinear_u8(f, IMG_WH).astype(np.float32) for f in frames], 0)
        images = (images.astype(np.float32) / 255).transpose([0, 3, 1, 2])
        t1 = time.perf_counter()
        g, _ = planner.plan(net, images, poses, K, dr, bbox, seed=0, selector=selector, **THRES)
        return t1 - t0, time.perf_counter() - t1, g

    def route_b():
        t0 = time.perf_counter()
        g, inner = session.plan(frames, poses, K, dr, bbox, seed=0)
        return time.perf_counter() - t0, inner, g

    for _ in range(a.warmup):
        ga, gb = route_a()[2], route_b()[2]
    same = len(ga['index']) == len(gb['index']) and np.array_equal(ga['index'], gb['index'])
    ra, pa, b, bi = [], [], [], []
    for _ in range(a.calls):                                                 # alternating: both routes see the same machine state
        r, p, _ = route_a()
        ra.append(r), pa.append(p)
        t, inner, _ = route_b()
        b.append(t), bi.append(inner)
    tot = np.asarray(ra) + np.asarray(pa)
    res = {'shape': {'views': V, 'src_hw': SRC_HW, 'img_wh': IMG_WH, 'volume_resolution': 40, 'weights': 'synthetic'},
           'calls': a.calls, 'warmup': a.warmup, 'unit': 'ms, host clock around the whole call (ends in a device synchronisation)',
           'a_host_resize': {'p50': pct(ra, 50), 'p99': pct(ra, 99)},
           'a_plan_eager': {'p50': pct(pa, 50), 'p99': pct(pa, 99)},
           'a_total': {'p50': pct(tot, 50), 'p99': pct(tot, 99), 'p10': pct(tot, 10), 'p90': pct(tot, 90),
                       'spread_p90_minus_p10': pct(tot, 90) - pct(tot, 10)},
           'b_session_plan': {'p50': pct(b, 50), 'p99': pct(b, 99), 'p10': pct(b, 10), 'p90': pct(b, 90)},
           'b_session_plan_first_copy_to_read_back': {'p50': pct(bi, 50), 'p99': pct(bi, 99)},
           'b_wins_by_more_than_a_spread': bool(pct(tot, 50) - pct(b, 50) > pct(tot, 90) - pct(tot, 10)),
           'grasps': {'a': int(len(ga['index'])), 'b': int(len(gb['index'])), 'same_voxels': bool(same)},
           'graph_captures': session.captures, 'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
