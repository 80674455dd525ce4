"""Wall time of one plan at the reference planner's operating point (src/nr/main.py:188-209: 6 views, 640x360 renderings
-> 512x288, 40^3, one scene per call), synthetic weights, from the SAME uint8 frames on two routes:
  (a) today's route: host resize_bilinear_u8 per view + / 255 + transpose, then planner.plan() (eager forward + selection);
      the host image preparation is timed on its own and the two are summed per call;
  (b) PlannerSession.plan(): pinned upload of the uint8 frames, one captured-graph replay, one read-back.
Both are timed with a host clock around the whole call (each ends in a device synchronisation), alternating a, b, a, b ...
after a warm-up, and reported as p50 / p99 with (a)'s spread.  Writes profiles/planner_session.json.
Usage: python tools/time_planner.py [--calls 60] [--warmup 5] [--out profiles/planner_session.json]

--real: the real-robot route instead (planner.plan_real; src/nr/utils/grasp_utils.py:119-151), three legs on one box, alternating:
  (a) a PlannerSession WITHOUT the new outputs (the selection in index order, no cloud) -- to compare with the commit before the
      route existed, copy this file into a built checkout of that commit, run it there with --real --only-a (leg (a) uses nothing
      newer) and hand that run's JSON in with --parent-json: the requirement on (a) is that its p50 lies within the parent's own
      p10..p90.  Within one process the calls agree to 0.03 ms while two processes of the SAME checkout differ by up to 0.1 ms, so
      the comparison pools processes: --parent-json and --a-json (further --only-a runs of this checkout) take several files,
      run alternately, and the percentiles are taken over the pooled calls;
  (b) planner.real_session: grasp_utils.process's thresholds, the ranked top-10 and the surface cloud inside the graph;
  (c) the host route to the same result: leg (a)'s replay, the four volumes read back, then scipy / numpy process + select +
      argsort + extract_surface_points_from_volume as the reference runs them.
Writes profiles/planner_session_real.json with p10 / p50 / p90 per leg.
--real --normals: a fourth leg in the same alternation,
  (d) planner.real_session(normals=True): leg (b) plus the SDF gradient volume and the gather of its rows at the cloud's voxels in
      the graph, the rows read back with the index rows, unit normals on the host."""
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


def synthetic_net(real=True):
    """The synthetic checkpoint with a quality bias that leaves survivors; real: widths inside the 0..12 grasp_utils.process keeps."""
    shapes = {k: tuple(v.shape) for k, v in GraspNeRF(dict(CFG)).state_dict().items()}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_state_dict(shapes).items()}
    sd['vgn_net.conv_qual.bias'] = sd['vgn_net.conv_qual.bias'] + 2.5
    if real:
        sd['vgn_net.conv_width.bias'] = sd['vgn_net.conv_width.bias'] + 5.0
    return planner.load_model(dict(CFG), sd)


def session_legs(calls, legs, warmup=5):
    """The real-robot plan through planner.real_session with and without one further output in the session's graph (tools/time_mesh.py,
    tools/time_raycast.py): leg a, the ranked top-10 and the cloud; legs b and c, `legs(iso)` -> {name: further keywords of real_session
    and plan_real} with iso the synthetic checkpoint's median level.  Host clock around the whole call, alternating.
    -> (the result dict: shape, percentiles per leg, b / c minus a;  the last output of every leg;  iso)."""
    net = synthetic_net()
    hw = (IMG_WH[1], IMG_WH[0])
    frames = np.random.default_rng(0).integers(0, 256, (V, *hw, 3), dtype=np.uint8)
    poses = ring_cameras(V)
    K = np.float32([[357.048, 0, 255.8], [0, 357.048, 143.8], [0, 0, 1]])
    vol = planner.plan_real(net, frames, poses, K)[2]
    rg = (float(np.percentile(vol, 40)), float(np.percentile(vol, 60)))
    iso = float(np.float32(np.median(vol)))
    kw = dict(order='score', top_k=10, surface_rg=rg)
    a = 'a_session_ranked_top10_and_cloud'
    legs = {a: {}, **legs(iso)}
    sess = {k: planner.real_session(net, V, hw, IMG_WH, **kw, **m) for k, m in legs.items()}

    def run(k):
        t0 = time.perf_counter()
        out = planner.plan_real(net, frames, poses, K, **kw, **legs[k], session=sess[k])
        return time.perf_counter() - t0, out

    for _ in range(warmup):
        last = {k: run(k)[1] for k in legs}
    times = {k: [] for k in legs}
    for _ in range(calls):                                                   # alternating: the legs see the same machine state
        for k in legs:
            times[k].append(run(k)[0])
    res = {'shape': {'views': V, 'frames_hw': hw, 'volume_resolution': 40, 'weights': 'synthetic'}, 'calls': calls, 'warmup': warmup,
           'unit': 'ms, host clock around the whole plan_real(session=...) call (ends in a device synchronisation)',
           'device': torch.cuda.get_device_name(0)}
    for k, t in times.items():
        res[k] = {q: pct(t, p) for q, p in (('p10', 10), ('p50', 50), ('p90', 90))}
    res['same_grasps_and_cloud'] = bool(all(np.array_equal(last[k][0]['index'], last[a][0]['index']) and
                                            np.array_equal(last[k][3]['index'], last[a][3]['index']) for k in legs))
    b, c = list(legs)[1:]
    res['b_minus_a_p50'], res['c_minus_a_p50'] = res[b]['p50'] - res[a]['p50'], res[c]['p50'] - res[a]['p50']
    return res, last, iso


def host_real_route(tsdf, qual, rot, width, top_k, rg):
    """grasp_utils.process + select + sim_grasp's ranking + extract_surface_points_from_volume on the host, as the reference runs
    them (scipy.ndimage; grasp_utils.py:40-105, draw_utils.py:355-377)."""
    from scipy import ndimage
    tsdf, qual, rot, width = tsdf.squeeze(), qual.squeeze(), rot.squeeze(), width.squeeze()
    qual = ndimage.gaussian_filter(qual, sigma=1.0, mode='nearest')
    valid = ndimage.binary_dilation(tsdf > 0.1, iterations=2, mask=np.logical_not(np.logical_and(-1 < tsdf, tsdf < -0.1)))
    qual[valid == False] = 0.0                                               # noqa: E712
    qual[np.logical_or(width < 0, width > 12)] = 0.0
    q = qual.copy()
    q[q < 0.90] = 0.0
    q = np.where(q == ndimage.maximum_filter(q, size=4), q, 0.0)
    idx = np.argwhere(q)
    scores = q[idx[:, 0], idx[:, 1], idx[:, 2]]
    p = np.argsort(scores)[::-1][:top_k]
    quat = rot[:, idx[p, 0], idx[p, 1], idx[p, 2]].T
    ind = np.transpose(((tsdf > rg[0]) & (tsdf < rg[1])).nonzero())
    return idx[p], scores[p], quat, width[idx[p, 0], idx[p, 1], idx[p, 2]], ind, ind.astype(np.float64) * (0.3 / 40)


def main_real(a, net):
    """The --real legs (see the module docstring)."""
    V = 6
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (V, IMG_WH[1], IMG_WH[0], 3), dtype=np.uint8)     # run_real's frames are the network's size
    poses = ring_cameras(V)
    K = np.float32([[357.048, 0, 255.8], [0, 357.048, 143.8], [0, 0, 1]])
    Ks, top_k = np.repeat(K[None], V, 0), 10
    hw = (IMG_WH[1], IMG_WH[0])
    # run_real's box and depth range (grasp_utils.py:122-123) and grasp_utils.process's parameters without the third threshold
    # (:45-47,60), spelled out: leg (a) must run on a checkout that has no plan_real
    DR, BOX = (0.2, 0.8), ((-0.15, -0.15, 0.0), (0.15, 0.15, 0.3))
    kw = dict(gaussian_filter_sigma=1.0, min_width=0, max_width=12, tsdf_thres_high=-0.1, tsdf_thres_low=-1)
    plain = PlannerSession(net, V, hw, IMG_WH, voxel_size=0.3 / 40, **kw)
    vol = plain.plan(frames, poses, Ks, DR, BOX, return_volumes=True)[0]['volumes'][0]
    rg = (float(np.percentile(vol, 40)), float(np.percentile(vol, 60)))              # the synthetic volume has no zero crossing

    def leg_a():
        t0 = time.perf_counter()
        g, _ = plain.plan(frames, poses, Ks, DR, BOX)
        return time.perf_counter() - t0, g

    def leg_b():
        t0 = time.perf_counter()
        out = planner.plan_real(net, frames, poses, K, order='score', top_k=top_k, surface_rg=rg, session=real)
        return time.perf_counter() - t0, out

    def leg_c():
        t0 = time.perf_counter()
        g, _ = plain.plan(frames, poses, Ks, DR, BOX, return_volumes=True)
        out = host_real_route(*g['volumes'][:4], top_k, rg)
        return time.perf_counter() - t0, out

    def leg_d():
        t0 = time.perf_counter()
        out = planner.plan_real(net, frames, poses, K, order='score', top_k=top_k, surface_rg=rg, session=real_n, normals=True)
        return time.perf_counter() - t0, out

    def measure(legs):
        for _ in range(a.warmup):
            last = {k: f()[1] for k, f in legs.items()}
        times = {k: [] for k in legs}
        for _ in range(a.calls):                                             # alternating: the legs see the same machine state
            for k, f in legs.items():
                times[k].append(f()[0])
        return times, last

    # leg (a) on its own, before anything of the new route exists in the process: the procedure of a --only-a run, so that the two
    # are comparable; then (b) and (c), alternating
    times, last = measure({'a_session_without_new_outputs': leg_a})
    have_v2 = not a.only_a
    if have_v2:
        real = planner.real_session(net, V, hw, IMG_WH, order='score', top_k=top_k, surface_rg=rg)
        legs = {'b_session_ranked_top10_and_cloud': leg_b, 'c_host_route_numpy': leg_c}
        if a.normals:
            real_n = planner.real_session(net, V, hw, IMG_WH, order='score', top_k=top_k, surface_rg=rg, normals=True)
            legs['d_session_with_surface_normals'] = leg_d
        t2, l2 = measure(legs)
        times.update(t2), last.update(l2)
    res = {'shape': {'views': V, 'frames_hw': hw, 'volume_resolution': 40, 'weights': 'synthetic'}, 'calls': a.calls, 'warmup': a.warmup,
           'unit': 'ms, host clock around the whole call (ends in a device synchronisation)', 'library': os.path.basename(_lib_path()),
           'device': torch.cuda.get_device_name(0)}
    for k, t in times.items():
        res[k] = {'p10': pct(t, 10), 'p50': pct(t, 50), 'p90': pct(t, 90)}
    if a.only_a:
        res['a_calls_ms'] = [round(t * 1e3, 4) for t in times['a_session_without_new_outputs']]
    if have_v2:
        b, c = last['b_session_ranked_top10_and_cloud'], last['c_host_route_numpy']
        res['survivors'], res['cloud_points'] = int(real.selection['count'][0]), int(len(b[3]['index']))
        res['b_equals_c'] = bool(np.array_equal(b[0]['index'], c[0]) and np.array_equal(b[1], c[1]) and np.array_equal(b[3]['index'], c[4])
                                 and np.array_equal(b[3]['points'], c[5]))
        if a.normals:
            d = last['d_session_with_surface_normals']
            res['d_same_grasps_and_cloud_as_b'] = bool(np.array_equal(d[0]['index'], b[0]['index']) and np.array_equal(d[3]['index'], b[3]['index']))
            res['d_minus_b_p50'] = res['d_session_with_surface_normals']['p50'] - res['b_session_ranked_top10_and_cloud']['p50']
        res['b_p50_below_c_p50'] = bool(res['b_session_ranked_top10_and_cloud']['p50'] < res['c_host_route_numpy']['p50'])
    if a.parent_json:
        pool = lambda files: np.concatenate([json.load(open(f))['a_calls_ms'] for f in files]) / 1e3
        par = pool(a.parent_json)
        own = np.concatenate([pool(a.a_json)] if a.a_json else [] + [np.asarray(times['a_session_without_new_outputs'])])
        p50s = lambda files: [json.load(open(f))['a_session_without_new_outputs']['p50'] for f in files]
        res['a_parent_commit'] = {'processes': len(a.parent_json), 'p10': pct(par, 10), 'p50': pct(par, 50), 'p90': pct(par, 90),
                                  'p50_per_process': p50s(a.parent_json)}
        res['a_this_commit'] = {'processes': len(a.a_json) or 1, 'p10': pct(own, 10), 'p50': pct(own, 50), 'p90': pct(own, 90),
                                'p50_per_process': p50s(a.a_json) if a.a_json else [res['a_session_without_new_outputs']['p50']]}
        res['a_p50_within_parent_p10_p90'] = bool(pct(par, 10) <= pct(own, 50) <= pct(par, 90))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def _lib_path():
    from graspnerf_amd import _lib
    return _lib.LIB_PATH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--real', action='store_true', help='the real-robot route: profiles/planner_session_real.json')
    ap.add_argument('--normals', action='store_true', help='--real: leg (d), the session with the surface normals')
    ap.add_argument('--only-a', action='store_true', help='--real: leg (a) alone (a checkout from before the route has no other)')
    ap.add_argument('--parent-json', nargs='+', default=None, help='--real: JSONs of --real --only-a runs in a checkout of the parent commit')
    ap.add_argument('--a-json', nargs='*', default=None, help='--real: JSONs of --real --only-a runs of this checkout (pooled instead of this run\'s leg (a))')
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'planner_session_real.json' if a.real else 'planner_session.json')
    if not torch.cuda.is_available():
        sys.exit('time_planner.py measures on a ROCm GPU; there is nothing to time without one')
    net = synthetic_net(a.real)
    if a.real:
        return main_real(a, net)
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
