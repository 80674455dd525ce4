"""Cost of the finger closure of the ranked grasps (gnr_finger_closure_fwd, hand.FingerClosure) at the real-robot route's shape -- a 40^3
volume, the 2 048-row buffer of a default session and a top-10 list, the viewer's hand and a real one: p10 / p50 / p90 of single calls
between HIP events, next to the host route to the same bits -- the numpy float64 statement (tests/closure_reference.py) on this box's
CPU, on the same rows.  The volume and the grasps are tools/time_hand_clearance.py's.
Then the real-robot plan (planner.plan_real through planner.real_session), without and with closure=, host clock around the whole call,
alternating; the leg without is the graph a session recorded before this product existed (the parent commit's, 2c28280: "Gripper
clearance of the ranked grasps"), next to the p50 the earlier profiles of this directory recorded for it.
Usage: python tools/time_finger_closure.py [--calls 100] [--out profiles/finger_closure.json]"""
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
import closure_reference as CR                                               # noqa: E402
from graspnerf_amd.hand import CLOSURE_ROWS, FingerClosure                   # noqa: E402
from time_hand_clearance import A_LEG, R, REAL_HAND, ROWS, earlier_profiles  # noqa: E402
from time_mesh import scene                                                  # noqa: E402
from time_tsdf import event_ms, pct                                          # noqa: E402


def kernels(a):
    dev = torch.device('cuda:0')
    scale = 0.3 / R
    res = {'unit': 'ms per call between HIP events, p10 / p50 / p90 of single calls', 'calls': a.calls,
           'volume': 'a sphere and a torus, clipped signed distance (tools/time_mesh.py), 40^3', 'device': torch.cuda.get_device_name(0)}
    host_vol = scene(R, 0.0)
    vol = torch.from_numpy(host_vol[None]).to(dev)
    rng = np.random.default_rng(0)
    pos = rng.uniform(-2.0, R + 1.0, (ROWS, 3))
    quat = rng.normal(size=(ROWS, 4)).astype(np.float32)
    width = rng.uniform(1.33, 9.33, ROWS).astype(np.float32)
    P, Q, W = (torch.from_numpy(x[None]).to(dev) for x in (pos, quat, width))
    op = FingerClosure(dev)
    for name, rows, kw in (('rows_2048_viewer_hand', ROWS, {}), ('rows_2048_real_hand_open_0.08', ROWS, REAL_HAND), ('rows_10_viewer_hand', 10, {})):
        count = torch.tensor([rows], dtype=torch.int32, device=dev)
        call = lambda: op(vol, P, Q, W, count, scale=scale, **kw)
        got = [call()[k][0, :rows].cpu().numpy() for k in CLOSURE_ROWS]
        w = 0.08 if 'opening' in kw else 9.33 * scale
        rec = {'rows': rows, 'hand': kw or 'defaults', 'finger_contacts': int((got[2] >= 0).sum()),
               'volume_reads_per_grasp_at_most': CR.reads(w, scale, **{k: v for k, v in kw.items() if k == 'height'}),
               'device_ms': pct(event_ms(call, a.calls))}
        t0 = time.perf_counter()
        want = CR.closure_rows(host_vol, pos[:rows], quat[:rows], width[:rows], rows, scale, **kw)
        rec['host_statement_ms'] = {'once': round((time.perf_counter() - t0) * 1e3, 1), 'what': 'numpy float64 statement on the same rows'}
        rec['equals_host_statement'] = bool(all(np.array_equal(g.view(np.uint32), w_.view(np.uint32)) for g, w_ in zip(got, want)))
        res[name] = rec
    return res


def session(a):
    import time_planner as TP
    res, last, _ = TP.session_legs(a.calls, lambda iso: {'b_with_closure': dict(closure=dict(level=iso)),
                                                         'c_with_closure_of_a_real_hand': dict(closure=dict(REAL_HAND, level=iso))})
    res['a_is'] = 'the graph of a session without the product: what the parent commit (2c28280) records for the same keywords'
    before = earlier_profiles()
    res['a_p50_in_the_earlier_profiles'] = before
    if before:
        v = list(before.values())
        res['a_p50_spread_of_the_earlier_profiles'] = max(v) - min(v)
        res['a_p50_minus_their_mean'] = res[A_LEG]['p50'] - float(np.mean(v))
    g = last['b_with_closure'][0]
    res['held'] = [int(g['held'].sum()), len(g['held'])]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'finger_closure.json'))
    ap.add_argument('--skip-session', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_finger_closure.py measures on a ROCm GPU; there is nothing to time without one')
    if a.calls < 50:
        sys.exit('--calls must be at least 50')
    res = kernels(a)
    if not a.skip_session:
        res['planner_session'] = session(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
