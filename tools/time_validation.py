"""Time of ONE validation scene at the benched frame (6 views 288x512, 40^3 volume, full-frame query = 147 456 rays, 40 + 40
samples) on the GPU, split into the eval forward, the loss terms and the frame metrics (csrc/gnr_metrics.hip), next to the same
frame's metrics through the host twin (device-to-host copy of the outputs + numpy).  Host clock around work that ends in a device
synchronise; the metrics' kernel times from the library's own event brackets.  A record, not a gate.
    python tools/time_validation.py [--iters N] [--out profiles/validation.json]"""
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

from graspnerf_amd import _lib, metrics                       # noqa: E402
from graspnerf_amd.planner import full_frame_coords           # noqa: E402
from graspnerf_amd.renderer import GraspNeRF                  # noqa: E402
from graspnerf_amd.synth import synth_state_dict              # noqa: E402
from graspnerf_amd.trainer import train_losses                # noqa: E402
from graspnerf_amd.validation import Validator                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'validation.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_validation.py measures on the GPU: no device found')
    from test_train_step import _full_size_cfg, _full_size_scene
    net = GraspNeRF(_full_size_cfg())
    syn = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in syn.items()}, strict=True)
    net = net.cuda().eval()
    data = _full_size_scene(0)
    que = dict(data['que_imgs_info'])
    h, w = que['imgs'].shape[-2:]
    rng = np.random.Generator(np.random.PCG64(1))
    que['coords'] = torch.from_numpy(full_frame_coords(h, w)).cuda()
    que['true_depth'] = torch.from_numpy(rng.random((1, 1, h, w), dtype=np.float32) * np.float32(0.6) + np.float32(0.2)).cuda()
    data = dict(data, que_imgs_info=que, eval=True)

    def timed(f, n):
        for _ in range(3):
            r = f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {'median_ms': round(float(np.median(ts)), 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4), 'n': n}, r

    with torch.no_grad():
        t_fwd, out = timed(lambda: net(data), a.iters)
        t_loss, _ = timed(lambda: train_losses(out, data), a.iters)
        t_met, m = timed(lambda: metrics.frame_metrics(out, data), a.iters)
        t_scene, _ = timed(lambda: Validator().scene_terms(net, data), a.iters)
        _lib.timing_begin('gnr_frame_metrics')
        for _ in range(a.iters):
            metrics.frame_metrics(out, data)
        kern = {k: round(ms / cnt, 5) for k, (cnt, ms) in _lib.timing_end().items()}
        cpu = lambda o: {k: v.cpu() for k, v in o.items() if torch.is_tensor(v)}
        t_copy, host_out = timed(lambda: cpu(out), max(a.iters // 4, 3))
        host_data = {'que_imgs_info': cpu(que)}
        t_host, mh = timed(lambda: metrics.frame_metrics(host_out, host_data), max(a.iters // 4, 3))
    rec = {'what': 'one validation scene at the benched frame: 6 views 288x512, 40^3 volume, full-frame query (147456 rays), 40 + 40 samples',
           'command': 'python tools/time_validation.py --iters %d' % a.iters,
           'device': torch.cuda.get_device_name(0),
           'clock': 'host clock around work that ends in torch.cuda.synchronize(); kernel_ms: event brackets of gnr_timing_*',
           'eval_forward': t_fwd, 'loss_terms': t_loss, 'frame_metrics_device': t_met, 'frame_metrics_kernel_ms_per_launch': kern,
           'scene_total (forward + losses + metrics)': t_scene,
           'host_twin': {'device_to_host_copy_of_all_outputs': t_copy, 'frame_metrics_numpy': t_host},
           'values': {k: float(v) for k, v in m.items()},
           'host_twin_minus_device': {k: float(mh[k]) - float(m[k]) for k in m}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, 'w'), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == '__main__':
    main()
