"""A/B of the view-mask sample order of the inference render passes (include/gnr.h "sample order") in ONE process, per batch size:

  step      the forward step bench.py times (prepare + 40^3 volume + 512 rays x (40 + 40)) with the default options and with
            GNR_OPT_SAMPLE_ORDER_NATURAL, alternating, ms per step (HIP events around `--steps` steps) and per-kernel ms;
  chain     the coarse chain launch alone in the natural order and in the device sort's order GIVEN from outside
            (debug_render_by_depth_perm: no threshold, no key / sort launches), so the launch sizes below the threshold can be
            measured too, next to the cost of the sort alone.

   python tools/ab_sample_order.py [--batches 1 2 4 8 32] [--steps 30] [--reps 3]     -> one AB_JSON line"""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graspnerf_amd import weights, _lib
from graspnerf_amd.hotpath import HotPath, batch_scenes
from graspnerf_amd.synth import make_scene

ap = argparse.ArgumentParser()
ap.add_argument('--batches', type=int, nargs='+', default=[1, 2, 4, 8, 32])
ap.add_argument('--steps', type=int, default=30)
ap.add_argument('--reps', type=int, default=3)
a = ap.parse_args()
wnp = dict(np.load(os.path.join(ROOT, 'tests/golden/weights_seed0.npz')))
hp = HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))
scenes = [make_scene(i, 'cfg2') for i in range(max(a.batches))]
KEEP = ('k_chain.render', 'k_chain.volume', 'k_ray.render', 'k_points_rays', 'k_sample_order')


def timed(fn, n):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernels(fn, n):
    _lib.timing_begin()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return {k: round(v[1] / n, 4) for k, v in _lib.timing_end().items() if k.startswith(KEEP)}


out = {}
for B in a.batches:
    bref, bque = batch_scenes(scenes[:B])
    bref = {k: torch.from_numpy(v).cuda() for k, v in bref.items()}
    bque = {k: torch.from_numpy(v).cuda() for k, v in bque.items()}

    def step():
        prep = hp.prepare(bref, 40, 512, 40)
        hp.sample_volume(bref, 40, prepared=prep)
        return hp.render(bref, bque, prepared=prep)

    rec = {'step_ms': {'ordered': [], 'natural': []}}
    for rep in range(a.reps):
        for name in ('ordered', 'natural'):
            hp.set_option('sample_order_natural', name == 'natural')
            rec['step_ms'][name].append(round(timed(step, a.steps), 4))
    for name in ('ordered', 'natural'):
        hp.set_option('sample_order_natural', name == 'natural')
        rec['kernels_' + name] = kernels(step, 10)
    # the coarse chain launch alone, order given from outside
    hp.set_option('sample_order_natural', True)
    prep = hp.prepare(bref, 40, 512, 40)
    co, fi, _ = hp.render(bref, bque, prepared=prep, debug=True)
    rec['chain_ms'] = {}
    for lvl, o in (('coarse', co), ('fine', fi)):
        depth, keys = o['depth'].clone(), o['view_mask'].reshape(B, -1).clone()
        perm = hp.debug_sample_order(keys)
        nat = kernels(lambda: hp.render_by_depth(bref, bque, depth, lvl, prepared=prep), 10)
        srt = kernels(lambda: hp.debug_render_by_depth_perm(bref, bque, depth, perm, lvl, prepared=prep), 10)
        rec['chain_ms'][lvl] = {'natural': nat.get('k_chain.render'), 'ordered': srt.get('k_chain.render')}
    rec['sort_alone_ms'] = kernels(lambda: hp.debug_sample_order(keys), 10)
    hp.set_option('sample_order_natural', False)
    out[f'B{B}'] = rec
    print(f'B={B}', json.dumps(rec), flush=True)
print('AB_JSON ' + json.dumps(out))
