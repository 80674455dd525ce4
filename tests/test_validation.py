"""Validation pass, checkpoints and the loop around Trainer.step (graspnerf_amd/validation.py, trainer.py validate / fit /
save_checkpoint / load_checkpoint; ref: train/train_valid.py:11-46, train/trainer.py:115-218).

CPU: a stub network that returns fixed outputs per scene (the product's eval forward needs the GPU) drives the pass, the key
metric, the saving rules and the gloo exchange; the checkpoint round trip runs the model of tests/test_train_step.py.
gpu: the same model validates two scenes whose query view is the full 96x128 frame."""
import os
import socket

import numpy as np
import pytest
import torch

from graspnerf_amd import metrics, trainer as trainer_mod, validation
from graspnerf_amd.synth import synth_metric_frames
from graspnerf_amd.trainer import Trainer

H, W = 33, 64


class StubNet(torch.nn.Module):
    """Returns the frames its scene carries and one loss-like value that depends on its parameter; notes how it was called."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.tensor([0.5]))
        self.sub = torch.nn.Sequential(torch.nn.Identity())
        self.calls = []

    def forward(self, data):
        self.calls.append((self.training, self.sub.training, torch.is_grad_enabled(), data.get('eval'), data['step']))
        return dict(data['stub'], lv=(self.p - data['target']) ** 2)


def stub_losses(out, data, cfg=None):
    return {'loss_vgn': out['lv'], 'other': out['lv'] * 3.0}


def stub_losses_without_vgn(out, data, cfg=None):
    return {'loss_rgb_nr': out['lv']}


def stub_scene(i):
    gt, preds, dpr, dgt = synth_metric_frames(500 + i, H, W, 1, 2)
    t = torch.from_numpy
    return {'target': torch.tensor([0.1 * i]),
            'stub': {'pixel_colors_gt': t(gt), 'pixel_colors_nr': t(preds[0]), 'pixel_colors_nr_fine': t(preds[1]), 'render_depth': t(dpr)},
            'que_imgs_info': {'imgs': torch.zeros(1, 3, H, W), 'true_depth': t(dgt)[:, None]}}


def test_validate_means_key_metric_and_modes(monkeypatch):
    monkeypatch.setattr(trainer_mod, 'train_losses', stub_losses)
    net = StubNet()
    net.train()
    net.sub.eval()                                                 # a sub-module the caller keeps in eval mode stays there
    tr = Trainer(net)
    scenes = [stub_scene(i) for i in range(3)]
    results, val = tr.validate(scenes)
    lv = [(0.5 - 0.1 * i) ** 2 for i in range(3)]
    assert val == results['loss_vgn'] and abs(val - np.mean(lv)) < 1e-7          # the mean over the scenes (float32 terms)
    assert abs(results['other'] - 3 * np.mean(lv)) < 1e-6
    assert set(results) == {'loss_vgn', 'other', 'psnr_nr', 'psnr_nr_fine', 'ssim_nr', 'ssim_nr_fine', 'depth_mae'}
    per = [metrics.frame_metrics(s['stub'], s) for s in scenes]
    for k in ('psnr_nr', 'psnr_nr_fine', 'ssim_nr', 'ssim_nr_fine', 'depth_mae'):
        assert abs(results[k] - np.mean([float(m[k]) for m in per])) <= 1e-12 * abs(results[k]), k
    # eval() under no_grad with data['eval'] = True and the trainer's step; the modes come back as they were
    assert net.calls == [(False, False, False, True, 0)] * 3
    assert net.training and not net.sub.training
    net.eval()
    tr.validate(scenes[:1], step=7)
    assert not net.training and net.calls[-1] == (False, False, False, True, 7)


def test_missing_loss_vgn_gives_1e6_and_other_key_metrics(monkeypatch):
    monkeypatch.setattr(trainer_mod, 'train_losses', stub_losses_without_vgn)
    tr = Trainer(StubNet())
    scenes = [stub_scene(i) for i in range(2)]
    results, val = tr.validate(scenes)
    assert val == 1e6 and 'loss_vgn' not in results
    tr.validator = validation.Validator('psnr_nr')
    results, val = tr.validate(scenes)
    assert val == results['psnr_nr'] and 30 < val < 45
    with pytest.raises(KeyError):
        validation.Validator('no_such_metric')


def test_better_in_both_directions():
    lo, hi = validation.better('lower'), validation.better('higher')
    assert lo(1.0, 2.0) and not lo(2.0, 1.0) and not lo(1.0, 1.0)
    assert hi(2.0, 1.0) and not hi(1.0, 2.0) and not hi(1.0, 1.0)
    with pytest.raises(ValueError):
        validation.better('smaller')


def test_fit_saving_rules(monkeypatch, tmp_path):
    """Validation at step 0, every val_interval-th step and the last; the step-0 validation never saves; a better key metric writes
    model_best.pth, every save_interval-th step model.pth; best_para starts at 1e6 ('lower') / 0 ('higher'); a second fit resumes."""
    monkeypatch.setattr(trainer_mod, 'train_losses', stub_losses)
    scenes = [stub_scene(i) for i in range(2)]
    d = str(tmp_path / 'only_step0')
    tr = Trainer(StubNet(), {'lr_init': 1e-2})
    best = tr.fit([scenes[:1]], scenes, total_step=1, val_interval=10, save_interval=10, model_dir=d)
    assert [h[0] for h in tr.val_history] == [1] and best == 1e6 and os.listdir(d) == []       # validated, nothing saved

    d = str(tmp_path / 'lower')
    tr = Trainer(StubNet(), {'lr_init': 1e-2})
    best = tr.fit([scenes[:1], scenes[1:]], scenes, total_step=5, val_interval=2, save_interval=3, model_dir=d)
    assert [h[0] for h in tr.val_history] == [1, 2, 4, 5] and tr.step_id == 5
    vals = [h[2] for h in tr.val_history]
    assert best == min(vals[1:]) < 1e6                                  # (Adam walks p towards the targets: the loss falls)
    ck, ckb = torch.load(os.path.join(d, 'model.pth'), weights_only=False), torch.load(os.path.join(d, 'model_best.pth'), weights_only=False)
    assert set(ck) == {'step', 'best_para', 'network_state_dict', 'optimizer_state_dict'}
    assert ck['step'] == 3 and ck['best_para'] == vals[1] and sorted(os.listdir(d)) == ['model.pth', 'model_best.pth']
    assert ckb['best_para'] == best and ckb['step'] == [h[0] for h in tr.val_history if h[2] == best][0]
    # resumed: continues at the saved step with the saved best_para
    tr2 = Trainer(StubNet(), {'lr_init': 1e-2})
    seen = []
    step = tr2.step
    monkeypatch.setattr(tr2, 'step', lambda s: (seen.append(tr2.step_id), step(s))[1])
    tr2.fit([scenes[:1]], scenes, total_step=4, val_interval=2, save_interval=100, model_dir=d)
    assert seen == [3] and [h[0] for h in tr2.val_history] == [4]

    d = str(tmp_path / 'higher')
    tr = Trainer(StubNet(), {'lr_init': 1e-2})
    best = tr.fit([scenes[:1]], scenes, total_step=2, val_interval=1, save_interval=5, model_dir=d, key_metric_name='psnr_nr',
                  key_metric_prefer='higher')
    assert best == tr.val_history[1][2] > 0 and os.listdir(d) == ['model_best.pth']           # from 0: any PSNR is better


def _gloo_worker(rank, world, port, dirs, q):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world)
    trainer_mod.train_losses = stub_losses
    scenes = [stub_scene(i) for i in range(5)]
    tr = Trainer(StubNet(), {'lr_init': 1e-2})
    results, val = tr.validate(scenes)
    few, _ = tr.validate(scenes[:1])                                # fewer scenes than ranks: rank 1's shard is empty
    tr.fit([scenes[rank:rank + 1]], scenes, total_step=2, val_interval=1, save_interval=1, model_dir=dirs[rank])
    q.put((rank, results, val, few, sorted(os.listdir(dirs[rank])) if os.path.isdir(dirs[rank]) else None, tr.val_history))
    dist.barrier()
    dist.destroy_process_group()


def test_validation_exchange_over_gloo(monkeypatch, tmp_path):
    """2 ranks, 5 scenes (shards of 3 and 2): both ranks return the same results, equal to the one-process results; only rank 0 writes."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    dirs = [str(tmp_path / 'rank0'), str(tmp_path / 'rank1')]
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, dirs, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = {}
    for _ in ps:
        r = q.get(timeout=120)
        res[r[0]] = r[1:]
    for p in ps:
        p.join(60)
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert res[0][4] == res[1][4]                                  # the validations inside fit as well
    assert res[0][3] == ['model.pth', 'model_best.pth'] and res[1][3] is None
    monkeypatch.setattr(trainer_mod, 'train_losses', stub_losses)
    scenes = [stub_scene(i) for i in range(5)]
    one, val = Trainer(StubNet()).validate(scenes)
    assert set(one) == set(res[0][0]) and abs(val - res[0][1]) <= 1e-12 * abs(val)
    for k, v in one.items():
        assert abs(res[0][0][k] - v) <= 1e-12 * abs(v), k          # (float64 sums of the same terms in another order)
    few, _ = Trainer(StubNet()).validate(scenes[:1])
    assert few == res[0][2]


def test_checkpoint_round_trip(tmp_path):
    """Two steps, save, load into a fresh Trainer: parameters, Adam moments, step_id and best_para equal bitwise; the next step runs at
    the scheduled learning rate of the resumed step; a plain torch.optim.Adam loads the optimiser state; planner.load_model loads the
    file strictly; the load moves the version counters the packed copies of the hot path and the grasp head are keyed on."""
    from test_train_step import build, scene_data, CFG
    from graspnerf_amd import planner
    lr_cfg = {'lr_init': 1e-3, 'decay_step': 1, 'decay_rate': 0.5, 'lr_min': 1e-6}
    data = scene_data()
    tr = Trainer(build(), lr_cfg)
    for i in range(2):
        torch.manual_seed(i)
        tr.step([data])
    path = str(tmp_path / 'model_best.pth')
    tr.save_checkpoint(path, 0.125)
    ck = torch.load(path, map_location='cpu')                                          # (weights_only: tensors and plain numbers only)
    assert set(ck) == {'step', 'best_para', 'network_state_dict', 'optimizer_state_dict'} and ck['step'] == 2 and ck['best_para'] == 0.125
    assert list(ck['network_state_dict']) == list(tr.net.state_dict())

    fresh = build(weight_seed=3)
    tr2 = Trainer(fresh, lr_cfg)
    versions = [p._version for p in fresh.parameters()]
    assert tr2.load_checkpoint(path) == 0.125 and tr2.step_id == 2
    assert all(p._version > v for p, v in zip(fresh.parameters(), versions))
    for (k, a), b in zip(tr.net.state_dict().items(), fresh.state_dict().values()):
        assert torch.equal(a, b), k
    sa, sb = tr.optimizer.state_dict(), tr2.optimizer.state_dict()
    assert len(sa['state']) == len(sb['state']) == len(tr.params)
    for i, st in sa['state'].items():
        assert float(sb['state'][i]['step']) == float(st['step']) == 2.0
        assert torch.equal(st['exp_avg'], sb['state'][i]['exp_avg']) and torch.equal(st['exp_avg_sq'], sb['state'][i]['exp_avg_sq'])
    torch.manual_seed(9)
    log2 = tr2.step([data])
    torch.manual_seed(9)
    log = tr.step([data])
    assert log2['lr'] == log['lr'] == 1e-3 * 0.25
    assert all(torch.equal(a, b) for a, b in zip(tr.net.state_dict().values(), fresh.state_dict().values())), 'the resumed step differs'

    plain = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(p)) for p in tr.params], lr=1e-3)
    plain.load_state_dict(ck['optimizer_state_dict'])
    assert float(plain.state_dict()['state'][0]['step']) == 2.0 and not plain.param_groups[0].get('fused')
    net = planner.load_model(CFG, checkpoint=path, device='cpu')                       # strict=True inside
    assert torch.equal(net.state_dict()['vgn_net.conv_qual.weight'], ck['network_state_dict']['vgn_net.conv_qual.weight'])


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
def full_frame_scene(i, device='cuda'):
    """A scene of tests/test_train_step.py whose query view is the whole 96x128 frame (12 288 rays) with a seeded true depth."""
    from test_train_step import scene_data
    from graspnerf_amd.planner import full_frame_coords
    d = scene_data(device, scene_id=i)
    que = dict(d['que_imgs_info'])
    h, w = que['imgs'].shape[-2:]
    rng = np.random.Generator(np.random.PCG64(900 + i))
    que['coords'] = torch.from_numpy(full_frame_coords(h, w)).to(device)
    que['true_depth'] = torch.from_numpy(rng.random((1, 1, h, w), dtype=np.float32) * np.float32(0.6) + np.float32(0.2)).to(device)
    return dict(d, que_imgs_info=que)


@pytest.mark.gpu
def test_validate_on_gpu_matches_host_twin_and_per_scene_calls(monkeypatch):
    from test_train_step import build
    net = build('cuda')
    tr = Trainer(net, {'lr_init': 1e-3})
    scenes = [full_frame_scene(0), full_frame_scene(1)]
    seen = []
    real = metrics.frame_metrics
    monkeypatch.setattr(metrics, 'frame_metrics', lambda out, data, *a, **k: (seen.append((out, data)), real(out, data, *a, **k))[1])
    torch.manual_seed(3)
    results, val = tr.validate(scenes)
    monkeypatch.setattr(metrics, 'frame_metrics', real)
    keys = ('psnr_nr', 'psnr_nr_fine', 'ssim_nr', 'ssim_nr_fine', 'depth_mae')
    print({k: results[k] for k in keys + ('loss_vgn',)})
    assert all(np.isfinite(results[k]) for k in keys + ('loss_vgn',)) and val == results['loss_vgn']
    assert len(seen) == 2 and seen[0][0]['pixel_colors_nr'].shape == (1, 96 * 128, 3) and seen[0][0]['pixel_colors_nr'].is_cuda
    assert net.training and all(m.training for m in tr._mode_modules())
    # the same forwards' outputs through the host twin after a .cpu() copy, and through per-scene calls of frame_metrics
    cpu = lambda o: {k: v.cpu() for k, v in o.items() if torch.is_tensor(v)}
    host = [real(cpu(o), {'que_imgs_info': cpu(d['que_imgs_info'])}) for o, d in seen]
    dev = [real(o, d) for o, d in seen]
    tol = {'psnr_nr': 1e-4, 'psnr_nr_fine': 1e-4, 'ssim_nr': 1e-9, 'ssim_nr_fine': 1e-9, 'depth_mae': 1e-5 * results['depth_mae']}
    for k in keys:
        assert dev[0][k].is_cuda and dev[0][k].dtype == torch.float64
        hm, dm = np.mean([float(m[k]) for m in host]), np.mean([float(m[k]) for m in dev])
        print(k, results[k], 'host twin', hm, 'per scene', dm)
        assert abs(results[k] - hm) <= tol[k] and abs(results[k] - dm) <= 1e-12 * abs(dm), k


@pytest.mark.gpu
def test_fit_on_gpu_saves_and_resumes(tmp_path):
    from test_train_step import build, scene_data
    d = str(tmp_path / 'run')
    val_scenes = [full_frame_scene(0), full_frame_scene(1)]
    batches = [[scene_data('cuda', 2)], [scene_data('cuda', 3)]]
    tr = Trainer(build('cuda'), {'lr_init': 1e-3})
    torch.manual_seed(1)
    best = tr.fit(batches, val_scenes, total_step=3, val_interval=2, save_interval=2, model_dir=d)
    assert [h[0] for h in tr.val_history] == [1, 2, 3]
    vals = [h[2] for h in tr.val_history]
    ck, ckb = torch.load(os.path.join(d, 'model.pth'), weights_only=False), torch.load(os.path.join(d, 'model_best.pth'), weights_only=False)
    assert ck['step'] == 2 and ck['best_para'] == vals[1]
    # the first saved best is the validation after step 2 (better than the initial 1e6); the one after step 3 replaces it only if better
    assert ckb['step'] == (3 if vals[2] < vals[1] else 2) and ckb['best_para'] == best == min(vals[1:])
    tr2 = Trainer(build('cuda', weight_seed=3), {'lr_init': 1e-3})
    seen = []
    step = tr2.step
    tr2.step = lambda s: (seen.append(tr2.step_id), step(s))[1]
    torch.manual_seed(2)
    tr2.fit(batches, val_scenes, total_step=4, val_interval=2, save_interval=4, model_dir=d)
    assert seen == [2, 3] and tr2.step_id == 4 and [h[0] for h in tr2.val_history] == [4]
    assert torch.load(os.path.join(d, 'model.pth'), weights_only=False)['step'] == 4
    assert tr2.skipped_steps() == 0
