"""The Python front end of the HIP path (graspnerf_amd/hotpath.py HotPath, graspnerf_amd/renderer.py NeuralRayRenderer): one store for the
per-call options, one pool for the grow-only training buffers, one path that makes the packed weights current.  Small configuration of
tests/test_train_step.py: volume 16^3, 16 + 16 samples per ray, scene cfg1."""
import types

import pytest
import torch

from graspnerf_amd import _lib, weights
from test_train_step import build, scene_data

FIXED, FP32 = _lib.OPTIONS['feature_grad_fixed'], _lib.OPTIONS['fp32_chain']


def test_option_store_keeps_what_it_was_asked_and_merges_only_that():
    from graspnerf_amd.hotpath import HotPath
    nr = build().nr_net                                                   # on the CPU: no HotPath, the store alone
    assert nr._hot is None and nr._hot_options == {}
    assert nr.set_hot_option('feature_grad_fixed', True) is bool(HotPath.default_options & FIXED)
    assert nr.set_hot_option('feature_grad_fixed', False) is True
    assert nr.set_hot_option('fp32_chain', True) is bool(HotPath.default_options & FP32)
    assert nr._hot_options == {'feature_grad_fixed': False, 'fp32_chain': True}
    others = _lib.OPTIONS['geo_dual_fp32'] | _lib.OPTIONS['static_tiles']
    stand_in = types.SimpleNamespace(options=FIXED | others)
    nr._merge_hot_options(stand_in)
    assert stand_in.options == FP32 | others                              # one bit cleared, one set, the others left alone
    stand_in.options = 0
    nr._merge_hot_options(stand_in)
    assert stand_in.options == FP32


@pytest.mark.gpu
def test_options_set_on_the_hot_path_survive_a_forward():
    """Bits set on the HotPath itself used to be overwritten by the renderer's copy at the next hot() / hot_for_training()."""
    from graspnerf_amd.hotpath import HotPath
    from graspnerf_amd.trainer import Trainer
    net = build('cuda')
    Trainer(net, reproducible_feature_grads=True)
    nr, data = net.nr_net, scene_data('cuda')
    h = nr.hot()
    assert h.set_option('fp32_chain', True) is False
    assert h.options & (FIXED | FP32) == FIXED | FP32
    assert nr.hot() is h and h.options & (FIXED | FP32) == FIXED | FP32
    assert nr.hot_for_training() is h and h.options & (FIXED | FP32) == FIXED | FP32
    with torch.no_grad():
        net.eval()
        net(dict(data, eval=True, full_vol=True))
    torch.cuda.synchronize()
    assert nr._hot is h and h.options & (FIXED | FP32) == FIXED | FP32
    assert nr.set_hot_option('feature_grad_fixed', False) is True
    assert h.options & (FIXED | FP32) == FP32                              # that bit only
    net.to('cuda')                                                         # a rebuild: the defaults plus what set_hot_option was asked
    h2 = nr.hot()
    assert h2 is not h and h2.options == HotPath.default_options & ~FIXED and not h2.options & FP32


def _train_grads(net, data, release=False):
    """One training forward + backward -> every parameter's gradient; release: the training workspaces go back between the two."""
    from graspnerf_amd import losses
    from graspnerf_amd.trainer import train_losses
    for a in (net.nr_net.agg_net, net.nr_net.fine_agg_net):
        a.step = 0
    net.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    loss = losses.total_loss(train_losses(net(data), data))
    if release:
        net.nr_net._hot.release_training_workspaces()
    loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


@pytest.mark.gpu
def test_release_of_the_training_workspaces_is_complete_and_harmless():
    """Fixed-point feature gradients and MIOpen's deterministic solvers: a step's gradients are the same bits from run to run, so a
    release that lost a saved state or a scratch buffer would show."""
    net = build('cuda').train()
    net.nr_net.set_hot_option('feature_grad_fixed', True)
    data = scene_data('cuda')
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        g0 = _train_grads(net, data)
        pool = net.nr_net._hot._bufs
        assert {'volume', (1, 'coarse'), (2, 'fine'), 'geo_dual_fwd', 'geo_dual_bwd', 'composite_bwd', 'ray_tail_dual_bwd',
                'depth_mean_bwd'} <= set(pool)
        net.eval()
        assert net.nr_net._hot._bufs == {}                                 # (a) every buffer, geo_dual_fwd's scratch included
        net.train()
        g1 = _train_grads(net, data, release=True)                         # (b) forward -> release -> backward
        g2 = _train_grads(net, data)                                       # (c) a whole step after a release
    finally:
        torch.backends.cudnn.deterministic = was
    for name, g in (('release between forward and backward', g1), ('step after a release', g2)):
        diff = {k: float((g[k] - g0[k]).abs().max()) for k in g0 if not torch.equal(g[k], g0[k])}
        print(name, 'parameters whose gradient differs:', diff)
        assert not diff, (name, diff)


@pytest.mark.gpu
def test_eval_and_training_handles_share_one_weight_sync():
    from graspnerf_amd.trainer import Trainer
    net = build('cuda')
    nr, data = net.nr_net, scene_data('cuda')
    tr = Trainer(net, {'lr_init': 1e-2})
    packed = lambda lvl: torch.from_numpy(weights.pack_state_dict(nr.state_dict(), lvl)).cuda()
    canon = lambda lvl: weights.canonical_blob_device(nr._params(), lvl, as_tensor=True)
    h = nr.hot()
    first = h.wc.clone()
    assert torch.equal(first, packed('coarse'))
    for i in range(2):
        torch.manual_seed(6 + i)
        tr.step([data])
        # the eval handle first: the training handle after it must still bring the backward blobs up to date
        assert nr.hot() is h and torch.equal(h.wc, packed('coarse')) and torch.equal(h.wf, packed('fine'))
        assert nr.hot_for_training() is h and torch.equal(h.wc, packed('coarse'))
        assert all(torch.equal(h.can_dev[lvl], canon(lvl)) for lvl in ('coarse', 'fine'))
    assert not torch.equal(h.wc, first)
    stepped = h.wc.clone()
    with torch.no_grad():
        dict(nr.named_parameters())['agg_net.agg_impl.geometry_fc.2.weight'].data.mul_(1.5)    # bypasses the version counters
    assert torch.equal(nr.hot().wc, stepped)
    nr.invalidate_packed()
    assert torch.equal(nr.hot().wc, packed('coarse')) and not torch.equal(nr.hot().wc, stepped)
    assert torch.equal(nr.hot_for_training().can_dev['coarse'], canon('coarse'))
