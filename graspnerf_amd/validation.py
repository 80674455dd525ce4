"""Validation pass of the training loop (ref: src/nr/train/train_valid.py:11-46 ValidationEvaluator; the trainer runs it with
`val_losses + val_metrics`, train/trainer.py:166-169).

Every scene of this rank's shard goes through the eval forward (`data['eval'] = True`, under eval() and no_grad), the configured
loss terms (trainer.train_losses: where `loss_vgn`, the default key metric, comes from) and metrics.frame_metrics.  What a scene
contributes stays on the device: one float64 vector per scene is added into an accumulator of per-key sums and the scene count,
the ranks exchange it with ONE all-reduce, and ONE device-to-host copy per pass reads it back (the reference copies every term of
every scene to the host).  The `vis_img` image dumps of the reference (metrics.py:86-114: file output through skimage) are not built."""
import torch
import torch.distributed as dist

from . import metrics as _metrics
from .sharding import scene_shard


def better(prefer):
    """train/trainer.py:112-113"""
    if prefer not in ('higher', 'lower'):
        raise ValueError("key_metric_prefer must be 'higher' or 'lower'")
    return (lambda x, y: x > y) if prefer == 'higher' else (lambda x, y: x < y)


class Validator:
    def __init__(self, key_metric_name='loss_vgn', loss_fn=None, eval_margin_ratio=1.0, ssim=True, volume_depth=False):
        """loss_fn(out, data) -> dict of terms (default trainer.train_losses);  eval_margin_ratio, ssim: metrics.frame_metrics.
        volume_depth=True adds `volume_depth_mae` per scene: the volume's camera-space error -- the mean of |depth of the surface
        volume = 0 seen from the reference views (raycast.VolumeRaycaster) - true_depth| in metres over their pixels where the ray hit and
        true_depth > 0, NaN when there is none -- the quantity to put beside the render passes' depth_mae.  The ray cast and the reduction
        run on the device; the scene's box (six floats) is read on the host for the lattice's frame."""
        self.volume_depth, self._raycaster = bool(volume_depth), None
        if key_metric_name not in _metrics.name2key_metrics:
            raise KeyError(f'unknown key metric {key_metric_name!r} (metrics.name2key_metrics)')
        self.key_metric_name = key_metric_name
        self.loss_fn = loss_fn
        self.eval_margin_ratio, self.ssim = eval_margin_ratio, ssim

    def scene_terms(self, net, data, step=0):
        """One scene: eval forward, loss terms, frame metrics -> dict of tensors on the device of the outputs."""
        loss_fn = self.loss_fn
        if loss_fn is None:
            from .trainer import train_losses as loss_fn
        data = dict(data, eval=True, step=step)                             # train_valid.py:23-24
        out = net(data)
        terms = dict(loss_fn(out, data))
        terms.update(_metrics.frame_metrics(out, data, self.eval_margin_ratio, self.ssim))
        if self.volume_depth:
            terms['volume_depth_mae'] = self.volume_depth_mae(out, data)
        return terms

    def volume_depth_mae(self, out, data):
        """Device scalar [1]: see __init__.  The voxel centres are sample_volume's: bbox3d[0] + (i + 0.5) * (box edge / R)."""
        from .raycast import VolumeRaycaster, depth_mae
        ref = data['ref_imgs_info']
        if 'volume' not in out or 'true_depth' not in ref:
            raise KeyError("volume_depth=True needs cfg['sample_volume'] and ref_imgs_info['true_depth']")
        vol, true = out['volume'], ref['true_depth']
        if self._raycaster is None or self._raycaster.device != vol.device:
            self._raycaster = VolumeRaycaster(vol.device)
        R = vol.shape[-1]
        box = ref['bbox3d'].detach().to('cpu', torch.float64).numpy()
        scale = float(box[1, 0] - box[0, 0]) / R
        res = self._raycaster(vol, ref['poses'], ref['Ks'], true.shape[-2:], origin=box[0] + 0.5 * scale, scale=scale)
        return depth_mae(res['depth'][0], true[:, 0].to(torch.float32)).reshape(1)

    def __call__(self, net, scenes, step=0):
        """scenes: the GLOBAL sequence of `data` dicts (every rank passes the same list and evaluates its sharding.scene_shard).
        -> (results, key_metric_value): results[k] = mean of term k over all scenes of all ranks (train_valid.py:38-46; the
        reference keeps the per-scene arrays and its logger takes their means), the key metric by metrics.name2key_metrics --
        `loss_vgn` missing gives 1e6."""
        ready = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if ready else (0, 1)
        lo, hi = scene_shard(len(scenes), rank, world)
        modes = [(m, m.training) for m in net.modules()]
        keys, acc = None, None
        net.eval()
        try:
            with torch.no_grad():
                for i in range(lo, hi):
                    terms = self.scene_terms(net, scenes[i], step)
                    if keys is None:
                        keys = sorted(terms)
                    elif sorted(terms) != keys:
                        raise RuntimeError(f'validation scene {i} produced other terms than scene {lo}')
                    vec = torch.stack([terms[k].detach().to(torch.float64).mean() for k in keys] + [torch.ones((), dtype=torch.float64, device=terms[keys[0]].device)])
                    acc = vec if acc is None else acc + vec
        finally:
            for m, flag in modes:                                           # (flags only: train() would walk the modules again)
                m.training = flag
        if world > 1:
            if len(scenes) < world:                                         # a rank without a scene learns the layout from rank 0 (which owns scene 0)
                box = [keys]
                dist.broadcast_object_list(box, src=0)
                keys = box[0]
            if acc is None:
                dev = next((p.device for p in net.parameters()), torch.device('cpu'))
                acc = torch.zeros(len(keys) + 1, dtype=torch.float64, device=dev)
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        if acc is None:
            return {}, _metrics.name2key_metrics[self.key_metric_name]({})
        host = acc.tolist()                                                 # the pass's one device-to-host copy
        n = host[-1]
        results = {k: v / n for k, v in zip(keys, host[:-1])}
        return results, _metrics.name2key_metrics[self.key_metric_name](results)
