"""Record the reference's frame metrics for seeded frames -> tests/golden/golden_frame_metrics.npz.

Imports the reference's compute_psnr, compute_mae (network/metrics.py) and color_map_backward (utils/base_utils.py) through
tools/ref_import.py and runs them exactly as written, the way PSNR_SSIM.__call__ strings them together (metrics.py:47-59,79-83).
`skimage` (and other packages the module pulls in without using them here) is absent in the build container: stand-in modules
satisfy the imports of network/metrics.py -- imsave and structural_similarity are never called -- as ref_import does for `easydict`.
The file holds seeds, shapes, margins and the recorded values only; tests/test_frame_metrics.py draws the same frames with
graspnerf_amd.synth.synth_metric_frames (PCG64 streams: predictions in [-0.1, 1.1], so both clips of the quantisation are hit).
Build container only: never imported by the product, the GPU tests, smoke() or bench.py.   python tools/make_metric_goldens.py"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from graspnerf_amd.synth import synth_metric_frames  # noqa: E402

# (h, w, eval_margin_ratio, B, n_pred, identical): tests/test_frame_metrics.py documents why these shapes
CASES = [(11, 11, 1.0, 1, 1, 0), (12, 37, 1.0, 3, 2, 0), (33, 64, 1.0, 1, 2, 0), (96, 128, 1.0, 3, 1, 0), (96, 128, 0.8, 1, 2, 0),
         (96, 128, 0.8, 3, 2, 0), (33, 64, 1.0, 1, 1, 1), (288, 512, 1.0, 2, 2, 0), (5, 7, 1.0, 1, 1, 0)]


def import_reference_metrics():
    """network/metrics.py pulls in the loss and drawing modules and, through them, packages that are absent here and that the three
    functions never touch (skimage, pyquaternion, cv2, open3d, ...): each missing one gets an empty stand-in module."""
    class _Any(types.ModuleType):
        __path__ = []

        def __getattr__(self, k):
            return None
    from ref_import import import_reference
    import_reference()
    for _ in range(64):
        try:
            from network import metrics
            from utils.base_utils import color_map_backward
            return metrics.compute_psnr, metrics.compute_mae, color_map_backward
        except ModuleNotFoundError as e:
            for m in [k for k in sys.modules if k.split('.')[0] in ('network', 'utils')]:
                del sys.modules[m]                         # half-imported reference modules: import them again
            sys.modules[e.name] = _Any(e.name)
    raise RuntimeError('could not import network.metrics')


def main():
    compute_psnr, compute_mae, color_map_backward = import_reference_metrics()
    rec = {'cases': np.array(CASES, np.float64), 'seeds': np.arange(100, 100 + len(CASES))}
    for ci, (h, w, ratio, B, n_pred, identical) in enumerate(CASES):
        gt, preds, depth_pr, depth_gt = synth_metric_frames(100 + ci, h, w, B, n_pred, bool(identical))
        h_margin, w_margin = int(h * (1 - ratio)) // 2, int(w * (1 - ratio)) // 2            # metrics.py:54-55
        psnr, mae = np.zeros((B, n_pred)), np.zeros(B)
        with np.errstate(divide='ignore'):
            for b in range(B):
                g = color_map_backward(gt[b].reshape(h, w, 3))[h_margin:h - h_margin, w_margin:w - w_margin]
                for p in range(n_pred):
                    q = color_map_backward(preds[p][b].reshape(h, w, 3))[h_margin:h - h_margin, w_margin:w - w_margin]
                    psnr[b, p] = compute_psnr(g, q)
                mae[b] = compute_mae(depth_pr[b].reshape(h, w), depth_gt[b])
        rec[f'psnr{ci}'], rec[f'mae{ci}'], rec[f'margins{ci}'] = psnr, mae, np.array([h_margin, w_margin])
        print(ci, (h, w, ratio, B, n_pred), psnr.round(3).tolist(), mae.tolist())
    assert np.isposinf(rec['psnr6'][0, 0])
    np.savez(os.path.join(ROOT, 'tests', 'golden', 'golden_frame_metrics.npz'), **rec)


if __name__ == '__main__':
    main()
