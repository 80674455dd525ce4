"""Frame metrics of a validation pass (ref: src/nr/network/metrics.py:14-84 PSNR_SSIM, :121-145 name2key_metrics).

`frame_metrics` takes the output dict of an eval forward with a full query frame and its `data`.  Device tensors go through the
HIP kernels of csrc/gnr_metrics.hip (include/gnr.h gnr_frame_metrics: B frames in three launches, float64 results that stay on
the device); host tensors go through `frame_metrics_host`, a numpy statement of the same formulas -- the kernel's host twin, as
planner.resize_bilinear_u8 is for the ingest kernel (the CPU tests and the gloo tests run it).  Both return the reference's keys
(`psnr_nr`, `psnr_nr_fine` when the fine level exists, `depth_mae`) and, as additions, `ssim_nr` / `ssim_nr_fine`: the value the
reference computes for its PSNR_SSIM class (metrics.py:71) and drops."""
import ctypes as C

import numpy as np
import torch

from . import _lib

WIN = 11                                                   # SSIM window (structural_similarity(win_size=11))
_SUFFIXES = ('nr', 'nr_fine')                              # metrics.py:41-42,76 (the 'dr' predictions do not exist on this path)


def crop_margins(h, w, eval_margin_ratio=1.0):
    """metrics.py:54-55"""
    return int(h * (1 - eval_margin_ratio)) // 2, int(w * (1 - eval_margin_ratio)) // 2


def _quantise(rgb):
    """color_map_backward (utils/base_utils.py:496-499) on float32: one multiply by 255, clip, truncation to uint8.
    -> uint8 image, whether every value was finite (a non-finite value is stored as 0 and makes the image's metrics NaN)."""
    rgb = np.asarray(rgb, np.float32)
    ok = np.isfinite(rgb)
    s = np.clip(np.where(ok, rgb, np.float32(0)) * np.float32(255), 0, 255).astype(np.uint8)
    return s, bool(ok.all())


def _window_sums(a):
    """a int64 [H,W] -> sums over every 11x11 window [H-10,W-10], exact."""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[WIN:, WIN:] - c[:-WIN, WIN:] - c[WIN:, :-WIN] + c[:-WIN, :-WIN]


def ssim_u8(x, y):
    """skimage.metrics.structural_similarity(x, y, win_size=11, multichannel=True, data_range=255) on uint8 [H,W,3]: per channel
    the 11x11 box means from exact integer window sums, S in float64, its mean over the frame without the 5-pixel border, then the
    mean of the channels."""
    if x.shape[0] < WIN or x.shape[1] < WIN:
        raise ValueError(f'SSIM needs a cropped frame of at least {WIN} x {WIN} pixels (the {WIN} x {WIN} window), got {x.shape[0]} x {x.shape[1]}')
    C1, C2, cov_norm = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2, 121.0 / 120.0
    ms = []
    for c in range(3):
        a, b = x[..., c].astype(np.int64), y[..., c].astype(np.int64)
        ux, uy, uxx, uyy, uxy = (_window_sums(v) / 121.0 for v in (a, b, a * a, b * b, a * b))
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        ms.append(S.sum() / S.size)
    return (ms[0] + ms[1] + ms[2]) / 3.0


def frame_metrics_host(gt, preds, depth_pr, depth_gt, h, w, h_margin=0, w_margin=0, ssim=True):
    """The formulas of gnr_frame_metrics in numpy.  gt [B,h*w,3], preds: list of [B,h*w,3], depth_pr [B,h*w], depth_gt [B,h,w]
    -> float64 [B, 2 * len(preds) + 1] = psnr per prediction, ssim per prediction (NaN when not asked for), depth_mae."""
    gt = np.asarray(gt, np.float32)
    B, n = gt.shape[0], len(preds)
    ch, cw = h - 2 * h_margin, w - 2 * w_margin
    if ch < 1 or cw < 1 or h_margin < 0 or w_margin < 0:
        raise ValueError('the crop margins leave no pixel')
    out = np.full((B, 2 * n + 1), np.nan, np.float64)
    crop = lambda a: a.reshape(h, w, 3)[h_margin:h - h_margin, w_margin:w - w_margin]
    with np.errstate(divide='ignore', invalid='ignore'):
        for b in range(B):
            d = np.abs(np.asarray(depth_pr, np.float32)[b].reshape(h, w) - np.asarray(depth_gt, np.float32)[b].reshape(h, w))
            out[b, 2 * n] = d.astype(np.float64).sum() / (float(h) * float(w))
            qg, g_ok = _quantise(crop(gt[b]))
            for p, pr in enumerate(preds):
                qp, p_ok = _quantise(crop(np.asarray(pr, np.float32)[b]))
                s = ssim_u8(qg, qp) if ssim else np.nan                # (refuses a crop below the window, finite or not)
                if not (g_ok and p_ok):
                    continue
                e = qg.astype(np.int64) - qp.astype(np.int64)
                mse = float((e * e).sum()) / (3.0 * ch * cw)
                out[b, p] = np.inf if mse == 0.0 else 10.0 * np.log10(255.0 * 255.0 / mse)
                out[b, n + p] = s
    return out


def frame_metrics_device(gt, preds, depth_pr, depth_gt, h, w, h_margin=0, w_margin=0, ssim=True):
    """gnr_frame_metrics on the current stream: contiguous float32 device tensors in, float64 [B, 2 * len(preds) + 1] on the device
    out (layout of frame_metrics_host).  Nothing waits for the device."""
    L = _lib.lib()
    B, n = gt.shape[0], len(preds)
    ts = [gt, depth_pr, depth_gt] + list(preds)
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == gt.device for t in ts):
        raise ValueError('frame_metrics_device: contiguous float32 tensors on one device')
    if gt.shape != (B, h * w, 3) or any(p.shape != gt.shape for p in preds) or depth_pr.numel() != B * h * w or depth_gt.numel() != B * h * w:
        raise ValueError(f'frame_metrics_device: gt / predictions [B,{h * w},3], depths of B * {h} * {w} values')
    need = L.gnr_frame_metrics_workspace_bytes(B, h, w, n, h_margin, w_margin, int(bool(ssim)))
    with torch.cuda.device(gt.device):
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=gt.device)     # (the caching allocator: stream-ordered reuse)
        out = torch.empty(B, 2 * n + 1, dtype=torch.float64, device=gt.device)
        ptrs = (C.c_void_p * max(n, 1))(*[p.data_ptr() for p in preds])
        rc = L.gnr_frame_metrics(gt.data_ptr(), ptrs, n, depth_pr.data_ptr(), depth_gt.data_ptr(), B, h, w, h_margin, w_margin,
                                 int(bool(ssim)), out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                 C.c_void_p(torch.cuda.current_stream(gt.device).cuda_stream))
    _lib.check(rc, 'gnr_frame_metrics')
    return out


def frame_metrics(out, data, eval_margin_ratio=1.0, ssim=True):
    """PSNR_SSIM.__call__ (metrics.py:40-84) on the outputs of an eval forward whose query view is the full frame.
    out: `pixel_colors_gt`, `pixel_colors_nr` [B,h*w,3] (`pixel_colors_nr_fine` with hierarchical sampling), `render_depth` [B,h*w];
    data: `que_imgs_info` with `imgs` [..,3,h,w] and `true_depth` [B,1,h,w] -- B = 1 for one scene, the scene-major stacks for several.
    -> {'psnr_nr', 'psnr_nr_fine', 'depth_mae', 'ssim_nr', 'ssim_nr_fine'}: float64 [B] on the device of the outputs."""
    que = data['que_imgs_info']
    h, w = (int(v) for v in que['imgs'].shape[-2:])
    depth_gt = que['true_depth']
    gt = out['pixel_colors_gt']
    B = gt.shape[0]
    names = [s for s in _SUFFIXES if 'pixel_colors_' + s in out]
    if names[:1] != ['nr']:
        raise KeyError('pixel_colors_nr')
    if gt.shape[1] != h * w:
        raise ValueError(f'frame_metrics needs the full query frame: {gt.shape[1]} rays for {h} x {w} pixels')
    hm, wm = crop_margins(h, w, eval_margin_ratio)
    if ssim and (h - 2 * hm < WIN or w - 2 * wm < WIN):
        raise _lib.GnrError(f'frame_metrics: SSIM needs a cropped frame of at least {WIN} x {WIN} pixels (the {WIN} x {WIN} window), '
                            f'got {h - 2 * hm} x {w - 2 * wm}')
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    preds = [f32(out['pixel_colors_' + s]) for s in names]
    depth_pr, depth_gt = f32(out['render_depth']).reshape(B, h * w), f32(depth_gt).reshape(B, h, w)
    if gt.is_cuda:
        res = frame_metrics_device(f32(gt), preds, depth_pr, depth_gt, h, w, hm, wm, ssim)
    else:
        res = torch.from_numpy(frame_metrics_host(f32(gt).numpy(), [p.numpy() for p in preds], depth_pr.numpy(), depth_gt.numpy(),
                                                  h, w, hm, wm, ssim))
    n = len(names)
    m = {'psnr_' + s: res[:, i] for i, s in enumerate(names)}
    m['depth_mae'] = res[:, 2 * n]
    if ssim:
        m.update({'ssim_' + s: res[:, n + i] for i, s in enumerate(names)})
    return m


# ---- key metrics of a validation pass (metrics.py:121-145): results hold one value per scene -------------------------------------
def _mean_of(key):
    return lambda results: float(np.mean(results[key]))


def _loss_vgn(results):
    return float(np.mean(results['loss_vgn'])) if 'loss_vgn' in results else 1e6


name2key_metrics = {'psnr_nr': _mean_of('psnr_nr'), 'psnr_nr_fine': _mean_of('psnr_nr_fine'), 'depth_mae': _mean_of('depth_mae'),
                    'loss_vgn': _loss_vgn, 'sdf_mae': _mean_of('sdf_mae')}
