"""Frame metrics of the validation pass (graspnerf_amd/metrics.py, csrc/gnr_metrics.hip, include/gnr.h gnr_frame_metrics).

CPU cases run the host twin (metrics.frame_metrics_host), `gpu` cases the kernels through the C ABI.
* PSNR / depth MAE against the reference's own compute_psnr / compute_mae / color_map_backward, recorded for seeded frames in
  tests/golden/golden_frame_metrics.npz (tools/make_metric_goldens.py; frames = synth.synth_metric_frames).
  PSNR 1e-4 dB absolute: the reference sums in float32 -- pairwise, relative error <= log2(n) 2^-24 ~ 1.2e-6 = 5e-6 dB -- and
  rounds its value to float32 (2.4e-6 near 40 dB); the device sum is exact: ~10x margin.  MAE 1e-5 relative by the same bound on
  the reference's float32 mean.
* SSIM against a float64 statement with scipy.ndimage.uniform_filter (the computation of skimage's structural_similarity with
  win_size=11, multichannel=True, data_range=255), 1e-9 absolute: a few ulps of double per S, and any summation order over
  n <= 4.4e5 terms adds at most n 2^-53 ~ 5e-11.
Shapes: the smallest at which the tiling can go wrong -- 11x11 = exactly one SSIM window; 12x37 narrower than any tile, odd;
33x64; 96x128 with eval_margin_ratio 1.0 and 0.8 (crop offsets 9 and 12); B = 1 and 3, n_pred = 1 and 2; 288x512 B = 2 as a size check."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, metrics
from graspnerf_amd.synth import synth_metric_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_frame_metrics.npz')))
CASES = [(int(h), int(w), float(r), int(B), int(n), bool(i)) for h, w, r, B, n, i in G['cases']]
SMALL = [ci for ci, c in enumerate(CASES) if c[0] * c[1] < 288 * 512]
PSNR_TOL, MAE_RTOL, SSIM_TOL = 1e-4, 1e-5, 1e-9
_cache = {}


def case(ci):
    """Frames, margins, recorded values and the scipy SSIM statement of one case (made once per session)."""
    if ci not in _cache:
        h, w, ratio, B, n, identical = CASES[ci]
        gt, preds, dpr, dgt = synth_metric_frames(int(G['seeds'][ci]), h, w, B, n, identical)
        hm, wm = metrics.crop_margins(h, w, ratio)
        assert [hm, wm] == G[f'margins{ci}'].tolist()
        want_ssim = h - 2 * hm >= 11 and w - 2 * wm >= 11
        ssim = np.array([[ssim_statement(quantise(crop(gt[b], h, w, hm, wm)), quantise(crop(p[b], h, w, hm, wm))) for p in preds]
                         for b in range(B)]) if want_ssim else None
        _cache[ci] = dict(h=h, w=w, B=B, n=n, hm=hm, wm=wm, gt=gt, preds=preds, dpr=dpr, dgt=dgt, psnr=G[f'psnr{ci}'], mae=G[f'mae{ci}'],
                          ssim=ssim)
    return _cache[ci]


def crop(img, h, w, hm, wm):
    return img.reshape(h, w, 3)[hm:h - hm, wm:w - wm]


def quantise(rgb):
    """numpy's statement of color_map_backward (utils/base_utils.py:496-499)"""
    return np.clip(rgb * 255, a_min=0, a_max=255).astype(np.uint8)


def ssim_statement(x, y):
    """float64 SSIM of two uint8 images [H,W,3]: 11x11 box means, sample covariance, mean over the frame without its 5-pixel border
    (where the filter's border mode does not reach), mean of the channels."""
    from scipy.ndimage import uniform_filter
    C1, C2, cov_norm = (0.01 * 255) ** 2, (0.03 * 255) ** 2, 121 / 120
    ms = []
    for c in range(3):
        a, b = x[..., c].astype(np.float64), y[..., c].astype(np.float64)
        ux, uy, uxx, uyy, uxy = (uniform_filter(v, size=11) for v in (a, b, a * a, b * b, a * b))
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        ms.append(S[5:-5, 5:-5].mean())
    return float(np.mean(ms))


def check_values(res, c, what):
    """res float64 [B, 2 n + 1] (psnr, ssim, mae) against the recorded reference values and the SSIM statement."""
    n = c['n']
    psnr, ssim, mae = res[:, :n], res[:, n:2 * n], res[:, 2 * n]
    inf = np.isposinf(c['psnr'])
    print(what, 'psnr', psnr.tolist(), 'max|d|', np.abs(psnr[~inf] - c['psnr'][~inf]).max(initial=0.0), 'mae rel', np.abs(mae / c['mae'] - 1).max())
    assert np.array_equal(np.isposinf(psnr), inf), what
    assert np.abs(psnr[~inf] - c['psnr'][~inf]).max(initial=0.0) <= PSNR_TOL, what
    assert np.abs(mae - c['mae']).max() <= MAE_RTOL * np.abs(c['mae']).max(), what
    if c['ssim'] is not None:
        print(what, 'ssim', ssim.tolist(), 'max|d|', np.abs(ssim - c['ssim']).max())
        assert np.abs(ssim - c['ssim']).max() <= SSIM_TOL, what
    else:
        assert np.isnan(ssim).all(), what


def host(c, ssim=None):
    return metrics.frame_metrics_host(c['gt'], c['preds'], c['dpr'], c['dgt'], c['h'], c['w'], c['hm'], c['wm'],
                                      ssim=c['ssim'] is not None if ssim is None else ssim)


def device(c, ssim=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return metrics.frame_metrics_device(t(c['gt']), [t(p) for p in c['preds']], t(c['dpr']), t(c['dgt']), c['h'], c['w'], c['hm'], c['wm'],
                                        ssim=c['ssim'] is not None if ssim is None else ssim)


# ---- host twin (CPU) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci', SMALL)
def test_host_twin_matches_reference_values_and_ssim_statement(ci):
    c = case(ci)
    check_values(host(c), c, f'host case {ci} {CASES[ci]}')


def test_host_twin_identical_images():
    """+inf PSNR as numpy gives it, SSIM exactly 1.0."""
    ci = next(i for i, c in enumerate(CASES) if c[5])
    res = host(case(ci))
    assert np.isposinf(res[0, 0]) and res[0, 1] == 1.0


def test_host_twin_non_finite_pixel_gives_nan_for_that_image_only():
    c = dict(case(2))
    preds = [p.copy() for p in c['preds']]
    preds[1][0, 700, 1] = np.nan
    res = host(dict(c, preds=preds))
    assert np.isnan(res[0, 1]) and np.isnan(res[0, 3]) and np.isfinite(res[0, [0, 2, 4]]).all()


def test_frame_metrics_keys_and_refusals_on_the_host():
    """The public function on host tensors: the reference's keys plus ssim_*, values per scene; a crop below the SSIM window is refused
    naming the window; PSNR and MAE alone take any size."""
    c = case(1)                                                         # 12 x 37, B = 3, two predictions
    t = torch.from_numpy
    out = {'pixel_colors_gt': t(c['gt']), 'pixel_colors_nr': t(c['preds'][0]), 'pixel_colors_nr_fine': t(c['preds'][1]),
           'render_depth': t(c['dpr'])}
    data = {'que_imgs_info': {'imgs': torch.zeros(3, 3, c['h'], c['w']), 'true_depth': t(c['dgt'])[:, None]}}
    m = metrics.frame_metrics(out, data)
    assert set(m) == {'psnr_nr', 'psnr_nr_fine', 'depth_mae', 'ssim_nr', 'ssim_nr_fine'}
    want = host(c)
    for k, col in (('psnr_nr', 0), ('psnr_nr_fine', 1), ('ssim_nr', 2), ('ssim_nr_fine', 3), ('depth_mae', 4)):
        assert m[k].dtype == torch.float64 and np.array_equal(m[k].numpy(), want[:, col]), k
    per_scene = [metrics.frame_metrics({k: v[b:b + 1] for k, v in out.items()},
                                       {'que_imgs_info': {'imgs': data['que_imgs_info']['imgs'], 'true_depth': data['que_imgs_info']['true_depth'][b:b + 1]}})
                 for b in range(3)]
    assert all(torch.equal(per_scene[b][k], m[k][b:b + 1]) for b in range(3) for k in m)
    del out['pixel_colors_nr_fine']
    assert set(metrics.frame_metrics(out, data, ssim=False)) == {'psnr_nr', 'depth_mae'}
    with pytest.raises(_lib.GnrError, match='11 x 11'):
        metrics.frame_metrics(out, data, eval_margin_ratio=0.8)         # 12 rows -> 10 after the crop
    small = case(8)                                                     # 5 x 7
    o = {'pixel_colors_gt': t(small['gt']), 'pixel_colors_nr': t(small['preds'][0]), 'render_depth': t(small['dpr'])}
    d = {'que_imgs_info': {'imgs': torch.zeros(1, 3, 5, 7), 'true_depth': t(small['dgt'])[:, None]}}
    with pytest.raises(_lib.GnrError, match='window'):
        metrics.frame_metrics(o, d)
    m = metrics.frame_metrics(o, d, ssim=False)
    assert abs(float(m['psnr_nr']) - small['psnr'][0, 0]) <= PSNR_TOL
    assert metrics.name2key_metrics['loss_vgn']({}) == 1e6 and metrics.name2key_metrics['psnr_nr']({'psnr_nr': np.array([1.0, 3.0])}) == 2.0


def test_entry_point_refuses_before_touching_the_device():
    """Null pointers, bad sizes, a crop below the SSIM window and a short workspace: refused with the documented code and the text in
    gnr_last_error.  Every call here is one that validation refuses (fake pointers); runs without a GPU."""
    L = _lib.lib()
    P = 4096
    ptrs = (C.c_void_p * 2)(P, P)
    need = L.gnr_frame_metrics_workspace_bytes(2, 33, 64, 2, 0, 0, 1)
    assert need > L.gnr_frame_metrics_workspace_bytes(2, 33, 64, 2, 0, 0, 0) > 0
    base = dict(gt=P, preds=ptrs, n_pred=2, depth_pr=P, depth_gt=P, B=2, h=33, w=64, hm=0, wm=0, ssim=1, out=P, ws=P, ws_bytes=need, stream=None)

    def refused(code, text, **kw):
        rc = L.gnr_frame_metrics(*dict(base, **kw).values())
        msg = L.gnr_last_error().decode()
        assert rc == code and text in msg, (kw, rc, msg)

    for k in ('gt', 'preds', 'depth_pr', 'depth_gt', 'out', 'ws'):
        refused(_lib.GNR_ERR_ARG, 'null pointer', **{k: None})
    refused(_lib.GNR_ERR_ARG, 'null prediction pointer', preds=(C.c_void_p * 2)(P, None))
    refused(_lib.GNR_ERR_ARG, 'n_pred', n_pred=0)
    refused(_lib.GNR_ERR_ARG, 'n_pred', n_pred=5)
    refused(_lib.GNR_ERR_SHAPE, 'h, w >= 1', h=0)
    refused(_lib.GNR_ERR_SHAPE, 'B in 1..65535', B=0)
    refused(_lib.GNR_ERR_SHAPE, 'margins', hm=17)
    refused(_lib.GNR_ERR_SHAPE, '11 x 11 window', h=10)
    refused(_lib.GNR_ERR_SHAPE, '11 x 11 window', hm=12)                 # 33 - 24 = 9 rows after cropping
    refused(_lib.GNR_ERR_SHAPE, '11 x 11 window', w=12, wm=1)
    refused(_lib.GNR_ERR_WORKSPACE, 'workspace', ws_bytes=need - 1)
    assert L.gnr_frame_metrics_workspace_bytes(1, 10, 64, 1, 0, 0, 1) == 0 and b'window' in L.gnr_last_error()
    assert L.gnr_frame_metrics_workspace_bytes(1, 10, 64, 1, 0, 0, 0) > 0    # PSNR and MAE alone take any h, w >= 1


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('ci', range(len(CASES)))
def test_kernel_matches_reference_values_ssim_statement_and_host_twin(ci):
    c = case(ci)
    a, b = device(c), device(c)
    assert a.dtype == torch.float64 and a.is_cuda
    same = torch.equal(a.view(torch.int64), b.view(torch.int64))          # bits, so that NaN == NaN
    res = a.cpu().numpy()
    check_values(res, c, f'device case {ci} {CASES[ci]}')
    assert same, 'two runs of the kernels returned different bits'
    tw = host(c)
    n = c['n']
    fin = np.isfinite(tw[:, :n])
    assert np.array_equal(np.isposinf(res[:, :n]), np.isposinf(tw[:, :n]))
    assert np.abs(res[:, :n][fin] - tw[:, :n][fin]).max(initial=0.0) <= PSNR_TOL
    assert np.abs(res[:, 2 * n] - tw[:, 2 * n]).max() <= MAE_RTOL * np.abs(tw[:, 2 * n]).max()
    if c['ssim'] is not None:
        assert np.abs(res[:, n:2 * n] - tw[:, n:2 * n]).max() <= SSIM_TOL
        nos = device(c, ssim=False).cpu().numpy()                         # PSNR / MAE do not depend on the SSIM launch
        assert np.array_equal(nos[:, :n], res[:, :n]) and np.array_equal(nos[:, 2 * n], res[:, 2 * n]) and np.isnan(nos[:, n:2 * n]).all()


@pytest.mark.gpu
def test_kernel_identical_images_and_non_finite_pixels():
    ci = next(i for i, c in enumerate(CASES) if c[5])
    res = device(case(ci)).cpu().numpy()
    assert np.isposinf(res[0, 0]) and res[0, 1] == 1.0
    c = dict(case(2))
    preds = [p.copy() for p in c['preds']]
    preds[1][0, 700, 1] = np.inf
    res = device(dict(c, preds=preds)).cpu().numpy()
    assert np.isnan(res[0, 1]) and np.isnan(res[0, 3]) and np.isfinite(res[0, [0, 2, 4]]).all()
    gt = c['gt'].copy()
    gt[0, 5, 0] = np.nan                                                  # the ground truth is part of every image pair
    res = device(dict(c, gt=gt)).cpu().numpy()
    assert np.isnan(res[0, :4]).all() and np.isfinite(res[0, 4])


@pytest.mark.gpu
def test_quantisation_is_bit_exact():
    """A frame of the 256 values k / 255 and their two fp32 neighbours each (where x * 255 sits on, just below and just above an
    integer): the integer sum of squared differences behind the device's PSNR equals numpy's color_map_backward statement."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255))
    vals = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.float32([-0.0, 1.5, -3.0])]).astype(np.float32)
    h, w = 12, 65                                                         # 780 pixels = 2340 values >= 3 x 771
    rng = np.random.Generator(np.random.PCG64(7))
    gt = rng.permutation(np.resize(vals, h * w * 3)).reshape(1, h * w, 3).astype(np.float32)
    pr = rng.permutation(np.resize(vals, h * w * 3)).reshape(1, h * w, 3).astype(np.float32)
    e = quantise(gt).astype(np.int64) - quantise(pr).astype(np.int64)
    sse = int((e * e).sum())
    t = lambda a: torch.from_numpy(a).cuda()
    z = torch.zeros(1, h * w, device='cuda')
    res = metrics.frame_metrics_device(t(gt), [t(pr)], z, z.reshape(1, h, w), h, w, 0, 0, ssim=False).cpu().numpy()
    got = 255.0 ** 2 / 10.0 ** (res[0, 0] / 10.0) * (3 * h * w)           # the SSE back from the PSNR: integers are 1 apart, 1e-9 of it
    print('sse', sse, 'from the device', got)
    assert round(got) == sse and abs(got - sse) < 1e-3


@pytest.mark.gpu
def test_kernel_launches_are_timed_under_their_labels():
    c = case(2)
    _lib.timing_begin('gnr_frame_metrics')
    device(c)
    rec = _lib.timing_end()
    assert {k: v[0] for k, v in rec.items()} == {'k_frame_pixels@gnr_frame_metrics': 1, 'k_frame_ssim@gnr_frame_metrics': 1,
                                                 'k_frame_finish@gnr_frame_metrics': 1}
