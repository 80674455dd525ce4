"""Device image ingest (csrc/gnr_ingest.hip, graspnerf_amd/ingest.py): n uint8 frames -> float [n,3,H,W] in [0,1] with the
bits of the planner's host route, `resize_bilinear_u8(img, wh).astype(np.float32).transpose(2, 0, 1) / 255` (cv2.resize's
INTER_LINEAR fixed point, ref: src/nr/main.py:167-172, 191-192).  The coefficient tables are made on the host by the library
and are compared here, entry for entry, with the numpy helper resize_bilinear_u8 itself uses."""
import ctypes as C

import numpy as np
import pytest

from graspnerf_amd import _lib, ingest, planner


def _tables_numpy(src_hw, dst_hw):
    x = ingest.axis_tables(dst_hw[1], src_hw[1])
    y = ingest.axis_tables(dst_hw[0], src_hw[0])
    return np.concatenate([*x, *y])


def _check_tables(src_hw, dst_hw):
    blob = ingest.tables_host(src_hw, dst_hw)
    n = 4 * (dst_hw[0] + dst_hw[1])
    assert blob.size == n + 256 and blob.size * 4 == _lib.lib().gnr_ingest_tables_bytes(dst_hw[0], dst_hw[1])
    assert np.array_equal(blob[:n].astype(np.int64), _tables_numpy(src_hw, dst_hw)), (src_hw, dst_hw)
    return blob[n:]


def test_tables_equal_the_numpy_helper_for_every_small_size():
    for s in range(1, 41):
        for d in range(1, 41):
            _check_tables((s, 41 - s), (d, 41 - d))                          # both axes at once: rows s -> d, columns 41-s -> 41-d
            _check_tables((s, s), (d, d))


@pytest.mark.parametrize('s,d', [(360, 288), (640, 512), (720, 288), (45, 90), (7, 7)])
def test_tables_at_the_planner_sizes(s, d):
    lut = _check_tables((s, 2 * s), (d, 2 * d))
    assert np.array_equal(lut.view(np.float32), np.arange(256, dtype=np.float32) / np.float32(255))


def test_same_size_tables_reproduce_the_input():
    i0, i1, c0, c1 = ingest.axis_tables(9, 9)
    assert np.array_equal(i0, np.arange(9)) and np.all(c0 == 2048) and np.all(c1 == 0)


def test_refusals():
    L = _lib.lib()
    buf = (C.c_ubyte * 4096)()                                               # never dereferenced: every call below is refused first
    p = C.addressof(buf)
    ok = dict(frames=p, n=1, sh=4, sw=5, ch=3, rp=15, fp=60, tab=p, out=p, dh=3, dw=4)

    def call(**kw):
        a = {**ok, **kw}
        return L.gnr_ingest_u8(a['frames'], a['n'], a['sh'], a['sw'], a['ch'], a['rp'], a['fp'], a['tab'], a['out'], a['dh'], a['dw'], None)

    for k in ('frames', 'tab', 'out'):
        assert call(**{k: None}) == _lib.GNR_ERR_ARG
        assert b'null' in L.gnr_ingest_last_error()
    for ch in (0, 1, 2, 5):
        assert call(ch=ch, rp=64) == _lib.GNR_ERR_ARG
    assert b'channels' in L.gnr_ingest_last_error()
    for k in ('n', 'sh', 'sw', 'dh', 'dw'):
        assert call(**{k: 0}, rp=1 << 20) == _lib.GNR_ERR_SHAPE, k
        assert call(**{k: -3}, rp=1 << 20) == _lib.GNR_ERR_SHAPE, k
    for k in ('sh', 'sw', 'dh', 'dw'):
        assert call(**{k: 16385}, rp=1 << 20) == _lib.GNR_ERR_SHAPE, k
    assert call(rp=14) == _lib.GNR_ERR_ARG and b'row_pitch' in L.gnr_ingest_last_error()
    assert call(ch=4, rp=19) == _lib.GNR_ERR_ARG
    assert call(n=2, fp=59) == _lib.GNR_ERR_ARG and b'frame_pitch' in L.gnr_ingest_last_error()
    assert L.gnr_ingest_tables_host(4, 5, 3, 4, None) == _lib.GNR_ERR_ARG
    for bad in ((0, 5, 3, 4), (4, 16385, 3, 4), (4, 5, 0, 4), (4, 5, 3, 16385)):
        assert L.gnr_ingest_tables_host(*bad, p) == _lib.GNR_ERR_SHAPE
    assert L.gnr_ingest_tables_bytes(0, 4) == 0 and L.gnr_ingest_tables_bytes(3, 16385) == 0
    with pytest.raises(_lib.GnrError):
        ingest.tables_host((4, 5), (0, 4))


# ---- on the device ---------------------------------------------------------------------------------------------------
def _host(img, wh):
    return planner.resize_bilinear_u8(img[:, :, :3], wh).astype(np.float32).transpose(2, 0, 1) / 255


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope='module')
def dev_ingest():
    return ingest.DeviceIngest('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', [((5, 7), (3, 4)), ((6, 4), (11, 9)), ((9, 9), (9, 9)), ((1, 1), (4, 4)),
                                           ((36, 64), (29, 51)), ((360, 640), (288, 512))])
def test_device_ingest_is_bit_identical(dev_ingest, src_hw, dst_hw):
    import torch
    rng = np.random.default_rng(src_hw[0] * 1000 + dst_hw[1])
    img = rng.integers(0, 256, (*src_hw, 3), dtype=np.uint8)
    out = dev_ingest(torch.from_numpy(img)[None].cuda(), (dst_hw[1], dst_hw[0]))
    assert out.shape == (1, 3, *dst_hw)
    assert _same_bits(out[0].cpu().numpy(), _host(img, (dst_hw[1], dst_hw[0])))


@pytest.mark.gpu
def test_device_ingest_frames_channels_pitch_and_extremes(dev_ingest):
    import torch
    rng = np.random.default_rng(7)
    # n = 3 frames in one call, into a caller's buffer
    imgs = rng.integers(0, 256, (3, 36, 64, 3), dtype=np.uint8)
    buf = torch.full((3, 3, 29, 52), -1.0, device='cuda:0')
    out = dev_ingest(torch.from_numpy(imgs).cuda(), (52, 29), out=buf)
    assert out is buf
    for i in range(3):
        assert _same_bits(out[i].cpu().numpy(), _host(imgs[i], (52, 29))), i
    # RGBA with a random alpha: the 4th channel is ignored (imread(...)[:, :, :3])
    rgba = rng.integers(0, 256, (2, 10, 13, 4), dtype=np.uint8)
    out = dev_ingest(torch.from_numpy(rgba).cuda(), (9, 7))
    for i in range(2):
        assert _same_bits(out[i].cpu().numpy(), _host(rgba[i], (9, 7))), i
    # padded rows (and a padded frame pitch), the pad bytes at 255: they must not leak into the border pixels
    padded = np.full((2, 12 + 3, 17 + 5, 3), 255, np.uint8)
    padded[:, :12, :17] = rng.integers(0, 64, (2, 12, 17, 3), dtype=np.uint8)
    view = torch.from_numpy(padded).cuda()[:, :12, :17]
    assert not view.is_contiguous()
    out = dev_ingest(view, (23, 19))
    for i in range(2):
        assert _same_bits(out[i].cpu().numpy(), _host(padded[i, :12, :17], (23, 19))), i
    # all-255 and all-0 images: exactly 1.0 and 0.0 everywhere, also when upscaling
    for val in (255, 0):
        const = np.full((1, 21, 30, 3), val, np.uint8)
        for wh in ((16, 12), (47, 33)):
            out = dev_ingest(torch.from_numpy(const).cuda(), wh).cpu().numpy()
            assert _same_bits(out[0], _host(const[0], wh)) and np.all(out == np.float32(val / 255))
    with pytest.raises(ValueError):
        dev_ingest(torch.from_numpy(imgs).cuda().permute(0, 3, 1, 2), (52, 29))              # planar frames are not interleaved
    with pytest.raises(_lib.GnrError):
        dev_ingest(torch.from_numpy(imgs[..., :2].copy()).cuda(), (52, 29))                   # two channels
