"""Image ingest of the planner (ref: src/nr/main.py:167-172, 191-192): uint8 frames of any size -> the network's input,
float [n,3,H,W] in [0,1], with cv2.resize's INTER_LINEAR fixed point.  `axis_tables` is the per-axis half of
planner.resize_bilinear_u8 (host numpy); `DeviceIngest` runs the same arithmetic for all frames in one HIP launch
(csrc/gnr_ingest.hip), stream-ordered and capturable in a hipGraph."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def axis_tables(dn, sn):
    """One axis of cv2.resize(INTER_LINEAR) from sn to dn pixels -> (i0, i1, c0, c1), int64 [dn]: the two source indices of
    every destination pixel (half-pixel centres in float64, the weight rounded to float32, both borders clamped with weight
    0) and their 11-bit coefficients saturate_cast<short>(rint((1 - w) * 2^11)), saturate_cast<short>(rint(w * 2^11))."""
    f = (np.arange(dn, dtype=np.float64) + 0.5) * (sn / dn) - 0.5
    i0 = np.floor(f).astype(np.int64)
    w = (f - i0).astype(np.float32)
    lo = i0 < 0
    i0[lo], w[lo] = 0, 0.0
    hi = i0 >= sn - 1
    i0[hi], w[hi] = sn - 1, 0.0
    i1 = np.minimum(i0 + 1, sn - 1)
    c1 = np.clip(np.rint(w.astype(np.float64) * 2048), -32768, 32767).astype(np.int64)      # saturate_cast<short>(w * 2^11)
    c0 = np.clip(np.rint((1.0 - w.astype(np.float64)) * 2048), -32768, 32767).astype(np.int64)
    return i0, i1, c0, c1


def tables_host(src_hw, dst_hw):
    """The blob of gnr_ingest_tables_host as a numpy int32 array: x0 x1 a0 a1 [dst_w each], y0 y1 b0 b1 [dst_h each], then
    the bits of float32(i) / float32(255), i = 0..255.  No device work."""
    L = _lib.lib()
    (sh, sw), (dh, dw) = (int(v) for v in src_hw), (int(v) for v in dst_hw)
    nbytes = L.gnr_ingest_tables_bytes(dh, dw)
    blob = np.empty(max(nbytes, 4) // 4, np.int32)
    rc = L.gnr_ingest_tables_host(sh, sw, dh, dw, blob.ctypes.data_as(C.c_void_p) if nbytes else None)
    _lib.check(rc, 'gnr_ingest_tables_host')
    return blob


class DeviceIngest:
    """uint8 frames on the device -> float [n,3,H,W] in [0,1]: bit-identical to
    `resize_bilinear_u8(img, wh).astype(np.float32).transpose(2, 0, 1) / 255` per frame.  The coefficient tables are made on
    the host and uploaded once per (src_h, src_w, dst_h, dst_w); a call is one kernel launch on the current stream."""

    def __init__(self, device='cuda:0'):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.GnrError('the HIP image ingest needs a ROCm GPU; there is no CPU fallback')
        d = torch.device(device)
        self.device = d if d.index is not None else torch.device(d.type, torch.cuda.current_device())
        self._tables = {}

    def tables(self, src_hw, dst_hw):
        key = (int(src_hw[0]), int(src_hw[1]), int(dst_hw[0]), int(dst_hw[1]))
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = torch.from_numpy(tables_host(key[:2], key[2:])).to(self.device)
        return t

    def __call__(self, frames, dst_wh, out=None):
        """frames: uint8 device tensor [n,h,w,c], c = 3 or 4 (a 4th channel is ignored), channels interleaved (the last two
        strides are c and 1; rows and frames may be padded);  dst_wh = (W, H) as cv2.resize takes it."""
        if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.device == self.device):
            raise ValueError(f'frames must be a uint8 tensor [n,h,w,c] on {self.device}')
        n, h, w, c = frames.shape
        if frames.stride(3) != 1 or frames.stride(2) != c:
            raise ValueError('frames must have interleaved channels (strides [frame, row, c, 1])')
        dw, dh = int(dst_wh[0]), int(dst_wh[1])
        tab = self.tables((h, w), (dh, dw))                  # raises for a size the library refuses
        if out is None:
            out = torch.empty(n, 3, dh, dw, dtype=torch.float32, device=self.device)
        elif not (out.dtype == torch.float32 and out.shape == (n, 3, dh, dw) and out.is_contiguous() and out.device == self.device):
            raise ValueError(f'out must be a contiguous float32 tensor [{n},3,{dh},{dw}] on {self.device}')
        rc = self.L.gnr_ingest_u8(frames.data_ptr(), n, h, w, c, frames.stride(1), frames.stride(0), tab.data_ptr(), out.data_ptr(),
                                  dh, dw, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _lib.check(rc, 'gnr_ingest_u8')
        return out
