"""HIP grasp head: gd.networks.ConvNet.forward on fp32 implicit-GEMM MFMA kernels (csrc/gnr_head.hip).
State-dict keys are the reference's (`vgn_net.encoder.conv1.weight`, ... ; ref: src/gd/networks.py:39-47)."""
import ctypes as C

import numpy as np
import torch

from . import _lib

HEAD_KEYS = [('encoder.conv1', (16, 1, 5)), ('encoder.conv2', (32, 16, 3)), ('encoder.conv3', (64, 32, 3)),
             ('decoder.conv1', (64, 64, 3)), ('decoder.conv2', (32, 64, 3)), ('decoder.conv3', (16, 32, 5)),
             ('conv_qual', (1, 16, 5)), ('conv_rot', (4, 16, 5)), ('conv_width', (1, 16, 5))]


def canonical_blob(state_dict, prefix=''):
    parts = []
    for name, (co, ci, k) in HEAD_KEYS:
        w, b = state_dict[prefix + name + '.weight'], state_dict[prefix + name + '.bias']
        w = w.detach().cpu().numpy() if hasattr(w, 'detach') else np.asarray(w)
        b = b.detach().cpu().numpy() if hasattr(b, 'detach') else np.asarray(b)
        if tuple(w.shape) != (co, ci, k, k, k) or tuple(b.shape) != (co,):
            raise ValueError(f'{name}: unexpected shape {tuple(w.shape)}')
        parts += [np.asarray(w, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)]
    blob = np.concatenate(parts)
    assert blob.size == _lib.lib().gnr_head_canonical_floats()
    return blob


def pack(canonical):
    L = _lib.lib()
    canonical = np.ascontiguousarray(canonical, np.float32)
    out = np.zeros(L.gnr_head_packed_floats(), np.float32)
    rc = L.gnr_pack_grasp_head(canonical.ctypes.data_as(_lib.c_float_p), out.ctypes.data_as(_lib.c_float_p))
    _lib.check(rc, 'gnr_pack_grasp_head')
    return out


def activation_layout(B, R):
    """(name, float offset, shape) of the six post-ReLU activations a1..a6 in the workspace of gnr_grasp_head_fwd(B, R), laid out as
    that function lays them out (a1 [B,16,d1^3], a2 [B,32,d2^3], a3 / a4 [B,64,d3^3], a5 [B,32,10^3], a6 [B,16,20^3], then 4096 bytes that
    hold the three nearest-neighbour index maps).  A layout change in the library fails the assertion here."""
    if B < 1 or not 8 <= R <= 64:
        raise ValueError(f'the grasp head takes B >= 1 and R in 8..64, not B = {B}, R = {R}')
    d1 = (R - 1) // 2 + 1
    d2 = (d1 - 1) // 2 + 1
    d3 = (d2 - 1) // 2 + 1
    out, off = [], 0
    for i, (c, d) in enumerate([(16, d1), (32, d2), (64, d3), (64, d3), (32, 10), (16, 20)]):
        out.append((f'a{i + 1}', off, (B, c, d, d, d)))
        off += B * c * d ** 3
    assert 4 * off + 4096 == _lib.lib().gnr_grasp_head_workspace_bytes(B, R), 'workspace layout of gnr_grasp_head_fwd has changed'
    return out


class GraspHead:
    """gd.networks.ConvNet.forward for a volume [B,1,R,R,R] with B >= 1 and a volume edge R in 8..64 (the library refuses anything else
    with GNR_ERR_SHAPE).  The encoder halves R three times (d -> (d - 1) // 2 + 1); up to R = 40 (bottleneck edge d3 <= 5) decoder.conv1
    and decoder.conv2 run on the LDS-staged kernel, from R = 41 on the direct-gather kernel.  The outputs are 40^3 whatever R is."""

    def __init__(self, state_dict, prefix='', device='cuda:0'):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.GnrError('the HIP grasp head needs a ROCm GPU; there is no CPU fallback')
        self.device = torch.device(device)
        self.w = torch.from_numpy(pack(canonical_blob(state_dict, prefix))).to(self.device)
        self._ws = None

    def __call__(self, volume):
        """volume [B,1,R,R,R] (cuda, fp32) -> (qual [B,1,40,40,40], rot [B,4,40,40,40], width [B,1,40,40,40])"""
        vol = volume.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, R = vol.shape[:3]
        need = self.L.gnr_grasp_head_workspace_bytes(B, R)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        q = torch.empty(B, 1, 40, 40, 40, device=self.device)
        r = torch.empty(B, 4, 40, 40, 40, device=self.device)
        w = torch.empty(B, 1, 40, 40, 40, device=self.device)
        rc = self.L.gnr_grasp_head_fwd(B, R, vol.data_ptr(), self.w.data_ptr(), q.data_ptr(), r.data_ptr(), w.data_ptr(),
                                       self._ws.data_ptr(), self._ws.numel(),
                                       C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _lib.check(rc, 'gnr_grasp_head_fwd')
        return q, r, w

    def activations(self, B, R):
        """Views of a1..a6 (the post-ReLU output of encoder.conv1..3 and decoder.conv1..3) in the workspace of the last call, which must
        have been a call with this B and R: {'a1': [B,16,d1,d1,d1], ..., 'a6': [B,16,20,20,20]}.  The next call overwrites them."""
        layout = activation_layout(B, R)
        if self._ws is None or self._ws.numel() < self.L.gnr_grasp_head_workspace_bytes(B, R):
            raise _lib.GnrError('activations(): no call with this B and R has been made')
        return {name: self._ws[4 * off:4 * (off + int(np.prod(shape)))].view(torch.float32).view(shape) for name, off, shape in layout}
