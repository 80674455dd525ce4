"""Depth and gradient images of a scalar volume from any camera, on the device (csrc/gnr_raycast.hip, gnr_volume_raycast_fwd): what the
SDF volume of sample_volume, or a fused TSDF grid, looks like from a camera.  include/gnr.h states the arithmetic; the images are
the bits of the float64 statement tests/raycast_reference.py.  No reference counterpart."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .grasp_post import unit_normals

RAYCAST_DEFAULTS = dict(iso=0.0, step=0.5, bisections=4)


class VolumeRaycaster:
    """The depth images [B,V,h,w] of the iso-surface vol = iso of B volumes from V cameras each; with a gradient volume also the
    gradient images [B,V,h,w,3].  The output buffers are kept per shape and written again by the next call of that shape, so their
    addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.GnrError('the HIP volume ray cast needs a ROCm GPU; there is no CPU fallback')
        self.device = torch.device(device)
        self._out = {}

    def __call__(self, vol, poses, Ks, hw, *, origin, scale, iso=0.0, step=0.5, bisections=4, near=0.0, far=float('inf'), gradient=None):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]), 2 <= R <= 256;  poses [B,V,3,4] world->camera, Ks [B,V,3,3] (one scene's
        [V,..] serve every scene);  hw = (h, w);  lattice point i of the volume sits at world origin + i * scale.
        -> {'depth': [B,V,h,w] float32, camera-z metres, 0 where the ray meets no surface;  'gradient': [B,V,h,w,3] float32 when a
        gradient volume [B,R,R,R,3] is given: its rows interpolated to the hit points, not normalised, 0 on a miss}.
        The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        vol = torch.as_tensor(vol, dtype=torch.float32, device=d).contiguous()
        R = vol.shape[-1]
        if vol.dim() < 3 or tuple(vol.shape[-3:]) != (R, R, R) or vol.numel() % R ** 3:
            raise ValueError(f'vol must be [B,R,R,R], got {tuple(vol.shape)}')
        B = vol.numel() // R ** 3
        poses = torch.as_tensor(poses, dtype=torch.float32, device=d)
        Ks = torch.as_tensor(Ks, dtype=torch.float32, device=d)
        if poses.dim() not in (3, 4) or tuple(poses.shape[-2:]) != (3, 4) or Ks.dim() not in (3, 4) or tuple(Ks.shape[-2:]) != (3, 3):
            raise ValueError(f'poses must be [B,V,3,4] and Ks [B,V,3,3], got {tuple(poses.shape)} and {tuple(Ks.shape)}')
        V = poses.shape[-3]
        try:
            poses, Ks = poses.expand(B, V, 3, 4).contiguous(), Ks.expand(B, V, 3, 3).contiguous()
        except RuntimeError:
            raise ValueError(f'cameras {tuple(poses.shape)} / {tuple(Ks.shape)} do not fit {B} scene(s) of {V} view(s)') from None
        h, w = int(hw[0]), int(hw[1])
        g = None
        if gradient is not None:
            g = torch.as_tensor(gradient, dtype=torch.float32, device=d).contiguous()
            if tuple(g.shape) != (B, R, R, R, 3):
                raise ValueError(f'gradient must be [{B},{R},{R},{R},3], got {tuple(g.shape)}')
        key = (B, V, h, w, g is not None)
        out = self._out.get(key)
        if out is None:
            out = {'depth': torch.empty(B, V, max(h, 0), max(w, 0), dtype=torch.float32, device=d)}
            if g is not None:
                out['gradient'] = torch.empty(B, V, max(h, 0), max(w, 0), 3, dtype=torch.float32, device=d)
            self._out[key] = out
        p = _lib.GnrRaycastParams(B=B, V=V, h=h, w=w, R=R, bisections=int(bisections), iso=float(iso), scale=float(scale), step=float(step),
                                  near_s=float(near), far_s=float(far))
        p.origin[:] = [float(c) for c in origin]
        rc = self.L.gnr_volume_raycast_fwd(C.byref(p), vol.data_ptr(), None if g is None else g.data_ptr(), poses.data_ptr(), Ks.data_ptr(),
                                           out['depth'].data_ptr(), None if g is None else out['gradient'].data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream(d).cuda_stream))
        _lib.check(rc, 'gnr_volume_raycast_fwd')
        return dict(out)


def images_from_raycast(res, b=0):
    """Scene b of a VolumeRaycaster result -> numpy dict: `volume_depth` [V,h,w] float32; a result with `gradient` adds
    `volume_depth_normals` [V,h,w,3] float64 = g / |g| computed on the host like the cloud's (a miss stays zero)."""
    out = {'volume_depth': res['depth'][b].cpu().numpy()}
    if 'gradient' in res:
        g = res['gradient'][b].cpu().numpy()
        out['volume_depth_normals'] = unit_normals(g).reshape(g.shape)
    return out


def depth_mae(depth, true_depth):
    """Device scalar: the mean of |depth - true_depth| over the pixels where both are > 0 (the ray hit and the label exists); NaN when
    there is no such pixel.  float64 accumulation on the device."""
    both = (depth > 0) & (true_depth > 0)
    err = torch.where(both, (depth.double() - true_depth.double()).abs(), torch.zeros((), dtype=torch.float64, device=depth.device))
    return err.sum() / both.sum()              # 0 / 0: NaN
