"""Depth and gradient images of a scalar volume from any camera, on the device (csrc/gnr_raycast.hip, gnr_volume_raycast_fwd): what the
SDF volume of sample_volume, or a fused TSDF grid, looks like from a camera.  include/gnr.h states the arithmetic; the images are
the bits of the float64 statement tests/raycast_reference.py.  No reference counterpart."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .grasp_post import DeviceOp, checked_params, expand_cameras, gradient_batch, unit_normals, volume_batch

RAYCAST_DEFAULTS = dict(iso=0.0, step=0.5, bisections=4)


def volume_origin(bbox_lo, voxel_size):
    """World position of voxel (0,0,0)'s centre of the volume sampled over the box that starts at bbox_lo: the lattice origin of its
    ray cast (float64)."""
    return np.asarray(bbox_lo, np.float64) + 0.5 * voxel_size


def depth_params(volume_depth, **more):
    """A plan's `volume_depth` argument -> None, or the ray cast's parameters (True: the plan's own cameras and image size, iso = 0,
    half-voxel steps, four bisections);  extrinsics -> float32 [V',3,4], intrinsic -> float32 [3,3], hw -> (h, w).  more: further keys
    the caller takes, with their defaults (a session's `origin`)."""
    out = checked_params('volume_depth', volume_depth, {'extrinsics': None, 'intrinsic': None, 'hw': None, **RAYCAST_DEFAULTS, **more})
    if out is None:
        return None
    if out['extrinsics'] is not None:
        ext = np.stack([np.asarray(e, np.float32) for e in out['extrinsics']], 0)
        if ext.ndim != 3 or ext.shape[1:] not in ((3, 4), (4, 4)):
            raise ValueError(f'volume_depth extrinsics must be V world->camera [3|4,4], got {ext.shape}')
        out['extrinsics'] = np.ascontiguousarray(ext[:, :3, :])
    if out['intrinsic'] is not None:
        out['intrinsic'] = np.ascontiguousarray(np.asarray(out['intrinsic'], np.float32).reshape(3, 3))
    if out['hw'] is not None:
        out['hw'] = (int(out['hw'][0]), int(out['hw'][1]))
    out['iso'], out['step'], out['bisections'] = float(out['iso']), float(out['step']), int(out['bisections'])
    return out


class VolumeRaycaster(DeviceOp):
    """The depth images [B,V,h,w] of the iso-surface vol = iso of B volumes from V cameras each; with a gradient volume also the
    gradient images [B,V,h,w,3].  The output buffers are kept per shape and written again by the next call of that shape, so their
    addresses are stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'volume ray cast')
        self._out = {}

    def __call__(self, vol, poses, Ks, hw, *, origin, scale, iso=0.0, step=0.5, bisections=4, near=0.0, far=float('inf'), gradient=None):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]), 2 <= R <= 256;  poses [B,V,3,4] world->camera, Ks [B,V,3,3] (one scene's
        [V,..] serve every scene);  hw = (h, w);  lattice point i of the volume sits at world origin + i * scale.
        -> {'depth': [B,V,h,w] float32, camera-z metres, 0 where the ray meets no surface;  'gradient': [B,V,h,w,3] float32 when a
        gradient volume [B,R,R,R,3] is given: its rows interpolated to the hit points, not normalised, 0 on a miss}.
        The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        vol, B, R = volume_batch(vol, d)
        poses = torch.as_tensor(poses, dtype=torch.float32, device=d)
        Ks = torch.as_tensor(Ks, dtype=torch.float32, device=d)
        if poses.dim() not in (3, 4) or tuple(poses.shape[-2:]) != (3, 4) or Ks.dim() not in (3, 4) or tuple(Ks.shape[-2:]) != (3, 3):
            raise ValueError(f'poses must be [B,V,3,4] and Ks [B,V,3,3], got {tuple(poses.shape)} and {tuple(Ks.shape)}')
        V = poses.shape[-3]
        poses, Ks = (c.contiguous() for c in expand_cameras(poses, Ks, B, V))
        h, w = int(hw[0]), int(hw[1])
        g = gradient_batch(gradient, B, R, d)
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
                                           out['depth'].data_ptr(), None if g is None else out['gradient'].data_ptr(), self._stream())
        _lib.check(rc, 'gnr_volume_raycast_fwd')
        return dict(out)


COLOR_KEYS = ('color', 'color_weight')                       # what of surface_color.SurfaceColorizer.pixels a plan keeps beside the depth


def raycast_rows(res, b):
    """The device images of scene b of a VolumeRaycaster result (with the colour images, when SurfaceColorizer.pixels completed it)."""
    return {k: res[k][b] for k in ('depth', 'gradient', *COLOR_KEYS) if k in res}


def images_from_rows(rows):
    """raycast_rows on the host (numpy) -> `volume_depth` [V,h,w] float32; with `gradient` also `volume_depth_normals` [V,h,w,3]
    float64 = g / |g| computed on the host like the cloud's (a miss stays zero); with `color` / `color_weight` also `volume_color`
    [V,h,w,3] and `volume_color_weight` [V,h,w] float32, as they are."""
    out = {'volume_depth': rows['depth']}
    if 'gradient' in rows:
        out['volume_depth_normals'] = unit_normals(rows['gradient']).reshape(rows['gradient'].shape)
    out.update({'volume_' + k: rows[k] for k in COLOR_KEYS if k in rows})
    return out


def images_from_raycast(res, b=0):
    """Scene b of a VolumeRaycaster result -> numpy dict (images_from_rows)."""
    return images_from_rows({k: v.cpu().numpy() for k, v in raycast_rows(res, b).items()})


def depth_mae(depth, true_depth):
    """Device scalar: the mean of |depth - true_depth| over the pixels where both are > 0 (the ray hit and the label exists); NaN when
    there is no such pixel.  float64 accumulation on the device."""
    both = (depth > 0) & (true_depth > 0)
    err = torch.where(both, (depth.double() - true_depth.double()).abs(), torch.zeros((), dtype=torch.float64, device=depth.device))
    return err.sum() / both.sum()              # 0 / 0: NaN
