"""View colours of surface points, on the device (csrc/gnr_surface_color.hip, gnr_surface_color_points_fwd / _pixels_fwd): the rows of
the surface cloud or of the mesh's vertices, or the hit points of ray-cast depth images, take the colour of the source images they are
seen in -- weighted by how squarely the volume's own normal faces each camera, with visibility decided by a march through the volume.
include/gnr.h states the arithmetic; the results are the bits of the float64 statement tests/surface_color_reference.py.  No reference
counterpart."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .grasp_post import VIEW_KEYS, DeviceOp, checked_params, expand_cameras, volume_batch

COLOR_DEFAULTS = dict(step=0.5, bias=1.5, cos_min=0.0, fill=(0.0, 0.0, 0.0))


def color_params(view_colors, **more):
    """A plan's `view_colors` argument -> None, or the colouring's parameters (True: half-voxel steps of the occlusion march, which
    starts 1.5 voxels off the point, every view that faces the point at all, black where no view does).  more: further keys the caller
    takes, with their defaults (a session's `origin`)."""
    out = checked_params('view_colors', view_colors, {**COLOR_DEFAULTS, **more})
    if out is None:
        return None
    out['step'], out['bias'], out['cos_min'] = float(out['step']), float(out['bias']), float(out['cos_min'])
    out['fill'] = tuple(float(c) for c in out['fill'])
    if len(out['fill']) != 3:
        raise ValueError(f'view_colors fill must be three numbers, got {out["fill"]}')
    return out


def cloud_level(rg):
    """The level below which a voxel occludes a point of the surface cloud with tsdf in rg: the middle of the range as float32 (0 for
    the real route's (-0.2, 0.2))."""
    return float(np.float32(0.5 * (float(rg[0]) + float(rg[1]))))


class SurfaceColorizer(DeviceOp):
    """The view colours of points [B,max_n,3] (.points) or of the pixels of depth images [B,Vc,h,w] (.pixels) of B volumes from V source
    images each.  The output buffers are kept per shape and written again by the next call of that shape, so their addresses are
    stable for a captured graph."""

    def __init__(self, device='cuda:0'):
        super().__init__(device, 'surface colouring')
        self._out = {}

    def _sources(self, vol, images, poses, Ks):
        d = self.device
        vol, B, R = volume_batch(vol, d)
        images = torch.as_tensor(images, dtype=torch.float32, device=d)
        if images.dim() not in (4, 5) or images.shape[-3] != 3:
            raise ValueError(f'images must be [B,V,3,H,W], got {tuple(images.shape)}')
        V, H, W = images.shape[-4], images.shape[-2], images.shape[-1]
        try:
            images = images.expand(B, V, 3, H, W).contiguous()
        except RuntimeError:
            raise ValueError(f'images {tuple(images.shape)} do not fit {B} scene(s)') from None
        poses, Ks = self._cameras(poses, Ks, B, V, 'poses', 'Ks')
        return vol, B, R, images, V, H, W, poses, Ks

    def _cameras(self, poses, Ks, B, V, *names):
        d = self.device
        poses = torch.as_tensor(poses, dtype=torch.float32, device=d)
        Ks = torch.as_tensor(Ks, dtype=torch.float32, device=d)
        if poses.dim() not in (3, 4) or tuple(poses.shape[-2:]) != (3, 4) or Ks.dim() not in (3, 4) or tuple(Ks.shape[-2:]) != (3, 3):
            raise ValueError(f'{names[0]} must be [B,V,3,4] and {names[1]} [B,V,3,3], got {tuple(poses.shape)} and {tuple(Ks.shape)}')
        return tuple(c.contiguous() for c in expand_cameras(poses, Ks, B, V))

    @staticmethod
    def _params(B, V, H, W, R, origin, scale, point_offset, iso, step, bias, cos_min, fill):
        p = _lib.GnrSurfaceColorParams(B=B, V=V, H=H, W=W, R=R, iso=float(iso), scale=float(scale), step=float(step), bias=float(bias),
                                       cos_min=float(cos_min))
        p.origin[:] = [float(c) for c in origin]
        p.point_offset[:] = [float(c) for c in point_offset]
        p.fill[:] = [float(c) for c in fill]
        return p

    def _buffers(self, key, *shape):
        out = self._out.get(key)
        if out is None:
            d = self.device
            out = self._out[key] = (torch.zeros(*shape, 3, dtype=torch.float32, device=d), torch.zeros(*shape, dtype=torch.float32, device=d),
                                    torch.zeros(*shape, dtype=torch.int32, device=d))
        return out

    def points(self, vol, points, count, images, poses, Ks, *, origin, scale, point_offset=(0.0, 0.0, 0.0), iso=0.0, step=0.5, bias=1.5,
               cos_min=0.0, fill=(0.0, 0.0, 0.0)):
        """vol [B,R,R,R] (or [B,1,R,R,R], or one [R,R,R]), 2 <= R <= 256;  points [B,max_n,3] float64, at world point_offset + points;
        count [B] or [B,k] int32 device tensor, its first column the rows of each scene (a SurfaceExtractor's or a MeshExtractor's
        `count`);  images [B,V,3,H,W] float32, poses [B,V,3,4] world->camera, Ks [B,V,3,3] (one scene's serve every scene), V <= 32;
        lattice point i of the volume sits at world origin + i * scale.
        -> {'view_colors': [B,max_n,3] float32, 'view_weight': [B,max_n] float32 (the sum of the contributing views' cosines; 0: no view,
        the colour is `fill`), 'view_mask': [B,max_n] int32 (bit v: view v contributed)}; rows beyond the count keep what they held.
        The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        vol, B, R, images, V, H, W, poses, Ks = self._sources(vol, images, poses, Ks)
        points = torch.as_tensor(points, dtype=torch.float64, device=d).contiguous()
        if points.dim() == 2:
            points = points[None]
        if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3:
            raise ValueError(f'points must be [{B},max_n,3], got {tuple(points.shape)}')
        if not torch.is_tensor(count) or count.dtype != torch.int32 or count.device != points.device or count.shape[0] != B or \
                not count.is_contiguous():
            raise ValueError(f'count must be a contiguous int32 device tensor [{B}] or [{B},k]')
        n, stride = points.shape[1], count.numel() // B
        colors, weight, mask = self._buffers(('points', B, n), B, n)
        p = self._params(B, V, H, W, R, origin, scale, point_offset, iso, step, bias, cos_min, fill)
        rc = self.L.gnr_surface_color_points_fwd(C.byref(p), vol.data_ptr(), points.data_ptr(), count.data_ptr(), stride, n, images.data_ptr(),
                                                 poses.data_ptr(), Ks.data_ptr(), colors.data_ptr(), weight.data_ptr(), mask.data_ptr(),
                                                 self._stream())
        _lib.check(rc, 'gnr_surface_color_points_fwd')
        return dict(zip(VIEW_KEYS, (colors, weight, mask)))

    def pixels(self, vol, depth, cam_poses, cam_Ks, images, poses, Ks, *, origin, scale, iso=0.0, step=0.5, bias=1.5, cos_min=0.0,
               fill=(0.0, 0.0, 0.0)):
        """depth [B,Vc,h,w] float32 (a VolumeRaycaster's: camera-z metres, 0 where the ray met no surface) seen from cam_poses [B,Vc,3,4] /
        cam_Ks [B,Vc,3,3];  the rest as for points().
        -> {'color': [B,Vc,h,w,3] float32 (`fill` on a miss and where no view contributes), 'color_weight': [B,Vc,h,w] float32,
        'color_mask': [B,Vc,h,w] int32}.  The tensors are this object's: the next call with the same shape writes them again."""
        d = self.device
        vol, B, R, images, V, H, W, poses, Ks = self._sources(vol, images, poses, Ks)
        depth = torch.as_tensor(depth, dtype=torch.float32, device=d).contiguous()
        if depth.dim() == 3:
            depth = depth[None]
        if depth.dim() != 4 or depth.shape[0] != B:
            raise ValueError(f'depth must be [{B},Vc,h,w], got {tuple(depth.shape)}')
        Vc, h, w = depth.shape[1:]
        cam_poses, cam_Ks = self._cameras(cam_poses, cam_Ks, B, Vc, 'cam_poses', 'cam_Ks')
        colors, weight, mask = self._buffers(('pixels', B, Vc, h, w), B, Vc, h, w)
        p = self._params(B, V, H, W, R, origin, scale, (0.0, 0.0, 0.0), iso, step, bias, cos_min, fill)
        rc = self.L.gnr_surface_color_pixels_fwd(C.byref(p), vol.data_ptr(), depth.data_ptr(), cam_poses.data_ptr(), cam_Ks.data_ptr(), Vc, h, w,
                                                 images.data_ptr(), poses.data_ptr(), Ks.data_ptr(), colors.data_ptr(), weight.data_ptr(),
                                                 mask.data_ptr(), self._stream())
        _lib.check(rc, 'gnr_surface_color_pixels_fwd')
        return {'color': colors, 'color_weight': weight, 'color_mask': mask}
