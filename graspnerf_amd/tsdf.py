"""Depth route: TSDF fusion of posed depth images on the device (csrc/gnr_tsdf.hip) -- `TSDFVolume` and `create_tsdf` of the
reference's src/gd/perception.py:66-128, which drive Open3D's UniformTSDFVolume on the host.  The grid feeds the grasp head and
process + select (gd/detection.py:13-40, the VGN baseline: planner.plan_depth); `grid * 2 - 1` is the trainer's `sdf_gt`
(dataset/database.py:207-209: sdf_gt_from_depth).
Differences: B scenes at once, device tensors out, `get_grid()` is [B,1,R,R,R] at any R in 2..256; the projection is computed
directly in float64 per voxel instead of Open3D's incrementally accumulated float32 one (include/gnr.h states the arithmetic);
there is no `get_cloud`."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .grasp_post import DeviceOp, expand_cameras


def rotation_matrix(q):
    """scipy's Rotation.from_quat(q).as_matrix() of a UNIT quaternion (x, y, z, w), float64; the caller normalises."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class TSDFVolume(DeviceOp):
    """Integration of posed depth images into B truncated signed distance volumes of `resolution`^3 voxels over the cube
    [origin, origin + size]^3; perception.py's TSDFVolume(size, resolution) is B = 1 with the origin at zero."""

    def __init__(self, size, resolution, B=1, origin=(0.0, 0.0, 0.0), device='cuda:0', sdf_trunc=None, depth_scale=1.0, depth_trunc=2.0):
        super().__init__(device, 'TSDF fusion')
        self.size, self.resolution, self.B = float(size), int(resolution), int(B)
        self.voxel_size = self.size / self.resolution
        self.sdf_trunc = 4 * self.voxel_size if sdf_trunc is None else float(sdf_trunc)
        self.depth_scale, self.depth_trunc = float(depth_scale), float(depth_trunc)
        o = np.asarray(origin.detach().cpu() if torch.is_tensor(origin) else origin, np.float32)
        self._origin_host = np.broadcast_to(o, (self.B, 3)).copy()
        self.origin = torch.from_numpy(self._origin_host).to(self.device)
        self._raycaster = None
        R = self.resolution
        self.tsdf = torch.empty(self.B, R, R, R, device=self.device)
        self.weight = torch.empty(self.B, R, R, R, device=self.device)
        self.reset()

    def reset(self):
        _lib.check(self.L.gnr_tsdf_reset(self.B, self.resolution, self.tsdf.data_ptr(), self.weight.data_ptr(), self._stream()), 'gnr_tsdf_reset')

    def _depth(self, depth):
        """-> (device tensor [B,V,h,w] float32 or 16-bit, dtype code)"""
        if not torch.is_tensor(depth):
            depth = np.asarray(depth)
            if depth.dtype == np.uint16:
                depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16))       # (the bits travel; the kernel reads uint16)
            else:
                depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32))
        elif depth.dtype == getattr(torch, 'uint16', None):
            depth = depth.view(torch.int16)
        elif depth.dtype != torch.float32:
            raise ValueError(f'depth must be float32 or uint16, got {depth.dtype}')
        if depth.dim() < 2 or depth.dim() > 4:
            raise ValueError(f'depth must be [h,w], [V,h,w] or [B,V,h,w], got {tuple(depth.shape)}')
        depth = depth.reshape((1,) * (4 - depth.dim()) + tuple(depth.shape))
        if depth.shape[0] != self.B:
            raise ValueError(f'depth is for {depth.shape[0]} scene(s), the volume holds {self.B}')
        return depth.to(self.device).contiguous(), _lib.GNR_DEPTH_U16 if depth.dtype == torch.int16 else _lib.GNR_DEPTH_F32

    def _cameras(self, intrinsic, extrinsic, V):
        """-> Ks [B,V,3,3], poses [B,V,3,4] float32 on the device.  Device tensors stay on the device (nothing waits for the host:
        a fusion from device tensors can be captured in a graph)."""
        if all(hasattr(intrinsic, k) for k in ('fx', 'fy', 'cx', 'cy')):                   # perception.CameraIntrinsic
            intrinsic = [[intrinsic.fx, 0.0, intrinsic.cx], [0.0, intrinsic.fy, intrinsic.cy], [0.0, 0.0, 1.0]]
        K = intrinsic if torch.is_tensor(intrinsic) else torch.from_numpy(np.asarray(intrinsic, np.float32))
        if K.shape[-2:] != (3, 3):
            raise ValueError(f'intrinsic must be [..,3,3], got {tuple(K.shape)}')
        E = extrinsic
        if not torch.is_tensor(E):
            E = np.asarray(E, np.float64)
            if E.shape[-1] == 7 and E.shape[-2:] not in ((4, 4), (3, 4)):                  # Transform.to_list(): [qx,qy,qz,qw,tx,ty,tz]
                flat = E.reshape(-1, 7)
                E = np.stack([np.concatenate([rotation_matrix(e[:4] / np.linalg.norm(e[:4])), e[4:, None]], 1) for e in flat]).reshape(E.shape[:-1] + (3, 4))
            E = torch.from_numpy(np.ascontiguousarray(E, np.float32))
        if E.shape[-2:] == (4, 4):
            E = E[..., :3, :]
        elif E.shape[-2:] != (3, 4):
            raise ValueError(f'extrinsic must be [..,4,4], [..,3,4] or [..,7], got {tuple(E.shape)}')
        return tuple(c.to(self.device, torch.float32).contiguous() for c in expand_cameras(K, E, self.B, V))

    def integrate(self, depth, intrinsic, extrinsic):
        """depth [h,w], [V,h,w] or [B,V,h,w], float32 or uint16 (numpy or device tensor), in units of 1 / depth_scale metres;
        intrinsic: 3x3, [..,3,3] or an object with fx, fy, cx, cy;  extrinsic: world(volume)->camera as 4x4 / 3x4 (or stacks of
        them) or the reference's 7-list [qx,qy,qz,qw,tx,ty,tz].  The views are fused in the order given."""
        depth, code = self._depth(depth)
        _, V, h, w = depth.shape
        K, E = self._cameras(intrinsic, extrinsic, V)
        p = _lib.GnrTsdfParams(B=self.B, V=V, h=h, w=w, R=self.resolution, depth_dtype=code, voxel_size=self.voxel_size,
                               sdf_trunc=self.sdf_trunc, depth_scale=self.depth_scale, depth_trunc=self.depth_trunc)
        rc = self.L.gnr_tsdf_integrate(C.byref(p), depth.data_ptr(), E.data_ptr(), K.data_ptr(), self.origin.data_ptr(),
                                       self.tsdf.data_ptr(), self.weight.data_ptr(), self._stream())
        _lib.check(rc, 'gnr_tsdf_integrate')

    def _grid(self, mode):
        out = torch.empty_like(self.tsdf)
        rc = self.L.gnr_tsdf_grid(self.B, self.resolution, self.tsdf.data_ptr(), self.weight.data_ptr(), mode, out.data_ptr(), self._stream())
        _lib.check(rc, 'gnr_tsdf_grid')
        return out

    def get_grid(self):
        """[B,1,R,R,R]: (tsdf + 1) / 2 of the observed voxels with -0.98 <= tsdf < 0.98, 0 elsewhere (perception.py:109-117)."""
        return self._grid(_lib.GNR_TSDF_GRID).unsqueeze(1)

    def sdf_label(self):
        """[B,R,R,R]: get_grid() * 2 - 1, the trainer's sdf_gt (database.py:207-209); -1 marks a voxel without a label."""
        return self._grid(_lib.GNR_TSDF_SDF_LABEL)

    def render_depth(self, intrinsic, extrinsics, hw, step=0.5, bisections=4):
        """Depth images [B,V,h,w] (device, float32 camera-z metres, 0: no surface) of the fused grid's zero level from the cameras
        `extrinsics` (V of them, as integrate takes them) -- the projection of the grid back into images (raycast.VolumeRaycaster).
        The volume is tsdf where weight > 0 and 1 elsewhere: unobserved space reads as outside.  The voxel centres are the lattice:
        origin + 0.5 * voxel_size, one voxel_size apart."""
        from .raycast import VolumeRaycaster
        E = extrinsics if torch.is_tensor(extrinsics) else np.asarray(extrinsics, np.float64)
        matrices = tuple(E.shape[-2:]) in ((4, 4), (3, 4))                         # else the 7-lists [qx,qy,qz,qw,tx,ty,tz]
        lead = E.shape[:-2] if matrices else E.shape[:-1]
        K, P = self._cameras(intrinsic, E, lead[-1] if lead else 1)
        if self._raycaster is None:
            self._raycaster = VolumeRaycaster(self.device)
        vol = torch.where(self.weight > 0, self.tsdf, torch.ones((), device=self.device))
        half = 0.5 * self.voxel_size
        rows = self._origin_host.astype(np.float64)
        if (rows == rows[0]).all():
            return self._raycaster(vol, P, K, hw, origin=rows[0] + half, scale=self.voxel_size, iso=0.0, step=step, bisections=bisections)['depth']
        return torch.cat([self._raycaster(vol[b:b + 1], P[b:b + 1], K[b:b + 1], hw, origin=rows[b] + half, scale=self.voxel_size, iso=0.0,
                                          step=step, bisections=bisections)['depth'].clone() for b in range(self.B)], 0)


def create_tsdf(size, resolution, depth_imgs, intrinsic, extrinsics, device='cuda:0'):
    """perception.py:123-128: depth_imgs [V,h,w], one intrinsic, extrinsics [V,7] (or matrices) -> a fused TSDFVolume."""
    tsdf = TSDFVolume(size, resolution, device=device)
    tsdf.integrate(depth_imgs, intrinsic, extrinsics)           # the V views in order, in one launch: the bits of V calls
    return tsdf


def sdf_gt_from_depth(ref_imgs_info, resolution, size=0.3):
    """The SDF label [R,R,R] of a training scene from its depth images: true_depth [V,1,h,w] fused with poses [V,3,4] and Ks [V,3,3]
    over the workspace cube at bbox3d[0] -- the voxel centres are those of sample_volume."""
    ref = ref_imgs_info
    depth = ref['true_depth']
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f'true_depth must be [V,1,h,w], got {tuple(depth.shape)}')
    vol = TSDFVolume(size, resolution, origin=ref['bbox3d'][0], device=depth.device if depth.is_cuda else 'cuda:0')
    vol.integrate(depth[:, 0].to(torch.float32), ref['Ks'], ref['poses'])
    return vol.sdf_label()[0]
