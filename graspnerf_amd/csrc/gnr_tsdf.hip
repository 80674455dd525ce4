// Depth route: fusion of posed depth images into a truncated signed distance volume on the device -- Open3D's
// UniformTSDFVolume::Integrate + extract_voxel_point_cloud as src/gd/perception.py:66-128 drives them (no colour), the grid of
// gd/detection.py:13-40 (VGN) and the trainer's label of dataset/database.py:207-209.
// One thread per voxel, z fastest, the view loop inside the thread in the order given: nothing is atomic, and V views in one call
// are V calls of one view.  The projection, the depth decisions, the signed distance and t = min(1, sdf / trunc) are float64; t is
// rounded once to float32, and the running average and the grid are float32 like Open3D's voxels.  Every operation is one correctly
// rounded IEEE operation in the order written here (contraction is off for the whole file), which is the order of the float64
// statement in tests/tsdf_reference.py: the results are its bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gnr_host.h"

#pragma clang fp contract(off)

namespace gnr_tsdf {

using namespace gnr;

struct Shape { int V, h, w, R; double voxel, trunc, depth_scale, depth_trunc; };

__device__ inline double depth_at(const float* d, size_t i) { return (double)d[i]; }
__device__ inline double depth_at(const unsigned short* d, size_t i) { return (double)d[i]; }

// launch grid: (blocks per scene, B), hence B <= 65535;  depth [B,V,h,w], poses [B,V,3,4], Ks [B,V,3,3], origin [B,3], tsdf / weight [B,R,R,R]
template <typename D>
__global__ __launch_bounds__(256) void k_tsdf_integrate(const D* __restrict__ depth, const float* __restrict__ poses,
                                                        const float* __restrict__ Ks, const float* __restrict__ origin,
                                                        float* __restrict__ tsdf, float* __restrict__ weight, Shape s) {
    const unsigned R = (unsigned)s.R, n = R * R * R;                  // R <= 256: n <= 2^24
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const int b = blockIdx.y;
    const int z = (int)(t % R), y = (int)((t / R) % R), x = (int)(t / (R * R));
    const float* o = origin + (size_t)b * 3;
    const double px = (double)o[0] + ((double)x + 0.5) * s.voxel;
    const double py = (double)o[1] + ((double)y + 0.5) * s.voxel;
    const double pz = (double)o[2] + ((double)z + 0.5) * s.voxel;
    const double wmax = (double)s.w - 1e-4, hmax = (double)s.h - 1e-4;
    const size_t i = (size_t)b * n + t;
    float tv = tsdf[i], wv = weight[i];
    for (int view = 0; view < s.V; ++view) {
        const size_t bv = (size_t)b * s.V + view;
        const float* P = poses + bv * 12;
        const float* K = Ks + bv * 9;
        const double cz = (((double)P[8] * px + (double)P[9] * py) + (double)P[10] * pz) + (double)P[11];
        if (cz <= 0.0) continue;
        const double cx = (((double)P[0] * px + (double)P[1] * py) + (double)P[2] * pz) + (double)P[3];
        const double cy = (((double)P[4] * px + (double)P[5] * py) + (double)P[6] * pz) + (double)P[7];
        const double fx = (double)K[0], fy = (double)K[4], ppx = (double)K[2], ppy = (double)K[5];
        const double uf = ((cx * fx) / cz + ppx) + 0.5;
        const double vf = ((cy * fy) / cz + ppy) + 0.5;
        if (!(uf >= 1e-4 && uf < wmax && vf >= 1e-4 && vf < hmax)) continue;
        const int u = (int)uf, v = (int)vf;                        // in [0, w) x [0, h) by the test above
        double d = depth_at(depth, (bv * s.h + (size_t)v) * s.w + (size_t)u) / s.depth_scale;
        if (d >= s.depth_trunc) d = 0.0;
        if (d <= 0.0) continue;
        const double a = ((double)u - ppx) / fx, c = ((double)v - ppy) / fy;
        const double m = __dsqrt_rn((a * a + c * c) + 1.0);          // camera-z depth -> distance along the ray (integer pixel)
        const double sdf = (d - cz) * m;
        if (sdf > -s.trunc) {
            const float tn = (float)fmin(1.0, sdf / s.trunc);
            tv = (tv * wv + tn) / (wv + 1.0f);
            wv = wv + 1.0f;
        }
    }
    tsdf[i] = tv;
    weight[i] = wv;
}

// get_grid (perception.py:109-117 over extract_voxel_point_cloud): (tsdf + 1) / 2 of the observed, unsaturated voxels, else 0;
// label: grid * 2 - 1 (database.py:207-209), -1 = "no label"
__global__ __launch_bounds__(256) void k_tsdf_grid(const float* __restrict__ tsdf, const float* __restrict__ weight, int label,
                                                   float* __restrict__ out, size_t n) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t i = (size_t)blockIdx.y * n + t;
    const float v = tsdf[i];
    float g = 0.f;
    if (weight[i] != 0.f && v < 0.98f && v >= -0.98f) g = (v + 1.0f) * 0.5f;
    out[i] = label ? g * 2.0f - 1.0f : g;
}

// the state after a reset.  (A kernel, not a pair of memset nodes: in a captured graph the second replay of
// hipMemsetAsync(tsdf) + hipMemsetAsync(weight) left a repeating 64-byte pattern of garbage in the state on this stack.)
__global__ __launch_bounds__(256) void k_tsdf_reset(float* __restrict__ tsdf, float* __restrict__ weight, size_t n) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t i = (size_t)blockIdx.y * n + t;
    tsdf[i] = 0.f;
    weight[i] = 0.f;
}

}  // namespace gnr_tsdf

using namespace gnr_tsdf;

extern "C" int gnr_tsdf_reset(int B, int R, float* tsdf, float* weight, void* stream) {
    const Refuse no{"gnr_tsdf_reset"};
    if (!tsdf || !weight) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    const size_t n = (size_t)R * R * R;
    return launch<k_tsdf_reset>("k_tsdf_reset@gnr_tsdf_reset", (hipStream_t)stream, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, tsdf,
                                weight, n);
}

extern "C" int gnr_tsdf_integrate(const GnrTsdfParams* p, const void* depth, const float* poses, const float* Ks, const float* origin,
                                  float* tsdf, float* weight, void* stream) {
    const Refuse no{"gnr_tsdf_integrate"};
    if (!p || !depth || !poses || !Ks || !origin || !tsdf || !weight) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, p->B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, p->R)) return rc;
    if (p->V < 1) return no(GNR_ERR_SHAPE, "V must be >= 1");
    if (p->h < 1 || p->w < 1) return no(GNR_ERR_SHAPE, "h and w must be >= 1");
    if (p->depth_dtype != GNR_DEPTH_F32 && p->depth_dtype != GNR_DEPTH_U16)
        return no(GNR_ERR_ARG, "depth_dtype must be GNR_DEPTH_F32 or GNR_DEPTH_U16");
    if (!(p->voxel_size > 0.0) || !(p->sdf_trunc > 0.0) || !(p->depth_scale > 0.0) || !(p->depth_trunc > 0.0))
        return no(GNR_ERR_ARG, "voxel_size, sdf_trunc, depth_scale and depth_trunc must be > 0");
    const Shape s{p->V, p->h, p->w, p->R, p->voxel_size, p->sdf_trunc, p->depth_scale, p->depth_trunc};
    const size_t n = (size_t)p->R * p->R * p->R;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)p->B), block(256);
    if (p->depth_dtype == GNR_DEPTH_U16)
        return launch<k_tsdf_integrate<unsigned short>>("k_tsdf_integrate.u16@gnr_tsdf_integrate", (hipStream_t)stream, grid, block, 0,
                                                        (const unsigned short*)depth, poses, Ks, origin, tsdf, weight, s);
    return launch<k_tsdf_integrate<float>>("k_tsdf_integrate@gnr_tsdf_integrate", (hipStream_t)stream, grid, block, 0, (const float*)depth,
                                           poses, Ks, origin, tsdf, weight, s);
}

extern "C" int gnr_tsdf_grid(int B, int R, const float* tsdf, const float* weight, int mode, float* out, void* stream) {
    const Refuse no{"gnr_tsdf_grid"};
    if (!tsdf || !weight || !out) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (mode != GNR_TSDF_GRID && mode != GNR_TSDF_SDF_LABEL) return no(GNR_ERR_ARG, "mode must be GNR_TSDF_GRID or GNR_TSDF_SDF_LABEL");
    const size_t n = (size_t)R * R * R;
    return launch<k_tsdf_grid>("k_tsdf_grid@gnr_tsdf_grid", (hipStream_t)stream, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, tsdf,
                               weight, mode == GNR_TSDF_SDF_LABEL ? 1 : 0, out, n);
}
