// Ray cast of a scalar volume on the device: depth (and gradient) images of the iso-surface vol = iso of B volumes seen from V cameras
// each -- what the volume the grasp head consumes looks like from a camera.  No reference counterpart (like gnr_mesh.hip); the
// statement is include/gnr.h's and tests/raycast_reference.py's.
// One lane per pixel, one wavefront per 8 x 8 pixel tile of one view (neighbouring rays read neighbouring voxels), four tiles side by
// side per block.  The volume is read through the vector cache (40^3 floats = 256 KB: L2 resident, too large for a block's LDS).
// The march is data dependent: a lane stops at its first outside -> inside sample pair or at the end of its ray, a wavefront leaves
// the loop when a ballot finds no lane marching; the loop is bounded by the box's diagonal whatever the cameras hold.  Plain loads
// and stores, nothing atomic, no workspace: every pixel is a pure function of the input bits.
// The ray, the slabs, the samples, the trilinear values, the bisection and the secant step are float64, every operation one correctly
// rounded IEEE operation in the order written here (contraction is off for the whole file, as in gnr_tsdf.hip and gnr_mesh.hip): the
// results are the bits of the numpy statement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_host.h"
#include "gnr_trilinear.h"       // base_of, value_at: the trilinear form, shared with gnr_surface_color.hip

#pragma clang fp contract(off)

namespace gnr_raycast {

using namespace gnr;

struct Shape {
    int V, h, w, R, bisections, nmax;
    unsigned tiles_x, tiles, blocks;           // 8 x 8 tiles per row and per view; blocks of four tiles per view
    double iso, scale, step, near_s, far_s, origin[3];
};

// launch grid: (blocks of four tiles, B, views), both x and z strided (B <= 65535);  block 256 = 4 wavefronts, wavefront j of block i
// owns tile 4 i + j of the view, lane l its pixel (l & 7, l >> 3)
__global__ __launch_bounds__(256) void k_volume_raycast(const float* __restrict__ vol, const float* __restrict__ grad,
                                                        const float* __restrict__ poses, const float* __restrict__ Ks,
                                                        float* __restrict__ depth, float* __restrict__ gradient, Shape sh) {
    const int R = sh.R, b = blockIdx.y;
    const size_t n3 = (size_t)R * R * R;
    const float* v = vol + (size_t)b * n3;
    const float* g = grad ? grad + (size_t)b * n3 * 3 : nullptr;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const double top = (double)(R - 1);
    for (int view = blockIdx.z; view < sh.V; view += gridDim.z) {
        const size_t bv = (size_t)b * sh.V + view;
        const float* P = poses + bv * 12;
        const float* K = Ks + bv * 9;
        const double fx = (double)K[0], fy = (double)K[4], cx = (double)K[2], cy = (double)K[5];
        double e[3], rx[3], ry[3], rz[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            rx[a] = (double)P[a]; ry[a] = (double)P[4 + a]; rz[a] = (double)P[8 + a];
            const double eye = -((rx[a] * (double)P[3] + ry[a] * (double)P[7]) + rz[a] * (double)P[11]);
            e[a] = (eye - sh.origin[a]) / sh.scale;
        }
        for (unsigned blk = blockIdx.x; blk < sh.blocks; blk += gridDim.x) {
            const unsigned tile = blk * 4u + wave;                 // (tiles <= 2^28: neither this nor a pixel coordinate wraps)
            const unsigned px = (tile % sh.tiles_x) * 8u + (lane & 7u), py = (tile / sh.tiles_x) * 8u + (lane >> 3);
            const bool pixel = tile < sh.tiles && px < (unsigned)sh.w && py < (unsigned)sh.h;       // the padding of a ragged tile marches nothing, writes nothing
            const double dcx = ((double)px - cx) / fx, dcy = ((double)py - cy) / fy;
            double d[3];
            double s0 = sh.near_s, s1 = sh.far_s;
            bool ok = pixel;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                d[a] = ((rx[a] * dcx + ry[a] * dcy) + rz[a]) / sh.scale;
                if (d[a] == 0.0) {
                    ok = ok && 0.0 <= e[a] && e[a] <= top;
                } else {
                    const double ta = (0.0 - e[a]) / d[a], tb = (top - e[a]) / d[a];
                    s0 = fmax(s0, fmin(ta, tb));
                    s1 = fmin(s1, fmax(ta, tb));
                }
            }
            ok = ok && s0 < s1 && isfinite(s1);
            double ds = 0.0, sp = 0.0, fp = 0.0, A = 0.0, Bs = 0.0, fA = 0.0, fB = 0.0;
            int n = 0;
            if (ok) {
                ds = sh.step / __dsqrt_rn((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                const double nf = ceil((s1 - s0) / ds);
                n = nf <= (double)sh.nmax ? (int)nf : sh.nmax;     // (a NaN or an infinity takes the bound)
                sp = fmin(s0 + 0.0 * ds, s1);
                fp = value_at(v, 1, R, e, d, sp) - sh.iso;
            }
            bool hit = false, march = ok && n >= 1;
            for (int k = 1; k <= sh.nmax; ++k) {
                if (__ballot(march) == 0ull) break;
                if (march) {
                    const double sk = fmin(s0 + (double)k * ds, s1);
                    const double fk = value_at(v, 1, R, e, d, sk) - sh.iso;
                    if (fp >= 0.0 && fk < 0.0) {
                        hit = true; A = sp; Bs = sk; fA = fp; fB = fk;
                    }
                    sp = sk; fp = fk;
                    march = !hit && k < n;
                }
            }
            double s = 0.0;
            if (hit) {
                for (int i = 0; i < sh.bisections; ++i) {
                    const double m = 0.5 * (A + Bs);
                    const double fm = value_at(v, 1, R, e, d, m) - sh.iso;
                    if (fm < 0.0) { Bs = m; fB = fm; } else { A = m; fA = fm; }
                }
                s = A + (Bs - A) * (fA / (fA - fB));
            }
            if (!pixel) continue;
            const size_t o = (bv * sh.h + py) * sh.w + px;
            depth[o] = hit ? (float)s : 0.f;
            if (g) {
                float out[3] = {0.f, 0.f, 0.f};
                if (hit) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) out[q] = (float)value_at(g + q, 3, R, e, d, s);
                }
                gradient[o * 3] = out[0]; gradient[o * 3 + 1] = out[1]; gradient[o * 3 + 2] = out[2];
            }
        }
    }
}

}  // namespace gnr_raycast

using namespace gnr_raycast;

extern "C" int gnr_volume_raycast_fwd(const GnrRaycastParams* p, const float* vol, const float* grad, const float* poses, const float* Ks,
                                      float* depth, float* gradient, void* stream) {
    const Refuse no{"gnr_volume_raycast_fwd"};
    if (!p || !vol || !poses || !Ks || !depth) return no(GNR_ERR_ARG, "null pointer");
    if ((grad == nullptr) != (gradient == nullptr)) return no(GNR_ERR_ARG, "grad and gradient must be both given or both NULL");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, p->B)) return rc;
    if (p->V < 1) return no(GNR_ERR_SHAPE, "V must be >= 1");
    if (p->h < 1 || p->w < 1) return no(GNR_ERR_SHAPE, "h and w must be >= 1");
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, p->R)) return rc;
    if (p->bisections < 0 || p->bisections > 32) return no(GNR_ERR_ARG, "bisections must be in 0..32");
    if (!isfinite(p->scale) || !isfinite(p->step) || !(p->scale > 0.0) || !(p->step > 0.0))
        return no(GNR_ERR_ARG, "scale and step must be finite and > 0");
    if (!isfinite(p->iso) || !isfinite(p->origin[0]) || !isfinite(p->origin[1]) || !isfinite(p->origin[2]))
        return no(GNR_ERR_ARG, "iso and origin must be finite");
    if (!(p->near_s >= 0.0) || !(p->far_s > p->near_s)) return no(GNR_ERR_ARG, "near_s must be >= 0 and far_s > near_s");
    const double most = ceil(sqrt(3.0) * (double)(p->R - 1) / p->step) + 1.0;   // the march's loop bound
    if (!(most <= (double)GNR_RAYCAST_MAX_SAMPLES))
        return no(GNR_ERR_ARG, "step too small, a ray would take more than GNR_RAYCAST_MAX_SAMPLES (65536) samples");
    const unsigned long long tiles_x = ((unsigned long long)p->w + 7) / 8, tiles_y = ((unsigned long long)p->h + 7) / 8;
    const unsigned long long blocks = (tiles_x * tiles_y + 3) / 4;
    if (tiles_x * tiles_y > (1ull << 28)) return no(GNR_ERR_SHAPE, "h and w must give at most 2^28 tiles of 8 x 8 pixels");
    Shape sh{p->V, p->h, p->w, p->R, p->bisections, (int)most, (unsigned)tiles_x, (unsigned)(tiles_x * tiles_y), (unsigned)blocks, (double)p->iso, p->scale, p->step,
             p->near_s, p->far_s, {p->origin[0], p->origin[1], p->origin[2]}};
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)p->B, (unsigned)(p->V < 64 ? p->V : 64));
    return launch<k_volume_raycast>("k_volume_raycast@gnr_volume_raycast_fwd", (hipStream_t)stream, grid, dim3(256), 0, vol, grad, poses, Ks,
                                    depth, gradient, sh);
}
