// View colours of surface points on the device: every point (a row of the surface cloud or of the mesh's vertices, or the hit point
// of a pixel of a ray-cast depth image) takes the colour of the source images it is seen in, weighted by the cosine between the
// volume's own normal and the direction to each camera, with visibility decided by a march through the volume towards the eye.  No
// reference counterpart (like gnr_mesh.hip and gnr_raycast.hip); the statement is include/gnr.h's and tests/surface_color_reference.py's.
// Mapping: one lane per point, its views one after the other in that lane -- the sum over the views is then in view order by
// construction, with no cross-lane step whose order would have to be fixed.  Pixels: one wavefront per 8 x 8 pixel tile of one target
// camera, four tiles per block, as k_volume_raycast (neighbouring pixels have neighbouring hit points: their marches read neighbouring
// voxels and their taps neighbouring texels).  Points: one wavefront per 64 consecutive rows, four per block (the cloud's rows are in
// np.nonzero order and the mesh's in cell order, so neighbouring rows are mostly neighbouring voxels).  The source cameras are
// block-uniform and are read as scalars.  The volume (40^3 floats = 256 KB) and the images are read through the vector cache: L2
// resident, too large for a block's LDS.  A few hundred to a few thousand points fill a handful of wavefronts, which the march's chain
// of dependent loads then bounds; spreading one point's views over lanes would shorten that chain at the price of an ordered
// cross-lane sum.  The mapping is the simplest that meets the constraints and is not tuned.  Measured (tools/time_surface_color.py,
// profiles/surface_color.json; a 40^3 volume, six 288 x 512 source frames, p50): 6 024 cloud rows 0.157 ms, 2 716 mesh vertices 0.164 ms,
// the 884 736 pixels of six depth frames (9 % hit) 0.294 ms.
// The march is data dependent: a lane stops at its first sample outside the box (visible) or below the level (occluded), a wavefront
// leaves the loop when a ballot finds no lane marching; the loop is bounded by the box's diagonal whatever the cameras hold.  Plain
// loads and stores, nothing atomic, no workspace: every output is a pure function of the input bits.  Everything is float64, every
// operation one correctly rounded IEEE operation in the order written here (contraction is off for the whole file).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "gnr_host.h"
#include "gnr_trilinear.h"

#pragma clang fp contract(off)

namespace gnr_surface_color {

using namespace gnr;

struct Shape {
    int V, H, W, R, nmax;
    int pixels;                                // 1: a point per pixel of depth[B,Vc,hc,wc];  0: a point per row of points[B,max_n,3]
    int Vc, hc, wc, max_n, count_stride;
    unsigned tiles_x, tiles, blocks;           // pixels: 8 x 8 tiles per row and per camera, blocks of four tiles;  points: blocks of 256 rows
    double iso, scale, step, bias, cos_min, origin[3], offset[3], fill[3];
};

// world->camera (R | t) and the intrinsics of one camera as float64;  eye_a = -((R[0][a] t[0] + R[1][a] t[1]) + R[2][a] t[2])
struct Camera {
    double r[3][3], t[3], fx, fy, cx, cy, eye[3];
    __device__ Camera(const float* __restrict__ P, const float* __restrict__ K) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int j = 0; j < 3; ++j) r[a][j] = (double)P[4 * a + j];
            t[a] = (double)P[4 * a + 3];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) eye[a] = -((r[0][a] * t[0] + r[1][a] * t[1]) + r[2][a] * t[2]);
        fx = (double)K[0]; fy = (double)K[4]; cx = (double)K[2]; cy = (double)K[5];
    }
};

// bilinear tap of one channel [H,W] at (u, v): base clamp(floor(.), 0, size-2) per axis (in range whatever u, v hold); x in both rows,
// then y
__device__ inline double tap(const float* __restrict__ img, int W, int ix, int iy, double tx, double ty) {
    const float* c = img + (size_t)iy * W + ix;
    const double a00 = (double)c[0], a01 = (double)c[1], a10 = (double)c[W], a11 = (double)c[W + 1];
    const double r0 = a00 + tx * (a01 - a00), r1 = a10 + tx * (a11 - a10);
    return r0 + ty * (r1 - r0);
}

// launch grid: (blocks, B, Vc or 1), x and z strided (B <= 65535);  block 256 = 4 wavefronts.  pixels: wavefront j of block i owns tile
// 4 i + j of the camera, lane l its pixel (l & 7, l >> 3);  points: thread t of block i owns row 256 i + t
__global__ __launch_bounds__(256) void k_surface_color(const float* __restrict__ vol, const double* __restrict__ points,
                                                       const int* __restrict__ count, const float* __restrict__ depth,
                                                       const float* __restrict__ cam_poses, const float* __restrict__ cam_Ks,
                                                       const float* __restrict__ images, const float* __restrict__ poses,
                                                       const float* __restrict__ Ks, float* __restrict__ colors,
                                                       float* __restrict__ weight, int* __restrict__ views, Shape sh) {
    const int R = sh.R, b = blockIdx.y;
    const float* v = vol + (size_t)b * R * R * R;
    const size_t plane = (size_t)sh.H * sh.W;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const double top = (double)(R - 1);
    int rows = 0;
    if (!sh.pixels) {
        const int n = count[(size_t)b * sh.count_stride];
        rows = n < sh.max_n ? n : sh.max_n;                       // (a negative count: no row)
    }
    const int cams = sh.pixels ? sh.Vc : 1;
    for (int cam = blockIdx.z; cam < cams; cam += gridDim.z) {
        for (unsigned blk = blockIdx.x; blk < sh.blocks; blk += gridDim.x) {
            // ---- the point of this lane -------------------------------------------------------------------------------------
            bool live = false, owned = false;                     // owned: this lane writes an output;  live: it has a point to colour
            size_t o = 0;
            double x[3] = {0.0, 0.0, 0.0};
            if (sh.pixels) {
                const unsigned tile = blk * 4u + wave;            // (tiles <= 2^28: neither this nor a pixel coordinate wraps)
                const unsigned px = (tile % sh.tiles_x) * 8u + (lane & 7u), py = (tile / sh.tiles_x) * 8u + (lane >> 3);
                owned = tile < sh.tiles && px < (unsigned)sh.wc && py < (unsigned)sh.hc;   // the padding of a ragged tile writes nothing
                if (owned) {
                    const size_t bc = (size_t)b * sh.Vc + cam;
                    o = (bc * sh.hc + py) * sh.wc + px;
                    const double s = (double)depth[o];
                    live = !(s <= 0.0);
                    const Camera tc(cam_poses + bc * 12, cam_Ks + bc * 9);
                    const double dcx = ((double)px - tc.cx) / tc.fx, dcy = ((double)py - tc.cy) / tc.fy;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const double dw = (tc.r[0][a] * dcx + tc.r[1][a] * dcy) + tc.r[2][a];
                        x[a] = tc.eye[a] + s * dw;
                    }
                }
            } else {
                const unsigned long long r = (unsigned long long)blk * 256u + threadIdx.x;
                owned = live = r < (unsigned long long)(rows > 0 ? rows : 0);              // rows beyond the count are left untouched
                if (owned) {
                    o = (size_t)b * sh.max_n + (size_t)r;
#pragma unroll
                    for (int a = 0; a < 3; ++a) x[a] = sh.offset[a] + points[o * 3 + a];
                }
            }
            // ---- its index position and the volume's normal there ---------------------------------------------------------------
            double p[3], g[3] = {0.0, 0.0, 0.0}, n2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = (x[a] - sh.origin[a]) / sh.scale;
            if (live) {
                g[0] = value_at(v, 1, R, p[0] + 0.5, p[1], p[2]) - value_at(v, 1, R, p[0] - 0.5, p[1], p[2]);
                g[1] = value_at(v, 1, R, p[0], p[1] + 0.5, p[2]) - value_at(v, 1, R, p[0], p[1] - 0.5, p[2]);
                g[2] = value_at(v, 1, R, p[0], p[1], p[2] + 0.5) - value_at(v, 1, R, p[0], p[1], p[2] - 0.5);
                n2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
                live = !(n2 == 0.0);
            }
            const double norm = __dsqrt_rn(n2);
            // ---- the views, in their order ------------------------------------------------------------------------------------------
            double acc[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
            unsigned mask = 0u;
            for (int view = 0; view < sh.V; ++view) {
                const size_t bv = (size_t)b * sh.V + view;
                const Camera sc(poses + bv * 12, Ks + bv * 9);
                double pc[3], d[3], q[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    pc[a] = ((sc.r[a][0] * x[0] + sc.r[a][1] * x[1]) + sc.r[a][2] * x[2]) + sc.t[a];
                    q[a] = (sc.eye[a] - sh.origin[a]) / sh.scale - p[a];
                }
                bool ok = live && pc[2] > 0.0;
                const double u = pc[0] * sc.fx / pc[2] + sc.cx, w = pc[1] * sc.fy / pc[2] + sc.cy;
                ok = ok && 0.0 <= u && u <= (double)(sh.W - 1) && 0.0 <= w && w <= (double)(sh.H - 1);
                const double L = __dsqrt_rn((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
                ok = ok && !(L == 0.0);
#pragma unroll
                for (int a = 0; a < 3; ++a) d[a] = q[a] / L;
                const double c = ((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]) / norm;
                ok = ok && c > sh.cos_min;
                // the occlusion march towards the eye: `ok` turns false at a sample below the level, the march ends at one outside the box
                bool march = ok;
                for (int k = 0; k < sh.nmax; ++k) {
                    if (__ballot(march) == 0ull) break;
                    if (march) {
                        const double sk = sh.bias + (double)k * sh.step;
                        if (!(sk < L)) {
                            march = false;
                        } else {
                            const double sx = p[0] + sk * d[0], sy = p[1] + sk * d[1], sz = p[2] + sk * d[2];
                            if (!(0.0 <= sx && sx <= top && 0.0 <= sy && sy <= top && 0.0 <= sz && sz <= top)) {
                                march = false;
                            } else if (value_at(v, 1, R, sx, sy, sz) - sh.iso < 0.0) {
                                march = false; ok = false;
                            }
                        }
                    }
                }
                if (ok) {
                    double tx, ty;
                    const int ix = base_of(u, sh.W, tx), iy = base_of(w, sh.H, ty);
                    const float* img = images + bv * 3 * plane;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + c * tap(img + ch * plane, sh.W, ix, iy, tx, ty);
                    wsum = wsum + c;
                    mask |= 1u << view;
                }
            }
            if (!owned) continue;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) colors[o * 3 + ch] = (float)(wsum > 0.0 ? acc[ch] / wsum : sh.fill[ch]);
            weight[o] = (float)wsum;
            views[o] = (int)mask;
        }
    }
}

static int check(const Refuse& no, const GnrSurfaceColorParams* p, double& most) {
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, p->B)) return rc;
    if (p->V < 1 || p->V > 32) return no(GNR_ERR_SHAPE, "V must be in 1..32 (one bit of the view mask each)");
    if (p->H < 2 || p->W < 2) return no(GNR_ERR_SHAPE, "H and W must be >= 2");
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, p->R)) return rc;
    if (!isfinite(p->scale) || !isfinite(p->step) || !(p->scale > 0.0) || !(p->step > 0.0))
        return no(GNR_ERR_ARG, "scale and step must be finite and > 0");
    if (!isfinite(p->bias) || !(p->bias >= 0.0)) return no(GNR_ERR_ARG, "bias must be finite and >= 0");
    bool finite = isfinite(p->iso) && isfinite(p->cos_min);
    for (int a = 0; a < 3; ++a) finite = finite && isfinite(p->origin[a]) && isfinite(p->point_offset[a]) && isfinite(p->fill[a]);
    if (!finite) return no(GNR_ERR_ARG, "iso, origin, point_offset, cos_min and fill must be finite");
    most = ceil(sqrt(3.0) * (double)(p->R - 1) / p->step) + 1.0;                  // the march's loop bound
    if (!(most <= (double)GNR_RAYCAST_MAX_SAMPLES))
        return no(GNR_ERR_ARG, "step too small, a march would take more than GNR_RAYCAST_MAX_SAMPLES (65536) samples");
    return GNR_OK;
}

static Shape shape_of(const GnrSurfaceColorParams* p, double most) {
    Shape sh{};
    sh.V = p->V; sh.H = p->H; sh.W = p->W; sh.R = p->R; sh.nmax = (int)most;
    sh.iso = (double)p->iso; sh.scale = p->scale; sh.step = p->step; sh.bias = p->bias; sh.cos_min = p->cos_min;
    for (int a = 0; a < 3; ++a) { sh.origin[a] = p->origin[a]; sh.offset[a] = p->point_offset[a]; sh.fill[a] = (double)p->fill[a]; }
    return sh;
}

}  // namespace gnr_surface_color

using namespace gnr_surface_color;

extern "C" int gnr_surface_color_points_fwd(const GnrSurfaceColorParams* p, const float* vol, const double* points, const int* count,
                                            int count_stride, int max_n, const float* images, const float* poses, const float* Ks,
                                            float* colors, float* weight, int* views, void* stream) {
    const Refuse no{"gnr_surface_color_points_fwd"};
    if (!p || !vol || !points || !count || !images || !poses || !Ks || !colors || !weight || !views) return no(GNR_ERR_ARG, "null pointer");
    double most = 0.0;
    if (const int rc = check(no, p, most)) return rc;
    if (max_n < 1) return no(GNR_ERR_SHAPE, "max_n must be >= 1");
    if (count_stride < 1) return no(GNR_ERR_ARG, "count_stride must be >= 1");
    Shape sh = shape_of(p, most);
    sh.pixels = 0; sh.max_n = max_n; sh.count_stride = count_stride;
    sh.blocks = (unsigned)(((unsigned long long)max_n + 255) / 256);
    const dim3 grid(sh.blocks < 65536u ? sh.blocks : 65536u, (unsigned)p->B, 1u);
    return launch<k_surface_color>("k_surface_color@gnr_surface_color_points_fwd", (hipStream_t)stream, grid, dim3(256), 0, vol, points, count,
                                   (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, images, poses, Ks, colors, weight, views, sh);
}

extern "C" int gnr_surface_color_pixels_fwd(const GnrSurfaceColorParams* p, const float* vol, const float* depth, const float* cam_poses,
                                            const float* cam_Ks, int Vc, int hc, int wc, const float* images, const float* poses,
                                            const float* Ks, float* colors, float* weight, int* views, void* stream) {
    const Refuse no{"gnr_surface_color_pixels_fwd"};
    if (!p || !vol || !depth || !cam_poses || !cam_Ks || !images || !poses || !Ks || !colors || !weight || !views)
        return no(GNR_ERR_ARG, "null pointer");
    double most = 0.0;
    if (const int rc = check(no, p, most)) return rc;
    if (Vc < 1) return no(GNR_ERR_SHAPE, "Vc must be >= 1");
    if (hc < 1 || wc < 1) return no(GNR_ERR_SHAPE, "hc and wc must be >= 1");
    const unsigned long long tiles_x = ((unsigned long long)wc + 7) / 8, tiles_y = ((unsigned long long)hc + 7) / 8;
    if (tiles_x * tiles_y > (1ull << 28)) return no(GNR_ERR_SHAPE, "hc and wc must give at most 2^28 tiles of 8 x 8 pixels");
    Shape sh = shape_of(p, most);
    sh.pixels = 1; sh.Vc = Vc; sh.hc = hc; sh.wc = wc;
    sh.tiles_x = (unsigned)tiles_x; sh.tiles = (unsigned)(tiles_x * tiles_y); sh.blocks = (unsigned)((tiles_x * tiles_y + 3) / 4);
    const dim3 grid(sh.blocks < 65536u ? sh.blocks : 65536u, (unsigned)p->B, (unsigned)(Vc < 64 ? Vc : 64));
    return launch<k_surface_color>("k_surface_color@gnr_surface_color_pixels_fwd", (hipStream_t)stream, grid, dim3(256), 0, vol,
                                   (const double*)nullptr, (const int*)nullptr, depth, cam_poses, cam_Ks, images, poses, Ks, colors, weight, views, sh);
}
