// Gripper clearance of the ranked grasps against the volume, on the device: per grasp the smallest trilinear value of the volume over a
// lattice of samples of the hand's four boxes (two fingers, palm, tail), once with the hand at the grasp and once over everything the
// boxes pass through on the straight approach from the pre-grasp pose.  No reference counterpart (like gnr_mesh.hip, gnr_raycast.hip and
// gnr_surface_color.hip); the statement is include/gnr.h's and tests/hand_reference.py's.
// Mapping: one wavefront per grasp, four per block, grid (ceil(rows / 4), B), x strided.  The pose, the matrix and the four boxes'
// layouts are the same in every lane of a wavefront; box after box, the lanes stride over the box's samples and decode (i_x, i_y, i_z)
// by integer division.  Each lane keeps two running (value, ordinal) minima and two counts; a lane meets its ordinals in ascending
// order, so a strict `<` keeps the first.  The cross-lane step is a `__shfl_xor` butterfly on (value, ordinal) pairs -- the smaller value, on
// equal values (-0.0 and 0.0 included) the smaller ordinal -- so the result does not depend on how the samples were spread over the
// lanes; lane 0 stores.  The volume (40^3 floats = 256 KB) is read through the vector cache: L2 resident, too large for a block's LDS.
// Measured (tools/time_hand_clearance.py, profiles/hand_clearance.json; a 40^3 volume, p50): 2 048 rows of the viewer's hand (2.57 M
// samples inside the volume) 0.041 ms, of a 2 cm x 1 cm hand opened to 0.08 m (7.57 M) 0.087 ms, a top-10 list 0.026 ms.
// A wavefront per grasp leaves most of the device idle at small counts: a top_k = 10 list is 10 wavefronts on 3 CUs, each walking
// ~2 500 samples in 39 rounds of dependent loads, and costs two thirds of 2 048 rows.  Spreading one grasp over a block would shorten
// that at the price of an LDS step in the reduction; the mapping is the simplest that meets the constraints and is not tuned.
// Every loop is bounded by the parameters (the host refuses a hand whose widest opening, R voxels, has more than GNR_HAND_MAX_SAMPLES
// samples; the device clamps the width to [0, R] before it sizes anything) and every volume index goes through base_of's clamp, so no
// content of pos, quat, width or count reads out of bounds or runs long.  Plain loads and stores, nothing atomic, no workspace: every
// output is a pure function of the input bits.  Everything is float64, every operation one correctly rounded IEEE operation in the
// order written here (contraction is off for the whole file).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "gnr_host.h"
#include "gnr_trilinear.h"

#pragma clang fp contract(off)

namespace gnr_hand {

using namespace gnr;

struct Shape {
    int R, max_n, rows, count_stride;          // rows = min(top_k or max_n, max_n): the most rows a scene writes
    unsigned blocks;                           // of four rows
    double height, finger, tail, depth, opening, cell, approach, scale;
};

// one box: (lo, step, n) per axis, the z lattice's backward part m, and the number of its samples n_x n_y (n_z + m)
struct Box {
    double lo[3], step[3];
    int n[3], m, total;
};

// the sample lattice of one axis of extent e: n = fmax(2, ceil(e / cell) + 1), step = e / (n - 1).  (n as a double: the host sums the
// counts before anything is cast)
__host__ __device__ inline double count_of(double e, double cell) { return fmax(2.0, ceil(e / cell) + 1.0); }
__host__ __device__ inline double back_of(double approach, double step) { return approach > 0.0 ? ceil(approach / step) : 0.0; }

// the four boxes of a hand opened to w metres (w in [0, R * scale]: the counts fit an int by the host's check)
__device__ inline void layout(const Shape& sh, double w, Box (&box)[4]) {
    const double h = sh.height, f = sh.finger, t = sh.tail, d = sh.depth, hw = 0.5 * w;
    const double lo[4][3] = {{-0.5 * h, -hw - f, -f}, {-0.5 * h, hw, -f}, {-0.5 * h, -hw, -f}, {-0.5 * h, -0.5 * f, -t - f}};
    const double ext[4][3] = {{h, f, d + f}, {h, f, d + f}, {h, w, f}, {h, f, t}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double n = count_of(ext[k][a], sh.cell);
            box[k].lo[a] = lo[k][a];
            box[k].step[a] = ext[k][a] / (n - 1.0);
            box[k].n[a] = (int)n;
        }
        box[k].m = (int)back_of(sh.approach, box[k].step[2]);
        box[k].total = box[k].n[0] * box[k].n[1] * (box[k].n[2] + box[k].m);
    }
}

// (value, ordinal) minimum: the smaller value, on equal values the smaller ordinal (an empty pair holds ordinal INT32_MAX)
__device__ inline void take(double& v, int& o, double ov, int oo) {
    if (ov < v || (ov == v && oo < o)) { v = ov; o = oo; }
}

// launch grid: (blocks, B), x strided (B <= 65535);  block 256 = 4 wavefronts, wavefront j of block i owns row 4 i + j
__global__ __launch_bounds__(256) void k_hand_clearance(const float* __restrict__ vol, const double* __restrict__ pos,
                                                        const float* __restrict__ quat, const float* __restrict__ width,
                                                        const int* __restrict__ count, float* __restrict__ clearance,
                                                        int* __restrict__ worst, int* __restrict__ inside, Shape sh) {
    const int R = sh.R, b = blockIdx.y;
    const float* v = vol + (size_t)b * R * R * R;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const double top = (double)(R - 1);
    const int n = count[(size_t)b * sh.count_stride];
    const int rows = n < sh.rows ? n : sh.rows;                   // (a negative count: no row)
    for (unsigned blk = blockIdx.x; blk < sh.blocks; blk += gridDim.x) {
        const unsigned r = blk * 4u + wave;
        if (rows <= 0 || r >= (unsigned)rows) continue;           // wave-uniform: rows beyond the count are left untouched
        const size_t o = (size_t)b * sh.max_n + r;
        // ---- the pose and the boxes of this grasp (the same in every lane) --------------------------------------------------------
        double wv = sh.opening >= 0.0 ? sh.opening / sh.scale : (double)width[o];
        wv = fmin(fmax(wv, 0.0), (double)R);
        const double w = wv * sh.scale;
        Box box[4];
        layout(sh, w, box);
        double qx = (double)quat[o * 4 + 0], qy = (double)quat[o * 4 + 1], qz = (double)quat[o * 4 + 2], qw = (double)quat[o * 4 + 3];
        const double qn = fmax(__dsqrt_rn(((qx * qx + qy * qy) + qz * qz) + qw * qw), 1e-12);
        qx = qx / qn; qy = qy / qn; qz = qz / qn; qw = qw / qn;
        const double M[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)},
                                {2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)},
                                {2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)}};
        const double g[3] = {pos[o * 3 + 0], pos[o * 3 + 1], pos[o * 3 + 2]};
        // ---- this lane's samples: box after box, the lanes stride over a box's samples, so every lane meets ascending ordinals ----------
        double best[2] = {INFINITY, INFINITY};                    // [0] at the grasp, [1] on the approach
        int at[2] = {INT32_MAX, INT32_MAX}, in[2] = {0, 0};
        int first = 0;                                            // the ordinal of the box's first sample
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Box& bx = box[k];
            const int nz = bx.n[2] + bx.m, nyz = bx.n[1] * nz;
            for (int s = (int)lane; s < bx.total; s += 64) {
                const int ix = s / nyz, rem = s - ix * nyz;
                const int iy = rem / nz, iz = rem - iy * nz - bx.m;
                const double lx = bx.lo[0] + (double)ix * bx.step[0], ly = bx.lo[1] + (double)iy * bx.step[1],
                             lz = bx.lo[2] + (double)iz * bx.step[2];
                double p[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) p[a] = g[a] + ((M[a][0] * lx + M[a][1] * ly) + M[a][2] * lz) / sh.scale;
                if (!(0.0 <= p[0] && p[0] <= top && 0.0 <= p[1] && p[1] <= top && 0.0 <= p[2] && p[2] <= top)) continue;
                const double val = value_at(v, 1, R, p[0], p[1], p[2]);
                if (val < best[1]) { best[1] = val; at[1] = first + s; }
                in[1] += 1;
                if (iz >= 0) {
                    if (val < best[0]) { best[0] = val; at[0] = first + s; }
                    in[0] += 1;
                }
            }
            first += bx.total;
        }
        // ---- across the lanes ---------------------------------------------------------------------------------------------------------
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double ov = __shfl_xor(best[c], d);
                const int oo = __shfl_xor(at[c], d);
                take(best[c], at[c], ov, oo);
                in[c] += __shfl_xor(in[c], d);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                clearance[o * 2 + c] = (float)(in[c] > 0 ? fmin(best[c], 1.0) : 1.0);
                worst[o * 2 + c] = in[c] > 0 ? at[c] : -1;
                inside[o * 2 + c] = in[c];
            }
        }
    }
}

}  // namespace gnr_hand

using namespace gnr_hand;

extern "C" int gnr_hand_clearance_fwd(const GnrHandParams* p, const float* vol, const double* pos, const float* quat, const float* width,
                                      const int* count, int count_stride, int B, int R, int max_n, int top_k, float* clearance, int* worst,
                                      int* inside, void* stream) {
    const char* fn = "gnr_hand_clearance_fwd";
    char text[160];
    auto no = [&](int code, const char* what) { snprintf(text, sizeof text, "%s: %s", fn, what); return fail(code, text); };
    if (!p || !vol || !pos || !quat || !width || !count || !clearance || !worst || !inside) return no(GNR_ERR_ARG, "null pointer");
    if (B < 1 || B > 65535) return no(GNR_ERR_SHAPE, "B must be in 1..65535");
    if (R < 2 || R > 256) return no(GNR_ERR_SHAPE, "R must be in 2..256");
    if (max_n < 1) return no(GNR_ERR_SHAPE, "max_n must be >= 1");
    if (count_stride < 1) return no(GNR_ERR_ARG, "count_stride must be >= 1");
    if (top_k < 0) return no(GNR_ERR_ARG, "top_k must be >= 0 (0: every row)");
    const double dims[6] = {p->height, p->finger_width, p->tail_length, p->depth, p->spacing, p->scale};
    for (double x : dims)
        if (!isfinite(x) || !(x > 0.0)) return no(GNR_ERR_ARG, "height, finger_width, tail_length, depth, spacing and scale must be finite and > 0");
    if (!isfinite(p->approach) || !(p->approach >= 0.0)) return no(GNR_ERR_ARG, "approach must be finite and >= 0");
    if (!isfinite(p->opening)) return no(GNR_ERR_ARG, "opening must be finite (negative: each grasp's own width)");
    // the samples of the widest hand, R voxels: the same operations as the device's layout(), summed as doubles before any cast
    const double cell = p->spacing * p->scale, f = p->finger_width, wmax = (double)R * p->scale;
    const double ext[4][3] = {{p->height, f, p->depth + f}, {p->height, f, p->depth + f}, {p->height, wmax, f}, {p->height, f, p->tail_length}};
    double most = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double nz = count_of(ext[k][2], cell), m = back_of(p->approach, ext[k][2] / (nz - 1.0));
        most += count_of(ext[k][0], cell) * count_of(ext[k][1], cell) * (nz + m);
    }
    if (!(most <= (double)GNR_HAND_MAX_SAMPLES))
        return no(GNR_ERR_ARG, "spacing too small or approach too long, a grasp would take more than GNR_HAND_MAX_SAMPLES (4194304) samples");
    Shape sh{};
    sh.R = R; sh.max_n = max_n; sh.count_stride = count_stride;
    sh.rows = top_k > 0 && top_k < max_n ? top_k : max_n;
    sh.blocks = (unsigned)(((unsigned long long)sh.rows + 3) / 4);
    sh.height = p->height; sh.finger = f; sh.tail = p->tail_length; sh.depth = p->depth; sh.opening = p->opening;
    sh.cell = cell; sh.approach = p->approach; sh.scale = p->scale;
    const dim3 grid(sh.blocks < 65536u ? sh.blocks : 65536u, (unsigned)B, 1u);
    return launch<k_hand_clearance>("k_hand_clearance@gnr_hand_clearance_fwd", (hipStream_t)stream, grid, dim3(256), 0, vol, pos, quat, width,
                                    count, clearance, worst, inside, sh);
}
