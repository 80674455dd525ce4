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
// The second kernel of the file, k_finger_closure (further down, with its own notes), closes the fingers of the same hand on the
// volume; the two share the opening, the pose, the placement of a local point and the launch shape.  The third, k_grasp_objects
// (gnr_grasp_objects_fwd), shares them too: it reads gnr_objects.hip's label volume at the samples between the pads.
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

// the opening in metres of a row whose own width is `own` voxels: one opening for every grasp or the row's, clamped to [0, R] voxels
__device__ inline double width_of(const Shape& sh, float own) {
    const double wv = sh.opening >= 0.0 ? sh.opening / sh.scale : (double)own;
    return fmin(fmax(wv, 0.0), (double)sh.R) * sh.scale;
}

// the pose of a grasp: the matrix of its quaternion (x, y, z, w; divided by fmax(|q|, 1e-12)) and its position in lattice units
__device__ inline void pose_of(const float* __restrict__ q, const double* __restrict__ pos, double (&M)[3][3], double (&g)[3]) {
    double qx = (double)q[0], qy = (double)q[1], qz = (double)q[2], qw = (double)q[3];
    const double qn = fmax(__dsqrt_rn(((qx * qx + qy * qy) + qz * qz) + qw * qw), 1e-12);
    qx = qx / qn; qy = qy / qn; qz = qz / qn; qw = qw / qn;
    const double m[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)},
                            {2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)},
                            {2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)}};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g[a] = pos[a];
#pragma unroll
        for (int c = 0; c < 3; ++c) M[a][c] = m[a][c];
    }
}

// the lattice position of the hand-local point (lx, ly, lz) metres
__device__ inline void place(const double (&M)[3][3], const double (&g)[3], double scale, double lx, double ly, double lz, double (&p)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = g[a] + ((M[a][0] * lx + M[a][1] * ly) + M[a][2] * lz) / scale;
}

// whether every component of p lies in [0, top] (a NaN does not)
__device__ inline bool within(const double (&p)[3], double top) {
    return 0.0 <= p[0] && p[0] <= top && 0.0 <= p[1] && p[1] <= top && 0.0 <= p[2] && p[2] <= top;
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
        const double w = width_of(sh, width[o]);
        Box box[4];
        layout(sh, w, box);
        double M[3][3], g[3];
        pose_of(quat + o * 4, pos + o * 3, M, g);
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
                place(M, g, sh.scale, lx, ly, lz, p);
                if (!within(p, top)) continue;
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

// ---- finger closure -----------------------------------------------------------------------------------------------------------------
// Per grasp: where the two fingers stop when the hand closes.  Each finger's inner face carries n_x n_z pad rays; a ray marches
// f(t) = value - level along the closing direction from the open position (t = 0) to the centre plane (t = hw) in n_y steps, brackets the
// first change from f >= 0 to f < 0, halves the bracket `bisections` times and takes one secant step (the ray cast's refinement).  A finger
// stops at the smallest t* of its rays; at that point the gradient of the trilinear interpolant gives the cosine of the grip.
// Mapping: k_hand_clearance's -- one wavefront per grasp, four per block, the lanes stride over the 2 n_x n_z (finger, ray) pairs, each
// lane marches and refines its own rays (a lane meets a finger's ordinals in ascending order: a strict `<` keeps the first).  The march
// ends at a different k in every lane and only the lanes with a bracket refine; all of them are past their loops before the
// `__shfl_xor` butterfly on the (travel, ordinal) pairs of the two fingers, which uses take()'s rule, so the result does not depend on how
// the rays fell on the lanes.  Lanes 0 and 1 then hold both winners; lane c evaluates finger c's gradient and stores its columns.
// Not tuned: the viewer's hand has 90 pairs, so 26 lanes do two rays and 38 one, and a short list is a handful of wavefronts (as for
// the clearance); a ray's samples are dependent loads from the L2-resident volume.  Timings: tools/time_finger_closure.py.
struct Closure {
    double level;
    int bisections;
};

// the pad rays of one axis: n = fmax(2, ceil(e / cell) + 1) is count_of's; the march of a finger that travels hw metres at most
__host__ __device__ inline double march_of(double hw, double cell) { return fmax(1.0, ceil(hw / cell)); }

// the gradient (lattice units) of the trilinear interpolant at p: value_at's base corners and t's
__device__ inline void gradient_at(const float* __restrict__ c, int R, const double (&p)[3], double (&gr)[3]) {
    double tx, ty, tz;
    const int ix = base_of(p[0], R, tx), iy = base_of(p[1], R, ty), iz = base_of(p[2], R, tz);
    const size_t sy = (size_t)R, sx = (size_t)R * R;
    c += ((size_t)ix * R + iy) * sy + (size_t)iz;
    const double c000 = (double)c[0], c001 = (double)c[1], c010 = (double)c[sy], c011 = (double)c[sy + 1];
    const double c100 = (double)c[sx], c101 = (double)c[sx + 1], c110 = (double)c[sx + sy], c111 = (double)c[sx + sy + 1];
    const double c00 = c000 + tz * (c001 - c000), c01 = c010 + tz * (c011 - c010);
    const double c10 = c100 + tz * (c101 - c100), c11 = c110 + tz * (c111 - c110);
    const double c0 = c00 + ty * (c01 - c00), c1 = c10 + ty * (c11 - c10);
    gr[0] = c1 - c0;
    const double e0 = c01 - c00, e1 = c11 - c10;
    gr[1] = e0 + tx * (e1 - e0);
    const double d00 = c001 - c000, d01 = c011 - c010, d10 = c101 - c100, d11 = c111 - c110;
    const double d0 = d00 + ty * (d01 - d00), d1 = d10 + ty * (d11 - d10);
    gr[2] = d0 + tx * (d1 - d0);
}

// launch grid and rows: k_hand_clearance's
__global__ __launch_bounds__(256) void k_finger_closure(const float* __restrict__ vol, const double* __restrict__ pos,
                                                        const float* __restrict__ quat, const float* __restrict__ width,
                                                        const int* __restrict__ count, float* __restrict__ travel,
                                                        float* __restrict__ cosine, int* __restrict__ contact, float* __restrict__ closed,
                                                        Shape sh, Closure cl) {
    const int R = sh.R, b = blockIdx.y;
    const float* v = vol + (size_t)b * R * R * R;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const double top = (double)(R - 1);
    const int n = count[(size_t)b * sh.count_stride];
    const int rows = n < sh.rows ? n : sh.rows;                   // (a negative count: no row)
    // the pad rays are the same for every grasp
    const double nxd = count_of(sh.height, sh.cell), nzd = count_of(sh.depth, sh.cell);
    const double sx = sh.height / (nxd - 1.0), sz = sh.depth / (nzd - 1.0);
    const int nz = (int)nzd, rays = (int)nxd * nz;
    for (unsigned blk = blockIdx.x; blk < sh.blocks; blk += gridDim.x) {
        const unsigned r = blk * 4u + wave;
        if (rows <= 0 || r >= (unsigned)rows) continue;           // wave-uniform: rows beyond the count are left untouched
        const size_t o = (size_t)b * sh.max_n + r;
        // ---- the pose and the travel of this grasp (the same in every lane) -------------------------------------------------------
        const double hw = 0.5 * width_of(sh, width[o]);
        double M[3][3], g[3];
        pose_of(quat + o * 4, pos + o * 3, M, g);
        const double nyd = march_of(hw, sh.cell), ds = hw / nyd;
        const int ny = (int)nyd;
        // the lattice position of ray `ray` of finger c after a travel of t
        auto at = [&](int c, int ray, double t, double (&p)[3]) {
            const int ix = ray / nz, iz = ray - ix * nz;
            const double u = hw - t;
            place(M, g, sh.scale, -0.5 * sh.height + (double)ix * sx, c ? u : -u, (double)iz * sz, p);
        };
        // ---- this lane's rays --------------------------------------------------------------------------------------------------------
        double best[2] = {INFINITY, INFINITY};                    // the smallest t* of finger 0 and of finger 1
        int who[2] = {INT32_MAX, INT32_MAX};
        for (int s = (int)lane; s < 2 * rays; s += 64) {
            const int c = s >= rays ? 1 : 0, ray = s - c * rays;
            auto f = [&](double t) {
                double p[3];
                at(c, ray, t, p);
                return (within(p, top) ? value_at(v, 1, R, p[0], p[1], p[2]) : 1.0) - cl.level;
            };
            double A = fmin(0.0 * ds, hw), fA = f(A), B = 0.0, fB = 0.0, t = 0.0;
            if (!(fA < 0.0)) {                                    // (else the pad starts inside: t* = 0)
                bool hit = false;
                for (int k = 1; k <= ny; ++k) {
                    const double tk = fmin((double)k * ds, hw), fk = f(tk);
                    if (fA >= 0.0 && fk < 0.0) { B = tk; fB = fk; hit = true; break; }
                    A = tk; fA = fk;
                }
                if (!hit) continue;
                for (int i = 0; i < cl.bisections; ++i) {
                    const double m = 0.5 * (A + B), fm = f(m);
                    if (fm < 0.0) { B = m; fB = fm; } else { A = m; fA = fm; }
                }
                t = A + (B - A) * (fA / (fA - fB));
            }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (c == k && t < best[k]) { best[k] = t; who[k] = ray; }
        }
        // ---- across the lanes (every lane is past its loops) -------------------------------------------------------------------------
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double ot = __shfl_xor(best[c], d);
                const int oo = __shfl_xor(who[c], d);
                take(best[c], who[c], ot, oo);
            }
        }
        const double T0 = who[0] != INT32_MAX ? best[0] : hw, T1 = who[1] != INT32_MAX ? best[1] : hw;
        if (lane < 2) {
            const int c = (int)lane, ray = c ? who[1] : who[0];
            const double T = c ? T1 : T0;
            double cs = 0.0;
            if (ray != INT32_MAX) {
                double p[3], gr[3];
                at(c, ray, T, p);
                gradient_at(v, R, p, gr);
                const double dot = (gr[0] * M[0][1] + gr[1] * M[1][1]) + gr[2] * M[2][1];
                const double norm = fmax(__dsqrt_rn((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]), 1e-12);
                cs = c ? dot / norm : -dot / norm;
            }
            travel[o * 2 + c] = (float)T;
            cosine[o * 2 + c] = (float)cs;
            contact[o * 2 + c] = ray != INT32_MAX ? ray : -1;
            if (c == 0) closed[o] = (float)((hw - T0) + (hw - T1));
        }
    }
}

// ---- which object a grasp closes on ----------------------------------------------------------------------------------------------------
// Per grasp: the samples of one box, the closing region between the pads, vote for the label (gnr_volume_objects_fwd's) at their
// nearest voxel.  Mapping and rows: k_hand_clearance's.  No histogram is kept: pass after pass, the lanes stride over the samples and
// find the smallest label above the last pass's and its votes (a min and two sums over the lanes), so the labels are met in ascending
// order and a strict `>` keeps the smaller of two labels with equal votes.  One pass per different label and one that finds none: two
// or three for a hand between objects; the bound is the number of samples.  Integers throughout, any order of the lanes.
__global__ __launch_bounds__(256) void k_grasp_objects(const int* __restrict__ labels, const double* __restrict__ pos,
                                                       const float* __restrict__ quat, const float* __restrict__ width,
                                                       const int* __restrict__ count, int* __restrict__ object, int* __restrict__ votes,
                                                       int* __restrict__ distinct, int* __restrict__ inside, Shape sh) {
    const int R = sh.R, b = blockIdx.y;
    const int* lab = labels + (size_t)b * R * R * R;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const double top = (double)(R - 1);
    const int n = count[(size_t)b * sh.count_stride];
    const int rows = n < sh.rows ? n : sh.rows;                   // (a negative count: no row)
    for (unsigned blk = blockIdx.x; blk < sh.blocks; blk += gridDim.x) {
        const unsigned r = blk * 4u + wave;
        if (rows <= 0 || r >= (unsigned)rows) continue;           // wave-uniform: rows beyond the count are left untouched
        const size_t o = (size_t)b * sh.max_n + r;
        const double w = width_of(sh, width[o]);
        const double lo[3] = {-0.5 * sh.height, -(0.5 * w), 0.0}, ext[3] = {sh.height, w, sh.depth};
        double step[3];
        int nn[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double na = count_of(ext[a], sh.cell);
            step[a] = ext[a] / (na - 1.0);
            nn[a] = (int)na;
        }
        const int nyz = nn[1] * nn[2], total = nn[0] * nyz;
        double M[3][3], g[3];
        pose_of(quat + o * 4, pos + o * 3, M, g);
        int cur = 0, best = 0, most = 0, kinds = 0, in = 0;
        for (int pass = 0; pass <= total; ++pass) {
            int mn = INT32_MAX, cnt = 0, taken = 0;               // the smallest label above `cur` this lane met, its votes, the samples taken
            for (int s = (int)lane; s < total; s += 64) {
                const int ix = s / nyz, rem = s - ix * nyz;
                const int iy = rem / nn[2], iz = rem - iy * nn[2];
                double p[3];
                place(M, g, sh.scale, lo[0] + (double)ix * step[0], lo[1] + (double)iy * step[1], lo[2] + (double)iz * step[2], p);
                if (!within(p, top)) continue;
                taken += 1;
                const int vi = (int)floor(p[0] + 0.5), vj = (int)floor(p[1] + 0.5), vk = (int)floor(p[2] + 0.5);   // in 0 .. R-1
                const int L = lab[((size_t)vi * R + vj) * R + vk];
                if (L > cur) {
                    if (L < mn) { mn = L; cnt = 1; }
                    else if (L == mn) cnt += 1;
                }
            }
            int low = mn;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { const int ol = __shfl_xor(low, d); low = ol < low ? ol : low; }
            int c = mn == low ? cnt : 0;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { c += __shfl_xor(c, d); taken += __shfl_xor(taken, d); }
            if (pass == 0) in = taken;
            if (low == INT32_MAX) break;                          // (the same in every lane)
            kinds += 1;
            if (c > most) { best = low; most = c; }
            cur = low;
        }
        if (lane == 0) { object[o] = best; votes[o] = most; distinct[o] = kinds; inside[o] = in; }
    }
}

}  // namespace gnr_hand

using namespace gnr_hand;

// The refusals the two entry points share, in one order and one text each, and the shape of the launch.  `pointers`: none is null.
static int shape_of(const Refuse& no, const GnrHandParams* p, bool pointers, int count_stride, int B, int R, int max_n, int top_k, Shape& sh) {
    if (!p || !pointers) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (max_n < 1) return no(GNR_ERR_SHAPE, "max_n must be >= 1");
    if (count_stride < 1) return no(GNR_ERR_ARG, "count_stride must be >= 1");
    if (top_k < 0) return no(GNR_ERR_ARG, "top_k must be >= 0 (0: every row)");
    const double dims[6] = {p->height, p->finger_width, p->tail_length, p->depth, p->spacing, p->scale};
    for (double x : dims)
        if (!isfinite(x) || !(x > 0.0)) return no(GNR_ERR_ARG, "height, finger_width, tail_length, depth, spacing and scale must be finite and > 0");
    if (!isfinite(p->approach) || !(p->approach >= 0.0)) return no(GNR_ERR_ARG, "approach must be finite and >= 0");
    if (!isfinite(p->opening)) return no(GNR_ERR_ARG, "opening must be finite (negative: each grasp's own width)");
    sh = Shape{};
    sh.R = R; sh.max_n = max_n; sh.count_stride = count_stride;
    sh.rows = top_k > 0 && top_k < max_n ? top_k : max_n;
    sh.blocks = (unsigned)(((unsigned long long)sh.rows + 3) / 4);
    sh.height = p->height; sh.finger = p->finger_width; sh.tail = p->tail_length; sh.depth = p->depth; sh.opening = p->opening;
    sh.cell = p->spacing * p->scale; sh.approach = p->approach; sh.scale = p->scale;
    return GNR_OK;
}

static dim3 grid_of(const Shape& sh, int B) { return dim3(sh.blocks < 65536u ? sh.blocks : 65536u, (unsigned)B, 1u); }

extern "C" int gnr_hand_clearance_fwd(const GnrHandParams* p, const float* vol, const double* pos, const float* quat, const float* width,
                                      const int* count, int count_stride, int B, int R, int max_n, int top_k, float* clearance, int* worst,
                                      int* inside, void* stream) {
    const Refuse no{"gnr_hand_clearance_fwd"};
    Shape sh;
    if (int rc = shape_of(no, p, vol && pos && quat && width && count && clearance && worst && inside, count_stride, B, R, max_n, top_k, sh)) return rc;
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
    return launch<k_hand_clearance>("k_hand_clearance@gnr_hand_clearance_fwd", (hipStream_t)stream, grid_of(sh, B), dim3(256), 0, vol, pos, quat,
                                    width, count, clearance, worst, inside, sh);
}

extern "C" int gnr_finger_closure_fwd(const GnrHandParams* p, double level, int bisections, const float* vol, const double* pos,
                                      const float* quat, const float* width, const int* count, int count_stride, int B, int R, int max_n,
                                      int top_k, float* travel, float* cosine, int* contact, float* closed, void* stream) {
    const Refuse no{"gnr_finger_closure_fwd"};
    Shape sh;
    if (int rc = shape_of(no, p, vol && pos && quat && width && count && travel && cosine && contact && closed, count_stride, B, R, max_n, top_k, sh))
        return rc;
    if (!isfinite(level)) return no(GNR_ERR_ARG, "level must be finite");
    if (bisections < 0 || bisections > 16) return no(GNR_ERR_ARG, "bisections must be in 0..16");
    // the volume reads of the widest hand, R voxels: the device's counts, as doubles before any cast
    const double rays = 2.0 * count_of(p->height, sh.cell) * count_of(p->depth, sh.cell);
    const double most = rays * (march_of(0.5 * ((double)R * p->scale), sh.cell) + 1.0 + (double)bisections + 2.0);
    if (!(most <= (double)GNR_HAND_MAX_SAMPLES))
        return no(GNR_ERR_ARG, "spacing too small, a grasp would take more than GNR_HAND_MAX_SAMPLES (4194304) volume reads");
    const Closure cl{level, bisections};
    return launch<k_finger_closure>("k_finger_closure@gnr_finger_closure_fwd", (hipStream_t)stream, grid_of(sh, B), dim3(256), 0, vol, pos, quat,
                                    width, count, travel, cosine, contact, closed, sh, cl);
}

extern "C" int gnr_grasp_objects_fwd(const GnrHandParams* p, const int* labels, const double* pos, const float* quat, const float* width,
                                     const int* count, int count_stride, int B, int R, int max_n, int top_k, int* object, int* votes,
                                     int* distinct, int* inside, void* stream) {
    const Refuse no{"gnr_grasp_objects_fwd"};
    Shape sh;
    if (int rc = shape_of(no, p, labels && pos && quat && width && count && object && votes && distinct && inside, count_stride, B, R, max_n, top_k, sh))
        return rc;
    // the samples of the widest hand, R voxels: the device's counts, as doubles before any cast
    const double most = count_of(p->height, sh.cell) * count_of((double)R * p->scale, sh.cell) * count_of(p->depth, sh.cell);
    if (!(most <= (double)GNR_HAND_MAX_SAMPLES))
        return no(GNR_ERR_ARG, "spacing too small, a grasp would take more than GNR_HAND_MAX_SAMPLES (4194304) samples");
    return launch<k_grasp_objects>("k_grasp_objects@gnr_grasp_objects_fwd", (hipStream_t)stream, grid_of(sh, B), dim3(256), 0, labels, pos, quat,
                                   width, count, object, votes, distinct, inside, sh);
}
