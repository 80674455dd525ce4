// The trilinear value of a scalar (or interleaved) float32 volume in float64, shared by the ray cast (gnr_raycast.hip) and the view
// colours (gnr_surface_color.hip): include/gnr.h's `trilinear`.  Device code only; contraction is off in every function here (as in
// the files that include it), so every operation below is one correctly rounded IEEE operation in the order written.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace gnr {

// the base corner b = clamp(floor(p), 0, R-2) and t = p - b of one axis (fmax drops a NaN: the index is in range whatever p holds)
__device__ inline int base_of(double p, int R, double& t) {
#pragma clang fp contract(off)
    const double b = fmin(fmax(floor(p), 0.0), (double)(R - 2));
    t = p - b;
    return (int)b;
}

// trilinear value at the index position (px, py, pz) of a field whose voxel (x,y,z) sits at c[(x R R + y R + z) * stride]: the eight
// float32 corners convert to float64; z first, then y, then x, each a + t (b - a)
__device__ inline double value_at(const float* __restrict__ c, size_t stride, int R, double px, double py, double pz) {
#pragma clang fp contract(off)
    double tx, ty, tz;
    const int ix = base_of(px, R, tx), iy = base_of(py, R, ty), iz = base_of(pz, R, tz);
    const size_t sz = stride, sy = (size_t)R * stride, sx = (size_t)R * R * stride;
    c += ((size_t)ix * R + iy) * sy + (size_t)iz * sz;
    const double c000 = (double)c[0], c001 = (double)c[sz], c010 = (double)c[sy], c011 = (double)c[sy + sz];
    const double c100 = (double)c[sx], c101 = (double)c[sx + sz], c110 = (double)c[sx + sy], c111 = (double)c[sx + sy + sz];
    const double c00 = c000 + tz * (c001 - c000), c01 = c010 + tz * (c011 - c010);
    const double c10 = c100 + tz * (c101 - c100), c11 = c110 + tz * (c111 - c110);
    const double c0 = c00 + ty * (c01 - c00), c1 = c10 + ty * (c11 - c10);
    return c0 + tx * (c1 - c0);
}

// ... at the index position e + s d
__device__ inline double value_at(const float* __restrict__ c, size_t stride, int R, const double (&e)[3], const double (&d)[3], double s) {
#pragma clang fp contract(off)
    return value_at(c, stride, R, e[0] + s * d[0], e[1] + s * d[1], e[2] + s * d[2]);
}

}  // namespace gnr
