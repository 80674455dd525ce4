// The solid rule of the volume operators (gnr_volume_objects_fwd, gnr_volume_distance_fwd): voxel (i, j, k) of value v is solid when
//     lower < v < level  and  k >= z_min,
// compared in float64.  One device function for the kernels, one host function for the three refusals of its parameters.
#pragma once
#include <math.h>

#include "gnr_host.h"

namespace gnr {

// S: a kernel's own Shape, any struct with the fields level, lower (double) and z_min (int)
template <typename S>
__device__ inline bool solid_at(const S& sh, float v, int k) {
    const double x = (double)v;
    return sh.lower < x && x < sh.level && k >= sh.z_min;
}

static inline int check_solid(const Refuse& no, double level, double lower, int z_min, int R) {
    if (z_min < 0 || z_min > R) return no(GNR_ERR_ARG, "z_min must be in 0..R");
    if (!isfinite(level)) return no(GNR_ERR_ARG, "level must be finite");
    if (isnan(lower)) return no(GNR_ERR_ARG, "lower must not be a NaN (-inf: none)");
    return GNR_OK;
}

}  // namespace gnr
