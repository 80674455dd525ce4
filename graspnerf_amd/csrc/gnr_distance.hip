// Distance field of the volume, on the device: the exact Euclidean distance transform of the solid mask of B volumes -- per voxel the
// squared distance to the nearest solid voxel of its scene and that voxel's index, the same to the nearest free voxel, the signed
// metric field built from the two, and the label (gnr_volume_objects_fwd's) of the nearest solid voxel.  No reference counterpart (like
// gnr_objects.hip and gnr_hand.hip); the statement is include/gnr.h's and tests/distance_reference.py's.  Everything up to `esdf` is
// integer, so any order of execution gives the same bits; `esdf` is float64, one correctly rounded operation per line in the order of
// the header (contraction is off for the whole file, as in gnr_tsdf.hip), rounded once to float32.
// The transform is separable: three line passes, along k, then j, then i.  A pass gives every voxel x of a line
//     min over x' of g[x'] + (x - x')^2,   of several x' the smallest,
// and the site that x' carried.  With this order and tie rule the site that survives is the smallest linear index among the voxels
// that attain the distance (the pass along k leaves the smallest k' per (i', j'), the pass along j the smallest j' and with it the
// smallest k' of that j', the pass along i the smallest i').  A line is minimised by brute force over a copy of it in LDS: at most 256
// candidates per output, no branch that depends on the data beyond the select.
//   k_line_k      one workgroup per 32 lines along k (32 R contiguous voxels): reads vol, writes per voxel the nearest site of its
//                 own line (a linear index, -1: the line has none).  The value of that pass, (k - k')^2, is not stored: the next pass
//                 takes it from the index.
//   k_line<1>     along j: a tile of R x 32 voxels of one plane i, the 32 neighbours in k, so that a wavefront's loads and stores are
//                 two runs of 128 contiguous bytes; writes values and sites.
//   k_line<2>     along i, tiles of R x 32 over (j, k); writes the caller's d2 / nearest (3 R^2 / -1: the scene has no site).
//   k_field       per voxel esdf and nearest_label.
// The transform to the solid voxels and the one to the free voxels are the two z-slices of each launch's grid.  LDS holds the values
// only (33 words per row of 32: the pass along k fills it transposed); a thread that has found its x' fetches the site x' carried from
// global memory.  In the passes along j and i a thread keeps four outputs, 8 apart, per LDS read.
// No atomics, no communication between workgroups, every loop bounded by R, plain vector stores only.  Everything a call reads from
// its workspace it has written in the same call (a tile's rows beyond the lattice are filled in LDS, never read from memory), so a
// captured call replays.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_host.h"
#include "gnr_solid.h"

#pragma clang fp contract(off)

namespace gnr_distance {

using namespace gnr;

constexpr int KT = 32;                         // lines per tile: the neighbours in k (along j, i) that one half wavefront covers
constexpr int LS = KT + 1;                     // words per LDS row
constexpr int INF = 1 << 29;                   // "no site": above every real value (3 * 255^2), and INF + 3 * 255^2 fits an int

struct Shape {
    int R, n, cols;                            // n = R^3 voxels of a scene, cols = R^2 lines of a pass
    int z_min;
    double level, lower, scale, offset;
};
struct Out { int* p[2]; };                     // per transform: 0 to the solid voxels, 1 to the free ones
struct In { const int* p[2]; };

// launch grid: (ceil(R^2 / 32), B, transforms), 256 threads
__global__ __launch_bounds__(256) void k_line_k(const float* __restrict__ vol, Out site_out, Shape sh) {
    __shared__ int g[256 * LS];
    const int R = sh.R, tid = threadIdx.x, first = (int)blockIdx.x * KT * R;       // (first < R^3 <= 2^24)
    const bool want_solid = blockIdx.z == 0;
    const size_t scene = (size_t)blockIdx.y * sh.n;
    const int span = sh.n - first < KT * R ? sh.n - first : KT * R;                // the voxels of this tile inside the scene
    for (int e = tid; e < KT * R; e += 256) {
        const int x = e % R, col = e / R;
        int v = INF;
        if (e < span && solid_at(sh, vol[scene + first + e], x) == want_solid) v = 0;
        g[x * LS + col] = v;
    }
    __syncthreads();
    int* out = site_out.p[blockIdx.z] + scene + first;
    for (int e = tid; e < span; e += 256) {
        const int x = e % R, col = e / R;
        int best = INF, arg = 0;
        for (int xp = 0; xp < R; ++xp) {
            const int d = x - xp, c = g[xp * LS + col] + d * d;
            if (c < best) { best = c; arg = xp; }
        }
        out[e] = best < INF ? first + col * R + arg : -1;
    }
}

// launch grid: k_line_k's.  PASS 1: along j, values from the sites of the pass along k;  PASS 2: along i, the last.
template <int PASS>
__global__ __launch_bounds__(256) void k_line(In val_in, In site_in, Out val_out, Out site_out, Shape sh) {
    __shared__ int g[256 * LS];
    const int R = sh.R, tid = threadIdx.x, col = tid % KT, c = (int)blockIdx.x * KT + col, t = blockIdx.z;
    const bool live = c < sh.cols;
    const size_t scene = (size_t)blockIdx.y * sh.n;
    const int stride = PASS == 1 ? R : R * R;
    const int base = PASS == 1 ? (c / R) * R * R + c % R : c;                      // voxel 0 of line c (base + 255 * stride < 2^25)
    const int* sites = site_in.p[t] + scene;
    for (int x = tid / KT; x < R; x += 256 / KT) {
        int v = INF;
        if (live) {
            if (PASS == 1) {
                const int s = sites[base + x * stride];
                if (s >= 0) { const int d = c % R - s % R; v = d * d; }
            } else {
                v = val_in.p[t][scene + base + x * stride];
            }
        }
        g[x * LS + col] = v;
    }
    __syncthreads();
    if (!live) return;
    for (int x0 = tid / KT; x0 < R; x0 += 4 * (256 / KT)) {
        int best[4], arg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { best[u] = INT32_MAX; arg[u] = 0; }
        for (int xp = 0; xp < R; ++xp) {
            const int v = g[xp * LS + col];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = x0 + u * (256 / KT) - xp, cand = v + d * d;
                if (cand < best[u]) { best[u] = cand; arg[u] = xp; }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int x = x0 + u * (256 / KT);
            if (x >= R) continue;
            const size_t o = scene + base + x * stride;
            const int s = sites[base + arg[u] * stride];
            val_out.p[t][o] = PASS == 2 && best[u] >= INF ? 3 * R * R : best[u];
            site_out.p[t][o] = s;
        }
    }
}

// launch grid: (ceil(n / 256), B), 256 threads
__global__ __launch_bounds__(256) void k_field(const float* __restrict__ vol, const int* __restrict__ d2_solid, const int* __restrict__ d2_free,
                                               const int* __restrict__ nearest_solid, const int* __restrict__ labels,
                                               float* __restrict__ esdf, int* __restrict__ nearest_label, Shape sh) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= sh.n) return;
    const size_t scene = (size_t)blockIdx.y * sh.n, o = scene + i;
    if (esdf) {
        const bool solid = solid_at(sh, vol[o], i % sh.R);
        double t = sqrt((double)(solid ? d2_free[o] : d2_solid[o]));
        t = t - sh.offset;
        t = t * sh.scale;
        esdf[o] = (float)(solid ? -t : t);
    }
    if (nearest_label) {
        const int s = nearest_solid[o];
        nearest_label[o] = s >= 0 ? labels[scene + s] : 0;
    }
}

// the workspace: per transform the sites of the pass along k, then the values and the sites of the pass along j.  The pass along i
// writes a free pair the caller did not ask for over the two site arrays of the pass along k, which nothing reads any more.
struct Work { Out site_k, val_j, site_j; size_t total; };

static Work carve(int B, int R, void* base) {
    const size_t n = (size_t)B * R * R * R;
    Carve c(base);
    Work k;
    for (int t = 0; t < 2; ++t) { k.site_k.p[t] = c.take<int>(n); k.val_j.p[t] = c.take<int>(n); k.site_j.p[t] = c.take<int>(n); }
    k.total = c.total();
    return k;
}

}  // namespace gnr_distance

using namespace gnr_distance;

extern "C" size_t gnr_volume_distance_workspace_bytes(int B, int R) {
    return scenes_ok(B) && lattice_ok(R) ? carve(B, R, nullptr).total : 0;
}

extern "C" int gnr_volume_distance_fwd(const GnrDistanceParams* p, const float* vol, const int* labels, int B, int R, int* d2_solid,
                                       int* nearest_solid, int* d2_free, int* nearest_free, float* esdf, int* nearest_label, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const Refuse no{"gnr_volume_distance_fwd"};
    if (!p || !vol || !d2_solid || !nearest_solid || !workspace) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_ARG, B)) return rc;         // GNR_ERR_ARG where the siblings say GNR_ERR_SHAPE: the tests pin it
    if (int rc = check_lattice(no, GNR_ERR_ARG, R)) return rc;
    if (int rc = check_solid(no, p->level, p->lower, p->z_min, R)) return rc;
    if (!(isfinite(p->scale) && p->scale > 0)) return no(GNR_ERR_ARG, "scale must be finite and > 0");
    if (!(isfinite(p->surface_offset) && p->surface_offset >= 0)) return no(GNR_ERR_ARG, "surface_offset must be finite and >= 0");
    if (nearest_label && !labels) return no(GNR_ERR_ARG, "nearest_label needs labels");
    if (!d2_free != !nearest_free) return no(GNR_ERR_ARG, "d2_free and nearest_free go together");
    const Work k = carve(B, R, workspace);
    if (workspace_bytes < k.total) return no(GNR_ERR_WORKSPACE, "workspace too small");
    Shape sh{};
    sh.R = R; sh.n = R * R * R; sh.cols = R * R;
    sh.z_min = p->z_min; sh.level = p->level; sh.lower = p->lower; sh.scale = p->scale; sh.offset = p->surface_offset;
    const unsigned transforms = d2_free || esdf ? 2u : 1u;
    if (!d2_free) { d2_free = k.site_k.p[0]; nearest_free = k.site_k.p[1]; }       // (read by k_field alone, and only with esdf)
    const Out d2{{d2_solid, d2_free}}, nearest{{nearest_solid, nearest_free}};
    auto in = [](const Out& o) { return In{{o.p[0], o.p[1]}}; };
    hipStream_t st = (hipStream_t)stream;
    const dim3 lines((unsigned)((sh.cols + KT - 1) / KT), (unsigned)B, transforms);
    if (int rc = launch<k_line_k>("k_line_k@gnr_volume_distance_fwd", st, lines, dim3(256), 0, vol, k.site_k, sh)) return rc;
    if (int rc = launch<k_line<1>>("k_line_j@gnr_volume_distance_fwd", st, lines, dim3(256), 0, In{{nullptr, nullptr}}, in(k.site_k), k.val_j, k.site_j, sh)) return rc;
    if (int rc = launch<k_line<2>>("k_line_i@gnr_volume_distance_fwd", st, lines, dim3(256), 0, in(k.val_j), in(k.site_j), d2, nearest, sh)) return rc;
    if (!esdf && !nearest_label) return GNR_OK;
    return launch<k_field>("k_field@gnr_volume_distance_fwd", st, dim3((unsigned)((sh.n + 255) / 256), (unsigned)B), dim3(256), 0, vol,
                           (const int*)d2_solid, (const int*)d2_free, (const int*)nearest_solid, labels, esdf, nearest_label, sh);
}
