// Objects of the volume, on the device: connected-component labelling of the solid voxels of B volumes, with ndimage.label's numbering
// (components in raster order of their first voxel), per component its size, box and coordinate sums, and a copy of the volume with the
// small components set to free.  No reference counterpart (like gnr_mesh.hip and gnr_hand.hip); the statement is include/gnr.h's and
// tests/objects_reference.py's.  Everything is integer beyond the one threshold compare, so any order of execution gives the same bits.
// Union-find in global memory over int32 parents (a voxel's index inside its own scene; -1: not solid), as six launches:
//   k_init     parent = own index where solid, -1 elsewhere; sizes 0; the status word 0; the statistics rows to their empty values.
//   k_union    each solid voxel unites with its solid neighbours of smaller index (3 / 9 / 13 of them); find() and unite() are
//              gnr_union.h's (shared with gnr_parts.hip): the larger root hooks under the smaller with an atomic min, so a tree's root
//              is its smallest index.
//   k_flatten  parent = root, for every solid voxel; the sizes, added at the root voxel (one add per wavefront and root); the roots of
//              each chunk of 1024 voxels counted (gnr_compact.h).
//   k_scan     the chunk counts scanned per scene; their sum is the scene's count.
//   k_rank     every root takes label 1 + its rank among the roots of its scene, and, when that is a statistics row, stores its size.
//   k_label    labels of the other voxels (the root's), the boxes and sums (one atomic per wavefront, label and column), `cleaned`.
// Visibility (gnr_union.h states the rules).  k_union and k_flatten change parent[] while other workgroups follow it: every access to
// parent[] in those two launches is an agent-scope relaxed atomic through a global pointer.  A kernel boundary makes the next launch's
// plain loads safe: k_rank and k_label read parent[], size[] and the root labels plainly.
// No thread ever waits for another.  Every loop carries a bound from the parameters: a find follows at most R^3 links, a unite retries
// at most R^3 times; running into the bound sets GNR_OBJECTS_STATUS_BOUND in the status word (the first int of the workspace) and ends
// the loop.
// Everything a call reads from its workspace it has written in the same call (k_init), so a captured call replays.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_host.h"
#include "gnr_solid.h"
#include "gnr_union.h"

namespace gnr_objects {

using namespace gnr;
static_assert(UNION_STATUS_BOUND == GNR_OBJECTS_STATUS_BOUND, "find() and unite() flag the status word's bound bit");

struct Shape {
    int R, n, nc;                              // n = R^3 voxels of a scene, nc chunks of 1024 of them
    int z_min, order, max_objects, min_voxels; // order: how many axes a neighbour may differ in (1, 2, 3 for 6, 18, 26)
    double level, lower;
    float free_value;
};

// launch grid: (ceil(n / 256), B), 256 threads.  The rows of the statistics are spread over all threads of the grid.
__global__ __launch_bounds__(256) void k_init(const float* __restrict__ vol, int* __restrict__ parent, int* __restrict__ size,
                                              int* __restrict__ status, int* __restrict__ voxels, int* __restrict__ bbox,
                                              unsigned long long* __restrict__ sums, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), b = blockIdx.y;
    if (t < sh.n) {
        const size_t o = (size_t)b * sh.n + t;
        parent[o] = solid_at(sh, vol[o], t % sh.R) ? t : -1;
        size[o] = 0;
    }
    const size_t threads = (size_t)gridDim.x * gridDim.y * 256u, me = ((size_t)b * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
    if (me == 0) *status = 0;
    const size_t rows = (size_t)gridDim.y * (size_t)sh.max_objects;
    for (size_t r = me; r < rows; r += threads) {
        voxels[r] = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) { bbox[r * 6 + a] = sh.R; bbox[r * 6 + 3 + a] = -1; sums[r * 3 + a] = 0ull; }
    }
}

// launch grid: k_init's
__global__ __launch_bounds__(256) void k_union(int* parent_all, int* status, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), R = sh.R;
    if (t >= sh.n) return;
    int* parent = parent_all + (size_t)blockIdx.y * sh.n;
    if (ld(parent + t) < 0) return;
    const int k = t % R, j = (t / R) % R, i = t / (R * R);
    for (int c = 0; c < 13; ++c) {             // the 13 offsets (di, dj, dk) of the 3x3x3 block in front of its centre, in raster order
        const int di = c / 9 - 1, dj = (c / 3) % 3 - 1, dk = c % 3 - 1;
        if ((di != 0) + (dj != 0) + (dk != 0) > sh.order) continue;
        const int ii = i + di, jj = j + dj, kk = k + dk;
        if (ii < 0 || jj < 0 || jj >= R || kk < 0 || kk >= R) continue;       // (ii <= i < R)
        const int nb = (ii * R + jj) * R + kk;
        if (ld(parent + nb) < 0) continue;
        unite(parent, t, nb, sh.n, status);
    }
}

// launch grid: (nc, B), 1024 threads; every thread stays to the end (ballots, the workgroup's rank)
__global__ __launch_bounds__(1024) void k_flatten(int* parent_all, int* size_all, int* __restrict__ chunk, int* status, Shape sh) {
    __shared__ int wave_tot[16];
    const int t = (int)(blockIdx.x * 1024u + threadIdx.x), b = blockIdx.y, lane = threadIdx.x & 63;
    int* parent = parent_all + (size_t)b * sh.n;
    int* size = size_all + (size_t)b * sh.n;
    int r = -1;
    if (t < sh.n) {
        const int p = ld(parent + t);
        if (p >= 0) {
            r = find(parent, t, sh.n, status);
            if (r != p) st(parent + t, r);
        }
    }
    // sizes: one add per wavefront and root
    unsigned long long todo = __ballot(r >= 0);
    for (int s = 0; s < 64 && todo; ++s) {
        const int lead = __ffsll((long long)todo) - 1;
        const int rl = __shfl(r, lead);
        const unsigned long long m = __ballot(r == rl);
        if (lane == lead) atomicAdd(size + rl, __popcll(m));
        todo &= ~m;
    }
    int tot;
    block_rank(r >= 0 && r == t, wave_tot, tot);
    if (threadIdx.x == 0) chunk[(size_t)b * sh.nc + blockIdx.x] = tot;
}

// launch grid: (nc, B), 1024 threads
__global__ __launch_bounds__(1024) void k_rank(const int* __restrict__ parent, const int* __restrict__ size, const int* __restrict__ chunk,
                                               int* __restrict__ labels, int* __restrict__ voxels, Shape sh) {
    __shared__ int wave_tot[16];
    const int t = (int)(blockIdx.x * 1024u + threadIdx.x), b = blockIdx.y;
    const size_t o = (size_t)b * sh.n + (t < sh.n ? t : 0);
    const bool root = t < sh.n && parent[o] == t;
    int tot;
    const int pos = chunk[(size_t)b * sh.nc + blockIdx.x] + block_rank(root, wave_tot, tot);
    if (!root) return;
    labels[o] = pos + 1;
    if (pos < sh.max_objects) voxels[(size_t)b * sh.max_objects + pos] = size[o];
}

// launch grid: k_init's; every thread stays to the end (ballots and shuffles).  labels[] is read at the roots (k_rank's) and written
// at every other voxel.
__global__ __launch_bounds__(256) void k_label(const float* __restrict__ vol, const int* __restrict__ parent, const int* __restrict__ size,
                                               int* labels, int* __restrict__ bbox, unsigned long long* __restrict__ sums,
                                               float* __restrict__ cleaned, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), b = blockIdx.y, R = sh.R;
    int L = 0;
    if (t < sh.n) {
        const size_t base = (size_t)b * sh.n, o = base + t;
        const int p = parent[o];
        if (p >= 0) L = labels[base + p];
        if (p != t) labels[o] = L;
        if (cleaned) cleaned[o] = p >= 0 && size[base + p] < sh.min_voxels ? sh.free_value : vol[o];
    }
    add_to_rows(L, L >= 1 && L <= sh.max_objects, t, R, b, sh.max_objects, bbox, sums);
}

struct Work { int *status, *parent, *size, *chunk; size_t total; };

static Work carve(int B, int R, void* base) {
    const size_t n = (size_t)R * R * R, nc = (n + 1023) / 1024;
    Carve c(base);                                                             // the status word has the first 256 bytes to itself
    return Work{c.take<int>(1), c.take<int>(B * n), c.take<int>(B * n), c.take<int>(B * nc), c.total()};          // (in this order)
}

}  // namespace gnr_objects

using namespace gnr_objects;

extern "C" size_t gnr_volume_objects_workspace_bytes(int B, int R) {
    return scenes_ok(B) && lattice_ok(R) ? carve(B, R, nullptr).total : 0;
}

extern "C" int gnr_volume_objects_fwd(const GnrObjectsParams* p, const float* vol, int B, int R, int* labels, int* count, int* voxels,
                                      int* bbox, unsigned long long* sums, float* cleaned, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    const Refuse no{"gnr_volume_objects_fwd"};
    if (!p || !vol || !labels || !count || !voxels || !bbox || !sums || !workspace) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (p->connectivity != 6 && p->connectivity != 18 && p->connectivity != 26) return no(GNR_ERR_ARG, "connectivity must be 6, 18 or 26");
    if (p->max_objects < 1) return no(GNR_ERR_SHAPE, "max_objects must be >= 1");
    if (int rc = check_solid(no, p->level, p->lower, p->z_min, R)) return rc;
    if (!isfinite(p->free_value)) return no(GNR_ERR_ARG, "free_value must be finite");
    const Work k = carve(B, R, workspace);
    if (workspace_bytes < k.total) return no(GNR_ERR_WORKSPACE, "workspace too small");
    Shape sh{};
    sh.R = R; sh.n = R * R * R; sh.nc = (sh.n + 1023) / 1024;
    sh.z_min = p->z_min; sh.order = p->connectivity == 6 ? 1 : p->connectivity == 18 ? 2 : 3;
    sh.max_objects = p->max_objects; sh.min_voxels = p->min_voxels;
    sh.level = p->level; sh.lower = p->lower; sh.free_value = p->free_value;
    int *status = k.status, *parent = k.parent, *size = k.size, *chunk = k.chunk;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g256((unsigned)((sh.n + 255) / 256), (unsigned)B), g1024((unsigned)sh.nc, (unsigned)B);
    if (int rc = launch<k_init>("k_init@gnr_volume_objects_fwd", st, g256, dim3(256), 0, vol, parent, size, status, voxels, bbox, sums, sh)) return rc;
    if (int rc = launch<k_union>("k_union@gnr_volume_objects_fwd", st, g256, dim3(256), 0, parent, status, sh)) return rc;
    if (int rc = launch<k_flatten>("k_flatten@gnr_volume_objects_fwd", st, g1024, dim3(1024), 0, parent, size, chunk, status, sh)) return rc;
    if (int rc = launch<k_scan>("k_scan@gnr_volume_objects_fwd", st, dim3((unsigned)B), dim3(1024), 0, chunk, sh.nc, count)) return rc;
    if (int rc = launch<k_rank>("k_rank@gnr_volume_objects_fwd", st, g1024, dim3(1024), 0, (const int*)parent, (const int*)size, (const int*)chunk,
                                labels, voxels, sh))
        return rc;
    return launch<k_label>("k_label@gnr_volume_objects_fwd", st, g256, dim3(256), 0, vol, (const int*)parent, (const int*)size, labels, bbox, sums,
                           cleaned, sh);
}
