// Parts of the volume, on the device: the solid voxels (height > 0) of B integer height fields split at their necks -- a watershed by
// steepest ascent, neighbouring basins joined where the pass between them is no neck, ndimage.label's numbering of the parts (in raster
// order of their first voxel), per part its size, box, coordinate sums and peak.  The intended height is gnr_volume_distance_fwd's
// d2_free: two convex things that touch are two hills joined over a low pass.  No reference counterpart (like gnr_objects.hip); the
// statement is include/gnr.h's and tests/parts_reference.py's.  Everything is integer beyond the one double multiply and compare of
// the neck test, so any order of execution gives the same bits.  Eight launches; every index is a voxel's inside its own scene:
//   k_up     up = the voxel of the largest (height, -index) among a solid voxel and its solid neighbours (6 / 18 / 26), -1 where not
//            solid; parent = own index; the per-voxel accumulators, the status word, the basin counts and the statistics rows reset.
//   k_walk   basin = the summit (up[x] == x) the links from the voxel end at.  up[] is read-only in this launch: plain loads.
//   k_join   each solid voxel looks at its solid neighbours of smaller index (3 / 9 / 13); where the two basins differ and the join
//            test holds -- on the two basins' own peaks, never on those of an already merged set, so the joins do not depend on any
//            order -- their summits are united in parent[] (gnr_union.h: the larger root hooks under the smaller, lock-free).
//   k_flat   part = the root of the voxel's summit; at that root the part's size and smallest voxel (one atomic per wavefront and
//            root; the lanes are consecutive voxels, so the first lane of a root holds the wavefront's smallest) and, from the summits
//            alone, the peak as one 64-bit max of (height << 32) | ~index.  The voxel of the largest (height, -index) of a part is a
//            summit: were up[x] != x, up[x] would lie in x's basin, so in its part, and be larger.  The summits counted per scene.
//   k_root   root = the smallest voxel of the voxel's part -- gnr_objects.hip's flattened parent --; the roots of each chunk of 1024
//            voxels counted (gnr_compact.h).
//   k_scan   the chunk counts scanned per scene; their sum is the scene's count (gnr_union.h).
//   k_rank   every root takes label 1 + its rank among the roots of its scene and, when that is a statistics row, stores the part's
//            size, peak and peak voxel.
//   k_label  labels of the other voxels (the root's), the boxes and sums (one atomic per wavefront, label and column; gnr_union.h).
// Visibility (gnr_union.h states the rules).  k_join changes parent[] while other workgroups follow it: every access to parent[] there
// is an agent-scope relaxed atomic through a global pointer; k_flat reads it through the same find().  Everything else that one
// launch writes and another reads crosses a kernel boundary and is read plainly; the accumulators of k_flat are atomic
// read-modify-writes that nothing reads before the next launch.
// No thread ever waits for another.  Every loop carries a bound from the parameters: a walk and a find follow at most R^3 links, a
// unite retries at most R^3 times; running into the bound sets GNR_PARTS_STATUS_BOUND in the status word (the first int of the
// workspace) and ends the loop.  Everything a call reads from its workspace it has written in the same call (k_up), so a captured call
// replays.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_host.h"
#include "gnr_union.h"

namespace gnr_parts {

using namespace gnr;
static_assert(UNION_STATUS_BOUND == GNR_PARTS_STATUS_BOUND, "find() and unite() flag the status word's bound bit");

struct Shape {
    int R, n, nc;                              // n = R^3 voxels of a scene, nc chunks of 1024 of them
    int order, max_parts, min_peak;            // order: how many axes a neighbour may differ in (1, 2, 3 for 6, 18, 26)
    double neck2;                              // neck * neck
};

// a 64-bit key that orders voxels by (height, -index); height > 0
__device__ inline unsigned long long key_of(int height, int index) {
    return ((unsigned long long)(unsigned)height << 32) | (unsigned)~index;
}

// launch grid: (ceil(n / 256), B), 256 threads.  The rows of the statistics are spread over all threads of the grid.
__global__ __launch_bounds__(256) void k_up(const int* __restrict__ height, int* __restrict__ up, int* __restrict__ parent,
                                            int* __restrict__ first, int* __restrict__ size, unsigned long long* __restrict__ top,
                                            int* __restrict__ status, int* __restrict__ basins, int* __restrict__ voxels,
                                            int* __restrict__ bbox, unsigned long long* __restrict__ sums, int* __restrict__ peak,
                                            int* __restrict__ peak_voxel, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), b = blockIdx.y, R = sh.R;
    if (t < sh.n) {
        const size_t base = (size_t)b * sh.n, o = base + t;
        const int h = height[o];
        int best = -1;
        if (h > 0) {
            unsigned long long bk = key_of(h, t);
            best = t;
            const int k = t % R, j = (t / R) % R, i = t / (R * R);
            for (int c = 0; c < 27; ++c) {     // the 3x3x3 block around the voxel
                const int di = c / 9 - 1, dj = (c / 3) % 3 - 1, dk = c % 3 - 1;
                const int axes = (di != 0) + (dj != 0) + (dk != 0);
                if (axes == 0 || axes > sh.order) continue;
                const int ii = i + di, jj = j + dj, kk = k + dk;
                if (ii < 0 || ii >= R || jj < 0 || jj >= R || kk < 0 || kk >= R) continue;
                const int nb = (ii * R + jj) * R + kk, hn = height[base + nb];
                if (hn <= 0) continue;
                const unsigned long long nk = key_of(hn, nb);
                if (nk > bk) { bk = nk; best = nb; }
            }
        }
        up[o] = best;
        parent[o] = t;
        first[o] = INT32_MAX;
        size[o] = 0;
        top[o] = 0ull;
    }
    const size_t threads = (size_t)gridDim.x * gridDim.y * 256u, me = ((size_t)b * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
    if (me == 0) *status = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) basins[b] = 0;
    const size_t rows = (size_t)gridDim.y * (size_t)sh.max_parts;
    for (size_t r = me; r < rows; r += threads) {
        voxels[r] = 0;
        peak[r] = 0;
        peak_voxel[r] = -1;
#pragma unroll
        for (int a = 0; a < 3; ++a) { bbox[r * 6 + a] = R; bbox[r * 6 + 3 + a] = -1; sums[r * 3 + a] = 0ull; }
    }
}

// launch grid: k_up's
__global__ __launch_bounds__(256) void k_walk(const int* __restrict__ up_all, int* __restrict__ basin, int* status, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t >= sh.n) return;
    const size_t base = (size_t)blockIdx.y * sh.n;
    const int* up = up_all + base;
    int x = up[t];
    if (x >= 0) {
        bool ended = false;
        x = t;
        for (int s = 0; s <= sh.n; ++s) {      // (every link strictly increases (height, -index): at most n - 1 of them)
            const int p = up[x];
            if (p == x || (unsigned)p >= (unsigned)sh.n) { ended = true; break; }
            x = p;
        }
        if (!ended) flag_bound(status);
    }
    basin[base + t] = x;
}

// launch grid: k_up's
__global__ __launch_bounds__(256) void k_join(const int* __restrict__ height_all, const int* __restrict__ basin_all, int* parent_all,
                                              int* status, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), R = sh.R;
    if (t >= sh.n) return;
    const size_t base = (size_t)blockIdx.y * sh.n;
    const int* height = height_all + base;
    const int* basin = basin_all + base;
    int* parent = parent_all + base;
    const int a = basin[t];
    if (a < 0) return;
    const int h = height[t], pa = height[a];
    const int k = t % R, j = (t / R) % R, i = t / (R * R);
    for (int c = 0; c < 13; ++c) {             // the 13 offsets (di, dj, dk) of the 3x3x3 block in front of its centre, in raster order
        const int di = c / 9 - 1, dj = (c / 3) % 3 - 1, dk = c % 3 - 1;
        if ((di != 0) + (dj != 0) + (dk != 0) > sh.order) continue;
        const int ii = i + di, jj = j + dj, kk = k + dk;
        if (ii < 0 || jj < 0 || jj >= R || kk < 0 || kk >= R) continue;       // (ii <= i < R)
        const int nb = (ii * R + jj) * R + kk, bb = basin[nb];
        if (bb < 0 || bb == a) continue;
        const int hn = height[nb], pb = height[bb];
        const int pass = h < hn ? h : hn, low = pa < pb ? pa : pb;
        if (low <= sh.min_peak || (double)pass >= sh.neck2 * (double)low) unite(parent, a, bb, sh.n, status);
    }
}

// launch grid: k_up's; every thread stays to the end (ballots and shuffles).  part[] is the array that held up[].
__global__ __launch_bounds__(256) void k_flat(const int* __restrict__ height, const int* __restrict__ basin, int* parent_all,
                                              int* __restrict__ part, int* first_all, int* size_all, unsigned long long* top_all,
                                              int* basins, int* status, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), b = blockIdx.y, lane = threadIdx.x & 63;
    const size_t base = (size_t)b * sh.n;
    int r = -1;
    bool summit = false;
    if (t < sh.n) {
        const int a = basin[base + t];
        if (a >= 0) {
            r = find(parent_all + base, a, sh.n, status);
            summit = a == t;
            if (summit) atomicMax(top_all + base + r, key_of(height[base + t], t));
        }
        part[base + t] = r;
    }
    unsigned long long todo = __ballot(r >= 0);
    for (int s = 0; s < 64 && todo; ++s) {
        const int lead = __ffsll((long long)todo) - 1;
        const int rl = __shfl(r, lead);
        const unsigned long long m = __ballot(r == rl);
        if (lane == lead) {
            atomicAdd(size_all + base + rl, __popcll(m));
            atomicMin(first_all + base + rl, t);
        }
        todo &= ~m;
    }
    const unsigned long long tops = __ballot(summit);
    if (lane == 0 && tops) atomicAdd(basins + b, __popcll(tops));
}

// launch grid: (nc, B), 1024 threads; every thread stays to the end (the workgroup's rank).  root[] is the array that held basin[].
__global__ __launch_bounds__(1024) void k_root(const int* __restrict__ part, const int* __restrict__ first, int* __restrict__ root,
                                               int* __restrict__ chunk, Shape sh) {
    __shared__ int wave_tot[16];
    const int t = (int)(blockIdx.x * 1024u + threadIdx.x), b = blockIdx.y;
    const size_t base = (size_t)b * sh.n;
    int r = -1;
    if (t < sh.n) {
        const int p = part[base + t];
        if (p >= 0) r = first[base + p];
        root[base + t] = r;
    }
    int tot;
    block_rank(r >= 0 && r == t, wave_tot, tot);
    if (threadIdx.x == 0) chunk[(size_t)b * sh.nc + blockIdx.x] = tot;
}

// launch grid: (nc, B), 1024 threads
__global__ __launch_bounds__(1024) void k_rank(const int* __restrict__ root, const int* __restrict__ part, const int* __restrict__ size,
                                               const unsigned long long* __restrict__ top, const int* __restrict__ chunk,
                                               int* __restrict__ labels, int* __restrict__ voxels, int* __restrict__ peak,
                                               int* __restrict__ peak_voxel, Shape sh) {
    __shared__ int wave_tot[16];
    const int t = (int)(blockIdx.x * 1024u + threadIdx.x), b = blockIdx.y;
    const size_t base = (size_t)b * sh.n, o = base + (t < sh.n ? t : 0);
    const bool is_root = t < sh.n && root[o] == t;
    int tot;
    const int pos = chunk[(size_t)b * sh.nc + blockIdx.x] + block_rank(is_root, wave_tot, tot);
    if (!is_root) return;
    labels[o] = pos + 1;
    if (pos < sh.max_parts) {
        const size_t row = (size_t)b * sh.max_parts + pos, at = base + part[o];
        const unsigned long long key = top[at];
        voxels[row] = size[at];
        peak[row] = (int)(key >> 32);
        peak_voxel[row] = (int)~(unsigned)key;
    }
}

// launch grid: k_up's; every thread stays to the end (ballots and shuffles).  labels[] is read at the roots (k_rank's) and written
// at every other voxel.
__global__ __launch_bounds__(256) void k_label(const int* __restrict__ root, int* labels, int* __restrict__ bbox,
                                               unsigned long long* __restrict__ sums, Shape sh) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), b = blockIdx.y;
    int L = 0;
    if (t < sh.n) {
        const size_t base = (size_t)b * sh.n, o = base + t;
        const int p = root[o];
        if (p >= 0) L = labels[base + p];
        if (p != t) labels[o] = L;
    }
    add_to_rows(L, L >= 1 && L <= sh.max_parts, t, sh.R, b, sh.max_parts, bbox, sums);
}

// up / part and basin / root share an array each: up is last read by k_walk and part first written by k_flat, basin is last read by
// k_flat and root first written by k_root
struct Work { int *status, *up, *basin, *parent, *first, *size; unsigned long long* top; int* chunk; size_t total; };

static Work carve(int B, int R, void* base) {
    const size_t n = (size_t)R * R * R, nc = (n + 1023) / 1024;
    Carve c(base);                                                             // the status word has the first 256 bytes to itself
    return Work{c.take<int>(1), c.take<int>(B * n), c.take<int>(B * n), c.take<int>(B * n), c.take<int>(B * n), c.take<int>(B * n),
                c.take<unsigned long long>(B * n), c.take<int>(B * nc), c.total()};                              // (in this order)
}

}  // namespace gnr_parts

using namespace gnr_parts;

extern "C" size_t gnr_volume_parts_workspace_bytes(int B, int R) {
    return scenes_ok(B) && lattice_ok(R) ? carve(B, R, nullptr).total : 0;
}

extern "C" int gnr_volume_parts_fwd(const GnrPartsParams* p, const int* height, int B, int R, int* labels, int* count, int* basins,
                                    int* voxels, int* bbox, unsigned long long* sums, int* peak, int* peak_voxel, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const Refuse no{"gnr_volume_parts_fwd"};
    if (!p || !height || !labels || !count || !basins || !voxels || !bbox || !sums || !peak || !peak_voxel || !workspace)
        return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (p->connectivity != 6 && p->connectivity != 18 && p->connectivity != 26) return no(GNR_ERR_ARG, "connectivity must be 6, 18 or 26");
    if (p->max_parts < 1) return no(GNR_ERR_SHAPE, "max_parts must be >= 1");
    if (p->min_peak < 0) return no(GNR_ERR_ARG, "min_peak must be >= 0");
    if (!(isfinite(p->neck) && p->neck >= 0.0 && p->neck <= 1.0)) return no(GNR_ERR_ARG, "neck must be finite and in 0..1");
    const Work k = carve(B, R, workspace);
    if (workspace_bytes < k.total) return no(GNR_ERR_WORKSPACE, "workspace too small");
    Shape sh{};
    sh.R = R; sh.n = R * R * R; sh.nc = (sh.n + 1023) / 1024;
    sh.order = p->connectivity == 6 ? 1 : p->connectivity == 18 ? 2 : 3;
    sh.max_parts = p->max_parts; sh.min_peak = p->min_peak; sh.neck2 = p->neck * p->neck;
    int *part = k.up, *root = k.basin;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g256((unsigned)((sh.n + 255) / 256), (unsigned)B), g1024((unsigned)sh.nc, (unsigned)B);
    if (int rc = launch<k_up>("k_up@gnr_volume_parts_fwd", st, g256, dim3(256), 0, height, k.up, k.parent, k.first, k.size, k.top, k.status, basins,
                              voxels, bbox, sums, peak, peak_voxel, sh))
        return rc;
    if (int rc = launch<k_walk>("k_walk@gnr_volume_parts_fwd", st, g256, dim3(256), 0, (const int*)k.up, k.basin, k.status, sh)) return rc;
    if (int rc = launch<k_join>("k_join@gnr_volume_parts_fwd", st, g256, dim3(256), 0, height, (const int*)k.basin, k.parent, k.status, sh)) return rc;
    if (int rc = launch<k_flat>("k_flat@gnr_volume_parts_fwd", st, g256, dim3(256), 0, height, (const int*)k.basin, k.parent, part, k.first, k.size,
                                k.top, basins, k.status, sh))
        return rc;
    if (int rc = launch<k_root>("k_root@gnr_volume_parts_fwd", st, g1024, dim3(1024), 0, (const int*)part, (const int*)k.first, root, k.chunk, sh))
        return rc;
    if (int rc = launch<k_scan>("k_scan@gnr_volume_parts_fwd", st, dim3((unsigned)B), dim3(1024), 0, k.chunk, sh.nc, count)) return rc;
    if (int rc = launch<k_rank>("k_rank@gnr_volume_parts_fwd", st, g1024, dim3(1024), 0, (const int*)root, (const int*)part, (const int*)k.size,
                                (const unsigned long long*)k.top, (const int*)k.chunk, labels, voxels, peak, peak_voxel, sh))
        return rc;
    return launch<k_label>("k_label@gnr_volume_parts_fwd", st, g256, dim3(256), 0, (const int*)root, labels, bbox, sums, sh);
}
