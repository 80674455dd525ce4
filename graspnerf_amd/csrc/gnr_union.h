// What the labelling operators share (gnr_objects.hip: connected components of the solid voxels; gnr_parts.hip: the joins of the
// watershed's basins): a lock-free union-find in global memory over int32 parents, the scan of the per-chunk root counts, and the
// boxes and coordinate sums of the statistics rows.  Device code only.
// Union-find.  parent[x] is an index inside the scene (the caller's base pointer), never larger than x; a root has parent[x] == x;
// anything else (-1: not a node) ends a walk.  unite() finds both roots and hooks the larger under the smaller with an atomic min, so
// a tree's root is its smallest index.  When the min returns something else than the root it expected, the node had a parent already
// (and the min may have replaced that link): it goes on uniting that former parent with the smaller root.  Each find also lowers the
// parent of the node it started from to the root it found (an atomic min again: a link only ever moves to a smaller member of what ends
// as one tree, and every link a min replaces is re-united by the thread that replaced it).
// Visibility.  Inside a launch that changes parent[], other workgroups -- on other XCDs, whose L2s are not coherent with this one's --
// change it while a thread follows it.  Every access to parent[] in such a launch is therefore an agent-scope atomic (relaxed loads
// that bypass the CU's L1, min / store at the memory side), through a global-address-space pointer, never a plain load and never a
// const __restrict__ one (that could take the scalar path).  Stale values would even be harmless to the result -- every value a parent
// ever held is an ancestor in the final tree -- but a plain load may be kept in a register across a loop.  A kernel boundary makes the
// next launch's plain loads safe.
// No thread ever waits for another: the algorithm is lock-free, there is no spin and no flag.  Every loop carries a bound `lim` from
// the parameters: a find follows at most lim links (each link goes to a smaller index), a unite retries at most lim times; running
// into the bound sets UNION_STATUS_BOUND in the caller's status word and ends the loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gnr_compact.h"

namespace gnr {

typedef __attribute__((address_space(1))) int gint;
#define GNR_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
constexpr int UNION_STATUS_BOUND = 1;          // GNR_OBJECTS_STATUS_BOUND, GNR_PARTS_STATUS_BOUND

__device__ inline int ld(int* p) { return __hip_atomic_load((gint*)p, GNR_RLX_AGENT); }
__device__ inline void st(int* p, int v) { __hip_atomic_store((gint*)p, v, GNR_RLX_AGENT); }
__device__ inline int lower_to(int* p, int v) { return __hip_atomic_fetch_min((gint*)p, v, GNR_RLX_AGENT); }
__device__ inline void flag_bound(int* status) { __hip_atomic_fetch_or((gint*)status, UNION_STATUS_BOUND, GNR_RLX_AGENT); }

// the root of node x: at most `lim` links, each to a smaller index (anything else -- there is nothing else -- ends the walk)
__device__ inline int find(int* parent, int x, int lim, int* status) {
    for (int s = 0; s <= lim; ++s) {
        const int p = ld(parent + x);
        if ((unsigned)p >= (unsigned)x) return x;
        x = p;
    }
    flag_bound(status);
    return x;
}

// one tree of the trees of nodes a and b
__device__ inline void unite(int* parent, int a, int b, int lim, int* status) {
    for (int s = 0; s <= lim; ++s) {
        const int ra = find(parent, a, lim, status), rb = find(parent, b, lim, status);
        if (ra != a) lower_to(parent + a, ra);
        if (rb != b) lower_to(parent + b, rb);
        if (ra == rb) return;
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int old = lower_to(parent + hi, lo);
        if (old == hi) return;                 // hi was a root and hangs under lo now
        a = old;                               // hi had the parent `old` (which the min may have replaced): old and lo remain to be united
        b = lo;
    }
    flag_bound(status);
}

// The chunk counts of every scene scanned in place; their sum is the scene's count.  launch grid: B, 1024 threads
static __global__ __launch_bounds__(1024) void k_scan(int* __restrict__ chunk, int nc, int* __restrict__ count) {
    __shared__ int wave_tot[16];
    const int total = scan_chunks(chunk + (size_t)blockIdx.x * nc, nc, wave_tot);
    if (threadIdx.x == 0) count[blockIdx.x] = total;
}

// The box and the coordinate sums of the statistics rows: voxel t = (i R + j) R + k of scene b carries label L (has: 1 <= L <= rows),
// row (b * rows + L - 1) takes the smallest and the largest i, j, k and their sums -- one atomic per wavefront, label and column.
// Every thread of the wavefront calls it (ballots and shuffles).
__device__ inline void add_to_rows(int L, bool has, int t, int R, int b, int rows, int* __restrict__ bbox, unsigned long long* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int c[3] = {t / (R * R), (t / R) % R, t % R};
    unsigned long long todo = __ballot(has);
    for (int s = 0; s < 64 && todo; ++s) {
        const int lead = __ffsll((long long)todo) - 1;
        const int Ll = __shfl(L, lead);
        const bool mine = has && L == Ll;
        const unsigned long long m = __ballot(mine);
        int lo[3], hi[3], sum[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = mine ? c[a] : INT32_MAX; hi[a] = mine ? c[a] : -1; sum[a] = mine ? c[a] : 0; }
        if (__popcll(m) > 1) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int ol = __shfl_xor(lo[a], d), oh = __shfl_xor(hi[a], d);
                    lo[a] = ol < lo[a] ? ol : lo[a];
                    hi[a] = oh > hi[a] ? oh : hi[a];
                    sum[a] += __shfl_xor(sum[a], d);
                }
            }
        }
        if (lane == lead) {
            const size_t row = (size_t)b * rows + (Ll - 1);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(bbox + row * 6 + a, lo[a]);
                atomicMax(bbox + row * 6 + 3 + a, hi[a]);
                atomicAdd(sums + row * 3 + a, (unsigned long long)sum[a]);
            }
        }
        todo &= ~m;
    }
}

}  // namespace gnr
