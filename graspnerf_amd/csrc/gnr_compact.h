// Ordered compaction on the device, shared by gnr_post.hip (ranked selection, surface cloud) and gnr_mesh.hip (surface mesh): flags are
// counted per chunk of 1024 items, the chunk counts scanned per scene, and every chunk writes its rows at rank + chunk offset, so the
// rows come out in ascending item order without atomics.  Device code only; the workgroups are 1024 threads (16 wavefronts of 64).
#pragma once
#include <hip/hip_runtime.h>

namespace gnr {

// Exclusive rank of this thread's first set flag among the set flags of a 1024-thread workgroup, flags ordered by (thread, slot), and
// the number of set flags.  NF flags per thread, one ballot each; wave_tot: 16 ints of LDS.  Every thread of the workgroup calls it.
template <int NF>
__device__ inline int block_rank(const bool (&f)[NF], int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int before = 0, mine = 0;
#pragma unroll
    for (int s = 0; s < NF; ++s) {
        const unsigned long long bal = __ballot(f[s]);
        before += __popcll(bal & below);
        mine += __popcll(bal);
    }
    __syncthreads();                                   // the readers of the previous call are done with wave_tot
    if (lane == 0) wave_tot[wave] = mine;
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < 16; ++w) { const int c = wave_tot[w]; if (w < wave) off += c; tot += c; }
    total = tot;
    return off + before;
}

__device__ inline int block_rank(bool f, int* wave_tot, int& total) {
    const bool one[1] = {f};
    return block_rank(one, wave_tot, total);
}

// Exclusive scan in place of the nc chunk counts of one scene by a 1024-thread workgroup; returns their sum to every thread.
__device__ inline int scan_chunks(int* c, int nc, int* wave_tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < nc; c0 += 1024) {
        const int t = c0 + threadIdx.x;
        const int v = t < nc ? c[t] : 0;
        int inc = v;
        for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(inc, d); if (lane >= d) inc += u; }
        __syncthreads();
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < 16; ++w) { const int s = wave_tot[w]; if (w < wave) off += s; tot += s; }
        if (t < nc) c[t] = base + off + inc - v;
        base += tot;
    }
    return base;
}

}  // namespace gnr
