// Retreat of the ranked grasps, on the device: the fourth step of ClutterRemovalSim.execute_grasp (gd/simulation.py:369-422) answered
// from the labelled volume.  Per grasp the voxels of the part the hand holds (gnr_volume_parts_fwd's or gnr_volume_objects_fwd's label,
// gnr_grasp_objects_fwd's `object`) move K steps along the retreat -- back along the hand's own z, or straight up for a side grasp --
// by integer offsets, and every step counts the moving voxels that land inside another part.  No reference counterpart; the statement
// is include/gnr.h's and tests/retreat_reference.py's.
// Mapping: one block of four wavefronts per grasp, grid (min(rows, 65536), B), x strided.  The pose, the direction and the part's box
// are the same in every lane.  Wavefront 0 computes the K offsets and keeps in LDS only the steps whose offset differs from the step
// before (step 0 is no offset): a repeated offset repeats its count, so neither the largest count nor the first step above the
// tolerance can be a repeat -- with half a voxel between steps and an axis-aligned retreat that halves the work.  The threads then
// walk the box with the last axis fastest (a box row is one contiguous run of labels); a wavefront none of whose lanes holds a moving
// voxel goes on to its next 64; the others test their voxels against four steps at a time: four independent loads from the label
// volume (L2 resident: 40^3 ints = 256 KB), then per step ballot -> popcount -> one LDS add by lane 0 when any lane hit.  The largest
// count and the first step above the tolerance are LDS max / min over the kept steps; a second walk, at that step alone and only for
// a blocked grasp, takes the LDS minimum of the hitting voxels' indices, and thread 0 reads the blocker there and stores the row.
// LDS atomics on integers only (any order, the same bits), no global atomics, no workspace, plain vector loads and stores.
// Every loop is bounded by the parameters and R: K <= GNR_RETREAT_MAX_STEPS by the host's refusal, the box is clamped to the lattice
// before it sizes anything, a held label indexes bbox only inside 1..max_parts, an offset is clamped to [-R, R] as a double before it
// becomes an int (|o| >= R already moves every voxel out), and a target is read only after its three components passed 0 <= t < R --
// so no content of bbox, held, quat or count ends a loop later or moves an access out of the scene's lattice.
// Float64 throughout the pose and the offsets, single correctly rounded operations in the order of the statement (contraction is off
// for the whole file); everything else is integers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_host.h"

#pragma clang fp contract(off)

namespace gnr_retreat {

using namespace gnr;

struct Shape {
    int R, max_n, rows, count_stride;          // rows = min(top_k or max_n, max_n): the most rows a scene writes
    int K, tolerance, max_parts;
    double T, sl, side_cos, scale;             // T = retreat / scale voxels in K steps of sl
};

// T, K (as a double: the host compares it with the cap before any cast) and sl of the parameters
static inline void steps_of(double retreat, double step, double scale, double& T, double& K, double& sl) {
    T = retreat / scale;
    K = fmax(1.0, ceil(T / step));
    sl = T / K;
}

// the offset of step k along one axis: rint(u * (k * sl)), as an integer of the statement -- clamped to [-R, R], where every voxel is out
__device__ inline int offset_of(double u, int k, double sl, int R) {
    const double d = rint(u * ((double)k * sl));
    return (int)fmin(fmax(d, -(double)R), (double)R);
}

// launch grid: (min(rows, 65536), B), x strided (B <= 65535);  block 256: one grasp
__global__ __launch_bounds__(256) void k_grasp_retreat(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                       const int* __restrict__ held, const float* __restrict__ quat,
                                                       const int* __restrict__ count, int* __restrict__ blocked_step,
                                                       int* __restrict__ blocker, int* __restrict__ overlap, int* __restrict__ moved,
                                                       int* __restrict__ side, float* __restrict__ travel, Shape sh) {
    __shared__ int4 s_step[GNR_RETREAT_MAX_STEPS];                // the kept steps: (o_x, o_y, o_z, k), k ascending
    __shared__ int s_hits[GNR_RETREAT_MAX_STEPS];                 // their counts
    __shared__ int s_kept, s_moved, s_most, s_first, s_voxel;
    const int R = sh.R, b = blockIdx.y;
    const int* lab = labels + (size_t)b * R * R * R;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int n = count[(size_t)b * sh.count_stride];
    const int rows = n < sh.rows ? n : sh.rows;                   // (a negative count: no row)
    for (unsigned r = blockIdx.x; r < (unsigned)sh.rows; r += gridDim.x) {
        if (rows <= 0 || r >= (unsigned)rows) break;              // block-uniform: rows beyond the count are left untouched
        __syncthreads();                                          // (the row before is done with the LDS)
        const size_t o = (size_t)b * sh.max_n + r;
        // ---- the direction and the part's box of this grasp (the same in every lane) ------------------------------------------------
        const float* q = quat + o * 4;
        double qx = (double)q[0], qy = (double)q[1], qz = (double)q[2], qw = (double)q[3];
        const double qn = fmax(__dsqrt_rn(((qx * qx + qy * qy) + qz * qz) + qw * qw), 1e-12);
        qx = qx / qn; qy = qy / qn; qz = qz / qn; qw = qw / qn;
        // column 2 of gnr_hand_clearance_fwd's matrix, negated: the hand moves back along its own z
        double u[3] = {-(2.0 * (qx * qz + qy * qw)), -(2.0 * (qy * qz - qx * qw)), -(1.0 - 2.0 * (qx * qx + qy * qy))};
        const double free_travel = sh.T * sh.scale;
        if (u[0] != u[0] || u[1] != u[1] || u[2] != u[2]) {       // not a number: the row moves nothing
            if (tid == 0) {
                blocked_step[o] = 0; blocker[o] = 0; overlap[o] = 0; moved[o] = 0; side[o] = 0;
                travel[o] = (float)free_travel;
            }
            continue;
        }
        const int sd = u[2] < sh.side_cos ? 1 : 0;
        if (sd) { u[0] = 0.0; u[1] = 0.0; u[2] = 1.0; }
        const int L = held[o];
        int lo[3] = {0, 0, 0}, nn[3] = {0, 0, 0};
        if (L >= 1 && L <= sh.max_parts) {
            const int* bx = bbox + ((size_t)b * sh.max_parts + (size_t)(L - 1)) * 6;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int l = bx[a] > 0 ? bx[a] : 0, h = bx[3 + a] < R - 1 ? bx[3 + a] : R - 1;
                lo[a] = l;
                nn[a] = h >= l ? h - l + 1 : 0;
            }
        }
        const int nyz = nn[1] * nn[2], total = nn[0] * nyz;       // at most R^3 <= 2^24
        // ---- the kept steps (wavefront 0) --------------------------------------------------------------------------------------------
        if (tid < 64u) {
            int kept = 0;
            for (int base = 1; base <= sh.K; base += 64) {
                const int k = base + (int)lane;
                int now[3] = {0, 0, 0};
                bool keep = false;
                if (k <= sh.K) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        now[a] = offset_of(u[a], k, sh.sl, R);
                        keep = keep || now[a] != offset_of(u[a], k - 1, sh.sl, R);
                    }
                }
                const unsigned long long m = __ballot(keep);
                if (keep) {
                    const int at = kept + __popcll(m & ((1ull << lane) - 1ull));
                    s_step[at] = make_int4(now[0], now[1], now[2], k);
                    s_hits[at] = 0;
                }
                kept += __popcll(m);
            }
            if (lane == 0) { s_kept = kept; s_moved = 0; s_most = 0; s_first = INT32_MAX; s_voxel = INT32_MAX; }
        }
        __syncthreads();
        const int kept = s_kept;
        // this thread's voxel of the 256 from `base` on: whether it moves, and where it is (0, 0, 0 when it does not)
        auto voxel_at = [&](int base, int& vi, int& vj, int& vk) {
            const int s = base + (int)tid;
            vi = 0; vj = 0; vk = 0;
            if (s >= total) return false;
            const int ix = s / nyz, rem = s - ix * nyz, iy = rem / nn[2];
            const int i = lo[0] + ix, j = lo[1] + iy, k = lo[2] + (rem - iy * nn[2]);
            if (lab[((size_t)i * R + j) * R + k] != L) return false;
            vi = i; vj = j; vk = k;
            return true;
        };
        // whether the moving voxel lands in another part at the step: the load is always inside the lattice (its own voxel otherwise)
        auto hits_at = [&](bool act, int vi, int vj, int vk, const int4& st) {
            const int ti = vi + st.x, tj = vj + st.y, tk = vk + st.z;
            const bool in = (unsigned)ti < (unsigned)R && (unsigned)tj < (unsigned)R && (unsigned)tk < (unsigned)R;
            const int t = lab[in ? ((size_t)ti * R + tj) * R + tk : ((size_t)vi * R + vj) * R + vk];
            return act && in && t != 0 && t != L;
        };
        // ---- every moving voxel against every kept step ---------------------------------------------------------------------------------
        for (int base = 0; base < total; base += 256) {
            int vi, vj, vk;
            const bool act = voxel_at(base, vi, vj, vk);
            const unsigned long long am = __ballot(act);
            if (am == 0ull) continue;                             // wave-uniform
            if (lane == 0) atomicAdd(&s_moved, __popcll(am));
            for (int s0 = 0; s0 < kept; s0 += 4) {
                bool h[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool live = s0 + j < kept;
                    h[j] = hits_at(act && live, vi, vj, vk, s_step[live ? s0 + j : s0]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned long long m = __ballot(h[j]);
                    if (lane == 0 && m != 0ull) atomicAdd(&s_hits[s0 + j], __popcll(m));
                }
            }
        }
        __syncthreads();
        // ---- the largest count, the first step above the tolerance (the kept steps ascend in k) -------------------------------------------
        for (int s = (int)tid; s < kept; s += 256) {
            const int c = s_hits[s];
            if (c > 0) atomicMax(&s_most, c);
            if (c > sh.tolerance) atomicMin(&s_first, s);
        }
        __syncthreads();
        const int first = s_first;
        if (first != INT32_MAX) {                                 // block-uniform: blocked -- the hitting voxel of the smallest index
            const int4 st = s_step[first];
            for (int base = 0; base < total; base += 256) {
                int vi, vj, vk;
                const bool act = voxel_at(base, vi, vj, vk);
                if (__ballot(act) == 0ull) continue;
                if (hits_at(act, vi, vj, vk, st)) atomicMin(&s_voxel, (vi * R + vj) * R + vk);
            }
            __syncthreads();
        }
        if (tid == 0) {
            int bs = 0, who = 0;
            if (first != INT32_MAX) {
                const int4 st = s_step[first];
                bs = st.w;
                const int v = s_voxel;                            // (a step above the tolerance >= 0 has a hitting voxel)
                if (v != INT32_MAX) who = lab[v + (st.x * R + st.y) * R + st.z];          // (hits_at found the target inside)
            }
            blocked_step[o] = bs; blocker[o] = who; overlap[o] = s_most; moved[o] = s_moved; side[o] = sd;
            travel[o] = (float)(bs > 0 ? ((double)(bs - 1) * sh.sl) * sh.scale : free_travel);
        }
    }
}

}  // namespace gnr_retreat

using namespace gnr_retreat;

extern "C" int gnr_grasp_retreat_fwd(const GnrRetreatParams* p, const int* labels, const int* bbox, const int* held, const float* quat,
                                     const int* count, int count_stride, int B, int R, int max_n, int top_k, int* blocked_step, int* blocker,
                                     int* overlap, int* moved, int* side, float* travel, void* stream) {
    const Refuse no{"gnr_grasp_retreat_fwd"};
    if (!p || !labels || !bbox || !held || !quat || !count || !blocked_step || !blocker || !overlap || !moved || !side || !travel)
        return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (max_n < 1) return no(GNR_ERR_SHAPE, "max_n must be >= 1");
    if (count_stride < 1) return no(GNR_ERR_ARG, "count_stride must be >= 1");
    if (top_k < 0) return no(GNR_ERR_ARG, "top_k must be >= 0 (0: every row)");
    const double lengths[3] = {p->retreat, p->step, p->scale};
    for (double x : lengths)
        if (!isfinite(x) || !(x > 0.0)) return no(GNR_ERR_ARG, "retreat, step and scale must be finite and > 0");
    if (!isfinite(p->side_cos)) return no(GNR_ERR_ARG, "side_cos must be finite");
    if (p->tolerance < 0) return no(GNR_ERR_ARG, "tolerance must be >= 0");
    if (p->max_parts < 1) return no(GNR_ERR_SHAPE, "max_parts must be >= 1");
    double T, K, sl;
    steps_of(p->retreat, p->step, p->scale, T, K, sl);
    if (!(K <= (double)GNR_RETREAT_MAX_STEPS))
        return no(GNR_ERR_ARG, "step too small or retreat too long, a grasp would take more than GNR_RETREAT_MAX_STEPS (1024) steps");
    Shape sh{};
    sh.R = R; sh.max_n = max_n; sh.count_stride = count_stride;
    sh.rows = top_k > 0 && top_k < max_n ? top_k : max_n;
    sh.K = (int)K; sh.tolerance = p->tolerance; sh.max_parts = p->max_parts;
    sh.T = T; sh.sl = sl; sh.side_cos = p->side_cos; sh.scale = p->scale;
    const dim3 grid(sh.rows < 65536 ? (unsigned)sh.rows : 65536u, (unsigned)B, 1u);
    return launch<k_grasp_retreat>("k_grasp_retreat@gnr_grasp_retreat_fwd", (hipStream_t)stream, grid, dim3(256), 0, labels, bbox, held, quat,
                                   count, blocked_step, blocker, overlap, moved, side, travel, sh);
}
