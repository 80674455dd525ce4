// Parts across two plans, on the device: how the labels of two label volumes of one workspace overlap (gnr_part_overlap_fwd), and what
// became of every part (gnr_part_track_fwd) -- which part of the second volume an old part mostly went to, what a new part is mostly
// made of, whether the two agree, and from that stayed / moved / gone / merged and same / new / fragment.  What the reference reads off
// its simulator after a grasp (check_success, remove_body, remove_and_wait; clutter_removal.py:92-150); no reference counterpart; the
// statement is include/gnr.h's and tests/track_reference.py's.
// k_overlap_fill writes every element of the table and of beyond (a kernel, not memset nodes: DESIGN 4.8).
// k_overlap: one thread per voxel, last axis fastest, grid (chunks of 256, B).  A thread reads its voxel of both volumes (two coalesced
// loads; a thread beyond the scene reads voxel 0 and credits nothing) and forms one key, i * (P + 1) + j, or -1 when a label lies
// beyond the rows.  A wavefront whose ballot of (i, j) != (0, 0) is empty -- free space in both plans -- does nothing; otherwise it
// loops over its distinct keys as k_contacts does: ballot, popcount, and the key's first lane issues one integer atomic: one atomic
// per wavefront and key, not one per voxel.  Agent-scope relaxed integer adds into the caller's table; nothing is read back inside
// the launch.
// k_track: one block of 256 threads per scene.  Rows: a wavefront takes every fourth row, its lanes lie across the columns (coalesced;
// five loads a lane in flight together), and a shuffle reduction gives the row's sum and the maximum of count * 512 + (511 - label)
// in 64 bits -- the larger count, then the smaller label, in whatever order the lanes meet.  Columns: thread b - 1 walks column b
// down the rows, so a wavefront reads 64 neighbouring words of one row at a time (coalesced); one thread takes the rows in ascending
// order, so "greater than" alone keeps the smaller label.  heir, source and the sizes go to LDS; after one barrier thread a - 1 has
// the fate of old part a and thread b - 1 the origin of new part b, pieces and absorbed are LDS integer adds, and the summary is
// ballot and popcount per wavefront, added in LDS.  Every loop is bounded by P + 1 or 64, __syncthreads stands outside divergent code,
// and no content of the table or of a count moves an address: nb and na are clamped to 0..P first.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_host.h"

#pragma clang fp contract(off)

namespace gnr_track {

using namespace gnr;

typedef __attribute__((address_space(1))) int gint;
__device__ inline void add_to(int* p, int v) { __hip_atomic_fetch_add((gint*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr int MAXP = GNR_TRACK_MAX_PARTS;
enum { STAYED = 0, MOVED = 1, GONE = 2, MERGED = 3 };
enum { SAME = 0, NEW = 1, FRAGMENT = 2 };

// launch grid: (ceil((P + 1)^2 / 256), B), block 256: thread x of scene b writes table element x, the first also beyond
__global__ __launch_bounds__(256) void k_overlap_fill(int* __restrict__ table, int* __restrict__ beyond, int cells) {
    const int b = blockIdx.y, x = (int)(blockIdx.x * 256u + threadIdx.x);
    if (x < cells) table[(size_t)b * cells + x] = 0;
    if (x == 0) beyond[b] = 0;
}

// launch grid: (ceil(R^3 / 256), B), block 256;  n = R^3
__global__ __launch_bounds__(256) void k_overlap(const int* __restrict__ before, const int* __restrict__ after, int* __restrict__ table,
                                                 int* __restrict__ beyond, int n, int P) {
    const int b = blockIdx.y;
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool live = t < n;
    const size_t self = (size_t)b * n + (live ? t : 0);           // (a thread beyond the scene reads voxel 0 and credits nothing)
    const int lane = threadIdx.x & 63;
    const int a = before[self], c = after[self];
    const bool out = a > P || c > P;
    const int i = a < 1 ? 0 : a, j = c < 1 ? 0 : c;
    const bool has = live && (out || i != 0 || j != 0);
    unsigned long long todo = __ballot(has);
    if (todo == 0ull) return;                                     // wave-uniform: free in both plans
    const int key = out ? -1 : i * (P + 1) + j;                   // (-1: beyond the rows; one key for all of them)
    int* tab = table + (size_t)b * (P + 1) * (P + 1);
    for (int s = 0; s < 64 && todo; ++s) {
        const int lead = __ffsll((long long)todo) - 1;
        const int kl = __shfl(key, lead);
        const unsigned long long m = __ballot(has && key == kl);
        if (lane == lead) add_to(kl < 0 ? beyond + b : tab + kl, __popcll(m));
        todo &= ~m;
    }
}

struct Rule {
    double share, stay;
    int P;
};

__device__ inline long long wave_max(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// launch grid: B, block 256: thread x is old part x + 1 and new part x + 1
__global__ __launch_bounds__(256) void k_track(const int* __restrict__ table, const int* __restrict__ count_before, const int* __restrict__ count_after,
                                               int* __restrict__ heir, int* __restrict__ shared, int* __restrict__ size_before,
                                               int* __restrict__ vacated, int* __restrict__ pieces, int* __restrict__ fate,
                                               int* __restrict__ source, int* __restrict__ size_after, int* __restrict__ fresh,
                                               int* __restrict__ absorbed, int* __restrict__ origin, int* __restrict__ summary, Rule ru) {
    __shared__ int s_heir[MAXP + 1], s_shared[MAXP + 1], s_size_b[MAXP + 1], s_vacated[MAXP + 1];     // per old part (index = label)
    __shared__ int s_source[MAXP + 1], s_size_a[MAXP + 1];                                              // per new part
    __shared__ int s_pieces[MAXP + 1], s_absorbed[MAXP + 1];
    __shared__ int s_sum[8];
    const int P = ru.P, W = P + 1, b = blockIdx.x, x = threadIdx.x, lane = x & 63, wave = x >> 6;
    int nb = count_before[b], na = count_after[b];
    nb = nb < 0 ? 0 : nb > P ? P : nb;
    na = na < 0 ? 0 : na > P ? P : na;
    const int* tab = table + (size_t)b * W * W;
    for (int q = x; q <= MAXP; q += 256) { s_pieces[q] = 0; s_absorbed[q] = 0; }
    if (x < 8) s_sum[x] = 0;
    // ---- the rows: heir, shared, size, vacated of every old part; a wavefront per row, lanes across the columns -----------------------
    for (int a = 1 + wave; a <= nb; a += 4) {                     // wave-uniform; at most 64 rounds
        const int* row = tab + (size_t)a * W;
        int v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {                             // columns 0..na <= 256: five loads, in flight together
            const int j = lane + 64 * q;
            v[q] = row[j <= na ? j : 0];                          // (a load never leaves columns 0..na)
        }
        unsigned sum = 0u;
        long long best = INT64_MIN;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int j = lane + 64 * q;
            if (j <= na) sum += (unsigned)v[q];
            if (j >= 1 && j <= na) {
                const long long key = (long long)v[q] * 512 + (511 - j);
                best = key > best ? key : best;
            }
        }
        sum = wave_sum(sum);
        best = wave_max(best);
        if (lane == 0) {
            const int size = (int)sum;
            const int t = na >= 1 ? (int)(best >> 9) : 0, lab = na >= 1 ? 511 - (int)(best & 511) : 0;
            const bool kept = t >= 1 && (double)t >= ru.share * (double)size;
            s_heir[a] = kept ? lab : 0;
            s_shared[a] = t;
            s_size_b[a] = size;
            s_vacated[a] = v[0];
        }
    }
    // ---- the columns: source, size, fresh of every new part; thread per column, a wavefront reads 64 neighbouring words of a row ------
    const int me = x + 1;                                         // the label of this thread's part, old and new
    int src = 0, t_src = 0, n_fresh = 0;
    unsigned col_sum = 0u;
    if (me <= na) {
        n_fresh = tab[me];
        col_sum = (unsigned)n_fresh;
        int top = 0;
#pragma unroll 8
        for (int i = 1; i <= nb; ++i) {                           // at most P rounds, ascending: "greater" keeps the smaller label
            const int c = tab[(size_t)i * W + me];
            col_sum += (unsigned)c;
            if (i == 1 || c > top) { top = c; src = i; }
        }
        t_src = top;
        const bool kept = nb >= 1 && t_src >= 1 && (double)t_src >= ru.share * (double)(int)col_sum;
        src = kept ? src : 0;
        s_source[me] = src;
        s_size_a[me] = (int)col_sum;
    }
    __syncthreads();
    // ---- fates and origins -------------------------------------------------------------------------------------------------------------
    int f = -1, o = -1, h = 0, sh = 0, sz = 0, vac = 0;
    if (me <= nb) {
        h = s_heir[me]; sh = s_shared[me]; sz = s_size_b[me]; vac = s_vacated[me];
        if (h == 0) {
            f = GONE;
        } else {
            atomicAdd(&s_absorbed[h], 1);
            if (s_source[h] != me) {
                f = MERGED;
            } else {
                const long long uni = (long long)sz + (long long)s_size_a[h] - (long long)sh;
                f = (double)sh >= ru.stay * (double)uni ? STAYED : MOVED;
            }
        }
    }
    if (me <= na) {
        if (src == 0) {
            o = NEW;
        } else {
            atomicAdd(&s_pieces[src], 1);
            o = s_heir[src] == me ? SAME : FRAGMENT;
        }
    }
    auto votes = [](bool mine) { return (int)__popcll(__ballot(mine)); };
    const int tally[6] = {votes(f == STAYED), votes(f == MOVED), votes(f == GONE), votes(f == MERGED), votes(o == NEW), votes(o == FRAGMENT)};
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd(&s_sum[2 + k], tally[k]);
    }
    __syncthreads();
    if (x < P) {
        const size_t at = (size_t)b * P + x;
        heir[at] = h; shared[at] = sh; size_before[at] = sz; vacated[at] = vac; pieces[at] = me <= nb ? s_pieces[me] : 0; fate[at] = f;
        source[at] = src; size_after[at] = (int)col_sum; fresh[at] = n_fresh; absorbed[at] = me <= na ? s_absorbed[me] : 0; origin[at] = o;
    }
    if (x < 8) summary[(size_t)b * 8 + x] = x == 0 ? nb : x == 1 ? na : s_sum[x];
}

}  // namespace gnr_track

using namespace gnr_track;

extern "C" int gnr_part_overlap_fwd(const GnrOverlapParams* p, const int* before, const int* after, int B, int R, int* table, int* beyond,
                                    void* stream) {
    const Refuse no{"gnr_part_overlap_fwd"};
    if (!p) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (p->max_parts < 1 || p->max_parts > GNR_TRACK_MAX_PARTS) return no(GNR_ERR_SHAPE, "max_parts must be in 1..GNR_TRACK_MAX_PARTS (256)");
    if (!before || !after || !table || !beyond) return no(GNR_ERR_ARG, "null pointer");
    const int P = p->max_parts, cells = (P + 1) * (P + 1), n = R * R * R;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch<k_overlap_fill>("k_overlap_fill@gnr_part_overlap_fwd", st, dim3((unsigned)((cells + 255) / 256), (unsigned)B), dim3(256), 0,
                                        table, beyond, cells))
        return rc;
    return launch<k_overlap>("k_overlap@gnr_part_overlap_fwd", st, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, before, after, table,
                             beyond, n, P);
}

extern "C" int gnr_part_track_fwd(const GnrTrackParams* p, const int* table, const int* count_before, const int* count_after, int B, int* heir,
                                  int* shared, int* size_before, int* vacated, int* pieces, int* fate, int* source, int* size_after, int* fresh,
                                  int* absorbed, int* origin, int* summary, void* stream) {
    const Refuse no{"gnr_part_track_fwd"};
    if (!p) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (p->max_parts < 1 || p->max_parts > GNR_TRACK_MAX_PARTS) return no(GNR_ERR_SHAPE, "max_parts must be in 1..GNR_TRACK_MAX_PARTS (256)");
    if (!(isfinite(p->share) && p->share >= 0.0 && p->share <= 1.0)) return no(GNR_ERR_ARG, "share must be finite and in 0..1");
    if (!(isfinite(p->stay) && p->stay >= 0.0 && p->stay <= 1.0)) return no(GNR_ERR_ARG, "stay must be finite and in 0..1");
    if (!table || !count_before || !count_after || !heir || !shared || !size_before || !vacated || !pieces || !fate || !source || !size_after ||
        !fresh || !absorbed || !origin || !summary)
        return no(GNR_ERR_ARG, "null pointer");
    Rule ru{};
    ru.share = p->share; ru.stay = p->stay; ru.P = p->max_parts;
    return launch<k_track>("k_track@gnr_part_track_fwd", (hipStream_t)stream, dim3((unsigned)B), dim3(256), 0, table, count_before, count_after,
                           heir, shared, size_before, vacated, pieces, fate, source, size_after, fresh, absorbed, origin, summary, ru);
}
