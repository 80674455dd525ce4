// Support of the parts, on the device: where two labels of a label volume touch and which lies on the other (gnr_part_contacts_fwd),
// and the graph that follows -- on whom a part rests, what it carries, what loses every footing when it is taken, the layers of an
// order of removal, what is grounded (gnr_part_support_fwd).  What the reference leaves to physics (remove_and_wait); no reference
// counterpart; the statement is include/gnr.h's and tests/support_reference.py's.
// k_contacts_fill writes every element of the tables (a kernel, not memset nodes: DESIGN 4.8).
// k_contacts: one thread per voxel, last axis fastest, grid (chunks of 256, B).  A thread reads its own label and those of the forward
// half of its neighbourhood (3, 9 or 13 offsets: every unordered pair of neighbours once; a neighbour outside the lattice is replaced
// by the voxel's own address, so a load never leaves the scene) and credits both ordered entries of a contact.  Per direction a
// wavefront whose ballot of contacts is empty -- the interior of a part, free space -- does nothing; otherwise it loops over its
// distinct (a, b) keys as add_to_rows does over labels: ballot, popcount, and the key's first lane issues the integer atomics: one
// atomic per wavefront, key and column, not one per voxel.  The floor column goes the same way.  Agent-scope relaxed integer adds into
// the caller's table; nothing is read back inside the launch.
// k_support: one block of 256 threads per scene, thread = part.  The relation sits in LDS as two 256-bit rows per part, "who rests on
// me" and "on whom I rest" (16 KB); thread a fills its own first row from row a and column a of the table, eight parts at a time so
// that their loads are in flight together, and sets its bit in the second rows of those parts (LDS integer or: any order).  carried, orphans and grounded are closures each thread runs on its own with
// a 256-bit set in registers (every word index is a compile-time constant: no scratch) and a work list: a part is expanded once, so a
// closure expands at most P parts; the orphans' test of a candidate runs once per footing that joined.  layer is the statement's
// rounds, block-wide: read, barrier, write, barrier, at most n times, ended early by a block-uniform flag.  Every loop is bounded by P,
// 64 or 32, __syncthreads stands outside divergent code, and no content of the table or of count moves an access: n is clamped to 0..P.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_closure.h"
#include "gnr_host.h"

#pragma clang fp contract(off)

namespace gnr_support {

using namespace gnr;

typedef __attribute__((address_space(1))) int gint;
__device__ inline void add_to(int* p, int v) { __hip_atomic_fetch_add((gint*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr int MAXP = GNR_SUPPORT_MAX_PARTS, WORDS = MAXP / 32;
static_assert(MAXP == CLOSURE_PARTS && WORDS == CLOSURE_WORDS, "close_over and bits_of (gnr_closure.h) work on sets of 256 parts");

// launch grid: (ceil(2 P P / 256), B), block 256: thread x of scene b writes pairs element x, the first P also floor, the first dropped
__global__ __launch_bounds__(256) void k_contacts_fill(int* __restrict__ pairs, int* __restrict__ floor, int* __restrict__ dropped, int P) {
    const int b = blockIdx.y, x = (int)(blockIdx.x * 256u + threadIdx.x);
    if (x < 2 * P * P) pairs[(size_t)b * 2 * P * P + x] = 0;
    if (x < P) floor[(size_t)b * P + x] = 0;
    if (x == 0) dropped[b] = 0;
}

// the forward half of the neighbourhood (positive linear offset), faces first, then edges, then corners: 3, 9, 13 of them
__host__ __device__ constexpr int forward(int d, int axis) {
    constexpr signed char F[13][3] = {{0, 0, 1},  {0, 1, 0},  {1, 0, 0},   {0, 1, -1}, {0, 1, 1},  {1, 0, -1}, {1, 0, 1},
                                      {1, -1, 0}, {1, 1, 0},  {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
    return F[d][axis];
}

struct Shape {
    int R, n, P, z_min;                        // n = R^3
};

// launch grid: (ceil(R^3 / 256), B), block 256;  ND: the offsets of the connectivity
template <int ND>
__global__ __launch_bounds__(256) void k_contacts(const int* __restrict__ labels, int* __restrict__ pairs, int* __restrict__ floor,
                                                  int* __restrict__ dropped, Shape sh) {
    const int R = sh.R, P = sh.P, b = blockIdx.y;
    const int* lab = labels + (size_t)b * sh.n;
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool live = t < sh.n;
    const int self = live ? t : 0;                                // (a thread beyond the scene reads voxel 0 and credits nothing)
    const int i = self / (R * R), j = (self / R) % R, k = self % R;
    const int lane = threadIdx.x & 63;
    const int a = lab[self];
    int nb[ND];
    bool in[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int di = forward(d, 0), dj = forward(d, 1), dk = forward(d, 2);
        in[d] = live && (unsigned)(i + di) < (unsigned)R && (unsigned)(j + dj) < (unsigned)R && (unsigned)(k + dk) < (unsigned)R;
        nb[d] = lab[in[d] ? self + (di * R + dj) * R + dk : self];
    }
    int* tab = pairs + (size_t)b * 2 * P * P;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int dk = forward(d, 2), c = nb[d];
        const bool has = in[d] && a >= 1 && c >= 1 && a != c;
        unsigned long long todo = __ballot(has);
        if (todo == 0ull) continue;                               // wave-uniform: the common case
        const bool rows = a <= P && c <= P;
        const int key = rows ? (a - 1) * P + (c - 1) : -1;        // (-1: beyond the rows; one key for all of them)
        for (int s = 0; s < 64 && todo; ++s) {
            const int lead = __ffsll((long long)todo) - 1;
            const int kl = __shfl(key, lead);
            const unsigned long long m = __ballot(has && key == kl);
            if (lane == lead) {
                const int cnt = __popcll(m);
                if (kl < 0) {
                    add_to(dropped + b, 2 * cnt);                 // both ordered pairs
                } else {
                    const int ra = kl / P, rc = kl - ra * P;
                    int* ac = tab + 2 * ((size_t)ra * P + rc);
                    int* ca = tab + 2 * ((size_t)rc * P + ra);
                    add_to(ac, cnt);                              // (u, w) = (this voxel, the neighbour)
                    add_to(ca, cnt);                              // (u, w) = (the neighbour, this voxel)
                    if (dk > 0) add_to(ac + 1, cnt);              // the neighbour is the higher one: c lies on a
                    if (dk < 0) add_to(ca + 1, cnt);              // this voxel is the higher one: a lies on c
                }
            }
            todo &= ~m;
        }
    }
    // the floor column
    const bool stands = live && a >= 1 && a <= P && k == sh.z_min;
    unsigned long long todo = __ballot(stands);
    for (int s = 0; s < 64 && todo; ++s) {
        const int lead = __ffsll((long long)todo) - 1;
        const int al = __shfl(a, lead);
        const unsigned long long m = __ballot(stands && a == al);
        if (lane == lead) add_to(floor + (size_t)b * P + (al - 1), __popcll(m));
        todo &= ~m;
    }
}

struct Rule {
    double lean;
    int P, min_contact, min_floor;
};

// launch grid: B, block 256: thread a is part a + 1
__global__ __launch_bounds__(256) void k_support(const int* __restrict__ pairs, const int* __restrict__ floor, const int* __restrict__ count,
                                                 int* __restrict__ below, int* __restrict__ above, int* __restrict__ carried,
                                                 int* __restrict__ orphans, int* __restrict__ layer, int* __restrict__ grounded,
                                                 unsigned char* __restrict__ rests_on, Rule ru) {
    __shared__ unsigned s_up[MAXP][WORDS];                        // bit c of row a: c rests on a
    __shared__ unsigned s_down[MAXP][WORDS];                      // bit c of row a: a rests on c
    __shared__ unsigned s_floor[WORDS];                           // bit a: on_floor(a)
    __shared__ int s_layer[MAXP];
    __shared__ int s_changed;
    const int P = ru.P, b = blockIdx.x, a = threadIdx.x;
    int n = count[b];
    n = n < 0 ? 0 : n > P ? P : n;
    const int* tab = pairs + (size_t)b * 2 * P * P;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) { s_up[a][w] = 0u; s_down[a][w] = 0u; }
    if (a < WORDS) s_floor[a] = 0u;
    if (a == 0) s_changed = 0;
    __syncthreads();
    // ---- the relation: row a and column a of the table -----------------------------------------------------------------------------
    if (a < n) {
        unsigned up[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) up[w] = 0u;
        const int stands = floor[(size_t)b * P + a];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            for (int q0 = 0; q0 < 32 && w * 32 + q0 < n; q0 += 8) {          // eight parts at a time: their loads are in flight together
                int N[8], o_ac[8], o_ca[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = w * 32 + q0 + j < n ? w * 32 + q0 + j : n - 1;     // (a load never leaves the n x n corner)
                    N[j] = tab[2 * ((size_t)a * P + c)];
                    o_ac[j] = tab[2 * ((size_t)a * P + c) + 1];
                    o_ca[j] = tab[2 * ((size_t)c * P + a) + 1];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = w * 32 + q0 + j;
                    const long long D = (long long)o_ac[j] - (long long)o_ca[j];
                    if (c < n && c != a && N[j] >= ru.min_contact && D > 0 && (double)D >= ru.lean * (double)N[j]) {
                        up[w] |= 1u << (q0 + j);
                        atomicOr(&s_down[c][a >> 5], 1u << (a & 31));
                    }
                }
            }
        }
#pragma unroll
        for (int w = 0; w < WORDS; ++w) s_up[a][w] = up[w];
        if (stands >= ru.min_floor) atomicOr(&s_floor[a >> 5], 1u << (a & 31));
    }
    __syncthreads();
    // ---- the closures of part a (registers; LDS is read only) ---------------------------------------------------------------------------
    int n_below = 0, n_above = 0, n_carried = 0, n_orphans = 0, is_grounded = 0;
    if (a < n) {
        unsigned S[WORDS], todo[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) { n_above += __popc(s_up[a][w]); n_below += __popc(s_down[a][w]); }
        // carried: everything reachable along "rests on"
#pragma unroll
        for (int w = 0; w < WORDS; ++w) S[w] = todo[w] = (w == (a >> 5)) ? 1u << (a & 31) : 0u;
        close_over(s_up, S, todo, nullptr);
        n_carried = bits_of(S) - 1;
        // grounded: the footings' footings reach the floor
#pragma unroll
        for (int w = 0; w < WORDS; ++w) S[w] = todo[w] = (w == (a >> 5)) ? 1u << (a & 31) : 0u;
        is_grounded = close_over(s_down, S, todo, s_floor) ? 1 : 0;
        // orphans: F = S.  A part x that joined F offers the parts resting on it; a candidate joins when it is not on the floor and
        // every footing of it is in F.  The last of a part's footings to be expanded finds the others in F.
#pragma unroll
        for (int w = 0; w < WORDS; ++w) S[w] = todo[w] = (w == (a >> 5)) ? 1u << (a & 31) : 0u;
        for (int sweep = 0; sweep <= MAXP; ++sweep) {             // close_over's sweeps
            bool any = false;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) any = any || todo[w] != 0u;
            if (!any) break;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                for (int e = 0; e < 32 && todo[w]; ++e) {
                    const int x = w * 32 + __ffs((int)todo[w]) - 1;
                    todo[w] &= todo[w] - 1u;
#pragma unroll
                    for (int v = 0; v < WORDS; ++v) {
                        unsigned cand = s_up[x][v] & ~S[v] & ~s_floor[v];
                        for (int q = 0; q < 32 && cand; ++q) {
                            const int c = v * 32 + __ffs((int)cand) - 1;
                            const unsigned bit = cand & (0u - cand);
                            cand &= cand - 1u;
                            bool all = true;
#pragma unroll
                            for (int y = 0; y < WORDS; ++y) all = all && (s_down[c][y] & ~S[y]) == 0u;
                            if (all) { S[v] |= bit; todo[v] |= bit; }
                        }
                    }
                }
            }
        }
        n_orphans = bits_of(S) - 1;
    }
    // ---- layer: the statement's rounds, block-wide ------------------------------------------------------------------------------------------
    s_layer[a] = (a < n && n_above == 0) ? 0 : -1;
    __syncthreads();
    for (int round = 0; round < n; ++round) {                     // n is block-uniform
        int mine = -1;
        if (a < n && s_layer[a] < 0) {
            bool ready = true;
            int top = -1;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                unsigned m = s_up[a][w];
                for (int q = 0; q < 32 && m; ++q) {
                    const int c = w * 32 + __ffs((int)m) - 1;
                    m &= m - 1u;
                    const int l = s_layer[c];
                    ready = ready && l >= 0;
                    top = l > top ? l : top;
                }
            }
            if (ready) mine = top + 1;
        }
        __syncthreads();                                          // every read of this round is done
        if (mine >= 0) { s_layer[a] = mine; s_changed = 1; }
        __syncthreads();
        const bool changed = s_changed != 0;
        __syncthreads();                                          // every thread has read the flag
        if (a == 0) s_changed = 0;
        if (!changed) break;                                      // block-uniform
    }
    __syncthreads();
    if (a < P) {
        const size_t o = (size_t)b * P + a;
        below[o] = n_below; above[o] = n_above; carried[o] = n_carried; orphans[o] = n_orphans;
        layer[o] = a < n ? s_layer[a] : -1;
        grounded[o] = is_grounded;
    }
    if (rests_on) {                                               // four bytes a store where the scene's rows are aligned (P even)
        unsigned char* out = rests_on + (size_t)b * P * P;
        auto at = [&](int x) {
            const int c = x / P, f = x - c * P;
            return (s_down[c][f >> 5] >> (f & 31)) & 1u;
        };
        const int cells = P * P, words = ((P & 1) || ((uintptr_t)out & 3u)) ? 0 : cells / 4;
        for (int x = a; x < words; x += 256)                      // at most P * P / 1024 = 64 rounds
            ((unsigned*)out)[x] = at(4 * x) | at(4 * x + 1) << 8 | at(4 * x + 2) << 16 | at(4 * x + 3) << 24;
        for (int x = 4 * words + a; x < cells; x += 256) out[x] = (unsigned char)at(x);       // at most P rounds
    }
}

}  // namespace gnr_support

using namespace gnr_support;

extern "C" int gnr_part_contacts_fwd(const GnrContactsParams* p, const int* labels, int B, int R, int* pairs, int* floor, int* dropped,
                                     void* stream) {
    const Refuse no{"gnr_part_contacts_fwd"};
    if (!p) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (p->max_parts < 1 || p->max_parts > GNR_SUPPORT_MAX_PARTS) return no(GNR_ERR_SHAPE, "max_parts must be in 1..GNR_SUPPORT_MAX_PARTS (256)");
    if (p->connectivity != 6 && p->connectivity != 18 && p->connectivity != 26) return no(GNR_ERR_ARG, "connectivity must be 6, 18 or 26");
    if (p->z_min < 0 || p->z_min > R) return no(GNR_ERR_ARG, "z_min must be in 0..R");
    if (!labels || !pairs || !floor || !dropped) return no(GNR_ERR_ARG, "null pointer");
    const int P = p->max_parts;
    Shape sh{};
    sh.R = R; sh.n = R * R * R; sh.P = P; sh.z_min = p->z_min;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch<k_contacts_fill>("k_contacts_fill@gnr_part_contacts_fwd", st, dim3((unsigned)((2 * P * P + 255) / 256), (unsigned)B), dim3(256),
                                         0, pairs, floor, dropped, P))
        return rc;
    const dim3 grid((unsigned)((sh.n + 255) / 256), (unsigned)B);
    const char* label = "k_contacts@gnr_part_contacts_fwd";
    if (p->connectivity == 6) return launch<k_contacts<3>>(label, st, grid, dim3(256), 0, labels, pairs, floor, dropped, sh);
    if (p->connectivity == 18) return launch<k_contacts<9>>(label, st, grid, dim3(256), 0, labels, pairs, floor, dropped, sh);
    return launch<k_contacts<13>>(label, st, grid, dim3(256), 0, labels, pairs, floor, dropped, sh);
}

extern "C" int gnr_part_support_fwd(const GnrSupportParams* p, const int* pairs, const int* floor, const int* count, int B, int* below,
                                    int* above, int* carried, int* orphans, int* layer, int* grounded, unsigned char* rests_on, void* stream) {
    const Refuse no{"gnr_part_support_fwd"};
    if (!p) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (p->max_parts < 1 || p->max_parts > GNR_SUPPORT_MAX_PARTS) return no(GNR_ERR_SHAPE, "max_parts must be in 1..GNR_SUPPORT_MAX_PARTS (256)");
    if (p->min_contact < 1) return no(GNR_ERR_ARG, "min_contact must be >= 1");
    if (p->min_floor < 1) return no(GNR_ERR_ARG, "min_floor must be >= 1");
    if (!(isfinite(p->lean) && p->lean >= 0.0 && p->lean <= 1.0)) return no(GNR_ERR_ARG, "lean must be finite and in 0..1");
    if (!pairs || !floor || !count || !below || !above || !carried || !orphans || !layer || !grounded) return no(GNR_ERR_ARG, "null pointer");
    Rule ru{};
    ru.lean = p->lean; ru.P = p->max_parts; ru.min_contact = p->min_contact; ru.min_floor = p->min_floor;
    return launch<k_support>("k_support@gnr_part_support_fwd", (hipStream_t)stream, dim3((unsigned)B), dim3(256), 0, pairs, floor, count, below,
                             above, carried, orphans, layer, grounded, rests_on, ru);
}
