// Balance of the parts, on the device: the feet a part stands on -- its voxels in the floor plane and those that lie on a footing --,
// their reach along 16 directions and the part's integer moments up to the second order (gnr_part_feet_fwd), and what follows: whether
// a part's centre of mass lies over its feet, by how much, and what tips and falls when a part is taken (gnr_part_balance_fwd).  What
// the reference leaves to physics (remove_and_wait); no reference counterpart; the statement is include/gnr.h's and
// tests/balance_reference.py's.
// k_feet_fill: one wavefront per part.  It walks the part's row of rests_on 64 footings at a time -- a ballot and a prefix popcount
// give every footing its rank in ascending label order --, writes the whole row of slots and the part's crowded, and the empty value
// into the part's rows of moments, feet and reach (a kernel, not memset nodes: DESIGN 4.8).
// k_feet: one thread per voxel, last axis fastest, grid (chunks of 256, B), as k_contacts.  A thread reads its own label and those of
// the neighbours one plane lower (1, 5 or 9 offsets; a neighbour outside the lattice is replaced by the voxel's own address, so a load
// never leaves the scene) and builds its 8-bit slot mask: bit 0 in the floor plane, bit slots[c,a] per lower neighbour with another
// label a.  slots is read only by the lanes that have such a neighbour, and only in wavefronts whose ballot finds one.  The moments go
// per label and the feet per (label, slot) as add_to_rows' statistics do: the wavefront loops over its distinct keys -- ballot,
// butterfly over the key's lanes, and the key's first lane issues the integer atomics: one per wavefront, key and column.  A
// wavefront's partial sums fit int32 (64 * 255^2); the global sums are 64-bit adds.  Agent-scope relaxed integer atomics into the
// caller's tables; nothing is read back inside the launch.
// k_balance: one block of 256 threads per scene, thread = part.  Thread c evaluates the balance rule of its own mass nine times -- over
// all its usable slots and with each of the eight slots left out --, in registers, every index a compile-time constant.  Then the
// block walks rests_on and slots together, coalesced, four cells a load where the tables are aligned and eight loads in flight a
// thread: "who rests on me" and "who tips when I go" become two 256-bit rows per part in LDS (16 KB; LDS integer or: any order), and
// tips is written.  falls is the closure of the second row under the first, one thread per part (close_over, gnr_closure.h).  Every
// loop is bounded by P, 16 or 8, __syncthreads stands outside divergent code, and no content of a table or of count moves an access:
// n is clamped to 0..P and a slot to 0..7.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_closure.h"
#include "gnr_host.h"

#pragma clang fp contract(off)

namespace gnr_balance {

using namespace gnr;

typedef __attribute__((address_space(1))) int gint;
__device__ inline void add_to(int* p, int v) { __hip_atomic_fetch_add((gint*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr int MAXP = GNR_BALANCE_MAX_PARTS, WORDS = MAXP / 32, SLOTS = GNR_BALANCE_SLOTS, DIRS = GNR_BALANCE_DIRECTIONS, HALF = DIRS / 2;
constexpr int NMOM = 10;
static_assert(MAXP == CLOSURE_PARTS && WORDS == CLOSURE_WORDS, "close_over and bits_of (gnr_closure.h) work on sets of 256 parts");
static_assert(SLOTS == 8 && DIRS == 16, "a slot mask is a byte; k_feet_fill fills a reach row with two stores a lane");

// the 16 directions (dx, dy) of the (i, j) plane: eight, then their negatives in the same order
__host__ __device__ constexpr int dir(int q, int axis) {
    constexpr signed char D[HALF][2] = {{1, 0}, {2, 1}, {1, 1}, {1, 2}, {0, 1}, {-1, 2}, {-1, 1}, {-2, 1}};
    return q < HALF ? D[q][axis] : -D[q - HALF][axis];
}
// |(dx, dy)|: 1, sqrt 2 or sqrt 5 as the nearest doubles
__host__ __device__ constexpr double length_of(int q) {
    const int d2 = dir(q, 0) * dir(q, 0) + dir(q, 1) * dir(q, 1);
    return d2 == 1 ? 1.0 : d2 == 2 ? 1.4142135623730951 : 2.23606797749979;
}

// launch grid: (ceil(P / 4), B), block 256: wavefront w of block x is part 4 x + w + 1
__global__ __launch_bounds__(256) void k_feet_fill(const unsigned char* __restrict__ rests_on, const int* __restrict__ count,
                                                   unsigned long long* __restrict__ moments, unsigned char* __restrict__ slots,
                                                   int* __restrict__ feet, int* __restrict__ reach, int* __restrict__ crowded, int P) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, c = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (c >= P) return;                                           // wave-uniform
    int n = count[b];
    n = n < 0 ? 0 : n > P ? P : n;
    const size_t row = (size_t)b * P + c;
    const unsigned char* rel = rests_on + row * P;
    unsigned char* out = slots + row * P;
    int footings = 0;
    for (int a0 = 0; a0 < P; a0 += 64) {                          // at most four rounds
        const int a = a0 + lane;
        const bool foot = c < n && a < n && a != c && rel[a] != 0;          // (a < n <= P: the load stays in the row)
        const unsigned long long m = __ballot(foot);
        const int rank = footings + __popcll(m & ((1ull << lane) - 1ull)) + 1;
        if (a < P) out[a] = (unsigned char)(foot ? (rank < SLOTS - 1 ? rank : SLOTS - 1) : 0);
        footings += __popcll(m);
    }
    if (lane == 0) crowded[row] = footings >= SLOTS ? 1 : 0;      // slot 7 holds two or more
    if (lane < NMOM) moments[row * NMOM + lane] = 0ull;
    if (lane < SLOTS) feet[row * SLOTS + lane] = 0;
    reach[row * SLOTS * DIRS + lane] = INT32_MIN;
    reach[row * SLOTS * DIRS + 64 + lane] = INT32_MIN;
}

// the neighbours one plane lower (di, dj; dk = -1): the face first, then the four edges, then the four corners: 1, 5, 9 of them
__host__ __device__ constexpr int lower(int d, int axis) {
    constexpr signed char F[9][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
    return F[d][axis];
}

struct Shape {
    int R, n, P, z_min;                        // n = R^3
};

// launch grid: (ceil(R^3 / 256), B), block 256;  ND: the lower offsets of the connectivity
template <int ND>
__global__ __launch_bounds__(256) void k_feet(const int* __restrict__ labels, const unsigned char* __restrict__ slots,
                                              unsigned long long* __restrict__ moments, int* __restrict__ feet, int* __restrict__ reach, Shape sh) {
    const int R = sh.R, P = sh.P, b = blockIdx.y;
    const int* lab = labels + (size_t)b * sh.n;
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool live = t < sh.n;
    const int self = live ? t : 0;                                // (a thread beyond the scene reads voxel 0 and credits nothing)
    const int i = self / (R * R), j = (self / R) % R, k = self % R;
    const int lane = threadIdx.x & 63;
    const int c = lab[self];
    const bool part = live && c >= 1 && c <= P;
    int nb[ND];
    bool in[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int di = lower(d, 0), dj = lower(d, 1);
        in[d] = live && k >= 1 && (unsigned)(i + di) < (unsigned)R && (unsigned)(j + dj) < (unsigned)R;
        nb[d] = lab[in[d] ? self + (di * R + dj) * R - 1 : self];
    }
    // ---- the slot mask ------------------------------------------------------------------------------------------------------------------
    unsigned mask = part && k == sh.z_min ? 1u : 0u;
    const unsigned char* srow = slots + ((size_t)b * P + (part ? c - 1 : 0)) * P;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int a = nb[d];
        const bool has = part && in[d] && a >= 1 && a <= P && a != c;
        if (__ballot(has) == 0ull) continue;                      // wave-uniform: the common case
        if (has) {
            const unsigned s = srow[a - 1] & (unsigned)(SLOTS - 1);
            if (s) mask |= 1u << s;
        }
    }
    // ---- the moments, per label -----------------------------------------------------------------------------------------------------------
    unsigned long long todo = __ballot(part);
    for (int e = 0; e < 64 && todo; ++e) {
        const int lead = __ffsll((long long)todo) - 1;
        const int cl = __shfl(c, lead);
        const bool mine = part && c == cl;
        const unsigned long long m = __ballot(mine);
        int sum[NMOM - 1] = {i, j, k, i * i, j * j, k * k, i * j, i * k, j * k};
#pragma unroll
        for (int a = 0; a < NMOM - 1; ++a) sum[a] = mine ? sum[a] : 0;
        if (__popcll(m) > 1) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
                for (int a = 0; a < NMOM - 1; ++a) sum[a] += __shfl_xor(sum[a], d);
            }
        }
        if (lane == lead) {
            unsigned long long* row = moments + ((size_t)b * P + (cl - 1)) * NMOM;
            atomicAdd(row, (unsigned long long)__popcll(m));
#pragma unroll
            for (int a = 0; a < NMOM - 1; ++a) atomicAdd(row + 1 + a, (unsigned long long)sum[a]);
        }
        todo &= ~m;
    }
    // ---- the feet, per (label, slot) ---------------------------------------------------------------------------------------------------
    if (__ballot(mask != 0u) == 0ull) return;                     // wave-uniform: the interior of a part, free space
    for (int s = 0; s < SLOTS; ++s) {
        const bool foot = (mask >> s) & 1u;
        todo = __ballot(foot);
        for (int e = 0; e < 64 && todo; ++e) {
            const int lead = __ffsll((long long)todo) - 1;
            const int cl = __shfl(c, lead);
            const bool mine = foot && c == cl;
            const unsigned long long m = __ballot(mine);
            int hi[HALF], lo[HALF];                               // the largest and the smallest dx i + dy j: the reach along d and along -d
#pragma unroll
            for (int q = 0; q < HALF; ++q) {
                const int p = dir(q, 0) * i + dir(q, 1) * j;
                hi[q] = mine ? p : INT32_MIN;
                lo[q] = mine ? p : INT32_MAX;
            }
            if (__popcll(m) > 1) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
                    for (int q = 0; q < HALF; ++q) {
                        const int oh = __shfl_xor(hi[q], d), ol = __shfl_xor(lo[q], d);
                        hi[q] = oh > hi[q] ? oh : hi[q];
                        lo[q] = ol < lo[q] ? ol : lo[q];
                    }
                }
            }
            if (lane == lead) {
                const size_t row = ((size_t)b * P + (cl - 1)) * SLOTS + s;
                add_to(feet + row, __popcll(m));
#pragma unroll
                for (int q = 0; q < HALF; ++q) {
                    atomicMax(reach + row * DIRS + q, hi[q]);
                    atomicMax(reach + row * DIRS + HALF + q, -lo[q]);
                }
            }
            todo &= ~m;
        }
    }
}

struct Rule {
    int P, min_floor;
};

// launch grid: B, block 256: thread c is part c + 1
__global__ __launch_bounds__(256) void k_balance(const long long* __restrict__ moments, const int* __restrict__ feet, const int* __restrict__ reach,
                                                 const unsigned char* __restrict__ slots, const unsigned char* __restrict__ rests_on,
                                                 const int* __restrict__ count, int* __restrict__ balanced, double* __restrict__ margin,
                                                 int* __restrict__ unsettles, int* __restrict__ falls, unsigned char* __restrict__ tips, Rule ru) {
    __shared__ unsigned s_up[MAXP][WORDS];                        // bit c of row a: c rests on a
    __shared__ unsigned s_tip[MAXP][WORDS];                       // bit c of row a: c tips when a is taken
    __shared__ unsigned s_unbal[MAXP];                            // bit s of entry c: c is not balanced once slot s is gone; bit 8: as it lies
    const int P = ru.P, b = blockIdx.x, c = threadIdx.x;
    int n = count[b];
    n = n < 0 ? 0 : n > P ? P : n;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) { s_up[c][w] = 0u; s_tip[c][w] = 0u; }
    // ---- the balance of part c's own mass: over all its usable slots (x == SLOTS) and without slot x ----------------------------------------
    unsigned unbal = 0u;
    double least = -INFINITY;
    if (c < n) {
        const size_t row = (size_t)b * P + c;
        const long long m = moments[row * NMOM], Si = moments[row * NMOM + 1], Sj = moments[row * NMOM + 2];
        unsigned use = 0u;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) use |= feet[row * SLOTS + s] >= (s == 0 ? ru.min_floor : 1) ? 1u << s : 0u;
        if (m < 1) use = 0u;                                      // no mass: nothing to balance
#pragma unroll
        for (int x = 0; x <= SLOTS; ++x) unbal |= (use & ~(1u << x) & 0xffu) == 0u ? 1u << x : 0u;       // no usable slot left
        if (use) {
            least = INFINITY;
            const int* rc = reach + row * SLOTS * DIRS;
#pragma unroll
            for (int q = 0; q < DIRS; ++q) {
                int rs[SLOTS];
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) rs[s] = rc[s * DIRS + q];
                const long long width = (dir(q, 0) < 0 ? -dir(q, 0) : dir(q, 0)) + (dir(q, 1) < 0 ? -dir(q, 1) : dir(q, 1));
                const long long lever = 2 * (dir(q, 0) * Si + dir(q, 1) * Sj);
#pragma unroll
                for (int x = 0; x <= SLOTS; ++x) {
                    const unsigned set = use & ~(1u << x) & 0xffu;
                    long long r = INT32_MIN;
#pragma unroll
                    for (int s = 0; s < SLOTS; ++s) r = ((set >> s) & 1u) && rs[s] > r ? rs[s] : r;
                    const long long num = m * (2 * r + width) - lever;
                    if (set && num < 0) unbal |= 1u << x;
                    if (x == SLOTS) {
                        const double v = (double)num / ((double)(2 * m) * length_of(q));
                        least = v < least ? v : least;
                    }
                }
            }
        }
    }
    s_unbal[c] = unbal;
    __syncthreads();
    // ---- who rests on whom, who tips when whom is taken: the two tables, walked together ----------------------------------------------------
    const unsigned char* rel = rests_on + (size_t)b * P * P;
    const unsigned char* slo = slots + (size_t)b * P * P;
    unsigned char* tip_rows = tips ? tips + (size_t)b * P * P : nullptr;
    auto cell = [&](int x, unsigned rests_byte, unsigned slot_byte) -> unsigned {      // cell x of the tables -> its tips byte
        const int up = x / P, a = x - up * P;                     // `up` rests on a
        const bool rests = up < n && a < n && up != a && rests_byte != 0u;
        const bool tip = rests && ((s_unbal[up] >> (slot_byte & (unsigned)(SLOTS - 1))) & 1u);
        if (rests) atomicOr(&s_up[a][up >> 5], 1u << (up & 31));
        if (tip) atomicOr(&s_tip[a][up >> 5], 1u << (up & 31));
        return tip ? 1u : 0u;
    };
    // four cells a load and a store where the scene's tables are aligned (P even), as k_support writes rests_on
    const int cells = P * P;
    const int words = ((P & 1) || (((uintptr_t)rel | (uintptr_t)slo | (uintptr_t)tip_rows) & 3u)) ? 0 : cells / 4;
    constexpr int AHEAD = 8;                                      // words a thread loads before it uses the first: their latencies overlap
    for (int w0 = c; w0 < words; w0 += 256 * AHEAD) {             // at most P * P / 8192 = 8 rounds
        unsigned rw[AHEAD], sw[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int w = w0 + 256 * u < words ? w0 + 256 * u : w0;      // (a load never leaves the scene's tables)
            rw[u] = ((const unsigned*)rel)[w];
            sw[u] = ((const unsigned*)slo)[w];
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int w = w0 + 256 * u;
            if (w >= words) break;
            unsigned tw = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) tw |= cell(4 * w + j, (rw[u] >> (8 * j)) & 255u, (sw[u] >> (8 * j)) & 255u) << (8 * j);
            if (tip_rows) ((unsigned*)tip_rows)[w] = tw;
        }
    }
    for (int x = 4 * words + c; x < cells; x += 256) {            // at most P rounds
        const unsigned t = cell(x, rel[x], slo[x]);
        if (tip_rows) tip_rows[x] = (unsigned char)t;
    }
    __syncthreads();
    // ---- what falls when part c is taken: the parts that tip and everything they carry (registers; LDS is read only) ------------------------
    int n_tip = 0, n_fall = 0;
    if (c < n) {
        unsigned S[WORDS], todo[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) S[w] = todo[w] = s_tip[c][w];
        n_tip = bits_of(S);
        close_over(s_up, S, todo, nullptr);
#pragma unroll
        for (int w = 0; w < WORDS; ++w) S[w] &= (w == (c >> 5)) ? ~(1u << (c & 31)) : ~0u;       // (a cycle may lead back to c itself)
        n_fall = bits_of(S);
    }
    if (c < P) {
        const size_t o = (size_t)b * P + c;
        balanced[o] = c < n && !((unbal >> SLOTS) & 1u) ? 1 : 0;
        margin[o] = least;
        unsettles[o] = n_tip;
        falls[o] = n_fall;
    }
}

}  // namespace gnr_balance

using namespace gnr_balance;

extern "C" int gnr_part_feet_fwd(const GnrFeetParams* p, const int* labels, const unsigned char* rests_on, const int* count, int B, int R,
                                 long long* moments, unsigned char* slots, int* feet, int* reach, int* crowded, void* stream) {
    const Refuse no{"gnr_part_feet_fwd"};
    if (!p) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (p->max_parts < 1 || p->max_parts > GNR_BALANCE_MAX_PARTS) return no(GNR_ERR_SHAPE, "max_parts must be in 1..GNR_BALANCE_MAX_PARTS (256)");
    if (p->connectivity != 6 && p->connectivity != 18 && p->connectivity != 26) return no(GNR_ERR_ARG, "connectivity must be 6, 18 or 26");
    if (p->z_min < 0 || p->z_min > R) return no(GNR_ERR_ARG, "z_min must be in 0..R");
    if (!labels || !rests_on || !count || !moments || !slots || !feet || !reach || !crowded) return no(GNR_ERR_ARG, "null pointer");
    const int P = p->max_parts;
    Shape sh{};
    sh.R = R; sh.n = R * R * R; sh.P = P; sh.z_min = p->z_min;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* mom = (unsigned long long*)moments;       // (sums of squares and counts: never negative)
    if (int rc = launch<k_feet_fill>("k_feet_fill@gnr_part_feet_fwd", st, dim3((unsigned)((P + 3) / 4), (unsigned)B), dim3(256), 0, rests_on, count,
                                     mom, slots, feet, reach, crowded, P))
        return rc;
    const dim3 grid((unsigned)((sh.n + 255) / 256), (unsigned)B);
    const char* label = "k_feet@gnr_part_feet_fwd";
    const unsigned char* slot_rows = slots;
    if (p->connectivity == 6) return launch<k_feet<1>>(label, st, grid, dim3(256), 0, labels, slot_rows, mom, feet, reach, sh);
    if (p->connectivity == 18) return launch<k_feet<5>>(label, st, grid, dim3(256), 0, labels, slot_rows, mom, feet, reach, sh);
    return launch<k_feet<9>>(label, st, grid, dim3(256), 0, labels, slot_rows, mom, feet, reach, sh);
}

extern "C" int gnr_part_balance_fwd(const GnrBalanceParams* p, const long long* moments, const int* feet, const int* reach,
                                    const unsigned char* slots, const unsigned char* rests_on, const int* count, int B, int* balanced,
                                    double* margin, int* unsettles, int* falls, unsigned char* tips, void* stream) {
    const Refuse no{"gnr_part_balance_fwd"};
    if (!p) return no(GNR_ERR_ARG, "null pointer");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (p->max_parts < 1 || p->max_parts > GNR_BALANCE_MAX_PARTS) return no(GNR_ERR_SHAPE, "max_parts must be in 1..GNR_BALANCE_MAX_PARTS (256)");
    if (p->min_floor < 1) return no(GNR_ERR_ARG, "min_floor must be >= 1");
    if (!moments || !feet || !reach || !slots || !rests_on || !count || !balanced || !margin || !unsettles || !falls) return no(GNR_ERR_ARG, "null pointer");
    Rule ru{};
    ru.P = p->max_parts; ru.min_floor = p->min_floor;
    return launch<k_balance>("k_balance@gnr_part_balance_fwd", (hipStream_t)stream, dim3((unsigned)B), dim3(256), 0, moments, feet, reach, slots,
                             rests_on, count, balanced, margin, unsettles, falls, tips, ru);
}
