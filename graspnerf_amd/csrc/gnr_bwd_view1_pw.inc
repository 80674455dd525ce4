// k_view1_bwd_pw: the first view loop's backward with PARTNER WAVEFRONTS (round 5; included by gnr_bwd.inc).
//
// k_view1_bwd keeps 291 registers of weight-gradient state per wavefront (160 in MFMA accumulator blocks, 131 in per-lane partial
// sums) next to a ~210-register forward + dX working set: 512 registers, one wavefront per SIMD, and nothing to hide its gathers,
// LDS round trips and scatter atomics behind (DESIGN.md 7).  Sharing the accumulators across the wavefronts of a workgroup needs
// four workgroup barriers per (tile, view) and per-stage block ownership; this kernel takes the other route to a second wavefront
// per SIMD: the two halves of the work get a wavefront EACH.
//   compute wavefront c (0..3): projection, gathers, forward recompute, the dX chain -- k_view1_bwd's code with every weight-
//       gradient product taken out: it writes the operand tiles of a stage (dY [16 points][<= 48], X [16][<= 48]) into a slot of
//       its pair's ring in LDS and goes on; ~210 registers;
//   partner wavefront 4 + c: consumes the slots in order -- the outer products of the stage on the matrix cores into ITS accumulator
//       blocks, the bias sums as column sums of the dY tile it reads anyway, the last-layer rows and the gate row as one-block stages
//       of their own (no per-lane partial sums anywhere), and, as the last stage of a (tile, view), the scatter atomics of the
//       feature-map gradient from the rows the compute wavefront parked; at the end it writes the pair's slot of the
//       deterministic reduction (same slots, same fixed-order reduce as before: nothing about the parameter gradients' bit
//       reproducibility changes -- one wavefront adds one pair's tiles in tile order).
// A pair synchronises through two counters in LDS (slots produced / consumed; the LDS executes a wavefront's instructions in order,
// release / acquire at workgroup scope add the waitcnts), never through a workgroup barrier: pairs drift freely, trip counts may
// differ.  512 threads, <= 256 registers, two wavefronts per SIMD, 154 KB of LDS: the weight image of k_view1_bwd + 4 rings of 3 slots.
// use_vis levels keep k_view1_bwd<true> (its 59 accumulator blocks do not fit the partner's 256 registers).
namespace gnr {

namespace l1p {
constexpr int NSLOT = 3;                            // ring depth per pair
constexpr int OUTER_UNROLL = 2;                     // k-steps of an outer product in flight (pw_outer); 4 (every k-step of a stage): 176 - 244 bytes
                                                    // of scratch on the partner; 1 or 2: none, 230 registers
constexpr int TSP = 48;                             // tile row stride: the 4 k-groups of an MFMA operand read disjoint banks (48 mod 64)
constexpr int SLOT = 2 * 16 * TSP;                  // dY tile | X tile (the scatter stage: 16 rows x 64 values | 16 x 8 tap records)
constexpr int RING = l1::TILES;                     // behind k_view1_bwd's weight image
constexpr int FLAGS = RING + 4 * NSLOT * SLOT;      // per pair: produced, consumed, kind[NSLOT]
constexpr int TOTAL = FLAGS + 4 * 8;
static_assert(TOTAL * 4 <= 160 * 1024, "k_view1_bwd_pw: LDS");
static_assert(16 * 64 + 16 * 8 + 1 <= SLOT, "the scatter rows, tap records and the scene-view index fit a slot");
}

DEV int pw_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
DEV void pw_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }

// one pair's ring of NSLOT slots, seen from either side
template <int NSLOT>
struct PwRingN {
    float* slots; int* produced; int* consumed; int* kind; int* dead;
    unsigned* status;                              // the backward's status word (BwdGuard::status): bit 4 = GNR_STATUS_LOST_PARTNER
    int seq;                                       // next slot to produce (compute side) / to consume (partner side)
    // A wavefront whose partner never answers must not hang the device: after 2^22 polls (a few tenths of a second) the wait gives up,
    // raises GNR_STATUS_LOST_PARTNER in the status word (gnr_range_status bit 4: the call's gradients are garbage, and the caller can
    // tell) and poisons the pair's counters so that both sides run to the end.
    static constexpr int MAX_POLLS = 1 << 22;
    DEV void spin(const int* p, int want_at_least) {
        for (int n = 0; pw_load(p) < want_at_least; ++n) {
            if (pw_load(dead)) return;
            __builtin_amdgcn_s_sleep(2);
            if (n > MAX_POLLS) {
                pw_store(dead, 1);
                if (status && (threadIdx.x & 63) == 0) atomicOr(status, 16u);
                return;
            }
        }
    }
    DEV float* acquire_free() {                    // compute side: the slot `seq` may be overwritten once the partner is past seq - NSLOT
        spin(consumed, seq - NSLOT + 1);
        return slots + (seq % NSLOT) * l1p::SLOT;
    }
    DEV void publish(int k) {                      // all lanes of the wavefront have written their part of the slot
        kind[seq % NSLOT] = k;
        ++seq;
        pw_store(produced, seq);
    }
    DEV const float* acquire_full(int& k) {        // partner side
        spin(produced, seq + 1);
        k = __builtin_amdgcn_readfirstlane(kind[seq % NSLOT]);
        return slots + (seq % NSLOT) * l1p::SLOT;
    }
    DEV void release() { ++seq; pw_store(consumed, seq); }
};
using PwRing = PwRingN<l1p::NSLOT>;

// partner side: acc[bi * NBJ + bj] += dY block bi (x) X block bj over the slot's 16 points; gb[bi] += this lane's share of the column
// sums of dY block bi (rows 4s + kg, column 16 bi + c: the four k-groups are added at the flush)
template <int NBI, int NBJ, int UNR = l1p::OUTER_UNROLL>
DEV void pw_outer(const float* __restrict__ slot, int lane, f4 (&acc)[NBI * NBJ], float (&gb)[NBI]) {
    const float* Ta = slot;
    const float* Tb = slot + 16 * l1p::TSP;
    const int c = lane & 15, kg = lane >> 4;
#pragma unroll UNR
    for (int s = 0; s < 4; ++s) {
        float av[NBI], bv[NBJ];
#pragma unroll
        for (int bi = 0; bi < NBI; ++bi) { av[bi] = Ta[(4 * s + kg) * l1p::TSP + 16 * bi + c]; gb[bi] += av[bi]; }
#pragma unroll
        for (int bj = 0; bj < NBJ; ++bj) bv[bj] = Tb[(4 * s + kg) * l1p::TSP + 16 * bj + c];
#pragma unroll
        for (int bi = 0; bi < NBI; ++bi)
#pragma unroll
            for (int bj = 0; bj < NBJ; ++bj) acc[bi * NBJ + bj] = mfma16(av[bi], bv[bj], acc[bi * NBJ + bj]);
    }
}
// column sums -> canonical bias entries: column 16 bi + c of the dY tile is entry `col` of the bias (natural / x layouts: the column
// index IS the canonical index), n valid columns
// (col0: the bias starts at column `col0` of the tile -- layers sharing a dY block)
template <int NBI>
DEV void pw_flush_bias(float* __restrict__ dst, int n, int lane, const float (&gb)[NBI], int col0 = 0) {
#pragma unroll
    for (int bi = 0; bi < NBI; ++bi) {
        float s = gb[bi];
        s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
        const int col = 16 * bi + (lane & 15) - col0;
        if (lane < 16 && col >= 0 && col < n) dst[col] = s;
    }
}

template <int NB>
DEV void pw_put_nat(float* __restrict__ T, int r, int g, const float (&x)[4 * NB], float scale, int col0 = 0) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
        *reinterpret_cast<f4*>(T + r * l1p::TSP + col0 + 16 * nb + 4 * g) = f4{x[4 * nb] * scale, x[4 * nb + 1] * scale, x[4 * nb + 2] * scale, x[4 * nb + 3] * scale};
}

enum { PW_STAGE = 0, PW_SKIP = 1 };
// Small layers share accumulator blocks (the partner's 213 persistent registers did not fit next to its working set: 312 bytes of
// scratch in round 5): neuray_fc.0 (8 x 32) leaves rows 8..15 of its two blocks free, and every layer whose X tile is 32 wide can
// drop its dY columns there -- the decoders' last-layer rows (mean 2, var 2, aw 1: columns 8..12 of the dY tile, X = h2) and
// neuray_fc.2's row (column 13, X = n1t in the first block only).  Their bias sums ride in the same column sums.  181 registers.
constexpr int W3_ROW0 = 8, NR2_ROW = 13;
enum { ST1_STAGE = 0, ST1_END = 1 };      // slot kinds: a stage of the pair in flight (the partner knows the order) / the compute wavefront is done

template <bool FX = false, bool BINS = false>      // BINS: the scatter rows are parked for k_scatter_gather (gnr_bwd_scatter.inc; float mode only)
__global__ __launch_bounds__(512, 2) void k_view1_bwd_pw(View1BwdArgs a) {
    static_assert(!(FX && BINS), "the binned scatter is the float mode's");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (bwd_guard_skip(a.guard)) return;
    // ---- the weight image of k_view1_bwd (pair form: C16 forward fragments, pkb::P1_* transposed fragments)
    for (int i = threadIdx.x; i < pk::BASE1; i += 512) lds[i] = a.wpk[pk::C16 + i];
    if (threadIdx.x < 304) lds[l1::BI + threadIdx.x] = a.wpk[pk::B_DEC1 + threadIdx.x];
    if (threadIdx.x < 184) lds[l1::TB + threadIdx.x] = a.wpk[pk::T_DEC3 + threadIdx.x];
    if (threadIdx.x < 4) lds[l1::SC + threadIdx.x] = a.wpk[pk::T_SCAL + threadIdx.x];
    for (int i = threadIdx.x; i < l1::T_PE0HV - l1::BW; i += 512) lds[l1::BW + i] = a.wbk[pkb::P1_BEGIN + i];
    for (int i = threadIdx.x; i < l1::TILES - l1::T_PE0HV; i += 512) lds[l1::T_PE0HV + i] = a.wbk[pkb::T_PE0HV + i];
    if (threadIdx.x < 32) reinterpret_cast<int*>(lds + l1p::FLAGS)[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), pair = wave & 3;
    const bool partner = wave >= 4;
    PwRing ring;
    ring.slots = lds + l1p::RING + pair * l1p::NSLOT * l1p::SLOT;
    {
        int* f = reinterpret_cast<int*>(lds + l1p::FLAGS) + pair * 8;
        ring.produced = f; ring.consumed = f + 1; ring.kind = f + 2; ring.dead = f + 6; ring.seq = 0;
        ring.status = a.guard.status;
    }
    const int V = a.V, tps = (a.P + 15) >> 4;
    if (partner && a.guard.lose_partner) return;                   // GNR_OPT_TEST_LOSE_PARTNER: the compute wavefronts' waits must give up and say so

    if (partner) {
        // =========================== partner wavefront: weight gradients, bias sums, scatter ===========================
        f4 gWr2[3], gWr1[1], gWnr0[2], gWpe2[4], gWpe0[6], gWd2[3][4], gWd1[3][4];
        float bR2[3] = {0.f, 0.f, 0.f}, bR1[1] = {0.f}, bNR0[1] = {0.f}, bPE2[2] = {0.f, 0.f}, bPE0[2] = {0.f, 0.f};
        float bD2[3][2], bD1[3][2];
        const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 3; ++q) gWr2[q] = z4;
        gWr1[0] = z4; gWnr0[0] = z4; gWnr0[1] = z4;
#pragma unroll
        for (int q = 0; q < 4; ++q) gWpe2[q] = z4;
#pragma unroll
        for (int q = 0; q < 6; ++q) gWpe0[q] = z4;
#pragma unroll
        for (int br = 0; br < 3; ++br) {
            bD2[br][0] = 0.f; bD2[br][1] = 0.f; bD1[br][0] = 0.f; bD1[br][1] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) { gWd2[br][q] = z4; gWd1[br][q] = z4; }
        }
        // One trip = the stages of one (tile, view) in the order the compute wavefront publishes them; a pair the compute side skips
        // publishes nothing, the end of its tile list publishes ST1_END.  (No (tile, view) loop and no "skipped pair" branch here: with that
        // branch the register allocator shuffled ~50 accumulator registers through scratch at every pair -- 1 044 bytes of scratch.)
        for (;;) {
            int k;
            const float* s = ring.acquire_full(k);
            if (k == ST1_END || pw_load(ring.dead)) break;
            pw_outer<3, 1>(s, lane, gWr2, bR2); ring.release();
            s = ring.acquire_full(k); pw_outer<1, 1>(s, lane, gWr1, bR1); ring.release();
            s = ring.acquire_full(k); pw_outer<1, 1>(s, lane, reinterpret_cast<f4(&)[1]>(gWnr0[0]), bNR0); ring.release();     // neuray_fc.2: row NR2_ROW
            s = ring.acquire_full(k); pw_outer<1, 2>(s, lane, gWnr0, bNR0); ring.release();
            s = ring.acquire_full(k); pw_outer<2, 2>(s, lane, gWpe2, bPE2); ring.release();
            s = ring.acquire_full(k); pw_outer<2, 3>(s, lane, gWpe0, bPE0); ring.release();
#pragma unroll
            for (int br = 0; br < 3; ++br) {
                s = ring.acquire_full(k); pw_outer<1, 2>(s, lane, gWnr0, bNR0); ring.release();                             // last-layer rows W3_ROW0 + 2 br
                s = ring.acquire_full(k); pw_outer<2, 2>(s, lane, gWd2[br], bD2[br]); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 2>(s, lane, gWd1[br], bD1[br]); ring.release();
            }
            // ---- scatter: rows [16][64] = d(ray channels | image-feature channels) of the 16 points, tap records [16][8] = 4 weights
            // (0 where the point is dead) + 4 pixel offsets, the scene-view index behind them; one wavefront instruction adds the 64
            // channels of ONE feature-map pixel  (BINS: no such stage -- the compute wavefront parks its rows in HBM itself, gnr_bwd_scatter.inc)
            if constexpr (!BINS) {
                s = ring.acquire_full(k);
                const float* taps = s + 16 * 64;
                const int bv = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(taps)[16 * 8]);
                const size_t gbase = (size_t)bv * a.fh * a.fw * 64 + lane;
                const float fxs = FX ? fx_scale(a.fx) : 0.f;
#pragma unroll 2
                for (int pp = 0; pp < 16; ++pp) {                      // (rolled: fully unrolled the 16 x (row + tap record) loads are hoisted in front of the atomics -- 140 registers the accumulators need)
                    const float val = s[pp * 64 + lane];
                    const f4 wq = *reinterpret_cast<const f4*>(taps + pp * 8);
                    const int* ip = reinterpret_cast<const int*>(taps + pp * 8 + 4);
                    if (wq.x != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[0] * 64, val * wq.x, fxs, a.fx.flag);
                    if (wq.y != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[1] * 64, val * wq.y, fxs, a.fx.flag);
                    if (wq.z != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[2] * 64, val * wq.z, fxs, a.fx.flag);
                    if (wq.w != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[3] * 64, val * wq.w, fxs, a.fx.flag);
                }
                ring.release();
            }
        }
        // ---- flush into the pair's slot of the deterministic reduction (canonical, state-dict order)
        float* gc = a.dpart + (size_t)(blockIdx.x * 4 + pair) * GP_STRIDE;
        const int d0w[3] = {can::MEAN0_W, can::VAR0_W, can::AW0_W}, d0b[3] = {can::MEAN0_B, can::VAR0_B, can::AW0_B};
        const int d2w[3] = {can::MEAN2_W, can::VAR2_W, can::AW2_W}, d2b[3] = {can::MEAN2_B, can::VAR2_B, can::AW2_B};
        const int d4w[3] = {can::MEAN4_W, can::VAR4_W, can::AW4_W}, d4b[3] = {can::MEAN4_B, can::VAR4_B, can::AW4_B};
#pragma unroll
        for (int br = 0; br < 3; ++br) {
            flush_blocks<2, 2>(gc + d0w[br], 32, 32, 32, lane, gWd1[br]);
            flush_blocks<2, 2>(gc + d2w[br], 32, 32, 32, lane, gWd2[br]);
            pw_flush_bias<2>(gc + d0b[br], 32, lane, bD1[br]);
            pw_flush_bias<2>(gc + d2b[br], 32, lane, bD2[br]);
            flush_blocks<1, 2>(gc + d4w[br], 32, br < 2 ? 2 : 1, 32, lane, gWnr0, W3_ROW0 + 2 * br);     // the branch's rows of the shared blocks
            pw_flush_bias<1>(gc + d4b[br], br < 2 ? 2 : 1, lane, bNR0, W3_ROW0 + 2 * br);
        }
        flush_blocks<2, 3>(gc + can::PE0_W, 34, 32, 34, lane, gWpe0);
        pw_flush_bias<2>(gc + can::PE0_B, 32, lane, bPE0);
        flush_blocks<2, 2>(gc + can::PE2_W, 32, 32, 32, lane, gWpe2);
        pw_flush_bias<2>(gc + can::PE2_B, 32, lane, bPE2);
        flush_blocks<1, 2>(gc + can::NR0_W, 32, 8, 32, lane, gWnr0);
        pw_flush_bias<1>(gc + can::NR0_B, 8, lane, bNR0);
        flush_blocks<1, 1>(gc + can::NR2_W, 8, 1, 8, lane, reinterpret_cast<const f4(&)[1]>(gWnr0[0]), NR2_ROW);
        pw_flush_bias<1>(gc + can::NR2_B, 1, lane, bNR0, NR2_ROW);
        flush_blocks<3, 1>(gc + can::RDF2_W, 16, 35, 16, lane, gWr2);
        pw_flush_bias<3>(gc + can::RDF2_B, 35, lane, bR2);
        flush_blocks<1, 1>(gc + can::RDF0_W, 4, 16, 4, lane, gWr1);
        pw_flush_bias<1>(gc + can::RDF0_B, 16, lane, bR1);
        return;
    }

    // =========================== compute wavefront: forward recompute + dX chain ===========================
    const float fsx = (float)a.fw / (float)(a.W - 1), fsy = (float)a.fh / (float)(a.H - 1);
    for (int tile = blockIdx.x * 4 + pair; tile < a.ntiles; tile += gridDim.x * 4) {
        const int b = tile / tps, ts = tile - b * tps;
        const int n_raw = ts * 16 + r;
        const bool row_ok = n_raw < a.P;
        const int n = row_ok ? n_raw : a.P - 1;
        const size_t pt = (size_t)b * a.P + n;
        float p[3], qd[3], lo, hi;
        {
            const f4 d0 = reinterpret_cast<const f4*>(a.desc)[pt * 2], d1 = reinterpret_cast<const f4*>(a.desc)[pt * 2 + 1];
            p[0] = d0.x; p[1] = d0.y; p[2] = d0.z; qd[0] = d0.w; qd[1] = d1.x; qd[2] = d1.y; lo = d1.z; hi = d1.w;
        }
#pragma unroll 1
        for (int v = 0; v < V; ++v) {
            asm volatile("" ::: "memory");
            const int bv = b * V + v;
            const float* vp = a.viewp + bv * VIEWP_FLOATS;
            ViewGeom vg;
            project_view<true>(vp, p, qd, a.H, a.W, vg);
            const float m = vg.m;
            if (a.skip_masked && __ballot(m != 0.f) == 0ull) {          // see k_view1_bwd: nothing flows through this (tile, view)
                if constexpr (BINS) a.sc.key[((size_t)tile * V + v) * 16 + r] = -1;      // binned scatter: 16 dead rows
                continue;                                                // (nothing is published: the partner follows stage ids, not pairs)
            }
            const Taps t = make_taps(vg.u, vg.v, fsx, fsy, -0.5f, a.fh, a.fw);
            const float w00 = t.w00 * m, w01 = t.w01 * m, w10 = t.w10 * m, w11 = t.w11 * m;
            float FR[8];
            {
                const float* fb = a.feat64 + (size_t)bv * a.fh * a.fw * 64 + 8 * g;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f4 a0 = reinterpret_cast<const f4*>(fb + (size_t)t.o00 * 64)[h], a1 = reinterpret_cast<const f4*>(fb + (size_t)t.o01 * 64)[h];
                    const f4 a2 = reinterpret_cast<const f4*>(fb + (size_t)t.o10 * 64)[h], a3 = reinterpret_cast<const f4*>(fb + (size_t)t.o11 * 64)[h];
                    const f4 fr = a0 * w00 + a1 * w01 + a2 * w10 + a3 * w11;
                    FR[4 * h] = fr.x; FR[4 * h + 1] = fr.y; FR[4 * h + 2] = fr.z; FR[4 * h + 3] = fr.w;
                }
            }
            // ---- forward recompute (the forward kernel's instruction sequence on the C16 image)
            float h1[3][8], h2[3][8], o5[5];
            f4 acc[2];
            const P8 frp = split8<0>(FR);
#pragma unroll
            for (int br = 0; br < 3; ++br) {
                load_bias<2>(lds + l1::B_DEC1 + br * 32, g, acc);
                mm16<1, 2, true>(lds + l1::DEC1 + br * 1024, lane, &frp, acc);
                elu_to<2, false>(acc, h1[br]);
                load_bias<2>(lds + l1::B_DEC2 + br * 32, g, acc);
                { const P8U hp = split8u<0>(h1[br]); mm16u<1, 2, true>(lds + l1::DEC2 + br * 1024, lane, &hp, acc); }
                elu_to<2>(acc, h2[br]);
            }
            o5[0] = gsum(dot8(lds + l1::T_DEC3, g, h2[0])) + lds[l1::T_DEC3_B];
            o5[1] = gsum(dot8(lds + l1::T_DEC3 + 32, g, h2[0])) + lds[l1::T_DEC3_B + 1];
            o5[2] = gsum(dot8(lds + l1::T_DEC3 + 64, g, h2[1])) + lds[l1::T_DEC3_B + 2];
            o5[3] = gsum(dot8(lds + l1::T_DEC3 + 96, g, h2[1])) + lds[l1::T_DEC3_B + 3];
            o5[4] = gsum(dot8(lds + l1::T_DEC3 + 128, g, h2[2])) + lds[l1::T_DEC3_B + 4];
            const float mean0 = softplus1(o5[0]), mean1 = softplus1(o5[1]);
            const float var0 = softplus1(o5[2]) + 0.05f, var1 = softplus1(o5[3]) + 0.05f;
            const float aw = sigmoid1(o5[4]);
            const float dinv = -rcp1(fmaxf(vg.z, 1e-5f));
            const float dhat = (dinv - vp[15]) * vp[17];
            const float nearv = dhat - lo, farv = dhat + hi;
            const float r00 = 0.5f + 0.5f * tanh1((nearv - mean0) * var0), r01 = 0.5f + 0.5f * tanh1((nearv - mean1) * var1);
            const float r10 = 0.5f + 0.5f * tanh1((farv - mean0) * var0), r11 = 0.5f + 0.5f * tanh1((farv - mean1) * var1);
            const float vis = ((1.f - r00) * aw + (1.f - r01) * (1.f - aw)) * m;
            const float hit = ((r10 - r00) * aw + (r11 - r01) * (1.f - aw)) * m;
            float e1[8], e[8];
            P8 e1p;
            const float hitp = (hit - 0.5f) * 2.f, visp = (vis - 0.5f) * 2.f;
            {
                load_bias<2>(lds + l1::B_PE1, g, acc);
                mm16<1, 2, true>(lds + l1::PE1, lane, &frp, acc);
                const float extra[1] = {g == 0 ? hitp : (g == 1 ? visp : 0.f)};
                mm<1, 2, 8>(lds + l1::PE1, lane, extra, acc);
                e1[0] = fmaxf(acc[0].x, 0.f); e1[1] = fmaxf(acc[0].y, 0.f); e1[2] = fmaxf(acc[0].z, 0.f); e1[3] = fmaxf(acc[0].w, 0.f);
                e1[4] = fmaxf(acc[1].x, 0.f); e1[5] = fmaxf(acc[1].y, 0.f); e1[6] = fmaxf(acc[1].z, 0.f); e1[7] = fmaxf(acc[1].w, 0.f);
                load_bias<2>(lds + l1::B_PE2, g, acc);
                e1p = split8<0>(e1);
                mm16<1, 2, true>(lds + l1::PE2F, lane, &e1p, acc);
                e[0] = acc[0].x; e[1] = acc[0].y; e[2] = acc[0].z; e[3] = acc[0].w; e[4] = acc[1].x; e[5] = acc[1].y; e[6] = acc[1].z; e[7] = acc[1].w;
            }
            float d1t[4], dft[12], n1t[4];
            const float ddg[1] = {g == 0 ? vg.dd[0] : (g == 1 ? vg.dd[1] : (g == 2 ? vg.dd[2] : vg.dd[3]))};
            {
                f4 acc1[1], acc3[3];
                load_bias<1>(lds + l1::B_RDF1, g, acc1);
                mm<1, 1>(lds + l1::RDF1, lane, ddg, acc1);
                elu_to<1>(acc1, d1t);
                load_bias<3>(lds + l1::B_RDF2, g, acc3);
                mm<4, 3>(lds + l1::RDF2, lane, d1t, acc3);
                elu_to<3>(acc3, dft);
                load_bias<1>(lds + l1::B_NR1, g, acc1);
                mm16<1, 1, true>(lds + l1::NR1, lane, &e1p, acc1);
                elu_to<1, false>(acc1, n1t);
            }
            const float gate = sigmoid1(gsum(dot4(lds + l1::T_NR2, g, n1t)) + lds[l1::SC + 0]);
            // ---- upstream, normalised by a power of two (grad_scale): gs in, gi = 1 / gs back out wherever values leave the chain
            float dX[9], de[8];
            const float* dsp = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
#pragma unroll
            for (int j = 0; j < 9; ++j) dX[j] = dsp[j * 64];
#pragma unroll
            for (int j = 0; j < 8; ++j) de[j] = dsp[(9 + j) * 64];
            float dgate = dsp[17 * 64];
            float gs, gi;
            {
                float am = fabsf(dgate);
#pragma unroll
                for (int j = 0; j < 9; ++j) am = fmaxf(am, fabsf(dX[j]));
#pragma unroll
                for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(de[j]));
                unsigned ambits = 0u;
                grad_scale(am, gs, gi, &ambits);
                if constexpr (BINS) { if (a.sc.upmax && lane == 0 && ambits != 0u) atomicMax(a.sc.upmax, ambits); }
#pragma unroll
                for (int j = 0; j < 9; ++j) dX[j] *= gs;
#pragma unroll
                for (int j = 0; j < 8; ++j) de[j] *= gs;
                dgate *= gs;
            }
            // ---- stage R2: ray_dir_fc.2   dY = da9 (x layout: column = canonical output index) | X = ELU output of ray_dir_fc.0
            float da9[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) da9[j] = dX[j] * elu_grad_t(dft[j]);
            {
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
#pragma unroll
                for (int j = 0; j < 8; ++j) Ta[r * l1p::TSP + 3 + 8 * g + j] = da9[j] * gi;
                if (g < 3) Ta[r * l1p::TSP + g] = da9[8] * gi;
                if (g == 3) {
#pragma unroll
                    for (int c = 35; c < 48; ++c) Ta[r * l1p::TSP + c] = 0.f;
                }
                pw_put_nat<1>(Tb, r, g, d1t, kLn2);
                ring.publish(ST1_STAGE);
            }
            f4 acc1[1] = {f4{0.f, 0.f, 0.f, 0.f}};
            mm<9, 1>(lds + l1::RDF2T, lane, da9, acc1);
            // ---- stage R1: ray_dir_fc.0   dY = da4 | X = dir diff (4 columns, the rest of the block zero)
            {
                const float da4[4] = {acc1[0].x * elu_grad_t(d1t[0]), acc1[0].y * elu_grad_t(d1t[1]), acc1[0].z * elu_grad_t(d1t[2]), acc1[0].w * elu_grad_t(d1t[3])};
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                pw_put_nat<1>(Ta, r, g, da4, gi);
                Tb[r * l1p::TSP + g] = ddg[0];
                Tb[r * l1p::TSP + 4 + 3 * g] = 0.f; Tb[r * l1p::TSP + 5 + 3 * g] = 0.f; Tb[r * l1p::TSP + 6 + 3 * g] = 0.f;
                ring.publish(ST1_STAGE);
            }
            // ---- neuray gate: stages NR2 (row: dY = dz in column 0 | X = ELU output of neuray_fc.0) and NR0 (dY = da4 | X = e)
            {
                const float dz = dgate * gate * (1.f - gate);
                float da4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) da4[j] = lds[l1::T_NR2 + g * 4 + j] * kLog2e * dz * elu_grad_t(n1t[j]);
                {
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    *reinterpret_cast<f4*>(Ta + r * l1p::TSP + 4 * g) = f4{0.f, g == 3 ? dz * gi : 0.f, 0.f, 0.f};            // column NR2_ROW = 13
                    pw_put_nat<1>(Tb, r, g, n1t, kLn2);
                    ring.publish(ST1_STAGE);
                }
                {
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    pw_put_nat<1>(Ta, r, g, da4, gi);
                    pw_put_nat<2>(Tb, r, g, e, 1.f);
                    ring.publish(ST1_STAGE);
                }
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                mm<4, 2>(lds + l1::NR0T, lane, da4, acc);
                de[0] += acc[0].x; de[1] += acc[0].y; de[2] += acc[0].z; de[3] += acc[0].w;
                de[4] += acc[1].x; de[5] += acc[1].y; de[6] += acc[1].z; de[7] += acc[1].w;
            }
            // ---- prob_embed.2 (stage PE2: dY = de | X = e1) and prob_embed.0 (stage PE0: dY = da | X = [ray features, hit', vis'])
            float dFR[8], dhit, dvis;
            {
                {
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    pw_put_nat<2>(Ta, r, g, de, gi);
                    pw_put_nat<2>(Tb, r, g, e1, 1.f);
                    ring.publish(ST1_STAGE);
                }
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                mm16g<1, 2>(lds + l1::PE2T, lane, de, acc);
                float da[8] = {acc[0].x, acc[0].y, acc[0].z, acc[0].w, acc[1].x, acc[1].y, acc[1].z, acc[1].w};
                float sh = 0.f, sv = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    da[j] = e1[j] > 0.f ? da[j] : 0.f;                      // ReLU'
                    sh = fmaf(lds[l1::T_PE0HV + g * 8 + j], da[j], sh);
                    sv = fmaf(lds[l1::T_PE0HV + 32 + g * 8 + j], da[j], sv);
                }
                dhit = 2.f * gsum(sh); dvis = 2.f * gsum(sv);
                {
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    pw_put_nat<2>(Ta, r, g, da, gi);
                    *reinterpret_cast<f4*>(Tb + r * l1p::TSP + 8 * g) = f4{FR[0], FR[1], FR[2], FR[3]};
                    *reinterpret_cast<f4*>(Tb + r * l1p::TSP + 8 * g + 4) = f4{FR[4], FR[5], FR[6], FR[7]};
                    if (g == 0) { Tb[r * l1p::TSP + 32] = hitp; Tb[r * l1p::TSP + 33] = visp; }
                    if (g == 1) {
#pragma unroll
                        for (int c = 34; c < 48; ++c) Tb[r * l1p::TSP + c] = 0.f;
                    }
                    ring.publish(ST1_STAGE);
                }
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                mm16g<1, 2>(lds + l1::PE0T, lane, da, acc);
                dFR[0] = acc[0].x; dFR[1] = acc[0].y; dFR[2] = acc[0].z; dFR[3] = acc[0].w;
                dFR[4] = acc[1].x; dFR[5] = acc[1].y; dFR[6] = acc[1].z; dFR[7] = acc[1].w;
            }
            // ---- hit / vis -> decoder outputs (dist_decoder.py:109-142)
            float do5[5];
            {
                const float daw = m * (dvis * ((1.f - r00) - (1.f - r01)) + dhit * ((r10 - r00) - (r11 - r01)));
                const float dc00 = m * aw * (-dvis - dhit), dc01 = m * (1.f - aw) * (-dvis - dhit);
                const float dc10 = m * aw * dhit, dc11 = m * (1.f - aw) * dhit;
                const float du00 = dc00 * 2.f * r00 * (1.f - r00), du01 = dc01 * 2.f * r01 * (1.f - r01);
                const float du10 = dc10 * 2.f * r10 * (1.f - r10), du11 = dc11 * 2.f * r11 * (1.f - r11);
                const float dmean0 = -var0 * (du00 + du10), dmean1 = -var1 * (du01 + du11);
                const float dvar0 = (nearv - mean0) * du00 + (farv - mean0) * du10, dvar1 = (nearv - mean1) * du01 + (farv - mean1) * du11;
                do5[0] = dmean0 * sigmoid1(o5[0]); do5[1] = dmean1 * sigmoid1(o5[1]);
                do5[2] = dvar0 * sigmoid1(o5[2]); do5[3] = dvar1 * sigmoid1(o5[3]);
                do5[4] = daw * aw * (1.f - aw);
            }
#pragma unroll
            for (int br = 0; br < 3; ++br) {
                const int r0 = 2 * br, nrow = br < 2 ? 2 : 1;
                float da2[8], da1[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float dh = 0.f;
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        if (q < nrow) dh = fmaf(lds[l1::T_DEC3 + (r0 + q) * 32 + g * 8 + j] * kLog2e, do5[r0 + q], dh);
                    da2[j] = dh * elu_grad_t(h2[br][j]);
                }
                {   // stage W3[br]: the last layer's rows   dY = d o5 (columns 0 (, 1)) | X = h2
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    // columns W3_ROW0 + 2 br (, + 1) = 8 + r0 (, 9 + r0): lane group 2 holds columns 8..11, group 3 column 12
                    *reinterpret_cast<f4*>(Ta + r * l1p::TSP + 4 * g) = f4{(br == 0 && g == 2) || (br == 2 && g == 3) ? do5[r0] * gi : 0.f, (br == 0 && g == 2) ? do5[br < 2 ? r0 + 1 : r0] * gi : 0.f,
                                                                      (br == 1 && g == 2) ? do5[r0] * gi : 0.f, (br == 1 && g == 2) ? do5[br < 2 ? r0 + 1 : r0] * gi : 0.f};
                    pw_put_nat<2>(Tb, r, g, h2[br], kLn2);
                    ring.publish(ST1_STAGE);
                }
                {   // stage D2[br]: dY = da2 | X = h1
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    pw_put_nat<2>(Ta, r, g, da2, gi);
                    pw_put_nat<2>(Tb, r, g, h1[br], kLn2);
                    ring.publish(ST1_STAGE);
                }
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                mm16g<1, 2>(lds + l1::DEC2T + br * 1024, lane, da2, acc);
                const float dh1[8] = {acc[0].x, acc[0].y, acc[0].z, acc[0].w, acc[1].x, acc[1].y, acc[1].z, acc[1].w};
#pragma unroll
                for (int j = 0; j < 8; ++j) da1[j] = dh1[j] * elu_grad_t(h1[br][j]);
                {   // stage D1[br]: dY = da1 | X = ray features
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    pw_put_nat<2>(Ta, r, g, da1, gi);
                    *reinterpret_cast<f4*>(Tb + r * l1p::TSP + 8 * g) = f4{FR[0], FR[1], FR[2], FR[3]};
                    *reinterpret_cast<f4*>(Tb + r * l1p::TSP + 8 * g + 4) = f4{FR[4], FR[5], FR[6], FR[7]};
                    ring.publish(ST1_STAGE);
                }
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                mm16g<1, 2>(lds + l1::DEC1T + br * 1024, lane, da1, acc);
                dFR[0] += acc[0].x; dFR[1] += acc[0].y; dFR[2] += acc[0].z; dFR[3] += acc[0].w;
                dFR[4] += acc[1].x; dFR[5] += acc[1].y; dFR[6] += acc[1].z; dFR[7] += acc[1].w;
            }
            // ---- scatter stage: rows [16][64] (ray channels 8g + j <- dFR, image-feature channels 32 + 8g + j <- d x), tap records [16][8]
            if constexpr (BINS) {
                // binned scatter (gnr_bwd_scatter.inc): this lane's 16 values of point r go to HBM as they sit in the registers -- row
                // position 16 g + j = ray channel 8 g + j (j < 8) / image channel 32 + 8 g + (j - 8): scatter_channel() -- with one
                // record per row (bin key, the four tap weights), and the row is counted into its bin
                const size_t row = ((size_t)tile * V + v) * 16 + r;
                f4* dst = reinterpret_cast<f4*>(a.sc.rows + row * 64 + 16 * g);
                dst[0] = f4{dFR[0] * gi, dFR[1] * gi, dFR[2] * gi, dFR[3] * gi};
                dst[1] = f4{dFR[4] * gi, dFR[5] * gi, dFR[6] * gi, dFR[7] * gi};
                dst[2] = f4{dX[0] * gi, dX[1] * gi, dX[2] * gi, dX[3] * gi};
                dst[3] = f4{dX[4] * gi, dX[5] * gi, dX[6] * gi, dX[7] * gi};
                if (g == 0) {
                    const bool live = row_ok && m != 0.f;
                    const int key = live ? bv * (a.fh * a.fw) + t.o00 : -1;
                    a.sc.key[row] = key;
                    a.sc.wts[row] = f4{w00, w01, w10, w11};
                    if (live) atomicAdd(&a.sc.cnt[key], 1);
                }
            } else {
                float* S = ring.acquire_free();
                *reinterpret_cast<f4*>(S + r * 64 + 8 * g) = f4{dFR[0] * gi, dFR[1] * gi, dFR[2] * gi, dFR[3] * gi};
                *reinterpret_cast<f4*>(S + r * 64 + 8 * g + 4) = f4{dFR[4] * gi, dFR[5] * gi, dFR[6] * gi, dFR[7] * gi};
                *reinterpret_cast<f4*>(S + r * 64 + 32 + 8 * g) = f4{dX[0] * gi, dX[1] * gi, dX[2] * gi, dX[3] * gi};
                *reinterpret_cast<f4*>(S + r * 64 + 32 + 8 * g + 4) = f4{dX[4] * gi, dX[5] * gi, dX[6] * gi, dX[7] * gi};
                if (g == 0) {
                    const bool live = row_ok && m != 0.f;
                    float* tp = S + 16 * 64 + r * 8;
                    *reinterpret_cast<f4*>(tp) = f4{live ? w00 : 0.f, live ? w01 : 0.f, live ? w10 : 0.f, live ? w11 : 0.f};
                    int* ip = reinterpret_cast<int*>(tp + 4);
                    ip[0] = t.o00; ip[1] = t.o01; ip[2] = t.o10; ip[3] = t.o11;
                    if (r == 0) reinterpret_cast<int*>(S + 16 * 64)[16 * 8] = bv;
                }
                ring.publish(ST1_STAGE);
            }
        }
    }
    ring.acquire_free();
    ring.publish(ST1_END);
}

}  // namespace gnr
