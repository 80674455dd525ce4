// k_view2_bwd_pw<RENDER>: the second view loop's backward with PARTNER WAVEFRONTS (round 5; included by gnr_bwd.inc behind
// gnr_bwd_view1_pw.inc, whose ring / slot / outer-product helpers it uses -- see there for the scheme).
//   compute wavefront c (0..3): forward recompute of base_fc / vis_fc / vis_fc2 (/ rgb_fc) on the C16 image and the dX chain on
//       the pair images pkb::P2_* -- k_view2_bwd's code without a weight-gradient accumulator; it writes d S1 and d G itself;
//   partner wavefront 4 + c: the outer products (44 accumulator blocks; 49 with the colour head), bias sums as column sums, the
//       single-row layers (vis_fc2.2, rgb_fc.4) as one-row stages, row 32 of vis_fc.2 as a 33rd column of vis_fc.2's dY tile.
// Tiles are 16 x 48: base_fc.2's 64 input columns and base_fc.0's 64 output columns are posted as two stages each.
// Both instantiations run on pairs here: without the accumulators the render instantiation's compute role has the registers
// the single-wavefront kernel lacked (k_view2_bwd<true> spilled 576 B with pair operands and stays on the fp32-input MFMA).
namespace gnr {

namespace l3p {
constexpr int RGB1 = l3::TILES, RGB2 = RGB1 + frag_floats(10, 1), B_RGB1 = RGB2 + frag_floats(4, 1), B_RGB2 = B_RGB1 + 16, T_RGB3 = B_RGB2 + 16,
              RGB2T = T_RGB3 + 16, RGB0HT = RGB2T + frag_floats(4, 1), T_RGB0V = RGB0HT + frag_floats(4, 2), RGB_END = T_RGB0V + 16;
constexpr int nslot(bool render) { return render ? 2 : 3; }                     // the colour head's fragments take a slot's room per pair
constexpr int ring(bool render) { return render ? RGB_END : l3::TILES; }
constexpr int flags(bool render) { return ring(render) + 4 * nslot(render) * l1p::SLOT; }
constexpr int total(bool render) { return flags(render) + 4 * 8; }
static_assert(total(false) * 4 <= 160 * 1024 && total(true) * 4 <= 160 * 1024, "k_view2_bwd_pw: LDS");
}

template <bool RENDER>
__global__ __launch_bounds__(512, 2) void k_view2_bwd_pw(View2BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (bwd_guard_skip(a.guard)) return;
    constexpr int NS = l3p::nslot(RENDER);
    // k-steps of an outer product in flight (partner side).  Volume instantiation: 4 (1.67 against 1.72 ms per launch, 12 B of prologue scratch);
    // the render instantiation spills 184 B at 4 and keeps 2
    constexpr int UO = RENDER ? l1p::OUTER_UNROLL : 4;
    for (int i = threadIdx.x; i < l3::BI; i += 512) lds[i] = a.wpk[pk::C16 + pk::c16_off(pk::BASE1) + i];
    if (threadIdx.x < 128) lds[l3::BI + threadIdx.x] = a.wpk[pk::B_BASE2 + threadIdx.x];
    if (threadIdx.x < 64) lds[l3::TB + threadIdx.x] = a.wpk[pk::T_VIS2R + threadIdx.x];
    if (threadIdx.x < 4) lds[l3::SC + threadIdx.x] = a.wpk[pk::T_SCAL + threadIdx.x];
    for (int i = threadIdx.x; i < pkb::P2_BASE1ET - pkb::P2_BEGIN; i += 512) lds[l3::BW + i] = a.wbk[pkb::P2_BEGIN + i];
    for (int i = threadIdx.x; i < pkb::P2_END - pkb::P2_BASE1ET; i += 512) lds[l3::BASE1ET + i] = a.wbk[pkb::P2_BASE1ET + i];
    if constexpr (RENDER) {
        for (int i = threadIdx.x; i < frag_floats(10, 1) + frag_floats(4, 1); i += 512) lds[l3p::RGB1 + i] = a.wpk[pk::RGB1 + i];
        if (threadIdx.x < 32) lds[l3p::B_RGB1 + threadIdx.x] = a.wpk[pk::B_RGB1 + threadIdx.x];
        if (threadIdx.x < 16) lds[l3p::T_RGB3 + threadIdx.x] = a.wpk[pk::T_RGB3 + threadIdx.x];
        for (int i = threadIdx.x; i < l3p::RGB_END - l3p::RGB2T; i += 512) lds[l3p::RGB2T + i] = a.wbk[pkb::RGB2T + i];
    }
    if (threadIdx.x < 32) reinterpret_cast<int*>(lds + l3p::flags(RENDER))[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), pair = wave & 3;
    const bool partner = wave >= 4;
    PwRingN<NS> ring;
    ring.slots = lds + l3p::ring(RENDER) + pair * NS * l1p::SLOT;
    {
        int* f = reinterpret_cast<int*>(lds + l3p::flags(RENDER)) + pair * 8;
        ring.produced = f; ring.consumed = f + 1; ring.kind = f + 2; ring.dead = f + 6; ring.seq = 0;
        ring.status = a.guard.status;
    }
    const int V = a.V;
    if (partner && a.guard.lose_partner) return;                   // GNR_OPT_TEST_LOSE_PARTNER

    if (partner) {
        // =========================== partner wavefront ===========================
        f4 gWvb2[2], gWvb1[4], gWv2[6], gWv1[4], gWb2a[4], gWb2b[4], gWxl[6], gWxh[6], gWel[4], gWeh[4], gWc4[1], gWc2[1], gWc0[3];
        float bvb2[1] = {0.f}, bvb1[2] = {0.f, 0.f}, bv2[3] = {0.f, 0.f, 0.f}, bv1[2] = {0.f, 0.f}, bb2[2] = {0.f, 0.f}, bb2x[2] = {0.f, 0.f};
        float b0l[2] = {0.f, 0.f}, b0h[2] = {0.f, 0.f}, b0x[2] = {0.f, 0.f}, bc4[1] = {0.f}, bc2[1] = {0.f}, bc0[1] = {0.f};
        const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
        gWvb2[0] = z4; gWvb2[1] = z4; gWc4[0] = z4; gWc2[0] = z4; gWc0[0] = z4; gWc0[1] = z4; gWc0[2] = z4;
#pragma unroll
        for (int q = 0; q < 4; ++q) { gWvb1[q] = z4; gWv1[q] = z4; gWb2a[q] = z4; gWb2b[q] = z4; gWel[q] = z4; gWeh[q] = z4; }
#pragma unroll
        for (int q = 0; q < 6; ++q) { gWv2[q] = z4; gWxl[q] = z4; gWxh[q] = z4; }
        // one trip = the stages of one (tile, view); a skipped pair publishes nothing, the end of the tile list ST1_END (k_view1_bwd_pw)
        {
            for (;;) {
                int k;
                const float* s = ring.acquire_full(k);
                if (k == ST1_END || pw_load(ring.dead)) break;
                if constexpr (RENDER) {
                    pw_outer<1, 1, UO>(s, lane, gWc4, bc4); ring.release();
                    s = ring.acquire_full(k); pw_outer<1, 1, UO>(s, lane, gWc2, bc2); ring.release();
                    s = ring.acquire_full(k); pw_outer<1, 3, UO>(s, lane, gWc0, bc0); ring.release();
                    s = ring.acquire_full(k);
                }
                pw_outer<1, 2, UO>(s, lane, gWvb2, bvb2); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 2, UO>(s, lane, gWvb1, bvb1); ring.release();
                s = ring.acquire_full(k); pw_outer<3, 2, UO>(s, lane, gWv2, bv2); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 2, UO>(s, lane, gWv1, bv1); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 2, UO>(s, lane, gWb2a, bb2); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 2, UO>(s, lane, gWb2b, bb2x); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 3, UO>(s, lane, gWxl, b0l); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 3, UO>(s, lane, gWxh, b0h); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 2, UO>(s, lane, gWel, b0x); ring.release();
                s = ring.acquire_full(k); pw_outer<2, 2, UO>(s, lane, gWeh, b0x); ring.release();
            }
        }
        float* gc = a.dpart + (size_t)(blockIdx.x * 4 + pair) * GP_STRIDE;
        flush_blocks<2, 3>(gc + can::BASE0_W + 140, 207, 32, 35, lane, gWxl);
        flush_blocks<2, 3>(gc + can::BASE0_W + 32 * 207 + 140, 207, 32, 35, lane, gWxh);
        flush_blocks<2, 2>(gc + can::BASE0_W + 175, 207, 32, 32, lane, gWel);
        flush_blocks<2, 2>(gc + can::BASE0_W + 32 * 207 + 175, 207, 32, 32, lane, gWeh);
        pw_flush_bias<2>(gc + can::BASE0_B, 32, lane, b0l);
        pw_flush_bias<2>(gc + can::BASE0_B + 32, 32, lane, b0h);
        flush_blocks<2, 2>(gc + can::BASE2_W, 64, 32, 32, lane, gWb2a);
        flush_blocks<2, 2>(gc + can::BASE2_W + 32, 64, 32, 32, lane, gWb2b);
        pw_flush_bias<2>(gc + can::BASE2_B, 32, lane, bb2);
        flush_blocks<2, 2>(gc + can::VIS0_W, 32, 32, 32, lane, gWv1);
        pw_flush_bias<2>(gc + can::VIS0_B, 32, lane, bv1);
        flush_blocks<3, 2>(gc + can::VIS2_W, 32, 33, 32, lane, gWv2);               // rows 0..31 + the visibility row 32
        pw_flush_bias<3>(gc + can::VIS2_B, 33, lane, bv2);
        flush_blocks<2, 2>(gc + can::VISB0_W, 32, 32, 32, lane, gWvb1);
        pw_flush_bias<2>(gc + can::VISB0_B, 32, lane, bvb1);
        flush_blocks<1, 2>(gc + can::VISB2_W, 32, 1, 32, lane, gWvb2);
        pw_flush_bias<1>(gc + can::VISB2_B, 1, lane, bvb2);
        if constexpr (RENDER) {
            flush_blocks<1, 3>(gc + can::RGB0_W, 37, 16, 37, lane, gWc0);
            pw_flush_bias<1>(gc + can::RGB0_B, 16, lane, bc0);
            flush_blocks<1, 1>(gc + can::RGB2_W, 16, 8, 16, lane, gWc2);
            pw_flush_bias<1>(gc + can::RGB2_B, 8, lane, bc2);
            flush_blocks<1, 1>(gc + can::RGB4_W, 8, 1, 8, lane, gWc4);
            pw_flush_bias<1>(gc + can::RGB4_B, 1, lane, bc4);
        }
        return;
    }

    // =========================== compute wavefront ===========================
    for (int tile = blockIdx.x * 4 + pair; tile < a.ntiles; tile += gridDim.x * 4) {
        f4 G[4];
        float inv_msum;
        {
            const float* sp = a.saveG + (size_t)tile * 17 * 64 + lane;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) G[nb] = f4{sp[(4 * nb) * 64], sp[(4 * nb + 1) * 64], sp[(4 * nb + 2) * 64], sp[(4 * nb + 3) * 64]};
            inv_msum = sp[16 * 64];
        }
        float dGacc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) dGacc[j] = 0.f;
        float pp3[3] = {0.f, 0.f, 0.f}, qd3[3] = {0.f, 0.f, 0.f};
        int bscene = 0;
        if constexpr (RENDER) {
            const int tps = (a.P + 15) >> 4;
            bscene = tile / tps;
            const int n = min((tile - bscene * tps) * 16 + r, a.P - 1);
            const size_t pt = (size_t)bscene * a.P + n;
            const f4 d0 = reinterpret_cast<const f4*>(a.desc)[pt * 2], d1 = reinterpret_cast<const f4*>(a.desc)[pt * 2 + 1];
            pp3[0] = d0.x; pp3[1] = d0.y; pp3[2] = d0.z; qd3[0] = d0.w; qd3[1] = d1.x; qd3[2] = d1.y;
        }
#pragma unroll 1
        for (int v = 0; v < V; ++v) {
            asm volatile("" ::: "memory");
            float X[9], E1[8], dH[8];
            const float* s1 = a.save1 + ((size_t)tile * V + v) * 19 * 64 + lane;
#pragma unroll
            for (int j = 0; j < 9; ++j) X[j] = s1[j * 64];
#pragma unroll
            for (int j = 0; j < 8; ++j) E1[j] = s1[(9 + j) * 64];
            const float m = s1[18 * 64];
            if constexpr (RENDER) {                                             // nothing flows through a view that no sample of the tile sees
                if (__ballot(m != 0.f) == 0ull) {
                    float* o1 = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
#pragma unroll
                    for (int j = 0; j < 17; ++j) o1[j * 64] = 0.f;              // (entry 17, d gate, is k_hoist_bwd's: it stores it for every pair)
                    continue;                                                   // (nothing is published: the partner follows the stages, not the pairs)
                }
            }
            constexpr int D2W = RENDER ? 10 : 9;
            const float* d2 = a.dS2 + ((size_t)tile * V + v) * D2W * 64 + lane;
#pragma unroll
            for (int j = 0; j < 8; ++j) dH[j] = d2[j * 64];
            float dv2 = d2[8 * 64];
            float gs, gi;
            float dclog = 0.f;
            if constexpr (RENDER) dclog = (m != 0.f) ? d2[9 * 64] : 0.f;
            {
                float am = fabsf(dv2);
#pragma unroll
                for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(dH[j]));
                if constexpr (RENDER) am = fmaxf(am, fabsf(dclog));
                grad_scale(am, gs, gi);
#pragma unroll
                for (int j = 0; j < 8; ++j) dH[j] *= gs;
                dv2 *= gs; dclog *= gs;
            }
            // ---- forward recompute of this view (the forward kernel's instruction sequence on the C16 image)
            const float w = m * inv_msum;
            float b1t[16], H0t[8], v1t[8], rest[8], Ht[8], t1t[8], xin[8], xin2[8], e[8];
            f4 acc4[4] = {G[0], G[1], G[2], G[3]}, acc[2];
            {
                const float x8[1] = {X[8]};
                mm<1, 4, 0>(lds + l3::BASE1 + 2 * pk::k32_floats(4), lane, x8, acc4);
                const P8 xe[2] = {split8<0>(X), split8<0>(E1)};
                mm16<2, 4, true>(lds + l3::BASE1, lane, xe, acc4);
                elu_to<4, false>(acc4, b1t);
                load_bias<2>(lds + l3::BI + 0, g, acc);
                { const P8U bp[2] = {split8u<0>(b1t), split8u<8>(b1t)}; mm16u<2, 2, true>(lds + l3::BASE2, lane, bp, acc); }
                elu_to<2>(acc, H0t);
#pragma unroll
                for (int j = 0; j < 8; ++j) xin[j] = H0t[j] * w;
                load_bias<2>(lds + l3::BI + 32, g, acc);
                { const P8U xp = split8u<0>(xin); mm16u<1, 2, true>(lds + l3::VIS1, lane, &xp, acc); }
                elu_to<2>(acc, v1t);
                load_bias<2>(lds + l3::BI + 64, g, acc);
                { const P8U vp8 = split8u<0>(v1t); mm16u<1, 2, true>(lds + l3::VIS2, lane, &vp8, acc); }
                elu_to<2>(acc, rest);
                load_bias<2>(lds + l3::B_PE2, g, acc);
                mm16<1, 2, true>(lds + l3::PE2F, lane, &xe[1], acc);
                e[0] = acc[0].x; e[1] = acc[0].y; e[2] = acc[0].z; e[3] = acc[0].w; e[4] = acc[1].x; e[5] = acc[1].y; e[6] = acc[1].z; e[7] = acc[1].w;
            }
            const float a_r = gsum(dot8(lds + l3::TB, g, v1t)) + lds[l3::SC + 1];
            const float logit = elu1(a_r), sg = sigmoid1(logit), vis1 = sg * m;
#pragma unroll
            for (int j = 0; j < 8; ++j) { Ht[j] = H0t[j] + rest[j]; xin2[j] = Ht[j] * vis1; }
            load_bias<2>(lds + l3::BI + 96, g, acc);
            { const P8U xp = split8u<0>(xin2); mm16u<1, 2, true>(lds + l3::VISB1, lane, &xp, acc); }
            elu_to<2>(acc, t1t);
            const float v2 = sigmoid1(gsum(dot8(lds + l3::TB + 32, g, t1t)) + lds[l3::SC + 2]) * m;
            // ---- colour head rgb_fc (ibrnet.py:506-509): stages C4 (row), C2, C0
            if constexpr (RENDER) {
                ViewGeom vg;
                project_view<true>(a.viewp + (bscene * V + v) * VIEWP_FLOATS, pp3, qd3, a.H, a.W, vg);
                f4 acc1[1];
                float c1t[4], c2t[4];
                load_bias<1>(lds + l3p::B_RGB1, g, acc1);
                mm<8, 1>(lds + l3p::RGB1, lane, Ht, acc1);
                const float ex[2] = {g == 0 ? v2 : (g == 1 ? vg.dd[0] : (g == 2 ? vg.dd[1] : vg.dd[2])), g == 0 ? vg.dd[3] : 0.f};
                mm<2, 1, 8>(lds + l3p::RGB1, lane, ex, acc1);
                elu_to<1>(acc1, c1t);
                load_bias<1>(lds + l3p::B_RGB2, g, acc1);
                mm<4, 1>(lds + l3p::RGB2, lane, c1t, acc1);
                elu_to<1>(acc1, c2t);
                float dc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) dc[j] = lds[l3p::T_RGB3 + g * 4 + j] * kLog2e * dclog * elu_grad_t(c2t[j]);
                {
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    *reinterpret_cast<f4*>(Ta + r * l1p::TSP + 4 * g) = f4{g == 0 ? dclog * gi : 0.f, 0.f, 0.f, 0.f};
                    pw_put_nat<1>(Tb, r, g, c2t, kLn2);
                    ring.publish(ST1_STAGE);
                }
                {
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    pw_put_nat<1>(Ta, r, g, dc, gi);
                    pw_put_nat<1>(Tb, r, g, c1t, kLn2);
                    ring.publish(ST1_STAGE);
                }
                acc1[0] = f4{0.f, 0.f, 0.f, 0.f};
                mm<4, 1>(lds + l3p::RGB2T, lane, dc, acc1);
                dc[0] = acc1[0].x * elu_grad_t(c1t[0]); dc[1] = acc1[0].y * elu_grad_t(c1t[1]);
                dc[2] = acc1[0].z * elu_grad_t(c1t[2]); dc[3] = acc1[0].w * elu_grad_t(c1t[3]);
                float sv = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) sv = fmaf(lds[l3p::T_RGB0V + g * 4 + j], dc[j], sv);
                dv2 += gsum(sv);
                {
                    float* S = ring.acquire_free();
                    float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                    pw_put_nat<1>(Ta, r, g, dc, gi);
                    pw_put_nat<2>(Tb, r, g, Ht, kLn2);
                    if (g == 0) { Tb[r * l1p::TSP + 32] = v2; Tb[r * l1p::TSP + 36] = vg.dd[3]; }
                    else Tb[r * l1p::TSP + 32 + g] = ex[0];
                    if (g == 1) {
#pragma unroll
                        for (int c = 37; c < 48; ++c) Tb[r * l1p::TSP + c] = 0.f;
                    }
                    ring.publish(ST1_STAGE);
                }
                f4 acc2[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
                mm<4, 2>(lds + l3p::RGB0HT, lane, dc, acc2);
                dH[0] += acc2[0].x; dH[1] += acc2[0].y; dH[2] += acc2[0].z; dH[3] += acc2[0].w;
                dH[4] += acc2[1].x; dH[5] += acc2[1].y; dH[6] += acc2[1].z; dH[7] += acc2[1].w;
            }
            // ---- vis_fc2: stages VB2 (row), VB1
            const float da_b2 = dv2 * v2 * (1.f - v2);
            float da[8], dx[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) da[j] = lds[l3::TB + 32 + g * 8 + j] * kLog2e * da_b2 * elu_grad_t(t1t[j]);
            {
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                *reinterpret_cast<f4*>(Ta + r * l1p::TSP + 4 * g) = f4{g == 0 ? da_b2 * gi : 0.f, 0.f, 0.f, 0.f};
                pw_put_nat<2>(Tb, r, g, t1t, kLn2);
                ring.publish(ST1_STAGE);
            }
            {
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                pw_put_nat<2>(Ta, r, g, da, gi);
                pw_put_nat<2>(Tb, r, g, xin2, kLn2);
                ring.publish(ST1_STAGE);
            }
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            mm16g<1, 2>(lds + l3::VISB1T, lane, da, acc);
            dx[0] = acc[0].x; dx[1] = acc[0].y; dx[2] = acc[0].z; dx[3] = acc[0].w; dx[4] = acc[1].x; dx[5] = acc[1].y; dx[6] = acc[1].z; dx[7] = acc[1].w;
            float dvis1 = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { dvis1 = fmaf(dx[j], Ht[j] * kLn2, dvis1); dH[j] = fmaf(dx[j], vis1, dH[j]); }
            dvis1 = gsum(dvis1);
            // ---- vis_fc.2: stage V2   dY = [d a (32 residual rows) | d a_r (the visibility row) in column 32] | X = v1
            const float da_r = dvis1 * m * sg * (1.f - sg) * (a_r > 0.f ? 1.f : logit + 1.f);
#pragma unroll
            for (int j = 0; j < 8; ++j) da[j] = dH[j] * elu_grad_t(rest[j]);
            {
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                pw_put_nat<2>(Ta, r, g, da, gi);
                *reinterpret_cast<f4*>(Ta + r * l1p::TSP + 32 + 4 * g) = f4{g == 0 ? da_r * gi : 0.f, 0.f, 0.f, 0.f};
                pw_put_nat<2>(Tb, r, g, v1t, kLn2);
                ring.publish(ST1_STAGE);
            }
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            mm16g<1, 2>(lds + l3::VIS2T, lane, da, acc);
            dx[0] = acc[0].x; dx[1] = acc[0].y; dx[2] = acc[0].z; dx[3] = acc[0].w; dx[4] = acc[1].x; dx[5] = acc[1].y; dx[6] = acc[1].z; dx[7] = acc[1].w;
            // ---- vis_fc.0: stage V1
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dv1 = fmaf(lds[l3::TB + g * 8 + j] * kLog2e, da_r, dx[j]);
                da[j] = dv1 * elu_grad_t(v1t[j]);
            }
            {
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                pw_put_nat<2>(Ta, r, g, da, gi);
                pw_put_nat<2>(Tb, r, g, xin, kLn2);
                ring.publish(ST1_STAGE);
            }
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            mm16g<1, 2>(lds + l3::VIS1T, lane, da, acc);
            dx[0] = acc[0].x; dx[1] = acc[0].y; dx[2] = acc[0].z; dx[3] = acc[0].w; dx[4] = acc[1].x; dx[5] = acc[1].y; dx[6] = acc[1].z; dx[7] = acc[1].w;
            // ---- base_fc.2: stages B2a / B2b (its 64 input columns in two halves)
#pragma unroll
            for (int j = 0; j < 8; ++j) da[j] = fmaf(dx[j], w, dH[j]) * elu_grad_t(H0t[j]);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                pw_put_nat<2>(Ta, r, g, da, gi);
                const float bh[8] = {b1t[8 * half], b1t[8 * half + 1], b1t[8 * half + 2], b1t[8 * half + 3], b1t[8 * half + 4], b1t[8 * half + 5], b1t[8 * half + 6], b1t[8 * half + 7]};
                pw_put_nat<2>(Tb, r, g, bh, kLn2);
                ring.publish(ST1_STAGE);
            }
            f4 d4[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) d4[nb] = f4{0.f, 0.f, 0.f, 0.f};
            mm16g<1, 4>(lds + l3::BASE2T, lane, da, d4);
            // ---- base_fc.0, per-view columns: stages (d a1 low | x), (d a1 high | x), (d a1 low | e), (d a1 high | e)
            float da1[16];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                da1[4 * nb] = d4[nb].x * elu_grad_t(b1t[4 * nb]); da1[4 * nb + 1] = d4[nb].y * elu_grad_t(b1t[4 * nb + 1]);
                da1[4 * nb + 2] = d4[nb].z * elu_grad_t(b1t[4 * nb + 2]); da1[4 * nb + 3] = d4[nb].w * elu_grad_t(b1t[4 * nb + 3]);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) dGacc[j] = fmaf(da1[j], gi, dGacc[j]);
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int half = st & 1;
                float* S = ring.acquire_free();
                float* Ta = S; float* Tb = S + 16 * l1p::TSP;
                const float dh[8] = {da1[8 * half], da1[8 * half + 1], da1[8 * half + 2], da1[8 * half + 3], da1[8 * half + 4], da1[8 * half + 5], da1[8 * half + 6], da1[8 * half + 7]};
                pw_put_nat<2>(Ta, r, g, dh, gi);
                if (st < 2) {
                    // x in canonical order [r g b | img feats]: slot j < 8 -> 3 + 8g + j, slot 8 -> colour channel g (g < 3)
#pragma unroll
                    for (int j = 0; j < 8; ++j) Tb[r * l1p::TSP + 3 + 8 * g + j] = X[j];
                    if (g < 3) Tb[r * l1p::TSP + g] = X[8];
                    if (g == 3) {
#pragma unroll
                        for (int c = 35; c < 48; ++c) Tb[r * l1p::TSP + c] = 0.f;
                    }
                } else {
                    pw_put_nat<2>(Tb, r, g, e, 1.f);
                }
                ring.publish(ST1_STAGE);
            }
            f4 d3[3];
            d3[0] = f4{0.f, 0.f, 0.f, 0.f}; d3[1] = d3[0]; d3[2] = d3[0];
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            mm16g<2, 3>(lds + l3::BASE1XT, lane, da1, d3);
            mm16g<2, 2>(lds + l3::BASE1ET, lane, da1, acc);
            float* o1 = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
            o1[0] = d3[0].x * gi; o1[64] = d3[0].y * gi; o1[128] = d3[0].z * gi; o1[192] = d3[0].w * gi;
            o1[256] = d3[1].x * gi; o1[320] = d3[1].y * gi; o1[384] = d3[1].z * gi; o1[448] = d3[1].w * gi;
            o1[512] = d3[2].x * gi;
            o1[9 * 64] = acc[0].x * gi; o1[10 * 64] = acc[0].y * gi; o1[11 * 64] = acc[0].z * gi; o1[12 * 64] = acc[0].w * gi;
            o1[13 * 64] = acc[1].x * gi; o1[14 * 64] = acc[1].y * gi; o1[15 * 64] = acc[1].z * gi; o1[16 * 64] = acc[1].w * gi;
        }
        float* og = a.dG + (size_t)tile * 16 * 64 + lane;
#pragma unroll
        for (int j = 0; j < 16; ++j) og[j * 64] = dGacc[j];
    }
    ring.acquire_free();
    ring.publish(ST1_END);
}

}  // namespace gnr
