// Backward twins of the volumetric path.  Included at the end of gnr_kernels.hip (shares its device helpers).
//
//   k_depth_mean_bwd                      backward of gnr_depth_mean_fwd (predict_mean_for_depth_loss, renderer.py:230-266)
//   k_ray_bwd, k_geo_bwd, k_view2_bwd,    the five stages of gnr_sample_volume_bwd (renderer.py:164-199 and everything it
//   k_hoist_bwd, k_view1_bwd              calls: dist_decoder.py:99-142, aggregate_net.py:35-70, ibrnet.py:447-495)
//   k_stats_unpack, k_red2_bwd            the per-view chain of a render pass (gnr_render_chain_fwd_train / _bwd)
//   (+ k_view2_bwd<true>, stages 2, 1)
//   k_ray_dual_bwd                        the per-ray tail of a render pass incl. the second-order path through the
//                                         in-forward SDF gradient (ibrnet.py:485-504): reverse pass on dual numbers
//   k_composite_bwd                       NeuS alpha + compositing (aggregate_net.py:105-121, render_ops.py:72-80)
//   k_unpack_feat_grad                    channel-last feature-map gradient -> NCHW
//
// Building blocks:
//  * dX = W^T dY runs on the same chained-MFMA tile as the forward: W^T is packed as A fragments (gnr_pack_weights_bwd),
//    dY sits in the activation (B operand) layout, so dX comes out in the activation layout of the previous layer.
//  * dW += dY X^T needs the point axis as K: both factors go through a [16 points][48] LDS tile per wavefront
//    (row stride 48 floats: the four k-groups of a k-step read disjoint banks) and come back as
//    A[row = feature][k = point], B[k = point][col = feature]; accumulators stay in registers across the wavefront's tiles
//    and are flushed once with atomics into the canonical (state-dict order) gradient blob.
//  * feature-map gradients are scattered with atomics into a channel-last [B*V][fh*fw][64] buffer (the layout the
//    forward gathers from) and converted to NCHW by k_unpack_feat_grad: float atomics by default (FX false), or -- bit-reproducible,
//    GNR_OPT_FEATURE_GRAD_FIXED -- as 64-bit integers in units of a launch-wide power-of-two quantum (FX true, FeatFx below).
namespace gnr {

// ---- bit-reproducible feature-map gradients (FX).  Float atomics add in arrival order, so the low bits of d_ray_feats /
// d_img_feats differ from run to run.  Integer adds commute: every contribution x is rounded ONCE to a multiple of the quantum
// q = 2^(e - 28), 2^e > max|upstream gradient of the launch| (an order-independent maximum over the launch's input gradient: k_absmax_bits),
// and added as a 64-bit integer.  Budget of the 63 value bits: 28 below the upstream maximum (precision), 14 above it (what the
// layers between the upstream gradient and the feature maps may amplify: |x| < 2^14 max, else the contribution is clamped and bit 3
// of gnr_range_status is raised), 20 for the number of contributions one feature-map entry can receive (4 taps x 64 000 points of
// a scene and view < 2^18), one spare.  Costs twice the atomic traffic of the float path (64-bit adds).
struct FeatFx { const unsigned* upmax; unsigned* flag; };       // bits of max|upstream| (k_absmax_bits), status word (bit 3 = clamped)
DEV int fx_exponent(unsigned bits) {                            // e with 2^e > max (max finite and > 0), clamped so that both scales are normal floats
    const float mx = __uint_as_float(bits);
    if (!(mx > 0.f) || !(mx < 3.0e38f)) return 0;
    int e;
    (void)frexpf(mx, &e);
    return max(min(e, 100), -90);
}
DEV float fx_scale(const FeatFx& f) { return ldexpf(1.f, 28 - fx_exponent(f.upmax[0])); }
// one contribution as a multiple of the quantum (scale = 1 / quantum, a power of two): clamped to the budget, rounded to nearest
DEV long long fx_quantise(float x, float scale, unsigned* __restrict__ flag) {
    float y = x * scale;                                        // (power of two: exact)
    if (!(fabsf(y) < 0x1p42f)) {                                // beyond the budget (or not finite): clamp, tell
        atomicOr(flag, 8u);
        y = (y != y) ? 0.f : copysignf(0x1p42f, y);
    }
    // round to nearest integer through the double's mantissa (|y| < 2^51): two instructions instead of a float -> int64 sequence
    return __double_as_longlong((double)y + 6755399441055744.0) - 0x4338000000000000LL;
}
template <bool FX>
DEV void feat_add(float* __restrict__ buf, size_t idx, float x, float scale, unsigned* __restrict__ flag) {
    if constexpr (!FX) {
        unsafeAtomicAdd(buf + idx, x);
    } else {
        atomicAdd(reinterpret_cast<unsigned long long*>(buf) + idx, (unsigned long long)fx_quantise(x, scale, flag));
    }
}
// bits of max |x| over a buffer (non-negative floats order like their bit patterns; NaN / inf land above every finite value and make
// fx_exponent fall back to 0).  *out zeroed by the caller.
// only_if: null, or the two status words of a backward range guard (BwdGuard, below): the pass runs only when they are flagged -- the
// binned view kernel collects the maximum itself and returns at once on a flagged pass, whose fp32 twin then needs this one
__global__ __launch_bounds__(256) void k_absmax_bits(const float* __restrict__ x, size_t n, unsigned* __restrict__ out, const unsigned* __restrict__ only_if0 = nullptr,
                                                     const unsigned* __restrict__ only_if1 = nullptr, const unsigned* __restrict__ only_if2 = nullptr) {
    if (only_if0) {
        const unsigned w = (__builtin_nontemporal_load(only_if0) & 5u) | (only_if1 ? __builtin_nontemporal_load(only_if1) & 2u : 0u) |
                           (only_if2 ? __builtin_nontemporal_load(only_if2) & 2u : 0u);
        if (w == 0u) return;
    }
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, __float_as_uint(x[i]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(out, m);
}

struct DepthMeanBwdArgs {
    const float* wpk; const float* wbk;          // forward / backward packed blobs of the level
    const float* feat64; const float* coords;    // as in the forward
    const float* dmean;                          // [B][V][pn][2] upstream gradient
    float* dfeat64;                              // [B*V][fh*fw][64] accumulated (ray channels 0..31 touched); FX: int64 entries
    float* dpart;                                // [wavefront slots][DM_STRIDE] partial mean_decoder gradients (k_grad_reduce sums them)
    int B, V, pn, H, W, fh, fw, ntiles;
    FeatFx fx;                                   // FX instantiation only
};


constexpr int TS = 48;                           // LDS tile row stride (floats)

// ---- deterministic parameter gradients: per-wavefront slots + fixed-order reduction ------------------------------
constexpr int GP_STRIDE = ((can::TOTAL_VIS + 63) / 64) * 64;     // slot of the view-chain / geometry kernels: canonical offsets
constexpr int DM_STRIDE = ((can::VAR0_W + 63) / 64) * 64;        // k_depth_mean_bwd: the mean_decoder's range [0, VAR0_W)
constexpr int GD_BASE = can::GEO0_W;                             // k_geo_dual_bwd_gemm: geometry_fc's range [GEO0_W, WQ), offsets - GD_BASE
constexpr int GD_STRIDE = ((can::WQ - can::GEO0_W + 63) / 64) * 64;
// per-ray tails (k_ray_bwd, k_ray_dual_bwd): dWq, dWk, dWv, dWfc [16][16] as floats, then 17 doubles:
// M[c] = sum ds * xhat_c (+ tangent part), S = sum ds.  LayerNorm / folded-output gradients follow from them (k_tail_finish).
namespace tp { constexpr int W = 0, MS = 1024, STRIDE = 1024 + 2 * 17 + 30; }
static_assert(tp::STRIDE % 2 == 0 && tp::MS % 2 == 0, "the doubles of a tail slot must be 8-byte aligned");

DEV int wave_slot() { return blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }
DEV float* grad_slot(float* part, int stride) { return part + (size_t)wave_slot() * stride; }

DEV double wave_sum64d(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// dst[dlo + i] += sum over slots (in slot order, double) of part[slot][lo + i], for up to four ranges
struct GradReduceArgs {
    const float* part; float* dst;
    int nslots, stride, nranges;
    int lo[4], hi[4], dlo[4];
};

__global__ __launch_bounds__(256) void k_grad_reduce(GradReduceArgs a) {
    __shared__ double sh[4][64];
    const int i = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int lin = blockIdx.x * 64 + i;
    int src = -1, dst = -1, base = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < a.nranges) {
            const int len = a.hi[k] - a.lo[k];
            if (src < 0 && lin < base + len) { src = a.lo[k] + (lin - base); dst = a.dlo[k] + (lin - base); }
            base += len;
        }
    }
    double s = 0.0;
    if (src >= 0) {
        const int per = (a.nslots + 3) >> 2, s0 = grp * per, s1 = min(a.nslots, s0 + per);
        const float* p = a.part + (size_t)s0 * a.stride + src;
#pragma unroll 8
        for (int t = s0; t < s1; ++t, p += a.stride) s += (double)*p;
    }
    sh[grp][i] = s;
    __syncthreads();
    if (grp == 0 && src >= 0) a.dst[dst] = (float)((double)a.dst[dst] + (((sh[0][i] + sh[1][i]) + sh[2][i]) + sh[3][i]));
}

// the tails' scalar sums: block c (16 blocks of 256 threads) adds M[c] and S over the slots in a fixed order and writes
// dLNw[c] = w_eff[c] M[c], dLNb[c] = w_eff[c] S, d w_eff[c] = LNw[c] M[c] + LNb[c] S, (block 0) d b_eff = S   (layout tl::, overwritten)
__global__ __launch_bounds__(256) void k_tail_finish(const float* __restrict__ part, int nslots, const float* __restrict__ wpk, float* __restrict__ dtail);

// dW[16*bi + row][16*bj + col] for bi, bj in {0,1}: Ta = dY tile, Tb = X tile, both [16 points][TS]
DEV void outer_accumulate(const float* __restrict__ Ta, const float* __restrict__ Tb, int lane, f4 (&acc)[4]) {
    const int c = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float a0 = Ta[(4 * s + kg) * TS + c], a1 = Ta[(4 * s + kg) * TS + 16 + c];
        const float b0 = Tb[(4 * s + kg) * TS + c], b1 = Tb[(4 * s + kg) * TS + 16 + c];
        acc[0] = mfma16(a0, b0, acc[0]); acc[1] = mfma16(a0, b1, acc[1]);
        acc[2] = mfma16(a1, b0, acc[2]); acc[3] = mfma16(a1, b1, acc[3]);
    }
}

// sum over the 16 points of a tile (lanes r = 0..15 of each group), result valid on every lane
DEV float rsum16(float x) {
    x += __shfl_xor(x, 1); x += __shfl_xor(x, 2); x += __shfl_xor(x, 4); x += __shfl_xor(x, 8);
    return x;
}

template <bool FX>
__global__ __launch_bounds__(256) void k_depth_mean_bwd(DepthMeanBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float w[4 * 1024 + 64 + 64 + 8];
    __shared__ __attribute__((aligned(16))) float tiles[4][2][16 * TS];
    float* W1 = w; float* W2 = w + 1024; float* W1T = w + 2048; float* W2T = w + 3072;
    float* B1 = w + 4096; float* B2 = w + 4128; float* T3 = w + 4160; float* TB = w + 4224;
    for (int i = threadIdx.x; i < 1024; i += 256) {
        W1[i] = a.wpk[pk::DEC1 + i]; W2[i] = a.wpk[pk::DEC2 + i];
        W1T[i] = a.wbk[pkb::DM_W1T + i]; W2T[i] = a.wbk[pkb::DM_W2T + i];
    }
    if (threadIdx.x < 32) { B1[threadIdx.x] = a.wpk[pk::B_DEC1 + threadIdx.x]; B2[threadIdx.x] = a.wpk[pk::B_DEC2 + threadIdx.x]; }
    if (threadIdx.x < 64) T3[threadIdx.x] = a.wpk[pk::T_DEC3 + threadIdx.x];
    if (threadIdx.x < 2) TB[threadIdx.x] = a.wpk[pk::T_DEC3_B + threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float* Ta = tiles[wave][0];
    float* Tb = tiles[wave][1];
    const int tpv = (a.pn + 15) >> 4;
    const float fsx = (float)a.fw / (float)(a.W - 1), fsy = (float)a.fh / (float)(a.H - 1);

    // gradient accumulators of this wavefront (flushed once)
    f4 gW2[4], gW1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { gW2[q] = f4{0.f, 0.f, 0.f, 0.f}; gW1[q] = f4{0.f, 0.f, 0.f, 0.f}; }
    float gb1[8], gb2[8], gW3a[8], gW3b[8], gb3a = 0.f, gb3b = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { gb1[j] = 0.f; gb2[j] = 0.f; gW3a[j] = 0.f; gW3b[j] = 0.f; }

    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
        const int bv = tile / tpv, b = bv / a.V;
        const int n_raw = (tile - bv * tpv) * 16 + r;
        const bool ok = n_raw < a.pn;
        const int n = ok ? n_raw : a.pn - 1;
        const float x = a.coords[((size_t)b * a.pn + n) * 2], y = a.coords[((size_t)b * a.pn + n) * 2 + 1];
        const Taps t = make_taps(x, y, fsx, fsy, -0.5f, a.fh, a.fw);
        const float* fb = a.feat64 + (size_t)bv * a.fh * a.fw * 64 + 8 * g;
        // ---- forward recompute (same arithmetic as k_depth_mean)
        float FR[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f4 a0 = reinterpret_cast<const f4*>(fb + (size_t)t.o00 * 64)[h], a1 = reinterpret_cast<const f4*>(fb + (size_t)t.o01 * 64)[h];
            const f4 a2 = reinterpret_cast<const f4*>(fb + (size_t)t.o10 * 64)[h], a3 = reinterpret_cast<const f4*>(fb + (size_t)t.o11 * 64)[h];
            const f4 fr = a0 * t.w00 + a1 * t.w01 + a2 * t.w10 + a3 * t.w11;
            FR[4 * h] = fr.x; FR[4 * h + 1] = fr.y; FR[4 * h + 2] = fr.z; FR[4 * h + 3] = fr.w;
        }
        f4 acc[2];
        float h1[8], h2[8];                                      // log2e * ELU(.)
        load_bias<2>(B1, g, acc);
        mm<8, 2>(W1, lane, FR, acc);
        elu_to<2>(acc, h1);
        load_bias<2>(B2, g, acc);
        mm<8, 2>(W2, lane, h1, acc);
        elu_to<2>(acc, h2);
        const float o0 = gsum(dot8(T3, g, h2)) + TB[0], o1 = gsum(dot8(T3 + 32, g, h2)) + TB[1];
        // ---- backward.  softplus' = sigmoid; the tables hold W3 / log2e (tilde inputs), h = h~ * ln2
        const float* dm = a.dmean + ((size_t)bv * a.pn + n) * 2;
        const float do0 = ok ? dm[0] * sigmoid1(o0) : 0.f, do1 = ok ? dm[1] * sigmoid1(o1) : 0.f;
        float da2[8], da1[8], dfr[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float w0 = T3[g * 8 + j] * kLog2e, w1 = T3[32 + g * 8 + j] * kLog2e;
            const float dh = w0 * do0 + w1 * do1;
            da2[j] = dh * (h2[j] > 0.f ? 1.f : fmaf(h2[j], kLn2, 1.f));     // ELU' = 1 | ELU + 1
            gW3a[j] = fmaf(do0, h2[j] * kLn2, gW3a[j]);
            gW3b[j] = fmaf(do1, h2[j] * kLn2, gW3b[j]);
            gb2[j] += da2[j];
        }
        if (g == 0) { gb3a += do0; gb3b += do1; }
        // dW2 += da2 (x) h1
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            *reinterpret_cast<f4*>(Ta + r * TS + 16 * nb + 4 * g) = f4{da2[4 * nb], da2[4 * nb + 1], da2[4 * nb + 2], da2[4 * nb + 3]};
            *reinterpret_cast<f4*>(Tb + r * TS + 16 * nb + 4 * g) = f4{h1[4 * nb] * kLn2, h1[4 * nb + 1] * kLn2, h1[4 * nb + 2] * kLn2, h1[4 * nb + 3] * kLn2};
        }
        wave_sync();
        outer_accumulate(Ta, Tb, lane, gW2);
        // dh1 = W2^T da2 ; da1 = dh1 * ELU'(a1)
        acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
        mm<8, 2>(W2T, lane, da2, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const float d[4] = {acc[nb].x, acc[nb].y, acc[nb].z, acc[nb].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 4 * nb + q;
                da1[j] = d[q] * (h1[j] > 0.f ? 1.f : fmaf(h1[j], kLn2, 1.f));
                gb1[j] += da1[j];
            }
        }
        // dW1 += da1 (x) FR     (FR channel 8g + j sits at tile column 8g + j)
        wave_sync();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            *reinterpret_cast<f4*>(Ta + r * TS + 16 * nb + 4 * g) = f4{da1[4 * nb], da1[4 * nb + 1], da1[4 * nb + 2], da1[4 * nb + 3]};
            *reinterpret_cast<f4*>(Tb + r * TS + 8 * g + 4 * nb) = f4{FR[4 * nb], FR[4 * nb + 1], FR[4 * nb + 2], FR[4 * nb + 3]};
        }
        wave_sync();
        outer_accumulate(Ta, Tb, lane, gW1);
        wave_sync();
        // dFR = W1^T da1 (comes out in the gather layout: channel 8g + j), scattered through the four taps
        acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
        mm<8, 2>(W1T, lane, da1, acc);
        dfr[0] = acc[0].x; dfr[1] = acc[0].y; dfr[2] = acc[0].z; dfr[3] = acc[0].w;
        dfr[4] = acc[1].x; dfr[5] = acc[1].y; dfr[6] = acc[1].z; dfr[7] = acc[1].w;
        if (a.dfeat64) {
            // through an LDS tile (free after outer_accumulate: the wave_sync above): one wavefront instruction adds the
            // 32 ray channels of TWO feature-map pixels (two 128-byte runs) instead of 4 channels of 16 pixels
            *reinterpret_cast<f4*>(Ta + r * TS + 8 * g) = f4{dfr[0], dfr[1], dfr[2], dfr[3]};
            *reinterpret_cast<f4*>(Ta + r * TS + 8 * g + 4) = f4{dfr[4], dfr[5], dfr[6], dfr[7]};
            if (g == 0) {
                *reinterpret_cast<f4*>(Tb + r * TS) = f4{ok ? t.w00 : 0.f, ok ? t.w01 : 0.f, ok ? t.w10 : 0.f, ok ? t.w11 : 0.f};
                int* ip = reinterpret_cast<int*>(Tb + r * TS + 4);
                ip[0] = t.o00; ip[1] = t.o01; ip[2] = t.o10; ip[3] = t.o11;
            }
            wave_sync();
            const int half = lane >> 5, ch = lane & 31;
            const size_t gbase = (size_t)bv * a.fh * a.fw * 64 + ch;
            const float fxs = FX ? fx_scale(a.fx) : 0.f;
            for (int pp = 0; pp < 8; ++pp) {
                const int q = pp + 8 * half;
                const float val = Ta[q * TS + ch];
                const f4 wq = *reinterpret_cast<const f4*>(Tb + q * TS);
                const int* ip = reinterpret_cast<const int*>(Tb + q * TS + 4);
                if (wq.x != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[0] * 64, val * wq.x, fxs, a.fx.flag);
                if (wq.y != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[1] * 64, val * wq.y, fxs, a.fx.flag);
                if (wq.z != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[2] * 64, val * wq.z, fxs, a.fx.flag);
                if (wq.w != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[3] * 64, val * wq.w, fxs, a.fx.flag);
            }
            wave_sync();                                  // the next tile's dW2 tiles overwrite Ta / Tb
        }
    }
    // ---- flush: canonical layout (state-dict order), weights [out][in], into this wavefront's slot
    float* gc = grad_slot(a.dpart, DM_STRIDE);
    {
        const int c = lane & 15, kg = lane >> 4;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                const f4 v2 = gW2[bi * 2 + bj], v1 = gW1[bi * 2 + bj];
                const float e2[4] = {v2.x, v2.y, v2.z, v2.w}, e1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int o = 16 * bi + 4 * kg + q, i = 16 * bj + c;
                    gc[can::MEAN2_W + o * 32 + i] = e2[q];
                    gc[can::MEAN0_W + o * 32 + i] = e1[q];
                }
            }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s1 = rsum16(gb1[j]), s2 = rsum16(gb2[j]), s3a = rsum16(gW3a[j]), s3b = rsum16(gW3b[j]);
        if (r == 0) {
            const int f = 16 * (j / 4) + 4 * g + (j % 4);          // natural layout: feature of register j in group g
            gc[can::MEAN0_B + f] = s1;
            gc[can::MEAN2_B + f] = s2;
            gc[can::MEAN4_W + f] = s3a;
            gc[can::MEAN4_W + 32 + f] = s3b;
        }
    }
    {
        const float sa = rsum16(gb3a), sb = rsum16(gb3b);
        if (lane == 0) { gc[can::MEAN4_B] = sa; gc[can::MEAN4_B + 1] = sb; }
    }
}

// channel-last gradient buffer -> NCHW: dfeat64 [BV][npix][64] -> d_ray_feats / d_img_feats [BV][32][npix] (either may be null)
// FX: the entries are 64-bit integers in units of the launch's quantum (FeatFx): value = q * 2^(e - 28), one rounding to float
template <bool FX>
__global__ __launch_bounds__(256) void k_unpack_feat_grad(const float* __restrict__ dfeat64, float* __restrict__ d_ray,
                                                          float* __restrict__ d_img, int npix, FeatFx fx) {
    __shared__ float tile[64][65];
    const int bv = blockIdx.y, p0 = blockIdx.x * 64, t = threadIdx.x;
    const size_t src0 = ((size_t)bv * npix + p0) * 64;
    const double quantum = FX ? ldexp(1.0, fx_exponent(fx.upmax[0]) - 28) : 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int idx = q * 256 + t, p = idx >> 6, c = idx & 63;
        float v = 0.f;
        if (p0 + p < npix) {
            if constexpr (FX) v = (float)((double)reinterpret_cast<const long long*>(dfeat64)[src0 + (size_t)p * 64 + c] * quantum);
            else v = dfeat64[src0 + (size_t)p * 64 + c];
        }
        tile[c][p] = v;
    }
    __syncthreads();
    const int tx = t & 63, ty = t >> 6;
    const size_t base = (size_t)bv * 32 * npix;
#pragma unroll
    for (int c0 = 0; c0 < 64; c0 += 4) {
        const int c = c0 + ty, p = p0 + tx;
        if (p < npix) {
            if (c < 32) { if (d_ray) d_ray[base + (size_t)c * npix + p] = tile[c][tx]; }
            else if (d_img) d_img[base + (size_t)(c - 32) * npix + p] = tile[c][tx];
        }
    }
}

}  // namespace gnr

// =========================================================================================================
// Backward of the volume path, stage 5 of 5 (see DESIGN.md): the per-column tail k_ray<false>
//   g16 -> +posenc -> 4-head self-attention -> fc + residual -> LayerNorm -> out_geometry_fc -> clip -> volume
// Upstream: d volume.  Outputs: d g16 per point and the tail's parameter gradients as per-wavefront partials (layout tp::;
// k_grad_reduce + k_tail_finish turn them into `dtail`: dWq, dWk, dWv, dWfc [16][16] each, dLNw[16], dLNb[16], A[16] = sum ds*n,
// Sds = sum ds; the last two unfold into out_geometry_fc.{0,1} on the host side of the ABI, gnr_capi.inc).
// Same lane packing as k_ray (one lane per sample, rays packed across wavefronts).
// =========================================================================================================
namespace gnr {

struct RayBwdArgs {
    const float* wpk; const float* rec; const float* dvol;
    float* dg16; float* dpart;          // dpart: [wavefront slots][tp::STRIDE] partial tail gradients (k_grad_reduce + k_tail_finish)
    int nrays, dn, rays_per_block, ray_stride, nblocks;
};
namespace tl { constexpr int WQ = 0, WK = 256, WV = 512, WFC = 768, LNW = 1024, LNB = 1040, A = 1056, SDS = 1072, TOTAL = 1073; }

DEV float wave_sum64(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__global__ __launch_bounds__(256) void k_tail_finish(const float* __restrict__ part, int nslots, const float* __restrict__ wpk, float* __restrict__ dtail) {
    __shared__ double shm[256], shs[256];
    const int c = blockIdx.x, t = threadIdx.x;
    double m = 0.0, s = 0.0;
    for (int slot = t; slot < nslots; slot += 256) {
        const double* gd = reinterpret_cast<const double*>(part + (size_t)slot * tp::STRIDE + tp::MS);
        m += gd[c]; s += gd[16];
    }
    shm[t] = m; shs[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {                   // fixed tree: same bits every run
        if (t < w) { shm[t] += shm[t + w]; shs[t] += shs[t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        const double M = shm[0], S = shs[0];
        const double we = wpk[pk::R_OUTVJP + c], lw = wpk[pk::R_LNW + c], lb = wpk[pk::R_LNB + c];
        dtail[tl::LNW + c] = (float)(we * M);
        dtail[tl::LNB + c] = (float)(we * S);
        dtail[tl::A + c] = (float)(lw * M + lb * S);
        if (c == 0) dtail[tl::SDS] = (float)S;
    }
}

__global__ __launch_bounds__(256, 2) void k_ray_bwd(RayBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int dn = a.dn, S = dn, rpb = a.rays_per_block;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rl = (int)threadIdx.x / S;
    const int slot = (int)threadIdx.x - rl * S;
    const bool in_blk = rl < rpb;
    rl = min(rl, rpb - 1);
    const int i = min(slot, dn - 1);
    float* sc = sm + (size_t)rl * a.ray_stride;
    float* Kb = sc; float* Vb = sc + dn * 16; float* Qb = sc + dn * 32; float* Ob = sc + dn * 48; float* St = sc + dn * 64;
    float* KN = Ob;
    const float* W = a.wpk;
    f4 gacc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) gacc[m] = f4{0.f, 0.f, 0.f, 0.f};
    // M[c] = sum ds xhat_c (+ the tangent part in the dual kernel), S = sum ds, in double from the lane on: thousands of O(1)
    // terms of either sign; dLNw = w_eff M, dLNb = w_eff S, d w_eff = LNw M + LNb S follow in k_tail_finish
    double gM[16], gS = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) gM[c] = 0.0;

    for (int blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        const int ray_u = blk * rpb + rl;
        const bool rvalid = in_blk && ray_u < a.nrays;
        const int ray = min(ray_u, a.nrays - 1);
        const bool act = rvalid && slot < dn;
        const size_t pt = (size_t)ray * dn + i;
        const float* rec = a.rec + pt * REC_VOL;
        float t[16];
        {
            const f4* r4 = reinterpret_cast<const f4*>(rec);
            const f4* pe = reinterpret_cast<const f4*>(W + pk::R_PE + i * 16);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f4 x = r4[q], e = pe[q];
                t[4 * q] = x.x + e.x; t[4 * q + 1] = x.y + e.y; t[4 * q + 2] = x.z + e.z; t[4 * q + 3] = x.w + e.w;
            }
        }
        const float nvalid = rec[16];
        const bool rowok = nvalid > 1.f;
        float q[16], kk[16], vv[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            float sq = 0.f, sk = 0.f, sv = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                sq = fmaf(W[pk::R_WQ + f * 16 + c], t[c], sq);
                sk = fmaf(W[pk::R_WK + f * 16 + c], t[c], sk);
                sv = fmaf(W[pk::R_WV + f * 16 + c], t[c], sv);
            }
            q[f] = sq; kk[f] = sk; vv[f] = sv;
        }
        __syncthreads();                                  // previous iteration's MFMA tiles are dead
        // every lane of the workgroup fills its slot (lanes beyond the last ray shadow it): the weight-gradient MFMAs
        // below contract over ALL 256 lanes, so no lane may ever compute on uninitialised LDS (0 * NaN)
        if (in_blk) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f4 k4 = {kk[4 * c], kk[4 * c + 1], kk[4 * c + 2], kk[4 * c + 3]};
                reinterpret_cast<f4*>(Kb + i * 16)[c] = k4;
                reinterpret_cast<f4*>(Vb + i * 16)[c] = f4{vv[4 * c], vv[4 * c + 1], vv[4 * c + 2], vv[4 * c + 3]};
                reinterpret_cast<f4*>(Qb + i * 16)[c] = f4{q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3]};
                KN[i * 16 + c] = k4.x * k4.x + k4.y * k4.y + k4.z * k4.z + k4.w * k4.w;
            }
        }
        __syncthreads();
        float amax[4];
        {
            f4 kmax = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < dn; ++j) {
                const f4 n = *reinterpret_cast<const f4*>(KN + j * 16);
                kmax.x = fmaxf(kmax.x, n.x); kmax.y = fmaxf(kmax.y, n.y); kmax.z = fmaxf(kmax.z, n.z); kmax.w = fmaxf(kmax.w, n.w);
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float qn = q[4 * h] * q[4 * h] + q[4 * h + 1] * q[4 * h + 1] + q[4 * h + 2] * q[4 * h + 2] + q[4 * h + 3] * q[4 * h + 3];
                amax[h] = rowok ? 0.5f * sqrtf(qn * kmax[h]) : -1e9f;
            }
        }
        float o[16], ainv[4];
        {
            float l[4];
            auto sweep = [&]() {
#pragma unroll
                for (int h = 0; h < 4; ++h) l[h] = 0.f;
#pragma unroll
                for (int f = 0; f < 16; ++f) o[f] = 0.f;
                for (int j = 0; j < dn; ++j) {
                    float sj[4];
                    head_logits(q, Kb + j * 16, rowok, sj);
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const f4 vj = reinterpret_cast<const f4*>(Vb + j * 16)[h];
                        const float pj = __expf(sj[h] - amax[h]);
                        l[h] += pj;
                        o[4 * h] = fmaf(pj, vj.x, o[4 * h]); o[4 * h + 1] = fmaf(pj, vj.y, o[4 * h + 1]);
                        o[4 * h + 2] = fmaf(pj, vj.z, o[4 * h + 2]); o[4 * h + 3] = fmaf(pj, vj.w, o[4 * h + 3]);
                    }
                }
            };
            sweep();
            if (!(fminf(fminf(l[0], l[1]), fminf(l[2], l[3])) > 1e-30f)) {
#pragma unroll
                for (int h = 0; h < 4; ++h) amax[h] = -3.0e38f;
                for (int j = 0; j < dn; ++j) {
                    float sj[4];
                    head_logits(q, Kb + j * 16, rowok, sj);
#pragma unroll
                    for (int h = 0; h < 4; ++h) amax[h] = fmaxf(amax[h], sj[h]);
                }
                sweep();
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                ainv[h] = 1.f / l[h];
                o[4 * h] *= ainv[h]; o[4 * h + 1] *= ainv[h]; o[4 * h + 2] *= ainv[h]; o[4 * h + 3] *= ainv[h];
            }
        }
        float y[16], xh[16];
        float mean = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            float s = t[c];
#pragma unroll
            for (int f = 0; f < 16; ++f) s = fmaf(W[pk::R_WFC + c * 16 + f], o[f], s);
            y[c] = s; mean += s;
        }
        mean *= (1.f / 16.f);
        float var = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) { const float d = y[c] - mean; var += d * d; }
        var *= (1.f / 16.f);
        const float rstd = 1.f / sqrtf(var + 1e-6f);
        float sraw = W[pk::R_OUTB];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            xh[c] = (y[c] - mean) * rstd;
            sraw = fmaf(W[pk::R_OUTVJP + c], xh[c] * W[pk::R_LNW + c] + W[pk::R_LNB + c], sraw);
        }
        // ---- backward
        const size_t o_idx = (size_t)ray * dn + (dn - 1 - i);          // the forward's z flip (renderer.py:197-198)
        const float ds = (act && sraw >= -1.f && sraw <= 1.f && nvalid >= 1.f) ? a.dvol[o_idx] : 0.f;
        gS += (double)ds;
        float dy[16];
        {
            float m1 = 0.f, m2 = 0.f, dxh[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const float dnc = ds * W[pk::R_OUTVJP + c];
                gM[c] = fma((double)ds, (double)xh[c], gM[c]);
                dxh[c] = dnc * W[pk::R_LNW + c];
                m1 += dxh[c]; m2 += dxh[c] * xh[c];
            }
            m1 *= (1.f / 16.f); m2 *= (1.f / 16.f);
#pragma unroll
            for (int c = 0; c < 16; ++c) dy[c] = rstd * (dxh[c] - m1 - xh[c] * m2);
        }
        float dO[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) s = fmaf(dy[c], W[pk::R_WFCT + f * 16 + c], s);
            dO[f] = s;
        }
        // dQ = sum_j P_ij (dA_ij - rs_i) k_j / 2 with rs_i = sum_j P_ij dA_ij = dO_i . o_i (the attention's own output: no swept sum for it)
        float dQ[16], rsv[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) rsv[h] = dO[4 * h] * o[4 * h] + dO[4 * h + 1] * o[4 * h + 1] + dO[4 * h + 2] * o[4 * h + 2] + dO[4 * h + 3] * o[4 * h + 3];
        {
            float A1[16];
#pragma unroll
            for (int f = 0; f < 16; ++f) A1[f] = 0.f;
            for (int j = 0; j < dn; ++j) {
                float sj[4];
                head_logits(q, Kb + j * 16, rowok, sj);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const f4 kj = reinterpret_cast<const f4*>(Kb + j * 16)[h];
                    const f4 vj = reinterpret_cast<const f4*>(Vb + j * 16)[h];
                    const float pj = __expf(sj[h] - amax[h]) * ainv[h];
                    const float dA = dO[4 * h] * vj.x + dO[4 * h + 1] * vj.y + dO[4 * h + 2] * vj.z + dO[4 * h + 3] * vj.w;
                    const float pd = pj * (dA - rsv[h]);
                    A1[4 * h] = fmaf(pd, kj.x, A1[4 * h]); A1[4 * h + 1] = fmaf(pd, kj.y, A1[4 * h + 1]);
                    A1[4 * h + 2] = fmaf(pd, kj.z, A1[4 * h + 2]); A1[4 * h + 3] = fmaf(pd, kj.w, A1[4 * h + 3]);
                }
            }
            const float sc2 = rowok ? 0.5f : 0.f;
#pragma unroll
            for (int f = 0; f < 16; ++f) dQ[f] = A1[f] * sc2;
        }
        __syncthreads();
        if (in_blk) {
#pragma unroll
            for (int c = 0; c < 4; ++c) reinterpret_cast<f4*>(Ob + i * 16)[c] = f4{dO[4 * c], dO[4 * c + 1], dO[4 * c + 2], dO[4 * c + 3]};
            reinterpret_cast<f4*>(St + i * 12)[0] = f4{amax[0], amax[1], amax[2], amax[3]};
            reinterpret_cast<f4*>(St + i * 12)[1] = f4{rowok ? ainv[0] : -ainv[0], ainv[1], ainv[2], ainv[3]};
            reinterpret_cast<f4*>(St + i * 12)[2] = f4{rsv[0], rsv[1], rsv[2], rsv[3]};
        }
        __syncthreads();
        float dK[16], dV[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) { dK[f] = 0.f; dV[f] = 0.f; }
        for (int qi = 0; qi < dn; ++qi) {
            const f4 mx4 = reinterpret_cast<const f4*>(St + qi * 12)[0];
            f4 il4 = reinterpret_cast<const f4*>(St + qi * 12)[1];
            const f4 rs4 = reinterpret_cast<const f4*>(St + qi * 12)[2];
            const bool ok = il4.x > 0.f;
            il4.x = fabsf(il4.x);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const f4 qv = reinterpret_cast<const f4*>(Qb + qi * 16)[h];
                const f4 dov = reinterpret_cast<const f4*>(Ob + qi * 16)[h];
                float s = 0.5f * (qv.x * kk[4 * h] + qv.y * kk[4 * h + 1] + qv.z * kk[4 * h + 2] + qv.w * kk[4 * h + 3]);
                s = ok ? s : -1e9f;
                const float pj = __expf(s - mx4[h]) * il4[h];
                const float dA = dov.x * vv[4 * h] + dov.y * vv[4 * h + 1] + dov.z * vv[4 * h + 2] + dov.w * vv[4 * h + 3];
                const float dL = ok ? pj * (dA - rs4[h]) * 0.5f : 0.f;
                dK[4 * h] = fmaf(dL, qv.x, dK[4 * h]); dK[4 * h + 1] = fmaf(dL, qv.y, dK[4 * h + 1]);
                dK[4 * h + 2] = fmaf(dL, qv.z, dK[4 * h + 2]); dK[4 * h + 3] = fmaf(dL, qv.w, dK[4 * h + 3]);
                dV[4 * h] = fmaf(pj, dov.x, dV[4 * h]); dV[4 * h + 1] = fmaf(pj, dov.y, dV[4 * h + 1]);
                dV[4 * h + 2] = fmaf(pj, dov.z, dV[4 * h + 2]); dV[4 * h + 3] = fmaf(pj, dov.w, dV[4 * h + 3]);
            }
        }
        // d g16 = d t
        if (act) {
            float* dg = a.dg16 + pt * 16;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                float r4v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = 4 * c4 + u;
                    float s = dy[c];
#pragma unroll
                    for (int f = 0; f < 16; ++f) {
                        s = fmaf(W[pk::R_WQT + c * 16 + f], dQ[f], s);
                        s = fmaf(W[pk::R_WKT + c * 16 + f], dK[f], s);
                        s = fmaf(W[pk::R_WVT + c * 16 + f], dV[f], s);
                    }
                    r4v[u] = s;
                }
                reinterpret_cast<f4*>(dg)[c4] = f4{r4v[0], r4v[1], r4v[2], r4v[3]};
            }
        }
        // ---- weight gradients: dW[f][c] += sum_points dY[f] X[c] as MFMAs with the workgroup's 256 lanes as K
        float* TY = sm;                       // [256][16]   (the attention scratch is dead after the barrier)
        float* TX = sm + 256 * 16;            // [256][16]
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            __syncthreads();
            const float* dYm = m == 0 ? dQ : (m == 1 ? dK : (m == 2 ? dV : dy));
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                reinterpret_cast<f4*>(TY + threadIdx.x * 16)[c] = act ? f4{dYm[4 * c], dYm[4 * c + 1], dYm[4 * c + 2], dYm[4 * c + 3]} : f4{0.f, 0.f, 0.f, 0.f};
                if (m == 0) reinterpret_cast<f4*>(TX + threadIdx.x * 16)[c] = f4{t[4 * c], t[4 * c + 1], t[4 * c + 2], t[4 * c + 3]};
                if (m == 3) reinterpret_cast<f4*>(TX + threadIdx.x * 16)[c] = f4{o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]};
            }
            __syncthreads();
            const int c16 = lane & 15, kg = lane >> 4;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const int p = 64 * wave + 4 * s + kg;
                gacc[m] = mfma16(TY[p * 16 + c16], TX[p * 16 + c16], gacc[m]);
            }
        }
    }
    // ---- flush
    {
        const int c16 = lane & 15, kg = lane >> 4;
        float* gt = grad_slot(a.dpart, tp::STRIDE);
#pragma unroll
        for (int m = 0; m < 4; ++m) {                     // dWq, dWk, dWv, dWfc at tp::W + 256 m (the order of tl::)
            const float e[4] = {gacc[m].x, gacc[m].y, gacc[m].z, gacc[m].w};
#pragma unroll
            for (int u = 0; u < 4; ++u) gt[tp::W + 256 * m + (4 * kg + u) * 16 + c16] = e[u];
        }
        double* gd = reinterpret_cast<double*>(gt + tp::MS);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const double s1 = wave_sum64d(gM[c]);
            if (lane == 0) gd[c] = s1;
        }
        const double ss = wave_sum64d(gS);
        if (lane == 0) gd[16] = ss;
    }
}

}  // namespace gnr

// =========================================================================================================
// Stage 4: geometry_fc (86 -> 64 -> 16, ELU, ELU) and the second cross-view reduction (ibrnet.py:482-489).
// In: the saved per-view state (h~_v[8 slots], v2_v) of the tile, the point, d g16.  Out: d(h_v, v2_v) per view
// (true scale) and the gradients of geometry_fc.{0,2}.  One wavefront per 16-point tile, chain layout of k_chain.
// =========================================================================================================
namespace gnr {

struct GeoBwdArgs {
    const float* wpk; const float* wbk;
    const float* desc;        // [B*P][8]
    const float* save2;       // [tiles][V][9][64]
    const float* dg16;        // [B*P][16]
    float* dS2;               // [tiles][V][9][64]   d h_v[8], d v2_v
    float* dpart;             // [wavefront slots][GP_STRIDE] partial parameter gradients
    int B, P, ntiles;
};

constexpr int TS2 = 112;      // LDS tile row stride for up to 96 columns (4 k-groups on disjoint banks)
// inter-stage gradient record of a (tile, view) between stages 3 / 2 / 1: d X[9] (stage 3: per-view columns of base_fc.0; stage 2
// adds the part through the cross-view statistics), d e[8] (stage 3), d gate (stage 2)
constexpr int DS1 = 18;

// acc[bi * NBJ + bj] += dY-block bi (x) X-block bj over the tile's 16 points
template <int NBI, int NBJ, int STR = TS2>
DEV void outer_acc(const float* __restrict__ Ta, const float* __restrict__ Tb, int lane, f4 (&acc)[NBI * NBJ]) {
    const int c = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float av[NBI], bv[NBJ];
#pragma unroll
        for (int bi = 0; bi < NBI; ++bi) av[bi] = Ta[(4 * s + kg) * STR + 16 * bi + c];
#pragma unroll
        for (int bj = 0; bj < NBJ; ++bj) bv[bj] = Tb[(4 * s + kg) * STR + 16 * bj + c];
#pragma unroll
        for (int bi = 0; bi < NBI; ++bi)
#pragma unroll
            for (int bj = 0; bj < NBJ; ++bj) acc[bi * NBJ + bj] = mfma16(av[bi], bv[bj], acc[bi * NBJ + bj]);
    }
}

// natural-layout registers (J = 4*NB) -> tile row r, column = feature (16*nb + 4g + t) + col0
template <int NB, int STR = TS2>
DEV void tile_put_nat(float* __restrict__ T, int r, int g, const float (&x)[4 * NB], float scale, int col0 = 0) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
        *reinterpret_cast<f4*>(T + r * STR + col0 + 16 * nb + 4 * g) = f4{x[4 * nb] * scale, x[4 * nb + 1] * scale, x[4 * nb + 2] * scale, x[4 * nb + 3] * scale};
}

// store NBI x NBJ accumulator blocks into a row-major [rows][ld] canonical matrix of the wavefront's slot (columns beyond ncols dropped)
// (row0: the matrix starts at block row `row0` -- several small layers may share an accumulator block, k_view1_bwd_pw)
template <int NBI, int NBJ>
DEV void flush_blocks(float* __restrict__ dst, int ld, int nrows, int ncols, int lane, const f4 (&acc)[NBI * NBJ], int row0 = 0) {
    const int c = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int bi = 0; bi < NBI; ++bi)
#pragma unroll
        for (int bj = 0; bj < NBJ; ++bj) {
            const f4 v = acc[bi * NBJ + bj];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = 16 * bi + 4 * kg + q - row0, i = 16 * bj + c;
                if (o >= 0 && o < nrows && i < ncols) dst[(size_t)o * ld + i] = e[q];
            }
        }
}

DEV float elu_grad_t(float ht) { return ht > 0.f ? 1.f : fmaf(ht, kLn2, 1.f); }     // ELU'(a) from log2e*ELU(a)

// ---- fp16-pair products in the backward twins (round 5).  k_view2_bwd / k_view1_bwd multiply on the f16 matrix cores like
// k_chain (gnr_kernels.hip, "fp16-pair layers"): the forward recompute reads the forward blob's C16 image with the forward
// kernel's own layer code, the dX chains read pair images of the transposed fragments (gnr_layout.h pkb::P2_* / P1_*).
// A GRADIENT has no natural scale (1e-9 per voxel of a mean loss, 1e+3 under a loss scale), and the pair form is exact only
// between ~1e-7 and 65 504: the upstream gradient of a (tile, view) is therefore normalised by a wave-uniform power of two
// s = 2^-e (its largest magnitude lands in [1, 2)) when it is read, the whole backward chain of the (tile, view) -- linear in the
// upstream gradient -- runs on the scaled values, and 1/s goes back in where values leave the chain: the weight-gradient tiles
// (tile_put_nat's scale), the bias sums (fma instead of add), the stores.  Powers of two: exact.
DEV void grad_scale(float lane_amax, float& s, float& inv, unsigned* wave_max_bits = nullptr) {
    unsigned m = __float_as_uint(lane_amax);                       // non-negative floats order like their bit patterns
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = m > t ? m : t; }
    m = __builtin_amdgcn_readfirstlane(m);
    if (wave_max_bits) *wave_max_bits = m;                         // (the fixed-point scatter's launch-wide maximum is the maximum of these)
    const float mx = __uint_as_float(m);
    // zero, denormal or non-finite upstream: no scaling (the chain then computes what the unscaled kernel computed)
    const bool ok = mx >= 1e-30f && mx <= 1e30f;
    const int e = ok ? __builtin_amdgcn_frexp_expf(mx) - 1 : 0;    // mx = f 2^e with f in [1, 2)
    s = __builtin_amdgcn_ldexpf(1.f, -e);
    inv = __builtin_amdgcn_ldexpf(1.f, e);
}
// y[nb] += W^T-fragment (pair image at w: KB blocks) x d  for a gradient operand d[8 KB] (already normalised by grad_scale)
template <int KB, int NB>
DEV void mm16g(const float* __restrict__ w, int lane, const float (&d)[8 * KB], f4 (&acc)[NB]) {
    P8 p[KB];
    p[0] = split8<0>(d);
    if constexpr (KB > 1) p[1] = split8<8>(d);
    mm16<KB, NB, true>(w, lane, p, acc);
}

template <int V>
__global__ __launch_bounds__(256, 1) void k_geo_bwd(GeoBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // LDS image: forward GEO1 (23x4), GEO2 (16x1), their biases; transposed GEO1^T (16 x 5 blocks), GEO2^T (4x4); tiles
    constexpr int F_GEO1 = 0, F_GEO2 = F_GEO1 + frag_floats(23, 4), F_B1 = F_GEO2 + frag_floats(16, 1), F_B2 = F_B1 + 64,
                  F_G1TA = F_B2 + 16, F_G1TB = F_G1TA + frag_floats(16, 4), F_G2T = F_G1TB + frag_floats(16, 1),
                  F_TILES = F_G2T + frag_floats(4, 4);
    for (int i = threadIdx.x; i < frag_floats(23, 4); i += 256) lds[F_GEO1 + i] = a.wpk[pk::GEO1 + i];
    for (int i = threadIdx.x; i < frag_floats(16, 1); i += 256) { lds[F_GEO2 + i] = a.wpk[pk::GEO2 + i]; lds[F_G1TB + i] = a.wbk[pkb::GEO1T_B + i]; }
    for (int i = threadIdx.x; i < frag_floats(16, 4); i += 256) lds[F_G1TA + i] = a.wbk[pkb::GEO1T_A + i];
    for (int i = threadIdx.x; i < frag_floats(4, 4); i += 256) lds[F_G2T + i] = a.wbk[pkb::GEO2T + i];
    if (threadIdx.x < 64) lds[F_B1 + threadIdx.x] = a.wpk[pk::B_GEO1 + threadIdx.x];
    if (threadIdx.x < 16) lds[F_B2 + threadIdx.x] = a.wpk[pk::B_GEO2 + threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float* Ta = lds + F_TILES + wave * 2 * 16 * TS2;
    float* Tb = Ta + 16 * TS2;
    const int tps = (a.P + 15) >> 4;

    f4 gW1[4 * 6], gW2[1 * 4];
#pragma unroll
    for (int q = 0; q < 24; ++q) gW1[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) gW2[q] = f4{0.f, 0.f, 0.f, 0.f};
    float gb1[16], gb2[4];
#pragma unroll
    for (int j = 0; j < 16; ++j) gb1[j] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) gb2[j] = 0.f;

    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
        const int b = tile / tps, ts = tile - b * tps;
        const int n_raw = ts * 16 + r;
        const bool row_ok = n_raw < a.P;
        const int n = row_ok ? n_raw : a.P - 1;
        const size_t pt = (size_t)b * a.P + n;
        float S2[V][9];
        {
            const float* sp = a.save2 + (size_t)tile * V * 9 * 64 + lane;
#pragma unroll
            for (int v = 0; v < V; ++v)
#pragma unroll
                for (int q = 0; q < 9; ++q) S2[v][q] = sp[(v * 9 + q) * 64];
        }
        // ---- forward recompute: statistics, Z, geometry_fc
        float vsum = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) vsum += S2[v][8];
        const float inv_vsum = rcp1(vsum + 1e-8f);
        float Z[23], wbar = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) wbar += S2[v][8] * inv_vsum;
        wbar *= (1.f / (float)V);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float mu = 0.f, va = 0.f;
#pragma unroll
            for (int v = 0; v < V; ++v) mu += S2[v][j] * (S2[v][8] * inv_vsum);
#pragma unroll
            for (int v = 0; v < V; ++v) { const float d = S2[v][j] - mu; va += (S2[v][8] * inv_vsum) * d * d; }
            Z[j] = mu; Z[8 + j] = va;
        }
        {
            const f4 d0 = reinterpret_cast<const f4*>(a.desc)[pt * 2];
            const float pc = g == 1 ? d0.x : (g == 2 ? d0.y : d0.z);
            float s1, c1, s2, c2, s4, c4;
            sincos_octaves(pc, s1, c1, s2, c2, s4, c4);
            const bool g0 = g == 0;
            Z[16] = g0 ? wbar : pc; Z[17] = g0 ? 0.f : s1; Z[18] = g0 ? 0.f : c1; Z[19] = g0 ? 0.f : s2;
            Z[20] = g0 ? 0.f : c2; Z[21] = g0 ? 0.f : s4; Z[22] = g0 ? 0.f : c4;
        }
        f4 U[4];
        float u64[16];
        load_bias<4>(lds + F_B1, g, U);
        mm<23, 4>(lds + F_GEO1, lane, Z, U);
        elu_to<4>(U, u64);
        f4 g16[1];
        float gg[4];
        load_bias<1>(lds + F_B2, g, g16);
        mm<16, 1>(lds + F_GEO2, lane, u64, g16);
        elu_to<1>(g16, gg);
        // ---- backward through geometry_fc.2
        float da2[4];
        {
            const f4 dg = row_ok ? reinterpret_cast<const f4*>(a.dg16 + pt * 16)[g] : f4{0.f, 0.f, 0.f, 0.f};
            da2[0] = dg.x * elu_grad_t(gg[0]); da2[1] = dg.y * elu_grad_t(gg[1]);
            da2[2] = dg.z * elu_grad_t(gg[2]); da2[3] = dg.w * elu_grad_t(gg[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) gb2[j] += da2[j];
        }
        wave_sync();
        tile_put_nat<1>(Ta, r, g, da2, 1.f);
        tile_put_nat<4>(Tb, r, g, u64, kLn2);
        wave_sync();
        outer_acc<1, 4>(Ta, Tb, lane, gW2);
        f4 dU[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) dU[nb] = f4{0.f, 0.f, 0.f, 0.f};
        mm<4, 4>(lds + F_G2T, lane, da2, dU);
        float da1[16];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            da1[4 * nb] = dU[nb].x * elu_grad_t(u64[4 * nb]); da1[4 * nb + 1] = dU[nb].y * elu_grad_t(u64[4 * nb + 1]);
            da1[4 * nb + 2] = dU[nb].z * elu_grad_t(u64[4 * nb + 2]); da1[4 * nb + 3] = dU[nb].w * elu_grad_t(u64[4 * nb + 3]);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) gb1[j] += da1[j];
        // geometry_fc.0: dW += da1 (x) [mean(32) var(32) wbar embed(21)] at true scale, canonical column order
        wave_sync();
        tile_put_nat<4>(Ta, r, g, da1, 1.f);
        {
            float mu_t[8], va_t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { mu_t[j] = Z[j]; va_t[j] = Z[8 + j]; }
            tile_put_nat<2>(Tb, r, g, mu_t, kLn2, 0);
            tile_put_nat<2>(Tb, r, g, va_t, kLn2 * kLn2, 32);
            if (g == 0) {
                Tb[r * TS2 + 64] = Z[16];
#pragma unroll
                for (int c = 86; c < 96; ++c) Tb[r * TS2 + c] = 0.f;
            } else {
#pragma unroll
                for (int k = 0; k < 7; ++k) Tb[r * TS2 + 65 + 3 * k + (g - 1)] = Z[16 + k];
            }
        }
        wave_sync();
        outer_acc<4, 6>(Ta, Tb, lane, gW1);
        // d Z = W1^T da1 : slots 0..15 (mean, var) and slot 16 on group 0 (wbar)
        f4 dZa[4], dZb[1];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) dZa[nb] = f4{0.f, 0.f, 0.f, 0.f};
        dZb[0] = f4{0.f, 0.f, 0.f, 0.f};
        mm<16, 4>(lds + F_G1TA, lane, da1, dZa);
        mm<16, 1>(lds + F_G1TB, lane, da1, dZb);
        float dmu[8], dva[8];
        dmu[0] = dZa[0].x; dmu[1] = dZa[0].y; dmu[2] = dZa[0].z; dmu[3] = dZa[0].w;
        dmu[4] = dZa[1].x; dmu[5] = dZa[1].y; dmu[6] = dZa[1].z; dmu[7] = dZa[1].w;
        dva[0] = dZa[2].x; dva[1] = dZa[2].y; dva[2] = dZa[2].z; dva[3] = dZa[2].w;
        dva[4] = dZa[3].x; dva[5] = dZa[3].y; dva[6] = dZa[3].z; dva[7] = dZa[3].w;
        const float dwbar = __shfl(dZb[0].x, r);                    // group 0's slot 16
        // ---- second reduction backward (true scale: h = h~ ln2)
        float dwp[V], accw = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float h = S2[v][j] * kLn2, d = (S2[v][j] - Z[j]) * kLn2;
                s = fmaf(dmu[j], h, s);
                s = fmaf(dva[j], d * d, s);
            }
            dwp[v] = gsum(s) + dwbar * (1.f / (float)V);
            accw = fmaf(S2[v][8] * inv_vsum, dwp[v], accw);
        }
        float* dp = a.dS2 + (size_t)tile * V * 9 * 64 + lane;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float wv = S2[v][8] * inv_vsum;
#pragma unroll
            for (int j = 0; j < 8; ++j) dp[(v * 9 + j) * 64] = wv * fmaf(2.f * (S2[v][j] - Z[j]) * kLn2, dva[j], dmu[j]);
            dp[(v * 9 + 8) * 64] = inv_vsum * (dwp[v] - accw);
        }
        wave_sync();
    }
    // ---- flush
    float* gc = grad_slot(a.dpart, GP_STRIDE);
    flush_blocks<4, 6>(gc + can::GEO0_W, 86, 64, 86, lane, gW1);
    flush_blocks<1, 4>(gc + can::GEO2_W, 64, 16, 64, lane, gW2);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float s = rsum16(gb1[j]);
        if (r == 0) gc[can::GEO0_B + 16 * (j / 4) + 4 * g + (j % 4)] = s;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float s = rsum16(gb2[j]);
        if (r == 0) gc[can::GEO2_B + 4 * g + j] = s;
    }
}

}  // namespace gnr

// =========================================================================================================
// Stage 3: the second view loop (ibrnet.py:474-481): base_fc (per-view part), vis_fc, vis_fc2.
// In per (tile, view): saved X[9], e1[8], m; the tile's hoisted pre-activation G; d(h_v, v2_v) from stage 4.
// Out: d G (summed over views), d X_v, d e_v (e = prob_embed.2 output) per view; gradients of base_fc.0 columns 140..206
// and bias, base_fc.2, vis_fc.{0,2}, vis_fc2.{0,2}.  The forward of the view is recomputed from the saved inputs.
// =========================================================================================================
namespace gnr {

// Range guard of the backward's view kernels (round 6).  The fp16-pair kernels recompute the forward and run the dX chains on pair
// operands: a feature or a weight beyond the pair range (bits 0 / 2 of the prepared scene's status word 0) or an activation that left it
// in the pass's training forward (bit 1 of that forward's launch slot; the render passes of a prepared scene share two slots and are
// guarded together) would turn their gradients into NaNs -- or, for a weight without
// a pair, into silently wrong numbers.  Every pair launch is therefore followed by the fp32-input-MFMA instantiation of the same
// kernel on the same arguments; run_if tells each which side of the flag it serves (nothing synchronises with the host):
//   0 always (GNR_OPT_FP32_CHAIN, partial test runs)   1 unless flagged (the pair kernels)   2 only if flagged (their fp32 twins)
// status: the backward's status word (bit 4 = GNR_STATUS_LOST_PARTNER); lose_partner: GNR_OPT_TEST_LOSE_PARTNER.
struct BwdGuard { const unsigned* word0; const unsigned* slot; const unsigned* slot2; int run_if; unsigned* status; int lose_partner; };
DEV bool bwd_guard_skip(const BwdGuard& g) {                      // wave-uniform; evaluated before anything is staged or stored
    if (g.run_if == 0) return false;
    const unsigned w = (g.word0 ? __builtin_nontemporal_load(g.word0) & 5u : 0u) | (g.slot ? __builtin_nontemporal_load(g.slot) & 2u : 0u) |
                       (g.slot2 ? __builtin_nontemporal_load(g.slot2) & 2u : 0u);
    return g.run_if == 1 ? w != 0u : w == 0u;
}

struct View2BwdArgs {
    const float* wpk; const float* wbk;
    const float* save1; const float* saveG; const float* dS2;     // dS2: [tiles][V][9 | 10][64] (+ d colour logit: RENDER)
    float* dS1;               // [tiles][V][DS1][64]: d X[9], d e[8], (d gate, d X[9] through the statistics: stage 2)
    float* dG;                // [tiles][16][64]
    float* dpart;             // [wavefront slots][GP_STRIDE] partial parameter gradients
    int V, ntiles;
    const float* desc; const float* viewp;      // RENDER: the colour head needs the direction differences
    int P, H, W;
    BwdGuard guard;
};

// BP (k_view2_bwd / k_view1_bwd): forward recompute + dX chains on the f16 matrix cores (fp16 pairs); false: fp32-input MFMA (rounds 1-4)
namespace l3 {                // LDS image of k_view2_bwd (floats)
constexpr int FW = 0, BASE1 = 0, BASE2 = frag_floats(17, 4), VIS1 = BASE2 + frag_floats(16, 2), VIS2 = VIS1 + 1024, VISB1 = VIS2 + 1024;
constexpr int BI = VISB1 + 1024, TB = BI + 128, SC = TB + 64, BW = SC + 4;
constexpr int PE2F = BW, B_PE2 = PE2F + 1024, VISB1T = B_PE2 + 32, VIS2T = VISB1T + 1024, VIS1T = VIS2T + 1024,
              BASE2T = VIS1T + 1024, BASE1XT = BASE2T + frag_floats(8, 4), BASE1ET = BASE1XT + frag_floats(16, 3);
constexpr int TILES = BASE1ET + frag_floats(16, 2);
// pair image (k_view2_bwd<false>): the blob's section pkb::P2_BEGIN .. has the same slots in the same order; only base_fc.0^T's x part
// is shorter there (three output blocks, not a padded fourth), so base_fc.0^T's e part is copied on its own
static_assert(VISB1T - BW == pkb::P2_VISB1T - pkb::P2_BEGIN && BASE1XT - BW == pkb::P2_BASE1XT - pkb::P2_BEGIN &&
              pkb::P2_BASE1ET - pkb::P2_BASE1XT <= BASE1ET - BASE1XT && pkb::P2_END - pkb::P2_BASE1ET == TILES - BASE1ET, "LDS image = the blob's pair section");
constexpr int TOTAL = TILES + 4 * 2 * 16 * TS2;
// colour head (RENDER), behind the tiles
constexpr int RGB1 = TOTAL, RGB2 = RGB1 + frag_floats(10, 1), B_RGB1 = RGB2 + frag_floats(4, 1), B_RGB2 = B_RGB1 + 16, T_RGB3 = B_RGB2 + 16,
              RGB2T = T_RGB3 + 16, RGB0HT = RGB2T + frag_floats(4, 1), T_RGB0V = RGB0HT + frag_floats(4, 2);
constexpr int TOTAL_RENDER = T_RGB0V + 16;
}

// BP: forward recompute + dX chains on fp16 pairs (the volume instantiation's default) / on the fp32-input MFMA (the range guard's
// fallback for both passes, GNR_OPT_FP32_CHAIN).  Pairs on the volume points only: the render instantiation (colour head: 4 more
// accumulator blocks, a second projection) sits at the 256-arch-register limit in the fp32 form already (32 B of scratch); with the
// pair operands it spills 576 B and runs 1.70 -> 3.22 ms per step (measured, profiles/r05_d_*), so it keeps the fp32-input MFMA.
template <bool RENDER, bool BP = !RENDER>
__global__ __launch_bounds__(256, 1) void k_view2_bwd(View2BwdArgs a) {
    static_assert(!(RENDER && BP), "k_view2_bwd<true> runs on the fp32-input MFMA");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (bwd_guard_skip(a.guard)) return;
    // forward fragments base_fc.0 (per-view part) .. vis_fc2.0: the C16 image's pair blocks (same slots, same sizes) or the fp32 CHAIN image
    for (int i = threadIdx.x; i < l3::BI; i += 256) lds[i] = a.wpk[(BP ? pk::C16 + pk::c16_off(pk::BASE1) : pk::BASE1) + i];
    if (threadIdx.x < 128) lds[l3::BI + threadIdx.x] = a.wpk[pk::B_BASE2 + threadIdx.x];
    if (threadIdx.x < 64) lds[l3::TB + threadIdx.x] = a.wpk[pk::T_VIS2R + threadIdx.x];
    if (threadIdx.x < 4) lds[l3::SC + threadIdx.x] = a.wpk[pk::T_SCAL + threadIdx.x];
    if constexpr (BP) {
        for (int i = threadIdx.x; i < pkb::P2_BASE1ET - pkb::P2_BEGIN; i += 256) lds[l3::BW + i] = a.wbk[pkb::P2_BEGIN + i];
        for (int i = threadIdx.x; i < pkb::P2_END - pkb::P2_BASE1ET; i += 256) lds[l3::BASE1ET + i] = a.wbk[pkb::P2_BASE1ET + i];
    } else {
        for (int i = threadIdx.x; i < l3::TILES - l3::BW; i += 256) lds[l3::BW + i] = a.wbk[pkb::V2_BEGIN + i];
    }
    if constexpr (RENDER) {
        for (int i = threadIdx.x; i < frag_floats(10, 1) + frag_floats(4, 1); i += 256) lds[l3::RGB1 + i] = a.wpk[pk::RGB1 + i];
        if (threadIdx.x < 32) lds[l3::B_RGB1 + threadIdx.x] = a.wpk[pk::B_RGB1 + threadIdx.x];
        if (threadIdx.x < 16) lds[l3::T_RGB3 + threadIdx.x] = a.wpk[pk::T_RGB3 + threadIdx.x];
        for (int i = threadIdx.x; i < l3::TOTAL_RENDER - l3::RGB2T; i += 256) lds[l3::RGB2T + i] = a.wbk[pkb::RGB2T + i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float* Ta = lds + l3::TILES + wave * 2 * 16 * TS2;
    float* Tb = Ta + 16 * TS2;
    const int V = a.V;

    f4 gWx[4 * 3], gWe[4 * 2], gWb2[2 * 4], gWv1[2 * 2], gWv2[2 * 2], gWvb1[2 * 2];
#pragma unroll
    for (int q = 0; q < 12; ++q) gWx[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) { gWe[q] = f4{0.f, 0.f, 0.f, 0.f}; gWb2[q] = f4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int q = 0; q < 4; ++q) { gWv1[q] = f4{0.f, 0.f, 0.f, 0.f}; gWv2[q] = f4{0.f, 0.f, 0.f, 0.f}; gWvb1[q] = f4{0.f, 0.f, 0.f, 0.f}; }
    float gb0[16], gbb2[8], gbv1[8], gbv2[8], gbvb1[8], gWv2r[8], gWvb2[8], gbv2r = 0.f, gbvb2 = 0.f;
    f4 gWc0[3], gWc2[1];
    float gbc0[4], gbc2[4], gWc4[4], gbc4 = 0.f;
    gWc0[0] = f4{0.f, 0.f, 0.f, 0.f}; gWc0[1] = gWc0[0]; gWc0[2] = gWc0[0]; gWc2[0] = gWc0[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) { gbc0[j] = 0.f; gbc2[j] = 0.f; gWc4[j] = 0.f; }
#pragma unroll
    for (int j = 0; j < 16; ++j) gb0[j] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { gbb2[j] = 0.f; gbv1[j] = 0.f; gbv2[j] = 0.f; gbvb1[j] = 0.f; gWv2r[j] = 0.f; gWvb2[j] = 0.f; }

    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
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
            if constexpr (RENDER) {                                             // see k_view1_bwd: nothing flows through a view that no sample of the tile sees
                if (__ballot(m != 0.f) == 0ull) {
                    float* o1 = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
#pragma unroll
                    for (int j = 0; j < 17; ++j) o1[j * 64] = 0.f;              // (entry 17, d gate, is k_hoist_bwd's: it stores it for every pair)
                    continue;
                }
            }
            constexpr int D2W = RENDER ? 10 : 9;
            const float* d2 = a.dS2 + ((size_t)tile * V + v) * D2W * 64 + lane;
#pragma unroll
            for (int j = 0; j < 8; ++j) dH[j] = d2[j * 64];
            float dv2 = d2[8 * 64];
            // the (tile, view)'s upstream gradient normalised by a power of two (grad_scale): gs in, gi = 1 / gs back out
            float gs = 1.f, gi = 1.f;
            float dclog_up = 0.f;
            if constexpr (RENDER) dclog_up = (m != 0.f) ? d2[9 * 64] : 0.f;
            if constexpr (BP) {
                float am = fabsf(dv2);
#pragma unroll
                for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(dH[j]));
                if constexpr (RENDER) am = fmaxf(am, fabsf(dclog_up));
                grad_scale(am, gs, gi);
#pragma unroll
                for (int j = 0; j < 8; ++j) dH[j] *= gs;
                dv2 *= gs; dclog_up *= gs;
            }
            // ---- forward recompute of this view (k_chain, second view loop; with pairs: the forward kernel's own instruction sequence)
            const float w = m * inv_msum;
            float b1t[16], H0t[8], v1t[8], rest[8], Ht[8], t1t[8], xin[8], xin2[8], e[8];
            f4 acc4[4] = {G[0], G[1], G[2], G[3]}, acc[2];
            if constexpr (BP) {
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
            } else {
                mm<9, 4>(lds + l3::BASE1, lane, X, acc4);
                mm<8, 4, 9>(lds + l3::BASE1, lane, E1, acc4);
                elu_to<4>(acc4, b1t);
                load_bias<2>(lds + l3::BI + 0, g, acc);
                mm<16, 2>(lds + l3::BASE2, lane, b1t, acc);
                elu_to<2>(acc, H0t);
#pragma unroll
                for (int j = 0; j < 8; ++j) xin[j] = H0t[j] * w;
                load_bias<2>(lds + l3::BI + 32, g, acc);
                mm<8, 2>(lds + l3::VIS1, lane, xin, acc);
                elu_to<2>(acc, v1t);
                load_bias<2>(lds + l3::BI + 64, g, acc);
                mm<8, 2>(lds + l3::VIS2, lane, v1t, acc);
                elu_to<2>(acc, rest);
            }
            const float a_r = gsum(dot8(lds + l3::TB, g, v1t)) + lds[l3::SC + 1];
            const float logit = elu1(a_r), sg = sigmoid1(logit), vis1 = sg * m;
#pragma unroll
            for (int j = 0; j < 8; ++j) { Ht[j] = H0t[j] + rest[j]; xin2[j] = Ht[j] * vis1; }
            load_bias<2>(lds + l3::BI + 96, g, acc);
            if constexpr (BP) { const P8U xp = split8u<0>(xin2); mm16u<1, 2, true>(lds + l3::VISB1, lane, &xp, acc); }
            else mm<8, 2>(lds + l3::VISB1, lane, xin2, acc);
            elu_to<2>(acc, t1t);
            const float v2 = sigmoid1(gsum(dot8(lds + l3::TB + 32, g, t1t)) + lds[l3::SC + 2]) * m;
            load_bias<2>(lds + l3::B_PE2, g, acc);
            if constexpr (BP) { const P8 ep = split8<0>(E1); mm16<1, 2, true>(lds + l3::PE2F, lane, &ep, acc); }
            else mm<8, 2>(lds + l3::PE2F, lane, E1, acc);
            e[0] = acc[0].x; e[1] = acc[0].y; e[2] = acc[0].z; e[3] = acc[0].w; e[4] = acc[1].x; e[5] = acc[1].y; e[6] = acc[1].z; e[7] = acc[1].w;
            // ---- colour head rgb_fc (ibrnet.py:506-509): logit = rgb_fc([h, v2, dir diff]); -1e9 where the view is masked
            if constexpr (RENDER) {
                const float dclog = dclog_up;                      // (scaled by gs)
                ViewGeom vg;
                project_view<true>(a.viewp + (bscene * V + v) * VIEWP_FLOATS, pp3, qd3, a.H, a.W, vg);
                f4 acc1[1];
                float c1t[4], c2t[4];
                load_bias<1>(lds + l3::B_RGB1, g, acc1);
                mm<8, 1>(lds + l3::RGB1, lane, Ht, acc1);
                const float ex[2] = {g == 0 ? v2 : (g == 1 ? vg.dd[0] : (g == 2 ? vg.dd[1] : vg.dd[2])), g == 0 ? vg.dd[3] : 0.f};
                mm<2, 1, 8>(lds + l3::RGB1, lane, ex, acc1);
                elu_to<1>(acc1, c1t);
                load_bias<1>(lds + l3::B_RGB2, g, acc1);
                mm<4, 1>(lds + l3::RGB2, lane, c1t, acc1);
                elu_to<1>(acc1, c2t);
                if (g == 0) gbc4 = fmaf(dclog, gi, gbc4);
                float dc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gWc4[j] = fmaf(dclog * gi, c2t[j] * kLn2, gWc4[j]);
                    dc[j] = lds[l3::T_RGB3 + g * 4 + j] * kLog2e * dclog * elu_grad_t(c2t[j]);
                    gbc2[j] = fmaf(dc[j], gi, gbc2[j]);
                }
                wave_sync();
                tile_put_nat<1>(Ta, r, g, dc, gi);
                tile_put_nat<1>(Tb, r, g, c1t, kLn2);
                wave_sync();
                outer_acc<1, 1>(Ta, Tb, lane, gWc2);
                acc1[0] = f4{0.f, 0.f, 0.f, 0.f};
                mm<4, 1>(lds + l3::RGB2T, lane, dc, acc1);
                dc[0] = acc1[0].x * elu_grad_t(c1t[0]); dc[1] = acc1[0].y * elu_grad_t(c1t[1]);
                dc[2] = acc1[0].z * elu_grad_t(c1t[2]); dc[3] = acc1[0].w * elu_grad_t(c1t[3]);
                float sv = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) { gbc0[j] = fmaf(dc[j], gi, gbc0[j]); sv = fmaf(lds[l3::T_RGB0V + g * 4 + j], dc[j], sv); }
                dv2 += gsum(sv);
                wave_sync();
                tile_put_nat<1>(Ta, r, g, dc, gi);
                tile_put_nat<2>(Tb, r, g, Ht, kLn2);
                if (g == 0) { Tb[r * TS2 + 32] = v2; Tb[r * TS2 + 36] = vg.dd[3]; }
                else Tb[r * TS2 + 32 + g] = ex[0];
                if (g == 1) {
#pragma unroll
                    for (int c = 37; c < 48; ++c) Tb[r * TS2 + c] = 0.f;
                }
                wave_sync();
                outer_acc<1, 3>(Ta, Tb, lane, gWc0);
                f4 acc2[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
                mm<4, 2>(lds + l3::RGB0HT, lane, dc, acc2);
                dH[0] += acc2[0].x; dH[1] += acc2[0].y; dH[2] += acc2[0].z; dH[3] += acc2[0].w;
                dH[4] += acc2[1].x; dH[5] += acc2[1].y; dH[6] += acc2[1].z; dH[7] += acc2[1].w;
            }
            // ---- backward: vis_fc2
            const float da_b2 = dv2 * v2 * (1.f - v2);
            if (g == 0) gbvb2 = fmaf(da_b2, gi, gbvb2);
            float da[8], dx[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                gWvb2[j] = fmaf(da_b2 * gi, t1t[j] * kLn2, gWvb2[j]);
                da[j] = lds[l3::TB + 32 + g * 8 + j] * kLog2e * da_b2 * elu_grad_t(t1t[j]);
                gbvb1[j] = fmaf(da[j], gi, gbvb1[j]);
            }
            wave_sync();
            tile_put_nat<2>(Ta, r, g, da, gi);
            tile_put_nat<2>(Tb, r, g, xin2, kLn2);
            wave_sync();
            outer_acc<2, 2>(Ta, Tb, lane, gWvb1);
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            if constexpr (BP) mm16g<1, 2>(lds + l3::VISB1T, lane, da, acc);
            else mm<8, 2>(lds + l3::VISB1T, lane, da, acc);
            dx[0] = acc[0].x; dx[1] = acc[0].y; dx[2] = acc[0].z; dx[3] = acc[0].w; dx[4] = acc[1].x; dx[5] = acc[1].y; dx[6] = acc[1].z; dx[7] = acc[1].w;
            float dvis1 = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { dvis1 = fmaf(dx[j], Ht[j] * kLn2, dvis1); dH[j] = fmaf(dx[j], vis1, dH[j]); }
            dvis1 = gsum(dvis1);
            // ---- vis_fc.2 (32 residual rows + the visibility row) and vis_fc.0
            const float da_r = dvis1 * m * sg * (1.f - sg) * (a_r > 0.f ? 1.f : logit + 1.f);
            if (g == 0) gbv2r = fmaf(da_r, gi, gbv2r);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                gWv2r[j] = fmaf(da_r * gi, v1t[j] * kLn2, gWv2r[j]);
                da[j] = dH[j] * elu_grad_t(rest[j]);
                gbv2[j] = fmaf(da[j], gi, gbv2[j]);
            }
            wave_sync();
            tile_put_nat<2>(Ta, r, g, da, gi);
            tile_put_nat<2>(Tb, r, g, v1t, kLn2);
            wave_sync();
            outer_acc<2, 2>(Ta, Tb, lane, gWv2);
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            if constexpr (BP) mm16g<1, 2>(lds + l3::VIS2T, lane, da, acc);
            else mm<8, 2>(lds + l3::VIS2T, lane, da, acc);
            dx[0] = acc[0].x; dx[1] = acc[0].y; dx[2] = acc[0].z; dx[3] = acc[0].w; dx[4] = acc[1].x; dx[5] = acc[1].y; dx[6] = acc[1].z; dx[7] = acc[1].w;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dv1 = fmaf(lds[l3::TB + g * 8 + j] * kLog2e, da_r, dx[j]);
                da[j] = dv1 * elu_grad_t(v1t[j]);
                gbv1[j] = fmaf(da[j], gi, gbv1[j]);
            }
            wave_sync();
            tile_put_nat<2>(Ta, r, g, da, gi);
            tile_put_nat<2>(Tb, r, g, xin, kLn2);
            wave_sync();
            outer_acc<2, 2>(Ta, Tb, lane, gWv1);
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            if constexpr (BP) mm16g<1, 2>(lds + l3::VIS1T, lane, da, acc);
            else mm<8, 2>(lds + l3::VIS1T, lane, da, acc);
            dx[0] = acc[0].x; dx[1] = acc[0].y; dx[2] = acc[0].z; dx[3] = acc[0].w; dx[4] = acc[1].x; dx[5] = acc[1].y; dx[6] = acc[1].z; dx[7] = acc[1].w;
            // ---- base_fc.2
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                da[j] = fmaf(dx[j], w, dH[j]) * elu_grad_t(H0t[j]);
                gbb2[j] = fmaf(da[j], gi, gbb2[j]);
            }
            wave_sync();
            tile_put_nat<2>(Ta, r, g, da, gi);
            tile_put_nat<4>(Tb, r, g, b1t, kLn2);
            wave_sync();
            outer_acc<2, 4>(Ta, Tb, lane, gWb2);
            f4 d4[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) d4[nb] = f4{0.f, 0.f, 0.f, 0.f};
            if constexpr (BP) mm16g<1, 4>(lds + l3::BASE2T, lane, da, d4);
            else mm<8, 4>(lds + l3::BASE2T, lane, da, d4);
            // ---- base_fc.0, per-view columns
            float da1[16];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                da1[4 * nb] = d4[nb].x * elu_grad_t(b1t[4 * nb]); da1[4 * nb + 1] = d4[nb].y * elu_grad_t(b1t[4 * nb + 1]);
                da1[4 * nb + 2] = d4[nb].z * elu_grad_t(b1t[4 * nb + 2]); da1[4 * nb + 3] = d4[nb].w * elu_grad_t(b1t[4 * nb + 3]);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) dGacc[j] = fmaf(da1[j], gi, dGacc[j]);
            wave_sync();
            tile_put_nat<4>(Ta, r, g, da1, gi);
            // x in canonical order [r g b | img feats]: slot j < 8 -> 3 + 8g + j, slot 8 -> colour channel g (g < 3)
#pragma unroll
            for (int j = 0; j < 8; ++j) Tb[r * TS2 + 3 + 8 * g + j] = X[j];
            if (g < 3) Tb[r * TS2 + g] = X[8];
            if (g == 3) {
#pragma unroll
                for (int c = 35; c < 48; ++c) Tb[r * TS2 + c] = 0.f;
            }
            wave_sync();
            outer_acc<4, 3>(Ta, Tb, lane, gWx);
            wave_sync();
            tile_put_nat<2>(Tb, r, g, e, 1.f);
            wave_sync();
            outer_acc<4, 2>(Ta, Tb, lane, gWe);
            f4 d3[3];
            d3[0] = f4{0.f, 0.f, 0.f, 0.f}; d3[1] = d3[0]; d3[2] = d3[0];
            acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
            if constexpr (BP) {
                mm16g<2, 3>(lds + l3::BASE1XT, lane, da1, d3);
                mm16g<2, 2>(lds + l3::BASE1ET, lane, da1, acc);
            } else {
                mm<16, 3>(lds + l3::BASE1XT, lane, da1, d3);
                mm<16, 2>(lds + l3::BASE1ET, lane, da1, acc);
            }
            float* o1 = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
            o1[0] = d3[0].x * gi; o1[64] = d3[0].y * gi; o1[128] = d3[0].z * gi; o1[192] = d3[0].w * gi;
            o1[256] = d3[1].x * gi; o1[320] = d3[1].y * gi; o1[384] = d3[1].z * gi; o1[448] = d3[1].w * gi;
            o1[512] = d3[2].x * gi;
            o1[9 * 64] = acc[0].x * gi; o1[10 * 64] = acc[0].y * gi; o1[11 * 64] = acc[0].z * gi; o1[12 * 64] = acc[0].w * gi;
            o1[13 * 64] = acc[1].x * gi; o1[14 * 64] = acc[1].y * gi; o1[15 * 64] = acc[1].z * gi; o1[16 * 64] = acc[1].w * gi;
        }
        float* og = a.dG + (size_t)tile * 16 * 64 + lane;
#pragma unroll
        for (int j = 0; j < 16; ++j) { og[j * 64] = dGacc[j]; gb0[j] += dGacc[j]; }
        wave_sync();
    }
    // ---- flush (canonical, state-dict order, into this wavefront's slot)
    float* gc = grad_slot(a.dpart, GP_STRIDE);
    flush_blocks<4, 3>(gc + can::BASE0_W + 140, 207, 64, 35, lane, gWx);
    flush_blocks<4, 2>(gc + can::BASE0_W + 175, 207, 64, 32, lane, gWe);
    flush_blocks<2, 4>(gc + can::BASE2_W, 64, 32, 64, lane, gWb2);
    flush_blocks<2, 2>(gc + can::VIS0_W, 32, 32, 32, lane, gWv1);
    flush_blocks<2, 2>(gc + can::VIS2_W, 32, 32, 32, lane, gWv2);
    flush_blocks<2, 2>(gc + can::VISB0_W, 32, 32, 32, lane, gWvb1);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float s = rsum16(gb0[j]);
        if (r == 0) gc[can::BASE0_B + 16 * (j / 4) + 4 * g + (j % 4)] = s;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int f = 16 * (j / 4) + 4 * g + (j % 4);
        const float s0 = rsum16(gbb2[j]), s1 = rsum16(gbv1[j]), s2 = rsum16(gbv2[j]), s3 = rsum16(gbvb1[j]), s4 = rsum16(gWv2r[j]), s5 = rsum16(gWvb2[j]);
        if (r == 0) {
            gc[can::BASE2_B + f] = s0; gc[can::VIS0_B + f] = s1;
            gc[can::VIS2_B + f] = s2; gc[can::VISB0_B + f] = s3;
            gc[can::VIS2_W + 32 * 32 + f] = s4; gc[can::VISB2_W + f] = s5;
        }
    }
    {
        const float s0 = rsum16(gbv2r), s1 = rsum16(gbvb2);
        if (lane == 0) { gc[can::VIS2_B + 32] = s0; gc[can::VISB2_B] = s1; }
    }
    if constexpr (RENDER) {
        flush_blocks<1, 3>(gc + can::RGB0_W, 37, 16, 37, lane, gWc0);
        flush_blocks<1, 1>(gc + can::RGB2_W, 16, 8, 16, lane, gWc2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s0 = rsum16(gbc0[j]), s1 = rsum16(gbc2[j]), s2 = rsum16(gWc4[j]);
            if (r == 0) {
                gc[can::RGB0_B + 4 * g + j] = s0;
                if (4 * g + j < 8) { gc[can::RGB2_B + 4 * g + j] = s1; gc[can::RGB4_W + 4 * g + j] = s2; }
            }
        }
        const float s = rsum16(gbc4);
        if (lane == 0) gc[can::RGB4_B] = s;
    }
}

}  // namespace gnr


// =========================================================================================================
// Stage 2: the view-invariant 140 columns of base_fc.0 and the first cross-view reduction (ibrnet.py:466-472).
// In: d G per tile, the saved X_v, gate_v, m_v.  Out: d X_v += (statistics path), d gate_v; gradient of
// base_fc.0[:, :140].  Weighted mean / variance with un-normalised weights w0 = gate * w: the derivative of the
// variance through the mean does not cancel (sum of w0 != 1) and is carried in d mu_eff.
// =========================================================================================================
namespace gnr {

struct HoistBwdArgs {
    const float* wbk; const float* save1; const float* saveG; const float* dG;
    float* dS1; float* dpart;      // dpart: [wavefront slots][GP_STRIDE] partial parameter gradients
    int ntiles;
};
constexpr int TS3 = 176;      // tile row stride for 144 columns

template <int V>
__global__ __launch_bounds__(256, 1) void k_hoist_bwd(HoistBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int F_A = 0, F_B = F_A + frag_floats(16, 4), F_C = F_B + frag_floats(16, 4), F_TILES = F_C + frag_floats(16, 1);
    for (int i = threadIdx.x; i < F_TILES; i += 256) lds[i] = a.wbk[pkb::HOISTT_A + i];
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float* Ta = lds + F_TILES + wave * 2 * 16 * TS3;
    float* Tb = Ta + 16 * TS3;
    f4 gW[4 * 9];
#pragma unroll
    for (int q = 0; q < 36; ++q) gW[q] = f4{0.f, 0.f, 0.f, 0.f};

    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
        float X[V][9], gate[V], wv[V];
        const float inv_msum = a.saveG[((size_t)tile * 17 + 16) * 64 + lane];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float* s1 = a.save1 + ((size_t)tile * V + v) * 19 * 64 + lane;
#pragma unroll
            for (int j = 0; j < 9; ++j) X[v][j] = s1[j * 64];
            gate[v] = s1[17 * 64];
            wv[v] = s1[18 * 64] * inv_msum;
        }
        float dG[16];
        {
            const float* dp = a.dG + (size_t)tile * 16 * 64 + lane;
#pragma unroll
            for (int j = 0; j < 16; ++j) dG[j] = dp[j * 64];
        }
        // statistics (forward recompute, true scale)
        float SV[36], S0 = 0.f, S1 = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) { S0 += gate[v] * wv[v]; S1 += wv[v]; }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float mu0 = 0.f, mu1 = 0.f, va0 = 0.f, va1 = 0.f;
#pragma unroll
            for (int v = 0; v < V; ++v) { mu0 += X[v][j] * (gate[v] * wv[v]); mu1 += X[v][j] * wv[v]; }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float d0 = X[v][j] - mu0, d1 = X[v][j] - mu1;
                va0 += (gate[v] * wv[v]) * d0 * d0; va1 += wv[v] * d1 * d1;
            }
            SV[j] = mu0; SV[9 + j] = va0; SV[18 + j] = mu1; SV[27 + j] = va1;
        }
        // base_fc.0[:, :140] gradient: d G (x) [mu0 var0 mu1 var1] in canonical column order 35*k + channel
        wave_sync();
        tile_put_nat<4, TS3>(Ta, r, g, dG, 1.f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) Tb[r * TS3 + 35 * k + 3 + 8 * g + j] = SV[9 * k + j];
            if (g < 3) Tb[r * TS3 + 35 * k + g] = SV[9 * k + 8];
        }
        if (g == 3) { Tb[r * TS3 + 140] = 0.f; Tb[r * TS3 + 141] = 0.f; Tb[r * TS3 + 142] = 0.f; Tb[r * TS3 + 143] = 0.f; }
        wave_sync();
        outer_acc<4, 9, TS3>(Ta, Tb, lane, gW);
        // stage 3's d X of the tile, read in ONE batch before anything is stored and AHEAD of the transposed products and the reduction's
        // arithmetic below (which hide its latency): as `o1[j] += ..` per view the 54 updates were dependent load / add / store round
        // trips (the compiler cannot prove the stores of one view apart from the loads of the next), and the kernel waited on memory
        // for 80 % of its time
        float dXa[V][9];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float* o1 = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
#pragma unroll
            for (int j = 0; j < 9; ++j) dXa[v][j] = o1[j * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        // d SV = W^T d G, slot layout (36 slots per lane group)
        float dSV[36];
        {
            f4 o4[4];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) o4[nb] = f4{0.f, 0.f, 0.f, 0.f};
                mm<16, 4>(lds + (half ? F_B : F_A), lane, dG, o4);
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    dSV[16 * half + 4 * nb] = o4[nb].x; dSV[16 * half + 4 * nb + 1] = o4[nb].y;
                    dSV[16 * half + 4 * nb + 2] = o4[nb].z; dSV[16 * half + 4 * nb + 3] = o4[nb].w;
                }
            }
            f4 o1[1] = {f4{0.f, 0.f, 0.f, 0.f}};
            mm<16, 1>(lds + F_C, lane, dG, o1);
            dSV[32] = o1[0].x; dSV[33] = o1[0].y; dSV[34] = o1[0].z; dSV[35] = o1[0].w;
        }
        // first reduction backward
        float dmu0e[9], dmu1e[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            dmu0e[j] = dSV[j] - 2.f * dSV[9 + j] * SV[j] * (1.f - S0);
            dmu1e[j] = dSV[18 + j] - 2.f * dSV[27 + j] * SV[18 + j] * (1.f - S1);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float* o1 = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
            const float w0 = gate[v] * wv[v];
            float dw0 = 0.f;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const float d0 = X[v][j] - SV[j], d1 = X[v][j] - SV[18 + j];
                o1[j * 64] = dXa[v][j] + w0 * fmaf(2.f * d0, dSV[9 + j], dmu0e[j]) + wv[v] * fmaf(2.f * d1, dSV[27 + j], dmu1e[j]);
                dw0 = fmaf(dmu0e[j], X[v][j], dw0);
                dw0 = fmaf(dSV[9 + j], d0 * d0, dw0);
            }
            o1[17 * 64] = gsum(dw0) * wv[v];
        }
        wave_sync();
    }
    flush_blocks<4, 9>(grad_slot(a.dpart, GP_STRIDE) + can::BASE0_W, 207, 64, 140, lane, gW);
}

}  // namespace gnr

// =========================================================================================================
// Stage 1: the first view loop (renderer.py:62-88, dist_decoder.py:99-142, aggregate_net.py:46-54, ibrnet.py:457-469):
// gather, mixture-of-logistics decoder -> hit / vis, prob_embed, ray_dir_fc, neuray_fc gate.
// In per (tile, view): d X_v, d e_v (base_fc part), d gate_v.  Out: feature-map gradients (scattered channel-last)
// and the gradients of the decoder, prob_embed, ray_dir_fc and neuray_fc.  The view's forward is recomputed.
// =========================================================================================================
#include "gnr_bwd_scatter.inc"
namespace gnr {

struct View1BwdArgs {
    const float* wpk; const float* wbk;
    const float* feat64; const float* viewp; const float* desc;
    const float* dS1;
    float* dfeat64; float* dpart;  // dpart: [wavefront slots][GP_STRIDE] partial parameter gradients
    int B, V, P, H, W, fh, fw, ntiles;
    int skip_masked;               // ray points: a (tile, view) pair without a valid sample has no gradient anywhere (weight 0) and is skipped
    FeatFx fx;                     // FX instantiations only (dfeat64 then holds int64 entries)
    ScatterBins sc;                // k_view1_bwd_pw<false, true>: the rows are parked for the binned scatter (gnr_bwd_scatter.inc)
    BwdGuard guard;
};

namespace l1 {                // LDS image of k_view1_bwd (floats)
constexpr int FW = 0;                                                     // pk::DEC1 .. pk::BASE1
constexpr int DEC1 = pk::DEC1, DEC2 = pk::DEC2, PE1 = pk::PE1, RDF1 = pk::RDF1, RDF2 = pk::RDF2, NR1 = pk::NR1;
constexpr int BI = pk::BASE1;                                             // 304 bias floats from pk::B_DEC1
constexpr int B_DEC1 = BI, B_DEC2 = BI + 96, B_PE1 = BI + 192, B_RDF1 = BI + 224, B_RDF2 = BI + 240, B_NR1 = BI + 288;
constexpr int TB = BI + 304;                                              // T_DEC3 (160), T_DEC3_B (8), T_NR2 (16)
constexpr int T_DEC3 = TB, T_DEC3_B = TB + 160, T_NR2 = TB + 168, SC = TB + 184;
constexpr int BW = SC + 4;                                                // backward section, pkb::V1_BEGIN ..
constexpr int DEC2T = BW, DEC1T = DEC2T + 3072, PE2F = DEC1T + 3072, B_PE2 = PE2F + 1024, PE2T = B_PE2 + 32,
              PE0T = PE2T + 1024, T_PE0HV = PE0T + 1024, NR0T = T_PE0HV + 64, RDF2T = NR0T + frag_floats(4, 2);
constexpr int TILES = RDF2T + frag_floats(9, 1);
// BP: [DEC2T, T_PE0HV) is the blob's pair section pkb::P1_BEGIN .. P1_END (same order, same sizes); T_PE0HV, NR0T, RDF2T
// (short layers: fp32) come from the fp32 section as before
static_assert(T_PE0HV - BW == pkb::P1_END - pkb::P1_BEGIN && PE2F - BW == pkb::P1_PE2F - pkb::P1_BEGIN && PE0T - BW == pkb::P1_PE0T - pkb::P1_BEGIN, "LDS image = the blob's pair section");
constexpr int TOTAL = TILES + 4 * 2 * 16 * TS2;
// use_vis (k_view1_bwd<true>): the fourth decoder branch behind the tiles -- forward fragments, bias tables, last-layer row and
// bias, transposed fragments
constexpr int V_DEC1 = TOTAL, V_DEC2 = V_DEC1 + 1024, V_B1 = V_DEC2 + 1024, V_B2 = V_B1 + 32, V_T3 = V_B2 + 32, V_SC = V_T3 + 32,
              V_DEC2T = V_SC + 4, V_DEC1T = V_DEC2T + 1024;
constexpr int TOTAL_VIS = V_DEC1T + 1024;
static_assert(pk::DEC1 == 0 && pk::B_PE1 == pk::B_DEC1 + 192 && pk::B_NR1 == pk::B_DEC1 + 288 && pk::T_NR2 == pk::T_DEC3 + 168, "layout");
}

template <bool USEVIS, bool FX = false, bool BP = true>      // BP: fp16 pairs / fp32-input MFMA, as for k_view2_bwd
__global__ __launch_bounds__(256, 1) void k_view1_bwd(View1BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (bwd_guard_skip(a.guard)) return;
    constexpr int NBR = USEVIS ? 4 : 3;                                    // decoder branches: mean, var, aw (, vis)
    if constexpr (USEVIS) {
        for (int i = threadIdx.x; i < 1024; i += 256) {
            constexpr bool BPV = BP;
            lds[l1::V_DEC1 + i] = a.wpk[(BPV ? pk::C16 + pk::c16_off(pk::DECV1) : pk::DECV1) + i];
            lds[l1::V_DEC2 + i] = a.wpk[(BPV ? pk::C16 + pk::c16_off(pk::DECV2) : pk::DECV2) + i];
            lds[l1::V_DEC2T + i] = a.wbk[(BPV ? pkb::P_DECV2T : pkb::DECV2T) + i]; lds[l1::V_DEC1T + i] = a.wbk[(BPV ? pkb::P_DECV1T : pkb::DECV1T) + i];
        }
        if (threadIdx.x < 32) {
            lds[l1::V_B1 + threadIdx.x] = a.wpk[pk::B_DECV1 + threadIdx.x]; lds[l1::V_B2 + threadIdx.x] = a.wpk[pk::B_DECV2 + threadIdx.x];
            lds[l1::V_T3 + threadIdx.x] = a.wpk[pk::T_DECV3 + threadIdx.x];
        }
        if (threadIdx.x == 0) lds[l1::V_SC] = a.wpk[pk::T_VIS];
    }
    // LDS offsets of branch br's images: the three branches of the level blob are contiguous, the vis branch sits behind the tiles
    auto o_dec1 = [](int br) { return br < 3 ? l1::DEC1 + br * 1024 : l1::V_DEC1; };
    auto o_dec2 = [](int br) { return br < 3 ? l1::DEC2 + br * 1024 : l1::V_DEC2; };
    auto o_b1 = [](int br) { return br < 3 ? l1::B_DEC1 + br * 32 : l1::V_B1; };
    auto o_b2 = [](int br) { return br < 3 ? l1::B_DEC2 + br * 32 : l1::V_B2; };
    auto o_dec2t = [](int br) { return br < 3 ? l1::DEC2T + br * 1024 : l1::V_DEC2T; };
    auto o_dec1t = [](int br) { return br < 3 ? l1::DEC1T + br * 1024 : l1::V_DEC1T; };
    // forward fragments decoder .. neuray_fc.0: the C16 image (pair blocks; ray_dir_fc stays fp32 there too) or the fp32 CHAIN image
    for (int i = threadIdx.x; i < pk::BASE1; i += 256) lds[i] = a.wpk[(BP ? pk::C16 : 0) + i];
    for (int i = threadIdx.x; i < 304; i += 256) lds[l1::BI + i] = a.wpk[pk::B_DEC1 + i];
    if (threadIdx.x < 184) lds[l1::TB + threadIdx.x] = a.wpk[pk::T_DEC3 + threadIdx.x];
    if (threadIdx.x < 4) lds[l1::SC + threadIdx.x] = a.wpk[pk::T_SCAL + threadIdx.x];
    if constexpr (BP) {
        for (int i = threadIdx.x; i < l1::T_PE0HV - l1::BW; i += 256) lds[l1::BW + i] = a.wbk[pkb::P1_BEGIN + i];
        for (int i = threadIdx.x; i < l1::TILES - l1::T_PE0HV; i += 256) lds[l1::T_PE0HV + i] = a.wbk[pkb::T_PE0HV + i];
    } else {
        for (int i = threadIdx.x; i < l1::TILES - l1::BW; i += 256) lds[l1::BW + i] = a.wbk[pkb::V1_BEGIN + i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float* Ta = lds + l1::TILES + wave * 2 * 16 * TS2;
    float* Tb = Ta + 16 * TS2;
    const int V = a.V, tps = (a.P + 15) >> 4;
    const float fsx = (float)a.fw / (float)(a.W - 1), fsy = (float)a.fh / (float)(a.H - 1);

    f4 gWd1[NBR][4], gWd2[NBR][4], gWpe0[2 * 3], gWpe2[4], gWnr0[2], gWr2[3], gWr1[1];
#pragma unroll
    for (int b3 = 0; b3 < NBR; ++b3)
#pragma unroll
        for (int q = 0; q < 4; ++q) { gWd1[b3][q] = f4{0.f, 0.f, 0.f, 0.f}; gWd2[b3][q] = f4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int q = 0; q < 6; ++q) gWpe0[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) gWpe2[q] = f4{0.f, 0.f, 0.f, 0.f};
    gWnr0[0] = f4{0.f, 0.f, 0.f, 0.f}; gWnr0[1] = gWnr0[0]; gWr1[0] = gWnr0[0];
    gWr2[0] = gWnr0[0]; gWr2[1] = gWnr0[0]; gWr2[2] = gWnr0[0];
    constexpr int NROW = USEVIS ? 6 : 5;                                   // last-layer rows: mean 2, var 2, aw 1 (, vis 1)
    float gW3[NROW][8], gb3[NROW], gbd1[NBR][8], gbd2[NBR][8], gbpe0[8], gbpe2[8], gbnr0[4], gWnr2[4], gbnr2 = 0.f, gbr1[4], gbr2[9];
#pragma unroll
    for (int q = 0; q < NROW; ++q) { gb3[q] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) gW3[q][j] = 0.f; }
#pragma unroll
    for (int q = 0; q < NBR; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) { gbd1[q][j] = 0.f; gbd2[q][j] = 0.f; }
#pragma unroll
    for (int j = 0; j < 8; ++j) { gbpe0[j] = 0.f; gbpe2[j] = 0.f; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { gbnr0[j] = 0.f; gWnr2[j] = 0.f; gbr1[j] = 0.f; }
#pragma unroll
    for (int j = 0; j < 9; ++j) gbr2[j] = 0.f;

    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
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
            // every quantity this view hands to the reductions carries the weight m = 0 (ibrnet.py:466-484; hit, vis, the rgb taps and the
            // bilinear taps are products with m): with no valid sample in the tile all of its gradients are exact zeros -- parameters,
            // feature maps (the scatter skips zero weights anyway) and points alike.  The forward's render instantiations skip the same pairs.
            if (a.skip_masked && __ballot(m != 0.f) == 0ull) continue;
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
            // ---- forward recompute
            float h1[NBR][8], h2[NBR][8], o5[5];
            f4 acc[2];
            P8 frp;
            if constexpr (BP) frp = split8<0>(FR);
#pragma unroll
            for (int br = 0; br < NBR; ++br) {
                load_bias<2>(lds + o_b1(br), g, acc);
                if constexpr (BP) { mm16<1, 2, true>(lds + o_dec1(br), lane, &frp, acc); elu_to<2, false>(acc, h1[br]); }
                else { mm<8, 2>(lds + o_dec1(br), lane, FR, acc); elu_to<2>(acc, h1[br]); }
                load_bias<2>(lds + o_b2(br), g, acc);
                if constexpr (BP) { const P8U hp = split8u<0>(h1[br]); mm16u<1, 2, true>(lds + o_dec2(br), lane, &hp, acc); }
                else mm<8, 2>(lds + o_dec2(br), lane, h1[br], acc);
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
            // r: the logistic CDFs; with use_vis both edges of both components are multiplied by the vis_decoder's sigmoid
            // (dist_decoder.py:133-134): c = pv * r
            const float r00 = 0.5f + 0.5f * tanh1((nearv - mean0) * var0), r01 = 0.5f + 0.5f * tanh1((nearv - mean1) * var1);
            const float r10 = 0.5f + 0.5f * tanh1((farv - mean0) * var0), r11 = 0.5f + 0.5f * tanh1((farv - mean1) * var1);
            float pv = 1.f;
            if constexpr (USEVIS) pv = sigmoid1(gsum(dot8(lds + l1::V_T3, g, h2[3])) + lds[l1::V_SC]);
            const float c00 = r00 * pv, c01 = r01 * pv, c10 = r10 * pv, c11 = r11 * pv;
            const float vis = ((1.f - c00) * aw + (1.f - c01) * (1.f - aw)) * m;
            const float hit = ((c10 - c00) * aw + (c11 - c01) * (1.f - aw)) * m;
            float e1[8], e[8];
            P8 e1p;
            const float hitp = (hit - 0.5f) * 2.f, visp = (vis - 0.5f) * 2.f;
            {
                load_bias<2>(lds + l1::B_PE1, g, acc);
                if constexpr (BP) mm16<1, 2, true>(lds + l1::PE1, lane, &frp, acc);
                else mm<8, 2>(lds + l1::PE1, lane, FR, acc);
                const float extra[1] = {g == 0 ? hitp : (g == 1 ? visp : 0.f)};
                mm<1, 2, 8>(lds + l1::PE1, lane, extra, acc);          // (the C16 slot keeps this k-step as an fp32 fragment at the same offset)
                e1[0] = fmaxf(acc[0].x, 0.f); e1[1] = fmaxf(acc[0].y, 0.f); e1[2] = fmaxf(acc[0].z, 0.f); e1[3] = fmaxf(acc[0].w, 0.f);
                e1[4] = fmaxf(acc[1].x, 0.f); e1[5] = fmaxf(acc[1].y, 0.f); e1[6] = fmaxf(acc[1].z, 0.f); e1[7] = fmaxf(acc[1].w, 0.f);
                load_bias<2>(lds + l1::B_PE2, g, acc);
                if constexpr (BP) { e1p = split8<0>(e1); mm16<1, 2, true>(lds + l1::PE2F, lane, &e1p, acc); }
                else mm<8, 2>(lds + l1::PE2F, lane, e1, acc);
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
                if constexpr (BP) { mm16<1, 1, true>(lds + l1::NR1, lane, &e1p, acc1); elu_to<1, false>(acc1, n1t); }
                else { mm<8, 1>(lds + l1::NR1, lane, e1, acc1); elu_to<1>(acc1, n1t); }
            }
            const float gate = sigmoid1(gsum(dot4(lds + l1::T_NR2, g, n1t)) + lds[l1::SC + 0]);
            // ---- upstream
            float dX[9], de[8];
            const float* dsp = a.dS1 + ((size_t)tile * V + v) * DS1 * 64 + lane;
#pragma unroll
            for (int j = 0; j < 9; ++j) dX[j] = dsp[j * 64];
#pragma unroll
            for (int j = 0; j < 8; ++j) de[j] = dsp[(9 + j) * 64];
            float dgate = dsp[17 * 64];
            // the (tile, view)'s upstream gradient normalised by a power of two (grad_scale): gs in, gi = 1 / gs back out
            float gs = 1.f, gi = 1.f;
            if constexpr (BP) {
                float am = fabsf(dgate);
#pragma unroll
                for (int j = 0; j < 9; ++j) am = fmaxf(am, fabsf(dX[j]));
#pragma unroll
                for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(de[j]));
                grad_scale(am, gs, gi);
#pragma unroll
                for (int j = 0; j < 9; ++j) dX[j] *= gs;
#pragma unroll
                for (int j = 0; j < 8; ++j) de[j] *= gs;
                dgate *= gs;
            }
            // ---- ray_dir_fc.2 / .0   (x = [rgb, img feats] + ray_dir_fc(dir diff): d df = d x)
            {
                float da9[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) { da9[j] = dX[j] * elu_grad_t(dft[j]); gbr2[j] = fmaf(da9[j], gi, gbr2[j]); }
                wave_sync();
#pragma unroll
                for (int j = 0; j < 8; ++j) Ta[r * TS2 + 3 + 8 * g + j] = da9[j] * gi;
                if (g < 3) Ta[r * TS2 + g] = da9[8] * gi;
                if (g == 3) {
#pragma unroll
                    for (int c = 35; c < 48; ++c) Ta[r * TS2 + c] = 0.f;
                }
                tile_put_nat<1>(Tb, r, g, d1t, kLn2);
                wave_sync();
                outer_acc<3, 1>(Ta, Tb, lane, gWr2);
                f4 acc1[1] = {f4{0.f, 0.f, 0.f, 0.f}};
                mm<9, 1>(lds + l1::RDF2T, lane, da9, acc1);
                float da4[4] = {acc1[0].x * elu_grad_t(d1t[0]), acc1[0].y * elu_grad_t(d1t[1]), acc1[0].z * elu_grad_t(d1t[2]), acc1[0].w * elu_grad_t(d1t[3])};
#pragma unroll
                for (int j = 0; j < 4; ++j) gbr1[j] = fmaf(da4[j], gi, gbr1[j]);
                wave_sync();
                tile_put_nat<1>(Ta, r, g, da4, gi);
                Tb[r * TS2 + g] = ddg[0];
                Tb[r * TS2 + 4 + 3 * g] = 0.f; Tb[r * TS2 + 5 + 3 * g] = 0.f; Tb[r * TS2 + 6 + 3 * g] = 0.f;
                wave_sync();
                outer_acc<1, 1>(Ta, Tb, lane, gWr1);
            }
            // ---- neuray_fc gate
            {
                const float dz = dgate * gate * (1.f - gate);
                if (g == 0) gbnr2 = fmaf(dz, gi, gbnr2);
                float da4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gWnr2[j] = fmaf(dz * gi, n1t[j] * kLn2, gWnr2[j]);
                    da4[j] = lds[l1::T_NR2 + g * 4 + j] * kLog2e * dz * elu_grad_t(n1t[j]);
                    gbnr0[j] = fmaf(da4[j], gi, gbnr0[j]);
                }
                wave_sync();
                tile_put_nat<1>(Ta, r, g, da4, gi);
                tile_put_nat<2>(Tb, r, g, e, 1.f);
                wave_sync();
                outer_acc<1, 2>(Ta, Tb, lane, gWnr0);
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                mm<4, 2>(lds + l1::NR0T, lane, da4, acc);
                de[0] += acc[0].x; de[1] += acc[0].y; de[2] += acc[0].z; de[3] += acc[0].w;
                de[4] += acc[1].x; de[5] += acc[1].y; de[6] += acc[1].z; de[7] += acc[1].w;
            }
            // ---- prob_embed.2, prob_embed.0
            float dFR[8], dhit, dvis;
            {
#pragma unroll
                for (int j = 0; j < 8; ++j) gbpe2[j] = fmaf(de[j], gi, gbpe2[j]);
                wave_sync();
                tile_put_nat<2>(Ta, r, g, de, gi);
                tile_put_nat<2>(Tb, r, g, e1, 1.f);
                wave_sync();
                outer_acc<2, 2>(Ta, Tb, lane, gWpe2);
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                if constexpr (BP) mm16g<1, 2>(lds + l1::PE2T, lane, de, acc);
                else mm<8, 2>(lds + l1::PE2T, lane, de, acc);
                float da[8] = {acc[0].x, acc[0].y, acc[0].z, acc[0].w, acc[1].x, acc[1].y, acc[1].z, acc[1].w};
                float sh = 0.f, sv = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    da[j] = e1[j] > 0.f ? da[j] : 0.f;                      // ReLU'
                    gbpe0[j] = fmaf(da[j], gi, gbpe0[j]);
                    sh = fmaf(lds[l1::T_PE0HV + g * 8 + j], da[j], sh);
                    sv = fmaf(lds[l1::T_PE0HV + 32 + g * 8 + j], da[j], sv);
                }
                dhit = 2.f * gsum(sh); dvis = 2.f * gsum(sv);
                wave_sync();
                tile_put_nat<2>(Ta, r, g, da, gi);
                *reinterpret_cast<f4*>(Tb + r * TS2 + 8 * g) = f4{FR[0], FR[1], FR[2], FR[3]};
                *reinterpret_cast<f4*>(Tb + r * TS2 + 8 * g + 4) = f4{FR[4], FR[5], FR[6], FR[7]};
                if (g == 0) { Tb[r * TS2 + 32] = hitp; Tb[r * TS2 + 33] = visp; }
                if (g == 1) {
#pragma unroll
                    for (int c = 34; c < 48; ++c) Tb[r * TS2 + c] = 0.f;
                }
                wave_sync();
                outer_acc<2, 3>(Ta, Tb, lane, gWpe0);
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                if constexpr (BP) mm16g<1, 2>(lds + l1::PE0T, lane, da, acc);
                else mm<8, 2>(lds + l1::PE0T, lane, da, acc);
                dFR[0] = acc[0].x; dFR[1] = acc[0].y; dFR[2] = acc[0].z; dFR[3] = acc[0].w;
                dFR[4] = acc[1].x; dFR[5] = acc[1].y; dFR[6] = acc[1].z; dFR[7] = acc[1].w;
            }
            // ---- hit / vis -> decoder outputs (dist_decoder.py:109-142)
            float do5[NROW];
            {
                const float daw = m * (dvis * ((1.f - c00) - (1.f - c01)) + dhit * ((c10 - c00) - (c11 - c01)));
                const float dc00 = m * aw * (-dvis - dhit), dc01 = m * (1.f - aw) * (-dvis - dhit);
                const float dc10 = m * aw * dhit, dc11 = m * (1.f - aw) * dhit;
                const float du00 = dc00 * pv * 2.f * r00 * (1.f - r00), du01 = dc01 * pv * 2.f * r01 * (1.f - r01);
                const float du10 = dc10 * pv * 2.f * r10 * (1.f - r10), du11 = dc11 * pv * 2.f * r11 * (1.f - r11);
                if constexpr (USEVIS) do5[5] = (dc00 * r00 + dc01 * r01 + dc10 * r10 + dc11 * r11) * pv * (1.f - pv);
                const float dmean0 = -var0 * (du00 + du10), dmean1 = -var1 * (du01 + du11);
                const float dvar0 = (nearv - mean0) * du00 + (farv - mean0) * du10, dvar1 = (nearv - mean1) * du01 + (farv - mean1) * du11;
                do5[0] = dmean0 * sigmoid1(o5[0]); do5[1] = dmean1 * sigmoid1(o5[1]);
                do5[2] = dvar0 * sigmoid1(o5[2]); do5[3] = dvar1 * sigmoid1(o5[3]);
                do5[4] = daw * aw * (1.f - aw);
                if (g == 0) {
#pragma unroll
                    for (int q = 0; q < NROW; ++q) gb3[q] = fmaf(do5[q], gi, gb3[q]);
                }
            }
#pragma unroll
            for (int br = 0; br < NBR; ++br) {
                const int r0 = br < 3 ? 2 * br : 5, nrow = br < 2 ? 2 : 1;
                float da2[8], da1[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float dh = 0.f;
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        if (q < nrow) {
                            dh = fmaf(lds[(br < 3 ? l1::T_DEC3 + (r0 + q) * 32 : l1::V_T3) + g * 8 + j] * kLog2e, do5[r0 + q], dh);
                            gW3[r0 + q][j] = fmaf(do5[r0 + q] * gi, h2[br][j] * kLn2, gW3[r0 + q][j]);
                        }
                    da2[j] = dh * elu_grad_t(h2[br][j]);
                    gbd2[br][j] = fmaf(da2[j], gi, gbd2[br][j]);
                }
                wave_sync();
                tile_put_nat<2>(Ta, r, g, da2, gi);
                tile_put_nat<2>(Tb, r, g, h1[br], kLn2);
                wave_sync();
                outer_acc<2, 2>(Ta, Tb, lane, gWd2[br]);
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                if constexpr (BP) mm16g<1, 2>(lds + o_dec2t(br), lane, da2, acc);
                else mm<8, 2>(lds + o_dec2t(br), lane, da2, acc);
                const float dh1[8] = {acc[0].x, acc[0].y, acc[0].z, acc[0].w, acc[1].x, acc[1].y, acc[1].z, acc[1].w};
#pragma unroll
                for (int j = 0; j < 8; ++j) { da1[j] = dh1[j] * elu_grad_t(h1[br][j]); gbd1[br][j] = fmaf(da1[j], gi, gbd1[br][j]); }
                wave_sync();
                tile_put_nat<2>(Ta, r, g, da1, gi);
                *reinterpret_cast<f4*>(Tb + r * TS2 + 8 * g) = f4{FR[0], FR[1], FR[2], FR[3]};
                *reinterpret_cast<f4*>(Tb + r * TS2 + 8 * g + 4) = f4{FR[4], FR[5], FR[6], FR[7]};
                wave_sync();
                outer_acc<2, 2>(Ta, Tb, lane, gWd1[br]);
                acc[0] = f4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
                if constexpr (BP) mm16g<1, 2>(lds + o_dec1t(br), lane, da1, acc);
                else mm<8, 2>(lds + o_dec1t(br), lane, da1, acc);
                dFR[0] += acc[0].x; dFR[1] += acc[0].y; dFR[2] += acc[0].z; dFR[3] += acc[0].w;
                dFR[4] += acc[1].x; dFR[5] += acc[1].y; dFR[6] += acc[1].z; dFR[7] += acc[1].w;
            }
            // ---- scatter: ray channels 8g + j <- dFR, image-feature channels 32 + 8g + j <- d x (slots 0..7).
            // Through an LDS tile so that one wavefront instruction adds the 64 channels of ONE feature-map pixel
            // (a single 256-byte line) instead of 4 channels of 16 pixels.
            wave_sync();
            *reinterpret_cast<f4*>(Ta + r * TS2 + 8 * g) = f4{dFR[0] * gi, dFR[1] * gi, dFR[2] * gi, dFR[3] * gi};
            *reinterpret_cast<f4*>(Ta + r * TS2 + 8 * g + 4) = f4{dFR[4] * gi, dFR[5] * gi, dFR[6] * gi, dFR[7] * gi};
            *reinterpret_cast<f4*>(Ta + r * TS2 + 32 + 8 * g) = f4{dX[0] * gi, dX[1] * gi, dX[2] * gi, dX[3] * gi};
            *reinterpret_cast<f4*>(Ta + r * TS2 + 32 + 8 * g + 4) = f4{dX[4] * gi, dX[5] * gi, dX[6] * gi, dX[7] * gi};
            if (g == 0) {
                const bool live = row_ok && m != 0.f;
                *reinterpret_cast<f4*>(Tb + r * TS2) = f4{live ? w00 : 0.f, live ? w01 : 0.f, live ? w10 : 0.f, live ? w11 : 0.f};
                int* ip = reinterpret_cast<int*>(Tb + r * TS2 + 4);
                ip[0] = t.o00; ip[1] = t.o01; ip[2] = t.o10; ip[3] = t.o11;
            }
            wave_sync();
            {
                const size_t gbase = (size_t)bv * a.fh * a.fw * 64 + lane;
                const float fxs = FX ? fx_scale(a.fx) : 0.f;
                for (int pp = 0; pp < 16; ++pp) {
                    const float val = Ta[pp * TS2 + lane];
                    const f4 wq = *reinterpret_cast<const f4*>(Tb + pp * TS2);
                    const int* ip = reinterpret_cast<const int*>(Tb + pp * TS2 + 4);
                    if (wq.x != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[0] * 64, val * wq.x, fxs, a.fx.flag);
                    if (wq.y != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[1] * 64, val * wq.y, fxs, a.fx.flag);
                    if (wq.z != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[2] * 64, val * wq.z, fxs, a.fx.flag);
                    if (wq.w != 0.f) feat_add<FX>(a.dfeat64, gbase + (size_t)ip[3] * 64, val * wq.w, fxs, a.fx.flag);
                }
            }
        }
        wave_sync();
    }
    // ---- flush
    float* gc = grad_slot(a.dpart, GP_STRIDE);
    // (the vis branch's slots lie behind the level's blob: d_canonical of a use_vis level has can::TOTAL_VIS floats)
    const int d0w[4] = {can::MEAN0_W, can::VAR0_W, can::AW0_W, can::VISD0_W}, d0b[4] = {can::MEAN0_B, can::VAR0_B, can::AW0_B, can::VISD0_B};
    const int d2w[4] = {can::MEAN2_W, can::VAR2_W, can::AW2_W, can::VISD2_W}, d2b[4] = {can::MEAN2_B, can::VAR2_B, can::AW2_B, can::VISD2_B};
    const int d4w[6] = {can::MEAN4_W, can::MEAN4_W + 32, can::VAR4_W, can::VAR4_W + 32, can::AW4_W, can::VISD4_W};
    const int d4b[6] = {can::MEAN4_B, can::MEAN4_B + 1, can::VAR4_B, can::VAR4_B + 1, can::AW4_B, can::VISD4_B};
#pragma unroll
    for (int br = 0; br < NBR; ++br) {
        flush_blocks<2, 2>(gc + d0w[br], 32, 32, 32, lane, gWd1[br]);
        flush_blocks<2, 2>(gc + d2w[br], 32, 32, 32, lane, gWd2[br]);
    }
    flush_blocks<2, 3>(gc + can::PE0_W, 34, 32, 34, lane, gWpe0);
    flush_blocks<2, 2>(gc + can::PE2_W, 32, 32, 32, lane, gWpe2);
    flush_blocks<1, 2>(gc + can::NR0_W, 32, 8, 32, lane, gWnr0);
    flush_blocks<3, 1>(gc + can::RDF2_W, 16, 35, 16, lane, gWr2);
    flush_blocks<1, 1>(gc + can::RDF0_W, 4, 16, 4, lane, gWr1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int f = 16 * (j / 4) + 4 * g + (j % 4);
#pragma unroll
        for (int br = 0; br < NBR; ++br) {
            const float s1 = rsum16(gbd1[br][j]), s2 = rsum16(gbd2[br][j]);
            if (r == 0) { gc[d0b[br] + f] = s1; gc[d2b[br] + f] = s2; }
        }
#pragma unroll
        for (int q = 0; q < NROW; ++q) {
            const float s = rsum16(gW3[q][j]);
            if (r == 0) gc[d4w[q] + f] = s;
        }
        const float s3 = rsum16(gbpe0[j]), s4 = rsum16(gbpe2[j]);
        if (r == 0) { gc[can::PE0_B + f] = s3; gc[can::PE2_B + f] = s4; }
    }
#pragma unroll
    for (int q = 0; q < NROW; ++q) {
        const float s = rsum16(gb3[q]);
        if (lane == 0) gc[d4b[q]] = s;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float s0 = rsum16(gbnr0[j]), s1 = rsum16(gWnr2[j]), s2 = rsum16(gbr1[j]);
        if (r == 0) {
            if (4 * g + j < 8) { gc[can::NR0_B + 4 * g + j] = s0; gc[can::NR2_W + 4 * g + j] = s1; }
            gc[can::RDF0_B + 4 * g + j] = s2;
        }
    }
    {
        const float s = rsum16(gbnr2);
        if (lane == 0) gc[can::NR2_B] = s;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const float s = rsum16(gbr2[j]);
        if (r == 0) {
            if (j < 8) gc[can::RDF2_B + 3 + 8 * g + j] = s;
            else if (g < 3) gc[can::RDF2_B + g] = s;
        }
    }
}

}  // namespace gnr


#include "gnr_bwd_view1_pw.inc"
#include "gnr_bwd_view2_pw.inc"

// =========================================================================================================
// Render path, per-view chain: everything up to the cross-view statistics and the colour blend.  The per-ray tail and
// the compositing have their own kernels further down (k_ray_dual_bwd, k_composite_bwd).
// k_stats_unpack: the chain's statistics -> [P][66] (mean 32, var 32, wbar, number of valid views), true scale.
// k_red2_bwd:     d(mean, var, wbar), d colours -> d(h_v, v2_v, colour logit_v)  (second reduction + colour blend)
// =========================================================================================================
namespace gnr {

__global__ void k_stats_unpack(const float* __restrict__ saveZ, float* __restrict__ stats, int P, int ntiles) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    if (tile >= ntiles) return;
    const int tps = (P + 15) >> 4, b = tile / tps, n = (tile - b * tps) * 16 + r;
    if (n >= P) return;
    const float* sp = saveZ + (size_t)tile * 18 * 64 + lane;
    float* o = stats + ((size_t)b * P + n) * 66;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int f = 16 * (j / 4) + 4 * g + (j % 4);
        o[f] = sp[j * 64] * kLn2;
        o[32 + f] = sp[(8 + j) * 64] * kLn2 * kLn2;
    }
    if (g == 0) { o[64] = sp[16 * 64]; o[65] = sp[17 * 64]; }
}

struct Red2BwdArgs {
    const float* save2;       // [tiles][V][11][64]
    const float* dstats;      // [B*P][65]  d mean, d var, d wbar
    const float* dcolors;     // [B*P][3]
    float* dS2;               // [tiles][V][10][64]
    int P, ntiles;
};

template <int V>
__global__ __launch_bounds__(256) void k_red2_bwd(Red2BwdArgs a) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    if (tile >= a.ntiles) return;
    const int tps = (a.P + 15) >> 4, b = tile / tps, n_raw = (tile - b * tps) * 16 + r;
    const bool row_ok = n_raw < a.P;
    const size_t pt = (size_t)b * a.P + min(n_raw, a.P - 1);
    float S2[V][11];
    const float* sp = a.save2 + (size_t)tile * V * 11 * 64 + lane;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int q = 0; q < 11; ++q) S2[v][q] = sp[(v * 11 + q) * 64];
    float vsum = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) vsum += S2[v][8];
    const float inv_vsum = rcp1(vsum + 1e-8f);
    float mu[8], dmu[8], dva[8];
    const float* ds = a.dstats + pt * 65;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float m = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) m += S2[v][j] * (S2[v][8] * inv_vsum);
        mu[j] = m;
        const int f = 16 * (j / 4) + 4 * g + (j % 4);
        dmu[j] = row_ok ? ds[f] : 0.f;
        dva[j] = row_ok ? ds[32 + f] : 0.f;
    }
    const float dwbar = row_ok ? ds[64] : 0.f;
    // colour blend: colour_c = sum_v softmax_v(logit) rgb_v,c ; lane group g < 3 holds channel g
    float cmax = -3.0e38f;
#pragma unroll
    for (int v = 0; v < V; ++v) cmax = fmaxf(cmax, S2[v][9]);
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) { const float e = __expf(S2[v][9] - cmax); den += e; num += S2[v][10] * e; }
    const float iden = rcp1(den), col = num * iden;
    const float dcol = (row_ok && g < 3) ? a.dcolors[pt * 3 + g] : 0.f;
    float dwp[V], accw = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float h = S2[v][j] * kLn2, d = (S2[v][j] - mu[j]) * kLn2;
            s = fmaf(dmu[j], h, s);
            s = fmaf(dva[j], d * d, s);
        }
        dwp[v] = gsum(s) + dwbar * (1.f / (float)V);
        accw = fmaf(S2[v][8] * inv_vsum, dwp[v], accw);
    }
    float* dp = a.dS2 + (size_t)tile * V * 10 * 64 + lane;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float wv = S2[v][8] * inv_vsum;
#pragma unroll
        for (int j = 0; j < 8; ++j) dp[(v * 10 + j) * 64] = wv * fmaf(2.f * (S2[v][j] - mu[j]) * kLn2, dva[j], dmu[j]);
        dp[(v * 10 + 8) * 64] = inv_vsum * (dwp[v] - accw);
        const float pv = __expf(S2[v][9] - cmax) * iden;
        dp[(v * 10 + 9) * 64] = gsum(dcol * pv * (S2[v][10] - col));
    }
}

}  // namespace gnr

// =========================================================================================================
// Render path, per-ray tail: reverse pass over [+posenc, attention, fc + residual, LayerNorm, folded out_geometry_fc,
// clip / mask] evaluated on DUAL numbers (value, derivative along gamma = dL / d sdf-gradient).  This is the second-order
// path of the reference's in-forward `autograd.grad(..., create_graph=True)` (ibrnet.py:497-504) without a double-backward
// graph:   Phi = sum_i a_i sdf_i + <gamma, d sum(sdf) / d p>  =  sum_i a_i sdf_i + d/d eps sum_i sdf_i(p + eps gamma),
// so every op is reversed for its value adjoint and for its tangent adjoint, plus the cross terms of the non-linear ops
// (softmax Jacobian, LayerNorm's 1/sigma).  graspnerf_amd/ray_tail.py::attn_core is the same algebra in tensor form.
//   in : g, gd [rays*dn][16] value / tangent of geometry_fc's output, a [rays*dn] = dL/d sdf, nvalid [rays*dn]
//   out: gbar, gdbar [rays*dn][16]; the tail's parameter gradients as per-wavefront partials (layout tp::)
// Row statistics that look like extra key sweeps collapse:  c_i = sum_j Pdbar_ij P_ij = odbar_i . o_i  and
// d_i = sum_j P_ij Pbar2_ij = obar_i . o_i + odbar_i . od_i - c_i r_i   (per head), so a ray costs two row sweeps
// (forward value + tangent; q adjoints) and one column sweep (k, v adjoints).  Lane packing of k_ray / k_ray_bwd.
// =========================================================================================================
namespace gnr {

struct RayDualArgs {
    const float* wpk; const float* g; const float* gd; const float* a; const float* nvalid;
    float* gbar; float* gdbar; float* dpart;          // dpart: as RayBwdArgs
    int nrays, dn, rays_per_block, ray_stride, nblocks;
};
namespace dl { constexpr int PER = 148, ST = 20; }      // LDS floats per sample: K Kd V Vd Q Qd Ob Odb (8 x 16) + 20 row statistics

DEV float dot4(const f4 a, const float* __restrict__ b) { return a.x * b[0] + a.y * b[1] + a.z * b[2] + a.w * b[3]; }
DEV float dot4(const f4 a, const f4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
DEV void axpy4(float s, const f4 v, float* __restrict__ acc) {
    acc[0] = fmaf(s, v.x, acc[0]); acc[1] = fmaf(s, v.y, acc[1]); acc[2] = fmaf(s, v.z, acc[2]); acc[3] = fmaf(s, v.w, acc[3]);
}
// y[f] = sum_c M[f*16 + c] x[c]
DEV void matvec16(const float* __restrict__ M, const float (&x)[16], float (&y)[16]) {
#pragma unroll
    for (int f = 0; f < 16; ++f) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) s = fmaf(M[f * 16 + c], x[c], s);
        y[f] = s;
    }
}
DEV void put16(float* __restrict__ dst, const float (&x)[16]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) reinterpret_cast<f4*>(dst)[c] = f4{x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]};
}
DEV void get16(const float* __restrict__ src, float (&x)[16]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const f4 v = reinterpret_cast<const f4*>(src)[c];
        x[4 * c] = v.x; x[4 * c + 1] = v.y; x[4 * c + 2] = v.z; x[4 * c + 3] = v.w;
    }
}

__global__ __launch_bounds__(256, 1) void k_ray_dual_bwd(RayDualArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int dn = a.dn, S = dn, rpb = a.rays_per_block;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rl = (int)threadIdx.x / S;
    const int slot = (int)threadIdx.x - rl * S;
    const bool in_blk = rl < rpb;
    rl = min(rl, rpb - 1);
    const int i = min(slot, dn - 1);
    float* sc = sm + (size_t)rl * a.ray_stride;
    float* Kb = sc; float* Kd = sc + dn * 16; float* Vb = sc + dn * 32; float* Vd = sc + dn * 48;
    float* Qb = sc + dn * 64; float* Qd = sc + dn * 80; float* Ob = sc + dn * 96; float* Od = sc + dn * 112;
    float* St = sc + dn * 128;
    float* KN = Ob;
    const float* W = a.wpk;
    f4 gacc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) gacc[m] = f4{0.f, 0.f, 0.f, 0.f};
    // M[c] = sum ds xhat_c (+ the tangent part in the dual kernel), S = sum ds, in double from the lane on: thousands of O(1)
    // terms of either sign; dLNw = w_eff M, dLNb = w_eff S, d w_eff = LNw M + LNb S follow in k_tail_finish
    double gM[16], gS = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) gM[c] = 0.0;

    for (int blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        const int ray_u = blk * rpb + rl;
        const bool rvalid = in_blk && ray_u < a.nrays;
        const int ray = min(ray_u, a.nrays - 1);
        const bool act = rvalid && slot < dn;
        const size_t pt = (size_t)ray * dn + i;
        float t[16], td[16];
        get16(a.g + pt * 16, t);
        get16(a.gd + pt * 16, td);
#pragma unroll
        for (int c = 0; c < 16; ++c) t[c] += W[pk::R_PE + i * 16 + c];
        const float nvalid = a.nvalid[pt];
        const bool rowok = nvalid > 1.f;
        float q[16], qd[16];
        matvec16(W + pk::R_WQ, t, q);
        matvec16(W + pk::R_WQ, td, qd);
        __syncthreads();                                  // previous iteration's MFMA tiles are dead
        {
            float kk[16], kd[16], vv[16], vd[16];
            matvec16(W + pk::R_WK, t, kk);
            matvec16(W + pk::R_WK, td, kd);
            matvec16(W + pk::R_WV, t, vv);
            matvec16(W + pk::R_WV, td, vd);
            // every lane of the workgroup fills its slot: see k_ray_bwd (the MFMAs contract over all 256 lanes)
            if (in_blk) {
                put16(Kb + i * 16, kk); put16(Kd + i * 16, kd); put16(Vb + i * 16, vv); put16(Vd + i * 16, vd);
                put16(Qb + i * 16, q); put16(Qd + i * 16, qd);
#pragma unroll
                for (int h = 0; h < 4; ++h)
                    KN[i * 16 + h] = kk[4 * h] * kk[4 * h] + kk[4 * h + 1] * kk[4 * h + 1] + kk[4 * h + 2] * kk[4 * h + 2] + kk[4 * h + 3] * kk[4 * h + 3];
            }
        }
        __syncthreads();
        float amax[4];
        {
            f4 kmax = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < dn; ++j) {
                const f4 n = *reinterpret_cast<const f4*>(KN + j * 16);
                kmax.x = fmaxf(kmax.x, n.x); kmax.y = fmaxf(kmax.y, n.y); kmax.z = fmaxf(kmax.z, n.z); kmax.w = fmaxf(kmax.w, n.w);
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float qn = q[4 * h] * q[4 * h] + q[4 * h + 1] * q[4 * h + 1] + q[4 * h + 2] * q[4 * h + 2] + q[4 * h + 3] * q[4 * h + 3];
                amax[h] = rowok ? 0.5f * sqrtf(qn * kmax[h]) : -1e9f;
            }
        }
        // ---- forward on dual numbers: o = P v,  r = sum_j P Sd,  od = sum_j P Sd v - r o + sum_j P vd
        float o[16], od[16], ainv[4], rr[4];
        {
            float l[4], ru[4], U[16], Pv[16];
            auto sweep = [&]() {
#pragma unroll
                for (int h = 0; h < 4; ++h) { l[h] = 0.f; ru[h] = 0.f; }
#pragma unroll
                for (int f = 0; f < 16; ++f) { o[f] = 0.f; U[f] = 0.f; Pv[f] = 0.f; }
                for (int j = 0; j < dn; ++j) {
                    float sj[4];
                    head_logits(q, Kb + j * 16, rowok, sj);
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const f4 kj = reinterpret_cast<const f4*>(Kb + j * 16)[h], kdj = reinterpret_cast<const f4*>(Kd + j * 16)[h];
                        const f4 vj = reinterpret_cast<const f4*>(Vb + j * 16)[h], vdj = reinterpret_cast<const f4*>(Vd + j * 16)[h];
                        const float sd = rowok ? 0.5f * (dot4(kj, qd + 4 * h) + dot4(kdj, q + 4 * h)) : 0.f;
                        const float pj = __expf(sj[h] - amax[h]);
                        l[h] += pj;
                        ru[h] = fmaf(pj, sd, ru[h]);
                        axpy4(pj, vj, o + 4 * h);
                        axpy4(pj * sd, vj, U + 4 * h);
                        axpy4(pj, vdj, Pv + 4 * h);
                    }
                }
            };
            sweep();
            if (!(fminf(fminf(l[0], l[1]), fminf(l[2], l[3])) > 1e-30f)) {
#pragma unroll
                for (int h = 0; h < 4; ++h) amax[h] = -3.0e38f;
                for (int j = 0; j < dn; ++j) {
                    float sj[4];
                    head_logits(q, Kb + j * 16, rowok, sj);
#pragma unroll
                    for (int h = 0; h < 4; ++h) amax[h] = fmaxf(amax[h], sj[h]);
                }
                sweep();
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                ainv[h] = 1.f / l[h];
                rr[h] = ru[h] * ainv[h];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int f = 4 * h + u;
                    o[f] *= ainv[h];
                    od[f] = (U[f] + Pv[f]) * ainv[h] - rr[h] * o[f];
                }
            }
        }
        // ---- fc + residual, LayerNorm on dual numbers
        float ybar[16], ydbar[16];
        {
            float y[16], yd[16];
            matvec16(W + pk::R_WFC, o, y);
            matvec16(W + pk::R_WFC, od, yd);
            float mean = 0.f, meand = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) { y[c] += t[c]; yd[c] += td[c]; mean += y[c]; meand += yd[c]; }
            mean *= (1.f / 16.f); meand *= (1.f / 16.f);
            float var = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) { y[c] -= mean; yd[c] -= meand; var = fmaf(y[c], y[c], var); }     // y := c, yd := cd
            var *= (1.f / 16.f);
            const float rs = 1.f / sqrtf(var + 1e-6f);
            float xh[16], xhd[16], m1 = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) { xh[c] = y[c] * rs; m1 = fmaf(xh[c], yd[c], m1); }
            m1 *= (1.f / 16.f);
            float u = W[pk::R_OUTB];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                xhd[c] = rs * (yd[c] - xh[c] * m1);
                u = fmaf(W[pk::R_OUTVJP + c], xh[c] * W[pk::R_LNW + c] + W[pk::R_LNB + c], u);
            }
            const bool live = act && u >= -1.f && u <= 1.f && nvalid >= 1.f;
            const float sbar = live ? a.a[pt] : 0.f, sdbar = live ? 1.f : 0.f;
            gS += (double)sbar;
            float xhbar[16], e[16], E1 = 0.f, rsbar = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const float we = W[pk::R_OUTVJP + c], lw = W[pk::R_LNW + c];
                const float nbar = sbar * we, ndbar = sdbar * we;
                gM[c] = fma((double)sbar, (double)xh[c], gM[c]);
                gM[c] = fma((double)sdbar, (double)xhd[c], gM[c]);
                xhbar[c] = lw * nbar;
                e[c] = lw * ndbar;
                E1 = fmaf(e[c], xh[c], E1);
                rsbar = fmaf(e[c], xhd[c], rsbar);
            }
            rsbar /= rs;
            const float E16 = E1 * (1.f / 16.f);
            float mcd = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                ydbar[c] = rs * (e[c] - xh[c] * E16);                       // cdbar
                mcd += ydbar[c];
                xhbar[c] -= rs * (m1 * e[c] + E16 * yd[c]);
                rsbar = fmaf(xhbar[c], y[c], rsbar);
            }
            mcd *= (1.f / 16.f);
            const float varbar = -0.5f * rs * rs * rs * rsbar;
            float mc = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                ydbar[c] -= mcd;
                ybar[c] = fmaf(rs, xhbar[c], (2.f / 16.f) * y[c] * varbar);   // cbar
                mc += ybar[c];
            }
            mc *= (1.f / 16.f);
#pragma unroll
            for (int c = 0; c < 16; ++c) ybar[c] -= mc;
        }
        float obar[16], odbar[16], cst[4], dd[4];
        matvec16(W + pk::R_WFCT, ybar, obar);
        matvec16(W + pk::R_WFCT, ydbar, odbar);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            float c1 = 0.f, d1 = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = 4 * h + u;
                c1 = fmaf(odbar[f], o[f], c1);
                d1 = fmaf(obar[f], o[f], d1);
                d1 = fmaf(odbar[f], od[f], d1);
            }
            cst[h] = c1; dd[h] = d1 - c1 * rr[h];
        }
        // ---- q adjoints: second row sweep
        float qbar[16], qdbar[16];
        {
#pragma unroll
            for (int f = 0; f < 16; ++f) { qbar[f] = 0.f; qdbar[f] = 0.f; }
            for (int j = 0; j < dn; ++j) {
                float sj[4];
                head_logits(q, Kb + j * 16, rowok, sj);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const f4 kj = reinterpret_cast<const f4*>(Kb + j * 16)[h], kdj = reinterpret_cast<const f4*>(Kd + j * 16)[h];
                    const f4 vj = reinterpret_cast<const f4*>(Vb + j * 16)[h], vdj = reinterpret_cast<const f4*>(Vd + j * 16)[h];
                    const float sd = 0.5f * (dot4(kj, qd + 4 * h) + dot4(kdj, q + 4 * h));
                    const float pj = __expf(sj[h] - amax[h]) * ainv[h];
                    const float pdb = dot4(vj, odbar + 4 * h);
                    const float pb = dot4(vj, obar + 4 * h) + dot4(vdj, odbar + 4 * h);
                    const float sdb = pj * (pdb - cst[h]);
                    const float sb = pj * (pb + pdb * (sd - rr[h]) - cst[h] * sd - dd[h]);
                    axpy4(sb, kj, qbar + 4 * h);
                    axpy4(sdb, kdj, qbar + 4 * h);
                    axpy4(sdb, kj, qdbar + 4 * h);
                }
            }
            const float sc2 = rowok ? 0.5f : 0.f;
#pragma unroll
            for (int f = 0; f < 16; ++f) { qbar[f] *= sc2; qdbar[f] *= sc2; }
        }
        __syncthreads();                                  // KN (aliases Ob) is dead
        if (in_blk) {
            put16(Ob + i * 16, obar);
            put16(Od + i * 16, odbar);
            f4* st = reinterpret_cast<f4*>(St + i * dl::ST);
            st[0] = f4{amax[0], amax[1], amax[2], amax[3]};
            st[1] = f4{rowok ? ainv[0] : -ainv[0], ainv[1], ainv[2], ainv[3]};
            st[2] = f4{rr[0], rr[1], rr[2], rr[3]};
            st[3] = f4{cst[0], cst[1], cst[2], cst[3]};
            st[4] = f4{dd[0], dd[1], dd[2], dd[3]};
        }
        __syncthreads();
        // ---- k, v adjoints: column sweep (this lane's key / value against every query row of its ray)
        float kbar[16], kdbar[16], vbar[16], vdbar[16];
        {
            float kk[16], kd[16], vv[16], vd[16];
            get16(Kb + i * 16, kk); get16(Kd + i * 16, kd); get16(Vb + i * 16, vv); get16(Vd + i * 16, vd);
#pragma unroll
            for (int f = 0; f < 16; ++f) { kbar[f] = 0.f; kdbar[f] = 0.f; vbar[f] = 0.f; vdbar[f] = 0.f; }
            for (int qi = 0; qi < dn; ++qi) {
                const f4* st = reinterpret_cast<const f4*>(St + qi * dl::ST);
                const f4 mx4 = st[0], rs4 = st[2], cs4 = st[3], dd4 = st[4];
                f4 il4 = st[1];
                const bool ok = il4.x > 0.f;
                il4.x = fabsf(il4.x);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const f4 qv = reinterpret_cast<const f4*>(Qb + qi * 16)[h], qdv = reinterpret_cast<const f4*>(Qd + qi * 16)[h];
                    const f4 ob = reinterpret_cast<const f4*>(Ob + qi * 16)[h], odb = reinterpret_cast<const f4*>(Od + qi * 16)[h];
                    float s = 0.5f * dot4(qv, kk + 4 * h);
                    s = ok ? s : -1e9f;
                    const float sd = ok ? 0.5f * (dot4(qdv, kk + 4 * h) + dot4(qv, kd + 4 * h)) : 0.f;
                    const float pj = __expf(s - mx4[h]) * il4[h];
                    const float pd = pj * (sd - rs4[h]);
                    const float pdb = dot4(odb, vv + 4 * h);
                    const float pb = dot4(ob, vv + 4 * h) + dot4(odb, vd + 4 * h);
                    const float sdb = ok ? 0.5f * pj * (pdb - cs4[h]) : 0.f;
                    const float sb = ok ? 0.5f * pj * (pb + pdb * (sd - rs4[h]) - cs4[h] * sd - dd4[h]) : 0.f;
                    axpy4(pj, ob, vbar + 4 * h);
                    axpy4(pd, odb, vbar + 4 * h);
                    axpy4(pj, odb, vdbar + 4 * h);
                    axpy4(sb, qv, kbar + 4 * h);
                    axpy4(sdb, qdv, kbar + 4 * h);
                    axpy4(sdb, qv, kdbar + 4 * h);
                }
            }
        }
        // gbar = tbar, gdbar = tdbar (residual + the three projections)
        if (act) {
            float* dg = a.gbar + pt * 16;
            float* dgd = a.gdbar + pt * 16;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                float r4v[4], r4d[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = 4 * c4 + u;
                    float s = ybar[c], sdv = ydbar[c];
#pragma unroll
                    for (int f = 0; f < 16; ++f) {
                        s = fmaf(W[pk::R_WQT + c * 16 + f], qbar[f], s);
                        s = fmaf(W[pk::R_WKT + c * 16 + f], kbar[f], s);
                        s = fmaf(W[pk::R_WVT + c * 16 + f], vbar[f], s);
                        sdv = fmaf(W[pk::R_WQT + c * 16 + f], qdbar[f], sdv);
                        sdv = fmaf(W[pk::R_WKT + c * 16 + f], kdbar[f], sdv);
                        sdv = fmaf(W[pk::R_WVT + c * 16 + f], vdbar[f], sdv);
                    }
                    r4v[u] = s; r4d[u] = sdv;
                }
                reinterpret_cast<f4*>(dg)[c4] = f4{r4v[0], r4v[1], r4v[2], r4v[3]};
                reinterpret_cast<f4*>(dgd)[c4] = f4{r4d[0], r4d[1], r4d[2], r4d[3]};
            }
        }
        // ---- weight gradients: dW[f][c] += sum_points (dY[f] X[c] + dYd[f] Xd[c]) as MFMAs with the 256 lanes as K
        float* TY = sm;                       // [256][16]   (the attention scratch is dead after the barrier)
        float* TX = sm + 256 * 16;            // [256][16]
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            __syncthreads();
            const float* dYm = m == 0 ? qbar : m == 1 ? qdbar : m == 2 ? kbar : m == 3 ? kdbar : m == 4 ? vbar : m == 5 ? vdbar : m == 6 ? ybar : ydbar;
            const float* Xm = m == 6 ? o : m == 7 ? od : (m & 1) ? td : t;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                reinterpret_cast<f4*>(TY + threadIdx.x * 16)[c] = act ? f4{dYm[4 * c], dYm[4 * c + 1], dYm[4 * c + 2], dYm[4 * c + 3]} : f4{0.f, 0.f, 0.f, 0.f};
                reinterpret_cast<f4*>(TX + threadIdx.x * 16)[c] = f4{Xm[4 * c], Xm[4 * c + 1], Xm[4 * c + 2], Xm[4 * c + 3]};
            }
            __syncthreads();
            const int c16 = lane & 15, kg = lane >> 4;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const int p = 64 * wave + 4 * s + kg;
                gacc[m >> 1] = mfma16(TY[p * 16 + c16], TX[p * 16 + c16], gacc[m >> 1]);
            }
        }
    }
    // ---- flush (layout tl::, as k_ray_bwd)
    {
        const int c16 = lane & 15, kg = lane >> 4;
        float* gt = grad_slot(a.dpart, tp::STRIDE);
#pragma unroll
        for (int m = 0; m < 4; ++m) {                     // dWq, dWk, dWv, dWfc at tp::W + 256 m (the order of tl::)
            const float e[4] = {gacc[m].x, gacc[m].y, gacc[m].z, gacc[m].w};
#pragma unroll
            for (int u = 0; u < 4; ++u) gt[tp::W + 256 * m + (4 * kg + u) * 16 + c16] = e[u];
        }
        double* gd = reinterpret_cast<double*>(gt + tp::MS);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const double s1 = wave_sum64d(gM[c]);
            if (lane == 0) gd[c] = s1;
        }
        const double ss = wave_sum64d(gS);
        if (lane == 0) gd[16] = ss;
    }
}

}  // namespace gnr

// =========================================================================================================
// Render path, NeuS alpha + compositing (aggregate_net.py:105-121, render_ops.py:72-80, renderer.py:110-123), backward.
// Forward values are k_ray<true>'s.  One thread per ray: a forward sweep rebuilds alpha_k and the exclusive transmittance
// T_k, a reverse sweep carries S_k = sum_{j>k} dT_j T_j (the closed form of cumprod's backward for positive factors).
//   upstream: dpix [R,3], ddepth [R] | null, wgerr [R] = d L / d sum_k (|grad_k| - 1)^2 of the ray, dalpha, dhit [R*dn] | null
//   out: a = dL/d sdf [R*dn], gamma = dL/d grad [R*dn,3] (the two upstreams of the per-ray tail), dcol [R*dn,3],
//        dvar[0] = dL/d deviation_network.variance (per-wavefront partials in double, added in a fixed order by k_dvar_finish)
// =========================================================================================================
namespace gnr {

struct CompBwdArgs {
    const float* wpk; const float *sdf, *grad, *col, *depth, *qdir;
    const float *dpix, *ddepth, *wgerr, *dalpha, *dhit;
    float *a_out, *gamma, *dcol;
    double* dvar_part;        // [blocks] per-wavefront partial of d deviation_network.variance (k_dvar_finish adds them in order)
    int nrays, dn;
};

__global__ __launch_bounds__(64) void k_composite_bwd(CompBwdArgs a) {
    const int ray_u = blockIdx.x * 64 + threadIdx.x;
    const bool live = ray_u < a.nrays;
    const int ray = min(ray_u, a.nrays - 1), dn = a.dn;
    const float var = a.wpk[pk::R_VARIANCE];
    const float es = __expf(var * 10.f);
    const float inv_s = fminf(fmaxf(es, 1e-6f), 1e6f);
    const float qd[3] = {a.qdir[ray * 3], a.qdir[ray * 3 + 1], a.qdir[ray * 3 + 2]};
    const size_t p0 = (size_t)ray * dn;
    float al[MAX_DN_FWD], Tk[MAX_DN_FWD];
    auto alpha_of = [&](int k, float& tcos, float& prv, float& nxt, float& pc, float& nc, float& dist) {
        const float* g = a.grad + (p0 + k) * 3;
        const float z = a.depth[p0 + k];
        dist = (k + 1 < dn) ? a.depth[p0 + k + 1] - z : 1e6f;
        tcos = -(qd[0] * g[0] + qd[1] * g[1] + qd[2] * g[2]);
        const float icos = fminf(tcos, 0.f), sdf = a.sdf[p0 + k];
        nxt = sdf + icos * dist * 0.5f; prv = sdf - icos * dist * 0.5f;
        pc = sigmoid1(prv * inv_s); nc = sigmoid1(nxt * inv_s);
        return (pc - nc + 1e-5f) / (pc + 1e-5f);
    };
    float T = 1.f;
    for (int k = 0; k < dn; ++k) {
        float tcos, prv, nxt, pc, nc, dist;
        const float r = alpha_of(k, tcos, prv, nxt, pc, nc, dist);
        const float alpha = fminf(fmaxf(r, 0.f), 1.f);
        al[k] = alpha; Tk[k] = T;
        T *= 1.f - alpha + 1e-10f;
    }
    const float dp[3] = {a.dpix[ray * 3], a.dpix[ray * 3 + 1], a.dpix[ray * 3 + 2]};
    const float dd = a.ddepth ? a.ddepth[ray] : 0.f, wg = a.wgerr ? a.wgerr[ray] : 0.f;
    float S = 0.f, dinv = 0.f;
    for (int k = dn - 1; k >= 0; --k) {
        const size_t pt = p0 + k;
        const float* c = a.col + pt * 3;
        const float* g = a.grad + pt * 3;
        const float hp = al[k] * Tk[k];
        const float dhp = dp[0] * c[0] + dp[1] * c[1] + dp[2] * c[2] + dd * a.depth[pt] + (a.dhit ? a.dhit[pt] : 0.f);
        float dal = dhp * Tk[k] + (a.dalpha ? a.dalpha[pt] : 0.f);
        dal -= S / (1.f - al[k] + 1e-10f);
        S = fmaf(dhp * al[k], Tk[k], S);
        float tcos, prv, nxt, pc, nc, dist;
        const float r = alpha_of(k, tcos, prv, nxt, pc, nc, dist);
        const float dr = (r >= 0.f && r <= 1.f) ? dal : 0.f;
        const float D = pc + 1e-5f;
        const float dN = dr / D, dD = -dr * (pc - nc + 1e-5f) / (D * D);
        const float dup = (dN + dD) * pc * (1.f - pc), dun = -dN * nc * (1.f - nc);      // d (prv*inv_s), d (nxt*inv_s)
        dinv = fmaf(dup, prv, fmaf(dun, nxt, dinv));
        const float dprv = dup * inv_s, dnxt = dun * inv_s;
        const float dtc = (tcos < 0.f) ? (dnxt - dprv) * dist * 0.5f : 0.f;
        const float gl = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
        const float ge = gl > 0.f ? wg * 2.f * (gl - 1.f) / gl : 0.f;
        if (live) {
            a.a_out[pt] = dprv + dnxt;
            a.gamma[pt * 3] = fmaf(ge, g[0], -qd[0] * dtc);
            a.gamma[pt * 3 + 1] = fmaf(ge, g[1], -qd[1] * dtc);
            a.gamma[pt * 3 + 2] = fmaf(ge, g[2], -qd[2] * dtc);
            a.dcol[pt * 3] = hp * dp[0]; a.dcol[pt * 3 + 1] = hp * dp[1]; a.dcol[pt * 3 + 2] = hp * dp[2];
        }
    }
    // inv_s = clip(exp(10 v), 1e-6, 1e6)
    const double dv = wave_sum64d((live && es >= 1e-6f && es <= 1e6f) ? (double)(dinv * 10.f * inv_s) : 0.0);
    if (threadIdx.x == 0) a.dvar_part[blockIdx.x] = dv;
}

// dvar[0] = sum of the partials, fixed order (one block of 256 threads)
__global__ __launch_bounds__(256) void k_dvar_finish(const double* __restrict__ part, int n, float* __restrict__ dvar) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) s += part[i];
    sh[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    if (t == 0) dvar[0] = (float)sh[0];
}

}  // namespace gnr

// =========================================================================================================
// Render path, per-ray tail: the two ELU layers of geometry_fc (86 -> 64 -> 16, ibrnet.py:488-489) on dual numbers, around
// k_ray_dual_bwd.  Input x = [mean 32, var 32, wbar, embed(p) 21]; the tangent enters through embed only
// (xd = d embed(p + eps gamma) / d eps, 21 columns).  One lane per point, hidden units streamed with wave-uniform weight
// rows read from the level's canonical (state-dict order, true scale) blob.
//   k_geo_dual_fwd: g = ELU(W2 ELU(W1 x + b1) + b2) and its tangent gd          -> inputs of k_ray_dual_bwd
//   k_geo_dual_bwd: (gbar, gdbar) -> d stats [P][66] and the gradients of geometry_fc.{0,2}: value and tangent adjoints
//                   with the ELU'' cross terms; weight gradients as 16x16 MFMAs with the workgroup's points as K
//                   (x gets a column of ones so that db1 rides in dW1's tile).
// Algebra: graspnerf_amd/ray_tail.py::tail_backward.
// =========================================================================================================
namespace gnr {

struct GeoDualArgs {
    const float* canon; const float* stats; const float* pts; const float* gamma;
    const float* gbar; const float* gdbar;
    float* g; float* gd; float* dstats; float* dpart;      // dpart: [wavefront slots][GD_STRIDE] partial geometry_fc gradients (offsets - GD_BASE)
    int P, nblocks;
    float* ybuf;     // backward: [288][P] per-point adjoints handed from k_geo_dual_bwd_pts to k_geo_dual_bwd_gemm (column c of point p at c * P + p)
};

DEV void geo_dual_inputs(const GeoDualArgs& a, size_t pt, float (&x)[86], float (&xd)[21]) {
    const float* st = a.stats + pt * 66;
#pragma unroll
    for (int c = 0; c < 65; ++c) x[c] = st[c];
    const float* p = a.pts + pt * 3;
    const float* gm = a.gamma + pt * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float pc = p[c], gc = gm[c];
        float s1, c1, s2, c2, s4, c4;
        sincos_octaves(pc, s1, c1, s2, c2, s4, c4);
        x[65 + c] = pc; x[68 + c] = s1; x[71 + c] = c1; x[74 + c] = s2; x[77 + c] = c2; x[80 + c] = s4; x[83 + c] = c4;
        xd[c] = gc; xd[3 + c] = c1 * gc; xd[6 + c] = -s1 * gc; xd[9 + c] = 2.f * c2 * gc; xd[12 + c] = -2.f * s2 * gc;
        xd[15 + c] = 4.f * c4 * gc; xd[18 + c] = -4.f * s4 * gc;
    }
}

// hidden unit k of geometry_fc.0 on dual numbers: pre-activation and its tangent
DEV void geo_hidden(const float* __restrict__ canon, int k, const float (&x)[86], const float (&xd)[21], float& h1p, float& h1pd) {
    const float* w = canon + can::GEO0_W + k * 86;
    float s = canon[can::GEO0_B + k], t = 0.f;
#pragma unroll
    for (int c = 0; c < 86; ++c) s = fmaf(w[c], x[c], s);
#pragma unroll
    for (int c = 0; c < 21; ++c) t = fmaf(w[65 + c], xd[c], t);
    h1p = s; h1pd = t;
}

// gp = W2 ELU(h1p) + b2 and its tangent, streamed over the 64 hidden units
DEV void geo_dual_forward(const float* __restrict__ canon, const float (&x)[86], const float (&xd)[21], float (&gp)[16], float (&gpd)[16]) {
#pragma unroll
    for (int f = 0; f < 16; ++f) { gp[f] = canon[can::GEO2_B + f]; gpd[f] = 0.f; }
    for (int k = 0; k < 64; ++k) {
        float h1p, h1pd;
        geo_hidden(canon, k, x, xd, h1p, h1pd);
        const float ex = __expf(h1p);
        const float h1 = h1p > 0.f ? h1p : ex - 1.f, h1d = (h1p > 0.f ? 1.f : ex) * h1pd;
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            const float w2 = canon[can::GEO2_W + f * 64 + k];
            gp[f] = fmaf(w2, h1, gp[f]);
            gpd[f] = fmaf(w2, h1d, gpd[f]);
        }
    }
}

// only_if: null, or the range word of k_geo_dual_fwd_mm -- the launch returns at once unless that kernel flagged its outputs
__global__ __launch_bounds__(256) void k_geo_dual_fwd(GeoDualArgs a, const unsigned* __restrict__ only_if) {
    if (only_if && __builtin_nontemporal_load(only_if) == 0u) return;
    const int pt_u = blockIdx.x * 256 + threadIdx.x;
    if (pt_u >= a.P) return;
    const size_t pt = pt_u;
    float x[86], xd[21], gp[16], gpd[16], g[16], gd[16];
    geo_dual_inputs(a, pt, x, xd);
    geo_dual_forward(a.canon, x, xd, gp, gpd);
#pragma unroll
    for (int f = 0; f < 16; ++f) {
        const float ex = __expf(gp[f]);
        g[f] = gp[f] > 0.f ? gp[f] : ex - 1.f;
        gd[f] = (gp[f] > 0.f ? 1.f : ex) * gpd[f];
    }
    put16(a.g + pt * 16, g);
    put16(a.gd + pt * 16, gd);
}

// ---- backward of geometry_fc on dual numbers, as two kernels (round 3).
// The first version did everything in one kernel, one lane per point: ~22 k FMA per point on the VALU (the layer forward and reverse,
// hidden units streamed with wave-uniform weight rows) AND the weight gradients as 16 x 16 MFMAs over the workgroup's points, whose
// operand tiles take 1 KB of LDS per point -- so 128 points = two wavefronts per CU, half a wavefront per SIMD, was all a CU could hold
// and the vector work ran at a fraction of the machine (1.15 ms per pass of 164 k points).  Now:
//   k_geo_dual_bwd_pts   one lane per point, no LDS tiles: 8 wavefronts per CU; writes d stats and hands the per-point adjoints
//                        (h1p-bar, h1pd-bar, h1, h1d: 4 x 64, gp-bar, gpd-bar: 2 x 16) over as columns [288][P] (coalesced both ways);
//   k_geo_dual_bwd_gemm  dW1 (+ db1), dW2, db2 = the outer products over the points on the matrix cores, operands from that buffer.
namespace gd2 {
constexpr int NT = 64, NW = 2;                   // points per workgroup of the GEMM kernel, its wavefronts (thread = (point, half))
constexpr int SX = 112, SXD = 48;                // row strides: the four k-groups of an MFMA operand read disjoint banks
constexpr int TX = 0, TXD = TX + NT * SX, TYA = TXD + NT * SXD, TYB = TYA + NT * 16, TH = TYB + NT * 16, THD = TH + NT * 16;
constexpr int TG = THD + NT * 16, TGD = TG + NT * 16, TOTAL = TGD + NT * 16;
constexpr int YCOLS = 288;                       // ybuf columns: h1p-bar [0,64) h1pd-bar [64,128) h1 [128,192) h1pd [192,256) gp-bar [256,272) gpd-bar [272,288)
}

// only_if: null, or the range word of k_geo_dual_bwd_pts_mm -- the launch returns at once unless that kernel flagged its outputs
__global__ __launch_bounds__(256, 2) void k_geo_dual_bwd_pts(GeoDualArgs a, const unsigned* __restrict__ only_if) {
    if (only_if && __builtin_nontemporal_load(only_if) == 0u) return;
    __shared__ __attribute__((aligned(16))) float w2t[64 * 16];                 // geometry_fc.2 weight, [k][f]: one broadcast read per hidden unit
    for (int i = threadIdx.x; i < 1024; i += 256) w2t[(i & 63) * 16 + (i >> 6)] = a.canon[can::GEO2_W + i];
    __syncthreads();
    const int pt_u = blockIdx.x * 256 + threadIdx.x;
    const bool act = pt_u < a.P;
    const size_t pt = act ? pt_u : a.P - 1;
    const float* canon = a.canon;
    float gpbar[16], gpdbar[16];
    float* ybw = a.ybuf + pt;                              // column c of this point: ybw[c * P]
    const size_t Pn = (size_t)a.P;
    {
        float x[86], xd[21];
        geo_dual_inputs(a, pt, x, xd);
        float gp[16], gpd[16], gbar[16], gdbar[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) { gp[f] = canon[can::GEO2_B + f]; gpd[f] = 0.f; }
#pragma unroll 1
        for (int k = 0; k < 64; ++k) {
            float h1p, h1pd;
            geo_hidden(canon, k, x, xd, h1p, h1pd);
            const float ex = __expf(h1p);
            const float h1 = h1p > 0.f ? h1p : ex - 1.f, h1d = (h1p > 0.f ? 1.f : ex) * h1pd;
            if (act) { ybw[(128 + k) * Pn] = h1; ybw[(192 + k) * Pn] = h1pd; }      // the reverse loop reads them back instead of recomputing the layer
#pragma unroll
            for (int f4i = 0; f4i < 4; ++f4i) {
                const f4 w = reinterpret_cast<const f4*>(w2t + k * 16)[f4i];
                gp[4 * f4i] = fmaf(w.x, h1, gp[4 * f4i]); gp[4 * f4i + 1] = fmaf(w.y, h1, gp[4 * f4i + 1]);
                gp[4 * f4i + 2] = fmaf(w.z, h1, gp[4 * f4i + 2]); gp[4 * f4i + 3] = fmaf(w.w, h1, gp[4 * f4i + 3]);
                gpd[4 * f4i] = fmaf(w.x, h1d, gpd[4 * f4i]); gpd[4 * f4i + 1] = fmaf(w.y, h1d, gpd[4 * f4i + 1]);
                gpd[4 * f4i + 2] = fmaf(w.z, h1d, gpd[4 * f4i + 2]); gpd[4 * f4i + 3] = fmaf(w.w, h1d, gpd[4 * f4i + 3]);
            }
        }
        get16(a.gbar + pt * 16, gbar);
        get16(a.gdbar + pt * 16, gdbar);
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            const float ex = __expf(gp[f]);
            const float e2 = gp[f] > 0.f ? 1.f : ex, d2 = gp[f] > 0.f ? 0.f : ex;
            gpbar[f] = act ? e2 * gbar[f] + d2 * gpd[f] * gdbar[f] : 0.f;
            gpdbar[f] = act ? e2 * gdbar[f] : 0.f;
        }
    }
    float* yb = ybw;
    const size_t P = Pn;
    if (act) {
#pragma unroll
        for (int f = 0; f < 16; ++f) { yb[(256 + f) * P] = gpbar[f]; yb[(272 + f) * P] = gpdbar[f]; }
    }
    float dst[65];
#pragma unroll
    for (int c = 0; c < 65; ++c) dst[c] = 0.f;
#pragma unroll 2
    for (int k = 0; k < 64; ++k) {
        const float h1 = yb[(128 + k) * P], h1pd = yb[(192 + k) * P];       // written by this lane above (ELU value: > 0 <=> pre-activation > 0; e^a = h1 + 1 otherwise)
        const float e1 = h1 > 0.f ? 1.f : h1 + 1.f, d1 = h1 > 0.f ? 0.f : h1 + 1.f;
        float hb = 0.f, hdb = 0.f;
#pragma unroll
        for (int f4i = 0; f4i < 4; ++f4i) {
            const f4 w = reinterpret_cast<const f4*>(w2t + k * 16)[f4i];
            hb = fmaf(w.x, gpbar[4 * f4i], hb); hb = fmaf(w.y, gpbar[4 * f4i + 1], hb); hb = fmaf(w.z, gpbar[4 * f4i + 2], hb); hb = fmaf(w.w, gpbar[4 * f4i + 3], hb);
            hdb = fmaf(w.x, gpdbar[4 * f4i], hdb); hdb = fmaf(w.y, gpdbar[4 * f4i + 1], hdb); hdb = fmaf(w.z, gpdbar[4 * f4i + 2], hdb); hdb = fmaf(w.w, gpdbar[4 * f4i + 3], hdb);
        }
        const float h1pbar = e1 * hb + d1 * h1pd * hdb, h1pdbar = e1 * hdb;
        const float* w = canon + can::GEO0_W + k * 86;
#pragma unroll
        for (int c = 0; c < 65; ++c) dst[c] = fmaf(w[c], h1pbar, dst[c]);
        if (act) {
            yb[k * P] = h1pbar;
            yb[(64 + k) * P] = h1pdbar;
        }
    }
    if (act) {
        float* ds = a.dstats + pt * 66;
#pragma unroll
        for (int c = 0; c < 65; ++c) ds[c] = dst[c];
        ds[65] = 0.f;
    }
}

// Workgroup = 64 points x 2 wavefronts (round 4; before: 128 points, 131 KB of tiles, ONE workgroup = two wavefronts per CU): the 65 KB of
// tiles let two workgroups share a CU.  Thread (point p, half h): half 0 builds the input tile (x, its tangent) and loads the adjoints of
// geometry_fc.0's pre-activation, half 1 loads geometry_fc.2's adjoints and the hidden activations; the outer products over the 64 points are
// split by output COLUMNS: wavefront 0 owns dW1[:, 0:48] and dW2, wavefront 1 dW1[:, 48:87] (x columns 48..85, the ones column = db1, and the
// tangent products, which land in columns 64..85) -- five MFMAs per k-step each.
__global__ __launch_bounds__(128, 2) void k_geo_dual_bwd_gemm(GeoDualArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    using namespace gd2;
    const int tid = threadIdx.x, lane = tid & 63, pl = tid & 63;                       // pl: the thread's point inside the block
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                          // scalar: the two roles branch without exec masks
    const int c16 = lane & 15, kg = lane >> 4;
    const size_t P = (size_t)a.P;
    f4 aA[4][3], aB[4];                                  // wave 0: dW1 column blocks 0..2, dW2;  wave 1: dW1 column blocks 3..5 (aB unused)
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
        aB[bi] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int bj = 0; bj < 3; ++bj) aA[bi][bj] = f4{0.f, 0.f, 0.f, 0.f};
    }
    float gb2[16];                                       // wave 1: sum of geometry_fc.2's adjoints (db2)
#pragma unroll
    for (int f = 0; f < 16; ++f) gb2[f] = 0.f;

    for (int blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        const int pt_u = blk * NT + pl;
        const bool act = pt_u < a.P;
        const size_t pt = act ? pt_u : a.P - 1;
        const float* yb = a.ybuf + pt;
        __syncthreads();                                  // previous block's MFMAs are done with every tile
        if (wave == 0) {
            float x[86], xd[21];
            geo_dual_inputs(a, pt, x, xd);
            float* tx = sm + TX + pl * SX;
#pragma unroll
            for (int c4 = 0; c4 < 21; ++c4) reinterpret_cast<f4*>(tx)[c4] = f4{x[4 * c4], x[4 * c4 + 1], x[4 * c4 + 2], x[4 * c4 + 3]};
            reinterpret_cast<f4*>(tx)[21] = f4{x[84], x[85], 1.f, 0.f};            // column 86 = 1: db1 rides in dW1's tile
            reinterpret_cast<f4*>(tx)[22] = f4{0.f, 0.f, 0.f, 0.f};
            reinterpret_cast<f4*>(tx)[23] = f4{0.f, 0.f, 0.f, 0.f};
            float* txd = sm + TXD + pl * SXD;                                      // tangent columns 64..95 of the input
            txd[0] = 0.f;
#pragma unroll
            for (int c = 0; c < 21; ++c) txd[1 + c] = xd[c];
#pragma unroll
            for (int c = 22; c < 32; ++c) txd[c] = 0.f;
        } else {
            float gpbar[16], gpdbar[16];
#pragma unroll
            for (int f = 0; f < 16; ++f) {
                gpbar[f] = act ? yb[(256 + f) * P] : 0.f;
                gpdbar[f] = act ? yb[(272 + f) * P] : 0.f;
                gb2[f] += gpbar[f];
            }
            put16(sm + TG + pl * 16, gpbar);
            put16(sm + TGD + pl * 16, gpdbar);
        }
#pragma unroll
        for (int bi = 0; bi < 4; ++bi) {
            if (bi > 0) __syncthreads();                  // the previous hidden block's MFMAs have read TYA..THD
            if (wave == 0) {
                float ya[16], ybv[16];
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const int k = 16 * bi + kk;
                    ya[kk] = act ? yb[k * P] : 0.f; ybv[kk] = act ? yb[(64 + k) * P] : 0.f;
                }
                put16(sm + TYA + pl * 16, ya); put16(sm + TYB + pl * 16, ybv);
            } else {
                float hh[16], hd[16];
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const int k = 16 * bi + kk;
                    hh[kk] = act ? yb[(128 + k) * P] : 0.f;
                    hd[kk] = act ? (hh[kk] > 0.f ? 1.f : hh[kk] + 1.f) * yb[(192 + k) * P] : 0.f;       // h1d = ELU'(a) h1pd
                }
                put16(sm + TH + pl * 16, hh); put16(sm + THD + pl * 16, hd);
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll 4
                for (int s2 = 0; s2 < 16; ++s2) {
                    const int p = 4 * s2 + kg;
                    const float yav = sm[TYA + p * 16 + c16];
#pragma unroll
                    for (int bj = 0; bj < 3; ++bj) aA[bi][bj] = mfma16(yav, sm[TX + p * SX + 16 * bj + c16], aA[bi][bj]);
                    aB[bi] = mfma16(sm[TG + p * 16 + c16], sm[TH + p * 16 + c16], aB[bi]);
                    aB[bi] = mfma16(sm[TGD + p * 16 + c16], sm[THD + p * 16 + c16], aB[bi]);
                }
            } else {
#pragma unroll 4
                for (int s2 = 0; s2 < 16; ++s2) {
                    const int p = 4 * s2 + kg;
                    const float yav = sm[TYA + p * 16 + c16], ybb = sm[TYB + p * 16 + c16];
#pragma unroll
                    for (int bj = 0; bj < 3; ++bj) aA[bi][bj] = mfma16(yav, sm[TX + p * SX + 16 * (3 + bj) + c16], aA[bi][bj]);
                    aA[bi][1] = mfma16(ybb, sm[TXD + p * SXD + c16], aA[bi][1]);
                    aA[bi][2] = mfma16(ybb, sm[TXD + p * SXD + 16 + c16], aA[bi][2]);
                }
            }
        }
    }
    // ---- flush: D row = 4 kg + u (output feature inside the block), column = c16.  Every entry of geometry_fc's range is stored in
    // both wavefronts' slots: a wavefront writes zeros where the other one owns the sum (the reduction adds all slots over the whole range)
    float* gc = grad_slot(a.dpart, GD_STRIDE) - GD_BASE;
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
#pragma unroll
        for (int bj = 0; bj < 6; ++bj) {
            const bool mine = (bj >= 3) == (wave == 1);
            const f4 v = aA[bi][bj % 3];
            const float e[4] = {mine ? v.x : 0.f, mine ? v.y : 0.f, mine ? v.z : 0.f, mine ? v.w : 0.f};
            const int c = 16 * bj + c16;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = 16 * bi + 4 * kg + u;
                if (c < 86) gc[can::GEO0_W + f * 86 + c] = e[u];
                else if (c == 86) gc[can::GEO0_B + f] = e[u];
            }
        }
        const float e2[4] = {aB[bi].x, aB[bi].y, aB[bi].z, aB[bi].w};          // (zero in wave 1: never accumulated)
#pragma unroll
        for (int u = 0; u < 4; ++u) gc[can::GEO2_W + (4 * kg + u) * 64 + 16 * bi + c16] = e2[u];
    }
#pragma unroll
    for (int f = 0; f < 16; ++f) {
        const float sb = wave_sum64(gb2[f]);                                  // (zero in wave 0)
        if (lane == 0) gc[can::GEO2_B + f] = sb;
    }
}

}  // namespace gnr

#include "gnr_bwd_geo_dual_mm.inc"
