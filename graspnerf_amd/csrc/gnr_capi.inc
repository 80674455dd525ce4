// C-ABI entry points (declared in include/gnr.h).  Included at the end of gnr_kernels.hip.
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <type_traits>

#include "gnr_host.h"

namespace gnr {

static thread_local char g_err[512] = "";     // the library's one error text: written by gnr_internal_fail (fail(), gnr_host.h), read by gnr_last_error

struct Workspace {
    float* feat64; float* viewp; unsigned* range_flag;             // persistent between gnr_prepare and the forwards
    float* desc; float* rec; float* depth_c; float* depth_f; float* depth_m; float* gerr_part; unsigned char* vmask_pts;   // per call
    int* ray_perm;                                                  // per call: Morton order of the rays (k_ray_order)
    int* sample_perm; unsigned char* sample_keys;                   // per render pass: view-mask order of the samples (k_points_rays, k_sample_order); used up to MAX_SORT_SAMPLES
    size_t total;
};

// Region A (feat64, viewp) depends only on the scene dims; region B is re-carved by every call from
// its own point count (P points and rn rays per scene), so the entry points stay stateless.
static Workspace carve(const GnrScene* s, size_t P, size_t rn, void* base) {
    Workspace w;
    char* p = (char*)base;
    size_t off = 0;
    const size_t BV = (size_t)s->B * s->V;
    auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += al256(bytes); return q; };
    w.feat64 = (float*)take(BV * s->fh * s->fw * 64 * sizeof(float));
    w.viewp = (float*)take(BV * VIEWP_FLOATS * sizeof(float));
    w.range_flag = (unsigned*)take(512);                            // 64 status words (range guard of the pair form, gnr_kernels.hip RangeWatch) + 64 words of tile counters (ChainArgs::tile_ctr)
    w.desc = (float*)take((size_t)s->B * P * DESC_FLOATS * sizeof(float));
    w.rec = (float*)take((size_t)s->B * P * REC_RAY * sizeof(float));
    w.depth_c = (float*)take((size_t)s->B * P * sizeof(float));
    w.depth_f = (float*)take((size_t)s->B * P * sizeof(float));
    w.depth_m = (float*)take((size_t)s->B * P * sizeof(float));
    w.gerr_part = (float*)take((size_t)s->B * (rn > 0 ? rn : 1) * sizeof(float));
    w.vmask_pts = (unsigned char*)take((size_t)s->B * P);
    w.ray_perm = (int*)take((size_t)s->B * (rn > 0 ? rn : 1) * sizeof(int));
    // ray samples only (rn == 0: volume points, never ordered).  Reserved for every P, also above MAX_SORT_SAMPLES where no pass uses it: the
    // total grows with P, so a workspace sized for P serves every call of the same rn with fewer points
    w.sample_perm = rn > 0 ? (int*)take((size_t)s->B * P * sizeof(int)) : nullptr;
    w.sample_keys = rn > 0 ? (unsigned char*)take((size_t)s->B * P) : nullptr;
    w.total = off;
    return w;
}

// The 64 status words of a workspace (Workspace::range_flag; zeroed by gnr_prepare, ORed by gnr_range_status).  Word 0 carries the bits that
// concern every launch on the prepared scene (0 = a feature, 2 = a weight beyond the fp16-pair range); the launch slots carry bit 1 of
// their launch; the last words belong to the per-ray kernel's tail, the backward and the fixed-point scatter.
enum StatusSlot { RS_SCENE = 0, RS_VOLUME = 1, RS_COARSE = 2, RS_FINE = 3, RS_VOLUME_TRAIN = 4, RS_COARSE_TRAIN = 5, RS_DEPTHS_TRAIN = 6,
                  RS_VOLUME_GRAD = 7 /* gnr_sample_volume_grad_fwd: its chain launch */, RS_VOLUME_GRAD_RAY = 8 /* ... and its per-column kernel's matrix-core tail */,
                  RS_BACKWARD = 61 /* bit 4: GNR_STATUS_LOST_PARTNER */, RS_RAY_WATCH = 62 /* k_ray<true>'s matrix-core tail */,
                  RS_FEAT_FX = 63 /* bit 3: a clamped fixed-point contribution */, RS_WORDS = 64 };
static_assert(RS_VOLUME_GRAD_RAY < RS_BACKWARD && RS_FEAT_FX < RS_WORDS, "status slots");
static inline bool opt(const GnrScene* s, unsigned bit) { return (s->options & bit) != 0; }

static int check_scene(const GnrScene* s) {
    if (!s || !s->imgs || !s->img_feats || !s->ray_feats || !s->poses || !s->Ks || !s->depth_range)
        return fail(GNR_ERR_ARG, "GnrScene: null pointer");
    if (s->options & ~GNR_OPT_ALL) return fail(GNR_ERR_ARG, "GnrScene.options: unknown bits (GNR_OPT_*)");
    if (s->B < 1 || s->H < 2 || s->W < 2 || s->fh < 1 || s->fw < 1) return fail(GNR_ERR_SHAPE, "GnrScene: bad dims");
    if (s->V < 2 || s->V > 8) return fail(GNR_ERR_SHAPE, "GnrScene: V must be in 2..8");
    return GNR_OK;
}

// kernels index points with 32-bit ints (B*P points, a few launches round the count up to a multiple of 256)
static int check_points(const GnrScene* s, size_t P) {
    if ((size_t)s->B * P > ((size_t)1 << 31) - 1024) return fail(GNR_ERR_SHAPE, "too many points in one call (B*P must stay below 2^31): split the rays / scenes");
    return GNR_OK;
}

// the brick-ordered traversal of k_chain is a bijection only for these grid sizes (otherwise plain column order)
static bool brick_order_ok(int R) { return R % 8 == 0; }

static int num_cus() {
    static int n = 0;
    if (!n) {
        hipDeviceProp_t prop;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
        n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return n;
}

// ---- deterministic parameter gradients (csrc/gnr_bwd.inc): slot counts of the partial buffers and the fixed-order reduction ----
// The view-chain / geometry backward kernels run at most one workgroup of four wavefronts per CU, the per-ray tails and the
// depth-mean / geometry-GEMM kernels up to two workgroups per CU.
static size_t chain_part_floats() { return (size_t)4 * num_cus() * GP_STRIDE; }
static size_t tail_part_floats(int waves_per_block) { return (size_t)2 * num_cus() * waves_per_block * tp::STRIDE; }
// grid of the backward's chain stages: four tiles (wavefronts) per workgroup, at most one workgroup per CU
static int chain_blocks(int ntiles) { return (ntiles + 3) / 4 < num_cus() ? (ntiles + 3) / 4 : num_cus(); }

struct GradRange { int lo, hi, dlo; };

// ---- optional in-situ timing of the library's kernels (bench.py: roofline.achieved, train-step split) -------------
// Between gnr_timing_begin() and gnr_timing_end() every kernel launch of this library is bracketed by a pair of HIP
// events recorded on ITS launch stream (no synchronisation is added to the path); gnr_timing_end() waits for them and
// reports count and total milliseconds per label ("kernel@entry point").  Process-wide switch, measurement only.
// The autograd backward thread and the main thread both launch kernels: slots are claimed with an atomic counter.
struct KTiming {
    static constexpr int MAX = 16384;
    std::atomic<bool> on{false}; std::atomic<int> n{0};
    char only[64] = "";              // when non-empty: only labels containing this substring are bracketed
    struct Rec { const char* label; hipEvent_t e0, e1; } rec[MAX];
};
static KTiming g_kt;

// The kernels with a view loop are templates on the view count: f(std::integral_constant<int, V>) for the scene's V (check_scene: 2..8)
template <typename F>
static int with_views(int V, F&& f) {
    switch (V) {
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        case 6: return f(std::integral_constant<int, 6>());
        case 7: return f(std::integral_constant<int, 7>());
        case 8: return f(std::integral_constant<int, 8>());
        default: return fail(GNR_ERR_SHAPE, "unsupported view count");
    }
}

static int launch_grad_reduce(const float* part, int nslots, int stride, float* dst, const GradRange* rg, int nranges,
                              hipStream_t st, const char* label) {
    GradReduceArgs a;
    memset(&a, 0, sizeof(a));
    a.part = part; a.dst = dst; a.nslots = nslots; a.stride = stride; a.nranges = nranges;
    int total = 0;
    for (int k = 0; k < nranges; ++k) { a.lo[k] = rg[k].lo; a.hi[k] = rg[k].hi; a.dlo[k] = rg[k].dlo; total += rg[k].hi - rg[k].lo; }
    if (total <= 0 || nslots <= 0) return GNR_OK;
    return launch<k_grad_reduce>(label, st, dim3((total + 63) / 64), dim3(256), 0, a);
}

// partials of a per-ray tail kernel (layout tp::) -> dtail (layout tl::, overwritten)
static int launch_tail_reduce(const float* part, int nslots, const float* wpk, float* dtail, hipStream_t st) {
    GNR_HIP(hipMemsetAsync(dtail, 0, tl::TOTAL * sizeof(float), st));
    const GradRange rg[1] = {{tp::W, tp::W + 1024, tl::WQ}};
    if (int rc = launch_grad_reduce(part, nslots, tp::STRIDE, dtail, rg, 1, st, "k_grad_reduce@tail")) return rc;
    return launch<k_tail_finish>("k_tail_finish", st, dim3(16), dim3(256), 0, part, nslots, wpk, dtail);
}

// GNR_OPT_POISON_PARTIALS: fill a partial buffer with NaN bit patterns before its kernels run, so that a slot entry the kernels fail
// to store shows up in the reduced gradient
static int poison_partials(void* p, size_t bytes, hipStream_t st, unsigned options) {
    if (options & GNR_OPT_POISON_PARTIALS) GNR_HIP(hipMemsetAsync(p, 0xFF, bytes, st));
    return GNR_OK;
}


template <int V, bool RENDER, bool SAVE, bool USEVIS, bool SP>
static int launch_chain_one(const ChainArgs& a, hipStream_t st, const char* label) {
    constexpr size_t lds_bytes = (size_t)(SP ? pk::C16_END : pk::CHAIN_END) * sizeof(float);
    const int tps = (a.P + 15) / 16;
    const long ntiles = (long)a.B * tps;
    constexpr int WPB = kChainThreads / 64;
    long blocks = (ntiles + WPB - 1) / WPB;
    const long maxb = num_cus();
    if (blocks > maxb) blocks = maxb;
    return launch<k_chain<V, RENDER, SAVE, USEVIS, SP>, lds_bytes>(label, st, dim3((unsigned)blocks), dim3(kChainThreads), lds_bytes, a);
}

// One chain launch of the product = the pair kernel + its fp32-MFMA twin on the same arguments with only_if_flagged set: the
// twin's wavefronts read the range word and return while it is zero (no host round trip; ~5 us of launch per chain launch),
// and recompute the whole launch on the fp32-input MFMA when a feature or an activation left the fp16-pair range.
// force_fp32 (GNR_OPT_FP32_CHAIN): the fp32-MFMA instantiation alone, the pair kernel is skipped
template <int V, bool RENDER, bool SAVE = false, bool USEVIS = false>
static int launch_chain_t(const ChainArgs& a, hipStream_t st, bool force_fp32, const char* label_as = nullptr, const char* twin_as = nullptr) {
    const char* label = label_as ? label_as : RENDER ? (SAVE ? "k_chain.render.train" : "k_chain.render") : (SAVE ? "k_chain.volume.train" : "k_chain.volume");
    if constexpr (GNR_SPLIT16 != 0) {
        ChainArgs b = a;
        b.only_if_flagged = 0;
        if (force_fp32) return launch_chain_one<V, RENDER, SAVE, USEVIS, false>(b, st, label);
        if (int rc = launch_chain_one<V, RENDER, SAVE, USEVIS, true>(b, st, label)) return rc;
        if (!a.range_flag || !GNR_RANGE_GUARD) return GNR_OK;
        b.only_if_flagged = 1;
        return launch_chain_one<V, RENDER, SAVE, USEVIS, false>(b, st, twin_as ? twin_as : RENDER ? "k_chain.render.fp32_twin" : "k_chain.volume.fp32_twin");
    } else {
        ChainArgs b = a;
        b.only_if_flagged = 0;
        return launch_chain_one<V, RENDER, SAVE, USEVIS, false>(b, st, label);
    }
}

// use_vis (GnrScene.use_vis: the levels' decoders carry the fourth branch, gnr_pack_vis_decoder / gnr_pack_vis_decoder_bwd)
// label_as / twin_as: timing labels of an entry point that names its launches itself (null: the kernel's own)
template <bool RENDER, bool SAVE = false>
static int launch_chain(const GnrScene* s, const ChainArgs& a, hipStream_t st, const char* label_as = nullptr, const char* twin_as = nullptr) {
    if (s->use_vis != 0 && s->use_vis != 1) return fail(GNR_ERR_ARG, "GnrScene.use_vis must be 0 or 1");
    const bool f32 = opt(s, GNR_OPT_FP32_CHAIN);
    return with_views(s->V, [&](auto v) {
        constexpr int V = decltype(v)::value;
        return s->use_vis ? launch_chain_t<V, RENDER, SAVE, true>(a, st, f32, label_as, twin_as) : launch_chain_t<V, RENDER, SAVE, false>(a, st, f32, label_as, twin_as);
    });
}
// The range guard and the tile hand-out of a chain launch: the scene's status words, the watch word of this launch (slot) and, unless
// GNR_OPT_STATIC_TILES, the tile counters behind them (part: the half of a GNR_OPT_SPLIT_LAUNCH call, each with counters of its own)
constexpr int TILE_CTR_VOLUME_GRAD = 2;                  // (parts 0 and 1: the halves of a GNR_OPT_SPLIT_LAUNCH call)
static void wire_chain(ChainArgs& a, const GnrScene* s, const Workspace& w, int slot, int part = 0) {
    a.range_flag = w.range_flag;
    a.range_launch = w.range_flag ? w.range_flag + slot : nullptr;
    a.tile_ctr = (w.range_flag && !opt(s, GNR_OPT_STATIC_TILES)) ? w.range_flag + RS_WORDS + 16 * part : nullptr;
}

// The backward's view kernels (csrc/gnr_bwd.inc).  Default: the partner-wavefront kernels (gnr_bwd_view{1,2}_pw.inc: same outputs, same
// slots of the deterministic reduction); GNR_OPT_VIEW{1,2}_ONE_WAVEFRONT: one wavefront per tile; use_vis levels take k_view1_bwd<true>
// (the fourth decoder branch does not fit the partner's registers).
static bool view1_partner(const GnrScene* s) { return !opt(s, GNR_OPT_VIEW1_ONE_WAVEFRONT) && !opt(s, GNR_OPT_FP32_CHAIN) && !s->use_vis; }
static bool view2_partner(const GnrScene* s) { return !opt(s, GNR_OPT_VIEW2_ONE_WAVEFRONT) && !opt(s, GNR_OPT_FP32_CHAIN); }
// What tells the two chain backwards (gnr_sample_volume_bwd, gnr_render_chain_bwd) apart in the stages they share (chain_bwd):
//   slot, slot2: the watch words of the training forwards the backward follows -- the volume's, or the render passes' RS_COARSE_TRAIN and
//                RS_DEPTHS_TRAIN together (the backward is not told which of them it follows); slot2 < 0: none
//   rg:          the ranges of the canonical blob its stages store (launch_grad_reduce; the third one with use_vis only)
struct BwdEntry {
    bool volume;
    int slot, slot2;
    GradRange rg[3];
    const char *view2, *view2_twin, *view1, *view1_twin, *scatter_place, *scatter_scan, *scatter_fill, *scatter_gather, *unpack, *reduce;   // timing labels
};
// decoder .. geometry_fc [0, WQ), neuray_fc [NR0_W, VARIANCE) (+ the vis branch behind the blob)
static const BwdEntry BWD_VOLUME = {
    true, RS_VOLUME_TRAIN, -1, {{0, can::WQ, 0}, {can::NR0_W, can::VARIANCE, can::NR0_W}, {can::TOTAL, can::TOTAL_VIS, can::TOTAL}},
    "k_view2_bwd@gnr_sample_volume_bwd", "k_view2_bwd.fp32_twin@gnr_sample_volume_bwd",
    "k_view1_bwd@gnr_sample_volume_bwd", "k_view1_bwd.fp32_twin@gnr_sample_volume_bwd",
    "k_scatter_place@gnr_sample_volume_bwd", "k_scatter_scan@gnr_sample_volume_bwd", "k_scatter_fill@gnr_sample_volume_bwd",
    "k_scatter_gather@gnr_sample_volume_bwd", "k_unpack_feat_grad@gnr_sample_volume_bwd", "k_grad_reduce@gnr_sample_volume_bwd"};
// decoder .. vis_fc2 [0, GEO0_W), rgb_fc + neuray_fc [RGB0_W, VARIANCE) (+ the vis branch behind the blob)
static const BwdEntry BWD_RENDER = {
    false, RS_COARSE_TRAIN, RS_DEPTHS_TRAIN, {{0, can::GEO0_W, 0}, {can::RGB0_W, can::VARIANCE, can::RGB0_W}, {can::TOTAL, can::TOTAL_VIS, can::TOTAL}},
    "k_view2_bwd@gnr_render_chain_bwd", "k_view2_bwd.fp32_twin@gnr_render_chain_bwd",
    "k_view1_bwd@gnr_render_chain_bwd", "k_view1_bwd.fp32_twin@gnr_render_chain_bwd",
    "k_scatter_place@gnr_render_chain_bwd", "k_scatter_scan@gnr_render_chain_bwd", "k_scatter_fill@gnr_render_chain_bwd",
    "k_scatter_gather@gnr_render_chain_bwd", "k_unpack_feat_grad@gnr_render_chain_bwd", "k_grad_reduce@gnr_render_chain_bwd"};
// range guard of a backward pass (BwdGuard, gnr_bwd.inc)
static BwdGuard bwd_guard(const GnrScene* s, const Workspace& w, const BwdEntry& e, int run_if) {
    unsigned* f = w.range_flag;
    return BwdGuard{f, f ? f + e.slot : nullptr, (f && e.slot2 >= 0) ? f + e.slot2 : nullptr, f ? run_if : 0,
                    f ? f + RS_BACKWARD : nullptr, opt(s, GNR_OPT_TEST_LOSE_PARTNER) ? 1 : 0};
}
// The channel-last feature-gradient buffer of an entry point: nfeat entries of 8 bytes (the fixed-point mode's; the float mode uses
// the first half) + one 256-byte line for the launch's upstream maximum.
static size_t feat_grad_bytes(const GnrScene* s) { return al256((size_t)s->B * s->V * s->fh * s->fw * 64 * 8) + 256; }
struct FeatGradBuf { float* buf; FeatFx fx; bool fixed; };
// zero the buffer and, in the fixed-point mode, take the maximum of the launch's upstream gradient
static int feat_grad_begin(const GnrScene* s, void* region, const Workspace& w, const float* upstream, size_t n_upstream, hipStream_t st, FeatGradBuf* out,
                           const BwdGuard* only_if_flagged = nullptr) {     // only_if_flagged: the binned view kernel collects the maximum itself
                                                                            // (ScatterBins::upmax); this pass serves the flagged case (the fp32 twin)
    const size_t nfeat = (size_t)s->B * s->V * s->fh * s->fw * 64;
    out->buf = (float*)region;
    out->fixed = opt(s, GNR_OPT_FEATURE_GRAD_FIXED);
    unsigned* upmax = (unsigned*)((char*)region + al256(nfeat * 8));
    out->fx = FeatFx{upmax, w.range_flag ? w.range_flag + RS_FEAT_FX : nullptr};      // status: bit 3 (gnr_range_status ORs the words)
    GNR_HIP(hipMemsetAsync(region, 0, out->fixed ? al256(nfeat * 8) + 256 : nfeat * sizeof(float), st));
    if (out->fixed) {
        int blocks = (int)((n_upstream + 256 * 16 - 1) / (256 * 16));
        if (blocks > 4 * num_cus()) blocks = 4 * num_cus();
        if (blocks < 1) blocks = 1;
        const BwdGuard* g = only_if_flagged;
        return launch<k_absmax_bits>("k_absmax_bits", st, dim3(blocks), dim3(256), 0, upstream, n_upstream, upmax, g ? g->word0 : nullptr,
                                     g ? g->slot : nullptr, g ? g->slot2 : nullptr);
    }
    return GNR_OK;
}
static int feat_grad_unpack(const GnrScene* s, const FeatGradBuf& g, float* d_ray_feats, float* d_img_feats, const char* label, hipStream_t st) {
    const int npix = s->fh * s->fw;
    const dim3 grid((npix + 63) / 64, s->B * s->V);
    return g.fixed ? launch<k_unpack_feat_grad<true>>(label, st, grid, dim3(256), 0, g.buf, d_ray_feats, d_img_feats, npix, g.fx)
                   : launch<k_unpack_feat_grad<false>>(label, st, grid, dim3(256), 0, g.buf, d_ray_feats, d_img_feats, npix, g.fx);
}

// Binned scatter of the feature-map gradient (csrc/gnr_bwd_scatter.inc): its buffers inside a training workspace, for T tiles of 16 points
struct ScatterWs { size_t rows, wts, key, cnt, cursor, list, nseg, total; };
static ScatterWs carve_scatter(const GnrScene* s, size_t T) {
    ScatterWs c;
    const size_t N = T * s->V * 16, bins = (size_t)s->B * s->V * s->fh * s->fw;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    c.rows = take(N * 64 * sizeof(float));
    c.wts = take(N * 4 * sizeof(float));
    c.key = take(N * sizeof(int));
    c.cnt = take(bins * sizeof(int));
    c.cursor = take(bins * sizeof(int));
    c.list = take(N * sizeof(int));
    c.nseg = take((size_t)s->B * s->V * sizeof(int));
    c.total = off;
    return c;
}
static ScatterBins scatter_bins(const GnrScene* s, size_t T, char* base) {
    const ScatterWs c = carve_scatter(s, T);
    return ScatterBins{(float*)(base + c.rows), (f4*)(base + c.wts), (int*)(base + c.key), (int*)(base + c.cnt), (int*)(base + c.cursor),
                       (int*)(base + c.list), (int*)(base + c.nseg)};
}
// the launches behind k_view1_bwd_pw when it parked its rows: places of the bins, row ids into them, sums per pixel.
// guard: the view kernel's -- on a range-flagged pass that kernel parked nothing (no key, no weight, no row), and these return at once too.
// path: SCATTER_PATH_AUTO = by the feature map's size; the other two are gnr_debug_feature_scatter's (a 3 x 3 map through scan + fill).
constexpr size_t PLACE_LDS = 150 * 1024;                       // k_scatter_place counts a scene-view's pixels in LDS
enum { SCATTER_PATH_AUTO = 0, SCATTER_PATH_PLACE = 1, SCATTER_PATH_SCAN_FILL = 2 };
static int launch_scatter_bins(const GnrScene* s, const ScatterBins& sc, float* dfeat64, int ntiles, const BwdEntry& e, bool fixed, const FeatFx& fx,
                               const BwdGuard& guard, hipStream_t st, int path = SCATTER_PATH_AUTO) {
    const int BV = s->B * s->V, npix = s->fh * s->fw, cap = (ntiles / s->B) * 16, N = ntiles * s->V * 16;
    if (path == SCATTER_PATH_AUTO) path = (size_t)npix * sizeof(int) <= PLACE_LDS ? SCATTER_PATH_PLACE : SCATTER_PATH_SCAN_FILL;
    if (path == SCATTER_PATH_PLACE) {
        if (int rc = launch<k_scatter_place, PLACE_LDS>(e.scatter_place, st, dim3(BV), dim3(1024), (size_t)npix * sizeof(int), (const int*)sc.cnt,
                                                        (const int*)sc.key, sc.list, sc.nseg, npix, cap, s->V, guard)) return rc;
    } else {
        if (int rc = launch<k_scatter_scan>(e.scatter_scan, st, dim3(BV), dim3(1024), 0, (const int*)sc.cnt, sc.cursor, sc.nseg, npix, cap, guard)) return rc;
        if (int rc = launch<k_scatter_fill>(e.scatter_fill, st, dim3((N + 255) / 256), dim3(256), 0, (const int*)sc.key, sc.cursor, sc.list, N, guard)) return rc;
    }
    ScatterGatherArgs g{sc, dfeat64, BV, cap, npix, s->fh, s->fw, fx, guard};
    const int chunks = BV * ((cap + 63) / 64);
    return fixed ? launch<k_scatter_gather<true>>(e.scatter_gather, st, dim3((chunks + 3) / 4), dim3(256), 0, g)
                 : launch<k_scatter_gather<false>>(e.scatter_gather, st, dim3((chunks + 3) / 4), dim3(256), 0, g);
}

// One launch of the first view loop's backward = the fp16-pair kernel of the call's options (partner wavefronts + binned scatter by
// default) and, behind it, the fp32-input-MFMA instantiation of k_view1_bwd on the same arguments: BwdGuard::run_if makes the former
// return at once when the pass is range-flagged and the latter unless (~6 us of launch; nothing synchronises with the host).
// GNR_OPT_FP32_CHAIN: the fp32 instantiation alone.
template <bool USEVIS, bool BP>
static int launch_view1_single(const char* label, const View1BwdArgs& a, bool fixed, int blocks, hipStream_t st) {
    constexpr size_t lds = (USEVIS ? l1::TOTAL_VIS : l1::TOTAL) * sizeof(float);
    return fixed ? launch<k_view1_bwd<USEVIS, true, BP>, lds>(label, st, dim3(blocks), dim3(256), lds, a)
                 : launch<k_view1_bwd<USEVIS, false, BP>, lds>(label, st, dim3(blocks), dim3(256), lds, a);
}
static bool view1_bins(const GnrScene* s) { return view1_partner(s) && !opt(s, GNR_OPT_DIRECT_SCATTER) && !opt(s, GNR_OPT_FP32_CHAIN); }
static int launch_view1_bwd(const GnrScene* s, const Workspace& w, const BwdEntry& e, View1BwdArgs a, bool fixed, int ntiles, char* scatter_region, hipStream_t st) {
    const int blocks = chain_blocks(ntiles);
    const bool f32 = opt(s, GNR_OPT_FP32_CHAIN);
    const bool pw = view1_partner(s);
    const bool bins = view1_bins(s) && scatter_region;       // (both feature-gradient modes: the rows are parked as floats either way)
    if (!f32) {
        a.guard = bwd_guard(s, w, e, 1);
        if (bins) {
            a.sc = scatter_bins(s, (size_t)ntiles, scatter_region);
            a.sc.upmax = fixed ? const_cast<unsigned*>(a.fx.upmax) : nullptr;
            GNR_HIP(hipMemsetAsync(a.sc.cnt, 0, (size_t)s->B * s->V * s->fh * s->fw * sizeof(int), st));
        }
        constexpr size_t ldsp = l1p::TOTAL * sizeof(float);
        int rc;
        if (pw && bins) rc = launch<k_view1_bwd_pw<false, true>, ldsp>(e.view1, st, dim3(blocks), dim3(512), ldsp, a);
        else if (pw && fixed) rc = launch<k_view1_bwd_pw<true>, ldsp>(e.view1, st, dim3(blocks), dim3(512), ldsp, a);
        else if (pw) rc = launch<k_view1_bwd_pw<false>, ldsp>(e.view1, st, dim3(blocks), dim3(512), ldsp, a);
        else if (s->use_vis) rc = launch_view1_single<true, true>(e.view1, a, fixed, blocks, st);
        else rc = launch_view1_single<false, true>(e.view1, a, fixed, blocks, st);
        if (rc) return rc;
        if (bins)                                               // (a flagged pass parked nothing -- cnt is cleared, key / wts / rows hold whatever was there:
                                                                //  the scatter kernels return under the same guard, the twin below scatters directly)
            if (int rc2 = launch_scatter_bins(s, a.sc, a.dfeat64, ntiles, e, fixed, a.fx, a.guard, st)) return rc2;
        a.sc = ScatterBins{};
    }
    a.guard = bwd_guard(s, w, e, f32 ? 0 : 2);
    if (!f32 && !a.guard.run_if) return GNR_OK;
    const char* label = f32 ? e.view1 : e.view1_twin;
    return s->use_vis ? launch_view1_single<true, false>(label, a, fixed, blocks, st) : launch_view1_single<false, false>(label, a, fixed, blocks, st);
}

// k_ray, k_ray_bwd and k_ray_dual_bwd keep `ray_floats` floats of LDS per ray and give a ray `slots` lanes: -> rays per workgroup, what
// its 256 lanes and the LDS budget hold (0: a ray does not fit), and the LDS stride of a ray.  Consecutive rays start 16 banks apart: a
// wavefront spans up to 3 rays whose broadcast reads then hit disjoint banks.
static int pack_rays(int ray_floats, int slots, int lds_budget_bytes, int* ray_stride) {
    *ray_stride = ((ray_floats + 63) / 64) * 64 + 16;
    const int fit = lds_budget_bytes / (*ray_stride * (int)sizeof(float));
    return 256 / slots < fit ? 256 / slots : fit;
}

// (RS_RAY_WATCH: the watch word of k_ray<true>'s matrix-core tail, bit 1.  Sticky until the next gnr_prepare: once tripped, every later
// k_ray<true> launch on the prepared scene is followed by its fp32 recomputation.)
// k_ray packs floor(256/slots) rays into a workgroup (slots = lanes per ray); two workgroups share a CU's LDS.
// VOLG: the volume output mode (gnr_sample_volume_grad_fwd)
template <bool RENDER, bool VOLG = false>
static int launch_ray(RayArgs& a, hipStream_t st) {
    const int fdn = (RENDER && a.fine_depth) ? a.fdn : 0;
    a.slots = a.dn > fdn ? a.dn : fdn;
    int ray_floats = a.dn * ray_per(RENDER);
    if (RENDER && ray_floats < rt::END) ray_floats = rt::END;
    const int lds_budget = (RENDER ? 52 : 78) * 1024;      // three (kRayBlocks) / two workgroups per CU
    const int rpb = pack_rays(ray_floats, a.slots, lds_budget, &a.ray_stride);
    if (rpb < 1) return fail(GNR_ERR_SHAPE, "k_ray: a ray does not fit the LDS budget");
    a.rays_per_block = rpb;
    constexpr size_t MAX_LDS = 80 * 1024;
    const size_t lds_bytes = (size_t)rpb * a.ray_stride * sizeof(float);
    const dim3 grid((unsigned)((a.nrays + rpb - 1) / rpb));
    if (int rc = launch<k_ray<RENDER, true, VOLG>, MAX_LDS>(VOLG ? "k_ray.render@volume_grad" : RENDER ? "k_ray.render" : "k_ray.volume", st, grid, dim3(256), lds_bytes, a)) return rc;
    if (RENDER && a.range_word) {
        // the fp32 twin of the matrix-core tail: returns at once unless that launch flagged a non-finite value (range guard, k_ray)
        a.only_if = a.range_word;
        return launch<k_ray<RENDER, false, VOLG>, MAX_LDS>(VOLG ? "k_ray.render.fp32_twin@volume_grad" : "k_ray.render.fp32_twin", st, grid, dim3(256), lds_bytes, a);
    }
    return GNR_OK;
}

}  // namespace gnr

using namespace gnr;

extern "C" const char* gnr_last_error(void) { return g_err; }
extern "C" const char* gnr_dominant_kernel_name(void) { return "k_chain"; }

extern "C" size_t gnr_workspace_bytes(const GnrScene* scene, int volume_res, int rn, int dn_max) {
    if (!scene) return 0;
    const size_t pv = (size_t)volume_res * volume_res * volume_res, pr = (size_t)rn * dn_max;
    return carve(scene, pv > pr ? pv : pr, rn, nullptr).total;
}

extern "C" int gnr_prepare(const GnrScene* s, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!ws) return fail(GNR_ERR_ARG, "workspace is null");
    // the carve only needs the leading regions here
    Workspace w = carve(s, 0, 0, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int npix = s->fh * s->fw, BV = s->B * s->V;
    // k_view_setup first: it also zeroes the range word that k_repack_feats and the chain launches OR into
    if (int rc = launch<k_view_setup>("k_view_setup@gnr_prepare", st, dim3((BV + 63) / 64), dim3(64), 0, s->poses, s->Ks, s->depth_range, w.viewp, BV, w.range_flag)) return rc;
    return launch<k_repack_feats>("k_repack_feats@gnr_prepare", st, dim3((npix + 63) / 64, BV), dim3(256), 0, s->ray_feats, s->img_feats, w.feat64, npix, w.range_flag);
}

// range guard of the pair form: bit 0 = a feature-map value beyond +-6e4 or not finite (k_repack_feats), bit 1 = an activation or
// cross-view statistic beyond the fp16 range inside a chain launch since the last gnr_prepare, bit 2 = a weight without an fp16 pair.
// Bits 0 and 2 concern every launch on the prepared scene (each is recomputed on the fp32-input MFMA; the pair kernel returns at once);
// bit 1 is kept per launch slot (volume, coarse pass, fine pass, training passes), so only the launches that tripped it are recomputed.
// The status is the OR over the slots.  Synchronises the stream.
extern "C" int gnr_range_status(const GnrScene* s, const void* ws, size_t ws_bytes, unsigned* flags_out, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!ws || !flags_out) return fail(GNR_ERR_ARG, "gnr_range_status: null pointer");
    Workspace w = carve(s, 0, 0, const_cast<void*>(ws));
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    unsigned words[RS_WORDS];                              // StatusSlot: word 0 scene-wide bits (feature, weight); then bit 1 of each launch slot, ...
    GNR_HIP(hipMemcpyAsync(words, w.range_flag, sizeof(words), hipMemcpyDeviceToHost, st));
    GNR_HIP(hipStreamSynchronize(st));
    unsigned f = 0;
    for (int i = 0; i < RS_WORDS; ++i) f |= words[i];
    *flags_out = f;
    return GNR_OK;
}

// byte offset of the 64 status words inside a workspace (callers that test GNR_STATUS_LOST_PARTNER on the device: graspnerf_amd/trainer.py)
extern "C" size_t gnr_status_words_offset(const GnrScene* s) {
    if (!s) return 0;
    char* const base = (char*)4096;                         // (carve leaves every pointer null for a null base)
    Workspace w = carve(s, 0, 0, base);
    return (size_t)((char*)w.range_flag - base);
}

// A library-owned second stream per device (GNR_OPT_SPLIT_LAUNCH), created on first use: fork / join events order it against the caller's
// stream, so the caller sees one stream-ordered call.  Not a setting: nothing a call computes depends on it.
struct SideStream { hipStream_t st = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
static SideStream* side_stream() {
    static SideStream tab[64];
    static std::atomic<unsigned long long> made{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    SideStream& e = tab[dev & 63];
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(made.load() & bit)) {
        static std::mutex mu;
        std::lock_guard<std::mutex> lk(mu);
        if (!(made.load() & bit)) {
            if (hipStreamCreateWithFlags(&e.st, hipStreamNonBlocking) != hipSuccess) return nullptr;
            if (hipEventCreateWithFlags(&e.fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess) return nullptr;
            made.fetch_or(bit);
        }
    }
    return &e;
}

static int volume_impl(const GnrScene* s, const float* bbox_min, int R, const float* wc, float* sdf_out,
                       unsigned char* vmask_out, void* ws, size_t ws_bytes, hipStream_t st, bool points, bool chain, bool ray,
                       float* dbg = nullptr) {
    if (int rc = check_points(s, (size_t)R * R * R)) return rc;
    Workspace w = carve(s, (size_t)R * R * R, 0, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    const int P = R * R * R;
    // the inference path's chain kernel computes the grid points itself (ChainArgs::pts_R); the per-column kernel never reads them: no k_points_volume
    const bool inline_pts = chain && ray && !dbg && R * R * R < (1 << 22);
    if (points && !inline_pts)
        if (int rc = launch<k_points_volume>("k_points_volume@volume_impl", st, dim3((s->B * P + 255) / 256), dim3(256), 0, bbox_min, w.desc, R, s->B)) return rc;
    // GNR_OPT_SPLIT_LAUNCH: scenes [0, B/2) on the caller's stream, [B/2, B) on the library's side stream: the second half's chain launch
    // starts on the CUs the first half's workgroups leave, the first half's per-column kernel on those the second half's leave
    const bool split = opt(s, GNR_OPT_SPLIT_LAUNCH) && chain && ray && !dbg && s->B >= 2;
    SideStream* side = split ? side_stream() : nullptr;
    if (split && !side) return fail(GNR_ERR_HIP, "side stream");
    const int nparts = split ? 2 : 1;
    if (split) { GNR_HIP(hipEventRecord(side->fork, st)); GNR_HIP(hipStreamWaitEvent(side->st, side->fork, 0)); }
    for (int part = 0; part < nparts; ++part) {
        const int b0 = part == 0 ? 0 : s->B / 2, nb = split ? (part == 0 ? s->B / 2 : s->B - s->B / 2) : s->B;
        hipStream_t ps = part == 0 ? st : side->st;
        if (chain) {
            ChainArgs a{wc, w.feat64, s->imgs, w.viewp, w.desc, w.rec, nullptr, vmask_out ? w.vmask_pts : nullptr, dbg,
                        nb, P, s->H, s->W, s->fh, s->fw, brick_order_ok(R) ? R : 0};
            a.b0 = b0;
            if (inline_pts) { a.bbox_min = bbox_min; a.pts_R = R; }
            wire_chain(a, s, w, RS_VOLUME, part);
            if (int rc = launch_chain<false>(s, a, ps)) return rc;
        }
        if (ray) {
            RayArgs r;
            memset(&r, 0, sizeof(r));
            const size_t ray0 = (size_t)b0 * R * R, pt0 = ray0 * R;
            r.wpk = wc; r.rec = w.rec + pt0 * REC_VOL; r.desc = w.desc + pt0 * DESC_FLOATS; r.vmask_pts = vmask_out ? w.vmask_pts + pt0 : nullptr;
            r.nrays = nb * R * R; r.dn = R; r.rays_per_scene = R * R; r.volume = sdf_out ? sdf_out + pt0 : nullptr; r.vmask_out = vmask_out ? vmask_out + pt0 : nullptr;
            if (int rc = launch_ray<false>(r, ps)) return rc;
        }
    }
    if (split) { GNR_HIP(hipEventRecord(side->join, side->st)); GNR_HIP(hipStreamWaitEvent(st, side->join, 0)); }
    return GNR_OK;
}

extern "C" int gnr_sample_volume_fwd(const GnrScene* s, const float* bbox_min, int R, const float* wc, float* sdf_out,
                                     unsigned char* vmask_out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!bbox_min || !wc || !sdf_out || !ws) return fail(GNR_ERR_ARG, "gnr_sample_volume_fwd: null pointer");
    if (R < 2 || R > MAX_DN) return fail(GNR_ERR_SHAPE, "volume_res must be in 2..64");
    return volume_impl(s, bbox_min, R, wc, sdf_out, vmask_out, ws, ws_bytes, (hipStream_t)stream, true, true, true);
}

// The SDF gradient volume (ibrnet.py:485-513: the VJP with ones of a column's SDF values w.r.t. its query points, which the reference's volume
// path computes and drops, aggregate_net.py:133-134): the volume's R^2 columns as rays of R samples through the render-record chain and
// k_ray<true>'s volume output mode.  Workspace = the region of a render call of R^2 rays x R samples + the chain's colour outputs (not used).
static size_t volume_grad_colors_bytes(const GnrScene* s, int R) { return al256((size_t)s->B * R * R * R * 3 * sizeof(float)); }
extern "C" size_t gnr_sample_volume_grad_workspace_bytes(const GnrScene* s, int R) {
    if (!s || R < 1 || R > MAX_DN) return 0;
    return carve(s, (size_t)R * R * R, (size_t)R * R, nullptr).total + volume_grad_colors_bytes(s, R);
}
extern "C" int gnr_sample_volume_grad_fwd(const GnrScene* s, const float* bbox_min, int R, const float* wc, float* grad_out, float* sdf_out,
                                          float* grad_error_out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!bbox_min || !wc || !grad_out || !ws) return fail(GNR_ERR_ARG, "gnr_sample_volume_grad_fwd: null pointer");
    if (R < 3 || R > MAX_DN) return fail(GNR_ERR_SHAPE, "gnr_sample_volume_grad_fwd: volume_res must be in 3..64 (the per-column kernel with the VJP takes 3 to 64 samples)");
    const int P = R * R * R, rn = R * R;
    if (int rc = check_points(s, (size_t)P)) return rc;
    Workspace w = carve(s, (size_t)P, (size_t)rn, ws);
    if (ws_bytes < w.total + volume_grad_colors_bytes(s, R)) return fail(GNR_ERR_WORKSPACE, "workspace too small (gnr_sample_volume_grad_workspace_bytes)");
    float* colors = (float*)((char*)ws + w.total);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch<k_points_volume>("k_points_volume@volume_grad", st, dim3((s->B * P + 255) / 256), dim3(256), 0, bbox_min, w.desc, R, s->B)) return rc;
    ChainArgs a{wc, w.feat64, s->imgs, w.viewp, w.desc, w.rec, colors, nullptr, nullptr, s->B, P, s->H, s->W, s->fh, s->fw, 0};
    wire_chain(a, s, w, RS_VOLUME_GRAD, TILE_CTR_VOLUME_GRAD);
    if (int rc = launch_chain<true>(s, a, st, "k_chain.render@volume_grad", "k_chain.render.fp32_twin@volume_grad")) return rc;
    RayArgs r;
    memset(&r, 0, sizeof(r));
    r.wpk = wc; r.rec = w.rec; r.desc = w.desc; r.nrays = s->B * rn; r.dn = R; r.rays_per_scene = rn;
    r.grad = grad_out; r.volume = sdf_out; r.gerr_part = grad_error_out ? w.gerr_part : nullptr;
    r.range_word = w.range_flag ? w.range_flag + RS_VOLUME_GRAD_RAY : nullptr;
    if (int rc = launch_ray<true, true>(r, st)) return rc;
    if (grad_error_out)
        return launch<k_gerr_reduce>("k_gerr_reduce@volume_grad", st, dim3(s->B, 1), dim3(256), 0, w.gerr_part, grad_error_out, rn, R, rn);
    return GNR_OK;
}

// bring-up aid: per-point intermediates of k_chain on the volume points, point (column) order.
// dbg[B*res^3][32]: [0..V) hit, [8..8+V) vis, [16..16+V) v2, [24] n_valid, [25] wbar, [26] mean f0,
// [27] var f0, [28] mean0 of rgb ch0, [29] base_fc.0 hoisted pre-activation f0, [30] geometry_fc out f0, [31] sum v2
extern "C" int gnr_debug_volume_chain(const GnrScene* s, const float* bbox_min, int R, const float* wc, float* dbg,
                                      void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!bbox_min || !wc || !dbg || !ws) return fail(GNR_ERR_ARG, "gnr_debug_volume_chain: null pointer");
    return volume_impl(s, bbox_min, R, wc, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream, true, true, false, dbg);
}

// Morton order of the scene's rays for the inference render passes (k_ray_order): -> w.ray_perm, or null when a scene has
// more rays than the sort's LDS holds (the passes then run in the caller's order, as before)
static int order_rays(const GnrScene* s, const GnrRays* q, Workspace& w, hipStream_t st, const int** perm_out) {
    *perm_out = nullptr;
    if (!opt(s, GNR_OPT_RAY_ORDER_MORTON) || q->rn > MAX_SORT_RAYS || q->rn < 2) return GNR_OK;
    int shift = 0;
    while (((s->W > s->H ? s->W : s->H) >> shift) > 1024) ++shift;
    if (int rc = launch<k_ray_order>("k_ray_order@render_pass", st, dim3(s->B), dim3(256), 0, q->coords, w.ray_perm, q->rn, shift)) return rc;
    *perm_out = w.ray_perm;
    return GNR_OK;
}

// View-mask order of a render pass's samples (csrc/gnr_sample_order.h) behind its k_points_rays: -> w.sample_perm, or null = natural order:
//   GNR_OPT_SAMPLE_ORDER_NATURAL;  more than MAX_SORT_SAMPLES samples per scene;  a launch of fewer than SAMPLE_ORDER_MIN_TILES_PER_SLOT tiles
//   per wavefront slot of the device.  Measured at 512 rays x 40 (0.625 B tiles per slot; profiles/sample_order_ab.json): the two chain launches
//   of a step gain 0.00 / 0.04 / 0.04 / 0.07 / 0.22 ms at B = 1 / 2 / 4 / 8 / 32, and the two sorts of the EARLIER kernel (one workgroup per
//   scene, 43 us a launch) cost 0.09 ms at every B: the step lost 0.05 ms at B = 4, 0.02 at B = 8 and won 0.10 at B = 32; break-even near
//   B = 12 = 7.5 tiles per slot.  k_sample_order now runs one workgroup per SO_CHUNK samples; its break-even has NOT been measured yet
//   (profiles/sample_place_ab.json), so the constant stays at the last measured one.  Not below 1: less than a tile per slot has no order to gain.
constexpr int SAMPLE_ORDER_MIN_TILES_PER_SLOT = 8;
static bool sample_order_wanted(const GnrScene* s, const Workspace& w, int P) {
    if (opt(s, GNR_OPT_SAMPLE_ORDER_NATURAL) || !w.sample_perm || !w.sample_keys || P > MAX_SORT_SAMPLES) return false;
    const long ntiles = (long)s->B * ((P + 15) / 16), slots = (long)num_cus() * (kChainThreads / 64);
    return ntiles >= SAMPLE_ORDER_MIN_TILES_PER_SLOT * slots;
}
static int launch_sample_order(const unsigned char* keys, int* perm, int B, int P, hipStream_t st) {
    return launch<k_sample_order>("k_sample_order@render_pass", st, dim3((P + SO_CHUNK - 1) / SO_CHUNK, B), dim3(SO_THREADS), 0, keys, perm, P);
}
// The per-ray kernel's arguments for a render pass (inference: render_pass; training: gnr_render_tail_fwd_train) on the records the pass's
// chain left in the workspace; desc = the pass's point descriptors.  The caller adds the resampler's outputs and the ray order.
static RayArgs render_ray_args(const GnrScene* s, const GnrRays* q, const float* depth, int dn, const float* wl, const GnrRenderOut* out,
                               const Workspace& w, const float* desc) {
    RayArgs r;
    memset(&r, 0, sizeof(r));
    r.wpk = wl; r.rec = w.rec; r.desc = desc; r.depth = depth; r.colors = out->colors_nr; r.que_dr = q->que_depth_range;
    r.nrays = s->B * q->rn; r.dn = dn; r.rays_per_scene = q->rn;
    r.sdf = out->sdf_values; r.alpha = out->alpha_values; r.hit = out->hit_prob_nr; r.pix = out->pixel_colors_nr;
    r.rdepth = out->render_depth; r.gerr_part = out->sdf_gradient_error ? w.gerr_part : nullptr; r.grad = out->sdf_gradient;
    r.rmask = out->ray_mask; r.view_num = q->ray_mask_view_num; r.point_num = q->ray_mask_point_num;
    r.range_word = w.range_flag ? w.range_flag + RS_RAY_WATCH : nullptr;
    return r;
}
// ... and what follows that kernel: the chunk means of the eikonal term and the rays' ground-truth colours (want_gt; gt_also: a second copy)
static int render_ray_epilogue(const GnrScene* s, const GnrRays* q, const GnrRenderOut* out, int dn, const Workspace& w, const char* gerr_label,
                               const char* gt_label, bool want_gt, float* gt_also, hipStream_t st) {
    const int B = s->B, rn = q->rn;
    if (out->sdf_gradient_error) {
        const int chunk = q->ray_batch_num > 0 ? q->ray_batch_num : rn;
        if (int rc = launch<k_gerr_reduce>(gerr_label, st, dim3(B, (rn + chunk - 1) / chunk), dim3(256), 0, w.gerr_part, out->sdf_gradient_error, rn, dn, chunk)) return rc;
    }
    if (out->pixel_colors_gt && q->que_imgs && want_gt)
        if (int rc = launch<k_pixel_gt>(gt_label, st, dim3((B * rn + 255) / 256), dim3(256), 0, q->que_imgs, q->coords, out->pixel_colors_gt, rn, s->H, s->W, B, gt_also)) return rc;
    return GNR_OK;
}
// gt_also / skip_gt: the ground-truth colours of the rays are the same in both passes of gnr_render_rays_fwd: the coarse pass's launch writes
// the fine pass's array too (gt_also), the fine pass skips its own (skip_gt)
static int render_pass(const GnrScene* s, const GnrRays* q, const float* depth, int dn, const float* wl, GnrRenderOut* out,
                       Workspace& w, hipStream_t st, float* fine_depth, int* fine_inds, int fdn, const float* fine_u = nullptr,
                       const int* perm = nullptr, int range_slot = RS_COARSE, float* gt_also = nullptr, bool skip_gt = false, bool gen_depth = false,
                       const int* sample_perm_in = nullptr) {      // sample_perm_in: gnr_debug_render_by_depth_perm (a caller-given order instead of the pass's own)
    if (!out || !out->colors_nr) return fail(GNR_ERR_ARG, "GnrRenderOut.colors_nr is required");
    const int B = s->B, rn = q->rn;
    const int P = rn * dn;
    const bool ordered = !sample_perm_in && sample_order_wanted(s, w, P);      // the pass's own view-mask order: keys from k_points_rays, then the sort
    if (int rc = launch<k_points_rays>("k_points_rays@render_pass", st, dim3((B * P + 255) / 256), dim3(256), 0, q->coords, q->que_pose, q->que_K,
                                       q->que_depth_range, depth, w.desc, rn, dn, B, perm, gen_depth ? const_cast<float*>(depth) : nullptr,     // gen_depth: the coarse pass's depths are generated here, into `depth`
                                       ordered ? w.sample_keys : nullptr, w.viewp, s->V, s->H, s->W)) return rc;
    if (ordered)
        if (int rc = launch_sample_order(w.sample_keys, w.sample_perm, B, P, st)) return rc;
    ChainArgs a{wl, w.feat64, s->imgs, w.viewp, w.desc, w.rec, out->colors_nr, out->view_mask, nullptr,
                B, P, s->H, s->W, s->fh, s->fw, 0};
    wire_chain(a, s, w, range_slot);                       // watch word of this pass (RS_COARSE: coarse / by-depth, RS_FINE)
    a.ray_perm = perm; a.perm_rn = rn; a.perm_dn = dn;
    a.sample_perm = ordered ? w.sample_perm : sample_perm_in;
    if (int rc = launch_chain<true>(s, a, st)) return rc;
    RayArgs r = render_ray_args(s, q, depth, dn, wl, out, w, w.desc);
    r.fine_depth = fine_depth; r.fine_inds = fine_inds; r.fdn = fdn; r.fine_u = fine_u; r.ray_perm = perm;
    if (int rc = launch_ray<true>(r, st)) return rc;
    if (int rc = render_ray_epilogue(s, q, out, dn, w, "k_gerr_reduce@render_pass", "k_pixel_gt@render_pass", !skip_gt, gt_also, st)) return rc;
    if (out->depth && out->depth != depth)
        GNR_HIP(hipMemcpyAsync(out->depth, depth, (size_t)B * P * sizeof(float), hipMemcpyDeviceToDevice, st));
    return GNR_OK;
}

// by_depth: the entry point takes its sample count as an argument; GnrRays.dn / .fdn are not used
static int check_rays(const GnrRays* q, bool by_depth = false) {
    if (!q || !q->coords || !q->que_pose || !q->que_K || !q->que_depth_range) return fail(GNR_ERR_ARG, "GnrRays: null pointer");
    if (q->rn < 1) return fail(GNR_ERR_SHAPE, "GnrRays: rn must be positive");
    if (!by_depth && (q->dn < 3 || q->dn > MAX_DN || q->fdn < 1 || q->fdn > MAX_DN)) return fail(GNR_ERR_SHAPE, "GnrRays: dn/fdn must be in 3..64");
    if (q->fine_depth_use_all != 0 && q->fine_depth_use_all != 1) return fail(GNR_ERR_ARG, "GnrRays: fine_depth_use_all must be 0 or 1");
    if (q->ray_batch_num < 0) return fail(GNR_ERR_SHAPE, "GnrRays: ray_batch_num must be >= 0");
    return GNR_OK;
}

extern "C" int gnr_render_by_depth_fwd(const GnrScene* s, const GnrRays* q, const float* depth, int dn, const float* wl,
                                       GnrRenderOut* out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (int rc = check_rays(q, true)) return rc;
    if (!depth || !wl || !ws) return fail(GNR_ERR_ARG, "gnr_render_by_depth_fwd: null pointer");
    if (dn < 3 || dn > MAX_DN_FWD) return fail(GNR_ERR_SHAPE, "dn must be in 3..128");
    if (int rc = check_points(s, (size_t)q->rn * dn)) return rc;
    Workspace w = carve(s, (size_t)q->rn * dn, q->rn, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    const int* perm = nullptr;
    if (int rc = order_rays(s, q, w, (hipStream_t)stream, &perm)) return rc;
    return render_pass(s, q, depth, dn, wl, out, w, (hipStream_t)stream, nullptr, nullptr, 0, nullptr, perm);
}

// Test tooling: gnr_render_by_depth_fwd with a caller-given order of every scene's samples (sample_perm [B][rn*dn] int32 on the device, each
// row a permutation of 0 .. rn*dn-1) in place of the pass's own: the outputs do not depend on it.
extern "C" int gnr_debug_render_by_depth_perm(const GnrScene* s, const GnrRays* q, const float* depth, int dn, const float* wl,
                                              GnrRenderOut* out, const int* sample_perm, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (int rc = check_rays(q, true)) return rc;
    if (!depth || !wl || !ws || !sample_perm) return fail(GNR_ERR_ARG, "gnr_debug_render_by_depth_perm: null pointer");
    if (dn < 3 || dn > MAX_DN_FWD) return fail(GNR_ERR_SHAPE, "dn must be in 3..128");
    if (int rc = check_points(s, (size_t)q->rn * dn)) return rc;
    Workspace w = carve(s, (size_t)q->rn * dn, q->rn, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    const int* perm = nullptr;
    if (int rc = order_rays(s, q, w, (hipStream_t)stream, &perm)) return rc;
    return render_pass(s, q, depth, dn, wl, out, w, (hipStream_t)stream, nullptr, nullptr, 0, nullptr, perm, RS_COARSE, nullptr, false, false, sample_perm);
}

// Test tooling: the device sort alone -- keys [B][P] bytes on the device -> perm [B][P] int32 (what a render pass builds from its own keys;
// no threshold).  gnr_sample_order_host: the same permutation of one scene on the host (csrc/gnr_sample_order.h; no device work).
// gnr_sample_order_offsets: byte offsets of the keys [B][P] and the permutation [B][P] of the LAST render pass inside a workspace that was
// carved for P = rn * dn_max samples per scene (gnr_workspace_bytes' arguments); GNR_ERR_SHAPE when such a workspace has neither.
extern "C" int gnr_debug_sample_order(const unsigned char* keys, int B, int P, int* perm, void* stream) {
    if (!keys || !perm) return fail(GNR_ERR_ARG, "gnr_debug_sample_order: null pointer");
    if (B < 1 || P < 1 || P > MAX_SORT_SAMPLES) return fail(GNR_ERR_SHAPE, "gnr_debug_sample_order: 1 <= P <= 2^18 samples per scene");
    return launch_sample_order(keys, perm, B, P, (hipStream_t)stream);
}
extern "C" int gnr_sample_order_host(const unsigned char* keys, int P, int* perm_out) {
    if (!keys || !perm_out) return fail(GNR_ERR_ARG, "gnr_sample_order_host: null pointer");
    if (P < 1) return fail(GNR_ERR_SHAPE, "gnr_sample_order_host: P must be positive");
    int start[256], hist[256] = {0};
    for (int i = 0; i < P; ++i) ++hist[keys[i]];
    for (int k = 0; k < 256; ++k) {
        start[k] = 0;
        for (int k2 = 0; k2 < 256; ++k2) if (sorder::key_before(k2, k)) start[k] += hist[k2];
    }
    for (int i = 0; i < P; ++i) perm_out[sorder::slot_of(start[keys[i]]++, P)] = i;
    return GNR_OK;
}
// gnr_sample_order_host_chunked: the placement by chunks of `chunk` samples (csrc/gnr_sample_order.h) as k_sample_order runs it, one chunk
// after the other: every chunk counts the scene's keys again -- in front of it and from it on -- and places its samples from those counts.
extern "C" int gnr_sample_order_host_chunked(const unsigned char* keys, int P, int chunk, int* perm_out) {
    if (!keys || !perm_out) return fail(GNR_ERR_ARG, "gnr_sample_order_host_chunked: null pointer");
    if (P < 1 || chunk < 1) return fail(GNR_ERR_SHAPE, "gnr_sample_order_host_chunked: P and chunk must be positive");
    for (int c0 = 0; c0 < P; c0 += chunk) {
        int before[sorder::KEYS] = {0}, rest[sorder::KEYS] = {0}, by_rank[sorder::KEYS], scan[sorder::KEYS], in_chunk[sorder::KEYS] = {0};
        for (int i = 0; i < P; ++i) ++(i < c0 ? before : rest)[keys[i]];
        for (int k = 0; k < sorder::KEYS; ++k) by_rank[sorder::key_rank(k)] = before[k] + rest[k];
        for (int r = 0, run = 0; r < sorder::KEYS; ++r) { scan[r] = run; run += by_rank[r]; }
        for (int i = c0; i < P && i - c0 < chunk; ++i) perm_out[sorder::slot_of(sorder::chunk_pos(scan, before, keys[i], in_chunk[keys[i]]++), P)] = i;
    }
    return GNR_OK;
}
extern "C" int gnr_sample_order_offsets(const GnrScene* s, int rn, int dn_max, size_t* keys_off, size_t* perm_off) {
    if (!s || !keys_off || !perm_off) return fail(GNR_ERR_ARG, "gnr_sample_order_offsets: null pointer");
    if (rn < 1 || dn_max < 1) return fail(GNR_ERR_SHAPE, "gnr_sample_order_offsets: rn, dn_max must be positive");
    char* const base = (char*)4096;
    Workspace w = carve(s, (size_t)rn * dn_max, rn, base);
    if ((size_t)rn * dn_max > (size_t)MAX_SORT_SAMPLES) return fail(GNR_ERR_SHAPE, "gnr_sample_order_offsets: more samples per scene than the sort handles");
    *keys_off = (size_t)((char*)w.sample_keys - base); *perm_off = (size_t)((char*)w.sample_perm - base);
    return GNR_OK;
}

extern "C" int gnr_render_rays_fwd(const GnrScene* s, const GnrRays* q, const float* wc, const float* wf, GnrRenderOut* coarse,
                                   GnrRenderOut* fine, const float* fine_depth_in, int* fine_inds_out, void* ws, size_t ws_bytes,
                                   void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (int rc = check_rays(q)) return rc;
    // fine == NULL: cfg use_hierarchical_sampling false (renderer.py:153-162: render_impl returns the coarse pass's outputs only --
    // no inverse-CDF resampling, no fine pass; packed_fine is not read)
    if (!wc || !coarse || !ws || (fine && !wf)) return fail(GNR_ERR_ARG, "gnr_render_rays_fwd: null pointer");
    if (!fine && (fine_depth_in || fine_inds_out)) return fail(GNR_ERR_ARG, "gnr_render_rays_fwd: fine depths / indices without a fine pass");
    hipStream_t st = (hipStream_t)stream;
    // fine_depth_use_all: the fine pass renders the dn coarse + fdn resampled depths of a ray, merged (renderer.py:145-146)
    const int fine_dn = !fine ? 0 : (q->fine_depth_use_all ? q->dn + q->fdn : q->fdn);
    const int dmax = q->dn > fine_dn ? q->dn : fine_dn;
    if (int rc = check_points(s, (size_t)q->rn * dmax)) return rc;
    Workspace w = carve(s, (size_t)q->rn * dmax, q->rn, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    const int B = s->B;
    // the depths of a pass are generated straight into the caller's output array when there is one (same [B,rn,dn] layout as the workspace
    // copy: no device-to-device copy at the end of the pass)
    float* depth_c = coarse->depth ? coarse->depth : w.depth_c;
    // (the coarse depths are generated by the coarse pass's k_points_rays: gen_depth)
    const int* perm = nullptr;                             // both passes render the same rays: one sort
    if (int rc = order_rays(s, q, w, st, &perm)) return rc;
    if (!fine) return render_pass(s, q, depth_c, q->dn, wc, coarse, w, st, nullptr, nullptr, 0, nullptr, perm, RS_COARSE, nullptr, false, true);
    float* depth_f = (fine->depth && !fine_depth_in && !q->fine_depth_use_all) ? fine->depth : w.depth_f;     // the coarse pass's resampled depths
    const bool one_gt = coarse->pixel_colors_gt && fine->pixel_colors_gt && q->que_imgs && coarse->pixel_colors_gt != fine->pixel_colors_gt;
    if (int rc = render_pass(s, q, depth_c, q->dn, wc, coarse, w, st, depth_f, fine_inds_out, q->fdn, q->fine_u, perm, RS_COARSE,
                             one_gt ? fine->pixel_colors_gt : nullptr, false, true)) return rc;
    const float* fdepth = fine_depth_in ? fine_depth_in : depth_f;          // fine_depth_in: [B,rn,fine_dn], sorted
    if (q->fine_depth_use_all && !fine_depth_in) {
        const int n = B * q->rn * fine_dn;
        float* depth_m = fine->depth ? fine->depth : w.depth_m;
        if (int rc = launch<k_merge_depths>("k_merge_depths@gnr_render_rays_fwd", st, dim3((n + 255) / 256), dim3(256), 0, depth_c, depth_f, depth_m, B * q->rn, q->dn, q->fdn)) return rc;
        fdepth = depth_m;
    }
    return render_pass(s, q, fdepth, fine_dn, wf, fine, w, st, nullptr, nullptr, 0, nullptr, perm, RS_FINE, nullptr, one_gt);
}

// predict_mean_for_depth_loss (renderer.py:222-266) for one level; uses feat64 from gnr_prepare.
// fine_depth_use_all under training (renderer.py:145-146): sort(cat(coarse depths, resampled depths)) per ray as a rank merge of the two
// ascending lists (k_merge_depths: the kernel the inference entry point runs inside gnr_render_rays_fwd)
extern "C" int gnr_merge_depths(const float* depth_a, int na, const float* depth_b, int nb, float* out, int nrays, void* stream) {
    if (!depth_a || !depth_b || !out) return fail(GNR_ERR_ARG, "gnr_merge_depths: null pointer");
    if (nrays < 1 || na < 1 || nb < 1 || na + nb > MAX_DN_FWD) return fail(GNR_ERR_SHAPE, "gnr_merge_depths: 1 <= na, nb and na + nb <= 128");
    const long n = (long)nrays * (na + nb);
    if (n > ((long)1 << 31) - 1024) return fail(GNR_ERR_SHAPE, "gnr_merge_depths: too many samples in one call");
    return launch<k_merge_depths>("k_merge_depths@gnr_merge_depths", (hipStream_t)stream, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, depth_a, depth_b, out, nrays, na, nb);
}

extern "C" int gnr_depth_mean_fwd(const GnrScene* s, const float* coords, int pn, const float* level_weights, float* mean_out,
                                  void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!coords || !level_weights || !mean_out || !ws) return fail(GNR_ERR_ARG, "gnr_depth_mean_fwd: null pointer");
    if (pn < 1) return fail(GNR_ERR_SHAPE, "pn must be positive");
    Workspace w = carve(s, 0, 0, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    DepthMeanArgs a{level_weights, w.feat64, coords, mean_out, s->B, s->V, pn, s->H, s->W, s->fh, s->fw};
    const long tiles = (long)s->B * s->V * ((pn + 15) / 16);
    return launch<k_depth_mean>("k_depth_mean@gnr_depth_mean_fwd", (hipStream_t)stream, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, a);
}

// backward of gnr_depth_mean_fwd for one level.  dmean [B,V,pn,2]; gradients are ACCUMULATED into
// d_canonical [gnr_canonical_weights_floats()] and, through the workspace's channel-last buffer, written to
// d_ray_feats [B,V,32,fh,fw] (overwritten; may be null).
// scratch for the channel-last feature-map gradient of gnr_depth_mean_bwd (caller-owned, separate from the workspace
// so that the states of a pending gnr_sample_volume_bwd in the workspace stay intact)
static size_t depth_mean_part_bytes() { return al256((size_t)2 * num_cus() * 4 * DM_STRIDE * sizeof(float)); }
extern "C" size_t gnr_depth_mean_bwd_workspace_bytes(const GnrScene* s) {
    if (!s) return 0;
    return feat_grad_bytes(s) + depth_mean_part_bytes();
}

extern "C" int gnr_depth_mean_bwd(const GnrScene* s, const float* coords, int pn, const float* level_weights,
                                  const float* level_weights_bwd, const float* dmean, float* d_canonical, float* d_ray_feats,
                                  void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!coords || !level_weights || !level_weights_bwd || !dmean || !d_canonical || !ws)
        return fail(GNR_ERR_ARG, "gnr_depth_mean_bwd: null pointer");
    if (pn < 1) return fail(GNR_ERR_SHAPE, "pn must be positive");
    Workspace w = carve(s, 0, 0, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    if (!scratch || scratch_bytes < gnr_depth_mean_bwd_workspace_bytes(s))
        return fail(GNR_ERR_WORKSPACE, "gnr_depth_mean_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    float* dpart = (float*)scratch;                                             // partial mean_decoder gradients, then the feature-gradient buffer
    FeatGradBuf fg{nullptr, FeatFx{nullptr, nullptr}, false};
    if (d_ray_feats)
        if (int rc = feat_grad_begin(s, (char*)scratch + depth_mean_part_bytes(), w, dmean, (size_t)s->B * s->V * pn * 2, st, &fg)) return rc;
    const int ntiles = s->B * s->V * ((pn + 15) / 16);
    DepthMeanBwdArgs a{level_weights, level_weights_bwd, w.feat64, coords, dmean, fg.buf, dpart,
                       s->B, s->V, pn, s->H, s->W, s->fh, s->fw, ntiles, fg.fx};
    int blocks = (ntiles + 3) / 4;
    const int cap = 2 * num_cus();
    if (blocks > cap) blocks = cap;
    if (int rc = poison_partials(dpart, (size_t)blocks * 4 * DM_STRIDE * sizeof(float), st, s->options)) return rc;
    if (int rc = fg.fixed ? launch<k_depth_mean_bwd<true>>("k_depth_mean_bwd@gnr_depth_mean_bwd", st, dim3(blocks), dim3(256), 0, a)
                          : launch<k_depth_mean_bwd<false>>("k_depth_mean_bwd@gnr_depth_mean_bwd", st, dim3(blocks), dim3(256), 0, a)) return rc;
    {
        const GradRange rg[1] = {{can::MEAN0_W, can::VAR0_W, can::MEAN0_W}};
        if (int rc = launch_grad_reduce(dpart, blocks * 4, DM_STRIDE, d_canonical, rg, 1, st, "k_grad_reduce@gnr_depth_mean_bwd")) return rc;
    }
    if (fg.buf)
        if (int rc = feat_grad_unpack(s, fg, d_ray_feats, nullptr, "k_unpack_feat_grad@gnr_depth_mean_bwd", st)) return rc;
    return GNR_OK;
}

// ---- training forward + backward of sample_volume ---------------------------------------------------------
// Training workspace (caller-owned, lives from the training forward to the backward): saved per-view states and
// the inter-stage gradients.  Offsets in bytes, see gnr_train_workspace_layout().
struct TrainWs { size_t save1, save2, saveG, dg16, dS2, dG, dS1, dfeat64, dtail, dpart, dtail_part, scatter, total; };
static TrainWs carve_train(const GnrScene* s, int R) {
    TrainWs t;
    const size_t P = (size_t)R * R * R, T = (size_t)s->B * ((P + 15) / 16), V = s->V;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off += al256(floats * sizeof(float)); return o; };
    t.save1 = take(T * V * 19 * 64);
    t.save2 = take(T * V * 9 * 64);
    t.saveG = take(T * 17 * 64);
    t.dg16 = take((size_t)s->B * P * 16);
    t.dS2 = take(T * V * 9 * 64);
    t.dG = take(T * 16 * 64);
    t.dS1 = take(T * V * DS1 * 64);
    t.dfeat64 = take(feat_grad_bytes(s) / sizeof(float));  // (8-byte entries: the fixed-point mode's)
    t.dtail = take(tl::TOTAL);
    t.dpart = take(chain_part_floats());                   // partial parameter gradients of stages 4..1 (csrc/gnr_bwd.inc)
    t.dtail_part = take(tail_part_floats(4));              // ... of the tail (stage 5)
    t.scatter = take(carve_scatter(s, T).total / sizeof(float));   // binned scatter of the feature-map gradient (gnr_bwd_scatter.inc)
    t.total = off;
    return t;
}

extern "C" size_t gnr_sample_volume_train_workspace_bytes(const GnrScene* s, int R) {
    if (!s || R < 2 || R > MAX_DN) return 0;
    return carve_train(s, R).total;
}

// byte offsets of {save1, save2, saveG, dg16, dS2, dG, dS1, dfeat64, dtail} inside the training workspace (tests, tooling)
extern "C" int gnr_train_workspace_layout(const GnrScene* s, int R, size_t* out9) {
    if (!s || !out9) return GNR_ERR_ARG;
    const TrainWs t = carve_train(s, R);
    const size_t v[9] = {t.save1, t.save2, t.saveG, t.dg16, t.dS2, t.dG, t.dS1, t.dfeat64, t.dtail};
    for (int i = 0; i < 9; ++i) out9[i] = v[i];
    return GNR_OK;
}

// sample_volume forward that also saves what the backward needs (same values as gnr_sample_volume_fwd)
extern "C" int gnr_sample_volume_fwd_train(const GnrScene* s, const float* bbox_min, int R, const float* wc, float* sdf_out,
                                           void* ws, size_t ws_bytes, void* tws, size_t tws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!bbox_min || !wc || !sdf_out || !ws || !tws) return fail(GNR_ERR_ARG, "gnr_sample_volume_fwd_train: null pointer");
    if (R < 2 || R > MAX_DN) return fail(GNR_ERR_SHAPE, "volume_res must be in 2..64");
    const TrainWs t = carve_train(s, R);
    if (tws_bytes < t.total) return fail(GNR_ERR_WORKSPACE, "training workspace too small");
    if (int rc = check_points(s, (size_t)R * R * R)) return rc;
    Workspace w = carve(s, (size_t)R * R * R, 0, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int P = R * R * R;
    if (int rc = launch<k_points_volume>("k_points_volume@gnr_sample_volume_fwd_train", st, dim3((s->B * P + 255) / 256), dim3(256), 0, bbox_min, w.desc, R, s->B)) return rc;
    char* tb = (char*)tws;
    ChainArgs a{wc, w.feat64, s->imgs, w.viewp, w.desc, w.rec, nullptr, nullptr, nullptr, s->B, P, s->H, s->W, s->fh, s->fw,
                brick_order_ok(R) ? R : 0, (float*)(tb + t.save1), (float*)(tb + t.save2), (float*)(tb + t.saveG)};
    wire_chain(a, s, w, RS_VOLUME_TRAIN);
    if (int rc = launch_chain<false, true>(s, a, st)) return rc;
    RayArgs r;
    memset(&r, 0, sizeof(r));
    r.wpk = wc; r.rec = w.rec; r.desc = w.desc;
    r.nrays = s->B * R * R; r.dn = R; r.rays_per_scene = R * R; r.volume = sdf_out;
    return launch_ray<false>(r, st);
}

// One launch of the second view loop's backward: the kernel of the call's options (partner wavefronts by default) under the range
// guard, and behind it the fp32-input-MFMA instantiation of k_view2_bwd (launch_view1_bwd has the scheme).  The render pass's
// single-wavefront kernel IS the fp32 instantiation: with GNR_OPT_VIEW2_ONE_WAVEFRONT it serves both sides of the flag in one launch.
template <bool RENDER>
static int launch_view2_bwd(const GnrScene* s, const Workspace& w, const BwdEntry& e, View2BwdArgs a, int blocks, hipStream_t st) {
    constexpr size_t lds1 = (RENDER ? l3::TOTAL_RENDER : l3::TOTAL) * sizeof(float), ldsp = l3p::total(RENDER) * sizeof(float);
    const bool f32 = opt(s, GNR_OPT_FP32_CHAIN);
    const bool pw = view2_partner(s);
    const bool single_is_f32 = RENDER && !pw;               // k_view2_bwd<true> has no pair form
    if (!f32 && !single_is_f32) {
        a.guard = bwd_guard(s, w, e, 1);
        if (pw) {
            if (int rc = launch<k_view2_bwd_pw<RENDER>, ldsp>(e.view2, st, dim3(blocks), dim3(512), ldsp, a)) return rc;
        } else if constexpr (!RENDER) {
            if (int rc = launch<k_view2_bwd<false, true>, lds1>(e.view2, st, dim3(blocks), dim3(256), lds1, a)) return rc;
        }
    }
    const bool always = f32 || single_is_f32;
    a.guard = bwd_guard(s, w, e, always ? 0 : 2);
    if (!always && !a.guard.run_if) return GNR_OK;
    return launch<k_view2_bwd<RENDER, false>, lds1>(always ? e.view2 : e.view2_twin, st, dim3(blocks), dim3(256), lds1, a);
}

// dynamic LDS of k_geo_bwd / k_hoist_bwd: their weight fragments + two tiles per wavefront.  (Their timing labels, and k_red2_bwd's, end in
// "@launch_<kernel>_bwd", not in an entry point's name: tools/ and profiles/ key on the labels as they are.)
constexpr size_t GEO_BWD_LDS = (frag_floats(23, 4) + frag_floats(16, 1) + 64 + 16 + frag_floats(16, 4) + frag_floats(16, 1) + frag_floats(4, 4) +
                                4 * 2 * 16 * TS2) * sizeof(float);
constexpr size_t HOIST_BWD_LDS = (2 * frag_floats(16, 4) + frag_floats(16, 1) + 4 * 2 * 16 * TS3) * sizeof(float);

// The parameter stages of a chain backward run the same grid (chain_blocks): one slot of the partial-gradient buffer per wavefront, summed
// once at the end (chain_bwd).  A partial run (tests: stage by stage) leaves ranges of the slots unwritten: zero them; a full run stores
// every entry (GNR_OPT_POISON_PARTIALS shows one that it does not).
static int chain_partials_begin(const GnrScene* s, float* dpart, int ntiles, int stages, hipStream_t st) {
    const size_t bytes = (size_t)chain_blocks(ntiles) * 4 * GP_STRIDE * sizeof(float);
    if ((stages & 15) == 0) return GNR_OK;
    if ((stages & 15) != 15) { GNR_HIP(hipMemsetAsync(dpart, 0, bytes, st)); return GNR_OK; }
    return poison_partials(dpart, bytes, st, s->options);
}

// The stages gnr_sample_volume_bwd and gnr_render_chain_bwd share, behind the stages of their own: second view loop (stages bit 2) ->
// hoisted columns + first reduction (bit 1) -> first view loop + feature-map gradients (bit 0) -> the fixed-order sum of the partial
// parameter gradients into d_canonical.  BwdWs: the sections of the entry's training workspace they work on; desc = the P points' descriptors.
struct BwdWs { const float *desc, *save1, *saveG, *dS2; float *dG, *dS1, *dpart; char *dfeat64, *scatter; };
static int chain_bwd(const GnrScene* s, const Workspace& w, const BwdEntry& e, const BwdWs& t, const float* wl, const float* wb, int P, int stages,
                     float* d_canonical, float* d_ray_feats, float* d_img_feats, hipStream_t st) {
    const int ntiles = s->B * ((P + 15) / 16), blocks = chain_blocks(ntiles);
    if (stages & 4) {                                    // stage 3: second view loop
        View2BwdArgs a{wl, wb, t.save1, t.saveG, t.dS2, t.dS1, t.dG, t.dpart, s->V, ntiles, nullptr, nullptr, 0, 0, 0};
        if (!e.volume) { a.desc = t.desc; a.viewp = w.viewp; a.P = P; a.H = s->H; a.W = s->W; }     // (the colour head needs the direction differences)
        if (int rc = e.volume ? launch_view2_bwd<false>(s, w, e, a, blocks, st) : launch_view2_bwd<true>(s, w, e, a, blocks, st)) return rc;
    }
    if (stages & 2) {                                    // stage 2: hoisted columns + first reduction
        HoistBwdArgs a{wb, t.save1, t.saveG, t.dG, t.dS1, t.dpart, ntiles};
        if (int rc = with_views(s->V, [&](auto v) {
                return launch<k_hoist_bwd<decltype(v)::value>, HOIST_BWD_LDS>("k_hoist_bwd@launch_hoist_bwd", st, dim3(blocks), dim3(256), HOIST_BWD_LDS, a);
            })) return rc;
    }
    if (stages & 1) {                                    // stage 1: first view loop + feature-map gradients
        FeatGradBuf fg;
        const BwdGuard gmax = bwd_guard(s, w, e, 2);
        if (int rc = feat_grad_begin(s, t.dfeat64, w, t.dS1, (size_t)ntiles * s->V * DS1 * 64, st, &fg, (view1_bins(s) && gmax.run_if) ? &gmax : nullptr)) return rc;
        View1BwdArgs a{wl, wb, w.feat64, w.viewp, t.desc, t.dS1, fg.buf, t.dpart,
                       s->B, s->V, P, s->H, s->W, s->fh, s->fw, ntiles, e.volume ? 0 : 1, fg.fx};
        if (int rc = launch_view1_bwd(s, w, e, a, fg.fixed, ntiles, t.scatter, st)) return rc;
        if (d_ray_feats || d_img_feats)
            if (int rc = feat_grad_unpack(s, fg, d_ray_feats, d_img_feats, e.unpack, st)) return rc;
    }
    if (stages & 15)                                     // every entry of every slot was stored by exactly one of the stages (or zeroed in a partial run)
        return launch_grad_reduce(t.dpart, blocks * 4, GP_STRIDE, d_canonical, e.rg, s->use_vis ? 3 : 2, st, e.reduce);
    return GNR_OK;
}

// out_geometry_fc.{0,1} and the attention / LayerNorm gradients from the tail accumulators into the canonical blob
__global__ void k_tail_unfold(const float* __restrict__ dtail, const float* __restrict__ canon, float* __restrict__ dcanon) {
    const int t = threadIdx.x;                     // 256 threads
    dcanon[can::WQ + t] += dtail[tl::WQ + t];
    dcanon[can::WK + t] += dtail[tl::WK + t];
    dcanon[can::WV + t] += dtail[tl::WV + t];
    dcanon[can::WFC + t] += dtail[tl::WFC + t];
    const float sds = dtail[tl::SDS];
    // s = w1 . (W0 n + b0) + b1 :  dW0[k][c] = w1[k] A[c], db0[k] = w1[k] Sds, dw1[k] = W0[k].A + b0[k] Sds, db1 = Sds
    const int k = t >> 4, c = t & 15;
    dcanon[can::OUT0_W + t] += canon[can::OUT1_W + k] * dtail[tl::A + c];
    if (t < 16) {
        dcanon[can::LN_W + t] += dtail[tl::LNW + t];
        dcanon[can::LN_B + t] += dtail[tl::LNB + t];
        dcanon[can::OUT0_B + t] += canon[can::OUT1_W + t] * sds;
        float s = canon[can::OUT0_B + t] * sds;
        for (int cc = 0; cc < 16; ++cc) s += canon[can::OUT0_W + t * 16 + cc] * dtail[tl::A + cc];
        dcanon[can::OUT1_W + t] += s;
    }
    if (t == 0) dcanon[can::OUT1_B] += sds;
}

// Backward of gnr_sample_volume_fwd_train.  dvol [B,1,R,R,R]; gradients are ACCUMULATED into d_canonical
// (state-dict order, coarse level).  `stages` selects how far the backward runs (bit 4: tail, bit 3: geometry_fc +
// second reduction, ...): tests check the chain stage by stage through the training workspace.
extern "C" int gnr_sample_volume_bwd(const GnrScene* s, int R, const float* wc, const float* wb, const float* canonical_dev,
                                     const float* dvol, float* d_canonical, float* d_ray_feats, float* d_img_feats,
                                     void* ws, size_t ws_bytes, void* tws, size_t tws_bytes, int stages, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!wc || !wb || !canonical_dev || !dvol || !d_canonical || !ws || !tws) return fail(GNR_ERR_ARG, "gnr_sample_volume_bwd: null pointer");
    if (R < 2 || R > MAX_DN) return fail(GNR_ERR_SHAPE, "volume_res must be in 2..64");
    const TrainWs t = carve_train(s, R);
    if (tws_bytes < t.total) return fail(GNR_ERR_WORKSPACE, "training workspace too small");
    Workspace w = carve(s, (size_t)R * R * R, 0, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* tb = (char*)tws;
    auto sec = [tb](size_t off) { return (float*)(tb + off); };
    const int P = R * R * R, ntiles = s->B * ((P + 15) / 16);
    if (int rc = chain_partials_begin(s, sec(t.dpart), ntiles, stages, st)) return rc;
    if (stages & 16) {                                   // stage 5: tail
        RayBwdArgs a{wc, w.rec, dvol, sec(t.dg16), sec(t.dtail_part), s->B * R * R, R, 0, 0, 0};
        const int rpb = pack_rays(R * 76, R, 78 * 1024, &a.ray_stride);
        if (rpb < 1) return fail(GNR_ERR_SHAPE, "k_ray_bwd: a ray does not fit the LDS budget");
        a.rays_per_block = rpb;
        a.nblocks = (a.nrays + rpb - 1) / rpb;
        size_t lds_bytes = (size_t)rpb * a.ray_stride * sizeof(float);
        if (lds_bytes < 2 * 256 * 16 * sizeof(float)) lds_bytes = 2 * 256 * 16 * sizeof(float);
        int blocks = a.nblocks < 2 * num_cus() ? a.nblocks : 2 * num_cus();
        if (int rc = poison_partials(sec(t.dtail_part), (size_t)blocks * 4 * tp::STRIDE * sizeof(float), st, s->options)) return rc;
        if (int rc = launch<k_ray_bwd, 80 * 1024>("k_ray_bwd@gnr_sample_volume_bwd", st, dim3(blocks), dim3(256), lds_bytes, a)) return rc;
        if (int rc = launch_tail_reduce(sec(t.dtail_part), blocks * 4, wc, sec(t.dtail), st)) return rc;
        if (int rc = launch<k_tail_unfold>("k_tail_unfold@gnr_sample_volume_bwd", st, dim3(1), dim3(256), 0, (const float*)sec(t.dtail), canonical_dev, d_canonical)) return rc;
    }
    if (stages & 8) {                                    // stage 4: geometry_fc + second reduction
        GeoBwdArgs a{wc, wb, w.desc, sec(t.save2), sec(t.dg16), sec(t.dS2), sec(t.dpart), s->B, P, ntiles};
        if (int rc = with_views(s->V, [&](auto v) {
                return launch<k_geo_bwd<decltype(v)::value>, GEO_BWD_LDS>("k_geo_bwd@launch_geo_bwd", st, dim3(chain_blocks(ntiles)), dim3(256), GEO_BWD_LDS, a);
            })) return rc;
    }
    const BwdWs b{w.desc, sec(t.save1), sec(t.saveG), sec(t.dS2), sec(t.dG), sec(t.dS1), sec(t.dpart), tb + t.dfeat64, tb + t.scatter};
    return chain_bwd(s, w, BWD_VOLUME, b, wc, wb, P, stages, d_canonical, d_ray_feats, d_img_feats, st);
}

// ---- render path, hybrid training: per-view chain in HIP (both directions), per-ray tail in PyTorch ----------
struct RenderTrainWs { size_t desc, save1, save2, saveG, saveZ, dS2, dG, dS1, dfeat64, dpart, scatter, total; };
static RenderTrainWs carve_render_train(const GnrScene* s, int rn, int dn) {
    RenderTrainWs t;
    const size_t P = (size_t)rn * dn, T = (size_t)s->B * ((P + 15) / 16), V = s->V;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off += al256(floats * sizeof(float)); return o; };
    t.desc = take((size_t)s->B * P * DESC_FLOATS);
    t.save1 = take(T * V * 19 * 64);
    t.save2 = take(T * V * 11 * 64);
    t.saveG = take(T * 17 * 64);
    t.saveZ = take(T * 18 * 64);
    t.dS2 = take(T * V * 10 * 64);
    t.dG = take(T * 16 * 64);
    t.dS1 = take(T * V * DS1 * 64);
    t.dfeat64 = take(feat_grad_bytes(s) / sizeof(float));
    t.dpart = take(chain_part_floats());                   // partial parameter gradients of the pass's chain backward
    t.scatter = take(carve_scatter(s, T).total / sizeof(float));   // binned scatter of the feature-map gradient (gnr_bwd_scatter.inc)
    t.total = off;
    return t;
}

extern "C" size_t gnr_render_chain_train_workspace_bytes(const GnrScene* s, int rn, int dn) {
    if (!s || rn < 1 || dn < 3 || dn > MAX_DN_FWD) return 0;
    return carve_render_train(s, rn, dn).total;
}

// One render pass up to the cross-view statistics, saving what the backward needs.
//   stats_out [B, rn*dn, 66]: mean(32) var(32) wbar, number of valid views;  colors_out [B, rn*dn, 3]
//   depth == NULL: the coarse pass -- sample_depth (render_ops.py:146-170) on the device, dn = rays->dn
//   depth_out [B,rn,dn], pts_out [B,rn*dn,3], qdir_out [B,rn,3] (each nullable): the sample depths the pass used and its ray
//   geometry (render_ops.py:4-39) as plain tensors, for the pass's tail / compositing backward
extern "C" int gnr_render_chain_fwd_train(const GnrScene* s, const GnrRays* q, const float* depth, int dn, const float* wl,
                                          float* stats_out, float* colors_out, float* depth_out, float* pts_out, float* qdir_out,
                                          void* ws, size_t ws_bytes, void* tws, size_t tws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (int rc = check_rays(q)) return rc;
    if (!wl || !stats_out || !colors_out || !ws || !tws) return fail(GNR_ERR_ARG, "gnr_render_chain_fwd_train: null pointer");
    if (!depth && dn != q->dn) return fail(GNR_ERR_SHAPE, "gnr_render_chain_fwd_train: the coarse pass (depth == NULL) samples rays->dn depths");
    // a pass on caller-given depths may carry the coarse and the resampled depths of a ray together (fine_depth_use_all,
    // renderer.py:145-146): up to 128 samples, like the forward entry points; the coarse pass and its resampler stay at 64
    if (dn < 3 || dn > (depth ? MAX_DN_FWD : MAX_DN)) return fail(GNR_ERR_SHAPE, "dn must be in 3..64 (3..128 with caller-given depths)");
    const RenderTrainWs t = carve_render_train(s, q->rn, dn);
    if (tws_bytes < t.total) return fail(GNR_ERR_WORKSPACE, "training workspace too small");
    if (int rc = check_points(s, (size_t)q->rn * dn)) return rc;
    Workspace w = carve(s, (size_t)q->rn * dn, q->rn, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* tb = (char*)tws;
    const int B = s->B, P = q->rn * dn, ntiles = B * ((P + 15) / 16);
    float* desc = (float*)(tb + t.desc);
    const int range_slot = depth ? RS_DEPTHS_TRAIN : RS_COARSE_TRAIN;      // watch word of this training pass
    const dim3 pgrid((B * P + 255) / 256);
    if (!depth) {
        if (int rc = launch<k_coarse_depth>("k_coarse_depth@gnr_render_chain_fwd_train", st, pgrid, dim3(256), 0, q->que_depth_range, w.depth_c, q->rn, dn, B)) return rc;
        depth = w.depth_c;
    }
    if (depth_out && depth_out != depth)
        GNR_HIP(hipMemcpyAsync(depth_out, depth, (size_t)B * P * sizeof(float), hipMemcpyDeviceToDevice, st));
    // (no ray order, no generated depths, no sample keys: the training pass keeps the caller's order)
    if (int rc = launch<k_points_rays>("k_points_rays@gnr_render_chain_fwd_train", st, pgrid, dim3(256), 0, q->coords, q->que_pose, q->que_K, q->que_depth_range,
                                       depth, desc, q->rn, dn, B, (const int*)nullptr, (float*)nullptr, (unsigned char*)nullptr, (const float*)nullptr, 0, 0, 0)) return rc;
    if (pts_out || qdir_out)
        if (int rc = launch<k_desc_unpack>("k_desc_unpack@gnr_render_chain_fwd_train", st, pgrid, dim3(256), 0, (const float*)desc, pts_out, qdir_out, dn, B * P)) return rc;
    ChainArgs a{wl, w.feat64, s->imgs, w.viewp, desc, w.rec, colors_out, nullptr, nullptr, B, P, s->H, s->W, s->fh, s->fw, 0,
                (float*)(tb + t.save1), (float*)(tb + t.save2), (float*)(tb + t.saveG), (float*)(tb + t.saveZ)};
    wire_chain(a, s, w, range_slot);
    if (int rc = launch_chain<true, true>(s, a, st)) return rc;
    return launch<k_stats_unpack>("k_stats_unpack@gnr_render_chain_fwd_train", st, dim3((ntiles + 3) / 4), dim3(256), 0, (const float*)(tb + t.saveZ), stats_out, P, ntiles);
}

// Backward of gnr_render_chain_fwd_train: d stats [B,P,65] (mean, var, wbar), d colours [B,P,3] -> gradients of the
// level's parameters (ACCUMULATED, state-dict order) and of the feature maps (overwritten; may be null).
extern "C" int gnr_render_chain_bwd(const GnrScene* s, int rn, int dn, const float* wl, const float* wb, const float* dstats,
                                    const float* dcolors, float* d_canonical, float* d_ray_feats, float* d_img_feats,
                                    void* ws, size_t ws_bytes, void* tws, size_t tws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!wl || !wb || !dstats || !dcolors || !d_canonical || !ws || !tws) return fail(GNR_ERR_ARG, "gnr_render_chain_bwd: null pointer");
    const RenderTrainWs t = carve_render_train(s, rn, dn);
    if (tws_bytes < t.total) return fail(GNR_ERR_WORKSPACE, "training workspace too small");
    Workspace w = carve(s, 0, 0, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* tb = (char*)tws;
    auto sec = [tb](size_t off) { return (float*)(tb + off); };
    const int P = rn * dn, ntiles = s->B * ((P + 15) / 16);
    if (int rc = chain_partials_begin(s, sec(t.dpart), ntiles, 15, st)) return rc;
    Red2BwdArgs a{sec(t.save2), dstats, dcolors, sec(t.dS2), P, ntiles};
    if (int rc = with_views(s->V, [&](auto v) {
            return launch<k_red2_bwd<decltype(v)::value>>("k_red2_bwd@launch_red2_bwd", st, dim3((ntiles + 3) / 4), dim3(256), 0, a);
        })) return rc;
    const BwdWs b{sec(t.desc), sec(t.save1), sec(t.saveG), sec(t.dS2), sec(t.dG), sec(t.dS1), sec(t.dpart), tb + t.dfeat64, tb + t.scatter};
    return chain_bwd(s, w, BWD_RENDER, b, wl, wb, P, 15, d_canonical, d_ray_feats, d_img_feats, st);
}

// ---- test tooling of the binned scatter (include/gnr.h) -----------------------------------------------------
// byte offsets of {rows, wts, key, cnt, cursor, list, nseg} of the binned scatter inside a training workspace + the number of rows:
// dn == 0: the volume's (gnr_sample_volume_train_workspace_bytes(scene, n)), else a render pass's (rn = n rays x dn samples)
extern "C" int gnr_scatter_workspace_layout(const GnrScene* s, int n, int dn, size_t* out8) {
    if (int rc = check_scene(s)) return rc;
    if (!out8) return fail(GNR_ERR_ARG, "gnr_scatter_workspace_layout: null pointer");
    size_t base, T;
    if (dn == 0) {
        if (n < 2 || n > MAX_DN) return fail(GNR_ERR_SHAPE, "volume_res must be in 2..64");
        base = carve_train(s, n).scatter;
        T = (size_t)s->B * (((size_t)n * n * n + 15) / 16);
    } else {
        if (n < 1 || dn < 3 || dn > MAX_DN_FWD) return fail(GNR_ERR_SHAPE, "gnr_scatter_workspace_layout: rn >= 1, dn in 3..128");
        base = carve_render_train(s, n, dn).scatter;
        T = (size_t)s->B * (((size_t)n * dn + 15) / 16);
    }
    const ScatterWs c = carve_scatter(s, T);
    const size_t v[8] = {base + c.rows, base + c.wts, base + c.key, base + c.cnt, base + c.cursor, base + c.list, base + c.nseg, T * s->V * 16};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return GNR_OK;
}

// the stage alone on caller-given rows: its scratch = the sanitised keys, cnt, cursor, list, nseg
struct DebugScatterWs { size_t key, cnt, cursor, list, nseg, total; };
static bool debug_scatter_shape_ok(int B, int V, int fh, int fw, int tps) {
    if (B < 1 || V < 1 || fh < 1 || fw < 1 || tps < 1) return false;
    const unsigned long long bins = (unsigned long long)B * V * fh * fw, rows = (unsigned long long)B * tps * V * 16;
    return bins < (1ull << 26) && rows < (1ull << 26) && (unsigned long long)fh * fw < (1ull << 24);      // (keys, row ids and 64 x either as ints / size_t)
}
static DebugScatterWs carve_debug_scatter(int B, int V, int fh, int fw, int tps) {
    DebugScatterWs c;
    const size_t N = (size_t)B * tps * V * 16, bins = (size_t)B * V * fh * fw;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    c.key = take(N * sizeof(int));
    c.cnt = take(bins * sizeof(int));
    c.cursor = take(bins * sizeof(int));
    c.list = take(N * sizeof(int));
    c.nseg = take((size_t)B * V * sizeof(int));
    c.total = off;
    return c;
}
extern "C" size_t gnr_debug_feature_scatter_bytes(int B, int V, int fh, int fw, int tiles_per_scene, size_t* raw_bytes) {
    if (!debug_scatter_shape_ok(B, V, fh, fw, tiles_per_scene)) return 0;
    if (raw_bytes) *raw_bytes = al256((size_t)B * V * fh * fw * 64 * 8) + 256;
    return carve_debug_scatter(B, V, fh, fw, tiles_per_scene).total;
}
static const BwdEntry BWD_DEBUG_SCATTER = {
    false, 0, -1, {}, nullptr, nullptr, nullptr, nullptr,
    "k_scatter_place@gnr_debug_feature_scatter", "k_scatter_scan@gnr_debug_feature_scatter", "k_scatter_fill@gnr_debug_feature_scatter",
    "k_scatter_gather@gnr_debug_feature_scatter", "k_unpack_feat_grad@gnr_debug_feature_scatter", nullptr};
extern "C" int gnr_debug_feature_scatter(int B, int V, int fh, int fw, int tiles_per_scene, const float* rows, const float* wts, const int* key,
                                         unsigned upmax_bits, int fixed, int path, float* d_ray_feats, float* d_img_feats, void* raw,
                                         size_t raw_bytes, void* scratch, size_t scratch_bytes, unsigned* status_out2, void* stream) {
    if (!rows || !wts || !key || !raw || !scratch || !status_out2) return fail(GNR_ERR_ARG, "gnr_debug_feature_scatter: null pointer");
    if (!debug_scatter_shape_ok(B, V, fh, fw, tiles_per_scene)) return fail(GNR_ERR_SHAPE, "gnr_debug_feature_scatter: B, V, fh, fw, tiles >= 1; B*V*fh*fw and the rows below 2^26");
    if (path != SCATTER_PATH_AUTO && path != SCATTER_PATH_PLACE && path != SCATTER_PATH_SCAN_FILL) return fail(GNR_ERR_ARG, "gnr_debug_feature_scatter: path is 0 (by size), 1 (LDS placement) or 2 (scan + fill)");
    const size_t npix = (size_t)fh * fw;
    if (path == SCATTER_PATH_PLACE && npix * sizeof(int) > PLACE_LDS) return fail(GNR_ERR_SHAPE, "gnr_debug_feature_scatter: the LDS placement holds at most 38400 pixels");
    const DebugScatterWs c = carve_debug_scatter(B, V, fh, fw, tiles_per_scene);
    const size_t need_raw = al256((size_t)B * V * npix * 64 * 8) + 256;
    if (scratch_bytes < c.total || raw_bytes < need_raw) return fail(GNR_ERR_WORKSPACE, "gnr_debug_feature_scatter: scratch or raw buffer too small");
    hipStream_t st = (hipStream_t)stream;
    GnrScene s;
    memset(&s, 0, sizeof(s));
    s.B = B; s.V = V; s.fh = fh; s.fw = fw;
    char* sb = (char*)scratch;
    unsigned* status = status_out2;                               // device: [0] bit 3 (a clamped contribution), [1] keys neutralised
    unsigned* upmax = (unsigned*)((char*)raw + al256((size_t)B * V * npix * 64 * 8));
    const int ntiles = B * tiles_per_scene, N = ntiles * V * 16;
    ScatterBins sc{const_cast<float*>(rows), reinterpret_cast<f4*>(const_cast<float*>(wts)), (int*)(sb + c.key), (int*)(sb + c.cnt),
                   (int*)(sb + c.cursor), (int*)(sb + c.list), (int*)(sb + c.nseg), fixed ? upmax : nullptr};
    GNR_HIP(hipMemsetAsync(sc.cnt, 0, (size_t)B * V * npix * sizeof(int), st));
    GNR_HIP(hipMemsetAsync(status, 0, 2 * sizeof(unsigned), st));
    GNR_HIP(hipMemsetAsync(raw, 0, fixed ? need_raw : (size_t)B * V * npix * 64 * sizeof(float), st));      // (as feat_grad_begin clears it)
    if (int rc = launch<k_scatter_debug_keys>("k_scatter_debug_keys@gnr_debug_feature_scatter", st, dim3((N + 255) / 256), dim3(256), 0, key, sc.key, sc.cnt,
                                              status + 1, fixed ? upmax : (unsigned*)nullptr, upmax_bits, N, V, tiles_per_scene, (int)npix)) return rc;
    const FeatGradBuf fg{(float*)raw, FeatFx{upmax, status}, fixed != 0};
    const BwdGuard always{nullptr, nullptr, nullptr, 0, nullptr, 0};
    if (int rc = launch_scatter_bins(&s, sc, fg.buf, ntiles, BWD_DEBUG_SCATTER, fg.fixed, fg.fx, always, st, path)) return rc;
    if (d_ray_feats || d_img_feats)
        if (int rc = feat_grad_unpack(&s, fg, d_ray_feats, d_img_feats, BWD_DEBUG_SCATTER.unpack, st)) return rc;
    return GNR_OK;
}

// Forward of the per-ray tail + NeuS alpha + compositing of a training render pass: k_ray<true> on the records the chain of
// gnr_render_chain_fwd_train left in `ws` (call it right after that chain, before anything else uses `ws`).
// out->colors_nr is the INPUT (the chain's colours); every other non-null member of `out` is written as in
// gnr_render_by_depth_fwd (sdf_values, sdf_gradient, alpha_values, hit_prob_nr, pixel_colors_nr, render_depth, ray_mask,
// sdf_gradient_error [B,n_chunks], pixel_colors_gt).
// fine_depth_out [B,rn,rays->fdn] (nullable): the inverse-CDF resampling of this (coarse) pass, sorted (render_ops.py:172-229,
// renderer.py:146-148) -- with rays->fine_u the is_train draws, else the eval midpoints.
extern "C" int gnr_render_tail_fwd_train(const GnrScene* s, const GnrRays* q, const float* depth, int dn, const float* wl,
                                         GnrRenderOut* out, float* fine_depth_out, void* ws, size_t ws_bytes, void* tws,
                                         size_t tws_bytes, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (int rc = check_rays(q)) return rc;
    if (!depth || !wl || !out || !out->colors_nr || !ws || !tws) return fail(GNR_ERR_ARG, "gnr_render_tail_fwd_train: null pointer");
    if (dn < 3 || dn > MAX_DN_FWD) return fail(GNR_ERR_SHAPE, "dn must be in 3..128");
    if (fine_depth_out && dn > MAX_DN) return fail(GNR_ERR_SHAPE, "the inverse-CDF resampler (fine_depth_out) takes at most 64 samples per ray");
    const RenderTrainWs t = carve_render_train(s, q->rn, dn);
    if (tws_bytes < t.total) return fail(GNR_ERR_WORKSPACE, "training workspace too small");
    Workspace w = carve(s, (size_t)q->rn * dn, q->rn, ws);
    if (ws_bytes < w.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    RayArgs r = render_ray_args(s, q, depth, dn, wl, out, w, (const float*)((char*)tws + t.desc));
    if (fine_depth_out) { r.fine_depth = fine_depth_out; r.fdn = q->fdn; r.fine_u = q->fine_u; }
    if (int rc = launch_ray<true>(r, st)) return rc;
    return render_ray_epilogue(s, q, out, dn, w, "k_gerr_reduce@gnr_render_tail_fwd_train", "k_pixel_gt@gnr_render_tail_fwd_train", true, nullptr, st);
}

// Backward of NeuS alpha + compositing for a flat list of rays (k_composite_bwd): see csrc/gnr_bwd.inc.
//   a_out [nrays*dn], gamma_out [nrays*dn,3], dcol_out [nrays*dn,3] are overwritten; dvar_out[0] is overwritten.
//   scratch: gnr_composite_bwd_workspace_bytes(nrays) bytes (per-wavefront partials of dvar, added in a fixed order)
extern "C" size_t gnr_composite_bwd_workspace_bytes(int nrays) { return nrays > 0 ? al256((size_t)((nrays + 63) / 64) * sizeof(double)) : 0; }

extern "C" int gnr_composite_bwd(const float* wl, const float* sdf, const float* grad, const float* col, const float* depth,
                                 const float* qdir, const float* dpix, const float* ddepth, const float* wgerr,
                                 const float* dalpha, const float* dhit, float* a_out, float* gamma_out, float* dcol_out,
                                 float* dvar_out, int nrays, int dn, void* scratch, size_t scratch_bytes, void* stream) {
    if (!wl || !sdf || !grad || !col || !depth || !qdir || !dpix || !a_out || !gamma_out || !dcol_out || !dvar_out || !scratch)
        return fail(GNR_ERR_ARG, "gnr_composite_bwd: null pointer");
    if (nrays < 1) return fail(GNR_ERR_SHAPE, "nrays must be >= 1");
    if (dn < 3 || dn > MAX_DN_FWD) return fail(GNR_ERR_SHAPE, "dn must be in 3..128");
    if (scratch_bytes < gnr_composite_bwd_workspace_bytes(nrays)) return fail(GNR_ERR_WORKSPACE, "gnr_composite_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (nrays + 63) / 64;
    CompBwdArgs c{wl, sdf, grad, col, depth, qdir, dpix, ddepth, wgerr, dalpha, dhit, a_out, gamma_out, dcol_out, (double*)scratch, nrays, dn};
    if (int rc = launch<k_composite_bwd>("k_composite_bwd@gnr_composite_bwd", st, dim3(blocks), dim3(64), 0, c)) return rc;
    return launch<k_dvar_finish>("k_dvar_finish@gnr_composite_bwd", st, dim3(1), dim3(256), 0, (const double*)scratch, blocks, dvar_out);
}

extern "C" int gnr_ray_tail_grad_floats(void) { return tl::TOTAL; }

// Backward of the per-ray tail with the second-order path (k_ray_dual_bwd, csrc/gnr_bwd.inc): rays are a flat list.
//   g, gd [nrays*dn,16], a, nvalid [nrays*dn] -> gbar, gdbar [nrays*dn,16]; dtail [gnr_ray_tail_grad_floats()] is
//   overwritten: dWq, dWk, dWv, dWfc [16][16], dLNw, dLNb [16], d w_eff [16], d b_eff of the folded out_geometry_fc.
//   scratch: gnr_ray_tail_dual_bwd_workspace_bytes() bytes (per-wavefront partial gradients, summed in a fixed order)
extern "C" size_t gnr_ray_tail_dual_bwd_workspace_bytes(void) { return al256(tail_part_floats(4) * sizeof(float)); }

extern "C" int gnr_ray_tail_dual_bwd(const float* wl, const float* g, const float* gd, const float* a, const float* nvalid,
                                     float* gbar, float* gdbar, float* dtail, int nrays, int dn, void* scratch, size_t scratch_bytes,
                                     unsigned options, void* stream) {
    if (!wl || !g || !gd || !a || !nvalid || !gbar || !gdbar || !dtail || !scratch) return fail(GNR_ERR_ARG, "gnr_ray_tail_dual_bwd: null pointer");
    if (options & ~GNR_OPT_ALL) return fail(GNR_ERR_ARG, "gnr_ray_tail_dual_bwd: unknown option bits");
    if (nrays < 1) return fail(GNR_ERR_SHAPE, "nrays must be >= 1");
    if (dn < 3 || dn > MAX_DN_FWD) return fail(GNR_ERR_SHAPE, "dn must be in 3..128");
    if (scratch_bytes < gnr_ray_tail_dual_bwd_workspace_bytes()) return fail(GNR_ERR_WORKSPACE, "gnr_ray_tail_dual_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    RayDualArgs r{wl, g, gd, a, nvalid, gbar, gdbar, (float*)scratch, nrays, dn, 0, 0, 0};
    constexpr size_t MAX_LDS = 160 * 1024;                   // one workgroup per CU
    const int rpb = pack_rays(dn * dl::PER, dn, (int)MAX_LDS, &r.ray_stride);
    if (rpb < 1) return fail(GNR_ERR_SHAPE, "k_ray_dual_bwd: a ray does not fit the LDS budget");
    r.rays_per_block = rpb;
    r.nblocks = (nrays + rpb - 1) / rpb;
    size_t lds_bytes = (size_t)rpb * r.ray_stride * sizeof(float);
    if (lds_bytes < 2 * 256 * 16 * sizeof(float)) lds_bytes = 2 * 256 * 16 * sizeof(float);
    const int blocks = r.nblocks < num_cus() ? r.nblocks : num_cus();
    if (int rc = poison_partials(scratch, (size_t)blocks * 4 * tp::STRIDE * sizeof(float), st, options)) return rc;
    if (int rc = launch<k_ray_dual_bwd, MAX_LDS>("k_ray_dual_bwd@gnr_ray_tail_dual_bwd", st, dim3(blocks), dim3(256), lds_bytes, r)) return rc;
    return launch_tail_reduce((const float*)scratch, blocks * 4, wl, dtail, st);
}

// geometry_fc on dual numbers around gnr_ray_tail_dual_bwd (k_geo_dual_fwd[_mm] / k_geo_dual_bwd, csrc/gnr_bwd.inc, gnr_bwd_geo_dual_mm.inc).
//   canon: the level's canonical blob on the device; stats [P,66], pts, gamma [P,3] -> g, gd [P,16]
//   scratch: gnr_geo_dual_fwd_workspace_bytes() bytes = the call's fp16-pair fragment image (k_pack_geo_dual) + its range word.
//   GNR_OPT_GEO_DUAL_FP32: the fp32 FMA kernel, one lane per point (what also recomputes a call whose matrix-core outputs came out non-finite)
extern "C" size_t gnr_geo_dual_fwd_workspace_bytes(void) { return al256(gdf::TOTAL * sizeof(float)) + 256; }
extern "C" int gnr_geo_dual_fwd(const float* canon, const float* stats, const float* pts, const float* gamma, float* g, float* gd,
                                int P, void* scratch, size_t scratch_bytes, unsigned options, void* stream) {
    if (!canon || !stats || !pts || !gamma || !g || !gd) return fail(GNR_ERR_ARG, "gnr_geo_dual_fwd: null pointer");
    if (options & ~GNR_OPT_ALL) return fail(GNR_ERR_ARG, "gnr_geo_dual_fwd: unknown option bits");
    if (P < 1) return fail(GNR_ERR_SHAPE, "P must be >= 1");
    hipStream_t st = (hipStream_t)stream;
    GeoDualArgs a{canon, stats, pts, gamma, nullptr, nullptr, g, gd, nullptr, nullptr, P, 0, nullptr};
    if (options & GNR_OPT_GEO_DUAL_FP32)
        return launch<k_geo_dual_fwd>("k_geo_dual_fwd@gnr_geo_dual_fwd", st, dim3((P + 255) / 256), dim3(256), 0, a, (const unsigned*)nullptr);
    if (!scratch) return fail(GNR_ERR_ARG, "gnr_geo_dual_fwd: null scratch");
    if (scratch_bytes < gnr_geo_dual_fwd_workspace_bytes()) return fail(GNR_ERR_WORKSPACE, "gnr_geo_dual_fwd: scratch too small");
    float* frags = (float*)scratch;
    unsigned* range_word = (unsigned*)((char*)scratch + al256(gdf::TOTAL * sizeof(float)));
    if (int rc = launch<k_pack_geo_dual>("k_pack_geo_dual@gnr_geo_dual_fwd", st, dim3(16), dim3(256), 0, canon, frags)) return rc;
    GNR_HIP(hipMemsetAsync(range_word, 0, sizeof(unsigned), st));
    const int ngroups = (P + 15) / 16;
    int blocks = (ngroups + 3) / 4;
    if (blocks > 4 * num_cus()) blocks = 4 * num_cus();
    if (int rc = launch<k_geo_dual_fwd_mm>("k_geo_dual_fwd@gnr_geo_dual_fwd", st, dim3(blocks), dim3(256), gdf::W2T * sizeof(float), a, (const float*)frags, ngroups, range_word)) return rc;
    // the fp32 twin: returns at once unless the matrix-core kernel flagged its outputs (a weight or an operand beyond the fp16 range)
    return launch<k_geo_dual_fwd>("k_geo_dual_fwd.fp32_twin", st, dim3((P + 255) / 256), dim3(256), 0, a, (const unsigned*)range_word);
}

//   gbar, gdbar [P,16] -> dstats [P,66] (overwritten, column 65 = 0); gradients of geometry_fc.{0,2} ACCUMULATED into
//   d_canonical (state-dict order).  scratch: gnr_geo_dual_bwd_workspace_bytes(P) bytes (the per-point adjoints between the two kernels)
static size_t geo_dual_part_bytes() { return al256((size_t)2 * num_cus() * gd2::NW * GD_STRIDE * sizeof(float)); }
// scratch: [partial gradients] [per-point adjoints P x 288] [the call's fp16-pair fragment image, 64 KB (k_pack_geo_dual)]
extern "C" size_t gnr_geo_dual_bwd_workspace_bytes(int P) {
    return P > 0 ? al256((size_t)P * gd2::YCOLS * sizeof(float)) + geo_dual_part_bytes() + al256(gdf::TOTAL * sizeof(float)) + 256 : 0;
}
// GNR_OPT_GEO_DUAL_FP32: the per-point half as fp32 FMAs, one lane per point (k_geo_dual_bwd_pts) instead of the fp16-pair chain
// (k_geo_dual_bwd_pts_mm); same outputs to rounding.
extern "C" int gnr_geo_dual_bwd(const float* canon, const float* stats, const float* pts, const float* gamma, const float* gbar,
                                const float* gdbar, float* dstats, float* d_canonical, int P, void* scratch, size_t scratch_bytes,
                                unsigned options, void* stream) {
    if (!canon || !stats || !pts || !gamma || !gbar || !gdbar || !dstats || !d_canonical || !scratch) return fail(GNR_ERR_ARG, "gnr_geo_dual_bwd: null pointer");
    if (options & ~GNR_OPT_ALL) return fail(GNR_ERR_ARG, "gnr_geo_dual_bwd: unknown option bits");
    if (P < 1) return fail(GNR_ERR_SHAPE, "P must be >= 1");
    if (scratch_bytes < gnr_geo_dual_bwd_workspace_bytes(P)) return fail(GNR_ERR_WORKSPACE, "gnr_geo_dual_bwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    float* dpart = (float*)scratch;                          // partial geometry_fc gradients first, the per-point adjoints behind them
    GeoDualArgs a{canon, stats, pts, gamma, gbar, gdbar, nullptr, nullptr, dstats, dpart, P, (P + gd2::NT - 1) / gd2::NT,
                  (float*)((char*)scratch + geo_dual_part_bytes())};
    const dim3 pgrid((P + 255) / 256);                       // k_geo_dual_bwd_pts: one lane per point
    if (!(options & GNR_OPT_GEO_DUAL_FP32)) {
        constexpr size_t PTS_LDS = gdf::TOTAL * sizeof(float);
        float* frags = (float*)((char*)scratch + geo_dual_part_bytes() + al256((size_t)P * gd2::YCOLS * sizeof(float)));
        if (int rc = launch<k_pack_geo_dual>("k_pack_geo_dual@gnr_geo_dual_bwd", st, dim3(16), dim3(256), 0, canon, frags)) return rc;
        const int ngroups = (P + 15) / 16;
        int pblocks = (ngroups + 3) / 4;
        if (pblocks > 2 * num_cus()) pblocks = 2 * num_cus();
        unsigned* range_word = (unsigned*)((char*)frags + al256(gdf::TOTAL * sizeof(float)));
        GNR_HIP(hipMemsetAsync(range_word, 0, sizeof(unsigned), st));
        if (int rc = launch<k_geo_dual_bwd_pts_mm, PTS_LDS>("k_geo_dual_bwd_pts@gnr_geo_dual_bwd", st, dim3(pblocks), dim3(256), PTS_LDS, a, (const float*)frags, ngroups, range_word)) return rc;
        // the fp32 twin: returns at once unless the matrix-core kernel flagged its outputs (a weight beyond the fp16 range)
        if (int rc = launch<k_geo_dual_bwd_pts>("k_geo_dual_bwd_pts.fp32_twin", st, pgrid, dim3(256), 0, a, (const unsigned*)range_word)) return rc;
    } else {
        if (int rc = launch<k_geo_dual_bwd_pts>("k_geo_dual_bwd_pts@gnr_geo_dual_bwd", st, pgrid, dim3(256), 0, a, (const unsigned*)nullptr)) return rc;
    }
    const int blocks = a.nblocks < 2 * num_cus() ? a.nblocks : 2 * num_cus();
    const int slots = blocks * gd2::NW;
    if (int rc = poison_partials(dpart, (size_t)slots * GD_STRIDE * sizeof(float), st, options)) return rc;
    constexpr size_t GEMM_LDS = gd2::TOTAL * sizeof(float);
    if (int rc = launch<k_geo_dual_bwd_gemm, GEMM_LDS>("k_geo_dual_bwd_gemm@gnr_geo_dual_bwd", st, dim3(blocks), dim3(64 * gd2::NW), GEMM_LDS, a)) return rc;
    const GradRange rg[1] = {{0, can::WQ - can::GEO0_W, can::GEO0_W}};
    return launch_grad_reduce(dpart, slots, GD_STRIDE, d_canonical, rg, 1, st, "k_grad_reduce@gnr_geo_dual_bwd");
}

// fail() of every translation unit (gnr_host.h) ends here: not part of the public ABI
extern "C" int gnr_internal_fail(int code, const char* what, int hip_error) {
    const hipError_t e = (hipError_t)hip_error;
    snprintf(g_err, sizeof(g_err), "%s%s%s", what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString(e) : "");
    return code;
}

// TimingScope of every translation unit (gnr_host.h): claims a slot and records the opening event; -1 when the label is not bracketed
extern "C" int gnr_internal_timing_open(const char* label, void* stream) {
    if (!label || !g_kt.on.load() || (g_kt.only[0] && !strstr(label, g_kt.only))) return -1;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return -1;
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return -1; }
    const int i = g_kt.n.fetch_add(1);
    if (i >= KTiming::MAX) { g_kt.n.fetch_sub(1); hipEventDestroy(e0); hipEventDestroy(e1); return -1; }
    g_kt.rec[i] = KTiming::Rec{label, e0, e1};
    hipEventRecord(e0, (hipStream_t)stream);
    return i;
}
extern "C" void gnr_internal_timing_close(int idx, void* stream) {
    if (idx >= 0 && idx < g_kt.n.load()) hipEventRecord(g_kt.rec[idx].e1, (hipStream_t)stream);
}

extern "C" int gnr_timing_begin_only(const char* label_substring) {
    g_kt.on = false;
    for (int i = 0, n = g_kt.n.exchange(0); i < n; ++i) { hipEventDestroy(g_kt.rec[i].e0); hipEventDestroy(g_kt.rec[i].e1); }
    snprintf(g_kt.only, sizeof(g_kt.only), "%s", label_substring ? label_substring : "");
    g_kt.on = true;
    return GNR_OK;
}
extern "C" int gnr_timing_begin(void) { return gnr_timing_begin_only(nullptr); }

// Stops the recording, waits for the recorded events and writes one line per label, "label count total_ms\n", into report
// (truncated to report_bytes, always NUL-terminated).  Returns the number of launches recorded.
extern "C" int gnr_timing_end(char* report, size_t report_bytes) {
    g_kt.on = false;
    struct Agg { const char* label; int n; double ms; } agg[256];
    int na = 0;
    const int total = g_kt.n.exchange(0);
    hipError_t bad = hipSuccess;
    for (int i = 0; i < total; ++i) {                       // every event pair is destroyed, whatever happens to its reading
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(g_kt.rec[i].e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_kt.rec[i].e0, g_kt.rec[i].e1);
        hipEventDestroy(g_kt.rec[i].e0);
        hipEventDestroy(g_kt.rec[i].e1);
        if (e != hipSuccess) { bad = e; continue; }
        int k = 0;
        while (k < na && strcmp(agg[k].label, g_kt.rec[i].label) != 0) ++k;
        if (k == na) { if (na == 256) continue; agg[na++] = Agg{g_kt.rec[i].label, 0, 0.0}; }
        agg[k].n += 1; agg[k].ms += ms;
    }
    if (bad != hipSuccess) return fail(GNR_ERR_HIP, "gnr_timing_end: reading an event pair", bad);
    if (report && report_bytes) {
        size_t off = 0;
        report[0] = 0;
        for (int k = 0; k < na; ++k) {
            const int w = snprintf(report + off, report_bytes - off, "%s %d %.6f\n", agg[k].label, agg[k].n, agg[k].ms);
            if (w < 0 || (size_t)w >= report_bytes - off) { report[off] = 0; break; }
            off += (size_t)w;
        }
    }
    return total;
}

// Test tooling: LDS is not cleared between kernels, so a kernel that reads LDS it did not write computes on what the previous
// kernel left there.  gnr_debug_fill_lds floods the LDS of every CU with a 32-bit pattern (workgroups of 160 KB, four per CU's worth
// of launches so that every CU takes some); a test runs the path after two different patterns and asks for the same bits
// (tests/test_range_guard.py: lanes that shadow a ray beyond the launch must not influence anything).
namespace gnr {
__global__ __launch_bounds__(256) void k_fill_lds(unsigned pattern, int words, unsigned* sink) {
    extern __shared__ unsigned fill_sm[];
    for (int e = threadIdx.x; e < words; e += 256) fill_sm[e] = pattern;
    __syncthreads();
    if (sink && fill_sm[(threadIdx.x * 977) % words] != pattern) *sink = 1u;       // (keeps the stores alive)
}
}  // namespace gnr
extern "C" int gnr_debug_fill_lds(unsigned pattern, void* stream) {
    constexpr int BYTES = 160 * 1024 - 256;
    return launch<k_fill_lds, BYTES>(nullptr, (hipStream_t)stream, dim3(1024), dim3(256), BYTES, pattern, BYTES / 4, (unsigned*)nullptr);   // (no timing label)
}

// the two calls bench.py round 1 used: average duration of the volume k_chain launches
extern "C" int gnr_chain_timing_begin(void) { return gnr_timing_begin_only("k_chain.volume"); }
extern "C" int gnr_chain_timing_end(float* avg_ms_out, int* count_out) {
    char buf[16384];
    const int rc = gnr_timing_end(buf, sizeof(buf));
    if (rc < 0) return rc;
    int n = 0; double ms = 0.0;
    for (const char* p = buf; *p;) {
        char label[128]; int c = 0; double t = 0.0;
        if (sscanf(p, "%127s %d %lf", label, &c, &t) == 3 && strcmp(label, "k_chain.volume") == 0) { n += c; ms += t; }
        const char* nl = strchr(p, '\n');
        if (!nl) break;
        p = nl + 1;
    }
    if (avg_ms_out) *avg_ms_out = n ? (float)(ms / n) : 0.f;
    if (count_out) *count_out = n;
    return GNR_OK;
}

extern "C" int gnr_time_chain_kernel(const GnrScene* s, int R, const float* wc, void* ws, size_t ws_bytes, int iters,
                                     float* ms_out, void* stream) {
    if (int rc = check_scene(s)) return rc;
    if (!wc || !ws || !ms_out || iters < 1) return fail(GNR_ERR_ARG, "gnr_time_chain_kernel: bad argument");
    hipStream_t st = (hipStream_t)stream;
    // descriptors for a centred default workspace box
    float* bbox_dev = nullptr;
    GNR_HIP(hipMalloc(&bbox_dev, sizeof(float) * 3 * s->B));
    {
        float* h = (float*)malloc(sizeof(float) * 3 * s->B);
        for (int b = 0; b < s->B; ++b) { h[3 * b] = -0.15f; h[3 * b + 1] = -0.15f; h[3 * b + 2] = -0.05f; }
        hipMemcpy(bbox_dev, h, sizeof(float) * 3 * s->B, hipMemcpyHostToDevice);
        free(h);
    }
    int rc = volume_impl(s, bbox_dev, R, wc, nullptr, nullptr, ws, ws_bytes, st, true, true, false);   // warm-up
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    if (!rc) {
        hipEventRecord(e0, st);
        for (int i = 0; i < iters && !rc; ++i)
            rc = volume_impl(s, bbox_dev, R, wc, nullptr, nullptr, ws, ws_bytes, st, false, true, false);
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        *ms_out = ms / (float)iters;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(bbox_dev);
    return rc;
}

#if GNR_WAVE_CLOCK
// measurement build only (tools/wave_clock.py): the stamps the last k_chain launches left (which: 0 volume, 1 render)
extern "C" int gnr_dbg_wave_clock(int which, unsigned long long* waves_host, unsigned* tiles_host) {
    if (which < 0 || which > 1 || !waves_host || !tiles_host) return GNR_ERR_ARG;
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(waves_host, HIP_SYMBOL(gnr::g_wave_clock), sizeof(unsigned long long) * 4096 * 8, sizeof(unsigned long long) * 4096 * 8 * which) != hipSuccess) return GNR_ERR_HIP;
    if (hipMemcpyFromSymbol(tiles_host, HIP_SYMBOL(gnr::g_tile_clock), sizeof(unsigned) * (1 << 17), sizeof(unsigned) * (1 << 17) * which) != hipSuccess) return GNR_ERR_HIP;
    return 0;
}
#endif
