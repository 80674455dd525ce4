// Binned scatter of the feature-map gradient (round 6; included by gnr_bwd.inc in front of the first view loop's kernels).
//
// The backward of the bilinear gather (ops.py:14-34 / render_ops.py:54-70 feeding dist_decoder.py:64-107, aggregate_net.py:46-54)
// adds, per (view, point), a 64-channel row into the four feature-map pixels of the tap.  As float atomics straight out of
// k_view1_bwd_pw that is 4 x 64 atomic dwords per (view, point) -- 786 M per 8-scene volume launch at the measured one atomic dword
// per cycle and CU (profiles/r04_g_atomic_rates_ubench.txt): 1.28 of the kernel's 3.40 ms, 8.4 GB of L2 <-> HBM traffic for 0.11 GB of
// result.  But a volume launch drops ~100 tap rows on every pixel it touches: the sums can be formed BEFORE anything is added to the
// feature-map gradient.
//
//   k_view1_bwd_pw<false, BINS = true>   the compute wavefront parks the 16 rows of a (tile, view) in HBM as they sit in its registers
//                                        (four 16-byte stores per lane, 64 contiguous bytes; no trip through the partner's ring),
//                                        one record per row (bin key = scene-view * npix + top-left tap pixel, -1 = dead row; the
//                                        four tap weights), and counts the row into its bin (one 16-lane integer atomic)
//   k_scatter_place                      per scene-view, one workgroup: exclusive prefix of the bin counts -> the bins' places in `list`,
//                                        then the row ids into them (LDS atomics on the bins' cursors; k_scatter_scan + k_scatter_fill:
//                                        the same through global memory, for feature maps whose cursors do not fit the LDS)
//   k_scatter_gather                     one wavefront per 64 consecutive list entries (perfectly balanced, whatever the bin sizes):
//                                        lane = channel, the rows of a bin are summed in registers with their four tap weights
//                                        and leave as 2 x 64 (the next bin is the right-hand neighbour: the right pixels' sums ride along)
//                                        or 4 x 64 atomic dwords per (bin, chunk)
//
// Atomic dwords per volume launch: 786 M -> ~40 M.  The rows cross HBM once each way (0.79 GB written, read once).
// Range guard: on a flagged pass the view kernel returns before it parks anything -- key / wts / rows then hold whatever the workspace
// held -- so the four kernels below take its BwdGuard and return at the same place: nothing is placed, nothing is gathered.
// Tests: tests/test_feature_scatter.py runs the stage alone (gnr_debug_feature_scatter) against a float64 and an integer model.
// Float mode: the order inside a bin follows the cursor atomics, so the low bits vary from run to run exactly as the direct float
// scatter's did.  Bit-reproducible mode (GNR_OPT_FEATURE_GRAD_FIXED): the same rows, summed as 64-bit integers (k_scatter_gather<true>).
namespace gnr {

struct ScatterBins {             // device buffers of one launch (carved from the training workspace); rows == nullptr: direct atomics
    float* rows;                 // [N][64]           N = ntiles * V * 16 rows, row id = (tile * V + v) * 16 + point of the tile
    f4* wts;                     // [N]               w00 w01 w10 w11 (x the in-image mask)
    int* key;                    // [N]               (b * V + v) * npix + o00, or -1
    int* cnt;                    // [B * V * npix]    rows per bin (zeroed before the launch)
    int* cursor;                 // [B * V * npix]    next free place of the bin in `list`
    int* list;                   // [B * V][cap]      row ids, bin after bin; cap = rows of a scene-view = (tiles per scene) * 16
    int* nseg;                   // [B * V]           live rows of the scene-view
    unsigned* upmax;             // fixed-point mode: bits of the launch's largest upstream gradient, collected by the view kernel itself
                                 // (it reads every upstream value anyway; k_absmax_bits would read dS1 -- 0.9 GB -- a second time); else null
};

// one workgroup per scene-view: cursor[bin] = seg * cap + (rows in the bins before it)
__global__ __launch_bounds__(1024) void k_scatter_scan(const int* __restrict__ cnt, int* __restrict__ cursor, int* __restrict__ nseg, int npix, int cap, BwdGuard guard) {
    __shared__ int wsum[16];
    if (bwd_guard_skip(guard)) return;
    const int seg = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (npix + 1023) / 1024;
    const int lo = min(t * per, npix), hi = min(lo + per, npix);
    const int* c = cnt + (size_t)seg * npix;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += c[i];
    int inc = s;                                                   // inclusive scan inside the wavefront
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    int run = seg * cap + base + inc - s;
    int* cu = cursor + (size_t)seg * npix;
    for (int i = lo; i < hi; ++i) { cu[i] = run; run += c[i]; }
    if (t == 1023) nseg[seg] = base + inc;
}

// Row ids into their bins' places, one atomic per row on the bins' cursors in global memory.  Fallback of k_scatter_place for feature maps
// whose cursors do not fit the LDS: returning atomics on one address serialise at the memory side (~0.5 us each across XCDs), and a
// pixel that collects a few hundred rows holds the whole launch up (0.166 ms per 8-scene volume launch, whatever the aggregation
// inside a wavefront).
__global__ __launch_bounds__(256) void k_scatter_fill(const int* __restrict__ key, int* __restrict__ cursor, int* __restrict__ list, int n, BwdGuard guard) {
    if (bwd_guard_skip(guard)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = key[i];
    if (k >= 0) list[atomicAdd(&cursor[k], 1)] = i;
}

// Scan + fill of one scene-view in one workgroup, the cursors in LDS: prefix of the bin counts, then every row of the scene-view
// takes its place with an LDS atomic (ds_add_rtn: no trip to the memory side, no cross-XCD serialisation).  The rows of scene b,
// view v are the 16-row groups (tile * V + v) of the scene's tiles.  Dynamic LDS: npix ints.
__global__ __launch_bounds__(1024) void k_scatter_place(const int* __restrict__ cnt, const int* __restrict__ key, int* __restrict__ list, int* __restrict__ nseg,
                                                        int npix, int cap, int V, BwdGuard guard) {
    extern __shared__ int cur[];
    __shared__ int wsum[16];
    if (bwd_guard_skip(guard)) return;
    const int seg = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (npix + 1023) / 1024;
    const int lo = min(t * per, npix), hi = min(lo + per, npix);
    const int* c = cnt + (size_t)seg * npix;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += c[i];
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    int run = base + inc - s;
    for (int i = lo; i < hi; ++i) { cur[i] = run; run += c[i]; }
    if (t == 1023) nseg[seg] = base + inc;
    __syncthreads();
    const int b = seg / V, v = seg - b * V, tps = cap >> 4;
    int* lp = list + (size_t)seg * cap;
    const int key0 = seg * npix;
    constexpr int U = 16;                                          // keys in flight per thread (the loop is bound by the loads' latency)
    for (int i0 = 0; i0 < cap; i0 += U * 1024) {
        int row[U], k[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 1024 + t;                       // position among the scene-view's rows: 16 per tile
            row[u] = ((b * tps + (i >> 4)) * V + v) * 16 + (i & 15);
            k[u] = i < cap ? key[row[u]] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k[u] >= 0) lp[atomicAdd(&cur[k[u] - key0], 1)] = row[u];
    }
}

// Test tooling (gnr_debug_feature_scatter): what the view kernel does for the bins of caller-given rows.  key_in -> key with every
// key outside its own row's scene-view range [seg * npix, (seg + 1) * npix) turned into -1 (counted in *neutralised: nothing behind
// this kernel can then leave cnt / cursor / list / the LDS cursors), the live rows counted into their bins, and the bits of the
// upstream maximum put where the fixed-point kernels look for them.  Row i = ((b * tps + tile) * V + v) * 16 + point.
__global__ __launch_bounds__(256) void k_scatter_debug_keys(const int* __restrict__ key_in, int* __restrict__ key, int* __restrict__ cnt,
                                                            unsigned* __restrict__ neutralised, unsigned* __restrict__ upmax, unsigned upmax_bits,
                                                            int n, int V, int tps, int npix) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && upmax) upmax[0] = upmax_bits;
    if (i >= n) return;
    const int pair = i >> 4, v = pair % V, b = (pair / V) / tps, seg = b * V + v;
    int k = key_in[i];
    if (k != -1 && (k < seg * npix || k >= (seg + 1) * npix)) { k = -1; atomicAdd(neutralised, 1u); }
    key[i] = k;
    if (k >= 0) atomicAdd(&cnt[k], 1);
}

struct ScatterGatherArgs {
    ScatterBins sc;
    float* dfeat64;              // [B * V][npix][64]  (FX: 64-bit entries)
    int nsegs, cap, npix, fh, fw;
    FeatFx fx;                   // FX instantiation only
    BwdGuard guard;              // the guard of the view kernel that parked the rows
};

// position of a value in a parked row -> channel of the channel-last feature-map gradient: the compute wavefront's lane (point r, group g)
// stores its 8 ray-feature and its 8 image-feature gradients as 16 consecutive floats at 16 g
DEV int scatter_channel(int pos) { const int g = pos >> 4, j = pos & 15; return j < 8 ? 8 * g + j : 32 + 8 * g + (j - 8); }

// one bin's sums -> the feature-map gradient.  left: the pixels (x0, y0) / (x0, y0 + 1); right: (x0 + 1, ...).  At the last column / row
// the far taps carry weight 0 (make_taps) and are skipped.  T = float (float atomics) or long long (multiples of the quantum, 64-bit adds).
template <class T>
DEV void scatter_add(float* __restrict__ base, size_t idx, T x) {
    if constexpr (sizeof(T) == 4) unsafeAtomicAdd(base + idx, x);
    else {      // a double holding an integer of magnitude < 2^51 (64 rows x 2^42 at most) -> the same integer, through the mantissa
        const long long q = __double_as_longlong(x + 6755399441055744.0) - 0x4338000000000000LL;
        atomicAdd(reinterpret_cast<unsigned long long*>(base) + idx, (unsigned long long)q);
    }
}
// one contribution as a multiple of the quantum, rounded to nearest even and clamped exactly like fx_quantise, but kept as a double:
// the sums of a chunk (64 rows x |q| <= 2^42) are integers below 2^53, i.e. exact in double arithmetic -- one v_add_f64 per tap
// instead of a float -> int64 sequence and a 64-bit integer add
DEV double fx_quantise_d(float x, float scale, unsigned* __restrict__ flag) {
    float y = x * scale;
    if (!(fabsf(y) < 0x1p42f)) {
        atomicOr(flag, 8u);
        y = (y != y) ? 0.f : copysignf(0x1p42f, y);
    }
    return (double)__builtin_rintf(y);
}
template <class T>
DEV void scatter_flush(float* __restrict__ dfeat, int key, int seg, int npix, int fh, int fw, int lane, T a00, T a01, T a10, T a11, bool left, bool right) {
    const int o = key - seg * npix, y0 = o / fw, x0 = o - y0 * fw;
    const size_t p = (size_t)key * 64 + scatter_channel(lane);
    const int dx = x0 < fw - 1 ? 64 : 0, dy = y0 < fh - 1 ? fw * 64 : 0;
    if (left) {
        scatter_add(dfeat, p, a00);
        if (dy) scatter_add(dfeat, p + dy, a10);
    }
    if (right && dx) {
        scatter_add(dfeat, p + dx, a01);
        if (dy) scatter_add(dfeat, p + dx + dy, a11);
    }
}

// FX (GNR_OPT_FEATURE_GRAD_FIXED): every contribution row x tap weight is rounded ONCE to a multiple of the launch's quantum -- exactly
// the rounding of the direct 64-bit scatter (feat_add<true>) -- and the sums are integers: whatever order the cursor atomics put the rows
// of a bin in, and wherever the 64-row chunks cut it, the feature-map gradient comes out the same bits (and the same bits as the direct
// fixed-point scatter's).  The bit-reproducible mode costs what the float mode costs (0.3 ms per volume launch instead of +1.9 ms).
template <bool FX>
__global__ __launch_bounds__(256) void k_scatter_gather(ScatterGatherArgs a) {
    using T = std::conditional_t<FX, double, float>;
    if (bwd_guard_skip(a.guard)) return;
    const int lane = threadIdx.x & 63;
    const int chunk = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int cps = (a.cap + 63) >> 6;
    const int seg = chunk / cps, c = chunk - seg * cps;
    if (seg >= a.nsegs) return;
    const int left = a.sc.nseg[seg] - c * 64;
    if (left <= 0) return;
    const int n = __builtin_amdgcn_readfirstlane(min(left, 64));
    const int* lp = a.sc.list + (size_t)seg * a.cap + c * 64;
    const int idx = lane < n ? lp[lane] : 0;
    const int key = lane < n ? a.sc.key[idx] : -1;
    const f4 w = lane < n ? a.sc.wts[idx] : f4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ rows = a.sc.rows + lane;
    const float fxs = FX ? fx_scale(a.fx) : 0.f;
    T a00 = 0, a01 = 0, a10 = 0, a11 = 0;
    int cur = __builtin_amdgcn_readlane(key, 0);
    for (int j0 = 0; j0 < n; j0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = min(j0 + u, n - 1);
            v[u] = rows[(size_t)__builtin_amdgcn_readlane(idx, j) * 64];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            if (j < n) {
                const int k = __builtin_amdgcn_readlane(key, j);
                if (k != cur) {
                    // the list is in raster order: when the next bin is the right-hand neighbour, this bin's right pixels are that bin's
                    // left pixels -- their sums ride along instead of leaving as atomics (two rows per bin instead of four)
                    const bool carry = k == cur + 1 && (cur - seg * a.npix) % a.fw != a.fw - 1;
                    scatter_flush<T>(a.dfeat64, cur, seg, a.npix, a.fh, a.fw, lane, a00, a01, a10, a11, true, !carry);
                    cur = k;
                    a00 = carry ? a01 : T(0); a10 = carry ? a11 : T(0); a01 = 0; a11 = 0;
                }
                const float w00 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(w.x), j));
                const float w01 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(w.y), j));
                const float w10 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(w.z), j));
                const float w11 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(w.w), j));
                if constexpr (FX) {                         // (a tap of weight 0 adds nothing and raises no flag, as in the direct scatter)
                    if (w00 != 0.f) a00 += fx_quantise_d(v[u] * w00, fxs, a.fx.flag);
                    if (w01 != 0.f) a01 += fx_quantise_d(v[u] * w01, fxs, a.fx.flag);
                    if (w10 != 0.f) a10 += fx_quantise_d(v[u] * w10, fxs, a.fx.flag);
                    if (w11 != 0.f) a11 += fx_quantise_d(v[u] * w11, fxs, a.fx.flag);
                } else {
                    a00 = fmaf(v[u], w00, a00); a01 = fmaf(v[u], w01, a01); a10 = fmaf(v[u], w10, a10); a11 = fmaf(v[u], w11, a11);
                }
            }
        }
    }
    scatter_flush<T>(a.dfeat64, cur, seg, a.npix, a.fh, a.fw, lane, a00, a01, a10, a11, true, true);
}

}  // namespace gnr
