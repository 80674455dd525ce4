// Grasp post-processing on the device: the reference planner's process() + select()  (src/nr/main.py:23-84), which
// call scipy.ndimage on the host for every plan.  64 000 voxels per scene: byte/float streaming work, one thread per
// voxel, no MFMA.  Bit-exact with scipy: the Gaussian accumulates in fp64 in scipy's order and rounds to fp32 after
// every axis (ni_filters.c, symmetric branch); dilation and the max filter are exact by nature.
// Also the real-robot route of src/nr/utils/grasp_utils.py:40-151 and draw_utils.py:355-377: process with its own outside threshold,
// the survivors ranked by score (k_rank) and the surface point cloud (k_surf_*).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gnr_compact.h"
#include "gnr_host.h"

namespace gnr_post {

using namespace gnr;

struct GaussW { double w[GNR_GAUSS_MAX_RADIUS + 1]; int radius; };

// one axis of gaussian_filter(mode='nearest'): out = fp32( w0*in[i] + sum_{k=r..1} (in[i-k] + in[i+k]) * w[k] ), fp64 inside
__global__ void k_gauss_axis(const float* __restrict__ in, float* __restrict__ out, int R, int stride, GaussW g, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = (int)((t / (size_t)stride) % (size_t)R);
    const float* p = in + t;
    double acc = (double)p[0] * g.w[0];
    for (int k = g.radius; k >= 1; --k) {
        const int lo = max(i - k, 0) - i, hi = min(i + k, R - 1) - i;
        acc += ((double)p[(ptrdiff_t)lo * stride] + (double)p[(ptrdiff_t)hi * stride]) * g.w[k];
    }
    out[t] = (float)acc;
}

// outside = tsdf > outside ; may_change = !(low < tsdf < high)      (main.py:45-49: outside == high; grasp_utils.py:59-60: 0.1 / -0.1)
__global__ void k_masks(const float* __restrict__ tsdf, unsigned char* __restrict__ x, unsigned char* __restrict__ m,
                        float outside, float high, float low, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float v = tsdf[t];
    x[t] = v > outside ? 1 : 0;
    m[t] = (low < v && v < high) ? 0 : 1;
}

// one iteration of binary_dilation(structure = 6-neighbourhood, mask, border_value=0)
__global__ void k_dilate(const unsigned char* __restrict__ x, const unsigned char* __restrict__ m, unsigned char* __restrict__ y,
                         int R, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int k = (int)(t % R), j = (int)((t / R) % R), i = (int)((t / ((size_t)R * R)) % R);
    unsigned char v = x[t];
    if (m[t] && !v) {
        const int R2 = R * R;
        v = (i > 0 && x[t - R2]) || (i + 1 < R && x[t + R2]) || (j > 0 && x[t - R]) || (j + 1 < R && x[t + R]) ||
            (k > 0 && x[t - 1]) || (k + 1 < R && x[t + 1]);
    }
    y[t] = v;
}

// processed quality (main.py:50-55) and its thresholded copy (main.py:61)
__global__ void k_finalize(const float* __restrict__ qs, const unsigned char* __restrict__ valid, const float* __restrict__ width,
                           float* __restrict__ qual_out, float* __restrict__ qthr, float min_w, float max_w, float thr, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float w = width[t];
    float q = qs[t];
    if (!valid[t] || w < min_w || w > max_w) q = 0.f;
    qual_out[t] = q;
    qthr[t] = q < thr ? 0.f : q;
}

// non-maximum suppression: keep q where q == maximum_filter(q, size, mode='reflect') and q != 0   (main.py:64-68)
__global__ void k_nms(const float* __restrict__ q, unsigned char* __restrict__ keep, int R, int size, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int k = (int)(t % R), j = (int)((t / R) % R), i = (int)((t / ((size_t)R * R)) % R);
    const float* vol = q + (t - ((size_t)i * R + j) * R - k);
    const float c = q[t];
    if (c == 0.f) { keep[t] = 0; return; }
    const int left = size / 2, right = size - size / 2 - 1;
    auto refl = [R](int a) { return a < 0 ? -a - 1 : (a >= R ? 2 * R - 1 - a : a); };
    float m = c;
    for (int di = -left; di <= right; ++di) {
        const int ii = refl(i + di);
        for (int dj = -left; dj <= right; ++dj) {
            const int jj = refl(j + dj);
            const float* row = vol + ((size_t)ii * R + jj) * R;
            for (int dk = -left; dk <= right; ++dk) m = fmaxf(m, row[refl(k + dk)]);
        }
    }
    keep[t] = (c == m) ? 1 : 0;
}

// ordered compaction (np.argwhere order = ascending linear index), one workgroup per volume   (main.py:70-77); rows of max_n
// entries, the first `limit` <= max_n survivors stored
__global__ __launch_bounds__(1024) void k_compact(const unsigned char* __restrict__ keep, const float* __restrict__ q,
                                                  const float* __restrict__ rot, const float* __restrict__ width, int R, int max_n,
                                                  int limit, int* __restrict__ count, int* __restrict__ index, float* __restrict__ score,
                                                  float* __restrict__ quat, float* __restrict__ width_out) {
    __shared__ int wave_tot[16];
    __shared__ int base_s;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n = (size_t)R * R * R;
    const unsigned char* kb = keep + (size_t)b * n;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (size_t c0 = 0; c0 < n; c0 += 1024) {
        const size_t t = c0 + threadIdx.x;
        const bool f = t < n && kb[t];
        const unsigned long long bal = __ballot(f);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wave; ++w) off += wave_tot[w];
        const int pos = off + before;
        if (f && pos < limit) {
            const int k = (int)(t % R), j = (int)((t / R) % R), i = (int)(t / ((size_t)R * R));
            const size_t o = (size_t)b * max_n + pos;
            index[o * 3] = i; index[o * 3 + 1] = j; index[o * 3 + 2] = k;
            score[o] = q[(size_t)b * n + t];
            for (int c = 0; c < 4; ++c) quat[o * 4 + c] = rot[((size_t)b * 4 + c) * n + t];
            width_out[o] = width[(size_t)b * n + t];
        }
        __syncthreads();
        if (threadIdx.x == 0) { int s = base_s; for (int w = 0; w < 16; ++w) s += wave_tot[w]; base_s = s; }
        __syncthreads();
    }
    if (threadIdx.x == 0) count[b] = base_s;
}

// float -> unsigned whose ASCENDING order is the floats' DESCENDING order (negative scores included): the usual order-preserving
// map (flip every bit of a negative, the sign bit of a non-negative), complemented
__device__ inline unsigned key_desc(float v) {
    const unsigned u = __float_as_uint(v);
    return ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
}

// Ranked selection (grasp_utils.py:105, np.argsort(scores)[::-1][:top_k], over ALL survivors), one workgroup per volume:
//   1. ordered compaction of the survivors' (key, linear index) pairs, as k_compact;
//   2. a stable least-significant-bit-first binary radix sort of the pairs by key, 32 passes between two buffers (a pass whose bit
//      is the same in every key moves nothing and is skipped): stable, so equal scores stay in ascending linear index;
//   3. the first `limit` pairs become the output rows.
// ka/kb, ia/ib: [B, R^3] each.  count[b] = all survivors.
__global__ __launch_bounds__(1024) void k_rank(const unsigned char* __restrict__ keep, const float* __restrict__ q,
                                               const float* __restrict__ rot, const float* __restrict__ width, int R, int max_n,
                                               int limit, unsigned* ka, unsigned* kb, int* ia, int* ib, int* __restrict__ count,
                                               int* __restrict__ index, float* __restrict__ score, float* __restrict__ quat,
                                               float* __restrict__ width_out) {
    __shared__ int wave_tot[16];
    __shared__ int zeros[32];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t n = (size_t)R * R * R;
    const unsigned char* kp = keep + (size_t)b * n;
    const float* qb = q + (size_t)b * n;
    ka += (size_t)b * n; kb += (size_t)b * n; ia += (size_t)b * n; ib += (size_t)b * n;
    if (tid < 32) zeros[tid] = 0;
    int m = 0;
    for (size_t c0 = 0; c0 < n; c0 += 1024) {
        const size_t t = c0 + tid;
        const bool f = t < n && kp[t];
        int tot;
        const int pos = m + block_rank(f, wave_tot, tot);
        if (f) { ka[pos] = key_desc(qb[t]); ia[pos] = (int)t; }
        m += tot;
    }
    __syncthreads();                                   // the pairs are written (and zeros[] is cleared)
    for (int c0 = 0; c0 < m; c0 += 1024) {             // zeros[bit] = keys whose bit is 0: a permutation does not change it
        const bool v = c0 + tid < m;
        const unsigned key = v ? ka[c0 + tid] : 0u;
        for (int bit = 0; bit < 32; ++bit) {
            const unsigned long long bal = __ballot(v && !((key >> bit) & 1u));
            if ((tid & 63) == 0 && bal) atomicAdd(&zeros[bit], __popcll(bal));
        }
    }
    __syncthreads();
    for (int bit = 0; bit < 32; ++bit) {
        const int nz = zeros[bit];
        if (nz == 0 || nz == m) continue;              // uniform over the workgroup
        int b0 = 0, b1 = nz;
        for (int c0 = 0; c0 < m; c0 += 1024) {
            const bool v = c0 + tid < m;
            const unsigned key = v ? ka[c0 + tid] : 0u;
            const int id = v ? ia[c0 + tid] : 0;
            const bool z = v && !((key >> bit) & 1u);
            int tz;
            const int rz = block_rank(z, wave_tot, tz);
            const int valid = min(m - c0, 1024);
            if (v) {
                const int pos = z ? b0 + rz : b1 + (tid - rz);         // tid - rz: the ones in front of this thread
                kb[pos] = key; ib[pos] = id;
            }
            b0 += tz; b1 += valid - tz;
        }
        __syncthreads();                               // this pass's writes, before the next pass reads them
        unsigned* tk = ka; ka = kb; kb = tk;
        int* ti = ia; ia = ib; ib = ti;
    }
    const int rows = min(m, limit);
    for (int r = tid; r < rows; r += 1024) {
        const size_t t = (size_t)ia[r];
        const int k = (int)(t % R), j = (int)((t / R) % R), i = (int)(t / ((size_t)R * R));
        const size_t o = (size_t)b * max_n + r;
        index[o * 3] = i; index[o * 3 + 1] = j; index[o * 3 + 2] = k;
        score[o] = qb[t];
        for (int c = 0; c < 4; ++c) quat[o * 4 + c] = rot[((size_t)b * 4 + c) * n + t];
        width_out[o] = width[(size_t)b * n + t];
    }
    if (tid == 0) count[b] = m;
}

// ---- surface point cloud (draw_utils.py:355-377): the voxels with lo < vol < hi in nonzero (ascending linear index) order ----
// 1. voxels in range per chunk of 1024;  2. exclusive scan of the chunk counts per volume;  3. every chunk writes its rows.
__device__ inline bool in_range(float v, float lo, float hi) { return v > lo && v < hi; }

__global__ __launch_bounds__(1024) void k_surf_count(const float* __restrict__ vol, size_t n, float lo, float hi, int* __restrict__ chunk) {
    __shared__ int wave_tot[16];
    const size_t t = (size_t)blockIdx.x * 1024 + threadIdx.x;
    int tot;
    block_rank(t < n && in_range(vol[(size_t)blockIdx.y * n + t], lo, hi), wave_tot, tot);
    if (threadIdx.x == 0) chunk[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

__global__ __launch_bounds__(1024) void k_surf_scan(int* __restrict__ chunk, int nc, int* __restrict__ count) {
    __shared__ int wave_tot[16];
    const int total = scan_chunks(chunk + (size_t)blockIdx.x * nc, nc, wave_tot);
    if (threadIdx.x == 0) count[blockIdx.x] = total;
}

struct SurfColor { int value_map; float rgb[3]; float a, b, m; };

__global__ __launch_bounds__(1024) void k_surf_write(const float* __restrict__ vol, int R, size_t n, float lo, float hi, SurfColor col,
                                                     double scale, const int* __restrict__ chunk, int max_n, int* __restrict__ index,
                                                     double* __restrict__ points, float* __restrict__ colors) {
    __shared__ int wave_tot[16];
    const int b = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * 1024 + threadIdx.x;
    const float v = t < n ? vol[(size_t)b * n + t] : 0.f;
    const bool f = t < n && in_range(v, lo, hi);
    int tot;
    const int pos = chunk[(size_t)b * gridDim.x + blockIdx.x] + block_rank(f, wave_tot, tot);
    if (!f || pos >= max_n) return;
    const int k = (int)(t % R), j = (int)((t / R) % R), i = (int)(t / ((size_t)R * R));
    const size_t o = ((size_t)b * max_n + pos) * 3;
    index[o] = i; index[o + 1] = j; index[o + 2] = k;
    points[o] = (double)i * scale; points[o + 1] = (double)j * scale; points[o + 2] = (double)k * scale;
    float r = col.rgb[0], g = col.rgb[1], bl = col.rgb[2];
    if (col.value_map) {                               // draw_utils.py:364-370, float32, no multiplication: nothing to contract
        const bool low = v <= col.m;
        r = low ? v - col.a : -v + col.b;
        g = low ? 0.f : 1.f - r;
        bl = low ? 1.f - r : 0.f;
    }
    colors[o] = r; colors[o + 1] = g; colors[o + 2] = bl;
}

// rows of a gradient volume at the voxels of a surface cloud: out[b][r] = grad[b][index[b][r]] for r < min(count[b], max_n)
__global__ __launch_bounds__(256) void k_surf_gradient(const float* __restrict__ grad, const int* __restrict__ index, const int* __restrict__ count,
                                                       int R, int max_n, float* __restrict__ out) {
    const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    const int n = min(count[b], max_n);
    if (r >= n) return;
    const size_t o = ((size_t)b * max_n + r) * 3;
    // (an index outside the volume is not gnr_surface_points_fwd's: clamped, never read out of bounds)
    const int i = min(max(index[o], 0), R - 1), j = min(max(index[o + 1], 0), R - 1), k = min(max(index[o + 2], 0), R - 1);
    const float* g = grad + (((size_t)b * R + i) * R + j) * (size_t)R * 3 + (size_t)k * 3;
    out[o] = g[0]; out[o + 1] = g[1]; out[o + 2] = g[2];
}

}  // namespace gnr_post

using namespace gnr_post;

extern "C" const char* gnr_post_last_error(void) { return gnr_last_error(); }       // alias: the library has one error text

// the select workspace: two float and three byte volumes, then, to rank by score, two key and two index volumes
struct SelectWork { float *fa, *fb; unsigned char *xa, *xb, *mk; unsigned *ka, *kb; int *ia, *ib; size_t total; };

static SelectWork carve_select(int B, int R, int order, void* base) {
    const size_t n = (size_t)B * R * R * R;
    Carve c(base);
    SelectWork k{c.take<float>(n), c.take<float>(n), c.take<unsigned char>(n), c.take<unsigned char>(n), c.take<unsigned char>(n)};     // (in this order)
    if (order == GNR_SELECT_ORDER_SCORE) { k.ka = c.take<unsigned>(n); k.kb = c.take<unsigned>(n); k.ia = c.take<int>(n); k.ib = c.take<int>(n); }
    k.total = c.total();
    return k;
}

extern "C" size_t gnr_grasp_select_workspace_bytes(int B, int R) {
    return B < 1 || R < 1 ? 0 : carve_select(B, R, GNR_SELECT_ORDER_INDEX, nullptr).total;
}

extern "C" size_t gnr_grasp_select_v2_workspace_bytes(int B, int R, int order) {
    return B < 1 || R < 1 ? 0 : carve_select(B, R, order, nullptr).total;
}

// Both select entry points: `who` = 0 the original call (its refusals keep their texts), 1 the v2 call.
static int select_impl(int who, const float* tsdf, const float* qual, const float* rot, const float* width, int B, int R,
                       const GnrSelectParams* p, float outside, int order, int top_k, float* qual_out, int* count, int* index,
                       float* score, float* quat, float* width_out, int max_n, void* ws, size_t ws_bytes, void* stream) {
    const Refuse no{who ? "gnr_grasp_select_v2_fwd" : "gnr_grasp_select_fwd"};
    if (!tsdf || !qual || !rot || !width || !p || !qual_out || !count || !index || !score || !quat || !width_out || !ws)
        return no(GNR_ERR_ARG, "null pointer");
    if (B < 1 || !lattice_ok(R) || max_n < 1) return no(GNR_ERR_SHAPE, "bad B / R / max_n");
    if (p->gauss_radius < 0 || p->gauss_radius > GNR_GAUSS_MAX_RADIUS || p->dilate_iterations < 0 || p->max_filter_size < 1 ||
        p->max_filter_size > 16)
        return no(GNR_ERR_ARG, "bad filter parameters");
    // (the next three are the v2 call's alone: the original call passes GNR_SELECT_ORDER_INDEX and top_k 0)
    if (order != GNR_SELECT_ORDER_INDEX && order != GNR_SELECT_ORDER_SCORE)
        return no(GNR_ERR_ARG, "order must be GNR_SELECT_ORDER_INDEX or GNR_SELECT_ORDER_SCORE");
    if (top_k < 0) return no(GNR_ERR_ARG, "top_k must be >= 0 (0: as many as max_n)");
    if (order == GNR_SELECT_ORDER_SCORE && R > GNR_SELECT_SCORE_MAX_R)
        return no(GNR_ERR_SHAPE, "GNR_SELECT_ORDER_SCORE takes R <= 64 (2^18 voxels per scene to rank)");
    const SelectWork k = carve_select(B, R, order, ws);
    if (ws_bytes < k.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)B * R * R * R;
    float *fa = k.fa, *fb = k.fb;
    unsigned char *xa = k.xa, *xb = k.xb, *mk = k.mk;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    GaussW g;
    g.radius = p->gauss_radius;
    for (int k = 0; k <= GNR_GAUSS_MAX_RADIUS; ++k) g.w[k] = k <= p->gauss_radius ? p->gauss_w[k] : 0.0;
    // Gaussian, axes in scipy's order (0, 1, 2), fp32 rounding after each
    const dim3 grid(blocks), block(256);
    if (int rc = launch<k_gauss_axis>(nullptr, st, grid, block, 0, qual, fa, R, R * R, g, n)) return rc;
    if (int rc = launch<k_gauss_axis>(nullptr, st, grid, block, 0, fa, fb, R, R, g, n)) return rc;
    if (int rc = launch<k_gauss_axis>(nullptr, st, grid, block, 0, fb, fa, R, 1, g, n)) return rc;
    if (int rc = launch<k_masks>(nullptr, st, grid, block, 0, tsdf, xa, mk, outside, p->tsdf_thres_high, p->tsdf_thres_low, n)) return rc;
    unsigned char *xin = xa, *xout = xb;
    for (int it = 0; it < p->dilate_iterations; ++it) {
        if (int rc = launch<k_dilate>(nullptr, st, grid, block, 0, xin, mk, xout, R, n)) return rc;
        unsigned char* tmp = xin; xin = xout; xout = tmp;
    }
    if (int rc = launch<k_finalize>(nullptr, st, grid, block, 0, fa, xin, width, qual_out, fb, p->min_width, p->max_width, p->threshold, n)) return rc;
    if (int rc = launch<k_nms>(nullptr, st, grid, block, 0, fb, xout, R, p->max_filter_size, n)) return rc;
    const int limit = top_k > 0 && top_k < max_n ? top_k : max_n;
    if (order == GNR_SELECT_ORDER_INDEX)
        return launch<k_compact>(nullptr, st, dim3(B), dim3(1024), 0, xout, fb, rot, width, R, max_n, limit, count, index, score, quat, width_out);
    return launch<k_rank>(nullptr, st, dim3(B), dim3(1024), 0, xout, fb, rot, width, R, max_n, limit, k.ka, k.kb, k.ia, k.ib, count, index, score,
                          quat, width_out);
}

extern "C" int gnr_grasp_select_fwd(const float* tsdf, const float* qual, const float* rot, const float* width, int B, int R,
                                    const GnrSelectParams* p, float* qual_out, int* count, int* index, float* score, float* quat,
                                    float* width_out, int max_n, void* ws, size_t ws_bytes, void* stream) {
    return select_impl(0, tsdf, qual, rot, width, B, R, p, p ? p->tsdf_thres_high : 0.f, GNR_SELECT_ORDER_INDEX, 0, qual_out, count, index,
                       score, quat, width_out, max_n, ws, ws_bytes, stream);
}

extern "C" int gnr_grasp_select_v2_fwd(const float* tsdf, const float* qual, const float* rot, const float* width, int B, int R,
                                       const GnrSelectParamsV2* p, float* qual_out, int* count, int* index, float* score, float* quat,
                                       float* width_out, int max_n, void* ws, size_t ws_bytes, void* stream) {
    return select_impl(1, tsdf, qual, rot, width, B, R, p ? &p->select : nullptr, p ? p->tsdf_thres_outside : 0.f, p ? p->order : 0,
                       p ? p->top_k : 0, qual_out, count, index, score, quat, width_out, max_n, ws, ws_bytes, stream);
}

// the surface cloud's workspace: the chunk counts [B, chunks of 1024 voxels]
struct SurfaceWork { int* chunk; size_t total; };

static SurfaceWork carve_surface(int B, int R, void* base) {
    Carve c(base);
    return SurfaceWork{c.take<int>(B * (((size_t)R * R * R + 1023) / 1024)), c.total()};
}

extern "C" size_t gnr_surface_points_workspace_bytes(int B, int R) {
    return B < 1 || R < 1 ? 0 : carve_surface(B, R, nullptr).total;
}

extern "C" int gnr_surface_points_fwd(const float* vol, int B, int R, const GnrSurfaceParams* p, int* count, int* index, double* points,
                                      float* colors, int max_n, void* ws, size_t ws_bytes, void* stream) {
    const Refuse no{"gnr_surface_points_fwd"};
    if (!vol || !p || !count || !index || !points || !colors || !ws) return no(GNR_ERR_ARG, "null pointer");
    if (!scenes_ok(B) || R < 1 || R > MAX_LATTICE || max_n < 1) return no(GNR_ERR_SHAPE, "bad B / R / max_n (R <= 256)");
    if (p->color_mode != GNR_SURFACE_COLOR_FIXED && p->color_mode != GNR_SURFACE_COLOR_VALUE)
        return no(GNR_ERR_ARG, "color_mode must be GNR_SURFACE_COLOR_FIXED or GNR_SURFACE_COLOR_VALUE");
    const SurfaceWork k = carve_surface(B, R, ws);
    if (ws_bytes < k.total) return fail(GNR_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)R * R * R;
    const int nc = (int)((n + 1023) / 1024);
    int* chunk = k.chunk;
    SurfColor col;
    col.value_map = p->color_mode == GNR_SURFACE_COLOR_VALUE;
    for (int c = 0; c < 3; ++c) col.rgb[c] = p->color[c];
    col.a = p->bound_a; col.b = p->bound_b;
    col.m = (p->bound_a + p->bound_b) / 2.f;
    const dim3 grid(nc, B), block(1024);
    if (int rc = launch<k_surf_count>(nullptr, st, grid, block, 0, vol, n, p->lo, p->hi, chunk)) return rc;
    if (int rc = launch<k_surf_scan>(nullptr, st, dim3(B), block, 0, chunk, nc, count)) return rc;
    return launch<k_surf_write>(nullptr, st, grid, block, 0, vol, R, n, p->lo, p->hi, col, p->scale, (const int*)chunk, max_n, index, points, colors);
}

extern "C" int gnr_surface_gradient_fwd(const float* grad, const int* index, const int* count, int B, int R, int max_points, float* out, void* stream) {
    const Refuse no{"gnr_surface_gradient_fwd"};
    if (!grad || !index || !count || !out) return no(GNR_ERR_ARG, "null pointer");
    if (!scenes_ok(B) || R < 1 || R > MAX_LATTICE || max_points < 0) return no(GNR_ERR_SHAPE, "bad B / R / max_points (1 <= R <= 256, max_points >= 0)");
    if (max_points == 0) return GNR_OK;
    return launch<k_surf_gradient>(nullptr, (hipStream_t)stream, dim3((max_points + 255) / 256, B), dim3(256), 0, grad, index, count, R, max_points, out);
}
