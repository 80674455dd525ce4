// Frame metrics of a validation pass on the device (reference: src/nr/network/metrics.py:14-30,40-84 -- PSNR_SSIM.__call__,
// compute_psnr, compute_mae; utils/base_utils.py:496-499 -- color_map_backward): B frames at once -> float64 results per scene.
//   PSNR per prediction: both images quantised as color_map_backward does (ONE fp32 multiply by 255, clip to [0,255], truncation to
//     uint8), cropped by the margins; the squared differences are integers <= 65 025 and are summed as 64-bit integers (exact in any
//     order: integer atomics), the rest is double.  mse == 0 -> +inf (as numpy), a non-finite pixel of the crop -> NaN.
//   depth MAE: mean of the fp32 |depth_pr - depth_gt| over the UNCROPPED frame (as the reference), summed in double in a fixed order:
//     one partial per workgroup in the workspace, one fixed-order second stage (the pattern of k_grad_reduce).  No float atomics.
//   SSIM per prediction (the reference computes it, metrics.py:71, and drops it): skimage.metrics.structural_similarity(gt, pr,
//     win_size=11, multichannel=True, data_range=255) on the quantised, cropped images.  The 11x11 window sums of x, y, xx, yy, xy
//     are integers < 2^23 (121 * 255^2) kept exact in int32 (separable: a horizontal pass into LDS, then a vertical one over a
//     tile with a 5-pixel halo); S is evaluated in double without contraction, and summed in a fixed order like the MAE.
// Launch-bound and bandwidth-trivial (7 MB at 288x512 with two predictions): no matrix cores, no vector-width games.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "gnr_host.h"

namespace gnr_metrics {

using namespace gnr;

constexpr int PIX_PER_BLOCK = 1024;                 // k_frame_pixels: 256 lanes x 4 pixels
constexpr int WIN = 11, HALO = WIN - 1;             // SSIM window; a tile of TH x TW window positions reads (TH + 10) x (TW + 10) pixels
constexpr int TH = 16, TW = 32, IH = TH + HALO, IW = TW + HALO;

struct Dims {
    int B, h, w, n_pred, hm, wm;                    // margins of the crop (metrics.py:54-57)
    int ch, cw;                                     // cropped size
    int nblk;                                       // workgroups of k_frame_pixels per scene
    int tx, ty;                                     // SSIM tiles per cropped frame
};

static Dims dims(int B, int h, int w, int n_pred, int hm, int wm) {
    Dims d{B, h, w, n_pred, hm, wm, h - 2 * hm, w - 2 * wm, 0, 0, 0};
    d.nblk = (int)(((long long)h * w + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK);
    d.tx = d.cw >= WIN ? (d.cw - HALO + TW - 1) / TW : 0;
    d.ty = d.ch >= WIN ? (d.ch - HALO + TH - 1) / TH : 0;
    return d;
}

struct Work {
    unsigned long long* sse;                        // [B][n_pred]     zeroed by the entry point
    int* bad;                                       // [B][n_pred]     zeroed by the entry point: a non-finite pixel inside the crop
    double* mae_part;                               // [B][nblk]
    double* ssim_part;                              // [B][n_pred][3][tx * ty]   (ssim only)
    size_t zero_bytes, total;
};

static Work carve(const Dims& d, bool ssim, void* base) {
    Work k;
    Carve c(base);
    const size_t bp = (size_t)d.B * d.n_pred;
    k.sse = c.take<unsigned long long>(bp);
    k.bad = c.take<int>(bp);
    k.zero_bytes = c.total();
    k.mae_part = c.take<double>((size_t)d.B * d.nblk);
    k.ssim_part = ssim ? c.take<double>(bp * 3 * (size_t)d.tx * d.ty) : nullptr;
    k.total = c.total();
    return k;
}

struct Preds { const float* p[GNR_METRICS_MAX_PRED]; };

// color_map_backward (base_utils.py:496-499): rgb * 255 in fp32, np.clip to [0, 255], astype(uint8) = truncation
__device__ __forceinline__ int quant(float v) {
    const float s = v * 255.0f;
    return (int)fminf(fmaxf(s, 0.0f), 255.0f);      // (a NaN comes out as 0; its image is flagged and reported as NaN)
}
__device__ __forceinline__ bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// Tree sum of one double per lane of a 256-lane workgroup: the same shape every run, so the same bits.  Every lane gets the result.
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// ---- stage 1: squared error of the quantised images inside the crop, |depth difference| over the whole frame -----------------
__global__ __launch_bounds__(256) void k_frame_pixels(const float* __restrict__ gt, Preds pr, const float* __restrict__ depth_pr,
                                                      const float* __restrict__ depth_gt, Dims d, Work k) {
    __shared__ double red[256];
    __shared__ unsigned long long red_u[256];
    const int b = blockIdx.y, t = threadIdx.x;
    const long long npix = (long long)d.h * d.w;
    unsigned sse[GNR_METRICS_MAX_PRED] = {0, 0, 0, 0};     // (4 pixels x 3 channels x 65 025 fits)
    unsigned bad = 0;
    double mae = 0.0;
    for (int j = 0; j < PIX_PER_BLOCK / 256; ++j) {
        const long long i = (long long)blockIdx.x * PIX_PER_BLOCK + j * 256 + t;
        if (i >= npix) break;
        const size_t at = (size_t)b * npix + i;
        mae += (double)fabsf(depth_pr[at] - depth_gt[at]);
        const int y = (int)(i / d.w), x = (int)(i - (long long)y * d.w);
        if (y < d.hm || y >= d.h - d.hm || x < d.wm || x >= d.w - d.wm) continue;
        const float* g = gt + 3 * at;
        const bool gbad = !finite3(g);
        const int g0 = quant(g[0]), g1 = quant(g[1]), g2 = quant(g[2]);
        for (int p = 0; p < d.n_pred; ++p) {
            const float* v = pr.p[p] + 3 * at;
            if (gbad || !finite3(v)) bad |= 1u << p;
            const int e0 = quant(v[0]) - g0, e1 = quant(v[1]) - g1, e2 = quant(v[2]) - g2;
            sse[p] += (unsigned)(e0 * e0 + e1 * e1 + e2 * e2);
        }
    }
    const double m = block_sum(mae, red);
    if (t == 0) k.mae_part[(size_t)b * d.nblk + blockIdx.x] = m;
    for (int p = 0; p < d.n_pred; ++p) {
        __syncthreads();
        red_u[t] = sse[p];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) red_u[t] += red_u[t + s];
            __syncthreads();
        }
        if (t == 0 && red_u[0]) atomicAdd(&k.sse[(size_t)b * d.n_pred + p], red_u[0]);      // integer adds commute: exact in any order
        if ((bad >> p) & 1u) atomicOr(&k.bad[(size_t)b * d.n_pred + p], 1);
    }
}

// ---- stage 2: SSIM map of one tile of window positions, three channels, summed per channel ------------------------------------
// grid (tx * ty, n_pred, B).  Window position (oy, ox) of the cropped frame covers its pixels [oy, oy + 11) x [ox, ox + 11): the
// positions are skimage's S map with its 5-pixel border removed.
__global__ __launch_bounds__(256) void k_frame_ssim(const float* __restrict__ gt, Preds pr, Dims d, Work k) {
#pragma clang fp contract(off)
    __shared__ unsigned char qx[3][IH * IW], qy[3][IH * IW];
    __shared__ int hs[5][IH * TW];
    __shared__ double red[256];
    const int t = threadIdx.x, p = blockIdx.y, b = blockIdx.z;
    const int tile = blockIdx.x, ty0 = (tile / d.tx) * TH, tx0 = (tile % d.tx) * TW;
    const int oh = d.ch - HALO, ow = d.cw - HALO;           // window positions of the cropped frame
    const size_t frame = (size_t)b * d.h * d.w;
    const float* x = gt + 3 * frame;
    const float* y = pr.p[p] + 3 * frame;
    for (int i = t; i < IH * IW; i += 256) {
        const int r = i / IW, c = i - r * IW;
        const int cy = ty0 + r, cx = tx0 + c;               // cropped coordinates; outside: zeros that no valid position reads
        const bool in = cy < d.ch && cx < d.cw;
        const size_t at = in ? 3 * ((size_t)(cy + d.hm) * d.w + (cx + d.wm)) : 0;
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) {
            qx[c3][i] = in ? (unsigned char)quant(x[at + c3]) : 0;
            qy[c3][i] = in ? (unsigned char)quant(y[at + c3]) : 0;
        }
    }
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double cov_norm = 121.0 / 120.0;
    for (int c3 = 0; c3 < 3; ++c3) {
        __syncthreads();                                    // the tile is loaded / the previous channel's sums are consumed
        for (int i = t; i < IH * TW; i += 256) {            // horizontal 11-tap sums of every row of the tile
            const int r = i / TW, c = i - r * TW;
            int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const int a = qx[c3][r * IW + c + j], e = qy[c3][r * IW + c + j];
                sx += a; sy += e; sxx += a * a; syy += e * e; sxy += a * e;
            }
            hs[0][i] = sx; hs[1][i] = sy; hs[2][i] = sxx; hs[3][i] = syy; hs[4][i] = sxy;
        }
        __syncthreads();
        double acc = 0.0;
        for (int i = t; i < TH * TW; i += 256) {            // vertical 11-tap sums, S in double
            const int r = i / TW, c = i - r * TW;
            if (ty0 + r >= oh || tx0 + c >= ow) continue;
            int s[5] = {0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < WIN; ++j)
#pragma unroll
                for (int q = 0; q < 5; ++q) s[q] += hs[q][(r + j) * TW + c];
            const double ux = s[0] / 121.0, uy = s[1] / 121.0, uxx = s[2] / 121.0, uyy = s[3] / 121.0, uxy = s[4] / 121.0;
            const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
            const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
            acc += (A1 * A2) / (B1 * B2);
        }
        const double sum = block_sum(acc, red);
        if (t == 0) k.ssim_part[(((size_t)b * d.n_pred + p) * 3 + c3) * ((size_t)d.tx * d.ty) + tile] = sum;
    }
}

// ---- stage 3: one workgroup per scene adds the partials in a fixed order and writes the scene's row ---------------------------
// out [B][2 * n_pred + 1]: psnr[n_pred], ssim[n_pred] (NaN when not asked for), depth_mae
__device__ double fixed_sum(const double* part, int n, double* red) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += part[i];
    return block_sum(v, red);
}

__global__ __launch_bounds__(256) void k_frame_finish(Dims d, Work k, int ssim, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int b = blockIdx.x, t = threadIdx.x;
    double* row = out + (size_t)b * (2 * d.n_pred + 1);
    const double mae = fixed_sum(k.mae_part + (size_t)b * d.nblk, d.nblk, red) / ((double)d.h * (double)d.w);
    if (t == 0) row[2 * d.n_pred] = mae;
    for (int p = 0; p < d.n_pred; ++p) {
        const bool bad = k.bad[(size_t)b * d.n_pred + p] != 0;
        double s = nan("");
        if (ssim) {
            const int nt = d.tx * d.ty;
            const double n = (double)(d.ch - HALO) * (double)(d.cw - HALO);
            double m[3];
            for (int c3 = 0; c3 < 3; ++c3) m[c3] = fixed_sum(k.ssim_part + (((size_t)b * d.n_pred + p) * 3 + c3) * (size_t)nt, nt, red) / n;
            s = (m[0] + m[1] + m[2]) / 3.0;
        }
        if (t == 0) {
            const double mse = (double)k.sse[(size_t)b * d.n_pred + p] / (3.0 * (double)d.ch * (double)d.cw);
            row[p] = bad ? nan("") : (mse == 0.0 ? (double)INFINITY : 10.0 * log10(255.0 * 255.0 / mse));
            row[d.n_pred + p] = bad ? nan("") : s;
        }
    }
}

static int check_dims(const Refuse& say, int B, int h, int w, int n_pred, int hm, int wm, int ssim, Dims* out) {
    if (n_pred < 1 || n_pred > GNR_METRICS_MAX_PRED) return say(GNR_ERR_ARG, "n_pred must be in 1..4");
    if (!scenes_ok(B) || h < 1 || w < 1 || (long long)h * w > (1ll << 31) - PIX_PER_BLOCK)
        return say(GNR_ERR_SHAPE, "B in 1..65535, h, w >= 1, h * w below 2^31");
    if (hm < 0 || wm < 0 || 2 * (long long)hm >= h || 2 * (long long)wm >= w) return say(GNR_ERR_SHAPE, "the crop margins leave no pixel");
    const Dims d = dims(B, h, w, n_pred, hm, wm);
    if (ssim && (d.ch < WIN || d.cw < WIN)) return say(GNR_ERR_SHAPE, "SSIM needs a cropped frame of at least 11 x 11 pixels (the 11 x 11 window)");
    if ((long long)d.tx * d.ty > 0x7fffffffLL) return say(GNR_ERR_SHAPE, "too many SSIM tiles for one launch");
    *out = d;
    return GNR_OK;
}

}  // namespace gnr_metrics

using namespace gnr_metrics;

extern "C" {

size_t gnr_frame_metrics_workspace_bytes(int B, int h, int w, int n_pred, int h_margin, int w_margin, int ssim) {
    Dims d;
    if (check_dims(Refuse{"gnr_frame_metrics_workspace_bytes"}, B, h, w, n_pred, h_margin, w_margin, ssim, &d) != GNR_OK) return 0;
    return carve(d, ssim != 0, nullptr).total;
}

int gnr_frame_metrics(const float* gt, const float* const* preds, int n_pred, const float* depth_pr, const float* depth_gt, int B, int h,
                      int w, int h_margin, int w_margin, int ssim, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    const Refuse no{"gnr_frame_metrics"};
    if (!gt || !preds || !depth_pr || !depth_gt || !out || !workspace) return no(GNR_ERR_ARG, "null pointer");
    Dims d;
    if (int rc = check_dims(no, B, h, w, n_pred, h_margin, w_margin, ssim, &d)) return rc;
    Preds pr{};
    for (int p = 0; p < n_pred; ++p) {
        if (!preds[p]) return no(GNR_ERR_ARG, "null prediction pointer");
        pr.p[p] = preds[p];
    }
    const Work k = carve(d, ssim != 0, workspace);
    if (workspace_bytes < k.total) return no(GNR_ERR_WORKSPACE, "workspace smaller than gnr_frame_metrics_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    if (const hipError_t e = hipMemsetAsync(workspace, 0, k.zero_bytes, st)) return fail(GNR_ERR_HIP, "gnr_frame_metrics: hipMemsetAsync", e);
    if (int rc = launch<k_frame_pixels>("k_frame_pixels@gnr_frame_metrics", st, dim3(d.nblk, B), dim3(256), 0, gt, pr, depth_pr, depth_gt, d, k)) return rc;
    if (ssim)
        if (int rc = launch<k_frame_ssim>("k_frame_ssim@gnr_frame_metrics", st, dim3(d.tx * d.ty, n_pred, B), dim3(256), 0, gt, pr, d, k)) return rc;
    return launch<k_frame_finish>("k_frame_finish@gnr_frame_metrics", st, dim3(B), dim3(256), 0, d, k, ssim, out);
}

}  // extern "C"
