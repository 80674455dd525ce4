// Image ingest of the planner on the device (reference: src/nr/main.py:167-172, 191-192 -- imread(...)[:, :, :3],
// cv2.resize(img, wh) with INTER_LINEAR, / 255, HWC -> CHW): n uint8 frames -> float [n,3,dst_h,dst_w] in ONE launch, with the
// bits of planner.resize_bilinear_u8 (OpenCV's fixed-point bilinear: 11-bit coefficients, a horizontal pass at scale 2^11, a
// vertical pass with (.. + 2) >> 2).  The per-axis source indices and coefficients come from the host (float64 positions and a
// floor that a fused multiply-add would move at exact half-pixel positions: gnr_ingest_tables_host); the kernel is int32
// arithmetic (255 * 2048 and 2048 * 32640 fit) and a 256-entry table of float(i) / 255, so no device float rounding is involved.
// Launch-bound and bandwidth-trivial (4 MB in, 11 MB out at the planner's shape): one lane makes four consecutive x of one
// output row for the three planes (16-byte coalesced stores), byte gathers from the L2-resident source rows, no LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_host.h"

namespace gnr_ingest {

using namespace gnr;

typedef float f4 __attribute__((ext_vector_type(4)));

// blob: int32 x0[dw] x1[dw] a0[dw] a1[dw] y0[dh] y1[dh] b0[dh] b1[dh], then float lut[256]
static size_t table_words(int dh, int dw) { return 4 * (size_t)dw + 4 * (size_t)dh; }

// One axis of resize_bilinear_u8.axis(): i0 = floor((i + 0.5) * (sn / dn) - 0.5) in float64, the weight rounded to float32,
// both borders clamped with weight 0, rint(w * 2^11) / rint((1 - w) * 2^11) saturated to short.
static void axis_table(int dn, int sn, int* i0, int* i1, int* c0, int* c1) {
#pragma clang fp contract(off)
    const double scale = (double)sn / (double)dn;
    for (int i = 0; i < dn; ++i) {
        const double prod = ((double)i + 0.5) * scale;
        const double f = prod - 0.5;
        const double fl = floor(f);
        long long j = (long long)fl;
        float w = (float)(f - fl);
        if (j < 0) { j = 0; w = 0.f; }
        if (j >= sn - 1) { j = sn - 1; w = 0.f; }
        const double r1 = nearbyint((double)w * 2048.0), r0 = nearbyint((1.0 - (double)w) * 2048.0);
        i0[i] = (int)j;
        i1[i] = (int)(j + 1 < sn - 1 ? j + 1 : sn - 1);
        c0[i] = (int)fmin(fmax(r0, -32768.0), 32767.0);
        c1[i] = (int)fmin(fmax(r1, -32768.0), 32767.0);
    }
}

struct Args {
    const unsigned char* frames; const int* tab; const float* lut; float* out;
    size_t row_pitch, frame_pitch;
    int src_h, src_w, ch, dh, dw;
    unsigned groups, total;
};

__device__ __forceinline__ int clampi(int i, int hi) { return min(max(i, 0), hi); }

template <bool VEC>
__global__ __launch_bounds__(256) void k_ingest_u8(Args a) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.total) return;
    const unsigned row = t / a.groups, q = t - row * a.groups;
    const unsigned f = row / (unsigned)a.dh;
    const int y = (int)(row - f * (unsigned)a.dh), xb = 4 * (int)q;
    const int* tx = a.tab;
    const int* ty = a.tab + 4 * (size_t)a.dw;
    // the indices are clamped to the source once more: a blob made for another source size must not read out of bounds
    const int y0 = clampi(ty[y], a.src_h - 1), y1 = clampi(ty[a.dh + y], a.src_h - 1), b0 = ty[2 * a.dh + y], b1 = ty[3 * a.dh + y];
    const unsigned char* r0 = a.frames + (size_t)f * a.frame_pitch + (size_t)y0 * a.row_pitch;
    const unsigned char* r1 = a.frames + (size_t)f * a.frame_pitch + (size_t)y1 * a.row_pitch;
    float o[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = min(xb + k, a.dw - 1);
        const int x0 = clampi(tx[x], a.src_w - 1) * a.ch, x1 = clampi(tx[a.dw + x], a.src_w - 1) * a.ch;
        const int a0 = tx[2 * a.dw + x], a1 = tx[3 * a.dw + x];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s0 = (int)r0[x0 + c] * a0 + (int)r0[x1 + c] * a1;      // horizontal pass, scale 2^11
            const int s1 = (int)r1[x0 + c] * a0 + (int)r1[x1 + c] * a1;
            const int v = (((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2;
            o[c][k] = a.lut[min(max(v, 0), 255)];
        }
    }
    const size_t plane = (size_t)a.dh * a.dw;
    float* dst = a.out + (size_t)f * 3 * plane + (size_t)y * a.dw + xb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (VEC) {
            *reinterpret_cast<f4*>(dst + c * plane) = f4{o[c][0], o[c][1], o[c][2], o[c][3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (xb + k < a.dw) dst[c * plane + k] = o[c][k];
        }
    }
}

}  // namespace gnr_ingest

using namespace gnr_ingest;

extern "C" {

const char* gnr_ingest_last_error(void) { return gnr_last_error(); }       // alias: the library has one error text

size_t gnr_ingest_tables_bytes(int dst_h, int dst_w) {
    if (dst_h < 1 || dst_w < 1 || dst_h > GNR_INGEST_MAX_DIM || dst_w > GNR_INGEST_MAX_DIM) return 0;
    return (table_words(dst_h, dst_w) + 256) * 4;
}

int gnr_ingest_tables_host(int src_h, int src_w, int dst_h, int dst_w, void* tables_host) {
    const Refuse no{"gnr_ingest_tables_host"};
    if (!tables_host) return no(GNR_ERR_ARG, "null pointer");
    if (src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || src_h > GNR_INGEST_MAX_DIM || src_w > GNR_INGEST_MAX_DIM ||
        dst_h > GNR_INGEST_MAX_DIM || dst_w > GNR_INGEST_MAX_DIM)
        return no(GNR_ERR_SHAPE, "every dimension must be in 1..16384");
    int* t = static_cast<int*>(tables_host);
    axis_table(dst_w, src_w, t, t + dst_w, t + 2 * dst_w, t + 3 * dst_w);
    int* ty = t + 4 * (size_t)dst_w;
    axis_table(dst_h, src_h, ty, ty + dst_h, ty + 2 * dst_h, ty + 3 * dst_h);
    float* lut = reinterpret_cast<float*>(t + table_words(dst_h, dst_w));
    for (int i = 0; i < 256; ++i) lut[i] = (float)i / 255.0f;              // host IEEE division: np.float32(i) / np.float32(255)
    return GNR_OK;
}

int gnr_ingest_u8(const unsigned char* frames, int n, int src_h, int src_w, int channels, size_t row_pitch, size_t frame_pitch,
                  const void* tables_dev, float* out, int dst_h, int dst_w, void* stream) {
    const Refuse no{"gnr_ingest_u8"};
    if (!frames || !tables_dev || !out) return no(GNR_ERR_ARG, "null pointer");
    if (channels != 3 && channels != 4) return no(GNR_ERR_ARG, "channels must be 3 or 4");
    if (n < 1 || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || src_h > GNR_INGEST_MAX_DIM || src_w > GNR_INGEST_MAX_DIM ||
        dst_h > GNR_INGEST_MAX_DIM || dst_w > GNR_INGEST_MAX_DIM)
        return no(GNR_ERR_SHAPE, "n >= 1 and every dimension in 1..16384");
    if (row_pitch < (size_t)src_w * (size_t)channels) return no(GNR_ERR_ARG, "row_pitch < src_w * channels");
    if (n > 1 && frame_pitch < (size_t)(src_h - 1) * row_pitch + (size_t)src_w * (size_t)channels)
        return no(GNR_ERR_ARG, "frame_pitch shorter than one frame");
    const unsigned groups = (unsigned)(dst_w + 3) / 4;
    const unsigned long long total = (unsigned long long)n * (unsigned)dst_h * groups;
    if (total > 0x7fffffffULL) return no(GNR_ERR_SHAPE, "too many output pixels for one launch");
    const int* tab = static_cast<const int*>(tables_dev);
    Args a{frames, tab, reinterpret_cast<const float*>(tab + table_words(dst_h, dst_w)), out, row_pitch, frame_pitch,
           src_h, src_w, channels, dst_h, dst_w, groups, (unsigned)total};
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    if (dst_w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) return launch<k_ingest_u8<true>>(nullptr, st, grid, dim3(256), 0, a);
    return launch<k_ingest_u8<false>>(nullptr, st, grid, dim3(256), 0, a);
}

}  // extern "C"
