// Image preprocessing on the device: Pillow's Image.resize(size, Image.BICUBIC) for 8-bit RGB, bit for bit, fused with the
// /255, -mean, /std normalisation of load_im_flexible (reference utils/datasets/preprocess.py:32-60).  No unit of its own:
// included from api.hip.
//
// Pillow resamples 8-bit images in integer arithmetic: per output coordinate a window [first, first + n) of input coordinates
// and n coefficients with 22 fractional bits; out = clip8((2^21 + sum pixel * k) >> 22) in int32; the horizontal pass first,
// into a uint8 intermediate image, then the vertical pass.  The windows and coefficients come from double arithmetic and are
// computed by the CALLER on the host (utils/datasets/preprocess.py: resize_tables); the device only multiplies, adds, shifts
// and clamps, so there is nothing to prove about its floating point.  The normalised value is looked up in the caller's
// [3,256] table, which is computed on the host as well (the same division on the GPU is a multiplication by a reciprocal).
//
// Two kernels, `batch` images of any sizes -> one output size per launch pair:
//   resize_rows_kernel   horizontal: [in_h, in_w, 3] -> intermediate [in_h, out_w, 3] with a 16-byte row pitch.  The 3-byte
//                        pixels are not dword-aligned, so a work-group stages the segment of `hr` input rows that its `xt`
//                        output columns read in LDS with aligned dword loads (all of them in flight at once), next to the
//                        columns' coefficients; one thread per output byte then reads bytes from LDS only.
//   resize_cols_kernel   vertical: channel-agnostic on byte columns, 12 bytes (4 pixels) per thread and tap = three dword
//                        loads from the pitched intermediate; a wave shares one output row, so its coefficients are
//                        wave-uniform.  Writes the uint8 HWC image and / or the normalised float32 CHW planes (16-byte
//                        stores) straight into the caller's batch slot.  An axis that keeps its size has no table: the
//                        vertical kernel then runs with the single coefficient 2^22 (exactly the identity), the horizontal
//                        one is not launched for that item and the vertical one reads the source.
#include "p2p_common.h"
#include <algorithm>
#include <cmath>

namespace p2p {

constexpr int RZ_THREADS = 256;
constexpr int RZ_GROUP = 64;                  // items per launch (descriptors travel as kernel arguments)
constexpr int RZ_LDS = 64 * 1024;             // dynamic LDS budget of the horizontal kernel
constexpr int RZ_XT_MAX = 128;                // output columns per work-group, at most
constexpr int RZ_HR_MAX = 8;                  // input rows per work-group, at most
constexpr int RZ_PRECISION = 22;
constexpr int RZ_MAX_SIDE = 16384;

struct RzItem {
    const unsigned char *src;                 // [in_h, in_w, 3]
    const int *tab_x, *tab_y;                 // bounds [out,2] then coefficients [out,ksize]; null = the axis keeps its size
    int in_h, in_w, kx, ky;
    int xt;                                   // output columns per work-group of the horizontal kernel
};

struct RzArgs {
    RzItem it[RZ_GROUP];
    unsigned char *mid;                       // intermediate images, mid_item bytes apart, rows mid_pitch bytes apart
    size_t mid_item;
    int mid_pitch;
    int out_h, out_w;
    int hr, span_cap;                         // horizontal kernel: rows per work-group, LDS bytes per staged row (multiple of 4)
    unsigned char *out_u8;                    // [B, out_h, out_w, 3] or null
    float *out_f;                             // item i at out_f + i * out_f_item: [3, out_h, out_w]; or null
    size_t out_f_item;
    const float *lut;                         // [3,256]
};

__device__ __forceinline__ unsigned char rz_clip8(int acc) {
    return (unsigned char)min(max(acc >> RZ_PRECISION, 0), 255);
}

__global__ __launch_bounds__(RZ_THREADS) void resize_rows_kernel(RzArgs a) {
    P2P_DYN_SHARED(unsigned char, rsm);
    const RzItem it = a.it[blockIdx.z];
    if (!it.tab_x) return;                                             // block-uniform: this item has no horizontal pass
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * it.xt, r0 = blockIdx.y * a.hr;
    if (x0 >= a.out_w || r0 >= it.in_h) return;
    const int nx = min(it.xt, a.out_w - x0), nr = min(a.hr, it.in_h - r0);
    const int *bounds = it.tab_x, *coef = it.tab_x + 2 * a.out_w;
    unsigned *lpix = (unsigned *)rsm;                                  // [hr][span_cap / 4]
    int *lk = (int *)(rsm + (size_t)a.hr * a.span_cap);                // [nx][kx]
    int *lb = lk + it.xt * it.kx;                                      // [nx][2]: first - p0, taps
    // the input pixels [p0, p1) this work-group's columns read (windows move right with the column)
    const int p0 = min(max(bounds[2 * x0], 0), it.in_w - 1);
    int p1 = bounds[2 * (x0 + nx - 1)] + bounds[2 * (x0 + nx - 1) + 1];
    p1 = min(min(max(p1, p0 + 1), it.in_w), p0 + (a.span_cap - 6) / 3);        // the last bound only matters for a malformed table
    const int cap_w = a.span_cap >> 2;
    const int nw = min((3 + (p1 - p0) * 3 + 3) >> 2, cap_w);           // dwords per row, whatever the row's alignment
    const unsigned char *src_end = it.src + (size_t)it.in_h * it.in_w * 3;
    for (int d = tid; d < nr * nw; d += RZ_THREADS) {
        const int r = d / nw, w = d - r * nw;
        const unsigned char *first = it.src + ((size_t)(r0 + r) * it.in_w + p0) * 3;
        const unsigned char *p = first - ((uintptr_t)first & 3) + 4 * w;       // aligned
        unsigned v;
        if (p >= it.src && p + 4 <= src_end) {
            v = *(const unsigned *)p;
        } else {                                                       // the dword straddles an end of the image: bytes
            v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (p + b >= it.src && p + b < src_end) v |= (unsigned)p[b] << (8 * b);
        }
        lpix[r * cap_w + w] = v;
    }
    for (int i = tid; i < nx * it.kx; i += RZ_THREADS) lk[i] = coef[(size_t)x0 * it.kx + i];
    for (int i = tid; i < nx; i += RZ_THREADS) {
        const int first = min(max(bounds[2 * (x0 + i)], p0), p1 - 1);
        lb[2 * i] = first - p0;
        lb[2 * i + 1] = min(min(max(bounds[2 * (x0 + i) + 1], 0), it.kx), p1 - first);
    }
    __syncthreads();
    unsigned char *mid = a.mid + (size_t)blockIdx.z * a.mid_item;
    const int rowb = nx * 3;
    for (int o = tid; o < nr * rowb; o += RZ_THREADS) {
        const int r = o / rowb, q = o - r * rowb, xo = q / 3, c = q - 3 * xo;
        const unsigned char *first = it.src + ((size_t)(r0 + r) * it.in_w + p0) * 3;
        const unsigned char *px = rsm + (size_t)r * a.span_cap + ((uintptr_t)first & 3) + lb[2 * xo] * 3 + c;
        const int n = lb[2 * xo + 1];
        const int *k = lk + xo * it.kx;
        int acc = 1 << (RZ_PRECISION - 1);
#pragma unroll 4
        for (int t = 0; t < n; ++t) acc += (int)px[3 * t] * k[t];
        mid[(size_t)(r0 + r) * a.mid_pitch + (size_t)x0 * 3 + q] = rz_clip8(acc);
    }
}

__global__ __launch_bounds__(RZ_THREADS) void resize_cols_kernel(RzArgs a) {
    __shared__ float slut[768];
    const int tid = threadIdx.x;
    if (a.out_f)
        for (int i = tid; i < 768; i += RZ_THREADS) slut[i] = a.lut[i];
    __syncthreads();
    const RzItem it = a.it[blockIdx.z];
    const int yy = blockIdx.y * (RZ_THREADS / 64) + __builtin_amdgcn_readfirstlane(tid >> 6);     // one output row per wave
    const int g = blockIdx.x * 64 + (tid & 63);                        // group of 4 pixels = 12 byte columns
    const int rowb = a.out_w * 3, j0 = 12 * g;
    if (yy >= a.out_h || j0 >= rowb) return;
    const unsigned char *base = it.src;
    size_t pitch = (size_t)it.in_w * 3;
    if (it.tab_x) {
        base = a.mid + (size_t)blockIdx.z * a.mid_item;
        pitch = (size_t)a.mid_pitch;
    }
    int first = yy, n = 1;
    const int *k = nullptr;
    if (it.tab_y) {
        first = min(max(it.tab_y[2 * yy], 0), it.in_h - 1);
        n = min(min(max(it.tab_y[2 * yy + 1], 0), it.ky), it.in_h - first);
        k = it.tab_y + 2 * a.out_h + (size_t)yy * it.ky;
    }
    const int nb = min(12, rowb - j0);
    int acc[12];
#pragma unroll
    for (int b = 0; b < 12; ++b) acc[b] = 1 << (RZ_PRECISION - 1);
    const unsigned char *p = base + (size_t)first * pitch + j0;
    if (nb == 12 && ((uintptr_t)p & 3) == 0 && (pitch & 3) == 0) {
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const unsigned *q = (const unsigned *)(p + (size_t)t * pitch);
            const unsigned v0 = q[0], v1 = q[1], v2 = q[2];
            const int kt = k ? k[t] : (1 << RZ_PRECISION);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                acc[b] += (int)((v0 >> (8 * b)) & 255u) * kt;
                acc[4 + b] += (int)((v1 >> (8 * b)) & 255u) * kt;
                acc[8 + b] += (int)((v2 >> (8 * b)) & 255u) * kt;
            }
        }
    } else {
        for (int t = 0; t < n; ++t) {
            const unsigned char *q = p + (size_t)t * pitch;
            const int kt = k ? k[t] : (1 << RZ_PRECISION);
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (b < nb) acc[b] += (int)q[b] * kt;
        }
    }
    unsigned char v[12];
#pragma unroll
    for (int b = 0; b < 12; ++b) v[b] = rz_clip8(acc[b]);
    if (a.out_u8) {
        unsigned char *o = a.out_u8 + ((size_t)blockIdx.z * a.out_h + yy) * rowb + j0;
        if (nb == 12 && ((uintptr_t)o & 3) == 0) {
#pragma unroll
            for (int w = 0; w < 3; ++w)
                ((unsigned *)o)[w] = (unsigned)v[4 * w] | ((unsigned)v[4 * w + 1] << 8) | ((unsigned)v[4 * w + 2] << 16) |
                                     ((unsigned)v[4 * w + 3] << 24);
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (b < nb) o[b] = v[b];
        }
    }
    if (a.out_f) {
        const size_t plane = (size_t)a.out_h * a.out_w;
        float *o = a.out_f + (size_t)blockIdx.z * a.out_f_item + (size_t)yy * a.out_w + 4 * g;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float *oc = o + c * plane;
            if (nb == 12 && ((uintptr_t)oc & 15) == 0) {
                f32x4 f;
#pragma unroll
                for (int i = 0; i < 4; ++i) f[i] = slut[c * 256 + v[3 * i + c]];
                *(f32x4 *)oc = f;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (3 * i + c < nb) oc[i] = slut[c * 256 + v[3 * i + c]];
            }
        }
    }
}

// Taps per output coordinate: the same double operations as Pillow's precompute_coeffs (and as resize_tables on the Python side).
static int rz_ksize(int in_size, int out_size) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(2.0 * filterscale) * 2 + 1;
}

// LDS bytes per staged row for xt output columns: the columns' windows span at most xt * scale + the window of one column
static int rz_span_bytes(int in_size, int out_size, int ksize, int xt) {
    const int px = (int)ceil((double)xt * in_size / out_size) + ksize + 2;
    return ((px * 3 + 6) + 3) & ~3;
}

static int rz_mid_pitch(int out_w) { return (out_w * 3 + 15) & ~15; }

}  // namespace p2p

extern "C" size_t p2p_resize_workspace_bytes(int batch, int max_in_h, int max_in_w, int out_h, int out_w) {
    using namespace p2p;
    if (batch < 1 || max_in_h < 1 || max_in_w < 1 || out_h < 1 || out_w < 1) return 0;
    if (max_in_h > RZ_MAX_SIDE || max_in_w > RZ_MAX_SIDE || out_h > RZ_MAX_SIDE || out_w > RZ_MAX_SIDE) return 0;
    return (size_t)batch * max_in_h * rz_mid_pitch(out_w);
}

extern "C" int p2p_resize_bicubic_batch(const p2p_resize_item *items, int batch, int out_h, int out_w, uint8_t *out_u8,
                                        float *out_f32, size_t out_f32_stride, const float *lut, void *workspace,
                                        size_t workspace_bytes, p2p_stream_t stream) {
    using namespace p2p;
    P2P_REQUIRE(items && (out_u8 || out_f32), P2P_EINVAL, "p2p_resize_bicubic_batch: null argument (items, or both outputs)");
    P2P_REQUIRE(!out_f32 || lut, P2P_EINVAL, "p2p_resize_bicubic_batch: null lut with a float32 output");
    P2P_REQUIRE(batch >= 1 && out_h >= 1 && out_w >= 1, P2P_EINVAL, "p2p_resize_bicubic_batch: bad sizes (batch %d, output %d x %d)",
                batch, out_h, out_w);
    P2P_REQUIRE(out_h <= RZ_MAX_SIDE && out_w <= RZ_MAX_SIDE, P2P_EUNSUPPORTED,
                "p2p_resize_bicubic_batch: output %d x %d (sides up to %d)", out_h, out_w, RZ_MAX_SIDE);
    P2P_REQUIRE(!out_f32 || out_f32_stride >= (size_t)3 * out_h * out_w, P2P_EINVAL,
                "p2p_resize_bicubic_batch: out_f32_stride %zu below one item (%zu floats)", out_f32_stride, (size_t)3 * out_h * out_w);
    int max_h = 0, max_w = 0;
    bool any_x = false;
    for (int i = 0; i < batch; ++i) {
        const p2p_resize_item &s = items[i];
        P2P_REQUIRE(s.pixels, P2P_EINVAL, "p2p_resize_bicubic_batch: item %d: null pixels", i);
        P2P_REQUIRE(s.in_h >= 1 && s.in_w >= 1, P2P_EINVAL, "p2p_resize_bicubic_batch: item %d: bad size %d x %d", i, s.in_h, s.in_w);
        P2P_REQUIRE(s.in_h <= RZ_MAX_SIDE && s.in_w <= RZ_MAX_SIDE, P2P_EUNSUPPORTED,
                    "p2p_resize_bicubic_batch: item %d: %d x %d (sides up to %d)", i, s.in_h, s.in_w, RZ_MAX_SIDE);
        P2P_REQUIRE((s.in_w == out_w) == (s.table_x == nullptr) && (s.in_h == out_h) == (s.table_y == nullptr), P2P_EINVAL,
                    "p2p_resize_bicubic_batch: item %d: an axis has a table exactly when its size changes (null table otherwise)", i);
        P2P_REQUIRE((!s.table_x || s.ksize_x == rz_ksize(s.in_w, out_w)) && (!s.table_y || s.ksize_y == rz_ksize(s.in_h, out_h)),
                    P2P_EINVAL, "p2p_resize_bicubic_batch: item %d: ksize (%d, %d) does not belong to these sizes (%d, %d)", i,
                    s.ksize_x, s.ksize_y, s.table_x ? rz_ksize(s.in_w, out_w) : 0, s.table_y ? rz_ksize(s.in_h, out_h) : 0);
        if (s.table_x) {
            const int kx = rz_ksize(s.in_w, out_w);
            P2P_REQUIRE(kx * 4 + 8 + rz_span_bytes(s.in_w, out_w, kx, 1) <= RZ_LDS, P2P_EUNSUPPORTED,
                        "p2p_resize_bicubic_batch: item %d: width %d -> %d needs %d taps per pixel (too many for one work-group)", i,
                        s.in_w, out_w, kx);
            any_x = true;
        }
        max_h = std::max(max_h, s.in_h);
        max_w = std::max(max_w, s.in_w);
    }
    const size_t need = p2p_resize_workspace_bytes(batch, max_h, max_w, out_h, out_w);
    P2P_REQUIRE(!any_x || (workspace && workspace_bytes >= need), P2P_ENOMEM,
                "p2p_resize_bicubic_batch: workspace of %zu bytes needed (p2p_resize_workspace_bytes), got %zu", need,
                workspace ? workspace_bytes : (size_t)0);
    P2P_REQUIRE(!any_x || ((uintptr_t)workspace & 15) == 0, P2P_EINVAL, "p2p_resize_bicubic_batch: workspace must be 16-byte aligned");
    const size_t mid_item = (size_t)max_h * rz_mid_pitch(out_w);
    for (int b0 = 0; b0 < batch; b0 += RZ_GROUP) {
        const int nb = std::min(RZ_GROUP, batch - b0);
        RzArgs a{};
        a.mid = (unsigned char *)workspace + (size_t)b0 * mid_item;
        a.mid_item = mid_item;
        a.mid_pitch = rz_mid_pitch(out_w);
        a.out_h = out_h;
        a.out_w = out_w;
        a.out_u8 = out_u8 ? out_u8 + (size_t)b0 * out_h * out_w * 3 : nullptr;
        a.out_f = out_f32 ? out_f32 + (size_t)b0 * out_f32_stride : nullptr;
        a.out_f_item = out_f32_stride;
        a.lut = lut;
        int span_cap = 0, coef_cap = 0, grid_x = 0, grid_rows = 0;
        for (int i = 0; i < nb; ++i) {
            const p2p_resize_item &s = items[b0 + i];
            RzItem &it = a.it[i];
            it.src = s.pixels;
            it.tab_x = s.table_x;
            it.tab_y = s.table_y;
            it.in_h = s.in_h;
            it.in_w = s.in_w;
            it.kx = s.table_x ? s.ksize_x : 0;
            it.ky = s.table_y ? s.ksize_y : 0;
            it.xt = 1;
            if (!s.table_x) continue;
            // the most columns per work-group whose coefficients and one staged row take at most half the LDS budget together
            int xt = RZ_XT_MAX;
            while (xt > 1 && xt * (it.kx * 4 + 8) + rz_span_bytes(s.in_w, out_w, it.kx, xt) > RZ_LDS / 2) xt >>= 1;
            it.xt = xt;
            span_cap = std::max(span_cap, rz_span_bytes(s.in_w, out_w, it.kx, xt));
            coef_cap = std::max(coef_cap, xt * (it.kx * 4 + 8));
            grid_x = std::max(grid_x, ceil_div(out_w, xt));
            grid_rows = std::max(grid_rows, s.in_h);
        }
        if (grid_x) {
            // span_cap and coef_cap may come from different items: each is at most RZ_LDS - 8 - (the other's value at xt = 1),
            // and one row always fits beside the coefficients (checked above per item, and xt only shrinks towards 1)
            int hr = std::min(RZ_HR_MAX, (RZ_LDS - coef_cap) / span_cap);
            P2P_REQUIRE(hr >= 1, P2P_EUNSUPPORTED, "p2p_resize_bicubic_batch: the widths of this batch do not fit one launch; split it");
            a.hr = hr;
            a.span_cap = span_cap;
            const size_t lds = (size_t)hr * span_cap + coef_cap;
            hipLaunchKernelGGL(resize_rows_kernel, dim3(grid_x, ceil_div(grid_rows, hr), nb), dim3(RZ_THREADS), lds,
                               (hipStream_t)stream, a);
            const int st = check_launch("resize_rows_kernel");
            if (st != P2P_OK) return st;
        }
        hipLaunchKernelGGL(resize_cols_kernel, dim3(ceil_div(ceil_div(out_w, 4), 64), ceil_div(out_h, RZ_THREADS / 64), nb),
                           dim3(RZ_THREADS), 0, (hipStream_t)stream, a);
        const int st = check_launch("resize_cols_kernel");
        if (st != P2P_OK) return st;
    }
    return P2P_OK;
}
