// The matching operators of the reference as entry points of their own (networks/modules.py, networks/ncn/model.py), for callers
// that build their own coarse stage from the pieces: the plain feature correlation, the 4-D max-pool of a caller's volume, the
// per-position L2 normalisation, and the key reset of a stand-alone mutual matching (whose maxima and apply kernels are the coarse
// stage's, coarse.hip section 3).  A stand-alone Conv4d layer is the PLANAR form of the generic consensus kernel
// (consensus_generic.hip).  Every kernel takes the batch item from blockIdx.z and sums in an order its sizes alone fix: an item's
// result is bit-identical alone and in any batch.  Device code is restricted to what the kernel emulator of the test-suite runs.
// Compiled as part of coarse.hip.
#pragma once
#include "coarse_common.h"

namespace p2p {

// ------------------------------------------------------------------------------------------------
// FeatCorrelation (modules.py:41-53): out[pa][pb] = sum_c A[c][pa] * B[c][pb], no normalisation
// ------------------------------------------------------------------------------------------------
// Exact fp32 on v_mfma_f32_16x16x4_f32: a wave owns 16 A positions x 64 B positions (four accumulators share the A operand), a
// work-group 64 x 64; K = the channels in ascending order, four per MFMA (lane (l15, kb) supplies channel 4 s + kb).  Channels
// past the last one are zeros; positions past the last one multiply a clamped copy and are not stored.
__global__ __launch_bounds__(256) void correlation_kernel(CorrelationArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, kb = lane >> 4;
    const float *A = a.A + blockIdx.z * a.sA, *B = a.B + blockIdx.z * a.sB;
    float *out = a.out + blockIdx.z * a.sOut;
    const int r0 = ((int)blockIdx.y * 4 + wave) * 16, c0 = (int)blockIdx.x * 64;
    const int ra = min(r0 + l15, a.nA - 1);
    int cb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cb[j] = min(c0 + 16 * j + l15, a.nB - 1);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nsteps = (a.C + 3) >> 2;
    for (int s = 0; s < nsteps; ++s) {
        const int c = 4 * s + kb;
        const bool ok = c < a.C;
        const size_t cc = (size_t)(ok ? c : a.C - 1);
        const float av = A[cc * a.nA + ra];
        float bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = B[cc * a.nB + cb[j]];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? av : 0.f, ok ? bv[j] : 0.f, acc[j], 0, 0, 0);
    }
    // accumulator register r = A position r0 + 4 kb + r, column l15 = B position c0 + 16 j + l15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * kb + r;
        if (row >= a.nA) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = c0 + 16 * j + l15;
            if (col < a.nB) out[(size_t)row * a.nB + col] = acc[j][r];
        }
    }
}

void launch_correlation(const CorrelationArgs &a, int batch, hipStream_t stream) {
    hipLaunchKernelGGL(correlation_kernel, dim3(ceil_div(a.nB, 64), ceil_div(a.nA, 64), batch), dim3(256), 0, stream, a);
}

// ------------------------------------------------------------------------------------------------
// maxpool4d (modules.py:11-34) of a caller's volume: one thread per pooled cell
// ------------------------------------------------------------------------------------------------
// The k^4 values of a window in the reference's slice order (i, j, k, l); the first maximum wins, as in torch.max over the
// concatenated slices; a NaN beats every number.  code: s = ((i k + j) k + k') k + l (optional).
__global__ __launch_bounds__(256) void maxpool4d_kernel(MaxPool4dArgs a) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= a.cells) return;
    const float *x = a.x + blockIdx.z * a.cells * (size_t)(a.k * a.k * a.k * a.k);
    size_t g = o;
    const int d = (int)(g % a.p3); g /= a.p3;
    const int c = (int)(g % a.p2); g /= a.p2;
    const int b = (int)(g % a.p1);
    const int aa = (int)(g / a.p1);
    const int k = a.k;
    const size_t W1 = (size_t)a.p1 * k, H2 = (size_t)a.p2 * k, W2 = (size_t)a.p3 * k;
    float best = -INFINITY;
    int code = 0, s = 0;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j)
            for (int kk = 0; kk < k; ++kk) {
                const float *row = x + ((((size_t)aa * k + i) * W1 + (size_t)b * k + j) * H2 + (size_t)c * k + kk) * W2 + (size_t)d * k;
                for (int l = 0; l < k; ++l, ++s) {
                    const float v = row[l];
                    if (s == 0 || v > best || (v != v && best == best)) { best = v; code = s; }      // the first NaN wins, as in torch.max
                }
            }
    a.pooled[blockIdx.z * a.cells + o] = best;
    if (a.code) a.code[blockIdx.z * a.cells + o] = (uint8_t)code;
}

void launch_maxpool4d(const MaxPool4dArgs &a, int batch, hipStream_t stream) {
    hipLaunchKernelGGL(maxpool4d_kernel, dim3((unsigned)((a.cells + 255) / 256), 1, batch), dim3(256), 0, stream, a);
}

// ------------------------------------------------------------------------------------------------
// L2Normalize (modules.py:6): y = x / sqrt(sum_C x^2 + 1e-6) over the middle axis of [outer][C][inner]
// ------------------------------------------------------------------------------------------------
// One thread per (outer, inner) position: the squares are added in ascending channel order (one fma each), then every channel is
// divided by the root (IEEE division and square root).
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float *__restrict__ x, size_t positions, int C, size_t inner,
                                                           float *__restrict__ y) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= positions) return;
    const size_t o = p / inner, i = p - o * inner;
    const float *xp = x + o * C * inner + i;
    float *yp = y + o * C * inner + i;
    float ss = 0.f;
    for (int c = 0; c < C; ++c) {
        const float v = xp[(size_t)c * inner];
        ss = fmaf(v, v, ss);
    }
    const float norm = sqrtf(ss + 1e-6f);
    for (int c = 0; c < C; ++c) yp[(size_t)c * inner] = xp[(size_t)c * inner] / norm;
}

void launch_l2_normalize(const float *x, size_t outer, int C, size_t inner, float *y, hipStream_t stream) {
    const size_t positions = outer * inner;
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)((positions + 255) / 256)), dim3(256), 0, stream, x, positions, C, inner, y);
}

// ------------------------------------------------------------------------------------------------
// MutualMatching (ncn/model.py:157-176) on a caller's volume: reset of the maxima keys (maxima_kernel raises the column keys
// with atomicMax), then launch_maxima and launch_mm_apply of the coarse stage
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reset_keys_kernel(int *keys, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = KEY_NEG_INF;
}

void launch_mutual_matching(const float *x, int nA, int nB, float *y, int *keys, size_t sKeys, int batch, hipStream_t stream) {
    const size_t n = sKeys * batch, nel = (size_t)nA * nB;
    int *rkey = keys, *ckey = keys + ((nA + 3) & ~3);
    hipLaunchKernelGGL(reset_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, keys, n);
    launch_maxima(x, nA, nB, rkey, ckey, nel, sKeys, nullptr, (unsigned)batch, stream);
    launch_mm_apply(x, nA, nB, rkey, ckey, y, nel, sKeys, nel, nullptr, nullptr, (size_t)batch, stream);
}

}  // namespace p2p
