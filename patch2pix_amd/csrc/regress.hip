// Fine stage of the Patch2Pix matching path on gfx950: one workgroup per proposal runs
//   patch gather (4 pyramid levels, both images) -> per-pixel L2 normalisation ->
//   conv 3x3 s2 (518->512) -> BN -> conv 3x3 s1 (512->512) -> BN -> ReLU -> 8x8 max ->
//   FC 512 -> 512 -> 256 -> 5 -> tanh/sigmoid parse -> clamp
// and, when a second regressor is given, feeds its own result through that one as well.
//
// Reference semantics: networks/utils.py:4-36 (gather), networks/patch2pix.py:157-184 (mini batch),
// networks/modules.py:56-112 (FeatRegressNet), networks/patch2pix.py:138-155 (parse).
//
// Mapping to CDNA4
//   * a proposal is a 64-row (8x8 output pixels) implicit GEMM against 512 output channels; the
//     8 waves of the workgroup each own 64 output channels (2x2 tiles of v_mfma_f32_32x32x2_f32),
//     so the 16x16x259x2 patch is never written to HBM and the 512x8x8 intermediate lives in LDS;
//   * the A operand comes from LDS: the patch is stored *deduplicated* (levels 1-3 are nearest
//     neighbour up-samplings, so a 16x16 window only touches 9x9 / 5x5 / 3x3 distinct cells) and
//     the per-pixel L2 scale is applied when the fragment is read;
//   * the B operand (weights) is streamed straight from L2 into VGPRs in a layout packed at load
//     time in exact consumption order: one global_load_dwordx4 per lane feeds four k-steps;
//   * fp32 MFMA is bit-identical to an fma chain, so results match an fp32 CPU evaluation to
//     round-off of the (fixed, documented) summation order: taps outer, channels inner.
// This file: the kernel, its weight packer and its launcher (the handle and the C ABI: regress_api.hip).
#include "regress_common.h"

namespace p2p {

// LDS carve-up (floats)
constexpr int TILE_L0 = 0, TILE_L1 = 768, TILE_L2 = 5952, TILE_L3 = 7552, TILE_IMG = 8704;
constexpr int HSTRIDE = 68;                       // row stride of the conv1 output H[c][64 px]
constexpr int LDS_UNION = 512 * HSTRIDE;          // max(2*TILE_IMG, 512*HSTRIDE)
constexpr int LDS_SCALE = LDS_UNION;              // [2][256] per-pixel 1/||f||
constexpr int LDS_V = LDS_SCALE + 512;            // [512] pooled conv features
constexpr int LDS_F1 = LDS_V + 512;               // [512]
constexpr int LDS_F2 = LDS_F1 + 512;              // [256]
constexpr int LDS_MISC = LDS_F2 + 256;            // [16] raw outputs / current proposal
constexpr int LDS_FLOATS = LDS_MISC + 16;
constexpr size_t LDS_BYTES = size_t(LDS_FLOATS) * 4;

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// One chunk = 8 K values = 4 k-steps for both m-tiles and both n-tiles (16 MFMAs).
#define P2P_CHUNK_MFMA(A0, A1)                                   \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {              \
        acc00 = MFMA(A0[q], b0[q], acc00);                       \
        acc01 = MFMA(A0[q], b1[q], acc01);                       \
        acc10 = MFMA(A1[q], b0[q], acc10);                       \
        acc11 = MFMA(A1[q], b1[q], acc11);                       \
    }

__global__ __launch_bounds__(NT, 2) void regress_kernel(RegressArgs args) {
    P2P_DYN_SHARED(float, smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const int prop = blockIdx.x;
    int it = 0;
    while (it + 1 < args.nitems && prop >= args.start[it + 1]) ++it;
    if (args.dev_counts && prop - args.start[it] >= args.dev_counts[it]) return;      // empty slot (whole work-group)
    const ItemDev &I = args.item[it];

    float *tiles = smem;
    float *Hbuf = smem;
    float *scale = smem + LDS_SCALE;
    float *V = smem + LDS_V;
    float *F1 = smem + LDS_F1;
    float *F2 = smem + LDS_F2;
    float *misc = smem + LDS_MISC;

    // current proposal (float coordinates; exact for the int64 coarse matches)
    if (tid < 4) {
        float v;
        if (args.is_float) v = ((const float *)args.proposals)[prop * 4 + tid];
        else v = (float)((const long long *)args.proposals)[prop * 4 + tid];
        misc[8 + tid] = v;
    }
    __syncthreads();

    for (int lvl = 0; lvl < args.nlevels; ++lvl) {
        const RegDev &R = args.reg[lvl];
        // ---------------------------------------------------------------- proposal geometry
        // x, y = trunc(match) (networks/utils.py:19); window origin = centre - 8 (:8-15)
        int x0[2], y0[2];
        x0[0] = (int)misc[8 + 0] - 8; y0[0] = (int)misc[8 + 1] - 8;
        x0[1] = (int)misc[8 + 2] - 8; y0[1] = (int)misc[8 + 3] - 8;
        __syncthreads();   // everyone has read misc / finished with the previous level's LDS

        // ---------------------------------------------------------------- gather (dedup tiles)
        for (int img = 0; img < 2; ++img) {
            const int Hh = I.H[img], Ww = I.W[img];
            float *t = tiles + img * TILE_IMG;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int Rr = (j == 0) ? 16 : (j == 1) ? 9 : (j == 2) ? 5 : 3;
                const int Cc = (j == 0) ? 3 : (j == 3) ? 128 : 64;
                const int off = (j == 0) ? TILE_L0 : (j == 1) ? TILE_L1 : (j == 2) ? TILE_L2 : TILE_L3;
                const int Hj = Hh >> j, Wj = Ww >> j;                 // index clamp: dim // ds (networks/utils.py:22-23)
                    const int Ha = level_dim(Hh, j), Wa = level_dim(Ww, j);  // extent of the backbone's map
                const int r0 = clampi(y0[img] >> j, 0, Hj - 1);
                const int c0 = clampi(x0[img] >> j, 0, Wj - 1);
                const float *src = I.pyr[img][j];
                for (int e = tid; e < Cc * Rr * Rr; e += NT) {
                    const int c = e / (Rr * Rr);
                    const int rem = e - c * (Rr * Rr);
                    const int r = rem / Rr;
                    const int cc = rem - r * Rr;
                    const int sy = min(r0 + r, Hj - 1);
                    const int sx = min(c0 + cc, Wj - 1);
                    t[off + e] = src[((size_t)c * Ha + sy) * Wa + sx];
                }
            }
        }
        __syncthreads();

        // ---------------------------------------------------------------- per-pixel L2 scale
        {
            const int img = tid >> 8, pix = tid & 255, py = pix >> 4, px = pix & 15;
            const float *t = tiles + img * TILE_IMG;
            float ss = 0.f;
            {
                const float *p = t + TILE_L0 + patch_cell(y0[img], py, 0, I.H[img]) * 16 + patch_cell(x0[img], px, 0, I.W[img]);
#pragma unroll
                for (int c = 0; c < 3; ++c) { float v = p[c * 256]; ss = fmaf(v, v, ss); }
            }
#pragma unroll
            for (int j = 1; j < 4; ++j) {
                const int Rr = (j == 1) ? 9 : (j == 2) ? 5 : 3;
                const int Cc = (j == 3) ? 128 : 64;
                const int off = (j == 1) ? TILE_L1 : (j == 2) ? TILE_L2 : TILE_L3;
                const float *p = t + off + patch_cell(y0[img], py, j, I.H[img]) * Rr + patch_cell(x0[img], px, j, I.W[img]);
                for (int c = 0; c < Cc; ++c) { float v = p[c * Rr * Rr]; ss = fmaf(v, v, ss); }
            }
            scale[tid] = 1.0f / sqrtf(ss + 1e-6f);
        }
        __syncthreads();

        // ---------------------------------------------------------------- conv1: 3x3, stride 2, pad 1
        f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
        {
            // weight stream: b* = current chunk, c* = next chunk, the loads issued below are two ahead
            const f32x4 *bp = (const f32x4 *)R.wp1 + (size_t)wave * (K1_CHUNKS + PF) * 128 + lane;
            f32x4 b0 = bp[0], b1 = bp[64], c0 = bp[128], c1 = bp[192];
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - ky * 3;
                // per-lane source pixel of both m-tiles for this tap
                int pyc[2], pxc[2];
                bool ok[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int p = 32 * t + l31;
                    const int py = 2 * (p >> 3) + ky - 1, px = 2 * (p & 7) + kx - 1;
                    ok[t] = (py >= 0) && (px >= 0);
                    pyc[t] = max(py, 0);
                    pxc[t] = max(px, 0);
                }
                float a0[4], a1[4];
                // --- chunk 0: level 0 of both images; k = 2q+half -> (img0 c0,c1,c2, img1 c0,c1,c2, 0, 0)
                {
                    f32x4 n0 = bp[256], n1 = bp[320];
                    bp += 128;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int pofs = pyc[t] * 16 + pxc[t];
                        const float s0 = ok[t] ? scale[pofs] : 0.f;
                        const float s1 = ok[t] ? scale[256 + pofs] : 0.f;
                        const float *t0 = tiles + TILE_L0 + patch_cell(y0[0], pyc[t], 0, I.H[0]) * 16 +
                                          patch_cell(x0[0], pxc[t], 0, I.W[0]);
                        const float *t1 = tiles + TILE_IMG + TILE_L0 + patch_cell(y0[1], pyc[t], 0, I.H[1]) * 16 +
                                          patch_cell(x0[1], pxc[t], 0, I.W[1]);
                        float v0 = t0[half * 256] * s0;                                   // img0 c0 | c1
                        float v1 = half ? t1[0] * s1 : t0[512] * s0;                      // img0 c2 | img1 c0
                        float v2 = t1[(1 + half) * 256] * s1;                             // img1 c1 | c2
                        if (t == 0) { a0[0] = v0; a0[1] = v1; a0[2] = v2; a0[3] = 0.f; }
                        else        { a1[0] = v0; a1[1] = v1; a1[2] = v2; a1[3] = 0.f; }
                    }
                    P2P_CHUNK_MFMA(a0, a1)
                    b0 = c0; b1 = c1; c0 = n0; c1 = n1;
                }
                // --- chunks 1..64: (img, level 1..3) segments, 8 channels per chunk
                for (int img = 0; img < 2; ++img) {
                    const float s0 = ok[0] ? scale[img * 256 + pyc[0] * 16 + pxc[0]] : 0.f;
                    const float s1 = ok[1] ? scale[img * 256 + pyc[1] * 16 + pxc[1]] : 0.f;
#pragma unroll
                    for (int j = 1; j < 4; ++j) {
                        const int Rr = (j == 1) ? 9 : (j == 2) ? 5 : 3;
                        const int CS = Rr * Rr;
                        const int nchunk = (j == 3) ? 16 : 8;
                        const int off = (j == 1) ? TILE_L1 : (j == 2) ? TILE_L2 : TILE_L3;
                        const float *base = tiles + img * TILE_IMG + off + half * CS;
                        const float *p0 = base + patch_cell(y0[img], pyc[0], j, I.H[img]) * Rr +
                                          patch_cell(x0[img], pxc[0], j, I.W[img]);
                        const float *p1 = base + patch_cell(y0[img], pyc[1], j, I.H[img]) * Rr +
                                          patch_cell(x0[img], pxc[1], j, I.W[img]);
#pragma unroll
                        for (int q = 0; q < 4; ++q) { a0[q] = p0[2 * q * CS] * s0; a1[q] = p1[2 * q * CS] * s1; }
                        for (int ch = 0; ch < nchunk; ++ch) {
                            f32x4 n0 = bp[256], n1 = bp[320];
                            bp += 128;
                            // A fragments of the next chunk (re-reads the last one at the segment end)
                            const int chn = min(ch + 1, nchunk - 1);
                            float an0[4], an1[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                an0[q] = p0[(chn * 8 + 2 * q) * CS];
                                an1[q] = p1[(chn * 8 + 2 * q) * CS];
                            }
                            P2P_CHUNK_MFMA(a0, a1)
#pragma unroll
                            for (int q = 0; q < 4; ++q) { a0[q] = an0[q] * s0; a1[q] = an1[q] * s1; }
                            b0 = c0; b1 = c1; c0 = n0; c1 = n1;
                        }
                    }
                }
            }
        }
        __syncthreads();   // all waves are done reading the patch tiles

        // BN1 (folded scale/shift) and spill H[c][px] to LDS for conv2's A operand
        {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = wave * 64 + u * 32 + l31;
                const float s = R.bn1s[n], b = R.bn1b[n];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const f32x16 &a = (t == 0) ? (u == 0 ? acc00 : acc01) : (u == 0 ? acc10 : acc11);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 v;
                        v[0] = fmaf(a[4 * g + 0], s, b);
                        v[1] = fmaf(a[4 * g + 1], s, b);
                        v[2] = fmaf(a[4 * g + 2], s, b);
                        v[3] = fmaf(a[4 * g + 3], s, b);
                        *(f32x4 *)(Hbuf + n * HSTRIDE + 32 * t + 8 * g + 4 * half) = v;
                    }
                }
            }
        }
        __syncthreads();

        // ---------------------------------------------------------------- conv2: 3x3, stride 1, pad 1
        acc00 = (f32x16){0}; acc01 = (f32x16){0}; acc10 = (f32x16){0}; acc11 = (f32x16){0};
        {
            const f32x4 *bp = (const f32x4 *)R.wp2 + (size_t)wave * (K2_CHUNKS + PF) * 128 + lane;
            f32x4 b0 = bp[0], b1 = bp[64], c0 = bp[128], c1 = bp[192];
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - ky * 3;
                const float *p0, *p1;
                float m0, m1;
                {
                    const int oy = (l31 >> 3) + ky - 1, ox = (l31 & 7) + kx - 1;
                    const bool okx = (ox >= 0) && (ox < 8);
                    const bool ok0 = okx && (oy >= 0);                 // m-tile 0: rows 0..3 (+ky-1 <= 4)
                    const bool ok1 = okx && (oy + 4 < 8);              // m-tile 1: rows 4..7 (+ky-1 >= 3)
                    m0 = ok0 ? 1.f : 0.f;
                    m1 = ok1 ? 1.f : 0.f;
                    p0 = Hbuf + half * HSTRIDE + (ok0 ? oy * 8 + ox : 0);
                    p1 = Hbuf + half * HSTRIDE + (ok1 ? (oy + 4) * 8 + ox : 0);
                }
                float a0[4], a1[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { a0[q] = p0[2 * q * HSTRIDE] * m0; a1[q] = p1[2 * q * HSTRIDE] * m1; }
                for (int ch = 0; ch < K2_CHUNKS_PER_TAP; ++ch) {
                    f32x4 n0 = bp[256], n1 = bp[320];
                    bp += 128;
                    const int chn = min(ch + 1, K2_CHUNKS_PER_TAP - 1);
                    float an0[4], an1[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        an0[q] = p0[(chn * 8 + 2 * q) * HSTRIDE];
                        an1[q] = p1[(chn * 8 + 2 * q) * HSTRIDE];
                    }
                    P2P_CHUNK_MFMA(a0, a1)
#pragma unroll
                    for (int q = 0; q < 4; ++q) { a0[q] = an0[q] * m0; a1[q] = an1[q] * m1; }
                    b0 = c0; b1 = c1; c0 = n0; c1 = n1;
                }
            }
        }

        // BN2 -> ReLU -> max over the 8x8 outputs (BN before max: its scale may be negative)
        {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = wave * 64 + u * 32 + l31;
                const float s = R.bn2s[n], b = R.bn2b[n];
                const f32x16 &aa = (u == 0) ? acc00 : acc01;
                const f32x16 &ab = (u == 0) ? acc10 : acc11;
                float m = 0.f;                                  // ReLU folded into the max
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    m = fmaxf(m, fmaf(aa[r], s, b));
                    m = fmaxf(m, fmaf(ab[r], s, b));
                }
                m = fmaxf(m, __shfl_xor(m, 32));
                if (half == 0) V[n] = m;
            }
        }
        __syncthreads();

        // ---------------------------------------------------------------- FC tail + parse
        fc_tail_parse(R, I, args, lvl, prop, tid, V, F1, F2, misc);
    }
}

// ---- host side: the weight streams and the launch ------------------------------------------------

// channel (0..517) of the concatenated [im1 259 | im2 259] regressor input for conv1 K index r (0..519)
// inside one tap; -1 for the two padding slots.
static int conv1_channel_of(int r) {
    if (r < 8) {
        if (r >= 6) return -1;
        return (r / 3) * 259 + (r % 3);
    }
    const int img = (r - 8) / 256, cc = (r - 8) % 256;
    return img * 259 + 3 + cc;
}

// wp1 [WP1_FLOATS], wp2 [WP2_FLOATS]: the PF chunks behind every wave's stream are not written (the caller zeroes them)
void pack_f32_weights(const float *conv1_w, const float *conv2_w, float *wp1, float *wp2) {
    // conv1: Wp1[w][kc][u][lane][q] = W1[n = 64w+32u+(lane&31)][channel(kidx)][tap],
    //        kidx = 8*(kc % 65) + 2q + (lane>>5), tap = kc / 65
    for (int w = 0; w < 8; ++w)
        for (int kc = 0; kc < K1_CHUNKS; ++kc) {
            const int tap = kc / K1_CHUNKS_PER_TAP, kin = kc % K1_CHUNKS_PER_TAP;
            for (int u = 0; u < 2; ++u)
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < 4; ++q) {
                        const int n = 64 * w + 32 * u + (lane & 31);
                        const int ch = conv1_channel_of(8 * kin + 2 * q + (lane >> 5));
                        const size_t dst = ((((size_t)w * (K1_CHUNKS + PF) + kc) * 2 + u) * 64 + lane) * 4 + q;
                        wp1[dst] = (ch < 0) ? 0.f : conv1_w[((size_t)n * 518 + ch) * 9 + tap];
                    }
        }
    // conv2: kidx = 8*(kc % 64) + 2q + (lane>>5) is the input channel, tap = kc / 64
    for (int w = 0; w < 8; ++w)
        for (int kc = 0; kc < K2_CHUNKS; ++kc) {
            const int tap = kc / K2_CHUNKS_PER_TAP, kin = kc % K2_CHUNKS_PER_TAP;
            for (int u = 0; u < 2; ++u)
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < 4; ++q) {
                        const int n = 64 * w + 32 * u + (lane & 31);
                        const int ch = 8 * kin + 2 * q + (lane >> 5);
                        const size_t dst = ((((size_t)w * (K2_CHUNKS + PF) + kc) * 2 + u) * 64 + lane) * 4 + q;
                        wp2[dst] = conv2_w[((size_t)n * 512 + ch) * 9 + tap];
                    }
        }
}

// one work-group per proposal slot
int launch_regress_f32(const RegressArgs &a, int n, hipStream_t stream) {
    static DeviceOnce attr_set;
    const int dev = raise_lds_limit(attr_set, {{(const void *)regress_kernel, (int)LDS_BYTES}});
    if (dev < 0) return dev;
    hipLaunchKernelGGL(regress_kernel, dim3(n), dim3(NT), LDS_BYTES, stream, a);
    return check_launch("regress_kernel");
}

}  // namespace p2p
