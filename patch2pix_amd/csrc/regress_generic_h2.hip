// Fine stage, shape-generic path, mode P2P_REGRESS_GENERIC_FP16X2: the convolution stack of a generic regressor on
// v_mfma_f32_32x32x16_f16 with the project's fp16x2 scheme -- every fp32 operand, scaled by an exact power of two, is two fp16
// planes (x = hi + lo to 2^-22 |x|), a product is three MFMAs (lo b_hi + hi b_lo + hi b_hi; the dropped lo b_lo is <= 2^-22 of
// the product), accumulation is fp32, the scales are undone exactly.  The gather, the FC tail and the final Linear are those of
// regress_generic.hip (exact fp32); so are the activation layout in the workspace and the chunking.
//   weights      pack_conv_planes (host_pack.h): per output channel the exponent that brings its largest |w| into [2^11, 2^12),
//                folded into the BatchNorm scale
//   layer 0      reads L2-normalised patches (|x| <= 1) under the fixed scale 2^12 (NOTES.md round 3)
//   inner layer  reads its input under a per-SAMPLE power of two: the producing layer reduces max |value it stores| of a sample
//                into a zeroed word of the workspace (atomicMax on the float bits; max is exact in any order), the consumer
//                scales the sample so that this maximum lies in [2^11, 2^12).  The exponent is a function of the sample's own
//                activations, never of its neighbours in the chunk: outputs do not depend on chunk, batch or launch
// Device code is restricted to what the kernel emulator of the test-suite runs.  Compiled as part of api.hip (through
// regress_api.hip, behind regress_generic.hip), not as a unit of its own.
#include "regress_common.h"

namespace p2p {

typedef _Float16 gh8 __attribute__((ext_vector_type(8)));
#define P2P_MFMA_F16_32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

// ---- convolution as implicit GEMM ------------------------------------------------------------------------------------------
// Rows = (sample, output pixel) of the chunk, columns = output channels, K = (slab of 16 input channels, tap), slabs outer.
// A work-group owns 32 * wrows consecutive rows; wave w takes row tile w % wrows and the column pair (2 x 32 channels)
// blockIdx.y * (4 / wrows) + w / wrows.  Per slab the work-group stages the 16 channels of EVERY input pixel of the samples
// its rows touch (a sample's whole map: window and halo of each of its rows): a thread reads 8 channels as two 16-byte loads,
// multiplies by the sample's scale, splits into the planes ONCE and writes them as two 16-byte LDS stores; channels past ci
// (the K padding of the last slab) and samples of empty slots are zeros without a load.  The taps then read LDS: lane (row r,
// half h) takes channels 8 h .. 8 h + 7 of its row's input pixel as one ds_read_b128 per plane, out-of-map taps are zeros in
// registers (no shared zero pixel: NOTES.md, bank conflicts).  The B planes come from global memory in fragment order, one tap
// ahead.  An output sums slab by slab, tap by tap, lo b_hi, hi b_lo, hi b_hi, and every GEN_H2_FLUSH slabs the MFMA chain is
// added into a second accumulator set and restarts: the order depends on the layer alone.
// Epilogue: x 2^-e of the row's sample, BatchNorm fold (the weight exponents are in the scale); inner layers store the map
// (masked) and reduce max |v| per sample; the last one applies ReLU and reduces the maximum over the map into V[sample][co].
struct GenConvH2Args {
    GenConvH2 H;
    const int *amax_in;
    int *amax_out;
};

__global__ __launch_bounds__(256) void gen_conv_h2_kernel(RegressArgs a, GenChunk ch, GenConvArgs c, GenConvH2Args h) {
    P2P_DYN_SHARED(unsigned char, smem);
    float *sscale = (float *)smem, *sinv = sscale + 128;      // per staged sample: 2^e (0 = empty slot) and 2^-e
    unsigned char *spix = smem + GEN_H2_HEAD;
    const GenConv &L = c.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int nwr = h.H.wrows, P = L.ho * L.wo, HW = L.hi * L.wi;
    const int R0 = blockIdx.x * nwr * 32;                     // first row of the work-group (< c.rows by the grid)
    const int s_lo = R0 / P, nsamp = min(R0 + nwr * 32 - 1, c.rows - 1) / P - s_lo + 1;       // at most 128 (host: lds_bytes)
    if (tid < nsamp) {
        const int s = s_lo + tid;
        int it;
        float sc = 0.f, inv = 0.f;
        if (gen_slot_live(a, ch.p0 + s / c.spp, &it)) {
            // biased exponent E of the sample's largest input magnitude m = 1.f x 2^(E - 127): 2^(138 - E) m lies in [2^11, 2^12)
            const int E = h.amax_in ? clampi((h.amax_in[s] >> 23) & 255, 12, 254) : 126;       // layer 0: |x| <= 1 -> 2^12
            sc = __int_as_float((265 - E) << 23);
            inv = __int_as_float((E - 11) << 23);
        }
        sscale[tid] = sc;
        sinv[tid] = inv;
    }
    __syncthreads();
    bool any = false;
    for (int i = 0; i < nsamp; ++i) any |= sscale[i] != 0.f;
    if (!any) return;                                         // a work-group of empty slots (every thread takes this branch)

    const int wr = wave % nwr, cp = blockIdx.y * (4 / nwr) + wave / nwr;
    const int r0 = R0 + wr * 32, row = r0 + l31;
    const int s = row / P, pix = row - s * P, oy = pix / L.wo, ox = pix - oy * L.wo;
    const int s_first = r0 / P, s_last = min(r0 + 31, c.rows - 1) / P;
    bool active = r0 < c.rows && 2 * cp < L.ntiles;           // wave-uniform: this wave has a tile, and a live sample in it
    if (active) {
        bool live = false;
        for (int q = s_first; q <= s_last; ++q) live |= sscale[q - s_lo] != 0.f;
        active = __builtin_amdgcn_readfirstlane(live);
    }
    const bool rowok = active && row < c.rows && sscale[min(s - s_lo, nsamp - 1)] != 0.f;
    const unsigned char *arow = spix + (size_t)((s - s_lo) * HW) * GEN_H2_PIX + 16 * half;      // read only where rowok

    const int taps = L.ker * L.ker;
    const size_t wstep = (size_t)L.ntiles * 2048;             // bytes from one (slab, tap) to the next
    const unsigned char *wl = h.H.w + (size_t)cp * 4096 + lane * 16;
    f32x16 acc0, acc1, sum0, sum1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; sum0[i] = 0.f; sum1[i] = 0.f; }
    gh8 bh0 = {}, bl0 = {}, bh1 = {}, bl1 = {};
    if (active) {
        bh0 = *(const gh8 *)wl; bl0 = *(const gh8 *)(wl + 1024);
        bh1 = *(const gh8 *)(wl + 2048); bl1 = *(const gh8 *)(wl + 3072);
    }
    const int nitems = nsamp * HW * 2;                        // (pixel, 8-channel half) units of a slab
#pragma unroll 1
    for (int sl = 0; sl < h.H.nslab; ++sl) {
        if (sl) __syncthreads();                              // every wave is done with the previous slab
#pragma unroll 1
        for (int i = tid; i < nitems; i += 256) {
            const int pi = i >> 1, hf = i & 1, chn = 16 * sl + 8 * hf;
            const float sc = sscale[pi / HW];
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (sc != 0.f && chn < L.ci) {
                const float *src = c.in + ((size_t)s_lo * HW + pi) * L.ci + chn;
                v0 = *(const f32x4 *)src;
                v1 = *(const f32x4 *)(src + 4);
            }
            gh8 hi, lo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0 = v0[j] * sc, x1 = v1[j] * sc;
                const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
                hi[j] = h0; hi[4 + j] = h1;
                lo[j] = (_Float16)(x0 - (float)h0); lo[4 + j] = (_Float16)(x1 - (float)h1);
            }
            unsigned char *dst = spix + (size_t)pi * GEN_H2_PIX + 16 * hf;
            *(gh8 *)dst = hi;
            *(gh8 *)(dst + 32) = lo;
        }
        __syncthreads();
        if (active) {
            int ky = 0, kx = 0;
#pragma unroll 1
            for (int tap = 0; tap < taps; ++tap) {
                wl += wstep;                                  // the next step's B planes (past the last one: a step of zeros)
                const gh8 nh0 = *(const gh8 *)wl, nl0 = *(const gh8 *)(wl + 1024);
                const gh8 nh1 = *(const gh8 *)(wl + 2048), nl1 = *(const gh8 *)(wl + 3072);
                const int iy = oy * L.str - 1 + ky, ix = ox * L.str - 1 + kx;
                gh8 ah = {}, al = {};
                if (rowok && iy >= 0 && iy < L.hi && ix >= 0 && ix < L.wi) {
                    const unsigned char *ap = arow + (iy * L.wi + ix) * GEN_H2_PIX;
                    ah = *(const gh8 *)ap;
                    al = *(const gh8 *)(ap + 32);
                }
                acc0 = P2P_MFMA_F16_32(al, bh0, acc0);
                acc1 = P2P_MFMA_F16_32(al, bh1, acc1);
                acc0 = P2P_MFMA_F16_32(ah, bl0, acc0);
                acc1 = P2P_MFMA_F16_32(ah, bl1, acc1);
                acc0 = P2P_MFMA_F16_32(ah, bh0, acc0);
                acc1 = P2P_MFMA_F16_32(ah, bh1, acc1);
                bh0 = nh0; bl0 = nl0; bh1 = nh1; bl1 = nl1;
                if (++kx == L.ker) { kx = 0; ++ky; }
            }
            if ((sl & (GEN_H2_FLUSH - 1)) == GEN_H2_FLUSH - 1) {
#pragma unroll
                for (int i = 0; i < 16; ++i) { sum0[i] += acc0[i]; sum1[i] += acc1[i]; acc0[i] = 0.f; acc1[i] = 0.f; }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) { sum0[i] += acc0[i]; sum1[i] += acc1[i]; }

    // accumulator register r = row (r & 3) + 8 (r >> 2) + 4 half of the tile, column l31
    const bool whole = r0 + 31 < c.rows && s_last == s_first;            // one (live) sample fills the tile
    const float inv_first = sinv[s_first - s_lo];
    float amax = 0.f;                                                     // inner layers: max |v| this lane stored for sample acur
    int acur = -1;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = (cp * 2 + t) * 32 + l31;
        const bool nok = n < L.co;
        const float sc = nok ? h.H.scale[n] : 0.f, sh = nok ? L.shift[n] : 0.f;
        const f32x16 &acc = t ? sum1 : sum0;
        if (whole && c.last) {
            float m = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) m = fmaxf(m, fmaf(acc[r] * inv_first, sc, sh));
            m = fmaxf(m, __shfl_xor(m, 32));
            if (nok && half == 0) atomicMax((int *)c.out + (size_t)s_first * L.co + n, __float_as_int(m));
            continue;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (!nok || orow >= c.rows) continue;
            const int os = orow / P;
            const float inv = sinv[os - s_lo];
            if (inv == 0.f) continue;                                     // a row of an empty slot
            const float v = fmaf(acc[r] * inv, sc, sh);
            if (c.last) {
                atomicMax((int *)c.out + (size_t)os * L.co + n, __float_as_int(fmaxf(v, 0.f)));
                continue;
            }
            c.out[(size_t)orow * L.co + n] = v;
            if (os != acur) {
                if (acur >= 0) atomicMax(h.amax_out + acur, __float_as_int(amax));
                acur = os;
                amax = 0.f;
            }
            amax = fmaxf(amax, fabsf(v));
        }
    }
    if (c.last) return;
    if (whole) {                                                          // one word per wave: every lane holds sample s_first or nothing
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
        if (lane == 0) atomicMax(h.amax_out + s_first, __float_as_int(amax));
    } else if (acur >= 0) {
        atomicMax(h.amax_out + acur, __float_as_int(amax));
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// samples the rows [k R, (k + 1) R) of a work-group can touch, over every k (the pattern repeats after P work-groups)
static int gen_h2_samples(int R, int P) {
    int most = 1;
    for (int k = 0; k < P; ++k) most = std::max(most, (k * R + R - 1) / P - (k * R) / P + 1);
    return most;
}

int regressor_generic_ensure_h2(GenReg *g) {
    if (g->mem_h2.uploaded()) return P2P_OK;
    const GenNet &N = g->net;
    DeviceBlob b;
    size_t ow[GEN_MAX_LAYERS], os[GEN_MAX_LAYERS];
    GenConvH2 H[GEN_MAX_LAYERS] = {};
    for (int i = 0; i < N.n_conv; ++i) {
        const GenConv &L = N.conv[i];
        const int taps = L.ker * L.ker;
        H[i].nslab = (g->cin[i] + 15) / 16;
        // the most row tiles per work-group whose staged samples fit the default LDS limit (one tile always does: within the
        // limits of p2p_regressor_config it needs at most 41 KB)
        for (int wr = 4; wr >= 1; wr >>= 1) {
            H[i].wrows = wr;
            H[i].lds_bytes = GEN_H2_HEAD + gen_h2_samples(32 * wr, L.ho * L.wo) * L.hi * L.wi * GEN_H2_PIX;
            if (H[i].lds_bytes <= 65536) break;
        }
        P2P_REQUIRE(H[i].lds_bytes <= 65536, P2P_EUNSUPPORTED,
                    "p2p_regressor_set_mode: conv layer %d would stage %d bytes of LDS in P2P_REGRESS_GENERIC_FP16X2", i, H[i].lds_bytes);
        ow[i] = b.take<unsigned char>((conv_planes_halfs(g->cin[i], taps, L.ntiles) + (size_t)L.ntiles * 1024) * sizeof(uint16_t));
        os[i] = b.take<float>(L.co);
    }
    std::vector<int> texp;
    for (int i = 0; i < N.n_conv; ++i) {
        const GenConv &L = N.conv[i];
        texp.assign(L.co, 0);
        pack_conv_planes(g->conv_w_host[i].data(), L.co, g->cin[i], L.ker * L.ker, L.ntiles, (uint16_t *)b.at<unsigned char>(ow[i]), texp.data());
        float *sc = b.at<float>(os[i]);
        for (int n = 0; n < L.co; ++n) sc[n] = std::ldexp(g->scale_host[i][n], -texp[n]);
    }
    const int st = b.upload("p2p_regressor_set_mode: the fp16x2 weight planes of the generic regressor");
    if (st != P2P_OK) return st;
    g->mem_h2 = std::move(b);
    for (int i = 0; i < N.n_conv; ++i) {
        H[i].w = g->mem_h2.dev<unsigned char>(ow[i]);
        H[i].scale = g->mem_h2.dev<float>(os[i]);
        g->h2[i] = H[i];
    }
    return P2P_OK;
}

int launch_gen_conv_h2(const RegressArgs &a, const GenChunk &ch, const GenConvArgs &c, const GenConvH2 &H, const int *amax_in,
                       int *amax_out, hipStream_t stream) {
    GenConvH2Args h;
    h.H = H; h.amax_in = amax_in; h.amax_out = amax_out;
    const dim3 grid(ceil_div(c.rows, 32 * H.wrows), ceil_div(c.L.ntiles / 2, 4 / H.wrows));
    hipLaunchKernelGGL(gen_conv_h2_kernel, grid, dim3(256), (size_t)H.lds_bytes, stream, a, ch, c, h);
    return check_launch("gen_conv_h2_kernel");
}

}  // namespace p2p
