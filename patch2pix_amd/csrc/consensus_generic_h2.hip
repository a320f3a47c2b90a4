// Coarse stage, shape-generic path, mode P2P_COARSE_GENERIC_FP16X2: every layer with more than one input channel of a generic
// consensus stack on v_mfma_f32_16x16x32_f16 with the project's fp16x2 scheme -- every fp32 operand, scaled by an exact power of
// two, is two fp16 planes (x = hi + lo to 2^-22 |x|), a product is three MFMAs (lo b_hi + hi b_lo + hi b_hi; the dropped
// lo b_lo is <= 2^-22 of the product), accumulation is fp32, the scales are undone exactly.  The first layer (one input channel,
// 1/16 of a hidden layer's work) stays on the exact kernel of consensus_generic.hip, as do the activation layout in the
// workspace (fp32 [pair][a][b][c][d][channel]) and the launch order (per branch, layer by layer).
//   weights      pack_conv4d_planes (host_pack.h): per output channel the exponent that brings its largest |w| into
//                [2^11, 2^12), undone in the epilogue before bias and ReLU; the transposed branch is a second packing
//   activations  one power of two per PAIR, layer and branch: the producing layer (the exact first one included) reduces
//                max |value it stores| of the pair into a zeroed word of the workspace (atomicMax on the float bits; max is exact
//                in any order), the consumer scales the pair so that this maximum lies in [2^11, 2^12).  The exponent is a
//                function of the pair's own activations: outputs do not depend on batch position, batch size or workspace
// Implicit GEMM: rows = 16 consecutive cells along d, columns = output channels padded to 16, K = (da, tap of the slice, input
// channel).  A work-group owns the output tile (a, 4 b, 4 c, 16 d): wave w takes b0 + w and the four rows c0 .. c0 + 3, so one
// pair of B fragments feeds twelve MFMAs.  Per da the work-group stages the slice a + da - k / 2 of its window plus halo,
// (4 + 2p) x (4 + 2p) x (16 + 2p) cells: a thread reads 8 channels of a cell (two 16-byte loads), multiplies by the pair's
// scale, splits into the planes ONCE and writes them as two 16-byte LDS stores; cells outside the volume and channels past the
// last one are zeros without a load, so the tap loop has no bounds check (every lane reads its own cell: no shared zero cell
// on the hot path).  A slice outside the volume is skipped (it would add zeros).  LDS holds 2 planes x NH channel halves,
// each [cell] x 16 bytes with a stride of whole bank rows: the 16 lanes of a ds_read_b128 group read 16 consecutive slots.
// One MFMA covers 32 / CL taps (CL = 8 NH staged channels, 8 or 16) of the slice's k^3 in the order (db, dc, dd); taps past
// the last one read a zero cell and meet zero weights.  An output sums slice by slice, step by step, lo b_hi, hi b_lo, hi b_hi,
// and after every slice the MFMA chain is added into a second accumulator and restarts (at most 63 steps per chain): the order
// depends on the layer alone.  The direct branch's last layer stores y, the transposed branch's adds to it.
// Device code is restricted to what the kernel emulator of the test-suite runs.  Compiled as part of coarse.hip, behind
// consensus_generic.hip.
#pragma once
#include "coarse_common.h"

namespace p2p {

typedef _Float16 nch8 __attribute__((ext_vector_type(8)));
#define P2P_NCH2_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)

constexpr int NCH2_TB = 4, NCH2_TC = 4;    // rows of a work-group: one b per wave, four c per wave
constexpr int NCH2_TAPS = 128;             // table entries: 5^3 = 125 rounded up to whole steps of 2 or 4 taps
constexpr int NCH2_HEAD = NCH2_TAPS * 4;   // bytes of the tap table in front of the staged cells

struct NcH2Args {
    const float *in;         // [pair][cells][cpi]
    float *out;              // [pair][cells][cpo]
    size_t s_in, s_out;      // floats between pairs
    const unsigned char *w;  // fragments [da][step][plane][lane][8] fp16
    const float *wscale;     // [16] 2^-texp of the output channel
    const float *bias;       // [16]
    const int *amax_in;      // the pair's max |input| (float bits)
    int *amax_out;           // null for the last layer
    size_t s_amax;           // words between pairs
    int d0, d1, d2, d3, nb, nc, nd;
    int k, cpi, cpo, nh, nstep, sub;     // sub: cells between two LDS sub-arrays (a multiple of 16, > staged cells)
    int add;
};

__global__ __launch_bounds__(256) void nc_generic_h2_kernel(NcH2Args a) {
    P2P_DYN_SHARED(unsigned char, smem);
    int *taps = (int *)smem;               // staged-cell offset (db, dc, dd) of a tap of the slice, -1 past the last
    unsigned char *cells = smem + NCH2_HEAD;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int k = a.k, pad = k >> 1, SC = NCH2_TC + 2 * pad, SD = 16 + 2 * pad;
    const int ncell = (NCH2_TB + 2 * pad) * SC * SD, ntap = k * k * k;
    const int NH = a.nh, tpm = 4 / NH;     // channel halves of a staged cell; taps per MFMA
    int t = blockIdx.x;
    const int dt0 = (t % a.nd) * 16; t /= a.nd;
    const int c0 = (t % a.nc) * NCH2_TC; t /= a.nc;
    const int b0 = (t % a.nb) * NCH2_TB;
    const int aa = t / a.nb;
    const float *in = a.in + (size_t)blockIdx.z * a.s_in;
    float *out = a.out + (size_t)blockIdx.z * a.s_out;

    // biased exponent E of the pair's largest input magnitude m = 1.f x 2^(E - 127): 2^(138 - E) m lies in [2^11, 2^12)
    const int E = min(max((a.amax_in[(size_t)blockIdx.z * a.s_amax] >> 23) & 255, 12), 254);
    const float sc = __int_as_float((265 - E) << 23), inv = __int_as_float((E - 11) << 23);

    for (int i = tid; i < NCH2_TAPS; i += 256)
        taps[i] = i < ntap ? ((i / (k * k)) * SC + (i / k) % k) * SD + i % k : -1;
    if (tid < 2 * NH) *(nch8 *)(cells + ((size_t)tid * a.sub + ncell) * 16) = (nch8){};      // the zero cell of each sub-array

    const int tsub = g / NH, half = g & (NH - 1);
    const bool active = b0 + wave < a.d1;                       // wave-uniform
    const int base = wave * SC * SD + l15;                      // staged cell of row rt, tap offset 0: + rt * SD
    const unsigned char *ahi = cells + (size_t)half * a.sub * 16, *alo = ahi + (size_t)NH * a.sub * 16;
    const unsigned char *wl = a.w + lane * 16;
    f32x4 acc[NCH2_TC], sum[NCH2_TC];
#pragma unroll
    for (int rt = 0; rt < NCH2_TC; ++rt) { acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f}; sum[rt] = acc[rt]; }
    const int nitems = ncell * NH;
    bool staged = false;
#pragma unroll 1
    for (int da = 0; da < k; ++da, wl += (size_t)a.nstep * 2048) {
        const int ia = aa + da - pad;
        if (ia < 0 || ia >= a.d0) continue;                     // (the whole work-group)
        if (staged) __syncthreads();                            // every wave is done with the previous slice
        staged = true;
#pragma unroll 1
        for (int i = tid; i < nitems; i += 256) {
            const int cell = NH == 2 ? i >> 1 : i, hf = NH == 2 ? i & 1 : 0;
            const int sd = cell % SD, q = cell / SD, sc_ = q % SC, sb = q / SC;
            const int ib = b0 + sb - pad, ic = c0 + sc_ - pad, id = dt0 + sd - pad;
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (ib >= 0 && ib < a.d1 && ic >= 0 && ic < a.d2 && id >= 0 && id < a.d3) {
                const float *src = in + ((((size_t)ia * a.d1 + ib) * a.d2 + ic) * a.d3 + id) * a.cpi + 8 * hf;
                v0 = *(const f32x4 *)src;
                if (a.cpi > 4) v1 = *(const f32x4 *)(src + 4);
            }
            nch8 hi, lo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0 = v0[j] * sc, x1 = v1[j] * sc;
                const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
                hi[j] = h0; hi[4 + j] = h1;
                lo[j] = (_Float16)(x0 - (float)h0); lo[4 + j] = (_Float16)(x1 - (float)h1);
            }
            *(nch8 *)(cells + ((size_t)hf * a.sub + cell) * 16) = hi;
            *(nch8 *)(cells + ((size_t)(NH + hf) * a.sub + cell) * 16) = lo;
        }
        __syncthreads();
        if (!active) continue;
        nch8 bh = *(const nch8 *)wl, bl = *(const nch8 *)(wl + 1024);
#pragma unroll 1
        for (int s = 0; s < a.nstep; ++s) {
            const unsigned char *wn = wl + (size_t)min(s + 1, a.nstep - 1) * 2048;      // the next step's B planes
            const nch8 nbh = *(const nch8 *)wn, nbl = *(const nch8 *)(wn + 1024);
            const int tp = taps[s * tpm + tsub];
            nch8 ah[NCH2_TC], al[NCH2_TC];
#pragma unroll
            for (int rt = 0; rt < NCH2_TC; ++rt) {
                const int cell = tp >= 0 ? base + rt * SD + tp : ncell;
                ah[rt] = *(const nch8 *)(ahi + (size_t)cell * 16);
                al[rt] = *(const nch8 *)(alo + (size_t)cell * 16);
            }
#pragma unroll
            for (int rt = 0; rt < NCH2_TC; ++rt) acc[rt] = P2P_NCH2_MFMA(al[rt], bh, acc[rt]);
#pragma unroll
            for (int rt = 0; rt < NCH2_TC; ++rt) acc[rt] = P2P_NCH2_MFMA(ah[rt], bl, acc[rt]);
#pragma unroll
            for (int rt = 0; rt < NCH2_TC; ++rt) acc[rt] = P2P_NCH2_MFMA(ah[rt], bh, acc[rt]);
            bh = nbh; bl = nbl;
        }
#pragma unroll
        for (int rt = 0; rt < NCH2_TC; ++rt) {
            sum[rt] += acc[rt];
            acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    if (!active) return;

    // accumulator register r = cell dt0 + 4 g + r of the row, column l15 = output channel
    const float ws = a.wscale[l15], bias = a.bias[l15];
    float amax = 0.f;
#pragma unroll
    for (int rt = 0; rt < NCH2_TC; ++rt) {
        const int c = c0 + rt;
        if (c >= a.d2 || l15 >= a.cpo) continue;
        const size_t row0 = (((size_t)aa * a.d1 + b0 + wave) * a.d2 + c) * a.d3;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int od = dt0 + 4 * g + r;
            if (od >= a.d3) continue;
            float *dst = out + (row0 + od) * a.cpo + l15;
            const float v = fmaxf(sum[rt][r] * inv * ws + bias, 0.f);
            *dst = a.add ? *dst + v : v;
            amax = fmaxf(amax, v);
        }
    }
    if (!a.amax_out) return;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
    if (lane == 0) atomicMax(a.amax_out + (size_t)blockIdx.z * a.s_amax, __float_as_int(amax));
}

// the max words of `pairs` pairs (n words each, s words apart) start at zero
__global__ void nc_generic_h2_zero_kernel(int *words, size_t s, int n) {
    if ((int)threadIdx.x < n) words[(size_t)blockIdx.x * s + threadIdx.x] = 0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int nch2_lds_bytes(int k, int nh, int *sub) {
    const int pad = k >> 1, ncell = (NCH2_TB + 2 * pad) * (NCH2_TC + 2 * pad) * (16 + 2 * pad);
    *sub = (ncell + 1 + 15) & ~15;
    return NCH2_HEAD + 2 * nh * *sub * 16;
}
constexpr int NCH2_LDS_MAX = NCH2_HEAD + 4 * 1296 * 16;      // k = 5, sixteen staged channels: 8 x 8 x 20 cells + the zero cell

// packs and uploads the weight planes of every layer behind the first on the first selection of the mode
int nc_generic_ensure_h2(NcGen *g) {
    if (g->mem_h2.uploaded() || g->n_layers < 2) return P2P_OK;
    DeviceBlob b;
    const int nbr = g->symmetric ? 2 : 1;
    size_t ow[NCG_MAX_LAYERS][2], os[NCG_MAX_LAYERS];
    NcH2Layer H[NCG_MAX_LAYERS] = {};
    for (int i = 1; i < g->n_layers; ++i) {
        const NcGenLayer &L = g->layer[i];
        H[i].nh = L.cpi == 16 ? 2 : 1;
        H[i].nstep = (int)conv4d_planes_steps(L.k, H[i].nh);
        H[i].lds_bytes = nch2_lds_bytes(L.k, H[i].nh, &H[i].sub);
        for (int br = 0; br < nbr; ++br) ow[i][br] = b.take<unsigned char>(conv4d_planes_halfs(L.k, H[i].nh) * sizeof(uint16_t));
        os[i] = b.take<float>(16);
    }
    int texp[16];
    for (int i = 1; i < g->n_layers; ++i) {
        const NcGenLayer &L = g->layer[i];
        for (int br = 0; br < nbr; ++br)
            pack_conv4d_planes(g->w_host[i].data(), L.k, L.co, L.ci, H[i].nh, br, (uint16_t *)b.at<unsigned char>(ow[i][br]), texp);
        float *sc = b.at<float>(os[i]);
        for (int n = 0; n < 16; ++n) sc[n] = n < L.co ? std::ldexp(1.0f, -texp[n]) : 1.0f;      // (the same for both branches)
    }
    const int st = b.upload("p2p_ncn_set_mode: the fp16x2 weight planes of the generic consensus net");
    if (st != P2P_OK) return st;
    g->mem_h2 = std::move(b);
    for (int i = 1; i < g->n_layers; ++i) {
        H[i].w[0] = g->mem_h2.dev<unsigned char>(ow[i][0]);
        H[i].w[1] = g->symmetric ? g->mem_h2.dev<unsigned char>(ow[i][1]) : nullptr;
        H[i].wscale = g->mem_h2.dev<float>(os[i]);
        g->h2[i] = H[i];
    }
    return P2P_OK;
}

int launch_nc_generic_h2_zero(int *words, size_t s_words, int pairs, hipStream_t stream) {
    hipLaunchKernelGGL(nc_generic_h2_zero_kernel, dim3((unsigned)pairs), dim3(64), 0, stream, words, s_words, NCH2_WORDS);
    return check_launch("nc_generic_h2_zero_kernel");
}

// one layer (not the first) of one branch; a: the volume, the buffers and the flags as launch_nc_generic filled them in
int launch_nc_generic_h2_layer(const NcGenArgs &a, const NcGenLayer &L, const NcH2Layer &H, int br, const int *amax_in, int *amax_out,
                               int pairs, hipStream_t stream) {
    static DeviceOnce raised;
    if (raise_lds_limit(raised, {{(const void *)nc_generic_h2_kernel, NCH2_LDS_MAX}}) < 0) return P2P_EHIP;
    NcH2Args h{};
    h.in = a.in; h.out = a.out; h.s_in = a.s_in; h.s_out = a.s_out;
    h.w = H.w[br]; h.wscale = H.wscale; h.bias = L.bias;
    h.amax_in = amax_in; h.amax_out = amax_out; h.s_amax = a.s_amax;
    h.d0 = a.d0; h.d1 = a.d1; h.d2 = a.d2; h.d3 = a.d3;
    h.nb = ceil_div(a.d1, NCH2_TB); h.nc = ceil_div(a.d2, NCH2_TC); h.nd = a.nd;
    h.k = L.k; h.cpi = L.cpi; h.cpo = L.cpo; h.nh = H.nh; h.nstep = H.nstep; h.sub = H.sub;
    h.add = a.add;
    const long long groups = (long long)a.d0 * h.nb * h.nc * h.nd;      // <= the row tiles launch_nc_generic has checked
    hipLaunchKernelGGL(nc_generic_h2_kernel, dim3((unsigned)groups, 1, (unsigned)pairs), dim3(256), (size_t)H.lds_bytes, stream, h);
    return check_launch("nc_generic_h2_kernel");
}

}  // namespace p2p
