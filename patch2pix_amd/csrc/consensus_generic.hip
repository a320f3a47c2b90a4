// Coarse stage, shape-generic path: every NeighConsensus stack within the limits of include/p2p_hip.h (p2p_ncn_config), exact
// fp32 on the matrix cores.  The tuned kernel (consensus.hip) is built around 1 -> 16 -> 1 channels and 3^4 taps with the hidden
// volume in LDS; this file trades that fusion for generality: one launch per layer and branch over the volumes of a call, the
// hidden activations in the caller's workspace as fp32 [pair][a][b][c][d][channel], channels innermost and padded to 4, 8 or 16.
//
// A layer is a "same" 4-D cross-correlation (conv4d.py:12-74: zero padding k / 2 on all four axes, bias, ReLU) as an implicit
// GEMM on v_mfma_f32_16x16x4_f32: rows = 16 consecutive cells along the innermost axis d, columns = the up-to-16 output
// channels (zero-padded to 16), K = (tap, input channel), taps outer in the order (da, db, dc, dd).  A super-step is four MFMAs
// = 16 K values; lane (row, kb = lane >> 4) supplies value j of MFMA j:
//   first layer (one input channel, the caller's volume):  tap 16 S + 4 kb + j             -- four 4-byte loads
//   other layers (CP = 4, 8 or 16 padded channels):        tap (4 / Q) S + kb / Q, channels 4 (kb % Q) + j, Q = CP / 4
//                                                                                          -- one 16-byte load
// Taps past the last one and channels past the last one meet zero weights.  A tap outside the volume contributes zeros: the
// address is clamped into the volume, the load is unconditional and the zero is selected when the value is used.
// The transposed branch of symmetric_mode, T(net(T(x))), reads the same volume in the same cell order: in x's coordinates the
// weight of offset (da, db, dc, dd) is w[dc][dd][da][db], so only the packing differs (gen_nc_pack); no permuted copy exists.
// The direct branch's last layer stores y, the transposed branch's last layer adds to it (plain read-add-write: one lane per
// word, launches of one stream run in order).  Every output sums its K terms super-step by super-step, j = 0..3: the order
// depends on the configuration alone -- not on the pair's position in the batch, the batch size or the workspace.
// The handle (NcGen) holds every layer's fragments and biases in one DeviceBlob (host_pack.h).
// Device code is restricted to what the kernel emulator of the test-suite runs.  Compiled as part of coarse.hip.
#pragma once
#include "coarse_common.h"

#include <algorithm>
#include <vector>

namespace p2p {

#define P2P_NCG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int NCG_MAX_LAYERS = 4;
constexpr int NCG_MAX_TAPS = 640;          // 5^4 = 625, rounded up to whole super-steps of 16 taps

struct NcGenLayer {
    int k, ci, co;           // kernel side, input / output channels
    int cpi, cpo;            // padded channels of the input / output activations (input of layer 0: 1; output of the last: 1)
    int nsteps;              // super-steps of 16 K values
    const float *w[2];       // B fragments [step][lane][4] of the direct / transposed branch
    const float *bias;       // [16], zero past co
};

// a layer behind the first in mode P2P_COARSE_GENERIC_FP16X2 (consensus_generic_h2.hip)
struct NcH2Layer {
    const unsigned char *w[2];   // fp16 plane fragments of the direct / transposed branch (pack_conv4d_planes, host_pack.h)
    const float *wscale;         // [16] 2^-texp of the output channel
    int nh, nstep, sub, lds_bytes;
};
constexpr int NCH2_WORDS = 2 * NCG_MAX_LAYERS;      // max words of a pair: word br * NCG_MAX_LAYERS + i = max |output of layer i|

struct NcGen {
    int n_layers, symmetric, cpmax;
    NcGenLayer layer[NCG_MAX_LAYERS];
    DeviceBlob mem;          // one device allocation: every layer's fragments and biases
    std::vector<float> w_host[NCG_MAX_LAYERS];      // the stored weights of the layers behind the first, for the planes
    DeviceBlob mem_h2;       // the fp16x2 planes, packed and uploaded on the mode's first selection
    NcH2Layer h2[NCG_MAX_LAYERS];
};

struct NcGenArgs {
    const float *in;         // [pair][cells][cpi]
    float *out;              // [pair][cells][cpo]
    size_t s_in, s_out;      // floats between pairs
    const float *w, *bias;
    int d0, d1, d2, d3, nd;  // the volume, tiles of 16 cells per row of d
    int k, cpi, cpo, nsteps;
    int tiles;               // per pair
    int add;                 // last layer of the transposed branch: out += result
    int ci;                  // PLANAR only: the real input channels (channel ch of a cell sits ch * cells floats further on)
    size_t cells;            // PLANAR only: cells of the volume = floats between two channel planes
    int *amax;               // P2P_COARSE_GENERIC_FP16X2 (consensus_generic_h2.hip): the pair's max |stored value| is reduced into
    size_t s_amax;           // amax[pair * s_amax] (float bits, zeroed by the launcher); null: nothing is reduced
};

int launch_nc_generic_h2_zero(int *words, size_t s_words, int pairs, hipStream_t stream);
int launch_nc_generic_h2_layer(const NcGenArgs &a, const NcGenLayer &L, const NcH2Layer &H, int br, const int *amax_in, int *amax_out,
                               int pairs, hipStream_t stream);

__device__ __forceinline__ int ncg_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// FIRST: the layer reads the caller's one-channel volume (cpi == 1)
// PLANAR: one stand-alone Conv4d layer (p2p_conv4d_*, conv4d.py:12-74) on the caller's tensors: input [pair][ci][cells] and
// output [pair][co][cells] channel-major as PyTorch lays them out, bias, NO ReLU; the K order is the one of the stack's layers
template <bool FIRST, bool PLANAR>
__global__ __launch_bounds__(256) void nc_generic_kernel(NcGenArgs a) {
    __shared__ int taps[NCG_MAX_TAPS];       // (da, db, dc, dd) of a tap, one byte each; taps past the last repeat it (zero weights)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kb = lane >> 4;
    const int k = a.k, ntap = k * k * k * k;
    for (int t = tid; t < NCG_MAX_TAPS; t += 256) {
        const int u = min(t, ntap - 1);
        taps[t] = ((u / (k * k * k)) << 24) | (((u / (k * k)) % k) << 16) | (((u / k) % k) << 8) | (u % k);
    }
    __syncthreads();
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= a.tiles) return;              // (whole waves, behind the only barrier)
    int g = tile;
    const int dt0 = (g % a.nd) * 16; g /= a.nd;
    const int c = g % a.d2; g /= a.d2;
    const int b = g % a.d1;
    const int aa = g / a.d1;
    const int pad = k >> 1;
    const float *in = a.in + (size_t)blockIdx.z * a.s_in;
    float *out = a.out + (size_t)blockIdx.z * a.s_out;
    const int d = dt0 + l15;                 // this lane's cell of the row (rows past the volume multiply clamped copies)
    const float *wl = a.w + (size_t)lane * 4;

    // the value(s) of one tap for this lane: clamped address, and whether the tap lies inside the volume
    auto locate = [&](int tap, bool *ok) {
        const int tp = taps[tap];
        const int ia = aa + (tp >> 24) - pad, ib = b + ((tp >> 16) & 255) - pad, ic = c + ((tp >> 8) & 255) - pad, id = d + (tp & 255) - pad;
        *ok = ia >= 0 && ia < a.d0 && ib >= 0 && ib < a.d1 && ic >= 0 && ic < a.d2 && id >= 0 && id < a.d3;
        return (size_t)((ncg_clamp(ia, a.d0 - 1) * a.d1 + ncg_clamp(ib, a.d1 - 1)) * a.d2 + ncg_clamp(ic, a.d2 - 1)) * a.d3 + ncg_clamp(id, a.d3 - 1);
    };

    // one super-step of the K axis into `acc` (FIRST: sixteen taps of the one input channel; else tps taps x cpi channels)
    const int Q = FIRST ? 1 : a.cpi >> 2, tps = 4 / Q;           // quads of channels per cell; taps per super-step
    const int tsub = kb / Q, coff = 4 * (kb - tsub * Q);
    auto step = [&](int S, f32x4 &acc) {
        if (FIRST) {
            f32x4 av;
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) av[j] = in[locate(16 * S + 4 * kb + j, &ok[j])];
            const f32x4 bv = *(const f32x4 *)(wl + (size_t)S * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = P2P_NCG_MFMA(ok[j] ? av[j] : 0.f, bv[j], acc);
        } else {
            bool ok;
            const size_t cell = locate(tps * S + tsub, &ok);
            f32x4 ld;
            if constexpr (PLANAR) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {      // channels past the last one: a clamped plane, zero selected
                    const float v = in[(size_t)min(coff + j, a.ci - 1) * a.cells + cell];
                    ld[j] = coff + j < a.ci ? v : 0.f;
                }
            } else {
                ld = *(const f32x4 *)(in + cell * a.cpi + coff);
            }
            const f32x4 bv = *(const f32x4 *)(wl + (size_t)S * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = P2P_NCG_MFMA(ok ? ld[j] : 0.f, bv[j], acc);
        }
    };
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PLANAR) {
        // four partial sums, super-step S into sum S % 4, then (s0 + s1) + (s2 + s3): the rounding error of a stand-alone layer
        // grows with a quarter of the K axis, as that of the reference's slice-wise convolutions does
        f32x4 part[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) part[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int S = 0; S < a.nsteps; S += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (S + u < a.nsteps) step(S + u, part[u]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = (part[0][r] + part[1][r]) + (part[2][r] + part[3][r]);
    } else {
        for (int S = 0; S < a.nsteps; ++S) step(S, acc);
    }
    // accumulator register r = cell dt0 + 4 kb + r of the row, column l15 = output channel
    const bool col = l15 < a.cpo;
    const float bias = a.bias[l15];
    const size_t row0 = (size_t)((aa * a.d1 + b) * a.d2 + c) * a.d3;
    float amax = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int od = dt0 + 4 * kb + r;
        if (!col || od >= a.d3) continue;
        if constexpr (PLANAR) {
            out[(size_t)l15 * a.cells + row0 + od] = acc[r] + bias;
            continue;
        }
        float *dst = out + (row0 + od) * a.cpo + l15;
        const float v = fmaxf(acc[r] + bias, 0.f);
        *dst = a.add ? *dst + v : v;
        amax = fmaxf(amax, v);
    }
    if constexpr (!PLANAR) {
        if (!a.amax) return;                  // (the whole wave)
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
        if (lane == 0) atomicMax(a.amax + (size_t)blockIdx.z * a.s_amax, __float_as_int(amax));
    }
}

// ---- host: packing, the handle, the launches -----------------------------------------------------------------------------------
static int ncg_pad_channels(int c) { return c <= 4 ? 4 : (c <= 8 ? 8 : 16); }

// stored weight [k(da)][co][ci][k(db)][k(dc)][k(dd)] (conv4d.py:119-120) -> B fragments out[(S * 64 + lane) * 4 + j] of branch br
// in the K order of nc_generic_kernel; column n = lane & 15 is output channel n
static void gen_nc_pack(const float *w, const NcGenLayer &L, bool first, int br, float *out) {
    const int k = L.k, ntap = k * k * k * k;
    auto W = [&](int o, int i, int da, int db, int dc, int dd) {
        return w[((((size_t)(da * L.co + o) * L.ci + i) * k + db) * k + dc) * k + dd];
    };
    const int Q = L.cpi / 4;
    for (int S = 0; S < L.nsteps; ++S)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j) {
                const int n = lane & 15, kb = lane >> 4;
                const int tap = first ? 16 * S + 4 * kb + j : (4 / Q) * S + kb / Q;
                const int ch = first ? 0 : 4 * (kb % Q) + j;
                float v = 0.f;
                if (tap < ntap && ch < L.ci && n < L.co) {
                    const int da = tap / (k * k * k), db = (tap / (k * k)) % k, dc = (tap / k) % k, dd = tap % k;
                    v = br ? W(n, ch, dc, dd, da, db) : W(n, ch, da, db, dc, dd);
                }
                out[((size_t)S * 64 + lane) * 4 + j] = v;
            }
}

int nc_generic_create(const p2p_ncn_config *cfg, const p2p_ncn_tensors *t, NcGen **out) {
    const char *F = "p2p_ncn_create_config";
    P2P_REQUIRE(cfg && t && out, P2P_EINVAL, "%s: null argument", F);
    P2P_REQUIRE(cfg->n_layers >= 1, P2P_EINVAL, "%s: n_layers %d must be positive", F, cfg->n_layers);
    P2P_REQUIRE(cfg->n_layers <= NCG_MAX_LAYERS, P2P_EUNSUPPORTED, "%s: n_layers %d: at most 4 layers are implemented", F, cfg->n_layers);
    for (int i = 0; i < cfg->n_layers; ++i) {
        const int k = cfg->kernel_size[i], c = cfg->channels[i];
        P2P_REQUIRE(k > 0 && c > 0, P2P_EINVAL, "%s: kernel_size / channels [%d] = %d / %d must be positive", F, i, k, c);
        P2P_REQUIRE(k == 3 || k == 5, P2P_EUNSUPPORTED, "%s: kernel_size[%d] = %d: kernel sizes 3 and 5 are implemented", F, i, k);
        P2P_REQUIRE(c <= 16, P2P_EUNSUPPORTED, "%s: channels[%d] = %d: at most 16 channels are implemented", F, i, c);
    }
    P2P_REQUIRE(cfg->channels[cfg->n_layers - 1] == 1, P2P_EUNSUPPORTED, "%s: the last layer has %d channels: the consensus volume has one", F,
                cfg->channels[cfg->n_layers - 1]);
    for (int i = 0; i < cfg->n_layers; ++i)
        P2P_REQUIRE(t->w[i] && t->b[i], P2P_EINVAL, "%s: null pointer among the tensors of layer %d", F, i);

    NcGen *g = new NcGen();
    g->n_layers = cfg->n_layers; g->symmetric = cfg->symmetric != 0; g->cpmax = 0;
    const int nbr = g->symmetric ? 2 : 1;
    size_t o_w[NCG_MAX_LAYERS][2], o_b[NCG_MAX_LAYERS];
    auto take = [&](size_t n) { return g->mem.take<float>(n); };
    for (int i = 0; i < g->n_layers; ++i) {
        NcGenLayer &L = g->layer[i];
        const bool last = i + 1 == g->n_layers;
        L.k = cfg->kernel_size[i]; L.ci = i ? cfg->channels[i - 1] : 1; L.co = cfg->channels[i];
        L.cpi = i ? g->layer[i - 1].cpo : 1;
        L.cpo = last ? 1 : ncg_pad_channels(L.co);
        if (!last) g->cpmax = std::max(g->cpmax, L.cpo);
        const int ntap = L.k * L.k * L.k * L.k;
        L.nsteps = i ? ceil_div(ntap * L.cpi, 16) : ceil_div(ntap, 16);
        for (int br = 0; br < nbr; ++br) o_w[i][br] = take((size_t)L.nsteps * 256);
        o_b[i] = take(16);
    }
    float *h = g->mem.at<float>(0);
    for (int i = 0; i < g->n_layers; ++i) {
        const NcGenLayer &L = g->layer[i];
        for (int br = 0; br < nbr; ++br) gen_nc_pack(t->w[i], L, i == 0, br, &h[o_w[i][br]]);
        if (i) g->w_host[i].assign(t->w[i], t->w[i] + (size_t)L.k * L.k * L.k * L.k * L.co * L.ci);
        for (int q = 0; q < L.co; ++q) h[o_b[i] + q] = t->b[i][q];
    }
    const int st = g->mem.upload("p2p_ncn_create_config: the packed consensus net");
    if (st != P2P_OK) {
        delete g;
        return st;
    }
    const float *mem = g->mem.dev<float>();
    for (int i = 0; i < g->n_layers; ++i) {
        NcGenLayer &L = g->layer[i];
        L.w[0] = mem + o_w[i][0];
        L.w[1] = g->symmetric ? mem + o_w[i][1] : nullptr;
        L.bias = mem + o_b[i];
    }
    *out = g;
    return P2P_OK;
}

void nc_generic_destroy(NcGen *g) { delete g; }      // (NcGen is complete in this unit only)

// scratch of one volume: the two activation buffers layers alternate between (a single layer needs none: one block)
// P2P_COARSE_GENERIC_FP16X2 adds one block of max words behind them
size_t nc_generic_ws_bytes(const NcGen &g, size_t cells, int mode) {
    const size_t act = std::max<size_t>(256, (2 * cells * g.cpmax * sizeof(float) + 255) & ~size_t(255));
    return act + (mode == P2P_COARSE_GENERIC_FP16X2 && g.n_layers > 1 ? 256 : 0);
}

// NeighConsensus.forward for `pairs` volumes: X / Y / act of pair z sit z * s_x / s_y / s_act floats further on
int launch_nc_generic(const NcGen &g, int mode, const float *X, size_t s_x, float *Y, size_t s_y, float *act, size_t s_act, int pairs,
                      int d0, int d1, int d2, int d3, hipStream_t stream) {
    // cell offsets are computed in 32 bits
    P2P_REQUIRE((unsigned long long)d0 * d1 * d2 * d3 < (1ull << 31), P2P_EUNSUPPORTED,
                "consensus volume %d x %d x %d x %d has 2^31 cells or more", d0, d1, d2, d3);
    const size_t cells = (size_t)d0 * d1 * d2 * d3;
    float *buf[2] = {act, act + cells * g.cpmax};
    NcGenArgs a{};
    a.d0 = d0; a.d1 = d1; a.d2 = d2; a.d3 = d3; a.nd = ceil_div(d3, 16);
    const long long tiles = (long long)d0 * d1 * d2 * a.nd;
    P2P_REQUIRE(tiles < (1ll << 31) - 4, P2P_EUNSUPPORTED, "consensus volume: %lld row tiles in one launch", tiles);
    a.tiles = (int)tiles;
    const dim3 grid((unsigned)((tiles + 3) / 4), 1, (unsigned)pairs);
    const bool h2 = mode == P2P_COARSE_GENERIC_FP16X2 && g.n_layers > 1;      // (a single layer is the exact first layer)
    int *words = h2 ? (int *)act + nc_generic_ws_bytes(g, cells, 0) / sizeof(int) : nullptr;
    if (h2) {
        P2P_REQUIRE(g.mem_h2.uploaded(), P2P_EINVAL, "consensus net: the planes of P2P_COARSE_GENERIC_FP16X2 were never packed");
        const int st = launch_nc_generic_h2_zero(words, s_act, pairs, stream);
        if (st != P2P_OK) return st;
        a.s_amax = s_act;
    }
    for (int br = 0; br < (g.symmetric ? 2 : 1); ++br)
        for (int i = 0; i < g.n_layers; ++i) {
            const NcGenLayer &L = g.layer[i];
            const bool last = i + 1 == g.n_layers;
            a.in = i ? buf[(i - 1) & 1] : X; a.s_in = i ? s_act : s_x;
            a.out = last ? Y : buf[i & 1]; a.s_out = last ? s_y : s_act;
            a.w = L.w[br]; a.bias = L.bias;
            a.k = L.k; a.cpi = L.cpi; a.cpo = L.cpo; a.nsteps = L.nsteps;
            a.add = last && br == 1;
            a.amax = h2 && !last ? words + br * NCG_MAX_LAYERS + i : nullptr;
            if (h2 && i) {
                const int st = launch_nc_generic_h2_layer(a, L, g.h2[i], br, words + br * NCG_MAX_LAYERS + i - 1, a.amax, pairs, stream);
                if (st != P2P_OK) return st;
                continue;
            }
            if (i == 0) hipLaunchKernelGGL((nc_generic_kernel<true, false>), grid, dim3(256), 0, stream, a);
            else hipLaunchKernelGGL((nc_generic_kernel<false, false>), grid, dim3(256), 0, stream, a);
            const int st = check_launch("nc_generic_kernel");
            if (st != P2P_OK) return st;
        }
    return P2P_OK;
}

// ---- one stand-alone Conv4d layer (p2p_conv4d_*): the same packing and the same kernel, PLANAR -----------------------------------
struct Conv4dLayer {
    NcGenLayer L;
    DeviceBlob mem;
};

int conv4d_create(const float *weight, const float *bias, int c_in, int c_out, int k, Conv4dLayer **out) {
    Conv4dLayer *h = new Conv4dLayer();
    NcGenLayer &L = h->L;
    L.k = k; L.ci = c_in; L.co = c_out;
    L.cpi = c_in == 1 ? 1 : ncg_pad_channels(c_in);
    L.cpo = c_out;
    const int ntap = k * k * k * k;
    L.nsteps = ceil_div(ntap * L.cpi, 16);
    const size_t o_w = h->mem.take<float>((size_t)L.nsteps * 256), o_b = h->mem.take<float>(16);
    float *host = h->mem.at<float>(0);
    gen_nc_pack(weight, L, c_in == 1, 0, &host[o_w]);
    for (int q = 0; q < c_out; ++q) host[o_b + q] = bias ? bias[q] : 0.f;
    const int st = h->mem.upload("p2p_conv4d_create: the packed filters");
    if (st != P2P_OK) {
        delete h;
        return st;
    }
    L.w[0] = h->mem.dev<float>(o_w); L.w[1] = nullptr;
    L.bias = h->mem.dev<float>(o_b);
    *out = h;
    return P2P_OK;
}

void conv4d_destroy(Conv4dLayer *h) { delete h; }
void conv4d_dims(const Conv4dLayer &h, int *c_in, int *c_out) { *c_in = h.L.ci; *c_out = h.L.co; }

// x [pairs][ci][cells] -> y [pairs][co][cells]
int launch_conv4d(const Conv4dLayer &h, const float *x, float *y, int pairs, int d0, int d1, int d2, int d3, hipStream_t stream) {
    P2P_REQUIRE((unsigned long long)d0 * d1 * d2 * d3 < (1ull << 31), P2P_EUNSUPPORTED,
                "p2p_conv4d_forward: volume %d x %d x %d x %d has 2^31 cells or more", d0, d1, d2, d3);
    const NcGenLayer &L = h.L;
    NcGenArgs a{};
    a.cells = (size_t)d0 * d1 * d2 * d3;
    a.d0 = d0; a.d1 = d1; a.d2 = d2; a.d3 = d3; a.nd = ceil_div(d3, 16);
    const long long tiles = (long long)d0 * d1 * d2 * a.nd;
    P2P_REQUIRE(tiles < (1ll << 31) - 4, P2P_EUNSUPPORTED, "p2p_conv4d_forward: %lld row tiles in one launch", tiles);
    a.tiles = (int)tiles;
    a.in = x; a.s_in = a.cells * L.ci;
    a.out = y; a.s_out = a.cells * L.co;
    a.w = L.w[0]; a.bias = L.bias;
    a.k = L.k; a.cpi = L.cpi; a.cpo = L.cpo; a.nsteps = L.nsteps; a.ci = L.ci;
    const dim3 grid((unsigned)((tiles + 3) / 4), 1, (unsigned)pairs);
    if (L.ci == 1) hipLaunchKernelGGL((nc_generic_kernel<true, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((nc_generic_kernel<false, true>), grid, dim3(256), 0, stream, a);
    return check_launch("nc_generic_kernel (Conv4d)");
}

}  // namespace p2p
