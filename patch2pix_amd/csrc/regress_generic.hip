// Fine stage, shape-generic path: every FeatRegressNet configuration within the limits of include/p2p_hip.h
// (p2p_regressor_config), exact fp32 on the matrix cores.  The tuned kernels (regress.hip, regress_h2.hip, regress_wino.hip) are
// built around 518 / 512 channels and the 8x8 map; this file trades their fusion for generality: a chunk of proposals goes
// through the network layer by layer, one launch per layer, activations in the caller's workspace (layout: regress_common.h).
// The handle (GenReg) holds every packed weight, fold and bias in one DeviceBlob (host_pack.h).  The opt-in second arithmetic of a
// generic handle (P2P_REGRESS_GENERIC_FP16X2) replaces gen_conv_kernel alone: regress_generic_h2.hip, chosen in gen_run_level.
// Device code is restricted to what the kernel emulator of the test-suite runs: the two fp32 MFMA shapes, __shfl_xor,
// atomicMax on int.  Compiled as part of api.hip (through regress_api.hip), not as a unit of its own.
#include "regress_common.h"

namespace p2p {

#define P2P_MFMA_F32_32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// the item of slot `prop`, and whether the slot holds a proposal (with device-side counts: the first dev_counts[item] do)
__device__ __forceinline__ bool gen_slot_live(const RegressArgs &a, int prop, int *item) {
    int it = 0;
    while (it + 1 < a.nitems && prop >= a.start[it + 1]) ++it;
    *item = it;
    return !(a.dev_counts && prop - a.start[it] >= a.dev_counts[it]);
}

// what every launch of a chunk knows: slots [p0, p0 + cnt) of the launch's arrays, the level, the chunk's parked mid matches
struct GenChunk {
    int p0, cnt, lvl;
    float *mid;           // [cnt][4] un-truncated matches of level 0 = proposals of level 1
};

// ---- gather + L2 normalisation: one work-group per (proposal, image), one thread per patch pixel ---------------------------
// select_local_patch_feats (networks/utils.py:4-36) over the selected levels, then L2Normalize over the selected channels
// (modules.py:6, eps inside the root).  Coordinates as in regress.hip: trunc of the float / int64 proposal, window origin =
// centre - 8, floor division by the level's stride, clamp to dim // stride - 1, rows of the map ceil(dim / stride) apart.
struct GenGather {
    float *out;           // [sample][16][16][c0]
    int n_feat, feat_idx[4], post, feat_dim, c0;
};
__global__ __launch_bounds__(256) void gen_gather_kernel(RegressArgs a, GenChunk ch, GenGather g) {
    const int s = blockIdx.x >> 1, img = blockIdx.x & 1, prop = ch.p0 + s, tid = threadIdx.x;
    int it;
    if (!gen_slot_live(a, prop, &it)) return;      // empty slot (whole work-group): its activations are never read
    const ItemDev &I = a.item[it];
    float cx, cy;
    if (ch.lvl > 0) {
        cx = ch.mid[(size_t)s * 4 + 2 * img];
        cy = ch.mid[(size_t)s * 4 + 2 * img + 1];
    } else if (a.is_float) {
        cx = ((const float *)a.proposals)[(size_t)prop * 4 + 2 * img];
        cy = ((const float *)a.proposals)[(size_t)prop * 4 + 2 * img + 1];
    } else {
        cx = (float)((const long long *)a.proposals)[(size_t)prop * 4 + 2 * img];
        cy = (float)((const long long *)a.proposals)[(size_t)prop * 4 + 2 * img + 1];
    }
    const int x0 = (int)cx - 8, y0 = (int)cy - 8, py = tid >> 4, px = tid & 15;
    const int H = I.H[img], W = I.W[img];
    float ss = 0.f;
#pragma unroll 1
    for (int f = 0; f < g.n_feat; ++f) {
        const int j = g.feat_idx[f], C = (j == 0) ? 3 : (j == 3) ? 128 : 64;
        const int Ha = level_dim(H, j), Wa = level_dim(W, j);
        const int sy = clampi((y0 + py) >> j, 0, (H >> j) - 1), sx = clampi((x0 + px) >> j, 0, (W >> j) - 1);
        const float *src = I.pyr[img][j] + (size_t)sy * Wa + sx;
        const size_t plane = (size_t)Ha * Wa;
        for (int c = 0; c < C; ++c) {
            const float v = src[c * plane];
            ss = fmaf(v, v, ss);
        }
    }
    const float inv = 1.0f / sqrtf(ss + 1e-6f);
    const int sample = g.post ? 2 * s + img : s;
    float *dst = g.out + ((size_t)sample * 256 + tid) * g.c0;
    int o = g.post ? 0 : img * g.feat_dim;
#pragma unroll 1
    for (int f = 0; f < g.n_feat; ++f) {
        const int j = g.feat_idx[f], C = (j == 0) ? 3 : (j == 3) ? 128 : 64;
        const int Ha = level_dim(H, j), Wa = level_dim(W, j);
        const int sy = clampi((y0 + py) >> j, 0, (H >> j) - 1), sx = clampi((x0 + px) >> j, 0, (W >> j) - 1);
        const float *src = I.pyr[img][j] + (size_t)sy * Wa + sx;
        const size_t plane = (size_t)Ha * Wa;
        for (int c = 0; c < C; ++c) dst[o + c] = src[c * plane] * inv;
        o += C;
    }
    // the channels that pad the row to a multiple of 8 ('pre': behind image 2's) are zeros, not workspace bytes
    if (g.post || img == 1)
        for (; o < g.c0; ++o) dst[o] = 0.f;
}

// ---- convolution as implicit GEMM on v_mfma_f32_32x32x2_f32 --------------------------------------------------------------------
// Rows = (sample, output pixel) of the chunk, columns = output channels, K = (tap, input channel), taps outer.  A wave owns 32
// rows x 64 columns (two accumulator tiles); the four waves of a work-group take four row tiles of the same columns, so that
// the weight fragments they stream hit in the vector L1.  K step: a slab of 8 channels of one tap = four MFMAs per tile; lane
// (row r, half h) holds channels 4 h .. 4 h + 3 of the slab as ONE 16-byte load, MFMA j multiplies channels j (half 0) and
// 4 + j (half 1) -- the weights are packed to match (gen_pack_conv).  Out-of-map taps, rows past the chunk and rows of empty
// slots contribute zeros without a load.  An output sums tap by tap, slab by slab, j = 0..3: the order depends on the layer alone.
// Epilogue: BatchNorm fold; inner layers store the map (masked), the last one applies ReLU and reduces the maximum over the map
// into V[sample][co] with atomicMax on the bits of the non-negative values (V is zeroed before; max is exact in any order).
struct GenConvArgs {
    const float *in;      // [sample][hi][wi][ci]
    float *out;           // [sample][ho][wo][co] (inner layers) or V [sample][co] (last layer)
    GenConv L;
    int spp, last, rows;  // rows = cnt * spp * ho * wo
};
__global__ __launch_bounds__(256) void gen_conv_kernel(RegressArgs a, GenChunk ch, GenConvArgs c) {
    const GenConv &L = c.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int P = L.ho * L.wo;
    const int r0 = (blockIdx.x * 4 + wave) * 32;            // first row of this wave's tile
    if (r0 >= c.rows) return;
    // which samples of the tile hold a proposal: bit i = sample s_first + i (wave-uniform; at most 32 samples touch 32 rows)
    const int s_first = r0 / P, s_last = min(r0 + 31, c.rows - 1) / P;
    unsigned live = 0;
    for (int s = s_first; s <= s_last; ++s) {
        int it;
        if (gen_slot_live(a, ch.p0 + s / c.spp, &it)) live |= 1u << (s - s_first);
    }
    if (!live) return;                                      // (whole waves; a work-group of empty slots exits whole)

    const int row = r0 + l31;
    const int s = row / P, pix = row - s * P, oy = pix / L.wo, ox = pix - oy * L.wo;
    const bool rowok = row < c.rows && ((live >> (s - s_first)) & 1u);
    const int nslab = L.ci >> 3;
    const float *wl = L.w + ((size_t)blockIdx.y * 2 * 64 + lane) * 4;
    const size_t wstep = (size_t)L.ntiles * 256;            // floats from one (tap, slab) to the next
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll 1
    for (int ky = 0; ky < L.ker; ++ky) {
#pragma unroll 1
        for (int kx = 0; kx < L.ker; ++kx) {
            const int iy = oy * L.str - 1 + ky, ix = ox * L.str - 1 + kx;
            const bool ok = rowok && iy >= 0 && iy < L.hi && ix >= 0 && ix < L.wi;
            const float *ap = c.in + (((long long)s * L.hi + iy) * L.wi + ix) * L.ci + 4 * half;    // read only where ok
            for (int sl = 0; sl < nslab; ++sl) {
                f32x4 av = {0.f, 0.f, 0.f, 0.f};
                if (ok) av = *(const f32x4 *)(ap + 8 * sl);
                const f32x4 b0 = *(const f32x4 *)wl, b1 = *(const f32x4 *)(wl + 256);
                wl += wstep;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc0 = P2P_MFMA_F32_32(av[j], b0[j], acc0);
                    acc1 = P2P_MFMA_F32_32(av[j], b1[j], acc1);
                }
            }
        }
    }
    // accumulator register r = row (r & 3) + 8 (r >> 2) + 4 half of the tile, column l31
    const bool whole = c.last && r0 + 31 < c.rows && (r0 + 31) / P == s_first;       // one live sample fills the tile
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = (blockIdx.y * 2 + t) * 32 + l31;
        const bool nok = n < L.co;
        const float sc = nok ? L.scale[n] : 0.f, sh = nok ? L.shift[n] : 0.f;
        const f32x16 &acc = t ? acc1 : acc0;
        if (whole) {
            float m = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) m = fmaxf(m, fmaf(acc[r], sc, sh));
            m = fmaxf(m, __shfl_xor(m, 32));
            if (nok && half == 0) atomicMax((int *)c.out + (size_t)s_first * L.co + n, __float_as_int(m));
            continue;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int os = orow / P;
            if (!nok || orow >= c.rows || !((live >> (os - s_first)) & 1u)) continue;
            const float v = fmaf(acc[r], sc, sh);
            if (c.last) atomicMax((int *)c.out + (size_t)os * L.co + n, __float_as_int(fmaxf(v, 0.f)));
            else c.out[(size_t)orow * L.co + n] = v;
        }
    }
}

// ---- FC layer: Linear + folded BatchNorm1d + ReLU over the chunk's proposals on v_mfma_f32_16x16x4_f32 -------------------
// Rows = proposals (16 per work-group), a wave per 16-column tile; K order as fc_batch_parse: super-step S multiplies
// k = 16 S + 4 (lane >> 4) + j.  x rows of empty slots hold zeros (V is zeroed per level) or finite values of their own.
struct GenFcArgs {
    const float *x;       // [cnt][k]
    float *y;             // [cnt][n]
    GenFc L;
};
__global__ __launch_bounds__(256) void gen_fc_kernel(GenChunk ch, GenFcArgs f) {
    const GenFc &L = f.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kb = lane >> 4, ntl = L.n >> 4;
    const int t = blockIdx.y * 4 + wave;
    if (t >= ntl) return;
    const int row = blockIdx.x * 16 + l15;
    const bool ok = row < ch.cnt;
    const float *xp = f.x + (size_t)row * L.k + 4 * kb;
    const float *wl = L.w + ((size_t)t * 64 + lane) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int S = 0; S < (L.k >> 4); ++S) {
        f32x4 av = {0.f, 0.f, 0.f, 0.f};
        if (ok) av = *(const f32x4 *)(xp + 16 * S);
        const f32x4 bv = *(const f32x4 *)(wl + (size_t)S * ntl * 256);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = P2P_MFMA_F32_16(av[j], bv[j], acc);
    }
    const int n = 16 * t + l15;
    const float b = L.bias[n], sc = L.scale[n], sh = L.shift[n];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int orow = blockIdx.x * 16 + 4 * kb + r;
        if (orow < ch.cnt) f.y[(size_t)orow * L.n + n] = fmaxf(fmaf(acc[r] + b, sc, sh), 0.f);
    }
}

// ---- final Linear to 5 (one fp32 fma chain in k order per output) + parse_regressor_out: thread = (proposal, output) ---------
struct GenOutArgs {
    const float *x, *w, *b;      // [cnt][k], [5][k], [5]
    int k, more;                 // more: a further level follows (park the un-truncated matches)
};
__global__ __launch_bounds__(256) void gen_out_kernel(RegressArgs a, GenChunk ch, GenOutArgs f) {
    const int i = blockIdx.x * 256 + threadIdx.x, row = i >> 3, o = i & 7;
    if (row >= ch.cnt || o >= 5) return;
    const int prop = ch.p0 + row;
    int it;
    if (!gen_slot_live(a, prop, &it)) return;      // empty slot: outputs untouched
    const float *x = f.x + (size_t)row * f.k, *w = f.w + (size_t)o * f.k;
    float s = 0.f;
    for (int k = 0; k < f.k; ++k) s = fmaf(w[k], x[k], s);
    s += f.b[o];
    const int lvl = ch.lvl;
    if (a.raw[lvl]) a.raw[lvl][(size_t)prop * 5 + o] = s;
    if (o < 4) {
        float base;       // the proposal the offsets are relative to, un-truncated (patch2pix.py:145)
        if (lvl > 0) base = ch.mid[(size_t)row * 4 + o];
        else if (a.is_float) base = ((const float *)a.proposals)[(size_t)prop * 4 + o];
        else base = (float)((const long long *)a.proposals)[(size_t)prop * 4 + o];
        const float fm = regress_parse_one(s, o, base, a.item[it]);
        if (a.matches[lvl]) a.matches[lvl][(size_t)prop * 4 + o] = fm;
        if (f.more) ch.mid[(size_t)row * 4 + o] = fm;
    } else {
        if (a.probs[lvl]) a.probs[lvl][prop] = regress_parse_one(s, 4, 0.f, a.item[it]);
    }
}

// ---- host: validation, packing, the handle ----------------------------------------------------------------------------------
static const int GEN_LEVEL_CH[4] = {3, 64, 64, 128};

static int gen_check_dim(int d, const char *what, int i) {
    P2P_REQUIRE(d > 0, P2P_EINVAL, "p2p_regressor_create_config: %s[%d] = %d must be positive", what, i, d);
    P2P_REQUIRE(d % 16 == 0 && d >= 16 && d <= 1024, P2P_EUNSUPPORTED,
                "p2p_regressor_create_config: %s[%d] = %d: dims are multiples of 16 in [16, 1024]", what, i, d);
    return P2P_OK;
}

// conv weight [co][cin][k][k] (torch) -> B fragments: out[(((tap * nslab + slab) * ntiles + t) * 64 + lane) * 4 + j] =
// W[32 t + (lane & 31)][8 slab + 4 (lane >> 5) + j][tap], zero past co and past cin
static void gen_pack_conv(const float *w, int co, int cin, int ci_pad, int ker, int ntiles, float *out) {
    const int nslab = ci_pad / 8, taps = ker * ker;
    for (int tap = 0; tap < taps; ++tap)
        for (int sl = 0; sl < nslab; ++sl)
            for (int t = 0; t < ntiles; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int n = 32 * t + (lane & 31), chn = 8 * sl + 4 * (lane >> 5) + j;
                        const size_t dst = ((((size_t)tap * nslab + sl) * ntiles + t) * 64 + lane) * 4 + j;
                        out[dst] = (n < co && chn < cin) ? w[((size_t)n * cin + chn) * taps + tap] : 0.f;
                    }
}
static bool gen_bn_null(const p2p_bn_params &bn) { return !bn.weight || !bn.bias || !bn.running_mean || !bn.running_var; }

int regressor_generic_create(const p2p_regressor_config *cfg, const p2p_regressor_tensors *t, GenReg **out) {
    const char *F = "p2p_regressor_create_config";
    P2P_REQUIRE(cfg && t && out, P2P_EINVAL, "%s: null argument", F);
    // ---- the configuration against the limits of include/p2p_hip.h
    P2P_REQUIRE(cfg->n_feat >= 1 && cfg->n_feat <= 4, P2P_EINVAL, "%s: n_feat %d must be within [1, 4]", F, cfg->n_feat);
    int feat_dim = 0;
    for (int i = 0; i < cfg->n_feat; ++i) {
        const int j = cfg->feat_idx[i];
        P2P_REQUIRE(j != 4, P2P_EUNSUPPORTED, "%s: feat_idx contains level 4: p2p_pyramid carries levels 0..3 only", F);
        P2P_REQUIRE(j >= 0 && j <= 3, P2P_EINVAL, "%s: feat_idx[%d] = %d is no pyramid level", F, i, j);
        P2P_REQUIRE(i == 0 || j > cfg->feat_idx[i - 1], P2P_EINVAL, "%s: feat_idx must be strictly ascending", F);
        feat_dim += GEN_LEVEL_CH[j];
    }
    P2P_REQUIRE(cfg->feat_comb == P2P_FEAT_COMB_PRE || cfg->feat_comb == P2P_FEAT_COMB_POST, P2P_EINVAL,
                "%s: feat_comb %d is neither P2P_FEAT_COMB_PRE nor P2P_FEAT_COMB_POST", F, cfg->feat_comb);
    P2P_REQUIRE(cfg->psize == 16, P2P_EUNSUPPORTED, "%s: psize %d: only 16 is implemented", F, cfg->psize);
    P2P_REQUIRE(cfg->n_conv >= 1, P2P_EINVAL, "%s: n_conv %d: at least one convolution", F, cfg->n_conv);
    P2P_REQUIRE(cfg->n_conv <= GEN_MAX_LAYERS, P2P_EUNSUPPORTED, "%s: n_conv %d: at most 4 convolutions are implemented", F, cfg->n_conv);
    P2P_REQUIRE(cfg->n_fc >= 0, P2P_EINVAL, "%s: negative n_fc", F);
    P2P_REQUIRE(cfg->n_fc <= GEN_MAX_LAYERS, P2P_EUNSUPPORTED, "%s: n_fc %d: at most 4 hidden FC layers are implemented", F, cfg->n_fc);
    const bool post = cfg->feat_comb == P2P_FEAT_COMB_POST;
    int side = 16;
    for (int i = 0; i < cfg->n_conv; ++i) {
        const int st = gen_check_dim(cfg->conv_dim[i], "conv_dim", i);
        if (st != P2P_OK) return st;
        const int k = cfg->conv_ker[i], s = cfg->conv_str[i];
        P2P_REQUIRE(k > 0 && s > 0, P2P_EINVAL, "%s: conv_ker / conv_str [%d] = %d / %d must be positive", F, i, k, s);
        P2P_REQUIRE(k == 1 || k == 3 || k == 5, P2P_EUNSUPPORTED, "%s: conv_ker[%d] = %d: kernel sizes 1, 3 and 5 are implemented", F, i, k);
        P2P_REQUIRE(s == 1 || s == 2, P2P_EUNSUPPORTED, "%s: conv_str[%d] = %d: strides 1 and 2 are implemented", F, i, s);
        P2P_REQUIRE(side + 2 - k >= 0, P2P_EINVAL, "%s: layer %d (kernel %d) would shrink the %dx%d map below 1x1", F, i, k, side, side);
        side = (side + 2 - k) / s + 1;
    }
    for (int i = 0; i < cfg->n_fc; ++i) {
        const int st = gen_check_dim(cfg->fc_dim[i], "fc_dim", i);
        if (st != P2P_OK) return st;
    }
    // ---- the tensors
    for (int i = 0; i < cfg->n_conv; ++i)
        P2P_REQUIRE(t->conv_w[i] && !gen_bn_null(t->conv_bn[i]), P2P_EINVAL, "%s: null pointer among the tensors of conv layer %d", F, i);
    for (int i = 0; i < cfg->n_fc; ++i)
        P2P_REQUIRE(t->fc_w[i] && t->fc_b[i] && !gen_bn_null(t->fc_bn[i]), P2P_EINVAL, "%s: null pointer among the tensors of FC layer %d", F, i);
    P2P_REQUIRE(t->out_w && t->out_b, P2P_EINVAL, "%s: null pointer for the final Linear", F);

    GenReg *g = new GenReg();
    g->cfg.n_feat = cfg->n_feat;
    for (int i = 0; i < cfg->n_feat; ++i) g->cfg.feat_idx[i] = cfg->feat_idx[i];
    g->cfg.feat_comb = cfg->feat_comb;
    g->cfg.n_conv = cfg->n_conv;
    for (int i = 0; i < cfg->n_conv; ++i) {
        g->cfg.conv_dim[i] = cfg->conv_dim[i]; g->cfg.conv_ker[i] = cfg->conv_ker[i]; g->cfg.conv_str[i] = cfg->conv_str[i];
    }
    g->cfg.n_fc = cfg->n_fc;
    for (int i = 0; i < cfg->n_fc; ++i) g->cfg.fc_dim[i] = cfg->fc_dim[i];
    g->cfg.psize = cfg->psize;

    GenNet &N = g->net;
    N.n_feat = cfg->n_feat;
    for (int i = 0; i < 4; ++i) N.feat_idx[i] = g->cfg.feat_idx[i];
    N.post = post; N.feat_dim = feat_dim; N.spp = post ? 2 : 1;
    N.n_conv = cfg->n_conv; N.n_fc = cfg->n_fc;
    N.fc_in = (post ? 2 : 1) * cfg->conv_dim[cfg->n_conv - 1];
    // one blob: per conv layer weights / scale / shift, per FC layer weights / bias / scale / shift, the final Linear
    auto take = [&](size_t n) { return g->mem.take<float>(n); };
    size_t o_cw[4], o_cs[4], o_cb[4], o_fw[4], o_fb[4], o_fs[4], o_fh[4];
    const int cin0 = post ? feat_dim : 2 * feat_dim;
    int cin = cin0, hw = 16;
    g->act_a = g->act_b = 0;
    for (int i = 0; i < cfg->n_conv; ++i) {
        GenConv &L = N.conv[i];
        L.ci = (cin + 7) & ~7; L.co = cfg->conv_dim[i]; L.ker = cfg->conv_ker[i]; L.str = cfg->conv_str[i];
        L.hi = L.wi = hw;
        hw = (hw + 2 - L.ker) / L.str + 1;
        L.ho = L.wo = hw;
        L.ntiles = 2 * ((L.co + 63) / 64);
        o_cw[i] = take((size_t)L.ker * L.ker * (L.ci / 8) * L.ntiles * 256);
        o_cs[i] = take(L.co); o_cb[i] = take(L.co);
        size_t &act = (i & 1) ? g->act_b : g->act_a;         // layer i reads buffer i & 1 and writes the other one
        act = std::max(act, (size_t)L.hi * L.wi * L.ci);
        cin = L.co;
    }
    int k = N.fc_in;
    g->fc_max = 0;
    for (int i = 0; i < cfg->n_fc; ++i) {
        GenFc &L = N.fc[i];
        L.k = k; L.n = cfg->fc_dim[i];
        o_fw[i] = take((size_t)L.k * L.n); o_fb[i] = take(L.n); o_fs[i] = take(L.n); o_fh[i] = take(L.n);
        g->fc_max = std::max(g->fc_max, (size_t)L.n);
        k = L.n;
    }
    N.k_out = k;
    const size_t o_ow = take((size_t)5 * k), o_ob = take(8);
    g->per_prop = 4 + N.fc_in + 2 * g->fc_max + N.spp * (g->act_a + g->act_b);

    float *h = g->mem.at<float>(0);
    cin = cin0;
    for (int i = 0; i < cfg->n_conv; ++i) {
        const GenConv &L = N.conv[i];
        gen_pack_conv(t->conv_w[i], L.co, cin, L.ci, L.ker, L.ntiles, &h[o_cw[i]]);
        fold_bn(t->conv_bn[i], L.co, &h[o_cs[i]], &h[o_cb[i]]);
        // host copies: the planes of P2P_REGRESS_GENERIC_FP16X2 are packed from them on that mode's first selection
        g->cin[i] = cin;
        g->conv_w_host[i].assign(t->conv_w[i], t->conv_w[i] + (size_t)L.co * cin * L.ker * L.ker);
        g->scale_host[i].assign(&h[o_cs[i]], &h[o_cs[i]] + L.co);
        cin = L.co;
    }
    g->amax_pp = (size_t)N.spp * (cfg->n_conv - 1);
    for (int i = 0; i < cfg->n_fc; ++i) {
        const GenFc &L = N.fc[i];
        pack_fc_mfma(t->fc_w[i], L.n, L.k, &h[o_fw[i]]);
        for (int q = 0; q < L.n; ++q) h[o_fb[i] + q] = t->fc_b[i][q];
        fold_bn(t->fc_bn[i], L.n, &h[o_fs[i]], &h[o_fh[i]]);
    }
    for (int q = 0; q < 5 * k; ++q) h[o_ow + q] = t->out_w[q];
    for (int q = 0; q < 5; ++q) h[o_ob + q] = t->out_b[q];

    const int st = g->mem.upload("p2p_regressor_create_config: the packed regressor");
    if (st != P2P_OK) {
        delete g;
        return st;
    }
    const float *mem = g->mem.dev<float>();
    for (int i = 0; i < cfg->n_conv; ++i) {
        N.conv[i].w = mem + o_cw[i]; N.conv[i].scale = mem + o_cs[i]; N.conv[i].shift = mem + o_cb[i];
    }
    for (int i = 0; i < cfg->n_fc; ++i) {
        N.fc[i].w = mem + o_fw[i]; N.fc[i].bias = mem + o_fb[i]; N.fc[i].scale = mem + o_fs[i]; N.fc[i].shift = mem + o_fh[i];
    }
    N.out_w = mem + o_ow; N.out_b = mem + o_ob;
    *out = g;
    return P2P_OK;
}

// regress_generic_h2.hip: one convolution layer of mode P2P_REGRESS_GENERIC_FP16X2 over the chunk.  amax_in: the per-sample words
// the layer derives its input scales from (null: layer 0, fixed scale), amax_out: the words its stores are reduced into (null:
// the last layer)
int launch_gen_conv_h2(const RegressArgs &a, const GenChunk &ch, const GenConvArgs &c, const GenConvH2 &H, const int *amax_in,
                       int *amax_out, hipStream_t stream);

// one level of one chunk: gather, the conv stack (by the handle's mode), the FC tail, the outputs
static int gen_run_level(const GenReg &R, const RegressArgs &a, const GenChunk &ch, float *ws, size_t U, bool more,
                         hipStream_t stream) {
    const GenNet &N = R.net;
    float *V = ws + gen_ws_v(R, U), *act[2] = {ws + gen_ws_act(R, U, 0), ws + gen_ws_act(R, U, 1)};
    float *fc[2] = {ws + gen_ws_fc(R, U, 0), ws + gen_ws_fc(R, U, 1)};
    GenGather g;
    g.out = act[0]; g.n_feat = N.n_feat; g.post = N.post; g.feat_dim = N.feat_dim; g.c0 = N.conv[0].ci;
    for (int i = 0; i < 4; ++i) g.feat_idx[i] = N.feat_idx[i];
    hipLaunchKernelGGL(gen_gather_kernel, dim3(2 * ch.cnt), dim3(256), 0, stream, a, ch, g);
    int st = check_launch("gen_gather_kernel");
    if (st != P2P_OK) return st;
    P2P_HIP_CHECK(hipMemsetAsync(V, 0, (size_t)ch.cnt * N.fc_in * sizeof(float), stream));
    const bool h2 = R.mode == P2P_REGRESS_GENERIC_FP16X2;
    int *amax = h2 ? (int *)(ws + gen_ws_amax(R, U)) : nullptr;      // [layer boundary][sample] (that mode's part of the workspace)
    const size_t nsamp = (size_t)ch.cnt * N.spp;
    if (h2 && N.n_conv > 1) P2P_HIP_CHECK(hipMemsetAsync(amax, 0, (N.n_conv - 1) * nsamp * sizeof(int), stream));
    for (int i = 0; i < N.n_conv; ++i) {
        GenConvArgs c;
        c.in = act[i & 1]; c.L = N.conv[i]; c.spp = N.spp; c.last = i + 1 == N.n_conv;
        c.out = c.last ? V : act[(i + 1) & 1];
        c.rows = ch.cnt * N.spp * c.L.ho * c.L.wo;
        if (h2) {
            st = launch_gen_conv_h2(a, ch, c, R.h2[i], i ? amax + (i - 1) * nsamp : nullptr, c.last ? nullptr : amax + i * nsamp, stream);
            if (st != P2P_OK) return st;
            continue;
        }
        hipLaunchKernelGGL(gen_conv_kernel, dim3(ceil_div(c.rows, GEN_ROWS), c.L.ntiles / 2), dim3(256), 0, stream, a, ch, c);
        st = check_launch("gen_conv_kernel");
        if (st != P2P_OK) return st;
    }
    const float *x = V;
    for (int i = 0; i < N.n_fc; ++i) {
        GenFcArgs f;
        f.x = x; f.y = fc[i & 1]; f.L = N.fc[i];
        hipLaunchKernelGGL(gen_fc_kernel, dim3(ceil_div(ch.cnt, 16), ceil_div(f.L.n / 16, 4)), dim3(256), 0, stream, ch, f);
        st = check_launch("gen_fc_kernel");
        if (st != P2P_OK) return st;
        x = f.y;
    }
    GenOutArgs o;
    o.x = x; o.w = N.out_w; o.b = N.out_b; o.k = N.k_out; o.more = more;
    hipLaunchKernelGGL(gen_out_kernel, dim3(ceil_div(ch.cnt * 8, 256)), dim3(256), 0, stream, a, ch, o);
    return check_launch("gen_out_kernel");
}

int launch_regress_generic(const GenReg &reg1, const GenReg *reg2, const RegressArgs &a, int n, size_t workspace_bytes,
                           hipStream_t stream) {
    // the chunk: the largest multiple of GEN_UNIT proposals whose scratch fits (the caller checked that one unit does)
    const size_t unit_bytes = gen_per_prop(reg1) * GEN_UNIT * sizeof(float);
    size_t U = std::min<size_t>(workspace_bytes / unit_bytes, GEN_CAP / GEN_UNIT) * GEN_UNIT;
    U = std::min(U, ((size_t)n + GEN_UNIT - 1) / GEN_UNIT * GEN_UNIT);
    for (int p0 = 0; p0 < n; p0 += (int)U) {
        GenChunk ch;
        ch.p0 = p0; ch.cnt = std::min<int>((int)U, n - p0); ch.mid = a.ws + gen_ws_mid(reg1, U);
        for (int lvl = 0; lvl < a.nlevels; ++lvl) {
            ch.lvl = lvl;
            const int st = gen_run_level(lvl ? *reg2 : reg1, a, ch, a.ws, U, lvl + 1 < a.nlevels, stream);
            if (st != P2P_OK) return st;
        }
    }
    return P2P_OK;
}

}  // namespace p2p
